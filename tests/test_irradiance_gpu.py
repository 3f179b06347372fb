"""nrays_irradiance_points_device / nrays_irradiance_points on the GPU: every result is compared BIT FOR BIT with the numpy mirror irradiance_points_ref (the
definition of include/nrays_abi.h restated; its properties are tested without a GPU in tests/test_irradiance.py) — grids with one and several probes an axis,
every band count, sizes around a wave, points inside, on probes, on the last planes, outside every face and non-finite, validity words with NaN-poisoned rows,
the facing factor, skipped points, every combination of absent outputs, both forms, a call of more than one chunk, the handle's render state, and a furnace."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

import nrays_amd as nr
from nrays_amd import abi, math3d
from tests.test_gather_maps import furnace_scene
from tests.test_irradiance import U, furnace_bound, interior_points, random_grid, same, unit_vectors
from tests.test_occlusion_gpu import STAT_FIELDS, bits
from tests.test_shade_points_gpu import quad_scene

pytestmark = pytest.mark.gpu

GRIDS = [(2, 2, 2), (3, 1, 2), (1, 1, 1), (4, 3, 5)]
SIZES = (1, 63, 64, 65, 257)
_SCENE = []


def scene():
    """One handle for the module: the call reads nothing of the scene but its device, its stream ordering and its staging arena."""
    if not _SCENE:
        _SCENE.append(quad_scene())
    return _SCENE[0]


def point_mix(grid, n, seed):
    """n points that cycle through: inside the grid, exactly on a probe, on the last planes (g = counts - 1), outside each of the six faces, and with NaN / +inf /
    -inf components."""
    rng = np.random.default_rng(seed)
    inside = interior_points(seed + 1, grid, n)
    probes = nr.probe_grid_positions(grid.origin, grid.cell, grid.counts)
    lo = np.asarray(grid.origin, np.float64)
    span = np.array([(c - 1) * s if c > 1 else 0.0 for c, s in zip(grid.counts, grid.cell)])
    out = inside.copy()
    for i in range(n):
        kind, a = i % 14, int(rng.integers(0, 3))
        if kind == 1:
            out[i] = probes[int(rng.integers(0, len(probes)))]
        elif kind == 2:
            out[i, a] = lo[a] + span[a]
        elif kind == 3:
            out[i] = lo + span
        elif 4 <= kind < 10:
            f = kind - 4
            out[i, f // 2] = lo[f // 2] + (span[f // 2] + rng.uniform(0.01, 5.0) if f % 2 else -rng.uniform(0.01, 5.0))
        elif kind >= 10:
            out[i, a] = (math.nan, math.inf, -math.inf, math.nan)[kind - 10]
            if kind == 13:
                out[i] = (math.inf, math.nan, -math.inf)
    return out


def validity(kind, grid, seed):
    """(valid words, the coefficients with NaN in every invalid probe's row)."""
    P = len(grid.sh)
    if kind is None:
        return None, grid.sh
    if kind == "zero":
        return np.zeros(P, np.uint32), np.full_like(grid.sh, np.nan)
    rng = np.random.default_rng(seed)
    v = (rng.integers(0, 1 << 31, size=P).astype(np.uint32) << np.uint32(1)) | (rng.uniform(size=P) < 0.6).astype(np.uint32)  # only bit 0 counts
    sh = grid.sh.copy()
    sh[(v & 1) == 0] = np.nan
    return v, sh


def check(got, want, where=""):
    for name, a, b in zip(("rgb", "sh", "weight"), got, want):
        if a is not None:
            a = a.cpu().numpy() if hasattr(a, "cpu") else a
            assert same(a, b), (name, where)


@pytest.mark.parametrize("bands", [1, 2, 3])
@pytest.mark.parametrize("counts", GRIDS)
def test_equals_the_mirror_bit_for_bit(gpu, counts, bands):
    sc, _ = scene()
    g0 = random_grid(100 + bands, counts, bands)
    for n, vkind, facing in itertools.product(SIZES, (None, "mixed", "zero"), (False, True)):
        valid, sh = validity(vkind, g0, n)
        g = g0._replace(sh=sh, valid=valid)
        p, nm = point_mix(g, n, 7 * n + bands), unit_vectors(n, n)
        got = nr.irradiance_points(sc, p, nm, g, facing=facing, want_sh=True, want_weight=True)
        assert got.rgb.dtype == np.float32 and got.rgb.shape == (n, 3) and got.sh.shape == (n, bands * bands, 3) and got.weight.shape == (n,)
        check(got, nr.irradiance_points_ref(p, nm, g, facing=facing), (n, vkind, facing))
        if vkind == "zero":
            assert all((x.view(np.uint32) == 0).all() for x in got)
        if vkind is None and not facing:
            assert (np.abs(got.weight.astype(np.float64) - 1.0) <= 21 * U).all() and np.isfinite(got.rgb).all()  # (21 roundings: tests/test_irradiance.py)
    assert same(sc.irradiance_points(p, nm, g), nr.irradiance_points_ref(p, nm, g)[0])  # the method, rgb alone


def test_skipped_points_are_zeros_and_their_points_and_normals_are_not_read(gpu):
    import torch
    sc, _ = scene()
    g = random_grid(110, (4, 3, 5))
    n = 257
    p, nm = point_mix(g, n, 111), unit_vectors(112, n)
    flags = (np.random.default_rng(113).integers(0, 2, size=n).astype(np.uint32)) | np.uint32(6)
    live = (flags & 1) != 0
    want = nr.irradiance_points_ref(np.where(live[:, None], p, 0.0), np.where(live[:, None], nm, 0.0), g, True, flags)
    p[~live] = np.nan; nm[~live] = np.nan
    got = nr.irradiance_points(sc, p, nm, g, True, flags, True, True)
    check(got, want)
    assert all((x[~live].view(np.uint32) == 0).all() for x in got) and not (got.weight[live] == 0).any()  # (a live point with an infinite component: NaN under facing)
    dev = nr.irradiance_points(sc, torch.from_numpy(p).cuda(), torch.from_numpy(nm).cuda(), g, True, torch.from_numpy(flags.view(np.int32)).cuda(), True, True)
    check(dev, want)


def _raw(sc, form, n, p, nm, flags, g, outs, facing):
    """The entry point itself with the outputs as given (None: NULL).  host: numpy arrays; device: tensors."""
    lib = abi.load_hip_lib()
    addr = (lambda a: None if a is None else a.ctypes.data) if form == "host" else (lambda t: None if t is None else t.data_ptr())
    grid = abi.NraysIrradianceGrid((C.c_double * 3)(*g.origin), (C.c_double * 3)(*g.cell), (C.c_uint32 * 3)(*g.counts), int(round(math.sqrt(g.sh.shape[-2]))),
                                   addr(g.sh), addr(g.valid), g.measure, 0)
    fl = abi.IRRADIANCE_FACING if facing else 0
    if form == "host":
        cast = lambda a, t: None if a is None else a.ctypes.data_as(C.POINTER(t))  # noqa: E731
        return lib.nrays_irradiance_points(sc.device_handle(), n, cast(p, C.c_double), cast(nm, C.c_double), cast(flags, C.c_uint32), C.byref(grid),
                                           *(cast(o, C.c_float) for o in outs), fl)
    import torch
    rc = lib.nrays_irradiance_points_device(sc.device_handle(), n, addr(p), addr(nm), addr(flags), C.byref(grid), *(addr(o) for o in outs), fl, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("form", ["host", "device"])
def test_every_combination_of_absent_outputs(gpu, form):
    """An output that is not passed is not written (its sentinel-filled buffer stays); without out_rgb and out_sh the call is a bad argument."""
    import torch
    sc, _ = scene()
    n = 65
    g = random_grid(120, (3, 1, 2), 2)
    valid, sh = validity("mixed", g, 121)
    g = g._replace(sh=sh, valid=valid)
    p, nm = point_mix(g, n, 122), unit_vectors(123, n)
    want = nr.irradiance_points_ref(p, nm, g, True)
    to = (lambda a: a) if form == "host" else (lambda a: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda())
    back = (lambda a: a) if form == "host" else (lambda t: t.cpu().numpy())
    gd = g._replace(sh=to(g.sh), valid=to(g.valid))
    pd, nd = to(p), to(nm)
    for use in itertools.product((False, True), repeat=3):
        bufs = [to(np.full(shape, 7.0, np.float32)) for shape in ((n, 3), (n, 4, 3), (n,))]
        rc = _raw(sc, form, n, pd, nd, None, gd, [b if u else None for b, u in zip(bufs, use)], True)
        if not (use[0] or use[1]):
            assert rc == abi.ERR_BAD_ARG and all((back(b) == 7.0).all() for b in bufs)
            continue
        assert rc == abi.OK, abi.load_hip_lib().nrays_last_error()
        for b, u, w in zip(bufs, use, want):
            assert same(back(b), w) if u else (back(b) == 7.0).all(), use


def test_statuses(gpu):
    sc, _ = scene()
    g = random_grid(130, (2, 2, 2))
    n = 4
    p, nm = interior_points(131, g, n), unit_vectors(132, n)
    outs = [np.full((n, 3), 7.0, np.float32), None, None]
    run = lambda grid=g, n=n, p=p, nm=nm, outs=outs: _raw(sc, "host", n, p, nm, None, grid, outs, False)  # noqa: E731
    assert run() == abi.OK and not (outs[0] == 7.0).any()
    outs[0][:] = 7.0
    assert run(n=0) == abi.OK and (outs[0] == 7.0).all()
    big = np.zeros((1, 9, 3), np.float32)  # (never read: the counts are refused first)
    bad = [g._replace(counts=(0, 2, 2)), g._replace(counts=(2, 1025, 2)), g._replace(counts=(1024, 1024, 8), sh=big), g._replace(cell=(0.5, 0.0, 0.5)),
           g._replace(cell=(0.5, -0.5, 0.5)), g._replace(cell=(math.nan, 0.5, 0.5)), g._replace(cell=(math.inf, 0.5, 0.5)), g._replace(origin=(0.0, math.nan, 0.0)),
           g._replace(origin=(math.inf, 0.0, 0.0)), g._replace(measure=math.inf), g._replace(measure=math.nan)]
    for grid in bad:
        assert run(grid) == abi.ERR_BAD_ARG, grid[:3]
    assert run(p=None) == abi.ERR_BAD_ARG and run(nm=None) == abi.ERR_BAD_ARG and run(outs=[None, None, np.zeros(n, np.float32)]) == abi.ERR_BAD_ARG
    lib = abi.load_hip_lib()
    cast = lambda a, t: a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    for bands, sh, reserved, flags, null_grid in ((0, g.sh, 0, 0, False), (4, g.sh, 0, 0, False), (3, None, 0, 0, False), (3, g.sh, 1, 0, False), (3, g.sh, 0, 2, False),
                                                  (3, g.sh, 0, 0x80000001, False), (3, g.sh, 0, 0, True)):
        grid = abi.NraysIrradianceGrid((C.c_double * 3)(*g.origin), (C.c_double * 3)(*g.cell), (C.c_uint32 * 3)(*g.counts), bands, None if sh is None else sh.ctypes.data, None,
                                       g.measure, reserved)
        rc = lib.nrays_irradiance_points(sc.device_handle(), n, cast(p, C.c_double), cast(nm, C.c_double), None, None if null_grid else C.byref(grid),
                                         cast(outs[0], C.c_float), None, None, flags)
        assert rc == abi.ERR_BAD_ARG, (bands, reserved, flags, null_grid)
    assert (outs[0] == 7.0).all()
    # a cell on an axis with one probe may hold anything
    one = random_grid(133, (2, 1, 2), cell=(0.5, math.nan, 0.25))
    p1 = interior_points(134, one, n)
    for facing in (False, True):
        assert same(nr.irradiance_points(sc, p1, nm, one, facing), nr.irradiance_points_ref(p1, nm, one, facing)[0])


def test_the_host_form_equals_the_device_form_on_torchs_current_stream(gpu):
    import torch
    sc, _ = scene()
    g = random_grid(140, (4, 3, 5))
    valid, sh = validity("mixed", g, 141)
    g = g._replace(sh=sh, valid=valid)
    n = 257
    p, nm = point_mix(g, n, 142), unit_vectors(143, n)
    host = nr.irradiance_points(sc, p, nm, g, True, None, True, True)
    check(host, nr.irradiance_points_ref(p, nm, g, True))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        gd = g._replace(sh=torch.from_numpy(g.sh).cuda(), valid=torch.from_numpy(g.valid.view(np.int32)).cuda())
        dev = nr.irradiance_points(sc, torch.from_numpy(p).cuda(), torch.from_numpy(nm).cuda(), gd, True, None, True, True)
        assert all(x.is_cuda for x in dev)
    s.synchronize()
    check(dev, host)
    mixed = nr.irradiance_points(sc, torch.from_numpy(p).cuda(), torch.from_numpy(nm).cuda(), g, True)  # a numpy grid next to tensors is uploaded
    torch.cuda.synchronize()
    assert same(mixed.cpu().numpy(), host.rgb)


def test_a_call_of_more_than_one_chunk_repeats_with_its_points(gpu):
    """n = 2^22 + 17 points that repeat with period 4099 (coprime to the chunk): the outputs repeat with that period bitwise across the chunk boundary, and the
    first period equals the mirror."""
    import torch
    sc, _ = scene()
    period, n = 4099, (1 << 22) + 17
    g = random_grid(150, (2, 2, 2), 2)
    valid = np.full(8, 0xfffffff1, np.uint32)
    valid[5] = 0xfffffff0  # one invalid probe
    sh = g.sh.copy(); sh[5] = np.nan
    g = g._replace(sh=sh, valid=valid)
    base_p = interior_points(152, g, period) * 1.5 - 0.25  # some outside
    base_n = unit_vectors(153, period)
    idx = torch.arange(n, device="cuda") % period
    p, nm = torch.from_numpy(base_p).cuda()[idx], torch.from_numpy(base_n).cuda()[idx]
    gd = g._replace(sh=torch.from_numpy(g.sh).cuda(), valid=torch.from_numpy(g.valid.view(np.int32)).cuda())
    got = nr.irradiance_points(sc, p, nm, gd, True, None, True, True)
    torch.cuda.synchronize()
    want = nr.irradiance_points_ref(base_p, base_n, g, True)
    for name, t, w in zip(got._fields, got, want):
        assert t.shape[0] == n
        first = t[:period]
        assert same(first.cpu().numpy(), w), name
        assert torch.equal(t.view(torch.int32), first.view(torch.int32)[idx]), name


def test_a_call_leaves_the_render_state_alone(gpu):
    import torch
    sc, cam = quad_scene()  # (a fresh handle: its first render is this test's)
    w, h = 128, 72
    proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], w, h)
    first = nr.render(sc, (w, h), 1, 0.0, cam["eye"], proj)
    st1, perm1 = nr.get_stats(sc), nr.last_permutation(sc)
    g = random_grid(160, (3, 1, 2))
    p, nm = point_mix(g, 320, 161), unit_vectors(162, 320)
    with torch.cuda.stream(torch.cuda.Stream()):
        dev = nr.irradiance_points(sc, torch.from_numpy(p).cuda(), torch.from_numpy(nm).cuda(), g, want_sh=True, want_weight=True)
    torch.cuda.synchronize()
    check(dev, nr.irradiance_points_ref(p, nm, g))
    st_mid = nr.get_stats(sc)
    assert nr.last_permutation(sc) == perm1
    second = nr.render(sc, (w, h), 1, 0.0, cam["eye"], proj)
    st2 = nr.get_stats(sc)
    assert np.array_equal(bits(first), bits(second)) and nr.last_permutation(sc) == perm1
    for fld in STAT_FIELDS:
        assert getattr(st1, fld) == getattr(st_mid, fld) == getattr(st2, fld), fld


@pytest.mark.parametrize("device", [None, "cuda"])
def test_furnace_probes_baked_in_a_closed_cube_light_a_point_with_pi_times_the_radiance(gpu, device):
    """The closed cube of tests/test_gather_maps.py has an ambient term and no lights: every ray of a probe returns the same colour L, so the probes hold a constant
    radiance and the irradiance at any interior point and normal is pi L within the bound tests/test_irradiance.py derives on the CPU."""
    sc = furnace_scene()
    dirs = nr.sphere_dirs(1024)
    grid = nr.bake_probe_grid(sc, (0.25, 0.25, 0.25), (0.5, 0.5, 0.5), (2, 2, 2), dirs, device=device)
    to_np = lambda t: t.cpu().numpy() if device else t  # noqa: E731
    pos = nr.probe_grid_positions(grid.origin, grid.cell, grid.counts)
    assert pos.min() == 0.25 and pos.max() == 0.75 and to_np(grid.sh).shape == (8, 9, 3)
    # L: what trace_rays returns for the probes' own rays
    o = np.ascontiguousarray(np.broadcast_to(pos[:, None, :], (8, 1024, 3))).reshape(-1, 3)
    d = np.ascontiguousarray(np.broadcast_to(dirs[None], (8, 1024, 3))).reshape(-1, 3)
    col = nr.trace_rays(sc, o, d, keys=nr.gather_ray_keys(np.arange(8, dtype=np.uint64), 1024).reshape(-1))
    assert (bits(col) == bits(col[:1])).all(), "the furnace's radiance is not constant"
    L = col[0]
    assert same(to_np(grid.sh), nr.sh_fold_ref(d.reshape(8, 1024, 3), col.reshape(8, 1024, 3)))
    p = np.random.default_rng(170).uniform(0.05, 0.95, size=(200, 3))
    nm = unit_vectors(171, 200)
    host_grid = grid._replace(sh=to_np(grid.sh))
    bound, _ = furnace_bound(dirs, L)
    for facing in (False, True):
        if device:
            import torch
            got = nr.irradiance_points(sc, torch.from_numpy(p).cuda(), torch.from_numpy(nm).cuda(), grid, facing, None, True, True)
        else:
            got = sc.irradiance_points(p, nm, grid, facing, None, True, True)
        check(got, nr.irradiance_points_ref(p, nm, host_grid, facing))
        err = np.abs(to_np(got.rgb).astype(np.float64) - math.pi * L.astype(np.float64))
        print("furnace (%s, facing %s): relative error %.3g, bound %.3g" % (device or "host", facing, (err / (math.pi * L)).max(), (bound / (math.pi * L)).max()))
        assert (err <= bound).all()
