"""Gathered light as spherical harmonics (nrays_gather_sh_points_device / nrays_gather_sh_points; nrays_amd.gather_sh_points, gather_probes) on the GPU: the
coefficients against sh_fold_ref of trace_rays on the very same rays and keys, bit for bit — every scene kind, the queue, an area light, with and without rotations,
host and device form, hinted and unhinted —; the band prefix; the fold kernel alone on colours of every magnitude; skipped points; the chunk seam at the largest
table; probes; the statuses; the handle's render state.  Every handle here is created under NRAYS_RAY_REORDER=2, so that a hinted call is reordered whatever its size."""
import ctypes as C
import math

import numpy as np
import pytest

import nrays_amd as nr
from nrays_amd import abi, math3d
from tests.test_gather_gpu import ray_colours
from tests.test_gather_order_gpu import KS, NS, fresh
from tests.test_occlusion_gpu import STAT_FIELDS, bits, case
from tests.test_shade_points import rich_analytic_scene
from tests.test_trace_rays_gpu import _glass_scene
from tools import scenes_util as su

pytestmark = pytest.mark.gpu
BACKGROUND = (0.2, 0.5, 0.9)


@pytest.fixture(autouse=True)
def reorder_always(monkeypatch):
    monkeypatch.setenv("NRAYS_RAY_REORDER", "2")  # read when a handle is created


def device_sh(sc, points, normals, L, rot=None, bias=1e-3, energy=1.0, max_depth=0, bands=3, hit_flags=None, keys=None, stream=None, unordered=False):
    """gather_sh_points on torch tensors (on `stream` when given), copied back."""
    import torch
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    tp, tn = up(points), up(normals)
    thf = None if hit_flags is None else up(np.ascontiguousarray(hit_flags, dtype=np.uint32).view(np.int32))
    tk = None if keys is None else up(np.ascontiguousarray(keys, dtype=np.uint64).view(np.int64))
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            r = nr.gather_sh_points(sc, tp, tn, L, rot, bias, energy, max_depth, bands, hit_flags=thf, keys=tk, unordered=unordered)
        stream.synchronize()
    else:
        r = nr.gather_sh_points(sc, tp, tn, L, rot, bias, energy, max_depth, bands, hit_flags=thf, keys=tk, unordered=unordered)
    torch.cuda.synchronize()
    assert r.dtype == torch.float32 and tuple(r.shape) == (len(points), bands * bands, 3)
    return r.cpu().numpy()


def reference(sc, points, normals, L, rot, bias, energy, max_depth, keys, bands):
    """The definition, from parts that existed before: trace_rays on occlusion_rays() with gather_ray_keys(), folded by the numpy mirror."""
    _, rd = nr.occlusion_rays(points, normals, L, rot, bias, keys)
    return nr.sh_fold_ref(rd, ray_colours(sc, points, normals, L, rot, bias, energy, max_depth, keys), bands)


# ---- 1: the definition -------------------------------------------------------------------------------------------------------------------------------------
# hair: opaque meshes only; mixed: meshes and shapes; analytic and glass: double-branching, the queue runs; area: an area light reads the per-ray keys.
@pytest.mark.parametrize("name", ["hair", "mixed", "analytic", "glass", "area"])
def test_equals_the_mirror_fold_of_trace_rays_bit_for_bit(gpu, name):
    import torch
    c = fresh(name)
    sc = c["scene"]
    stream = torch.cuda.Stream()
    differ, nonzero = 0, 0
    for k in KS:
        L = nr.hemisphere_dirs(k)
        for n in NS:
            p, nm, keys = c["points"][:n], c["normals"][:n], c["keys"][:n]
            max_depth = 1 if (k + n) % 2 else 0
            for rot in (None, nr.rotation_table(5)):
                _, rd = nr.occlusion_rays(p, nm, L, rot, 1e-3, keys)
                colours = ray_colours(sc, p, nm, L, rot, 1e-3, 1.0, max_depth, keys)
                for bands in (1, 2, 3):
                    want = nr.sh_fold_ref(rd, colours, bands)
                    got = [nr.gather_sh_points(sc, p, nm, L, rot, 1e-3, 1.0, max_depth, bands, keys=keys),
                           nr.gather_sh_points(sc, p, nm, L, rot, 1e-3, 1.0, max_depth, bands, keys=keys, unordered=True),
                           device_sh(sc, p, nm, L, rot, 1e-3, 1.0, max_depth, bands, keys=keys, stream=stream),
                           device_sh(sc, p, nm, L, rot, 1e-3, 1.0, max_depth, bands, keys=keys, stream=stream, unordered=True)]
                    bad = [int((bits(g) != bits(want)).any(axis=(1, 2)).sum()) for g in got]
                    if any(bad):
                        print("%s k = %d n = %d R = %s bands = %d max_depth = %d: points that differ (host, host hinted, device, device hinted) %s" %
                              (name, k, n, rot is not None, bands, max_depth, bad))
                    differ += sum(bad)
                    assert got[0].shape == (n, bands * bands, 3) and got[0].dtype == np.float32
                    for g in got:
                        assert np.array_equal(bits(g), bits(want))
                nonzero += int((want[:, 1:] != 0.0).any(axis=(1, 2)).sum())
    assert differ == 0 and nonzero > 500  # (the higher bands really carry light)


# ---- 2: the band prefix ------------------------------------------------------------------------------------------------------------------------------------
def test_lower_bands_are_a_prefix_of_the_higher(gpu):
    c = fresh("mixed")
    L, rot = nr.hemisphere_dirs(70), nr.rotation_table(5)
    p, nm, keys = c["points"][:65], c["normals"][:65], c["keys"][:65]
    for unordered in (False, True):
        b = {bands: nr.gather_sh_points(c["scene"], p, nm, L, rot, 1e-3, 1.0, 1, bands, keys=keys, unordered=unordered) for bands in (1, 2, 3)}
        assert np.array_equal(bits(b[3][:, :1]), bits(b[1])) and np.array_equal(bits(b[3][:, :4]), bits(b[2]))
        assert (b[3][:, 4:] != 0.0).any()
    # coefficient 0 is K0 times each colour, folded: not the mean colour times K0, but close to it
    mean = nr.gather_points(c["scene"], p, nm, L, rot, 1e-3, 1.0, 1, keys=keys)
    assert np.allclose(b[1][:, 0], np.float32(nr.scene.SH_K[0]) * mean, rtol=1e-5, atol=1e-7)


# ---- 3: the fold kernel alone ------------------------------------------------------------------------------------------------------------------------------
def _wild_colours(rng, n, k):
    """Magnitudes 1e-30 .. 1e30 of either sign; every eleventh value one of +-0, +-inf, NaN, and values whose product with a basis value lies below 2^-126."""
    col = (10.0 ** rng.uniform(-30.0, 30.0, size=(n, k, 3)) * rng.choice([-1.0, 1.0], size=(n, k, 3))).astype(np.float32)
    special = np.asarray([0.0, -0.0, np.inf, -np.inf, np.nan, 3e-38, -2e-38, 1.5e-39, 1e-45, 2.0 ** -126], np.float32)
    flat = col.reshape(-1)
    idx = np.arange(0, flat.size, 11)
    flat[idx] = special[np.arange(len(idx)) % len(special)]  # (in turn: from ten of them on, each is there)
    return col


@pytest.mark.parametrize("n", [1, 67])
@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 129, 1024])
def test_the_fold_kernel_alone_equals_the_mirror(gpu, k, n):
    """Tiles of 32 directions: k around one and two tiles' ends and the largest table; n = 67: nine workgroups of eight points, the last with three."""
    sc = fresh("mixed")["scene"]
    rng = np.random.default_rng(1000 * k + n)
    nm = rng.normal(size=(n, 3))
    nm /= np.sqrt((nm * nm).sum(axis=1))[:, None]
    p = rng.uniform(-3.0, 3.0, size=(n, 3))
    keys = rng.integers(0, 2 ** 63, size=n, dtype=np.int64).astype(np.uint64)
    L, rot = nr.hemisphere_dirs(k), nr.rotation_table(5)
    seen_nan, seen_sub = 0, 0
    for colours in (_wild_colours(rng, n, k), rng.uniform(0.0, 2.0, size=(n, k, 3)).astype(np.float32) * np.float32(1e-38)):
        for R in (rot, None):
            _, rd = nr.occlusion_rays(p, nm, L, R, 1e-3, keys)
            for bands in (1, 2, 3):
                want = nr.sh_fold_ref(rd, colours, bands)
                got = nr.gather_sh_fold(sc, p, nm, L, colours, R, 1e-3, bands, keys=keys)
                assert got.shape == want.shape and got.dtype == np.float32
                nan = np.isnan(want)
                assert np.isnan(got[nan]).all()
                assert np.array_equal(bits(got)[~nan], bits(want)[~nan])
                seen_nan += int(nan.sum())
                seen_sub += int(((np.abs(want) < 2.0 ** -126) & (want != 0.0)).sum())
    assert seen_sub > 0  # subnormal results are held to the bit
    if k >= 63:
        assert seen_nan > 0
    got, ms = nr.gather_sh_fold(sc, p, nm, L, colours, rot, 1e-3, 3, keys=keys, want_ms=True)
    assert ms > 0.0 and got.shape == (n, 9, 3)


# ---- 4: skipped points -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "analytic"])
@pytest.mark.parametrize("form", ["host", "device"])
def test_skipped_points_are_zero_and_leave_their_neighbours_alone(gpu, form, name):
    c = fresh(name)
    sc = c["scene"]
    L, rot = nr.hemisphere_dirs(16), nr.rotation_table(5)
    if form == "host":
        run = lambda p, nm, hf, keys, **kw: nr.gather_sh_points(sc, p, nm, L, rot, 1e-3, 1.0, 1, 3, hit_flags=hf, keys=keys, **kw)  # noqa: E731
    else:
        run = lambda p, nm, hf, keys, **kw: device_sh(sc, p, nm, L, rot, 1e-3, 1.0, 1, 3, hit_flags=hf, keys=keys, **kw)  # noqa: E731
    n = 130
    p, nm, keys = c["points"][:n].copy(), c["normals"][:n].copy(), c["keys"][:n]
    base = run(p, nm, None, keys)
    assert (base != 0.0).any(axis=(1, 2)).sum() > n // 2
    assert np.array_equal(bits(run(p, nm, np.full(n, 3, np.uint32), keys, unordered=True)), bits(base))
    skipped = np.arange(n) % 3 == 1
    hf = np.where(skipped, np.asarray([0, 2, 0xfffffffe, 0], np.uint32)[(np.arange(n) // 3) % 4], 1).astype(np.uint32)  # bit 0 clear, whatever else is set
    p[skipped], nm[skipped] = np.nan, np.nan
    for unordered in (False, True):
        got = run(p, nm, hf, keys, unordered=unordered)
        assert (bits(got[skipped]) == 0).all()
        assert np.array_equal(bits(got[~skipped]), bits(base[~skipped]))
    p[:], nm[:] = np.nan, np.nan
    for unordered in (False, True):
        assert (bits(run(p, nm, np.zeros(n, np.uint32), keys, unordered=unordered)) == 0).all()  # every point skipped
    # the fold kernel alone: a skipped point's colours are not read either
    colours = np.full((n, 16, 3), np.nan, np.float32)
    assert (bits(nr.gather_sh_fold(sc, p, nm, L, colours, rot, 1e-3, 3, hit_flags=np.zeros(n, np.uint32), keys=keys)) == 0).all()


# ---- 5: the chunk seam at the largest table ------------------------------------------------------------------------------------------------------------------
def test_across_the_chunk_seam_at_1024_directions(gpu):
    """k = 1024: a chunk holds 4096 points; n = 4096 + 3 leaves three points to the second chunk, whose default keys go on from the first chunk's."""
    sc = fresh("tiny")["scene"]
    c = case("tiny")
    n = 4096 + 3
    L, rot = nr.hemisphere_dirs(1024), nr.rotation_table(5)
    reps = -(-n // 320)
    p, nm = (np.ascontiguousarray(np.tile(a, (reps, 1))[:n]) for a in (c["points"], c["normals"]))
    whole = nr.gather_sh_points(sc, p, nm, L, rot, 1e-3, 1.0, 1, 3)
    assert whole.shape == (n, 9, 3)
    tail = nr.gather_sh_points(sc, p[-3:], nm[-3:], L, rot, 1e-3, 1.0, 1, 3, keys=np.arange(4096, 4099, dtype=np.uint64))
    assert np.array_equal(bits(whole[-3:]), bits(tail)) and (tail != 0.0).any()
    assert (bits(whole[:320]) != bits(whole[320:640])).any()  # the same point under another key: another rotation somewhere
    dev = device_sh(sc, p, nm, L, rot, 1e-3, 1.0, 1, 3, unordered=True)
    assert np.array_equal(bits(dev), bits(whole))
    want = reference(sc, p[-3:], nm[-3:], L, rot, 1e-3, 1.0, 1, np.arange(4096, 4099, dtype=np.uint64), 3)
    assert np.array_equal(bits(tail), bits(want))


# ---- 6: probes -----------------------------------------------------------------------------------------------------------------------------------------------
def test_gather_probes_is_gather_sh_points_with_the_z_normal_and_no_bias(gpu):
    import torch
    c = fresh("analytic")
    sc = c["scene"]
    pos = c["points"][:65] + 0.25 * c["normals"][:65]
    L = nr.sphere_dirs(70)
    up = np.tile([0.0, 0.0, 1.0], (65, 1))
    for bands in (1, 3):
        want = nr.gather_sh_points(sc, pos, up, L, None, 0.0, 1.0, 1, bands, keys=c["keys"][:65])
        got = nr.gather_probes(sc, pos, L, bands, 1.0, 1, keys=c["keys"][:65])
        assert got.shape == (65, bands * bands, 3) and np.array_equal(bits(got), bits(want)) and (got != 0.0).any()
        assert np.array_equal(bits(nr.gather_probes(sc, pos, L, bands, 1.0, 1, keys=c["keys"][:65], unordered=False)), bits(want))
        assert np.array_equal(bits(sc.gather_probes(pos, L, bands, 1.0, 1, keys=c["keys"][:65])), bits(want))  # Scene.gather_probes
    dev = nr.gather_probes(sc, torch.from_numpy(pos).cuda(), L, 3, 1.0, 1, keys=torch.from_numpy(c["keys"][:65].view(np.int64)).cuda())
    torch.cuda.synchronize()
    assert np.array_equal(bits(dev.cpu().numpy()), bits(want))
    # the frame of (0, 0, 1) reproduces the table: the rays leave the position itself along the table's directions, bit for bit
    o, d = nr.occlusion_ray_probe(sc, pos, up, L, None, 0.0)
    assert np.array_equal(d.view(np.uint64), np.broadcast_to(L[None], d.shape).copy().view(np.uint64))
    assert np.array_equal(o.view(np.uint64), np.broadcast_to(pos[:, None, :], o.shape).copy().view(np.uint64))


def test_a_probe_in_the_open_sees_pi_times_the_background(gpu):
    """Every one of the 1024 rays misses the scene (asserted with intersects_rays), so the radiance is the background from every direction and the irradiance is
    pi * background for every normal.  1e-3 relative: four times the 2.3e-4 deviation of sphere_dirs(1024) as a quadrature (tests/test_gather_sh.py); the f32
    fold of 1024 terms stays below 1e-4."""
    sc = nr.Scene([nr.SceneNode(su.default_material(), 0.0, 0.0, 1.0, 1.0, nr.Isometry3((0, 0, 0)), nr.Ball(1.0))], [nr.Light((0.0, 5.0, 0.0), 0.0, 1, (1, 1, 1))], BACKGROUND)
    L = nr.sphere_dirs(1024)
    pos = None
    for cand in ((1000.0, 0.0, 0.0), (0.0, 1000.0, 0.0), (577.0, 577.0, 577.0), (-700.0, 300.0, 650.0)):
        lit, _ = nr.intersects_rays(sc, np.tile(cand, (1024, 1)), L, np.full(1024, np.inf))
        if lit.all():
            pos = np.asarray([cand], np.float64)
            break
    assert pos is not None, "every candidate position has a ray that meets the ball"
    sh = nr.gather_probes(sc, pos, L, 3)
    axes = np.asarray([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)
    e = nr.sh_irradiance(sh[0].astype(np.float64), axes)
    want = math.pi * np.asarray(BACKGROUND)
    rel = float(np.abs(e / want - 1.0).max())
    print("open probe: max relative deviation from pi * background %.3g" % rel)
    assert e.shape == (6, 3)
    assert rel <= 1e-3


# ---- 7: statuses ---------------------------------------------------------------------------------------------------------------------------------------------
def _raw_call(sc, form, n, arrays, params, bands=3, flags=0, null=(), scene=True):
    """One library call with host or device pointers; returns (status, out_sh)."""
    import torch
    lib = abi.load_hip_lib()
    order = ("points", "normals", "hit_flags", "keys", "params")
    h = sc.device_handle() if scene else None
    if form == "device":
        held = {k: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v.view(np.int32) if v.dtype == np.uint32 else v).cuda() for k, v in arrays.items()}
        tables = {k: None if params[k] is None else torch.from_numpy(np.ascontiguousarray(params[k], dtype=np.float64)).cuda() for k in ("dirs", "rotations")}
        adr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        ptrs = {k: adr(t) for k, t in held.items()}
    else:
        ct = {np.dtype(np.float64): C.c_double, np.dtype(np.uint32): C.c_uint32, np.dtype(np.uint64): C.c_uint64, np.dtype(np.float32): C.c_float}
        tables = {k: None if params[k] is None else np.ascontiguousarray(params[k], dtype=np.float64) for k in ("dirs", "rotations")}
        adr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        ptrs = {k: v.ctypes.data_as(C.POINTER(ct[v.dtype])) for k, v in arrays.items()}
    st = abi.NraysGatherParams(params["num_dirs"], params["num_rotations"], adr(tables["dirs"]), adr(tables["rotations"]), params["bias"], params["energy"], params["max_depth"])
    ptrs["params"] = C.byref(st)
    args = [None if k in null else ptrs[k] for k in order]
    out = None if "out_sh" in null else ptrs["out_sh"]
    if form == "device":
        rc = lib.nrays_gather_sh_points_device(h, n, *args, bands, out, flags, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc, held["out_sh"].cpu().numpy()
    return lib.nrays_gather_sh_points(h, n, *args, bands, out, flags), arrays["out_sh"]


@pytest.mark.parametrize("form", ["host", "device"])
def test_statuses(gpu, form):
    c = fresh("analytic")
    sc, n, k, R = c["scene"], 16, 8, 3
    arrays = dict(points=c["points"][:n].copy(), normals=c["normals"][:n].copy(), hit_flags=np.ones(n, np.uint32), keys=c["keys"][:n].copy(), out_sh=np.full((n, 9, 3), 7.0, np.float32))
    params = dict(num_dirs=k, num_rotations=R, dirs=nr.hemisphere_dirs(k), rotations=nr.rotation_table(R), bias=1e-3, energy=1.0, max_depth=1)
    call = lambda **kw: _raw_call(sc, form, kw.pop("n", n), arrays, dict(params, **kw.pop("p", {})), **kw)  # noqa: E731

    def refused(**kw):
        rc, out = call(**kw)
        assert rc == abi.ERR_BAD_ARG and (out == 7.0).all(), kw

    for n_ in (0, n):
        for bands in (0, 4, 9, 1 << 31):
            refused(bands=bands, n=n_)
        for flags in (2, 4, 3, 1 << 31, (1 << 31) | 1):
            refused(flags=flags, n=n_)
    for flags in (0, 1):
        for name in ("points", "normals", "params", "out_sh"):
            refused(null=(name,), flags=flags)
        refused(scene=False, flags=flags)
        for p in (dict(dirs=None), dict(num_dirs=0), dict(num_dirs=1025), dict(num_rotations=1025), dict(rotations=None), dict(bias=np.inf), dict(energy=np.nan)):
            refused(p=p, flags=flags)
        rc, out = call(n=0, flags=flags)
        assert rc == abi.OK and (out == 7.0).all()  # without work; nothing so far wrote the output
    for bands in (1, 2, 3):
        want = nr.gather_sh_points(sc, arrays["points"], arrays["normals"], params["dirs"], params["rotations"], 1e-3, 1.0, 1, bands, keys=arrays["keys"])
        for flags in (0, 1):
            arrays["out_sh"][:] = 7.0
            rc, out = call(flags=flags, bands=bands)
            C_ = bands * bands
            assert rc == abi.OK and np.array_equal(bits(out.reshape(-1)[:n * C_ * 3].reshape(n, C_, 3)), bits(want))
            assert (out.reshape(-1)[n * C_ * 3:] == 7.0).all()  # n x C x 3 floats and no more
    arrays["out_sh"][:] = 7.0
    rc, out = call(flags=1, null=("hit_flags", "keys"), p=dict(num_rotations=0, rotations=None))  # every point live, key i; no rotation: a NULL table is fine
    assert rc == abi.OK and np.array_equal(bits(out), bits(nr.gather_sh_points(sc, arrays["points"], arrays["normals"], params["dirs"], None, 1e-3, 1.0, 1, 3)))
    # the probe checks its arguments the same way
    lib, dp = abi.load_hip_lib(), C.POINTER(C.c_double)
    tables = (np.ascontiguousarray(params["dirs"]), np.ascontiguousarray(params["rotations"]))
    st = abi.NraysGatherParams(k, R, tables[0].ctypes.data, tables[1].ctypes.data, 1e-3, 1.0, 0)
    colours, out = np.zeros((n, k, 3), np.float32), np.full((n, 9, 3), 7.0, np.float32)
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    base = [sc.device_handle(), n, arrays["points"].ctypes.data_as(dp), arrays["normals"].ctypes.data_as(dp), None, None, C.byref(st)]
    assert lib.nrays_debug_gather_sh_fold(*base, 0, fp(colours), fp(out), None) == abi.ERR_BAD_ARG
    assert lib.nrays_debug_gather_sh_fold(*base, 4, fp(colours), fp(out), None) == abi.ERR_BAD_ARG
    assert lib.nrays_debug_gather_sh_fold(*base, 3, None, fp(out), None) == abi.ERR_BAD_ARG
    assert lib.nrays_debug_gather_sh_fold(*base, 3, fp(colours), None, None) == abi.ERR_BAD_ARG
    assert (out == 7.0).all()
    assert lib.nrays_debug_gather_sh_fold(*base, 3, fp(colours), fp(out), None) == abi.OK and (bits(out) == 0).all()


# ---- 8: the handle's state -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["analytic", "glass"])
def test_a_batch_leaves_the_render_state_alone(gpu, name):
    import torch
    from tests.test_gather_order_gpu import _tile_costs
    make = {"analytic": rich_analytic_scene, "glass": _glass_scene}[name]
    c = case("analytic")  # (points near the glass scene's shapes too: both scenes sit around the origin)
    L, rot = nr.hemisphere_dirs(16), nr.rotation_table(5)
    w, h = 128, 72

    def frames_and_stats(sc, cam, batch):
        proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], w, h)
        first = nr.render(sc, (w, h), 1, 0.0, cam["eye"], proj)
        st1, perm, costs = nr.get_stats(sc), nr.last_permutation(sc), _tile_costs(sc)
        got = None
        if batch:
            got = device_sh(sc, c["points"], c["normals"], L, rot, 1e-3, 1.0, 2, 3, keys=c["keys"], stream=torch.cuda.Stream(), unordered=True)
            assert np.array_equal(bits(nr.gather_sh_points(sc, c["points"], c["normals"], L, rot, 1e-3, 1.0, 2, 3, keys=c["keys"])), bits(got))  # unhinted, host form
        assert nr.last_permutation(sc) == perm and _tile_costs(sc) == costs
        second = nr.render(sc, (w, h), 1, 0.0, cam["eye"], proj)
        assert nr.last_permutation(sc) == perm
        return first, second, st1, nr.get_stats(sc), got

    plain = frames_and_stats(*make(), batch=False)
    mixed = frames_and_stats(*make(), batch=True)
    other, _ = make()
    assert np.array_equal(bits(mixed[4]), bits(nr.gather_sh_points(other, c["points"], c["normals"], L, rot, 1e-3, 1.0, 2, 3, keys=c["keys"])))  # (after a render, on another stream)
    assert (mixed[4] != 0.0).any()
    for a, b in zip(plain[:2], mixed[:2]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for st_plain, st_mixed in zip(plain[2:4], mixed[2:4]):
        for fld in STAT_FIELDS:
            assert getattr(st_plain, fld) == getattr(st_mixed, fld), fld
