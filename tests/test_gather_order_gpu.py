"""The reorder inside the gather call on the GPU (nrays_gather_points_device_ex / nrays_gather_points_ex with NRAYS_RAYS_UNORDERED; gather_points(unordered=True)):
the hinted result equals the unhinted one by bit pattern on every permutation of the trace kernel, where the queue runs and where the per-ray keys are read, for
sizes around a wave and across the chunk seam, in the host and the device form; skipped points; the probe (nrays_debug_gather_order) against nrays_debug_ray_order
on the same rays; the statuses; the handle's render state.  Every handle here is created under NRAYS_RAY_REORDER=2 (reorder whatever the size) unless a test says
otherwise, and the scenes are built here for that reason: the shared cases of the other modules may hold handles created without it (their POINTS are used)."""
import ctypes as C

import numpy as np
import pytest

import nrays_amd as nr
from nrays_amd import abi, math3d
from tests.test_gather_gpu import reference, scene_flags
from tests.test_occlusion_gpu import SCENES, STAT_FIELDS, bits, case, hit_points
from tests.test_shade_points import rich_analytic_scene
from tests.test_trace_rays_gpu import _glass_scene
from tools import scenes_util as su

pytestmark = pytest.mark.gpu
KS, NS = (1, 7, 16, 70), (1, 63, 65, 257)


@pytest.fixture(autouse=True)
def reorder_always(monkeypatch):
    monkeypatch.setenv("NRAYS_RAY_REORDER", "2")  # read when a handle is created


def _camera_points(sc, cam, w, h, seed, count=320):
    proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], w, h)
    o, d, _ = nr.camera_rays((w, h), cam["eye"], proj, seed=seed)
    hits = nr.closest_hits(sc, o, d, want=("normal", "flags"))
    p, nm = hit_points(o, d, hits)
    sel = np.flatnonzero((hits.flags & 1) != 0)
    sel = sel[np.linspace(0, len(sel) - 1, count).astype(int)]
    return np.ascontiguousarray(p[sel]), np.ascontiguousarray(nm[sel])


def _make(name):
    """A fresh scene (so that its handle is created under this module's switch) with 320 surface points, normals and odd keys."""
    keys = case("analytic")["keys"]
    if name in SCENES:
        c = case(name)
        return dict(scene=SCENES[name]()[0], points=c["points"], normals=c["normals"], keys=keys)
    if name == "no_elide":
        from tests.test_elision_gpu import _nonfinite_scene
        sc, cam = _nonfinite_scene("light")
        p, nm = _camera_points(sc, cam, 52, 30, 6)
    elif name == "area":
        sc, cam = su.primitives_scene(light_radius=0.1, nsample=3)
        p, nm = _camera_points(sc, cam, 40, 30, 2)
    else:
        sc, cam = _glass_scene()
        p, nm = _camera_points(sc, cam, 40, 30, 4)
    return dict(scene=sc, points=p, normals=nm, keys=keys)


_FRESH = {}


def fresh(name):
    """Per scene, made once under NRAYS_RAY_REORDER=2 and shared; nothing writes the arrays."""
    if name not in _FRESH:
        _FRESH[name] = _make(name)
        sc = _FRESH[name]["scene"]
        assert nr.gather_order(sc, _FRESH[name]["points"][:2], _FRESH[name]["normals"][:2], nr.hemisphere_dirs(4))[3][2]  # this handle reorders whatever the size
    return _FRESH[name]


def device_gather(sc, points, normals, L, rot=None, bias=1e-3, energy=1.0, max_depth=0, hit_flags=None, keys=None, stream=None, unordered=True):
    """gather_points on torch tensors (on `stream` when given), copied back."""
    import torch
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    tp, tn = up(points), up(normals)
    thf = None if hit_flags is None else up(np.ascontiguousarray(hit_flags, dtype=np.uint32).view(np.int32))
    tk = None if keys is None else up(np.ascontiguousarray(keys, dtype=np.uint64).view(np.int64))
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            r = nr.gather_points(sc, tp, tn, L, rot, bias, energy, max_depth, hit_flags=thf, keys=tk, unordered=unordered)
        stream.synchronize()
    else:
        r = nr.gather_points(sc, tp, tn, L, rot, bias, energy, max_depth, hit_flags=thf, keys=tk, unordered=unordered)
    torch.cuda.synchronize()
    assert r.dtype == torch.float32 and tuple(r.shape) == (len(points), 3)
    return r.cpu().numpy()


# ---- 1: bit identity ---------------------------------------------------------------------------------------------------------------------------------------
# hair: opaque meshes only, <false, kFeatMesh>; mixed: <false, kFeatAll>; no_elide: a non-finite light, <true, kFeatAll>; analytic and glass: double-branching,
# the queue runs with the pair as the pixel; area: an area light reads the per-ray keys.
@pytest.mark.parametrize("name", ["hair", "mixed", "no_elide", "analytic", "glass", "area"])
def test_hinted_equals_unhinted_bit_for_bit(gpu, name):
    import torch
    c = fresh(name)
    sc = c["scene"]
    flags = scene_flags(sc)
    assert ((flags & 8) != 0) == (name in ("analytic", "glass"))
    if name == "hair":
        assert (flags & ~16) == 2
    rot = nr.rotation_table(5)
    stream = torch.cuda.Stream()
    differ, nonzero = 0, 0
    for k in KS:
        L = nr.hemisphere_dirs(k)
        for n in NS:
            p, nm, keys = c["points"][:n], c["normals"][:n], c["keys"][:n]
            max_depth = 1 if (k + n) % 2 else 0
            plain = nr.gather_points(sc, p, nm, L, rot, 1e-3, 1.0, max_depth, keys=keys)
            host = nr.gather_points(sc, p, nm, L, rot, 1e-3, 1.0, max_depth, keys=keys, unordered=True)
            dev = device_gather(sc, p, nm, L, rot, 1e-3, 1.0, max_depth, keys=keys, stream=stream)
            bad = int((bits(host) != bits(plain)).any(axis=1).sum()) + int((bits(dev) != bits(plain)).any(axis=1).sum())
            print("%s k = %d n = %d max_depth = %d: %d points differ" % (name, k, n, max_depth, bad))
            differ += bad
            nonzero += int((plain != 0.0).any(axis=1).sum())
            assert host.shape == (n, 3) and host.dtype == np.float32
            assert np.array_equal(bits(host), bits(plain)) and np.array_equal(bits(dev), bits(plain))
    assert differ == 0 and nonzero > 500  # (of 1544 points in all: they really gather light)
    if name == "no_elide":
        assert (~np.isfinite(plain)).any()  # the case really produces non-finite colours


def test_hinted_equals_the_fold_of_trace_rays(gpu):
    """The definition itself, from parts that existed before: trace_rays on occlusion_rays() with gather_ray_keys(), folded in numpy f32."""
    c = fresh("mixed")
    for k, max_depth in ((16, 1), (7, 0)):
        L, rot = nr.hemisphere_dirs(k), nr.rotation_table(5)
        want = reference(c["scene"], c["points"], c["normals"], L, rot, 1e-3, 0.15, max_depth, c["keys"])
        got = nr.gather_points(c["scene"], c["points"], c["normals"], L, rot, 1e-3, 0.15, max_depth, keys=c["keys"], unordered=True)
        assert np.array_equal(bits(got), bits(want))
    c = fresh("area")
    L = nr.hemisphere_dirs(16)
    want = reference(c["scene"], c["points"], c["normals"], L, None, 1e-3, 1.0, 1, c["keys"])
    assert np.array_equal(bits(nr.gather_points(c["scene"], c["points"], c["normals"], L, None, 1e-3, 1.0, 1, keys=c["keys"], unordered=True)), bits(want))
    other = nr.gather_points(c["scene"], c["points"], c["normals"], L, None, 1e-3, 1.0, 1, keys=c["keys"] + np.uint64(2), unordered=True)
    assert (bits(other) != bits(want)).any()  # without rotations the rays are the same: only the light samples moved, so the rays' keys were read


# ---- 2: the chunk seam -------------------------------------------------------------------------------------------------------------------------------------
def test_across_the_chunk_seam_with_default_keys(gpu):
    """k = 16, n = 2^22 / 16 + 17: the second chunk holds 17 points (272 pairs in a grid sized for them) and its default keys go on from the first chunk's."""
    c = fresh("analytic")
    sc = c["scene"]
    n = (1 << 22) // 16 + 17
    L, rot = nr.hemisphere_dirs(16), nr.rotation_table(5)
    reps = -(-n // 320)
    p, nm = (np.ascontiguousarray(np.tile(a, (reps, 1))[:n]) for a in (c["points"], c["normals"]))
    plain = nr.gather_points(sc, p, nm, L, rot, 1e-3, 1.0, 1)
    host = nr.gather_points(sc, p, nm, L, rot, 1e-3, 1.0, 1, unordered=True)
    print("chunk seam: %d of %d points differ" % (int((bits(host) != bits(plain)).any(axis=1).sum()), n))
    assert np.array_equal(bits(host), bits(plain))
    assert (bits(host[:320]) != bits(host[320:640])).any()  # the same point under another key: another rotation somewhere
    tail = device_gather(sc, p[-17:], nm[-17:], L, rot, 1e-3, 1.0, 1, keys=np.arange(n - 17, n, dtype=np.uint64))
    assert np.array_equal(bits(tail), bits(host[-17:]))


# ---- 3: skipped points -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "analytic"])
@pytest.mark.parametrize("form", ["host", "device"])
def test_skipped_points_are_zero_and_leave_their_neighbours_alone(gpu, form, name):
    c = fresh(name)
    sc = c["scene"]
    L, rot = nr.hemisphere_dirs(16), nr.rotation_table(5)
    if form == "host":
        run = lambda p, nm, hf, keys, **kw: nr.gather_points(sc, p, nm, L, rot, 1e-3, 1.0, 1, hit_flags=hf, keys=keys, **kw)  # noqa: E731
    else:
        run = lambda p, nm, hf, keys, **kw: device_gather(sc, p, nm, L, rot, 1e-3, 1.0, 1, hit_flags=hf, keys=keys, **kw)  # noqa: E731
    n = 130
    p, nm, keys = c["points"][:n].copy(), c["normals"][:n].copy(), c["keys"][:n]
    base = run(p, nm, None, keys, unordered=False)
    assert (base != 0.0).any(axis=1).sum() > n // 2
    assert np.array_equal(bits(run(p, nm, None, keys, unordered=True)), bits(base))
    assert np.array_equal(bits(run(p, nm, np.full(n, 3, np.uint32), keys, unordered=True)), bits(base))
    skipped = np.arange(n) % 2 == 1
    hf = np.where(skipped, np.asarray([0, 2, 0xfffffffe, 0], np.uint32)[(np.arange(n) // 2) % 4], 1).astype(np.uint32)  # bit 0 clear, whatever else is set
    p[skipped], nm[skipped] = np.nan, np.nan
    p[1] = np.inf
    got = run(p, nm, hf, keys, unordered=True)
    assert (bits(got[skipped]) == 0).all()
    assert np.array_equal(bits(got[~skipped]), bits(base[~skipped]))
    p[:], nm[:] = np.nan, np.nan
    assert (bits(run(p, nm, np.zeros(n, np.uint32), keys, unordered=True)) == 0).all()  # a chunk without a live pair: zeros, no error


# ---- 4: the probe ------------------------------------------------------------------------------------------------------------------------------------------
def _bins(keys, K, B):
    return keys >> np.uint64(K - B)


@pytest.mark.parametrize("k, R", [(16, 5), (7, 0), (70, 3)])
def test_probe_equals_ray_order_on_the_same_rays(gpu, k, R):
    c = fresh("mixed")
    sc = c["scene"]
    n = 257
    p, nm, keys = c["points"][:n].copy(), c["normals"][:n].copy(), c["keys"][:n]
    L, rot = nr.hemisphere_dirs(k), nr.rotation_table(R) if R else None
    ro, rd = nr.occlusion_rays(p, nm, L, rot, 1e-3, keys)
    ro, rd = ro.reshape(-1, 3), rd.reshape(-1, 3)
    # every point live
    want_keys, _, want_frame, (K, B, _) = nr.ray_order(sc, ro, rd)
    got_keys, order, frame, info = nr.gather_order(sc, p, nm, L, rot, 1e-3, keys=keys)
    assert info == (K, B, True, n * k)
    assert np.array_equal(bits(frame), bits(want_frame)) and np.array_equal(got_keys, want_keys)
    assert np.array_equal(np.sort(order), np.arange(n * k)) and (np.diff(_bins(got_keys[order], K, B).astype(np.int64)) >= 0).all()
    assert len(np.unique(_bins(got_keys, K, B))) > 16  # (the order is a real one)
    # some points skipped, NaN behind them: the frame and the keys of the live rays only
    live = (np.arange(n) % 3 != 1) & (np.arange(n) != 0)
    hf = np.where(live, 3, 2).astype(np.uint32)
    p[~live], nm[~live] = np.nan, np.nan
    pairs = np.flatnonzero(np.repeat(live, k))
    want_keys, _, want_frame, _ = nr.ray_order(sc, ro[pairs], rd[pairs])
    got_keys, order, frame, info = nr.gather_order(sc, p, nm, L, rot, 1e-3, hit_flags=hf, keys=keys)
    assert info == (K, B, True, len(pairs))
    assert np.array_equal(bits(frame), bits(want_frame)) and np.array_equal(got_keys[pairs], want_keys)
    assert (got_keys[np.flatnonzero(~np.repeat(live, k))] == 0).all()  # a skipped point's entries: as the wrapper filled them
    assert np.array_equal(np.sort(order), pairs) and (np.diff(_bins(got_keys[order], K, B).astype(np.int64)) >= 0).all()
    # no live pair at all
    got_keys, order, frame, info = nr.gather_order(sc, p, nm, L, rot, 1e-3, hit_flags=np.zeros(n, np.uint32), keys=keys)
    assert info == (K, B, True, 0) and len(order) == 0 and (got_keys == 0).all()
    # default keys: point i has key i
    a = nr.gather_order(sc, c["points"][:n], c["normals"][:n], L, rot, 1e-3)
    b = nr.gather_order(sc, c["points"][:n], c["normals"][:n], L, rot, 1e-3, keys=np.arange(n, dtype=np.uint64))
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[2]), bits(b[2]))


@pytest.mark.parametrize("switch, small, large", [(None, False, True), ("2", True, True), ("0", False, False)])
def test_probe_reports_whether_a_hinted_call_is_reordered(gpu, monkeypatch, switch, small, large):
    """The rule of the ray batches on the call's n * num_dirs rays: from 2^19 by default (2^15 points x 16 directions), always under =2, never under =0."""
    if switch is None:
        monkeypatch.delenv("NRAYS_RAY_REORDER")
    else:
        monkeypatch.setenv("NRAYS_RAY_REORDER", switch)
    c = case("mixed")
    sc = SCENES["mixed"]()[0]
    L = nr.hemisphere_dirs(16)
    assert nr.gather_order(sc, c["points"][:100], c["normals"][:100], L)[3][2] is small
    reps = -(-(1 << 15) // 320)
    p, nm = (np.ascontiguousarray(np.tile(a, (reps, 1))) for a in (c["points"], c["normals"]))
    assert nr.gather_order(sc, p[:(1 << 15) - 1], nm[:(1 << 15) - 1], L)[3][2] is small
    assert nr.gather_order(sc, p[:1 << 15], nm[:1 << 15], L)[3][2] is large
    # whatever the handle decides, the values are the same
    plain = nr.gather_points(sc, c["points"], c["normals"], L, None, 1e-3, 1.0, 1)
    assert np.array_equal(bits(nr.gather_points(sc, c["points"], c["normals"], L, None, 1e-3, 1.0, 1, unordered=True)), bits(plain))


# ---- 5: statuses -------------------------------------------------------------------------------------------------------------------------------------------
def _raw_call(sc, form, n, arrays, params, flags=0, null=(), scene=True):
    """One call of an _ex entry point with host or device pointers; returns (status, out_rgb)."""
    import torch
    lib = abi.load_hip_lib()
    order = ("points", "normals", "hit_flags", "keys", "params", "out_rgb")
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
    if form == "device":
        rc = lib.nrays_gather_points_device_ex(h, n, *args, flags, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc, held["out_rgb"].cpu().numpy()
    return lib.nrays_gather_points_ex(h, n, *args, flags), arrays["out_rgb"]


@pytest.mark.parametrize("form", ["host", "device"])
def test_statuses(gpu, form):
    c = fresh("analytic")
    sc, n, k, R = c["scene"], 16, 8, 3
    arrays = dict(points=c["points"][:n].copy(), normals=c["normals"][:n].copy(), hit_flags=np.ones(n, np.uint32), keys=c["keys"][:n].copy(), out_rgb=np.full((n, 3), 7.0, np.float32))
    params = dict(num_dirs=k, num_rotations=R, dirs=nr.hemisphere_dirs(k), rotations=nr.rotation_table(R), bias=1e-3, energy=1.0, max_depth=1)
    call = lambda **kw: _raw_call(sc, form, kw.pop("n", n), arrays, dict(params, **kw.pop("p", {})), **kw)  # noqa: E731
    for flags in (2, 3, 1 << 31, (1 << 31) | 1):
        for n_ in (0, n):
            assert call(flags=flags, n=n_)[0] == abi.ERR_BAD_ARG, flags
    for flags in (0, 1):
        for name in ("points", "normals", "params", "out_rgb"):
            assert call(null=(name,), flags=flags)[0] == abi.ERR_BAD_ARG, name
        assert call(scene=False, flags=flags)[0] == abi.ERR_BAD_ARG
        for p in (dict(dirs=None), dict(num_dirs=0), dict(num_dirs=1025), dict(num_rotations=1025), dict(rotations=None), dict(bias=np.inf), dict(energy=np.nan)):
            assert call(p=p, flags=flags)[0] == abi.ERR_BAD_ARG, p
        rc, out = call(n=0, flags=flags)
        assert rc == abi.OK and (out == 7.0).all()  # without work; nothing so far wrote the output
    want = nr.gather_points(sc, arrays["points"], arrays["normals"], params["dirs"], params["rotations"], 1e-3, 1.0, 1, keys=arrays["keys"])
    for flags in (0, 1):
        rc, out = call(flags=flags)
        assert rc == abi.OK and np.array_equal(bits(out), bits(want))
    rc, out = call(flags=1, null=("hit_flags", "keys"), p=dict(num_rotations=0, rotations=None))  # every point live, key i; no rotation: a NULL table is fine
    assert rc == abi.OK and np.array_equal(bits(out), bits(nr.gather_points(sc, arrays["points"], arrays["normals"], params["dirs"], None, 1e-3, 1.0, 1)))


# ---- 6: the handle's state ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["analytic", "glass"])
def test_a_hinted_batch_leaves_the_render_state_alone(gpu, name):
    import torch
    make = {"analytic": rich_analytic_scene, "glass": _glass_scene}[name]
    c = case("analytic")  # (points near the glass scene's shapes too: both scenes sit around the origin)
    L, rot = nr.hemisphere_dirs(16), nr.rotation_table(5)
    w, h = 128, 72

    def frames_and_stats(sc, cam, batch):
        proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], w, h)
        first = nr.render(sc, (w, h), 1, 0.0, cam["eye"], proj)
        st1, perm, costs = nr.get_stats(sc), nr.last_permutation(sc), _tile_costs(sc)
        got = device_gather(sc, c["points"], c["normals"], L, rot, 1e-3, 1.0, 2, keys=c["keys"], stream=torch.cuda.Stream()) if batch else None
        assert nr.last_permutation(sc) == perm and _tile_costs(sc) == costs
        second = nr.render(sc, (w, h), 1, 0.0, cam["eye"], proj)
        assert nr.last_permutation(sc) == perm
        return first, second, st1, nr.get_stats(sc), got

    plain = frames_and_stats(*make(), batch=False)
    mixed = frames_and_stats(*make(), batch=True)
    other, _ = make()
    assert np.array_equal(bits(mixed[4]), bits(nr.gather_points(other, c["points"], c["normals"], L, rot, 1e-3, 1.0, 2, keys=c["keys"])))  # (after a render, on another stream)
    assert (mixed[4] != 0.0).any()
    for a, b in zip(plain[:2], mixed[:2]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for st_plain, st_mixed in zip(plain[2:4], mixed[2:4]):
        for fld in STAT_FIELDS:
            assert getattr(st_plain, fld) == getattr(st_mixed, fld), fld


def _tile_costs(sc):
    """What the handle reports about its last render's tiles, without the timing (nrays_get_tile_costs; the status too: not every frame records them)."""
    t = abi.NraysTileCosts()
    rc = abi.load_hip_lib().nrays_get_tile_costs(sc.device_handle(), C.byref(t))
    return (rc, t.tiles, t.sum_cycles, t.max_cycles, t.resident_waves)
