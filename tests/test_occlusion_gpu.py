"""Ambient occlusion at caller-supplied points (nrays_occlusion_points_device / nrays_occlusion_points; nrays_amd.occlusion_points, occlusion_hits) on the
GPU: the library's own rays against the numpy mirror bit for bit (nrays_debug_occlusion_rays), the fused outputs against the fold of intersects_rays on
those very rays bit for bit, the CPU oracle's expectation (tests/test_occlusion.py), sizes around a wave and across the chunk seam, every number of lanes
per point, skipped points, the NULL output, the device path, occlusion_hits, the statuses, and the handle's render state."""
import ctypes as C
import math

import numpy as np
import pytest

import nrays_amd as nr
from nrays_amd import abi, math3d
from tests.test_occlusion import SPECIAL_NORMALS, call_args, fold, oracle_case, quad_scene, unit_normals
from tests.test_shade_points import opaque, rich_analytic_scene, scattered_rays
from tests.test_trace_rays import analytic_scene
from tools import scenes_util as su
from tools import standins

pytestmark = pytest.mark.gpu
ORACLE_TOL = 4.0 * 2.0 ** -24  # DESIGN §3's derived bound for a bilinear sample; the mean of k such values keeps it
STAT_FIELDS = ("rays_primary", "rays_reflection", "rays_refraction", "rays_shadow", "rays_shadow_elided", "rays_primary_traced", "generations")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


# ---- scenes -------------------------------------------------------------------------------------------------------------------------------------------------
def _camera(cam, w, h, seed):
    proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], w, h)
    o, d, _ = nr.camera_rays((w, h), cam["eye"], proj, seed=seed)
    return o, d


def _tiny():
    """Two balls, a box and a PLANE, every node opaque: few enough leaves for the stackless queries of a render; the batch queries visit the plane as a pseudo-leaf."""
    sc, cam = analytic_scene()
    return (opaque(sc), cam) + _camera(cam, 40, 30, 1)


def _analytic():
    """Nine shapes and a plane — a TLAS to walk —, three of them half-transparent."""
    sc, cam = rich_analytic_scene()
    return (sc, cam) + scattered_rays(np.random.default_rng(41), 1500)


def _hair():
    """Opaque meshes only: the kFeatMesh kernels."""
    sc, cam = standins.hairball_scene(strands=400)
    return (sc, cam) + _camera(cam, 48, 48, 3)


def _quads():
    """Meshes only, one with an opacity map (texels 0, 0.5 and 1) and a colour texture."""
    sc, cam = quad_scene()
    return (sc, cam) + _camera(cam, 40, 40, 9)


def _mixed():
    """The quads with a half-transparent ball and an opaque capsule standing on the floor: meshes and analytic shapes in one TLAS."""
    q, cam = quad_scene()
    glass = nr.PhongMaterial((0.1, 0.1, 0.15), (0.6, 0.7, 0.9), (1, 1, 1), None, None, 80.0)
    nodes = list(q._nodes) + [nr.SceneNode(glass, 0.0, 0.0, 0.5, 1.0, nr.Isometry3((0.9, 0.45, 0.2)), nr.Ball(0.45)),
                              nr.SceneNode(su.default_material(), 0.0, 0.0, 1.0, 1.0, nr.Isometry3((-1.0, 0.5, -0.6)), nr.Capsule(0.3, 0.2))]
    return (nr.Scene(nodes, q._lights, q._background), cam) + _camera(cam, 40, 40, 9)


SCENES = {"tiny": _tiny, "analytic": _analytic, "hair": _hair, "quads": _quads, "mixed": _mixed}
FINITE_TOI = {"tiny": 2.5, "analytic": 2.5, "hair": 0.5, "quads": 1.5, "mixed": 1.5}
_CASES = {}


def hit_points(o, d, hits):
    """What occlusion_hits() builds from a numpy CastHits: the points, and the normals on the side the rays came from."""
    toi = np.where((hits.flags & 1) != 0, hits.toi, 0.0)
    step = d * toi[:, None]
    nm = hits.normal
    facing = (nm[:, 0] * d[:, 0] + nm[:, 1] * d[:, 1]) + nm[:, 2] * d[:, 2]
    return o + step, np.where((facing > 0)[:, None], -nm, nm)


def case(name):
    """Per scene, computed once and shared (nothing writes them): the scene, its rays and their closest hits, and 320 surface points with normals and odd keys."""
    if name not in _CASES:
        sc, cam, o, d = SCENES[name]()
        hits = nr.closest_hits(sc, o, d, want=("normal", "flags"))
        p, nm = hit_points(o, d, hits)
        sel = np.flatnonzero((hits.flags & 1) != 0)
        sel = sel[np.linspace(0, len(sel) - 1, 320).astype(int)]
        assert len(np.unique(sel)) > 250
        keys = np.random.default_rng(5).integers(0, 2**63, size=320, dtype=np.int64).astype(np.uint64) * np.uint64(2) + np.uint64(1)
        _CASES[name] = dict(scene=sc, cam=cam, o=o, d=d, hits=hits, points=np.ascontiguousarray(p[sel]), normals=np.ascontiguousarray(nm[sel]), keys=keys)
    return _CASES[name]


def reference(sc, points, normals, L, rot, bias, max_toi, keys):
    """The definition, from parts that existed before: the mirror's rays through intersects_rays, folded in numpy f32 in the order of j."""
    ro, rd = nr.occlusion_rays(points, normals, L, rot, bias, keys)
    n, k = ro.shape[:2]
    lit, filt = nr.intersects_rays(sc, ro.reshape(-1, 3), rd.reshape(-1, 3), np.full(n * k, max_toi))
    return fold(filt.reshape(n, k, 3), lit.reshape(n, k))


def device_occlusion(sc, points, normals, L, rot=None, bias=1e-3, max_toi=math.inf, hit_flags=None, keys=None, stream=None):
    """occlusion_points on torch tensors (on `stream` when given), copied back: (filter, open uint32)."""
    import torch
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    tp, tn = up(points), up(normals)
    thf = None if hit_flags is None else up(np.ascontiguousarray(hit_flags, dtype=np.uint32).view(np.int32))
    tk = None if keys is None else up(np.ascontiguousarray(keys, dtype=np.uint64).view(np.int64))
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            r = nr.occlusion_points(sc, tp, tn, L, rot, bias, max_toi, hit_flags=thf, keys=tk)
        stream.synchronize()
    else:
        r = nr.occlusion_points(sc, tp, tn, L, rot, bias, max_toi, hit_flags=thf, keys=tk)
    torch.cuda.synchronize()
    assert r.filter.dtype == torch.float32 and tuple(r.filter.shape) == (len(points), 3) and r.open.dtype == torch.int32 and tuple(r.open.shape) == (len(points),)
    return r.filter.cpu().numpy(), r.open.cpu().numpy().view(np.uint32)


# ---- 1: the library's rays are the mirror's --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [0, 5])
def test_probe_rays_equal_the_mirror_bit_for_bit(gpu, R):
    """The check that finds a contracted or reordered operation: every double of every ray, by bit pattern."""
    c = case("analytic")
    rng = np.random.default_rng(11)
    nm = np.concatenate([c["normals"], unit_normals(rng, 3000), SPECIAL_NORMALS])
    p = np.concatenate([c["points"], rng.uniform(-50.0, 50.0, size=(len(nm) - len(c["points"]), 3))])
    keys = rng.integers(0, 2**63, size=len(nm), dtype=np.int64).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    rot = nr.rotation_table(R) if R else None
    for L, bias, k in ((nr.hemisphere_dirs(16), 1e-3, keys), (nr.hemisphere_dirs(7, cosine=False), 0.37, None), (np.asarray([(-0.0, 0.0, 1.0), (0.3, -0.4, 0.5)]), 0.0, keys)):
        mo, md = nr.occlusion_rays(p, nm, L, rot, bias, k)
        po, pd = nr.occlusion_ray_probe(c["scene"], p, nm, L, rot, bias, k)
        print("R = %d, k = %d: %d of %d doubles differ" % (R, len(L), int((bits(md) != bits(pd)).sum() + (bits(mo) != bits(po)).sum()), 2 * md.size))
        assert np.array_equal(bits(mo), bits(po)) and np.array_equal(bits(md), bits(pd))
    if R:  # the keys matter, and the default key of point i is i
        assert not np.array_equal(md, nr.occlusion_rays(p, nm, L, rot, bias, None)[1])
        assert np.array_equal(bits(nr.occlusion_ray_probe(c["scene"], p, nm, L, rot, bias, None)[1]), bits(nr.occlusion_ray_probe(c["scene"], p, nm, L, rot, bias, np.arange(len(p)))[1]))


# ---- 2: the fused outputs are the fold of intersects_rays on those rays -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SCENES))
def test_equals_the_fold_of_intersects_rays_bit_for_bit(gpu, name):
    c = case(name)
    sc = c["scene"]
    if name in ("hair", "quads"):
        flags = (C.c_uint32 * 2)()
        abi.check(abi.load_hip_lib().nrays_debug_scene_flags(sc.device_handle(), flags))
        assert (flags[0] & ~16) == 2 if name == "hair" else (flags[0] & 7) == 6  # opaque meshes only: the kFeatMesh kernel; with the opacity map: kFeatAll
    seen_open, seen_partial = 0, 0
    for k in (1, 2, 7, 16):
        L = nr.hemisphere_dirs(k)
        for R in (0, 5):
            rot = nr.rotation_table(R) if R else None
            for max_toi in (math.inf, FINITE_TOI[name]):
                want_f, want_o = reference(sc, c["points"], c["normals"], L, rot, 1e-3, max_toi, c["keys"])
                got = nr.occlusion_points(sc, c["points"], c["normals"], L, rot, 1e-3, max_toi, keys=c["keys"])
                bad = int((bits(got.filter) != bits(want_f)).any(axis=1).sum() + (got.open != want_o).sum())
                print("%s k = %d R = %d max_toi = %s: %d points differ; open rays %d of %d" % (name, k, R, max_toi, bad, int(want_o.sum()), want_o.size * k))
                assert got.filter.dtype == np.float32 and got.open.dtype == np.uint32
                assert np.array_equal(bits(got.filter), bits(want_f)) and np.array_equal(got.open, want_o)
                seen_open += int(want_o.sum())
                seen_partial += int(((want_f > 0.0) & (want_f < 1.0)).any(axis=1).sum())
    assert seen_open > 1000 and seen_partial > 100  # (open and blocked rays both; means that are neither 0 nor 1)
    if name in ("analytic", "quads", "mixed"):  # colour filters of transparent hits, not only 0 and 1 per ray
        got = nr.occlusion_points(sc, c["points"], c["normals"], nr.hemisphere_dirs(1), None, 1e-3, math.inf)
        assert ((got.filter > 0.0) & (got.filter < 1.0)).any()


@pytest.mark.parametrize("k", [16, 20, 64, 70])
def test_every_number_of_lanes_per_point_gives_the_same_values(gpu, k, monkeypatch):
    """A point gets 8 or 64 lanes (k >= 8, k >= 64), on a forced handle any of 1, 8, 64; k = 20 and 70 leave a partial last round.  All of them are the sequential
    fold."""
    c = case("analytic")
    L, rot = nr.hemisphere_dirs(k), nr.rotation_table(5)
    n = 257
    p, nm, keys = c["points"][:n], c["normals"][:n], c["keys"][:n]
    want_f, want_o = reference(c["scene"], p, nm, L, rot, 1e-3, math.inf, keys)
    assert 0 < want_o.sum() < n * k
    got = nr.occlusion_points(c["scene"], p, nm, L, rot, 1e-3, math.inf, keys=keys)
    assert np.array_equal(bits(got.filter), bits(want_f)) and np.array_equal(got.open, want_o)
    for lanes in ("0", "3", "6"):
        monkeypatch.setenv("NRAYS_OCCLUSION_LANES", lanes)  # read when the handle is created
        sc, _ = rich_analytic_scene()
        got = nr.occlusion_points(sc, p, nm, L, rot, 1e-3, math.inf, keys=keys)
        assert np.array_equal(bits(got.filter), bits(want_f)) and np.array_equal(got.open, want_o), lanes


# ---- 3: the oracle's expectation ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["analytic", "quads"])
def test_against_the_cpu_oracle(gpu, name):
    c = oracle_case(name)
    got = nr.occlusion_points(c["scene"], **call_args(c))
    err = float(np.abs(got.filter - c["filter"]).max())
    print("%s: max |hip - oracle| %.3g (bound %.3g), open counts differ at %d of %d points" % (name, err, ORACLE_TOL, int((got.open != c["open"]).sum()), len(c["open"])))
    assert np.array_equal(got.open, c["open"])
    assert err <= ORACLE_TOL


# ---- 4: sizes, pieces, keys, the device path -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, (1 << 22) // 16 + 17])
def test_sizes_pieces_default_keys_and_the_device_path(gpu, n):
    """The 320 points of the analytic case tiled to n, k = 16 with 5 rotations (the keys matter).  Default keys: point i has key i, also across the chunk seam at
    2^22 / 16 points.  The host form against the device form on a stream of its own."""
    import torch
    c = case("analytic")
    sc = c["scene"]
    L, rot = nr.hemisphere_dirs(16), nr.rotation_table(5)
    reps = -(-n // 320)
    p, nm = (np.ascontiguousarray(np.tile(a, (reps, 1))[:n]) for a in (c["points"], c["normals"]))
    host = nr.occlusion_points(sc, p, nm, L, rot, 1e-3, 2.5)
    assert host.filter.shape == (n, 3) and host.open.shape == (n,)
    dev_f, dev_o = device_occlusion(sc, p, nm, L, rot, 1e-3, 2.5, stream=torch.cuda.Stream())
    assert np.array_equal(bits(dev_f), bits(host.filter)) and np.array_equal(dev_o, host.open)
    if n <= 64:
        f, o = device_occlusion(sc, p, nm, L, rot, 1e-3, 2.5, keys=np.arange(n, dtype=np.uint64))
        assert np.array_equal(bits(f), bits(host.filter)) and np.array_equal(o, host.open)
    else:  # (pieces under explicit keys against one call under the default keys)
        cuts = [0, n // 3, n // 3 + 1, n - 5, n]
        parts = [device_occlusion(sc, p[a:b], nm[a:b], L, rot, 1e-3, 2.5, keys=np.arange(a, b, dtype=np.uint64)) for a, b in zip(cuts[:-1], cuts[1:])]
        assert np.array_equal(bits(np.concatenate([f for f, _ in parts])), bits(host.filter)) and np.array_equal(np.concatenate([o for _, o in parts]), host.open)
    if n <= 320:  # against the definition, under the default keys
        want_f, want_o = reference(sc, p, nm, L, rot, 1e-3, 2.5, None)
        assert np.array_equal(bits(host.filter), bits(want_f)) and np.array_equal(host.open, want_o)
    if n > 640:  # the same point under another key: another rotation somewhere
        assert (bits(host.filter[:320]) != bits(host.filter[320:640])).any()
        tail = device_occlusion(sc, p[-17:], nm[-17:], L, rot, 1e-3, 2.5, keys=np.arange(n - 17, n, dtype=np.uint64))
        assert np.array_equal(bits(tail[0]), bits(host.filter[-17:])) and np.array_equal(tail[1], host.open[-17:])


# ---- 5: skipped points, the NULL output ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("k", [4, 16])
def test_skipped_points_are_zero_and_leave_their_neighbours_alone(gpu, form, k):
    """k = 4: a lane per point; k = 16: eight lanes per point."""
    c = case("mixed")
    sc = c["scene"]
    L, rot = nr.hemisphere_dirs(k), nr.rotation_table(5)
    if form == "host":
        run = lambda p, nm, hf, keys: tuple(nr.occlusion_points(sc, p, nm, L, rot, 1e-3, math.inf, hit_flags=hf, keys=keys))  # noqa: E731
    else:
        run = lambda p, nm, hf, keys: device_occlusion(sc, p, nm, L, rot, 1e-3, math.inf, hit_flags=hf, keys=keys)  # noqa: E731
    n = 130
    p, nm, keys = c["points"][:n].copy(), c["normals"][:n].copy(), c["keys"][:n]
    base_f, base_o = run(p, nm, None, keys)
    assert base_o.sum() > 0
    lanes = [0, 31, 63, 64, 129]
    keep = np.setdiff1d(np.arange(n), lanes)
    f, o = run(p[keep], nm[keep], np.full(len(keep), 3, np.uint32), keys[keep])
    assert np.array_equal(bits(f), bits(base_f[keep])) and np.array_equal(o, base_o[keep])
    hf = np.full(n, 1, np.uint32)
    hf[lanes] = [0, 2, 0xfffffffe, 0, 2]  # bit 0 clear, whatever else is set
    p[lanes], nm[lanes] = np.nan, np.nan
    p[lanes[1]] = np.inf
    f, o = run(p, nm, hf, keys)
    assert (bits(f[lanes]) == 0).all() and (o[lanes] == 0).all()
    assert np.array_equal(bits(f[keep]), bits(base_f[keep])) and np.array_equal(o[keep], base_o[keep])
    f, o = run(p, nm, np.zeros(n, np.uint32), keys)  # every point skipped
    assert (bits(f) == 0).all() and (o == 0).all()


def _raw_call(sc, form, n, arrays, params, flags=0, null=(), scene=True, stream=None):
    """One library call with host or device pointers; returns (status, out_filter, out_open) as numpy arrays."""
    import torch
    lib = abi.load_hip_lib()
    order = ("points", "normals", "hit_flags", "keys", "params", "out_filter", "out_open")
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
    st = abi.NraysOcclusionParams(params["num_dirs"], params["num_rotations"], adr(tables["dirs"]), adr(tables["rotations"]), params["bias"], params["max_toi"])
    ptrs["params"] = C.byref(st)
    args = [None if k in null else ptrs[k] for k in order]
    if form == "device":
        rc = lib.nrays_occlusion_points_device(h, n, *args, flags, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc, held["out_filter"].cpu().numpy(), held["out_open"].cpu().numpy().view(np.uint32)
    return lib.nrays_occlusion_points(h, n, *args, flags), arrays["out_filter"], arrays["out_open"]


def _raw_setup(n=16, k=8, R=3):
    c = case("analytic")
    arrays = dict(points=c["points"][:n].copy(), normals=c["normals"][:n].copy(), hit_flags=np.ones(n, np.uint32), keys=c["keys"][:n].copy(),
                  out_filter=np.full((n, 3), 7.0, np.float32), out_open=np.full(n, 7, np.uint32))
    params = dict(num_dirs=k, num_rotations=R, dirs=nr.hemisphere_dirs(k), rotations=nr.rotation_table(R), bias=1e-3, max_toi=math.inf)
    return c, arrays, params


@pytest.mark.parametrize("form", ["host", "device"])
def test_out_open_may_be_null(gpu, form):
    c, arrays, params = _raw_setup()
    want = nr.occlusion_points(c["scene"], arrays["points"], arrays["normals"], params["dirs"], params["rotations"], 1e-3, math.inf, keys=arrays["keys"])
    rc, f, o = _raw_call(c["scene"], form, 16, arrays, params, null=("out_open",))
    assert rc == abi.OK and np.array_equal(bits(f), bits(want.filter)) and (o == 7).all()  # nothing was stored there
    rc, f, o = _raw_call(c["scene"], form, 16, arrays, params)
    assert rc == abi.OK and np.array_equal(bits(f), bits(want.filter)) and np.array_equal(o, want.open)
    rc, f, o = _raw_call(c["scene"], form, 16, arrays, params, null=("hit_flags", "keys"))
    want = nr.occlusion_points(c["scene"], arrays["points"], arrays["normals"], params["dirs"], params["rotations"], 1e-3, math.inf)
    assert rc == abi.OK and np.array_equal(bits(f), bits(want.filter)) and np.array_equal(o, want.open)


# ---- statuses -------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "device"])
def test_statuses(gpu, form):
    c, arrays, params = _raw_setup()
    sc = c["scene"]
    call = lambda **kw: _raw_call(sc, form, kw.pop("n", 16), arrays, dict(params, **kw.pop("p", {})), **kw)  # noqa: E731
    for flags in (1, 2, 1 << 31, 3):
        assert call(flags=flags)[0] == abi.ERR_BAD_ARG, flags
    for name in ("points", "normals", "params", "out_filter"):
        assert call(null=(name,))[0] == abi.ERR_BAD_ARG, name
    assert call(scene=False)[0] == abi.ERR_BAD_ARG
    bad_params = [dict(dirs=None), dict(num_dirs=0), dict(num_dirs=1025), dict(num_rotations=1025), dict(rotations=None), dict(max_toi=math.nan), dict(max_toi=0.0),
                  dict(max_toi=-1.0), dict(max_toi=-math.inf), dict(bias=math.inf), dict(bias=-math.inf), dict(bias=math.nan)]
    for p in bad_params:
        assert call(p=p)[0] == abi.ERR_BAD_ARG, p
    rc, f, o = call(n=0)
    assert rc == abi.OK and (f == 7.0).all() and (o == 7).all()  # without work; nothing so far wrote the outputs
    assert call(n=0, flags=1)[0] == abi.ERR_BAD_ARG and call(n=0, p=dict(num_dirs=0))[0] == abi.ERR_BAD_ARG
    rc, f, o = call(p=dict(num_rotations=0, rotations=None))  # no rotation: a NULL table is fine
    want = nr.occlusion_points(sc, arrays["points"], arrays["normals"], params["dirs"], None, 1e-3, math.inf)
    assert rc == abi.OK and np.array_equal(bits(f), bits(want.filter)) and np.array_equal(o, want.open)
    # the probe's checks
    lib = abi.load_hip_lib()
    dp = C.POINTER(C.c_double)
    p, nm = arrays["points"], arrays["normals"]
    L = np.ascontiguousarray(params["dirs"])
    ro, rd = np.full((16, 8, 3), 7.0), np.full((16, 8, 3), 7.0)
    st = abi.NraysOcclusionParams(8, 0, L.ctypes.data, None, 1e-3, math.inf)
    good = [sc.device_handle(), 16, p.ctypes.data_as(dp), nm.ctypes.data_as(dp), None, C.byref(st), ro.ctypes.data_as(dp), rd.ctypes.data_as(dp)]
    for i in (0, 2, 3, 5, 6, 7):
        assert lib.nrays_debug_occlusion_rays(*[None if j == i else a for j, a in enumerate(good)]) == abi.ERR_BAD_ARG, i
    assert lib.nrays_debug_occlusion_rays(*[0 if j == 1 else a for j, a in enumerate(good)]) == abi.OK and (ro == 7.0).all()
    assert lib.nrays_debug_occlusion_rays(*good) == abi.OK and np.array_equal(bits(rd), bits(nr.occlusion_rays(p, nm, L, None, 1e-3)[1]))


# ---- occlusion_hits -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["quads", "tiny"])
def test_occlusion_hits_on_tensors_equals_the_numpy_form(gpu, name):
    import torch
    c = case(name)
    sc, o, d = c["scene"], c["o"], c["d"]
    L, rot = nr.hemisphere_dirs(7), nr.rotation_table(4)
    want = nr.occlusion_hits(sc, o, d, c["hits"], L, rot, 1e-3, 4.0)
    hit = (c["hits"].flags & 1) != 0
    assert hit.sum() > 300 and (name != "tiny" or (~hit).sum() > 50)  # (the tiny scene's camera sees the sky)
    assert (bits(want.filter[~hit]) == 0).all() and (want.open[~hit] == 0).all() and want.open[hit].sum() > 0
    p, nm = hit_points(o, d, c["hits"])
    direct = nr.occlusion_points(sc, p, nm, L, rot, 1e-3, 4.0, hit_flags=c["hits"].flags)
    assert np.array_equal(bits(want.filter), bits(direct.filter)) and np.array_equal(want.open, direct.open)
    assert (((nm * d).sum(axis=1) <= 0) | ~hit).all()  # every normal faces its ray
    to, td = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = nr.occlusion_hits(sc, to, td, nr.closest_hits(sc, to, td), L, rot, 1e-3, 4.0)
    s.synchronize()
    assert np.array_equal(bits(got.filter.cpu().numpy()), bits(want.filter)) and np.array_equal(got.open.cpu().numpy().view(np.uint32), want.open)
    assert np.array_equal(bits(sc.occlusion_points(p, nm, L, rot, 1e-3, 4.0, hit_flags=c["hits"].flags).filter), bits(want.filter))  # Scene.occlusion_points
    with pytest.raises(ValueError):
        nr.occlusion_hits(sc, to, td, c["hits"], L)  # tensors and arrays mixed


# ---- the handle's state -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["analytic", "quads"])
def test_a_batch_leaves_the_render_state_alone(gpu, name):
    import torch
    c = case(name)
    sc, cam = {"analytic": rich_analytic_scene, "quads": quad_scene}[name]()
    L, rot = nr.hemisphere_dirs(16), nr.rotation_table(5)
    want = nr.occlusion_points(c["scene"], c["points"], c["normals"], L, rot, 1e-3, math.inf, keys=c["keys"])
    w, h = 128, 72
    proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], w, h)
    first = nr.render(sc, (w, h), 1, 0.0, cam["eye"], proj)
    st1, perm1 = nr.get_stats(sc), nr.last_permutation(sc)
    f, o = device_occlusion(sc, c["points"], c["normals"], L, rot, 1e-3, math.inf, keys=c["keys"], stream=torch.cuda.Stream())
    assert np.array_equal(bits(f), bits(want.filter)) and np.array_equal(o, want.open)  # (a fresh handle of the same scene, after a render, on another stream)
    assert nr.last_permutation(sc) == perm1
    second = nr.render(sc, (w, h), 1, 0.0, cam["eye"], proj)
    st2 = nr.get_stats(sc)
    assert np.array_equal(first.view(np.uint32), second.view(np.uint32))
    assert nr.last_permutation(sc) == perm1
    for fld in STAT_FIELDS:
        assert getattr(st1, fld) == getattr(st2, fld), fld
