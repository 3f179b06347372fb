"""Closest-hit queries on caller-supplied rays (nrays_cast_rays_device / nrays_cast_rays; nrays_amd.closest_hits) on the GPU: bit for bit
against the test probe nrays_debug_cast_batch (k_cast_batch mode 0, the yardstick), against the fixtures derived independently of this code
base, the triangle index, the optional outputs, max_toi as a filter of the finished query, the unordered hint, the handle's render state
and the blocking host form."""
import ctypes as C
import math

import numpy as np
import pytest

import nrays_amd as nr
from nrays_amd import abi, math3d
from tests import test_kat_independent as kat
from tools import scenes_util as su
from tools import standins

pytestmark = pytest.mark.gpu

FIELDS = nr.CastHits._fields
RECORD = np.dtype([("toi", "<f8"), ("normal", "<f8", (3,)), ("uv", "<f8", (2,)), ("node", "<i4"), ("flags", "<u4")])  # NraysCastResult
STAT_FIELDS = ("rays_primary", "rays_reflection", "rays_refraction", "rays_shadow", "rays_shadow_elided", "rays_primary_traced", "generations")
INF_BITS = np.float64(np.inf).view(np.uint64)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a.astype(np.int64)


def probe(sc, o, d):
    """nrays_debug_cast_batch mode 0 on the rays: one NraysCastResult per ray, as a structured array."""
    n = len(o)
    res = (abi.NraysCastResult * n)()
    dp = C.POINTER(C.c_double)
    abi.check(abi.load_hip_lib().nrays_debug_cast_batch(sc.device_handle(), 0, n, np.ascontiguousarray(o).ctypes.data_as(dp), np.ascontiguousarray(d).ctypes.data_as(dp), None, res))
    assert C.sizeof(abi.NraysCastResult) == RECORD.itemsize
    return np.frombuffer(res, dtype=RECORD).copy()


def device_cast(sc, o, d, max_toi=None, stream=None, **kw):
    """The device form on torch tensors (on `stream` when given), copied back: a dict of numpy arrays, None for an output not wanted."""
    import torch
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()  # noqa: E731
    to, td, tt = up(o), up(d), up(max_toi)
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            r = nr.closest_hits(sc, to, td, tt, **kw)
        stream.synchronize()
    else:
        r = nr.closest_hits(sc, to, td, tt, **kw)
    torch.cuda.synchronize()
    return {k: None if v is None else v.cpu().numpy() for k, v in r._asdict().items()}


def assert_same(a, b, what=""):
    """Two results equal in every output both carry, bit for bit."""
    for k in FIELDS:
        if a[k] is None or b[k] is None:
            continue
        assert a[k].shape == b[k].shape, (what, k)
        ne = bits(a[k]) != bits(b[k])
        assert not ne.any(), "%s: %d values of %s differ" % (what, int(ne.sum()), k)


def assert_misses(r, m):
    """The rays of mask m carry the documented miss values."""
    assert (r["node"][m] == -1).all() and (bits(r["toi"][m]) == INF_BITS).all()
    assert (bits(r["normal"][m]) == 0).all() and (bits(r["uv"][m]) == 0).all()
    assert (r["prim"][m] == -1).all() and (r["flags"][m] == 0).all()


def filtered(r, keep):
    """The unbounded result `r` with the rays outside `keep` turned into misses, on the host."""
    out = {k: v.copy() for k, v in r.items()}
    m = ~keep
    out["toi"][m] = np.inf; out["node"][m] = -1; out["normal"][m] = 0.0; out["uv"][m] = 0.0; out["prim"][m] = -1; out["flags"][m] = 0
    return out


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------------
def mixed_scene():
    """One node of each of the seven shape kinds; the cuboid, the cone and the mesh (a small torus with uvs) are rotated."""
    white, tex = su.default_material(), nr.PhongMaterial((0.2, 0.2, 0.2), (1, 1, 1), (0.5, 0.5, 0.5), su.checker_texture(32, 4), None, 60.0)
    iso = nr.Isometry3
    pts, idx, uvs = su.torus_mesh(12, 8, 0.9, 0.35)
    nodes = [nr.SceneNode(nr.UVMaterial(), 0.0, 0.0, 1.0, 1.0, iso((-3.0, 0.0, 0.0)), nr.Ball(0.9)),
             nr.SceneNode(white, 0.0, 0.0, 1.0, 1.0, iso((-1.0, 0.2, 1.0), (0.3, 0.5, -0.2)), nr.Cuboid((0.6, 0.8, 0.5))),
             nr.SceneNode(nr.NormalMaterial(), 0.0, 0.0, 1.0, 1.0, iso((1.2, 0.0, 0.5)), nr.Cylinder(0.8, 0.5)),
             nr.SceneNode(white, 0.0, 0.0, 1.0, 1.0, iso((3.0, 0.3, 0.0)), nr.Capsule(0.6, 0.4)),
             nr.SceneNode(tex, 0.0, 0.0, 1.0, 1.0, iso((0.0, 2.2, 1.0), (0.0, 0.0, math.radians(35.0))), nr.Cone(0.7, 0.6)),
             nr.SceneNode(white, 0.0, 0.0, 1.0, 1.0, iso((0.0, -1.5, 0.0)), nr.Plane((0.0, 1.0, 0.0))),
             nr.SceneNode(tex, 0.0, 0.0, 1.0, 1.0, iso((0.5, -0.3, -1.5), (math.radians(25.0), math.radians(20.0), 0.0)), nr.TriMesh(pts, idx, uvs))]
    return nr.Scene(nodes, [nr.Light((0.0, 10.0, -3.0), 0.0, 1, (1, 1, 1))]), dict(eye=(0.5, 3.0, -9.0), at=(0.0, 0.0, 0.0), fovy=50.0)


def small_mesh_scene():
    """Opaque meshes only (two BLASes: a rotated torus with uvs, a floor without): the kFeatMesh instantiation."""
    pts, idx, uvs = su.torus_mesh(16, 8)
    tex = nr.PhongMaterial((0.2, 0.2, 0.2), (1, 1, 1), (0.5, 0.5, 0.5), su.checker_texture(32, 4), None, 60.0)
    fl = su.f32_exact([[-6, -1.25, -6], [6, -1.25, -6], [6, -1.25, 6], [-6, -1.25, 6]])
    fl_idx = np.asarray([[0, 2, 1], [0, 3, 2]], dtype=np.uint32)
    nodes = [nr.SceneNode(tex, 0.0, 0.0, 1.0, 1.0, nr.Isometry3((0.0, 0.0, 0.0), (0.0, math.radians(20.0), math.radians(10.0))), nr.TriMesh(pts, idx, uvs)),
             nr.SceneNode(su.default_material(), 0.0, 0.0, 1.0, 1.0, nr.Isometry3(), nr.TriMesh(fl, fl_idx))]
    return nr.Scene(nodes, [nr.Light((3.0, 6.0, -6.0), 0.0, 1, (1, 1, 1))]), dict(eye=(0.5, 3.0, -9.0), at=(0.0, 0.0, 0.0), fovy=40.0)


SCENES = {
    "mixed": mixed_scene,
    "mesh_only": small_mesh_scene,
    "hair": lambda: standins.hairball_scene(strands=150),  # tests/test_node_quorum_gpu.py's builder at its smallest size
    "tiny_balls": lambda: su.balls_scene(tex_size=(256, 128)),
}
SCENE_FLAGS = {"mesh_only": (2, 0), "hair": (2, 1)}  # nrays_debug_scene_flags: opaque meshes only (hair-like: quorum-ended node phases)


def fan(cam, w, h):
    proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], w, h)
    o, d, _ = nr.camera_rays((w, h), cam["eye"], proj)
    return o, d


def away_rays(n, seed):
    """Rays that start above everything and point further up: no shape is ahead of them (the planes of these scenes face up and lie below)."""
    rng = np.random.default_rng(seed)
    o = np.stack([rng.uniform(-4, 4, n), np.full(n, 20.0), rng.uniform(-4, 4, n)], 1)
    d = np.stack([rng.uniform(-1, 1, n), rng.uniform(0.5, 1.5, n), rng.uniform(-1, 1, n)], 1)
    return o, d / np.linalg.norm(d, axis=1, keepdims=True)


_CASES = {}


def case(name):
    """(scene, origins, dirs, the probe's records, the unbounded all-outputs result), computed once per scene and shared (nothing writes them)."""
    if name not in _CASES:
        sc, cam = SCENES[name]()
        o, d = fan(cam, 64, 64)
        mo, md = away_rays(256, 7)
        o, d = np.concatenate([o, mo]), np.concatenate([d, md])
        _CASES[name] = (sc, o, d, probe(sc, o, d), device_cast(sc, o, d))
    return _CASES[name]


# ---- 1: against the probe ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SCENES))
def test_equals_the_probe_bit_for_bit(gpu, name):
    sc, o, d, pr, r = case(name)
    if name in SCENE_FLAGS:
        flags = (C.c_uint32 * 2)()
        abi.check(abi.load_hip_lib().nrays_debug_scene_flags(sc.device_handle(), flags))
        assert (flags[0] & ~16, flags[1]) == SCENE_FLAGS[name], tuple(flags)
    hit = (pr["flags"] & 1) != 0
    assert hit[:4096].sum() > 100 and (~hit[:4096]).sum() > 100 and not hit[4096:].any()
    assert np.array_equal((r["flags"] & 1) != 0, hit) and np.array_equal(r["node"] >= 0, hit)
    for k in ("toi", "normal", "uv"):
        assert np.array_equal(bits(r[k][hit]), bits(pr[k][hit])), k
    assert np.array_equal(r["node"][hit], pr["node"][hit])
    assert np.array_equal(r["flags"][hit] & 3, pr["flags"][hit] & 3) and (r["flags"] & ~3 == 0).all()
    assert np.isfinite(r["toi"][hit]).all()
    assert_misses(r, ~hit)
    # out_prim: a triangle of the node's mesh where the node is a mesh, -1 on an analytic shape
    tris = [len(nd.geometry.indices) if isinstance(nd.geometry, nr.TriMesh) else 0 for nd in sc._nodes]
    ntri = np.asarray(tris)[np.maximum(r["node"], 0)]
    on_mesh = hit & (ntri > 0)
    assert (r["prim"][hit & ~on_mesh] == -1).all()
    assert (r["prim"][on_mesh] >= 0).all() and (r["prim"][on_mesh] < ntri[on_mesh]).all()
    if name == "mixed":
        assert set(r["node"][hit]) == set(range(7))  # every shape kind is hit
        assert ((r["flags"][hit] & 2) != 0).any() and ((r["flags"][hit] & 2) == 0).any()


# ---- 2: against the independent fixtures (tests/golden/kat_independent*.npz; the tolerances are those of the shared checks) -----------------------
def hits_cast(scene, o, d):
    """closest_hits in the shape the fixture checks take: (hit mask, (1, 8) record of toi, normal, has_uv, u, v, node)."""
    r = nr.closest_hits(scene, np.asarray([o], dtype=np.float64), np.asarray([d], dtype=np.float64))
    hit = (r.flags & 1) != 0
    out = np.zeros((1, 8))
    if hit[0]:
        out[0] = (r.toi[0], r.normal[0, 0], r.normal[0, 1], r.normal[0, 2], 1.0 if r.flags[0] & 2 else 0.0, r.uv[0, 0], r.uv[0, 1], r.node[0])
    return hit, out


@pytest.mark.parametrize("kind", [kat.BALL, kat.CUBOID, kat.CYLINDER, kat.CAPSULE, kat.CONE])
def test_shapes_against_independent_fixtures(gpu, kind):
    kat.check_shape_cases(kind, hits_cast, "cast_rays")


def test_triangles_planes_meshes_and_ties_against_independent_fixtures(gpu):
    from tests import test_kat_independent2 as kat2
    kat.check_triangle_cases(hits_cast, "cast_rays")
    kat2.check_planes(hits_cast, "cast_rays")
    kat2.check_meshes(hits_cast, "cast_rays")
    kat2.check_ties(hits_cast, "cast_rays")


# ---- 3: out_prim --------------------------------------------------------------------------------------------------------------------------------
def test_prim_is_the_triangle_index(gpu):
    """A 4 x 4 grid of quads (32 triangles) over a gently uneven height field, rotated and moved, as node 1 behind a ball: one ray per
    triangle from 0.3 above its centroid along the face normal.  The heights vary by 0.06 over cells of 0.5, so a normal leans by at most 7
    degrees and a ray drifts 0.04 sideways on its way down — inside its own triangle, whose centroid is 0.1 from the nearest edge."""
    g = np.arange(5, dtype=np.float64) * 0.5 - 1.0
    xx, zz = np.meshgrid(g, g, indexing="ij")
    yy = 0.03 * np.sin(3.0 * xx + 1.0) * np.cos(2.0 * zz)
    pts = su.f32_exact(np.stack([xx, yy, zz], -1).reshape(-1, 3))
    idx = []
    for i in range(4):
        for j in range(4):
            a, b, c, e = i * 5 + j, (i + 1) * 5 + j, (i + 1) * 5 + j + 1, i * 5 + j + 1
            idx += [(a, c, b), (a, e, c)]
    idx = np.asarray(idx, dtype=np.uint32)
    w, t = np.asarray([0.4, -0.3, 0.25]), np.asarray([0.5, 1.0, -0.5])
    R = kat.rotation(w)
    nodes = [nr.SceneNode(su.default_material(), 0.0, 0.0, 1.0, 1.0, nr.Isometry3((0.0, -4.0, 0.0)), nr.Ball(1.0)),
             nr.SceneNode(su.default_material(), 0.0, 0.0, 1.0, 1.0, nr.Isometry3(tuple(t), tuple(w)), nr.TriMesh(pts, idx))]
    sc = nr.Scene(nodes, [])
    p = np.asarray(pts, dtype=np.float64)[idx]  # (32, 3 corners, 3)
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    n *= np.sign(n[:, 1])[:, None]  # the side the height field faces
    cen = p.mean(axis=1)
    o, d = (cen + 0.3 * n) @ R.T + t, -n @ R.T
    for r in (device_cast(sc, o, d), nr.closest_hits(sc, o, d)._asdict()):
        assert np.array_equal(r["prim"], np.arange(32)) and (r["node"] == 1).all()
        assert np.abs(r["toi"] - 0.3).max() <= 1e-6 and (r["flags"] == 1).all()
        assert np.abs(np.abs((r["normal"] * d).sum(axis=1)) - 1.0).max() <= 1e-6


# ---- 4: optional outputs and max_toi --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("want", [(), ("normal",), ("prim", "flags"), ("uv", "flags")], ids=lambda w: "+".join(w) or "none")
def test_null_outputs_leave_the_others_alone(gpu, want):
    sc, o, d, _, full = case("mixed")
    r = device_cast(sc, o, d, want=want)
    assert [k for k in FIELDS if r[k] is not None] == ["toi", "node"] + [k for k in nr.scene.CAST_OUTPUTS if k in want]
    assert_same(r, full, "want=%s" % (want,))
    h = nr.closest_hits(sc, o[:500], d[:500], want=want)._asdict()  # the host form skips the same read-backs
    assert_same(h, {k: v[:500] for k, v in full.items()}, "host want=%s" % (want,))


@pytest.mark.parametrize("name", ["mixed", "mesh_only"])
def test_max_toi_filters_the_finished_query(gpu, name):
    sc, o, d, _, full = case(name)
    hit, toi = full["node"] >= 0, full["toi"]
    n = len(o)
    assert_same(device_cast(sc, o, d, max_toi=toi), full, "max_toi = toi")  # (a miss has toi +inf: unbounded)
    assert_same(device_cast(sc, o, d, max_toi=np.full(n, np.inf)), full, "max_toi = +inf")
    assert (toi[hit] > 0.0).all()
    assert_misses(device_cast(sc, o, d, max_toi=np.nextafter(toi, 0.0)), hit)
    assert_misses(device_cast(sc, o, d, max_toi=np.full(n, np.nan)), np.ones(n, bool))
    rng = np.random.default_rng(3)
    t = np.where(hit, toi, 10.0) * rng.uniform(0.5, 1.5, n)
    t[::7] = toi[::7]; t[3::11] = np.nan; t[5::13] = np.inf; t[6::17] = -1.0; t[8::19] = 0.0
    with np.errstate(invalid="ignore"):
        keep = hit & (toi <= t)
    assert 0.2 * hit.sum() < keep.sum() < 0.8 * hit.sum()
    assert_same(device_cast(sc, o, d, max_toi=t), filtered(full, keep), "random max_toi")
    assert_same(nr.closest_hits(sc, o[:700], d[:700], t[:700])._asdict(), {k: v[:700] for k, v in filtered(full, keep).items()}, "random max_toi, host")


# ---- 5: the unordered hint --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "mesh_only"])
def test_hinted_equals_unhinted_bit_for_bit(gpu, monkeypatch, name):
    monkeypatch.setenv("NRAYS_RAY_REORDER", "2")  # read when the handle is created: every hinted batch is reordered, whatever its size
    sc, cam = SCENES[name]()
    o, d = fan(cam, 280, 250)
    perm = np.random.default_rng(5).permutation(len(o))
    o, d = o[perm], d[perm]
    assert len(o) == 70000 and nr.ray_order(sc, o[:64], d[:64])[3][2]
    plain = device_cast(sc, o, d)
    assert 3000 < (plain["node"] >= 0).sum() < 67000
    assert_same(device_cast(sc, o, d, unordered=True), plain, "hinted")
    t = np.where(plain["node"] >= 0, plain["toi"], 1.0) * np.random.default_rng(6).uniform(0.7, 1.3, len(o))
    assert_same(device_cast(sc, o, d, max_toi=t, unordered=True, want=("prim",)), device_cast(sc, o, d, max_toi=t), "hinted, bounded")
    assert_same(nr.closest_hits(sc, o[:3000], d[:3000], unordered=True)._asdict(), {k: v[:3000] for k, v in plain.items()}, "hinted, host")


def _raw_device_call(sc, n=16, flags=0, null=()):
    """nrays_cast_rays_device called directly with n downward rays; the arguments named in `null` are NULL."""
    import torch
    o = torch.zeros((16, 3), dtype=torch.float64, device="cuda"); o[:, 1] = 5.0
    d = torch.zeros((16, 3), dtype=torch.float64, device="cuda"); d[:, 1] = -1.0
    toi, node = torch.zeros(16, dtype=torch.float64, device="cuda"), torch.zeros(16, dtype=torch.int32, device="cuda")
    a = dict(scene=sc.device_handle(), origins=o.data_ptr(), dirs=d.data_ptr(), out_toi=toi.data_ptr(), out_node=node.data_ptr())
    a.update({k: None for k in null})
    rc = abi.load_hip_lib().nrays_cast_rays_device(a["scene"], n, a["origins"], a["dirs"], None, a["out_toi"], a["out_node"], None, None, None, None, flags,
                                                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, toi.cpu().numpy(), node.cpu().numpy()


def _raw_host_call(sc, n=16, flags=0, null=()):
    o = np.zeros((16, 3)); o[:, 1] = 5.0
    d = np.zeros((16, 3)); d[:, 1] = -1.0
    toi, node = np.zeros(16), np.zeros(16, np.int32)
    dp = C.POINTER(C.c_double)
    a = dict(scene=sc.device_handle(), origins=o.ctypes.data_as(dp), dirs=d.ctypes.data_as(dp), out_toi=toi.ctypes.data_as(dp), out_node=node.ctypes.data_as(C.POINTER(C.c_int32)))
    a.update({k: None for k in null})
    rc = abi.load_hip_lib().nrays_cast_rays(a["scene"], n, a["origins"], a["dirs"], None, a["out_toi"], a["out_node"], None, None, None, None, flags)
    return rc, toi, node


@pytest.mark.parametrize("call", [_raw_device_call, _raw_host_call], ids=["device", "host"])
def test_statuses(gpu, call):
    sc = case("tiny_balls")[0]
    rc, toi, node = call(sc)
    assert rc == abi.OK and (node == 2).all() and np.abs(toi - 4.0).max() <= 1e-12  # the middle ball (node 2, radius 1) from 5 above its centre
    for flags in (2, 4, 1 << 31, 3):
        assert call(sc, flags=flags)[0] == abi.ERR_BAD_ARG, flags
    for name in ("scene", "origins", "dirs", "out_toi", "out_node"):
        assert call(sc, null=(name,))[0] == abi.ERR_BAD_ARG, name
    rc, toi, node = call(sc, n=0)
    assert rc == abi.OK and (toi == 0.0).all() and (node == 0).all()  # without work


# ---- 6: the handle's state --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "mesh_only"])
def test_a_batch_leaves_the_render_state_alone(gpu, name):
    import torch
    sc, cam = SCENES[name]()
    w, h = 128, 72
    proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], w, h)
    first = nr.render(sc, (w, h), 1, 0.0, cam["eye"], proj)
    st1 = nr.get_stats(sc)
    _, o, d, _, full = case(name)
    assert_same(device_cast(sc, o, d, stream=torch.cuda.Stream()), full, "on another stream, after a render")
    second = nr.render(sc, (w, h), 1, 0.0, cam["eye"], proj)
    st2 = nr.get_stats(sc)
    assert np.array_equal(first.view(np.uint32), second.view(np.uint32))
    for f in STAT_FIELDS:
        assert getattr(st1, f) == getattr(st2, f), f


# ---- 7: the host form -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "hair"])
def test_host_form_equals_the_device_form(gpu, name):
    sc, o, d, _, full = case(name)
    pick = np.random.default_rng(9).choice(len(o), 1000, replace=False)
    r = nr.closest_hits(sc, o[pick], d[pick])
    assert r.flags.dtype == np.uint32 and r.node.dtype == np.int32 and r.normal.shape == (1000, 3) and r.uv.shape == (1000, 2)
    assert_same(r._asdict(), {k: v[pick] for k, v in full.items()}, "host form")
    assert_same(sc.cast_rays(o[pick], d[pick])._asdict(), r._asdict(), "Scene.cast_rays")
