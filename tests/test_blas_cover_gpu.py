"""Every BLAS of the DEVICE builder (nrays_amd/csrc/bvh_device.hip) covers its triangles — tests/blas_cover.py's property (shape, nesting, cover within e(T)),
which needs no second builder — on the dumps of nrays_debug_blas_build with the device flag: the case meshes of tests/test_blas_cover.py with and without
pre-splitting, and the 10 000-triangle hair mesh on every path of the pre-splitting (one walk + k_place_extra, two walks, the piece list's overflow into
the second walk, one workgroup striding over all triangles; the sliver mesh among the cases makes the threshold iterate onto the budget).

Then rays through the seams: one device-built, pre-split hair mesh as a one-node scene (NRAYS_GPU_BUILD_MIN=1), and for up to 4 096 seam interior samples p
of its dump (points of a triangle T one f64 step behind a face of one of T's regions) a ray from p + 0.25 n towards p and one from p - 0.25 n, n = T's unit
normal.  closest_hits, ordered and unordered, must name the brute force's hit (oracle.cast(bruteforce=True): flag, node, toi bit for bit, and the triangle
where the one-triangle-per-node twin of the scene gives the same distance), intersects_rays with max_toi just past p must be blocked where the brute force
hits within max_toi, and every ray must hit at or before p: a sliver that no leaf covers would let exactly these rays through.  Again under a rotated
isometry (the transformed BLAS path).  "Just past p" is 0.25 + 1e-9: p lies within e(T) ~ 1e-16 of T and the origin and the normal are rounded once each,
so T is met at 0.25 +- 1e-15; 1e-9 is far above that and far below the strands' spacing."""
import ctypes as C
import time

import numpy as np
import pytest

import nrays_amd as nr
import oracle
from nrays_amd import abi, math3d
from tests import blas_cover as bc

pytestmark = pytest.mark.gpu


def _build(pts, idx, presplit):
    p64 = np.ascontiguousarray(np.asarray(pts, np.float32).astype(np.float64)); idx = np.ascontiguousarray(idx, np.uint32)
    m = abi.NraysMesh(len(p64), len(idx), p64.ctypes.data_as(C.POINTER(C.c_double)), None, idx.ctypes.data_as(C.POINTER(C.c_uint32)))
    cap = 12 * len(idx) + 64
    nodes = np.zeros((cap, 32), np.float32); tri = np.zeros(cap, np.uint32)
    d = abi.NraysBlasDump()
    d.node_capacity = cap; d.ref_capacity = cap
    d.nodes = nodes.ctypes.data_as(C.POINTER(C.c_float)); d.tri_ids = tri.ctypes.data_as(C.POINTER(C.c_uint32))
    abi.check(abi.load_hip_lib().nrays_debug_blas_build(C.byref(m), 1 | (0 if presplit else 2), C.byref(d)))
    assert d.num_nodes <= cap and d.num_refs <= cap
    return dict(nodes=nodes[:d.num_nodes].copy(), tri=tri[:d.num_refs].copy(), root=d.root, depth=d.max_depth, hairy=d.hairy)


@pytest.fixture(scope="module")
def meshes():
    m = bc.case_meshes()
    m["hair10k"] = bc.hair10k()
    return m


def _check(name, pts, idx, presplit, **kw):
    t0 = time.time()
    d = _build(pts, idx, presplit)
    rep = bc.validate(d, pts, idx, presplit, seam_every=max(1, len(idx) // 1200), **kw)
    print(bc.line(name, rep, time.time() - t0))
    assert bc.clean(rep), bc.line(name, rep)
    return d, rep


CASES = ("hair800", "hairball", "slivers", "sheet", "copies", "hair64", "hair255", "hair256", "hair257", "fat_soup")


@pytest.mark.parametrize("presplit", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_device_blas_covers_its_triangles(gpu, meshes, case, presplit):
    pts, idx = meshes[case]
    d, rep = _check("device %s%s" % (case, " pre-split" if presplit else ""), pts, idx, presplit)
    if not presplit:
        assert len(d["tri"]) == len(idx)
    elif case.startswith("hair"):
        assert d["hairy"] == 1 and len(d["tri"]) > 4 * len(idx) and rep["seam"] > 0
    elif case == "slivers":
        assert len(idx) < len(d["tri"]) <= 3 * len(idx) + 1024  # split, and the threshold settled on the budget


@pytest.mark.parametrize("path", ["one_walk", "two_walks", "piece_overflow", "one_workgroup"])
def test_every_presplit_path_covers_its_triangles(gpu, meshes, monkeypatch, capfd, path):
    pts, idx = meshes["hair10k"]
    if path == "two_walks":
        monkeypatch.setenv("NRAYS_PRESPLIT_ONE_WALK", "0")
    elif path == "piece_overflow":
        monkeypatch.setenv("NRAYS_DEBUG_PIECE_CAP", "3")
        monkeypatch.setenv("NRAYS_BUILD_TIMES", "1")
    elif path == "one_workgroup":
        monkeypatch.setenv("NRAYS_SPLIT_GRID", "1")
    d, rep = _check("device hair10k %s" % path, pts, idx, True)
    assert d["hairy"] == 1 and len(d["tri"]) > 4 * len(idx) and rep["seam"] > 0
    if path == "piece_overflow":
        assert "piece list overflow" in capfd.readouterr().err


# ---- rays through the seams --------------------------------------------------------------------------------------------------------

PLACEMENTS = {"identity": nr.Isometry3.identity, "rotated": lambda: nr.Isometry3((0.37, -1.21, 2.05), (0.3, -0.5, 0.8))}
LIMIT = 0.25 + 1e-9
_rays = {}


def _scene(pts, idx, iso):
    node = lambda p, i: nr.SceneNode(nr.NormalMaterial(), 0.0, 0.0, 1.0, 1.0, iso(), nr.TriMesh(p, i))  # noqa: E731
    return node, [nr.Light((0.0, 10.0, 0.0), 0.0, 1, (1, 1, 1))]


def _seam_rays(meshes, place):
    """Once per placement, then read-only: (origins, directions, brute-force hit, brute-force record, triangle or -1)."""
    if place not in _rays:
        pts, idx = meshes["hair800"]
        d = _build(pts, idx, True)
        rep = bc.validate(d, pts, idx, True, keep_samples=True)
        assert bc.clean(rep) and d["hairy"] == 1
        p, tri = rep["interior"]
        assert len(p) > 4096
        pick = np.linspace(0, len(p) - 1, 4096).astype(np.int64)
        p, tri = p[pick], tri[pick]
        V = np.asarray(pts, np.float32)[idx.astype(np.int64)].astype(np.float64)[tri]
        n = np.cross(V[:, 1] - V[:, 0], V[:, 2] - V[:, 0]); n /= np.linalg.norm(n, axis=1, keepdims=True)
        o = np.concatenate([p + 0.25 * n, p - 0.25 * n]); dirs = np.concatenate([-n, n])
        iso = PLACEMENTS[place]
        R = np.array(math3d.rotation_from_axis_angle(iso().axis_angle), np.float64).reshape(3, 3); T = np.array(iso().translation, np.float64)
        o = np.ascontiguousarray(o @ R.T + T); dirs = np.ascontiguousarray(dirs @ R.T)
        node, lights = _scene(pts, idx, iso)
        p64 = np.asarray(pts, np.float32).astype(np.float64)
        one = nr.Scene([node(p64, idx)], lights, (0.0, 0.0, 0.0))
        per_tri = nr.Scene([node(p64[idx[t].astype(np.int64)], np.asarray([[0, 1, 2]], np.uint32)) for t in range(len(idx))], lights, (0.0, 0.0, 0.0))
        hit, out = oracle.cast(one.descriptor, o, dirs, bruteforce=True)
        thit, tout = oracle.cast(per_tri.descriptor, o, dirs, bruteforce=True)
        agree = (thit == hit) & (~hit | (tout[:, 0] == out[:, 0]))
        prim = np.where(hit & agree, tout[:, 7].astype(np.int64), -1)
        assert hit.all() and (out[:, 0] <= LIMIT).all(), ("the brute force itself misses a sample", int((~hit).sum()), float(out[:, 0].max()))
        assert (prim >= 0).mean() > 0.99
        for a in (o, dirs, hit, out, prim):
            a.setflags(write=False)
        _rays[place] = (o, dirs, hit, out, prim)
    return _rays[place]


@pytest.mark.parametrize("unordered", [False, True], ids=["ordered", "unordered"])
@pytest.mark.parametrize("place", sorted(PLACEMENTS))
def test_rays_through_the_seams_hit_what_the_brute_force_hits(gpu, meshes, monkeypatch, capfd, place, unordered):
    o, dirs, hit, out, prim = _seam_rays(meshes, place)
    monkeypatch.setenv("NRAYS_GPU_BUILD_MIN", "1")
    monkeypatch.setenv("NRAYS_BUILD_TIMES", "1")
    if unordered:
        monkeypatch.setenv("NRAYS_RAY_REORDER", "2")  # read when a scene is created: the reorder then runs at any batch size
    pts, idx = meshes["hair800"]
    node, lights = _scene(pts, idx, PLACEMENTS[place])
    sc = nr.Scene([node(np.asarray(pts, np.float32).astype(np.float64), idx)], lights, (0.0, 0.0, 0.0))
    got = nr.closest_hits(sc, np.array(o), np.array(dirs), unordered=unordered)
    assert "device BLAS build" in capfd.readouterr().err
    assert np.array_equal(got.node >= 0, hit), np.flatnonzero((got.node >= 0) != hit)[:5]
    assert (got.node[hit] == 0).all()
    assert np.array_equal(got.toi[hit], out[hit, 0])
    assert (got.toi <= LIMIT).all(), float(got.toi.max())  # every ray meets something at or before p
    known = hit & (prim >= 0)
    assert np.array_equal(got.prim[known], prim[known])
    lit, _ = nr.intersects_rays(sc, np.array(o), np.array(dirs), np.full(len(o), LIMIT), unordered=unordered)
    assert np.array_equal(~lit, hit & (out[:, 0] <= LIMIT)) and not lit.any()
    print("%s %s: %d rays, %d triangles named, farthest hit %.17g" % (place, "unordered" if unordered else "ordered", len(o), known.sum(), got.toi.max()))
