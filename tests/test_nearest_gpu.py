"""Nearest-surface queries on the device (k_nearest_points through nrays_nearest_points / nrays_nearest_points_device) against the numpy mirror nearest_points_ref:
every output by BIT PATTERN, winner indices equal — with one exception the definition itself names: a ball's uv goes through atan2 and asin, which are not among
+ - * / sqrt, and is compared within 2^-50 (four ulps of a value below 1).  The cases are tests/nearest_cases.py's; every reference is computed once a module."""
import functools

import numpy as np
import pytest

import nrays_amd as nr
from nrays_amd import restated
from tests import blas_cover as bc
from tests import nearest_cases as nc
from tests import stack_cases as sc_
from tests.test_blas_cover_gpu import _build

pytestmark = pytest.mark.gpu
FIELDS = nr.NearestHits._fields


def assert_same(got, want, nodes, what=""):
    """Two NearestHits agree: bit patterns, except the uv of records on a ball (module docstring)."""
    ball = np.asarray([n.geometry.kind == nr.abi.SHAPE_BALL for n in nodes] + [False])[np.asarray(want.node)]
    for name in FIELDS:
        g, w = getattr(got, name), getattr(want, name)
        if g is None:
            continue
        g = np.asarray(g.cpu()) if hasattr(g, "cpu") else np.asarray(g)
        if name == "uv":
            assert np.abs(g[ball] - w[ball]).max(initial=0.0) <= 2.0 ** -50, (what, name)
            g, w = g[~ball], w[~ball]
        if name == "flags":
            g = g.astype(np.uint32)
        bad = ~((g == w) | ((g != g) & (w != w))) if g.dtype.kind == "f" else g != w
        if g.dtype.kind == "f":
            bad |= np.signbit(g) != np.signbit(w)
        assert not bad.any(), (what, name, np.argwhere(bad)[:4].tolist(), g[bad][:4], w[bad][:4])


@functools.lru_cache(None)
def mirror(case):
    nodes, pts = CASES[case]()
    out = nr.nearest_points_ref(nodes, pts)
    return nodes, pts, out


def _ladder_case(name):
    nodes, _ = sc_.scene_nodes(name)
    rng = np.random.default_rng(3)
    far = rng.uniform(-1.0, 1.0, (768, 3)) * 2.0 ** rng.uniform(-8, 62, (768, 1))  # far points: the walk defers and comes back
    near = np.stack([-2.0 ** rng.uniform(-60, 60, 256), rng.uniform(-2, 4, 256), rng.uniform(-2, 4, 256)], axis=1)
    return nodes, np.concatenate([far, near])


CASES = {
    "voronoi": lambda: (nc.one_triangle_nodes(), nc.voronoi_points()[0]),
    "voronoi_below": lambda: (nc.one_triangle_nodes(), nc.voronoi_points()[0] * [1, 1, -1]),
    "tie_triangles": lambda: (nc.two_triangle_nodes(), nc.tie_points()),
    "tie_nodes": lambda: (nc.two_triangle_nodes(split=True), nc.tie_points()),
    "analytic": lambda: (nc.analytic_nodes(), nc.analytic_points()),
    "grid": lambda: (nc.grid_nodes(), nc.grid_points()),
    "grid_turned": lambda: (nc.grid_nodes(nc.ISO), nc.grid_points()),
    "cross": lambda: (nc.cross_nodes(), nc.cross_points()),
    "deep_mesh": lambda: _ladder_case("a_rotated"),
    "deep_planes": lambda: _ladder_case("d_planes"),
}


@pytest.mark.parametrize("case", ["voronoi", "voronoi_below", "tie_triangles", "tie_nodes", "analytic", "grid_turned", "cross"])
def test_the_device_equals_the_mirror_bit_for_bit(gpu, case):
    nodes, pts, want = mirror(case)
    got = nr.nearest_points(nc.scene(nodes), np.array(pts))
    assert_same(got, want, nodes, case)
    if case == "analytic":
        assert len(pts) == nc.N_POINTS and set(np.unique(want.node)) == set(range(6))  # every shape and the plane win somewhere
    if case.startswith("tie"):
        assert (want.node[:64] == 0).all() and (want.prim[:64] == 0).all()


@pytest.mark.parametrize("builder", ["device", "host"])
def test_the_grid_mesh_at_the_device_builders_threshold_under_both_builders(gpu, monkeypatch, capfd, builder):
    nodes, pts, want = mirror("grid")
    assert len(nodes[0].geometry.indices) == 2048 and len(pts) == nc.N_POINTS
    monkeypatch.setenv("NRAYS_BUILD_TIMES", "1")
    if builder == "host":
        monkeypatch.setenv("NRAYS_GPU_BUILD", "0")
    got = nr.nearest_points(nc.scene(nodes), np.array(pts))
    assert ("device BLAS build" in capfd.readouterr().err) == (builder == "device")
    assert_same(got, want, nodes, builder)
    k = nc.N_POINTS // 3
    assert want.dist[:k].max() < 2.0 ** -40 and want.dist[-k:].min() > 1.0  # on the surface (up to the rounding of the samples) ... and far


@pytest.mark.parametrize("builder", ["device", "host"])
def test_a_pre_split_mesh_either_side_of_every_seam(gpu, monkeypatch, builder):
    """hair800 of tests/blas_cover.py, which the pre-split splits: points of a triangle one f64 step behind a face of one of its regions (the dump's seam samples), the
    same one more f64 step to either side in every coordinate, and off the surface by 2^-7 along +-normal."""
    pts, idx = bc.case_meshes()["hair800"]
    d = _build(pts, idx, True)
    rep = bc.validate(d, pts, idx, True, keep_samples=True)
    assert bc.clean(rep) and len(d["tri"]) > 4 * len(idx)
    p, tri = rep["interior"]
    pick = np.linspace(0, len(p) - 1, 768).astype(np.int64)
    p, tri = p[pick], tri[pick]
    V = np.asarray(pts, np.float32)[idx.astype(np.int64)].astype(np.float64)[tri]
    n = np.cross(V[:, 1] - V[:, 0], V[:, 2] - V[:, 0]); n /= np.linalg.norm(n, axis=1, keepdims=True)
    q = np.concatenate([p, np.nextafter(p, np.inf), np.nextafter(p, -np.inf), p + n * 2.0 ** -7, p - n * 2.0 ** -7])
    if builder == "device":
        monkeypatch.setenv("NRAYS_GPU_BUILD_MIN", "1")
    else:
        monkeypatch.setenv("NRAYS_GPU_BUILD", "0")
    for iso in (None, nc.ISO):
        nodes = [nc.node(nr.TriMesh(np.asarray(pts, np.float32).astype(np.float64), idx), iso)]
        w = q if iso is None else q @ nc.frame(iso)[0].T + nc.frame(iso)[1]
        want = nr.nearest_points_ref(nodes, w)
        assert_same(nr.nearest_points(nc.scene(nodes), np.array(w)), want, nodes, builder)
        assert want.dist[:3 * 768].max() < 2.0 ** -40 and (want.node == 0).all()


@pytest.mark.parametrize("case", ["deep_mesh", "deep_planes"])
def test_a_ladder_deeper_than_the_lds_slots(gpu, case):
    nodes, pts, want = mirror(case)
    depth = max(len(n.geometry.indices) for n in nodes if n.geometry.kind == nr.abi.SHAPE_TRIMESH)
    assert depth == 121 and sc_.lds_stack() == 24
    assert_same(nr.nearest_points(nc.scene(nodes), np.array(pts)), want, nodes, case)
    assert len(np.unique(want.prim)) > 30  # rungs all along the ladder win


def test_max_dist_edges(gpu):
    nodes, pts, full = mirror("analytic")
    k = len(pts)
    md = full.dist.copy()
    md[1::5] = np.nextafter(md[1::5], 0.0); md[2::5] = np.nan; md[3::5] = -1.0; md[4::5] = np.inf
    sc = nc.scene(nodes)
    got, want = nr.nearest_points(sc, np.array(pts), md), nr.nearest_points_ref(nodes, pts, md)
    assert_same(got, want, nodes)
    pos = full.dist > 0
    assert (got.node[0::5] >= 0).all() and (got.node[4::5] >= 0).all()         # equal to the distance keeps the hit; +inf too
    assert (got.node[1::5][pos[1::5]] == -1).all() and (got.node[2::5] == -1).all() and (got.node[3::5] == -1).all()  # nextafter below loses it; NaN, negative: misses
    on = full.point.copy()  # the nearest points themselves, with max_dist 0: on the surface up to the rounding of the record, so found exactly where the mirror finds them
    zero = nr.nearest_points(sc, on, np.zeros(k))
    assert_same(zero, nr.nearest_points_ref(nodes, on, np.zeros(k)), nodes)
    tri = nr.nearest_points(nc.scene(nc.one_triangle_nodes()), nc.voronoi_points()[0][7:], np.zeros(7))
    assert (tri.node == 0).all() and not tri.dist.any()  # 0 on a surface point is found


def test_skipped_points_hold_garbage_and_every_optional_output_may_be_absent(gpu):
    import torch
    nodes, pts, full = mirror("cross")
    n = len(pts)
    hf = np.where(np.arange(n) % 3 == 0, 2, 1).astype(np.uint32)
    garbage = np.where((hf & 1)[:, None] != 0, pts, np.nan)
    garbage[::6] = 1e308
    want = nr.nearest_points_ref(nodes, pts, None, hf)
    sc = nc.scene(nodes)
    assert_same(nr.nearest_points(sc, garbage, None, hf), want, nodes)
    assert (want.node[::3] == -1).all() and not want.point[::3].any() and np.isinf(want.dist[::3]).all()
    tp, thf = torch.from_numpy(garbage).cuda(), torch.from_numpy(hf.view(np.int32)).cuda()
    for drop in nr.marshal.NEAREST_OUTPUTS + ((),):
        keep = tuple(f for f in nr.marshal.NEAREST_OUTPUTS if f != drop)
        for got in (nr.nearest_points(sc, garbage, None, hf, want=keep), nr.nearest_points(sc, tp, None, thf, want=keep)):
            assert all((getattr(got, f) is None) == (f == drop) for f in nr.marshal.NEAREST_OUTPUTS)
            assert_same(got, want, nodes, "without %s" % (drop,))
    torch.cuda.synchronize()


def test_the_chunk_boundary_in_the_device_form(gpu):
    import torch
    n = (1 << 22) + 65
    nodes = nc.two_triangle_nodes()
    rng = np.random.default_rng(11)
    base = np.concatenate([nc.tie_points(), rng.uniform(-3.0, 3.0, (1024 - 192, 3))])
    pts = np.tile(base, (n // 1024 + 1, 1))[:n]
    pts[(1 << 22) - 3:(1 << 22) + 3] = rng.uniform(-3.0, 3.0, (6, 3))  # either side of the seam: points of their own
    want = nr.nearest_points_ref(nodes, np.concatenate([base, pts[(1 << 22) - 3:(1 << 22) + 3]]))
    got = nr.nearest_points(nc.scene(nodes), torch.from_numpy(pts).cuda())
    torch.cuda.synchronize()
    rows = np.concatenate([np.arange(1024), np.arange((1 << 22) - 3, (1 << 22) + 3)])
    tail = np.arange((1 << 22) + 3, n)
    for name in FIELDS:
        g = getattr(got, name).cpu().numpy()
        w = getattr(want, name)
        assert nc.same(g[rows].astype(w.dtype), w), name
        assert nc.same(g[tail].astype(w.dtype), w[tail % 1024]), name  # the second chunk's 65 points
        assert nc.same(g[1024:2048].astype(w.dtype), w[:1024]), name


def test_an_empty_scene_misses_every_point(gpu):
    pts = nc.voronoi_points()[0]
    got = nr.nearest_points(nc.scene([]), pts)
    assert_same(got, nr.nearest_points_ref([], pts), [])
    assert (got.node == -1).all() and np.isinf(got.dist).all() and (got.prim == -1).all() and not got.flags.any() and not got.point.any()


def test_the_bound_probe_equals_its_mirror_bit_for_bit(gpu):
    pts, boxes = nc.bound_cases()
    assert nc.same(nr.nearest_bound_probe(pts, boxes), nr.nearest_box_bound_ref(pts, boxes))
    for _, _, box, p, _ in nc.margin_cases():
        assert nc.same(nr.nearest_bound_probe(p, [box]), nr.nearest_box_bound_ref(p, [box]))


def test_no_ray_finds_anything_nearer_and_the_ray_towards_the_point_finds_it(gpu):
    """Independent of the mirror.  tau = 2^-40 (|p| + the scene's bounding radius): f64's 2^-53 with 2^13 for the few dozen operations either side; derived, not measured."""
    nodes, p = nc.cross_nodes(), np.array(nc.cross_points())
    sc = nc.scene(nodes)
    got = nr.nearest_points(sc, p)
    tau = nc.cross_tau(p)
    assert (got.flags & 1).all()
    dirs = nr.sphere_dirs(32)
    dirs = dirs / np.linalg.norm(dirs, axis=1, keepdims=True)
    o, d = np.repeat(p, 32, axis=0), np.tile(dirs, (len(p), 1))
    hits = nr.closest_hits(sc, o, d, want=())
    assert (hits.toi.reshape(len(p), 32) >= (got.dist - tau)[:, None]).all()
    # left out: near ties, and rays that only TOUCH their target — an acute convex feature (the cone's rim and apex, the mesh's boundary) is nearest to points from which the ray
    # towards it grazes the node there instead of entering it, and a grazing contact is a tie between a hit and a miss (nearest_cases.ray_only_touches, independent of the device)
    left_out = nc.near_ties(nodes, p, tau) | nc.ray_only_touches(nodes, p, got.node, got.point)
    use = ~left_out & (got.flags & 4 == 0) & (got.dist > 2.0 ** -20)
    assert left_out.mean() <= 0.02 and use.sum() > 512
    to = (got.point[use] - p[use]) / got.dist[use, None]
    back = nr.closest_hits(sc, np.ascontiguousarray(p[use]), np.ascontiguousarray(to), want=())
    assert np.array_equal(back.node, got.node[use])
    assert (np.abs(back.toi - got.dist[use]) <= tau[use]).all(), float(np.abs(back.toi - got.dist[use]).max())


def test_the_records_pass_unfiltered_into_shade_points(gpu):
    nodes, p, want = mirror("cross")
    mat = nr.PhongMaterial((0.25, 0.5, 0.25), (0.5, 0.5, 0.5), (0.25, 0.25, 0.25), None, None, 20.0)
    lit = [nr.SceneNode(mat if k % 2 else n.material, 0.0, 0.0, 1.0, 1.0, n.transform, n.geometry) for k, n in enumerate(nodes)]
    sc = nc.scene(lit)
    md = np.where(np.arange(len(p)) % 4 == 0, 0.25, np.inf)  # some misses among them
    got, ref = nr.nearest_points(sc, np.array(p), md), nr.nearest_points_ref(lit, p, md)
    view = lambda r: -np.asarray(r.normal)  # noqa: E731  (looking at the surface from the query point's side)
    a = nr.shade_points(sc, got.point, got.normal, view(got), got.node, uvs=got.uv, hit_flags=got.flags)
    balls = np.asarray([n.geometry.kind == nr.abi.SHAPE_BALL for n in lit] + [False])[ref.node]
    b = nr.shade_points(sc, ref.point, ref.normal, view(ref), ref.node, uvs=np.where(balls[:, None], got.uv, ref.uv), hit_flags=ref.flags)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and (ref.node == -1).any() and a[ref.node >= 0].any()
    assert not a[ref.node == -1].any()


def test_probe_clearance_is_the_distance_and_the_behind_bit(gpu):
    nodes, p, want = mirror("cross")
    sc = nc.scene(nodes)
    c = nr.probe_clearance(sc, np.array(p), max_dist=0.5)
    assert nc.same(c.dist, np.where(want.dist <= 0.5, want.dist, np.inf)) and np.array_equal(c.behind, (want.flags & 4 != 0) & (want.dist <= 0.5))
    assert c.behind.any() and np.isinf(c.dist).any()
