"""Nearest-surface queries at caller-supplied points (nrays_nearest_points_device / nrays_nearest_points; nrays_amd.nearest_points, probe_clearance,
nearest_points_ref, nearest_box_bound_ref), the parts that need no GPU: the header, the ctypes table and the Rust declarations, the argument checks of the Python
wrapper, and the definition on its numpy mirror — the triangle routine against exact rationals, one case per Voronoi region and the tie-breaks, every analytic
shape against an independent closed form, the walk's box bound against exact rationals, and the cull's margin on an adversarial set with three mutants.
tests/test_nearest_gpu.py compares the device with the mirror by bit pattern on the cases of tests/nearest_cases.py.

Measured here (float64, 3 000 cases a family; the cap is 2^-44 s^2): worst |d2 - exact| / s^2 = 2^-51.5 random, 2^-51.1 far, 2^-83 near the surface, 2^-51.3 slivers,
2^-51.4 slivers collinear in f32, 2^-51.7 collinear, 2^-51.0 collapsed to a point, 2^-52.5 offset by 1000.  Ericson's routine exactly as printed reaches 2^-9.5 on the
collinear family (its interior branch divides rounding noise by rounding noise); the definition's last branch therefore lets the three edge projections compete."""
import ctypes as C
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import nrays_amd as nr
from nrays_amd import abi, restated
from tests import nearest_cases as nc
from tests.test_gather import FFI, GPU_RS, HEADER, HEADER_TEXT, _NoDevice, _c_params, no_library  # noqa: F401  (no_library is a fixture)

_IN = ["NraysScene*", "uint32_t", "const double*", "const double*", "const uint32_t*", "double*", "int32_t*", "double*", "double*", "double*", "int32_t*", "uint32_t*", "uint32_t"]
EXPECTED = {"nrays_nearest_points_device": _IN + ["void*"], "nrays_nearest_points": _IN}
RUST_TYPES = {"NraysScene*": "*mut NraysScene", "uint32_t": "u32", "const double*": "*const f64", "const uint32_t*": "*const u32", "double*": "*mut f64", "int32_t*": "*mut i32",
              "uint32_t*": "*mut u32", "void*": "*mut c_void"}
CAP = Fraction(1, 2 ** 44)


# ---- declarations ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_header_ctypes_and_rust_declare_the_same_function(name):
    assert _c_params(name) == EXPECTED[name]
    assert name in abi.HIP_SYMBOLS and name in abi.POST_V7_SYMBOLS
    res, args = abi.HIP_SYMBOLS[name]
    assert res is C.c_int and len(args) == len(EXPECTED[name]) and args[1] is C.c_uint32 and args[12] is C.c_uint32
    m = re.search(r"pub fn %s\((.*?)\) -> c_int;" % name, FFI)
    assert m, "%s is not declared in gpu_ffi.rs" % name
    assert [p.split(": ", 1)[1] for p in m.group(1).split(", ")] == [RUST_TYPES[t] for t in EXPECTED[name]]
    assert "pub fn nearest_points(" in GPU_RS and "pub unsafe fn nearest_points_device(" in GPU_RS
    assert "nrays_nearest_points(" in GPU_RS and "nrays_nearest_points_device(" in GPU_RS


def test_the_bound_probe_is_declared_everywhere():
    assert _c_params("nrays_debug_nearest_bound") == ["uint32_t", "uint32_t", "const double*", "const double*", "double*"]
    assert abi.HIP_SYMBOLS["nrays_debug_nearest_bound"][1] == [C.c_uint32, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
    assert re.search(r"pub fn nrays_debug_nearest_bound\(n: u32, boxes: u32, points: \*const f64, box_bounds: \*const f64, out: \*mut f64\) -> c_int;", FFI)


def test_the_symbols_are_exported_and_the_abi_version_is_still_7(built):
    assert re.search(r"#define NRAYS_ABI_VERSION 7\b", HEADER) and abi.ABI_VERSION == 7 and abi.load_hip_lib().nrays_abi_version() == 7
    note = re.search(r"Added after 7 WITHOUT a bump.*?\*/", HEADER_TEXT, re.S).group(0)
    exported = subprocess.check_output(["nm", "-D", "--defined-only", abi.HIP_LIB_PATH]).decode()
    for name in list(EXPECTED) + ["nrays_debug_nearest_bound"]:
        assert re.search(r"%s\b" % name, note), name
        assert (" T " + name + "\n") in exported, name
        assert getattr(abi.load_hip_lib(), name).argtypes == abi.HIP_SYMBOLS[name][1]


def test_the_python_names_exist():
    for name in ("nearest_points", "probe_clearance", "nearest_points_ref", "nearest_box_bound_ref", "nearest_bound_probe"):
        assert callable(getattr(nr, name)), name
    assert nr.NearestHits._fields == ("dist", "node", "point", "normal", "uv", "prim", "flags") and nr.NEAREST_BEHIND == 4
    assert nr.NearestHits._fields[1:] == tuple(f for f in ("node", "point") + nr.CastHits._fields[2:])  # closest_hits' record, plus point and dist
    from nrays_amd import scenefile
    for cls in (nr.Scene, scenefile.FileScene):
        for name in ("nearest_points", "probe_clearance"):
            assert callable(getattr(cls, name)), name


def test_without_a_scene_or_with_a_flag_every_call_is_a_bad_arg(built):
    """NULL scene / points / out_dist / out_node and any flag bit return before any HIP call: this test runs without a device.  The outputs stay untouched."""
    lib = abi.load_hip_lib()
    p, dist, node = (C.c_double * 3)(0.0, 0.0, 1.0), (C.c_double * 1)(7.0), (C.c_int32 * 1)(7)
    fake = C.c_void_p(8)  # a non-null handle that must never be dereferenced: the other checks come first only for NULL pointers and flags
    assert lib.nrays_nearest_points(None, 1, p, None, None, dist, node, None, None, None, None, None, 0) == abi.ERR_BAD_ARG
    assert lib.nrays_nearest_points_device(None, 1, C.addressof(p), None, None, C.addressof(dist), C.addressof(node), None, None, None, None, None, 0, None) == abi.ERR_BAD_ARG
    for args in ((None, None, None, dist, node), (p, None, None, None, node), (p, None, None, dist, None)):
        assert lib.nrays_nearest_points(fake, 1, *args, None, None, None, None, None, 0) == abi.ERR_BAD_ARG
    for flags in (1, 2, 1 << 31):
        assert lib.nrays_nearest_points(fake, 1, p, None, None, dist, node, None, None, None, None, None, flags) == abi.ERR_BAD_ARG
    assert lib.nrays_nearest_points(fake, 0, p, None, None, dist, node, None, None, None, None, None, 0) == abi.OK  # n == 0: no work
    assert lib.nrays_debug_nearest_bound(1, 1, None, None, None) == abi.ERR_BAD_ARG
    assert dist[0] == 7.0 and node[0] == 7


def test_nearest_points_rejects_bad_arguments_before_any_library_call(no_library):
    import torch
    sc = _NoDevice()
    good = dict(points=np.zeros((4, 3)))
    bad = [dict(points=None), dict(points=np.zeros((4, 2))), dict(points=np.zeros(12)), dict(points=np.zeros((4, 3), np.int64)), dict(max_dist=np.zeros(3)), dict(max_dist=np.zeros((4, 1))),
           dict(max_dist=np.zeros(4, np.int32)), dict(hit_flags=np.ones(5, np.uint32)), dict(hit_flags=np.ones(4, np.float32)), dict(want=("toi",)), dict(want=("point", "dist")),
           dict(max_dist=torch.zeros(4, dtype=torch.float64)), dict(points=torch.zeros((4, 3), dtype=torch.float64))]  # numpy and torch mixed; a host tensor
    for kw in bad:
        with pytest.raises(ValueError):
            nr.nearest_points(sc, **dict(good, **kw))
    with pytest.raises(ValueError):
        nr.probe_clearance(sc, np.zeros((4, 2)))


# ---- the triangle routine against exact rationals ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", nc.FAMILIES)
def test_the_triangle_routine_stays_within_the_cap_of_the_exact_squared_distance(family):
    worst = Fraction(0)
    for a, b, c, p in nc.family_cases(family, 3000):
        _, _, q, _ = restated.tri_closest_ref(a, b, c, p)
        d2 = float(restated._d2_of(p, q))
        s = Fraction(float(np.abs(p).max())) + Fraction(float(max(np.abs(a).max(), np.abs(b).max(), np.abs(c).max())))
        err = abs(Fraction(d2) - nc.exact_tri_d2(a, b, c, p))
        worst = max(worst, err / (s * s) if s else err)
        assert err <= CAP * s * s, (family, a, b, c, p, d2)
    print("%s: worst |d2 - exact| / s^2 = 2^%.1f" % (family, np.log2(float(worst)) if worst else -np.inf))


# ---- Voronoi regions and ties --------------------------------------------------------------------------------------------------------------------------------------
def test_one_case_per_voronoi_region_on_and_off_the_triangle():
    pts, region = nc.voronoi_points()
    a, b, c = nc.TRI
    v, w, q, got = restated.tri_closest_ref(a, b, c, pts)
    assert got.tolist() == region.tolist()
    out = nr.nearest_points_ref(nc.one_triangle_nodes(), pts)
    assert (out.node == 0).all() and (out.prim == 0).all() and (out.flags & 3 == 3).all()
    for i, p in enumerate(pts):
        assert Fraction(float(out.dist[i])) ** 2 == nc.exact_tri_d2(a, b, c, p) or abs(out.dist[i] ** 2 - float(nc.exact_tri_d2(a, b, c, p))) <= 2.0 ** -50
    assert np.array_equal(out.dist[7:], np.zeros(7)) and np.array_equal(out.point[7:], pts[7:])  # exactly on a vertex, an edge, the face: distance 0 at the point itself
    assert np.array_equal(out.uv, np.stack([v, w], axis=1))  # TRI_UV maps the corners to (0, 0), (1, 0), (0, 1): the uv IS (v, w)
    assert np.array_equal(out.normal[:7], np.tile([0.0, 0.0, 1.0], (7, 1))) and not (out.flags[:7] & 4).any()  # z = +0.5: the front of the winding
    below = nr.nearest_points_ref(nc.one_triangle_nodes(), pts[:7] * [1, 1, -1])
    assert np.array_equal(below.normal, np.tile([0.0, 0.0, -1.0], (7, 1))) and (below.flags & 4 == 4).all() and np.array_equal(below.dist, out.dist[:7])


def test_among_equal_keys_the_smaller_triangle_and_the_smaller_node_win():
    pts = nc.tie_points()
    n = len(pts) // 3
    one, two = nr.nearest_points_ref(nc.two_triangle_nodes(), pts), nr.nearest_points_ref(nc.two_triangle_nodes(split=True), pts)
    assert (one.prim[:n] == 0).all() and (two.node[:n] == 0).all() and (one.node == 0).all() and (two.prim == 0).all()  # on the mirror plane: the smaller index
    assert (one.prim[n:2 * n] == 0).all() and (one.prim[2 * n:] == 1).all() and (two.node[n:2 * n] == 0).all() and (two.node[2 * n:] == 1).all()  # a step either side
    assert nc.same(one.dist, two.dist) and nc.same(one.point, two.point)
    swapped = nr.nearest_points_ref(nc.two_triangle_nodes(split=True)[::-1], pts[:n])
    assert (swapped.node == 0).all() and np.array_equal(swapped.point[:, 0], -two.point[:n, 0])  # the winner follows the INDEX, not the side


def test_max_dist_hit_flags_and_the_empty_scene():
    pts, _ = nc.voronoi_points()
    nodes = nc.one_triangle_nodes()
    full = nr.nearest_points_ref(nodes, pts)
    md = full.dist.copy(); md[1] = np.nextafter(md[1], 0.0); md[2] = np.nan; md[3] = -1.0; md[4] = np.inf
    out = nr.nearest_points_ref(nodes, pts, md)
    lost = np.zeros(len(pts), bool); lost[[1, 2, 3]] = True
    assert np.array_equal(out.node, np.where(lost, -1, 0)) and np.isinf(out.dist[lost]).all() and nc.same(out.dist[~lost], full.dist[~lost])
    assert (out.flags[lost] == 0).all() and (out.prim[lost] == -1).all() and not out.point[lost].any() and (out.node[7:] == 0).all()  # max_dist 0 on the surface: found
    hf = np.ones(len(pts), np.uint32); hf[::2] = 2
    skipped = nr.nearest_points_ref(nodes, np.where((hf & 1)[:, None] != 0, pts, np.nan), None, hf)
    assert (skipped.node[::2] == -1).all() and nc.same(skipped.dist[1::2], full.dist[1::2])
    empty = nr.nearest_points_ref([], pts)
    assert (empty.node == -1).all() and np.isinf(empty.dist).all() and (empty.flags == 0).all()


# ---- analytic shapes against independent closed forms ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(nc.SHAPES) + ["plane"])
def test_each_analytic_shape_agrees_with_an_independent_closed_form(kind):
    geo, iso = (nr.Plane((0.0, 1.0, 0.0)), nc.PLANE_ISO) if kind == "plane" else (nc.SHAPES[kind](), nc.PLACES[kind])
    R, T = nc.frame(iso)
    rng = np.random.default_rng(13)
    local = np.concatenate([nc.special_local_points(kind if kind != "plane" else "ball"), rng.uniform(-2.0, 2.0, (600, 3))])
    p = local @ R.T + T
    out = nr.nearest_points_ref([nc.node(geo, iso)], p)
    dist, inside = nc.independent_distance(geo.kind, geo.params, iso, p)
    tol = 2.0 ** -44 * (np.abs(p).max() + np.abs(T).max() + 2.0)
    assert (out.node == 0).all() and (out.prim == -1).all()
    assert np.abs(out.dist - dist).max() <= tol, (kind, np.abs(out.dist - dist).argmax())
    edge = dist <= tol  # (on the surface itself "inside" is a matter of rounding)
    assert np.array_equal((out.flags & 4 != 0)[~edge], inside[~edge])
    assert np.abs(np.linalg.norm(out.point - p, axis=1) - out.dist).max() <= tol  # the point is where the distance says
    d_pt, _ = nc.independent_distance(geo.kind, geo.params, iso, out.point)
    assert np.abs(d_pt).max() <= tol  # ... and on the surface
    assert np.abs(np.linalg.norm(out.normal, axis=1) - 1.0).max() <= 2.0 ** -50
    off = ~edge
    with np.errstate(all="ignore"):
        along = ((p - out.point) * out.normal).sum(axis=1) / out.dist
    assert (np.abs(np.abs(along[off]) - 1.0) <= 2.0 ** -30).all()  # the normal lies along p - point ...
    assert ((along[off] > 0) == ~inside[off]).all() or kind == "plane"  # ... towards p outside, away from it inside (a plane's normal always faces p)
    if kind == "plane":
        assert (along[off] > 0).all()
    assert (out.flags & 2 != 0).all() == (kind == "ball") and ((out.flags & 2 != 0).any() == (kind == "ball"))


# ---- the box bound ---------------------------------------------------------------------------------------------------------------------------------------------
def test_the_box_bound_never_exceeds_the_exact_squared_distance():
    pts, boxes = nc.bound_cases()
    B = nr.nearest_box_bound_ref(pts, boxes)
    assert np.isfinite(B).all() and (B >= 0).all()
    loose = Fraction(0)
    for i, p in enumerate(pts):
        for j, b in enumerate(boxes):
            exact = nc.exact_box_d2(p, b)
            assert Fraction(float(B[i, j])) <= exact, (p, b, B[i, j])
            if exact > Fraction(10) ** -280 and exact < Fraction(10) ** 300:
                loose = max(loose, 1 - Fraction(float(B[i, j])) / exact)
    assert loose <= Fraction(1, 2 ** 49)  # ... and gives away no more than its own factor
    assert B[0, 0] == 0.0 and B[1, 0] == 0.0 and B[2, 0] == 0.0  # inside, on a face, at a corner: exactly zero


# ---- the margin ------------------------------------------------------------------------------------------------------------------------------------------------
def _violations(case, bound_of, skips):
    """How many (point, geometry-in-the-box) pairs of a case the rule `skips(bound, margin, key)` would cull although the mirror's key for that geometry is `key`."""
    name, nodes, box, pts, coord = case
    d2, _ = restated.nearest_node_d2_ref(nodes[0], pts)
    b = bound_of(pts, box)
    scale2 = (np.abs(pts).max(axis=1) + coord) ** 2
    return int(np.count_nonzero(skips(b, restated.nearest_margin_ref(b, scale2), d2)))


def _origin_tie():
    """Everything at the origin of a scene of extent 0: bound, margin and key are all exactly 0, and an equal bound must still be visited."""
    p = np.zeros((1, 3))
    return ("origin", [nc.node(nr.TriMesh(np.zeros((3, 3)), np.asarray([[0, 1, 2]], np.uint32)))], np.zeros(6), p, 0.0)


def test_the_margin_is_conservative_on_the_adversarial_set_and_every_mutant_is_caught():
    cases = nc.margin_cases() + [_origin_tie()]
    product = lambda pts, box: nr.nearest_box_bound_ref(pts, [box])[:, 0]  # noqa: E731
    for case in cases:
        assert _violations(case, product, restated.nearest_skips_ref) == 0, case[0]
    mutants = {
        "margin dropped": (product, lambda b, m, best: b > best),
        "< in place of <=": (product, lambda b, m, best: b - m >= best),  # (visits only what lies strictly below)
        "bound to the box centre": (lambda pts, box: ((pts - (box[:3] + box[3:]) / 2.0) ** 2).sum(axis=1), restated.nearest_skips_ref),
    }
    for name, (bound_of, skips) in mutants.items():
        caught = {case[0]: _violations(case, bound_of, skips) for case in cases}
        print(name, caught)
        assert any(caught.values()), name


# ---- the cross-check's point set ---------------------------------------------------------------------------------------------------------------------------------
def test_the_cross_check_leaves_out_at_most_two_percent_of_its_points():
    """The point set of the GPU cross-check (tests/test_nearest_gpu.py), on the mirror alone: the near ties and the rays that only touch an acute feature
    (nearest_cases.ray_only_touches) are together at most 2 % of the points.  With seed 29: no tie, 14 touching rays of 1 024 (13 at the mesh's boundary, one at the cone's
    rim); 302 more points lie behind their surface and are not asked either."""
    p = nc.cross_points()
    out = nr.nearest_points_ref(nc.cross_nodes(), p)
    left_out = nc.near_ties(nc.cross_nodes(), p, nc.cross_tau(p)) | nc.ray_only_touches(nc.cross_nodes(), p, out.node, out.point)
    print("left out: %d of %d" % (left_out.sum(), len(p)))
    assert left_out.mean() <= 0.02 and (out.flags & 1).all()
    usable = ~left_out & (out.flags & 4 == 0) & (out.dist > 2.0 ** -20)
    assert usable.mean() > 0.5
