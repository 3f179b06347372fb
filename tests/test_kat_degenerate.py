"""The analytic shape casts at DEGENERATE and NEAR-DEGENERATE rays against tests/golden/kat_degenerate.npz
(tests/golden/make_kat_degenerate.py: 60-digit mpmath on the shapes' convex gauges, no formula shared with oracle/nrays_oracle.c or
trace_device.h).  The closed forms of cylinder, cone and capsule are this project's own arithmetic (DESIGN D-3) and the oracle
restates the kernels line for line, so "HIP == oracle" cannot see a mistake both share; the random rays of kat_independent{,2}.npz never
have an exactly zero component, never run parallel to an axis, a face or a generator, never pass the apex and never graze.

A row the generator found WELL CONDITIONED (twelve perturbed solves) is held to the bound of tests/test_kat_independent.py,
|toi - exact| <= 1e-11 max(1, toi), and to its normal checks (unit to 1e-12, the plane through the hit point supports the shape to
1e-9 size, facing the ray for outside origins; a solid interior origin: toi == 0).  A SKIMMING row is held to hit / miss only, and only
where |g_min| >= margin * size, and its hit point must lie on the surface, |g(x)| <= 1e-9 size.  Nothing is dropped silently: COUNTS is
what the generator printed.

Measured, oracle and device alike (the device's figures equal the oracle's to the digit): |toi - exact| / max(1, toi) <= 1.4e-15 in every class
(worst: capsule perpendicular/rot), plane residual <= 3.0e-15 size, |g(x)| <= 2.9e-15 size on the skimming hits; 24 rows stay unasserted inside their
margin (rays that touch the apex only; cone rays in the base plane's neighbourhood).  On the cast_cone and cast_capsule before the repair (DESIGN D-3)
the same file fails 71 near_generator rows (worst 0.19) and 3 of generator_parallel/rot (0.19: the exact A == 0 directions once rotated), 24 of
cone_generator_skim_hit (1.6e-7), 22 hit / miss answers of cone_generator_skim_miss, 2 of apex/rot (1.1e-8) and returns a ZERO normal on 2 seam/rot rows.

The lattice mesh at the end is an exact class for triangles: integer vertices, integer origins, rays straight down through every interior
vertex and edge midpoint — every product and sum is exact in f64, so the toi is the integer and the tie goes to the smallest triangle index."""
import os

import numpy as np
import pytest

import nrays_amd as nr
import oracle
from tools import scenes_util as su

BALL, CUBOID, CYLINDER, CAPSULE, CONE = 0, 1, 2, 3, 4
NAMES = {BALL: "ball", CUBOID: "cuboid", CYLINDER: "cylinder", CAPSULE: "capsule", CONE: "cone"}
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat_degenerate.npz")

COUNTS = {  # (shape, class): (rows, hits, well conditioned) — printed by make_kat_degenerate.py; "/rot": the same rays under a generic rotation
    ("ball", "grazing_hit"): (16, 16, 0),
    ("ball", "grazing_hit/rot"): (16, 16, 0),
    ("ball", "grazing_miss"): (16, 0, 16),
    ("ball", "grazing_miss/rot"): (16, 0, 16),
    ("ball", "zero_components"): (44, 32, 44),
    ("ball", "zero_components/rot"): (44, 32, 44),
    ("cuboid", "corner_edge"): (18, 18, 18),
    ("cuboid", "corner_edge/rot"): (18, 18, 18),
    ("cuboid", "grazing_hit"): (24, 24, 24),
    ("cuboid", "grazing_hit/rot"): (24, 24, 24),
    ("cuboid", "grazing_miss"): (24, 0, 24),
    ("cuboid", "grazing_miss/rot"): (24, 0, 24),
    ("cuboid", "zero_components"): (46, 32, 46),
    ("cuboid", "zero_components/rot"): (46, 32, 46),
    ("cylinder", "along_axis"): (24, 24, 24),
    ("cylinder", "along_axis/rot"): (24, 24, 24),
    ("cylinder", "axis_parallel_inside"): (20, 20, 20),
    ("cylinder", "axis_parallel_inside/rot"): (20, 20, 20),
    ("cylinder", "axis_parallel_outside"): (16, 0, 16),
    ("cylinder", "axis_parallel_outside/rot"): (16, 0, 16),
    ("cylinder", "grazing_hit"): (48, 48, 32),
    ("cylinder", "grazing_hit/rot"): (48, 48, 32),
    ("cylinder", "grazing_miss"): (48, 0, 48),
    ("cylinder", "grazing_miss/rot"): (48, 0, 48),
    ("cylinder", "near_axis"): (160, 120, 160),
    ("cylinder", "near_axis/rot"): (160, 120, 160),
    ("cylinder", "perpendicular"): (100, 64, 100),
    ("cylinder", "perpendicular/rot"): (100, 64, 100),
    ("capsule", "along_axis"): (24, 24, 24),
    ("capsule", "along_axis/rot"): (24, 24, 24),
    ("capsule", "axis_parallel_inside"): (20, 20, 20),
    ("capsule", "axis_parallel_inside/rot"): (20, 20, 20),
    ("capsule", "axis_parallel_outside"): (16, 0, 16),
    ("capsule", "axis_parallel_outside/rot"): (16, 0, 16),
    ("capsule", "grazing_hit"): (48, 48, 0),
    ("capsule", "grazing_hit/rot"): (48, 48, 0),
    ("capsule", "grazing_miss"): (48, 0, 48),
    ("capsule", "grazing_miss/rot"): (48, 0, 48),
    ("capsule", "hemisphere_only"): (40, 32, 40),
    ("capsule", "hemisphere_only/rot"): (40, 32, 40),
    ("capsule", "near_axis"): (160, 120, 160),
    ("capsule", "near_axis/rot"): (160, 120, 160),
    ("capsule", "perpendicular"): (100, 84, 100),
    ("capsule", "perpendicular/rot"): (100, 84, 100),
    ("capsule", "seam"): (48, 48, 48),
    ("capsule", "seam/rot"): (48, 48, 48),
    ("cone", "along_axis"): (24, 24, 24),
    ("cone", "along_axis/rot"): (24, 24, 24),
    ("cone", "apex"): (40, 24, 36),
    ("cone", "apex/rot"): (40, 24, 36),
    ("cone", "axis_parallel_inside"): (20, 20, 20),
    ("cone", "axis_parallel_inside/rot"): (20, 20, 20),
    ("cone", "axis_parallel_outside"): (16, 0, 16),
    ("cone", "axis_parallel_outside/rot"): (16, 0, 16),
    ("cone", "cone_generator_skim_hit"): (24, 24, 24),
    ("cone", "cone_generator_skim_hit/rot"): (24, 24, 24),
    ("cone", "cone_generator_skim_miss"): (24, 0, 24),
    ("cone", "cone_generator_skim_miss/rot"): (24, 0, 24),
    ("cone", "generator_parallel"): (40, 20, 40),
    ("cone", "generator_parallel/rot"): (40, 20, 40),
    ("cone", "grazing_hit"): (40, 40, 16),
    ("cone", "grazing_hit/rot"): (40, 40, 16),
    ("cone", "grazing_miss"): (40, 0, 40),
    ("cone", "grazing_miss/rot"): (40, 0, 40),
    ("cone", "near_generator"): (160, 160, 160),
    ("cone", "near_generator/rot"): (160, 160, 160),
    ("cone", "perpendicular"): (100, 60, 92),
    ("cone", "perpendicular/rot"): (100, 60, 92),
    ("cone", "steeper"): (48, 40, 48),
    ("cone", "steeper/rot"): (48, 40, 48),
}
# the naive root pair (-B +- sq) / A, restated below, misses the toi bound on this many near-generator rows (of 320; non-solid interior and outside origins)
NAIVE_FAILS_AT_LEAST = 40

_cache = {}


def fixture():
    if not _cache:
        z = np.load(FIXTURE)
        _cache["cases"], _cache["classes"] = z["cases"], z["classes"]
        _cache["cases"].setflags(write=False)
    return _cache["cases"], _cache["classes"]


def gauge(kind, prm, p):
    """The shape's convex gauge in f64 (g <= 0 inside), as the generator's header defines it."""
    x, y, z = p
    if kind == BALL:
        return np.sqrt(x * x + y * y + z * z) - prm[0]
    if kind == CUBOID:
        return max(abs(x) - prm[0], abs(y) - prm[1], abs(z) - prm[2])
    hh, r = prm[0], prm[1]
    if kind == CAPSULE:
        yc = max(-hh, min(hh, y))
        return np.sqrt(x * x + (y - yc) ** 2 + z * z) - r
    rho = np.hypot(x, z)
    if kind == CYLINDER:
        return max(abs(y) - hh, rho - r)
    return max(abs(y) - hh, rho - r * (hh - y) / (2 * hh))


def support(kind, prm, n):
    """h(n) = max over the shape of n . p (local frame)."""
    if kind == BALL:
        return prm[0] * np.linalg.norm(n)
    if kind == CUBOID:
        return float(np.sum(np.asarray(prm) * np.abs(n)))
    hh, r = prm[0], prm[1]
    rad = np.hypot(n[0], n[2])
    if kind == CYLINDER:
        return hh * abs(n[1]) + r * rad
    if kind == CAPSULE:
        return hh * abs(n[1]) + r * np.linalg.norm(n)
    return max(hh * n[1], -hh * n[1] + r * rad)


def rotation(w):
    th = np.linalg.norm(w)
    if th == 0.0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def geometry(kind, prm):
    return {BALL: lambda: nr.Ball(prm[0]), CUBOID: lambda: nr.Cuboid(tuple(prm)), CYLINDER: lambda: nr.Cylinder(prm[0], prm[1]),
            CAPSULE: lambda: nr.Capsule(prm[0], prm[1]), CONE: lambda: nr.Cone(prm[0], prm[1])}[kind]()


def groups():
    """One scene per (shape, parameters, transform, solid): [(row indices, scene)], 32 of them, built once."""
    if "groups" not in _cache:
        cases, _ = fixture()
        keys = {}
        for i, c in enumerate(cases):
            keys.setdefault(tuple(c[0:11]), []).append(i)
        out = []
        for key, idx in keys.items():
            kind, prm, t, w, solid = int(key[0]), key[1:4], key[4:7], key[7:10], bool(key[10])
            node = nr.SceneNode(su.default_material(), 0.0, 0.0, 1.0, 1.0, nr.Isometry3(tuple(t), tuple(w)), geometry(kind, prm), None, solid)
            out.append((np.array(idx), nr.Scene([node], [])))
        _cache["groups"] = out
    return _cache["groups"]


def asserted(c):
    """Is hit / miss of this row asserted?  Always where well conditioned; a skimming row only outside its margin."""
    return bool(c[22]) or abs(c[20]) >= c[23] * c[21]


def check_rows(idx, hit, out, worst, label):
    """The record-path answers `hit`, `out` (oracle.cast's layout) of the rows `idx` against the fixture; the worst figures go to `worst`."""
    cases, classes = fixture()
    for j, i in enumerate(idx):
        c = cases[i]
        kind, prm, t, w, solid = int(c[0]), c[1:4], c[4:7], c[7:10], bool(c[10])
        o, d, want_hit, toi, was_inside, size, well = c[11:14], c[14:17], bool(c[17]), c[18], bool(c[19]), c[21], bool(c[22])
        tag = (NAMES[kind], str(classes[i]))
        ctx = (label, tag, int(i), list(c))
        wst = worst.setdefault(tag, {"toi_rel": 0.0, "surface": 0.0, "plane": 0.0, "unit": 0.0, "asserted": 0, "unasserted": 0})
        if not asserted(c):
            wst["unasserted"] += 1
        else:
            wst["asserted"] += 1
            assert bool(hit[j]) == want_hit, ctx
        if not hit[j]:
            continue
        got_toi, n = out[j, 0], out[j, 1:4]
        assert out[j, 7] == 0, ctx
        if was_inside and solid and want_hit:
            assert got_toi == 0.0, ctx
            continue
        R = rotation(w)
        ol, dl, nl = R.T @ (o - t), R.T @ d, R.T @ n
        x = ol + dl * got_toi
        if not (well and want_hit):  # a skimming hit: on the surface
            wst["surface"] = max(wst["surface"], abs(gauge(kind, prm, x)) / size)
            assert abs(gauge(kind, prm, x)) <= 1e-9 * size, ctx
            continue
        wst["toi_rel"] = max(wst["toi_rel"], abs(got_toi - toi) / max(1.0, toi))
        assert abs(got_toi - toi) <= 1e-11 * max(1.0, toi), ctx + (got_toi,)
        wst["unit"] = max(wst["unit"], abs(np.linalg.norm(n) - 1.0))
        assert abs(np.linalg.norm(n) - 1.0) <= 1e-12, ctx
        # ball and cuboid report the RAY-FACING normal for interior origins (SURVEY B-4 / B-5); the convex closed forms the exit point's outward normal (D-3)
        outward = -nl if (was_inside and kind in (BALL, CUBOID)) else nl
        res = abs(support(kind, prm, outward) - outward @ x) / size
        wst["plane"] = max(wst["plane"], res)
        assert res <= 1e-9, ctx + (res,)
        if was_inside and kind not in (BALL, CUBOID):
            assert nl @ dl > 0, ctx
        else:
            assert nl @ dl < 0, ctx


def report(worst, label):
    for tag in sorted(worst):
        w = worst[tag]
        print("%s %-8s %-32s asserted %3d / skimming inside its margin %2d: |toi - exact| / max(1, toi) %.2e, |g(x)| / size %.2e, plane residual / size %.2e, "
              "| |n| - 1 | %.2e" % (label, tag[0], tag[1], w["asserted"], w["unasserted"], w["toi_rel"], w["surface"], w["plane"], w["unit"]))


def check_fixture(cast, label, also=None):
    """`cast(scene, o, d)` -> (hit mask, (n, 8) records); `also(scene, rows, o, d, hit, out)`: further paths of the same scene (the GPU file)."""
    cases, _ = fixture()
    worst = {}
    try:
        for idx, scene in groups():
            o, d = np.ascontiguousarray(cases[idx, 11:14]), np.ascontiguousarray(cases[idx, 14:17])
            hit, out = cast(scene, o, d)
            check_rows(idx, hit, out, worst, label)
            if also is not None:
                also(scene, cases[idx], o, d, hit, out)
    finally:
        report(worst, label)
    assert set(worst) == set(COUNTS)


def test_the_fixture_holds_the_classes_the_generator_printed():
    cases, classes = fixture()
    got = {}
    for kind in NAMES:
        for cls in set(classes[cases[:, 0] == kind]):
            m = (cases[:, 0] == kind) & (classes == cls)
            got[(NAMES[kind], str(cls))] = (int(m.sum()), int(cases[m, 17].sum()), int(cases[m, 22].sum()))
    assert got == COUNTS
    assert all(n > 0 for n, _, _ in COUNTS.values()) and len(cases) == 3368 and len(groups()) == 32
    # the exact zeros are in the file: identity rows of the zero classes have a zero direction component, -0.0 among them
    ident = (cases[:, 7:10] == 0).all(axis=1)
    d = cases[ident & np.isin(classes, ["zero_components", "axis_parallel_inside", "perpendicular", "along_axis"]), 14:17]
    assert ((d == 0).sum(axis=1) >= 1).all() and np.signbit(d[d == 0]).any()
    near = cases[classes == "near_generator"]
    assert near[:, 22].all() and near[:, 17].all()  # well conditioned hits, every one: the 1e-11 bound applies to the rays of the cancelling roots


def test_oracle_casts_against_the_degenerate_fixture():
    check_fixture(lambda scene, o, d: oracle.cast(scene.descriptor, o, d), "oracle")


# ---- the cone's closed form restated with either root pair: the near-generator class must convict the naive one -------------
def cone_toi(hh, r, lo, ld, solid, naive):
    """cast_cone's interval arithmetic in Python floats (IEEE f64, unfused), on a LOCAL ray: toi or None."""
    k = r / (2.0 * hh); k2 = k * k
    ow, dw = hh - lo[1], -ld[1]
    s0, s1 = -np.inf, np.inf
    if dw == 0.0:
        if ow < 0.0 or ow > 2.0 * hh:
            return None
    else:
        ta, tb = (0.0 - ow) / dw, (2.0 * hh - ow) / dw
        s0, s1 = min(ta, tb), max(ta, tb)
    tc = -(lo[0] * ld[0] + lo[2] * ld[2] + ow * dw) / (ld[0] * ld[0] + ld[1] * ld[1] + ld[2] * ld[2])
    px, pz, pw = lo[0] + ld[0] * tc, lo[2] + ld[2] * tc, ow + dw * tc  # the quadratic about the ray's point nearest the apex
    A = ld[0] * ld[0] + ld[2] * ld[2] - k2 * dw * dw
    B = px * ld[0] + pz * ld[2] - k2 * pw * dw
    C = px * px + pz * pz - k2 * pw * pw
    t0, t1 = s0, s1
    if A != 0.0:
        disc = B * B - A * C
        if disc < 0.0 and A > 0.0:
            return None
        if disc >= 0.0 and (A > 0.0 or disc > 0.0):
            sq = np.sqrt(disc)
            if naive:
                r1, r2 = (-B - sq) / A, (-B + sq) / A
            else:
                q = -(B + np.copysign(sq, B))
                r1 = q / A
                r2 = C / q if q != 0.0 else r1
            lo_r, hi_r = min(r1, r2) + tc, max(r1, r2) + tc
            if A > 0.0:
                t0, t1 = max(t0, lo_r), min(t1, hi_r)
            elif dw > 0.0:
                t0 = max(hi_r, s0)
            else:
                t1 = min(lo_r, s1)
    elif B == 0.0:
        if C > 0.0:
            return None
    else:
        ts = -C / (2.0 * B) + tc
        if B > 0.0:
            t1 = min(t1, ts)
        else:
            t0 = max(t0, ts)
    if not (t0 <= t1) or t1 < 0.0:
        return None
    return t0 if t0 > 0.0 else (0.0 if solid else t1)


def _near_generator_misses(naive):
    cases, classes = fixture()
    rows = cases[np.isin(classes, ["near_generator", "near_generator/rot"])]
    bad, worst = 0, 0.0
    for c in rows:
        R = rotation(c[7:10])
        got = cone_toi(c[1], c[2], R.T @ (c[11:14] - c[4:7]), R.T @ c[14:17], bool(c[10]), naive)
        err = np.inf if got is None else abs(got - c[18]) / max(1.0, c[18])
        bad += err > 1e-11
        worst = max(worst, err)
    return bad, len(rows), worst


def test_the_naive_root_pair_fails_the_near_generator_class():
    """The power of the class: (-B +- sq) / A, the cone's root pair before the repair, must exceed the bound on the rays a few ulps off a
    generator, and the stable pair q = -(B + copysign(sq, B)), q / A, C / q must not — otherwise the oracle test passes for the wrong reason."""
    bad, n, worst = _near_generator_misses(naive=True)
    print("naive root pair: %d of %d near-generator rows beyond 1e-11 max(1, toi), worst %.2e" % (bad, n, worst))
    assert n == 320 and bad >= NAIVE_FAILS_AT_LEAST and worst > 1e-3
    bad, n, worst = _near_generator_misses(naive=False)
    print("stable root pair: %d of %d, worst %.2e" % (bad, n, worst))
    assert bad == 0


# ---- the lattice mesh: an exact class for triangles -------------------------------------------------------------------------
def lattice_mesh(cells):
    """cells x cells quads over [0, cells]^2 at integer heights y = (3 i + 5 j) mod 4; quad (i, j) is triangles 2 (j cells + i) and + 1,
    split along the diagonal from (i, j) to (i + 1, j + 1)."""
    g = np.arange(cells + 1)
    ii, jj = np.meshgrid(g, g, indexing="xy")
    pts = np.stack([ii, (3 * ii + 5 * jj) % 4, jj], axis=-1).reshape(-1, 3).astype(np.float64)
    vid = lambda i, j: j * (cells + 1) + i
    tris = []
    for j in range(cells):
        for i in range(cells):
            tris += [(vid(i, j), vid(i + 1, j), vid(i + 1, j + 1)), (vid(i, j), vid(i + 1, j + 1), vid(i, j + 1))]
    return pts, np.array(tris, dtype=np.uint32)


def lattice_rays(cells):
    """Rays straight down and straight up through every interior vertex and every interior edge midpoint (doubled coordinates keep the midpoints
    exact), and rays one unit beside the mesh.  Returns origins, directions, the exact toi (inf: a miss) and the smallest index among the tied triangles."""
    pts, tris = lattice_mesh(cells)
    P = pts[tris.astype(np.int64)]
    o, d, toi, prim, normal = [], [], [], [], []
    ax, az, bx, bz, cx, cz = (2 * P[:, 0, 0], 2 * P[:, 0, 2], 2 * P[:, 1, 0], 2 * P[:, 1, 2], 2 * P[:, 2, 0], 2 * P[:, 2, 2])
    for x2 in range(1, 2 * cells):  # every interior point of the half-integer lattice is a vertex, the midpoint of an axis-parallel edge, or of a diagonal
        for z2 in range(1, 2 * cells):
            # exact containment in the xz projection, with integers (doubled coordinates); the edges belong to both neighbours
            e0 = (bx - ax) * (z2 - az) - (bz - az) * (x2 - ax)
            e1 = (cx - bx) * (z2 - bz) - (cz - bz) * (x2 - bx)
            e2 = (ax - cx) * (z2 - cz) - (az - cz) * (x2 - cx)
            tied = np.nonzero(((e0 >= 0) & (e1 >= 0) & (e2 >= 0)) | ((e0 <= 0) & (e1 <= 0) & (e2 <= 0)))[0]
            k = tied[0]
            area = e0[k] + e1[k] + e2[k]
            y = (e1[k] * P[k, 0, 1] + e2[k] * P[k, 1, 1] + e0[k] * P[k, 2, 1]) / area  # the weights are 0, 1/2 or 1: a vertex height or the mean of two
            assert len(tied) >= 2 and y * 2 == int(y * 2)
            n = np.cross(P[k, 1] - P[k, 0], P[k, 2] - P[k, 0]); n /= np.linalg.norm(n)
            for s in (1.0, -1.0):
                o.append((x2 / 2.0, y + s * 8.0, z2 / 2.0)); d.append((0.0, -s, 0.0)); toi.append(8.0); prim.append(k)
                normal.append(n if n[1] * s > 0 else -n)  # the flat normal of the smallest tied triangle, facing the ray's origin
    for x, z in ((-1.0, 1.0), (cells + 1.0, 2.0), (2.0, -1.0), (1.0, cells + 1.0)):
        for s in (1.0, -1.0):
            o.append((x, s * 8.0, z)); d.append((0.0, -s, 0.0)); toi.append(np.inf); prim.append(-1); normal.append(np.zeros(3))
    return np.array(o), np.array(d), np.array(toi), np.array(prim), np.array(normal)


def lattice_scene(cells, translation):
    pts, tris = lattice_mesh(cells)
    return nr.Scene([nr.SceneNode(su.default_material(), 0.0, 0.0, 1.0, 1.0, nr.Isometry3(tuple(translation)), nr.TriMesh(pts, tris))], [])


@pytest.mark.parametrize("translation", [(0.0, 0.0, 0.0), (7.0, -3.0, 11.0)])
def test_oracle_rays_through_lattice_vertices_and_edge_midpoints_are_exact(translation):
    """4 x 4 quads, 32 triangles (the host builder).  The oracle's record has no triangle index: the winner of the tie shows in the normal."""
    o, d, toi, prim, normal = lattice_rays(4)
    assert len(o) == 2 * (9 + 24 + 16) + 8 and (prim >= 0).sum() == len(o) - 8
    hit, out = oracle.cast(lattice_scene(4, translation).descriptor, o + np.array(translation), d)
    assert np.array_equal(hit, np.isfinite(toi))
    assert np.array_equal(out[hit, 0], toi[hit]) and (out[hit, 7] == 0).all()
    assert np.abs(out[hit, 1:4] - normal[hit]).max() <= 1e-15
