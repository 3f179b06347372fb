"""Shared case builders of tests/test_nearest.py (the numpy mirror against exact rationals and independent closed forms) and tests/test_nearest_gpu.py (the device
against the mirror by bit pattern).  Everything here is made once per process and left unchanged."""
import functools
import math
from fractions import Fraction

import numpy as np

import nrays_amd as nr
from nrays_amd import abi, math3d

F32 = np.float32
MAT = lambda: nr.NormalMaterial()  # noqa: E731
ISO = nr.Isometry3((0.375, -1.25, 2.0), (0.3, -0.5, 0.8))  # a rotated, translated isometry
N_POINTS = 4128  # tests/stack_cases.py's count: 16 full workgroups and a part of one


def f32x(a):
    return np.asarray(a, F32).astype(np.float64)


def node(geometry, iso=None, material=None):
    return nr.SceneNode(material or MAT(), 0.0, 0.0, 1.0, 1.0, iso or nr.Isometry3(), geometry)


def scene(nodes):
    return nr.Scene(nodes, [nr.Light((0.0, 10.0, 0.0), 0.0, 1, (1, 1, 1))], (0.25, 0.5, 0.75))


def same(a, b):
    """Bit patterns equal, any NaN equal to any NaN; integer arrays by value."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return bool((a.astype(np.int64) == b.astype(np.int64)).all())
    return bool(((a.view(np.uint64) == b.astype(np.float64).view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


# ---- one and two triangles -------------------------------------------------------------------------------------------------------------------------------------
TRI = f32x([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
TRI_UV = f32x([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])


def one_triangle_nodes():
    return [node(nr.TriMesh(TRI, np.asarray([[0, 1, 2]], np.uint32), TRI_UV))]


def voronoi_points():
    """(points, expected region): one point per Voronoi region of TRI off the plane, then exactly on each vertex, on each edge and on the face."""
    pts = [(-1.0, -1.0, 0.5), (3.0, -0.5, 0.5), (1.0, -1.0, 0.5), (-0.5, 2.0, 0.5), (-1.0, 0.5, 0.5), (2.0, 2.0, 0.5), (0.5, 0.25, 0.5),
           (0.0, 0.0, 0.0), (2.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.5, 0.0), (1.0, 0.5, 0.0), (0.5, 0.25, 0.0)]
    # (a point ON a vertex or an edge falls to the first test of Ericson's order that accepts it: the vertex tests come before the edges', both before the interior)
    region = [0, 1, 2, 3, 4, 5, 6, 0, 1, 2, 3, 4, 5, 6]
    return np.asarray(pts, np.float64), np.asarray(region)


def two_triangle_nodes(split=False):
    """Two triangles mirrored in the plane x = 0 — every point of that plane is equidistant from both: one mesh of two triangles, or (`split`) two nodes of one."""
    a = f32x([[0.5, 0.0, 0.0], [2.5, 0.0, 0.0], [0.5, 1.0, 0.0]])
    b = a * np.asarray([-1.0, 1.0, 1.0])
    if split:
        return [node(nr.TriMesh(a, np.asarray([[0, 1, 2]], np.uint32))), node(nr.TriMesh(b, np.asarray([[0, 1, 2]], np.uint32)))]
    return [node(nr.TriMesh(np.concatenate([a, b]), np.asarray([[0, 1, 2], [3, 4, 5]], np.uint32)))]


def tie_points(n=64, seed=3):
    """Points of the plane x = 0, and the same a step to either side of it."""
    rng = np.random.default_rng(seed)
    p = np.zeros((n, 3)); p[:, 1:] = rng.uniform(-2.0, 3.0, (n, 2))
    return np.concatenate([p, p + [2.0 ** -30, 0, 0], p - [2.0 ** -30, 0, 0]])


# ---- the analytic scene ----------------------------------------------------------------------------------------------------------------------------------------
SHAPES = {"ball": lambda: nr.Ball(0.75), "cuboid": lambda: nr.Cuboid((0.5, 0.75, 1.0)), "cylinder": lambda: nr.Cylinder(0.75, 0.5), "capsule": lambda: nr.Capsule(0.5, 0.375),
          "cone": lambda: nr.Cone(0.75, 0.5)}
PLACES = {"ball": nr.Isometry3((-3.0, 0.5, 0.25), (0.2, 0.4, -0.3)), "cuboid": nr.Isometry3((0.0, 0.25, 0.0), (0.3, -0.5, 0.8)), "cylinder": nr.Isometry3((3.0, 0.5, -0.5), (-0.7, 0.1, 0.2)),
          "capsule": nr.Isometry3((0.5, 0.5, 3.0), (0.0, 0.0, 0.0)), "cone": nr.Isometry3((-0.5, 0.75, -3.0), (1.1, 0.3, -0.4))}
PLANE_ISO = nr.Isometry3((0.0, -1.5, 0.0), (0.0, 0.0, 0.1))


def analytic_nodes():
    """One node per analytic shape, rotated and translated (the capsule only translated), plus a tilted plane below them."""
    return [node(SHAPES[k](), PLACES[k]) for k in SHAPES] + [node(nr.Plane((0.0, 1.0, 0.0)), PLANE_ISO)]


def frame(iso):
    return np.array(math3d.rotation_from_axis_angle(iso.axis_angle), np.float64).reshape(3, 3), np.array(iso.translation, np.float64)


def special_local_points(kind):
    """Local points of a shape of SHAPES: outside, inside, on the axis, at the centre, on a rim / edge / corner, on the surface."""
    base = [(2.0, 1.5, -1.0), (0.125, 0.0625, -0.1), (0.0, 0.3, 0.0), (0.0, 2.0, 0.0), (0.0, -2.0, 0.0), (0.0, 0.0, 0.0), (1.5, 0.0, 0.0), (0.2, 0.6, 0.1), (0.3, -0.7, -0.2)]
    rim = {"ball": [(0.75, 0.0, 0.0)], "cuboid": [(0.5, 0.75, 1.0), (0.5, 0.75, 0.0), (0.5, 0.0, 0.0), (1.0, 1.5, 0.25)], "cylinder": [(0.5, 0.75, 0.0), (0.0, 0.75, 0.0), (0.5, 0.0, 0.0), (1.0, 1.0, 0.0)],
           "capsule": [(0.375, 0.0, 0.0), (0.0, 0.875, 0.0), (0.0, 0.5, 0.0)], "cone": [(0.5, -0.75, 0.0), (0.0, 0.75, 0.0), (0.0, -0.75, 0.0), (0.25, 0.0, 0.0), (1.0, -1.0, 0.0)]}
    return np.asarray(base + rim[kind], np.float64)


@functools.lru_cache(None)
def analytic_points(n=N_POINTS, seed=17):
    """Points all over the analytic scene: a cloud around it, each shape's special points under its isometry, and points under the plane."""
    rng = np.random.default_rng(seed)
    sp = []
    for k in SHAPES:
        R, T = frame(PLACES[k])
        sp.append(special_local_points(k) @ R.T + T)
    sp = np.concatenate(sp)
    cloud = rng.uniform(-5.0, 5.0, (n - len(sp), 3))
    cloud[::7] *= 40.0
    p = np.concatenate([sp, cloud])
    p.setflags(write=False)
    return p


# ---- the grid mesh at the device builder's threshold ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def grid_mesh(cells=32):
    """A wavy cells x cells grid of 2 cells^2 triangles (2 048: the device builder's threshold) with uvs, coordinates f32-exact."""
    g = np.arange(cells + 1, dtype=np.float64) / 8.0 - cells / 16.0
    x, z = np.meshgrid(g, g, indexing="xy")
    y = f32x(0.25 * np.sin(1.7 * x) * np.cos(1.3 * z))
    pts = np.stack([x, y, z], axis=-1).reshape(-1, 3)
    uv = f32x(np.stack([(x - g[0]) / (g[-1] - g[0]), (z - g[0]) / (g[-1] - g[0])], axis=-1).reshape(-1, 2))
    i = (np.arange(cells)[:, None] * (cells + 1) + np.arange(cells)[None, :]).reshape(-1)
    idx = np.concatenate([np.stack([i, i + 1, i + cells + 2], 1), np.stack([i, i + cells + 2, i + cells + 1], 1)]).astype(np.uint32)
    for a in (pts, idx, uv):
        a.setflags(write=False)
    return f32x(pts), idx, uv


def grid_nodes(iso=None):
    pts, idx, uv = grid_mesh()
    return [node(nr.TriMesh(pts, idx, uv), iso)]


@functools.lru_cache(None)
def grid_points(n=N_POINTS, seed=23):
    """A third on the surface (barycentric combinations of a triangle's corners), a third within a cell of it, a third far."""
    pts, idx, _ = grid_mesh()
    rng = np.random.default_rng(seed)
    k = n // 3
    t = rng.integers(0, len(idx), 2 * k)
    w = rng.dirichlet((1.0, 1.0, 1.0), 2 * k)
    V = pts[idx[t].astype(np.int64)]
    on = (V * w[:, :, None]).sum(axis=1)
    near = on[k:] + rng.uniform(-0.125, 0.125, (k, 3))
    far = rng.uniform(-30.0, 30.0, (n - 2 * k, 3))
    p = np.concatenate([on[:k], near, far])
    p.setflags(write=False)
    return p


# ---- exact rationals -------------------------------------------------------------------------------------------------------------------------------------------
def _fr(v):
    return [Fraction(float(x)) for x in v]


def _seg_d2(p, a, b):
    ab = [y - x for x, y in zip(a, b)]
    ap = [y - x for x, y in zip(a, p)]
    den = sum(x * x for x in ab)
    t = Fraction(0) if den == 0 else max(Fraction(0), min(Fraction(1), sum(x * y for x, y in zip(ab, ap)) / den))
    return sum((pp - (x + t * d)) ** 2 for pp, x, d in zip(p, a, ab))


def exact_tri_d2(a, b, c, p):
    """The exact squared distance from p to the triangle: the minimum over the three clamped edge projections and the plane projection when it falls inside."""
    a, b, c, p = _fr(a), _fr(b), _fr(c), _fr(p)
    best = min(_seg_d2(p, a, b), _seg_d2(p, b, c), _seg_d2(p, c, a))
    ab = [y - x for x, y in zip(a, b)]; ac = [y - x for x, y in zip(a, c)]; ap = [y - x for x, y in zip(a, p)]
    n = [ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]]
    nn = sum(x * x for x in n)
    if nn != 0:
        d00, d01, d11 = sum(x * x for x in ab), sum(x * y for x, y in zip(ab, ac)), sum(x * x for x in ac)
        d20, d21 = sum(x * y for x, y in zip(ap, ab)), sum(x * y for x, y in zip(ap, ac))
        den = d00 * d11 - d01 * d01
        v, w = (d11 * d20 - d01 * d21) / den, (d00 * d21 - d01 * d20) / den
        if v >= 0 and w >= 0 and v + w <= 1:
            best = min(best, sum(x * y for x, y in zip(ap, n)) ** 2 / nn)
    return best


FAMILIES = ("random", "far", "near_surface", "sliver", "sliver_collinear_f32", "collinear", "point", "offset_1000")


def family_cases(name, count, seed=41):
    """`count` cases (a, b, c, p) of a family, f32-exact triangles and float64 points."""
    rng = np.random.default_rng(seed + FAMILIES.index(name))
    out = []
    for _ in range(count):
        a, b, c = (f32x(rng.uniform(-2.0, 2.0, 3)) for _ in range(3))
        p = rng.uniform(-3.0, 3.0, 3)
        if name == "far":
            p = rng.uniform(-1.0, 1.0, 3) * 10.0 ** rng.uniform(2, 8)
        elif name == "near_surface":
            w = rng.dirichlet((1.0, 1.0, 1.0))
            p = a * w[0] + b * w[1] + c * w[2] + rng.uniform(-1e-9, 1e-9, 3)
        elif name == "sliver":
            c = f32x(a + (b - a) * rng.uniform(0.1, 0.9) + rng.uniform(-1e-6, 1e-6, 3))
        elif name == "sliver_collinear_f32":
            c = f32x(a + (b - a) * rng.uniform(0.1, 0.9))
        elif name == "collinear":
            d = f32x(rng.integers(-8, 9, 3) / 8.0)
            a = f32x(rng.integers(-8, 9, 3) / 4.0); b = f32x(a + d * 2.0); c = f32x(a + d * rng.integers(-3, 6))
        elif name == "point":
            b = a.copy(); c = a.copy()
        elif name == "offset_1000":
            o = f32x(rng.integers(-1, 2, 3) * 1000.0)
            a, b, c = f32x(a + o), f32x(b + o), f32x(c + o)
            p = o + rng.uniform(-3.0, 3.0, 3)
        out.append((a, b, c, np.asarray(p, np.float64)))
    return out


def exact_box_d2(p, box):
    p, lo, hi = _fr(p), _fr(np.asarray(box[:3], F32)), _fr(np.asarray(box[3:], F32))
    return sum(max(l - x, x - h, Fraction(0)) ** 2 for x, l, h in zip(p, lo, hi))


def bound_cases():
    """(points, boxes) of the bound's checks: inside, on a face, at a corner, far, at huge coordinates and at denormal gaps."""
    tiny = 5e-324
    boxes = np.asarray([[-1, -2, -3, 1, 2, 3], [0.5, 0.5, 0.5, 0.75, 1.5, 2.5], [1e30, -1e30, 0, 2e30, 1e30, 1], [0, 0, 0, 0, 0, 0],
                        [-3.0e38, -3.0e38, -3.0e38, 3.0e38, 3.0e38, 3.0e38], [1.0, 1.0, 1.0, 1.0 + 2.0 ** -23, 1.0 + 2.0 ** -23, 1.0 + 2.0 ** -23]], np.float64)
    rng = np.random.default_rng(5)
    pts = [(0, 0, 0), (1, 0, 0), (1, 2, 3), (-1, -2, -3), (1 + 2.0 ** -52, 2, 3), (np.nextafter(1.0, 2.0), np.nextafter(2.0, 3.0), np.nextafter(3.0, 4.0)), (tiny, -tiny, tiny),
           (1e-170, 1e-170, 1e-170), (1e-160, 0, 0), (1e300, -1e300, 1e300), (1.7e308, 1.7e308, -1.7e308), (1e154, 1e154, 1e154), (1e38, -1e38, 1e38), (3.5e38, 0, 0),
           (1.0 - 2.0 ** -53, 1.0, 1.0), (1.0 + 2.0 ** -23 + 2.0 ** -52, 1.0, 1.0), (0.5, 0.5, 0.5), (0.75, 1.5, 2.5)]
    pts = np.concatenate([np.asarray(pts, np.float64), rng.uniform(-4.0, 4.0, (64, 3)), rng.uniform(-1.0, 1.0, (32, 3)) * 10.0 ** rng.uniform(-300, 300, (32, 1))])
    return pts, boxes


# ---- independent closed forms of the analytic shapes (no code shared with the mirror: rho and y are computed here, the frame through a matrix product) --------------
def independent_distance(kind, params, iso, p):
    """(unsigned distance from the world points p to the shape's surface, strictly inside) in math3d terms."""
    R, T = frame(iso)
    q = (np.asarray(p, np.float64) - T) @ R  # R^T (p - T), row vectors
    p0, p1, p2 = params
    if kind == abi.SHAPE_BALL:
        ln = np.linalg.norm(q, axis=1)
        return np.abs(ln - p0), ln < p0
    if kind == abi.SHAPE_PLANE:
        t = q @ np.asarray(params)
        return np.abs(t), t < 0
    if kind == abi.SHAPE_CUBOID:
        e = np.abs(q) - np.asarray(params)
        outside = np.linalg.norm(np.maximum(e, 0.0), axis=1)
        inside = -e.max(axis=1)
        return np.where((e <= 0).all(axis=1), inside, outside), (e < 0).all(axis=1)
    rho, y = np.hypot(q[:, 0], q[:, 2]), q[:, 1]
    if kind == abi.SHAPE_CYLINDER:
        er, ey = rho - p1, np.abs(y) - p0
        return np.where((er <= 0) & (ey <= 0), np.minimum(-er, -ey), np.hypot(np.maximum(er, 0), np.maximum(ey, 0))), (er < 0) & (ey < 0)
    if kind == abi.SHAPE_CAPSULE:
        ln = np.hypot(rho, y - np.clip(y, -p0, p0))
        return np.abs(ln - p1), ln < p1
    if kind == abi.SHAPE_CONE:  # apex (0, +hh), base radius r at -hh
        def seg(ax, ay, bx, by):
            dx, dy = bx - ax, by - ay
            t = np.clip(((rho - ax) * dx + (y - ay) * dy) / (dx * dx + dy * dy), 0.0, 1.0)
            return np.hypot(rho - (ax + t * dx), y - (ay + t * dy))
        d = np.minimum(seg(0.0, -p0, p1, -p0), seg(p1, -p0, 0.0, p0))
        return d, (y > -p0) & (rho * 2.0 * p0 < p1 * (p0 - y))
    raise KeyError(kind)


# ---- the margin's adversarial set --------------------------------------------------------------------------------------------------------------------------------
ROT45 = nr.Isometry3((3.0, 2.0, 1.0), (math.pi / 4.0, 0.0, 0.0))  # 45 degrees about x: the world z of a local point mixes its y and z (margin_cases sets the translation's z)


def tight_box(world_pts):
    """The f32 box around world points, rounded outward only where a coordinate is not f32-exact: a face through an f32-exact coordinate TOUCHES the geometry."""
    lo, hi = world_pts.min(axis=0), world_pts.max(axis=0)
    l32, h32 = lo.astype(F32), hi.astype(F32)
    l32 = np.where(l32.astype(np.float64) > lo, np.nextafter(l32, F32(-np.inf)), l32)
    h32 = np.where(h32.astype(np.float64) < hi, np.nextafter(h32, F32(np.inf)), h32)
    return np.concatenate([l32, h32]).astype(np.float64)


def margin_cases(seed=7, per=400):
    """[(name, nodes of one triangle, box (6,) around its world geometry, points, coordinate bound)]: the triangle touching its box face (untransformed; the points above
    that face), the point at an f32 corner of the box, and the instance turned by 45 degrees whose top corner sits at its f32-exact translation, so that the world box's
    top face passes through the geometry while the key is computed in the turned local frame."""
    rng = np.random.default_rng(seed)
    idx = np.asarray([[0, 1, 2]], np.uint32)
    out = []
    flat = f32x([[1000.0, 1000.0, 1000.0], [1001.0, 1000.25, 1000.0], [1000.25, 1001.0, 999.5]])  # AB lies in the face z = 1000
    pts = np.stack([rng.uniform(999.5, 1001.5, per), rng.uniform(999.5, 1001.5, per), 1000.0 + 10.0 ** rng.uniform(-9, 0, per)], axis=1)
    out.append(("face", [node(nr.TriMesh(flat, idx))], tight_box(flat), pts, 1001.0))
    box = tight_box(flat)
    corner = np.asarray([[box[3 if i & 1 else 0], box[4 if i & 2 else 1], box[5 if i & 4 else 2]] for i in range(8)], np.float64)
    out.append(("corner", [node(nr.TriMesh(flat, idx))], box, np.concatenate([corner, np.nextafter(corner, np.inf), np.nextafter(corner, -np.inf)]), 1001.0))
    # the turned instance: its highest corner v0 lies 1024 units from the local origin, and the translation's z is chosen so that v0's world z is the f32-exact 2048:
    # the world box's top face passes through v0, while the key is computed from pl = R^T (p - T), whose rounding (2^-53 of ~1448) is not small beside a distance of 1e-3
    v0 = np.asarray([0.0, 1024.0, 1024.0])
    local = f32x([v0, v0 + [1.0, -0.5, -0.75], v0 + [-0.5, -1.0, -0.25]])
    R, _ = frame(ROT45)
    z0 = (R[2, 0] * v0[0] + R[2, 1] * v0[1]) + R[2, 2] * v0[2]
    iso = nr.Isometry3((3.0, 2.0, 2048.0 - z0), ROT45.axis_angle)
    T = np.asarray(iso.translation)
    world = np.stack([(R[k, 0] * local[:, 0] + R[k, 1] * local[:, 1]) + R[k, 2] * local[:, 2] for k in range(3)], axis=1) + T
    assert world[0, 2] == 2048.0 and world[:, 2].argmax() == 0
    pts = world[0] + np.stack([np.zeros(per), np.zeros(per), 10.0 ** rng.uniform(-6, -1, per)], axis=1)
    out.append(("rot45", [node(nr.TriMesh(local, idx), iso)], tight_box(world), pts, float(np.abs(world).max() + np.abs(T).max())))
    return out


# ---- the cross-check scene ---------------------------------------------------------------------------------------------------------------------------------------
GRID_ISO = nr.Isometry3((0.25, -0.875, 0.5), (0.0, 0.3, 0.0))
CROSS_SEED = 29


def cross_nodes():
    """The analytic scene and the grid mesh, scaled by 2.5 (its footprint then reaches beyond the point cloud: few points are nearest to its boundary), turned and lowered."""
    pts, idx, uv = grid_mesh()
    return analytic_nodes() + [node(nr.TriMesh(f32x(pts * 2.5), idx, uv), GRID_ISO)]


@functools.lru_cache(None)
def cross_points(n=1024, seed=CROSS_SEED):
    """A cloud over the scene; in z it stops short of the cone, whose rim and apex are acute features (ray_only_touches)."""
    rng = np.random.default_rng(seed)
    p = np.stack([rng.uniform(-4.5, 4.5, n), rng.uniform(-1.5, 3.0, n), rng.uniform(-1.75, 4.5, n)], axis=1)
    p.setflags(write=False)
    return p


CROSS_RADIUS = 9.0  # every bounded node of cross_nodes() lies within this distance of the origin


def cross_tau(p):
    """2^-40 (|p| + the scene's bounding radius): f64's 2^-53 with 2^13 for the few dozen operations either side."""
    return 2.0 ** -40 * (np.linalg.norm(p, axis=1) + CROSS_RADIUS)


def near_ties(nodes, p, tau):
    """Points whose two nearest NODES are closer than tau to a tie (the ray towards the nearest point may then meet the other one first)."""
    d = np.sqrt(np.stack([nr.restated.nearest_node_d2_ref(nd, p)[0] for nd in nodes], axis=1))
    d.sort(axis=1)
    return d[:, 1] - d[:, 0] < tau


def ray_only_touches(nodes, p, node_ids, q):
    """Whether the ray from p towards the surface point q of node node_ids[i] merely TOUCHES that node at q instead of entering it.  At a convex feature whose interior angle is
    acute — the cone's rim (71.6 degrees) and apex (36.9), a mesh's boundary edge (0) — the points nearest to the feature span more directions (180 degrees less the
    interior angle) than lead into the solid: from most of them the ray grazes q, and whether a cast reports a grazing contact is decided by rounding, like a tie between a
    hit and a miss.  Independent of the code under test: a closed shape by independent_distance's inside test one step of 2^-20 behind q along the ray, the plane never, the
    grid mesh by q lying on the rim of its footprint."""
    d = (q - p) / np.linalg.norm(q - p, axis=1, keepdims=True)
    out = np.zeros(len(p), bool)
    for k in np.unique(node_ids[node_ids >= 0]):
        nd, at = nodes[int(k)], node_ids == k
        g = nd.geometry
        if g.kind == abi.SHAPE_TRIMESH:
            R, T = frame(nd.transform)
            local = (q[at] - T) @ R
            half = float(np.abs(np.asarray(g.points)[:, [0, 2]]).max())
            out[at] = np.abs(local[:, [0, 2]]).max(axis=1) >= half - 2.0 ** -20
        elif g.kind != abi.SHAPE_PLANE:
            out[at] = ~independent_distance(g.kind, g.params, nd.transform, q[at] + d[at] * 2.0 ** -20)[1] & ~independent_distance(g.kind, g.params, nd.transform, p[at])[1]  # (from outside)
    return out
