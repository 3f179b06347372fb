"""The traversal stack beyond its LDS slots (trace_device.h: Stack — kLdsStack slots per lane in LDS, deeper ones in the lane's column of an
HBM region): the meshes, scenes and rays that make a lane hold more than kLdsStack entries, and the proof that they do.

The ladder: rungs perpendicular to x at x = sign * ratio^k (f32-exact), each a kite over part of the square [-1, 3]^2 in (y, z) — "plain"
rungs along one diagonal, every fourth rung "flipped" along the other.  Every rung has the same box up to its x, so the flip pattern does
not change the tree.  The SAH of build_bvh peels a few far rungs off per level: a chain as deep as the mesh has rungs / 5, which a ray
along the ladder descends to its end with two or three deferred siblings per level.  A ray beside the plain kites finds its hit — on a
flipped rung, or none — only after popping back up the chain, out of its HBM slots; different lanes meet different rungs.

simulate() walks a dumped 4-wide tree (the NraysBlasDump layout) in the visiting orders of traverse() and returns the largest number of
slots in use per ray, the bottom marker and the sentinel included.  It is evidence of reach, not an expected value of the device: its box
tests are exact f64 slabs, the device's f32 culling accepts slightly more; and it walks ONE mesh — what a scene keeps on the stack below the
sentinel (plane pseudo-leaves, deferred TLAS children) comes on top of its figure.
tests/test_stack_spill.py asserts the reach, tests/test_stack_spill_gpu.py runs the same cases on the device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import nrays_amd as nr
from nrays_amd import math3d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nrays_amd", "csrc")
F32 = np.float32
EMPTY = -2 ** 31                      # kEmptyChild
BACKGROUND = (0.25, 0.5, 0.75)
N_RAYS = 4128                         # 16 workgroups of 256 and a seventeenth of 32 rays: 64 blocks of 64 and half a block
CLASSES = ("near", "far", "oblique", "between")


def _define(path, name):
    m = re.search(r"^#define %s (\d+)" % name, open(os.path.join(CSRC, path)).read(), re.M)
    assert m, (path, name)
    return int(m.group(1))


def lds_stack():
    """kLdsStack as the kernels are compiled (trace_device.h: NR_LDS_STACK)."""
    return _define("trace_device.h", "NR_LDS_STACK")


def max_leaf():
    return _define("scene_build.cpp", "NR_MAX_LEAF")


def need(max_depth, planes=0):
    """derive_scene_facts' sizing rule: the slots a lane may use, LDS and HBM together."""
    return 6 * (max_depth + 1) + planes + 9


# ---------------------------------------------------------------- the host builder ------------------------------------------------------------

class BuildShim:
    """tests/bvh_build_shim.cpp: nrays_amd/csrc/bvh_build.cpp compiled by the host compiler."""

    def __init__(self, directory):
        out = os.path.join(str(directory), "libbvh_build_shim.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-I", CSRC, "-I", os.path.join(ROOT, "include"), "-o", out,
                               os.path.join(ROOT, "tests", "bvh_build_shim.cpp"), os.path.join(CSRC, "bvh_build.cpp")])
        self.lib = C.CDLL(out)
        self.lib.bvh_shim_build.restype = C.c_uint32
        self.lib.bvh_shim_build.argtypes = [C.c_uint32, C.POINTER(C.c_float), C.c_int32, C.c_float, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_int32)]

    def build(self, pts, idx):
        """The tree nrays_scene_create's host builder gives the mesh: one box per triangle (pre-splitting leaves the rungs alone: no box is
        emptier than the average box is large), NR_MAX_LEAF, the default primitive cost.  Same keys as the dump of nrays_debug_blas_build."""
        tri = np.asarray(pts, F32)[np.asarray(idx, np.int64)]
        return self.build_boxes(np.concatenate([tri.min(axis=1), tri.max(axis=1)], axis=1), max_leaf())

    def build_boxes(self, boxes, leaf):
        boxes = np.ascontiguousarray(boxes, F32)
        n = len(boxes)
        nodes = np.zeros((2 * n + 4, 32), F32)
        order = np.zeros(n, np.uint32)
        info = (C.c_int32 * 2)()
        k = self.lib.bvh_shim_build(n, boxes.ctypes.data_as(C.POINTER(C.c_float)), leaf, 0.0, len(nodes), nodes.ctypes.data_as(C.POINTER(C.c_float)),
                                    order.ctypes.data_as(C.POINTER(C.c_uint32)), info)
        assert k <= len(nodes)
        return dict(nodes=nodes[:k].copy(), tri=order, root=int(info[0]), depth=int(info[1]))


# ---------------------------------------------------------------- the ladder -------------------------------------------------------------------

PLAIN_YZ = ((-1.0, -1.0), (3.0, 2.0), (2.0, 3.0))    # a kite along the square's diagonal: 3.5 of the square's 16
FLIPPED_YZ = ((-1.0, 3.0), (3.0, 0.0), (2.0, -1.0))  # the same along the other diagonal, wound the other way


def ladder(ratio=2.0, kmin=-60, kmax=60, sign=-1.0, period=4, phase=1):
    """(points (3 n, 3) f32, indices (n, 3), x of each rung, flipped mask).  Rung j = k - kmin is flipped when j % period == phase."""
    ks = np.arange(kmin, kmax + 1)
    x = sign * np.float64(ratio) ** ks
    assert np.array_equal(x.astype(F32).astype(np.float64), x) and np.abs(np.log2(np.abs(x))).max() <= 60
    flipped = np.arange(len(ks)) % period == phase
    pts = np.zeros((len(ks), 3, 3))
    pts[:, :, 0] = x[:, None]
    pts[:, :, 1:] = np.where(flipped[:, None, None], np.array(FLIPPED_YZ), np.array(PLAIN_YZ))
    return pts.reshape(-1, 3).astype(F32), np.arange(3 * len(ks), dtype=np.uint32).reshape(-1, 3), x, flipped


def ladder_uvs(n):
    """Per-vertex uvs (f32-exact): rung j maps to the strip u in [j / 128, (j + 1) / 128] of a texture — which rung a ray met shows in its uv."""
    j = np.arange(n, dtype=np.float64)[:, None]
    uv = np.stack([np.concatenate([j, j + 1, j], axis=1) / 128.0, np.tile(np.array([0.0, 0.0, 1.0]), (n, 1))], axis=2)
    return uv.reshape(-1, 2).astype(F32)


PLACEMENTS = {
    "world": nr.Isometry3.identity,                                                      # the kFeatNoXform kernels
    "translated": lambda: nr.Isometry3((0.0, -1.25, 2.0), (0.0, 0.0, 0.0)),              # identity rotation: co = o - t
    # about x: the rung's plane turns, and x — up to 2^60 — never mixes into y and z, where the rungs are 4 wide (the matrix has exact zeros there);
    # no translation along x: a world coordinate t + x cannot hold the rungs next to the origin (x down to 2^-60) apart
    "rotated": lambda: nr.Isometry3((0.0, -1.25, 2.0), (0.7, 0.0, 0.0)),
    "rotated_b": lambda: nr.Isometry3((0.0, 14.0, -1.0), (-1.9, 0.0, 0.0)),
}


def rotation(iso):
    return np.array(math3d.rotation_from_axis_angle(iso.axis_angle), np.float64).reshape(3, 3), np.array(iso.translation, np.float64)


def to_world(iso, o, d):
    R, T = rotation(iso)
    return np.ascontiguousarray(o @ R.T + T), np.ascontiguousarray(d @ R.T)


def to_local(iso, o, d):
    """As traverse() moves a ray into an instance: inv_rot(o - t), inv_rot(d)."""
    R, T = rotation(iso)
    return (o - T) @ R, d @ R


CLASS_OF = (0, 2, 0, 3, 0, 2, 1, 3)   # three near, two oblique, two between, one far in every eight consecutive rays


def ray_classes(n=N_RAYS):
    """The pattern moves on by three with every 256 rays: the lanes with one thread index in neighbouring workgroups walk different ways, so
    that a stack slot read from another workgroup's column is not by chance the slot's own value."""
    i = np.arange(n)
    return np.array(CLASS_OF)[(i + 3 * (i // 256)) % len(CLASS_OF)]


def ladder_rays(x, flipped, seed, n=N_RAYS, spread=(-1.25, 3.25)):
    """Rays in the ladder's own frame, the four classes interleaved ray by ray.  Lateral positions are uniform over a 4.5 x 4.5 square around
    the rung's 4 x 4 one, so a share of every class misses the root box and stays at two slots.
    near: from just in front of the first rung (at half its distance from the origin, so that f32 tells the entry distances of all rungs
    apart as f64 does), along the ladder; far: from beyond the last rung, back along it (the nearest child is the short one at every level:
    a shallow class); oblique: from either end, aimed at a random point of a random rung or of its square; between: from the middle of a
    gap, three in four towards the origin."""
    rng = np.random.default_rng(seed)
    lo, hi = np.abs(x).min(), np.abs(x).max()
    s = np.sign(x[0])
    o = np.zeros((n, 3)); d = np.zeros((n, 3))
    o[:, 1:] = rng.uniform(spread[0], spread[1], (n, 2))
    cls = ray_classes(n)
    m = cls == 0
    o[m, 0] = -s * 0.5 * lo; d[m, 0] = s
    m = cls == 1
    o[m, 0] = s * 1.5 * hi; d[m, 0] = -s
    m = cls == 2
    j = rng.integers(0, len(x), n)
    a, b = rng.random(n), rng.random(n)
    fold = a + b > 1
    a, b = np.where(fold, 1 - a, a), np.where(fold, 1 - b, b)              # uniform over the triangle
    corners = np.where(flipped[j][:, None, None], np.array(FLIPPED_YZ), np.array(PLAIN_YZ))
    on_rung = corners[:, 0] + a[:, None] * (corners[:, 1] - corners[:, 0]) + b[:, None] * (corners[:, 2] - corners[:, 0])
    tyz = np.where((rng.random(n) < 0.5)[:, None], on_rung, rng.uniform(-1.0, 3.0, (n, 2)))
    o[m, 0] = np.where(rng.random(n) < 0.3, s * 1.5 * hi, -s * 0.5 * lo)[m]
    tgt = np.concatenate([x[j][:, None], tyz], axis=1)
    d[m] = (tgt - o)[m]
    m = cls == 3
    jj = rng.integers(0, len(x) - 1, n)
    o[m, 0] = (0.5 * (x[jj] + x[jj + 1]))[m]
    d[m, 0] = np.where(rng.random(n) < 0.75, -s, s)[m]
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


# ---------------------------------------------------------------- the stack simulator ---------------------------------------------------------

def _planes(nodes):
    """(mn (N, 4, 3), mx (N, 4, 3), child refs (N, 4)) of a dumped tree (device_types.h: BvhNode — lower planes in slots 0 / 4 / 3, upper in 1 / 6 / 7)."""
    q = np.asarray(nodes, F32).reshape(-1, 8, 4)
    mn = np.stack([q[:, 0], q[:, 4], q[:, 3]], axis=2).astype(np.float64)
    mx = np.stack([q[:, 1], q[:, 6], q[:, 7]], axis=2).astype(np.float64)
    return mn, mx, q[:, 2].view(np.int32).astype(np.int64)


def _slab(mn, mx, o, d, best):
    """Exact f64 slabs of m rays against their (m, 4, 3) boxes (ncollide's ray / AABB rule, a zero component included): the entry distances
    (m, 4), +inf where the ray cannot enter the box before `best`."""
    o, d = o[:, None, :], d[:, None, :]
    with np.errstate(all="ignore"):
        t0 = (mn - o) / d; t1 = (mx - o) / d
        inside = (o >= mn) & (o <= mx)
        near = np.where(d != 0, np.minimum(t0, t1), np.where(inside, -np.inf, np.inf))
        farr = np.where(d != 0, np.maximum(t0, t1), np.where(inside, np.inf, -np.inf))
    tn = np.maximum(near.max(axis=2), 0.0)
    tf = np.minimum(farr.min(axis=2), best[:, None])
    return np.where(tn <= tf, tn, np.inf)


def _tri_toi(a, b, c, o, d):
    """ncollide's ray / triangle test in f64, both faces, row by row: the distance, +inf for a miss."""
    ab, ac = b - a, c - a
    n = np.cross(ab, ac)
    dn = (n * d).sum(axis=1)
    ap = o - a
    t = (ap * n).sum(axis=1)
    e = -np.cross(d, ap)
    sgn = np.where(t < 0, -1.0, 1.0)
    v = sgn * (ac * e).sum(axis=1)
    w = -sgn * (ab * e).sum(axis=1)
    dabs = np.abs(dn)
    ok = (dn != 0) & ~((t < 0) & (dn < 0)) & ~((t > 0) & (dn > 0)) & (v >= 0) & (v <= dabs) & (w >= 0) & (v + w <= dabs)
    with np.errstate(all="ignore"):
        return np.where(ok, np.abs(t) / dabs, np.inf)


def simulate(tree, tris, o, d, shadow=False, any_hit=False, limit=np.inf, base=2, key32=False, per_leaf=False):
    """The largest number of stack slots each ray holds while traverse() walks `tree` (a dict as BuildShim.build returns: nodes, tri, root).
    `base` = the slots in use when the walk starts: the bottom marker and the sentinel.  tris: (T, 3, 3) f64 vertices by triangle index.
    shadow=False: the closest-hit order — the four children sorted by entry distance with the 5-comparator network of traverse() (a tie
    keeps the slot order), the farthest pushed first, the nearest visited next; a popped leaf is tested without a new box test.
    shadow=True: the last child the ray enters is visited next, the others are pushed in slot order; `limit` bounds the distance from the
    start; any_hit=True ends a ray's walk at its first hit within the limit (an opaque node), otherwise the closest hit is kept.
    per_leaf: every leaf is a node of its own (a TLAS over one-triangle meshes, each transparent to shadow rays): its hit is collected when
    its sentinel comes up and the distance bound starts again at `limit`, so a hit never culls another leaf.
    key32: the sort compares the entry distances rounded to f32, as the device's keys are — distances that differ in f64 only then tie.
    All rays step together, each with a stack of its own.  Returns (heights (n,), the triangle of the result or -1)."""
    mn, mx, ch = _planes(tree["nodes"])
    order = np.asarray(tree["tri"], np.int64)
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    n = len(o)
    cap = 4 * len(ch) + 8
    stack = np.full((n, cap), EMPTY, np.int64)
    sp = np.zeros(n, np.int64)
    high = np.full(n, base, np.int64)
    limit = np.array(np.broadcast_to(np.asarray(limit, np.float64), (n,)))
    best = limit.copy() if shadow else np.full(n, np.inf)
    bprim = np.full(n, -1, np.int64)
    cur = np.full(n, tree["root"], np.int64)

    def push(rows, vals):
        stack[rows, sp[rows]] = vals
        sp[rows] += 1

    def pop(rows):
        empty = sp[rows] == 0
        sp[rows] -= np.where(empty, 0, 1)
        return np.where(empty, EMPTY, stack[rows, sp[rows]])

    while True:
        at_node = np.flatnonzero(cur >= 0)
        if len(at_node):
            r = at_node
            c = ch[cur[r]].copy()
            k = _slab(mn[cur[r]], mx[cur[r]], o[r], d[r], best[r])
            k = np.where(c == EMPTY, np.inf, k)       # an absent child's box is inverted: no ray enters it, whatever min / max make of its slabs
            if not shadow:
                ks = k.astype(F32).astype(np.float64) if key32 else k.copy()
                ks[np.isinf(k)] = np.inf
                for a, b in ((0, 1), (2, 3), (0, 2), (1, 3), (1, 2)):
                    sw = ks[:, b] < ks[:, a]
                    ks[sw, a], ks[sw, b] = ks[sw, b], ks[sw, a]
                    c[sw, a], c[sw, b] = c[sw, b], c[sw, a]
                for s in (3, 2, 1):
                    m = ks[:, s] < np.inf
                    push(r[m], c[m, s])
                high[r] = np.maximum(high[r], base + sp[r])
                go = ks[:, 0] < np.inf
                cur[r[go]] = c[go, 0]
                cur[r[~go]] = pop(r[~go])
            else:
                h = k < np.inf
                last = np.where(h.any(axis=1), 3 - np.argmax(h[:, ::-1], axis=1), -1)
                for s in range(3):
                    m = h[:, s] & (s < last)
                    push(r[m], c[m, s])
                high[r] = np.maximum(high[r], base + sp[r])
                go = last >= 0
                cur[r[go]] = c[go, last[go]]
                cur[r[~go]] = pop(r[~go])
            continue
        r = np.flatnonzero(cur != EMPTY)
        if not len(r):
            break
        v = ~cur[r]
        first, count = v >> 3, (v & 7) + 1
        nxt = pop(r)
        ended = np.zeros(len(r), bool)
        for j in range(8):
            m = (j < count) & ~ended
            if not m.any():
                continue
            t = order[np.where(m, first + j, 0)]
            toi = np.where(m, _tri_toi(tris[t, 0], tris[t, 1], tris[t, 2], o[r], d[r]), np.inf)
            if shadow and any_hit:
                blk = np.isfinite(toi) & (toi <= limit[r])
                bprim[r[blk]] = t[blk]
                ended |= blk
            else:
                better = (toi < best[r]) | ((toi == best[r]) & np.isfinite(toi) & ((bprim[r] < 0) | (t < bprim[r])))
                if per_leaf:
                    better = np.isfinite(toi) & (toi <= limit[r]) & (bprim[r] < 0)
                else:
                    best[r[better]] = toi[better]
                bprim[r[better]] = t[better]
        cur[r] = np.where(ended, EMPTY, nxt)
    return high, bprim


# ---------------------------------------------------------------- the scenes ------------------------------------------------------------------

LIGHTS = lambda: [nr.Light((0.0, 10.0, 0.0), 0.0, 1, (1, 1, 1))]  # noqa: E731


def _mesh_node(pts, idx, iso, material=None, alpha=1.0, refl=0.0, refr=1.0, uvs=None):
    return nr.SceneNode(material or nr.NormalMaterial(), refl, 0.0, alpha, refr, iso, nr.TriMesh(pts, idx, uvs))


def _ladder_node(iso, **kw):
    pts, idx, _, _ = ladder()
    return _mesh_node(pts, idx, iso, uvs=ladder_uvs(len(idx)), **kw)


def _small_meshes(count, seed):
    """Two-triangle quads beside the two ladders' corridors (lateral positions outside both [-2, 4]^2 squares, in front of the near ends): their
    instances give the TLAS levels, and the boxes of its inner nodes span the corridors, so a ray that enters a ladder has TLAS children deferred."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        y = [-6.0, 7.5, 22.0][i % 3] + rng.integers(-4, 5) * 0.125
        c = np.array([-rng.integers(1, 160) * 0.25, y, [-7.0, 8.0][(i // 3) % 2] + rng.integers(-4, 5) * 0.125])
        q = np.array([[0, 0, 0], [0, 0.5, 0], [0, 0, 0.5], [0, 0.5, 0.5]], np.float64) + c
        out.append(_mesh_node(q.astype(F32), np.array([[0, 1, 2], [1, 3, 2]], np.uint32), nr.Isometry3.identity()))
    return out


SCENES = ("a_world", "a_translated", "a_rotated", "b_alpha", "c_tlas", "d_planes", "e_hair", "f_bounce")
# (g) is no ladder scene in the sense of the conditions: its shadow TLAS keeps the long child in slot 0, which the shadow order visits last, so a
# lane passes the LDS part by a few slots only (tests/test_stack_spill.py states what it does reach).  It is here for what its answer depends on.
ALL_SCENES = SCENES + ("g_rungs",)


def scene_nodes(name):
    """(nodes of the scene, [(index of a ladder node, its isometry)]).  Every ladder is the same mesh: one tree."""
    pts, idx, _, _ = ladder()
    if name.startswith("a_"):
        iso = PLACEMENTS[name[2:]]
        return [_ladder_node(iso())], [(0, iso())]
    if name == "b_alpha":     # transparent to shadow rays: every hit of the node is collected under the sentinel, nothing ends the walk early
        iso = PLACEMENTS["rotated"]
        mat = nr.PhongMaterial((0.5, 0.25, 0.75), (0.5, 0.5, 0.5), (0.25, 0.25, 0.25), None, None, 20.0)
        return [_ladder_node(iso(), material=mat, alpha=0.5)], [(0, iso())]
    if name == "c_tlas":
        a, b = PLACEMENTS["rotated"], PLACEMENTS["rotated_b"]
        return [_ladder_node(a())] + _small_meshes(15, 5) + [_ladder_node(b())] + _small_meshes(15, 6), [(0, a()), (16, b())]
    if name == "d_planes":    # analytic shapes beside the mesh: kFeatAll, the plane pseudo-leaves lie at the bottom of the stack
        iso = PLACEMENTS["translated"]
        mat = nr.PhongMaterial((0.5, 0.5, 0.5), (0.5, 0.5, 0.5), (0, 0, 0), None, None, 20.0)
        planes = [nr.SceneNode(mat, 0.0, 0.0, 1.0, 1.0, nr.Isometry3((0.0, -9.0, 0.0), (0.0, 0.0, 0.0)), nr.Plane((0.0, 1.0, 0.0))),
                  nr.SceneNode(mat, 0.0, 0.0, 1.0, 1.0, nr.Isometry3((0.0, 0.0, -11.0), (0.0, 0.0, 0.0)), nr.Plane((0.0, 0.0, 1.0))),
                  nr.SceneNode(mat, 0.0, 0.0, 1.0, 1.0, nr.Isometry3((-3.0, 9.0, 1.0), (0.0, 0.0, 0.0)), nr.Ball(1.5))]
        return planes + [_ladder_node(iso())], [(3, iso())]
    if name == "e_hair":      # a hair-like mesh beside it: the scene is `incoherent`, node phases end by quorum and parked lanes push their node
        from tools import standins
        iso = PLACEMENTS["world"]
        hp, hi, _ = standins.hairball_geometry(strands=4, sides=3, segments=11)
        hair = _mesh_node((hp * 0.25).astype(F32), hi, nr.Isometry3((-2.0, 9.0, 1.0), (0.0, 0.0, 0.0)))
        return [_ladder_node(iso()), hair], [(0, iso())]
    if name == "f_bounce":    # reflects and refracts: k_bounce's queries at max_depth 2
        iso = PLACEMENTS["translated"]
        mat = nr.PhongMaterial((0.25, 0.5, 0.25), (0.5, 0.5, 0.5), (0.25, 0.25, 0.25), None, None, 20.0)
        return [_ladder_node(iso(), material=mat, alpha=0.5, refl=0.25, refr=1.125)], [(0, iso())]
    if name == "g_rungs":     # every rung a node of its own, transparent to shadow rays: the shadow TLAS is the chain, a BLAS's sentinel lies on top
        nodes = []            # of it, and a shadow ray's filter is the product over EVERY rung it crosses — powers of two, exact in any order
        for j in range(len(idx)):
            ka = tuple(0.5 if ((j % 7 + 1) >> c) & 1 else 1.0 for c in range(3))
            nodes.append(_mesh_node(pts[3 * j:3 * j + 3], idx[:1], nr.Isometry3.identity(), nr.PhongMaterial(ka, (0, 0, 0), (0, 0, 0), None, None, 20.0), alpha=0.0))
        return nodes, []
    raise KeyError(name)


def world_box_f32(lo, hi, terms=None):
    """scene_build.cpp's world_box for an unrotated box with the f64 faces lo, hi (n x 3): each face rounded outward to f32 and moved one step further, or moved
    outward by 2^-48 x `terms` (per axis |centre| + |translation| + half extent) and rounded outward, whichever is further out.  terms None: local space is world
    space, every sum is exact, no margin.  Returns n x 6 f32."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)

    def down(v):
        f = v.astype(F32)
        return np.where(f.astype(np.float64) > v, np.nextafter(f, F32(-np.inf)), f).astype(F32)
    m = 0.0 if terms is None else 2.0 ** -48 * np.asarray(terms, np.float64)
    mn = np.minimum(np.nextafter(down(lo), F32(-np.inf)), down(lo - m))
    mx = np.maximum(np.nextafter(-down(-hi), F32(np.inf)), -down(-(hi + m)))
    return np.concatenate([mn, mx], axis=1).astype(F32)


def rungs_tree(shim):
    """The shadow TLAS of scene (g) as scene_build.cpp builds it: one instance per rung, its box the triangle's widened by an f32 ulp (world_box: the rungs are
    untransformed), one instance per leaf."""
    pts, idx, _, _ = ladder()
    tri = pts[idx.astype(np.int64)]
    return shim.build_boxes(world_box_f32(tri.min(axis=1), tri.max(axis=1)), 1)


def trees(shim):
    pts, idx, _, _ = ladder()
    return dict(ladder=shim.build(pts, idx), rungs=rungs_tree(shim))


def make_scene(name):
    nodes, _ = scene_nodes(name)
    return nr.Scene(nodes, LIGHTS(), BACKGROUND)


def scene_rays(name):
    """World rays of the scene: the ladder's rays moved by its isometry; with two ladders, waves alternate between them in halves (32 rays each)."""
    _, ladders = scene_nodes(name)
    _, _, x, flipped = ladder()
    o, d = ladder_rays(x, flipped, 700 + ALL_SCENES.index(name))
    if not ladders:
        return o, d, np.zeros(len(o), np.int64)
    which = (np.arange(len(o)) // 32) % len(ladders)
    wo, wd = np.zeros_like(o), np.zeros_like(d)
    for k, (_, iso) in enumerate(ladders):
        a, b = to_world(iso, o, d)
        wo[which == k], wd[which == k] = a[which == k], b[which == k]
    return np.ascontiguousarray(wo), np.ascontiguousarray(wd), which


def reach(tr, name, shadow, key32=False):
    """simulate() on the scene's rays, each in the frame of the ladder it was made for; tr = trees().  Shadow order: unbounded, and ending at
    the first hit unless the ladder is transparent to shadow rays.  Scene (g): the closest-hit TLAS holds one instance (nodes of one isometry
    share a BLAS — the ladder's tree again), the shadow TLAS one per rung."""
    _, ladders = scene_nodes(name)
    pts, idx, _, _ = ladder()
    tris = pts.astype(np.float64)[idx.astype(np.int64)]
    o, d, which = scene_rays(name)
    if name == "g_rungs":
        if shadow:
            return simulate(tr["rungs"], tris, o, d, shadow=True, per_leaf=True)[0]
        return simulate(tr["ladder"], tris, o, d, key32=key32)[0]
    heights = np.zeros(len(o), np.int64)
    for k, (_, iso) in enumerate(ladders):
        lo, ld = to_local(iso, o, d)
        m = which == k
        heights[m] = simulate(tr["ladder"], tris, lo[m], ld[m], shadow=shadow, any_hit=name not in ("b_alpha", "f_bounce"), key32=key32)[0]
    return heights


# ---------------------------------------------------------------- the brute force, once per scene ---------------------------------------------

_expected = {}


def expected(name):
    """The oracle's brute force over all triangles (no BVT, tie rule D-2) on the scene's rays, computed once and left unchanged: (origins, dirs,
    hit, records (n, 8) as oracle.cast returns them, the triangle's index in its ladder or -1).  The triangle comes from a second scene in which
    every rung is a node of its own — the brute force then names the rung as the node; -1 where that scene's mesh gates differ (knife edges)
    or the hit is not on a ladder."""
    if name not in _expected:
        import oracle
        nodes, ladders = scene_nodes(name)
        pts, idx, _, _ = ladder()
        o, d, _ = scene_rays(name)
        hit, out = oracle.cast(nr.Scene(nodes, LIGHTS(), BACKGROUND).descriptor, o, d, bruteforce=True)
        rungs, owner = [], []
        for k, (ni, iso) in enumerate(ladders):
            for t in range(len(idx)):
                rungs.append(_mesh_node(pts[3 * t:3 * t + 3], idx[:1], iso, uvs=ladder_uvs(len(idx))[3 * t:3 * t + 3]))
                owner.append((ni, t))
        others = [nd for i, nd in enumerate(nodes) if i not in [ni for ni, _ in ladders]]
        prim = np.full(len(o), -1, np.int64)
        if not ladders:
            prim[hit] = out[hit, 7].astype(np.int64)           # scene (g): the rung is the node
        else:
            thit, tout = oracle.cast(nr.Scene(others + rungs, LIGHTS(), BACKGROUND).descriptor, o, d, bruteforce=True)
            tn = tout[:, 7].astype(np.int64) - len(others)
            ok = hit & thit & (tout[:, 0] == out[:, 0]) & (tn >= 0)
            own = np.array(owner, np.int64)
            ok[ok] &= own[tn[ok], 0] == out[ok, 7].astype(np.int64)
            prim[ok] = own[tn[ok], 1]
        for a in (o, d, hit, out, prim):
            a.setflags(write=False)
        _expected[name] = (o, d, hit, out, prim)
    return _expected[name]


# ---------------------------------------------------------------- the record of the reach ----------------------------------------------------

def reach_shares(heights):
    """What profiles/stack_spill_reach.json holds per scene and order."""
    L = lds_stack()
    blocks = [heights[i:i + 64] for i in range(0, len(heights), 64)]
    cls = ray_classes(len(heights))
    return dict(rays_beyond_lds=round(float((heights > L).mean()), 4), rays_12_beyond=round(float((heights >= L + 12).mean()), 4),
                rays_at_most_4=round(float((heights <= 4).mean()), 4), blocks_beyond_lds=round(float(np.mean([(b > L).any() for b in blocks])), 4),
                blocks_mixed=round(float(np.mean([(b >= L + 12).any() and (b <= L - 4).any() for b in blocks])), 4), max_slots=int(heights.max()),
                rays_by_class={CLASSES[c]: [int(((heights[cls == c] >= lo) & (heights[cls == c] <= hi)).sum()) for lo, hi in slot_bins()] for c in range(4)})


def slot_bins():
    """The bins of the record's rays_by_class: at most 4 slots, up to kLdsStack - 4, up to kLdsStack, up to kLdsStack + 11, more."""
    L = lds_stack()
    return [(0, 4), (5, L - 4), (L - 3, L), (L + 1, L + 11), (L + 12, 10 ** 6)]


def reach_record(shim):
    pts, idx, x, flipped = ladder()
    tr = trees(shim)
    tree = tr["ladder"]
    rec = dict(lds_stack=lds_stack(), rungs=len(x), flipped=int(flipped.sum()), rays=N_RAYS, tree_nodes=len(tree["nodes"]), tree_depth=tree["depth"],
               need=need(tree["depth"]), rungs_tlas_nodes=len(tr["rungs"]["nodes"]), rungs_tlas_depth=tr["rungs"]["depth"], note="simulated slots in use per ray (tests/stack_cases.py: simulate, exact f64 box tests, one mesh; bottom marker and sentinel included)",
               slot_bins=[[lo, min(hi, 999)] for lo, hi in slot_bins()], scenes={})
    for name in ALL_SCENES:
        rec["scenes"][name] = {"closest": reach_shares(reach(tr, name, False)), "shadow": reach_shares(reach(tr, name, True))}
    return rec


if __name__ == "__main__":      # python -m tests.stack_cases: rewrites the record
    import json
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        record = reach_record(BuildShim(tmp))
    with open(os.path.join(ROOT, "profiles", "stack_spill_reach.json"), "w") as f:
        json.dump(record, f, indent=1, sort_keys=True)
        f.write("\n")


# ---------------------------------------------------------------- the composite calls ---------------------------------------------------------

def composite_case(name, n=516):
    """Points just in front of the (first) ladder's first rung with the normal along the ladder, and six unit directions about it — the normal
    itself, two a nanoradian or two off it (they leave the rungs' corridor some 2^31 units down, inside the chain's first levels),
    one well off it, two pointing away from the ladder (they meet nothing and stay at two slots) — for occlusion_points, gather_points, gather_sh_points and gather_maps_points with bias 0.  Returns (points, normals,
    directions, odd keys); the rays are nr.occlusion_rays(points, normals, directions, None, 0.0, keys)."""
    _, ladders = scene_nodes(name)
    _, _, x, _ = ladder()
    iso = ladders[0][1]
    rng = np.random.default_rng(900 + ALL_SCENES.index(name))
    s = np.sign(x[0])
    p = np.zeros((n, 3)); p[:, 0] = -s * 0.5 * np.abs(x).min(); p[:, 1:] = rng.uniform(-1.25, 3.25, (n, 2))
    nm = np.zeros((n, 3)); nm[:, 0] = s
    wp, wn = to_world(iso, p, nm)
    polar = np.array([0.0, 1e-9, 2e-9, 0.5, 2.0, 2.6]); azimuth = np.array([0.0, 0.7, 2.9, 4.1, 5.3, 1.9])
    L = np.stack([np.sin(polar) * np.cos(azimuth), np.sin(polar) * np.sin(azimuth), np.cos(polar)], axis=1)
    keys = rng.integers(0, 2 ** 63, size=n, dtype=np.int64).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    return np.ascontiguousarray(wp), np.ascontiguousarray(wn), L, keys


def composite_reach(tr, name, shadow, key32=False):
    """simulate() on the rays of composite_case, in the order (point, direction)."""
    _, ladders = scene_nodes(name)
    pts, idx, _, _ = ladder()
    p, nm, L, keys = composite_case(name)
    ro, rd = nr.occlusion_rays(p, nm, L, None, 0.0, keys)
    lo, ld = to_local(ladders[0][1], ro.reshape(-1, 3), rd.reshape(-1, 3))
    return simulate(tr["ladder"], pts.astype(np.float64)[idx.astype(np.int64)], lo, ld, shadow=shadow, any_hit=name not in ("b_alpha", "f_bounce"), key32=key32)[0]


def phong_scene():
    """An opaque Phong ladder under the rotated placement, its light 2^-42 in front of the first rung beside both kites (FRAME_EYE):
    Material::compute's shadow rays run from the hit points back along the ladder (shade_points, and trace_rays as its yardstick)."""
    iso = PLACEMENTS["rotated"]()
    mat = nr.PhongMaterial((0.25, 0.25, 0.5), (0.5, 0.75, 0.5), (0.5, 0.5, 0.5), None, None, 20.0)
    light, _ = to_world(iso, np.array([FRAME_EYE]), np.zeros((1, 3)))
    return nr.Scene([_ladder_node(iso, material=mat)], [nr.Light(tuple(light[0]), 0.0, 1, (1, 1, 1))], BACKGROUND)


# ---------------------------------------------------------------- a ladder without meshes: the pipelined frames --------------------------------

PLATES_CAMERA = dict(eye=(9.0, 4.25, 0.75), at=(-100.0, 4.0, 1.0), fovy=70.0)
PLATES_SIZE = (128, 128)
PLATES_ALPHA = 2.0 ** -6           # nearly clear: a shadow ray's filter loses 1 / 64 per plate crossed, so it tells how many it crossed
# a light far down each ladder, in a gap between two plates: the shadow rays of a hit on a first plate cross some eighty plates, every one a
# transparent node of the shadow TLAS, and their filter is the product over all of them
PLATES_LIGHTS = ((-1.5 * 2.0 ** 20, 1.5, 1.25), (-1.5 * 2.0 ** 22, 7.5, 0.75))
PLATES_OFFSETS = (0.0, 6.0)      # two ladders side by side in y: lanes in one's square hold other node refs than lanes in the other's


def _plates():
    ks = np.arange(-60, 61)
    x = np.tile(-2.0 ** ks, len(PLATES_OFFSETS))
    return x, np.abs(x) / 8.0, np.repeat(np.array(PLATES_OFFSETS), len(ks)) + 1.0


def plates_scene():
    """Only scenes without meshes are pipelined (frame_path.hip: pipeline_prepare), and only while every corner of the scene's box lies in front
    of the eye and its picture fills less than half of the frame — so the eye cannot stand next to the chain's deep end, where f32 tells the
    entry distances apart (frame_camera).  From nine units away the PRIMARY rays do not go deep on the device: the plates nearer to x = 0 than
    9 x 2^-21 get one sort key.  What goes deep are the rays that go on: two ladders of 121 cuboid plates over the rungs' square, an eighth of
    their distance thick, every one nearly clear and not refracting (alpha 2^-6, index 1); a pixel inside either square meets the first
    plate, and its ray goes on from that plate's back, 2^-60 from the chain's deep end, straight down the ladder (max_depth >= 1).  The
    shadow rays of those hits run down the ladders to PLATES_LIGHTS through some eighty transparent nodes each."""
    x, h, y = _plates()
    mats = [nr.NormalMaterial(), nr.PhongMaterial((1.0, 1.0, 1.0), (0.5, 0.5, 0.75), (0.5, 0.5, 0.5), None, None, 20.0)]
    nodes = [nr.SceneNode(mats[j & 1], 0.0, 0.0, PLATES_ALPHA, 1.0, nr.Isometry3((float(x[j]), float(y[j]), 1.0), (0.0, 0.0, 0.0)), nr.Cuboid((float(h[j]), 2.0, 2.0)))
             for j in range(len(x))]
    return nr.Scene(nodes, [nr.Light(pos, 0.0, 1, (1, 1, 1)) for pos in PLATES_LIGHTS], BACKGROUND), dict(PLATES_CAMERA)


def plates_cameras(n):
    """n pairwise different cameras for consecutive frames: the eye moves by a fraction of a pixel per frame, the window of blocks that can see the
    scene stays what it is."""
    e = PLATES_CAMERA["eye"]
    return [dict(PLATES_CAMERA, eye=(e[0] + k * 2e-3, e[1] + k * 6e-4, e[2])) for k in range(n)]


def plates_reach(shim, key32=True, cam=None):
    """simulate() in closest-hit order, sort keys rounded to f32, over the TLAS scene_build.cpp builds (leaves of one, the boxes of world_box: the
    plate's, an f32 ulp wider (world_box_f32); a plate stands in as a triangle over its front face): the primary rays of the plates' frame, and for those that
    meet a plate the ray that goes on from the plate's back in the same direction.  Returns (tree, heights of the primary rays, heights of the
    rays that go on (0 where there is none), the plate the primary ray meets or -1)."""
    x, h, y = _plates()
    mn = np.stack([x - h, y - 2.0, np.full_like(x, -1.0)], axis=1)
    mx = np.stack([x + h, y + 2.0, np.full_like(x, 3.0)], axis=1)
    terms = np.stack([np.abs(x) + h, np.abs(y) + 2.0, np.full_like(x, 3.0)], axis=1)   # (no face of a plate lies near a coordinate plane: the margin moves none of them)
    tree = shim.build_boxes(world_box_f32(mn, mx, terms), 1)
    tris = np.zeros((len(x), 3, 3))
    tris[:, :, 0] = (x + h)[:, None]
    tris[:, :, 1] = (y - 2.0)[:, None] + np.array([0.0, 8.0, 0.0])
    tris[:, :, 2] = np.array([-1.0, -1.0, 7.0])
    cam = cam or PLATES_CAMERA
    proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], *PLATES_SIZE)
    o, d = nr.camera_rays(PLATES_SIZE, cam["eye"], proj)[:2]
    o, d = np.asarray(o, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3)
    heights, found = simulate(tree, tris, o, d, key32=key32)
    m = found >= 0
    back = (x - h)[found[m]]
    t = (back - o[m, 0]) / d[m, 0]
    on = o[m] + d[m] * t[:, None]
    on[:, 0] = np.nextafter(back, -np.inf)                     # just behind the plate
    onward = np.zeros(len(o), np.int64)
    onward[m] = simulate(tree, tris, on, d[m], key32=key32)[0]
    return tree, heights, onward, found


def plates_shadow_reach(shim):
    """simulate() in shadow order (every plate a transparent node: nothing ends the walk, no hit culls another) on the shadow rays of the plates'
    frame: from the points where the primary rays meet a plate to each of PLATES_LIGHTS.  Returns heights (hits, lights)."""
    tree, _, _, found = plates_reach(shim)
    x, h, y = _plates()
    tris = np.zeros((len(x), 3, 3))
    tris[:, :, 0] = (x + h)[:, None]
    tris[:, :, 1] = (y - 2.0)[:, None] + np.array([0.0, 8.0, 0.0])
    tris[:, :, 2] = np.array([-1.0, -1.0, 7.0])
    proj = math3d.inverse_projection(PLATES_CAMERA["eye"], PLATES_CAMERA["at"], PLATES_CAMERA["fovy"], *PLATES_SIZE)
    o, d = nr.camera_rays(PLATES_SIZE, PLATES_CAMERA["eye"], proj)[:2]
    o, d = np.asarray(o, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3)
    m = found >= 0
    p = o[m] + d[m] * (((x + h)[found[m]] - o[m, 0]) / d[m, 0])[:, None]
    p[:, 0] = np.nextafter((x + h)[found[m]], np.inf)            # just in front of the plate
    return np.stack([simulate(tree, tris, p, np.array(light) - p, shadow=True, per_leaf=True, limit=1.0)[0] for light in PLATES_LIGHTS], axis=1)


# ---------------------------------------------------------------- the frames --------------------------------------------------------------------

FRAME_SIZE = (64, 64)
FRAME_EYE = (2.0 ** -42, 1.0, -0.5)      # in the ladder's frame: 2^-42 in front of the first rung, beside both kites
FRAME_LOOK = (-0.3, 1.0, 0.2)            # across the ladder and a little into it
FRAME_EYE_BOUNCE = (2.0 ** -42, 1.0, 1.0)  # scene (f): in front of both kites — the first rungs are hit at once, and the rays that go on from there
                                           # (k_bounce's) start next to the first rung themselves


def frame_camera(name):
    """The camera of the 64 x 64 frames.  A camera some units in front of the ladder does NOT reach the HBM slots on the device: from a distance d
    the rungs nearer to x = 0 than d 2^-21 get one f32 sort key and the walk stops descending (23 slots at most from x = 6).  This eye stands
    2^-42 in front of the first rung (of the scene's first ladder), at a lateral position no kite covers, and looks across the ladder with a
    field of 90 degrees: the two thirds of the pixels whose rays point into x < 0 walk the chain to its end before they meet a rung further
    down, the others leave the scene at once."""
    _, ladders = scene_nodes(name)
    eye = FRAME_EYE_BOUNCE if name == "f_bounce" else FRAME_EYE
    pts = np.array([eye, tuple(eye[a] + FRAME_LOOK[a] for a in range(3))])
    w, _ = to_world(ladders[0][1], pts, pts)
    return dict(eye=tuple(w[0]), at=tuple(w[1]), fovy=90.0)


def frame_reach(tr, name, key32=True):
    """simulate() in closest-hit order on the primary rays of frame_camera(name), in the ladder's frame.  Returns (heights, the rung hit or -1,
    origins, directions) in image order."""
    _, ladders = scene_nodes(name)
    pts, idx, _, _ = ladder()
    cam = frame_camera(name)
    proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], *FRAME_SIZE)
    o, d = nr.camera_rays(FRAME_SIZE, cam["eye"], proj)[:2]
    lo, ld = to_local(ladders[0][1], np.asarray(o, np.float64).reshape(-1, 3), np.asarray(d, np.float64).reshape(-1, 3))
    h, f = simulate(tr["ladder"], pts.astype(np.float64)[idx.astype(np.int64)], lo, ld, key32=key32)
    return h, f, lo, ld


def shade_shadow_reach(tr):
    """simulate() in shadow order on the rays Material::compute casts in phong_scene(): from the closest hits of scene a_rotated's rays to the light."""
    iso = PLACEMENTS["rotated"]()
    pts, idx, _, _ = ladder()
    o, d, hit, out, _ = expected("a_rotated")
    lo, ld = to_local(iso, o[hit], d[hit])
    p = lo + ld * out[hit, 0][:, None]
    to_light = np.array(FRAME_EYE) - p
    return simulate(tr["ladder"], pts.astype(np.float64)[idx.astype(np.int64)], p, to_light, shadow=True, any_hit=True, limit=1.0)[0]
