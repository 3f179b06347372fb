"""Is a dumped bottom-level BVH a correct BVH?  A check that needs no second builder (tests/test_blas_cover.py: the host builder through
tests/blas_probe_shim.cpp; tests/test_blas_cover_gpu.py: the device builder through nrays_debug_blas_build).  numpy only.

A dump is `nodes` (n x 32 f32: the 128-byte 4-wide nodes of device_types.h — lower planes of the four children in slots 0 / 4 / 3 and upper
planes in slots 1 / 6 / 7 for x / y / z, child refs in slot 2), `tri` (the triangle behind every reference), `root`, `depth`, and the mesh.

1. SHAPE.  Every node is reached from the root exactly once; a child ref is kEmptyChild with the inverted box (+FLT_MAX / -FLT_MAX), an
   in-range node index, or a leaf ~((first << 3) | (count - 1)); the leaf ranges tile [0, num_refs) exactly once; every triangle occurs in
   `tri` (exactly once without pre-splitting); the reported depth is the depth the walk finds (root node = 0).
2. NESTING.  The boxes of a node's children lie inside the box the parent's slot holds for that node; the root's inside the mesh's f32
   bounds.  Exact comparison.
3. COVER.  R(L) = the intersection of the boxes on the path root -> leaf L.  For every triangle T and every sampled point p of T some leaf
   that references T must have p in R(L), faces included: a ray that hits T at p is inside every box of that path at p, so the
   conservative f32 slab test cannot cull T.

Samples are computed in float64 from the f32-exact vertices and clamped to T's own bounding box (a true point of T never leaves it):
  grid       barycentric weights k / 8 (corners and edge midpoints included);
  seam edge  for every region R(L) of T, every axis and both faces the plane at np.nextafter(face, outward) in float64 — ONE F64 STEP
             outside, not one f32 step — where it lies strictly inside T's extent on that axis, cut with T's edges; the axis coordinate is
             set to the plane exactly.  These points sit right behind every cut of the pre-splitting: a piece box rounded to nearest
             instead of outward loses exactly them, while the grid and a step of one f32 ulp would not notice;
  seam interior  the midpoint of the two edge points of such a plane (returned for the ray test, not checked here).

TOLERANCE.  A sample may lie outside every region of T by at most e(T) = 4 * 2^-53 * max |vertex coordinate of T|.  An edge sample's free
coordinates are a + (b - a) * t with t in [0, 1], three roundings in float64.  With M = max |coordinate of T| and u = 2^-53: (1) b - a of two
f32-exact numbers is exact unless their exponents lie more than 29 apart, and then |b - a| <= M (1 + 2^-29): error <= M u (1 + 2^-29), else 0;
(2) the product is at most |b - a| <= 2 M: error <= 2 M u, and <= M u (1 + 2^-29) in the inexact case of (1); (3) the sum lies between a and
b: error <= M u.  In all: <= 3 M u (1 + 2^-29) < 4 M u.  A grid sample (i a + j b + k c) / 8 has exact products (24 + 3 bits), two rounded
sums and an exact division: <= 2 M u.  The rounding of t itself (two more roundings) moves the point ALONG the edge, where it stays a point
of T up to the same order; e(T) does not count it, and need not: the builders round every box outward to f32, 2^29 times coarser than e(T),
so a correct tree shows slack 0 (a vertex on a face) and ANY positive slack is worth explaining.  The worst slack seen is reported."""
import numpy as np

EMPTY = -2**31
LO, HI, CHILD = (0, 4, 3), (1, 6, 7), 2
FLT_MAX = np.finfo(np.float32).max


# ---- the case meshes ------------------------------------------------------------------------------------------------------------

def _f32(a):
    return np.ascontiguousarray(np.asarray(a, np.float32))


def hair(strands, segments, seed=5):
    """Thin quads (two triangles each) along randomly wandering strands in a 2-unit cube: hair-like (every box is almost empty)."""
    rng = np.random.default_rng(seed)
    pts, idx = [], []
    for _ in range(strands):
        p = rng.uniform(-1.0, 1.0, 3)
        d = rng.normal(size=3); d /= np.linalg.norm(d)
        for _ in range(segments):
            d = d + 0.25 * rng.normal(size=3); d /= np.linalg.norm(d)
            q = p + d * rng.uniform(0.15, 0.3)
            s = np.cross(d, rng.normal(size=3)); s *= 0.002 / np.linalg.norm(s)
            b = len(pts)
            pts += [p - s, p + s, q + s, q - s]
            idx += [(b, b + 1, b + 2), (b, b + 2, b + 3)]
            p = q
    return _f32(pts), np.asarray(idx, np.uint32)


def hair_of(n_tris, seed=9):
    """A hair mesh of exactly n_tris triangles (one strand per 8 quads)."""
    quads = (n_tris + 1) // 2
    strands = (quads + 7) // 8
    pts, idx = hair(strands, 8, seed)
    return pts, np.ascontiguousarray(idx[:n_tris])


def soup(n, seed, spread=1.0, size=0.05):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-spread, spread, (n, 1, 3))
    pts = (c + rng.uniform(-size, size, (n, 3, 3))).reshape(-1, 3)
    return _f32(pts), np.arange(3 * n, dtype=np.uint32).reshape(n, 3)


def slivers():
    """tests/test_device_build_gpu.py: test_degenerate_and_huge_triangles_do_not_derail_the_build — a small soup plus 24 giant slivers, one
    of them a line, one a point."""
    rng = np.random.default_rng(11)
    pts, _ = soup(6000, 21, 1.0, 0.01)
    big = []
    for k in range(24):
        a = rng.uniform(-40, 40, 3); b = a + rng.uniform(-80, 80, 3); c = a + (b - a) * 0.5 + rng.uniform(-1e-3, 1e-3, 3)
        if k == 0: c = b
        if k == 1: b = a; c = a
        big += [a, b, c]
    pts = _f32(np.concatenate([pts.astype(np.float64), np.asarray(big)]))
    return pts, np.arange(len(pts), dtype=np.uint32).reshape(-1, 3)


def sheet(n=600, seed=4):
    pts, idx = soup(n, seed, 2.0, 0.03)
    pts[:, 1] = 0.25
    return pts, idx


def copies(n=100):
    tri = np.asarray([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    return _f32(np.tile(tri, (n, 1))), np.arange(3 * n, dtype=np.uint32).reshape(n, 3)


def hairball(strands=40, sides=6, segments=20):
    from tools import standins
    pts, idx, _ = standins.hairball_geometry(strands=strands, sides=sides, segments=segments)
    return _f32(pts), np.ascontiguousarray(idx, np.uint32)


def case_meshes():
    """name -> (points f32, indices u32).  Made once by the test modules and left unchanged."""
    return {"hair800": hair(40, 10), "hairball": hairball(), "slivers": slivers(), "sheet": sheet(), "copies": copies(),
            "hair64": hair_of(64), "hair255": hair_of(255), "hair256": hair_of(256), "hair257": hair_of(257), "fat_soup": soup(700, 9, 1.0, 0.2)}


def hair10k():
    return hair(500, 10, seed=6)


# ---- the tree --------------------------------------------------------------------------------------------------------------------

def child_boxes(nodes):
    """(lo, hi): n x 4 x 3 each, and refs: n x 4 int32."""
    n = np.asarray(nodes, np.float32).reshape(-1, 8, 4)
    lo = np.stack([n[:, s, :] for s in LO], axis=2)
    hi = np.stack([n[:, s, :] for s in HI], axis=2)
    return lo, hi, n[:, CHILD, :].view(np.int32)


def mesh_bounds(pts, idx):
    used = np.asarray(pts, np.float32)[np.asarray(idx).ravel()]
    return used.min(axis=0), used.max(axis=0)


def walk(nodes, root, num_refs, bounds):
    """Level by level from the root.  Returns (shape violations, nesting violations, depth found, leaves) with leaves = dict of arrays:
    first, count, lo, hi (the region R(L), f64), node, slot (-1 / -1 for a root leaf).  A node reached again is counted and not entered."""
    nodes = np.asarray(nodes, np.float32).reshape(-1, 32)
    n = len(nodes)
    shape = nesting = 0
    b_lo, b_hi = np.asarray(bounds[0], np.float64), np.asarray(bounds[1], np.float64)
    L = dict(first=[], count=[], lo=[], hi=[], node=[], slot=[])
    if root == EMPTY or root >= n:  # no tree at all (a dump is never of an empty mesh), or a root that is no node
        return 1, 0, 0, {k: np.zeros((0, 3) if k in ("lo", "hi") else 0, np.float64 if k in ("lo", "hi") else np.int64) for k in L}
    if root < 0:
        v = ~int(root) & 0xffffffff
        shape += n != 0
        leaves = dict(first=np.asarray([v >> 3]), count=np.asarray([(v & 7) + 1]), lo=b_lo[None], hi=b_hi[None], node=np.asarray([-1]), slot=np.asarray([-1]))
        return shape, 0, 0, leaves
    lo, hi, refs = child_boxes(nodes)
    visits = np.zeros(n, np.int64)
    front = np.asarray([root]); p_lo, p_hi = b_lo[None], b_hi[None]; r_lo, r_hi = b_lo[None], b_hi[None]
    visits[root] = 1
    depth = level = 0
    while len(front):
        depth = level
        c_lo, c_hi, c_ref = lo[front].astype(np.float64), hi[front].astype(np.float64), refs[front].astype(np.int64)
        empty = c_ref == EMPTY
        shape += int((empty & ~((c_lo == FLT_MAX).all(axis=2) & (c_hi == -float(FLT_MAX)).all(axis=2))).sum())
        shape += int(empty.all(axis=1).sum())  # a node without a child
        inside = (c_lo >= p_lo[:, None, :]).all(axis=2) & (c_hi <= p_hi[:, None, :]).all(axis=2)
        nesting += int((~empty & ~inside).sum())
        k_lo, k_hi = np.maximum(c_lo, r_lo[:, None, :]), np.minimum(c_hi, r_hi[:, None, :])
        leaf = ~empty & (c_ref < 0)
        fi, si = np.nonzero(leaf)
        v = (~c_ref[fi, si]) & 0xffffffff
        L["first"].append(v >> 3); L["count"].append((v & 7) + 1); L["lo"].append(k_lo[fi, si]); L["hi"].append(k_hi[fi, si])
        L["node"].append(front[fi]); L["slot"].append(si)
        inner = ~empty & (c_ref >= 0)
        bad = inner & (c_ref >= n)
        shape += int(bad.sum())
        fi, si = np.nonzero(inner & ~bad)
        nxt = c_ref[fi, si]
        np.add.at(visits, nxt, 1)
        uniq, where = np.unique(nxt, return_index=True)
        where = where[visits[uniq] == np.bincount(nxt, minlength=n)[uniq]]  # not seen on an earlier level; one of this level's arrivals enters
        fi, si = fi[where], si[where]
        front = c_ref[fi, si]; p_lo, p_hi = c_lo[fi, si], c_hi[fi, si]; r_lo, r_hi = k_lo[fi, si], k_hi[fi, si]
        level += 1
    shape += int((visits != 1).sum())
    leaves = {k: (np.concatenate(v) if v else np.zeros(0)) for k, v in L.items()}
    order = np.argsort(leaves["first"], kind="stable")
    leaves = {k: v[order] for k, v in leaves.items()}
    f, c = leaves["first"], leaves["count"]
    if len(f) == 0 or f[0] != 0 or f[-1] + c[-1] != num_refs:
        shape += 1
    shape += int((f[1:] != f[:-1] + c[:-1]).sum())
    return shape, nesting, depth, leaves


# ---- the samples -----------------------------------------------------------------------------------------------------------------

_GRID = np.asarray([(i, j, 8 - i - j) for i in range(9) for j in range(9 - i)], np.float64)


def grid_samples(tri):
    """tri: 3 x 3 f64.  45 points."""
    return (_GRID[:, :1] * tri[0] + _GRID[:, 1:2] * tri[1] + _GRID[:, 2:] * tri[2]) / 8.0


def seam_samples(tri, r_lo, r_hi, interior=False):
    """The seam edge samples of triangle `tri` for its regions, and per plane the interior sample: (edge points e x 3, interior points i x 3)."""
    t_lo, t_hi = tri.min(axis=0), tri.max(axis=0)
    edge, inner = [], []
    for ax in range(3):
        planes = np.unique(np.concatenate([np.nextafter(r_lo[:, ax], -np.inf), np.nextafter(r_hi[:, ax], np.inf)]))
        planes = planes[(planes > t_lo[ax]) & (planes < t_hi[ax])]
        if not len(planes):
            continue
        hits = np.zeros((3, len(planes)), bool); ps = np.zeros((3, len(planes), 3))
        for k in range(3):
            a, b = tri[k], tri[(k + 1) % 3]
            if a[ax] == b[ax]:
                continue
            hits[k] = (planes >= min(a[ax], b[ax])) & (planes <= max(a[ax], b[ax]))
            t = (planes - a[ax]) / (b[ax] - a[ax])
            ps[k] = a[None, :] + (b - a)[None, :] * t[:, None]
            ps[k, :, ax] = planes
            edge.append(ps[k][hits[k]])
        if interior:  # the two crossings of each plane (a plane through a vertex meets three edges, two of them in that vertex: the pair furthest apart)
            pairs = ((0, 1), (1, 2), (0, 2))
            dist = np.stack([np.where(hits[i] & hits[j], np.abs(ps[i] - ps[j]).sum(axis=1), -1.0) for i, j in pairs])
            best = dist.argmax(axis=0); cols = np.nonzero(dist.max(axis=0) >= 0.0)[0]
            pi, pj = np.asarray(pairs)[best[cols]].T
            m = 0.5 * (ps[pi, cols] + ps[pj, cols]); m[:, ax] = planes[cols]
            inner.append(m)
    e = np.concatenate(edge) if edge else np.zeros((0, 3))
    i = np.concatenate(inner) if inner else np.zeros((0, 3))
    return np.clip(e, t_lo, t_hi), np.clip(i, t_lo, t_hi)


def _slack(p, r_lo, r_hi):
    """How far each point is from the nearest of the regions (0: inside one)."""
    out = np.maximum(np.maximum(r_lo[None] - p[:, None, :], p[:, None, :] - r_hi[None]), 0.0).max(axis=2)
    return out.min(axis=1)


def validate(dump, pts, idx, presplit, seam_every=1, keep_samples=False):
    """dump: dict(nodes, tri, root, depth).  seam_every = k takes the seam samples of every k-th triangle only (0: none; the grid is always taken
    on all): the larger case meshes would otherwise spend their time here.  Returns a report: violations per rule ("shape", "nesting", "cover"), "detail" (what the counts are
    made of), "worst_slack", the numbers of samples ("grid", "seam"), "uncovered_grid" / "uncovered_seam", and with keep_samples the seam samples themselves: "seam_edge" and
    "interior", each (points x 3, triangle per point); the interior ones are for the ray test."""
    pts = np.asarray(pts, np.float32); idx = np.asarray(idx, np.int64)
    tri_ids = np.asarray(dump["tri"], np.int64)
    nt, nr = len(idx), len(tri_ids)
    shape, nesting, depth, lv = walk(dump["nodes"], int(dump["root"]), nr, mesh_bounds(pts, idx))
    detail = dict(walk_shape=shape, depth_found=depth)
    if depth != int(dump["depth"]):
        shape += 1
    seen = np.bincount(tri_ids[tri_ids < nt], minlength=nt)
    detail["missing_triangles"] = int((seen == 0).sum())
    shape += int((seen == 0).sum()) + int((tri_ids >= nt).sum())
    if not presplit:
        shape += int((seen > 1).sum())
    # one region per reference, grouped by triangle
    first, count = lv["first"].astype(np.int64), lv["count"].astype(np.int64)
    ref_leaf = np.repeat(np.arange(len(first)), count); ref_pos = np.concatenate([np.arange(f, f + c) for f, c in zip(first, count)]) if len(first) else np.zeros(0, np.int64)
    ok = ref_pos < nr
    ref_leaf, ref_pos = ref_leaf[ok], ref_pos[ok]
    ref_tri = tri_ids[ref_pos]
    order = np.argsort(ref_tri, kind="stable")
    ref_leaf, ref_tri = ref_leaf[order], ref_tri[order]
    start = np.searchsorted(ref_tri, np.arange(nt + 1))
    V = pts[idx].astype(np.float64)  # nt x 3 x 3
    worst = 0.0
    n_grid = n_seam = bad_grid = bad_seam = 0
    kept = dict(seam_edge=([], []), interior=([], []))
    for t in range(nt):
        leaves = np.unique(ref_leaf[start[t]:start[t + 1]])
        if not len(leaves):
            continue  # counted under shape
        r_lo, r_hi = lv["lo"][leaves], lv["hi"][leaves]
        tri = V[t]
        tol = 4.0 * 2.0**-53 * np.abs(tri).max()
        g = np.clip(grid_samples(tri), tri.min(axis=0), tri.max(axis=0))
        s = _slack(g, r_lo, r_hi)
        n_grid += len(g); bad_grid += int((s > tol).sum()); worst = max(worst, float(s.max()))
        if seam_every and t % seam_every == 0:
            e, inner = seam_samples(tri, r_lo, r_hi, keep_samples)
            if len(e):
                s = _slack(e, r_lo, r_hi)
                n_seam += len(e); bad_seam += int((s > tol).sum()); worst = max(worst, float(s.max()))
            if keep_samples:
                for name, q in (("seam_edge", e), ("interior", inner)):
                    kept[name][0].append(q); kept[name][1].append(np.full(len(q), t))
    rep = dict(shape=int(shape), nesting=int(nesting), cover=bad_grid + bad_seam, worst_slack=worst, grid=n_grid, seam=n_seam, uncovered_grid=bad_grid,
               uncovered_seam=bad_seam, detail=detail, leaves=lv, refs=nr)
    if keep_samples:
        for name, (q, t) in kept.items():
            rep[name] = (np.concatenate(q), np.concatenate(t)) if q else (np.zeros((0, 3)), np.zeros(0, np.int64))
    return rep


def clean(rep):
    return rep["shape"] == 0 and rep["nesting"] == 0 and rep["cover"] == 0


def line(name, rep, seconds=None):
    """One report line for the test log."""
    return "%-22s refs %7d  grid %7d  seam %7d  uncovered %d + %d  shape %d  nesting %d  worst slack %.3g%s" % (
        name, rep["refs"], rep["grid"], rep["seam"], rep["uncovered_grid"], rep["uncovered_seam"], rep["shape"], rep["nesting"], rep["worst_slack"],
        "" if seconds is None else "  %.2f s" % seconds)
