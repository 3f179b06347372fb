"""The f32 box culling of the traversals (nrays_amd/csrc/trace_device.h: make_rayf, best_f32, load_planes, box_keys4,
zero_axis_cull) against the reference's f64 ray / AABB test: the restatements and the case sets, shared by
tests/test_box_cull.py (CPU: the mirror) and tests/test_box_cull_gpu.py (the kernels, through nrays_debug_box_cull).

THE TESTED STATEMENT.  For a ray (o, d), a current best distance `best` and an f32 box,

    the reference accepts the box and max(tmin, 0) <= best   ==>   the key of the box's slot is finite.

A key may be finite where the reference rejects (a superset).  The reference is ncollide's ray_aabb with solid = true
(AABB::toi_with_ray, SURVEY B-3) in f64: `ray_aabb_f64` below, written from that description — the slab interval of every axis
from one reciprocal of the direction component (ncollide's `denom`), and, because B-3 writes the two distances as quotients,
the same test with a division per plane as well: a case either form accepts counts as accepted.  `ray_aabb_exact` is the same
test in rational arithmetic (fractions.Fraction), applied to the cases whose f64 comparisons are within a few roundings of a
tie; a class is judged by the f64 forms, which are the reference's arithmetic, and the share on which the exact one disagrees
is reported (<= 1 %).

THE MIRROR (`mirror_keys`) restates make_rayf, best_f32, box_keys4 and zero_axis_cull in numpy float32, operation for
operation, from a GIVEN f32 reciprocal per axis: the device's own (GPU test: keys must be equal bit for bit), or the
correctly rounded one and its two f32 neighbours (CPU test: the statement for any reciprocal within 1 ulp).  The fma is
rounded ONCE: the product of two f32 is exact in f64, the f64 sum is brought to round-to-odd with the error term of TwoSum,
and the cast to f32 is then the only rounding that counts (round-to-odd needs two spare bits; f64 has 29).
`inv_threshold` restates the cut-offs of inv_f32.  Keys are compared after `+ 0.0f` (the sign of a zero key is not pinned:
fmaxf(-0, +0) may return either).

WHAT THE DIRECTIONS OF A CLASS MUST SATISFY: at least one component of ordinary size (the classes keep the length within
1e-12 .. 3.4e38).  A direction whose EVERY component is below 1e-30 is outside the statement: zero_axis_cull's margin of 1e-20
stands for "reaches the slab within 1e10 units of t" (trace_device.h), and such a ray may take 1e12.

TIGHTNESS (`tightness_cases`).  box_keys4 accepts iff n <= f * kSlack with n = max_a tn_a, f = min_a tf_a.  From the comment
in trace_device.h, per plane of axis a, in t: an absolute part (margin e = 2^-21 |p| plus the roundings of o32, p and the
addend, 3 * 2^-24 |p|, p = o_a inv_a) and a relative part (3 * 2^-24 for inv32 + 2^-24 for the fma = 2^-22 of t), and kSlack =
1.4e-6 = 2^-19.45 on f.  Carried to space by |d_a| (t |d_a| = |b_a - o_a| <= |o_a| + |b_a|), the f32 test accepts nothing the
exact test rejects for the box grown on every axis by
    (2^-21 + 3 * 2^-24) |o_a| + (2^-22 + 2^-19.45) (|o_a| + |b_a|) <= 2.29e-6 |o_a| + 1.63e-6 |b_a|  <  0.61 * 2^-18 (|o_a| + max|b_a|).
The growth the family uses, 2^-18 (|o_a| + max |b_a|), is therefore a bound the documented margins imply with a factor 1.6 to
spare (8 x the absolute margin alone, 2.7 x kSlack alone): a case the exact test rejects for the grown box must get +inf.
"""
import fractions

import numpy as np

F32, F64 = np.float32, np.float64
DBL_MAX = np.finfo(F64).max
FLT_MAX = np.finfo(F32).max
INF32 = F32(np.inf)
K21 = F32(2.0 ** -21)
KSLACK = F32(1.0000014)
BEST_FACTOR = F32(1.0000004)
ZERO_MARGIN_REL = F32(2.384185791015625e-07)  # 2^-22
GROW = 2.0 ** -18


# ---------------------------------------------------------------- the reference: f64 and exact --------------------------------
def ray_aabb_f64(o, d, mn, mx, divide=False):
    """ncollide ray_aabb (solid = true) on n cases: (accepted, toi = max(tmin, 0)); toi is meaningless where rejected."""
    o, d, mn, mx = (np.asarray(a, F64) for a in (o, d, mn, mx))
    n = len(o)
    tmin, tmax, ok = np.full(n, -DBL_MAX), np.full(n, DBL_MAX), np.ones(n, bool)
    with np.errstate(all="ignore"):
        for a in range(3):
            z = d[:, a] == 0.0
            if divide:
                tn, tf = (mn[:, a] - o[:, a]) / d[:, a], (mx[:, a] - o[:, a]) / d[:, a]
            else:
                denom = 1.0 / d[:, a]
                tn, tf = (mn[:, a] - o[:, a]) * denom, (mx[:, a] - o[:, a]) * denom
            sw = tn > tf
            tn, tf = np.where(sw, tf, tn), np.where(sw, tn, tf)
            tmin = np.where(~z & (tn > tmin), tn, tmin)
            tmax = np.where(~z & (tf < tmax), tf, tmax)
            ok &= np.where(z, ~((o[:, a] < mn[:, a]) | (o[:, a] > mx[:, a])), ~((tmax < 0.0) | (tmin > tmax)))
    return ok, np.where(tmin < 0.0, 0.0, tmin)


def reference_accepts(o, d, mn, mx, best):
    """The left side of the tested statement, in the reference's f64 arithmetic (either way of forming the distances)."""
    acc = np.zeros(len(o), bool)
    for divide in (False, True):
        ok, toi = ray_aabb_f64(o, d, mn, mx, divide)
        acc |= ok & (toi <= best)
    return acc


def near_tie(o, d, mn, mx, best, rel=1e-13):
    """Cases in which a comparison of the f64 test is within `rel` of a tie (every distance carries at most 3 roundings of
    2^-53): only there can the exact test decide otherwise than the f64 one."""
    o, d, mn, mx = (np.asarray(a, F64) for a in (o, d, mn, mx))
    n = len(o)
    with np.errstate(all="ignore"):
        tn = np.where(d != 0.0, (mn - o) / d, -np.inf)
        tf = np.where(d != 0.0, (mx - o) / d, np.inf)
        lo, hi = np.minimum(tn, tf).max(axis=1), np.maximum(tn, tf).min(axis=1)
        lo0 = np.maximum(lo, 0.0)
        scale = np.maximum(np.abs(lo), np.abs(hi))
        near = ~(np.abs(hi - lo0) > rel * scale) | ~(np.abs(hi) > 1e-290) | ~(np.abs(best - lo0) > rel * np.maximum(np.abs(best), lo0))
        near |= ~np.isfinite(lo) & (d != 0.0).any(axis=1) | ~np.isfinite(hi) & (d != 0.0).any(axis=1)
    return near.reshape(n)


def ray_aabb_exact(o, d, mn, mx, best=None, grow=(0.0, 0.0, 0.0)):
    """One case in rational arithmetic: the slab test over the reals, the box grown by grow[a] on both sides of axis a."""
    Fr = fractions.Fraction
    lo, hi = None, None
    for a in range(3):
        oa, da, g = Fr(float(o[a])), Fr(float(d[a])), Fr(float(grow[a]))
        l, h = Fr(float(mn[a])) - g, Fr(float(mx[a])) + g
        if da == 0:
            if oa < l or oa > h:
                return False
            continue
        t1, t2 = (l - oa) / da, (h - oa) / da
        if t1 > t2:
            t1, t2 = t2, t1
        lo = t1 if lo is None or t1 > lo else lo
        hi = t2 if hi is None or t2 < hi else hi
    if lo is None:
        return True
    if hi < 0 or lo > hi:
        return False
    return best is None or max(lo, Fr(0)) <= Fr(float(best))


def exact_accepts(case, idx, grow=None):
    o, d, box, best = case["o"], case["d"], case["box"].astype(F64), case["best"]
    return np.array([ray_aabb_exact(o[i], d[i], box[i, :3], box[i, 3:], best[i], (0.0, 0.0, 0.0) if grow is None else grow[i]) for i in idx], bool)


# ---------------------------------------------------------------- the f32 mirror ------------------------------------------------
def fma32(a, b, c):
    """fl32(a * b + c) with ONE rounding, elementwise on float32 arrays."""
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    with np.errstate(all="ignore"):
        p, c64 = a.astype(F64) * b.astype(F64), c.astype(F64)
        s = p + c64
        bb = s - p
        err = (p - (s - bb)) + (c64 - bb)
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0.0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0.0, np.inf, -np.inf)), s)
        return s.astype(F32)


def inv_exact(d):
    """The correctly rounded f32 reciprocal of fl32(d) (no f64 quotient of an f32 lies within 2^-53 of an f32 tie)."""
    with np.errstate(all="ignore"):
        x = np.asarray(d, F64).astype(F32)
        return x, (1.0 / x.astype(F64)).astype(F32)


LONG_INV, LONG_ADD = F32(1e-8), F32(1e29)


def inv_threshold(x, r, long_fix=True):
    """inv_f32's cut-offs on a raw reciprocal r of x = fl32(d): 0 = the axis does not constrain the ray (a component that is zero in f32,
    |x| <= 1e-30 or |r| >= 1e30: zero_axis_cull's rule applies; or one beyond 1e30, |r| <= 1e-30: no rule applies)."""
    with np.errstate(all="ignore"):
        keep = (np.abs(x) > F32(1e-30)) & (np.abs(r) < F32(1e30))
        if long_fix:
            keep &= np.abs(r) > F32(1e-30)
        return np.where(keep, r, F32(0.0)).astype(F32)


def all_long(d, inv):
    """make_rayf's special case: every axis unconstrained and none zero in f32 — all three components beyond 1e30.  `inv` as inv_f32 returns it,
    or as the probe reports it (x already replaced by the constant)."""
    inv = np.asarray(inv, F32)
    with np.errstate(all="ignore"):
        big = ~(np.abs(np.asarray(d, F64).astype(F32)) < F32(1.0))
        return big.all(axis=1) & ((inv[:, 0] == 0) | (inv[:, 0] == LONG_INV)) & (inv[:, 1] == 0) & (inv[:, 2] == 0)


def inv_reported(d, inv):
    """The reciprocals as inv_f32 returned them, from the probe's report (RayF::ix after make_rayf's special case)."""
    out = np.array(inv, F32)
    out[all_long(d, inv), 0] = 0.0
    return out


def inv_candidates(d, long_fix=True, flush=False):
    """inv32 as inv_f32 returns it for the correctly rounded reciprocal and its two neighbours.  flush: a reciprocal below the
    smallest normal f32 comes back as 0 (what the parent commit's code met on a device that flushes there)."""
    x, r = inv_exact(d)
    out = []
    with np.errstate(all="ignore"):
        for rr in (np.nextafter(r, -INF32), r, np.nextafter(r, INF32)):
            rr = np.where(np.isfinite(r), rr, r).astype(F32)
            if flush:
                rr = np.where(np.abs(rr) < np.finfo(F32).tiny, F32(0.0), rr).astype(F32)
            out.append(inv_threshold(x, rr, long_fix))
    return out


def node_planes(box, slot):
    """(lower, upper): (n, 3, 4) planes of the node nrays_debug_box_cull builds — the box in child `slot`, three absent children."""
    n = len(box)
    lo, hi = np.full((n, 3, 4), FLT_MAX, F32), np.full((n, 3, 4), -FLT_MAX, F32)
    lo[np.arange(n), :, slot] = box[:, :3]
    hi[np.arange(n), :, slot] = box[:, 3:]
    return lo, hi


def mirror_keys(o, d, best, box, slot, inv, e_scale=K21, kslack=KSLACK, best_factor=BEST_FACTOR, zero_margin=True, swap=False,
                clamp0=True, zero_strict=False, long_fix=True):
    """(keys (n, 4) f32, bits (n,) u32) of one node visit.  `inv`: (n, 3) f32, inv_f32's result per axis.  The keyword arguments
    are the mutants of tests/test_box_cull.py; the defaults are the product."""
    o, d = np.asarray(o, F64), np.asarray(d, F64)
    inv = inv_reported(d, inv) if long_fix else np.asarray(inv, F32)
    n = len(o)
    lo, hi = node_planes(np.asarray(box, F32), np.asarray(slot))
    with np.errstate(all="ignore"):
        o32, d32 = o.astype(F32), d.astype(F32)
        p = o32 * inv
        e = np.abs(p) * F32(e_scale)
        nn = np.where(inv != 0, -p - e, -INF32).astype(F32)
        nf = np.where(inv != 0, -p + e, INF32).astype(F32)
        neg = inv < 0
        zero = (inv == 0) & (np.abs(d32) < F32(1.0)) if long_fix else (inv == 0)
        bits = (neg * np.array([16, 32, 64], np.uint32)).sum(axis=1).astype(np.uint32) | (zero * np.array([1, 2, 4], np.uint32)).sum(axis=1).astype(np.uint32)
        if long_fix:        # all three components beyond 1e30: the x axis keeps a slab that only an absent child's inverted box fails
            al = all_long(d, inv)
            inv = inv.copy()
            inv[al, 0], nn[al, 0], nf[al, 0] = LONG_INV, -LONG_ADD, LONG_ADD
        near = np.where(neg[:, :, None] != swap, hi, lo)
        far = np.where(neg[:, :, None] != swap, lo, hi)
        tn = fma32(near, inv[:, :, None], nn[:, :, None])
        tf = fma32(far, inv[:, :, None], nf[:, :, None])
        tbest = (np.asarray(best, F64).astype(F32) * F32(best_factor) + F32(1e-37)).astype(F32)
        zn = np.fmax(tn[:, 2], F32(0.0)) if clamp0 else tn[:, 2]
        kn = np.fmax(np.fmax(tn[:, 0], tn[:, 1]), zn)
        kf = np.fmin(np.fmin(tf[:, 0], tf[:, 1]), np.fmin(tf[:, 2], tbest[:, None]))
        keys = np.where(kn <= kf * F32(kslack), kn, INF32).astype(F32)
        # zero_axis_cull: for a zero axis the "entry" plane fetched is the lower one (inverse 0 is not negative)
        m = (np.abs(o32) * ZERO_MARGIN_REL + F32(1e-20)).astype(F32) if zero_margin else np.zeros_like(o32)
        a, b = (o32 + m).astype(F32)[:, :, None], (o32 - m).astype(F32)[:, :, None]
        out = ((a <= near) | (b >= far)) if zero_strict else ((a < near) | (b > far))
        keys = np.where((out & zero[:, :, None]).any(axis=1), INF32, keys).astype(F32)
    return keys, bits


def same_keys(a, b):
    with np.errstate(all="ignore"):
        return (np.asarray(a, F32) + F32(0.0)).view(np.uint32) == (np.asarray(b, F32) + F32(0.0)).view(np.uint32)


def ulps32(a, b):
    """Distance of two finite f32 arrays of equal sign in units of the last place."""
    ia, ib = np.asarray(a, F32).view(np.int32).astype(np.int64), np.asarray(b, F32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


# ---------------------------------------------------------------- the case sets -------------------------------------------------
def _f32(a):
    return np.asarray(a, F64).astype(F32)


def _boxes(rng, n, centre, extent, flat=None):
    """f32 boxes: centres uniform in +-centre (an array: per case), extents log-uniform in `extent`; `flat[i]` of the axes of box i
    (random ones) collapse to mn == mx."""
    c = rng.uniform(-1.0, 1.0, (n, 3)) * np.asarray(centre, F64).reshape(-1, 1)
    h = 10.0 ** rng.uniform(np.log10(extent[0]), np.log10(extent[1]), (n, 3)) * 0.5
    mn, mx = _f32(c - h), _f32(c + h)
    mx = np.maximum(mx, mn)
    if flat is not None:
        rank = np.argsort(np.argsort(rng.random((n, 3)), axis=1), axis=1)
        for k in range(3):
            sel = rank[:, k] < flat
            mx[sel, k] = mn[sel, k]
    return mn, mx


def _targets(rng, n, mn, mx, interior=0.1):
    """A point of each box: per axis the lower plane, the upper plane (both f32-exact) or the interior — faces, edges, corners, interior."""
    code = rng.integers(0, 3, (n, 3))
    code[rng.random(n) < interior] = 2
    t = rng.random((n, 3))
    q = np.where(code == 0, mn, np.where(code == 1, mx, mn.astype(F64) + t * (mx.astype(F64) - mn.astype(F64))))
    return q.astype(F64)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _case(o, d, mn, mx, best=None, rng=None):
    n = len(o)
    return {"o": np.ascontiguousarray(o, F64), "d": np.ascontiguousarray(d, F64), "best": np.full(n, DBL_MAX) if best is None else np.ascontiguousarray(best, F64),
            "box": np.ascontiguousarray(np.concatenate([mn, mx], axis=1), F32), "slot": (np.arange(n) % 4).astype(np.uint32)}


def _nudge(rng, n, exact_share=0.02):
    """Per axis a signed relative offset, log-uniform in 1e-12 .. 1e-5: from far inside what f64 resolves to past the f32 margins.
    A share `exact_share` of the cases gets none: those rays graze to within the roundings of f64, where the f64 test and the exact
    one part (condition: on at most 1 % of a class)."""
    r = 10.0 ** rng.uniform(-12, -5, (n, 3)) * np.where(rng.random((n, 3)) < 0.5, -1.0, 1.0)
    r[rng.random(n) < exact_share] = 0.0
    return r


def _aimed(rng, n, mn, mx, dist, behind=0.2, scale=None, interior=0.1):
    """Rays aimed at a point q of the box from an origin `dist` away: o = q - t u in f64 (nudged, see _nudge), d = u * scale.  A share
    `behind` points away from q.  Through an edge or a corner the ray touches the box in q alone unless its signs lead into the box."""
    q = _targets(rng, n, mn, mx, interior)
    u = _unit(rng, n)
    t = 10.0 ** rng.uniform(np.log10(dist[0]), np.log10(dist[1]), n)
    o = q - t[:, None] * u
    o = o + _nudge(rng, n) * (np.abs(o) + np.abs(q))
    d = u * np.where(rng.random(n) < behind, -1.0, 1.0)[:, None]
    if scale is not None:
        d = d * scale[:, None]
    return o, d


def class_ordinary(n=32768, seed=101):
    rng = np.random.default_rng(seed)
    mn, mx = _boxes(rng, n, np.full(n, 8.0), (1e-2, 4.0))
    o, d = _aimed(rng, n, mn, mx, (1e-2, 30.0))
    d *= rng.uniform(0.5, 2.0, n)[:, None]
    return _case(o, d, mn, mx)


def class_far_origin(n=32768, seed=102):
    """Origin (and box) 1e3 .. 1e7 from the coordinate origin, boxes of extent 1e-4 .. 1 at 1e-3 .. 10 from the ray's origin: |p| = |o inv|
    is huge against t, and the absolute margin e carries the test."""
    rng = np.random.default_rng(seed)
    mn, mx = _boxes(rng, n, 10.0 ** rng.uniform(3, 7, n), (1e-4, 1.0))
    o, d = _aimed(rng, n, mn, mx, (1e-3, 10.0), behind=0.1)
    return _case(o, d, mn, mx)


def class_far_box(n=16384, seed=109):
    """The same boxes near the coordinate origin, seen from 1e3 .. 1e7 away: t is huge, and the relative slack carries the test."""
    rng = np.random.default_rng(seed)
    mn, mx = _boxes(rng, n, np.full(n, 10.0), (1e-4, 1.0))
    o, d = _aimed(rng, n, mn, mx, (1e3, 1e7))
    return _case(o, d, mn, mx)


def class_flat(n=24576, seed=103):
    rng = np.random.default_rng(seed)
    flat = rng.choice([1, 2, 3], n, p=[0.7, 0.2, 0.1])
    mn, mx = _boxes(rng, n, np.full(n, 8.0), (1e-2, 4.0), flat=flat)
    o, d = _aimed(rng, n, mn, mx, (1e-2, 30.0), behind=0.1, interior=0.5)
    # in-plane rays for a part: the direction component of a collapsed axis exactly 0, the origin in the plane
    k = rng.integers(0, 3, n)
    sel = (mn[np.arange(n), k] == mx[np.arange(n), k]) & (rng.random(n) < 0.3)
    d[sel, k[sel]] = 0.0
    o[sel, k[sel]] = mn[sel, k[sel]]
    return _case(o, d, mn, mx)


def class_zero_origin(n=32768, seed=104):
    """Origin coordinates exactly 0 (one, two or all three): the absolute margin e vanishes there.  A third of the boxes has a
    face in the coordinate plane of a zero origin coordinate, at either side, met under either sign of the direction."""
    rng = np.random.default_rng(seed)
    mn, mx = _boxes(rng, n, np.full(n, 4.0), (1e-2, 4.0))
    zero = rng.random((n, 3)) < 0.55
    zero[rng.random(n) < 0.25] = True
    zero[~zero.any(axis=1), 0] = True
    k = rng.integers(0, 3, n)
    rows = np.arange(n)
    face = zero[rows, k] & (rng.random(n) < 0.45)
    lower = rng.random(n) < 0.5
    ext = (mx - mn)[rows, k]
    mn[face & lower, k[face & lower]] = 0.0
    mx[face & lower, k[face & lower]] = ext[face & lower]
    mx[face & ~lower, k[face & ~lower]] = 0.0
    mn[face & ~lower, k[face & ~lower]] = -ext[face & ~lower]
    q = _targets(rng, n, mn, mx)
    o = np.where(zero, 0.0, q - rng.uniform(-1.0, 1.0, (n, 3)) * 10.0 ** rng.uniform(-2, 1.5, (n, 1)))
    s = 10.0 ** rng.uniform(-1, 1, n) * np.where(rng.random(n) < 0.3, -1.0, 1.0)
    d = (q - o) * s[:, None]
    d = d + _nudge(rng, n) * np.abs(d).max(axis=1, keepdims=True)  # (the origin keeps its exact zeros)
    # the ray inside the coordinate plane (component exactly 0) for a part of the face cases
    inplane = face & (rng.random(n) < 0.3)
    d[inplane, k[inplane]] = 0.0
    dead = ~(np.abs(d).max(axis=1) > 1e-6)
    d[dead] = _unit(rng, int(dead.sum()))
    return _case(o, d, mn, mx)


def _tiny_components():
    """Direction components around the f32-zero cut-off of inv_f32 (|x| > 1e-30f, |1 / x| < 1e30f): exactly 0, f32 denormals,
    1e-36 .. 1e-31, and the f32 neighbours of 1e-30 on both sides (1 / 1e30 = 1e-30: both cut-offs sit there)."""
    t = F32(1e-30)
    near = [t]
    lo = hi = t
    for _ in range(4):
        lo, hi = np.nextafter(lo, F32(0.0)), np.nextafter(hi, INF32)
        near += [lo, hi]
    vals = [0.0, 1.4e-45, 1e-40, 1.1754942e-38, 1e-36, 1e-35, 1e-34, 1e-33, 1e-32, 1e-31, 3e-31, 9.9e-31, 1.01e-30, 2e-30, 1e-29] + [float(v) for v in near]
    vals += [float(t) * (1.0 + 2.0 ** -26), float(t) * (1.0 - 2.0 ** -26)]  # not f32: round to 1e-30f from either side
    return np.array(vals, F64)


def class_tiny_dir(n=32768, seed=105):
    """One or two components at the f32-zero threshold, the others ordinary.  On a tiny axis the origin sits on a face of the slab,
    one f32 ulp inside or outside it, at an f64 value within half an f32 ulp of it, or — with the face in the coordinate plane —
    1e-38 .. 1e-21 outside it, where only the constant of zero_axis_cull's margin is left."""
    rng = np.random.default_rng(seed)
    tiny = _tiny_components()
    mn, mx = _boxes(rng, n, np.full(n, 2.0), (0.5, 4.0))
    rows = np.arange(n)
    q = mn.astype(F64) + rng.uniform(0.05, 0.95, (n, 3)) * (mx.astype(F64) - mn.astype(F64))
    u = _unit(rng, n)
    u = np.where(np.abs(u) < 0.1, 0.1 * np.where(u < 0, -1.0, 1.0), u)
    t = 10.0 ** rng.uniform(-2, 1, n) * np.where(rng.random(n) < 0.7, 1.0, 0.0)  # origin inside the box on the ordinary axes for a part
    o = q - t[:, None] * u
    d = u.copy()
    k1 = rng.integers(0, 3, n)
    two = rng.random(n) < 0.25
    k2 = (k1 + 1 + rng.integers(0, 2, n)) % 3
    for k, on in ((k1, np.ones(n, bool)), (k2, two)):
        idx = rows[on]
        kk = k[on]
        d[idx, kk] = tiny[rng.integers(0, len(tiny), len(idx))] * np.where(rng.random(len(idx)) < 0.5, -1.0, 1.0)
        upper = rng.random(len(idx)) < 0.5
        plane0 = rng.random(len(idx)) < 0.3   # the face into the coordinate plane
        ext = (mx - mn)[idx, kk]
        pm = plane0 & ~upper
        mn[idx[pm], kk[pm]] = 0.0; mx[idx[pm], kk[pm]] = ext[pm]
        pm = plane0 & upper
        mx[idx[pm], kk[pm]] = 0.0; mn[idx[pm], kk[pm]] = -ext[pm]
        f = np.where(upper, mx[idx, kk], mn[idx, kk]).astype(F32)
        outward = np.where(upper, 1.0, -1.0)
        mode = rng.integers(0, 6, len(idx))
        ulp = (np.nextafter(np.abs(f), INF32) - np.abs(f)).astype(F64)
        pos = f.astype(F64)
        pos = np.where(mode == 1, np.nextafter(f, np.where(outward > 0, INF32, -INF32).astype(F32)).astype(F64), pos)
        pos = np.where(mode == 2, np.nextafter(f, np.where(outward > 0, -INF32, INF32).astype(F32)).astype(F64), pos)
        pos = np.where(mode == 3, f.astype(F64) + outward * 0.3 * ulp, pos)
        pos = np.where(mode == 4, f.astype(F64) - outward * 0.3 * ulp, pos)
        pos = np.where(mode == 5, (mn[idx, kk].astype(F64) + mx[idx, kk].astype(F64)) * 0.5, pos)
        far_out = plane0 & (mode <= 2)
        pos = np.where(far_out, outward * 10.0 ** rng.uniform(-38, -21, len(idx)), pos)
        o[idx, kk] = pos
    return _case(o, d, mn, mx)


def class_dir_length(n=32768, seed=106):
    rng = np.random.default_rng(seed)
    mn, mx = _boxes(rng, n, np.full(n, 8.0), (1e-2, 4.0))
    scale = 10.0 ** rng.integers(-12, 13, n).astype(F64) * rng.uniform(1.0, 9.9, n)
    o, d = _aimed(rng, n, mn, mx, (1e-2, 30.0), scale=scale)
    return _case(o, d, mn, mx)


def class_dir_huge(n=32768, seed=107):
    """Lengths 1e36 .. 10^38.5, every component clamped into the f32 range; a tenth has a component of exactly +-FLT_MAX."""
    rng = np.random.default_rng(seed)
    mn, mx = _boxes(rng, n, np.full(n, 8.0), (1e-2, 4.0))
    scale = 10.0 ** rng.uniform(36.0, 38.5, n)
    o, d = _aimed(rng, n, mn, mx, (1e-2, 30.0), scale=scale)
    d = np.clip(d, -float(FLT_MAX), float(FLT_MAX))
    sel = rng.random(n) < 0.1
    k = np.abs(d).argmax(axis=1)
    d[sel, k[sel]] = np.sign(d[sel, k[sel]]) * float(FLT_MAX)
    return _case(o, d, mn, mx)


def class_best_entry(n=32768, seed=108):
    """`best` (a closest hit's toi, or max_toi) at the box's entry distance: exactly, +-1 and +-2 f64 ulps, 1e-12 .. 1e-5 of it
    below and above (half of all these round DOWN to f32), denormal, and DBL_MAX."""
    rng = np.random.default_rng(seed)
    mn, mx = _boxes(rng, n, np.full(n, 8.0), (1e-2, 4.0))
    q = mn.astype(F64) + rng.uniform(0.02, 0.98, (n, 3)) * (mx.astype(F64) - mn.astype(F64))
    u = _unit(rng, n)
    t = 10.0 ** rng.uniform(-2, 1.5, n) * np.where(rng.random(n) < 0.15, 0.0, 1.0)
    o = q - t[:, None] * u
    d = u * 10.0 ** rng.uniform(-1, 1, n)[:, None]
    at0 = rng.random(n) < 0.3   # from the coordinate origin: e = 0, only kSlack and the slack of best_f32 are left
    o[at0] = 0.0
    d[at0] = q[at0] * 10.0 ** rng.uniform(-1, 1, (int(at0.sum()), 1))
    _, toi = ray_aabb_f64(o, d, mn, mx)
    # modes 0..4 sit within two f64 roundings of the tie, where the exact test and the f64 one part: ~100 cases each
    mode = rng.choice(9, n, p=[0.003, 0.003, 0.003, 0.003, 0.003, 0.1, 0.1, 0.3925, 0.3925])
    best = toi.copy()
    for m, steps in ((1, 1), (2, -1), (3, 2), (4, -2)):
        b = toi.copy()
        for _ in range(abs(steps)):
            b = np.nextafter(b, np.inf if steps > 0 else -np.inf)
        best = np.where(mode == m, b, best)
    best = np.where(mode == 5, 5e-324 * rng.integers(1, 1000, n), best)
    best = np.where(mode == 6, DBL_MAX, best)
    best = np.where(mode == 7, toi * (1.0 - 10.0 ** rng.uniform(-12, -5, n)), best)
    best = np.where(mode == 8, toi * (1.0 + 10.0 ** rng.uniform(-12, -5, n)), best)
    return _case(o, d, mn, mx, best=np.maximum(best, 0.0))


CLASSES = {"ordinary": class_ordinary, "far_origin": class_far_origin, "far_box": class_far_box, "flat": class_flat, "zero_origin": class_zero_origin, "tiny_dir": class_tiny_dir,
           "dir_length": class_dir_length, "dir_huge": class_dir_huge, "best_entry": class_best_entry}

_cache = {}


def cases(name):
    """A class with its verdicts, computed once: 'ref' = the f64 reference accepts (the left side of the statement), 'tie' = an
    f64 comparison is near a tie, 'exact' = the exact verdict (equal to 'ref' away from ties, by the rounding bound in near_tie)."""
    if name not in _cache:
        c = CLASSES[name]()
        mn, mx = c["box"][:, :3].astype(F64), c["box"][:, 3:].astype(F64)
        c["ref"] = reference_accepts(c["o"], c["d"], mn, mx, c["best"])
        c["tie"] = near_tie(c["o"], c["d"], mn, mx, c["best"])
        ex = c["ref"].copy()
        idx = np.flatnonzero(c["tie"])
        ex[idx] = exact_accepts(c, idx)
        c["exact"] = ex
        for v in c.values():
            v.setflags(write=False)
        _cache[name] = c
    return _cache[name]


def tightness_cases(n=32768, seed=201):
    """Rays that miss: aimed at a point pushed OFF the box along the axes, by 2^-24 .. 2^-8 of (|o_a| + max |b_a|).  Direction components
    in [1e-3, 1] in magnitude, coordinates up to 1e6: nothing overflows, no axis is f32-zero.  'clear' = the exact test rejects even the
    box grown by GROW (|o_a| + max |b_a|) per axis: those must get +inf."""
    if "tight" in _cache:
        return _cache["tight"]
    rng = np.random.default_rng(seed)
    cen = 10.0 ** rng.uniform(-1, 5.5, n)
    mn, mx = _boxes(rng, n, cen, (1e-2, 10.0))
    code = rng.integers(0, 2, (n, 3))
    q = np.where(code == 0, mn, mx).astype(F64)
    u = rng.uniform(1e-3, 1.0, (n, 3)) * np.where(rng.random((n, 3)) < 0.5, -1.0, 1.0)
    t = 10.0 ** rng.uniform(-1, np.log10(np.minimum(cen * 10.0, 3e5)), n)
    o0 = q - t[:, None] * u
    mag = np.abs(o0) + np.maximum(np.abs(mn), np.abs(mx))
    rel = 2.0 ** rng.uniform(-24, -8, (n, 1))
    push = rel * mag * np.where(code == 0, -1.0, 1.0)
    o = o0 + push
    c = _case(o, u, mn, mx)
    c["push"] = rel.reshape(n)
    c["grow"] = GROW * (np.abs(c["o"]) + np.maximum(np.abs(mn), np.abs(mx)).astype(F64))
    c["ref"] = reference_accepts(c["o"], c["d"], mn.astype(F64), mx.astype(F64), c["best"])
    gmn, gmx = mn.astype(F64) - c["grow"], mx.astype(F64) + c["grow"]
    grown = reference_accepts(c["o"], c["d"], gmn, gmx, c["best"])
    tie = near_tie(c["o"], c["d"], gmn, gmx, c["best"])
    idx = np.flatnonzero(tie)
    grown[idx] = exact_accepts(c, idx, grow=c["grow"])
    c["clear"] = ~grown
    for v in c.values():
        v.setflags(write=False)
    _cache["tight"] = c
    return c


def violations(c, keys):
    """Indices at which the statement fails: the reference accepts, the slot's key is +inf."""
    k = np.asarray(keys)[np.arange(len(c["slot"])), c["slot"]]
    return np.flatnonzero(c["ref"] & ~np.isfinite(k))


def probe(mode, c):
    """nrays_debug_box_cull on a case set: (keys (n, 4) f32, bits (n,) u32, inv32 (n, 3) f32)."""
    import ctypes as C
    from nrays_amd import abi
    n = len(c["o"])
    keys, bits, inv = np.empty((n, 4), F32), np.empty(n, np.uint32), np.empty((n, 3), F32)
    dp, fp, up = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    arr = [np.ascontiguousarray(c[k]) for k in ("o", "d", "best", "box", "slot")]
    abi.check(abi.load_hip_lib().nrays_debug_box_cull(mode, n, arr[0].ctypes.data_as(dp), arr[1].ctypes.data_as(dp), arr[2].ctypes.data_as(dp), arr[3].ctypes.data_as(fp),
                                                      arr[4].ctypes.data_as(up), keys.ctypes.data_as(fp), bits.ctypes.data_as(up), inv.ctypes.data_as(fp)))
    return keys, bits, inv


PUSH_BUCKETS = ((-24, -21), (-21, -18), (-18, -15), (-15, -8))


def extra_acceptance_by_push(c, finite):
    """Tightness family: device accepts - reference accepts in percentage points, by how far (relative, log2) the ray was pushed off the box."""
    out = {}
    for lo, hi in PUSH_BUCKETS:
        sel = (c["push"] >= 2.0 ** lo) & (c["push"] < 2.0 ** hi)
        out["2^%d..2^%d" % (lo, hi)] = round(100.0 * float(finite[sel].mean() - c["ref"][sel].mean()), 2)
    return out
