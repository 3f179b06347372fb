#!/usr/bin/env python
"""Known answers for the analytic shape casts at DEGENERATE and NEAR-DEGENERATE rays, derived independently of
oracle/nrays_oracle.c and of the kernels (trace_device.h) — the rays the random fixtures of make_kat_independent{,2}.py never
hold: exact zero direction components, rays parallel to an axis, a face or a cone generator, through the apex, a corner, an edge
or the capsule's seam, directions a few ulps off a generator or the axis, and lines that graze a surface by 1e-9 of its size.

TRUTH.  A shape is its convex gauge g(p) only (g <= 0 inside):
    ball      |p| - r                                  cuboid    max(|x| - hx, |y| - hy, |z| - hz)
    cylinder  max(|y| - hh, rho - r)                   capsule   dist(p, axis segment) - r
    cone      max(|y| - hh, rho - r (hh - y) / (2 hh))           (apex at +hh, base disc at -hh, rho = hypot(x, z))
Along a ray g is convex: a ternary search finds its minimum over t >= 0 (above zero: a miss), bisection on either side of the
minimiser the entry and the exit, all in 60-digit mpmath.  Thin chords a sampled sweep would step over are found the same way.
The local ray is recovered in mp from the STORED f64 world ray and transform, so the truth belongs to the numbers the casts get.

DIRECTIONS ARE USED AS GIVEN: no direction is normalised after it was written down, and every toi is in the parameter of the
stored direction.  Classes that need an exact zero of the cone's A = dx^2 + dz^2 - k^2 dy^2 use small-integer directions such as
(1, -2, 0) with k = 0.5; the grazing classes use unit tangents (to rounding).

TRANSFORMS.  Every local case is stored twice: under the identity with a dyadic translation (o + t is exact, the zeros reach the
cast), and under a generic rotation, where the zeros become rounding residues (class name + "/rot").  Each of those rows twice
more: solid off and on (the truth differs for interior origins only: toi = 0).

CONDITIONING.  Each case is solved twelve times more, with each of the six local ray components moved by +-2^-50 max(size, |o|).
`well` = hit / miss / origin-inside never flips and the toi moves by at most 1e-12 max(1, toi): those rows are held to
|toi - exact| <= 1e-11 max(1, toi), the bound of tests/test_kat_independent.py.  The others are SKIMMING rows: hit / miss only, and
only where |g_min| >= margin * size (column `margin`), plus a hit point on the surface.  size = max(parameters).
The near-generator rays from well inside and from far outside must be well conditioned; main() asserts it.

MARGINS.  The grazing lines lie in the tangent plane at a random surface point, moved by +-m along the outward normal,
m = 1e-9 (1 + 2^-10) size: the 2^-10 keeps the rounding of the stored f64 ray from carrying |g_min| below the test's 1e-9 size.
MEASURED (repaired oracle, this fixture): every grazing class is decided at 1e-9, `cone_generator_skim` included — a line m off the cone's side whose
tangent is 1e-12 off a generator, |g_min| = 1.12e-9 size (hh 1, r 1) and 1.42e-9 size (hh 1, r 2) in the gauge's radial measure.  The cast_cone before
the repair called 22 of its 48 misses hits; the one that forms its quadratic about the ray's point nearest the apex answers all 96 rows, and the same
lines at m = 1e-10, 1e-11 and 1e-12 size as well (48 lines each, 0 wrong): a factor of a thousand to spare, so the class keeps the common margin and
no class has a wider one.

  python tests/golden/make_kat_degenerate.py      # rewrites tests/golden/kat_degenerate.npz (seed fixed), prints the class counts
"""
import os
import sys
from multiprocessing import Pool

import numpy as np
from mpmath import mp, mpf, sqrt, sin, cos

mp.dps = 60
HERE = os.path.dirname(os.path.abspath(__file__))
BALL, CUBOID, CYLINDER, CAPSULE, CONE = 0, 1, 2, 3, 4  # NraysShapeKind
NAMES = {BALL: "ball", CUBOID: "cuboid", CYLINDER: "cylinder", CAPSULE: "capsule", CONE: "cone"}
OFFSETS = [s * e for e in (2.0 ** -52, 2.0 ** -40, 1e-9, 1e-6, 1e-3) for s in (1.0, -1.0)]
GRAZE = 1e-9 * (1.0 + 2.0 ** -10)
T_IDENTITY = (2.0, -1.5, 0.25)
T_ROTATED, W_ROTATED = (0.3, -1.7, 2.1), (0.7, -1.1, 0.4)
COLUMNS = ["kind", "p0", "p1", "p2", "tx", "ty", "tz", "wx", "wy", "wz", "solid", "ox", "oy", "oz", "dx", "dy", "dz", "hit", "toi", "origin_inside",
           "g_min", "size", "well", "margin"]


def gauge(kind, prm, p):
    x, y, z = p
    if kind == BALL:
        return sqrt(x * x + y * y + z * z) - prm[0]
    if kind == CUBOID:
        return max(abs(x) - prm[0], abs(y) - prm[1], abs(z) - prm[2])
    hh, r = prm[0], prm[1]
    if kind == CAPSULE:
        yc = max(-hh, min(hh, y))
        return sqrt(x * x + (y - yc) ** 2 + z * z) - r
    rho = sqrt(x * x + z * z)
    if kind == CYLINDER:
        return max(abs(y) - hh, rho - r)
    return max(abs(y) - hh, rho - r * (hh - y) / (2 * hh))


def rodrigues(w):
    """Rotation matrix of the scaled-axis vector w (Isometry3::new), 60 digits."""
    th = sqrt(w[0] ** 2 + w[1] ** 2 + w[2] ** 2)
    if th == 0:
        return [[mpf(1), 0, 0], [0, mpf(1), 0], [0, 0, mpf(1)]]
    k = [c / th for c in w]
    s, c = sin(th), cos(th)
    K = [[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]]
    return [[(1 if i == j else 0) + s * K[i][j] + (1 - c) * sum(K[i][m] * K[m][j] for m in range(3)) for j in range(3)] for i in range(3)]


def to_local(R, t, o, d):
    ol = [sum(R[j][i] * (o[j] - t[j]) for j in range(3)) for i in range(3)]  # R^T (o - t)
    dl = [sum(R[j][i] * d[j] for j in range(3)) for i in range(3)]
    return ol, dl


def solve(kind, prm, ol, dl, n_tern, n_bis):
    """(hit, toi, origin_inside, g_min): the entry parameter, or for an interior origin the exit parameter (non-solid)."""
    f = lambda t: gauge(kind, prm, [ol[i] + t * dl[i] for i in range(3)])
    norm = lambda v: sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    tmax = (norm(ol) + 3 * (prm[0] + prm[1] + prm[2])) / norm(dl)  # o + tmax d is outside the bounding sphere
    g0 = f(mpf(0))
    a, b = mpf(0), tmax
    for _ in range(n_tern):
        m1, m2 = a + (b - a) / 3, b - (b - a) / 3
        if f(m1) <= f(m2):
            b = m2
        else:
            a = m1
    tm = (a + b) / 2
    gmin = min(f(tm), g0)
    if g0 <= 0:
        lo, hi = mpf(0), tmax
        for _ in range(n_bis):
            mid = (lo + hi) / 2
            if f(mid) <= 0:
                lo = mid
            else:
                hi = mid
        return True, (lo + hi) / 2, True, gmin
    if gmin > 0:
        return False, mpf(0), False, gmin
    lo, hi = mpf(0), tm
    for _ in range(n_bis):
        mid = (lo + hi) / 2
        if f(mid) <= 0:
            hi = mid
        else:
            lo = mid
    return True, (lo + hi) / 2, False, gmin


def solve_case(job):
    """One stored world ray: the truth and the conditioning verdict."""
    kind, prm, t, w, o_w, d_w = job
    mp.dps = 60
    m = lambda v: [mpf(float(c)) for c in v]
    prm_m = m(prm)
    ol, dl = to_local(rodrigues(m(w)), m(t), m(o_w), m(d_w))
    hit, toi, inside, gmin = solve(kind, prm_m, ol, dl, 150, 130)
    size = max(prm)
    delta = mpf(2) ** -50 * max(mpf(size), sqrt(sum(c * c for c in ol)))
    well = True
    for i in range(6):
        for s in (1, -1):
            o2, d2 = list(ol), list(dl)
            if i < 3:
                o2[i] += s * delta
            else:
                d2[i - 3] += s * delta
            h2, t2, in2, _ = solve(kind, prm_m, o2, d2, 110, 80)
            if h2 != hit or in2 != inside or abs(t2 - toi) > mpf("1e-12") * max(1, toi):
                well = False
                break
        if not well:
            break
    return bool(hit), float(toi), bool(inside), float(gmin), bool(well)


# ---------------------------------------------------------------- the local cases, per shape ---------------------------------
def unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.linalg.norm(v)


def tangent(rng, n):
    """A random unit vector orthogonal to the unit vector n."""
    while True:
        v = rng.normal(size=3)
        v -= n * (v @ n)
        if np.linalg.norm(v) > 0.3:
            return unit(v)


def grazing(add, rng, P, n, u, size, cls_miss="grazing_miss", cls_hit="grazing_hit", margin=GRAZE):
    P, n, u = np.asarray(P, float), np.asarray(n, float), np.asarray(u, float)
    for sign, cls in ((1.0, cls_miss), (-1.0, cls_hit)):
        add(cls, P + sign * margin * size * n - 3.0 * size * u, u, margin=margin / (1.0 + 2.0 ** -10))


def round_cases(kind, hh, r, add):
    """Classes the cylinder, the capsule and the cone share: parallel to the axis, along it, perpendicular to it."""
    x0, z0, far = 0.25 * r, 0.125 * r, hh + r + 2.0
    for sy in (1.0, -1.0):
        add("axis_parallel_inside", (x0, sy * far, z0), (0.0, -sy, 0.0))
        add("axis_parallel_inside", (x0, 0.0, z0), (0.0, sy, 0.0))
        add("axis_parallel_outside", (1.5 * r, sy * far, 0.0), (0.0, -sy, 0.0))
        add("axis_parallel_outside", (-x0, sy * far, 1.5 * r), (0.0, -sy, 0.0))
        add("along_axis", (0.0, sy * far, 0.0), (0.0, -sy, 0.0))
        add("along_axis", (0.0, 0.0, 0.0), (0.0, sy, 0.0))
        add("along_axis", (0.0, 0.5 * hh, 0.0), (0.0, sy, 0.0))
    add("axis_parallel_inside", (x0, far, -z0), (-0.0, -1.0, 0.0))
    for y in (0.0, 0.5 * hh, -0.5 * hh, hh + 0.25):
        for zz in (0.0, z0, 1.5 * r):
            add("perpendicular", (r + 2.0, y, zz), (-1.0, 0.0, 0.0))
        add("perpendicular", (x0, y, -(r + 2.0)), (0.0, 0.0, 1.0))
        add("perpendicular", (x0 + 1.8, y, -2.4), (-0.6, 0.0, 0.8))
        add("perpendicular", (x0, y, 0.0), (1.0, 0.0, -0.0))
    add("perpendicular", (0.0, -0.5 * hh, 0.0), (0.0, 0.0, -1.0))  # from the axis


def near_axis_cases(hh, r, add):
    x0, z0, far = 0.25 * r, 0.125 * r, hh + r + 2.0
    for e in OFFSETS:
        add("near_axis", (x0, 0.0, z0), (e, 1.0, 0.0))                 # from inside, up
        add("near_axis", (x0, -0.25 * hh, -z0), (0.6 * e, -1.0, 0.8 * e))  # from inside, down
        add("near_axis", (x0, far, z0), (e, -1.0, 0.5 * e))            # from outside, inside the radius
        add("near_axis", (r + 0.5, -far, 0.0), (-e, 1.0, 0.0))         # outside the radius: a miss


def build_cases(rng):
    """[(kind, prm, class, o_local, d_local, margin)]"""
    out = []
    for kind, prm in ((BALL, (1.5, 0.0, 0.0)), (CUBOID, (1.0, 0.5, 0.75)), (CYLINDER, (1.0, 0.5, 0.0)), (CYLINDER, (0.5, 1.25, 0.0)),
                      (CAPSULE, (1.0, 0.5, 0.0)), (CAPSULE, (0.5, 1.25, 0.0)), (CONE, (1.0, 1.0, 0.0)), (CONE, (1.0, 2.0, 0.0))):
        size = max(prm)

        def add(cls, o, d, margin=1e-9, kind=kind, prm=prm):
            out.append((kind, prm, cls, np.array(o, dtype=np.float64), np.array(d, dtype=np.float64), margin))

        if kind == BALL:
            r = prm[0]
            for ax in range(3):
                for s in (1.0, -1.0):
                    for off in (0.0, 0.5 * r, 1.5 * r):
                        o = np.zeros(3); o[ax] = s * (r + 2.0); o[(ax + 1) % 3] = off
                        d = np.zeros(3); d[ax] = -s
                        add("zero_components", o, d)
            add("zero_components", (r + 2.0, 0.25, -0.5), (-1.0, -0.0, 0.0))
            add("zero_components", (0.25, 0.0, -0.5), (0.0, 0.0, 1.0))           # from inside
            add("zero_components", (2.0, 2.5, 0.25), (-1.0, -1.0, 0.0))          # one zero component
            add("zero_components", (0.0, 2.0, 2.0), (-0.0, -1.0, -1.0))
            for _ in range(8):
                n = unit(rng.normal(size=3))
                grazing(add, rng, r * n, n, tangent(rng, n), size)
        elif kind == CUBOID:
            he = np.array(prm)
            for ax in range(3):
                for s in (1.0, -1.0):
                    for off in (0.25, 1.5):                                       # through the interior / beside the box
                        o = 0.25 * he * np.array([1.0, -1.0, 1.0]); o[ax] = s * (he[ax] + 2.0); o[(ax + 1) % 3] = off * he[(ax + 1) % 3]
                        d = np.zeros(3); d[ax] = -s
                        add("zero_components", o, d)
                d = np.full(3, -0.0); d[ax] = 1.0
                add("zero_components", 0.25 * he * np.array([1.0, 1.0, -1.0]), d)  # from inside, the zeros negative
                o = 0.25 * he; o[ax] = -(he[ax] + 2.0); d = np.array([0.0, -0.0, 0.0]); d[ax] = 1.0
                add("zero_components", o, d)
            add("zero_components", (3.0, 1.25, 0.25), (-1.0, -0.5, 0.0))          # one zero component: hits +x
            add("zero_components", (3.0, 1.25, 1.0), (-1.0, -0.5, -0.0))          # the same beside the slab of z: a miss
            add("zero_components", (0.25, 2.5, -2.25), (0.0, -1.0, 1.0))
            add("zero_components", (0.25, 0.125, -0.25), (0.5, 0.0, 1.0))         # from inside
            add("zero_components", (-0.5, -0.25, 0.5), (-1.0, 0.25, -0.0))
            corner = he.copy()
            for d in ((-1.0, -1.0, -1.0), (-1.0, -2.0, -0.5), (-0.25, -1.0, -0.5)):
                add("corner_edge", corner - 2.0 * np.array(d), d)                 # toi = 2 exactly
            for sgn in ((1.0, -1.0, 1.0), (-1.0, -1.0, -1.0)):
                c = he * np.array(sgn)
                add("corner_edge", c + 2.0 * np.array(sgn), -np.array(sgn))
            edge = np.array([he[0], he[1], 0.25 * he[2]])
            for d in ((-1.0, -1.0, 0.0), (-1.0, -2.0, 0.125), (-0.5, -0.25, -0.0)):
                add("corner_edge", edge - 2.0 * np.array(d), d)
            edge = np.array([-0.5 * he[0], he[1], -he[2]])
            add("corner_edge", edge - 4.0 * np.array((0.0, -1.0, 1.0)), (0.0, -1.0, 1.0))  # toi = 4
            for ax, s in ((0, 1.0), (1, -1.0), (2, 1.0)):
                for _ in range(4):
                    n = np.zeros(3); n[ax] = s
                    P = rng.uniform(-0.8, 0.8, 3) * he; P[ax] = s * he[ax]
                    grazing(add, rng, P, n, tangent(rng, n), size)
        else:
            hh, r = prm[0], prm[1]
            round_cases(kind, hh, r, add)
            k = r / (2.0 * hh)
            if kind in (CYLINDER, CAPSULE):
                near_axis_cases(hh, r, add)
                for _ in range(4):                                                # the lateral side
                    phi = rng.uniform(0, 2 * np.pi); n = np.array([np.cos(phi), 0.0, np.sin(phi)])
                    c = np.array([-np.sin(phi), 0.0, np.cos(phi)]); mix = rng.uniform(0.3, 1.0) * rng.choice([-1, 1])
                    u = unit(mix * c + np.sqrt(1 - mix * mix) * rng.choice([-1, 1]) * np.array([0.0, 1.0, 0.0]))
                    grazing(add, rng, r * n + np.array([0.0, rng.uniform(-0.8, 0.8) * hh, 0.0]), n, u, size)
            if kind == CYLINDER:
                for s in (1.0, -1.0):
                    for _ in range(4):                                            # the caps
                        phi, rho = rng.uniform(0, 2 * np.pi), rng.uniform(0, 0.8) * r
                        n = np.array([0.0, s, 0.0])
                        grazing(add, rng, (rho * np.cos(phi), s * hh, rho * np.sin(phi)), n, tangent(rng, n), size)
            if kind == CAPSULE:
                for s in (1.0, -1.0):
                    for _ in range(4):                                            # the hemispheres
                        n = unit(rng.normal(size=3)); n[1] = s * abs(n[1])
                        grazing(add, rng, np.array([0.0, s * hh, 0.0]) + r * n, n, tangent(rng, n), size)
                    # the seam circle |y| = hh between cylinder and hemisphere, and rays through one hemisphere only
                    add("seam", (r + 2.0, s * hh, 0.0), (-1.0, 0.0, 0.0))                       # toi = 2
                    add("seam", (r + 2.0, s * (hh + 2.0), 0.0), (-1.0, -s, 0.0))                # from the hemisphere's side, toi = 2
                    add("seam", (r + 2.0, s * (hh - 2.0), 0.0), (-1.0, s, 0.0))                 # from the cylinder's side, toi = 2
                    add("seam", (0.0, s * (hh - 1.0), -(r + 2.0)), (0.0, 0.5 * s, 1.0))         # toi = 2
                    add("seam", (0.6 * r + 1.2, s * hh, 0.8 * r + 1.6), (-0.6, 0.0, -0.8))
                    add("seam", (0.25 * r, s * hh, 0.0), (1.0, 0.0, 0.0))                       # from inside, in the seam's plane
                    add("hemisphere_only", (r + 2.0, s * (hh + 0.5 * r), 0.0), (-1.0, 0.0, 0.0))
                    add("hemisphere_only", (r + 2.0, s * (hh + 0.5 * r), 0.25 * r), (-1.0, -0.0, 0.0))
                    add("hemisphere_only", (2.0, s * (hh + 0.75 * r + 0.25), 0.125), (-1.0, -0.125 * s, 0.0))
                    add("hemisphere_only", (0.0, s * (hh + 0.5 * r), 0.125 * r), (1.0, 0.25 * s, 0.0))  # from inside the hemisphere, outward
                    add("hemisphere_only", (r + 2.0, s * (hh + 1.5 * r), 0.0), (-1.0, 0.0, 0.0))  # above it: a miss
            if kind == CONE:
                ik = 1.0 / k                                                      # 2 or 1: the generator through (r, -hh, 0) runs along (-1, 1/k, 0)
                apex = np.array([0.0, hh, 0.0])
                add("apex", (0.0, hh + 2.0, 0.0), (0.0, -1.0, 0.0))               # along the axis, toi = 2
                add("apex", (0.0, -hh - 2.0, 0.0), (0.0, 1.0, 0.0))               # through the base, leaves at the apex
                add("apex", (0.0, 0.0, 0.0), (0.0, 1.0, 0.0))
                for d in ((1.0, -4.0 * ik, 0.0), (-0.5, -2.0 * ik, 0.5), (0.0, -4.0, -1.0 * k)):
                    add("apex", apex - 2.0 * np.array(d), d)                      # obliquely, into the cone: toi = 2
                    add("apex", apex - 0.25 * np.array(d), -np.array(d))          # from inside, leaves through the apex
                add("apex", apex - 2.0 * np.array((1.0, -0.25 * ik, 0.0)), (1.0, -0.25 * ik, 0.0))  # touches the apex only: undecided
                inside = np.array([0.125, 0.0, 0.0625])
                c, zc = 0.25, 0.5
                ws = (c * c + zc * zc) / (2.0 * k * c)                            # the depth at which x = k w - c, z = zc meets the side
                entry = np.array([k * ws - c, hh - ws, zc])
                down, up = np.array([1.0, -ik, 0.0]), np.array([-1.0, ik, 0.0])
                add("generator_parallel", entry - 3.0 * down, down)               # from outside towards the base, toi = 3
                add("generator_parallel", inside, up)
                add("generator_parallel", inside, down)
                add("generator_parallel", inside, (-3.0, 5.0 * ik, -4.0))         # 9 + 16 = k^2 (5 / k)^2
                add("generator_parallel", inside, (3.0, -5.0 * ik, 4.0))
                add("generator_parallel", (k * -1.0 + 0.5, hh + 1.0, 0.0), down)  # beside the cone: a miss
                for d in (up, down):
                    add("generator_parallel", (k * 1.0, hh - 1.0, 0.5), d)        # B == 0: in the tangent plane of the double cone, a miss
                    add("generator_parallel", (k * 0.5, hh - 0.5, -0.25), d)
                add("steeper", (0.25 * r, hh + 2.0, 0.0), (0.0, -1.0, 0.0))       # A < 0, through the apex plane, then the side
                add("steeper", (0.125 * r, -hh - 2.0, 0.125 * r), (0.0, 1.0, 0.0))  # through the base
                for d in ((1.0, -4.0 * ik, 0.0), (-0.25, -2.0 * ik, 0.5)):
                    d = np.array(d)
                    add("steeper", np.array([0.0625, hh + 1.0, -0.125]) - 1.0 * d, d)
                    add("steeper", np.array([0.125 * r, -hh, 0.0625 * r]) + 2.0 * d, -d)  # through the base, upward
                    add("steeper", inside, d)
                    add("steeper", inside, -d)
                    add("steeper", np.array([1.5 * r, hh + 1.0, 0.0]), d * np.array([-1.0, 1.0, 1.0]))
                for e in OFFSETS:                                                 # the rays of the cancelling roots
                    add("near_generator", inside, (-1.0, ik * (1.0 + e), 0.0))
                    add("near_generator", inside, (1.0, -ik * (1.0 + e), 0.0))
                    add("near_generator", inside, (-3.0, 5.0 * ik * (1.0 + e), -4.0))
                    add("near_generator", entry - 3.0 * down, (1.0, -ik * (1.0 + e), 0.0))
                n_side = lambda phi: np.array([np.cos(phi), k, np.sin(phi)]) / np.sqrt(1.0 + k * k)
                gen = lambda phi: unit([k * np.cos(phi), -1.0, k * np.sin(phi)])
                for _ in range(6):                                                # the side
                    phi, w = rng.uniform(0, 2 * np.pi), rng.uniform(0.3, 0.8) * 2.0 * hh
                    cdir = np.array([-np.sin(phi), 0.0, np.cos(phi)]); mix = rng.uniform(0.3, 1.0) * rng.choice([-1, 1])
                    u = unit(mix * cdir + np.sqrt(1 - mix * mix) * rng.choice([-1, 1]) * gen(phi))
                    grazing(add, rng, (k * w * np.cos(phi), hh - w, k * w * np.sin(phi)), n_side(phi), u, size)
                for _ in range(4):                                                # the base
                    phi, rho = rng.uniform(0, 2 * np.pi), rng.uniform(0, 0.8) * r
                    n = np.array([0.0, -1.0, 0.0])
                    grazing(add, rng, (rho * np.cos(phi), -hh, rho * np.sin(phi)), n, tangent(rng, n), size)
                for s in (1.0, -1.0):                                             # along a generator, 1e-12 off it
                    for _ in range(3):
                        phi, w = rng.uniform(0, 2 * np.pi), rng.uniform(0.3, 0.8) * 2.0 * hh
                        cdir = np.array([-np.sin(phi), 0.0, np.cos(phi)])
                        u = unit(s * gen(phi) + 1e-12 * cdir)
                        grazing(add, rng, (k * w * np.cos(phi), hh - w, k * w * np.sin(phi)), n_side(phi), u, size,
                                "cone_generator_skim_miss", "cone_generator_skim_hit")
    return out


def main():
    rng = np.random.default_rng(0x44454745)  # "DEGE"
    cases = build_cases(rng)
    R64 = np.array([[float(v) for v in row] for row in rodrigues([mpf(c) for c in W_ROTATED])])
    jobs, meta = [], []
    for kind, prm, cls, o, d, margin in cases:
        t = np.array(T_IDENTITY)
        o_w = o + t
        if "grazing" not in cls and "skim" not in cls and 0.6 not in np.abs(d):  # (the random points and the 3-4-5 unit directions are not dyadic)
            assert np.array_equal(o_w - t, o), (cls, o)  # the translation is exact: the local ray IS the one written down
        jobs.append((kind, prm, T_IDENTITY, (0.0, 0.0, 0.0), tuple(o_w), tuple(d)))
        meta.append((cls, margin))
        jobs.append((kind, prm, T_ROTATED, W_ROTATED, tuple(R64 @ o + np.array(T_ROTATED)), tuple(R64 @ d)))
        meta.append((cls + "/rot", margin))
    with Pool(int(sys.argv[1]) if len(sys.argv) > 1 else (os.cpu_count() or 4)) as pool:
        solved = pool.map(solve_case, jobs, chunksize=4)
    rows, classes = [], []
    for (kind, prm, t, w, o_w, d_w), (cls, margin), (hit, toi, inside, gmin, well) in zip(jobs, meta, solved):
        if cls.startswith("near_generator") and kind == CONE:
            assert well, ("a near-generator ray from well inside / far outside must be well conditioned", cls, o_w, d_w)
        for solid in (0.0, 1.0):
            rows.append([kind] + list(prm) + list(t) + list(w) + [solid] + list(o_w) + list(d_w) +
                        [float(hit), 0.0 if (solid and inside) else toi, float(inside), gmin, max(prm), float(well), margin])
            classes.append(cls)
    a = np.array(rows, dtype=np.float64)
    classes = np.array(classes)
    assert a.shape[1] == len(COLUMNS)
    np.savez_compressed(os.path.join(HERE, "kat_degenerate.npz"), cases=a, classes=classes, columns=np.array(COLUMNS))
    print("wrote", a.shape)
    print("COUNTS = {  # (shape, class): (rows, hits, well conditioned)")
    for kind in sorted(NAMES):
        for cls in sorted(set(classes[a[:, 0] == kind])):
            m = (a[:, 0] == kind) & (classes == cls)
            print('    ("%s", "%s"): (%d, %d, %d),' % (NAMES[kind], cls, m.sum(), int(a[m, 17].sum()), int(a[m, 22].sum())))
    print("}")


if __name__ == "__main__":
    main()
