// nearest_kernel.h — k_nearest_points: the nearest surface to caller-supplied points (nrays_nearest_points_device; the definition is in include/nrays_abi.h and
// restated bit for bit by restated.py: nearest_points_ref).  One lane per point.  The walk is distance-pruned, not slab-pruned, so it shares nothing with traverse() but the
// records, the Stack and the five-comparator network: per node a lower bound of the squared distance from the point to each child's box (nearest_box_bound), the
// children ordered by it, the nearest entered and the others deferred, a child skipped iff nearest_skips(bound, margin, best).  Planes are visited FIRST: their closed
// form tightens the bound before the TLAS is entered.  The stack is Stack as it is (one-dword refs): a node step pushes at most three refs and a BLAS visit one sentinel,
// which is the rule derive_scene_facts sizes the spill region by (the planes are not pushed here).  An entry pushed before the bound shrank is re-culled when it is popped
// only through its children's bounds (a node) or not at all (a leaf: its triangles are tested); DESIGN §"Nearest-surface queries".
// Only the winner's (d2, key, instance, triangle slot) are carried through the walk; its record is rebuilt once at the end.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/nrays_abi.h"
#include "trace_device.h"

#ifndef NRAYS_NEAREST_WAVES
#define NRAYS_NEAREST_WAVES 2 // second __launch_bounds__ argument of k_nearest_points, as the other traversal kernels of the batch families
#endif

namespace nrays {

// ---- the bound and the cull -------------------------------------------------------------------------------------------------------------------------------------
// A lower bound of the exact squared distance from p to the box [mn, mx] (f32 bounds, widened exactly): per axis the gap max(mn - p, p - mx, 0) — one rounding, the
// operands are exact —, the squares summed left to right (five roundings on the way: a factor below 1 + 2^-50 in all), scaled by 1 - 2^-50; a sum that overflowed counts
// as DBL_MAX, a bound below 1e-290 (where squares may have lost their low bits to underflow) as 0.  A NaN coordinate leaves no gap on its axis.
NR_DEV double nearest_box_bound(d3 p, float mnx, float mny, float mnz, float mxx, float mxy, float mxz) {
    const double gx = fmax(fmax((double)mnx - p.x, p.x - (double)mxx), 0.0);
    const double gy = fmax(fmax((double)mny - p.y, p.y - (double)mxy), 0.0);
    const double gz = fmax(fmax((double)mnz - p.z, p.z - (double)mxz), 0.0);
    const double s = fmin((gx * gx + gy * gy) + gz * gz, kDblMax);
    const double b = s * 0.99999999999999911182158029987; // 1 - 2^-50
    return b < 1e-290 ? 0.0 : b;
}
// The margin of a bound: 2^-38 (bound + scale2), scale2 = (max |p_k| + the scene's coordinate bound)^2.  Derivation: DESIGN §"Nearest-surface queries".
NR_DEV double nearest_margin(double bound, double scale2) { return 3.637978807091713e-12 * (bound + scale2); } // 2^-38
// A box is skipped iff its bound, less its margin, lies ABOVE the best key so far: equal bounds are visited (the tie-break), and a NaN (inf - inf) skips nothing.
NR_DEV bool nearest_skips(double bound, double margin, double best) { return bound - margin > best; }

// ---- closest points ---------------------------------------------------------------------------------------------------------------------------------------------
NR_DEV double dist2(d3 p, d3 q) { const d3 e = p - q; return (e.x * e.x + e.y * e.y) + e.z * e.z; }

NR_DEV double clamp01(double t) { return t >= 0.0 ? (t <= 1.0 ? t : 1.0) : 0.0; } // (a NaN, from an edge of length 0, is 0: the edge's first corner)
// Ericson, Real-Time Collision Detection §5.1.5, in its order and with its comparisons.  (v, w): the barycentric weights of b and c.
NR_DEV d3 tri_closest(d3 a, d3 b, d3 c, d3 p, double& v, double& w) {
    const d3 ab = b - a, ac = c - a, ap = p - a;
    const double d1 = dot(ab, ap), d2 = dot(ac, ap);
    if (d1 <= 0.0 && d2 <= 0.0) { v = 0.0; w = 0.0; return a; }
    const d3 bp = p - b;
    const double d3_ = dot(ab, bp), d4 = dot(ac, bp);
    if (d3_ >= 0.0 && d4 <= d3_) { v = 1.0; w = 0.0; return b; }
    const double vc = d1 * d4 - d3_ * d2;
    if (vc <= 0.0 && d1 >= 0.0 && d3_ <= 0.0) { v = d1 / (d1 - d3_); w = 0.0; return a + ab * v; }
    const d3 cp = p - c;
    const double d5 = dot(ab, cp), d6 = dot(ac, cp);
    if (d6 >= 0.0 && d5 <= d6) { v = 0.0; w = 1.0; return c; }
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) { w = d2 / (d2 - d6); v = 0.0; return a + ac * w; }
    const double va = d3_ * d6 - d5 * d4;
    if (va <= 0.0 && (d4 - d3_) >= 0.0 && (d5 - d6) >= 0.0) { w = (d4 - d3_) / ((d4 - d3_) + (d5 - d6)); v = 1.0 - w; return b + (c - b) * w; }
    // The projection falls inside, or the triangle is so thin that va, vb, vc are rounding noise (exactly collinear corners: their true value is 0 and the tests above
    // were decided by signs of noise).  So the interior point counts only with weights in range, and it competes with the three clamped edge projections, whose
    // parameters are already here: for a real triangle it wins, for a collinear one an edge holds the true closest point.  Strict <, in the order AB, AC, BC.
    const double den = (va + vb) + vc;
    v = vb / den; w = vc / den;
    d3 q = (a + ab * v) + ac * w;
    double best = (v >= 0.0 && w >= 0.0 && (1.0 - v) - w >= 0.0) ? dist2(p, q) : __longlong_as_double(0x7ff0000000000000ll);
    const double t1 = clamp01(d1 / (d1 - d3_)), t2 = clamp01(d2 / (d2 - d6)), t3 = clamp01((d4 - d3_) / ((d4 - d3_) + (d5 - d6)));
    const d3 q1 = a + ab * t1, q2 = a + ac * t2, q3 = b + (c - b) * t3;
    const double e1 = dist2(p, q1), e2 = dist2(p, q2), e3 = dist2(p, q3);
    if (e1 < best) { best = e1; q = q1; v = t1; w = 0.0; }
    if (e2 < best) { best = e2; q = q2; v = 0.0; w = t2; }
    if (e3 < best) { q = q3; v = 1.0 - t3; w = t3; }
    return q;
}

// An analytic shape's record in its local space: the closest point, the normal there (outside: (pl - ql) / |pl - ql|; inside or on the surface: the outward normal of
// the face that produced ql), the key, and whether pl lies strictly behind the surface.  15 dwords: returned in VGPRs.
struct NearRec { d3 q, n; double d2; uint32_t behind; };
NR_DEV double clampd(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }
// (rho, y) against the outline of a surface of revolution about local y; lifted back with (x / rho, z / rho), or (1, 0) on the axis.
NR_DEV void revolve(uint32_t kind, double hh, double r, double rho, double y, double& qr, double& qy, double& nr, double& ny, bool& behind) {
    if (kind == NRAYS_SHAPE_CYLINDER) { // the rectangle [0, r] x [-hh, hh]
        const double gs = r - rho, gc = hh - fabs(y);
        if (gs >= 0.0 && gc >= 0.0) { // inside or on it: the nearer face, the side among equals
            behind = gs > 0.0 && gc > 0.0;
            if (gs <= gc) { qr = r; qy = y; nr = 1.0; ny = 0.0; }
            else { qr = rho; qy = copysign(hh, y); nr = 0.0; ny = copysign(1.0, y); }
            return;
        }
        behind = false;
        qr = rho > r ? r : rho; qy = clampd(y, -hh, hh);
    } else if (kind == NRAYS_SHAPE_CAPSULE) { // the segment [-hh, hh] of the axis inflated by r
        const double yc = clampd(y, -hh, hh), ey = y - yc;
        const double len = sqrt(rho * rho + ey * ey);
        behind = len < r;
        if (len == 0.0) { nr = 1.0; ny = 0.0; } else { nr = rho / len; ny = ey / len; }
        qr = nr * r; qy = yc + ny * r;
        return;
    } else { // cone: the base segment (0, -hh) .. (r, -hh) and the slant segment (r, -hh) .. (0, hh): the apex is at +hh (cast_cone: ow = hh - y)
        const double up = y + hh, h2 = 2.0 * hh;
        const double br = rho > r ? r : rho, e0 = rho - br;
        const double db = e0 * e0 + up * up;
        const double t = clampd(((rho - r) * -r + up * h2) / (r * r + h2 * h2), 0.0, 1.0);
        const double sr = r + -r * t, sy = -hh + h2 * t;
        const double e1 = rho - sr, e2 = y - sy;
        const double ds = e1 * e1 + e2 * e2;
        const double f = (rho - r) * h2 + up * r; // which side of the slant: (2 hh, r) is its outward normal
        const bool base = db <= ds;
        qr = base ? br : sr; qy = base ? -hh : sy;
        behind = up > 0.0 && f < 0.0;
        if (up >= 0.0 && f <= 0.0) { // inside or on it: the face's own normal
            const double ln = sqrt(h2 * h2 + r * r);
            nr = base ? 0.0 : h2 / ln; ny = base ? -1.0 : r / ln;
            return;
        }
    }
    const double er = rho - qr, ey = y - qy, len = sqrt(er * er + ey * ey);
    nr = er / len; ny = ey / len;
}
NR_DEV NearRec nearest_shape(uint32_t kind, double p0, double p1, double p2, d3 pl) {
    NearRec o;
    if (kind == NRAYS_SHAPE_BALL) {
        const double len = sqrt((pl.x * pl.x + pl.y * pl.y) + pl.z * pl.z);
        if (len == 0.0) { o.q = D3(p0, 0.0, 0.0); o.n = D3(1.0, 0.0, 0.0); }
        else { o.q = pl * (p0 / len); o.n = pl / len; }
        o.behind = len < p0;
    } else if (kind == NRAYS_SHAPE_CUBOID) {
        const double g0 = p0 - fabs(pl.x), g1 = p1 - fabs(pl.y), g2 = p2 - fabs(pl.z);
        if (g0 >= 0.0 && g1 >= 0.0 && g2 >= 0.0) { // inside or on it: the nearest face, the lowest axis among equals
            const int ax = (g0 <= g1 && g0 <= g2) ? 0 : (g1 <= g2 ? 1 : 2);
            o.q = pl; o.n = D3(0.0, 0.0, 0.0);
            if (ax == 0) { o.q.x = copysign(p0, pl.x); o.n.x = copysign(1.0, pl.x); }
            else if (ax == 1) { o.q.y = copysign(p1, pl.y); o.n.y = copysign(1.0, pl.y); }
            else { o.q.z = copysign(p2, pl.z); o.n.z = copysign(1.0, pl.z); }
            o.behind = g0 > 0.0 && g1 > 0.0 && g2 > 0.0;
        } else {
            o.q = D3(clampd(pl.x, -p0, p0), clampd(pl.y, -p1, p1), clampd(pl.z, -p2, p2));
            o.n = (pl - o.q) / sqrt(dist2(pl, o.q));
            o.behind = 0u;
        }
    } else if (kind == NRAYS_SHAPE_PLANE) { // the half-space's boundary
        const d3 nrm = D3(p0, p1, p2);
        const double t = dot(nrm, pl);
        o.q = pl - nrm * t;
        o.behind = t < 0.0;
        o.n = o.behind ? -nrm : nrm;
    } else {
        const double rho = sqrt(pl.x * pl.x + pl.z * pl.z);
        const double cx = rho == 0.0 ? 1.0 : pl.x / rho, cz = rho == 0.0 ? 0.0 : pl.z / rho;
        double qr, qy, nr, ny; bool behind;
        revolve(kind, p0, p1, rho, pl.y, qr, qy, nr, ny, behind);
        o.q = D3(qr * cx, qy, qr * cz); o.n = D3(nr * cx, ny, nr * cz);
        o.behind = behind;
    }
    o.d2 = dist2(pl, o.q);
    return o;
}
// The query point in an instance's local space, with the shortcuts of the forward direction (nrays_surface_texels): p for an instance that does not move, p - T for one that
// does not turn.
NR_DEV d3 nearest_local(const Instance& in, uint32_t flags, d3 p) {
    if (flags & kInstNoXform) return p;
    Xform m; load_xform(in, m);
    return (flags & kInstIdentityRot) ? p - m.t : inv_rot(m, p - m.t);
}
__device__ __noinline__ NearRec nearest_analytic(GInstance inp, d3 p) {
    const auto& in = *inp;
    Xform m;
#pragma unroll
    for (int k = 0; k < 9; ++k) m.r[k] = in.rot[k];
    m.t = D3(in.trans[0], in.trans[1], in.trans[2]);
    const d3 pl = (in.flags & kInstNoXform) ? p : ((in.flags & kInstIdentityRot) ? p - m.t : inv_rot(m, p - m.t));
    return nearest_shape(in.kind, in.params[0], in.params[1], in.params[2], pl);
}

// ---- the walk ---------------------------------------------------------------------------------------------------------------------------------------------------
struct NearBest { double d2; unsigned long long key; uint32_t inst, prim; bool any; };

template <int FEAT>
NR_DEV void nearest_walk(const DScene& S, Stack& st, d3 p, double limit0, double scale2, NearBest& best) {
    constexpr bool kAnalytic = (FEAT & kFeatAnalytic) != 0, kMesh = (FEAT & kFeatMesh) != 0;
    best.d2 = __longlong_as_double(0x7ff0000000000000ll); best.key = ~0ULL; best.inst = 0u; best.prim = 0u; best.any = false;
    double lim = limit0; // what a box is culled against: the smaller of the caller's bound and the best key so far
    auto offer = [&](double d2, unsigned long long key, uint32_t inst, uint32_t prim) {
        if (d2 < best.d2 || (d2 == best.d2 && key < best.key)) { best.d2 = d2; best.key = key; best.inst = inst; best.prim = prim; best.any = true; lim = fmin(lim, d2); }
    };
    st.reset();
    if (kAnalytic) {
        for (uint32_t k = 0; k < S.num_planes; ++k) {
            const uint32_t at = (uint32_t)S.planes[k];
            const Instance& in = S.instances[at];
            offer(nearest_analytic((GInstance)&in, p).d2, (unsigned long long)(uint32_t)in.node_id << 32, at, 0u);
        }
    }
    d3 cp = p; // the point in the current (world or BLAS-local) space
    bool in_blas = false;
    uint32_t cur_inst = 0u;
    int32_t cur = S.closest_root;
    if (cur == kEmptyChild) cur = st.pop();
    for (;;) {
        while (cur >= 0) {
            const char* base = (const char*)S.nodes + ((size_t)(uint32_t)cur << 7);
            const float4 xl = *(const float4*)(base), xh = *(const float4*)(base + 16), yl = *(const float4*)(base + 64), yh = *(const float4*)(base + 96),
                         zl = *(const float4*)(base + 48), zh = *(const float4*)(base + 112);
            const int4 ch = *(const int4*)(base + 32);
            const float kMiss = __builtin_inff();
            auto key_of = [&](int32_t c, float mnx, float mny, float mnz, float mxx, float mxy, float mxz) -> float {
                if (c == kEmptyChild) return kMiss;
                const double b = nearest_box_bound(cp, mnx, mny, mnz, mxx, mxy, mxz);
                if (nearest_skips(b, nearest_margin(b, scale2), lim)) return kMiss;
                return (float)fmin(b, 3.0e38); // (the order only: finite, so that a far child is not taken for a culled one)
            };
            float k0 = key_of(ch.x, xl.x, yl.x, zl.x, xh.x, yh.x, zh.x), k1 = key_of(ch.y, xl.y, yl.y, zl.y, xh.y, yh.y, zh.y);
            float k2 = key_of(ch.z, xl.z, yl.z, zl.z, xh.z, yh.z, zh.z), k3 = key_of(ch.w, xl.w, yl.w, zl.w, xh.w, yh.w, zh.w);
            int32_t c0 = ch.x, c1 = ch.y, c2 = ch.z, c3 = ch.w;
#define NR_CSWAP(ka, ca, kb, cb) { bool sw = kb < ka; float tk = sw ? kb : ka; kb = sw ? ka : kb; ka = tk; int32_t tc = sw ? cb : ca; cb = sw ? ca : cb; ca = tc; }
            NR_CSWAP(k0, c0, k1, c1) NR_CSWAP(k2, c2, k3, c3) NR_CSWAP(k0, c0, k2, c2) NR_CSWAP(k1, c1, k3, c3) NR_CSWAP(k1, c1, k2, c2)
#undef NR_CSWAP
            if (k3 < kMiss) st.push(c3); // farthest first: the nearest deferred child is popped first
            if (k2 < kMiss) st.push(c2);
            if (k1 < kMiss) st.push(c1);
            cur = k0 < kMiss ? c0 : st.pop();
        }
        if (cur == kEmptyChild) break;
        if (kMesh && cur == kSentinel) { in_blas = false; cp = p; cur = st.pop(); continue; }
        const uint32_t lv = (uint32_t)~cur, first = lv >> 3, bits = lv & 7u;
        if (kMesh && in_blas) { // triangle leaf
            const float4* tq = (const float4*)(S.tris + first);
#pragma nounroll
            for (uint32_t k = 0; k <= bits; ++k, tq += 3) {
                const float4 t0 = tq[0], t1 = tq[1], t2 = tq[2];
                double v, w;
                const d3 q = tri_closest(D3(t0.x, t0.y, t0.z), D3(t1.x, t1.y, t1.z), D3(t2.x, t2.y, t2.z), cp, v, w);
                offer(dist2(cp, q), ((unsigned long long)__float_as_uint(t0.w) << 32) | __float_as_uint(t1.w), cur_inst, first + k);
            }
            cur = st.pop();
            continue;
        }
        if (kMesh && (!kAnalytic || (bits & kLeafMesh))) { // TLAS leaf: a BLAS
            cur_inst = first;
            const InstLink link = S.links[first];
            if (!(bits & kLeafNoXform)) cp = nearest_local(S.instances[first], link.flags, p);
            in_blas = true;
            st.push(kSentinel);
            cur = link.blas_root;
            if (cur == kEmptyChild) cur = st.pop();
            continue;
        }
        if (kAnalytic) {
            const Instance& in = S.instances[first];
            offer(nearest_analytic((GInstance)&in, p).d2, (unsigned long long)(uint32_t)in.node_id << 32, first, 0u);
        }
        cur = st.pop();
    }
}

// hit_flags bit 0 clear: the point is skipped — the miss record, its coordinates unread.  max_dist: NULL = unbounded; NaN or negative = a miss without a walk; the walk culls
// against max_dist^2 widened by 2^-48 (sqrt(d2) <= max_dist implies d2 below it), the answer is decided by sqrt(d2) <= max_dist alone.
template <int FEAT>
__global__ void __launch_bounds__(kBlock, NRAYS_NEAREST_WAVES) k_nearest_points(DScene S, uint32_t n, const double* __restrict__ points, const double* __restrict__ max_dist,
                                                                                 const uint32_t* __restrict__ hit_flags, double coord_bound, double* __restrict__ out_dist,
                                                                                 int32_t* __restrict__ out_node, double* __restrict__ out_point, double* __restrict__ out_normal,
                                                                                 double* __restrict__ out_uv, int32_t* __restrict__ out_prim, uint32_t* __restrict__ out_flags,
                                                                                 uint32_t* spill) {
    __shared__ uint32_t lds_stack[kLdsStack * kBlock];
    Stack st; st.setup(lds_stack, spill, nullptr);
    const double kInf = __longlong_as_double(0x7ff0000000000000ll);
    for (uint32_t base = blockIdx.x * kBlock; base < n; base += gridDim.x * kBlock) { // block-uniform trip count
        const uint32_t i = base + threadIdx.x;
        if (i >= n) continue;
        const size_t i3 = 3 * (size_t)i;
        bool found = false, has_uv = false, behind = false;
        double dist = kInf, u = 0.0, v = 0.0;
        d3 wp = D3(0.0, 0.0, 0.0), wn = D3(0.0, 0.0, 0.0);
        int32_t node = -1, prim = -1;
        const double md = max_dist ? max_dist[i] : kInf;
        if ((!hit_flags || (hit_flags[i] & 1u)) && md >= 0.0) {
            const d3 p = D3(points[i3], points[i3 + 1], points[i3 + 2]);
            const double scale = fmax(fmax(fabs(p.x), fabs(p.y)), fabs(p.z)) + coord_bound;
            NearBest best;
            nearest_walk<FEAT>(S, st, p, (md * md) * 1.0000000000000036 + 1e-300, scale * scale, best);
            if (best.any && sqrt(best.d2) <= md) { // the winner's record, rebuilt once
                found = true;
                dist = sqrt(best.d2);
                const Instance& in = S.instances[best.inst];
                Xform m; load_xform(in, m);
                const d3 pl = nearest_local(in, in.flags, p);
                d3 ql, nl;
                if ((FEAT & kFeatMesh) && (!(FEAT & kFeatAnalytic) || in.kind == NRAYS_SHAPE_TRIMESH)) {
                    const TriRec& tr = S.tris[best.prim];
                    const d3 a = D3(tr.v0[0], tr.v0[1], tr.v0[2]), b = D3(tr.v1[0], tr.v1[1], tr.v1[2]), c = D3(tr.v2[0], tr.v2[1], tr.v2[2]);
                    double bv, bw;
                    ql = tri_closest(a, b, c, pl, bv, bw);
                    const d3 cr = cross(b - a, c - a);
                    behind = dot(pl - a, cr) < 0.0;
                    nl = cr / norm(cr);
                    if (behind) nl = -nl;
                    node = (int32_t)tr.node_id; prim = (int32_t)tr.tri_id;
                    has_uv = (S.shade[tr.node_id].flags & 1u) != 0;
                    if (has_uv) {
                        const TriUv& t = S.triuvs[best.prim];
                        const double b0 = (1.0 - bv) - bw;
                        u = ((double)t.uv[0] * b0 + (double)t.uv[2] * bv) + (double)t.uv[4] * bw;
                        v = ((double)t.uv[1] * b0 + (double)t.uv[3] * bv) + (double)t.uv[5] * bw;
                    }
                } else {
                    const NearRec r = nearest_analytic((GInstance)&in, p);
                    ql = r.q; nl = r.n; behind = r.behind != 0u;
                    node = in.node_id;
                }
                if (in.flags & kInstNoXform) { wp = ql; wn = nl; }
                else if (in.flags & kInstIdentityRot) { wp = ql + m.t; wn = nl; }
                else { wp = rot(m, ql) + m.t; wn = rot(m, nl); }
                if ((FEAT & kFeatAnalytic) && in.kind == NRAYS_SHAPE_BALL) { // the ball cast's uv, from the world normal
                    has_uv = true;
                    u = 0.5 + atan2(wn.z, wn.x) / (kPi * 2.0);
                    v = 0.5 - asin(wn.y) / kPi;
                }
            }
        }
        out_dist[i] = dist;
        out_node[i] = node;
        if (out_point) { out_point[i3] = wp.x; out_point[i3 + 1] = wp.y; out_point[i3 + 2] = wp.z; }
        if (out_normal) { out_normal[i3] = wn.x; out_normal[i3 + 1] = wn.y; out_normal[i3 + 2] = wn.z; }
        if (out_uv) { out_uv[2 * (size_t)i] = u; out_uv[2 * (size_t)i + 1] = v; }
        if (out_prim) out_prim[i] = prim;
        if (out_flags) out_flags[i] = found ? (1u | (has_uv ? 2u : 0u) | (behind ? 4u : 0u)) : 0u;
    }
}

struct NearestLaunch {
    uint32_t grid; hipStream_t stream; const DScene* d; uint32_t n; const double* points; const double* max_dist; const uint32_t* hit_flags; double coord_bound;
    double* dist; int32_t* node; double* point; double* normal; double* uv; int32_t* prim; uint32_t* flags; uint32_t* spill;
};
bool launch_nearest_points(const NearestLaunch& a, int feat);
void launch_nearest_bound(uint32_t grid, hipStream_t stream, uint32_t n, uint32_t boxes, const double* points, const double* box, double* out);

} // namespace nrays
