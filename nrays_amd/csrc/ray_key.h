// ray_key.h — the spatial key a caller-ray batch is binned by when the caller says that its rays come in no useful order
// (NRAYS_RAYS_UNORDERED; ray_order.hip), and the quantisation frame the key is computed in.  Compiled into the device code
// (k_ray_bounds, k_ray_frame, k_ray_keys) and by the host compiler (tests/test_ray_order.py builds a shim around it), so that both
// give the same frame and the same keys bit for bit: f64 + - * / and integer arithmetic only, no libm call, -ffp-contract=off
// like everything else here (f64 + - * / agree between the host and gfx950).
//
// A key has kRayKeyBits (K) significant bits; the counting sort of ray_order.hip orders by the leading kRayBinBits (B):
//
//     [ octant, 3 bits ][ origin cell, up to 18 bits ][ direction cell, up to 18 bits ]   left-aligned in K = 39 bits
//
//   octant          the sign bits of the direction's x / y / z (what RayF::bits selects a node's planes by)
//   origin cell     Morton-like code of the ray's origin (clamped to the scene's bounding box) inside the bounds of the chunk's origins
//   direction cell  Morton-like code of the octahedral image (u, v) of the direction inside the bounds of the chunk's (u, v)
//
// The frame ADAPTS to the chunk: the bits of a field are dealt to its axes one by one, each to the axis whose cells are widest at that
// moment, so an axis without extent gets none and cells come out as square as powers of two allow.  A camera-like batch (one origin)
// has no origin field and its leading 21 bits are octant + 9 + 9 direction bits; an AO-like batch (origins all over a surface, the same
// direction distribution everywhere) leads with the octant and 18 origin bits.  The octant LEADS: with the origin cell first the waves of
// an AO batch touch half as many 8 x 8 grid tiles on the CPU count of tests/test_ray_order.py (4.6 against 9.3), but on the GPU the sponza
// stand-in's AO rays trace faster when a wave is uniform in its direction signs (a wave-uniform node visit is one scalar fetch only then):
// 4.24 against 4.43 ms hinted, 4.31 unhinted (profiles/ray_order_octant.log).  NR_RAY_KEY_OCTANT_FIRST=0 builds the other layout.
//
// Total for every bit pattern: NaN, infinities, a zero direction, an empty or zero-volume frame all give SOME key below 2^K — every
// float-to-integer conversion is of a value clamped into range first.  Non-finite origins / directions do not enter the bounds.
#pragma once
#include <stdint.h>

#ifndef NR_RAY_KEY_OCTANT_FIRST
#define NR_RAY_KEY_OCTANT_FIRST 1 // 0: [origin cell][octant][direction cell] — a tighter footprint, waves of mixed direction signs (A/B builds)
#endif
#if defined(__HIPCC__)
#define NR_RK_FN __host__ __device__ inline
#else
#define NR_RK_FN inline
#endif

namespace nrays {

constexpr int kRayKeyOriginBits = 18; // bits dealt to the origin axes that have extent
constexpr int kRayKeyDirBits = 18;    // ... to u and v
constexpr int kRayKeyAxisBits = 16;   // at most so many per axis
constexpr int kRayKeyBits = kRayKeyOriginBits + 3 + kRayKeyDirBits; // K
constexpr int kRayBinBits = 21;                                     // B: the counting sort's bins
// The frame as a flat array of doubles (NRAYS_RAY_FRAME_DOUBLES of include/nrays_abi.h):
//   [0..2] origin min xyz, [3..5] origin max, [6..7] (u, v) min, [8..9] (u, v) max,
//   [10] origin bits dealt, [11] their axes, two bits each, the key's most significant bit first in the lowest two,
//   [12] / [13] the same for (u, v), [14..19] the scene's bounding box the origins were clamped to (min xyz, max xyz; as the handle holds it).
constexpr int kRayFrameDoubles = 20;

NR_RK_FN uint64_t rk_bits(double x) { uint64_t u; __builtin_memcpy(&u, &x, 8); return u; }
NR_RK_FN bool rk_finite(double x) { return (rk_bits(x) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }
NR_RK_FN double rk_abs(double x) { return x < 0.0 ? 0.0 - x : x + 0.0; } // (never -0)

// Octahedral image of a direction: p = d / (|dx| + |dy| + |dz|), the lower half (z < 0) folded outward.  u, v in [-1, 1].
// false: a non-finite or zero direction (or one whose 1-norm overflows) — it gets u = v = 0 and stays out of the bounds.
NR_RK_FN bool rk_dir_uv(const double d[3], double& u, double& v) {
    u = 0.0; v = 0.0;
    if (!rk_finite(d[0]) || !rk_finite(d[1]) || !rk_finite(d[2])) return false;
    const double l1 = rk_abs(d[0]) + rk_abs(d[1]) + rk_abs(d[2]);
    if (!rk_finite(l1) || !(l1 > 0.0)) return false;
    const double px = d[0] / l1, py = d[1] / l1;
    if (d[2] < 0.0) {
        const double fu = 1.0 - rk_abs(py), fv = 1.0 - rk_abs(px);
        u = px < 0.0 ? 0.0 - fu : fu; v = py < 0.0 ? 0.0 - fv : fv;
    } else { u = px; v = py; }
    u = u + 0.0; v = v + 0.0; // -0 -> +0: min / max of the bounds must not depend on the order
    return true;
}

// Bounds of a set of rays: [0..2] origins, [3..4] (u, v).  min / max are exact and order-free.
struct RayBounds { double lo[5], hi[5]; };
NR_RK_FN void rk_bounds_init(RayBounds& b) { for (int k = 0; k < 5; ++k) { b.lo[k] = __builtin_huge_val(); b.hi[k] = -__builtin_huge_val(); } }
NR_RK_FN void rk_bounds_merge(RayBounds& b, const RayBounds& o) {
    for (int k = 0; k < 5; ++k) { b.lo[k] = o.lo[k] < b.lo[k] ? o.lo[k] : b.lo[k]; b.hi[k] = o.hi[k] > b.hi[k] ? o.hi[k] : b.hi[k]; }
}
// box: the scene's bounding box {min xyz, max xyz}; an axis of it that is empty or not finite does not clamp.
NR_RK_FN void rk_bounds_add(RayBounds& b, const double o[3], const double d[3], const double box[6]) {
    if (rk_finite(o[0]) && rk_finite(o[1]) && rk_finite(o[2])) {
        for (int a = 0; a < 3; ++a) {
            double x = o[a] + 0.0;
            if (rk_finite(box[a]) && rk_finite(box[3 + a]) && box[a] <= box[3 + a]) x = x < box[a] ? box[a] + 0.0 : (x > box[3 + a] ? box[3 + a] + 0.0 : x);
            b.lo[a] = x < b.lo[a] ? x : b.lo[a]; b.hi[a] = x > b.hi[a] ? x : b.hi[a];
        }
    }
    double uv[2];
    if (rk_dir_uv(d, uv[0], uv[1])) for (int k = 0; k < 2; ++k) { b.lo[3 + k] = uv[k] < b.lo[3 + k] ? uv[k] : b.lo[3 + k]; b.hi[3 + k] = uv[k] > b.hi[3 + k] ? uv[k] : b.hi[3 + k]; }
}

// Deals `total` bits to `axes` axes of extents ext[]: each to the axis whose cells are widest (the first of equals), halving them.
// Returns the number dealt (fewer than `total` only when no axis with extent has room left); code: the axes, two bits each.
NR_RK_FN int rk_deal_bits(const double* ext, int axes, int total, uint64_t& code) {
    double cell[3] = {0.0, 0.0, 0.0}; int nb[3] = {0, 0, 0};
    for (int a = 0; a < axes; ++a) cell[a] = ext[a];
    code = 0; int n = 0;
    for (; n < total; ++n) {
        int best = -1;
        for (int a = 0; a < axes; ++a) if (cell[a] > 0.0 && nb[a] < kRayKeyAxisBits && (best < 0 || cell[a] > cell[best])) best = a;
        if (best < 0) break;
        code |= (uint64_t)best << (2 * n); cell[best] = cell[best] * 0.5; ++nb[best];
    }
    return n;
}

NR_RK_FN void rk_frame_finish(const RayBounds& b, const double box[6], double frame[kRayFrameDoubles]) {
    double ext[5];
    for (int k = 0; k < 5; ++k) {
        double lo = b.lo[k], hi = b.hi[k];
        if (!(lo <= hi)) { lo = 0.0; hi = 0.0; } // no finite ray contributed
        const int at = k < 3 ? k : 6 + (k - 3), span = k < 3 ? 3 : 2;
        frame[at] = lo; frame[at + span] = hi; ext[k] = hi - lo; // (may overflow to +inf: still a valid extent)
    }
    uint64_t oc, dc;
    const int no = rk_deal_bits(ext, 3, kRayKeyOriginBits, oc), nd = rk_deal_bits(ext + 3, 2, kRayKeyDirBits, dc);
    frame[10] = (double)no; frame[11] = (double)oc; frame[12] = (double)nd; frame[13] = (double)dc; // (codes < 2^36: exact)
    for (int k = 0; k < 6; ++k) frame[14 + k] = box[k];
}

// x inside [lo, hi] -> a cell index of `bits` bits; NaN -> 0, outside -> the nearest end.
NR_RK_FN uint32_t rk_quantise(double x, double lo, double hi, int bits) {
    if (bits <= 0) return 0u;
    double t = (x - lo) / (hi - lo);
    t = t > 0.0 ? t : 0.0; // (NaN -> 0)
    t = t < 1.0 ? t : 1.0;
    const uint32_t top = (1u << bits) - 1u;
    const uint32_t q = (uint32_t)(t * (double)(1u << bits)); // in [0, 2^16]: defined
    return q > top ? top : q;
}
// Interleaves n bits of q[0..2] in the order of `code`, most significant first.
NR_RK_FN uint64_t rk_interleave(uint32_t q0, uint32_t q1, uint32_t q2, int r0, int r1, int r2, int n, uint64_t code) {
    uint64_t key = 0;
    for (int s = 0; s < n; ++s) {
        const uint32_t a = (uint32_t)(code >> (2 * s)) & 3u;
        uint32_t bit;
        if (a == 0u) { --r0; bit = (q0 >> r0) & 1u; } else if (a == 1u) { --r1; bit = (q1 >> r1) & 1u; } else { --r2; bit = (q2 >> r2) & 1u; }
        key = (key << 1) | bit;
    }
    return key;
}
NR_RK_FN void rk_axis_bits(int n, uint64_t code, int nb[3]) {
    int n0 = 0, n1 = 0, n2 = 0; // (no indexed store: the counts stay in registers on the device)
    for (int s = 0; s < n; ++s) { const uint32_t a = (uint32_t)(code >> (2 * s)) & 3u; n0 += a == 0u; n1 += a == 1u; n2 += a >= 2u; }
    nb[0] = n0; nb[1] = n1; nb[2] = n2;
}
// What a key computation needs of a frame, decoded once (wave-uniform on the device).
struct RayKeyFrame { double lo[5], hi[5]; int no, nd, ob[3], db[3]; uint64_t oc, dc; };
NR_RK_FN void rk_frame_decode(const double frame[kRayFrameDoubles], RayKeyFrame& f) {
    for (int a = 0; a < 3; ++a) { f.lo[a] = frame[a]; f.hi[a] = frame[3 + a]; }
    for (int k = 0; k < 2; ++k) { f.lo[3 + k] = frame[6 + k]; f.hi[3 + k] = frame[8 + k]; }
    // (the library wrote these four: small non-negative integers; anything else decodes to "no bits")
    const double no = frame[10], nd = frame[12], oc = frame[11], dc = frame[13];
    f.no = no >= 0.0 && no <= (double)kRayKeyOriginBits ? (int)no : 0; f.nd = nd >= 0.0 && nd <= (double)kRayKeyDirBits ? (int)nd : 0;
    f.oc = oc >= 0.0 && oc < 68719476736.0 ? (uint64_t)oc : 0ull; f.dc = dc >= 0.0 && dc < 68719476736.0 ? (uint64_t)dc : 0ull;
    rk_axis_bits(f.no, f.oc, f.ob); rk_axis_bits(f.nd, f.dc, f.db);
}
NR_RK_FN uint32_t rk_octant(const double d[3]) { return (uint32_t)(rk_bits(d[0]) >> 63) | ((uint32_t)(rk_bits(d[1]) >> 63) << 1) | ((uint32_t)(rk_bits(d[2]) >> 63) << 2); }
NR_RK_FN uint64_t rk_key(const RayKeyFrame& f, const double o[3], const double d[3]) {
    const uint64_t ok = rk_interleave(rk_quantise(o[0], f.lo[0], f.hi[0], f.ob[0]), rk_quantise(o[1], f.lo[1], f.hi[1], f.ob[1]), rk_quantise(o[2], f.lo[2], f.hi[2], f.ob[2]),
                                      f.ob[0], f.ob[1], f.ob[2], f.no, f.oc);
    double u, v;
    (void)rk_dir_uv(d, u, v);
    const uint64_t dk = rk_interleave(rk_quantise(u, f.lo[3], f.hi[3], f.db[0]), rk_quantise(v, f.lo[4], f.hi[4], f.db[1]), 0u, f.db[0], f.db[1], 0, f.nd, f.dc);
#if NR_RAY_KEY_OCTANT_FIRST
    const uint64_t key = (((((uint64_t)rk_octant(d)) << f.no) | ok) << f.nd) | dk;
#else
    const uint64_t key = (((ok << 3) | (uint64_t)rk_octant(d)) << f.nd) | dk;
#endif
    return key << (kRayKeyBits - f.no - 3 - f.nd);
}
// The octant field of a key computed in frame f (tests).
NR_RK_FN uint32_t rk_key_octant(const RayKeyFrame& f, uint64_t key) { return (uint32_t)(key >> (kRayKeyBits - (NR_RAY_KEY_OCTANT_FIRST ? 0 : f.no) - 3)) & 7u; }

} // namespace nrays
