// frame_path.hip — one frame of a handle: the small kernels around k_primary, the per-camera scheduling state, pipelined frames, and
// render_impl, the driver over those phases.
//
// Launch structure of one nrays_render (replaces scene::render, src/scene.rs:29-116):
//   k_tile_order     mesh scenes, from the second frame of a geometry on: wave tiles sorted by the previous frame's
//               per-tile cost (8 LDS counting sorts), so that the deep chains start first.
//   k_primary   persistent grid; one lane per pixel of an 8x8 wave tile, looping over the AA samples of the batch:
//               raygen -> [no ray of the tile passes the root box: background] -> closest hit -> Phong + shadow
//               rays -> continuation kept in registers (trace_chain) -> pixel write.  Only the second child of a
//               hit that spawns a reflection AND a refraction goes to the compacted HBM queue (wave ballots).
//   k_bounce    rounds over that queue (double-branching scenes only; bounce.hip), then k_fold_fixed.
//   k_resolve   divides by ray_per_pixel when it is > 1 (scene.rs:94).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/nrays_abi.h"
#include "bounce.h"
#include "device_types.h"
#include "primary_kernel.h"
#include "scene_build.h"
#include "scene_handle.h"
#include "tile_device.h"
#include "trace_device.h"
#include "wavefront.h"

namespace nrays {

// Wave tiles in descending order of last frame's cost.  XCD x's work list is the subset { i : i mod 8 == x } of the
// wave tiles (a uniform sample of the image), sorted by workgroup x with a 256-bucket counting sort in LDS
// on (exponent, 3 mantissa bits) of the cycle counts — an approximate order is all a work queue needs.
// Entry k of list x is stored at order[8 k + x].
__device__ __forceinline__ uint32_t cost_bucket(uint32_t c) {
    if (c == 0u) return 0u;
    uint32_t e = 31u - (uint32_t)__clz((int)c);
    uint32_t m = e >= 3u ? (c >> (e - 3u)) & 7u : (c << (3u - e)) & 7u;
    return e * 8u + m;
}
// Light-parallel tiles (split_lsl > 0, multi-light mesh frames): a tile whose cost exceeds split_factor x the frame's work per
// resident wave (its list's sum x 8 / waves: the lists are uniform samples of the image) would sit on the frame's critical path —
// it enters the list as 2^split_lsl entries (its parts, DRender::light_lsl), each priced at a third of the tile.  split_factor < 0
// splits every tile (tests).  order_len[x] receives the list's length.
// clear != 0: every cost is zeroed after its last read here — the frame that follows records into split entries by atomicMax, and a memset of its own
// would be one more launch between this kernel and k_primary.
__global__ void __launch_bounds__(1024) k_tile_order(uint32_t* __restrict__ cost, uint32_t* __restrict__ order, uint32_t n, unsigned long long* stats,
                                                     uint32_t split_lsl, float split_factor, uint32_t waves, uint32_t* __restrict__ order_len, uint32_t clear, float split_hyst) {
    __shared__ uint32_t hist[256];
    __shared__ unsigned long long wg_sum;
    __shared__ uint32_t wg_max, wg_total;
    const uint32_t x = blockIdx.x; // 0..7
    if (threadIdx.x < 256u) hist[threadIdx.x] = 0u;
    if (threadIdx.x == 0u) { wg_sum = 0ULL; wg_max = 0u; wg_total = 0u; }
    __syncthreads();
    unsigned long long my_sum = 0ULL; uint32_t my_max = 0u;
    for (uint32_t i = x + 8u * threadIdx.x; i < n; i += 8u * 1024u) { const uint32_t c = cost[i] & kCostMask; my_sum += c; my_max = c > my_max ? c : my_max; }
    if (stats || split_lsl) { // stats[2x] = sum of list x's tile costs, stats[2x + 1] = its largest one (both in the 16-cycle units of the cost array)
        if (my_sum) atomicAdd(&wg_sum, my_sum);
        if (my_max) atomicMax(&wg_max, my_max);
    }
    __syncthreads();
    if (stats && threadIdx.x == 0u) { stats[2u * x] = wg_sum; stats[2u * x + 1u] = (unsigned long long)wg_max; } // per list: no memset before the launch, the host adds them up
    const double per_wave = (double)(wg_sum * 8ULL) / (double)(waves ? waves : 1u);
    const unsigned long long thr = !split_lsl ? ~0ULL : (split_factor < 0.0f ? 0ULL : (unsigned long long)(split_factor * per_wave));
    const unsigned long long thr_keep = !split_lsl ? ~0ULL : (split_factor < 0.0f ? 0ULL : (unsigned long long)(split_factor * split_hyst * per_wave)); // a tile that ran in parts stays split down to here
    const uint32_t parts = 1u << split_lsl;
    auto heavy = [&](uint32_t rec) { const uint32_t c = rec & kCostMask; return split_lsl != 0u && (unsigned long long)c >= ((rec & kCostSplit) ? thr_keep : thr) && (split_factor < 0.0f || c != 0u); };
    for (uint32_t i = x + 8u * threadIdx.x; i < n; i += 8u * 1024u) {
        const uint32_t rec = cost[i], c = rec & kCostMask;
        if (heavy(rec)) atomicAdd(&hist[cost_bucket(c / 3u)], parts); else atomicAdd(&hist[cost_bucket(c)], 1u);
    }
    __syncthreads();
    if (threadIdx.x == 0) { // exclusive prefix, most expensive bucket first
        uint32_t acc = 0u;
        for (int b = 255; b >= 0; --b) { uint32_t c = hist[b]; hist[b] = acc; acc += c; }
        wg_total = acc;
    }
    __syncthreads();
    for (uint32_t i = x + 8u * threadIdx.x; i < n; i += 8u * 1024u) {
        const uint32_t rec = cost[i], c = rec & kCostMask;
        if (heavy(rec)) {
            const uint32_t at = atomicAdd(&hist[cost_bucket(c / 3u)], parts);
            for (uint32_t s = 0; s < parts; ++s) order[8u * (at + s) + x] = i | (s << 28) | kEntrySplit;
        } else order[8u * atomicAdd(&hist[cost_bucket(c)], 1u) + x] = i;
        if (clear) cost[i] = 0u;
    }
    if (order_len && threadIdx.x == 0u) order_len[x] = wg_total;
}

// A first guess of the wave-tile costs of a camera that has no history yet (the reference's caller renders every camera ONCE,
// examples/loader3d.rs:67-93: the first frame is the one that counts for it).  A mesh frame is as long as its deepest chains, and a
// chain is deep where the primary ray crosses many nodes that can continue it — alpha-mapped / transparent layers (scene.rs:229) and
// mirrors (scene.rs:204).  cost = 1 + 4 x (boxes of such nodes the ray through the tile's centre pixel crosses), f32 slab tests against
// their world AABBs: a few microseconds, and k_tile_order then starts those tiles first, as it does from recorded costs on later
// frames.  Scheduling only: pixels do not depend on it.
__global__ void k_seed_costs(DRender R, const float* __restrict__ boxes, uint32_t nboxes, uint32_t* __restrict__ cost, uint32_t nwt, uint32_t nrays) {
    const uint32_t wt = blockIdx.x * blockDim.x + threadIdx.x;
    if (wt >= nwt) return;
    const uint32_t tile = wt >> 2, sub = wt & 3u;
    const uint32_t tx = R.win_x0 + tile % R.win_nx, ty = R.win_y0 + tile / R.win_nx;
    uint32_t n = 0u;
    for (uint32_t q = 0; q < nrays; ++q) { // the tile's centre pixel, or the centres of its four quadrants
        const uint32_t px = nrays == 1u ? 4u : 2u + 4u * (q & 1u), py = nrays == 1u ? 4u : 2u + 4u * (q >> 1);
        const uint32_t i = tx * kTile + ((sub & 1u) << 3) + px, rl = ty * kTile + ((sub >> 1) << 3) + py;
        uint32_t j = rl;
        if (R.band_rows != 0 && R.band_owners > 1) j = ((rl / R.band_rows) * R.band_owners + R.band_owner) * R.band_rows + (rl % R.band_rows);
        const double dx = ((double)i / (double)R.width - 0.5) * 2.0, dy = -((double)j / (double)R.height - 0.5) * 2.0;
        double h[4];
        for (int r = 0; r < 4; ++r) h[r] = R.m[r] * dx + R.m[4 + r] * dy - R.m[8 + r] + R.m[12 + r];
        const float ox = (float)R.eye[0], oy = (float)R.eye[1], oz = (float)R.eye[2];
        const float ix = 1.0f / (float)(h[0] / h[3] - R.eye[0]), iy = 1.0f / (float)(h[1] / h[3] - R.eye[1]), iz = 1.0f / (float)(h[2] / h[3] - R.eye[2]);
        for (uint32_t b = 0; b < nboxes; ++b) {
            const float* bx = boxes + 6u * b;
            float t0 = (bx[0] - ox) * ix, t1 = (bx[3] - ox) * ix; float lo = fminf(t0, t1), hi = fmaxf(t0, t1);
            t0 = (bx[1] - oy) * iy; t1 = (bx[4] - oy) * iy; lo = fmaxf(lo, fminf(t0, t1)); hi = fminf(hi, fmaxf(t0, t1));
            t0 = (bx[2] - oz) * iz; t1 = (bx[5] - oz) * iz; lo = fmaxf(lo, fminf(t0, t1)); hi = fminf(hi, fmaxf(t0, t1));
            n += (hi >= fmaxf(lo, 0.0f)) ? 1u : 0u;
        }
    }
    cost[wt] = 1u + (nrays == 1u ? 4u : 1u) * n;
}

// Screen bounds of the scene for one camera: the pixel rectangle outside of which no primary ray can reach the scene's
// bounding box, so that k_primary can write the background for whole wave tiles without generating their rays.
// Raygen (generate_primary, scene.rs:74-89) sends the ray of sample position (ox, oy) from `eye` through
// P = h.xyz / h.w with h = M (dx, dy, -1, 1), dx = (ox / W - 0.5) 2, dy = -(oy / H - 0.5) 2; its direction is a positive
// multiple of sgn(h.w) D(dx, dy), D = h.xyz - eye h.w = Dc + dx Dx + dy Dy — AFFINE in (dx, dy).  A corner c of the
// box lies on the ray of (dx, dy) iff c - eye = a Dc + b Dx + g Dy with dx = b / a, dy = g / a and a sgn > 0 (in front).
// If that holds for all eight corners, every point of the box is a combination of the corners with weights of one sign,
// so its (dx, dy) lies between the corners' extremes: rays outside that rectangle miss the box, hence every node, hence
// return the background; a box entirely behind the eye is missed by every ray.  Everything else — a corner beside the eye, h.w changing sign over the frame, a
// degenerate matrix, planes in the scene — gives "every pixel may hit".  Two pixels of slack plus the jitter window
// cover the rounding of this f64 computation and of the rays themselves by many orders of magnitude.
struct ScreenBounds { int32_t i0, i1, j0, j1; };
static ScreenBounds screen_bounds(const HostScene& h, const NraysRenderParams* p) {
    const ScreenBounds all = {INT32_MIN, INT32_MAX, INT32_MIN, INT32_MAX}, none = {0, -1, 0, -1};
    if (!h.bounded) return all;
    for (int a = 0; a < 3; ++a) {
        if (!(h.bounds_mn[a] <= h.bounds_mx[a])) return none; // no bounded node at all
        if (!std::isfinite(h.bounds_mn[a]) || !std::isfinite(h.bounds_mx[a])) return all;
    }
    const double* M = p->inv_proj_view; // column-major
    const double* e = p->camera_eye;
    double hc[4], hx[4], hy[4];
    for (int r = 0; r < 4; ++r) { hc[r] = M[12 + r] - M[8 + r]; hx[r] = M[r]; hy[r] = M[4 + r]; }
    // h.w keeps one sign over the frame (it is affine in dx, dy: check the corners of a slightly larger rectangle)
    const double ext = 1.0 + 4.0 / std::min<double>(p->width, p->height) + std::fabs(p->window_width);
    double wmin = INFINITY, wmax = -INFINITY, wscale = std::fabs(hc[3]) + std::fabs(hx[3]) + std::fabs(hy[3]);
    for (int k = 0; k < 4; ++k) { double w = hc[3] + ((k & 1) ? ext : -ext) * hx[3] + ((k & 2) ? ext : -ext) * hy[3]; wmin = std::min(wmin, w); wmax = std::max(wmax, w); }
    if (!(wscale > 0.0) || !std::isfinite(wscale) || !(wmin > 1e-9 * wscale || wmax < -1e-9 * wscale)) return all;
    const double sgn = wmin > 0.0 ? 1.0 : -1.0;
    double Dc[3], Dx[3], Dy[3];
    for (int a = 0; a < 3; ++a) { Dc[a] = hc[a] - e[a] * hc[3]; Dx[a] = hx[a] - e[a] * hx[3]; Dy[a] = hy[a] - e[a] * hy[3]; }
    auto det3 = [](const double* u, const double* v, const double* w) {
        return u[0] * (v[1] * w[2] - v[2] * w[1]) - u[1] * (v[0] * w[2] - v[2] * w[0]) + u[2] * (v[0] * w[1] - v[1] * w[0]);
    };
    auto len = [](const double* v) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); };
    const double det = det3(Dc, Dx, Dy);
    if (!std::isfinite(det) || !(std::fabs(det) > 1e-9 * len(Dc) * len(Dx) * len(Dy))) return all;
    double xmin = INFINITY, xmax = -INFINITY, ymin = INFINITY, ymax = -INFINITY;
    double A[8], B[8], G[8];
    int behind = 0;
    for (int k = 0; k < 8; ++k) {
        double c[3];
        for (int a = 0; a < 3; ++a) c[a] = (double)((k >> a) & 1 ? h.bounds_mx[a] : h.bounds_mn[a]) - e[a];
        A[k] = det3(c, Dx, Dy) / det; B[k] = det3(Dc, c, Dy) / det; G[k] = det3(Dc, Dx, c) / det; // Cramer
        if (!std::isfinite(A[k]) || !std::isfinite(B[k]) || !std::isfinite(G[k])) return all;
        if (A[k] * sgn < -1e-9 * (std::fabs(A[k]) + std::fabs(B[k]) + std::fabs(G[k]))) ++behind;
    }
    if (behind == 8) return none; // the whole box lies behind the eye: its points are NEGATIVE multiples of every ray direction
    for (int k = 0; k < 8; ++k) {
        const double a_ = A[k], b_ = B[k], g_ = G[k];
        if (!(a_ * sgn > 1e-9 * (std::fabs(a_) + std::fabs(b_) + std::fabs(g_)))) return all; // beside / behind the eye
        const double dx = b_ / a_, dy = g_ / a_;
        if (!std::isfinite(dx) || !std::isfinite(dy)) return all;
        const double ox = (dx * 0.5 + 0.5) * (double)p->width, oy = (-dy * 0.5 + 0.5) * (double)p->height;
        xmin = std::min(xmin, ox); xmax = std::max(xmax, ox); ymin = std::min(ymin, oy); ymax = std::max(ymax, oy);
    }
    // pixel i takes its samples at ox in [i - window / 2, i + window / 2]
    const double slack = 2.0 + 0.5 * std::fabs(p->window_width);
    auto clampi = [](double v) { return (int32_t)std::max(-1.0e9, std::min(1.0e9, v)); };
    ScreenBounds r = {clampi(std::floor(xmin - slack)), clampi(std::ceil(xmax + slack)), clampi(std::floor(ymin - slack)), clampi(std::ceil(ymax + slack))};
    return r;
}

// What a cost order recorded for one camera is worth for another: the larger of (a) the angle between the two cameras' rays through each
// corner of the frame and (b) the parallax of the nearest geometry — |eye shift| over the distance from the eye to the scene's bounding box
// (at least a twentieth of its diagonal: a camera inside the scene) — both in pixels of the frame.  Tile costs vary over blocks of pixels, so
// an order stays useful while the view has shifted by less than a block (kNearPixels).  Scheduling only.
static CamSnap cam_snapshot(const HostScene& h, const NraysRenderParams* p) {
    CamSnap c; c.valid = false;
    const double* M = p->inv_proj_view;
    for (int a = 0; a < 3; ++a) c.eye[a] = p->camera_eye[a];
    for (int k = 0; k < 4; ++k) {
        const double dx = (k & 1) ? 1.0 : -1.0, dy = (k & 2) ? 1.0 : -1.0;
        double hh[4];
        for (int r = 0; r < 4; ++r) hh[r] = M[r] * dx + M[4 + r] * dy - M[8 + r] + M[12 + r];
        double d[3], n = 0.0;
        for (int a = 0; a < 3; ++a) { d[a] = hh[a] / hh[3] - c.eye[a]; n += d[a] * d[a]; }
        n = std::sqrt(n);
        if (!(n > 0.0) || !std::isfinite(n)) return c;
        for (int a = 0; a < 3; ++a) c.dir[k][a] = d[a] / n;
    }
    // angle of one pixel: the frame's diagonal chord over its diagonal in pixels
    double chord = 0.0;
    for (int a = 0; a < 3; ++a) chord += (c.dir[3][a] - c.dir[0][a]) * (c.dir[3][a] - c.dir[0][a]);
    c.pix_angle = std::sqrt(chord) / std::sqrt((double)p->width * p->width + (double)p->height * p->height);
    // distance to the nearest point of the bounded part of the scene
    double diag = 0.0, dist = 0.0; bool box = true;
    for (int a = 0; a < 3; ++a) {
        const double mn = h.bounds_mn[a], mx = h.bounds_mx[a];
        if (!(mn <= mx) || !std::isfinite(mn) || !std::isfinite(mx)) { box = false; break; }
        diag += (mx - mn) * (mx - mn);
        const double o = c.eye[a] < mn ? mn - c.eye[a] : (c.eye[a] > mx ? c.eye[a] - mx : 0.0);
        dist += o * o;
    }
    c.depth = box ? std::max(std::sqrt(dist), 0.05 * std::sqrt(diag)) : 1.0;
    c.valid = c.pix_angle > 0.0 && std::isfinite(c.pix_angle) && c.depth > 0.0;
    return c;
}
static double cam_shift_px(const CamSnap& a, const CamSnap& b) {
    if (!a.valid || !b.valid) return INFINITY;
    const double pa = std::min(a.pix_angle, b.pix_angle);
    double rot = 0.0, tr = 0.0;
    for (int k = 0; k < 4; ++k) { double q = 0.0; for (int x = 0; x < 3; ++x) q += (a.dir[k][x] - b.dir[k][x]) * (a.dir[k][x] - b.dir[k][x]); rot = std::max(rot, std::sqrt(q)); }
    for (int x = 0; x < 3; ++x) tr += (a.eye[x] - b.eye[x]) * (a.eye[x] - b.eye[x]);
    const double v = std::max(rot, std::sqrt(tr) / std::min(a.depth, b.depth)) / pa;
    return std::isfinite(v) ? v : INFINITY;
}

__global__ void k_resolve(float* out, size_t n, float spp) { // pxs.push(tot_c / ray_per_pixel as f32), scene.rs:94
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = out[i] / spp;
}

// The second half of a pipelined frame (pipeline_compose): every float of `out`, one workgroup per row — the window of blocks that can see the
// scene copied from the staging frame `win` the trace wrote (addressed like `out`), the background sums of fill_background_row_body
// everywhere else.  Frames without bands only (row = global row, no padding rows).  It runs beside the next frame's persistent trace
// grid: no LDS, a few registers, streaming 16-byte accesses.  [wi0, wi1) x [wr0, wr1): the window in pixels.
// stamp: null, or the frame's block of the ring's stamps (DRender::stamp) — thread 0 of every workgroup leaves its exit tick in word kStampHead + (row & stamp_mask) of it
// (Switches::host_stamps: the rows share stamp_mask + 1 words, nrays_get_stats takes their maximum), or, stamp_mask == ~0u, in the third word as every row did before.
__global__ void __launch_bounds__(256) k_compose(float* __restrict__ out, const float* __restrict__ win, uint32_t width, uint32_t spp, float bg0, float bg1, float bg2,
                                                 uint32_t wi0, uint32_t wi1, uint32_t wr0, uint32_t wr1, unsigned long long* stamp, uint32_t stamp_mask) {
    const uint32_t rl = blockIdx.x;
    auto leave = [&]() { if (stamp && threadIdx.x == 0u) atomicMax(&stamp[stamp_mask == ~0u ? 2u : kStampHead + (rl & stamp_mask)], (unsigned long long)__builtin_amdgcn_s_memrealtime()); };
    float b0 = 0.0f, b1 = 0.0f, b2 = 0.0f;
    for (uint32_t s = 0; s < spp; ++s) { b0 = b0 + bg0; b1 = b1 + bg1; b2 = b2 + bg2; }
    const bool split = rl >= wr0 && rl < wr1 && wi1 > wi0; // this row crosses the window
    const uint32_t f_lo = 3u * wi0, f_hi = 3u * wi1;       // floats [f_lo, f_hi) of such a row belong to the window
    __attribute__((address_space(1))) float* row = (__attribute__((address_space(1))) float*)(out + (size_t)rl * width * 3);
    const __attribute__((address_space(1))) float* src = (const __attribute__((address_space(1))) float*)(win + (size_t)rl * width * 3);
    if (((width * 3u) & 3u) == 0u && (((uintptr_t)out) & 15u) == 0u && (((uintptr_t)win) & 15u) == 0u) {
        typedef float f4v __attribute__((ext_vector_type(4)));
        const uint32_t nq = width * 3u / 4u;
        for (uint32_t q = threadIdx.x; q < nq; q += 256u) { // chunk q holds the floats 4q .. 4q + 3: the channels (q mod 3), (q + 1) mod 3, ...
            const uint32_t f = 4u * q, ph = q % 3u;
            f4v v = ph == 0u ? f4v{b0, b1, b2, b0} : (ph == 1u ? f4v{b1, b2, b0, b1} : f4v{b2, b0, b1, b2});
            if (split && f + 4u > f_lo && f < f_hi) {
                const f4v w = __builtin_nontemporal_load((const __attribute__((address_space(1))) f4v*)(src + f));
                for (uint32_t k = 0; k < 4u; ++k) if (f + k >= f_lo && f + k < f_hi) v[k] = w[k]; // (a chunk across the window's edge keeps the background outside)
            }
            __builtin_nontemporal_store(v, (__attribute__((address_space(1))) f4v*)(row + f));
        }
        leave();
        return;
    }
    for (uint32_t f = threadIdx.x; f < width * 3u; f += 256u) {
        const uint32_t i = f / 3u, c = f - i * 3u;
        row[f] = (split && i >= wi0 && i < wi1) ? src[f] : (c == 0u ? b0 : (c == 1u ? b1 : b2));
    }
    leave();
}

// =============================================================================================
// host side
// =============================================================================================
// Words of the cost-ordered work list (k_tile_order): entry k of XCD list x lives at order[8 k + x], and a list holds the wave
// tiles i = x (mod 8) — up to ceil(nwt / 8) of them — each as up to 2^lsl light-parallel parts.  The array therefore needs
// 8 * ceil(nwt / 8) << lsl words, not nwt << lsl: with nwt = 4 (mod 8) and every tile of one of the lists 0..3 split, the last
// entries of that list lie up to (4 << lsl) - 4 words beyond nwt << lsl.
static size_t order_slots(uint32_t nwt, uint32_t lsl) { return ((((size_t)nwt + 7u) / 8u) * 8u) << lsl; }

uint32_t tile_rows(const NraysRenderParams* p) {
    if (p->band_rows == 0 || p->band_owners <= 1) return p->height;
    uint32_t nb = (p->height + p->band_rows - 1) / p->band_rows;
    return ((nb + p->band_owners - 1) / p->band_owners) * p->band_rows;
}

// The primary kernel is instantiated per feature set (primary_kernel.h: NR_PRIMARY_PERMUTATIONS, one translation unit per group);
// instrumented renders and k_bounce use the full-featured code (their results are identical, only slower).  The frame names the
// permutations it could run, most specialised first; the first one the library holds is launched (a tuning build holds few).
static bool primary_permutation_exists(int feat) { // (of the full build; a tuning build, NR_ONLY, may fall back to the full kernel)
#define X(G, S, F, P, O) if (!S && (F & ~(int)kFeatLdsScene) == feat) return true;
    NR_PRIMARY_PERMUTATIONS(X)
#undef X
    return false;
}
static void launch_primary(NraysScene* sc, bool instrumented, int features, bool noxform, bool park, bool tiny, int occ, uint32_t grid, hipStream_t stream, const DScene& d, const DRender& R,
                           const QueueOut& qo, float* out, DeviceCounters* ctr, uint32_t* spill, uint32_t tx, uint32_t ty, uint32_t* work, uint32_t grab,
                           uint32_t* zero_counts, DeviceCounters* zero_ctr, hipEvent_t done = nullptr) {
    const PrimaryLaunch a{grid, stream, &d, &R, &qo, out, ctr, spill, tx, ty, work, grab, zero_counts, zero_ctr, done};
    auto launch = [&](bool stats, int feat, bool plain_, int occ_) {
        const bool launched =
               launch_primary_group0(a, stats, feat, plain_, occ_) || launch_primary_group1(a, stats, feat, plain_, occ_) || launch_primary_group2(a, stats, feat, plain_, occ_) ||
               launch_primary_group3(a, stats, feat, plain_, occ_) || launch_primary_group4(a, stats, feat, plain_, occ_) || launch_primary_group5(a, stats, feat, plain_, occ_) ||
               launch_primary_group6(a, stats, feat, plain_, occ_) || launch_primary_group7(a, stats, feat, plain_, occ_);
        if (launched) { // what nrays_debug_last_permutation reports: the permutation that ran, not the one the frame asked for first
            const uint32_t t[4] = {stats ? 1u : 0u, (uint32_t)feat, plain_ ? 1u : 0u, (uint32_t)occ_};
            if (sc->last.perm_launches && std::memcmp(t, sc->last.perm_last, sizeof t) != 0) sc->last.perm_mixed = true;
            std::memcpy(sc->last.perm_last, t, sizeof t);
            sc->last.perm_launches++;
        }
        return launched;
    };
    if (instrumented) { launch(true, kFeatAll, false, 0); return; }
    // plain frames: no RNG keys, one sample per pixel
    const bool plain = R.window_width == 0.0 && !R.use_rng && R.first_batch && R.sample_begin == 0u && R.sample_end == 1u && R.width <= 16384u && R.height <= 16384u;
    const bool mesh_only = features == 2 || features == 6 || features == 18 || features == 22;
    if (occ == 3) { // the three-wave builds of the alpha-shadow mesh permutations: + kFeatNoXform when every BLAS is untransformed, + kFeatPark
        if (features == 6 || features == 22) { if (launch(false, features + (noxform ? (int)kFeatNoXform : 0) + (park ? (int)kFeatPark : 0), plain, 3)) return; }
        else if (features == 7 || features == 23) { if (launch(false, features, false, 3)) return; }
    }
    if (noxform && mesh_only && launch(false, features + (int)kFeatNoXform, plain, 0)) return;
    if (tiny && plain && launch(false, features | (int)kFeatTinyScene, true, 0)) return; // (a tuning build without them: the permutations below)
    if (tiny && launch(false, features | (int)kFeatTinyScene, false, 0)) return;
    if (plain && launch(false, features, true, 0)) return;
    if (launch(false, features, false, 0)) return;
    launch(false, kFeatAll, false, 0); // bit 8 (double branching) only in the full kernels
}

// The ring's timing events are created by the first frame that records into a slot (1 024 hipEventCreate cost 0.6 ms of every scene creation; the
// first slots are created with the handle).  Every handle of the slot is checked: a creation that failed half-way is retried by the next frame.  Touches sc->ring only.
static int ensure_ring_slot(NraysScene* sc, int slot) {
    hipEvent_t* ev[4] = {&sc->ring.ev_begin[slot], &sc->ring.ev_pbegin[slot], &sc->ring.ev_pend[slot], &sc->ring.ev_end[slot]};
    for (hipEvent_t* e : ev) if (!*e && hipEventCreate(e) != hipSuccess) { *e = nullptr; return set_last_error(NRAYS_ERR_HIP, "event creation failed"); }
    return NRAYS_OK;
}

// analytic scenes: the sums / maxima k_tile_order reports per list, their pinned landing place and the event behind the read-back
// Every member is checked: an allocation that failed half-way (nrays_scene_create tolerates it) is completed by the first frame that sorts.  Touches sc->order only.
static int alloc_cost_stats(NraysScene* sc) {
    if (!sc->order.d_cost_stats && hipMalloc((void**)&sc->order.d_cost_stats, 16 * sizeof(unsigned long long)) != hipSuccess) { sc->order.d_cost_stats = nullptr; return set_last_error(NRAYS_ERR_OOM, "tile-cost statistics: device allocation failed"); }
    if (!sc->order.h_cost_stats && hipHostMalloc((void**)&sc->order.h_cost_stats, 16 * sizeof(unsigned long long), hipHostMallocDefault) != hipSuccess) { sc->order.h_cost_stats = nullptr; return set_last_error(NRAYS_ERR_OOM, "tile-cost statistics: pinned allocation failed"); }
    if (!sc->order.ev_stats && hipEventCreateWithFlags(&sc->order.ev_stats, hipEventDisableTiming) != hipSuccess) { sc->order.ev_stats = nullptr; return set_last_error(NRAYS_ERR_HIP, "tile-cost statistics: event creation failed"); }
    return NRAYS_OK;
}

// Pipelined frames: the handle's internal streams (pipe_depth of them; non-blocking: the caller's stream may be the legacy null stream, which a blocking stream would
// serialise with), their events, and per slot the staging rows of a window of up to `floats` floats.  Growing the staging rows drains the handle first.
// pipeline_ensure and pipeline_release change sc->pipe only (they read sw.pipe_depth, facts.spill_entries and, to drain, last.stream).
static int pipeline_ensure(NraysScene* sc, size_t floats) {
    for (int k = 0; k < sc->sw.pipe_depth; ++k) if (!sc->pipe.stream[k]) HIP_TRY(hipStreamCreateWithFlags(&sc->pipe.stream[k], hipStreamNonBlocking));
    for (int k = 0; k < sc->pipe.slots; ++k) {
        if (!sc->pipe.ev_traced[k]) HIP_TRY(hipEventCreateWithFlags(&sc->pipe.ev_traced[k], hipEventDisableTiming));
        if (!sc->pipe.ev_composed[k]) HIP_TRY(hipEventCreateWithFlags(&sc->pipe.ev_composed[k], hipEventDisableTiming));
    }
    for (int k = 0; k < sc->sw.pipe_depth; ++k) { const int rs = ensure_spill(sc, &sc->pipe.spill[k]); if (rs != NRAYS_OK) return rs; }
    if (floats > sc->pipe.floats) {
        if (sc->last.have) HIP_TRY(hipStreamSynchronize(sc->last.stream)); // every trace in flight has its compose there, or ordered before it
        for (int k = 0; k < sc->pipe.slots; ++k) if (sc->pipe.stage[k]) { (void)hipFree(sc->pipe.stage[k]); sc->pipe.stage[k] = nullptr; }
        sc->pipe.floats = 0;
        for (int k = 0; k < sc->pipe.slots; ++k) HIP_TRY(hipMalloc((void**)&sc->pipe.stage[k], floats * sizeof(float)));
        sc->pipe.floats = floats;
    }
    return NRAYS_OK;
}
void pipeline_release(NraysScene* sc) {
    for (int k = 0; k < NraysScene::kPipeStreams; ++k) if (sc->pipe.stream[k]) (void)hipStreamSynchronize(sc->pipe.stream[k]); // all of them drained before anything they use is freed
    for (int k = 0; k < NraysScene::kPipeStreams; ++k) {
        if (sc->pipe.stream[k]) { (void)hipStreamDestroy(sc->pipe.stream[k]); sc->pipe.stream[k] = nullptr; }
        if (sc->pipe.spill[k]) { (void)hipFree(sc->pipe.spill[k]); sc->pipe.spill[k] = nullptr; }
    }
    for (int k = 0; k < NraysScene::kPipeSlots; ++k) {
        if (sc->pipe.stage[k]) { (void)hipFree(sc->pipe.stage[k]); sc->pipe.stage[k] = nullptr; }
        if (sc->pipe.ev_traced[k]) { (void)hipEventDestroy(sc->pipe.ev_traced[k]); sc->pipe.ev_traced[k] = nullptr; }
        if (sc->pipe.ev_composed[k]) { (void)hipEventDestroy(sc->pipe.ev_composed[k]); sc->pipe.ev_composed[k] = nullptr; }
    }
    sc->pipe.floats = 0;
}

// The handle that rendered last, process-wide: a caller that alternates between handles (two handles, two streams, two frame buffers) already overlaps its frames on the
// device, and pipelining each handle on top of that oversubscribes the hardware queues (six streams: 0.044 ms per frame against 0.0285 on the direct path,
// profiles/pipelined_frames_full.log) — such frames stay on the direct path.
static std::atomic<NraysScene*> g_last_renderer{nullptr};

// ---- the frame's plan ------------------------------------------------------------------------------------------------------------------
// FramePlan (scene_handle.h): what plan_frame decides once per frame; the handle keeps the plan of its last parameter block (NraysScene::plan).

// NRAYS_HOST_TIMES=n (Switches::host_times_from): microseconds of host time this call spends up to a few marks, for the handle's frames n .. n + 3 (1: its first frames, tools/cold_probe.py)
struct HostTimes {
    bool on; unsigned long long frame; std::chrono::steady_clock::time_point t0;
    void mark(const char* what) const { if (on) fprintf(stderr, "  render_impl frame %llu: +%.1f us %s\n", frame, std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count(), what); }
};

// Fills the plan and the by-value DRender (everything but the sample range of a launch, what the schedulers decide and f.timed / f.slot).  No HIP call; the handle is only
// read, and only what never changes of it (sw, facts): the same parameter block gives the same plan (NraysScene::plan).
static int plan_frame(const NraysScene* sc, const NraysRenderParams* p, bool instrumented, FramePlan& f, DRender& R) {
    if (p->ray_per_pixel == 0) return set_last_error(NRAYS_ERR_BAD_ARG, "ray_per_pixel must be > 0 (scene.rs:37)");
    if (p->width == 0 || p->height == 0) return set_last_error(NRAYS_ERR_BAD_ARG, "empty resolution");
    if (p->band_owners > 1 && (p->band_rows == 0 || p->band_owner >= p->band_owners)) return set_last_error(NRAYS_ERR_BAD_ARG, "bad band parameters");
    const uint32_t rows = f.rows = tile_rows(p);
    const uint64_t npix_local = f.npix_local = (uint64_t)rows * p->width;
    if (npix_local >= (1ull << 31)) return set_last_error(NRAYS_ERR_UNSUPPORTED, "tile too large");
    // owned rows only (padding rows of the last band carry no rays)
    f.owned_rows = 0;
    if (p->band_rows == 0 || p->band_owners <= 1) f.owned_rows = p->height;
    else for (uint32_t j = 0; j < p->height; ++j) if (((j / p->band_rows) % p->band_owners) == p->band_owner) ++f.owned_rows;

    // sample batching keeps the number of primary rays (and hence continuation rays) per launch bounded
    // Continuation rays stay in registers (trace_chain); the HBM queue is only needed when one hit can
    // spawn both a reflection and a refraction.
    f.queued = sc->facts.host.any_double_branch;
    // Sample batching bounds the continuation rays one launch can append to that queue; a frame without a queue renders
    // all its samples in ONE launch (NRAYS_MAX_PRIMARY forces batching for the tests).
    const uint64_t kMaxPrimaryPerLaunch = sc->sw.max_primary_per_launch;
    const uint32_t batch = f.batch = (f.queued || sc->sw.max_primary_forced)
        ? (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(p->ray_per_pixel, kMaxPrimaryPerLaunch / std::max<uint64_t>(1, npix_local)))
        : p->ray_per_pixel;

    std::memset(&R, 0, sizeof R);
    R.width = p->width; R.height = p->height; R.rows_local = rows; R.spp = p->ray_per_pixel;
    R.max_depth = p->max_depth;
    R.band_rows = p->band_rows; R.band_owner = p->band_owner; R.band_owners = p->band_owners ? p->band_owners : 1;
    R.window_width = p->window_width; R.inv_width = 1.0 / (double)p->width; R.inv_height = 1.0 / (double)p->height;
    for (int a = 0; a < 3; ++a) R.eye[a] = p->camera_eye[a];
    for (int a = 0; a < 16; ++a) R.m[a] = p->inv_proj_view[a];
    R.seed = p->seed;
    R.use_rng = (p->window_width != 0.0 || sc->facts.host.any_area_light) ? 1u : 0u;
    { const ScreenBounds sb = sc->sw.cull_enabled ? screen_bounds(sc->facts.host, p) : ScreenBounds{INT32_MIN, INT32_MAX, INT32_MIN, INT32_MAX};
      R.cull_i0 = sb.i0; R.cull_i1 = sb.i1; R.cull_j0 = sb.j0; R.cull_j1 = sb.j1; }

    // lanes per pixel of an anti-aliased frame (sample-major mapping, see k_primary): the largest power of two <= min(batch, 64)
    uint32_t lane_log2 = 0;
    if (batch >= 2) { while (lane_log2 < 6u && (2u << lane_log2) <= batch) ++lane_log2; }
    if (sc->sw.lane_log2_override >= 0) lane_log2 = std::min<uint32_t>((uint32_t)sc->sw.lane_log2_override, lane_log2);
    R.lane_log2 = f.lane_log2 = lane_log2;
    const uint32_t bwl = f.bwl = lane_log2 ? (7u - lane_log2) >> 1 : 4u, bhl = f.bhl = lane_log2 ? (6u - lane_log2) >> 1 : 4u; // pixel block of a scheduling unit
    const uint32_t tiles_x = f.tiles_x = (p->width + (1u << bwl) - 1) >> bwl, tiles_y = f.tiles_y = (rows + (1u << bhl) - 1) >> bhl;
    const uint32_t ntiles = f.ntiles = lane_log2 ? (tiles_x * tiles_y + 3u) / 4u : tiles_x * tiles_y; // in units of four wave tiles
    // window of scheduling blocks that can see the scene (DRender::win_*); a block row of the compact buffer maps to
    // consecutive global rows as long as the bands are whole blocks high
    R.win_x0 = 0; R.win_nx = tiles_x; R.win_y0 = 0; R.win_ny = tiles_y;
    const bool banded = f.banded = p->band_rows != 0 && R.band_owners > 1;
    if (batch >= p->ray_per_pixel && !instrumented && (!banded || p->band_rows % (1u << bhl) == 0) && (R.cull_i0 != INT32_MIN || R.cull_i1 != INT32_MAX)) {
        const int64_t i0 = std::max<int64_t>(R.cull_i0, 0), i1 = std::min<int64_t>(R.cull_i1, (int64_t)p->width - 1);
        uint32_t x0 = 0, nx = 0, y0 = 0, ny = 0;
        if (i0 <= i1) { x0 = (uint32_t)(i0 >> bwl); nx = (uint32_t)(i1 >> bwl) - x0 + 1u; }
        for (uint32_t by = 0; by < tiles_y && nx; ++by) {
            const uint32_t rl0 = by << bhl;
            const int64_t j0 = banded ? (int64_t)((rl0 / p->band_rows) * R.band_owners + R.band_owner) * p->band_rows + (rl0 % p->band_rows) : (int64_t)rl0;
            const int64_t j1 = std::min<int64_t>(j0 + (1 << bhl) - 1, (int64_t)p->height - 1);
            if (j0 > j1 || j1 < R.cull_j0 || j0 > R.cull_j1) continue; // padding rows / outside the bounds
            if (ny == 0) y0 = by;
            ny = by - y0 + 1u;
        }
        if (ny == 0) nx = 0;
        R.win_x0 = x0; R.win_nx = nx; R.win_y0 = y0; R.win_ny = ny;
    }
    f.win_units = R.win_nx * R.win_ny; // scheduling blocks inside the window
    f.grab = sc->facts.host.any_mesh ? 1u : 0u; // 0 = workgroup lists through LDS; the specialised kernels fix their path at compile time
    if (sc->sw.grab_override >= 0) f.grab = (uint32_t)sc->sw.grab_override; // tiles per dequeue of the mesh kernels, A/B only (NRAYS_GRAB); pixels do not depend on it
    // persistent grid: exactly the workgroups that can be resident (one 4-wave workgroup per CU per wave/SIMD)
    // Waves per SIMD of the alpha-shadow mesh permutations (k_primary's OCC): three for multi-light frames (their long tiles are split
    // into light-parallel parts, so the frame is bound by its sum) and for frames with many tiles per resident wave, two otherwise
    // (the frame is as long as its longest tile, and that tile's wave is fastest at two).  NRAYS_OCC overrides.
    int occ = 0;
    if (!instrumented && (sc->facts.features == 6 || sc->facts.features == 7 || sc->facts.features == 22 || sc->facts.features == 23) && lane_log2 == 0u) {
        const uint64_t wave_tiles = (uint64_t)ntiles * 4u, waves2 = (uint64_t)sc->facts.num_cus * 8u;
        // (multi-light frames: from 6 wave tiles per resident wave on.  Round 5, after the shadow rays that are multiplied by 0 stopped being traced
        // (light_is_dark()): an owner's eighth of a 4K frame, 16 320 wave tiles, runs 1.22 - 1.29 ms at three waves against 1.40 - 1.44 at two, half a
        // 1080p frame 1.48 against 1.74; at 8 160 - 8 640 wave tiles the frame is as long as its longest split tile and two waves win, 1.10 / 0.97 ms
        // against 1.46 / 1.24: profiles/r05_rank_occupancy.log.  Round 4's threshold was 12: the eighth then ran 1.9 ms at two against 2.0 - 2.9.)
        const bool multi = (sc->facts.features & kFeatMultiSample) && sc->facts.light_lsl && sc->sw.light_split_factor != 0.0f;
        // One light: from 14 wave tiles per resident wave on (round 5: the 1080p sponza stand-in, 32 640 wave tiles, 1.125 ms at three waves against 1.23 at two — its sum of
        // tile cycles per resident wave, 1.14 ms at two waves, had passed its longest tile, 0.89; at 1600 x 900, 22 800 wave tiles, the longest tile still leads and two waves
        // win, 0.93 against 1.12: profiles/r05_rank_occupancy.log.  Round 4's threshold was 24.)
        // (with the long tiles of one-light frames split by pixels, NR_PIXEL_SPLIT, the longest tile stops leading earlier: 22 800 wave tiles 0.86 ms at three waves against 0.95,
        // 14 400 wave tiles 0.75 against 0.73 — from 9 on)
        occ = wave_tiles >= (multi ? 6u : (NR_PIXEL_SPLIT && sc->facts.light_lsl ? 9u : 14u)) * waves2 ? 3 : 0;
        if (sc->sw.occ_override >= 0) occ = sc->sw.occ_override == 3 ? 3 : 0;
    }
    f.occ = occ;
    f.grid = std::min<uint32_t>(std::min<uint32_t>(((ntiles + 7u) / 8u) * 8u, (uint32_t)kMaxGrid),
                                (uint32_t)sc->facts.num_cus * (uint32_t)(occ ? NR_OCC3_AS : waves_per_simd(instrumented ? kFeatAll : sc->facts.features)) * 256u / (uint32_t)kBlock);
    if (sc->sw.grid_wg_per_cu > 0) f.grid = std::min<uint32_t>(f.grid, (uint32_t)sc->facts.num_cus * (uint32_t)sc->sw.grid_wg_per_cu); // NRAYS_GRID_WG_PER_CU: occupancy sensitivity runs

    f.timed = false; f.slot = 0; // (render_impl: they change from call to call)
    // The staged ("wavefront") form of the trace loop (wavefront.hip) renders this frame instead of k_primary when the scene is eligible and
    // NRAYS_WAVEFRONT / the library's rule say so; pixels are identical either way.
    f.staged = !instrumented && wavefront_wanted(sc, p, lane_log2);
    f.single_launch = !f.staged && !instrumented && !f.queued && p->ray_per_pixel <= batch && p->ray_per_pixel == 1;
    f.sched_key = 0; f.cam = 0;
    if (!f.staged) {
        f.sched_key = (((uint64_t)p->width << 40) ^ ((uint64_t)rows << 20) ^ ((uint64_t)p->band_rows << 8) ^ ((uint64_t)p->band_owner << 4) ^ (uint64_t)R.band_owners ^ ((uint64_t)lane_log2 << 60))
                      + 0x9E3779B97F4A7C15ull * (((uint64_t)R.win_x0 << 48) ^ ((uint64_t)R.win_nx << 32) ^ ((uint64_t)R.win_y0 << 16) ^ (uint64_t)R.win_ny);
        uint64_t cam = 0xcbf29ce484222325ull; // FNV-1a over everything a tile's cost depends on besides the scene (which a handle never changes)
        auto mix = [&](const void* q, size_t n) { const unsigned char* b_ = (const unsigned char*)q; for (size_t i = 0; i < n; ++i) { cam ^= b_[i]; cam *= 0x100000001b3ull; } };
        mix(p->inv_proj_view, sizeof p->inv_proj_view); mix(p->camera_eye, sizeof p->camera_eye); mix(&p->window_width, sizeof p->window_width);
        mix(&p->ray_per_pixel, sizeof p->ray_per_pixel); mix(&p->max_depth, sizeof p->max_depth);
        f.cam = cam;
        f.snap = cam_snapshot(sc->facts.host, p);
    }
    return NRAYS_OK;
}

// What the frame's launches write besides `out`: the queue pair and the fixed-point sums of a double-branching scene, the spill region of deep trees.  Touches sc->buf only.
static int ensure_frame_buffers(NraysScene* sc, const FramePlan& f, hipStream_t stream) {
    if (f.queued) {
        const uint64_t want = std::min<uint64_t>(std::max<uint64_t>(4 * f.npix_local * f.batch, 1u << 16), 1ull << 27);
        int rc = ensure_queue_pair(sc->buf.queue, sc->buf.queue_capacity, (uint32_t)want);
        if (rc == NRAYS_OK) rc = ensure_fixed_sums(&sc->buf.d_fixed, &sc->buf.fixed_slots, &sc->buf.fixed_dirty, (size_t)f.npix_local * 3, stream);
        if (rc != NRAYS_OK) return rc;
    }
    return ensure_spill(sc, &sc->buf.d_spill);
}

// The per-handle state (queues, raygen tables, tile costs) assumes that the renders of one handle execute one after the other — pipelined
// frames, below, are the exception and say what they share — and `out` is written in call order: a render on a different stream than its
// predecessor is ordered behind it.  Touches sc->last only.
static int order_behind_previous(NraysScene* sc, hipStream_t stream) {
    if (!sc->last.have || sc->last.stream == stream) return NRAYS_OK;
    if (sc->last.timed && sc->last.done) { HIP_TRY(hipStreamWaitEvent(stream, sc->last.done, 0)); return NRAYS_OK; }
    return order_behind_stream(sc, sc->last.stream, stream); // the previous frame recorded no event (event_stride): mark the end of ITS stream now and wait on that — no host stall
}

// ---- per-camera scheduling state (pixels never depend on it) -----------------------------------------------------------------
// sc->order belongs to the phases of this section: record_costs, ensure_tile_arrays, schedule_mesh and schedule_analytic are the only code that writes it
// (render_impl adds the recording launch's events and cost_tiles / cost_grid / cost_split_lsl).  Of the rest of the handle the two schedulers write
// ring.ev_begin / ring.has_prepass of the frame's slot — a sort is part of the timed frame — and nothing else.
// The reference's caller renders every camera ONCE (examples/loader3d.rs:67-93), an interactive caller moves it a little every
// frame: what a frame may cost besides its tiles is decided here.
//   resting camera    the order recorded for it is reused; nothing is recorded, nothing sorted;
//   nearby camera     (shift of the view since the order's camera below kNearPixels, cam_shift_px()) the order is reused as it is for
//                     up to kMaxOrderAge frames; the last of them records its tile costs, the next one sorts them (ONE k_tile_order,
//                     which also clears the cost array) — a moving camera pays the sort every kMaxOrderAge + 1 frames;
//   cold camera       no usable history: mesh scenes guess (k_seed_costs + k_tile_order), analytic scenes run image-order lists;
//                     the frame records its costs, its successor sorts them.
static bool near_cam(const NraysScene* sc, const CamSnap& other, const CamSnap& snap) { return sc->sw.near_reuse && cam_shift_px(other, snap) <= sc->order.near_pixels; }
// This frame records its tile costs (DRender::tile_cost), for this geometry and camera.
static void record_costs(NraysScene* sc, const FramePlan& f, DRender& R, uint64_t key) {
    R.tile_cost = sc->order.d_tile_cost; sc->order.cost_key = key; sc->order.cost_cam = f.cam; sc->order.cost_snap = f.snap; sc->order.cost_valid = true;
}
// d_tile_cost / d_tile_order for nwt wave tiles (order_words words of order): re-allocated when too small, which invalidates the recorded costs and the order.
static int ensure_tile_arrays(NraysScene* sc, uint32_t nwt, size_t order_words) {
    if (nwt <= sc->order.tile_slots) return NRAYS_OK;
    if (sc->order.d_tile_cost) { (void)hipFree(sc->order.d_tile_cost); sc->order.d_tile_cost = nullptr; }
    if (sc->order.d_tile_order) { (void)hipFree(sc->order.d_tile_order); sc->order.d_tile_order = nullptr; }
    sc->order.tile_slots = 0; sc->order.cost_valid = false; sc->order.order_valid = false;
    HIP_TRY(hipMalloc((void**)&sc->order.d_tile_cost, (size_t)nwt * sizeof(uint32_t)));
    HIP_TRY(hipMalloc((void**)&sc->order.d_tile_order, order_words * sizeof(uint32_t)));
    sc->order.tile_slots = nwt;
    return NRAYS_OK;
}

// What a first frame would allocate, sized for frames up to 4K (larger ones re-allocate as before): the reference's caller
// renders a camera ONCE (loader3d.rs:67-93), so the first frame of a handle is the one that counts for it.  Failures are tolerated: the frame that needs a buffer tries again.
// (nrays_scene_create: allocate_handle_state calls it unless NRAYS_PREALLOC=0.)  Sets the tile arrays, list lengths, read-back buffers and events of sc->order, last.ev_switch,
// the ring's first slots, buf.d_spill.
void preallocate_first_frame(NraysScene* sc) {
    const uint32_t nwt = (3840u / 16u) * (2160u / 16u) * 4u;
    if (ensure_tile_arrays(sc, nwt, order_slots(nwt, sc->facts.light_lsl)) != NRAYS_OK) (void)hipGetLastError();
    if (sc->facts.light_lsl && hipMalloc((void**)&sc->order.d_order_len, 8 * sizeof(uint32_t)) != hipSuccess) { sc->order.d_order_len = nullptr; (void)hipGetLastError(); }
    // ... the analytic scenes' read-back buffers, the event a render on another stream waits for, and the ring's first slots
    if (!sc->facts.host.any_mesh && alloc_cost_stats(sc) != NRAYS_OK) { (void)hipGetLastError(); }
    if (hipEventCreateWithFlags(&sc->last.ev_switch, hipEventDisableTiming) != hipSuccess) { sc->last.ev_switch = nullptr; (void)hipGetLastError(); }
    for (int k = 0; k < 2; ++k) if (hipEventCreate(&sc->order.ev_rec[k]) != hipSuccess) { sc->order.ev_rec[k] = nullptr; (void)hipGetLastError(); }
    for (int k = 0; k < 8; ++k) (void)ensure_ring_slot(sc, k);
    if (ensure_spill(sc, &sc->buf.d_spill) != NRAYS_OK) { sc->buf.d_spill = nullptr; (void)hipGetLastError(); }
}

// mesh scenes: longest-processing-time-first from the previous frame of the same geometry (pixels do not depend on it)
// (not for the sample-major frames of anti-aliased renders: their wave tiles are a few pixels each — 8 M of them for config 5 —
// and far more even; recording, sorting and following the order costs more than the tail it removes: hairball 4K 64 spp
// 251 -> 222 ms without it, sponza 1080p 4 / 16 / 64 spp 2-4 %, profiles/r02_aa_lpt.log)
// May change: f.grab (1 when the frame follows an order); R.tile_order, R.tile_cost, R.light_lsl, R.order_len.  Launches k_seed_costs / k_tile_order.
static int schedule_mesh(NraysScene* sc, FramePlan& f, DRender& R, hipStream_t stream, bool instrumented) {
    const uint32_t kMaxOrderAge = sc->order.max_order_age;
    bool lpt = f.grab >= 1u && f.lane_log2 == 0u;
    lpt = lpt && sc->sw.lpt_enabled; // A/B switch (NRAYS_LPT=0)
    if (instrumented && sc->facts.light_lsl) lpt = false; // the instrumented kernel does not decode the split entries a plain frame's order may hold
    if (!lpt) return NRAYS_OK;
    const uint32_t nwt = std::max<uint32_t>(1u, f.lane_log2 ? f.win_units : f.win_units * 4u);
    // light-parallel tiles (DRender::light_lsl): multi-light mesh scenes; the order array then holds up to 2^lsl entries per tile
    // (one-light frames, NR_PIXEL_SPLIT: only while a single tile can lead the frame — below 24 wave tiles per resident wave at two waves per SIMD; beyond, no tile comes near
    // the frame's work per wave and the split machinery costs 0.7 %: profiles/r05_pixel_split_ab.log)
    const bool pixel_split_only = sc->facts.light_lsl && !(sc->facts.features & kFeatMultiSample);
    const uint32_t split_lsl = (sc->facts.light_lsl && sc->sw.light_split_factor != 0.0f && !instrumented && !(pixel_split_only && (uint64_t)nwt >= 24ull * (uint64_t)sc->facts.num_cus * 8ull)) ? sc->facts.light_lsl : 0u;
    { const int rc = ensure_tile_arrays(sc, nwt, order_slots(nwt, sc->facts.light_lsl)); if (rc != NRAYS_OK) return rc; }
    if (split_lsl && !sc->order.d_order_len) HIP_TRY(hipMalloc((void**)&sc->order.d_order_len, 8 * sizeof(uint32_t)));
    R.light_lsl = split_lsl; R.order_len = split_lsl ? sc->order.d_order_len : nullptr;
    const uint64_t key = f.sched_key ^ ((uint64_t)split_lsl << 56); // (an order that holds split entries is not one without them)
    const bool order_here = sc->order.order_valid && sc->order.order_key == key && !sc->order.order_seeded && sc->sw.lpt_reuse;
    bool record = false;
    if (order_here && sc->order.order_cam == f.cam) {
        R.tile_order = sc->order.d_tile_order; // resting camera
    } else if (order_here && kMaxOrderAge != 0u && sc->order.order_age < kMaxOrderAge && near_cam(sc, sc->order.order_snap, f.snap)) {
        R.tile_order = sc->order.d_tile_order; // nearby camera: the order as it is
        record = ++sc->order.order_age == kMaxOrderAge;
        if (record && split_lsl) HIP_TRY(hipMemsetAsync(sc->order.d_tile_cost, 0, (size_t)nwt * sizeof(uint32_t), stream)); // split entries record by atomicMax (rare frame: every kMaxOrderAge-th)
    } else {
        const bool costs_here = sc->order.cost_valid && sc->order.cost_key == key && (sc->order.cost_cam == f.cam || near_cam(sc, sc->order.cost_snap, f.snap));
        // no history for this view: a first guess from the boxes of the nodes that can continue a chain (k_seed_costs)
        const bool seeded = !costs_here && sc->sw.seed_enabled && sc->facts.seed_boxes != 0u && f.win_units > 0;
        if (seeded) {
            if (f.timed) HIP_TRY(hipEventRecord(sc->ring.ev_begin[f.slot], stream));
            hipLaunchKernelGGL(k_seed_costs, dim3((nwt + 255u) / 256u), dim3(256), 0, stream, R, (const float*)sc->facts.d_seed_boxes, sc->facts.seed_boxes, sc->order.d_tile_cost, nwt, sc->sw.seed_rays);
            HIP_TRY(hipGetLastError());
#ifdef NR_DEBUG_TILE_COSTS
            if (!sc->order.d_seed_copy) HIP_TRY(hipMalloc((void**)&sc->order.d_seed_copy, (size_t)sc->order.tile_slots * sizeof(uint32_t)));
            HIP_TRY(hipMemcpyAsync(sc->order.d_seed_copy, sc->order.d_tile_cost, (size_t)nwt * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream)); // tools/tile_dump.py: the guess beside the recorded costs
#endif
        }
        if (seeded || costs_here) {
            if (f.timed && !seeded) HIP_TRY(hipEventRecord(sc->ring.ev_begin[f.slot], stream));
            sc->ring.has_prepass[f.slot] = true;
            hipLaunchKernelGGL(k_tile_order, dim3(8), dim3(1024), 0, stream, sc->order.d_tile_cost, sc->order.d_tile_order, nwt, (unsigned long long*)nullptr,
                               split_lsl, sc->sw.light_split_factor, f.grid * (uint32_t)(kBlock / 64), split_lsl ? sc->order.d_order_len : (uint32_t*)nullptr, split_lsl ? 1u : 0u, sc->sw.split_hyst);
            HIP_TRY(hipGetLastError());
            R.tile_order = sc->order.d_tile_order;
            sc->order.order_valid = true; sc->order.order_key = key; sc->order.order_seeded = seeded; sc->order.order_age = 0;
            if (!seeded) { sc->order.order_cam = sc->order.cost_cam; sc->order.order_snap = sc->order.cost_snap; }
        } else if (split_lsl) HIP_TRY(hipMemsetAsync(sc->order.d_tile_cost, 0, (size_t)nwt * sizeof(uint32_t), stream));
        // a guessed order is replaced by the recorded one on the next frame; an order sorted from a NEARBY camera's costs serves this
        // one as it is (it ages like any other).  The frame that sorts its OWN camera's costs records once more: under the order it will
        // keep (nrays_get_tile_costs reports these).
        record = seeded || !costs_here || !sc->sw.lpt_reuse || sc->order.cost_cam == f.cam || kMaxOrderAge == 0u;
        if (!record) sc->order.cost_valid = false; // consumed (and, with split entries, cleared) by the sort
    }
    if (R.tile_order) f.grab = 1u;
    if (record) record_costs(sc, f, R, key);
    return NRAYS_OK;
}

// Analytic scenes (workgroup lists): the frames are a few hundred long tiles (deep reflection chains, ~10^5 cycles each) among
// thousands of short ones, and a long tile runs ~1.5x faster when it does not share its SIMD with another long one.  The first
// frame of a camera records the tile costs, the second sorts them (k_tile_order) and reads back their sum and maximum; when the
// frame's parallelism sum / max is below ~1.5 waves per SIMD of the chip, the following frames of that camera are rendered from
// the cost order with the long tiles on the first workgroup of each CU (DRender::lead_wgs, k_primary) — otherwise image order,
// as before (profiles/r02_analytic_lpt.log: balls 70.0 -> 52.4 us; primitives, whose every tile is long, stays at 201 us).
// May change: f.grid (NRAYS_LEAD_WGS=0: one workgroup per CU); R.tile_cost, R.tile_order, R.lead_wgs, R.lead_entries.  Launches k_tile_order.
static int schedule_analytic(NraysScene* sc, FramePlan& f, DRender& R, hipStream_t stream, bool instrumented) {
    if (!(f.grab == 0u && sc->sw.lpt_analytic && !instrumented && f.win_units > 0)) return NRAYS_OK;
    const uint32_t kMaxOrderAge = sc->order.max_order_age;
    const uint32_t nwt = f.lane_log2 ? f.win_units : f.win_units * 4u;
    { const int rc = ensure_tile_arrays(sc, nwt, nwt); if (rc != NRAYS_OK) return rc; }
    if (!sc->order.d_cost_stats || !sc->order.h_cost_stats || !sc->order.ev_stats) { const int rc = alloc_cost_stats(sc); if (rc != NRAYS_OK) return rc; }
    const uint64_t key = f.sched_key;
    const hipError_t stats_ready = sc->order.stats_pending ? hipEventQuery(sc->order.ev_stats) : hipErrorNotReady;
    if (sc->order.stats_pending && stats_ready != hipSuccess) (void)hipGetLastError(); // "not ready" must not surface as the launch error checked below
    if (sc->order.stats_pending && stats_ready == hipSuccess) { // the sums / maxima of the last sort's eight lists have arrived
        double sum = 0.0, mx = 0.0;
        for (int x = 0; x < 8; ++x) { sum += (double)sc->order.h_cost_stats[2 * x]; mx = std::max(mx, (double)sc->order.h_cost_stats[2 * x + 1]); }
        sc->order.lone_waves = mx > 0.0 && sum / mx < sc->sw.lone_factor * 4.0 * (double)sc->facts.num_cus;
        sc->order.lone_known = true; sc->order.lone_key = sc->order.stats_key;
        sc->order.stats_pending = false;
    }
    auto sort_costs = [&]() -> int {
        if (sc->order.stats_pending) HIP_TRY(hipEventSynchronize(sc->order.ev_stats)); // (a camera that changes every few frames: the previous read-back is long done)
        if (f.timed) HIP_TRY(hipEventRecord(sc->ring.ev_begin[f.slot], stream));
        sc->ring.has_prepass[f.slot] = true;
        hipLaunchKernelGGL(k_tile_order, dim3(8), dim3(1024), 0, stream, sc->order.d_tile_cost, sc->order.d_tile_order, nwt, sc->order.d_cost_stats, 0u, 0.0f, 0u, (uint32_t*)nullptr, 0u, 1.0f);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(sc->order.h_cost_stats, sc->order.d_cost_stats, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipEventRecord(sc->order.ev_stats, stream));
        sc->order.stats_pending = true; sc->order.stats_key = key;
        sc->order.order_valid = true; sc->order.order_key = key; sc->order.order_cam = sc->order.cost_cam; sc->order.order_snap = sc->order.cost_snap; sc->order.order_age = 0;
        return NRAYS_OK;
    };
    const bool order_here = sc->order.order_valid && sc->order.order_key == key;
    bool record = false;
    if (order_here && sc->order.order_cam == f.cam) {
        // steady state of a resting camera: nothing recorded, nothing sorted
    } else if (order_here && sc->order.order_age < kMaxOrderAge && near_cam(sc, sc->order.order_snap, f.snap)) {
        record = ++sc->order.order_age == kMaxOrderAge; // nearby camera: the order as it is; its last frame records for the re-sort
    } else if (sc->order.cost_valid && sc->order.cost_key == key && (sc->order.cost_cam == f.cam || near_cam(sc, sc->order.cost_snap, f.snap))) {
        const int rc = sort_costs(); if (rc != NRAYS_OK) return rc; // the frame after a recording one
    } else {
        sc->order.order_valid = false; // a cold camera: image-order lists, costs recorded
        record = true;
    }
    if (record) record_costs(sc, f, R, key);
    // (while the sums of a re-sort are on their way the decision of the previous sort of this geometry stands)
    if (sc->order.order_valid && sc->order.order_key == key && sc->order.lone_known && sc->order.lone_key == key && sc->order.lone_waves) {
        R.tile_order = sc->order.d_tile_order;
        if (sc->sw.lead_mode) { R.lead_wgs = std::min<uint32_t>(f.grid, (uint32_t)sc->facts.num_cus); R.lead_entries = R.lead_wgs * (uint32_t)sc->sw.lead_per_wg; } // two workgroups per CU: one of them owns the long tiles
        else f.grid = std::min<uint32_t>(f.grid, (uint32_t)sc->facts.num_cus);                         // NRAYS_LEAD_WGS=0: one workgroup per CU
    }
#ifdef NR_DEBUG_TILE_COSTS
    if (sc->sw.debug_record_always) R.tile_cost = sc->order.d_tile_cost; // tools/tile_costs.py: the costs of the steady-state frames
#endif
    return NRAYS_OK;
}

// ---- pipelined frames ----------------------------------------------------------------------------------------------------------
// A frame of an analytic scene that arrives while the handle's previous work is still in flight is split in two.  TRACE: the very
// k_primary launch of the direct path, on internal stream `ps` mod pipe_depth, storing the window's pixels into the staging rows
// of slot `ps` (launch index mod pipe_slots) and no background rows; it reads only what the library owns (scene records, the by-value camera, an order no frame in
// flight writes), so it is not ordered against the caller's stream and overlaps the tail of the frame before it.  COMPOSE: k_compose on
// the caller's stream behind the trace — `out` is written there alone, in call order, as on the direct path.
// Ordering of the shared state: launches n and n + pipe_depth run on the same internal stream, and only such launches share counter sets (n mod count_rot
// used, (n + pipe_depth) mod count_rot cleared: scene_handle.h), staging rows (n mod pipe_slots) and the traversal-stack spill region of their stream (pipe_spill; never the
// handle's d_spill); the trace also waits for the compose that read its staging rows pipe_slots launches ago.  Every direct frame comes behind all composes on the
// caller's stream, and the first pipelined frame after direct work makes ALL internal streams wait for the end of that work.
// The start of a burst (Switches::host_burst): the first frame after a host synchronisation goes direct, the second is the first pipelined frame "after direct work".  When that
// work is ONE plain direct frame of this handle, launch n on the caller's stream, straight behind pipelined frames (Pipe::burst_plain: one k_primary launch, nothing recorded or
// sorted, not instrumented / multi-sample / queued / banded / staged, no prepass; a second direct frame, a batch of caller rays or a failed call in between clear it), the
// traces n + 1 and n + 2 need not wait for it.  What they could share with it, item by item:
//   counter sets     launch n counts into set n mod 6 and clears set n + 3; trace n + 1 uses n + 1 and clears n + 4, trace n + 2 uses n + 2 and clears n + 5 (the frame sets
//                    likewise: the frames in between are single launches).  Trace n + 3 DOES share: it works from the set launch n clears and clears the set launch n counts
//                    into — it runs on internal stream n mod 3, which therefore waits for the end of launch n as before (depth 3 with its six sets only; else all wait);
//   spill region     launch n uses buf.d_spill, a trace the region of its own stream (pipe.spill);
//   work order       read only: neither launch n nor a pipelined frame records or sorts (R.tile_cost null, no prepass), so d_tile_order / d_tile_cost are written by nobody;
//   `out`            a trace writes its staging rows alone (ordered against the compose that last read them by the slot proof below, unchanged); `out` is written by launch n
//                    and by the composes, all on the caller's stream(s), in call order;
//   the queue pair, the fixed-point sums, cost_meta, the stamps: not touched by a plain launch (capacity 0, not queued, instrumented kernels only, R.stamp null).
// The internal streams are ordered behind everything older than launch n by the waits of the burst before (or of this rule, by induction: a stream that skipped a wait then
// ran no launch that shared anything with the frame it skipped).
// Not pipelined: frames that record or sort tile costs, instrumented / multi-sample / queued / banded / staged frames, mesh scenes
// (their moving frames sort every time), windows beyond half the frame (the copy would outweigh the rows it takes off the tracing waves).
struct PipeFrame {
    bool on;                         // this frame is split into a trace on an internal stream and a compose on the caller's
    int ps, pst;                     // its slot (staging rows, events) and its internal stream
    uint64_t launch;                 // its launch number (NraysScene::Pipe: composed_seen)
    hipStream_t lstream;             // the stream of the k_primary launch: the internal one, or the caller's on the direct path
    float* stage;                    // the slot's staging rows, addressed like `out`
    uint32_t wi0, wi1, wr0, wr1;     // the window in pixels
};
// Decides and prepares: eligibility, in-flight query, staging rows, slot and stream, the waits of the trace stream.  May change: f.grid, R.lead_wgs, R.lead_entries (the shape of the lists).
// Of the handle it writes sc->pipe (and creates last.ev_switch when no frame has yet); it reads order's outcome through R, ring.has_prepass, last.* and buf.launch_index.
static int pipeline_prepare(NraysScene* sc, const NraysRenderParams* p, FramePlan& f, DRender& R, hipStream_t stream, bool interleaved, const HostTimes& ht, PipeFrame& pf) {
    bool pipe = sc->pipe.enabled && f.single_launch && !sc->facts.d.no_elide && !f.banded && !sc->facts.host.any_mesh && f.grab == 0u && f.lane_log2 == 0u && !R.tile_cost &&
                !sc->ring.has_prepass[f.slot] && sc->last.have && f.win_units > 0u && 2ull * f.win_units <= (uint64_t)f.tiles_x * f.tiles_y;
#ifdef NR_DEBUG_TILE_COSTS
    pipe = false;
#endif
    if (pipe && !sc->sw.pipeline_always && interleaved) pipe = false; // another handle rendered in between (g_last_renderer)
    if (pipe && !sc->sw.pipeline_always) { // is the predecessor still in flight?  (a caller that waits for every frame stays on the direct path)
        // A call that comes within kInFlightProofUs of the return of the handle's last pipelined call is taken to be: its caller cannot have waited for that frame in between
        // (switches.h: half the shortest gap a synchronising caller produces).  Being wrong costs speed, never pixels — NRAYS_PIPELINE=2 pipelines every frame, in flight or not.
        const bool proved = sc->sw.host_time_proof && sc->pipe.last_pipelined &&
                            std::chrono::steady_clock::now() - sc->pipe.last_return <= std::chrono::nanoseconds((long long)(kInFlightProofUs * 1e3));
        if (!proved) {
            const hipError_t q = sc->pipe.last_pipelined ? hipEventQuery(sc->last.done) : hipStreamQuery(sc->last.stream);
            sc->pipe.n_inflight_queries++;
            if (q != hipSuccess) (void)hipGetLastError();
            else if (sc->pipe.last_pipelined) sc->pipe.composed_seen = sc->pipe.newest_launch; // (last.done is the newest compose's event)
            pipe = q == hipErrorNotReady;
        }
        ht.mark(proved ? "pipeline: in flight by the time since the last call" : "pipeline: in-flight query");
    }
    // the window in pixels; a slot holds its rows [wr0, wr1s) and is handed to the kernels as if it began at row 0 (no pitch, no kernel argument: the trace writes and the
    // compose reads those rows only)
    pf.wi0 = R.win_x0 << f.bwl; pf.wi1 = std::min<uint32_t>((R.win_x0 + R.win_nx) << f.bwl, p->width); pf.wr0 = R.win_y0 << f.bhl; pf.wr1 = (R.win_y0 + R.win_ny) << f.bhl;
    const uint32_t wr1s = std::min<uint32_t>(pf.wr1, f.rows);
    const size_t stage_skip = (size_t)pf.wr0 * p->width * 3;
    if (pipe && pipeline_ensure(sc, (size_t)(wr1s - pf.wr0) * p->width * 3) != NRAYS_OK) { // no room for the staging frames: direct from here on, and said so once
        (void)hipGetLastError(); sc->pipe.enabled = false; pipe = false;
        fprintf(stderr, "nrays: the staging frames of pipelined frames could not be allocated (%s); this handle renders every frame on the direct path\n", nrays_last_error());
    }
    // Three persistent trace grids compete for the two wave slots of a SIMD: with lead + second workgroups (two per CU) a trace holds every slot of the chip while its
    // long tiles run, and the third trace in flight mostly waits for slots; with ONE workgroup per CU (the NRAYS_LEAD_WGS=0 shape of the cost-ordered lists) two traces
    // fit side by side and the third takes the slots of whichever retires waves first.  Pixels do not depend on the shape of the lists.
    if (pipe && !sc->pipe.lead_wgs && R.lead_wgs) { R.lead_wgs = 0u; R.lead_entries = 0u; f.grid = std::min<uint32_t>(f.grid, (uint32_t)sc->facts.num_cus); }
    pf.on = pipe;
    pf.ps = (int)(sc->buf.launch_index % (uint64_t)sc->pipe.slots); pf.pst = pf.ps % sc->sw.pipe_depth; pf.launch = sc->buf.launch_index + 1u;
    pf.lstream = pipe ? sc->pipe.stream[pf.pst] : stream;
    pf.stage = pipe ? sc->pipe.stage[pf.ps] - stage_skip : nullptr;
    if (pipe) {
        if (!sc->pipe.last_pipelined) { // direct work (a frame that sorted, a batch of caller rays, ...) precedes: every internal stream behind its end
            // ... or, behind ONE plain direct frame (Pipe::burst_plain, the start of a burst: see above), only the stream of the launch that shares its counter sets
            const bool one_plain = sc->sw.host_burst && sc->pipe.burst_plain && sc->sw.pipe_depth == 3 && sc->buf.count_rot == 2 * sc->sw.pipe_depth && sc->buf.launch_index == sc->pipe.burst_launch + 1u;
            if (!sc->last.ev_switch) HIP_TRY(hipEventCreateWithFlags(&sc->last.ev_switch, hipEventDisableTiming));
            HIP_TRY(hipEventRecord(sc->last.ev_switch, stream)); // (`stream` is behind the handle's previous stream by now)
            for (int k = 0; k < sc->sw.pipe_depth; ++k)
                if (!one_plain || k == (int)(sc->pipe.burst_launch % (uint64_t)sc->pipe.slots) % sc->sw.pipe_depth) HIP_TRY(hipStreamWaitEvent(sc->pipe.stream[k], sc->last.ev_switch, 0));
        }
        // the compose that last read this slot's staging rows, pipe_slots frames ago: when the host can see that it is over the wait (5 us of host time, which bounds
        // the pipelined frame rate) is not enqueued.  It sees that without a call when a compose at or after that one has been seen finished (Pipe::composed_seen); else
        // from ONE query (1.2 - 1.4 us) of the newest compose that is pipe_depth launches old — the younger ones are surely in flight — whose answer also covers the
        // pipe_depth frames that follow; only when that one is not over from the slot's own event, as every frame did before (NRAYS_PIPELINE_LEAN=0: still does).
        const uint64_t need = sc->pipe.slot_launch[pf.ps];
        bool proved = sc->sw.lean_slots && need <= sc->pipe.composed_seen;
        if (!proved && sc->sw.lean_slots && pf.launch > (uint64_t)sc->sw.pipe_depth) {
            const uint64_t cand = pf.launch - (uint64_t)sc->sw.pipe_depth; const int cs = (int)((cand - 1u) % (uint64_t)sc->pipe.slots);
            if (cand > need && sc->pipe.slot_launch[cs] == cand) { // (a direct frame took that launch number: no event of its own)
                if (hipEventQuery(sc->pipe.ev_composed[cs]) == hipSuccess) { sc->pipe.composed_seen = cand; proved = true; } else (void)hipGetLastError();
            }
        }
        if (!proved) {
            if (hipEventQuery(sc->pipe.ev_composed[pf.ps]) == hipSuccess) sc->pipe.composed_seen = std::max(sc->pipe.composed_seen, need);
            else { (void)hipGetLastError(); HIP_TRY(hipStreamWaitEvent(pf.lstream, sc->pipe.ev_composed[pf.ps], 0)); sc->pipe.n_slot_waits++; }
        }
        ht.mark("pipeline: waits of the trace stream");
    }
    return NRAYS_OK;
}
// The second half of a pipelined frame: the caller's stream waits for the trace, then k_compose writes every float of `out`.
// (an error from here on leaves a trace in flight that no compose follows: it is drained, and what comes next is ordered as after direct work)  Touches sc->pipe only.
static int pipeline_compose(NraysScene* sc, const NraysRenderParams* p, const FramePlan& f, const PipeFrame& pf, float* d_out, hipStream_t stream, unsigned long long* stamp, const HostTimes& ht) {
    auto drained = [&](hipError_t e) { if (e != hipSuccess) { (void)hipStreamSynchronize(pf.lstream); sc->pipe.last_pipelined = false; sc->pipe.burst_plain = false; } return e; };
    HIP_TRY(drained(hipStreamWaitEvent(stream, sc->pipe.ev_traced[pf.ps], 0)));
    ht.mark("pipeline: wait of the caller's stream");
    hipExtLaunchKernelGGL(k_compose, dim3(f.rows), dim3(256), 0, stream, nullptr, sc->pipe.ev_composed[pf.ps], 0, d_out, (const float*)pf.stage, p->width, p->ray_per_pixel, sc->facts.d.background[0], sc->facts.d.background[1], sc->facts.d.background[2], pf.wi0, pf.wi1, pf.wr0, pf.wr1, stamp, sc->sw.host_stamps ? sc->sw.stamp_words - 1u : ~0u);
    HIP_TRY(drained(hipGetLastError()));
    sc->pipe.slot_launch[pf.ps] = sc->pipe.newest_launch = pf.launch;
    ht.mark("pipeline: k_compose launch");
    return NRAYS_OK;
}

// End-of-frame bookkeeping: the frame's last event, what the handle's next call orders itself behind, what nrays_get_stats reports.  Writes sc->last, the frame's
// slot of sc->ring and pipe.last_pipelined.
static int finish_frame(NraysScene* sc, const NraysRenderParams* p, const FramePlan& f, const PipeFrame& pf, hipStream_t stream, bool instrumented, uint8_t timed_by, bool plain_direct, const HostTimes& ht) {
    const bool pipelined = pf.on;
    // (a pipelined frame's kernel_ms_total runs from its trace to the end of its compose; its "done" event is the compose's)
    if ((!f.single_launch || pipelined) && f.timed && timed_by == NraysScene::Ring::kByEvents) HIP_TRY(hipEventRecord(sc->ring.ev_end[f.slot], stream));
    sc->last.timed = f.timed || pipelined;
    if (f.timed) {
        sc->ring.timed_by[f.slot] = timed_by;
        sc->ring.single_launch[f.slot] = f.single_launch && !pipelined;
        sc->last.done = sc->ring.single_launch[f.slot] ? sc->ring.ev_pend[f.slot] : sc->ring.ev_end[f.slot];
        sc->ring.frames_recorded++;
    }
    if (pipelined) sc->last.done = sc->pipe.ev_composed[pf.ps];
    // (the start of a burst, pipeline_prepare: a plain frame is one launch that recorded and sorted nothing — its scheduling state was read only)
    sc->pipe.burst_plain = !pipelined && sc->pipe.last_pipelined && plain_direct;
    sc->pipe.burst_launch = sc->buf.launch_index - 1u;
    sc->pipe.last_pipelined = pipelined;
    if (pipelined) sc->pipe.n_pipelined++; else sc->pipe.n_direct++;
    sc->last.stream = stream; sc->last.have = true;
    ht.mark("end (event records after the launch)");
    sc->last.primary = f.owned_rows * p->width * p->ray_per_pixel;
    sc->last.primary_first_batch = f.owned_rows * p->width * std::min<uint32_t>(f.batch, p->ray_per_pixel);
    sc->last.instrumented = instrumented;
    if (pipelined && sc->sw.host_time_proof) sc->pipe.last_return = std::chrono::steady_clock::now();
    return NRAYS_OK;
}

// The driver: plan, buffers, ordering, scheduling state, [pipeline], the launch loop with its bounce rounds, [compose], resolve, bookkeeping.
int render_impl(NraysScene* sc, const NraysRenderParams* p, float* d_out, hipStream_t stream, bool instrumented, uint32_t count_flags) {
    if (!sc || !p || !d_out) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    const bool interleaved = g_last_renderer.exchange(sc, std::memory_order_relaxed) != sc;
    const HostTimes ht{sc->sw.host_times_from && sc->ring.frames_total + 1 >= sc->sw.host_times_from && sc->ring.frames_total + 1 < sc->sw.host_times_from + 4, sc->ring.frames_total, std::chrono::steady_clock::now()};
    FramePlan f; DRender R;
    if (sc->sw.lean_plan && sc->plan.valid && sc->plan.instrumented == instrumented && std::memcmp(&sc->plan.p, p, sizeof *p) == 0) { f = sc->plan.f; R = sc->plan.R; } // a resting camera
    else {
        sc->plan.valid = false;
        const int rc = plan_frame(sc, p, instrumented, f, R); if (rc != NRAYS_OK) return rc;
        if (sc->sw.lean_plan) { std::memcpy(&sc->plan.p, p, sizeof *p); sc->plan.instrumented = instrumented; sc->plan.f = f; sc->plan.R = R; sc->plan.valid = true; }
    }
    f.timed = instrumented || (sc->ring.frames_total % sc->sw.event_stride) == 0;
    f.slot = (int)(sc->ring.frames_recorded % NraysScene::kRing);
    HIP_TRY(hipSetDevice(sc->facts.device));
    sc->last.perm_launches = 0; sc->last.perm_mixed = false; // (nrays_debug_last_permutation speaks of this render from here on)
    ht.mark("hipSetDevice");
    { int rc = ensure_frame_buffers(sc, f, stream); if (rc == NRAYS_OK) rc = order_behind_previous(sc, stream); if (rc != NRAYS_OK) return rc; }
    ht.mark("parameters, screen bounds, window");
    sc->ring.frames_total++;
    if (f.timed) { const int rc = ensure_ring_slot(sc, f.slot); if (rc != NRAYS_OK) return rc; }
    // events: [pbegin .. pend] brackets the first primary launch; the frame spans [pbegin .. end], and
    // `end` is only recorded separately when something follows the primary kernel
    sc->buf.d_counters = sc->buf.d_counters_set[sc->buf.frame_index % (uint64_t)sc->buf.count_rot];
    DeviceCounters* next_ctr = sc->buf.d_counters_set[(sc->buf.frame_index + (uint64_t)sc->buf.count_rot / 2u) % (uint64_t)sc->buf.count_rot]; // (scene_handle.h: the set of the next frame on this frame's stream)
    sc->buf.frame_index++;
    sc->ring.has_prepass[f.slot] = false;
    PipeFrame pf{}; // (direct until pipeline_prepare says otherwise)
    uint8_t timed_by = NraysScene::Ring::kByEvents;
    if (f.staged) {
        sc->buf.d_counts = sc->buf.d_counts_set[sc->buf.launch_index % (uint64_t)sc->buf.count_rot];
        uint32_t* next_counts = sc->buf.d_counts_set[(sc->buf.launch_index + (uint64_t)sc->buf.count_rot / 2u) % (uint64_t)sc->buf.count_rot];
        sc->buf.launch_index++;
        const int rc = wavefront_render(sc, p, R, d_out, stream, f.tiles_x, f.tiles_y, f.timed, f.slot, next_ctr, next_counts);
        if (rc != NRAYS_OK) return rc;
    } else {
        { int rc = schedule_mesh(sc, f, R, stream, instrumented); if (rc == NRAYS_OK) rc = schedule_analytic(sc, f, R, stream, instrumented); if (rc != NRAYS_OK) return rc; }
#ifdef NR_DEBUG_TILE_COSTS
        if (!sc->order.d_wave_times) HIP_TRY(hipMalloc((void**)&sc->order.d_wave_times, (size_t)kMaxGrid * (kBlock / 64) * 8 * sizeof(uint32_t)));
        HIP_TRY(hipMemsetAsync(sc->order.d_wave_times, 0, (size_t)kMaxGrid * (kBlock / 64) * 8 * sizeof(uint32_t), stream));
        R.wave_times = sc->order.d_wave_times; sc->order.dbg_grid = f.grid; R.dbg_mode = sc->sw.debug_wave_work;
#endif
        if (R.tile_cost) { sc->order.cost_tiles = f.lane_log2 ? f.win_units : f.win_units * 4u; sc->order.cost_grid = f.grid; sc->order.cost_split_lsl = R.light_lsl; }
        R.cost_meta = sc->order.d_cost_meta; // (read by the instrumented kernel only)
        ht.mark("scheduling state (seed / sort launches)");
        { const int rc = pipeline_prepare(sc, p, f, R, stream, interleaved, ht, pf); if (rc != NRAYS_OK) return rc; }
        // a timed pipelined frame is timed by its own kernels (Ring::d_stamps): none of the slot's events is recorded
        if (pf.on && f.timed && sc->sw.lean_stamps && sc->ring.d_stamps) { timed_by = NraysScene::Ring::kByStamps; R.stamp = sc->ring.d_stamps + (size_t)NraysScene::kStampBlock * (size_t)f.slot; }
        const bool ring_events = f.timed && timed_by == NraysScene::Ring::kByEvents;
        bool first_primary = true;
        for (uint32_t s0 = 0; s0 < p->ray_per_pixel; s0 += f.batch) {
            R.sample_begin = s0; R.sample_end = std::min<uint32_t>(p->ray_per_pixel, s0 + f.batch);
            R.first_batch = s0 == 0 ? 1u : 0u;
            sc->buf.d_counts = sc->buf.d_counts_set[sc->buf.launch_index % (uint64_t)sc->buf.count_rot];
            uint32_t* next_counts = sc->buf.d_counts_set[(sc->buf.launch_index + (uint64_t)sc->buf.count_rot / 2u) % (uint64_t)sc->buf.count_rot];
            sc->buf.launch_index++;
            QueueOut qo; qo.q = sc->buf.queue[1].q; qo.capacity = f.queued ? sc->buf.queue_capacity : 0; qo.count = sc->buf.d_counts + 1;
            qo.overflow = &sc->buf.d_counters->overflow;
            if (first_primary && ring_events) HIP_TRY(hipEventRecord(sc->ring.ev_pbegin[f.slot], pf.lstream));
            if (first_primary) ht.mark("event record before the launch");
            // a launch that records its tile costs is timed (nrays_get_tile_costs: NraysTileCosts::kernel_ms): by the ring's events when the frame has them, by a pair of its own otherwise
            const bool rec_events = first_primary && R.tile_cost && !f.timed && sc->order.ev_rec[0] && sc->order.ev_rec[1];
            if (first_primary && R.tile_cost) { sc->order.rec_events_valid = rec_events; sc->order.rec_slot = f.timed ? f.slot : -1; }
            if (rec_events) HIP_TRY(hipEventRecord(sc->order.ev_rec[0], stream));
            DScene dsc = sc->facts.d;
            if (instrumented && (count_flags & NRAYS_COUNT_AS_TIMED) && !sc->facts.d.no_elide) { // what the scene's plain kernel skips (trace_device.h: light_is_dark everywhere; shade_hit in the alpha-mapped mesh kernels)
                const int ft = primary_permutation_exists(sc->facts.features & ~(int)kFeatLdsScene) ? sc->facts.features : (int)kFeatAll; // the FEAT a plain frame of this scene is launched with
                dsc.stats_elide = 1u | (((ft & kFeatMesh) && (ft & kFeatAlphaShadow)) ? 2u : 0u);
            }
            // (a scene with a non-finite light / colour / texel: every frame by the kernel that skips nothing)
            const bool stats = instrumented || sc->facts.d.no_elide != 0u;
            R.no_rows = pf.on ? 1u : 0u; // a trace launch writes the window only
            launch_primary(sc, stats, sc->facts.features, sc->facts.noxform, sc->facts.park, sc->facts.tiny, f.occ, f.grid, pf.lstream, dsc, R, qo, pf.on ? pf.stage : d_out, sc->buf.d_counters,
                           pf.on ? sc->pipe.spill[pf.pst] : sc->buf.d_spill, f.tiles_x, f.tiles_y, sc->buf.d_counts + kMaxGenerations + 2, f.grab, next_counts, R.first_batch ? next_ctr : nullptr, pf.on ? sc->pipe.ev_traced[pf.ps] : nullptr);
            HIP_TRY(hipGetLastError());
            if (R.stamp && (sc->last.perm_last[0] || (sc->last.perm_last[1] & (uint32_t)kFeatMesh))) timed_by = NraysScene::Ring::kUntimed; // (a tuning build's fall-back kernel does not stamp)
            if (first_primary) ht.mark("k_primary launch");
            if (rec_events) HIP_TRY(hipEventRecord(sc->order.ev_rec[1], stream));
            if (first_primary) {
                if (ring_events) HIP_TRY(hipEventRecord(sc->ring.ev_pend[f.slot], pf.lstream));
                if (instrumented) HIP_TRY(hipMemcpyAsync(sc->ring.d_counters_primary, sc->buf.d_counters, sizeof(DeviceCounters), hipMemcpyDeviceToDevice, stream));
                first_primary = false;
            }
            if (f.queued) { // the queued second children of this batch: k_bounce rounds, folded into d_out before the next batch's k_primary continues its sums
                const BounceRounds rounds{sc->buf.queue, sc->buf.queue_capacity, sc->buf.d_counts, &sc->buf.d_counters->overflow, sc->buf.d_fixed, &sc->buf.fixed_dirty, sc->buf.d_counters, sc->buf.d_spill, &dsc, stats, p->max_depth, d_out, (size_t)f.npix_local * 3, sc->facts.num_cus};
                const int rc = run_bounce_rounds(rounds, stream, nullptr);
                if (rc != NRAYS_OK) return rc;
            }
        }
        if (pf.on) { const int rc = pipeline_compose(sc, p, f, pf, d_out, stream, R.stamp, ht); if (rc != NRAYS_OK) return rc; }
    }
    if (p->ray_per_pixel > 1) {
        size_t n = (size_t)f.npix_local * 3;
        hipLaunchKernelGGL(k_resolve, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, d_out, n, (float)p->ray_per_pixel);
        HIP_TRY(hipGetLastError());
    }
    // one launch of k_primary on the caller's stream that read the scheduling state and wrote none of it
    const bool plain_direct = !pf.on && !f.staged && f.single_launch && !f.banded && !instrumented && !R.tile_cost && !sc->ring.has_prepass[f.slot] && sc->facts.d.no_elide == 0u;
    return finish_frame(sc, p, f, pf, stream, instrumented, timed_by, plain_direct, ht);
}

} // namespace nrays
