// ray_order.hip — the caller-ray batches (nrays_trace_rays*, nrays_intersects_rays_device*, nrays_cast_rays*, nrays_shade_points*, nrays_occlusion_points*, nrays_gather_maps_points*, nrays_gather_points* and their _ex forms, nrays_gather_sh_points*, nrays_surface_texels*, nrays_dilate_texels*, nrays_debug_cast_batch, nrays_debug_box_cull; host side below the kernels), and
// first what the batches need that come in no useful order (NRAYS_RAYS_UNORDERED): the rays of a chunk are binned by a spatial key
// on the device and traced in bin order, every result written to the slot of the ray it belongs to.  The traversal lives on coherence
// inside a wave (a wave-uniform node visit is one scalar fetch for 64 lanes, and only when the lanes agree on the direction signs); a wave
// of 64 unrelated rays gets none of it.
//
// Launches of one chunk, all on the caller's stream, nothing read back, no kernel waits for another workgroup:
//   (memset)       the 2^B bin counters
//   k_ray_bounds   per-workgroup bounds of the origins (clamped to the scene's box) and of the directions' octahedral images
//   k_ray_frame    ONE workgroup merges them and deals the key's bits to the axes (ray_key.h: rk_frame_finish)
//   k_ray_keys     one lane per ray: key, bin = its leading B bits, rank = the ray's place inside its bin (returning atomic on the bin's counter)
//   k_bin_sums / k_bin_scan / k_bin_apply   exclusive prefix sum of the counters, in place (bvh_device.hip's three-launch scan, on a stream)
//   k_ray_place    order[start[bin] + rank] = ray
// then k_trace_rays_ordered / k_intersects_rays_ordered / k_cast_rays_ordered (ray_batch_kernel.h).  A counting sort on B bits, not a radix sort of the key: the
// order inside a bin is free, and need not be reproducible — a ray's arithmetic is its own, whatever wave it runs in.
//
// The atomics are spread over 2^21 counters, and the lanes of a wave that meet in one bin (the rays of a half-ordered batch do) are
// pre-reduced: they issue ONE atomic for their number (returning atomics on one word retire one every ~100 ns on this chip,
// DESIGN §5 "Scheduling").
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <new>
#include <string>

#include "../../include/nrays_abi.h"
#include "bounce.h"
#include "gather_maps_kernel.h"
#include "gather_sh_kernel.h"
#include "ray_batch_kernel.h"
#include "ray_key.h"
#include "scene_handle.h"
#include "surface_texels_kernel.h"
#include "texel_dilate_kernel.h"
#include "texel_filter_kernel.h"

static_assert(NRAYS_RAY_FRAME_DOUBLES == nrays::kRayFrameDoubles, "include/nrays_abi.h and ray_key.h disagree on the frame");

namespace nrays {

constexpr uint32_t kOrderBlock = 256u;     // threads per workgroup of the kernels below
constexpr uint32_t kBoundsMaxGrid = 1024u; // workgroups of k_ray_bounds (each writes 10 doubles)
constexpr uint32_t kNumBins = 1u << kRayBinBits;
struct SceneBox { double v[6]; };

// Merges the bounds of a workgroup's lanes: shuffles inside a wave, LDS across its four waves.  The result is valid in thread 0.
__device__ __forceinline__ void reduce_bounds(RayBounds& b, double* s /* [4 * 10] */) {
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        for (int off = 32; off > 0; off >>= 1) {
            const double lo = __shfl_down(b.lo[k], off), hi = __shfl_down(b.hi[k], off);
            b.lo[k] = lo < b.lo[k] ? lo : b.lo[k]; b.hi[k] = hi > b.hi[k] ? hi : b.hi[k];
        }
    }
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) for (int k = 0; k < 5; ++k) { s[wave * 10u + k] = b.lo[k]; s[wave * 10u + 5 + k] = b.hi[k]; }
    __syncthreads();
    if (threadIdx.x == 0u) {
        for (uint32_t w = 1; w < kOrderBlock / 64u; ++w)
            for (int k = 0; k < 5; ++k) { const double lo = s[w * 10u + k], hi = s[w * 10u + 5 + k]; b.lo[k] = lo < b.lo[k] ? lo : b.lo[k]; b.hi[k] = hi > b.hi[k] ? hi : b.hi[k]; }
    }
}

__global__ void __launch_bounds__(kOrderBlock) k_ray_bounds(uint32_t n, const double* __restrict__ ro, const double* __restrict__ rd, SceneBox box, double* __restrict__ partial) {
    __shared__ double s[4 * 10];
    RayBounds b; rk_bounds_init(b);
    for (uint32_t i = blockIdx.x * kOrderBlock + threadIdx.x; i < n; i += gridDim.x * kOrderBlock) {
        const size_t i3 = 3 * (size_t)i;
        const double o[3] = {ro[i3], ro[i3 + 1], ro[i3 + 2]}, d[3] = {rd[i3], rd[i3 + 1], rd[i3 + 2]};
        rk_bounds_add(b, o, d, box.v);
    }
    reduce_bounds(b, s);
    if (threadIdx.x == 0u) for (int k = 0; k < 5; ++k) { partial[blockIdx.x * 10u + k] = b.lo[k]; partial[blockIdx.x * 10u + 5 + k] = b.hi[k]; }
}

__global__ void __launch_bounds__(kOrderBlock) k_ray_frame(const double* __restrict__ partial, uint32_t parts, SceneBox box, double* __restrict__ frame) {
    __shared__ double s[4 * 10];
    RayBounds b; rk_bounds_init(b);
    for (uint32_t p = threadIdx.x; p < parts; p += kOrderBlock) {
        RayBounds o;
        for (int k = 0; k < 5; ++k) { o.lo[k] = partial[p * 10u + k]; o.hi[k] = partial[p * 10u + 5 + k]; }
        rk_bounds_merge(b, o);
    }
    reduce_bounds(b, s);
    if (threadIdx.x == 0u) {
        double f[kRayFrameDoubles];
        rk_frame_finish(b, box.v, f);
        for (int k = 0; k < kRayFrameDoubles; ++k) frame[k] = f[k];
    }
}

// The place of a lane's ray inside its bin.  The lanes of the wave that meet in one bin issue ONE atomic: their first lane adds their number, the others take their
// places from it.  The groups are found first (wave-uniform loop, one round per distinct bin, no memory access), then every group's atomic is in flight at once.
// Every lane of the wave calls it; an inactive lane issues nothing and its result means nothing.
__device__ __forceinline__ uint32_t wave_bin_rank(bool active, uint32_t bin, uint32_t* __restrict__ bins) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t leader = lane, below = 0u, count = 1u;
    unsigned long long todo = __ballot(active);
    while (todo) {
        const int l = __ffsll((long long)todo) - 1;
        const uint32_t b = (uint32_t)__shfl((int)bin, l);
        const unsigned long long same = __ballot(active && bin == b);
        if (active && bin == b) { leader = (uint32_t)l; below = (uint32_t)__popcll(same & ((1ull << lane) - 1ull)); count = (uint32_t)__popcll(same); }
        todo &= ~same;
    }
    uint32_t first = 0u;
    if (active && leader == lane) first = atomicAdd(&bins[bin], count);
    first = (uint32_t)__shfl((int)first, (int)leader);
    return first + below;
}

// One lane per ray (every lane of a workgroup stays to the end: the run detection below shuffles across the wave).
__global__ void __launch_bounds__(kOrderBlock) k_ray_keys(uint32_t n, const double* __restrict__ ro, const double* __restrict__ rd, const double* __restrict__ frame,
                                                          uint64_t* __restrict__ keys, uint32_t* __restrict__ bins, uint32_t* __restrict__ rank) {
    double fr[kRayFrameDoubles];
    for (int k = 0; k < kRayFrameDoubles; ++k) fr[k] = frame[k]; // wave-uniform
    RayKeyFrame f; rk_frame_decode(fr, f);
    const uint32_t i = blockIdx.x * kOrderBlock + threadIdx.x;
    const bool active = i < n;
    uint32_t bin = 0xffffffffu; // (no bin: the lanes past the end issue nothing)
    if (active) {
        const size_t i3 = 3 * (size_t)i;
        const double o[3] = {ro[i3], ro[i3 + 1], ro[i3 + 2]}, d[3] = {rd[i3], rd[i3 + 1], rd[i3 + 2]};
        const uint64_t key = rk_key(f, o, d);
        keys[i] = key;
        bin = (uint32_t)(key >> (kRayKeyBits - kRayBinBits)); // < 2^B: a key is below 2^K
    }
    const uint32_t r = wave_bin_rank(active, bin, bins);
    if (active) rank[i] = r;
}

// Exclusive prefix sum of the bin counters in place, three launches (as bvh_device.hip's exclusive_scan_u32; a thread owns 16 consecutive items).
constexpr uint32_t kScanItems = 16u, kScanBlock = kOrderBlock * kScanItems;
__global__ void __launch_bounds__(kOrderBlock) k_bin_sums(const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ block_sum) {
    __shared__ uint32_t s_w[4];
    const uint32_t base = blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
    uint32_t sum = 0;
    for (uint32_t k = 0; k < kScanItems; ++k) if (base + k < n) sum += in[base + k];
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off);
    if ((threadIdx.x & 63u) == 0u) s_w[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0u) block_sum[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}
__global__ void __launch_bounds__(1024) k_bin_scan(uint32_t* block_sum, uint32_t nb) { // in place: block_sum[b] becomes the sum of the blocks before b
    __shared__ uint32_t s_sum[1024];
    const uint32_t per = (nb + 1023u) / 1024u, lo = threadIdx.x * per, hi = min(nb, lo + per);
    uint32_t sum = 0;
    for (uint32_t b = lo; b < hi; ++b) sum += block_sum[b];
    s_sum[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < 1024u; off <<= 1) { uint32_t v = threadIdx.x >= off ? s_sum[threadIdx.x - off] : 0u; __syncthreads(); s_sum[threadIdx.x] += v; __syncthreads(); }
    uint32_t run = s_sum[threadIdx.x] - sum;
    for (uint32_t b = lo; b < hi; ++b) { const uint32_t v = block_sum[b]; block_sum[b] = run; run += v; }
}
__global__ void __launch_bounds__(kOrderBlock) k_bin_apply(uint32_t* __restrict__ io, uint32_t n, const uint32_t* __restrict__ block_base) { // a workgroup reads its items before it writes them
    __shared__ uint32_t s_t[kOrderBlock];
    const uint32_t base = blockIdx.x * kScanBlock + threadIdx.x * kScanItems;
    uint32_t v[kScanItems], sum = 0;
    for (uint32_t k = 0; k < kScanItems; ++k) { v[k] = base + k < n ? io[base + k] : 0u; sum += v[k]; }
    s_t[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < kOrderBlock; off <<= 1) { uint32_t q = threadIdx.x >= off ? s_t[threadIdx.x - off] : 0u; __syncthreads(); s_t[threadIdx.x] += q; __syncthreads(); }
    uint32_t run = block_base[blockIdx.x] + s_t[threadIdx.x] - sum;
    for (uint32_t k = 0; k < kScanItems; ++k) { if (base + k < n) io[base + k] = run; run += v[k]; }
}

__global__ void __launch_bounds__(kOrderBlock) k_ray_place(uint32_t n, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ rank, const uint32_t* __restrict__ start,
                                                           uint32_t* __restrict__ order) {
    const uint32_t i = blockIdx.x * kOrderBlock + threadIdx.x;
    if (i >= n) return;
    const uint32_t bin = (uint32_t)(keys[i] >> (kRayKeyBits - kRayBinBits)) & (kNumBins - 1u);
    const uint32_t at = start[bin] + rank[i];
    if (at < n) order[at] = i; // (always: the counts sum to n)
}

// ---- the same three steps on the (point, direction) pairs of a gather chunk (nrays_gather_points*_ex; ray_batch_kernel.h: gather_pair_ray) -----------------------
// Pair r = i * num_dirs + j is ray j of point i; the ray is rebuilt in registers, and only the pairs of LIVE points take part: a skipped point's point and normal
// are never read (they may be NaN), its pairs enter no bounds, take no bin and no place.
// k_gather_bounds is k_ray_bounds on the rays of the live pairs: min / max are exact and order-free, so k_ray_frame gives bit for bit the frame ray_order_chunk
// computes from those rays as arrays.
__global__ void __launch_bounds__(kOrderBlock) k_gather_bounds(uint32_t pairs, GatherPoints in, OcclusionSpec G, const double* __restrict__ dirs,
                                                               const double* __restrict__ rotations, SceneBox box, double* __restrict__ partial) {
    __shared__ double s[4 * 10];
    RayBounds b; rk_bounds_init(b);
    for (uint32_t r = blockIdx.x * kOrderBlock + threadIdx.x; r < pairs; r += gridDim.x * kOrderBlock) {
        const uint32_t i = r / G.num_dirs, j = r - i * G.num_dirs;
        if (!gather_point_live(in, i)) continue;
        d3 ro, rd;
        gather_pair_ray(in, i, j, G, dirs, rotations, ro, rd);
        const double o[3] = {ro.x, ro.y, ro.z}, d[3] = {rd.x, rd.y, rd.z};
        rk_bounds_add(b, o, d, box.v);
    }
    reduce_bounds(b, s);
    if (threadIdx.x == 0u) for (int k = 0; k < 5; ++k) { partial[blockIdx.x * 10u + k] = b.lo[k]; partial[blockIdx.x * 10u + 5 + k] = b.hi[k]; }
}
// One lane per pair (every lane of a workgroup stays to the end, as in k_ray_keys): key, bin, rank of the live pairs.
__global__ void __launch_bounds__(kOrderBlock) k_gather_keys(uint32_t pairs, GatherPoints in, OcclusionSpec G, const double* __restrict__ dirs,
                                                             const double* __restrict__ rotations, const double* __restrict__ frame, uint64_t* __restrict__ keys,
                                                             uint32_t* __restrict__ bins, uint32_t* __restrict__ rank) {
    double fr[kRayFrameDoubles];
    for (int k = 0; k < kRayFrameDoubles; ++k) fr[k] = frame[k]; // wave-uniform
    RayKeyFrame f; rk_frame_decode(fr, f);
    const uint32_t r = blockIdx.x * kOrderBlock + threadIdx.x;
    const uint32_t i = r / G.num_dirs, j = r - i * G.num_dirs;
    const bool active = r < pairs && gather_point_live(in, i);
    uint32_t bin = 0xffffffffu;
    if (active) {
        d3 ro, rd;
        gather_pair_ray(in, i, j, G, dirs, rotations, ro, rd);
        const double o[3] = {ro.x, ro.y, ro.z}, d[3] = {rd.x, rd.y, rd.z};
        const uint64_t key = rk_key(f, o, d);
        keys[r] = key;
        bin = (uint32_t)(key >> (kRayKeyBits - kRayBinBits)); // < 2^B
    }
    const uint32_t at = wave_bin_rank(active, bin, bins);
    if (active) rank[r] = at;
}
// start[]: the scanned counters, with the number of live pairs in start[2^B] (the scan ran over 2^B + 1 words, the last one zero).
__global__ void __launch_bounds__(kOrderBlock) k_gather_place(uint32_t pairs, uint32_t num_dirs, const uint32_t* __restrict__ hit_flags, const uint64_t* __restrict__ keys,
                                                              const uint32_t* __restrict__ rank, const uint32_t* __restrict__ start, uint32_t* __restrict__ order) {
    const uint32_t r = blockIdx.x * kOrderBlock + threadIdx.x;
    if (r >= pairs) return;
    if (hit_flags && (hit_flags[r / num_dirs] & 1u) == 0u) return;
    const uint32_t bin = (uint32_t)(keys[r] >> (kRayKeyBits - kRayBinBits)) & (kNumBins - 1u);
    const uint32_t at = start[bin] + rank[r];
    if (at < pairs) order[at] = r; // (always: the counts sum to the number of live pairs)
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
static void free_per_ray(TraceWorkspace* w) {
    if (w->d_ray_keys) (void)hipFree(w->d_ray_keys);
    if (w->d_ray_rank) (void)hipFree(w->d_ray_rank);
    if (w->d_ray_order) (void)hipFree(w->d_ray_order);
    w->d_ray_keys = nullptr; w->d_ray_rank = nullptr; w->d_ray_order = nullptr; w->order_rays = 0;
}
static void ray_order_release(TraceWorkspace* w) {
    free_per_ray(w);
    if (w->d_ray_frame) (void)hipFree(w->d_ray_frame);
    if (w->d_ray_partial) (void)hipFree(w->d_ray_partial);
    if (w->d_ray_bins) (void)hipFree(w->d_ray_bins);
    if (w->d_ray_scan) (void)hipFree(w->d_ray_scan);
    w->d_ray_frame = nullptr; w->d_ray_partial = nullptr; w->d_ray_bins = nullptr; w->d_ray_scan = nullptr;
}
// Grows the reorder buffers of `w` to n rays (n <= kTraceChunk).  NRAYS_OK or a negative status with the last error set.
static int ray_order_ensure(TraceWorkspace* w, uint32_t n) {
    if (n > kTraceChunk) return set_last_error(NRAYS_ERR_BAD_ARG, "ray_order_ensure: more rays than a chunk");
    if (!w->d_ray_frame) HIP_TRY(hipMalloc((void**)&w->d_ray_frame, kRayFrameDoubles * sizeof(double)));
    if (!w->d_ray_partial) HIP_TRY(hipMalloc((void**)&w->d_ray_partial, (size_t)kBoundsMaxGrid * 10 * sizeof(double)));
    if (!w->d_ray_bins) HIP_TRY(hipMalloc((void**)&w->d_ray_bins, (size_t)(kNumBins + 1u) * sizeof(uint32_t))); // (+ 1: gather_order_chunk's total)
    if (!w->d_ray_scan) HIP_TRY(hipMalloc((void**)&w->d_ray_scan, (size_t)((kNumBins + 1u + kScanBlock - 1u) / kScanBlock) * sizeof(uint32_t)));
    if (n > w->order_rays) {
        free_per_ray(w);
        HIP_TRY(hipMalloc((void**)&w->d_ray_keys, (size_t)n * sizeof(uint64_t)));
        HIP_TRY(hipMalloc((void**)&w->d_ray_rank, (size_t)n * sizeof(uint32_t)));
        HIP_TRY(hipMalloc((void**)&w->d_ray_order, (size_t)n * sizeof(uint32_t)));
        w->order_rays = n;
    }
    return NRAYS_OK;
}

// Enqueues the reorder of one chunk (device pointers) on `stream`: frame reduction, keys + bin counts, prefix sum, placement.  Launches only —
// nothing is read back and nothing waits.  Afterwards (in stream order) w->d_ray_order[j] = the ray to trace j-th, w->d_ray_keys / d_ray_frame
// hold the keys and the frame.
static int ray_order_chunk(const NraysScene* sc, TraceWorkspace* w, uint32_t n, const double* origins, const double* dirs, hipStream_t stream) {
    if (n == 0u || n > w->order_rays) return set_last_error(NRAYS_ERR_BAD_ARG, "ray_order_chunk: workspace too small");
    SceneBox box;
    for (int a = 0; a < 3; ++a) { box.v[a] = (double)sc->facts.host.bounds_mn[a]; box.v[3 + a] = (double)sc->facts.host.bounds_mx[a]; }
    const uint32_t ray_grid = (n + kOrderBlock - 1u) / kOrderBlock, parts = ray_grid < kBoundsMaxGrid ? ray_grid : kBoundsMaxGrid;
    const uint32_t scan_grid = (kNumBins + kScanBlock - 1u) / kScanBlock;
    HIP_TRY(hipMemsetAsync(w->d_ray_bins, 0, (size_t)kNumBins * sizeof(uint32_t), stream));
    hipLaunchKernelGGL(k_ray_bounds, dim3(parts), dim3(kOrderBlock), 0, stream, n, origins, dirs, box, w->d_ray_partial);
    hipLaunchKernelGGL(k_ray_frame, dim3(1), dim3(kOrderBlock), 0, stream, (const double*)w->d_ray_partial, parts, box, w->d_ray_frame);
    hipLaunchKernelGGL(k_ray_keys, dim3(ray_grid), dim3(kOrderBlock), 0, stream, n, origins, dirs, (const double*)w->d_ray_frame, w->d_ray_keys, w->d_ray_bins, w->d_ray_rank);
    hipLaunchKernelGGL(k_bin_sums, dim3(scan_grid), dim3(kOrderBlock), 0, stream, (const uint32_t*)w->d_ray_bins, kNumBins, w->d_ray_scan);
    hipLaunchKernelGGL(k_bin_scan, dim3(1), dim3(1024), 0, stream, w->d_ray_scan, scan_grid);
    hipLaunchKernelGGL(k_bin_apply, dim3(scan_grid), dim3(kOrderBlock), 0, stream, w->d_ray_bins, kNumBins, (const uint32_t*)w->d_ray_scan);
    hipLaunchKernelGGL(k_ray_place, dim3(ray_grid), dim3(kOrderBlock), 0, stream, n, (const uint64_t*)w->d_ray_keys, (const uint32_t*)w->d_ray_rank, (const uint32_t*)w->d_ray_bins, w->d_ray_order);
    HIP_TRY(hipGetLastError());
    return NRAYS_OK;
}

// (FEAT: kFeatAll, or kFeatMesh for scenes of opaque TriMesh nodes only — the permutation whose node phases end by quorum in
// hair-like meshes, so that the independent fixtures also cover that path.)
// nrays_debug_cast_batch: the closest-hit query with the deferred exact gates exactly as shade_hit runs it (ungated traversal, the
// winner checked against the reference's AABB gates, fully gated repeat for knife-edge rays), or the shadow query, on rays from memory.
template <int FEAT>
__global__ void __launch_bounds__(kBlock, NRAYS_WAVES_PER_SIMD) k_cast_batch(DScene S, uint32_t mode, uint32_t n, const double* __restrict__ ro, const double* __restrict__ rd,
                                                                              const double* __restrict__ max_toi, NraysCastResult* __restrict__ out, uint32_t* spill) {
    __shared__ uint32_t lds_stack[kLdsStack * kBlock];
    Stack st; st.setup(lds_stack, spill, nullptr);
    Cnt cnt; cnt.zero();
    for (uint32_t base = blockIdx.x * kBlock; base < n; base += gridDim.x * kBlock) {
        const uint32_t i = base + threadIdx.x;
        if (i >= n) continue;
        const d3 o = D3(ro[3 * (size_t)i], ro[3 * (size_t)i + 1], ro[3 * (size_t)i + 2]), d = D3(rd[3 * (size_t)i], rd[3 * (size_t)i + 1], rd[3 * (size_t)i + 2]);
        NraysCastResult r; r.toi = 0.0; r.normal[0] = r.normal[1] = r.normal[2] = 0.0; r.uv[0] = r.uv[1] = 0.0; r.node_id = -1; r.flags = 0u;
        Hit hit; f3 filter = F3(1.0f, 1.0f, 1.0f);
        if (mode == 1u) {
            const bool blocked = traverse<true, false, FEAT>(S, st, o, d, max_toi[i], hit, filter, cnt);
            r.flags = blocked ? 1u : 0u; r.normal[0] = filter.x; r.normal[1] = filter.y; r.normal[2] = filter.z;
        } else {
            Isect is; uint32_t node_id = 0; bool gated = false, any = false;
            for (;;) {
                any = traverse<false, false, FEAT>(S, st, o, d, kDblMax, hit, filter, cnt, gated, &is);
                if (!any) break;
                if (resolve_hit<false, FEAT, true>(S, o, d, hit, is, node_id) || gated) break;
                gated = true;
            }
            if (any) {
                r.toi = hit.t; r.normal[0] = is.n.x; r.normal[1] = is.n.y; r.normal[2] = is.n.z; r.uv[0] = is.u; r.uv[1] = is.v;
                r.node_id = (int32_t)node_id; r.flags = 1u | (is.has_uv ? 2u : 0u);
            }
        }
        out[i] = r;
    }
}

// nrays_debug_box_cull: ONE node visit of the traversals on a case from memory — make_rayf, best_f32, the fetch of the node's planes, box_keys4 and,
// for a ray with an f32-zero component, zero_axis_cull: the product functions themselves, in the order traverse() calls them.  Case i reads node i.
// uniform = 0: a case per lane, planes through load_planes.  uniform = 1: a case per WAVE (all its lanes compute the same case, so that they share
// the node and the direction signs as load_planes_uniform requires; the first lane writes), planes through the scalar fetch.
__global__ void __launch_bounds__(kBlock) k_box_cull(const BvhNode* __restrict__ nodes, uint32_t uniform, uint32_t n, const double* __restrict__ ro, const double* __restrict__ rd,
                                                     const double* __restrict__ best, float* __restrict__ keys, uint32_t* __restrict__ bits, float* __restrict__ inv32) {
    const uint32_t tid = blockIdx.x * kBlock + threadIdx.x, threads = gridDim.x * kBlock;
    const uint32_t step = uniform ? threads >> 6 : threads;
    for (uint32_t i = uniform ? tid >> 6 : tid; i < n; i += step) {
        const d3 o = D3(ro[3 * (size_t)i], ro[3 * (size_t)i + 1], ro[3 * (size_t)i + 2]), d = D3(rd[3 * (size_t)i], rd[3 * (size_t)i + 1], rd[3 * (size_t)i + 2]);
        const RayF rf = make_rayf(o, d);
        const float btf = best_f32(best[i]);
        float k0, k1, k2, k3;
        if (uniform) {
            const uint32_t ukey = (uint32_t)__builtin_amdgcn_readfirstlane((int)((i << 7) | rf.bits));
            const NodePlanes np = load_planes_uniform(nodes, ukey);
            box_keys4(np, rf, btf, k0, k1, k2, k3);
            if ((rf.bits & 7u)) zero_axis_cull((rf.bits & 7u), o, np, k0, k1, k2, k3);
        } else {
            const NodePlanes np = load_planes(nodes, (int32_t)i, rf);
            box_keys4(np, rf, btf, k0, k1, k2, k3);
            if ((rf.bits & 7u)) zero_axis_cull((rf.bits & 7u), o, np, k0, k1, k2, k3);
        }
        if (uniform && (threadIdx.x & 63u)) continue;
        keys[4 * (size_t)i] = k0; keys[4 * (size_t)i + 1] = k1; keys[4 * (size_t)i + 2] = k2; keys[4 * (size_t)i + 3] = k3;
        bits[i] = rf.bits;
        inv32[3 * (size_t)i] = rf.ix; inv32[3 * (size_t)i + 1] = rf.iy; inv32[3 * (size_t)i + 2] = rf.iz;
    }
}

// ---- caller-ray batches: nrays_trace_rays*, nrays_intersects_rays_device (Scene::trace / Scene::intersects_ray, scene.rs:147-193) ----------------
static int trace_workspace(NraysScene* sc, TraceWorkspace** out) {
    if (!sc->tw) {
        sc->tw = new (std::nothrow) TraceWorkspace();
        if (!sc->tw) return set_last_error(NRAYS_ERR_OOM, "trace workspace");
    }
    TraceWorkspace* w = sc->tw;
    if (!w->d_counts) HIP_TRY(hipMalloc((void**)&w->d_counts, kTraceCountWords * sizeof(uint32_t)));
    if (!w->d_counters) HIP_TRY(hipMalloc((void**)&w->d_counters, sizeof(DeviceCounters)));
    { const int rs = ensure_spill(sc, &w->d_spill); if (rs != NRAYS_OK) return rs; }
    *out = w;
    return NRAYS_OK;
}
void trace_workspace_release(NraysScene* sc) {
    TraceWorkspace* w = sc->tw;
    if (!w) return;
    if (w->used) (void)hipStreamSynchronize(w->last_stream);
    for (int k = 0; k < 2; ++k) if (w->queue[k].block) (void)hipFree(w->queue[k].block);
    for (void* q : {(void*)w->d_fixed, (void*)w->d_counts, (void*)w->d_counters, (void*)w->d_spill, w->d_stage, w->d_texel_owner, w->d_texel_off, (void*)w->d_texel_blocks, w->d_gather_rays, w->d_dilate_dx}) if (q) (void)hipFree(q);
    ray_order_release(w);
    delete w;
    sc->tw = nullptr;
}
// The handle's threading contract: a batch on another stream than the handle's previous work (its last render, its last batch) is
// ordered behind it, and a render that follows on yet another stream is ordered behind the batch (frame_path.hip: order_behind_previous waits on ev_switch
// recorded on sc->last.stream when last_timed is false).  Nothing a render reports (counters, timings, tile costs) is touched.
static int batch_begin(NraysScene* sc, TraceWorkspace* w, hipStream_t stream) {
    const hipStream_t prev[2] = {sc->last.have ? sc->last.stream : stream, w->used ? w->last_stream : stream};
    for (int k = 0; k < 2; ++k) {
        if (prev[k] == stream || (k == 1 && prev[1] == prev[0])) continue;
        const int rc = order_behind_stream(sc, prev[k], stream);
        if (rc != NRAYS_OK) return rc;
    }
    return NRAYS_OK;
}
static void batch_end(NraysScene* sc, TraceWorkspace* w, hipStream_t stream) {
    w->last_stream = stream; w->used = true;
    if (sc->last.have) { sc->last.stream = stream; sc->last.timed = false; sc->pipe.last_pipelined = false; sc->pipe.burst_plain = false; }
}
// Shading needs the permutation of the scene's own feature set: kFeatMesh for scenes of opaque meshes lit by one sample per hit, kFeatAll otherwise.
static bool batch_mesh_only(const NraysScene* sc) { return (sc->facts.features & ~(int)kFeatLdsScene) == (int)kFeatMesh; }

// A batch the caller called unordered (NRAYS_RAYS_UNORDERED) is reordered when the host can see that it pays: the reorder is eight launches in
// front of the trace (a launch of a handle has a period of ~11 us), which a small batch does not earn back.  kReorderMinRays: DESIGN §5b.
constexpr uint32_t kReorderMinRays = 1u << 19;
static bool reorder_pays(const NraysScene* sc, uint32_t n) { return sc->sw.ray_reorder == 2 || (sc->sw.ray_reorder != 0 && n >= kReorderMinRays); }
static int check_ray_flags(uint32_t flags) { return (flags & ~(uint32_t)NRAYS_RAYS_UNORDERED) ? set_last_error(NRAYS_ERR_BAD_ARG, "unknown ray-batch flag") : NRAYS_OK; }
// The reorder of one chunk (ray_order.hip) when it is due: *order = the order to trace in, or nullptr (trace the rays as they come).
static int chunk_order(NraysScene* sc, TraceWorkspace* w, bool reorder, uint32_t n, const double* o, const double* d, hipStream_t stream, const uint32_t** order) {
    *order = nullptr;
    if (!reorder) return NRAYS_OK;
    int rc = ray_order_ensure(w, n);
    if (rc == NRAYS_OK) rc = ray_order_chunk(sc, w, n, o, d, stream);
    if (rc == NRAYS_OK) *order = w->d_ray_order;
    return rc;
}

// One chunk (n <= kTraceChunk) of nrays_trace_rays_device: k_trace_rays (`order`: its ordered form, lane j traces ray order[j]), then — double-branching scenes only — the k_bounce rounds of the
// queued second children and k_fold_fixed, as a frame runs them for a sample batch (bounce.h: run_bounce_rounds).
static int trace_chunk(NraysScene* sc, TraceWorkspace* w, uint32_t n, const double* o, const double* d, const double* refr, const float* energy,
                       const unsigned long long* keys, unsigned long long key_base, uint32_t max_depth, float* out, hipStream_t stream, const uint32_t* order) {
    const bool queued = sc->facts.host.any_double_branch;
    if (queued) { // a frame's rule per pixel, per ray here: 4 slots, at least 2^16, at most 2^27
        const uint64_t want = std::min<uint64_t>(std::max<uint64_t>(4ull * n, 1u << 16), 1ull << 27);
        int rc = ensure_queue_pair(w->queue, w->queue_capacity, (uint32_t)want);
        if (rc == NRAYS_OK) rc = ensure_fixed_sums(&w->d_fixed, &w->fixed_slots, &w->fixed_dirty, (size_t)n * 3, stream);
        if (rc != NRAYS_OK) return rc;
    }
    HIP_TRY(hipMemsetAsync(w->d_counts, 0, kTraceCountWords * sizeof(uint32_t), stream));
    unsigned int* overflow = w->d_counts + kTraceCountWords - 1;
    QueueOut qo; qo.q = w->queue[1].q; qo.capacity = queued ? w->queue_capacity : 0u; qo.count = w->d_counts + 1; qo.overflow = overflow;
    const uint32_t grid = std::min<uint32_t>((n + kBlock - 1) / kBlock, (uint32_t)kMaxGrid);
    const uint32_t keyed = sc->facts.host.any_area_light ? 1u : 0u;
    // (a scene with a non-finite light / colour / texel: the kernel that skips nothing, as its renders; its counters go to the batch's own block)
    if (order && sc->facts.d.no_elide) hipLaunchKernelGGL((k_trace_rays_ordered<true, kFeatAll>), dim3(grid), dim3(kBlock), 0, stream, sc->facts.d, n, order, o, d, refr, energy, keys, key_base, keyed, max_depth, out, qo, w->d_counters, w->d_spill);
    else if (order && batch_mesh_only(sc)) hipLaunchKernelGGL((k_trace_rays_ordered<false, kFeatMesh>), dim3(grid), dim3(kBlock), 0, stream, sc->facts.d, n, order, o, d, refr, energy, keys, key_base, keyed, max_depth, out, qo, w->d_counters, w->d_spill);
    else if (order) hipLaunchKernelGGL((k_trace_rays_ordered<false, kFeatAll>), dim3(grid), dim3(kBlock), 0, stream, sc->facts.d, n, order, o, d, refr, energy, keys, key_base, keyed, max_depth, out, qo, w->d_counters, w->d_spill);
    else if (sc->facts.d.no_elide) hipLaunchKernelGGL((k_trace_rays<true, kFeatAll>), dim3(grid), dim3(kBlock), 0, stream, sc->facts.d, n, o, d, refr, energy, keys, key_base, keyed, max_depth, out, qo, w->d_counters, w->d_spill);
    else if (batch_mesh_only(sc)) hipLaunchKernelGGL((k_trace_rays<false, kFeatMesh>), dim3(grid), dim3(kBlock), 0, stream, sc->facts.d, n, o, d, refr, energy, keys, key_base, keyed, max_depth, out, qo, w->d_counters, w->d_spill);
    else hipLaunchKernelGGL((k_trace_rays<false, kFeatAll>), dim3(grid), dim3(kBlock), 0, stream, sc->facts.d, n, o, d, refr, energy, keys, key_base, keyed, max_depth, out, qo, w->d_counters, w->d_spill);
    HIP_TRY(hipGetLastError());
    if (!queued) return NRAYS_OK;
    const BounceRounds rounds{w->queue, w->queue_capacity, w->d_counts, overflow, w->d_fixed, &w->fixed_dirty, w->d_counters, w->d_spill, &sc->facts.d, sc->facts.d.no_elide != 0u, max_depth, out, (size_t)n * 3, sc->facts.num_cus};
    uint32_t overflowed = 0u;
    const int rc = run_bounce_rounds(rounds, stream, &overflowed);
    if (rc != NRAYS_OK) return rc;
    if (overflowed) return set_last_error(NRAYS_ERR_QUEUE_OVERFLOW, "continuation-ray queue overflow: some traced colours are incomplete");
    return NRAYS_OK;
}

static int trace_rays_device_impl(NraysScene* sc, uint32_t n, const double* o, const double* d, const double* refr, const float* energy,
                                  const uint64_t* keys, uint32_t max_depth, float* out, uint32_t flags, hipStream_t stream) {
    if (!sc || !o || !d || !out) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (check_ray_flags(flags) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    if (n == 0) return NRAYS_OK;
    HIP_TRY(hipSetDevice(sc->facts.device));
    TraceWorkspace* w = nullptr;
    int rc = trace_workspace(sc, &w);
    if (rc == NRAYS_OK) rc = batch_begin(sc, w, stream);
    if (rc != NRAYS_OK) return rc;
    const bool reorder = (flags & NRAYS_RAYS_UNORDERED) && reorder_pays(sc, n);
    for (uint32_t c0 = 0; c0 < n && rc == NRAYS_OK; c0 += std::min<uint32_t>(n - c0, kTraceChunk)) {
        const uint32_t nc = std::min<uint32_t>(n - c0, kTraceChunk);
        const uint32_t* order = nullptr;
        rc = chunk_order(sc, w, reorder, nc, o + 3 * (size_t)c0, d + 3 * (size_t)c0, stream, &order);
        if (rc != NRAYS_OK) break;
        rc = trace_chunk(sc, w, nc, o + 3 * (size_t)c0, d + 3 * (size_t)c0, refr ? refr + c0 : nullptr, energy ? energy + c0 : nullptr,
                         keys ? (const unsigned long long*)keys + c0 : nullptr, (unsigned long long)c0, max_depth, out + 3 * (size_t)c0, stream, order);
    }
    batch_end(sc, w, stream);
    return rc;
}

// The outputs of a closest-hit batch (nrays_cast_rays*): toi and node always, the rest where the caller wants them.
struct CastOut { double* toi; int32_t* node; double* normal; double* uv; int32_t* prim; uint32_t* flags; };
// One chunk (nc <= kTraceChunk) of nrays_cast_rays_device: the reorder when it is due, then k_cast_rays or its ordered form.  `out` is the chunk's.
static int cast_chunk(NraysScene* sc, TraceWorkspace* w, bool reorder, uint32_t nc, const double* o, const double* d, const double* t, const CastOut& out, hipStream_t stream) {
    const bool mesh = (sc->facts.features & ~(int)kFeatMultiSample) == (int)kFeatMesh; // (traversal only: as nrays_debug_cast_batch)
    const uint32_t grid = std::min<uint32_t>((nc + kBlock - 1) / kBlock, (uint32_t)kMaxGrid);
    const uint32_t* order = nullptr;
    const int rc = chunk_order(sc, w, reorder, nc, o, d, stream, &order);
    if (rc != NRAYS_OK) return rc;
    if (order && mesh) hipLaunchKernelGGL((k_cast_rays_ordered<kFeatMesh>), dim3(grid), dim3(kBlock), 0, stream, sc->facts.d, nc, order, o, d, t, out.toi, out.node, out.normal, out.uv, out.prim, out.flags, w->d_spill);
    else if (order) hipLaunchKernelGGL((k_cast_rays_ordered<kFeatAll>), dim3(grid), dim3(kBlock), 0, stream, sc->facts.d, nc, order, o, d, t, out.toi, out.node, out.normal, out.uv, out.prim, out.flags, w->d_spill);
    else if (mesh) hipLaunchKernelGGL((k_cast_rays<kFeatMesh>), dim3(grid), dim3(kBlock), 0, stream, sc->facts.d, nc, o, d, t, out.toi, out.node, out.normal, out.uv, out.prim, out.flags, w->d_spill);
    else hipLaunchKernelGGL((k_cast_rays<kFeatAll>), dim3(grid), dim3(kBlock), 0, stream, sc->facts.d, nc, o, d, t, out.toi, out.node, out.normal, out.uv, out.prim, out.flags, w->d_spill);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_last_error(NRAYS_ERR_HIP, std::string("k_cast_rays: ") + hipGetErrorString(e));
    return NRAYS_OK;
}
static CastOut cast_out_at(const CastOut& out, size_t c0) {
    return CastOut{out.toi + c0, out.node + c0, out.normal ? out.normal + 3 * c0 : nullptr, out.uv ? out.uv + 2 * c0 : nullptr, out.prim ? out.prim + c0 : nullptr,
                   out.flags ? out.flags + c0 : nullptr};
}
static int check_cast_args(const NraysScene* sc, const double* origins, const double* dirs, const CastOut& out, uint32_t flags) {
    if (!sc || !origins || !dirs || !out.toi || !out.node) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    return check_ray_flags(flags);
}

static int cast_rays_device_impl(NraysScene* sc, uint32_t n, const double* origins, const double* dirs, const double* max_toi, const CastOut& out, uint32_t flags,
                                 hipStream_t stream) {
    if (check_cast_args(sc, origins, dirs, out, flags) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    if (n == 0) return NRAYS_OK;
    HIP_TRY(hipSetDevice(sc->facts.device));
    TraceWorkspace* w = nullptr;
    int rc = trace_workspace(sc, &w);
    if (rc == NRAYS_OK) rc = batch_begin(sc, w, stream);
    if (rc != NRAYS_OK) return rc;
    const bool reorder = (flags & NRAYS_RAYS_UNORDERED) && reorder_pays(sc, n);
    for (uint32_t c0 = 0; c0 < n && rc == NRAYS_OK; c0 += std::min<uint32_t>(n - c0, kTraceChunk)) { // (chunks keep the kernel's 32-bit ray indices far from overflow)
        const uint32_t nc = std::min<uint32_t>(n - c0, kTraceChunk);
        rc = cast_chunk(sc, w, reorder, nc, origins + 3 * (size_t)c0, dirs + 3 * (size_t)c0, max_toi ? max_toi + c0 : nullptr, cast_out_at(out, c0), stream);
    }
    batch_end(sc, w, stream);
    return rc;
}

// The blocking form: one chunk at a time through the workspace's staging buffer.  A staged ray takes kCastStageBytes: origin, direction (3 f64), max_toi, toi (f64),
// normal (3 f64), uv (2 f64), node, prim, flags (32 bits) — the 8-byte fields first, so that every array is aligned for any chunk size.
constexpr size_t kStageUnit = 80, kCastStageBytes = 116; // TraceWorkspace::stage_rays counts units of kStageUnit bytes (a ray of nrays_trace_rays)
static size_t cast_stage_units(uint32_t rays) { return ((size_t)rays * kCastStageBytes + kStageUnit - 1) / kStageUnit; }
static int cast_rays_host_impl(NraysScene* sc, uint32_t n, const double* origins, const double* dirs, const double* max_toi, const CastOut& out, uint32_t flags) {
    if (check_cast_args(sc, origins, dirs, out, flags) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    if (n == 0) return NRAYS_OK;
    HIP_TRY(hipSetDevice(sc->facts.device));
    TraceWorkspace* w = nullptr;
    int rc = trace_workspace(sc, &w);
    if (rc != NRAYS_OK) return rc;
    const size_t cap = std::min<uint32_t>(n, kTraceChunk);
    rc = grow_device(&w->d_stage, &w->stage_rays, cast_stage_units((uint32_t)cap), kStageUnit);
    if (rc != NRAYS_OK) return rc;
    double* s_o = (double*)w->d_stage; double* s_d = s_o + 3 * cap; double* s_t = s_d + 3 * cap;
    CastOut s; s.toi = s_t + cap; s.normal = s.toi + cap; s.uv = s.normal + 3 * cap;
    s.node = (int32_t*)(s.uv + 2 * cap); s.prim = s.node + cap; s.flags = (uint32_t*)(s.prim + cap);
    if (!out.normal) s.normal = nullptr;
    if (!out.uv) s.uv = nullptr;
    if (!out.prim) s.prim = nullptr;
    if (!out.flags) s.flags = nullptr;
    rc = ensure_own_stream(sc);
    if (rc != NRAYS_OK) return rc;
    const hipStream_t stream = sc->buf.own_stream;
    rc = batch_begin(sc, w, stream);
    if (rc != NRAYS_OK) return rc;
    const bool reorder = (flags & NRAYS_RAYS_UNORDERED) && reorder_pays(sc, n);
    for (uint32_t c0 = 0; c0 < n && rc == NRAYS_OK; c0 += std::min<uint32_t>(n - c0, kTraceChunk)) {
        const uint32_t nc = std::min<uint32_t>(n - c0, kTraceChunk);
        hipError_t e = hipMemcpyAsync(s_o, origins + 3 * (size_t)c0, (size_t)nc * 24, hipMemcpyHostToDevice, stream);
        if (e == hipSuccess) e = hipMemcpyAsync(s_d, dirs + 3 * (size_t)c0, (size_t)nc * 24, hipMemcpyHostToDevice, stream);
        if (e == hipSuccess && max_toi) e = hipMemcpyAsync(s_t, max_toi + c0, (size_t)nc * 8, hipMemcpyHostToDevice, stream);
        if (e != hipSuccess) { rc = set_last_error(NRAYS_ERR_HIP, std::string("cast batch upload: ") + hipGetErrorString(e)); break; }
        rc = cast_chunk(sc, w, reorder, nc, s_o, s_d, max_toi ? s_t : nullptr, s, stream);
        if (rc != NRAYS_OK) break;
        const CastOut h = cast_out_at(out, c0);
        auto down = [&](void* dst, const void* src, size_t bytes) { return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream) : hipSuccess; };
        e = down(h.toi, s.toi, (size_t)nc * 8);
        if (e == hipSuccess) e = down(h.node, s.node, (size_t)nc * 4);
        if (e == hipSuccess) e = down(h.normal, s.normal, (size_t)nc * 24);
        if (e == hipSuccess) e = down(h.uv, s.uv, (size_t)nc * 16);
        if (e == hipSuccess) e = down(h.prim, s.prim, (size_t)nc * 4);
        if (e == hipSuccess) e = down(h.flags, s.flags, (size_t)nc * 4);
        const hipError_t es = hipStreamSynchronize(stream); // (always: the staging buffer is reused by the next chunk and the next call)
        if (e == hipSuccess) e = es;
        if (e != hipSuccess) rc = set_last_error(NRAYS_ERR_HIP, std::string("cast batch read-back: ") + hipGetErrorString(e));
    }
    batch_end(sc, w, stream);
    return rc;
}

// ---- nrays_shade_points*: Material::compute on caller-supplied surface points (material.rs:8-16, phong_material.rs:72-151) -----------------------
struct ShadeIn { const double* points; const double* normals; const double* view_dirs; const double* uvs; const int32_t* nodes; const uint32_t* hit_flags; const uint64_t* keys; };
static ShadeIn shade_in_at(const ShadeIn& in, size_t c0) {
    return ShadeIn{in.points + 3 * c0, in.normals + 3 * c0, in.view_dirs + 3 * c0, in.uvs ? in.uvs + 2 * c0 : nullptr, in.nodes + c0,
                   in.hit_flags ? in.hit_flags + c0 : nullptr, in.keys ? in.keys + c0 : nullptr};
}
static int check_shade_args(const NraysScene* sc, const ShadeIn& in, const float* out, uint32_t flags) {
    if (!sc || !in.points || !in.normals || !in.view_dirs || !in.nodes || !out) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (flags != 0u) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_shade_points: flags must be 0");
    return NRAYS_OK;
}
// One chunk (nc <= kTraceChunk) of nrays_shade_points_device; `in` and `out` are the chunk's, key_base the index of its first point in the batch.
// kFeatAll is right for every scene (it holds kFeatMultiSample: the shadow rays are traced inside the light loop); a scene with a non-finite
// light / colour / texel gets the kernel that skips nothing, as its renders, with the batch's own counter block.
static int shade_chunk(NraysScene* sc, TraceWorkspace* w, uint32_t nc, const ShadeIn& in, unsigned long long key_base, float* out, hipStream_t stream) {
    const uint32_t grid = std::min<uint32_t>((nc + kBlock - 1) / kBlock, (uint32_t)kMaxGrid);
    const uint32_t num_nodes = (uint32_t)sc->facts.host.shade.size();
    const unsigned long long* keys = (const unsigned long long*)in.keys;
    if (sc->facts.d.no_elide) hipLaunchKernelGGL((k_shade_points<true, kFeatAll>), dim3(grid), dim3(kBlock), 0, stream, sc->facts.d, nc, num_nodes, in.points, in.normals, in.view_dirs, in.uvs, in.nodes, in.hit_flags, keys, key_base, out, w->d_counters, w->d_spill);
    else hipLaunchKernelGGL((k_shade_points<false, kFeatAll>), dim3(grid), dim3(kBlock), 0, stream, sc->facts.d, nc, num_nodes, in.points, in.normals, in.view_dirs, in.uvs, in.nodes, in.hit_flags, keys, key_base, out, w->d_counters, w->d_spill);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_last_error(NRAYS_ERR_HIP, std::string("k_shade_points: ") + hipGetErrorString(e));
    return NRAYS_OK;
}

static int shade_points_device_impl(NraysScene* sc, uint32_t n, const ShadeIn& in, float* out, uint32_t flags, hipStream_t stream) {
    if (check_shade_args(sc, in, out, flags) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    if (n == 0) return NRAYS_OK;
    HIP_TRY(hipSetDevice(sc->facts.device));
    TraceWorkspace* w = nullptr;
    int rc = trace_workspace(sc, &w);
    if (rc == NRAYS_OK) rc = batch_begin(sc, w, stream);
    if (rc != NRAYS_OK) return rc;
    for (uint32_t c0 = 0; c0 < n && rc == NRAYS_OK; c0 += std::min<uint32_t>(n - c0, kTraceChunk)) { // (chunks keep the kernel's 32-bit point indices far from overflow)
        const uint32_t nc = std::min<uint32_t>(n - c0, kTraceChunk);
        rc = shade_chunk(sc, w, nc, shade_in_at(in, c0), (unsigned long long)c0, out + 4 * (size_t)c0, stream);
    }
    batch_end(sc, w, stream);
    return rc;
}

// The blocking form, through the workspace's staging buffer as cast_rays_host_impl.  A staged point takes kShadeStageBytes: point, normal, view direction (3 f64),
// uv (2 f64), key (u64), colour (4 f32), node, hit flags (32 bits) — the 8-byte fields first.
constexpr size_t kShadeStageBytes = 120;
static size_t shade_stage_units(uint32_t points) { return ((size_t)points * kShadeStageBytes + kStageUnit - 1) / kStageUnit; }
static int shade_points_host_impl(NraysScene* sc, uint32_t n, const ShadeIn& in, float* out, uint32_t flags) {
    if (check_shade_args(sc, in, out, flags) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    if (n == 0) return NRAYS_OK;
    HIP_TRY(hipSetDevice(sc->facts.device));
    TraceWorkspace* w = nullptr;
    int rc = trace_workspace(sc, &w);
    if (rc != NRAYS_OK) return rc;
    const size_t cap = std::min<uint32_t>(n, kTraceChunk);
    rc = grow_device(&w->d_stage, &w->stage_rays, shade_stage_units((uint32_t)cap), kStageUnit);
    if (rc != NRAYS_OK) return rc;
    double* s_p = (double*)w->d_stage; double* s_n = s_p + 3 * cap; double* s_v = s_n + 3 * cap; double* s_uv = s_v + 3 * cap;
    uint64_t* s_k = (uint64_t*)(s_uv + 2 * cap); float* s_out = (float*)(s_k + cap); int32_t* s_node = (int32_t*)(s_out + 4 * cap); uint32_t* s_hf = (uint32_t*)(s_node + cap);
    const ShadeIn s{s_p, s_n, s_v, in.uvs ? s_uv : nullptr, s_node, in.hit_flags ? s_hf : nullptr, in.keys ? s_k : nullptr};
    rc = ensure_own_stream(sc);
    if (rc != NRAYS_OK) return rc;
    const hipStream_t stream = sc->buf.own_stream;
    rc = batch_begin(sc, w, stream);
    if (rc != NRAYS_OK) return rc;
    for (uint32_t c0 = 0; c0 < n && rc == NRAYS_OK; c0 += std::min<uint32_t>(n - c0, kTraceChunk)) {
        const uint32_t nc = std::min<uint32_t>(n - c0, kTraceChunk);
        const ShadeIn h = shade_in_at(in, c0);
        auto up = [&](void* dst, const void* src, size_t bytes) { return src ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream) : hipSuccess; };
        hipError_t e = up(s_p, h.points, (size_t)nc * 24);
        if (e == hipSuccess) e = up(s_n, h.normals, (size_t)nc * 24);
        if (e == hipSuccess) e = up(s_v, h.view_dirs, (size_t)nc * 24);
        if (e == hipSuccess) e = up(s_uv, h.uvs, (size_t)nc * 16);
        if (e == hipSuccess) e = up(s_node, h.nodes, (size_t)nc * 4);
        if (e == hipSuccess) e = up(s_hf, h.hit_flags, (size_t)nc * 4);
        if (e == hipSuccess) e = up(s_k, h.keys, (size_t)nc * 8);
        if (e != hipSuccess) { rc = set_last_error(NRAYS_ERR_HIP, std::string("shade batch upload: ") + hipGetErrorString(e)); break; }
        rc = shade_chunk(sc, w, nc, s, (unsigned long long)c0, s_out, stream);
        if (rc != NRAYS_OK) break;
        e = hipMemcpyAsync(out + 4 * (size_t)c0, s_out, (size_t)nc * 16, hipMemcpyDeviceToHost, stream);
        const hipError_t es = hipStreamSynchronize(stream); // (always: the staging buffer is reused by the next chunk and the next call)
        if (e == hipSuccess) e = es;
        if (e != hipSuccess) rc = set_last_error(NRAYS_ERR_HIP, std::string("shade batch read-back: ") + hipGetErrorString(e));
    }
    batch_end(sc, w, stream);
    return rc;
}

// ---- nrays_occlusion_points*: ambient occlusion at caller-supplied points, the hemisphere rays built on the device ------------------------------------
struct OcclusionIn { const double* points; const double* normals; const uint32_t* hit_flags; const uint64_t* keys; };
static OcclusionIn occlusion_in_at(const OcclusionIn& in, size_t c0) {
    return OcclusionIn{in.points + 3 * c0, in.normals + 3 * c0, in.hit_flags ? in.hit_flags + c0 : nullptr, in.keys ? in.keys + c0 : nullptr};
}
static int check_occlusion_params(const NraysOcclusionParams* p) {
    if (!p || !p->dirs) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (p->num_dirs < 1u || p->num_dirs > 1024u) return set_last_error(NRAYS_ERR_BAD_ARG, "NraysOcclusionParams: num_dirs must be in 1 .. 1024");
    if (p->num_rotations > 1024u || (p->num_rotations && !p->rotations)) return set_last_error(NRAYS_ERR_BAD_ARG, "NraysOcclusionParams: num_rotations > 1024, or rotations is NULL");
    if (!(p->max_toi > 0.0)) return set_last_error(NRAYS_ERR_BAD_ARG, "NraysOcclusionParams: max_toi must be > 0 (+inf allowed)");
    if (!std::isfinite(p->bias)) return set_last_error(NRAYS_ERR_BAD_ARG, "NraysOcclusionParams: bias must be finite");
    return NRAYS_OK;
}
static int check_occlusion_args(const NraysScene* sc, const OcclusionIn& in, const NraysOcclusionParams* p, const float* out_filter, uint32_t flags) {
    if (!sc || !in.points || !in.normals || !out_filter) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (check_occlusion_params(p) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    if (flags != 0u) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_occlusion_points: flags must be 0");
    return NRAYS_OK;
}
static OcclusionSpec occlusion_spec(const NraysOcclusionParams* p) { return OcclusionSpec{p->num_dirs, p->num_rotations, p->bias, p->max_toi}; }
static uint32_t occlusion_chunk(const NraysOcclusionParams* p) { return std::max<uint32_t>(1u, kTraceChunk / p->num_dirs); } // points per chunk: at most kTraceChunk rays
// Lanes per point (log2), among the instantiated 0, 3 and 6: as many lanes as there are directions to give them.  Measured (profiles/occlusion_rate.json, sponza
// stand-in): at 2 M points x 16 directions 8 lanes take 3.07 ms against 4.77 ms with one lane per point and 3.03 ms for k_intersects_rays on the same rays; at
// 16 384 points x 64 directions 64 lanes take 0.136 ms, 8 lanes 0.205, one lane 1.47 (a grid of 64 workgroups).  The lanes of a point share its origin, and that is
// the coherence the traversal lives on; one lane per point is left to batches of fewer than 8 directions.  NRAYS_OCCLUSION_LANES=0|3|6 forces a form (the A/B of
// tools/trace_rays_rate.py --occlusion; the results do not depend on it).
static int occlusion_lanes_log2(const NraysScene* sc, uint32_t num_dirs) {
    int lp = 6;
    if (sc->sw.occlusion_lanes >= 0) lp = sc->sw.occlusion_lanes >= 6 ? 6 : (sc->sw.occlusion_lanes >= 3 ? 3 : 0);
    while (lp > 0 && (1u << lp) > num_dirs) lp -= 3;
    return lp;
}
// One chunk (nc <= occlusion_chunk) of nrays_occlusion_points_device; `in` and the outputs are the chunk's, key_base the index of its first point in the
// batch, dirs / rotations device copies of the tables.  The permutation: kFeatMesh or kFeatAll, as k_intersects_rays.
static int occlusion_chunk_launch(NraysScene* sc, TraceWorkspace* w, uint32_t nc, const OcclusionIn& in, unsigned long long key_base, const OcclusionSpec& spec,
                                  const double* dirs, const double* rotations, float* out_filter, uint32_t* out_open, hipStream_t stream) {
    const bool mesh = (sc->facts.features & ~(int)kFeatMultiSample) == (int)kFeatMesh; // (traversal only: as nrays_intersects_rays_device)
    const int lp = occlusion_lanes_log2(sc, spec.num_dirs);
    const uint32_t slots = nc << lp; // (nc * num_dirs <= kTraceChunk and 2^lp <= num_dirs)
    const uint32_t grid = std::min<uint32_t>((slots + kBlock - 1) / kBlock, (uint32_t)kMaxGrid);
    const unsigned long long* keys = (const unsigned long long*)in.keys;
#define NR_OCC_LAUNCH(FEAT, LP) hipLaunchKernelGGL((k_occlusion_points<FEAT, LP>), dim3(grid), dim3(kBlock), 0, stream, sc->facts.d, nc, in.points, in.normals, in.hit_flags, keys, key_base, spec, dirs, rotations, out_filter, out_open, w->d_spill)
    if (mesh) { if (lp == 0) NR_OCC_LAUNCH(kFeatMesh, 0); else if (lp == 3) NR_OCC_LAUNCH(kFeatMesh, 3); else NR_OCC_LAUNCH(kFeatMesh, 6); }
    else { if (lp == 0) NR_OCC_LAUNCH(kFeatAll, 0); else if (lp == 3) NR_OCC_LAUNCH(kFeatAll, 3); else NR_OCC_LAUNCH(kFeatAll, 6); }
#undef NR_OCC_LAUNCH
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_last_error(NRAYS_ERR_HIP, std::string("k_occlusion_points: ") + hipGetErrorString(e));
    return NRAYS_OK;
}

static int occlusion_points_device_impl(NraysScene* sc, uint32_t n, const OcclusionIn& in, const NraysOcclusionParams* p, float* out_filter, uint32_t* out_open,
                                        uint32_t flags, hipStream_t stream) {
    if (check_occlusion_args(sc, in, p, out_filter, flags) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    if (n == 0) return NRAYS_OK;
    HIP_TRY(hipSetDevice(sc->facts.device));
    TraceWorkspace* w = nullptr;
    int rc = trace_workspace(sc, &w);
    if (rc == NRAYS_OK) rc = batch_begin(sc, w, stream);
    if (rc != NRAYS_OK) return rc;
    const uint32_t chunk = occlusion_chunk(p);
    for (uint32_t c0 = 0; c0 < n && rc == NRAYS_OK; c0 += std::min<uint32_t>(n - c0, chunk)) {
        const uint32_t nc = std::min<uint32_t>(n - c0, chunk);
        rc = occlusion_chunk_launch(sc, w, nc, occlusion_in_at(in, c0), (unsigned long long)c0, occlusion_spec(p), p->dirs, p->rotations, out_filter + 3 * (size_t)c0,
                                    out_open ? out_open + c0 : nullptr, stream);
    }
    batch_end(sc, w, stream);
    return rc;
}

// The blocking form, through the workspace's staging buffer as shade_points_host_impl: the two tables first, then per staged point kOcclusionStageBytes —
// point, normal (3 f64), key (u64), filter (3 f32), hit flags, open count (32 bits), the 8-byte fields first.
constexpr size_t kOcclusionStageBytes = 76;
static int occlusion_points_host_impl(NraysScene* sc, uint32_t n, const OcclusionIn& in, const NraysOcclusionParams* p, float* out_filter, uint32_t* out_open, uint32_t flags) {
    if (check_occlusion_args(sc, in, p, out_filter, flags) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    if (n == 0) return NRAYS_OK;
    HIP_TRY(hipSetDevice(sc->facts.device));
    TraceWorkspace* w = nullptr;
    int rc = trace_workspace(sc, &w);
    if (rc != NRAYS_OK) return rc;
    const uint32_t chunk = occlusion_chunk(p);
    const size_t cap = std::min<uint32_t>(n, chunk), table = 3 * (size_t)p->num_dirs + 2 * (size_t)p->num_rotations;
    rc = grow_device(&w->d_stage, &w->stage_rays, (table * sizeof(double) + cap * kOcclusionStageBytes + kStageUnit - 1) / kStageUnit, kStageUnit);
    if (rc != NRAYS_OK) return rc;
    double* s_dirs = (double*)w->d_stage; double* s_rot = s_dirs + 3 * (size_t)p->num_dirs; double* s_p = s_dirs + table; double* s_n = s_p + 3 * cap;
    uint64_t* s_k = (uint64_t*)(s_n + 3 * cap); float* s_f = (float*)(s_k + cap); uint32_t* s_hf = (uint32_t*)(s_f + 3 * cap); uint32_t* s_open = s_hf + cap;
    const OcclusionIn s{s_p, s_n, in.hit_flags ? s_hf : nullptr, in.keys ? s_k : nullptr};
    rc = ensure_own_stream(sc);
    if (rc != NRAYS_OK) return rc;
    const hipStream_t stream = sc->buf.own_stream;
    rc = batch_begin(sc, w, stream);
    if (rc != NRAYS_OK) return rc;
    auto up = [&](void* dst, const void* src, size_t bytes) { return src && bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream) : hipSuccess; };
    hipError_t e = up(s_dirs, p->dirs, 24 * (size_t)p->num_dirs);
    if (e == hipSuccess) e = up(s_rot, p->rotations, 16 * (size_t)p->num_rotations);
    if (e != hipSuccess) rc = set_last_error(NRAYS_ERR_HIP, std::string("occlusion tables upload: ") + hipGetErrorString(e));
    for (uint32_t c0 = 0; c0 < n && rc == NRAYS_OK; c0 += std::min<uint32_t>(n - c0, chunk)) {
        const uint32_t nc = std::min<uint32_t>(n - c0, chunk);
        const OcclusionIn h = occlusion_in_at(in, c0);
        e = up(s_p, h.points, (size_t)nc * 24);
        if (e == hipSuccess) e = up(s_n, h.normals, (size_t)nc * 24);
        if (e == hipSuccess) e = up(s_hf, h.hit_flags, (size_t)nc * 4);
        if (e == hipSuccess) e = up(s_k, h.keys, (size_t)nc * 8);
        if (e != hipSuccess) { rc = set_last_error(NRAYS_ERR_HIP, std::string("occlusion batch upload: ") + hipGetErrorString(e)); break; }
        rc = occlusion_chunk_launch(sc, w, nc, s, (unsigned long long)c0, occlusion_spec(p), s_dirs, p->num_rotations ? s_rot : nullptr, s_f, out_open ? s_open : nullptr, stream);
        if (rc != NRAYS_OK) break;
        e = hipMemcpyAsync(out_filter + 3 * (size_t)c0, s_f, (size_t)nc * 12, hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess && out_open) e = hipMemcpyAsync(out_open + c0, s_open, (size_t)nc * 4, hipMemcpyDeviceToHost, stream);
        const hipError_t es = hipStreamSynchronize(stream); // (always: the staging buffer is reused by the next chunk and the next call)
        if (e == hipSuccess) e = es;
        if (e != hipSuccess) rc = set_last_error(NRAYS_ERR_HIP, std::string("occlusion batch read-back: ") + hipGetErrorString(e));
    }
    if (rc != NRAYS_OK) (void)hipStreamSynchronize(stream); // (the tables' upload reads the caller's memory)
    batch_end(sc, w, stream);
    return rc;
}

// ---- nrays_gather_points*: the mean of Scene::trace over the hemisphere rays of caller-supplied points, the rays built on the device --------------------------
// `hinted`: the _ex entry points, which take NRAYS_RAYS_UNORDERED; the others take no flag at all.
static int check_gather_args(const NraysScene* sc, const OcclusionIn& in, const NraysGatherParams* p, const float* out_rgb, uint32_t flags, bool hinted) {
    if (!sc || !in.points || !in.normals || !p || !p->dirs || !out_rgb) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (p->num_dirs < 1u || p->num_dirs > 1024u) return set_last_error(NRAYS_ERR_BAD_ARG, "NraysGatherParams: num_dirs must be in 1 .. 1024");
    if (p->num_rotations > 1024u || (p->num_rotations && !p->rotations)) return set_last_error(NRAYS_ERR_BAD_ARG, "NraysGatherParams: num_rotations > 1024, or rotations is NULL");
    if (!std::isfinite(p->bias) || !std::isfinite(p->energy)) return set_last_error(NRAYS_ERR_BAD_ARG, "NraysGatherParams: bias and energy must be finite");
    if (hinted) return check_ray_flags(flags);
    if (flags != 0u) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_gather_points: flags must be 0");
    return NRAYS_OK;
}
// A hinted call is reordered by the rule of the other batches, applied to its rays: n * num_dirs of them.
static bool gather_reorders(const NraysScene* sc, uint32_t n, const NraysGatherParams* p, uint32_t flags) {
    return (flags & NRAYS_RAYS_UNORDERED) && reorder_pays(sc, (uint32_t)std::min<uint64_t>((uint64_t)n * p->num_dirs, 0xffffffffull));
}
static uint32_t gather_out_floats(uint32_t bands) { return bands ? 3u * bands * bands : 3u; } // floats a point of the output: the mean colour, or bands^2 coefficients of three channels
static int check_sh_bands(uint32_t bands) {
    if (bands < 1u || bands > 3u) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_gather_sh_points: bands must be in 1 .. 3");
    return NRAYS_OK;
}
static uint32_t gather_chunk(const NraysGatherParams* p) { return std::max<uint32_t>(1u, kTraceChunk / p->num_dirs); } // points per chunk: at most kTraceChunk rays
// Double-branching scenes: the fold that k_gather_points left to the end of the chunk's k_bounce rounds — point i's num_dirs finished ray colours, summed in the
// order of j in f32 and divided once.  One lane per point; the colours were just written and sit in L2.
__global__ void __launch_bounds__(kOrderBlock) k_gather_fold(const float* __restrict__ rays, uint32_t n, uint32_t k, float* __restrict__ out) {
    const uint32_t i = blockIdx.x * kOrderBlock + threadIdx.x;
    if (i >= n) return;
    const float* c = rays + 3 * (size_t)i * k;
    float x = 0.0f, y = 0.0f, z = 0.0f;
    for (uint32_t j = 0; j < k; ++j) { x += c[3 * j]; y += c[3 * j + 1]; z += c[3 * j + 2]; }
    const float fk = (float)k;
    out[3 * (size_t)i] = x / fk; out[3 * (size_t)i + 1] = y / fk; out[3 * (size_t)i + 2] = z / fk;
}
// One chunk (nc <= gather_chunk) of nrays_gather_points_device; `in` and `out` are the chunk's, key_base the index of its first point in the batch, dirs / rotations
// device copies of the tables.  The permutation is trace_chunk's, the lanes per point are occlusion_chunk_launch's.  Double-branching scenes: the kernel stores the
// chunk's ray colours, trace_chunk's rounds run over the queued second children with a ray as the "pixel" (queue and sums sized by the chunk's RAYS, by trace_chunk's
// rule), and k_gather_fold folds: the only case with per-ray memory, 36 bytes a ray of the workspace beside the queue.
// The reorder of one gather chunk's pairs (pairs = nc * num_dirs <= kTraceChunk), enqueued on `stream` as ray_order_chunk enqueues a ray chunk's: launches only.
// Afterwards w->d_ray_order[0 .. m) holds the m live pairs in trace order and w->d_ray_bins[2^B] holds m; d_ray_keys / d_ray_frame hold the live pairs' keys and the frame.
static int gather_order_chunk(const NraysScene* sc, TraceWorkspace* w, uint32_t pairs, const GatherPoints& in, const OcclusionSpec& G, const double* dirs, const double* rotations,
                              hipStream_t stream) {
    if (pairs == 0u || pairs > w->order_rays) return set_last_error(NRAYS_ERR_BAD_ARG, "gather_order_chunk: workspace too small");
    SceneBox box;
    for (int a = 0; a < 3; ++a) { box.v[a] = (double)sc->facts.host.bounds_mn[a]; box.v[3 + a] = (double)sc->facts.host.bounds_mx[a]; }
    const uint32_t pair_grid = (pairs + kOrderBlock - 1u) / kOrderBlock, parts = pair_grid < kBoundsMaxGrid ? pair_grid : kBoundsMaxGrid;
    const uint32_t words = kNumBins + 1u, scan_grid = (words + kScanBlock - 1u) / kScanBlock; // (the last word stays zero and becomes the total)
    HIP_TRY(hipMemsetAsync(w->d_ray_bins, 0, (size_t)words * sizeof(uint32_t), stream));
    hipLaunchKernelGGL(k_gather_bounds, dim3(parts), dim3(kOrderBlock), 0, stream, pairs, in, G, dirs, rotations, box, w->d_ray_partial);
    hipLaunchKernelGGL(k_ray_frame, dim3(1), dim3(kOrderBlock), 0, stream, (const double*)w->d_ray_partial, parts, box, w->d_ray_frame);
    hipLaunchKernelGGL(k_gather_keys, dim3(pair_grid), dim3(kOrderBlock), 0, stream, pairs, in, G, dirs, rotations, (const double*)w->d_ray_frame, w->d_ray_keys, w->d_ray_bins, w->d_ray_rank);
    hipLaunchKernelGGL(k_bin_sums, dim3(scan_grid), dim3(kOrderBlock), 0, stream, (const uint32_t*)w->d_ray_bins, words, w->d_ray_scan);
    hipLaunchKernelGGL(k_bin_scan, dim3(1), dim3(1024), 0, stream, w->d_ray_scan, scan_grid);
    hipLaunchKernelGGL(k_bin_apply, dim3(scan_grid), dim3(kOrderBlock), 0, stream, w->d_ray_bins, words, (const uint32_t*)w->d_ray_scan);
    hipLaunchKernelGGL(k_gather_place, dim3(pair_grid), dim3(kOrderBlock), 0, stream, pairs, G.num_dirs, in.hit_flags, (const uint64_t*)w->d_ray_keys, (const uint32_t*)w->d_ray_rank,
                       (const uint32_t*)w->d_ray_bins, w->d_ray_order);
    HIP_TRY(hipGetLastError());
    return NRAYS_OK;
}

// One chunk (nc <= gather_chunk) of nrays_gather_points_device; `in` and `out` are the chunk's, key_base the index of its first point in the batch, dirs / rotations
// device copies of the tables.  The permutation is trace_chunk's, the lanes per point are occlusion_chunk_launch's.  Double-branching scenes: the kernel stores the
// chunk's ray colours, trace_chunk's rounds run over the queued second children with a ray as the "pixel" (queue and sums sized by the chunk's RAYS, by trace_chunk's
// rule), and k_gather_fold folds: the only case with per-ray memory, 36 bytes a ray of the workspace beside the queue.
// `reorder` (a hinted call that pays, nrays_gather_points*_ex): the chunk's pairs are binned (gather_order_chunk) and traced in bin order by k_gather_pairs_ordered, every
// scene through the cleared per-ray colours and k_gather_fold: 12 bytes of colour and 16 of sort state a ray of the chunk, whatever the scene.
// `bands` > 0 (nrays_gather_sh_points*): the same trace kernels, always through the per-ray colours — queued or not, reordered or not —, and k_gather_fold_sh
// (gather_sh_kernel.h) folds them into 3 * bands^2 floats a point of `out` instead of k_gather_fold's 3.
static int gather_chunk_launch(NraysScene* sc, TraceWorkspace* w, uint32_t nc, const OcclusionIn& in, unsigned long long key_base, const NraysGatherParams* p,
                               const double* dirs, const double* rotations, float* out, bool reorder, uint32_t bands, hipStream_t stream) {
    const bool queued = sc->facts.host.any_double_branch;
    const uint32_t pairs = nc * p->num_dirs; // (<= kTraceChunk)
    const size_t ray_floats = 3 * (size_t)pairs;
    if (queued) {
        const uint64_t want = std::min<uint64_t>(std::max<uint64_t>(4ull * pairs, 1u << 16), 1ull << 27);
        int rc = ensure_queue_pair(w->queue, w->queue_capacity, (uint32_t)want);
        if (rc == NRAYS_OK) rc = ensure_fixed_sums(&w->d_fixed, &w->fixed_slots, &w->fixed_dirty, ray_floats, stream);
        if (rc != NRAYS_OK) return rc;
    }
    const bool per_ray = queued || reorder || bands != 0u;
    if (per_ray) {
        const int rc = grow_device(&w->d_gather_rays, &w->gather_ray_floats, ray_floats, sizeof(float));
        if (rc != NRAYS_OK) return rc;
    }
    float* ray_out = per_ray ? (float*)w->d_gather_rays : nullptr;
    HIP_TRY(hipMemsetAsync(w->d_counts, 0, kTraceCountWords * sizeof(uint32_t), stream));
    unsigned int* overflow = w->d_counts + kTraceCountWords - 1;
    QueueOut qo; qo.q = w->queue[1].q; qo.capacity = queued ? w->queue_capacity : 0u; qo.count = w->d_counts + 1; qo.overflow = overflow;
    const GatherSpec spec{p->num_dirs, p->num_rotations, p->bias, p->energy, p->max_depth, sc->facts.host.any_area_light ? 1u : 0u};
    const bool stats = sc->facts.d.no_elide != 0u;
    const int feat = !stats && batch_mesh_only(sc) ? (int)kFeatMesh : (int)kFeatAll;
    if (reorder) {
        const GatherPoints pts{in.points, in.normals, in.hit_flags, (const unsigned long long*)in.keys, key_base};
        int rc = ray_order_ensure(w, pairs);
        if (rc == NRAYS_OK) rc = gather_order_chunk(sc, w, pairs, pts, OcclusionSpec{p->num_dirs, p->num_rotations, p->bias, 0.0}, dirs, rotations, stream);
        if (rc != NRAYS_OK) return rc;
        HIP_TRY(hipMemsetAsync(ray_out, 0, ray_floats * sizeof(float), stream)); // (a skipped point's pairs are never traced: exact zeros)
        const uint32_t grid = std::min<uint32_t>((pairs + kBlock - 1) / kBlock, (uint32_t)kMaxGrid); // (by the chunk's pairs: the live count stays on the device)
        const GatherPairsLaunch a{grid, stream, &sc->facts.d, pairs, w->d_ray_order, w->d_ray_bins + kNumBins, pts, spec, dirs, rotations, ray_out, &qo, w->d_counters, w->d_spill};
        if (!launch_gather_pairs_ordered(a, stats, feat)) return set_last_error(NRAYS_ERR_UNSUPPORTED, "k_gather_pairs_ordered: no such permutation");
    } else {
        const int lp = occlusion_lanes_log2(sc, p->num_dirs);
        const uint32_t slots = nc << lp; // (2^lp <= num_dirs)
        const uint32_t grid = std::min<uint32_t>((slots + kBlock - 1) / kBlock, (uint32_t)kMaxGrid);
        const GatherLaunch a{grid, stream, &sc->facts.d, nc, in.points, in.normals, in.hit_flags, (const unsigned long long*)in.keys, key_base, spec, dirs, rotations, out, ray_out, &qo,
                             w->d_counters, w->d_spill};
        if (!launch_gather_points(a, stats, feat, lp)) return set_last_error(NRAYS_ERR_UNSUPPORTED, "k_gather_points: no such permutation");
    }
    HIP_TRY(hipGetLastError());
    if (!ray_out) return NRAYS_OK;
    uint32_t overflowed = 0u;
    if (queued) {
        const BounceRounds rounds{w->queue, w->queue_capacity, w->d_counts, overflow, w->d_fixed, &w->fixed_dirty, w->d_counters, w->d_spill, &sc->facts.d, stats, p->max_depth, ray_out, ray_floats, sc->facts.num_cus};
        const int rc = run_bounce_rounds(rounds, stream, &overflowed);
        if (rc != NRAYS_OK) return rc;
    }
    if (bands) {
        const GatherPoints pts{in.points, in.normals, in.hit_flags, (const unsigned long long*)in.keys, key_base};
        const uint32_t grid = std::min<uint32_t>((nc + kShGroups - 1u) / kShGroups, kShMaxGrid);
        hipLaunchKernelGGL(k_gather_fold_sh, dim3(grid), dim3(kShBlock), 0, stream, (const float*)ray_out, nc, pts, OcclusionSpec{p->num_dirs, p->num_rotations, p->bias, 0.0}, dirs,
                           rotations, bands * bands, out);
    } else {
        hipLaunchKernelGGL(k_gather_fold, dim3((nc + kOrderBlock - 1u) / kOrderBlock), dim3(kOrderBlock), 0, stream, (const float*)ray_out, nc, p->num_dirs, out);
    }
    HIP_TRY(hipGetLastError());
    if (overflowed) return set_last_error(NRAYS_ERR_QUEUE_OVERFLOW, "continuation-ray queue overflow: some gathered colours are incomplete");
    return NRAYS_OK;
}

// `bands` = 0: nrays_gather_points* (3 floats a point); 1 .. 3: nrays_gather_sh_points* (3 * bands^2 floats a point), checked by the caller.
static int gather_points_device_impl(NraysScene* sc, uint32_t n, const OcclusionIn& in, const NraysGatherParams* p, float* out_rgb, uint32_t flags, bool hinted, uint32_t bands,
                                     hipStream_t stream) {
    if (check_gather_args(sc, in, p, out_rgb, flags, hinted) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    if (n == 0) return NRAYS_OK;
    HIP_TRY(hipSetDevice(sc->facts.device));
    TraceWorkspace* w = nullptr;
    int rc = trace_workspace(sc, &w);
    if (rc == NRAYS_OK) rc = batch_begin(sc, w, stream);
    if (rc != NRAYS_OK) return rc;
    const uint32_t chunk = gather_chunk(p);
    const bool reorder = gather_reorders(sc, n, p, flags);
    for (uint32_t c0 = 0; c0 < n && rc == NRAYS_OK; c0 += std::min<uint32_t>(n - c0, chunk)) {
        const uint32_t nc = std::min<uint32_t>(n - c0, chunk);
        rc = gather_chunk_launch(sc, w, nc, occlusion_in_at(in, c0), (unsigned long long)c0, p, p->dirs, p->rotations, out_rgb + gather_out_floats(bands) * (size_t)c0, reorder, bands,
                                 stream);
    }
    batch_end(sc, w, stream);
    return rc;
}

// The blocking form, through the workspace's staging buffer as occlusion_points_host_impl: the two tables first, then per staged point gather_stage_bytes() —
// point, normal (3 f64), key (u64), the output (3 f32, or 3 * bands^2 for the spherical-harmonic form), hit flags (32 bits), the 8-byte fields first.
static size_t gather_stage_bytes(uint32_t bands) { return 60u + 4u * (size_t)gather_out_floats(bands); }
static int gather_points_host_impl(NraysScene* sc, uint32_t n, const OcclusionIn& in, const NraysGatherParams* p, float* out_rgb, uint32_t flags, bool hinted, uint32_t bands) {
    if (check_gather_args(sc, in, p, out_rgb, flags, hinted) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    if (n == 0) return NRAYS_OK;
    HIP_TRY(hipSetDevice(sc->facts.device));
    TraceWorkspace* w = nullptr;
    int rc = trace_workspace(sc, &w);
    if (rc != NRAYS_OK) return rc;
    const uint32_t chunk = gather_chunk(p);
    const size_t cap = std::min<uint32_t>(n, chunk), table = 3 * (size_t)p->num_dirs + 2 * (size_t)p->num_rotations;
    rc = grow_device(&w->d_stage, &w->stage_rays, (table * sizeof(double) + cap * gather_stage_bytes(bands) + kStageUnit - 1) / kStageUnit, kStageUnit);
    if (rc != NRAYS_OK) return rc;
    double* s_dirs = (double*)w->d_stage; double* s_rot = s_dirs + 3 * (size_t)p->num_dirs; double* s_p = s_dirs + table; double* s_n = s_p + 3 * cap;
    const size_t out_floats = gather_out_floats(bands);
    uint64_t* s_k = (uint64_t*)(s_n + 3 * cap); float* s_c = (float*)(s_k + cap); uint32_t* s_hf = (uint32_t*)(s_c + out_floats * cap);
    const OcclusionIn s{s_p, s_n, in.hit_flags ? s_hf : nullptr, in.keys ? s_k : nullptr};
    rc = ensure_own_stream(sc);
    if (rc != NRAYS_OK) return rc;
    const hipStream_t stream = sc->buf.own_stream;
    rc = batch_begin(sc, w, stream);
    if (rc != NRAYS_OK) return rc;
    auto up = [&](void* dst, const void* src, size_t bytes) { return src && bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream) : hipSuccess; };
    hipError_t e = up(s_dirs, p->dirs, 24 * (size_t)p->num_dirs);
    if (e == hipSuccess) e = up(s_rot, p->rotations, 16 * (size_t)p->num_rotations);
    if (e != hipSuccess) rc = set_last_error(NRAYS_ERR_HIP, std::string("gather tables upload: ") + hipGetErrorString(e));
    const bool reorder = gather_reorders(sc, n, p, flags);
    for (uint32_t c0 = 0; c0 < n && rc == NRAYS_OK; c0 += std::min<uint32_t>(n - c0, chunk)) {
        const uint32_t nc = std::min<uint32_t>(n - c0, chunk);
        const OcclusionIn h = occlusion_in_at(in, c0);
        e = up(s_p, h.points, (size_t)nc * 24);
        if (e == hipSuccess) e = up(s_n, h.normals, (size_t)nc * 24);
        if (e == hipSuccess) e = up(s_hf, h.hit_flags, (size_t)nc * 4);
        if (e == hipSuccess) e = up(s_k, h.keys, (size_t)nc * 8);
        if (e != hipSuccess) { rc = set_last_error(NRAYS_ERR_HIP, std::string("gather batch upload: ") + hipGetErrorString(e)); break; }
        rc = gather_chunk_launch(sc, w, nc, s, (unsigned long long)c0, p, s_dirs, p->num_rotations ? s_rot : nullptr, s_c, reorder, bands, stream);
        if (rc != NRAYS_OK) break;
        e = hipMemcpyAsync(out_rgb + out_floats * (size_t)c0, s_c, (size_t)nc * out_floats * sizeof(float), hipMemcpyDeviceToHost, stream);
        const hipError_t es = hipStreamSynchronize(stream); // (always: the staging buffer is reused by the next chunk and the next call)
        if (e == hipSuccess) e = es;
        if (e != hipSuccess) rc = set_last_error(NRAYS_ERR_HIP, std::string("gather batch read-back: ") + hipGetErrorString(e));
    }
    if (rc != NRAYS_OK) (void)hipStreamSynchronize(stream); // (the tables' upload reads the caller's memory)
    batch_end(sc, w, stream);
    return rc;
}

// ---- nrays_gather_maps_points*: the light of baked maps at the closest hits of the hemisphere rays of caller-supplied points (gather_maps_kernel.h) -------------
static int check_gather_maps_args(const NraysScene* sc, const OcclusionIn& in, const NraysGatherMapsParams* p, const float* out_rgb, uint32_t flags) {
    if (!sc || !in.points || !in.normals || !p || !p->dirs || !p->maps || !p->node_map || !out_rgb) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (p->num_dirs < 1u || p->num_dirs > 1024u) return set_last_error(NRAYS_ERR_BAD_ARG, "NraysGatherMapsParams: num_dirs must be in 1 .. 1024");
    if (p->num_rotations > 1024u || (p->num_rotations && !p->rotations)) return set_last_error(NRAYS_ERR_BAD_ARG, "NraysGatherMapsParams: num_rotations > 1024, or rotations is NULL");
    if (!std::isfinite(p->bias) || !std::isfinite(p->miss_rgb[0]) || !std::isfinite(p->miss_rgb[1]) || !std::isfinite(p->miss_rgb[2]))
        return set_last_error(NRAYS_ERR_BAD_ARG, "NraysGatherMapsParams: bias and miss_rgb must be finite");
    if (!(p->max_toi > 0.0)) return set_last_error(NRAYS_ERR_BAD_ARG, "NraysGatherMapsParams: max_toi must be > 0 (+inf allowed)");
    if (p->num_maps < 1u || p->num_maps > NRAYS_GATHER_MAX_MAPS) return set_last_error(NRAYS_ERR_BAD_ARG, "NraysGatherMapsParams: num_maps must be in 1 .. 16");
    if (p->num_nodes != (uint32_t)sc->facts.host.shade.size()) return set_last_error(NRAYS_ERR_BAD_ARG, "NraysGatherMapsParams: num_nodes is not the scene's node count");
    for (uint32_t m = 0; m < p->num_maps; ++m) {
        const NraysTexture& t = p->maps[m];
        if (!t.texels || t.width == 0u || t.height == 0u) return set_last_error(NRAYS_ERR_BAD_ARG, "NraysGatherMapsParams: a map without texels");
        if (t.format != NRAYS_TEXEL_RGBA32F) return set_last_error(NRAYS_ERR_BAD_ARG, "NraysGatherMapsParams: a map's format must be NRAYS_TEXEL_RGBA32F");
        if ((t.interp != NRAYS_INTERP_BILINEAR && t.interp != NRAYS_INTERP_NEAREST) || (t.overflow != NRAYS_OVERFLOW_WRAP && t.overflow != NRAYS_OVERFLOW_CLAMP))
            return set_last_error(NRAYS_ERR_BAD_ARG, "NraysGatherMapsParams: a map's interp or overflow is unknown");
    }
    if (flags != 0u) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_gather_maps_points: flags must be 0");
    return NRAYS_OK;
}
static uint32_t gather_maps_chunk(const NraysGatherMapsParams* p) { return std::max<uint32_t>(1u, kTraceChunk / p->num_dirs); } // points per chunk: at most kTraceChunk rays
// The kernel's view of the checked parameters: the map records as the shading records hold a texture (ShadeTex), texel address `texels[m]`.
static void gather_maps_table(const NraysGatherMapsParams* p, const void* const* texels, GatherMapsTable* t) {
    std::memset(t, 0, sizeof *t);
    for (uint32_t m = 0; m < p->num_maps; ++m) {
        const NraysTexture& s = p->maps[m];
        t->map[m].texels = texels[m]; t->map[m].width = s.width; t->map[m].height = s.height; t->map[m].mode = s.format | (s.interp << 8) | (s.overflow << 16);
    }
}
// One chunk (nc <= gather_maps_chunk) of nrays_gather_maps_points_device; `in` and the outputs are the chunk's, key_base the index of its first point in the batch,
// node_map / dirs / rotations and the table's texels device memory.  The permutation is cast_chunk's, the lanes per point are occlusion_chunk_launch's.
static int gather_maps_chunk_launch(NraysScene* sc, TraceWorkspace* w, uint32_t nc, const OcclusionIn& in, unsigned long long key_base, const NraysGatherMapsParams* p,
                                    const GatherMapsTable& table, const int32_t* node_map, const double* dirs, const double* rotations, float* out_rgb, uint32_t* out_counts,
                                    hipStream_t stream) {
    const bool mesh = (sc->facts.features & ~(int)kFeatMultiSample) == (int)kFeatMesh; // (traversal only: as nrays_cast_rays_device)
    const int lp = occlusion_lanes_log2(sc, p->num_dirs);
    const uint32_t slots = nc << lp; // (nc * num_dirs <= kTraceChunk and 2^lp <= num_dirs)
    const uint32_t grid = std::min<uint32_t>((slots + kBlock - 1) / kBlock, (uint32_t)kMaxGrid);
    const GatherMapsSpec spec{p->num_dirs, p->num_rotations, p->bias, p->max_toi, p->num_maps, p->num_nodes, {p->miss_rgb[0], p->miss_rgb[1], p->miss_rgb[2]}};
    const GatherMapsLaunch a{grid, stream, &sc->facts.d, nc, in.points, in.normals, in.hit_flags, (const unsigned long long*)in.keys, key_base, spec, &table, node_map, dirs, rotations,
                             out_rgb, out_counts, w->d_spill};
    if (!launch_gather_maps_points(a, mesh ? (int)kFeatMesh : (int)kFeatAll, lp)) return set_last_error(NRAYS_ERR_UNSUPPORTED, "k_gather_maps_points: no such permutation");
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_last_error(NRAYS_ERR_HIP, std::string("k_gather_maps_points: ") + hipGetErrorString(e));
    return NRAYS_OK;
}

static int gather_maps_device_impl(NraysScene* sc, uint32_t n, const OcclusionIn& in, const NraysGatherMapsParams* p, float* out_rgb, uint32_t* out_counts, uint32_t flags,
                                   hipStream_t stream) {
    if (check_gather_maps_args(sc, in, p, out_rgb, flags) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    if (n == 0) return NRAYS_OK;
    HIP_TRY(hipSetDevice(sc->facts.device));
    TraceWorkspace* w = nullptr;
    int rc = trace_workspace(sc, &w);
    if (rc == NRAYS_OK) rc = batch_begin(sc, w, stream);
    if (rc != NRAYS_OK) return rc;
    const void* texels[NRAYS_GATHER_MAX_MAPS] = {};
    for (uint32_t m = 0; m < p->num_maps; ++m) texels[m] = p->maps[m].texels;
    GatherMapsTable table;
    gather_maps_table(p, texels, &table);
    const uint32_t chunk = gather_maps_chunk(p);
    for (uint32_t c0 = 0; c0 < n && rc == NRAYS_OK; c0 += std::min<uint32_t>(n - c0, chunk)) {
        const uint32_t nc = std::min<uint32_t>(n - c0, chunk);
        rc = gather_maps_chunk_launch(sc, w, nc, occlusion_in_at(in, c0), (unsigned long long)c0, p, table, p->node_map, p->dirs, p->rotations, out_rgb + 3 * (size_t)c0,
                                      out_counts ? out_counts + 2 * (size_t)c0 : nullptr, stream);
    }
    batch_end(sc, w, stream);
    return rc;
}

// The blocking form, through the workspace's staging buffer as gather_points_host_impl: the two tables first, then the maps' texels (16 bytes each, on a 16-byte
// boundary), node_map (padded to 8 bytes), then per staged point kGatherMapsStageBytes — point, normal (3 f64), key (u64), colour (3 f32), hit flags, the two
// counts (32 bits each), the 8-byte fields first.
constexpr size_t kGatherMapsStageBytes = 80;
static int gather_maps_host_impl(NraysScene* sc, uint32_t n, const OcclusionIn& in, const NraysGatherMapsParams* p, float* out_rgb, uint32_t* out_counts, uint32_t flags) {
    if (check_gather_maps_args(sc, in, p, out_rgb, flags) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    if (n == 0) return NRAYS_OK;
    HIP_TRY(hipSetDevice(sc->facts.device));
    TraceWorkspace* w = nullptr;
    int rc = trace_workspace(sc, &w);
    if (rc != NRAYS_OK) return rc;
    const uint32_t chunk = gather_maps_chunk(p);
    const size_t cap = std::min<uint32_t>(n, chunk);
    const size_t table_bytes = (24 * (size_t)p->num_dirs + 16 * (size_t)p->num_rotations + 15) / 16 * 16;
    size_t texel_bytes = 0;
    for (uint32_t m = 0; m < p->num_maps; ++m) texel_bytes += 16 * (size_t)p->maps[m].width * p->maps[m].height;
    const size_t node_bytes = (4 * (size_t)p->num_nodes + 7) / 8 * 8;
    rc = grow_device(&w->d_stage, &w->stage_rays, (table_bytes + texel_bytes + node_bytes + cap * kGatherMapsStageBytes + kStageUnit - 1) / kStageUnit, kStageUnit);
    if (rc != NRAYS_OK) return rc;
    char* base = (char*)w->d_stage;
    double* s_dirs = (double*)base; double* s_rot = s_dirs + 3 * (size_t)p->num_dirs;
    char* s_tex = base + table_bytes;
    int32_t* s_nodes = (int32_t*)(s_tex + texel_bytes);
    double* s_p = (double*)((char*)s_nodes + node_bytes); double* s_n = s_p + 3 * cap;
    uint64_t* s_k = (uint64_t*)(s_n + 3 * cap); float* s_c = (float*)(s_k + cap); uint32_t* s_hf = (uint32_t*)(s_c + 3 * cap); uint32_t* s_cnt = s_hf + cap;
    const OcclusionIn s{s_p, s_n, in.hit_flags ? s_hf : nullptr, in.keys ? s_k : nullptr};
    rc = ensure_own_stream(sc);
    if (rc != NRAYS_OK) return rc;
    const hipStream_t stream = sc->buf.own_stream;
    rc = batch_begin(sc, w, stream);
    if (rc != NRAYS_OK) return rc;
    auto up = [&](void* dst, const void* src, size_t bytes) { return src && bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream) : hipSuccess; };
    hipError_t e = up(s_dirs, p->dirs, 24 * (size_t)p->num_dirs);
    if (e == hipSuccess) e = up(s_rot, p->rotations, 16 * (size_t)p->num_rotations);
    if (e == hipSuccess) e = up(s_nodes, p->node_map, 4 * (size_t)p->num_nodes);
    const void* texels[NRAYS_GATHER_MAX_MAPS] = {};
    size_t off = 0;
    for (uint32_t m = 0; m < p->num_maps && e == hipSuccess; ++m) {
        const size_t bytes = 16 * (size_t)p->maps[m].width * p->maps[m].height;
        texels[m] = s_tex + off;
        e = up(s_tex + off, p->maps[m].texels, bytes);
        off += bytes;
    }
    if (e != hipSuccess) rc = set_last_error(NRAYS_ERR_HIP, std::string("gather maps tables upload: ") + hipGetErrorString(e));
    GatherMapsTable table;
    gather_maps_table(p, texels, &table);
    for (uint32_t c0 = 0; c0 < n && rc == NRAYS_OK; c0 += std::min<uint32_t>(n - c0, chunk)) {
        const uint32_t nc = std::min<uint32_t>(n - c0, chunk);
        const OcclusionIn h = occlusion_in_at(in, c0);
        e = up(s_p, h.points, (size_t)nc * 24);
        if (e == hipSuccess) e = up(s_n, h.normals, (size_t)nc * 24);
        if (e == hipSuccess) e = up(s_hf, h.hit_flags, (size_t)nc * 4);
        if (e == hipSuccess) e = up(s_k, h.keys, (size_t)nc * 8);
        if (e != hipSuccess) { rc = set_last_error(NRAYS_ERR_HIP, std::string("gather maps batch upload: ") + hipGetErrorString(e)); break; }
        rc = gather_maps_chunk_launch(sc, w, nc, s, (unsigned long long)c0, p, table, s_nodes, s_dirs, p->num_rotations ? s_rot : nullptr, s_c, out_counts ? s_cnt : nullptr, stream);
        if (rc != NRAYS_OK) break;
        e = hipMemcpyAsync(out_rgb + 3 * (size_t)c0, s_c, (size_t)nc * 12, hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess && out_counts) e = hipMemcpyAsync(out_counts + 2 * (size_t)c0, s_cnt, (size_t)nc * 8, hipMemcpyDeviceToHost, stream);
        const hipError_t es = hipStreamSynchronize(stream); // (always: the staging buffer is reused by the next chunk and the next call)
        if (e == hipSuccess) e = es;
        if (e != hipSuccess) rc = set_last_error(NRAYS_ERR_HIP, std::string("gather maps batch read-back: ") + hipGetErrorString(e));
    }
    if (rc != NRAYS_OK) (void)hipStreamSynchronize(stream); // (the tables' upload reads the caller's memory)
    batch_end(sc, w, stream);
    return rc;
}

// nrays_debug_occlusion_rays: ray j of point i, as k_occlusion_points generates it, to out[(i * num_dirs + j) * 3 ..].
__global__ void __launch_bounds__(kBlock) k_occlusion_rays(uint32_t n, const double* __restrict__ points, const double* __restrict__ normals,
                                                           const unsigned long long* __restrict__ keys, OcclusionSpec P, const double* __restrict__ dirs,
                                                           const double* __restrict__ rotations, double* __restrict__ out_origins, double* __restrict__ out_dirs) {
    const size_t rays = (size_t)n * P.num_dirs;
    for (size_t r = (size_t)blockIdx.x * kBlock + threadIdx.x; r < rays; r += (size_t)gridDim.x * kBlock) {
        const size_t i = r / P.num_dirs, j = r % P.num_dirs;
        const OccFrame f = occlusion_frame(D3(points[3 * i], points[3 * i + 1], points[3 * i + 2]), D3(normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]),
                                           keys ? keys[i] : (unsigned long long)i, P, rotations);
        const d3 d = occlusion_dir(f, P.num_rotations != 0u, dirs[3 * j], dirs[3 * j + 1], dirs[3 * j + 2]);
        out_origins[3 * r] = f.o.x; out_origins[3 * r + 1] = f.o.y; out_origins[3 * r + 2] = f.o.z;
        out_dirs[3 * r] = d.x; out_dirs[3 * r + 1] = d.y; out_dirs[3 * r + 2] = d.z;
    }
}

// nrays_debug_occlusion_rays: the generator of k_occlusion_points alone, on host arrays, blocking; buffers of its own (a test probe).
static int occlusion_rays_probe(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint64_t* keys, const NraysOcclusionParams* p,
                                double* out_origins, double* out_dirs) {
    if (!sc || !points || !normals || !out_origins || !out_dirs) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (check_occlusion_params(p) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    if (n == 0) return NRAYS_OK;
    HIP_TRY(hipSetDevice(sc->facts.device));
    int rc = ensure_own_stream(sc);
    if (rc != NRAYS_OK) return rc;
    const hipStream_t stream = sc->buf.own_stream;
    const size_t rays = (size_t)n * p->num_dirs, table = 3 * (size_t)p->num_dirs + 2 * (size_t)p->num_rotations;
    const size_t doubles = table + 6 * (size_t)n + (keys ? n : 0) + 6 * rays;
    double* d_all = nullptr;
    {
        const hipError_t e = hipMalloc((void**)&d_all, doubles * sizeof(double));
        if (e != hipSuccess) return set_last_error(e == hipErrorOutOfMemory ? NRAYS_ERR_OOM : NRAYS_ERR_HIP, std::string("occlusion probe: ") + hipGetErrorString(e));
    }
    double* d_dirs = d_all; double* d_rot = d_dirs + 3 * (size_t)p->num_dirs; double* d_p = d_all + table; double* d_n = d_p + 3 * (size_t)n;
    double* d_k = d_n + 3 * (size_t)n; double* d_oo = d_k + (keys ? n : 0); double* d_od = d_oo + 3 * rays;
    auto up = [&](void* dst, const void* src, size_t bytes) { return src && bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream) : hipSuccess; };
    hipError_t e = up(d_dirs, p->dirs, 24 * (size_t)p->num_dirs);
    if (e == hipSuccess) e = up(d_rot, p->rotations, 16 * (size_t)p->num_rotations);
    if (e == hipSuccess) e = up(d_p, points, 24 * (size_t)n);
    if (e == hipSuccess) e = up(d_n, normals, 24 * (size_t)n);
    if (e == hipSuccess) e = up(d_k, keys, 8 * (size_t)n);
    if (e == hipSuccess) {
        const uint32_t grid = (uint32_t)std::min<size_t>((rays + kBlock - 1) / kBlock, (size_t)kMaxGrid);
        hipLaunchKernelGGL(k_occlusion_rays, dim3(grid), dim3(kBlock), 0, stream, n, (const double*)d_p, (const double*)d_n, keys ? (const unsigned long long*)d_k : nullptr,
                           occlusion_spec(p), (const double*)d_dirs, p->num_rotations ? (const double*)d_rot : nullptr, d_oo, d_od);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out_origins, d_oo, 24 * rays, hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out_dirs, d_od, 24 * rays, hipMemcpyDeviceToHost, stream);
    const hipError_t es = hipStreamSynchronize(stream);
    if (e == hipSuccess) e = es;
    (void)hipFree(d_all);
    if (e != hipSuccess) return set_last_error(NRAYS_ERR_HIP, std::string("occlusion probe: ") + hipGetErrorString(e));
    return NRAYS_OK;
}

// ---- nrays_surface_texels*: the surface of a TriMesh node at the points of a lattice in uv space (surface_texels_kernel.h) -----------------------------------------
constexpr uint32_t kTexelMaxSide = 16384u, kTexelMaxPoints = 1u << 24;
static int check_texel_args(const NraysScene* sc, uint32_t node, uint32_t width, uint32_t height, const TexelOutputs* out /* null: the caller has none (the probe) */, uint32_t flags) {
    if (!sc || (out && (!out->points || !out->flags))) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (node >= sc->facts.host.surface.size()) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_surface_texels: no such node");
    if (width < 1u || width > kTexelMaxSide || height < 1u || height > kTexelMaxSide || (uint64_t)width * height > kTexelMaxPoints)
        return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_surface_texels: width and height must be in 1 .. 16384 and width * height <= 2^24");
    if (flags & ~(uint32_t)(NRAYS_TEXELS_CENTRES | NRAYS_TEXELS_FLIP_NORMALS)) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_surface_texels: unknown flag");
    const NodeSurface& s = sc->facts.host.surface[node];
    if (!s.mesh) return set_last_error(NRAYS_ERR_UNSUPPORTED, "nrays_surface_texels: the node is not a TriMesh");
    if (!s.has_uv) return set_last_error(NRAYS_ERR_UNSUPPORTED, "nrays_surface_texels: the node's mesh has no uvs");
    return NRAYS_OK;
}
static int texel_workspace(TraceWorkspace* w, size_t points, size_t records) {
    int rc = grow_device(&w->d_texel_owner, &w->texel_owner_words, points, sizeof(unsigned long long));
    if (rc == NRAYS_OK) rc = grow_device(&w->d_texel_off, &w->texel_off_words, std::max<size_t>(records, 1), sizeof(unsigned long long));
    if (rc != NRAYS_OK) return rc;
    if (!w->d_texel_blocks) HIP_TRY(hipMalloc((void**)&w->d_texel_blocks, (size_t)(kTexelMaxBlocks + 1u) * sizeof(unsigned long long)));
    return NRAYS_OK;
}
// The owner pass of one call: memset, count, scan, items.  Launches only; texel_workspace() has run.
static int texel_owner_pass(NraysScene* sc, TraceWorkspace* w, uint32_t node, uint32_t width, uint32_t height, uint32_t flags, hipStream_t stream) {
    const NodeSurface& s = sc->facts.host.surface[node];
    const TexelLattice L{width, height, (flags & NRAYS_TEXELS_CENTRES) ? 1u : 0u, node};
    unsigned long long* owner = (unsigned long long*)w->d_texel_owner; unsigned long long* off = (unsigned long long*)w->d_texel_off;
    HIP_TRY(hipMemsetAsync(owner, 0xff, (size_t)width * height * sizeof(unsigned long long), stream));
    if (s.count == 0u) return NRAYS_OK;
    if (s.count > kTexelMaxRecords) return set_last_error(NRAYS_ERR_UNSUPPORTED, "nrays_surface_texels: too many triangle records");
    const uint32_t rec_grid = (s.count + kTexelBlock - 1u) / kTexelBlock, scan_grid = (s.count + kTexelScanBlock - 1u) / kTexelScanBlock;
    unsigned long long* total = w->d_texel_blocks + kTexelMaxBlocks;
    hipLaunchKernelGGL(k_texel_count, dim3(rec_grid), dim3(kTexelBlock), 0, stream, sc->facts.d.tris, sc->facts.d.triuvs, s.first, s.count, L, off);
    hipLaunchKernelGGL(k_texel_sums, dim3(scan_grid), dim3(kTexelBlock), 0, stream, (const unsigned long long*)off, s.count, w->d_texel_blocks);
    hipLaunchKernelGGL(k_texel_scan, dim3(1), dim3(1024), 0, stream, w->d_texel_blocks, scan_grid, total);
    hipLaunchKernelGGL(k_texel_apply, dim3(scan_grid), dim3(kTexelBlock), 0, stream, off, s.count, (const unsigned long long*)w->d_texel_blocks);
    hipLaunchKernelGGL(k_texel_owner, dim3((uint32_t)sc->facts.num_cus * kTexelOwnerWgsPerCu), dim3(kTexelBlock), 0, stream, sc->facts.d.tris, sc->facts.d.triuvs, s.first, s.count, L,
                       (const unsigned long long*)off, (const unsigned long long*)total, owner);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_last_error(NRAYS_ERR_HIP, std::string("k_texel_owner: ") + hipGetErrorString(e));
    return NRAYS_OK;
}
static int texel_resolve_pass(NraysScene* sc, TraceWorkspace* w, uint32_t node, uint32_t width, uint32_t height, uint32_t flags, const TexelOutputs& out, hipStream_t stream) {
    const NodeSurface& s = sc->facts.host.surface[node];
    const TexelLattice L{width, height, (flags & NRAYS_TEXELS_CENTRES) ? 1u : 0u, node};
    TexelXform X;
    for (int k = 0; k < 9; ++k) X.m.r[k] = s.rot[k];
    X.m.t.x = s.trans[0]; X.m.t.y = s.trans[1]; X.m.t.z = s.trans[2];
    X.flags = s.flags; X.flip = (flags & NRAYS_TEXELS_FLIP_NORMALS) ? 1u : 0u;
    hipLaunchKernelGGL(k_texel_resolve, dim3((width * height + kTexelBlock - 1u) / kTexelBlock), dim3(kTexelBlock), 0, stream, sc->facts.d.tris, sc->facts.d.triuvs, L, X,
                       (const unsigned long long*)w->d_texel_owner, out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_last_error(NRAYS_ERR_HIP, std::string("k_texel_resolve: ") + hipGetErrorString(e));
    return NRAYS_OK;
}

static int surface_texels_device_impl(NraysScene* sc, uint32_t node, uint32_t width, uint32_t height, const TexelOutputs& out, uint32_t flags, hipStream_t stream) {
    { const int rc = check_texel_args(sc, node, width, height, &out, flags); if (rc != NRAYS_OK) return rc; }
    HIP_TRY(hipSetDevice(sc->facts.device));
    TraceWorkspace* w = nullptr;
    int rc = trace_workspace(sc, &w);
    if (rc == NRAYS_OK) rc = texel_workspace(w, (size_t)width * height, sc->facts.host.surface[node].count);
    if (rc == NRAYS_OK) rc = batch_begin(sc, w, stream);
    if (rc != NRAYS_OK) return rc;
    rc = texel_owner_pass(sc, w, node, width, height, flags, stream);
    if (rc == NRAYS_OK) rc = texel_resolve_pass(sc, w, node, width, height, flags, out, stream);
    batch_end(sc, w, stream);
    return rc;
}

// The blocking form, through the workspace's staging buffer as cast_rays_host_impl.  A staged lattice point takes kTexelStageBytes: point, normal (3 f64), uv (2 f64),
// node, prim, flags (32 bits) — the 8-byte fields first.
constexpr size_t kTexelStageBytes = 76;
static TexelOutputs texel_stage(void* block, size_t n, const TexelOutputs* want /* null: every output */) {
    TexelOutputs s; s.points = (double*)block; s.normals = s.points + 3 * n; s.uv = s.normals + 3 * n;
    s.node = (int32_t*)(s.uv + 2 * n); s.prim = s.node + n; s.flags = (uint32_t*)(s.prim + n);
    if (want && !want->normals) s.normals = nullptr;
    if (want && !want->uv) s.uv = nullptr;
    if (want && !want->node) s.node = nullptr;
    if (want && !want->prim) s.prim = nullptr;
    return s;
}
static int surface_texels_host_impl(NraysScene* sc, uint32_t node, uint32_t width, uint32_t height, const TexelOutputs& out, uint32_t flags) {
    { const int rc = check_texel_args(sc, node, width, height, &out, flags); if (rc != NRAYS_OK) return rc; }
    HIP_TRY(hipSetDevice(sc->facts.device));
    TraceWorkspace* w = nullptr;
    const size_t n = (size_t)width * height;
    int rc = trace_workspace(sc, &w);
    if (rc == NRAYS_OK) rc = texel_workspace(w, n, sc->facts.host.surface[node].count);
    if (rc == NRAYS_OK) rc = grow_device(&w->d_stage, &w->stage_rays, (n * kTexelStageBytes + kStageUnit - 1) / kStageUnit, kStageUnit);
    if (rc == NRAYS_OK) rc = ensure_own_stream(sc);
    if (rc != NRAYS_OK) return rc;
    const TexelOutputs s = texel_stage(w->d_stage, n, &out);
    const hipStream_t stream = sc->buf.own_stream;
    rc = batch_begin(sc, w, stream);
    if (rc != NRAYS_OK) return rc;
    rc = texel_owner_pass(sc, w, node, width, height, flags, stream);
    if (rc == NRAYS_OK) rc = texel_resolve_pass(sc, w, node, width, height, flags, s, stream);
    if (rc == NRAYS_OK) {
        auto down = [&](void* dst, const void* src, size_t bytes) { return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream) : hipSuccess; };
        hipError_t e = down(out.points, s.points, n * 24);
        if (e == hipSuccess) e = down(out.normals, s.normals, n * 24);
        if (e == hipSuccess) e = down(out.uv, s.uv, n * 16);
        if (e == hipSuccess) e = down(out.node, s.node, n * 4);
        if (e == hipSuccess) e = down(out.prim, s.prim, n * 4);
        if (e == hipSuccess) e = down(out.flags, s.flags, n * 4);
        const hipError_t es = hipStreamSynchronize(stream); // (always: the staging buffer is reused by the next call)
        if (e == hipSuccess) e = es;
        if (e != hipSuccess) rc = set_last_error(NRAYS_ERR_HIP, std::string("surface texels read-back: ") + hipGetErrorString(e));
    }
    batch_end(sc, w, stream);
    return rc;
}

// nrays_debug_surface_texels_passes: the two passes of nrays_surface_texels_device between events of their own, `repeats` times, into the staging buffer (a timing probe).
static int surface_texels_passes_probe(NraysScene* sc, uint32_t node, uint32_t width, uint32_t height, uint32_t flags, uint32_t repeats, float* out_ms) {
    { const int rc = check_texel_args(sc, node, width, height, nullptr, flags); if (rc != NRAYS_OK) return rc; }
    if (!out_ms || repeats == 0u) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    HIP_TRY(hipSetDevice(sc->facts.device));
    TraceWorkspace* w = nullptr;
    const size_t n = (size_t)width * height;
    int rc = trace_workspace(sc, &w);
    if (rc == NRAYS_OK) rc = texel_workspace(w, n, sc->facts.host.surface[node].count);
    if (rc == NRAYS_OK) rc = grow_device(&w->d_stage, &w->stage_rays, (n * kTexelStageBytes + kStageUnit - 1) / kStageUnit, kStageUnit);
    if (rc == NRAYS_OK) rc = ensure_own_stream(sc);
    if (rc != NRAYS_OK) return rc;
    const TexelOutputs s = texel_stage(w->d_stage, n, nullptr); // (every output)
    const hipStream_t stream = sc->buf.own_stream;
    rc = batch_begin(sc, w, stream);
    if (rc != NRAYS_OK) return rc;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    hipError_t e = hipSuccess;
    for (int k = 0; k < 3 && e == hipSuccess; ++k) e = hipEventCreate(&ev[k]);
    for (uint32_t r = 0; r < repeats && rc == NRAYS_OK && e == hipSuccess; ++r) {
        e = hipEventRecord(ev[0], stream);
        rc = texel_owner_pass(sc, w, node, width, height, flags, stream);
        if (e == hipSuccess) e = hipEventRecord(ev[1], stream);
        if (rc == NRAYS_OK) rc = texel_resolve_pass(sc, w, node, width, height, flags, s, stream);
        if (e == hipSuccess) e = hipEventRecord(ev[2], stream);
        if (e == hipSuccess) e = hipEventSynchronize(ev[2]);
        if (e == hipSuccess) e = hipEventElapsedTime(&out_ms[2 * r], ev[0], ev[1]);
        if (e == hipSuccess) e = hipEventElapsedTime(&out_ms[2 * r + 1], ev[1], ev[2]);
    }
    (void)hipStreamSynchronize(stream);
    for (int k = 0; k < 3; ++k) if (ev[k]) (void)hipEventDestroy(ev[k]);
    batch_end(sc, w, stream);
    if (rc == NRAYS_OK && e != hipSuccess) rc = set_last_error(NRAYS_ERR_HIP, std::string("nrays_debug_surface_texels_passes: ") + hipGetErrorString(e));
    return rc;
}

// ---- nrays_dilate_texels*: uncovered lattice points take the values of the nearest covered point within a radius (texel_dilate_kernel.h) -----------------------------
static_assert(kDilateMaxRadius == NRAYS_DILATE_MAX_RADIUS && kDilateFilled == NRAYS_TEXEL_FILLED, "texel_dilate_kernel.h restates the header's constants");
struct DilateArgs { uint32_t width, height; const uint32_t* flags_in; uint32_t radius, channels; float* values; int32_t* source; uint32_t* flags_out; };
static int check_dilate_args(const NraysScene* sc, const DilateArgs& a, uint32_t flags) {
    if (!sc || !a.flags_in) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (!a.values && !a.source && !a.flags_out) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_dilate_texels: no output (values, out_source and out_flags are all null)");
    if (a.values && (a.channels < 1u || a.channels > 4u)) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_dilate_texels: channels must be in 1 .. 4");
    if (a.radius < 1u || a.radius > NRAYS_DILATE_MAX_RADIUS) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_dilate_texels: radius must be in 1 .. 64");
    if (a.width < 1u || a.width > kTexelMaxSide || a.height < 1u || a.height > kTexelMaxSide || (uint64_t)a.width * a.height > kTexelMaxPoints)
        return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_dilate_texels: width and height must be in 1 .. 16384 and width * height <= 2^24");
    if (flags != 0u) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_dilate_texels: flags are reserved and must be 0");
    return NRAYS_OK;
}
// The two launches of one call.  The workspace holds width * height dx words.
static int dilate_passes(TraceWorkspace* w, const DilateArgs& a, hipStream_t stream) {
    const DilateLattice L{a.width, a.height, a.radius, (a.width + 63u) / 64u};
    int16_t* dx = (int16_t*)w->d_dilate_dx;
    const uint32_t T = a.radius <= kDilateShortRadius ? 16u : 64u; // (dilate_rows_per_group)
    const uint32_t vec4 = (a.values && a.channels == 4u && ((uintptr_t)a.values & 15u) == 0u) ? 1u : 0u;
    hipLaunchKernelGGL(k_dilate_rows, dim3((L.h * L.col_blocks + kDilateWaves - 1u) / kDilateWaves), dim3(kDilateBlock), 0, stream, L, a.flags_in, dx);
    hipLaunchKernelGGL(k_dilate_cols, dim3(L.col_blocks, (L.h + T - 1u) / T), dim3(kDilateBlock), (size_t)(T + 2u * a.radius) * 64u * sizeof(int16_t), stream, L,
                       (const int16_t*)dx, a.flags_in, a.values ? a.channels : 0u, vec4, a.values, a.source, a.flags_out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_last_error(NRAYS_ERR_HIP, std::string("k_dilate_cols: ") + hipGetErrorString(e));
    return NRAYS_OK;
}
static int dilate_texels_device_impl(NraysScene* sc, const DilateArgs& a, uint32_t flags, hipStream_t stream) {
    { const int rc = check_dilate_args(sc, a, flags); if (rc != NRAYS_OK) return rc; }
    HIP_TRY(hipSetDevice(sc->facts.device));
    TraceWorkspace* w = nullptr;
    int rc = trace_workspace(sc, &w);
    if (rc == NRAYS_OK) rc = grow_device(&w->d_dilate_dx, &w->dilate_points, (size_t)a.width * a.height, sizeof(int16_t));
    if (rc == NRAYS_OK) rc = batch_begin(sc, w, stream);
    if (rc != NRAYS_OK) return rc;
    rc = dilate_passes(w, a, stream);
    batch_end(sc, w, stream);
    return rc;
}
// The blocking form, through the workspace's staging buffer as surface_texels_host_impl: the values (16-byte aligned at the block's start), the flags — in and out in
// one array, which the device form allows — and the sources.
static int dilate_texels_host_impl(NraysScene* sc, const DilateArgs& a, uint32_t flags) {
    { const int rc = check_dilate_args(sc, a, flags); if (rc != NRAYS_OK) return rc; }
    HIP_TRY(hipSetDevice(sc->facts.device));
    TraceWorkspace* w = nullptr;
    const size_t n = (size_t)a.width * a.height, value_bytes = a.values ? n * a.channels * sizeof(float) : 0;
    int rc = trace_workspace(sc, &w);
    if (rc == NRAYS_OK) rc = grow_device(&w->d_dilate_dx, &w->dilate_points, n, sizeof(int16_t));
    if (rc == NRAYS_OK) rc = grow_device(&w->d_stage, &w->stage_rays, (value_bytes + n * 8 + kStageUnit - 1) / kStageUnit, kStageUnit);
    if (rc == NRAYS_OK) rc = ensure_own_stream(sc);
    if (rc != NRAYS_OK) return rc;
    DilateArgs s = a;
    s.values = a.values ? (float*)w->d_stage : nullptr;
    uint32_t* s_flags = (uint32_t*)((char*)w->d_stage + value_bytes);
    s.flags_in = s_flags; s.flags_out = a.flags_out ? s_flags : nullptr;
    s.source = a.source ? (int32_t*)(s_flags + n) : nullptr;
    const hipStream_t stream = sc->buf.own_stream;
    rc = batch_begin(sc, w, stream);
    if (rc != NRAYS_OK) return rc;
    hipError_t e = hipMemcpyAsync(s_flags, a.flags_in, n * 4, hipMemcpyHostToDevice, stream);
    if (e == hipSuccess && a.values) e = hipMemcpyAsync(s.values, a.values, value_bytes, hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) rc = set_last_error(NRAYS_ERR_HIP, std::string("dilate texels upload: ") + hipGetErrorString(e));
    if (rc == NRAYS_OK) rc = dilate_passes(w, s, stream);
    if (rc == NRAYS_OK) {
        auto down = [&](void* dst, const void* src, size_t bytes) { return dst ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, stream) : hipSuccess; };
        e = down(a.values, s.values, value_bytes);
        if (e == hipSuccess) e = down(a.source, s.source, n * 4);
        if (e == hipSuccess) e = down(a.flags_out, s_flags, n * 4);
    }
    const hipError_t es = hipStreamSynchronize(stream); // (always: the staging buffer is reused by the next call, and the uploads read the caller's arrays)
    if (e == hipSuccess) e = es;
    if (rc == NRAYS_OK && e != hipSuccess) rc = set_last_error(NRAYS_ERR_HIP, std::string("dilate texels read-back: ") + hipGetErrorString(e));
    batch_end(sc, w, stream);
    return rc;
}

// ---- nrays_filter_texels*: one pass of the 5 x 5 a-trous joint-bilateral filter over a baked map (texel_filter_kernel.h) ---------------------------------------------
static_assert(kFilterMaxStep == NRAYS_FILTER_MAX_STEP, "texel_filter_kernel.h restates the header's constant");
struct FilterArgs { uint32_t width, height; const uint32_t* flags_in; const double* points; const double* normals; uint32_t channels; const float* values_in; float* values_out;
                    uint32_t step; double pos_radius, normal_cos; };
static int check_filter_args(const NraysScene* sc, const FilterArgs& a, uint32_t flags) {
    if (!sc || !a.flags_in || !a.points || !a.normals || !a.values_in || !a.values_out) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (a.values_out == a.values_in) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_filter_texels: values_out must not be values_in (a pass reads its neighbours' inputs)");
    if (a.channels < 1u || a.channels > 4u) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_filter_texels: channels must be in 1 .. 4");
    if (a.step < 1u || a.step > NRAYS_FILTER_MAX_STEP) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_filter_texels: step must be in 1 .. 64");
    if (a.width < 1u || a.width > kTexelMaxSide || a.height < 1u || a.height > kTexelMaxSide || (uint64_t)a.width * a.height > kTexelMaxPoints)
        return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_filter_texels: width and height must be in 1 .. 16384 and width * height <= 2^24");
    if (!(a.pos_radius > 0.0)) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_filter_texels: pos_radius must be > 0 (+inf: no position weight)");
    if (!(a.normal_cos >= -1.0 && a.normal_cos < 1.0)) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_filter_texels: normal_cos must be in [-1, 1)");
    if (flags != 0u) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_filter_texels: flags are reserved and must be 0");
    return NRAYS_OK;
}
// The one launch of a call: per axis ceil(ceil(side / step) / tile) blocks of each of the `step` residue classes.
static int filter_pass(const FilterArgs& a, hipStream_t stream) {
    const uint32_t sub_w = (a.width + a.step - 1u) / a.step, sub_h = (a.height + a.step - 1u) / a.step;
    const FilterLattice L{a.width, a.height, a.step, (sub_w + kFilterTileX - 1u) / kFilterTileX, (sub_h + kFilterTileY - 1u) / kFilterTileY,
                          a.pos_radius * a.pos_radius, a.normal_cos, 1.0 - a.normal_cos};
    const dim3 grid(L.tiles_x * a.step, L.tiles_y * a.step);
    const uint32_t vec4 = (a.channels == 4u && (((uintptr_t)a.values_in | (uintptr_t)a.values_out) & 15u) == 0u) ? 1u : 0u;
    switch (a.channels) {
    case 1u: hipLaunchKernelGGL(k_filter_texels<1>, grid, dim3(kFilterBlock), 0, stream, L, a.flags_in, a.points, a.normals, a.values_in, a.values_out, 0u); break;
    case 2u: hipLaunchKernelGGL(k_filter_texels<2>, grid, dim3(kFilterBlock), 0, stream, L, a.flags_in, a.points, a.normals, a.values_in, a.values_out, 0u); break;
    case 3u: hipLaunchKernelGGL(k_filter_texels<3>, grid, dim3(kFilterBlock), 0, stream, L, a.flags_in, a.points, a.normals, a.values_in, a.values_out, 0u); break;
    default: hipLaunchKernelGGL(k_filter_texels<4>, grid, dim3(kFilterBlock), 0, stream, L, a.flags_in, a.points, a.normals, a.values_in, a.values_out, vec4); break;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return set_last_error(NRAYS_ERR_HIP, std::string("k_filter_texels: ") + hipGetErrorString(e));
    return NRAYS_OK;
}
static int filter_texels_device_impl(NraysScene* sc, const FilterArgs& a, uint32_t flags, hipStream_t stream) {
    { const int rc = check_filter_args(sc, a, flags); if (rc != NRAYS_OK) return rc; }
    HIP_TRY(hipSetDevice(sc->facts.device));
    TraceWorkspace* w = nullptr; // (for the handle's stream ordering alone: the call needs no workspace)
    int rc = trace_workspace(sc, &w);
    if (rc == NRAYS_OK) rc = batch_begin(sc, w, stream);
    if (rc != NRAYS_OK) return rc;
    rc = filter_pass(a, stream);
    batch_end(sc, w, stream);
    return rc;
}
// The blocking form, through the workspace's staging buffer as dilate_texels_host_impl: points, normals, the two value arrays (each at a multiple of 16 bytes), flags.
static int filter_texels_host_impl(NraysScene* sc, const FilterArgs& a, uint32_t flags) {
    { const int rc = check_filter_args(sc, a, flags); if (rc != NRAYS_OK) return rc; }
    HIP_TRY(hipSetDevice(sc->facts.device));
    TraceWorkspace* w = nullptr;
    const size_t n = (size_t)a.width * a.height, geo_bytes = n * 3 * sizeof(double), value_bytes = n * a.channels * sizeof(float), value_slot = (value_bytes + 15) & ~(size_t)15;
    int rc = trace_workspace(sc, &w);
    if (rc == NRAYS_OK) rc = grow_device(&w->d_stage, &w->stage_rays, (2 * geo_bytes + 2 * value_slot + n * 4 + kStageUnit - 1) / kStageUnit, kStageUnit);
    if (rc == NRAYS_OK) rc = ensure_own_stream(sc);
    if (rc != NRAYS_OK) return rc;
    char* base = (char*)w->d_stage;
    FilterArgs s = a;
    s.points = (const double*)base; s.normals = (const double*)(base + geo_bytes);
    s.values_in = (const float*)(base + 2 * geo_bytes); s.values_out = (float*)(base + 2 * geo_bytes + value_slot);
    s.flags_in = (const uint32_t*)(base + 2 * geo_bytes + 2 * value_slot);
    const hipStream_t stream = sc->buf.own_stream;
    rc = batch_begin(sc, w, stream);
    if (rc != NRAYS_OK) return rc;
    auto up = [&](const void* dst, const void* src, size_t bytes) { return hipMemcpyAsync((void*)dst, src, bytes, hipMemcpyHostToDevice, stream); };
    hipError_t e = up(s.points, a.points, geo_bytes);
    if (e == hipSuccess) e = up(s.normals, a.normals, geo_bytes);
    if (e == hipSuccess) e = up(s.values_in, a.values_in, value_bytes);
    if (e == hipSuccess) e = up(s.flags_in, a.flags_in, n * 4);
    if (e != hipSuccess) rc = set_last_error(NRAYS_ERR_HIP, std::string("filter texels upload: ") + hipGetErrorString(e));
    if (rc == NRAYS_OK) rc = filter_pass(s, stream);
    if (rc == NRAYS_OK) e = hipMemcpyAsync(a.values_out, s.values_out, value_bytes, hipMemcpyDeviceToHost, stream);
    const hipError_t es = hipStreamSynchronize(stream); // (always: the staging buffer is reused by the next call, and the uploads read the caller's arrays)
    if (e == hipSuccess) e = es;
    if (rc == NRAYS_OK && e != hipSuccess) rc = set_last_error(NRAYS_ERR_HIP, std::string("filter texels read-back: ") + hipGetErrorString(e));
    batch_end(sc, w, stream);
    return rc;
}

} // namespace nrays

using namespace nrays;

extern "C" {

int nrays_debug_cast_batch(NraysScene* sc, uint32_t mode, uint32_t n, const double* origins, const double* dirs, const double* max_toi, NraysCastResult* out) {
    if (!sc || !origins || !dirs || !out || mode > 1u || (mode == 1u && !max_toi)) return set_last_error(NRAYS_ERR_BAD_ARG, "bad cast-batch arguments");
    if (n == 0) return NRAYS_OK;
    HIP_TRY(hipSetDevice(sc->facts.device));
    if (sc->last.have) HIP_TRY(hipStreamSynchronize(sc->last.stream));
    { const int rs = ensure_spill(sc, &sc->buf.d_spill); if (rs != NRAYS_OK) return rs; }
    double *d_o = nullptr, *d_d = nullptr, *d_t = nullptr; NraysCastResult* d_r = nullptr;
    auto release = [&]() { if (d_o) (void)hipFree(d_o); if (d_d) (void)hipFree(d_d); if (d_t) (void)hipFree(d_t); if (d_r) (void)hipFree(d_r); };
#define CAST_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { release(); return set_last_error(e_ == hipErrorOutOfMemory ? NRAYS_ERR_OOM : NRAYS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } } while (0)
    const size_t vb = (size_t)n * 3 * sizeof(double);
    CAST_TRY(hipMalloc((void**)&d_o, vb)); CAST_TRY(hipMalloc((void**)&d_d, vb)); CAST_TRY(hipMalloc((void**)&d_r, (size_t)n * sizeof(NraysCastResult)));
    CAST_TRY(hipMemcpy(d_o, origins, vb, hipMemcpyHostToDevice)); CAST_TRY(hipMemcpy(d_d, dirs, vb, hipMemcpyHostToDevice));
    if (mode == 1u) { CAST_TRY(hipMalloc((void**)&d_t, (size_t)n * sizeof(double))); CAST_TRY(hipMemcpy(d_t, max_toi, (size_t)n * sizeof(double), hipMemcpyHostToDevice)); }
    const uint32_t grid = std::min<uint32_t>((n + kBlock - 1) / kBlock, (uint32_t)kMaxGrid);
    CAST_TRY(sc->buf.own_stream ? hipSuccess : hipStreamCreate(&sc->buf.own_stream));
    if ((sc->facts.features & ~(int)kFeatMultiSample) == (int)kFeatMesh) hipLaunchKernelGGL((k_cast_batch<kFeatMesh>), dim3(grid), dim3(kBlock), 0, sc->buf.own_stream, sc->facts.d, mode, n, d_o, d_d, d_t, d_r, sc->buf.d_spill);
    else hipLaunchKernelGGL((k_cast_batch<kFeatAll>), dim3(grid), dim3(kBlock), 0, sc->buf.own_stream, sc->facts.d, mode, n, d_o, d_d, d_t, d_r, sc->buf.d_spill);
    CAST_TRY(hipGetLastError());
    CAST_TRY(hipStreamSynchronize(sc->buf.own_stream));
    CAST_TRY(hipMemcpy(out, d_r, (size_t)n * sizeof(NraysCastResult), hipMemcpyDeviceToHost));
#undef CAST_TRY
    release();
    return NRAYS_OK;
}

int nrays_debug_box_cull(uint32_t mode, uint32_t n, const double* origins, const double* dirs, const double* best, const float* boxes, const uint32_t* slots,
                         float* keys, uint32_t* bits, float* inv32) {
    if (!origins || !dirs || !best || !boxes || !slots || !keys || !bits || !inv32 || mode > 1u) return set_last_error(NRAYS_ERR_BAD_ARG, "bad box-cull arguments");
    if (n > (1u << 24)) return set_last_error(NRAYS_ERR_BAD_ARG, "box-cull: more than 2^24 cases"); // (node index << 7 in 32 bits, as the scenes: scene_build.cpp)
    if (n == 0) return NRAYS_OK;
    for (uint32_t i = 0; i < n; ++i) if (slots[i] > 3u) return set_last_error(NRAYS_ERR_BAD_ARG, "box-cull: child slot above 3");
    std::vector<BvhNode> nodes;
    try { nodes.resize(n); } catch (const std::bad_alloc&) { return set_last_error(NRAYS_ERR_OOM, "box-cull nodes"); }
    const float absent_mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, absent_mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (uint32_t i = 0; i < n; ++i) {
        BvhNode& nd = nodes[i];
        for (int k = 0; k < 4; ++k) { nd.slot[5][k] = 0.0f; nd.set_box(k, absent_mn, absent_mx); nd.children()[k] = kEmptyChild; }
        nd.set_box((int)slots[i], boxes + 6 * (size_t)i, boxes + 6 * (size_t)i + 3);
    }
    BvhNode* d_n = nullptr; double *d_o = nullptr, *d_d = nullptr, *d_b = nullptr; float *d_k = nullptr, *d_i = nullptr; uint32_t* d_bits = nullptr;
    auto release = [&]() { for (void* q : {(void*)d_n, (void*)d_o, (void*)d_d, (void*)d_b, (void*)d_k, (void*)d_i, (void*)d_bits}) if (q) (void)hipFree(q); };
#define CULL_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { release(); return set_last_error(e_ == hipErrorOutOfMemory ? NRAYS_ERR_OOM : NRAYS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } } while (0)
    const size_t vb = (size_t)n * 3 * sizeof(double);
    CULL_TRY(hipMalloc((void**)&d_n, (size_t)n * sizeof(BvhNode))); CULL_TRY(hipMalloc((void**)&d_o, vb)); CULL_TRY(hipMalloc((void**)&d_d, vb));
    CULL_TRY(hipMalloc((void**)&d_b, (size_t)n * sizeof(double))); CULL_TRY(hipMalloc((void**)&d_k, (size_t)n * 4 * sizeof(float)));
    CULL_TRY(hipMalloc((void**)&d_i, (size_t)n * 3 * sizeof(float))); CULL_TRY(hipMalloc((void**)&d_bits, (size_t)n * sizeof(uint32_t)));
    CULL_TRY(hipMemcpy(d_n, nodes.data(), (size_t)n * sizeof(BvhNode), hipMemcpyHostToDevice));
    CULL_TRY(hipMemcpy(d_o, origins, vb, hipMemcpyHostToDevice)); CULL_TRY(hipMemcpy(d_d, dirs, vb, hipMemcpyHostToDevice));
    CULL_TRY(hipMemcpy(d_b, best, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    const uint64_t threads = mode == 1u ? (uint64_t)n * 64u : (uint64_t)n;
    const uint32_t grid = (uint32_t)std::min<uint64_t>((threads + kBlock - 1) / kBlock, (uint64_t)kMaxGrid);
    hipLaunchKernelGGL(k_box_cull, dim3(grid), dim3(kBlock), 0, (hipStream_t)0, (const BvhNode*)d_n, mode, n, (const double*)d_o, (const double*)d_d, (const double*)d_b, d_k, d_bits, d_i);
    CULL_TRY(hipGetLastError());
    CULL_TRY(hipDeviceSynchronize());
    CULL_TRY(hipMemcpy(keys, d_k, (size_t)n * 4 * sizeof(float), hipMemcpyDeviceToHost)); CULL_TRY(hipMemcpy(bits, d_bits, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    CULL_TRY(hipMemcpy(inv32, d_i, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost));
#undef CULL_TRY
    release();
    return NRAYS_OK;
}

int nrays_trace_rays_device(NraysScene* sc, uint32_t n, const double* origins, const double* dirs, const double* refr, const float* energy, const uint64_t* keys,
                            uint32_t max_depth, float* out_rgb, void* hip_stream) {
    return trace_rays_device_impl(sc, n, origins, dirs, refr, energy, keys, max_depth, out_rgb, 0u, (hipStream_t)hip_stream);
}
int nrays_trace_rays_device_ex(NraysScene* sc, uint32_t n, const double* origins, const double* dirs, const double* refr, const float* energy, const uint64_t* keys,
                               uint32_t max_depth, float* out_rgb, uint32_t flags, void* hip_stream) {
    return trace_rays_device_impl(sc, n, origins, dirs, refr, energy, keys, max_depth, out_rgb, flags, (hipStream_t)hip_stream);
}

static int trace_rays_host_impl(NraysScene* sc, uint32_t n, const double* origins, const double* dirs, const double* refr, const float* energy, const uint64_t* keys,
                                uint32_t max_depth, float* out_rgb, uint32_t flags) {
    if (!sc || !origins || !dirs || !out_rgb) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (check_ray_flags(flags) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    if (n == 0) return NRAYS_OK;
    HIP_TRY(hipSetDevice(sc->facts.device));
    TraceWorkspace* w = nullptr;
    int rc = trace_workspace(sc, &w);
    if (rc != NRAYS_OK) return rc;
    // device copies of one chunk's arrays: origins, directions (3 f64), refr (f64), keys (u64), energy (f32), colours (3 f32) — 80 bytes a ray
    rc = grow_device(&w->d_stage, &w->stage_rays, std::min<uint32_t>(n, kTraceChunk), kStageUnit);
    if (rc != NRAYS_OK) return rc;
    const size_t cap = w->stage_rays;
    double* s_o = (double*)w->d_stage; double* s_d = s_o + 3 * cap; double* s_r = s_d + 3 * cap;
    unsigned long long* s_k = (unsigned long long*)(s_r + cap); float* s_e = (float*)(s_k + cap); float* s_out = s_e + cap;
    rc = ensure_own_stream(sc);
    if (rc != NRAYS_OK) return rc;
    const hipStream_t stream = sc->buf.own_stream;
    rc = batch_begin(sc, w, stream);
    if (rc != NRAYS_OK) return rc;
    const bool reorder = (flags & NRAYS_RAYS_UNORDERED) && reorder_pays(sc, n);
    for (uint32_t c0 = 0; c0 < n && rc == NRAYS_OK; c0 += std::min<uint32_t>(n - c0, kTraceChunk)) {
        const uint32_t nc = std::min<uint32_t>(n - c0, kTraceChunk);
        auto up = [&](void* dst, const void* src, size_t bytes) { return hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream); };
        hipError_t e = up(s_o, origins + 3 * (size_t)c0, (size_t)nc * 24);
        if (e == hipSuccess) e = up(s_d, dirs + 3 * (size_t)c0, (size_t)nc * 24);
        if (e == hipSuccess && refr) e = up(s_r, refr + c0, (size_t)nc * 8);
        if (e == hipSuccess && keys) e = up(s_k, keys + c0, (size_t)nc * 8);
        if (e == hipSuccess && energy) e = up(s_e, energy + c0, (size_t)nc * 4);
        if (e != hipSuccess) { rc = set_last_error(NRAYS_ERR_HIP, std::string("trace batch upload: ") + hipGetErrorString(e)); break; }
        const uint32_t* order = nullptr;
        rc = chunk_order(sc, w, reorder, nc, s_o, s_d, stream, &order);
        if (rc != NRAYS_OK) break;
        rc = trace_chunk(sc, w, nc, s_o, s_d, refr ? s_r : nullptr, energy ? s_e : nullptr, keys ? s_k : nullptr, (unsigned long long)c0, max_depth, s_out, stream, order);
        if (rc == NRAYS_OK) {
            e = hipMemcpyAsync(out_rgb + 3 * (size_t)c0, s_out, (size_t)nc * 12, hipMemcpyDeviceToHost, stream);
            if (e == hipSuccess) e = hipStreamSynchronize(stream);
            if (e != hipSuccess) rc = set_last_error(NRAYS_ERR_HIP, std::string("trace batch read-back: ") + hipGetErrorString(e));
        }
    }
    batch_end(sc, w, stream);
    return rc;
}
int nrays_trace_rays(NraysScene* sc, uint32_t n, const double* origins, const double* dirs, const double* refr, const float* energy, const uint64_t* keys,
                     uint32_t max_depth, float* out_rgb) {
    return trace_rays_host_impl(sc, n, origins, dirs, refr, energy, keys, max_depth, out_rgb, 0u);
}
int nrays_trace_rays_ex(NraysScene* sc, uint32_t n, const double* origins, const double* dirs, const double* refr, const float* energy, const uint64_t* keys,
                        uint32_t max_depth, float* out_rgb, uint32_t flags) {
    return trace_rays_host_impl(sc, n, origins, dirs, refr, energy, keys, max_depth, out_rgb, flags);
}

static int intersects_rays_device_impl(NraysScene* sc, uint32_t n, const double* origins, const double* dirs, const double* max_toi, float* out_filter,
                                       uint32_t* out_lit, uint32_t flags, void* hip_stream) {
    if (!sc || !origins || !dirs || !max_toi || !out_filter || !out_lit) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (check_ray_flags(flags) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    if (n == 0) return NRAYS_OK;
    HIP_TRY(hipSetDevice(sc->facts.device));
    const hipStream_t stream = (hipStream_t)hip_stream;
    TraceWorkspace* w = nullptr;
    int rc = trace_workspace(sc, &w);
    if (rc == NRAYS_OK) rc = batch_begin(sc, w, stream);
    if (rc != NRAYS_OK) return rc;
    const bool mesh = (sc->facts.features & ~(int)kFeatMultiSample) == (int)kFeatMesh; // (traversal only: as nrays_debug_cast_batch)
    const bool reorder = (flags & NRAYS_RAYS_UNORDERED) && reorder_pays(sc, n);
    for (uint32_t c0 = 0; c0 < n; c0 += std::min<uint32_t>(n - c0, kTraceChunk)) { // (chunks keep the kernel's 32-bit ray indices far from overflow)
        const uint32_t nc = std::min<uint32_t>(n - c0, kTraceChunk);
        const uint32_t grid = std::min<uint32_t>((nc + kBlock - 1) / kBlock, (uint32_t)kMaxGrid);
        const double *o = origins + 3 * (size_t)c0, *d = dirs + 3 * (size_t)c0, *t = max_toi + c0;
        const uint32_t* order = nullptr;
        rc = chunk_order(sc, w, reorder, nc, o, d, stream, &order);
        if (rc != NRAYS_OK) break;
        if (order && mesh) hipLaunchKernelGGL((k_intersects_rays_ordered<kFeatMesh>), dim3(grid), dim3(kBlock), 0, stream, sc->facts.d, nc, order, o, d, t, out_filter + 3 * (size_t)c0, out_lit + c0, w->d_spill);
        else if (order) hipLaunchKernelGGL((k_intersects_rays_ordered<kFeatAll>), dim3(grid), dim3(kBlock), 0, stream, sc->facts.d, nc, order, o, d, t, out_filter + 3 * (size_t)c0, out_lit + c0, w->d_spill);
        else if (mesh) hipLaunchKernelGGL((k_intersects_rays<kFeatMesh>), dim3(grid), dim3(kBlock), 0, stream, sc->facts.d, nc, o, d, t, out_filter + 3 * (size_t)c0, out_lit + c0, w->d_spill);
        else hipLaunchKernelGGL((k_intersects_rays<kFeatAll>), dim3(grid), dim3(kBlock), 0, stream, sc->facts.d, nc, o, d, t, out_filter + 3 * (size_t)c0, out_lit + c0, w->d_spill);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) { rc = set_last_error(NRAYS_ERR_HIP, std::string("k_intersects_rays: ") + hipGetErrorString(e)); break; }
    }
    batch_end(sc, w, stream);
    return rc;
}
int nrays_intersects_rays_device(NraysScene* sc, uint32_t n, const double* origins, const double* dirs, const double* max_toi, float* out_filter,
                                 uint32_t* out_lit, void* hip_stream) {
    return intersects_rays_device_impl(sc, n, origins, dirs, max_toi, out_filter, out_lit, 0u, hip_stream);
}
int nrays_intersects_rays_device_ex(NraysScene* sc, uint32_t n, const double* origins, const double* dirs, const double* max_toi, float* out_filter,
                                    uint32_t* out_lit, uint32_t flags, void* hip_stream) {
    return intersects_rays_device_impl(sc, n, origins, dirs, max_toi, out_filter, out_lit, flags, hip_stream);
}

int nrays_cast_rays_device(NraysScene* sc, uint32_t n, const double* origins, const double* dirs, const double* max_toi, double* out_toi, int32_t* out_node,
                           double* out_normal, double* out_uv, int32_t* out_prim, uint32_t* out_flags, uint32_t flags, void* hip_stream) {
    return cast_rays_device_impl(sc, n, origins, dirs, max_toi, CastOut{out_toi, out_node, out_normal, out_uv, out_prim, out_flags}, flags, (hipStream_t)hip_stream);
}
int nrays_cast_rays(NraysScene* sc, uint32_t n, const double* origins, const double* dirs, const double* max_toi, double* out_toi, int32_t* out_node,
                    double* out_normal, double* out_uv, int32_t* out_prim, uint32_t* out_flags, uint32_t flags) {
    return cast_rays_host_impl(sc, n, origins, dirs, max_toi, CastOut{out_toi, out_node, out_normal, out_uv, out_prim, out_flags}, flags);
}

int nrays_shade_points_device(NraysScene* sc, uint32_t n, const double* points, const double* normals, const double* view_dirs, const double* uvs, const int32_t* nodes,
                              const uint32_t* hit_flags, const uint64_t* keys, float* out_rgba, uint32_t flags, void* hip_stream) {
    return shade_points_device_impl(sc, n, ShadeIn{points, normals, view_dirs, uvs, nodes, hit_flags, keys}, out_rgba, flags, (hipStream_t)hip_stream);
}
int nrays_shade_points(NraysScene* sc, uint32_t n, const double* points, const double* normals, const double* view_dirs, const double* uvs, const int32_t* nodes,
                       const uint32_t* hit_flags, const uint64_t* keys, float* out_rgba, uint32_t flags) {
    return shade_points_host_impl(sc, n, ShadeIn{points, normals, view_dirs, uvs, nodes, hit_flags, keys}, out_rgba, flags);
}

int nrays_occlusion_points_device(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const uint64_t* keys,
                                  const NraysOcclusionParams* params, float* out_filter, uint32_t* out_open, uint32_t flags, void* hip_stream) {
    return occlusion_points_device_impl(sc, n, OcclusionIn{points, normals, hit_flags, keys}, params, out_filter, out_open, flags, (hipStream_t)hip_stream);
}
int nrays_occlusion_points(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const uint64_t* keys,
                           const NraysOcclusionParams* params, float* out_filter, uint32_t* out_open, uint32_t flags) {
    return occlusion_points_host_impl(sc, n, OcclusionIn{points, normals, hit_flags, keys}, params, out_filter, out_open, flags);
}
int nrays_debug_occlusion_rays(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint64_t* keys, const NraysOcclusionParams* params,
                               double* out_origins, double* out_dirs) {
    return occlusion_rays_probe(sc, n, points, normals, keys, params, out_origins, out_dirs);
}

int nrays_gather_points_device(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const uint64_t* keys,
                               const NraysGatherParams* params, float* out_rgb, uint32_t flags, void* hip_stream) {
    return gather_points_device_impl(sc, n, OcclusionIn{points, normals, hit_flags, keys}, params, out_rgb, flags, false, 0u, (hipStream_t)hip_stream);
}
int nrays_gather_points_device_ex(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const uint64_t* keys,
                                  const NraysGatherParams* params, float* out_rgb, uint32_t flags, void* hip_stream) {
    return gather_points_device_impl(sc, n, OcclusionIn{points, normals, hit_flags, keys}, params, out_rgb, flags, true, 0u, (hipStream_t)hip_stream);
}
int nrays_gather_points(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const uint64_t* keys,
                        const NraysGatherParams* params, float* out_rgb, uint32_t flags) {
    return gather_points_host_impl(sc, n, OcclusionIn{points, normals, hit_flags, keys}, params, out_rgb, flags, false, 0u);
}
int nrays_gather_points_ex(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const uint64_t* keys,
                           const NraysGatherParams* params, float* out_rgb, uint32_t flags) {
    return gather_points_host_impl(sc, n, OcclusionIn{points, normals, hit_flags, keys}, params, out_rgb, flags, true, 0u);
}

int nrays_gather_maps_points_device(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const uint64_t* keys,
                                    const NraysGatherMapsParams* params, float* out_rgb, uint32_t* out_counts, uint32_t flags, void* hip_stream) {
    return gather_maps_device_impl(sc, n, OcclusionIn{points, normals, hit_flags, keys}, params, out_rgb, out_counts, flags, (hipStream_t)hip_stream);
}
int nrays_gather_maps_points(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const uint64_t* keys,
                             const NraysGatherMapsParams* params, float* out_rgb, uint32_t* out_counts, uint32_t flags) {
    return gather_maps_host_impl(sc, n, OcclusionIn{points, normals, hit_flags, keys}, params, out_rgb, out_counts, flags);
}

int nrays_surface_texels_device(NraysScene* sc, uint32_t node, uint32_t width, uint32_t height, double* out_points, double* out_normals, double* out_uv, int32_t* out_node,
                                int32_t* out_prim, uint32_t* out_flags, uint32_t flags, void* hip_stream) {
    return surface_texels_device_impl(sc, node, width, height, TexelOutputs{out_points, out_normals, out_uv, out_node, out_prim, out_flags}, flags, (hipStream_t)hip_stream);
}
int nrays_surface_texels(NraysScene* sc, uint32_t node, uint32_t width, uint32_t height, double* out_points, double* out_normals, double* out_uv, int32_t* out_node,
                         int32_t* out_prim, uint32_t* out_flags, uint32_t flags) {
    return surface_texels_host_impl(sc, node, width, height, TexelOutputs{out_points, out_normals, out_uv, out_node, out_prim, out_flags}, flags);
}
int nrays_debug_surface_texels_passes(NraysScene* sc, uint32_t node, uint32_t width, uint32_t height, uint32_t flags, uint32_t repeats, float* out_ms) {
    return surface_texels_passes_probe(sc, node, width, height, flags, repeats, out_ms);
}

int nrays_dilate_texels_device(NraysScene* sc, uint32_t width, uint32_t height, const uint32_t* flags_in, uint32_t radius, uint32_t channels, float* values, int32_t* out_source,
                               uint32_t* out_flags, uint32_t flags, void* hip_stream) {
    return dilate_texels_device_impl(sc, DilateArgs{width, height, flags_in, radius, channels, values, out_source, out_flags}, flags, (hipStream_t)hip_stream);
}
int nrays_dilate_texels(NraysScene* sc, uint32_t width, uint32_t height, const uint32_t* flags_in, uint32_t radius, uint32_t channels, float* values, int32_t* out_source,
                        uint32_t* out_flags, uint32_t flags) {
    return dilate_texels_host_impl(sc, DilateArgs{width, height, flags_in, radius, channels, values, out_source, out_flags}, flags);
}

int nrays_filter_texels_device(NraysScene* sc, uint32_t width, uint32_t height, const uint32_t* flags_in, const double* points, const double* normals, uint32_t channels,
                               const float* values_in, float* values_out, uint32_t step, double pos_radius, double normal_cos, uint32_t flags, void* hip_stream) {
    return filter_texels_device_impl(sc, FilterArgs{width, height, flags_in, points, normals, channels, values_in, values_out, step, pos_radius, normal_cos}, flags, (hipStream_t)hip_stream);
}
int nrays_filter_texels(NraysScene* sc, uint32_t width, uint32_t height, const uint32_t* flags_in, const double* points, const double* normals, uint32_t channels,
                        const float* values_in, float* values_out, uint32_t step, double pos_radius, double normal_cos, uint32_t flags) {
    return filter_texels_host_impl(sc, FilterArgs{width, height, flags_in, points, normals, channels, values_in, values_out, step, pos_radius, normal_cos}, flags);
}

int nrays_debug_ray_order(NraysScene* sc, uint32_t n, const double* origins, const double* dirs, uint64_t* out_keys, uint32_t* out_order, double* out_frame,
                          uint32_t out_info[4]) {
    if (!sc || !origins || !dirs || !out_keys || !out_order || !out_frame || !out_info) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (n > kTraceChunk) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_debug_ray_order: at most one chunk (2^22 rays)");
    out_info[0] = (uint32_t)kRayKeyBits; out_info[1] = (uint32_t)kRayBinBits; out_info[2] = reorder_pays(sc, n) ? 1u : 0u; out_info[3] = 0u;
    if (n == 0) return NRAYS_OK;
    HIP_TRY(hipSetDevice(sc->facts.device));
    TraceWorkspace* w = nullptr;
    int rc = trace_workspace(sc, &w);
    if (rc == NRAYS_OK) rc = ray_order_ensure(w, n);
    if (rc == NRAYS_OK) rc = ensure_own_stream(sc);
    if (rc != NRAYS_OK) return rc;
    const hipStream_t stream = sc->buf.own_stream;
    double* d_od = nullptr; // origins, then directions
    HIP_TRY(hipMalloc((void**)&d_od, (size_t)n * 48));
    rc = batch_begin(sc, w, stream);
    hipError_t e = hipSuccess;
    if (rc == NRAYS_OK) {
        e = hipMemcpyAsync(d_od, origins, (size_t)n * 24, hipMemcpyHostToDevice, stream);
        if (e == hipSuccess) e = hipMemcpyAsync(d_od + 3 * (size_t)n, dirs, (size_t)n * 24, hipMemcpyHostToDevice, stream);
        if (e == hipSuccess) rc = ray_order_chunk(sc, w, n, d_od, d_od + 3 * (size_t)n, stream);
        if (e == hipSuccess && rc == NRAYS_OK) e = hipMemcpyAsync(out_keys, w->d_ray_keys, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess && rc == NRAYS_OK) e = hipMemcpyAsync(out_order, w->d_ray_order, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess && rc == NRAYS_OK) e = hipMemcpyAsync(out_frame, w->d_ray_frame, NRAYS_RAY_FRAME_DOUBLES * sizeof(double), hipMemcpyDeviceToHost, stream);
        const hipError_t es = hipStreamSynchronize(stream);
        if (e == hipSuccess) e = es;
        batch_end(sc, w, stream);
    }
    (void)hipFree(d_od);
    if (rc == NRAYS_OK && e != hipSuccess) rc = set_last_error(NRAYS_ERR_HIP, std::string("nrays_debug_ray_order: ") + hipGetErrorString(e));
    return rc;
}

int nrays_gather_sh_points_device(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const uint64_t* keys,
                                  const NraysGatherParams* params, uint32_t bands, float* out_sh, uint32_t flags, void* hip_stream) {
    if (check_sh_bands(bands) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    return gather_points_device_impl(sc, n, OcclusionIn{points, normals, hit_flags, keys}, params, out_sh, flags, true, bands, (hipStream_t)hip_stream);
}
int nrays_gather_sh_points(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const uint64_t* keys,
                           const NraysGatherParams* params, uint32_t bands, float* out_sh, uint32_t flags) {
    if (check_sh_bands(bands) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    return gather_points_host_impl(sc, n, OcclusionIn{points, normals, hit_flags, keys}, params, out_sh, flags, true, bands);
}

int nrays_debug_gather_sh_fold(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const uint64_t* keys,
                               const NraysGatherParams* params, uint32_t bands, const float* ray_colours, float* out_sh, float* out_kernel_ms) {
    if (!ray_colours) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (check_sh_bands(bands) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    if (check_gather_args(sc, OcclusionIn{points, normals, hit_flags, keys}, params, out_sh, 0u, true) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    const uint64_t pairs64 = (uint64_t)n * params->num_dirs;
    if (pairs64 > kTraceChunk) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_debug_gather_sh_fold: at most one chunk (n * num_dirs <= 2^22)");
    if (out_kernel_ms) *out_kernel_ms = 0.0f;
    if (n == 0) return NRAYS_OK;
    HIP_TRY(hipSetDevice(sc->facts.device));
    int rc = ensure_own_stream(sc);
    if (rc != NRAYS_OK) return rc;
    const hipStream_t stream = sc->buf.own_stream;
    // the tables, then per point: point, normal (3 f64), key (u64), hit flags (32 bits), the output; then the colours — the 8-byte fields first
    const size_t table = 3 * (size_t)params->num_dirs + 2 * (size_t)params->num_rotations, out_floats = (size_t)n * gather_out_floats(bands), ray_floats = 3 * (size_t)pairs64;
    double* d_all = nullptr;
    HIP_TRY(hipMalloc((void**)&d_all, table * sizeof(double) + (size_t)n * 60 + (out_floats + ray_floats) * sizeof(float)));
    double* d_dirs = d_all; double* d_rot = d_dirs + 3 * (size_t)params->num_dirs; double* d_p = d_all + table; double* d_n = d_p + 3 * (size_t)n;
    uint64_t* d_k = (uint64_t*)(d_n + 3 * (size_t)n); uint32_t* d_hf = (uint32_t*)(d_k + n); float* d_out = (float*)(d_hf + n); float* d_rays = d_out + out_floats;
    hipEvent_t ev[2] = {nullptr, nullptr};
    auto up = [&](void* dst, const void* src, size_t bytes) { return src && bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream) : hipSuccess; };
    hipError_t e = up(d_dirs, params->dirs, 24 * (size_t)params->num_dirs);
    if (e == hipSuccess) e = up(d_rot, params->rotations, 16 * (size_t)params->num_rotations);
    if (e == hipSuccess) e = up(d_p, points, 24 * (size_t)n);
    if (e == hipSuccess) e = up(d_n, normals, 24 * (size_t)n);
    if (e == hipSuccess) e = up(d_k, keys, 8 * (size_t)n);
    if (e == hipSuccess) e = up(d_hf, hit_flags, 4 * (size_t)n);
    if (e == hipSuccess) e = up(d_rays, ray_colours, ray_floats * sizeof(float));
    if (e == hipSuccess && out_kernel_ms) { e = hipEventCreate(&ev[0]); if (e == hipSuccess) e = hipEventCreate(&ev[1]); }
    if (e == hipSuccess && out_kernel_ms) e = hipEventRecord(ev[0], stream);
    if (e == hipSuccess) {
        const GatherPoints pts{d_p, d_n, hit_flags ? d_hf : nullptr, keys ? (const unsigned long long*)d_k : nullptr, 0ull};
        const uint32_t grid = std::min<uint32_t>((n + kShGroups - 1u) / kShGroups, kShMaxGrid);
        hipLaunchKernelGGL(k_gather_fold_sh, dim3(grid), dim3(kShBlock), 0, stream, (const float*)d_rays, n, pts, OcclusionSpec{params->num_dirs, params->num_rotations, params->bias, 0.0},
                           (const double*)d_dirs, params->num_rotations ? (const double*)d_rot : nullptr, bands * bands, d_out);
        e = hipGetLastError();
    }
    if (e == hipSuccess && out_kernel_ms) e = hipEventRecord(ev[1], stream);
    if (e == hipSuccess) e = hipMemcpyAsync(out_sh, d_out, out_floats * sizeof(float), hipMemcpyDeviceToHost, stream);
    const hipError_t es = hipStreamSynchronize(stream); // (always: the uploads read the caller's memory)
    if (e == hipSuccess) e = es;
    if (e == hipSuccess && out_kernel_ms) e = hipEventElapsedTime(out_kernel_ms, ev[0], ev[1]);
    for (hipEvent_t v : ev) if (v) (void)hipEventDestroy(v);
    (void)hipFree(d_all);
    if (e != hipSuccess) rc = set_last_error(NRAYS_ERR_HIP, std::string("nrays_debug_gather_sh_fold: ") + hipGetErrorString(e));
    return rc;
}

int nrays_debug_gather_order(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const uint64_t* keys,
                             const NraysGatherParams* params, uint64_t* out_keys, uint32_t* out_order, double* out_frame, uint32_t out_info[4]) {
    if (!out_keys || !out_order || !out_frame || !out_info) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (check_gather_args(sc, OcclusionIn{points, normals, hit_flags, keys}, params, (const float*)out_frame /* (none is written: any non-NULL address) */, 0u, true) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    const uint64_t pairs64 = (uint64_t)n * params->num_dirs;
    if (pairs64 > kTraceChunk) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_debug_gather_order: at most one chunk (n * num_dirs <= 2^22)");
    const uint32_t pairs = (uint32_t)pairs64;
    out_info[0] = (uint32_t)kRayKeyBits; out_info[1] = (uint32_t)kRayBinBits; out_info[2] = reorder_pays(sc, pairs) ? 1u : 0u; out_info[3] = 0u;
    if (n == 0) return NRAYS_OK;
    HIP_TRY(hipSetDevice(sc->facts.device));
    TraceWorkspace* w = nullptr;
    int rc = trace_workspace(sc, &w);
    if (rc == NRAYS_OK) rc = ray_order_ensure(w, pairs);
    if (rc == NRAYS_OK) rc = ensure_own_stream(sc);
    if (rc != NRAYS_OK) return rc;
    const hipStream_t stream = sc->buf.own_stream;
    // the tables, then per point: point, normal (3 f64), key (u64), hit flags (32 bits) — the 8-byte fields first
    const size_t table = 3 * (size_t)params->num_dirs + 2 * (size_t)params->num_rotations;
    double* d_all = nullptr;
    HIP_TRY(hipMalloc((void**)&d_all, table * sizeof(double) + (size_t)n * 60));
    double* d_dirs = d_all; double* d_rot = d_dirs + 3 * (size_t)params->num_dirs; double* d_p = d_all + table; double* d_n = d_p + 3 * (size_t)n;
    uint64_t* d_k = (uint64_t*)(d_n + 3 * (size_t)n); uint32_t* d_hf = (uint32_t*)(d_k + n);
    rc = batch_begin(sc, w, stream);
    hipError_t e = hipSuccess;
    if (rc == NRAYS_OK) {
        auto up = [&](void* dst, const void* src, size_t bytes) { return src && bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, stream) : hipSuccess; };
        e = up(d_dirs, params->dirs, 24 * (size_t)params->num_dirs);
        if (e == hipSuccess) e = up(d_rot, params->rotations, 16 * (size_t)params->num_rotations);
        if (e == hipSuccess) e = up(d_p, points, 24 * (size_t)n);
        if (e == hipSuccess) e = up(d_n, normals, 24 * (size_t)n);
        if (e == hipSuccess) e = up(d_k, keys, 8 * (size_t)n);
        if (e == hipSuccess) e = up(d_hf, hit_flags, 4 * (size_t)n);
        if (e == hipSuccess) e = up(w->d_ray_keys, out_keys, (size_t)pairs * sizeof(uint64_t)); // (a skipped point's entries come back as the caller filled them)
        if (e == hipSuccess) {
            const GatherPoints pts{d_p, d_n, hit_flags ? d_hf : nullptr, keys ? (const unsigned long long*)d_k : nullptr, 0ull};
            rc = gather_order_chunk(sc, w, pairs, pts, OcclusionSpec{params->num_dirs, params->num_rotations, params->bias, 0.0}, d_dirs, params->num_rotations ? d_rot : nullptr, stream);
        }
        if (e == hipSuccess && rc == NRAYS_OK) e = hipMemcpyAsync(&out_info[3], w->d_ray_bins + kNumBins, sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess && rc == NRAYS_OK) e = hipStreamSynchronize(stream);
        if (e == hipSuccess && rc == NRAYS_OK && out_info[3] > pairs) rc = set_last_error(NRAYS_ERR_HIP, "nrays_debug_gather_order: more pairs placed than the chunk holds");
        if (e == hipSuccess && rc == NRAYS_OK) e = hipMemcpyAsync(out_keys, w->d_ray_keys, (size_t)pairs * sizeof(uint64_t), hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess && rc == NRAYS_OK && out_info[3]) e = hipMemcpyAsync(out_order, w->d_ray_order, (size_t)out_info[3] * sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess && rc == NRAYS_OK) e = hipMemcpyAsync(out_frame, w->d_ray_frame, NRAYS_RAY_FRAME_DOUBLES * sizeof(double), hipMemcpyDeviceToHost, stream);
        const hipError_t es = hipStreamSynchronize(stream);
        if (e == hipSuccess) e = es;
        batch_end(sc, w, stream);
    }
    (void)hipFree(d_all);
    if (rc == NRAYS_OK && e != hipSuccess) rc = set_last_error(NRAYS_ERR_HIP, std::string("nrays_debug_gather_order: ") + hipGetErrorString(e));
    return rc;
}

} // extern "C"
