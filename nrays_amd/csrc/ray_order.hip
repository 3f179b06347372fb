// ray_order.hip — the reorder of a chunk of rays that come in no useful order (NRAYS_RAYS_UNORDERED): the rays are binned by a spatial key
// on the device and traced in bin order, every result written to the slot of the ray it belongs to.  The traversal lives on coherence
// inside a wave (a wave-uniform node visit is one scalar fetch for 64 lanes, and only when the lanes agree on the direction signs); a wave
// of 64 unrelated rays gets none of it.  Holds the key / bin / scan / place kernels, their form for the (point, direction) pairs of a gather chunk,
// what ray_order.h declares (ray_order_ensure / ray_order_chunk / gather_order_chunk / ray_order_release) and the two probes nrays_debug_ray_order and
// nrays_debug_gather_order.  The batches that call it: ray_batches.hip, point_batches.hip, through batch_call.cpp's chunk_order.
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

#include <string>

#include "../../include/nrays_abi.h"
#include "batch_call.h"
#include "ray_batch_kernel.h"
#include "ray_key.h"
#include "ray_order.h"
#include "scene_handle.h"

static_assert(NRAYS_RAY_FRAME_DOUBLES == nrays::kRayFrameDoubles, "include/nrays_abi.h and ray_key.h disagree on the frame");

namespace nrays {

constexpr uint32_t kOrderBlock = 256u;     // threads per workgroup of the kernels below
constexpr uint32_t kBoundsMaxGrid = 1024u; // workgroups of k_ray_bounds (each writes 10 doubles)
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

// ---- the same three steps on the (point, direction) pairs of a gather chunk (nrays_gather_points*_ex; hemisphere_device.h: gather_pair_ray) -----------------------
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
void ray_order_release(TraceWorkspace* w) {
    free_per_ray(w);
    if (w->d_ray_frame) (void)hipFree(w->d_ray_frame);
    if (w->d_ray_partial) (void)hipFree(w->d_ray_partial);
    if (w->d_ray_bins) (void)hipFree(w->d_ray_bins);
    if (w->d_ray_scan) (void)hipFree(w->d_ray_scan);
    w->d_ray_frame = nullptr; w->d_ray_partial = nullptr; w->d_ray_bins = nullptr; w->d_ray_scan = nullptr;
}
int ray_order_ensure(TraceWorkspace* w, uint32_t n) {
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

int ray_order_chunk(const NraysScene* sc, TraceWorkspace* w, uint32_t n, const double* origins, const double* dirs, hipStream_t stream) {
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
int gather_order_chunk(const NraysScene* sc, TraceWorkspace* w, uint32_t pairs, const GatherPoints& in, const OcclusionSpec& G, const double* dirs, const double* rotations,
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

} // namespace nrays

using namespace nrays;

// The probes stage their inputs through the batch driver's arena (batch_call.h) and read the workspace's sort state back themselves.
static int ensure_order_buffers(TraceWorkspace* w, const void* rays) { return ray_order_ensure(w, *(const uint32_t*)rays); }
static int order_status(hipError_t e, const char* what) { return e == hipSuccess ? (int)NRAYS_OK : set_last_error(NRAYS_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }

extern "C" {

int nrays_debug_ray_order(NraysScene* sc, uint32_t n, const double* origins, const double* dirs, uint64_t* out_keys, uint32_t* out_order, double* out_frame,
                          uint32_t out_info[4]) {
    if (!sc || !origins || !dirs || !out_keys || !out_order || !out_frame || !out_info) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (n > kTraceChunk) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_debug_ray_order: at most one chunk (2^22 rays)");
    out_info[0] = (uint32_t)kRayKeyBits; out_info[1] = (uint32_t)kRayBinBits; out_info[2] = reorder_pays(sc, n) ? 1u : 0u; out_info[3] = 0u;
    if (n == 0) return NRAYS_OK;
    const char* what = "nrays_debug_ray_order";
    StageColumn cols[kRayColumns];
    ray_columns(cols, origins, dirs);
    BatchCall b;
    int rc = batch_open(&b, sc, true, nullptr, cols, kRayColumns, n, ensure_order_buffers, &n);
    if (rc != NRAYS_OK) return rc;
    TraceWorkspace* w = b.w;
    void* c[kRayColumns];
    batch_columns(b, 0, c);
    rc = batch_upload(b, 0, n, what);
    if (rc == NRAYS_OK) rc = ray_order_chunk(sc, w, n, (const double*)c[kRayO], (const double*)c[kRayD], b.stream);
    if (rc == NRAYS_OK) rc = order_status(hipMemcpyAsync(out_keys, w->d_ray_keys, (size_t)n * sizeof(uint64_t), hipMemcpyDeviceToHost, b.stream), what);
    if (rc == NRAYS_OK) rc = order_status(hipMemcpyAsync(out_order, w->d_ray_order, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, b.stream), what);
    if (rc == NRAYS_OK) rc = order_status(hipMemcpyAsync(out_frame, w->d_ray_frame, NRAYS_RAY_FRAME_DOUBLES * sizeof(double), hipMemcpyDeviceToHost, b.stream), what);
    rc = batch_drain(b, rc, what);
    batch_close(b);
    return rc;
}

int nrays_debug_gather_order(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const uint64_t* keys,
                             const NraysGatherParams* params, uint64_t* out_keys, uint32_t* out_order, double* out_frame, uint32_t out_info[4]) {
    if (!out_keys || !out_order || !out_frame || !out_info) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (check_gather_args(sc, points, normals, params, (const float*)out_frame /* (none is written: any non-NULL address) */, 0u, true) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    const uint64_t pairs64 = (uint64_t)n * params->num_dirs;
    if (pairs64 > kTraceChunk) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_debug_gather_order: at most one chunk (n * num_dirs <= 2^22)");
    const uint32_t pairs = (uint32_t)pairs64;
    out_info[0] = (uint32_t)kRayKeyBits; out_info[1] = (uint32_t)kRayBinBits; out_info[2] = reorder_pays(sc, pairs) ? 1u : 0u; out_info[3] = 0u;
    if (n == 0) return NRAYS_OK;
    const char* what = "nrays_debug_gather_order";
    StageColumn cols[kPointColumns];
    point_columns(cols, params->dirs, params->num_dirs, params->rotations, params->num_rotations, points, normals, hit_flags, keys);
    BatchCall b;
    int rc = batch_open(&b, sc, true, nullptr, cols, kPointColumns, n, ensure_order_buffers, &pairs);
    if (rc != NRAYS_OK) return rc;
    TraceWorkspace* w = b.w;
    void* c[kPointColumns];
    batch_columns(b, 0, c);
    rc = batch_upload_tables(b, what);
    if (rc == NRAYS_OK) rc = batch_upload(b, 0, n, what);
    // (a skipped point's entries come back as the caller filled them)
    if (rc == NRAYS_OK) rc = order_status(hipMemcpyAsync(w->d_ray_keys, out_keys, (size_t)pairs * sizeof(uint64_t), hipMemcpyHostToDevice, b.stream), what);
    if (rc == NRAYS_OK)
        rc = gather_order_chunk(sc, w, pairs, chunk_points(c, 0ull), hemisphere_spec(params->num_dirs, params->num_rotations, params->bias), (const double*)c[kPointDirs],
                                (const double*)c[kPointRotations], b.stream);
    if (rc == NRAYS_OK) rc = order_status(hipMemcpyAsync(&out_info[3], w->d_ray_bins + kNumBins, sizeof(uint32_t), hipMemcpyDeviceToHost, b.stream), what);
    if (rc == NRAYS_OK) rc = order_status(hipStreamSynchronize(b.stream), what);
    if (rc == NRAYS_OK && out_info[3] > pairs) rc = set_last_error(NRAYS_ERR_HIP, "nrays_debug_gather_order: more pairs placed than the chunk holds");
    if (rc == NRAYS_OK) rc = order_status(hipMemcpyAsync(out_keys, w->d_ray_keys, (size_t)pairs * sizeof(uint64_t), hipMemcpyDeviceToHost, b.stream), what);
    if (rc == NRAYS_OK && out_info[3]) rc = order_status(hipMemcpyAsync(out_order, w->d_ray_order, (size_t)out_info[3] * sizeof(uint32_t), hipMemcpyDeviceToHost, b.stream), what);
    if (rc == NRAYS_OK) rc = order_status(hipMemcpyAsync(out_frame, w->d_ray_frame, NRAYS_RAY_FRAME_DOUBLES * sizeof(double), hipMemcpyDeviceToHost, b.stream), what);
    rc = batch_drain(b, rc, what);
    batch_close(b);
    return rc;
}

} // extern "C"
