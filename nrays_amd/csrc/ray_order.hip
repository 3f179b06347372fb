// ray_order.hip — caller-ray batches that come in no useful order (NRAYS_RAYS_UNORDERED): the rays of a chunk are binned by a spatial key
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
// then k_trace_rays_ordered / k_intersects_rays_ordered (ray_batch_kernel.h).  A counting sort on B bits, not a radix sort of the key: the
// order inside a bin is free, and need not be reproducible — a ray's arithmetic is its own, whatever wave it runs in.
//
// The atomics are spread over 2^21 counters, and the lanes of a wave that meet in one bin (the rays of a half-ordered batch do) are
// pre-reduced: they issue ONE atomic for their number (returning atomics on one word retire one every ~100 ns on this chip,
// DESIGN §5 "Scheduling").
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/nrays_abi.h"
#include "ray_batch_kernel.h"
#include "ray_key.h"
#include "ray_order.h"

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
    // The lanes of the wave that meet in one bin issue ONE atomic: their first lane adds their number, the others take their places from it.
    // The groups are found first (wave-uniform loop, one round per distinct bin, no memory access), then every group's atomic is in flight at once.
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
    if (active) rank[i] = first + below;
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

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
#define RO_TRY(expr)                                                                                                                          \
    do {                                                                                                                                      \
        hipError_t e_ = (expr);                                                                                                               \
        if (e_ != hipSuccess) return set_last_error(e_ == hipErrorOutOfMemory ? NRAYS_ERR_OOM : NRAYS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

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
    if (!w->d_ray_frame) RO_TRY(hipMalloc((void**)&w->d_ray_frame, kRayFrameDoubles * sizeof(double)));
    if (!w->d_ray_partial) RO_TRY(hipMalloc((void**)&w->d_ray_partial, (size_t)kBoundsMaxGrid * 10 * sizeof(double)));
    if (!w->d_ray_bins) RO_TRY(hipMalloc((void**)&w->d_ray_bins, (size_t)kNumBins * sizeof(uint32_t)));
    if (!w->d_ray_scan) RO_TRY(hipMalloc((void**)&w->d_ray_scan, (size_t)((kNumBins + kScanBlock - 1u) / kScanBlock) * sizeof(uint32_t)));
    if (n > w->order_rays) {
        free_per_ray(w);
        RO_TRY(hipMalloc((void**)&w->d_ray_keys, (size_t)n * sizeof(uint64_t)));
        RO_TRY(hipMalloc((void**)&w->d_ray_rank, (size_t)n * sizeof(uint32_t)));
        RO_TRY(hipMalloc((void**)&w->d_ray_order, (size_t)n * sizeof(uint32_t)));
        w->order_rays = n;
    }
    return NRAYS_OK;
}

int ray_order_chunk(const NraysScene* sc, TraceWorkspace* w, uint32_t n, const double* origins, const double* dirs, hipStream_t stream) {
    if (n == 0u || n > w->order_rays) return set_last_error(NRAYS_ERR_BAD_ARG, "ray_order_chunk: workspace too small");
    SceneBox box;
    for (int a = 0; a < 3; ++a) { box.v[a] = (double)sc->host.bounds_mn[a]; box.v[3 + a] = (double)sc->host.bounds_mx[a]; }
    const uint32_t ray_grid = (n + kOrderBlock - 1u) / kOrderBlock, parts = ray_grid < kBoundsMaxGrid ? ray_grid : kBoundsMaxGrid;
    const uint32_t scan_grid = (kNumBins + kScanBlock - 1u) / kScanBlock;
    RO_TRY(hipMemsetAsync(w->d_ray_bins, 0, (size_t)kNumBins * sizeof(uint32_t), stream));
    hipLaunchKernelGGL(k_ray_bounds, dim3(parts), dim3(kOrderBlock), 0, stream, n, origins, dirs, box, w->d_ray_partial);
    hipLaunchKernelGGL(k_ray_frame, dim3(1), dim3(kOrderBlock), 0, stream, (const double*)w->d_ray_partial, parts, box, w->d_ray_frame);
    hipLaunchKernelGGL(k_ray_keys, dim3(ray_grid), dim3(kOrderBlock), 0, stream, n, origins, dirs, (const double*)w->d_ray_frame, w->d_ray_keys, w->d_ray_bins, w->d_ray_rank);
    hipLaunchKernelGGL(k_bin_sums, dim3(scan_grid), dim3(kOrderBlock), 0, stream, (const uint32_t*)w->d_ray_bins, kNumBins, w->d_ray_scan);
    hipLaunchKernelGGL(k_bin_scan, dim3(1), dim3(1024), 0, stream, w->d_ray_scan, scan_grid);
    hipLaunchKernelGGL(k_bin_apply, dim3(scan_grid), dim3(kOrderBlock), 0, stream, w->d_ray_bins, kNumBins, (const uint32_t*)w->d_ray_scan);
    hipLaunchKernelGGL(k_ray_place, dim3(ray_grid), dim3(kOrderBlock), 0, stream, n, (const uint64_t*)w->d_ray_keys, (const uint32_t*)w->d_ray_rank, (const uint32_t*)w->d_ray_bins, w->d_ray_order);
    RO_TRY(hipGetLastError());
    return NRAYS_OK;
}

void launch_trace_rays_ordered(bool stats, int feat, uint32_t grid, hipStream_t stream, const DScene& S, uint32_t n, const uint32_t* order, const double* ro, const double* rd,
                               const double* refr, const float* energy, const unsigned long long* keys, unsigned long long key_base, uint32_t keyed, uint32_t max_depth,
                               float* out, const QueueOut& qo, DeviceCounters* ctr, uint32_t* spill) {
    if (stats) hipLaunchKernelGGL((k_trace_rays_ordered<true, kFeatAll>), dim3(grid), dim3(kBlock), 0, stream, S, n, order, ro, rd, refr, energy, keys, key_base, keyed, max_depth, out, qo, ctr, spill);
    else if (feat == (int)kFeatMesh) hipLaunchKernelGGL((k_trace_rays_ordered<false, kFeatMesh>), dim3(grid), dim3(kBlock), 0, stream, S, n, order, ro, rd, refr, energy, keys, key_base, keyed, max_depth, out, qo, ctr, spill);
    else hipLaunchKernelGGL((k_trace_rays_ordered<false, kFeatAll>), dim3(grid), dim3(kBlock), 0, stream, S, n, order, ro, rd, refr, energy, keys, key_base, keyed, max_depth, out, qo, ctr, spill);
}
void launch_intersects_rays_ordered(int feat, uint32_t grid, hipStream_t stream, const DScene& S, uint32_t n, const uint32_t* order, const double* ro, const double* rd,
                                    const double* max_toi, float* out_filter, uint32_t* out_lit, uint32_t* spill) {
    if (feat == (int)kFeatMesh) hipLaunchKernelGGL((k_intersects_rays_ordered<kFeatMesh>), dim3(grid), dim3(kBlock), 0, stream, S, n, order, ro, rd, max_toi, out_filter, out_lit, spill);
    else hipLaunchKernelGGL((k_intersects_rays_ordered<kFeatAll>), dim3(grid), dim3(kBlock), 0, stream, S, n, order, ro, rd, max_toi, out_filter, out_lit, spill);
}

} // namespace nrays
