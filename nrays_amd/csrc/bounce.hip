// bounce.hip — the continuation queue's rounds, shared by the frames (frame_path.hip) and the caller-ray batches (ray_batches.hip, point_batches.hip):
//   k_bounce      rounds over the compacted HBM queue (double-branching scenes only): the per-ray work of k_primary, the weighted contribution added to
//                 the pixel's 64-bit fixed-point sum (order-independent), second children appended to the next round's queue;
//   k_fold_fixed  adds those sums to the frame (or to a chunk's colours) after the rounds of a sample batch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/nrays_abi.h"
#include "batch_call.h"
#include "bounce.h"
#include "primary_kernel.h"

namespace nrays {

// Value range of the fixed-point sums (2^-32 units in a signed 64-bit integer): a contribution is clamped to +-9.0e18 units (|x| <= 2.1e9 — colours
// are O(1)), a NaN contribution counts as 0 (the float atomicAdd it replaced would have poisoned the pixel; the reference's f32 sum too), and a sum of
// several clamped contributions can wrap — none of which a frame of finite O(1) radiances can reach.
__device__ __forceinline__ long long to_fixed(float x) {
    double v = (double)x * 4294967296.0;
    v = v > 9.0e18 ? 9.0e18 : (v < -9.0e18 ? -9.0e18 : v); // (NaN -> 0 below)
    return v == v ? __double2ll_rn(v) : 0ll;
}
// out += fixed-point sums of the queued chains (k_bounce), which are cleared for the next sample batch.
__global__ void k_fold_fixed(float* __restrict__ out, long long* __restrict__ fixed, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const long long f = fixed[i];
    if (f != 0ll) { out[i] = out[i] + (float)((double)f * (1.0 / 4294967296.0)); fixed[i] = 0ll; }
}

template <bool STATS>
__global__ void __launch_bounds__(kBlock, NRAYS_WAVES_PER_SIMD) k_bounce(DScene S, RayQueue qin, const uint32_t* __restrict__ count_in, uint32_t capacity,
                                                    QueueOut qo, long long* __restrict__ fixed, DeviceCounters* ctr, uint32_t* spill,
                                                    uint32_t max_depth) {
    __shared__ uint32_t lds_stack[kLdsStack * kBlock];
    Stack st; st.setup(lds_stack, spill, nullptr);
    Cnt cnt; cnt.zero();
    uint32_t n = *count_in;
    if (n > capacity) n = capacity;
    for (uint32_t base = blockIdx.x * kBlock; base < n; base += gridDim.x * kBlock) { // block-uniform trip count
        uint32_t idx = base + threadIdx.x;
        bool active = idx < n;
        RayState ray;
        ray.o = D3(0, 0, 0); ray.d = D3(0, 0, 1); ray.refr = 1.0; ray.energy = 0.0f; ray.weight = 0.0f; ray.key = 0; ray.pixel = 0;
        uint32_t depth = 0;
        if (active) queue_load(qin, idx, ray, depth);
        f3 c = trace_chain<STATS, kFeatAll>(S, st, active, ray, depth, max_depth, qo, cnt, true);
        if (active) {
            // The queued chains of a pixel finish in no particular order.  Their contributions are therefore summed as 64-bit
            // FIXED-POINT numbers (2^-32 units: integer addition is associative, so the sum does not depend on the order) and
            // folded into the frame by k_fold_fixed once the rounds of the batch are over: frames of double-branching scenes are
            // bit-reproducible.  The 2.3e-10 quantum is far below the f32 resolution of a pixel value.
            unsigned long long* f = (unsigned long long*)(fixed + (size_t)ray.pixel * 3);
            atomicAdd(f, (unsigned long long)to_fixed(c.x)); atomicAdd(f + 1, (unsigned long long)to_fixed(c.y)); atomicAdd(f + 2, (unsigned long long)to_fixed(c.z));
        }
    }
    flush_counters(ctr, cnt, STATS);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
int ensure_queue_pair(QueueMem* queue, uint32_t& queue_capacity, uint32_t capacity) {
    if (capacity <= queue_capacity) return NRAYS_OK;
    queue_capacity = 0; // (a failure below leaves the pair empty, not half-sized)
    for (int k = 0; k < 2; ++k) {
        if (queue[k].block) { (void)hipFree(queue[k].block); queue[k].block = nullptr; }
        size_t cap = capacity;
        size_t bytes = cap * (8 * 7 + 4 * 4 + 8);
        void* p = nullptr;
        HIP_TRY(hipMalloc(&p, bytes));
        queue[k].block = p;
        char* c = (char*)p;
        RayQueue& q = queue[k].q;
        for (int a = 0; a < 3; ++a) { q.o[a] = (double*)c; c += cap * 8; }
        for (int a = 0; a < 3; ++a) { q.d[a] = (double*)c; c += cap * 8; }
        q.refr = (double*)c; c += cap * 8;
        q.key = (unsigned long long*)c; c += cap * 8;
        q.energy = (float*)c; c += cap * 4;
        q.weight = (float*)c; c += cap * 4;
        q.pixel = (uint32_t*)c; c += cap * 4;
        q.depth = (uint32_t*)c; c += cap * 4;
    }
    queue_capacity = capacity;
    return NRAYS_OK;
}

int ensure_fixed_sums(long long** fixed, size_t* fixed_slots, bool* dirty, size_t slots, hipStream_t stream) {
    if (slots > *fixed_slots) {
        const int rc = grow_device((void**)fixed, fixed_slots, slots, sizeof(long long));
        if (rc != NRAYS_OK) return rc;
        HIP_TRY(hipMemsetAsync(*fixed, 0, slots * sizeof(long long), stream)); // k_fold_fixed leaves it cleared
    }
    // a frame that failed between its k_bounce rounds and k_fold_fixed left sums behind: they must not reach this frame
    if (*dirty) { HIP_TRY(hipMemsetAsync(*fixed, 0, *fixed_slots * sizeof(long long), stream)); *dirty = false; }
    return NRAYS_OK;
}

// rounds of queued second children (host-controlled: the count is read back after every round)
// k_bounce takes its ray count from device memory and strides over it, so a round can be launched without knowing the
// count: the host only looks (one small copy + a stream synchronisation) before every FOURTH round — to stop, and to size
// that group's grids — instead of before every round; a group's later rounds may find an empty queue and return at once.
int run_bounce_rounds(const BounceRounds& b, hipStream_t stream, uint32_t* overflow_seen) {
    uint32_t seen[2] = {0u, 0u}; // queue count of the round, overflow word — read together, after every round before it has run
    bool drained = false, folded = true;
    for (uint32_t r = 1; r <= (uint32_t)kMaxGenerations; ++r) {
        if ((r - 1u) % 4u == 0u) {
            HIP_TRY(hipMemcpyAsync(&seen[0], b.counts + r, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
            if (overflow_seen) HIP_TRY(hipMemcpyAsync(&seen[1], b.overflow, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            if (seen[0] == 0u) { drained = true; break; }
        }
        const uint32_t launch_n = std::min<uint32_t>(seen[0], b.capacity); // the group's first count bounds nothing, it only sizes the grid
        const uint32_t grid = std::max<uint32_t>(launch_grid(launch_n), std::min<uint32_t>((uint32_t)b.num_cus, kMaxGrid));
        QueueOut qn; qn.q = b.queue[(r + 1) & 1].q; qn.capacity = b.capacity; qn.count = b.counts + r + 1; qn.overflow = b.overflow;
        if (b.stats) hipLaunchKernelGGL(k_bounce<true>, dim3(grid), dim3(kBlock), 0, stream, *b.scene, b.queue[r & 1].q, b.counts + r, b.capacity, qn, b.fixed, b.counters, b.spill, b.max_depth);
        else hipLaunchKernelGGL(k_bounce<false>, dim3(grid), dim3(kBlock), 0, stream, *b.scene, b.queue[r & 1].q, b.counts + r, b.capacity, qn, b.fixed, b.counters, b.spill, b.max_depth);
        HIP_TRY(hipGetLastError());
        folded = false; *b.fixed_dirty = true;
    }
    if (!folded) { // the next batch's k_primary continues the running sums in `out`: fold this batch's queued chains in first
        hipLaunchKernelGGL(k_fold_fixed, dim3((unsigned)((b.out_floats + 255) / 256)), dim3(256), 0, stream, b.out, b.fixed, b.out_floats);
        HIP_TRY(hipGetLastError());
        *b.fixed_dirty = false;
    }
    if (overflow_seen) {
        if (!drained) { // the generation cap ended the rounds: the overflow word has not been read after the last of them
            HIP_TRY(hipMemcpyAsync(&seen[1], b.overflow, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
        }
        *overflow_seen = seen[1];
    }
    return NRAYS_OK;
}

int queued_trace_begin(const NraysScene* sc, TraceWorkspace* w, uint32_t rays, hipStream_t stream, QueueOut* qo) {
    const bool queued = sc->facts.host.any_double_branch;
    int rc = queued ? ensure_queue_pair(w->queue, w->queue_capacity, (uint32_t)std::min<uint64_t>(std::max<uint64_t>(4ull * rays, 1u << 16), 1ull << 27)) : (int)NRAYS_OK;
    if (rc == NRAYS_OK && queued) rc = ensure_fixed_sums(&w->d_fixed, &w->fixed_slots, &w->fixed_dirty, (size_t)rays * 3, stream);
    if (rc != NRAYS_OK) return rc;
    HIP_TRY(hipMemsetAsync(w->d_counts, 0, kTraceCountWords * sizeof(uint32_t), stream));
    qo->q = w->queue[1].q; qo->capacity = queued ? w->queue_capacity : 0u; qo->count = w->d_counts + 1; qo->overflow = w->d_counts + kTraceCountWords - 1;
    return NRAYS_OK;
}
int queued_trace_finish(const NraysScene* sc, TraceWorkspace* w, uint32_t rays, uint32_t max_depth, float* colours, const char* noun, hipStream_t stream) {
    const BounceRounds rounds{w->queue, w->queue_capacity, w->d_counts, w->d_counts + kTraceCountWords - 1, w->d_fixed, &w->fixed_dirty, w->d_counters, w->d_spill, &sc->facts.d,
                              sc->facts.d.no_elide != 0u, max_depth, colours, (size_t)rays * 3, sc->facts.num_cus};
    uint32_t overflowed = 0u;
    const int rc = run_bounce_rounds(rounds, stream, &overflowed);
    return rc != NRAYS_OK || !overflowed ? rc : set_last_error(NRAYS_ERR_QUEUE_OVERFLOW, std::string("continuation-ray queue overflow: some ") + noun + " colours are incomplete");
}

} // namespace nrays
