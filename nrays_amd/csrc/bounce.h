// bounce.h — the rounds over the queue of second children (double-branching scenes): what frame_path.hip runs after a sample batch's
// k_primary, ray_batches.hip after a chunk's k_trace_rays and point_batches.hip after a chunk's gather kernel.  bounce.hip holds k_bounce and k_fold_fixed.  Host only.
#pragma once
#include "scene_handle.h"

namespace nrays {

// The two continuation queues of a render (the handle's) or of a caller-ray batch (TraceWorkspace), grown to `capacity` rays.
int ensure_queue_pair(QueueMem* queue, uint32_t& queue_capacity, uint32_t capacity);
// The fixed-point sums of the queued chains, grown to `slots` and cleared — also when a failed call left sums behind between its rounds and its fold (`dirty`).
int ensure_fixed_sums(long long** fixed, size_t* fixed_slots, bool* dirty, size_t slots, hipStream_t stream);

struct BounceRounds {
    const QueueMem* queue; uint32_t capacity; // the pair (k_primary / k_trace_rays appended to queue[1]) and the rays each holds
    uint32_t* counts; unsigned int* overflow; // counts[r]: rays queued for round r; the word a full queue sets
    long long* fixed; bool* fixed_dirty;      // the sums, and whether rounds were enqueued whose fold was not
    DeviceCounters* counters; uint32_t* spill;
    const DScene* scene; bool stats;          // stats: the kernel that counts everything and skips nothing (instrumented frames, scenes that must not elide)
    uint32_t max_depth;
    float* out; size_t out_floats;            // what k_fold_fixed adds the sums to
    int num_cus;
};
// The rounds on `stream` (the host looks at the count before every fourth one), then k_fold_fixed when any ran.  overflow_seen != nullptr: the overflow word is read back with
// every count and once more when the generation cap ended the rounds (caller-ray batches report it per call; a frame's is read by nrays_get_stats / the blocking renders).
int run_bounce_rounds(const BounceRounds& b, hipStream_t stream, uint32_t* overflow_seen);

} // namespace nrays
