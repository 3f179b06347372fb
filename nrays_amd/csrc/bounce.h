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

// The queued trace of one chunk of a caller batch on its workspace (nrays_trace_rays*, nrays_gather_points*): `rays` rays, each the "pixel" of its own chain, 3 floats a ray.
// queued_trace_begin, before the chunk's trace kernel: the counters cleared and *qo filled; double-branching scenes: the queue pair by a frame's rule per pixel, per ray
// here (4 slots, at least 2^16, at most 2^27) and the fixed sums; other scenes: capacity 0.  queued_trace_finish, after it (double-branching scenes only): the rounds over
// `colours`, then an overflow as NRAYS_ERR_QUEUE_OVERFLOW, "... some <noun> colours are incomplete" (every launch is enqueued all the same).
struct QueueOut; // trace_device.h
int queued_trace_begin(const NraysScene* sc, TraceWorkspace* w, uint32_t rays, hipStream_t stream, QueueOut* qo);
int queued_trace_finish(const NraysScene* sc, TraceWorkspace* w, uint32_t rays, uint32_t max_depth, float* colours, const char* noun, hipStream_t stream);

} // namespace nrays
