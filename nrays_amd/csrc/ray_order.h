// ray_order.h — what the caller-batch code calls of ray_order.hip: the reorder buffers of the batch workspace and the reorder of one chunk.  Host only.
#pragma once
#include "ray_key.h"
#include "scene_handle.h"

namespace nrays {

struct GatherPoints; struct OcclusionSpec; // hemisphere_device.h
constexpr uint32_t kNumBins = 1u << kRayBinBits; // counters of the counting sort; TraceWorkspace::d_ray_bins holds one word more (a gather chunk's live pairs)

// Grows the reorder buffers of `w` to n rays (n <= kTraceChunk).  NRAYS_OK or a negative status with the last error set.
int ray_order_ensure(TraceWorkspace* w, uint32_t n);
void ray_order_release(TraceWorkspace* w);
// Enqueues the reorder of one chunk (device pointers) on `stream`: frame reduction, keys + bin counts, prefix sum, placement.  Launches only —
// nothing is read back and nothing waits.  Afterwards (in stream order) w->d_ray_order[j] = the ray to trace j-th, w->d_ray_keys / d_ray_frame
// hold the keys and the frame.
int ray_order_chunk(const NraysScene* sc, TraceWorkspace* w, uint32_t n, const double* origins, const double* dirs, hipStream_t stream);
// The reorder of one gather chunk's pairs (pairs = nc * num_dirs <= kTraceChunk), enqueued on `stream` as ray_order_chunk enqueues a ray chunk's: launches only.
// Afterwards w->d_ray_order[0 .. m) holds the m live pairs in trace order and w->d_ray_bins[2^B] holds m; d_ray_keys / d_ray_frame hold the live pairs' keys and the frame.
int gather_order_chunk(const NraysScene* sc, TraceWorkspace* w, uint32_t pairs, const GatherPoints& in, const OcclusionSpec& G, const double* dirs, const double* rotations,
                       hipStream_t stream);

} // namespace nrays
