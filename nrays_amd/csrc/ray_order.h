// ray_order.h — what nrays_hip.hip calls of ray_order.hip: the device-side reorder of a caller-ray chunk the caller called unordered
// (NRAYS_RAYS_UNORDERED) and the launches of the batch kernels' ordered forms.  Host only.
#pragma once
#include <hip/hip_runtime.h>

#include "scene_handle.h"
#include "trace_device.h"

namespace nrays {

// Grows the reorder buffers of `w` to n rays (n <= kTraceChunk).  NRAYS_OK or a negative status with the last error set.
int ray_order_ensure(TraceWorkspace* w, uint32_t n);
void ray_order_release(TraceWorkspace* w);
// Enqueues the reorder of one chunk (device pointers) on `stream`: frame reduction, keys + bin counts, prefix sum, placement.  Launches only —
// nothing is read back and nothing waits.  Afterwards (in stream order) w->d_ray_order[j] = the ray to trace j-th, w->d_ray_keys / d_ray_frame
// hold the keys and the frame.
int ray_order_chunk(const NraysScene* sc, TraceWorkspace* w, uint32_t n, const double* origins, const double* dirs, hipStream_t stream);

// k_trace_rays_ordered<stats, feat> with (stats, feat) one of k_trace_rays' three instantiations; k_intersects_rays_ordered<feat>.
void launch_trace_rays_ordered(bool stats, int feat, uint32_t grid, hipStream_t stream, const DScene& S, uint32_t n, const uint32_t* order, const double* ro, const double* rd,
                               const double* refr, const float* energy, const unsigned long long* keys, unsigned long long key_base, uint32_t keyed, uint32_t max_depth,
                               float* out, const QueueOut& qo, DeviceCounters* ctr, uint32_t* spill);
void launch_intersects_rays_ordered(int feat, uint32_t grid, hipStream_t stream, const DScene& S, uint32_t n, const uint32_t* order, const double* ro, const double* rd,
                                    const double* max_toi, float* out_filter, uint32_t* out_lit, uint32_t* spill);

} // namespace nrays
