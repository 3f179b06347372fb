// batch_call.h — the driver every caller-batch entry point runs through (batch_call.cpp; host only, no kernels).  A family — trace, intersects, cast, shade,
// material (ray_batches.hip), occlusion, gather, gather_sh, gather_maps, gather_maps_sh, probe_depth, irradiance, nearest, light (point_batches.hip), surface / dilate / filter texels (texel_calls.hip), the probes
// nrays_debug_cast_batch, nrays_debug_occlusion_rays and nrays_debug_light_rays — is four things of its own ("Adding a family on the C++ side"): its argument check (with the
// n == 0 return, before any HIP call), its column table (batch_stage.h), its launch struct with a launch_if chain, and its chunk lambda.  The driver holds the rest once:
//   batch_open    hipSetDevice, the handle's batch workspace, the family's own workspace (`ensure`), the staging arena, the stream — the caller's for the
//                 device form, the handle's own for the blocking form — and the ordering behind the handle's previous work
//   batch_run     the tables once; per chunk the `in` columns, the family's launch with the chunk's device pointers and key_base = its first item, the `out`
//                 columns, a synchronize.  The device form is the same loop with staging off: the pointers are the caller's, advanced to the chunk; nothing
//                 is copied and nothing waits.  The blocking form drains its stream before it returns, whatever failed: the uploads read the caller's
//                 memory, and the next call reuses the arena.
//   batch_close   the handle's "last work" bookkeeping
// A call allocates nothing on the heap: the columns are a fixed array of the family's frame, the launch a reference to its lambda.
#pragma once
#include "batch_stage.h"
#include "scene_handle.h"

namespace nrays {

struct BatchCall {
    NraysScene* sc = nullptr; TraceWorkspace* w = nullptr;
    hipStream_t stream = nullptr; bool staged = false; // staged: the blocking form (host arrays through the arena, on sc->buf.own_stream)
    const StageColumn* cols = nullptr; int ncols = 0;
    size_t off[kStageMaxColumns] = {};                 // staged: the columns' offsets in w->d_stage
};
// The family's own workspace (texel owner words, dilate dx words, the reorder buffers of a probe), ensured before the call is ordered behind the handle's work.
using BatchEnsure = int (*)(TraceWorkspace* w, const void* arg);
// The family's chunk launch on b.stream with b.w: nc items, col[k] the chunk's device pointer of column k (null: absent), key_base the index of the chunk's first item in the call.
// A reference to a callable on the caller's stack.
class ChunkLaunch {
    void* obj_; int (*call_)(void*, const BatchCall&, uint32_t, void* const*, unsigned long long);
public:
    template <class F> ChunkLaunch(F& f) : obj_(&f), call_([](void* o, const BatchCall& b, uint32_t nc, void* const* col, unsigned long long key_base) { return (*static_cast<F*>(o))(b, nc, col, key_base); }) {}
    int operator()(const BatchCall& b, uint32_t nc, void* const* col, unsigned long long key_base) const { return call_(obj_, b, nc, col, key_base); }
};

// `cap`: the most items a chunk of this call holds (sizes the arena; unused by the device form).  A negative status leaves nothing to close.
int batch_open(BatchCall* b, NraysScene* sc, bool staged, hipStream_t caller_stream, const StageColumn* cols, int ncols, size_t cap, BatchEnsure ensure = nullptr,
               const void* ensure_arg = nullptr);
void batch_close(const BatchCall& b);
// The pieces of batch_run, for the probes that put events or copies of their own between them.  `what` names the call in an error's text.
void batch_columns(const BatchCall& b, size_t c0, void** col);              // the device pointers of the chunk that starts at item c0
int batch_upload_tables(const BatchCall& b, const char* what);              // staged: enqueues the copies; device form: nothing
int batch_upload(const BatchCall& b, size_t c0, size_t nc, const char* what);
int batch_download(const BatchCall& b, size_t c0, size_t nc, const char* what);
int batch_drain(const BatchCall& b, int rc, const char* what);              // staged: synchronizes, always; the first error of rc and the stream
// A whole call of n > 0 items in chunks of `chunk`: open, run, close.  The first error.
int batch_run(NraysScene* sc, bool staged, hipStream_t caller_stream, const StageColumn* cols, int ncols, uint32_t n, uint32_t chunk, const char* what, ChunkLaunch launch,
              BatchEnsure ensure = nullptr, const void* ensure_arg = nullptr);

// ---- what the families share ----
// The permutation of a kernel that only traverses (kFeatMultiSample is the light loop's) and of one that shades (the scene's own feature set): kFeatMesh for
// scenes of opaque meshes, kFeatAll otherwise.
inline int traversal_feat(const NraysScene* sc) { return (sc->facts.features & ~(int)kFeatMultiSample) == (int)kFeatMesh ? (int)kFeatMesh : (int)kFeatAll; }
inline int shading_feat(const NraysScene* sc) { return (sc->facts.features & ~(int)kFeatLdsScene) == (int)kFeatMesh ? (int)kFeatMesh : (int)kFeatAll; }
inline uint32_t point_chunk(uint32_t num_dirs) { return stage_point_chunk(kTraceChunk, num_dirs); } // points per chunk: at most kTraceChunk rays
// A batch the caller called unordered (NRAYS_RAYS_UNORDERED) is reordered when the host can see that it pays: the reorder is eight launches in
// front of the trace (a launch of a handle has a period of ~11 us), which a small batch does not earn back.  kReorderMinRays: DESIGN §5b.
constexpr uint32_t kReorderMinRays = 1u << 19;
bool reorder_pays(const NraysScene* sc, uint32_t n);
int check_ray_flags(uint32_t flags);
// The reorder of one chunk (ray_order.hip) when it is due: *order = the order to trace in, or nullptr (trace the rays as they come).
int chunk_order(NraysScene* sc, TraceWorkspace* w, bool reorder, uint32_t n, const double* o, const double* d, hipStream_t stream, const uint32_t** order);
// Lanes per point (log2), among the instantiated 0, 3 and 6: as many lanes as there are directions to give them.  Measured (profiles/occlusion_rate.json, sponza
// stand-in): at 2 M points x 16 directions 8 lanes take 3.07 ms against 4.77 ms with one lane per point and 3.03 ms for k_intersects_rays on the same rays; at
// 16 384 points x 64 directions 64 lanes take 0.136 ms, 8 lanes 0.205, one lane 1.47 (a grid of 64 workgroups).  The lanes of a point share its origin, and that is
// the coherence the traversal lives on; one lane per point is left to batches of fewer than 8 directions.  NRAYS_OCCLUSION_LANES=0|3|6 forces a form (the A/B of
// tools/trace_rays_rate.py --occlusion; the results do not depend on it).
int occlusion_lanes_log2(const NraysScene* sc, uint32_t num_dirs);
// A kernel's launch is written in the unit that instantiates it (ray_batches.hip, gather_inst.hip, gather_order_inst.hip, gather_maps_inst.hip, probe_depth_inst.hip, light_points_inst.hip): an argument struct and
// `bool launch_<kernel>(const Args&, ...selectors...)`, a chain launch_if<...>(a, ...) || ... of the instantiated permutations; false = none, NRAYS_ERR_UNSUPPORTED here.
uint32_t launch_grid(uint64_t items);  // workgroups of kBlock lanes for `items` lanes, at most kMaxGrid: the kernels stride (ray_batches.hip, beside the kernels)
int launch_status(const char* kernel); // after a launch: hipGetLastError() as NRAYS_OK, or NRAYS_ERR_HIP with "<kernel>: <the error>"
int no_permutation(const char* kernel); // NRAYS_ERR_UNSUPPORTED, "<kernel>: no such permutation"
// What the families at surface points share: the check of the hemisphere's tables and bias ("null argument" or "<struct_name>: ..."; `with` / `with_finite`: a value of
// the struct reported together with the bias), the generator's view of them (max_toi 0) and the kernels' view of a chunk's point columns kPointPoints .. kPointKeys.
struct GatherPoints; struct OcclusionSpec; // hemisphere_device.h
int check_hemisphere(const char* struct_name, const double* dirs, uint32_t num_dirs, const double* rotations, uint32_t num_rotations, double bias, const char* with = nullptr,
                     bool with_finite = true);
OcclusionSpec hemisphere_spec(uint32_t num_dirs, uint32_t num_rotations, double bias);
GatherPoints chunk_points(void* const* col, unsigned long long key_base);
// point_batches.hip: the argument check of nrays_gather_points*, which the gather-order probe of ray_order.hip shares.  `hinted`: the _ex entry points, which take
// NRAYS_RAYS_UNORDERED; the others take no flag at all.
int check_gather_args(const NraysScene* sc, const double* points, const double* normals, const NraysGatherParams* p, const float* out_rgb, uint32_t flags, bool hinted);

} // namespace nrays
