// point_batches.hip — the caller-batch families that take surface points and build a hemisphere of rays a point on the device, each a check, a column table
// (batch_stage.h) and a chunk launch run by the driver of batch_call.h: nrays_occlusion_points* (k_occlusion_points: instantiated in ray_batches.hip beside the other traversal kernels, launched through launch_occlusion_points),
// nrays_gather_points* (+ _ex) and nrays_gather_sh_points* (kernels: gather_inst.hip, gather_order_inst.hip; k_gather_fold here, k_gather_fold_sh of gather_sh_kernel.h),
// nrays_gather_maps_points* (gather_maps_inst.hip).  Also two probes: nrays_debug_occlusion_rays (k_occlusion_rays) and nrays_debug_gather_sh_fold.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "../../include/nrays_abi.h"
#include "batch_call.h"
#include "bounce.h"
#include "gather_maps_kernel.h"
#include "gather_sh_kernel.h"
#include "ray_batch_kernel.h"
#include "ray_order.h"
#include "scene_handle.h"

namespace nrays {

constexpr uint32_t kFoldBlock = 256u; // threads per workgroup of k_gather_fold

// The points of a chunk, as the kernels take them (columns kPointPoints .. kPointKeys of the chunk).
struct PointsIn { const double* points; const double* normals; const uint32_t* hit_flags; const unsigned long long* keys; };
static PointsIn points_in(void* const* c) {
    return PointsIn{(const double*)c[kPointPoints], (const double*)c[kPointNormals], (const uint32_t*)c[kPointHit], (const unsigned long long*)c[kPointKeys]};
}

// ---- nrays_occlusion_points*: ambient occlusion at caller-supplied points, the hemisphere rays built on the device ------------------------------------
static int check_occlusion_params(const NraysOcclusionParams* p) {
    if (!p || !p->dirs) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (p->num_dirs < 1u || p->num_dirs > 1024u) return set_last_error(NRAYS_ERR_BAD_ARG, "NraysOcclusionParams: num_dirs must be in 1 .. 1024");
    if (p->num_rotations > 1024u || (p->num_rotations && !p->rotations)) return set_last_error(NRAYS_ERR_BAD_ARG, "NraysOcclusionParams: num_rotations > 1024, or rotations is NULL");
    if (!(p->max_toi > 0.0)) return set_last_error(NRAYS_ERR_BAD_ARG, "NraysOcclusionParams: max_toi must be > 0 (+inf allowed)");
    if (!std::isfinite(p->bias)) return set_last_error(NRAYS_ERR_BAD_ARG, "NraysOcclusionParams: bias must be finite");
    return NRAYS_OK;
}
static OcclusionSpec occlusion_spec(const NraysOcclusionParams* p) { return OcclusionSpec{p->num_dirs, p->num_rotations, p->bias, p->max_toi}; }
static int occlusion_points_impl(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const uint64_t* keys,
                                 const NraysOcclusionParams* p, float* out_filter, uint32_t* out_open, uint32_t flags, bool staged, hipStream_t stream) {
    if (!sc || !points || !normals || !out_filter) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (check_occlusion_params(p) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    if (flags != 0u) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_occlusion_points: flags must be 0");
    if (n == 0) return NRAYS_OK;
    StageColumn cols[kOccColumns];
    point_columns(cols, p->dirs, p->num_dirs, p->rotations, p->num_rotations, points, normals, hit_flags, keys);
    occlusion_columns(cols, out_filter, out_open);
    // One chunk (nc <= point_chunk); the permutation: kFeatMesh or kFeatAll, as k_intersects_rays.
    auto launch = [&](const BatchCall& b, uint32_t nc, void* const* c, unsigned long long key_base) -> int {
        const PointsIn in = points_in(c);
        const OcclusionSpec spec = occlusion_spec(p);
        const double *dirs = (const double*)c[kPointDirs], *rotations = (const double*)c[kPointRotations];
        float* filter = (float*)c[kOccFilter]; uint32_t* open = (uint32_t*)c[kOccOpen];
        const int lp = occlusion_lanes_log2(sc, spec.num_dirs);
        const uint32_t slots = nc << lp; // (nc * num_dirs <= kTraceChunk and 2^lp <= num_dirs)
        const uint32_t grid = std::min<uint32_t>((slots + kBlock - 1) / kBlock, (uint32_t)kMaxGrid);
        launch_occlusion_points(traversal_feat(sc), lp, grid, b.stream, sc->facts.d, nc, in.points, in.normals, in.hit_flags, in.keys, key_base, spec, dirs, rotations, filter, open, b.w->d_spill);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return set_last_error(NRAYS_ERR_HIP, std::string("k_occlusion_points: ") + hipGetErrorString(e));
        return NRAYS_OK;
    };
    return batch_run(sc, staged, stream, cols, kOccColumns, n, point_chunk(p->num_dirs), "occlusion batch", launch);
}

// ---- nrays_gather_points*: the mean of Scene::trace over the hemisphere rays of caller-supplied points, the rays built on the device --------------------------
int check_gather_args(const NraysScene* sc, const double* points, const double* normals, const NraysGatherParams* p, const float* out_rgb, uint32_t flags, bool hinted) {
    if (!sc || !points || !normals || !p || !p->dirs || !out_rgb) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
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
// Double-branching scenes: the fold that k_gather_points left to the end of the chunk's k_bounce rounds — point i's num_dirs finished ray colours, summed in the
// order of j in f32 and divided once.  One lane per point; the colours were just written and sit in L2.
__global__ void __launch_bounds__(kFoldBlock) k_gather_fold(const float* __restrict__ rays, uint32_t n, uint32_t k, float* __restrict__ out) {
    const uint32_t i = blockIdx.x * kFoldBlock + threadIdx.x;
    if (i >= n) return;
    const float* c = rays + 3 * (size_t)i * k;
    float x = 0.0f, y = 0.0f, z = 0.0f;
    for (uint32_t j = 0; j < k; ++j) { x += c[3 * j]; y += c[3 * j + 1]; z += c[3 * j + 2]; }
    const float fk = (float)k;
    out[3 * (size_t)i] = x / fk; out[3 * (size_t)i + 1] = y / fk; out[3 * (size_t)i + 2] = z / fk;
}
// One chunk (nc <= point_chunk) of nrays_gather_points*; `in` and `out` are the chunk's, key_base the index of its first point in the batch, dirs / rotations
// device copies of the tables.  The permutation is trace_chunk's, the lanes per point are k_occlusion_points'.  Double-branching scenes: the kernel stores the
// chunk's ray colours, trace_chunk's rounds run over the queued second children with a ray as the "pixel" (queue and sums sized by the chunk's RAYS, by trace_chunk's
// rule), and k_gather_fold folds: the only case with per-ray memory, 36 bytes a ray of the workspace beside the queue.
// `reorder` (a hinted call that pays, nrays_gather_points*_ex): the chunk's pairs are binned (gather_order_chunk) and traced in bin order by k_gather_pairs_ordered, every
// scene through the cleared per-ray colours and k_gather_fold: 12 bytes of colour and 16 of sort state a ray of the chunk, whatever the scene.
// `bands` > 0 (nrays_gather_sh_points*): the same trace kernels, always through the per-ray colours — queued or not, reordered or not —, and k_gather_fold_sh
// (gather_sh_kernel.h) folds them into 3 * bands^2 floats a point of `out` instead of k_gather_fold's 3.
static int gather_chunk_launch(NraysScene* sc, TraceWorkspace* w, uint32_t nc, const PointsIn& in, unsigned long long key_base, const NraysGatherParams* p,
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
    const int feat = stats ? (int)kFeatAll : shading_feat(sc);
    const GatherPoints pts{in.points, in.normals, in.hit_flags, in.keys, key_base};
    if (reorder) {
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
        const GatherLaunch a{grid, stream, &sc->facts.d, nc, in.points, in.normals, in.hit_flags, in.keys, key_base, spec, dirs, rotations, out, ray_out, &qo,
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
        const uint32_t grid = std::min<uint32_t>((nc + kShGroups - 1u) / kShGroups, kShMaxGrid);
        hipLaunchKernelGGL(k_gather_fold_sh, dim3(grid), dim3(kShBlock), 0, stream, (const float*)ray_out, nc, pts, OcclusionSpec{p->num_dirs, p->num_rotations, p->bias, 0.0}, dirs,
                           rotations, bands * bands, out);
    } else {
        hipLaunchKernelGGL(k_gather_fold, dim3((nc + kFoldBlock - 1u) / kFoldBlock), dim3(kFoldBlock), 0, stream, (const float*)ray_out, nc, p->num_dirs, out);
    }
    HIP_TRY(hipGetLastError());
    if (overflowed) return set_last_error(NRAYS_ERR_QUEUE_OVERFLOW, "continuation-ray queue overflow: some gathered colours are incomplete");
    return NRAYS_OK;
}
// `bands` = 0: nrays_gather_points* (3 floats a point); 1 .. 3: nrays_gather_sh_points* (3 * bands^2 floats a point), checked by the caller.
static int gather_points_impl(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const uint64_t* keys, const NraysGatherParams* p,
                              float* out, uint32_t flags, bool hinted, uint32_t bands, bool staged, hipStream_t stream) {
    if (check_gather_args(sc, points, normals, p, out, flags, hinted) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    if (n == 0) return NRAYS_OK;
    StageColumn cols[kGatherColumns];
    point_columns(cols, p->dirs, p->num_dirs, p->rotations, p->num_rotations, points, normals, hit_flags, keys);
    gather_columns(cols, out, gather_out_floats(bands), nullptr, p->num_dirs);
    const bool reorder = gather_reorders(sc, n, p, flags);
    auto launch = [&](const BatchCall& b, uint32_t nc, void* const* c, unsigned long long key_base) -> int {
        return gather_chunk_launch(sc, b.w, nc, points_in(c), key_base, p, (const double*)c[kPointDirs], (const double*)c[kPointRotations], (float*)c[kGatherOut], reorder, bands, b.stream);
    };
    return batch_run(sc, staged, stream, cols, kGatherColumns, n, point_chunk(p->num_dirs), "gather batch", launch);
}

// ---- nrays_gather_maps_points*: the light of baked maps at the closest hits of the hemisphere rays of caller-supplied points (gather_maps_kernel.h) -------------
static int check_gather_maps_args(const NraysScene* sc, const double* points, const double* normals, const NraysGatherMapsParams* p, const float* out_rgb, uint32_t flags) {
    if (!sc || !points || !normals || !p || !p->dirs || !p->maps || !p->node_map || !out_rgb) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
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
static int gather_maps_impl(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const uint64_t* keys, const NraysGatherMapsParams* p,
                            float* out_rgb, uint32_t* out_counts, uint32_t flags, bool staged, hipStream_t stream) {
    if (check_gather_maps_args(sc, points, normals, p, out_rgb, flags) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    if (n == 0) return NRAYS_OK;
    const void* texels[NRAYS_GATHER_MAX_MAPS]; size_t texel_count[NRAYS_GATHER_MAX_MAPS];
    for (uint32_t m = 0; m < p->num_maps; ++m) { texels[m] = p->maps[m].texels; texel_count[m] = (size_t)p->maps[m].width * p->maps[m].height; }
    StageColumn cols[kMapsTexels + NRAYS_GATHER_MAX_MAPS];
    point_columns(cols, p->dirs, p->num_dirs, p->rotations, p->num_rotations, points, normals, hit_flags, keys);
    const int ncols = gather_maps_columns(cols, out_rgb, out_counts, p->node_map, p->num_nodes, p->num_maps, texels, texel_count);
    const GatherMapsSpec spec{p->num_dirs, p->num_rotations, p->bias, p->max_toi, p->num_maps, p->num_nodes, {p->miss_rgb[0], p->miss_rgb[1], p->miss_rgb[2]}};
    // One chunk (nc <= point_chunk).  The permutation is k_cast_rays', the lanes per point are k_occlusion_points'.
    auto launch = [&](const BatchCall& b, uint32_t nc, void* const* c, unsigned long long key_base) -> int {
        GatherMapsTable table; // the kernel's view of the checked parameters: the map records as the shading records hold a texture (ShadeTex), at the chunk's texel addresses
        std::memset(&table, 0, sizeof table);
        for (uint32_t m = 0; m < p->num_maps; ++m) {
            const NraysTexture& s = p->maps[m];
            table.map[m].texels = c[kMapsTexels + m]; table.map[m].width = s.width; table.map[m].height = s.height; table.map[m].mode = s.format | (s.interp << 8) | (s.overflow << 16);
        }
        const PointsIn in = points_in(c);
        const int lp = occlusion_lanes_log2(sc, p->num_dirs);
        const uint32_t slots = nc << lp; // (nc * num_dirs <= kTraceChunk and 2^lp <= num_dirs)
        const uint32_t grid = std::min<uint32_t>((slots + kBlock - 1) / kBlock, (uint32_t)kMaxGrid);
        const GatherMapsLaunch a{grid, b.stream, &sc->facts.d, nc, in.points, in.normals, in.hit_flags, in.keys, key_base, spec, &table, (const int32_t*)c[kMapsNodeMap],
                                 (const double*)c[kPointDirs], (const double*)c[kPointRotations], (float*)c[kMapsRgb], (uint32_t*)c[kMapsCounts], b.w->d_spill};
        if (!launch_gather_maps_points(a, traversal_feat(sc), lp)) return set_last_error(NRAYS_ERR_UNSUPPORTED, "k_gather_maps_points: no such permutation");
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return set_last_error(NRAYS_ERR_HIP, std::string("k_gather_maps_points: ") + hipGetErrorString(e));
        return NRAYS_OK;
    };
    return batch_run(sc, staged, stream, cols, ncols, n, point_chunk(p->num_dirs), "gather maps batch", launch);
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

} // namespace nrays

using namespace nrays;

extern "C" {

int nrays_occlusion_points_device(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const uint64_t* keys,
                                  const NraysOcclusionParams* params, float* out_filter, uint32_t* out_open, uint32_t flags, void* hip_stream) {
    return occlusion_points_impl(sc, n, points, normals, hit_flags, keys, params, out_filter, out_open, flags, false, (hipStream_t)hip_stream);
}
int nrays_occlusion_points(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const uint64_t* keys,
                           const NraysOcclusionParams* params, float* out_filter, uint32_t* out_open, uint32_t flags) {
    return occlusion_points_impl(sc, n, points, normals, hit_flags, keys, params, out_filter, out_open, flags, true, nullptr);
}
int nrays_debug_occlusion_rays(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint64_t* keys, const NraysOcclusionParams* params,
                               double* out_origins, double* out_dirs) {
    return occlusion_rays_probe(sc, n, points, normals, keys, params, out_origins, out_dirs);
}

int nrays_gather_points_device(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const uint64_t* keys,
                               const NraysGatherParams* params, float* out_rgb, uint32_t flags, void* hip_stream) {
    return gather_points_impl(sc, n, points, normals, hit_flags, keys, params, out_rgb, flags, false, 0u, false, (hipStream_t)hip_stream);
}
int nrays_gather_points_device_ex(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const uint64_t* keys,
                                  const NraysGatherParams* params, float* out_rgb, uint32_t flags, void* hip_stream) {
    return gather_points_impl(sc, n, points, normals, hit_flags, keys, params, out_rgb, flags, true, 0u, false, (hipStream_t)hip_stream);
}
int nrays_gather_points(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const uint64_t* keys,
                        const NraysGatherParams* params, float* out_rgb, uint32_t flags) {
    return gather_points_impl(sc, n, points, normals, hit_flags, keys, params, out_rgb, flags, false, 0u, true, nullptr);
}
int nrays_gather_points_ex(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const uint64_t* keys,
                           const NraysGatherParams* params, float* out_rgb, uint32_t flags) {
    return gather_points_impl(sc, n, points, normals, hit_flags, keys, params, out_rgb, flags, true, 0u, true, nullptr);
}
int nrays_gather_sh_points_device(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const uint64_t* keys,
                                  const NraysGatherParams* params, uint32_t bands, float* out_sh, uint32_t flags, void* hip_stream) {
    if (check_sh_bands(bands) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    return gather_points_impl(sc, n, points, normals, hit_flags, keys, params, out_sh, flags, true, bands, false, (hipStream_t)hip_stream);
}
int nrays_gather_sh_points(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const uint64_t* keys,
                           const NraysGatherParams* params, uint32_t bands, float* out_sh, uint32_t flags) {
    if (check_sh_bands(bands) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    return gather_points_impl(sc, n, points, normals, hit_flags, keys, params, out_sh, flags, true, bands, true, nullptr);
}

int nrays_gather_maps_points_device(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const uint64_t* keys,
                                    const NraysGatherMapsParams* params, float* out_rgb, uint32_t* out_counts, uint32_t flags, void* hip_stream) {
    return gather_maps_impl(sc, n, points, normals, hit_flags, keys, params, out_rgb, out_counts, flags, false, (hipStream_t)hip_stream);
}
int nrays_gather_maps_points(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const uint64_t* keys,
                             const NraysGatherMapsParams* params, float* out_rgb, uint32_t* out_counts, uint32_t flags) {
    return gather_maps_impl(sc, n, points, normals, hit_flags, keys, params, out_rgb, out_counts, flags, true, nullptr);
}

// k_gather_fold_sh alone on caller-supplied ray colours, one chunk, through the staging arena; the kernel between events of its own when out_kernel_ms is wanted.
int nrays_debug_gather_sh_fold(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const uint64_t* keys,
                               const NraysGatherParams* params, uint32_t bands, const float* ray_colours, float* out_sh, float* out_kernel_ms) {
    if (!ray_colours) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (check_sh_bands(bands) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    if (check_gather_args(sc, points, normals, params, out_sh, 0u, true) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    if ((uint64_t)n * params->num_dirs > kTraceChunk) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_debug_gather_sh_fold: at most one chunk (n * num_dirs <= 2^22)");
    if (out_kernel_ms) *out_kernel_ms = 0.0f;
    if (n == 0) return NRAYS_OK;
    const char* what = "nrays_debug_gather_sh_fold";
    StageColumn cols[kGatherColumns];
    point_columns(cols, params->dirs, params->num_dirs, params->rotations, params->num_rotations, points, normals, hit_flags, keys);
    gather_columns(cols, out_sh, gather_out_floats(bands), ray_colours, params->num_dirs);
    BatchCall b;
    int rc = batch_open(&b, sc, true, nullptr, cols, kGatherColumns, n);
    if (rc != NRAYS_OK) return rc;
    void* c[kGatherColumns];
    batch_columns(b, 0, c);
    rc = batch_upload_tables(b, what);
    if (rc == NRAYS_OK) rc = batch_upload(b, 0, n, what);
    hipEvent_t ev[2] = {nullptr, nullptr};
    hipError_t e = hipSuccess;
    if (rc == NRAYS_OK && out_kernel_ms) { e = hipEventCreate(&ev[0]); if (e == hipSuccess) e = hipEventCreate(&ev[1]); if (e == hipSuccess) e = hipEventRecord(ev[0], b.stream); }
    if (rc == NRAYS_OK && e == hipSuccess) {
        const PointsIn in = points_in(c);
        const GatherPoints pts{in.points, in.normals, in.hit_flags, in.keys, 0ull};
        const uint32_t grid = std::min<uint32_t>((n + kShGroups - 1u) / kShGroups, kShMaxGrid);
        hipLaunchKernelGGL(k_gather_fold_sh, dim3(grid), dim3(kShBlock), 0, b.stream, (const float*)c[kGatherRays], n, pts, OcclusionSpec{params->num_dirs, params->num_rotations, params->bias, 0.0},
                           (const double*)c[kPointDirs], (const double*)c[kPointRotations], bands * bands, (float*)c[kGatherOut]);
        e = hipGetLastError();
    }
    if (rc == NRAYS_OK && e == hipSuccess && out_kernel_ms) e = hipEventRecord(ev[1], b.stream);
    if (rc == NRAYS_OK && e == hipSuccess) rc = batch_download(b, 0, n, what);
    rc = batch_drain(b, rc, what);
    if (rc == NRAYS_OK && e == hipSuccess && out_kernel_ms) e = hipEventElapsedTime(out_kernel_ms, ev[0], ev[1]);
    for (hipEvent_t v : ev) if (v) (void)hipEventDestroy(v);
    batch_close(b);
    if (rc == NRAYS_OK && e != hipSuccess) rc = set_last_error(NRAYS_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    return rc;
}

} // extern "C"
