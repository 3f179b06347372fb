// point_batches.hip — the caller-batch families that take surface points and build a hemisphere of rays a point on the device, each a check, a column table
// (batch_stage.h) and a chunk launch run by the driver of batch_call.h: nrays_occlusion_points* (k_occlusion_points: instantiated in ray_batches.hip beside the other traversal kernels, launched through launch_occlusion_points),
// nrays_gather_points* (+ _ex) and nrays_gather_sh_points* (kernels: gather_inst.hip, gather_order_inst.hip; k_gather_fold here, k_gather_fold_sh of gather_sh_kernel.h),
// nrays_gather_maps_points* (gather_maps_inst.hip), nrays_probe_depth_points* (probe_depth_inst.hip), nrays_gather_maps_sh_points* (gather_maps_sh_inst.hip, then the two
// folds), and the one family at points that builds no ray:
// nrays_irradiance_points* and nrays_irradiance_points_vis* (k_irradiance_points of irradiance_kernel.h, instantiated here), and the one that takes points anywhere in space:
// nrays_nearest_points* (k_nearest_points of nearest_kernel.h: nearest_inst.hip), and the one whose rays go towards a table of lights: nrays_light_points* (k_light_points of
// light_points_kernel.h: light_points_inst.hip).  Also four probes: nrays_debug_occlusion_rays (k_occlusion_rays), nrays_debug_light_rays (k_light_rays), nrays_debug_gather_sh_fold and
// nrays_debug_nearest_bound.  What the hemisphere kernels share on the device is hemisphere_device.h; what the two maps families and the three callers of
// k_gather_fold_sh share on the host is here (maps_texels, maps_spec, maps_table, launch_gather_fold_sh).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "../../include/nrays_abi.h"
#include "batch_call.h"
#include "bounce.h"
#include "gather_maps_kernel.h"
#include "gather_maps_sh_kernel.h"
#include "gather_sh_kernel.h"
#include "irradiance_kernel.h"
#include "light_points_kernel.h"
#include "nearest_kernel.h"
#include "probe_depth_kernel.h"
#include "ray_batch_kernel.h"
#include "ray_order.h"
#include "scene_handle.h"

namespace nrays {

constexpr uint32_t kFoldBlock = 256u; // threads per workgroup of k_gather_fold

GatherPoints chunk_points(void* const* c, unsigned long long key_base) {
    return GatherPoints{(const double*)c[kPointPoints], (const double*)c[kPointNormals], (const uint32_t*)c[kPointHit], (const unsigned long long*)c[kPointKeys], key_base};
}
OcclusionSpec hemisphere_spec(uint32_t num_dirs, uint32_t num_rotations, double bias) { return OcclusionSpec{num_dirs, num_rotations, bias, 0.0}; }

// ---- nrays_occlusion_points*: ambient occlusion at caller-supplied points, the hemisphere rays built on the device ------------------------------------
static int check_occlusion_params(const NraysOcclusionParams* p) {
    if (!p) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (check_hemisphere("NraysOcclusionParams", p->dirs, p->num_dirs, p->rotations, p->num_rotations, p->bias) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    if (!(p->max_toi > 0.0)) return set_last_error(NRAYS_ERR_BAD_ARG, "NraysOcclusionParams: max_toi must be > 0 (+inf allowed)");
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
        const int lp = occlusion_lanes_log2(sc, p->num_dirs); // (nc * num_dirs <= kTraceChunk and 2^lp <= num_dirs)
        const OcclusionLaunch a{launch_grid((uint64_t)nc << lp), b.stream, &sc->facts.d, nc, chunk_points(c, key_base), occlusion_spec(p), (const double*)c[kPointDirs],
                                (const double*)c[kPointRotations], (float*)c[kOccFilter], (uint32_t*)c[kOccOpen], b.w->d_spill};
        return launch_occlusion_points(a, traversal_feat(sc), lp) ? launch_status("k_occlusion_points") : no_permutation("k_occlusion_points");
    };
    return batch_run(sc, staged, stream, cols, kOccColumns, n, point_chunk(p->num_dirs), "occlusion batch", launch);
}

// ---- nrays_gather_points*: the mean of Scene::trace over the hemisphere rays of caller-supplied points, the rays built on the device --------------------------
int check_gather_args(const NraysScene* sc, const double* points, const double* normals, const NraysGatherParams* p, const float* out_rgb, uint32_t flags, bool hinted) {
    if (!sc || !points || !normals || !p || !out_rgb) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (check_hemisphere("NraysGatherParams", p->dirs, p->num_dirs, p->rotations, p->num_rotations, p->bias, "energy", std::isfinite(p->energy)) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
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
    const float fk = (float)k; // (store_mean, kept as text: through the call this kernel compiles to other instructions)
    out[3 * (size_t)i] = x / fk; out[3 * (size_t)i + 1] = y / fk; out[3 * (size_t)i + 2] = z / fk;
}
// k_gather_fold_sh (gather_sh_kernel.h) on the finished colours `rays` of a chunk's nc points: 3 * bands^2 floats a point to `out`.
static void launch_gather_fold_sh(hipStream_t stream, const float* rays, uint32_t nc, const GatherPoints& pts, const OcclusionSpec& hemi, const double* dirs, const double* rotations,
                                  uint32_t bands, float* out) {
    const uint32_t grid = std::min<uint32_t>((nc + kShGroups - 1u) / kShGroups, kShMaxGrid);
    hipLaunchKernelGGL(k_gather_fold_sh, dim3(grid), dim3(kShBlock), 0, stream, rays, nc, pts, hemi, dirs, rotations, bands * bands, out);
}
// One chunk (nc <= point_chunk) of nrays_gather_points*; `pts` and `out` are the chunk's, dirs / rotations
// device copies of the tables.  The permutation is launch_trace_rays', the lanes per point are occlusion_lanes_log2's.  Double-branching scenes: the kernel stores the
// chunk's ray colours, the rounds of queued_trace_finish run over the queued second children with a ray as the "pixel" (queue and sums sized by the chunk's RAYS, by queued_trace_begin's
// rule), and k_gather_fold folds: the only case with per-ray memory, 36 bytes a ray of the workspace beside the queue.
// `reorder` (a hinted call that pays, nrays_gather_points*_ex): the chunk's pairs are binned (gather_order_chunk) and traced in bin order by k_gather_pairs_ordered, every
// scene through the cleared per-ray colours and k_gather_fold: 12 bytes of colour and 16 of sort state a ray of the chunk, whatever the scene.
// `bands` > 0 (nrays_gather_sh_points*): the same trace kernels, always through the per-ray colours — queued or not, reordered or not —, and k_gather_fold_sh
// (gather_sh_kernel.h) folds them into 3 * bands^2 floats a point of `out` instead of k_gather_fold's 3.
static int gather_chunk_launch(NraysScene* sc, TraceWorkspace* w, uint32_t nc, const GatherPoints& pts, const NraysGatherParams* p, const double* dirs, const double* rotations,
                               float* out, bool reorder, uint32_t bands, hipStream_t stream) {
    const bool queued = sc->facts.host.any_double_branch;
    const uint32_t pairs = nc * p->num_dirs; // (<= kTraceChunk)
    const size_t ray_floats = 3 * (size_t)pairs;
    QueueOut qo;
    int rc = queued_trace_begin(sc, w, pairs, stream, &qo);
    const bool per_ray = queued || reorder || bands != 0u;
    if (rc == NRAYS_OK && per_ray) rc = grow_device(&w->d_gather_rays, &w->gather_ray_floats, ray_floats, sizeof(float));
    if (rc != NRAYS_OK) return rc;
    float* ray_out = per_ray ? (float*)w->d_gather_rays : nullptr;
    const GatherSpec spec{p->num_dirs, p->num_rotations, p->bias, p->energy, p->max_depth, sc->facts.host.any_area_light ? 1u : 0u};
    const OcclusionSpec hemi = hemisphere_spec(p->num_dirs, p->num_rotations, p->bias);
    const bool stats = sc->facts.d.no_elide != 0u;
    const int feat = stats ? (int)kFeatAll : shading_feat(sc);
    if (reorder) {
        rc = ray_order_ensure(w, pairs);
        if (rc == NRAYS_OK) rc = gather_order_chunk(sc, w, pairs, pts, hemi, dirs, rotations, stream);
        if (rc != NRAYS_OK) return rc;
        HIP_TRY(hipMemsetAsync(ray_out, 0, ray_floats * sizeof(float), stream)); // (a skipped point's pairs are never traced: exact zeros)
        // (the grid by the chunk's pairs: the live count stays on the device)
        const GatherPairsLaunch a{launch_grid(pairs), stream, &sc->facts.d, pairs, w->d_ray_order, w->d_ray_bins + kNumBins, pts, spec, dirs, rotations, ray_out, &qo, w->d_counters, w->d_spill};
        if (!launch_gather_pairs_ordered(a, stats, feat)) return no_permutation("k_gather_pairs_ordered");
    } else {
        const int lp = occlusion_lanes_log2(sc, p->num_dirs); // (2^lp <= num_dirs)
        const GatherLaunch a{launch_grid((uint64_t)nc << lp), stream, &sc->facts.d, nc, pts, spec, dirs, rotations, out, ray_out, &qo, w->d_counters, w->d_spill};
        if (!launch_gather_points(a, stats, feat, lp)) return no_permutation("k_gather_points");
    }
    HIP_TRY(hipGetLastError());
    if (!ray_out) return NRAYS_OK;
    if (queued) rc = queued_trace_finish(sc, w, pairs, p->max_depth, ray_out, "gathered", stream);
    if (rc != NRAYS_OK && rc != NRAYS_ERR_QUEUE_OVERFLOW) return rc; // (an overflow: the incomplete colours are folded all the same, and the status is the call's)
    if (bands) launch_gather_fold_sh(stream, ray_out, nc, pts, hemi, dirs, rotations, bands, out);
    else hipLaunchKernelGGL(k_gather_fold, dim3((nc + kFoldBlock - 1u) / kFoldBlock), dim3(kFoldBlock), 0, stream, (const float*)ray_out, nc, p->num_dirs, out);
    HIP_TRY(hipGetLastError());
    return rc;
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
        return gather_chunk_launch(sc, b.w, nc, chunk_points(c, key_base), p, (const double*)c[kPointDirs], (const double*)c[kPointRotations], (float*)c[kGatherOut], reorder, bands, b.stream);
    };
    return batch_run(sc, staged, stream, cols, kGatherColumns, n, point_chunk(p->num_dirs), "gather batch", launch);
}

// ---- nrays_gather_maps_points*: the light of baked maps at the closest hits of the hemisphere rays of caller-supplied points (gather_maps_kernel.h) -------------
static int check_gather_maps_args(const NraysScene* sc, const double* points, const double* normals, const NraysGatherMapsParams* p, const float* out_rgb, uint32_t flags) {
    if (!sc || !points || !normals || !p || !p->maps || !p->node_map || !out_rgb) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (check_hemisphere("NraysGatherMapsParams", p->dirs, p->num_dirs, p->rotations, p->num_rotations, p->bias, "miss_rgb",
                         std::isfinite(p->miss_rgb[0]) && std::isfinite(p->miss_rgb[1]) && std::isfinite(p->miss_rgb[2])) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
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
// What the two maps families make of the checked parameters: the host side of the texel columns, the kernels' spec, and per chunk the kernels' view of the maps —
// the map records as the shading records hold a texture (ShadeTex), at the chunk's texel addresses, columns first_texel_column .. of c.
static void maps_texels(const NraysGatherMapsParams* p, const void** texels, size_t* texel_count) {
    for (uint32_t m = 0; m < p->num_maps; ++m) { texels[m] = p->maps[m].texels; texel_count[m] = (size_t)p->maps[m].width * p->maps[m].height; }
}
static GatherMapsSpec maps_spec(const NraysGatherMapsParams* p) {
    return GatherMapsSpec{p->num_dirs, p->num_rotations, p->bias, p->max_toi, p->num_maps, p->num_nodes, {p->miss_rgb[0], p->miss_rgb[1], p->miss_rgb[2]}};
}
static GatherMapsTable maps_table(const NraysGatherMapsParams* p, void* const* c, int first_texel_column) {
    GatherMapsTable table;
    std::memset(&table, 0, sizeof table);
    for (uint32_t m = 0; m < p->num_maps; ++m) {
        const NraysTexture& s = p->maps[m];
        table.map[m].texels = c[first_texel_column + m]; table.map[m].width = s.width; table.map[m].height = s.height; table.map[m].mode = s.format | (s.interp << 8) | (s.overflow << 16);
    }
    return table;
}
static int gather_maps_impl(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const uint64_t* keys, const NraysGatherMapsParams* p,
                            float* out_rgb, uint32_t* out_counts, uint32_t flags, bool staged, hipStream_t stream) {
    if (check_gather_maps_args(sc, points, normals, p, out_rgb, flags) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    if (n == 0) return NRAYS_OK;
    const void* texels[NRAYS_GATHER_MAX_MAPS]; size_t texel_count[NRAYS_GATHER_MAX_MAPS];
    maps_texels(p, texels, texel_count);
    StageColumn cols[kMapsTexels + NRAYS_GATHER_MAX_MAPS];
    point_columns(cols, p->dirs, p->num_dirs, p->rotations, p->num_rotations, points, normals, hit_flags, keys);
    const int ncols = gather_maps_columns(cols, out_rgb, out_counts, p->node_map, p->num_nodes, p->num_maps, texels, texel_count);
    const GatherMapsSpec spec = maps_spec(p);
    // One chunk (nc <= point_chunk).  The permutation is the traversal's (traversal_feat), the lanes per point are occlusion_lanes_log2's.
    auto launch = [&](const BatchCall& b, uint32_t nc, void* const* c, unsigned long long key_base) -> int {
        const GatherMapsTable table = maps_table(p, c, kMapsTexels);
        const int lp = occlusion_lanes_log2(sc, p->num_dirs); // (nc * num_dirs <= kTraceChunk and 2^lp <= num_dirs)
        const GatherMapsLaunch a{launch_grid((uint64_t)nc << lp), b.stream, &sc->facts.d, nc, chunk_points(c, key_base), spec, &table, (const int32_t*)c[kMapsNodeMap],
                                 (const double*)c[kPointDirs], (const double*)c[kPointRotations], (float*)c[kMapsRgb], (uint32_t*)c[kMapsCounts], b.w->d_spill};
        return launch_gather_maps_points(a, traversal_feat(sc), lp) ? launch_status("k_gather_maps_points") : no_permutation("k_gather_maps_points");
    };
    return batch_run(sc, staged, stream, cols, ncols, n, point_chunk(p->num_dirs), "gather maps batch", launch);
}

// ---- nrays_probe_depth_points*: the depth moments, near / miss counts and nearest hit of the rays of caller-supplied points (probe_depth_kernel.h) -------------
// The settings NraysProbeDepthParams and NraysGatherDepthSpec share.
static int check_depth_settings(const char* struct_name, double max_dist, double near_dist, uint32_t res, uint32_t reserved) {
    const char* bad = !(std::isfinite(max_dist) && max_dist > 0.0) ? "max_dist must be finite and > 0" : !(std::isfinite(near_dist) && near_dist >= 0.0) ? "near_dist must be finite and >= 0"
                      : (res != 4u && res != 8u && res != 16u) ? "res must be 4, 8 or 16" : reserved != 0u ? "reserved must be 0" : nullptr;
    return bad ? set_last_error(NRAYS_ERR_BAD_ARG, std::string(struct_name) + ": " + bad) : NRAYS_OK;
}
static int check_probe_depth_args(const NraysScene* sc, const double* points, const double* normals, const NraysProbeDepthParams* p, const float* out_moments, uint32_t flags) {
    if (!sc || !points || !normals || !p || !out_moments) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (check_hemisphere("NraysProbeDepthParams", p->dirs, p->num_dirs, p->rotations, p->num_rotations, p->bias) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    if (check_depth_settings("NraysProbeDepthParams", p->max_dist, p->near_dist, p->res, p->reserved) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    if (flags != 0u) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_probe_depth_points: flags must be 0");
    return NRAYS_OK;
}
static int probe_depth_impl(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const uint64_t* keys, const NraysProbeDepthParams* p,
                            float* out_moments, uint32_t* out_counts, double* out_nearest, uint32_t* out_nearest_dir, uint32_t flags, bool staged, hipStream_t stream) {
    if (check_probe_depth_args(sc, points, normals, p, out_moments, flags) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    if (n == 0) return NRAYS_OK;
    StageColumn cols[kDepthColumns];
    point_columns(cols, p->dirs, p->num_dirs, p->rotations, p->num_rotations, points, normals, hit_flags, keys);
    probe_depth_columns(cols, out_moments, p->res, out_counts, out_nearest, out_nearest_dir);
    const ProbeDepthSpec spec{p->num_dirs, p->num_rotations, p->bias, p->max_dist, p->near_dist, p->res};
    // One chunk (nc <= point_chunk): the trace (the permutation is the traversal's, the lanes per point are occlusion_lanes_log2's) leaves rf of the chunk's rays in the
    // workspace, 4 bytes a ray, and the fold reads them in the order of j.
    auto launch = [&](const BatchCall& b, uint32_t nc, void* const* c, unsigned long long key_base) -> int {
        const size_t rays = (size_t)nc * p->num_dirs; // (<= kTraceChunk, or one point's)
        const int rc = grow_device(&b.w->d_gather_rays, &b.w->gather_ray_floats, rays, sizeof(float));
        if (rc != NRAYS_OK) return rc;
        const GatherPoints pts = chunk_points(c, key_base);
        const int lp = occlusion_lanes_log2(sc, p->num_dirs); // (nc * num_dirs <= kTraceChunk and 2^lp <= num_dirs)
        const ProbeDepthLaunch a{launch_grid((uint64_t)nc << lp), b.stream, &sc->facts.d, nc, pts, spec, (const double*)c[kPointDirs], (const double*)c[kPointRotations],
                                 (float*)b.w->d_gather_rays, (uint32_t*)c[kDepthCounts], (double*)c[kDepthNearest], (uint32_t*)c[kDepthNearestDir], b.w->d_spill};
        if (!launch_probe_depth_points(a, traversal_feat(sc), lp)) return no_permutation("k_probe_depth_points");
        HIP_TRY(hipGetLastError());
        const ProbeDepthFoldLaunch f{b.stream, nc, pts, spec, (const double*)c[kPointDirs], (const double*)c[kPointRotations], (const float*)b.w->d_gather_rays, (float*)c[kDepthMoments]};
        return launch_probe_depth_fold(f, p->res) ? launch_status("k_probe_depth_fold") : no_permutation("k_probe_depth_fold");
    };
    return batch_run(sc, staged, stream, cols, kDepthColumns, n, point_chunk(p->num_dirs), "probe depth batch", launch);
}

// ---- nrays_gather_maps_sh_points*: a probe filled from baked maps and what it sees of the geometry, from one traversal (gather_maps_sh_kernel.h) ------------------
static int gather_maps_sh_impl(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const uint64_t* keys, const NraysGatherMapsParams* p,
                               uint32_t bands, float* out_sh, uint32_t* out_counts, const NraysGatherDepthSpec* depth, float* out_moments, uint32_t* out_depth_counts,
                               double* out_nearest, uint32_t* out_nearest_dir, uint32_t flags, bool staged, hipStream_t stream) {
    if (check_gather_maps_args(sc, points, normals, p, out_sh, flags) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    if (check_sh_bands(bands) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    if (!depth && (out_moments || out_depth_counts || out_nearest || out_nearest_dir))
        return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_gather_maps_sh_points: depth outputs without a depth spec");
    if (depth && !out_moments) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (depth && check_depth_settings("NraysGatherDepthSpec", depth->max_dist, depth->near_dist, depth->res, depth->reserved) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    if (n == 0) return NRAYS_OK;
    const void* texels[NRAYS_GATHER_MAX_MAPS]; size_t texel_count[NRAYS_GATHER_MAX_MAPS];
    maps_texels(p, texels, texel_count);
    StageColumn cols[kStageMaxColumns];
    point_columns(cols, p->dirs, p->num_dirs, p->rotations, p->num_rotations, points, normals, hit_flags, keys);
    const int ncols = gather_maps_sh_columns(cols, out_sh, bands * bands, out_counts, out_moments, depth ? depth->res : 0u, out_depth_counts, out_nearest, out_nearest_dir, p->node_map,
                                             p->num_nodes, p->num_maps, texels, texel_count);
    const GatherMapsSpec spec = maps_spec(p);
    // One chunk (nc <= point_chunk): the trace (the permutations and the lanes per point as for nrays_gather_maps_points*) leaves c_ij of the chunk's rays in the workspace, 12 bytes
    // a ray, and with a depth spec rf behind them, 4 bytes a ray; the two folds of the parent calls read the planes in the order of j.
    auto launch = [&](const BatchCall& b, uint32_t nc, void* const* c, unsigned long long key_base) -> int {
        const size_t rays = (size_t)nc * p->num_dirs; // (<= kTraceChunk, or one point's)
        const int rc = grow_device(&b.w->d_gather_rays, &b.w->gather_ray_floats, rays * (depth ? 4u : 3u), sizeof(float));
        if (rc != NRAYS_OK) return rc;
        float* ray_rgb = (float*)b.w->d_gather_rays;
        const GatherMapsTable table = maps_table(p, c, kMapsShTexels);
        const GatherPoints pts = chunk_points(c, key_base);
        const double* dirs = (const double*)c[kPointDirs];
        const double* rotations = (const double*)c[kPointRotations];
        GatherMapsDepth dd{0.0, 0.0, nullptr, nullptr, nullptr, nullptr};
        if (depth) dd = GatherMapsDepth{depth->max_dist, depth->near_dist, ray_rgb + 3 * rays, (uint32_t*)c[kMapsShDepthCounts], (double*)c[kMapsShNearest], (uint32_t*)c[kMapsShNearestDir]};
        const int lp = occlusion_lanes_log2(sc, p->num_dirs); // (nc * num_dirs <= kTraceChunk and 2^lp <= num_dirs)
        const GatherMapsRaysLaunch a{launch_grid((uint64_t)nc << lp), b.stream, &sc->facts.d, nc, pts, spec, &table, (const int32_t*)c[kMapsShNodeMap], dirs, rotations, ray_rgb,
                                     (uint32_t*)c[kMapsShCounts], depth ? &dd : nullptr, b.w->d_spill};
        if (!launch_gather_maps_rays(a, traversal_feat(sc), lp)) return no_permutation("k_gather_maps_rays");
        HIP_TRY(hipGetLastError());
        launch_gather_fold_sh(b.stream, ray_rgb, nc, pts, hemisphere_spec(p->num_dirs, p->num_rotations, p->bias), dirs, rotations, bands, (float*)c[kMapsShSh]);
        if (!depth) return launch_status("k_gather_fold_sh");
        HIP_TRY(hipGetLastError());
        const ProbeDepthFoldLaunch f{b.stream, nc, pts, ProbeDepthSpec{p->num_dirs, p->num_rotations, p->bias, depth->max_dist, depth->near_dist, depth->res}, dirs, rotations,
                                     (const float*)dd.ray_rf, (float*)c[kMapsShMoments]};
        return launch_probe_depth_fold(f, depth->res) ? launch_status("k_probe_depth_fold") : no_permutation("k_probe_depth_fold");
    };
    return batch_run(sc, staged, stream, cols, ncols, n, point_chunk(p->num_dirs), "gather maps sh batch", launch);
}

// ---- nrays_irradiance_points*: the irradiance at caller-supplied points from a regular grid of SH probes (irradiance_kernel.h) ----------------------------------
template <int BANDS, bool WANT_SH, bool FACING, bool VIS>
static bool launch_if(const IrradianceLaunch& a, uint32_t bands, bool want_sh, bool facing, bool vis) {
    if (bands != (uint32_t)BANDS || want_sh != WANT_SH || facing != FACING || vis != VIS) return false;
    hipLaunchKernelGGL((k_irradiance_points<BANDS, WANT_SH, FACING, VIS>), dim3(a.grid), dim3(kBlock), 0, a.stream, a.n, a.points, a.normals, a.hit_flags, a.g, a.out_rgb, a.out_sh, a.out_weight);
    return true;
}
template <int BANDS, bool VIS>
static bool launch_if_bands(const IrradianceLaunch& a, uint32_t bands, bool want_sh, bool facing, bool vis) {
    return launch_if<BANDS, false, false, VIS>(a, bands, want_sh, facing, vis) || launch_if<BANDS, false, true, VIS>(a, bands, want_sh, facing, vis) ||
           launch_if<BANDS, true, false, VIS>(a, bands, want_sh, facing, vis) || launch_if<BANDS, true, true, VIS>(a, bands, want_sh, facing, vis);
}
bool launch_irradiance_points(const IrradianceLaunch& a, uint32_t bands, bool want_sh, bool facing, bool vis) {
    return launch_if_bands<1, false>(a, bands, want_sh, facing, vis) || launch_if_bands<2, false>(a, bands, want_sh, facing, vis) || launch_if_bands<3, false>(a, bands, want_sh, facing, vis) ||
           launch_if_bands<1, true>(a, bands, want_sh, facing, vis) || launch_if_bands<2, true>(a, bands, want_sh, facing, vis) || launch_if_bands<3, true>(a, bands, want_sh, facing, vis);
}
constexpr uint32_t kIrradianceMaxCount = 1024u, kIrradianceMaxProbes = 1u << 22;
static int check_irradiance_args(const NraysScene* sc, const double* points, const double* normals, const NraysIrradianceGrid* g, const float* out_rgb, const float* out_sh, uint32_t flags) {
    if (!sc || !points || !normals || !g || !g->sh) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (!out_rgb && !out_sh) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_irradiance_points: no output (out_rgb and out_sh are both null)");
    uint64_t probes = 1;
    for (int a = 0; a < 3; ++a) {
        if (g->counts[a] < 1u || g->counts[a] > kIrradianceMaxCount) return set_last_error(NRAYS_ERR_BAD_ARG, "NraysIrradianceGrid: counts must be in 1 .. 1024");
        probes *= g->counts[a];
        if (!std::isfinite(g->origin[a])) return set_last_error(NRAYS_ERR_BAD_ARG, "NraysIrradianceGrid: origin must be finite");
        if (g->counts[a] > 1u && !(std::isfinite(g->cell[a]) && g->cell[a] > 0.0))
            return set_last_error(NRAYS_ERR_BAD_ARG, "NraysIrradianceGrid: cell must be finite and > 0 on every axis with more than one probe");
    }
    if (probes > kIrradianceMaxProbes) return set_last_error(NRAYS_ERR_BAD_ARG, "NraysIrradianceGrid: at most 2^22 probes");
    if (g->bands < 1u || g->bands > 3u) return set_last_error(NRAYS_ERR_BAD_ARG, "NraysIrradianceGrid: bands must be in 1 .. 3");
    if (!std::isfinite(g->measure)) return set_last_error(NRAYS_ERR_BAD_ARG, "NraysIrradianceGrid: measure must be finite");
    if (g->reserved != 0u) return set_last_error(NRAYS_ERR_BAD_ARG, "NraysIrradianceGrid: reserved must be 0");
    if (flags & ~(uint32_t)NRAYS_IRRADIANCE_FACING) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_irradiance_points: unknown flag");
    return NRAYS_OK;
}
static int check_irradiance_vis(const NraysIrradianceVisibility* v) {
    if (!v || !v->moments) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (v->res != 4u && v->res != 8u && v->res != 16u) return set_last_error(NRAYS_ERR_BAD_ARG, "NraysIrradianceVisibility: res must be 4, 8 or 16");
    if (!(v->floor >= 0.0f && v->floor <= 1.0f)) return set_last_error(NRAYS_ERR_BAD_ARG, "NraysIrradianceVisibility: floor must be in [0, 1]");
    if (!std::isfinite(v->bias)) return set_last_error(NRAYS_ERR_BAD_ARG, "NraysIrradianceVisibility: bias must be finite");
    return NRAYS_OK;
}
// `v`: null for nrays_irradiance_points*; NraysIrradianceVisibility (checked here) for nrays_irradiance_points_vis*, one more table and the VIS permutations.
static int irradiance_points_impl(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const NraysIrradianceGrid* g,
                                  const NraysIrradianceVisibility* v, bool vis, float* out_rgb, float* out_sh, float* out_weight, uint32_t flags, bool staged, hipStream_t stream) {
    if (check_irradiance_args(sc, points, normals, g, out_rgb, out_sh, flags) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    if (vis && check_irradiance_vis(v) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    if (n == 0) return NRAYS_OK;
    const uint32_t coefs = g->bands * g->bands;
    const size_t probes = (size_t)g->counts[0] * g->counts[1] * g->counts[2];
    StageColumn cols[kIrrVisColumns];
    irradiance_columns(cols, g->sh, g->valid, probes, coefs, points, normals, hit_flags, out_rgb, out_sh, out_weight);
    const int ncols = vis ? irradiance_vis_columns(cols, v->moments, probes, v->res) : (int)kIrrColumns;
    auto launch = [&](const BatchCall& b, uint32_t nc, void* const* c, unsigned long long) -> int {
        IrradianceGrid k;
        for (int a = 0; a < 3; ++a) { k.origin[a] = g->origin[a]; k.counts[a] = g->counts[a]; k.cell[a] = g->counts[a] > 1u ? g->cell[a] : 0.0; }
        k.sh = (const float*)c[kIrrSh]; k.valid = (const uint32_t*)c[kIrrValid]; k.measure = g->measure;
        k.moments = vis ? (const float*)c[kIrrMoments] : nullptr; k.res = vis ? v->res : 0u; k.floor = vis ? v->floor : 0.0f; k.bias = vis ? v->bias : 0.0;
        const IrradianceLaunch a{launch_grid(nc), b.stream, nc, (const double*)c[kIrrPoints], (const double*)c[kIrrNormals], (const uint32_t*)c[kIrrHit], k,
                                 (float*)c[kIrrRgb], (float*)c[kIrrOutSh], (float*)c[kIrrWeight]};
        return launch_irradiance_points(a, g->bands, out_sh != nullptr, (flags & NRAYS_IRRADIANCE_FACING) != 0u, vis) ? launch_status("k_irradiance_points") : no_permutation("k_irradiance_points");
    };
    return batch_run(sc, staged, stream, cols, ncols, n, kTraceChunk, "irradiance batch", launch);
}

// ---- nrays_nearest_points*: the nearest surface to caller-supplied points (nearest_kernel.h) ----------------------------------------------------------------------
static int check_nearest_args(const NraysScene* sc, const double* points, const double* out_dist, const int32_t* out_node, uint32_t flags) {
    if (!sc || !points || !out_dist || !out_node) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (flags != 0u) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_nearest_points: flags must be 0");
    return NRAYS_OK;
}
// The scene's coordinate bound, the absolute term of the cull's margin (nearest_margin): the largest |coordinate| of a bounded node's world AABB plus the largest
// |translation| of an instance.  Every local coordinate the leaf arithmetic sees is within sqrt(3) times it.
static double nearest_coord_bound(const NraysScene* sc) {
    const HostScene& h = sc->facts.host;
    double box = 0.0, trans = 0.0;
    for (double v : h.node_aabbs) if (std::fabs(v) < 1e300) box = std::max(box, std::fabs(v)); // (a plane's AABB is +-MAX)
    for (const Instance& in : h.instances) for (double v : in.trans) if (std::isfinite(v)) trans = std::max(trans, std::fabs(v));
    return box + trans;
}
static int nearest_points_impl(NraysScene* sc, uint32_t n, const double* points, const double* max_dist, const uint32_t* hit_flags, double* out_dist, int32_t* out_node,
                               double* out_point, double* out_normal, double* out_uv, int32_t* out_prim, uint32_t* out_flags, uint32_t flags, bool staged, hipStream_t stream) {
    if (check_nearest_args(sc, points, out_dist, out_node, flags) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    if (n == 0) return NRAYS_OK;
    StageColumn cols[kNearColumns];
    nearest_columns(cols, points, max_dist, hit_flags, out_dist, out_node, out_point, out_normal, out_uv, out_prim, out_flags);
    const double coord_bound = nearest_coord_bound(sc);
    auto launch = [&](const BatchCall& b, uint32_t nc, void* const* c, unsigned long long) -> int {
        const NearestLaunch a{launch_grid(nc), b.stream, &sc->facts.d, nc, (const double*)c[kNearPoints], (const double*)c[kNearMaxDist], (const uint32_t*)c[kNearHit], coord_bound,
                              (double*)c[kNearDist], (int32_t*)c[kNearNode], (double*)c[kNearPoint], (double*)c[kNearNormal], (double*)c[kNearUv], (int32_t*)c[kNearPrim],
                              (uint32_t*)c[kNearFlags], b.w->d_spill};
        return launch_nearest_points(a, traversal_feat(sc)) ? launch_status("k_nearest_points") : no_permutation("k_nearest_points");
    };
    return batch_run(sc, staged, stream, cols, kNearColumns, n, kTraceChunk, "nearest batch", launch);
}

// ---- nrays_light_points*: direct light at caller-supplied points from a caller-supplied table of point lights (light_points_kernel.h: light_points_inst.hip) --------
constexpr uint32_t kLightMaxLights = 4096u;
static int check_point_lights(const NraysPointLights* l) {
    if (!l || !l->positions || !l->colors) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (l->num_lights < 1u || l->num_lights > kLightMaxLights) return set_last_error(NRAYS_ERR_BAD_ARG, "NraysPointLights: num_lights must be in 1 .. 4096");
    if (l->flags & ~(uint32_t)NRAYS_LIGHTS_INVERSE_SQUARE) return set_last_error(NRAYS_ERR_BAD_ARG, "NraysPointLights: unknown flag");
    if (!std::isfinite(l->bias)) return set_last_error(NRAYS_ERR_BAD_ARG, "NraysPointLights: bias must be finite");
    if (!(std::isfinite(l->offset) && l->offset >= 0.0)) return set_last_error(NRAYS_ERR_BAD_ARG, "NraysPointLights: offset must be finite and >= 0");
    if ((l->flags & NRAYS_LIGHTS_INVERSE_SQUARE) && !(std::isfinite(l->min_dist) && l->min_dist > 0.0))
        return set_last_error(NRAYS_ERR_BAD_ARG, "NraysPointLights: min_dist must be finite and > 0 with NRAYS_LIGHTS_INVERSE_SQUARE");
    return NRAYS_OK;
}
static LightSpec light_spec(const NraysPointLights* l) {
    const bool falloff = (l->flags & NRAYS_LIGHTS_INVERSE_SQUARE) != 0u;
    return LightSpec{l->num_lights, falloff ? 1u : 0u, l->bias, l->offset, falloff ? l->min_dist : 1.0};
}
static LightTables light_tables(void* const* c) { return LightTables{(const double*)c[kLightPositions], (const float*)c[kLightColors], (const double*)c[kLightNormals]}; }
static int light_points_impl(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const NraysPointLights* l, float* out_rgb,
                             uint32_t* out_counts, uint32_t flags, bool staged, hipStream_t stream) {
    if (!sc || !points || !normals || !out_rgb) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (check_point_lights(l) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    if (flags != 0u) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_light_points: flags must be 0");
    if (n == 0) return NRAYS_OK;
    StageColumn cols[kLightColumns];
    light_columns(cols, l->positions, l->colors, l->normals, l->num_lights, points, normals, hit_flags, out_rgb, out_counts);
    // One chunk (nc <= point_chunk); the permutation: kFeatMesh or kFeatAll, as k_intersects_rays; the lanes per point are occlusion_lanes_log2's, by the lights.
    auto launch = [&](const BatchCall& b, uint32_t nc, void* const* c, unsigned long long) -> int {
        const int lp = occlusion_lanes_log2(sc, l->num_lights); // (nc << lp <= kTraceChunk: nc * num_lights <= kTraceChunk and 2^lp <= num_lights, or nc == 1)
        const LightPointsLaunch a{launch_grid((uint64_t)nc << lp), b.stream, &sc->facts.d, nc, (const double*)c[kLightPoints], (const double*)c[kLightPointNormals],
                                  (const uint32_t*)c[kLightHit], light_spec(l), light_tables(c), (float*)c[kLightRgb], (uint32_t*)c[kLightCounts], b.w->d_spill};
        return launch_light_points(a, traversal_feat(sc), lp) ? launch_status("k_light_points") : no_permutation("k_light_points");
    };
    return batch_run(sc, staged, stream, cols, kLightColumns, n, point_chunk(l->num_lights), "light batch", launch);
}

// nrays_debug_occlusion_rays: ray j of point i of the chunk, as k_occlusion_points generates it, to out[(i * num_dirs + j) * 3 ..].  NULL keys: key_base + i.
__global__ void __launch_bounds__(kBlock) k_occlusion_rays(uint32_t n, const double* __restrict__ points, const double* __restrict__ normals,
                                                           const unsigned long long* __restrict__ keys, unsigned long long key_base, OcclusionSpec P,
                                                           const double* __restrict__ dirs, const double* __restrict__ rotations, double* __restrict__ out_origins,
                                                           double* __restrict__ out_dirs) {
    const size_t rays = (size_t)n * P.num_dirs;
    const GatherPoints in{points, normals, nullptr, keys, key_base};
    for (size_t r = (size_t)blockIdx.x * kBlock + threadIdx.x; r < rays; r += (size_t)gridDim.x * kBlock) {
        const size_t i = r / P.num_dirs, j = r % P.num_dirs;
        const OccFrame f = point_frame_live(in, i, P, rotations);
        const d3 d = hemisphere_dir(f, P.num_rotations != 0u, dirs, j);
        out_origins[3 * r] = f.o.x; out_origins[3 * r + 1] = f.o.y; out_origins[3 * r + 2] = f.o.z;
        out_dirs[3 * r] = d.x; out_dirs[3 * r + 1] = d.y; out_dirs[3 * r + 2] = d.z;
    }
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
// nrays_debug_occlusion_rays: the generator of k_occlusion_points alone, on host arrays, blocking, in the family's chunks (a test probe).
int nrays_debug_occlusion_rays(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint64_t* keys, const NraysOcclusionParams* p,
                               double* out_origins, double* out_dirs) {
    if (!sc || !points || !normals || !out_origins || !out_dirs) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (check_occlusion_params(p) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    if (n == 0) return NRAYS_OK;
    StageColumn cols[kOccRaysColumns];
    point_columns(cols, p->dirs, p->num_dirs, p->rotations, p->num_rotations, points, normals, nullptr, keys);
    occlusion_rays_columns(cols, out_origins, out_dirs, p->num_dirs);
    auto launch = [&](const BatchCall& b, uint32_t nc, void* const* c, unsigned long long key_base) -> int {
        const GatherPoints in = chunk_points(c, key_base);
        hipLaunchKernelGGL(k_occlusion_rays, dim3(launch_grid((uint64_t)nc * p->num_dirs)), dim3(kBlock), 0, b.stream, nc, in.points, in.normals, in.keys, in.key_base, occlusion_spec(p),
                           (const double*)c[kPointDirs], (const double*)c[kPointRotations], (double*)c[kOccRaysOrigins], (double*)c[kOccRaysDirs]);
        return launch_status("k_occlusion_rays");
    };
    return batch_run(sc, true, nullptr, cols, kOccRaysColumns, n, point_chunk(p->num_dirs), "occlusion probe", launch);
}

int nrays_light_points_device(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const NraysPointLights* lights,
                              float* out_rgb, uint32_t* out_counts, uint32_t flags, void* hip_stream) {
    return light_points_impl(sc, n, points, normals, hit_flags, lights, out_rgb, out_counts, flags, false, (hipStream_t)hip_stream);
}
int nrays_light_points(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const NraysPointLights* lights, float* out_rgb,
                       uint32_t* out_counts, uint32_t flags) {
    return light_points_impl(sc, n, points, normals, hit_flags, lights, out_rgb, out_counts, flags, true, nullptr);
}
// nrays_debug_light_rays: the generator of k_light_points alone, on host arrays, blocking, in the family's chunks (a test probe).
int nrays_debug_light_rays(NraysScene* sc, uint32_t n, const double* points, const double* normals, const NraysPointLights* l, double* out_origins, double* out_dirs,
                           double* out_tmax, float* out_w) {
    if (!sc || !points || !normals || !out_origins || !out_dirs || !out_tmax || !out_w) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (check_point_lights(l) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    if (n == 0) return NRAYS_OK;
    StageColumn cols[kLightRaysColumns];
    light_columns(cols, l->positions, l->colors, l->normals, l->num_lights, points, normals, nullptr, nullptr, nullptr);
    light_rays_columns(cols, out_origins, out_dirs, out_tmax, out_w, l->num_lights);
    auto launch = [&](const BatchCall& b, uint32_t nc, void* const* c, unsigned long long) -> int {
        launch_light_rays(LightRaysLaunch{launch_grid((uint64_t)nc * l->num_lights), b.stream, nc, (const double*)c[kLightPoints], (const double*)c[kLightPointNormals], light_spec(l),
                                          light_tables(c), (double*)c[kLightRaysOrigins], (double*)c[kLightRaysDirs], (double*)c[kLightRaysTmax], (float*)c[kLightRaysW]});
        return launch_status("k_light_rays");
    };
    return batch_run(sc, true, nullptr, cols, kLightRaysColumns, n, point_chunk(l->num_lights), "light probe", launch);
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

int nrays_gather_maps_sh_points_device(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const uint64_t* keys,
                                       const NraysGatherMapsParams* params, uint32_t bands, float* out_sh, uint32_t* out_counts, const NraysGatherDepthSpec* depth,
                                       float* out_moments, uint32_t* out_depth_counts, double* out_nearest, uint32_t* out_nearest_dir, uint32_t flags, void* hip_stream) {
    return gather_maps_sh_impl(sc, n, points, normals, hit_flags, keys, params, bands, out_sh, out_counts, depth, out_moments, out_depth_counts, out_nearest, out_nearest_dir, flags, false,
                               (hipStream_t)hip_stream);
}
int nrays_gather_maps_sh_points(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const uint64_t* keys,
                                const NraysGatherMapsParams* params, uint32_t bands, float* out_sh, uint32_t* out_counts, const NraysGatherDepthSpec* depth, float* out_moments,
                                uint32_t* out_depth_counts, double* out_nearest, uint32_t* out_nearest_dir, uint32_t flags) {
    return gather_maps_sh_impl(sc, n, points, normals, hit_flags, keys, params, bands, out_sh, out_counts, depth, out_moments, out_depth_counts, out_nearest, out_nearest_dir, flags, true,
                               nullptr);
}

int nrays_irradiance_points_device(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const NraysIrradianceGrid* grid,
                                   float* out_rgb, float* out_sh, float* out_weight, uint32_t flags, void* hip_stream) {
    return irradiance_points_impl(sc, n, points, normals, hit_flags, grid, nullptr, false, out_rgb, out_sh, out_weight, flags, false, (hipStream_t)hip_stream);
}
int nrays_irradiance_points(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const NraysIrradianceGrid* grid,
                            float* out_rgb, float* out_sh, float* out_weight, uint32_t flags) {
    return irradiance_points_impl(sc, n, points, normals, hit_flags, grid, nullptr, false, out_rgb, out_sh, out_weight, flags, true, nullptr);
}
int nrays_irradiance_points_vis_device(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const NraysIrradianceGrid* grid,
                                       const NraysIrradianceVisibility* vis, float* out_rgb, float* out_sh, float* out_weight, uint32_t flags, void* hip_stream) {
    return irradiance_points_impl(sc, n, points, normals, hit_flags, grid, vis, true, out_rgb, out_sh, out_weight, flags, false, (hipStream_t)hip_stream);
}
int nrays_irradiance_points_vis(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const NraysIrradianceGrid* grid,
                                const NraysIrradianceVisibility* vis, float* out_rgb, float* out_sh, float* out_weight, uint32_t flags) {
    return irradiance_points_impl(sc, n, points, normals, hit_flags, grid, vis, true, out_rgb, out_sh, out_weight, flags, true, nullptr);
}

int nrays_probe_depth_points_device(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const uint64_t* keys,
                                    const NraysProbeDepthParams* params, float* out_moments, uint32_t* out_counts, double* out_nearest, uint32_t* out_nearest_dir,
                                    uint32_t flags, void* hip_stream) {
    return probe_depth_impl(sc, n, points, normals, hit_flags, keys, params, out_moments, out_counts, out_nearest, out_nearest_dir, flags, false, (hipStream_t)hip_stream);
}
int nrays_probe_depth_points(NraysScene* sc, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const uint64_t* keys,
                             const NraysProbeDepthParams* params, float* out_moments, uint32_t* out_counts, double* out_nearest, uint32_t* out_nearest_dir, uint32_t flags) {
    return probe_depth_impl(sc, n, points, normals, hit_flags, keys, params, out_moments, out_counts, out_nearest, out_nearest_dir, flags, true, nullptr);
}

int nrays_nearest_points_device(NraysScene* sc, uint32_t n, const double* points, const double* max_dist, const uint32_t* hit_flags, double* out_dist, int32_t* out_node,
                                double* out_point, double* out_normal, double* out_uv, int32_t* out_prim, uint32_t* out_flags, uint32_t flags, void* hip_stream) {
    return nearest_points_impl(sc, n, points, max_dist, hit_flags, out_dist, out_node, out_point, out_normal, out_uv, out_prim, out_flags, flags, false, (hipStream_t)hip_stream);
}
int nrays_nearest_points(NraysScene* sc, uint32_t n, const double* points, const double* max_dist, const uint32_t* hit_flags, double* out_dist, int32_t* out_node, double* out_point,
                         double* out_normal, double* out_uv, int32_t* out_prim, uint32_t* out_flags, uint32_t flags) {
    return nearest_points_impl(sc, n, points, max_dist, hit_flags, out_dist, out_node, out_point, out_normal, out_uv, out_prim, out_flags, flags, true, nullptr);
}
// nrays_debug_nearest_bound: nearest_box_bound alone, points x boxes, on host arrays, blocking (a test probe; no scene).
int nrays_debug_nearest_bound(uint32_t n, uint32_t boxes, const double* points, const double* box_bounds, double* out) {
    if (!points || !box_bounds || !out) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (n == 0 || boxes == 0) return NRAYS_OK;
    const size_t total = (size_t)n * boxes;
    double *d_p = nullptr, *d_b = nullptr, *d_o = nullptr;
    hipError_t e = hipMalloc((void**)&d_p, 24 * (size_t)n);
    if (e == hipSuccess) e = hipMalloc((void**)&d_b, 48 * (size_t)boxes);
    if (e == hipSuccess) e = hipMalloc((void**)&d_o, 8 * total);
    if (e == hipSuccess) e = hipMemcpy(d_p, points, 24 * (size_t)n, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_b, box_bounds, 48 * (size_t)boxes, hipMemcpyHostToDevice);
    if (e == hipSuccess) { launch_nearest_bound(launch_grid(total), (hipStream_t)0, n, boxes, d_p, d_b, d_o); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipMemcpy(out, d_o, 8 * total, hipMemcpyDeviceToHost);
    for (double* q : {d_p, d_b, d_o}) if (q) (void)hipFree(q);
    return e == hipSuccess ? NRAYS_OK : set_last_error(NRAYS_ERR_HIP, std::string("nrays_debug_nearest_bound: ") + hipGetErrorString(e));
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
        launch_gather_fold_sh(b.stream, (const float*)c[kGatherRays], n, chunk_points(c, 0ull), hemisphere_spec(params->num_dirs, params->num_rotations, params->bias),
                              (const double*)c[kPointDirs], (const double*)c[kPointRotations], bands, (float*)c[kGatherOut]);
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
