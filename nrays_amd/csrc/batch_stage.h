// batch_stage.h — how the arrays of a caller-batch call lie in the workspace's staging arena (TraceWorkspace::d_stage), and every family's table of them.
// A family describes its arrays as a fixed table of columns; stage_layout() is the ONE computation of where they lie and how many bytes they take, so a
// size cannot disagree with a layout.  batch_call.cpp turns the offsets into device pointers and copies; the families (ray_batches.hip, point_batches.hip,
// texel_calls.hip, the probes of ray_order.hip) only fill tables and read a chunk's pointers by the indices below.
// Needs <cstddef> and <cstdint> alone: the host compiler builds it for tests/test_batch_stage.py (tests/batch_stage_shim.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

namespace nrays {

constexpr int kStageMaxColumns = 32; // the widest table: nrays_gather_maps_sh_points with 16 maps (29 columns)
enum : uint8_t { kStageIn = 1, kStageOut = 2, kStageInOut = 3 };

// One array of a call.  `ptr`: the caller's array — host memory in the blocking form, device memory in the device form; null = absent (the kernel gets null).
// A column holds item_bytes for every item of a chunk, uploaded / read back per chunk and advanced by the chunk's first item; a table (`table` = 1) holds
// table_items items of the whole call, uploaded once.  `align`: of the column's start in the arena (16 for the value arrays the vec4 paths read).
struct StageColumn { void* ptr; size_t item_bytes; size_t table_items; uint8_t dir, align, table; };

inline StageColumn stage_in(const void* p, size_t item_bytes, uint8_t align = 8) { return StageColumn{const_cast<void*>(p), item_bytes, 0, kStageIn, align, 0}; }
inline StageColumn stage_out(void* p, size_t item_bytes, uint8_t align = 8) { return StageColumn{p, item_bytes, 0, kStageOut, align, 0}; }
inline StageColumn stage_inout(void* p, size_t item_bytes, uint8_t align = 8) { return StageColumn{p, item_bytes, 0, kStageInOut, align, 0}; }
inline StageColumn stage_table(const void* p, size_t item_bytes, size_t items, uint8_t align = 8) { return StageColumn{const_cast<void*>(p), item_bytes, items, kStageIn, align, 1}; }

inline size_t stage_column_bytes(const StageColumn& c, size_t cap) { return c.item_bytes * (c.table ? c.table_items : cap); }
// A column the blocking form copies and hands to the kernel: the caller gave it, and it holds something.
inline bool stage_present(const StageColumn& c) { return c.ptr && (!c.table || c.table_items); }

// Offsets of the columns in an arena whose chunks hold up to `cap` items, and the arena's bytes.  Every column has its slot, present or not: the layout of a
// family depends on its sizes alone.
inline size_t stage_layout(const StageColumn* cols, int ncols, size_t cap, size_t* off) {
    size_t at = 0;
    for (int k = 0; k < ncols; ++k) {
        const size_t a = cols[k].align;
        at = (at + a - 1) / a * a;
        off[k] = at;
        at += stage_column_bytes(cols[k], cap);
    }
    return at;
}

// Points per chunk of the families that build num_dirs rays a point on the device: at most `chunk_rays` rays a chunk.
inline uint32_t stage_point_chunk(uint32_t chunk_rays, uint32_t num_dirs) { const uint32_t c = chunk_rays / num_dirs; return c ? c : 1u; }

// ---- the families' tables.  Within a table the `in` columns are in upload order, the `out` columns in read-back order, the tables in upload order. ----
// Rays: origins and directions (nrays_debug_ray_order stages these two alone), then what each family adds.
enum { kRayO, kRayD, kRayColumns };
inline int ray_columns(StageColumn* c, const double* origins, const double* dirs) {
    c[kRayO] = stage_in(origins, 24); c[kRayD] = stage_in(dirs, 24);
    return kRayColumns;
}
enum { kTraceRefr = kRayColumns, kTraceKeys, kTraceEnergy, kTraceOut, kTraceColumns };
inline int trace_columns(StageColumn* c, const double* origins, const double* dirs, const double* refr, const uint64_t* keys, const float* energy, float* out_rgb) {
    ray_columns(c, origins, dirs);
    c[kTraceRefr] = stage_in(refr, 8); c[kTraceKeys] = stage_in(keys, 8); c[kTraceEnergy] = stage_in(energy, 4); c[kTraceOut] = stage_out(out_rgb, 12);
    return kTraceColumns;
}
enum { kIsectToi = kRayColumns, kIsectFilter, kIsectLit, kIsectColumns };
inline int intersects_columns(StageColumn* c, const double* origins, const double* dirs, const double* max_toi, float* out_filter, uint32_t* out_lit) {
    ray_columns(c, origins, dirs);
    c[kIsectToi] = stage_in(max_toi, 8); c[kIsectFilter] = stage_out(out_filter, 12); c[kIsectLit] = stage_out(out_lit, 4);
    return kIsectColumns;
}
enum { kCastMaxToi = kRayColumns, kCastToi, kCastNode, kCastNormal, kCastUv, kCastPrim, kCastFlags, kCastColumns };
inline int cast_columns(StageColumn* c, const double* origins, const double* dirs, const double* max_toi, double* toi, int32_t* node, double* normal, double* uv, int32_t* prim,
                        uint32_t* flags) {
    ray_columns(c, origins, dirs);
    c[kCastMaxToi] = stage_in(max_toi, 8);
    c[kCastToi] = stage_out(toi, 8); c[kCastNode] = stage_out(node, 4); c[kCastNormal] = stage_out(normal, 24); c[kCastUv] = stage_out(uv, 16);
    c[kCastPrim] = stage_out(prim, 4); c[kCastFlags] = stage_out(flags, 4);
    return kCastColumns;
}
// nrays_debug_cast_batch: max_toi is the shadow query's (mode 1; null otherwise); one record a ray, result_bytes = sizeof(NraysCastResult).
enum { kCastProbeMaxToi = kRayColumns, kCastProbeOut, kCastProbeColumns };
inline int cast_probe_columns(StageColumn* c, const double* origins, const double* dirs, const double* max_toi, void* out, size_t result_bytes) {
    ray_columns(c, origins, dirs);
    c[kCastProbeMaxToi] = stage_in(max_toi, 8); c[kCastProbeOut] = stage_out(out, result_bytes);
    return kCastProbeColumns;
}
enum { kShadePoints, kShadeNormals, kShadeViews, kShadeUvs, kShadeNodes, kShadeHit, kShadeKeys, kShadeOut, kShadeColumns };
inline int shade_columns(StageColumn* c, const double* points, const double* normals, const double* view_dirs, const double* uvs, const int32_t* nodes, const uint32_t* hit_flags,
                         const uint64_t* keys, float* out_rgba) {
    c[kShadePoints] = stage_in(points, 24); c[kShadeNormals] = stage_in(normals, 24); c[kShadeViews] = stage_in(view_dirs, 24); c[kShadeUvs] = stage_in(uvs, 16);
    c[kShadeNodes] = stage_in(nodes, 4); c[kShadeHit] = stage_in(hit_flags, 4); c[kShadeKeys] = stage_in(keys, 8); c[kShadeOut] = stage_out(out_rgba, 16);
    return kShadeColumns;
}
// nrays_material_points*: the terms of the points' materials.  Every column but the nodes may be absent; ambient and specular are stored as one 16-byte vector.
enum { kMatNormals, kMatUvs, kMatNodes, kMatHit, kMatAmbient, kMatDiffuse, kMatSpecular, kMatNode, kMatColumns };
inline int material_columns(StageColumn* c, const double* normals, const double* uvs, const int32_t* nodes, const uint32_t* hit_flags, float* out_ambient, float* out_diffuse,
                            float* out_specular, double* out_node) {
    c[kMatNormals] = stage_in(normals, 24); c[kMatUvs] = stage_in(uvs, 16); c[kMatNodes] = stage_in(nodes, 4); c[kMatHit] = stage_in(hit_flags, 4);
    c[kMatAmbient] = stage_out(out_ambient, 16, 16); c[kMatDiffuse] = stage_out(out_diffuse, 12); c[kMatSpecular] = stage_out(out_specular, 16, 16);
    c[kMatNode] = stage_out(out_node, 32, 16);
    return kMatColumns;
}
// nrays_nearest_points*: points in, the nearest-surface record out; every output but the distance and the node may be absent.
enum { kNearPoints, kNearMaxDist, kNearHit, kNearDist, kNearNode, kNearPoint, kNearNormal, kNearUv, kNearPrim, kNearFlags, kNearColumns };
inline int nearest_columns(StageColumn* c, const double* points, const double* max_dist, const uint32_t* hit_flags, double* dist, int32_t* node, double* point, double* normal, double* uv,
                           int32_t* prim, uint32_t* flags) {
    c[kNearPoints] = stage_in(points, 24); c[kNearMaxDist] = stage_in(max_dist, 8); c[kNearHit] = stage_in(hit_flags, 4);
    c[kNearDist] = stage_out(dist, 8); c[kNearNode] = stage_out(node, 4); c[kNearPoint] = stage_out(point, 24); c[kNearNormal] = stage_out(normal, 24); c[kNearUv] = stage_out(uv, 16);
    c[kNearPrim] = stage_out(prim, 4); c[kNearFlags] = stage_out(flags, 4);
    return kNearColumns;
}
// Points with a hemisphere of directions: the two tables and the points (nrays_debug_gather_order stages these alone), then what each family adds.
enum { kPointDirs, kPointRotations, kPointPoints, kPointNormals, kPointHit, kPointKeys, kPointColumns };
inline int point_columns(StageColumn* c, const double* dirs, uint32_t num_dirs, const double* rotations, uint32_t num_rotations, const double* points, const double* normals,
                         const uint32_t* hit_flags, const uint64_t* keys) {
    c[kPointDirs] = stage_table(dirs, 24, num_dirs); c[kPointRotations] = stage_table(rotations, 16, num_rotations);
    c[kPointPoints] = stage_in(points, 24); c[kPointNormals] = stage_in(normals, 24); c[kPointHit] = stage_in(hit_flags, 4); c[kPointKeys] = stage_in(keys, 8);
    return kPointColumns;
}
enum { kOccFilter = kPointColumns, kOccOpen, kOccColumns };
inline int occlusion_columns(StageColumn* c, float* out_filter, uint32_t* out_open) { // (after point_columns)
    c[kOccFilter] = stage_out(out_filter, 12); c[kOccOpen] = stage_out(out_open, 4);
    return kOccColumns;
}
// nrays_debug_occlusion_rays: the num_dirs rays of a point, origins and directions.
enum { kOccRaysOrigins = kPointColumns, kOccRaysDirs, kOccRaysColumns };
inline int occlusion_rays_columns(StageColumn* c, double* out_origins, double* out_dirs, uint32_t num_dirs) { // (after point_columns)
    c[kOccRaysOrigins] = stage_out(out_origins, 24 * (size_t)num_dirs); c[kOccRaysDirs] = stage_out(out_dirs, 24 * (size_t)num_dirs);
    return kOccRaysColumns;
}
// out_floats: 3 (nrays_gather_points*) or 3 * bands^2 (nrays_gather_sh_points*).  ray_colours: nrays_debug_gather_sh_fold's input, 3 floats a ray; null elsewhere.
enum { kGatherOut = kPointColumns, kGatherRays, kGatherColumns };
inline int gather_columns(StageColumn* c, float* out, uint32_t out_floats, const float* ray_colours, uint32_t num_dirs) { // (after point_columns)
    c[kGatherOut] = stage_out(out, 4 * (size_t)out_floats); c[kGatherRays] = stage_in(ray_colours, ray_colours ? 12 * (size_t)num_dirs : 0);
    return kGatherColumns;
}
// map_texels[m], map_count[m]: the RGBA32F texels of map m and their number; column kMapsTexels + m.
enum { kMapsRgb = kPointColumns, kMapsCounts, kMapsNodeMap, kMapsTexels };
inline int gather_maps_columns(StageColumn* c, float* out_rgb, uint32_t* out_counts, const int32_t* node_map, uint32_t num_nodes, uint32_t num_maps, const void* const* map_texels,
                               const size_t* map_count) { // (after point_columns)
    c[kMapsRgb] = stage_out(out_rgb, 12); c[kMapsCounts] = stage_out(out_counts, 8); c[kMapsNodeMap] = stage_table(node_map, 4, num_nodes);
    for (uint32_t m = 0; m < num_maps; ++m) c[kMapsTexels + m] = stage_table(map_texels[m], 16, map_count[m], 16);
    return kMapsTexels + (int)num_maps;
}
// nrays_probe_depth_points*: per point res^2 texels of two moments, two counts, the nearest distance and its direction's index.
enum { kDepthMoments = kPointColumns, kDepthCounts, kDepthNearest, kDepthNearestDir, kDepthColumns };
inline int probe_depth_columns(StageColumn* c, float* out_moments, uint32_t res, uint32_t* out_counts, double* out_nearest, uint32_t* out_nearest_dir) { // (after point_columns)
    c[kDepthMoments] = stage_out(out_moments, 8 * (size_t)res * res); c[kDepthCounts] = stage_out(out_counts, 8);
    c[kDepthNearest] = stage_out(out_nearest, 8); c[kDepthNearestDir] = stage_out(out_nearest_dir, 4);
    return kDepthColumns;
}
// nrays_gather_maps_sh_points*: the outputs of a probe filled from maps — 3 * coefs floats of SH and the two counts of nrays_gather_maps_points*, then the four outputs of
// nrays_probe_depth_points* (absent without a depth spec: res = 0) — and the tables of gather_maps_columns; column kMapsShTexels + m holds map m.
enum { kMapsShSh = kPointColumns, kMapsShCounts, kMapsShMoments, kMapsShDepthCounts, kMapsShNearest, kMapsShNearestDir, kMapsShNodeMap, kMapsShTexels };
inline int gather_maps_sh_columns(StageColumn* c, float* out_sh, uint32_t coefs, uint32_t* out_counts, float* out_moments, uint32_t res, uint32_t* out_depth_counts, double* out_nearest,
                                  uint32_t* out_nearest_dir, const int32_t* node_map, uint32_t num_nodes, uint32_t num_maps, const void* const* map_texels,
                                  const size_t* map_count) { // (after point_columns)
    c[kMapsShSh] = stage_out(out_sh, 12 * (size_t)coefs); c[kMapsShCounts] = stage_out(out_counts, 8);
    c[kMapsShMoments] = stage_out(out_moments, 8 * (size_t)res * res); c[kMapsShDepthCounts] = stage_out(out_depth_counts, 8);
    c[kMapsShNearest] = stage_out(out_nearest, 8); c[kMapsShNearestDir] = stage_out(out_nearest_dir, 4);
    c[kMapsShNodeMap] = stage_table(node_map, 4, num_nodes);
    for (uint32_t m = 0; m < num_maps; ++m) c[kMapsShTexels + m] = stage_table(map_texels[m], 16, map_count[m], 16);
    return kMapsShTexels + (int)num_maps;
}
static_assert(kMapsShTexels + 16 <= kStageMaxColumns, "the widest table fits");
// nrays_irradiance_points*: points against a grid of SH probes.  The grid's coefficients (12 C bytes a probe) and validity words are tables; out_sh holds 3 C floats a point.
enum { kIrrSh, kIrrValid, kIrrPoints, kIrrNormals, kIrrHit, kIrrRgb, kIrrOutSh, kIrrWeight, kIrrColumns };
inline int irradiance_columns(StageColumn* c, const float* grid_sh, const uint32_t* grid_valid, size_t probes, uint32_t coefs, const double* points, const double* normals,
                              const uint32_t* hit_flags, float* out_rgb, float* out_sh, float* out_weight) {
    c[kIrrSh] = stage_table(grid_sh, 12 * (size_t)coefs, probes); c[kIrrValid] = stage_table(grid_valid, 4, probes);
    c[kIrrPoints] = stage_in(points, 24); c[kIrrNormals] = stage_in(normals, 24); c[kIrrHit] = stage_in(hit_flags, 4);
    c[kIrrRgb] = stage_out(out_rgb, 12); c[kIrrOutSh] = stage_out(out_sh, 12 * (size_t)coefs); c[kIrrWeight] = stage_out(out_weight, 4);
    return kIrrColumns;
}
// nrays_irradiance_points_vis*: the probes' depth moments (8 res^2 bytes a probe) are one more table, staged with the grid.
enum { kIrrMoments = kIrrColumns, kIrrVisColumns };
inline int irradiance_vis_columns(StageColumn* c, const float* moments, size_t probes, uint32_t res) { // (after irradiance_columns)
    c[kIrrMoments] = stage_table(moments, 8 * (size_t)res * res, probes);
    return kIrrVisColumns;
}
// nrays_light_points*: points against a table of point lights.  The lights' positions, colours and emitter normals (absent: the lights shine every way) are tables;
// hit_flags and out_counts may be absent.
enum { kLightPositions, kLightColors, kLightNormals, kLightPoints, kLightPointNormals, kLightHit, kLightRgb, kLightCounts, kLightColumns };
inline int light_columns(StageColumn* c, const double* positions, const float* colors, const double* light_normals, uint32_t num_lights, const double* points, const double* normals,
                         const uint32_t* hit_flags, float* out_rgb, uint32_t* out_counts) {
    c[kLightPositions] = stage_table(positions, 24, num_lights); c[kLightColors] = stage_table(colors, 12, num_lights); c[kLightNormals] = stage_table(light_normals, 24, num_lights);
    c[kLightPoints] = stage_in(points, 24); c[kLightPointNormals] = stage_in(normals, 24); c[kLightHit] = stage_in(hit_flags, 4);
    c[kLightRgb] = stage_out(out_rgb, 12); c[kLightCounts] = stage_out(out_counts, 8);
    return kLightColumns;
}
// nrays_debug_light_rays: the num_lights rays of a point — origins, directions, t_max and weights — after the tables and the points of light_columns.
enum { kLightRaysOrigins = kLightRgb, kLightRaysDirs, kLightRaysTmax, kLightRaysW, kLightRaysColumns };
inline int light_rays_columns(StageColumn* c, double* out_origins, double* out_dirs, double* out_tmax, float* out_w, uint32_t num_lights) { // (after light_columns)
    c[kLightRaysOrigins] = stage_out(out_origins, 24 * (size_t)num_lights); c[kLightRaysDirs] = stage_out(out_dirs, 24 * (size_t)num_lights);
    c[kLightRaysTmax] = stage_out(out_tmax, 8 * (size_t)num_lights); c[kLightRaysW] = stage_out(out_w, 4 * (size_t)num_lights);
    return kLightRaysColumns;
}
// Lattices (one chunk of width * height items).
enum { kTexelPoints, kTexelNormals, kTexelUv, kTexelNode, kTexelPrim, kTexelFlags, kTexelColumns };
inline int surface_texel_columns(StageColumn* c, double* points, double* normals, double* uv, int32_t* node, int32_t* prim, uint32_t* flags) {
    c[kTexelPoints] = stage_out(points, 24); c[kTexelNormals] = stage_out(normals, 24); c[kTexelUv] = stage_out(uv, 16);
    c[kTexelNode] = stage_out(node, 4); c[kTexelPrim] = stage_out(prim, 4); c[kTexelFlags] = stage_out(flags, 4);
    return kTexelColumns;
}
enum { kDilateFlagsIn, kDilateValues, kDilateSource, kDilateFlagsOut, kDilateColumns };
inline int dilate_columns(StageColumn* c, const uint32_t* flags_in, float* values, uint32_t channels, int32_t* source, uint32_t* flags_out) {
    c[kDilateFlagsIn] = stage_in(flags_in, 4); c[kDilateValues] = stage_inout(values, values ? 4 * (size_t)channels : 0, 16);
    c[kDilateSource] = stage_out(source, 4); c[kDilateFlagsOut] = stage_out(flags_out, 4);
    return kDilateColumns;
}
enum { kFilterPoints, kFilterNormals, kFilterValuesIn, kFilterValuesOut, kFilterFlags, kFilterColumns };
inline int filter_columns(StageColumn* c, const double* points, const double* normals, const float* values_in, float* values_out, uint32_t channels, const uint32_t* flags_in) {
    c[kFilterPoints] = stage_in(points, 24); c[kFilterNormals] = stage_in(normals, 24);
    c[kFilterValuesIn] = stage_in(values_in, 4 * (size_t)channels, 16); c[kFilterValuesOut] = stage_out(values_out, 4 * (size_t)channels, 16);
    c[kFilterFlags] = stage_in(flags_in, 4);
    return kFilterColumns;
}

} // namespace nrays
