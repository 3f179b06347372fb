// texel_calls.hip — the caller-batch families over a lattice in a mesh node's uv space, each a check, a column table (batch_stage.h) and its passes run by the
// driver of batch_call.h as one chunk: nrays_surface_texels* (surface_texels_kernel.h) with its timing probe nrays_debug_surface_texels_passes,
// nrays_dilate_texels* (texel_dilate_kernel.h), nrays_filter_texels* (texel_filter_kernel.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/nrays_abi.h"
#include "batch_call.h"
#include "scene_handle.h"
#include "surface_texels_kernel.h"
#include "texel_dilate_kernel.h"
#include "texel_filter_kernel.h"

namespace nrays {

// ---- nrays_surface_texels*: the surface of a TriMesh node at the points of a lattice in uv space (surface_texels_kernel.h) -----------------------------------------
constexpr uint32_t kTexelMaxSide = 16384u, kTexelMaxPoints = 1u << 24;
static int check_texel_args(const NraysScene* sc, uint32_t node, uint32_t width, uint32_t height, const TexelOutputs* out /* null: the caller has none (the probe) */, uint32_t flags) {
    if (!sc || (out && (!out->points || !out->flags))) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (node >= sc->facts.host.surface.size()) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_surface_texels: no such node");
    if (width < 1u || width > kTexelMaxSide || height < 1u || height > kTexelMaxSide || (uint64_t)width * height > kTexelMaxPoints)
        return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_surface_texels: width and height must be in 1 .. 16384 and width * height <= 2^24");
    if (flags & ~(uint32_t)(NRAYS_TEXELS_CENTRES | NRAYS_TEXELS_FLIP_NORMALS)) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_surface_texels: unknown flag");
    const NodeSurface& s = sc->facts.host.surface[node];
    if (!s.mesh) return set_last_error(NRAYS_ERR_UNSUPPORTED, "nrays_surface_texels: the node is not a TriMesh");
    if (!s.has_uv) return set_last_error(NRAYS_ERR_UNSUPPORTED, "nrays_surface_texels: the node's mesh has no uvs");
    return NRAYS_OK;
}
static int texel_workspace(TraceWorkspace* w, size_t points, size_t records) {
    int rc = grow_device(&w->d_texel_owner, &w->texel_owner_words, points, sizeof(unsigned long long));
    if (rc == NRAYS_OK) rc = grow_device(&w->d_texel_off, &w->texel_off_words, std::max<size_t>(records, 1), sizeof(unsigned long long));
    if (rc != NRAYS_OK) return rc;
    if (!w->d_texel_blocks) HIP_TRY(hipMalloc((void**)&w->d_texel_blocks, (size_t)(kTexelMaxBlocks + 1u) * sizeof(unsigned long long)));
    return NRAYS_OK;
}
// The owner pass of one call: memset, count, scan, items.  Launches only; texel_workspace() has run.
static int texel_owner_pass(NraysScene* sc, TraceWorkspace* w, uint32_t node, uint32_t width, uint32_t height, uint32_t flags, hipStream_t stream) {
    const NodeSurface& s = sc->facts.host.surface[node];
    const TexelLattice L{width, height, (flags & NRAYS_TEXELS_CENTRES) ? 1u : 0u, node};
    unsigned long long* owner = (unsigned long long*)w->d_texel_owner; unsigned long long* off = (unsigned long long*)w->d_texel_off;
    HIP_TRY(hipMemsetAsync(owner, 0xff, (size_t)width * height * sizeof(unsigned long long), stream));
    if (s.count == 0u) return NRAYS_OK;
    if (s.count > kTexelMaxRecords) return set_last_error(NRAYS_ERR_UNSUPPORTED, "nrays_surface_texels: too many triangle records");
    const uint32_t rec_grid = (s.count + kTexelBlock - 1u) / kTexelBlock, scan_grid = (s.count + kTexelScanBlock - 1u) / kTexelScanBlock;
    unsigned long long* total = w->d_texel_blocks + kTexelMaxBlocks;
    hipLaunchKernelGGL(k_texel_count, dim3(rec_grid), dim3(kTexelBlock), 0, stream, sc->facts.d.tris, sc->facts.d.triuvs, s.first, s.count, L, off);
    hipLaunchKernelGGL(k_texel_sums, dim3(scan_grid), dim3(kTexelBlock), 0, stream, (const unsigned long long*)off, s.count, w->d_texel_blocks);
    hipLaunchKernelGGL(k_texel_scan, dim3(1), dim3(1024), 0, stream, w->d_texel_blocks, scan_grid, total);
    hipLaunchKernelGGL(k_texel_apply, dim3(scan_grid), dim3(kTexelBlock), 0, stream, off, s.count, (const unsigned long long*)w->d_texel_blocks);
    hipLaunchKernelGGL(k_texel_owner, dim3((uint32_t)sc->facts.num_cus * kTexelOwnerWgsPerCu), dim3(kTexelBlock), 0, stream, sc->facts.d.tris, sc->facts.d.triuvs, s.first, s.count, L,
                       (const unsigned long long*)off, (const unsigned long long*)total, owner);
    return launch_status("k_texel_owner");
}
static int texel_resolve_pass(NraysScene* sc, TraceWorkspace* w, uint32_t node, uint32_t width, uint32_t height, uint32_t flags, const TexelOutputs& out, hipStream_t stream) {
    const NodeSurface& s = sc->facts.host.surface[node];
    const TexelLattice L{width, height, (flags & NRAYS_TEXELS_CENTRES) ? 1u : 0u, node};
    TexelXform X;
    for (int k = 0; k < 9; ++k) X.m.r[k] = s.rot[k];
    X.m.t.x = s.trans[0]; X.m.t.y = s.trans[1]; X.m.t.z = s.trans[2];
    X.flags = s.flags; X.flip = (flags & NRAYS_TEXELS_FLIP_NORMALS) ? 1u : 0u;
    hipLaunchKernelGGL(k_texel_resolve, dim3((width * height + kTexelBlock - 1u) / kTexelBlock), dim3(kTexelBlock), 0, stream, sc->facts.d.tris, sc->facts.d.triuvs, L, X,
                       (const unsigned long long*)w->d_texel_owner, out);
    return launch_status("k_texel_resolve");
}

// The blocking forms and nrays_debug_surface_texels_passes stage every output of a lattice; the caller's absent ones are not read back.
static int ensure_texel_workspace(TraceWorkspace* w, const void* arg) { const size_t* a = (const size_t*)arg; return texel_workspace(w, a[0], a[1]); }
static int surface_texels_impl(NraysScene* sc, uint32_t node, uint32_t width, uint32_t height, const TexelOutputs& out, uint32_t flags, bool staged, hipStream_t stream) {
    { const int rc = check_texel_args(sc, node, width, height, &out, flags); if (rc != NRAYS_OK) return rc; }
    StageColumn cols[kTexelColumns];
    surface_texel_columns(cols, out.points, out.normals, out.uv, out.node, out.prim, out.flags);
    const size_t need[2] = {(size_t)width * height, sc->facts.host.surface[node].count};
    auto launch = [&](const BatchCall& b, uint32_t, void* const* c, unsigned long long) -> int {
        const TexelOutputs o{(double*)c[kTexelPoints], (double*)c[kTexelNormals], (double*)c[kTexelUv], (int32_t*)c[kTexelNode], (int32_t*)c[kTexelPrim], (uint32_t*)c[kTexelFlags]};
        const int rc = texel_owner_pass(sc, b.w, node, width, height, flags, b.stream);
        return rc != NRAYS_OK ? rc : texel_resolve_pass(sc, b.w, node, width, height, flags, o, b.stream);
    };
    return batch_run(sc, staged, stream, cols, kTexelColumns, width * height, width * height, "surface texels", launch, ensure_texel_workspace, need);
}

// nrays_debug_surface_texels_passes: the two passes of nrays_surface_texels_device between events of their own, `repeats` times, into the staging arena (a timing probe).
static int surface_texels_passes_probe(NraysScene* sc, uint32_t node, uint32_t width, uint32_t height, uint32_t flags, uint32_t repeats, float* out_ms) {
    { const int rc = check_texel_args(sc, node, width, height, nullptr, flags); if (rc != NRAYS_OK) return rc; }
    if (!out_ms || repeats == 0u) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    StageColumn cols[kTexelColumns];
    surface_texel_columns(cols, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr); // (nothing is read back: the layout alone)
    const size_t need[2] = {(size_t)width * height, sc->facts.host.surface[node].count};
    BatchCall b;
    int rc = batch_open(&b, sc, true, nullptr, cols, kTexelColumns, need[0], ensure_texel_workspace, need);
    if (rc != NRAYS_OK) return rc;
    char* base = (char*)b.w->d_stage;
    const TexelOutputs s{(double*)(base + b.off[kTexelPoints]), (double*)(base + b.off[kTexelNormals]), (double*)(base + b.off[kTexelUv]), (int32_t*)(base + b.off[kTexelNode]),
                         (int32_t*)(base + b.off[kTexelPrim]), (uint32_t*)(base + b.off[kTexelFlags])}; // (every output)
    const hipStream_t stream = b.stream;
    TraceWorkspace* w = b.w;
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    hipError_t e = hipSuccess;
    for (int k = 0; k < 3 && e == hipSuccess; ++k) e = hipEventCreate(&ev[k]);
    for (uint32_t r = 0; r < repeats && rc == NRAYS_OK && e == hipSuccess; ++r) {
        e = hipEventRecord(ev[0], stream);
        rc = texel_owner_pass(sc, w, node, width, height, flags, stream);
        if (e == hipSuccess) e = hipEventRecord(ev[1], stream);
        if (rc == NRAYS_OK) rc = texel_resolve_pass(sc, w, node, width, height, flags, s, stream);
        if (e == hipSuccess) e = hipEventRecord(ev[2], stream);
        if (e == hipSuccess) e = hipEventSynchronize(ev[2]);
        if (e == hipSuccess) e = hipEventElapsedTime(&out_ms[2 * r], ev[0], ev[1]);
        if (e == hipSuccess) e = hipEventElapsedTime(&out_ms[2 * r + 1], ev[1], ev[2]);
    }
    (void)hipStreamSynchronize(stream);
    for (int k = 0; k < 3; ++k) if (ev[k]) (void)hipEventDestroy(ev[k]);
    batch_close(b);
    if (rc == NRAYS_OK && e != hipSuccess) rc = set_last_error(NRAYS_ERR_HIP, std::string("nrays_debug_surface_texels_passes: ") + hipGetErrorString(e));
    return rc;
}

// ---- nrays_dilate_texels*: uncovered lattice points take the values of the nearest covered point within a radius (texel_dilate_kernel.h) -----------------------------
static_assert(kDilateMaxRadius == NRAYS_DILATE_MAX_RADIUS && kDilateFilled == NRAYS_TEXEL_FILLED, "texel_dilate_kernel.h restates the header's constants");
struct DilateArgs { uint32_t width, height; const uint32_t* flags_in; uint32_t radius, channels; float* values; int32_t* source; uint32_t* flags_out; };
static int check_dilate_args(const NraysScene* sc, const DilateArgs& a, uint32_t flags) {
    if (!sc || !a.flags_in) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (!a.values && !a.source && !a.flags_out) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_dilate_texels: no output (values, out_source and out_flags are all null)");
    if (a.values && (a.channels < 1u || a.channels > 4u)) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_dilate_texels: channels must be in 1 .. 4");
    if (a.radius < 1u || a.radius > NRAYS_DILATE_MAX_RADIUS) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_dilate_texels: radius must be in 1 .. 64");
    if (a.width < 1u || a.width > kTexelMaxSide || a.height < 1u || a.height > kTexelMaxSide || (uint64_t)a.width * a.height > kTexelMaxPoints)
        return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_dilate_texels: width and height must be in 1 .. 16384 and width * height <= 2^24");
    if (flags != 0u) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_dilate_texels: flags are reserved and must be 0");
    return NRAYS_OK;
}
// The two launches of one call.  The workspace holds width * height dx words.
static int dilate_passes(TraceWorkspace* w, const DilateArgs& a, hipStream_t stream) {
    const DilateLattice L{a.width, a.height, a.radius, (a.width + 63u) / 64u};
    int16_t* dx = (int16_t*)w->d_dilate_dx;
    const uint32_t T = a.radius <= kDilateShortRadius ? 16u : 64u; // (dilate_rows_per_group)
    const uint32_t vec4 = (a.values && a.channels == 4u && ((uintptr_t)a.values & 15u) == 0u) ? 1u : 0u;
    hipLaunchKernelGGL(k_dilate_rows, dim3((L.h * L.col_blocks + kDilateWaves - 1u) / kDilateWaves), dim3(kDilateBlock), 0, stream, L, a.flags_in, dx);
    hipLaunchKernelGGL(k_dilate_cols, dim3(L.col_blocks, (L.h + T - 1u) / T), dim3(kDilateBlock), (size_t)(T + 2u * a.radius) * 64u * sizeof(int16_t), stream, L,
                       (const int16_t*)dx, a.flags_in, a.values ? a.channels : 0u, vec4, a.values, a.source, a.flags_out);
    return launch_status("k_dilate_cols");
}
// Device form: flags_in and flags_out may be one array.  Blocking form: the arena holds them apart.
static int dilate_texels_impl(NraysScene* sc, const DilateArgs& a, uint32_t flags, bool staged, hipStream_t stream) {
    { const int rc = check_dilate_args(sc, a, flags); if (rc != NRAYS_OK) return rc; }
    StageColumn cols[kDilateColumns];
    dilate_columns(cols, a.flags_in, a.values, a.channels, a.source, a.flags_out);
    const size_t n = (size_t)a.width * a.height;
    auto launch = [&](const BatchCall& b, uint32_t, void* const* c, unsigned long long) -> int {
        DilateArgs s = a;
        s.flags_in = (const uint32_t*)c[kDilateFlagsIn]; s.values = (float*)c[kDilateValues]; s.source = (int32_t*)c[kDilateSource]; s.flags_out = (uint32_t*)c[kDilateFlagsOut];
        return dilate_passes(b.w, s, b.stream);
    };
    return batch_run(sc, staged, stream, cols, kDilateColumns, (uint32_t)n, (uint32_t)n, "dilate texels", launch,
                     [](TraceWorkspace* w, const void* points) { return grow_device(&w->d_dilate_dx, &w->dilate_points, *(const size_t*)points, sizeof(int16_t)); }, &n);
}

// ---- nrays_filter_texels*: one pass of the 5 x 5 a-trous joint-bilateral filter over a baked map (texel_filter_kernel.h) ---------------------------------------------
static_assert(kFilterMaxStep == NRAYS_FILTER_MAX_STEP, "texel_filter_kernel.h restates the header's constant");
struct FilterArgs { uint32_t width, height; const uint32_t* flags_in; const double* points; const double* normals; uint32_t channels; const float* values_in; float* values_out;
                    uint32_t step; double pos_radius, normal_cos; };
static int check_filter_args(const NraysScene* sc, const FilterArgs& a, uint32_t flags) {
    if (!sc || !a.flags_in || !a.points || !a.normals || !a.values_in || !a.values_out) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (a.values_out == a.values_in) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_filter_texels: values_out must not be values_in (a pass reads its neighbours' inputs)");
    if (a.channels < 1u || a.channels > 4u) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_filter_texels: channels must be in 1 .. 4");
    if (a.step < 1u || a.step > NRAYS_FILTER_MAX_STEP) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_filter_texels: step must be in 1 .. 64");
    if (a.width < 1u || a.width > kTexelMaxSide || a.height < 1u || a.height > kTexelMaxSide || (uint64_t)a.width * a.height > kTexelMaxPoints)
        return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_filter_texels: width and height must be in 1 .. 16384 and width * height <= 2^24");
    if (!(a.pos_radius > 0.0)) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_filter_texels: pos_radius must be > 0 (+inf: no position weight)");
    if (!(a.normal_cos >= -1.0 && a.normal_cos < 1.0)) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_filter_texels: normal_cos must be in [-1, 1)");
    if (flags != 0u) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_filter_texels: flags are reserved and must be 0");
    return NRAYS_OK;
}
// The one launch of a call: per axis ceil(ceil(side / step) / tile) blocks of each of the `step` residue classes.
static int filter_pass(const FilterArgs& a, hipStream_t stream) {
    const uint32_t sub_w = (a.width + a.step - 1u) / a.step, sub_h = (a.height + a.step - 1u) / a.step;
    const FilterLattice L{a.width, a.height, a.step, (sub_w + kFilterTileX - 1u) / kFilterTileX, (sub_h + kFilterTileY - 1u) / kFilterTileY,
                          a.pos_radius * a.pos_radius, a.normal_cos, 1.0 - a.normal_cos};
    const dim3 grid(L.tiles_x * a.step, L.tiles_y * a.step);
    const uint32_t vec4 = (a.channels == 4u && (((uintptr_t)a.values_in | (uintptr_t)a.values_out) & 15u) == 0u) ? 1u : 0u;
    switch (a.channels) {
    case 1u: hipLaunchKernelGGL(k_filter_texels<1>, grid, dim3(kFilterBlock), 0, stream, L, a.flags_in, a.points, a.normals, a.values_in, a.values_out, 0u); break;
    case 2u: hipLaunchKernelGGL(k_filter_texels<2>, grid, dim3(kFilterBlock), 0, stream, L, a.flags_in, a.points, a.normals, a.values_in, a.values_out, 0u); break;
    case 3u: hipLaunchKernelGGL(k_filter_texels<3>, grid, dim3(kFilterBlock), 0, stream, L, a.flags_in, a.points, a.normals, a.values_in, a.values_out, 0u); break;
    default: hipLaunchKernelGGL(k_filter_texels<4>, grid, dim3(kFilterBlock), 0, stream, L, a.flags_in, a.points, a.normals, a.values_in, a.values_out, vec4); break;
    }
    return launch_status("k_filter_texels");
}
static int filter_texels_impl(NraysScene* sc, const FilterArgs& a, uint32_t flags, bool staged, hipStream_t stream) {
    { const int rc = check_filter_args(sc, a, flags); if (rc != NRAYS_OK) return rc; }
    StageColumn cols[kFilterColumns];
    filter_columns(cols, a.points, a.normals, a.values_in, a.values_out, a.channels, a.flags_in);
    auto launch = [&](const BatchCall& b, uint32_t, void* const* c, unsigned long long) -> int {
        FilterArgs s = a;
        s.points = (const double*)c[kFilterPoints]; s.normals = (const double*)c[kFilterNormals]; s.values_in = (const float*)c[kFilterValuesIn];
        s.values_out = (float*)c[kFilterValuesOut]; s.flags_in = (const uint32_t*)c[kFilterFlags];
        return filter_pass(s, b.stream);
    };
    return batch_run(sc, staged, stream, cols, kFilterColumns, a.width * a.height, a.width * a.height, "filter texels", launch); // (the workspace: for the handle's stream ordering alone)
}

} // namespace nrays

using namespace nrays;

extern "C" {

int nrays_surface_texels_device(NraysScene* sc, uint32_t node, uint32_t width, uint32_t height, double* out_points, double* out_normals, double* out_uv, int32_t* out_node,
                                int32_t* out_prim, uint32_t* out_flags, uint32_t flags, void* hip_stream) {
    return surface_texels_impl(sc, node, width, height, TexelOutputs{out_points, out_normals, out_uv, out_node, out_prim, out_flags}, flags, false, (hipStream_t)hip_stream);
}
int nrays_surface_texels(NraysScene* sc, uint32_t node, uint32_t width, uint32_t height, double* out_points, double* out_normals, double* out_uv, int32_t* out_node,
                         int32_t* out_prim, uint32_t* out_flags, uint32_t flags) {
    return surface_texels_impl(sc, node, width, height, TexelOutputs{out_points, out_normals, out_uv, out_node, out_prim, out_flags}, flags, true, nullptr);
}
int nrays_debug_surface_texels_passes(NraysScene* sc, uint32_t node, uint32_t width, uint32_t height, uint32_t flags, uint32_t repeats, float* out_ms) {
    return surface_texels_passes_probe(sc, node, width, height, flags, repeats, out_ms);
}

int nrays_dilate_texels_device(NraysScene* sc, uint32_t width, uint32_t height, const uint32_t* flags_in, uint32_t radius, uint32_t channels, float* values, int32_t* out_source,
                               uint32_t* out_flags, uint32_t flags, void* hip_stream) {
    return dilate_texels_impl(sc, DilateArgs{width, height, flags_in, radius, channels, values, out_source, out_flags}, flags, false, (hipStream_t)hip_stream);
}
int nrays_dilate_texels(NraysScene* sc, uint32_t width, uint32_t height, const uint32_t* flags_in, uint32_t radius, uint32_t channels, float* values, int32_t* out_source,
                        uint32_t* out_flags, uint32_t flags) {
    return dilate_texels_impl(sc, DilateArgs{width, height, flags_in, radius, channels, values, out_source, out_flags}, flags, true, nullptr);
}

int nrays_filter_texels_device(NraysScene* sc, uint32_t width, uint32_t height, const uint32_t* flags_in, const double* points, const double* normals, uint32_t channels,
                               const float* values_in, float* values_out, uint32_t step, double pos_radius, double normal_cos, uint32_t flags, void* hip_stream) {
    return filter_texels_impl(sc, FilterArgs{width, height, flags_in, points, normals, channels, values_in, values_out, step, pos_radius, normal_cos}, flags, false, (hipStream_t)hip_stream);
}
int nrays_filter_texels(NraysScene* sc, uint32_t width, uint32_t height, const uint32_t* flags_in, const double* points, const double* normals, uint32_t channels,
                        const float* values_in, float* values_out, uint32_t step, double pos_radius, double normal_cos, uint32_t flags) {
    return filter_texels_impl(sc, FilterArgs{width, height, flags_in, points, normals, channels, values_in, values_out, step, pos_radius, normal_cos}, flags, true, nullptr);
}

} // extern "C"
