// ray_batches.hip — the caller-batch families that take rays or surface points as arrays, each a check, a column table (batch_stage.h) and a chunk launch run by
// the driver of batch_call.h: nrays_trace_rays* (+ _ex), nrays_intersects_rays_device (+ _ex), nrays_cast_rays*, nrays_shade_points*, nrays_material_points*
// (k_material_points of material_points_kernel.h); their kernels are the templates of ray_batch_kernel.h, instantiated here, as is k_occlusion_points for point_batches.hip (launch_occlusion_points).  Also two probes with kernels of their own:
// nrays_debug_cast_batch (k_cast_batch; through the driver) and nrays_debug_box_cull (k_box_cull; no scene handle, buffers of its own).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <new>
#include <string>
#include <vector>

#include "../../include/nrays_abi.h"
#include "batch_call.h"
#include "bounce.h"
#include "material_points_kernel.h"
#include "ray_batch_kernel.h"
#include "scene_handle.h"

namespace nrays {

// (FEAT: kFeatAll, or kFeatMesh for scenes of opaque TriMesh nodes only — the permutation whose node phases end by quorum in
// hair-like meshes, so that the independent fixtures also cover that path.)
// nrays_debug_cast_batch: the closest-hit query with the deferred exact gates exactly as shade_hit runs it (closest_hit, trace_device.h: ungated traversal, the
// winner checked against the reference's AABB gates, fully gated repeat for knife-edge rays), or the shadow query, on rays from memory.
template <int FEAT>
__global__ void __launch_bounds__(kBlock, NRAYS_WAVES_PER_SIMD) k_cast_batch(DScene S, uint32_t mode, uint32_t n, const double* __restrict__ ro, const double* __restrict__ rd,
                                                                              const double* __restrict__ max_toi, NraysCastResult* __restrict__ out, uint32_t* spill) {
    __shared__ uint32_t lds_stack[kLdsStack * kBlock];
    Stack st; st.setup(lds_stack, spill, nullptr);
    Cnt cnt; cnt.zero();
    for (uint32_t base = blockIdx.x * kBlock; base < n; base += gridDim.x * kBlock) {
        const uint32_t i = base + threadIdx.x;
        if (i >= n) continue;
        const d3 o = D3(ro[3 * (size_t)i], ro[3 * (size_t)i + 1], ro[3 * (size_t)i + 2]), d = D3(rd[3 * (size_t)i], rd[3 * (size_t)i + 1], rd[3 * (size_t)i + 2]);
        NraysCastResult r; r.toi = 0.0; r.normal[0] = r.normal[1] = r.normal[2] = 0.0; r.uv[0] = r.uv[1] = 0.0; r.node_id = -1; r.flags = 0u;
        Hit hit; f3 filter = F3(1.0f, 1.0f, 1.0f);
        if (mode == 1u) {
            const bool blocked = traverse<true, false, FEAT>(S, st, o, d, max_toi[i], hit, filter, cnt);
            r.flags = blocked ? 1u : 0u; r.normal[0] = filter.x; r.normal[1] = filter.y; r.normal[2] = filter.z;
        } else {
            Isect is; uint32_t node_id = 0; bool gated = false, any = false;
            for (;;) { // (closest_hit, kept as text: through the call this kernel compiles to other instructions)
                any = traverse<false, false, FEAT>(S, st, o, d, kDblMax, hit, filter, cnt, gated, &is);
                if (!any) break;
                if (resolve_hit<false, FEAT, true>(S, o, d, hit, is, node_id) || gated) break;
                gated = true;
            }
            if (any) {
                r.toi = hit.t; r.normal[0] = is.n.x; r.normal[1] = is.n.y; r.normal[2] = is.n.z; r.uv[0] = is.u; r.uv[1] = is.v;
                r.node_id = (int32_t)node_id; r.flags = 1u | (is.has_uv ? 2u : 0u);
            }
        }
        out[i] = r;
    }
}

// nrays_debug_box_cull: ONE node visit of the traversals on a case from memory — make_rayf, best_f32, the fetch of the node's planes, box_keys4 and,
// for a ray with an f32-zero component, zero_axis_cull: the product functions themselves, in the order traverse() calls them.  Case i reads node i.
// uniform = 0: a case per lane, planes through load_planes.  uniform = 1: a case per WAVE (all its lanes compute the same case, so that they share
// the node and the direction signs as load_planes_uniform requires; the first lane writes), planes through the scalar fetch.
__global__ void __launch_bounds__(kBlock) k_box_cull(const BvhNode* __restrict__ nodes, uint32_t uniform, uint32_t n, const double* __restrict__ ro, const double* __restrict__ rd,
                                                     const double* __restrict__ best, float* __restrict__ keys, uint32_t* __restrict__ bits, float* __restrict__ inv32) {
    const uint32_t tid = blockIdx.x * kBlock + threadIdx.x, threads = gridDim.x * kBlock;
    const uint32_t step = uniform ? threads >> 6 : threads;
    for (uint32_t i = uniform ? tid >> 6 : tid; i < n; i += step) {
        const d3 o = D3(ro[3 * (size_t)i], ro[3 * (size_t)i + 1], ro[3 * (size_t)i + 2]), d = D3(rd[3 * (size_t)i], rd[3 * (size_t)i + 1], rd[3 * (size_t)i + 2]);
        const RayF rf = make_rayf(o, d);
        const float btf = best_f32(best[i]);
        float k0, k1, k2, k3;
        if (uniform) {
            const uint32_t ukey = (uint32_t)__builtin_amdgcn_readfirstlane((int)((i << 7) | rf.bits));
            const NodePlanes np = load_planes_uniform(nodes, ukey);
            box_keys4(np, rf, btf, k0, k1, k2, k3);
            if ((rf.bits & 7u)) zero_axis_cull((rf.bits & 7u), o, np, k0, k1, k2, k3);
        } else {
            const NodePlanes np = load_planes(nodes, (int32_t)i, rf);
            box_keys4(np, rf, btf, k0, k1, k2, k3);
            if ((rf.bits & 7u)) zero_axis_cull((rf.bits & 7u), o, np, k0, k1, k2, k3);
        }
        if (uniform && (threadIdx.x & 63u)) continue;
        keys[4 * (size_t)i] = k0; keys[4 * (size_t)i + 1] = k1; keys[4 * (size_t)i + 2] = k2; keys[4 * (size_t)i + 3] = k3;
        bits[i] = rf.bits;
        inv32[3 * (size_t)i] = rf.ix; inv32[3 * (size_t)i + 1] = rf.iy; inv32[3 * (size_t)i + 2] = rf.iz;
    }
}

uint32_t launch_grid(uint64_t items) { return (uint32_t)std::min<uint64_t>((items + kBlock - 1) / kBlock, (uint64_t)kMaxGrid); }

// ---- the launches of this unit's kernels (batch_call.h: the idiom).  `order` non-null selects the ordered form of a kernel: lane j serves ray order[j]. ------------------------
struct TraceLaunch {
    uint32_t grid; hipStream_t stream; const DScene* d; uint32_t n; const uint32_t* order; const double* o; const double* dir; const double* refr; const float* energy;
    const unsigned long long* keys; unsigned long long key_base; uint32_t keyed, max_depth; float* out; const QueueOut* qo; DeviceCounters* ctr; uint32_t* spill;
};
template <bool STATS, int FEAT, bool ORDERED>
static bool launch_if(const TraceLaunch& a, bool stats, int feat) {
    if (stats != STATS || feat != FEAT || (a.order != nullptr) != ORDERED) return false;
    if constexpr (ORDERED) hipLaunchKernelGGL((k_trace_rays_ordered<STATS, FEAT>), dim3(a.grid), dim3(kBlock), 0, a.stream, *a.d, a.n, a.order, a.o, a.dir, a.refr, a.energy, a.keys, a.key_base,
                                              a.keyed, a.max_depth, a.out, *a.qo, a.ctr, a.spill);
    else hipLaunchKernelGGL((k_trace_rays<STATS, FEAT>), dim3(a.grid), dim3(kBlock), 0, a.stream, *a.d, a.n, a.o, a.dir, a.refr, a.energy, a.keys, a.key_base, a.keyed, a.max_depth, a.out,
                            *a.qo, a.ctr, a.spill);
    return true;
}
static bool launch_trace_rays(const TraceLaunch& a, bool stats, int feat) {
    return launch_if<false, kFeatAll, false>(a, stats, feat) || launch_if<false, kFeatAll, true>(a, stats, feat) || launch_if<false, kFeatMesh, false>(a, stats, feat) ||
           launch_if<false, kFeatMesh, true>(a, stats, feat) || launch_if<true, kFeatAll, false>(a, stats, feat) || launch_if<true, kFeatAll, true>(a, stats, feat);
}
struct IntersectsLaunch {
    uint32_t grid; hipStream_t stream; const DScene* d; uint32_t n; const uint32_t* order; const double* o; const double* dir; const double* max_toi; float* out_filter; uint32_t* out_lit;
    uint32_t* spill;
};
template <int FEAT, bool ORDERED>
static bool launch_if(const IntersectsLaunch& a, int feat) {
    if (feat != FEAT || (a.order != nullptr) != ORDERED) return false;
    if constexpr (ORDERED) hipLaunchKernelGGL((k_intersects_rays_ordered<FEAT>), dim3(a.grid), dim3(kBlock), 0, a.stream, *a.d, a.n, a.order, a.o, a.dir, a.max_toi, a.out_filter, a.out_lit, a.spill);
    else hipLaunchKernelGGL((k_intersects_rays<FEAT>), dim3(a.grid), dim3(kBlock), 0, a.stream, *a.d, a.n, a.o, a.dir, a.max_toi, a.out_filter, a.out_lit, a.spill);
    return true;
}
static bool launch_intersects_rays(const IntersectsLaunch& a, int feat) {
    return launch_if<kFeatAll, false>(a, feat) || launch_if<kFeatAll, true>(a, feat) || launch_if<kFeatMesh, false>(a, feat) || launch_if<kFeatMesh, true>(a, feat);
}
struct CastLaunch {
    uint32_t grid; hipStream_t stream; const DScene* d; uint32_t n; const uint32_t* order; const double* o; const double* dir; const double* max_toi; double* toi; int32_t* node;
    double* normal; double* uv; int32_t* prim; uint32_t* flags; uint32_t* spill;
};
template <int FEAT, bool ORDERED>
static bool launch_if(const CastLaunch& a, int feat) {
    if (feat != FEAT || (a.order != nullptr) != ORDERED) return false;
    if constexpr (ORDERED) hipLaunchKernelGGL((k_cast_rays_ordered<FEAT>), dim3(a.grid), dim3(kBlock), 0, a.stream, *a.d, a.n, a.order, a.o, a.dir, a.max_toi, a.toi, a.node, a.normal, a.uv, a.prim,
                                              a.flags, a.spill);
    else hipLaunchKernelGGL((k_cast_rays<FEAT>), dim3(a.grid), dim3(kBlock), 0, a.stream, *a.d, a.n, a.o, a.dir, a.max_toi, a.toi, a.node, a.normal, a.uv, a.prim, a.flags, a.spill);
    return true;
}
static bool launch_cast_rays(const CastLaunch& a, int feat) {
    return launch_if<kFeatAll, false>(a, feat) || launch_if<kFeatAll, true>(a, feat) || launch_if<kFeatMesh, false>(a, feat) || launch_if<kFeatMesh, true>(a, feat);
}
// (kFeatAll is right for every scene: it holds kFeatMultiSample, and the shadow rays are traced inside the light loop)
struct ShadeLaunch {
    uint32_t grid; hipStream_t stream; const DScene* d; uint32_t n, num_nodes; const double* points; const double* normals; const double* view_dirs; const double* uvs; const int32_t* nodes;
    const uint32_t* hit_flags; const unsigned long long* keys; unsigned long long key_base; float* out; DeviceCounters* ctr; uint32_t* spill;
};
template <bool STATS>
static bool launch_if(const ShadeLaunch& a, bool stats) {
    if (stats != STATS) return false;
    hipLaunchKernelGGL((k_shade_points<STATS, kFeatAll>), dim3(a.grid), dim3(kBlock), 0, a.stream, *a.d, a.n, a.num_nodes, a.points, a.normals, a.view_dirs, a.uvs, a.nodes, a.hit_flags, a.keys,
                       a.key_base, a.out, a.ctr, a.spill);
    return true;
}
static bool launch_shade_points(const ShadeLaunch& a, bool stats) { return launch_if<false>(a, stats) || launch_if<true>(a, stats); }
// (one form: which outputs are stored is a null test in the kernel, uniform over the grid)
void launch_material_points(const MaterialLaunch& a) {
    hipLaunchKernelGGL(k_material_points, dim3(a.grid), dim3(kBlock), 0, a.stream, a.shade, a.n, a.num_nodes, a.normals, a.uvs, a.nodes, a.hit_flags, a.out_ambient, a.out_diffuse,
                       a.out_specular, a.out_node);
}
// k_occlusion_points (nrays_occlusion_points*, point_batches.hip) is instantiated in this unit, beside the other traversal kernels: in a unit without them the compiler
// allocates and schedules its LP = 3 and 6 forms differently (profiles/README.md, batch_driver_kres_*).  feat: kFeatMesh or kFeatAll; lp: 0, 3 or 6.
template <int FEAT, int LP>
static bool launch_if(const OcclusionLaunch& a, int feat, int lp) {
    if (feat != FEAT || lp != LP) return false;
    hipLaunchKernelGGL((k_occlusion_points<FEAT, LP>), dim3(a.grid), dim3(kBlock), 0, a.stream, *a.d, a.n, a.in.points, a.in.normals, a.in.hit_flags, a.in.keys, a.in.key_base, a.spec, a.dirs,
                       a.rotations, a.out_filter, a.out_open, a.spill);
    return true;
}
bool launch_occlusion_points(const OcclusionLaunch& a, int feat, int lp) {
    return launch_if<kFeatAll, 0>(a, feat, lp) || launch_if<kFeatAll, 3>(a, feat, lp) || launch_if<kFeatAll, 6>(a, feat, lp) || launch_if<kFeatMesh, 0>(a, feat, lp) ||
           launch_if<kFeatMesh, 3>(a, feat, lp) || launch_if<kFeatMesh, 6>(a, feat, lp);
}
struct CastBatchLaunch { uint32_t grid; hipStream_t stream; const DScene* d; uint32_t mode, n; const double* o; const double* dir; const double* max_toi; NraysCastResult* out; uint32_t* spill; };
template <int FEAT>
static bool launch_if(const CastBatchLaunch& a, int feat) {
    if (feat != FEAT) return false;
    hipLaunchKernelGGL((k_cast_batch<FEAT>), dim3(a.grid), dim3(kBlock), 0, a.stream, *a.d, a.mode, a.n, a.o, a.dir, a.max_toi, a.out, a.spill);
    return true;
}
static bool launch_cast_batch(const CastBatchLaunch& a, int feat) { return launch_if<kFeatAll>(a, feat) || launch_if<kFeatMesh>(a, feat); }

// ---- nrays_trace_rays*: Scene::trace on caller-supplied rays (scene.rs:147-193) ----------------------------------------------------------------------
// One chunk (nc <= kTraceChunk): the reorder when it is due, k_trace_rays or its ordered form, then — double-branching scenes only — the k_bounce rounds of the queued
// second children and k_fold_fixed, as a frame runs them for a sample batch (bounce.h).  The permutation: a scene with a non-finite light / colour / texel gets the
// kernel that skips nothing, as its renders (its counters go to the batch's own block); kFeatMesh for scenes of opaque meshes, kFeatAll otherwise.
static int trace_rays_impl(NraysScene* sc, uint32_t n, const double* o, const double* d, const double* refr, const float* energy, const uint64_t* keys, uint32_t max_depth,
                           float* out, uint32_t flags, bool staged, hipStream_t stream) {
    if (!sc || !o || !d || !out) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (check_ray_flags(flags) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    if (n == 0) return NRAYS_OK;
    StageColumn cols[kTraceColumns];
    trace_columns(cols, o, d, refr, keys, energy, out);
    const bool reorder = (flags & NRAYS_RAYS_UNORDERED) && reorder_pays(sc, n), stats = sc->facts.d.no_elide != 0u;
    auto launch = [&](const BatchCall& b, uint32_t nc, void* const* c, unsigned long long key_base) -> int {
        const double *co = (const double*)c[kRayO], *cd = (const double*)c[kRayD];
        const uint32_t* order = nullptr;
        QueueOut qo;
        int rc = chunk_order(sc, b.w, reorder, nc, co, cd, b.stream, &order);
        if (rc == NRAYS_OK) rc = queued_trace_begin(sc, b.w, nc, b.stream, &qo);
        if (rc != NRAYS_OK) return rc;
        const TraceLaunch a{launch_grid(nc), b.stream, &sc->facts.d, nc, order, co, cd, (const double*)c[kTraceRefr], (const float*)c[kTraceEnergy], (const unsigned long long*)c[kTraceKeys],
                            key_base, sc->facts.host.any_area_light ? 1u : 0u, max_depth, (float*)c[kTraceOut], &qo, b.w->d_counters, b.w->d_spill};
        if (!launch_trace_rays(a, stats, stats ? (int)kFeatAll : shading_feat(sc))) return no_permutation("k_trace_rays");
        HIP_TRY(hipGetLastError());
        return sc->facts.host.any_double_branch ? queued_trace_finish(sc, b.w, nc, max_depth, a.out, "traced", b.stream) : (int)NRAYS_OK;
    };
    return batch_run(sc, staged, stream, cols, kTraceColumns, n, kTraceChunk, "trace batch", launch);
}

// ---- nrays_intersects_rays_device*: Scene::intersects_ray (device form only) -----------------------------------------------------------------------------
static int intersects_rays_impl(NraysScene* sc, uint32_t n, const double* origins, const double* dirs, const double* max_toi, float* out_filter, uint32_t* out_lit, uint32_t flags,
                                hipStream_t stream) {
    if (!sc || !origins || !dirs || !max_toi || !out_filter || !out_lit) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (check_ray_flags(flags) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    if (n == 0) return NRAYS_OK;
    StageColumn cols[kIsectColumns];
    intersects_columns(cols, origins, dirs, max_toi, out_filter, out_lit);
    const bool reorder = (flags & NRAYS_RAYS_UNORDERED) && reorder_pays(sc, n);
    auto launch = [&](const BatchCall& b, uint32_t nc, void* const* c, unsigned long long) -> int {
        const double *o = (const double*)c[kRayO], *d = (const double*)c[kRayD];
        const uint32_t* order = nullptr;
        const int rc = chunk_order(sc, b.w, reorder, nc, o, d, b.stream, &order);
        if (rc != NRAYS_OK) return rc;
        const IntersectsLaunch a{launch_grid(nc), b.stream, &sc->facts.d, nc, order, o, d, (const double*)c[kIsectToi], (float*)c[kIsectFilter], (uint32_t*)c[kIsectLit], b.w->d_spill};
        return launch_intersects_rays(a, traversal_feat(sc)) ? launch_status("k_intersects_rays") : no_permutation("k_intersects_rays");
    };
    return batch_run(sc, false, stream, cols, kIsectColumns, n, kTraceChunk, "intersects batch", launch);
}

// ---- nrays_cast_rays*: the closest hit of caller-supplied rays: toi and node always, the rest where the caller wants them ---------------------------------------
static int cast_rays_impl(NraysScene* sc, uint32_t n, const double* origins, const double* dirs, const double* max_toi, double* out_toi, int32_t* out_node, double* out_normal,
                          double* out_uv, int32_t* out_prim, uint32_t* out_flags, uint32_t flags, bool staged, hipStream_t stream) {
    if (!sc || !origins || !dirs || !out_toi || !out_node) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (check_ray_flags(flags) != NRAYS_OK) return NRAYS_ERR_BAD_ARG;
    if (n == 0) return NRAYS_OK;
    StageColumn cols[kCastColumns];
    cast_columns(cols, origins, dirs, max_toi, out_toi, out_node, out_normal, out_uv, out_prim, out_flags);
    const bool reorder = (flags & NRAYS_RAYS_UNORDERED) && reorder_pays(sc, n);
    // One chunk: the reorder when it is due, then k_cast_rays or its ordered form.
    auto launch = [&](const BatchCall& b, uint32_t nc, void* const* c, unsigned long long) -> int {
        const double *o = (const double*)c[kRayO], *d = (const double*)c[kRayD];
        const uint32_t* order = nullptr;
        const int rc = chunk_order(sc, b.w, reorder, nc, o, d, b.stream, &order);
        if (rc != NRAYS_OK) return rc;
        const CastLaunch a{launch_grid(nc), b.stream, &sc->facts.d, nc, order, o, d, (const double*)c[kCastMaxToi], (double*)c[kCastToi], (int32_t*)c[kCastNode], (double*)c[kCastNormal],
                           (double*)c[kCastUv], (int32_t*)c[kCastPrim], (uint32_t*)c[kCastFlags], b.w->d_spill};
        return launch_cast_rays(a, traversal_feat(sc)) ? launch_status("k_cast_rays") : no_permutation("k_cast_rays");
    };
    return batch_run(sc, staged, stream, cols, kCastColumns, n, kTraceChunk, "cast batch", launch);
}

// ---- nrays_shade_points*: Material::compute on caller-supplied surface points (material.rs:8-16, phong_material.rs:72-151) -----------------------
// A scene with a non-finite light / colour / texel gets the kernel that skips nothing, as its renders, with the batch's own counter block.
static int shade_points_impl(NraysScene* sc, uint32_t n, const double* points, const double* normals, const double* view_dirs, const double* uvs, const int32_t* nodes,
                             const uint32_t* hit_flags, const uint64_t* keys, float* out, uint32_t flags, bool staged, hipStream_t stream) {
    if (!sc || !points || !normals || !view_dirs || !nodes || !out) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (flags != 0u) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_shade_points: flags must be 0");
    if (n == 0) return NRAYS_OK;
    StageColumn cols[kShadeColumns];
    shade_columns(cols, points, normals, view_dirs, uvs, nodes, hit_flags, keys, out);
    auto launch = [&](const BatchCall& b, uint32_t nc, void* const* c, unsigned long long key_base) -> int {
        const ShadeLaunch a{launch_grid(nc), b.stream, &sc->facts.d, nc, (uint32_t)sc->facts.host.shade.size(), (const double*)c[kShadePoints], (const double*)c[kShadeNormals],
                            (const double*)c[kShadeViews], (const double*)c[kShadeUvs], (const int32_t*)c[kShadeNodes], (const uint32_t*)c[kShadeHit], (const unsigned long long*)c[kShadeKeys],
                            key_base, (float*)c[kShadeOut], b.w->d_counters, b.w->d_spill};
        return launch_shade_points(a, sc->facts.d.no_elide != 0u) ? launch_status("k_shade_points") : no_permutation("k_shade_points");
    };
    return batch_run(sc, staged, stream, cols, kShadeColumns, n, kTraceChunk, "shade batch", launch);
}

// ---- nrays_material_points*: the terms of the points' materials without the lights (material.rs:7, phong_material.rs:39-70 and 120-121; material_points_kernel.h) -------
static int material_points_impl(NraysScene* sc, uint32_t n, const double* normals, const double* uvs, const int32_t* nodes, const uint32_t* hit_flags, float* out_ambient,
                                float* out_diffuse, float* out_specular, double* out_node, uint32_t flags, bool staged, hipStream_t stream) {
    if (!sc || !nodes) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (!out_ambient && !out_diffuse && !out_specular && !out_node) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_material_points: no output (every out_ pointer is null)");
    if (out_ambient && !normals) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_material_points: out_ambient needs normals");
    if (flags != 0u) return set_last_error(NRAYS_ERR_BAD_ARG, "nrays_material_points: flags must be 0");
    if (n == 0) return NRAYS_OK;
    StageColumn cols[kMatColumns];
    material_columns(cols, normals, uvs, nodes, hit_flags, out_ambient, out_diffuse, out_specular, out_node);
    auto launch = [&](const BatchCall& b, uint32_t nc, void* const* c, unsigned long long) -> int {
        const MaterialLaunch a{launch_grid(nc), b.stream, sc->facts.d.shade, nc, (uint32_t)sc->facts.host.shade.size(), (const double*)c[kMatNormals], (const double*)c[kMatUvs],
                               (const int32_t*)c[kMatNodes], (const uint32_t*)c[kMatHit], (float*)c[kMatAmbient], (float*)c[kMatDiffuse], (float*)c[kMatSpecular], (double*)c[kMatNode]};
        launch_material_points(a);
        return launch_status("k_material_points");
    };
    return batch_run(sc, staged, stream, cols, kMatColumns, n, kTraceChunk, "material batch", launch);
}

} // namespace nrays

using namespace nrays;

extern "C" {

// k_cast_batch on host arrays, blocking, in the families' chunks (a test probe).
static_assert(sizeof(NraysCastResult) == 56, "tests/batch_stage_shim.cpp restates the record's size");
int nrays_debug_cast_batch(NraysScene* sc, uint32_t mode, uint32_t n, const double* origins, const double* dirs, const double* max_toi, NraysCastResult* out) {
    if (!sc || !origins || !dirs || !out || mode > 1u || (mode == 1u && !max_toi)) return set_last_error(NRAYS_ERR_BAD_ARG, "bad cast-batch arguments");
    if (n == 0) return NRAYS_OK;
    StageColumn cols[kCastProbeColumns];
    cast_probe_columns(cols, origins, dirs, mode == 1u ? max_toi : nullptr, out, sizeof(NraysCastResult));
    auto launch = [&](const BatchCall& b, uint32_t nc, void* const* c, unsigned long long) -> int {
        const CastBatchLaunch a{launch_grid(nc), b.stream, &sc->facts.d, mode, nc, (const double*)c[kRayO], (const double*)c[kRayD], (const double*)c[kCastProbeMaxToi],
                                (NraysCastResult*)c[kCastProbeOut], b.w->d_spill};
        return launch_cast_batch(a, traversal_feat(sc)) ? launch_status("k_cast_batch") : no_permutation("k_cast_batch");
    };
    return batch_run(sc, true, nullptr, cols, kCastProbeColumns, n, kTraceChunk, "cast-batch probe", launch);
}

int nrays_debug_box_cull(uint32_t mode, uint32_t n, const double* origins, const double* dirs, const double* best, const float* boxes, const uint32_t* slots,
                         float* keys, uint32_t* bits, float* inv32) {
    if (!origins || !dirs || !best || !boxes || !slots || !keys || !bits || !inv32 || mode > 1u) return set_last_error(NRAYS_ERR_BAD_ARG, "bad box-cull arguments");
    if (n > (1u << 24)) return set_last_error(NRAYS_ERR_BAD_ARG, "box-cull: more than 2^24 cases"); // (node index << 7 in 32 bits, as the scenes: scene_build.cpp)
    if (n == 0) return NRAYS_OK;
    for (uint32_t i = 0; i < n; ++i) if (slots[i] > 3u) return set_last_error(NRAYS_ERR_BAD_ARG, "box-cull: child slot above 3");
    std::vector<BvhNode> nodes;
    try { nodes.resize(n); } catch (const std::bad_alloc&) { return set_last_error(NRAYS_ERR_OOM, "box-cull nodes"); }
    const float absent_mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, absent_mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (uint32_t i = 0; i < n; ++i) {
        BvhNode& nd = nodes[i];
        for (int k = 0; k < 4; ++k) { nd.slot[5][k] = 0.0f; nd.set_box(k, absent_mn, absent_mx); nd.children()[k] = kEmptyChild; }
        nd.set_box((int)slots[i], boxes + 6 * (size_t)i, boxes + 6 * (size_t)i + 3);
    }
    BvhNode* d_n = nullptr; double *d_o = nullptr, *d_d = nullptr, *d_b = nullptr; float *d_k = nullptr, *d_i = nullptr; uint32_t* d_bits = nullptr;
    auto release = [&]() { for (void* q : {(void*)d_n, (void*)d_o, (void*)d_d, (void*)d_b, (void*)d_k, (void*)d_i, (void*)d_bits}) if (q) (void)hipFree(q); };
#define CULL_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { release(); return set_last_error(e_ == hipErrorOutOfMemory ? NRAYS_ERR_OOM : NRAYS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } } while (0)
    const size_t vb = (size_t)n * 3 * sizeof(double);
    CULL_TRY(hipMalloc((void**)&d_n, (size_t)n * sizeof(BvhNode))); CULL_TRY(hipMalloc((void**)&d_o, vb)); CULL_TRY(hipMalloc((void**)&d_d, vb));
    CULL_TRY(hipMalloc((void**)&d_b, (size_t)n * sizeof(double))); CULL_TRY(hipMalloc((void**)&d_k, (size_t)n * 4 * sizeof(float)));
    CULL_TRY(hipMalloc((void**)&d_i, (size_t)n * 3 * sizeof(float))); CULL_TRY(hipMalloc((void**)&d_bits, (size_t)n * sizeof(uint32_t)));
    CULL_TRY(hipMemcpy(d_n, nodes.data(), (size_t)n * sizeof(BvhNode), hipMemcpyHostToDevice));
    CULL_TRY(hipMemcpy(d_o, origins, vb, hipMemcpyHostToDevice)); CULL_TRY(hipMemcpy(d_d, dirs, vb, hipMemcpyHostToDevice));
    CULL_TRY(hipMemcpy(d_b, best, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    const uint64_t threads = mode == 1u ? (uint64_t)n * 64u : (uint64_t)n;
    hipLaunchKernelGGL(k_box_cull, dim3(launch_grid(threads)), dim3(kBlock), 0, (hipStream_t)0, (const BvhNode*)d_n, mode, n, (const double*)d_o, (const double*)d_d, (const double*)d_b, d_k, d_bits, d_i);
    CULL_TRY(hipGetLastError());
    CULL_TRY(hipDeviceSynchronize());
    CULL_TRY(hipMemcpy(keys, d_k, (size_t)n * 4 * sizeof(float), hipMemcpyDeviceToHost)); CULL_TRY(hipMemcpy(bits, d_bits, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    CULL_TRY(hipMemcpy(inv32, d_i, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost));
#undef CULL_TRY
    release();
    return NRAYS_OK;
}

int nrays_trace_rays_device(NraysScene* sc, uint32_t n, const double* origins, const double* dirs, const double* refr, const float* energy, const uint64_t* keys,
                            uint32_t max_depth, float* out_rgb, void* hip_stream) {
    return trace_rays_impl(sc, n, origins, dirs, refr, energy, keys, max_depth, out_rgb, 0u, false, (hipStream_t)hip_stream);
}
int nrays_trace_rays_device_ex(NraysScene* sc, uint32_t n, const double* origins, const double* dirs, const double* refr, const float* energy, const uint64_t* keys,
                               uint32_t max_depth, float* out_rgb, uint32_t flags, void* hip_stream) {
    return trace_rays_impl(sc, n, origins, dirs, refr, energy, keys, max_depth, out_rgb, flags, false, (hipStream_t)hip_stream);
}
int nrays_trace_rays(NraysScene* sc, uint32_t n, const double* origins, const double* dirs, const double* refr, const float* energy, const uint64_t* keys,
                     uint32_t max_depth, float* out_rgb) {
    return trace_rays_impl(sc, n, origins, dirs, refr, energy, keys, max_depth, out_rgb, 0u, true, nullptr);
}
int nrays_trace_rays_ex(NraysScene* sc, uint32_t n, const double* origins, const double* dirs, const double* refr, const float* energy, const uint64_t* keys,
                        uint32_t max_depth, float* out_rgb, uint32_t flags) {
    return trace_rays_impl(sc, n, origins, dirs, refr, energy, keys, max_depth, out_rgb, flags, true, nullptr);
}

int nrays_intersects_rays_device(NraysScene* sc, uint32_t n, const double* origins, const double* dirs, const double* max_toi, float* out_filter,
                                 uint32_t* out_lit, void* hip_stream) {
    return intersects_rays_impl(sc, n, origins, dirs, max_toi, out_filter, out_lit, 0u, (hipStream_t)hip_stream);
}
int nrays_intersects_rays_device_ex(NraysScene* sc, uint32_t n, const double* origins, const double* dirs, const double* max_toi, float* out_filter,
                                    uint32_t* out_lit, uint32_t flags, void* hip_stream) {
    return intersects_rays_impl(sc, n, origins, dirs, max_toi, out_filter, out_lit, flags, (hipStream_t)hip_stream);
}

int nrays_cast_rays_device(NraysScene* sc, uint32_t n, const double* origins, const double* dirs, const double* max_toi, double* out_toi, int32_t* out_node,
                           double* out_normal, double* out_uv, int32_t* out_prim, uint32_t* out_flags, uint32_t flags, void* hip_stream) {
    return cast_rays_impl(sc, n, origins, dirs, max_toi, out_toi, out_node, out_normal, out_uv, out_prim, out_flags, flags, false, (hipStream_t)hip_stream);
}
int nrays_cast_rays(NraysScene* sc, uint32_t n, const double* origins, const double* dirs, const double* max_toi, double* out_toi, int32_t* out_node,
                    double* out_normal, double* out_uv, int32_t* out_prim, uint32_t* out_flags, uint32_t flags) {
    return cast_rays_impl(sc, n, origins, dirs, max_toi, out_toi, out_node, out_normal, out_uv, out_prim, out_flags, flags, true, nullptr);
}

int nrays_shade_points_device(NraysScene* sc, uint32_t n, const double* points, const double* normals, const double* view_dirs, const double* uvs, const int32_t* nodes,
                              const uint32_t* hit_flags, const uint64_t* keys, float* out_rgba, uint32_t flags, void* hip_stream) {
    return shade_points_impl(sc, n, points, normals, view_dirs, uvs, nodes, hit_flags, keys, out_rgba, flags, false, (hipStream_t)hip_stream);
}
int nrays_shade_points(NraysScene* sc, uint32_t n, const double* points, const double* normals, const double* view_dirs, const double* uvs, const int32_t* nodes,
                       const uint32_t* hit_flags, const uint64_t* keys, float* out_rgba, uint32_t flags) {
    return shade_points_impl(sc, n, points, normals, view_dirs, uvs, nodes, hit_flags, keys, out_rgba, flags, true, nullptr);
}
int nrays_material_points_device(NraysScene* sc, uint32_t n, const double* normals, const double* uvs, const int32_t* nodes, const uint32_t* hit_flags, float* out_ambient,
                                 float* out_diffuse, float* out_specular, double* out_node, uint32_t flags, void* hip_stream) {
    return material_points_impl(sc, n, normals, uvs, nodes, hit_flags, out_ambient, out_diffuse, out_specular, out_node, flags, false, (hipStream_t)hip_stream);
}
int nrays_material_points(NraysScene* sc, uint32_t n, const double* normals, const double* uvs, const int32_t* nodes, const uint32_t* hit_flags, float* out_ambient,
                          float* out_diffuse, float* out_specular, double* out_node, uint32_t flags) {
    return material_points_impl(sc, n, normals, uvs, nodes, hit_flags, out_ambient, out_diffuse, out_specular, out_node, flags, true, nullptr);
}

} // extern "C"
