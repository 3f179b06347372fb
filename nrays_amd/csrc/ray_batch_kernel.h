// ray_batch_kernel.h — the kernels of the caller-ray batches (nrays_trace_rays*, nrays_intersects_rays_device*, nrays_cast_rays*): k_trace_rays,
// k_intersects_rays and k_cast_rays trace ray j of a chunk in lane j; their _ordered forms trace ray order[j] there and
// write its result to ITS slot (a batch the caller called unordered, binned by ray_key.h's key).  ray_batches.hip launches both forms.  One body
// each, so that the two forms cannot drift apart.  k_shade_points (nrays_shade_points*) lights surface point j in lane j; it has no ordered form.
// k_occlusion_points (nrays_occlusion_points*) builds the hemisphere rays of a point in registers (hemisphere_device.h), traces them and folds them into one value;
// k_gather_points (nrays_gather_points*) runs Scene::trace on the same rays and folds the colours (instantiated in gather_inst.hip);
// k_gather_pairs_ordered traces the (point, direction) pairs of a reordered gather chunk in bin order (nrays_gather_points*_ex; gather_order_inst.hip).
// Templates and inline device code only: ray_batches.hip (which instantiates every kernel here that has no unit of its own), point_batches.hip, ray_order.hip,
// gather_inst.hip and gather_order_inst.hip include this header.
#pragma once
#include "hemisphere_device.h"
#include "primary_kernel.h"

namespace nrays {

// Scene::trace (scene.rs:163-193) on caller-supplied rays (nrays_trace_rays_device): ray i of the chunk is loaded as a depth-0 RayWithEnergy
// of weight 1 whose "pixel" is i, and traced exactly as k_primary traces a primary ray — the chain's sum goes straight to out[3i..3i+2],
// second children to the queue, whose k_bounce rounds and k_fold_fixed then add them as in a frame.  A ray's arithmetic is a one-sample
// pixel's.  NULL refr / energy: 1.0 (RayWithEnergy::new, ray_with_energy.rs:11); NULL keys: key_base + i.  `keyed`: the scene samples
// an area light (the keys are read by nothing else).
// ORDERED: lane j traces ray i = order[j].  Everything that names the ray — its arrays, its key, its output slot, the "pixel" of its queued
// chains and fixed-point sums — uses i, so a ray's result does not depend on where it was traced.
template <bool STATS, int FEAT, bool ORDERED>
__device__ __forceinline__ void trace_rays_body(uint32_t* lds_stack, const DScene& S, uint32_t n, const uint32_t* __restrict__ order, const double* __restrict__ ro,
                                                const double* __restrict__ rd, const double* __restrict__ refr, const float* __restrict__ energy,
                                                const unsigned long long* __restrict__ keys, unsigned long long key_base, uint32_t keyed,
                                                uint32_t max_depth, float* __restrict__ out, QueueOut qo, DeviceCounters* ctr, uint32_t* spill) {
    Stack st; st.setup(lds_stack, spill, nullptr);
    Cnt cnt; cnt.zero();
    for (uint32_t base = blockIdx.x * kBlock; base < n; base += gridDim.x * kBlock) { // block-uniform trip count
        const uint32_t slot = base + threadIdx.x;
        const bool active = slot < n;
        uint32_t idx = slot;
        if (ORDERED) idx = active ? order[slot] : 0u;
        RayState ray;
        ray.o = D3(0, 0, 0); ray.d = D3(0, 0, 1); ray.refr = 1.0; ray.energy = 0.0f; ray.weight = 0.0f; ray.key = 0; ray.pixel = 0;
        if (active) {
            const size_t i3 = 3 * (size_t)idx;
            ray.o = D3(ro[i3], ro[i3 + 1], ro[i3 + 2]); ray.d = D3(rd[i3], rd[i3 + 1], rd[i3 + 2]);
            ray.refr = refr ? refr[idx] : 1.0; ray.energy = energy ? energy[idx] : 1.0f; ray.weight = 1.0f;
            ray.key = keys ? keys[idx] : key_base + idx; ray.pixel = idx;
        }
        const f3 c = trace_chain<STATS, FEAT>(S, st, active, ray, 0u, max_depth, qo, cnt, keyed != 0u);
        if (active) { out[3 * (size_t)idx] = c.x; out[3 * (size_t)idx + 1] = c.y; out[3 * (size_t)idx + 2] = c.z; }
    }
    flush_counters(ctr, cnt, STATS);
}

template <bool STATS, int FEAT>
__global__ void __launch_bounds__(kBlock, NRAYS_WAVES_PER_SIMD) k_trace_rays(DScene S, uint32_t n, const double* __restrict__ ro, const double* __restrict__ rd,
                                                                              const double* __restrict__ refr, const float* __restrict__ energy,
                                                                              const unsigned long long* __restrict__ keys, unsigned long long key_base, uint32_t keyed,
                                                                              uint32_t max_depth, float* __restrict__ out, QueueOut qo, DeviceCounters* ctr, uint32_t* spill) {
    __shared__ uint32_t lds_stack[kLdsStack * kBlock];
    trace_rays_body<STATS, FEAT, false>(lds_stack, S, n, nullptr, ro, rd, refr, energy, keys, key_base, keyed, max_depth, out, qo, ctr, spill);
}
template <bool STATS, int FEAT>
__global__ void __launch_bounds__(kBlock, NRAYS_WAVES_PER_SIMD) k_trace_rays_ordered(DScene S, uint32_t n, const uint32_t* __restrict__ order, const double* __restrict__ ro,
                                                                                      const double* __restrict__ rd, const double* __restrict__ refr, const float* __restrict__ energy,
                                                                                      const unsigned long long* __restrict__ keys, unsigned long long key_base, uint32_t keyed,
                                                                                      uint32_t max_depth, float* __restrict__ out, QueueOut qo, DeviceCounters* ctr, uint32_t* spill) {
    __shared__ uint32_t lds_stack[kLdsStack * kBlock];
    trace_rays_body<STATS, FEAT, true>(lds_stack, S, n, order, ro, rd, refr, energy, keys, key_base, keyed, max_depth, out, qo, ctr, spill);
}

// Scene::intersects_ray (scene.rs:147-161) on caller-supplied rays (nrays_intersects_rays_device): k_cast_batch's mode 1 with the
// reference's Option<filter> as a lit flag and the filter (0, 0, 0 where an opaque node blocks the ray).
template <int FEAT, bool ORDERED>
__device__ __forceinline__ void intersects_rays_body(uint32_t* lds_stack, const DScene& S, uint32_t n, const uint32_t* __restrict__ order, const double* __restrict__ ro,
                                                     const double* __restrict__ rd, const double* __restrict__ max_toi, float* __restrict__ out_filter,
                                                     uint32_t* __restrict__ out_lit, uint32_t* spill) {
    Stack st; st.setup(lds_stack, spill, nullptr);
    Cnt cnt; cnt.zero();
    for (uint32_t base = blockIdx.x * kBlock; base < n; base += gridDim.x * kBlock) {
        const uint32_t slot = base + threadIdx.x;
        if (slot >= n) continue;
        const uint32_t i = ORDERED ? order[slot] : slot;
        const size_t i3 = 3 * (size_t)i;
        const d3 o = D3(ro[i3], ro[i3 + 1], ro[i3 + 2]), d = D3(rd[i3], rd[i3 + 1], rd[i3 + 2]);
        Hit hit; f3 filter = F3(1.0f, 1.0f, 1.0f);
        const bool blocked = traverse<true, false, FEAT>(S, st, o, d, max_toi[i], hit, filter, cnt);
        out_lit[i] = blocked ? 0u : 1u;
        out_filter[i3] = blocked ? 0.0f : filter.x; out_filter[i3 + 1] = blocked ? 0.0f : filter.y; out_filter[i3 + 2] = blocked ? 0.0f : filter.z;
    }
}

template <int FEAT>
__global__ void __launch_bounds__(kBlock, NRAYS_WAVES_PER_SIMD) k_intersects_rays(DScene S, uint32_t n, const double* __restrict__ ro, const double* __restrict__ rd,
                                                                                   const double* __restrict__ max_toi, float* __restrict__ out_filter,
                                                                                   uint32_t* __restrict__ out_lit, uint32_t* spill) {
    __shared__ uint32_t lds_stack[kLdsStack * kBlock];
    intersects_rays_body<FEAT, false>(lds_stack, S, n, nullptr, ro, rd, max_toi, out_filter, out_lit, spill);
}
template <int FEAT>
__global__ void __launch_bounds__(kBlock, NRAYS_WAVES_PER_SIMD) k_intersects_rays_ordered(DScene S, uint32_t n, const uint32_t* __restrict__ order, const double* __restrict__ ro,
                                                                                           const double* __restrict__ rd, const double* __restrict__ max_toi,
                                                                                           float* __restrict__ out_filter, uint32_t* __restrict__ out_lit, uint32_t* spill) {
    __shared__ uint32_t lds_stack[kLdsStack * kBlock];
    intersects_rays_body<FEAT, true>(lds_stack, S, n, order, ro, rd, max_toi, out_filter, out_lit, spill);
}

// Scene::trace's closest-hit query (scene.rs:164-166, 262-283) with SceneNode::cast's record (scene_node.rs:51-54) on caller-supplied rays
// (nrays_cast_rays_device): k_cast_batch's mode 0 — closest_hit (trace_device.h): ungated traversal, the winner checked against the reference's exact AABB
// gates, the fully gated repeat for knife-edge rays — with one array per field.  max_toi (NULL = unbounded) filters the FINISHED query (toi <= max_toi[i]
// keeps the hit; a NaN bound keeps nothing) and never enters the traversal, so a bounded result is the unbounded one or a miss.  The four
// optional outputs are kernel arguments: a NULL test is wave-uniform and a NULL output costs no store.  A miss writes node -1, toi +inf,
// zeros, prim -1, flags 0.
template <int FEAT, bool ORDERED>
__device__ __forceinline__ void cast_rays_body(uint32_t* lds_stack, const DScene& S, uint32_t n, const uint32_t* __restrict__ order, const double* __restrict__ ro,
                                               const double* __restrict__ rd, const double* __restrict__ max_toi, double* __restrict__ out_toi,
                                               int32_t* __restrict__ out_node, double* __restrict__ out_normal, double* __restrict__ out_uv,
                                               int32_t* __restrict__ out_prim, uint32_t* __restrict__ out_flags, uint32_t* spill) {
    Stack st; st.setup(lds_stack, spill, nullptr);
    Cnt cnt; cnt.zero();
    for (uint32_t base = blockIdx.x * kBlock; base < n; base += gridDim.x * kBlock) { // block-uniform trip count
        const uint32_t slot = base + threadIdx.x;
        if (slot >= n) continue;
        const uint32_t i = ORDERED ? order[slot] : slot;
        const size_t i3 = 3 * (size_t)i;
        const d3 o = D3(ro[i3], ro[i3 + 1], ro[i3 + 2]), d = D3(rd[i3], rd[i3 + 1], rd[i3 + 2]);
        Hit hit; f3 filter = F3(1.0f, 1.0f, 1.0f);
        Isect is; uint32_t node_id = 0; bool gated = false, any = false;
        for (;;) { // (closest_hit, kept as text: through the call this kernel's registers are numbered differently)
            any = traverse<false, false, FEAT>(S, st, o, d, kDblMax, hit, filter, cnt, gated, &is);
            if (!any) break;
            if (resolve_hit<false, FEAT, true>(S, o, d, hit, is, node_id) || gated) break;
            gated = true;
        }
        if (any && max_toi) any = hit.t <= max_toi[i];
        out_toi[i] = any ? hit.t : __longlong_as_double(0x7ff0000000000000ll);
        out_node[i] = any ? (int32_t)node_id : -1;
        if (out_normal) { out_normal[i3] = any ? is.n.x : 0.0; out_normal[i3 + 1] = any ? is.n.y : 0.0; out_normal[i3 + 2] = any ? is.n.z : 0.0; }
        if (out_uv) { out_uv[2 * (size_t)i] = any ? is.u : 0.0; out_uv[2 * (size_t)i + 1] = any ? is.v : 0.0; }
        if (out_prim) {
            int32_t prim = -1; // (an analytic shape)
            if (any && (FEAT & kFeatMesh) && (!(FEAT & kFeatAnalytic) || S.instances[hit.inst].kind == NRAYS_SHAPE_TRIMESH)) prim = (int32_t)S.tris[hit.prim].tri_id;
            out_prim[i] = prim;
        }
        if (out_flags) out_flags[i] = any ? (1u | (is.has_uv ? 2u : 0u)) : 0u;
    }
}

template <int FEAT>
__global__ void __launch_bounds__(kBlock, NRAYS_WAVES_PER_SIMD) k_cast_rays(DScene S, uint32_t n, const double* __restrict__ ro, const double* __restrict__ rd,
                                                                             const double* __restrict__ max_toi, double* __restrict__ out_toi, int32_t* __restrict__ out_node,
                                                                             double* __restrict__ out_normal, double* __restrict__ out_uv, int32_t* __restrict__ out_prim,
                                                                             uint32_t* __restrict__ out_flags, uint32_t* spill) {
    __shared__ uint32_t lds_stack[kLdsStack * kBlock];
    cast_rays_body<FEAT, false>(lds_stack, S, n, nullptr, ro, rd, max_toi, out_toi, out_node, out_normal, out_uv, out_prim, out_flags, spill);
}
template <int FEAT>
__global__ void __launch_bounds__(kBlock, NRAYS_WAVES_PER_SIMD) k_cast_rays_ordered(DScene S, uint32_t n, const uint32_t* __restrict__ order, const double* __restrict__ ro,
                                                                                     const double* __restrict__ rd, const double* __restrict__ max_toi, double* __restrict__ out_toi,
                                                                                     int32_t* __restrict__ out_node, double* __restrict__ out_normal, double* __restrict__ out_uv,
                                                                                     int32_t* __restrict__ out_prim, uint32_t* __restrict__ out_flags, uint32_t* spill) {
    __shared__ uint32_t lds_stack[kLdsStack * kBlock];
    cast_rays_body<FEAT, true>(lds_stack, S, n, order, ro, rd, max_toi, out_toi, out_node, out_normal, out_uv, out_prim, out_flags, spill);
}

// Material::compute (material.rs:8-16, phong_material.rs:72-151) on caller-supplied surface points (nrays_shade_points_device): the direct lighting
// of point i with the material of node nodes[i] — ambient term with the texture and opacity-map samples, Light::sample's jittered positions, one
// transparent-shadow query per sample, Phong folded light after light — as out[4i..4i+3], the reference's Point4<f32>: rgb and the MATERIAL's alpha
// (the node's alpha, refl_mix and refr_coeff are Scene::trace's business and are not applied).  The lane fills of an Isect and a RayState only what
// material_compute reads (normal, uv; view direction, key) and calls it as shade_hit does for a hit that has nothing precomputed (pre = false,
// alpha_in = -1).  FEAT must hold kFeatMultiSample: every shadow ray is then traced inside the light loop (the single-sample "pre" path lives in
// shade_hit).  light_is_dark applies as in a render; shade_hit's transparent-hit elision does not — the caller asked for this value itself.
// A point is SKIPPED — (0, 0, 0, 0), no scene record read — when bit 0 of hit_flags[i] is clear or nodes[i] is outside [0, num_nodes): the outputs
// of k_cast_rays can be passed on unfiltered.  hit_flags bit 1: the point carries a uv (only if `uvs` is there at all); NULL hit_flags: every point
// is shaded and carries a uv exactly when `uvs` is non-NULL.  NULL keys: key_base + i.  Points, normals and view directions are used as given and
// are expected to be finite.
template <bool STATS, int FEAT>
__global__ void __launch_bounds__(kBlock, NRAYS_WAVES_PER_SIMD) k_shade_points(DScene S, uint32_t n, uint32_t num_nodes, const double* __restrict__ points,
                                                                                const double* __restrict__ normals, const double* __restrict__ view_dirs,
                                                                                const double* __restrict__ uvs, const int32_t* __restrict__ nodes,
                                                                                const uint32_t* __restrict__ hit_flags, const unsigned long long* __restrict__ keys,
                                                                                unsigned long long key_base, float* __restrict__ out, DeviceCounters* ctr, uint32_t* spill) {
    static_assert((FEAT & kFeatMultiSample) != 0, "k_shade_points traces its shadow rays inside the light loop");
    __shared__ uint32_t lds_stack[kLdsStack * kBlock];
    Stack st; st.setup(lds_stack, spill, nullptr);
    Cnt cnt; cnt.zero();
    for (uint32_t base = blockIdx.x * kBlock; base < n; base += gridDim.x * kBlock) { // block-uniform trip count
        const uint32_t i = base + threadIdx.x;
        if (i >= n) continue;
        const size_t i3 = 3 * (size_t)i;
        const int32_t node = nodes[i];
        const uint32_t hf = hit_flags ? hit_flags[i] : 3u;
        f4 c; c.x = c.y = c.z = c.w = 0.0f;
        if ((hf & 1u) && node >= 0 && (uint32_t)node < num_nodes) {
            Isect is;
            is.toi = 0.0; is.hit = true;
            is.n = D3(normals[i3], normals[i3 + 1], normals[i3 + 2]);
            is.has_uv = uvs != nullptr && (hf & 2u) != 0u;
            is.u = is.has_uv ? uvs[2 * (size_t)i] : 0.0; is.v = is.has_uv ? uvs[2 * (size_t)i + 1] : 0.0;
            RayState ray;
            ray.o = D3(0, 0, 0); ray.d = D3(view_dirs[i3], view_dirs[i3 + 1], view_dirs[i3 + 2]);
            ray.refr = 1.0; ray.energy = 1.0f; ray.weight = 1.0f; ray.pixel = i;
            ray.key = keys ? keys[i] : key_base + i;
            d3 pt = D3(points[i3], points[i3 + 1], points[i3 + 2]);
            c = material_compute<STATS, FEAT>(S, st, S.shade[node], ray, pt, is, cnt, false, false, F3(1.0f, 1.0f, 1.0f), 0u, -1.0f);
        }
        float* o = out + 4 * (size_t)i;
        o[0] = c.x; o[1] = c.y; o[2] = c.z; o[3] = c.w;
    }
    flush_counters(ctr, cnt, STATS);
}

// ---- ambient occlusion at caller-supplied points (nrays_occlusion_points*) --------------------------------------------------------------------
// The rays, the lanes of a point and the mean are hemisphere_device.h's (point_lane, point_frame_live, hemisphere_dir, store_mean): k_occlusion_points traces
// the rays and k_occlusion_rays (nrays_debug_occlusion_rays) stores them.
// Point i of the chunk: num_dirs transparent-shadow queries (Scene::intersects_ray, what k_intersects_rays runs) from p + n * bias, folded in the
// order of the directions — f32 sum of the filters of the rays that got through, then ONE division by (float)num_dirs; out_open[i] counts them.
// 2^LP lanes serve a point: lane `sub` takes the directions j = sub (mod 2^LP), and after every round the 2^LP partial values are added in the order of j
// through __shfl, every lane of the point keeping the same running sum — the sequential f32 sum, so the result does not depend on LP.  The lanes of a point share
// its origin; the host (batch_call.cpp: occlusion_lanes_log2) gives a point as many lanes as its directions fill (measured: profiles/occlusion_rate.json).  LP = 0 is lane = point: no shuffle, and
// direction j is wave-uniform, so the compiler can fetch its three doubles with scalar loads.
// A point whose flag bit 0 is clear is skipped: zeros, no traversal, neither its point nor its normal read.  NULL keys: key_base + i.
template <int FEAT, int LP>
__global__ void __launch_bounds__(kBlock, NRAYS_WAVES_PER_SIMD) k_occlusion_points(DScene S, uint32_t n, const double* __restrict__ points, const double* __restrict__ normals,
                                                                                    const uint32_t* __restrict__ hit_flags, const unsigned long long* __restrict__ keys,
                                                                                    unsigned long long key_base, OcclusionSpec P, const double* __restrict__ dirs,
                                                                                    const double* __restrict__ rotations, float* __restrict__ out_filter,
                                                                                    uint32_t* __restrict__ out_open, uint32_t* spill) {
    __shared__ uint32_t lds_stack[kLdsStack * kBlock];
    Stack st; st.setup(lds_stack, spill, nullptr);
    Cnt cnt; cnt.zero();
    constexpr uint32_t kLanes = 1u << LP;
    const uint32_t k = P.num_dirs, slots = n << LP; // (n <= 2^22: batch_call.h's chunks)
    const bool rotate = P.num_rotations != 0u;
    const GatherPoints in{points, normals, hit_flags, keys, key_base};
    for (uint32_t base = blockIdx.x * kBlock; base < slots; base += gridDim.x * kBlock) { // block-uniform trip count
        const PointLane L = point_lane<LP>(base, n, in);
        const uint32_t i = L.i, sub = L.sub; const bool live = L.live;
        OccFrame f = neutral_frame();
        if (live) f = point_frame_live(in, i, P, rotations);
        f3 sum = F3(0.0f, 0.0f, 0.0f);
        uint32_t open = 0u;
        for (uint32_t j0 = 0; j0 < k; j0 += kLanes) { // wave-uniform rounds
            const uint32_t j = j0 + sub;
            f3 c = F3(0.0f, 0.0f, 0.0f);
            uint32_t lit = 0u;
            if (live && j < k) {
                const d3 d = hemisphere_dir(f, rotate, dirs, j);
                Hit hit; f3 filter = F3(1.0f, 1.0f, 1.0f);
                if (!traverse<true, false, FEAT>(S, st, f.o, d, P.max_toi, hit, filter, cnt)) { c = filter; lit = 1u; }
            }
            if constexpr (LP == 0) {
                sum.x += c.x; sum.y += c.y; sum.z += c.z; open += lit;
            } else {
#pragma unroll
                for (uint32_t s = 0; s < kLanes; ++s) {
                    const float cx = __shfl(c.x, (int)s, (int)kLanes), cy = __shfl(c.y, (int)s, (int)kLanes), cz = __shfl(c.z, (int)s, (int)kLanes);
                    const uint32_t l = (uint32_t)__shfl((int)lit, (int)s, (int)kLanes);
                    if (j0 + s < k) { sum.x += cx; sum.y += cy; sum.z += cz; open += l; }
                }
            }
        }
        if (i < n && sub == 0u) {
            store_mean(out_filter, i, sum, k);
            if (out_open) out_open[i] = open;
        }
    }
}
// The arguments of one k_occlusion_points launch; the instantiations are compiled in ray_batches.hip, beside the other traversal kernels.  false = no such permutation.
struct OcclusionLaunch {
    uint32_t grid; hipStream_t stream; const DScene* d; uint32_t n; GatherPoints in; OcclusionSpec spec; const double* dirs; const double* rotations; float* out_filter;
    uint32_t* out_open; uint32_t* spill;
};
bool launch_occlusion_points(const OcclusionLaunch& a, int feat, int lp);

// ---- incoming light at caller-supplied points (nrays_gather_points*): the mean of Scene::trace over a point's hemisphere rays -----------------------------
// The rays are hemisphere_device.h's (occlusion_frame / hemisphere_dir with the same point, normal, key, tables and bias as the occlusion call: bit for bit the same rays); ray j of point i
// is traced as k_trace_rays traces a ray it loads — a depth-0 RayWithEnergy of refr 1, energy P.energy, weight 1, key rng_hash(key_i, kSaltGather + j), "pixel" i —
// and the chains' sums are folded as the occlusion kernel folds its filters: 2^LP lanes serve a point, and after every round the 2^LP partial colours are added in
// the order of j through __shfl, every lane of the point keeping the same running sum — the sequential f32 sum, whatever LP.  trace_chain holds ballots and
// emit_rays: every lane of the wave reaches it in every round, the idle ones with alive = false.
// The frame is REBUILT in every round from the point, the normal and the key (a handful of f64 operations and one hash beside a whole trace): only those seven
// doubles' worth of registers stay live across trace_chain instead of the frame's 28 (profiles/gather_kres_change.txt, profiles/gather_isa_scratch.txt).
// ray_out != nullptr (double-branching scenes): nothing is folded here.  Ray j of point i is "pixel" i * num_dirs + j of the chunk and its chain's sum goes to
// ray_out[3 * pixel ..] (zeros for a skipped point), exactly as k_trace_rays stores a ray's; the k_bounce rounds and k_fold_fixed add the queued second children per
// RAY, as for a chunk of nrays_trace_rays, and k_gather_fold (point_batches.hip) then runs the sequential fold — so the result is the definition's bit for bit there too.
// A point whose flag bit 0 is clear is skipped: zeros, no traversal, neither its point nor its normal read.  NULL keys: key_base + i.
struct GatherSpec { uint32_t num_dirs, num_rotations; double bias; float energy; uint32_t max_depth, keyed; };

template <bool STATS, int FEAT, int LP>
__global__ void __launch_bounds__(kBlock, NRAYS_WAVES_PER_SIMD) k_gather_points(DScene S, uint32_t n, const double* __restrict__ points, const double* __restrict__ normals,
                                                                                 const uint32_t* __restrict__ hit_flags, const unsigned long long* __restrict__ keys,
                                                                                 unsigned long long key_base, GatherSpec P, const double* __restrict__ dirs,
                                                                                 const double* __restrict__ rotations, float* __restrict__ out, float* __restrict__ ray_out,
                                                                                 QueueOut qo, DeviceCounters* ctr, uint32_t* spill) {
    static_assert(LP >= 0 && LP <= 6, "the lanes of a point share a wave");
    __shared__ uint32_t lds_stack[kLdsStack * kBlock];
    Stack st; st.setup(lds_stack, spill, nullptr);
    Cnt cnt; cnt.zero();
    constexpr uint32_t kLanes = 1u << LP;
    const uint32_t k = P.num_dirs, slots = n << LP; // (n * num_dirs <= 2^22 and 2^LP <= num_dirs: batch_call.h's chunks)
    const bool rotate = P.num_rotations != 0u;
    const OcclusionSpec G{P.num_dirs, P.num_rotations, P.bias, 0.0};
    for (uint32_t base = blockIdx.x * kBlock; base < slots; base += gridDim.x * kBlock) { // block-uniform trip count
        const uint32_t slot = base + threadIdx.x, i = slot >> LP, sub = slot & (kLanes - 1u); // (point_lane and point_frame_live as text: through the calls this kernel compiles to other instructions)
        const bool live = i < n && (!hit_flags || (hit_flags[i] & 1u) != 0u); // (the same for all lanes of a point)
        f3 sum = F3(0.0f, 0.0f, 0.0f);
        for (uint32_t j0 = 0; j0 < k; j0 += kLanes) { // wave-uniform rounds
            const uint32_t j = j0 + sub;
            const bool alive = live && j < k;
            RayState ray;
            ray.o = D3(0, 0, 0); ray.d = D3(0, 0, 1); ray.refr = 1.0; ray.energy = 0.0f; ray.weight = 0.0f; ray.key = 0; ray.pixel = 0;
            if (alive) {
                const size_t i3 = 3 * (size_t)i;
                const unsigned long long key = keys ? keys[i] : key_base + i;
                const OccFrame f = occlusion_frame(D3(points[i3], points[i3 + 1], points[i3 + 2]), D3(normals[i3], normals[i3 + 1], normals[i3 + 2]), key, G, rotations);
                ray.o = f.o; ray.d = hemisphere_dir(f, rotate, dirs, j);
                ray.energy = P.energy; ray.weight = 1.0f; ray.pixel = ray_out ? i * k + j : i;
                ray.key = P.keyed ? rng_hash(key, kSaltGather + j) : 0ULL;
            }
            const f3 c = trace_chain<STATS, FEAT>(S, st, alive, ray, 0u, P.max_depth, qo, cnt, P.keyed != 0u);
            if (ray_out) { // (kernel argument: wave-uniform)
                if (i < n && j < k) { float* o = ray_out + 3 * ((size_t)i * k + j); o[0] = c.x; o[1] = c.y; o[2] = c.z; }
                continue;
            }
            if constexpr (LP == 0) {
                sum.x += c.x; sum.y += c.y; sum.z += c.z; // (a skipped point's chain is +0)
            } else {
#pragma unroll
                for (uint32_t s = 0; s < kLanes; ++s) {
                    const float cx = __shfl(c.x, (int)s, (int)kLanes), cy = __shfl(c.y, (int)s, (int)kLanes), cz = __shfl(c.z, (int)s, (int)kLanes);
                    if (j0 + s < k) { sum.x += cx; sum.y += cy; sum.z += cz; }
                }
            }
        }
        if (!ray_out && i < n && sub == 0u) {
            const float fk = (float)k;
            out[3 * (size_t)i] = sum.x / fk; out[3 * (size_t)i + 1] = sum.y / fk; out[3 * (size_t)i + 2] = sum.z / fk;
        }
    }
    flush_counters(ctr, cnt, STATS);
}

// The arguments of one k_gather_points launch.  The instantiations (trace_chain is the expensive template) are compiled in gather_inst.hip, a translation unit of
// their own beside point_batches.hip, which calls launch_gather_points: false = no such permutation.
struct GatherLaunch {
    uint32_t grid; hipStream_t stream; const DScene* d; uint32_t n; GatherPoints in; GatherSpec spec; const double* dirs; const double* rotations; float* out; float* ray_out;
    const QueueOut* qo; DeviceCounters* ctr; uint32_t* spill;
};
bool launch_gather_points(const GatherLaunch& a, bool stats, int feat, int lp);

// ---- the reordered form of a gather chunk (nrays_gather_points*_ex with NRAYS_RAYS_UNORDERED; host side: point_batches.hip; the binning kernels: ray_order.hip) -------------------
// A chunk's (point, direction) pairs — pair i * num_dirs + j is ray j of point i — are binned by ray_key.h's key and traced in bin order, one lane per pair; the
// rays exist in registers only, rebuilt from (i, j) wherever they are needed (bounds, keys, trace).  What crosses memory per ray is the sort state (key, rank,
// order: 16 bytes) and the colour (12 bytes), both of ONE chunk, in the handle's workspace.
// Bit 0 of a point's flags clear: the point is skipped — none of its pairs is live, neither its point nor its normal is read (hemisphere_device.h: gather_pair_ray).
// Lane t of the chunk traces pair order[t], t < *live (the number of placed pairs, known on the device only: the grid is sized by the chunk's `pairs` and the
// lanes at or beyond *live idle).  The RayState is k_gather_points' — energy, weight 1, refr 1, key rng_hash(key_i, kSaltGather + j) in keyed scenes — with the
// pair as its "pixel" always, and the chain's sum goes to ray_out[3 * pair ..] as k_trace_rays stores a ray's: the queue's rounds (double-branching scenes) and
// k_gather_fold follow.  ray_out was cleared before: a skipped point's pairs are never placed and stay zero.  Every lane of a wave reaches trace_chain.
template <bool STATS, int FEAT>
__global__ void __launch_bounds__(kBlock, NRAYS_WAVES_PER_SIMD) k_gather_pairs_ordered(DScene S, uint32_t pairs, const uint32_t* __restrict__ order, const uint32_t* __restrict__ live,
                                                                                        GatherPoints in, GatherSpec P, const double* __restrict__ dirs,
                                                                                        const double* __restrict__ rotations, float* __restrict__ ray_out, QueueOut qo,
                                                                                        DeviceCounters* ctr, uint32_t* spill) {
    __shared__ uint32_t lds_stack[kLdsStack * kBlock];
    Stack st; st.setup(lds_stack, spill, nullptr);
    Cnt cnt; cnt.zero();
    const uint32_t k = P.num_dirs, placed = *live, m = placed < pairs ? placed : pairs; // (uniform for the grid)
    const OcclusionSpec G{P.num_dirs, P.num_rotations, P.bias, 0.0};
    for (uint32_t base = blockIdx.x * kBlock; base < m; base += gridDim.x * kBlock) { // block-uniform trip count
        const uint32_t t = base + threadIdx.x;
        const uint32_t pair = t < m ? order[t] : 0xffffffffu;
        const bool alive = pair < pairs; // (always for t < m: the order holds pair indices)
        RayState ray;
        ray.o = D3(0, 0, 0); ray.d = D3(0, 0, 1); ray.refr = 1.0; ray.energy = 0.0f; ray.weight = 0.0f; ray.key = 0; ray.pixel = 0;
        if (alive) {
            const uint32_t i = pair / k, j = pair - i * k;
            gather_pair_ray(in, i, j, G, dirs, rotations, ray.o, ray.d);
            ray.energy = P.energy; ray.weight = 1.0f; ray.pixel = pair;
            ray.key = P.keyed ? rng_hash(gather_point_key(in, i), kSaltGather + j) : 0ULL;
        }
        const f3 c = trace_chain<STATS, FEAT>(S, st, alive, ray, 0u, P.max_depth, qo, cnt, P.keyed != 0u);
        if (alive) { float* o = ray_out + 3 * (size_t)pair; o[0] = c.x; o[1] = c.y; o[2] = c.z; }
    }
    flush_counters(ctr, cnt, STATS);
}

// The arguments of one k_gather_pairs_ordered launch; the instantiations are compiled in gather_order_inst.hip, as k_gather_points' are in gather_inst.hip.
struct GatherPairsLaunch {
    uint32_t grid; hipStream_t stream; const DScene* d; uint32_t pairs; const uint32_t* order; const uint32_t* live; GatherPoints in; GatherSpec spec; const double* dirs;
    const double* rotations; float* ray_out; const QueueOut* qo; DeviceCounters* ctr; uint32_t* spill;
};
bool launch_gather_pairs_ordered(const GatherPairsLaunch& a, bool stats, int feat);

} // namespace nrays
