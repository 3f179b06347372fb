// gather_maps_kernel.h — k_gather_maps_points (nrays_gather_maps_points*): the light that baked maps hold at the closest hits of a point's hemisphere rays, folded
// into one mean colour per point — one diffuse bounce of a light-map baker, on the device.  The rays are k_occlusion_points' (occlusion_frame / occlusion_dir),
// the query is k_cast_rays' (ungated traversal, resolve_hit, the gated repeat), the sample is the materials' (tex_sample) and the fold is k_occlusion_points'
// (2^LP lanes a point, added in the order of the directions through __shfl).  The definition is include/nrays_abi.h (NraysGatherMapsParams).
// Templates and inline device code only: gather_maps_inst.hip instantiates the kernel, point_batches.hip launches it through launch_gather_maps_points.
#pragma once
#include "../../include/nrays_abi.h"
#include "ray_batch_kernel.h"

namespace nrays {

// The maps travel in the kernel's arguments: NRAYS_GATHER_MAX_MAPS records of 24 bytes, read with the hit's map index (no device copy, nothing to upload per call).
struct GatherMapsTable { ShadeTex map[NRAYS_GATHER_MAX_MAPS]; };
struct GatherMapsSpec { uint32_t num_dirs, num_rotations; double bias, max_toi; uint32_t num_maps, num_nodes; float miss[3]; };
// The class of a ray's contribution; k_gather_maps_points counts the mapped and the missed ones.
constexpr uint32_t kGatherDark = 0u, kGatherMapped = 1u, kGatherMissed = 2u;

// The closest-hit query of cast_rays_body on ray (o, d), unbounded: the ungated traversal, the winner checked against the exact gates, the gated repeat.  true = a hit,
// with `hit`, `is` and `node_id` its record.  k_gather_maps_points and k_gather_maps_rays (gather_maps_sh_kernel.h) run it once per ray.
template <int FEAT>
NR_DEV bool gather_maps_query(const DScene& S, Stack& st, Cnt& cnt, d3 o, d3 d, Hit& hit, Isect& is, uint32_t& node_id) {
    f3 filter = F3(1.0f, 1.0f, 1.0f);
    bool gated = false, any = false;
    node_id = 0;
    for (;;) {
        any = traverse<false, false, FEAT>(S, st, o, d, kDblMax, hit, filter, cnt, gated, &is);
        if (!any) break;
        if (resolve_hit<false, FEAT, true>(S, o, d, hit, is, node_id) || gated) break;
        gated = true;
    }
    return any;
}
// The finished query -> its contribution and class; `any`: a hit that max_toi kept.  A miss brings P.miss; a hit on a node whose node_map entry names a map, with a
// record that carries a uv, brings x, y, z of Texture2d::sample of that map at the record's (u, v) — tex_sample, the value the library's materials get; every other
// hit is dark (+0).  Transparency and the side of the surface are not looked at.
NR_DEV f3 gather_maps_contribution(bool any, const Isect& is, uint32_t node_id, Cnt& cnt, const GatherMapsSpec& P, const GatherMapsTable& M, const int32_t* __restrict__ node_map,
                                   uint32_t& cls) {
    if (!any) { cls = kGatherMissed; return F3(P.miss[0], P.miss[1], P.miss[2]); }
    cls = kGatherDark;
    if (!is.has_uv || node_id >= P.num_nodes) return F3(0.0f, 0.0f, 0.0f);
    const int32_t m = node_map[node_id];
    if (m < 0 || (uint32_t)m >= P.num_maps) return F3(0.0f, 0.0f, 0.0f);
    const f4 c = tex_sample<false>(M.map[m], is.u, is.v, cnt);
    cls = kGatherMapped;
    return F3(c.x, c.y, c.z);
}
// Ray (o, d) -> its contribution and class: the query, max_toi filtering the FINISHED query, the contribution.
template <int FEAT>
NR_DEV f3 gather_maps_ray(const DScene& S, Stack& st, Cnt& cnt, d3 o, d3 d, const GatherMapsSpec& P, const GatherMapsTable& M, const int32_t* __restrict__ node_map,
                          uint32_t& cls) {
    Hit hit; Isect is; uint32_t node_id;
    bool any = gather_maps_query<FEAT>(S, st, cnt, o, d, hit, is, node_id);
    if (any) any = hit.t <= P.max_toi;
    return gather_maps_contribution(any, is, node_id, cnt, P, M, node_map, cls);
}

// Point i of the chunk: its num_dirs rays, each through gather_maps_ray, folded in the order of the directions — f32 sum, then ONE division by (float)num_dirs;
// out_counts[2i], [2i + 1] count the mapped and the missed rays.  The lanes of a point, the rounds and the shuffles are k_occlusion_points'; the two counts are
// per-lane integers folded through the same shuffles.  The frame is built once per point, as there: what stays live across the traversal is the closest-hit
// query's own state, which fits (profiles/gather_maps_kres.txt: no scratch).
// A point whose flag bit 0 is clear is skipped: zeros, no traversal, neither its point nor its normal read.  NULL keys: key_base + i.
template <int FEAT, int LP>
__global__ void __launch_bounds__(kBlock, NRAYS_WAVES_PER_SIMD) k_gather_maps_points(DScene S, uint32_t n, const double* __restrict__ points, const double* __restrict__ normals,
                                                                                      const uint32_t* __restrict__ hit_flags, const unsigned long long* __restrict__ keys,
                                                                                      unsigned long long key_base, GatherMapsSpec P, GatherMapsTable M,
                                                                                      const int32_t* __restrict__ node_map, const double* __restrict__ dirs,
                                                                                      const double* __restrict__ rotations, float* __restrict__ out_rgb,
                                                                                      uint32_t* __restrict__ out_counts, uint32_t* spill) {
    static_assert(LP >= 0 && LP <= 6, "the lanes of a point share a wave");
    __shared__ uint32_t lds_stack[kLdsStack * kBlock];
    Stack st; st.setup(lds_stack, spill, nullptr);
    Cnt cnt; cnt.zero();
    constexpr uint32_t kLanes = 1u << LP;
    const uint32_t k = P.num_dirs, slots = n << LP; // (n * num_dirs <= 2^22 and 2^LP <= num_dirs: batch_call.h's chunks)
    const bool rotate = P.num_rotations != 0u;
    const OcclusionSpec G{P.num_dirs, P.num_rotations, P.bias, 0.0};
    for (uint32_t base = blockIdx.x * kBlock; base < slots; base += gridDim.x * kBlock) { // block-uniform trip count
        const uint32_t slot = base + threadIdx.x, i = slot >> LP, sub = slot & (kLanes - 1u);
        const bool live = i < n && (!hit_flags || (hit_flags[i] & 1u) != 0u); // (the same for all lanes of a point)
        OccFrame f;
        f.o = f.t = f.u = f.n = D3(0.0, 0.0, 0.0); f.c = 1.0; f.s = 0.0;
        if (live) {
            const size_t i3 = 3 * (size_t)i;
            f = occlusion_frame(D3(points[i3], points[i3 + 1], points[i3 + 2]), D3(normals[i3], normals[i3 + 1], normals[i3 + 2]), keys ? keys[i] : key_base + i, G, rotations);
        }
        f3 sum = F3(0.0f, 0.0f, 0.0f);
        uint32_t mapped = 0u, missed = 0u;
        for (uint32_t j0 = 0; j0 < k; j0 += kLanes) { // wave-uniform rounds
            const uint32_t j = j0 + sub;
            f3 c = F3(0.0f, 0.0f, 0.0f);
            uint32_t cls = kGatherDark;
            if (live && j < k) {
                const d3 d = occlusion_dir(f, rotate, dirs[3 * (size_t)j], dirs[3 * (size_t)j + 1], dirs[3 * (size_t)j + 2]);
                c = gather_maps_ray<FEAT>(S, st, cnt, f.o, d, P, M, node_map, cls);
            }
            if constexpr (LP == 0) {
                sum.x += c.x; sum.y += c.y; sum.z += c.z; // (a skipped point's contribution is +0, its class dark)
                mapped += cls == kGatherMapped ? 1u : 0u; missed += cls == kGatherMissed ? 1u : 0u;
            } else {
#pragma unroll
                for (uint32_t s = 0; s < kLanes; ++s) {
                    const float cx = __shfl(c.x, (int)s, (int)kLanes), cy = __shfl(c.y, (int)s, (int)kLanes), cz = __shfl(c.z, (int)s, (int)kLanes);
                    const uint32_t l = (uint32_t)__shfl((int)cls, (int)s, (int)kLanes);
                    if (j0 + s < k) { sum.x += cx; sum.y += cy; sum.z += cz; mapped += l == kGatherMapped ? 1u : 0u; missed += l == kGatherMissed ? 1u : 0u; }
                }
            }
        }
        if (i < n && sub == 0u) {
            const float fk = (float)k;
            out_rgb[3 * (size_t)i] = sum.x / fk; out_rgb[3 * (size_t)i + 1] = sum.y / fk; out_rgb[3 * (size_t)i + 2] = sum.z / fk;
            if (out_counts) { out_counts[2 * (size_t)i] = mapped; out_counts[2 * (size_t)i + 1] = missed; }
        }
    }
}

// The arguments of one k_gather_maps_points launch; the instantiations are compiled in gather_maps_inst.hip.  false = no such permutation.
struct GatherMapsLaunch {
    uint32_t grid; hipStream_t stream; const DScene* d; uint32_t n; GatherPoints in; GatherMapsSpec spec; const GatherMapsTable* maps; const int32_t* node_map; const double* dirs;
    const double* rotations; float* out_rgb; uint32_t* out_counts; uint32_t* spill;
};
bool launch_gather_maps_points(const GatherMapsLaunch& a, int feat, int lp);

} // namespace nrays
