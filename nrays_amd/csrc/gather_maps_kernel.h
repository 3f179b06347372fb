// gather_maps_kernel.h — k_gather_maps_points (nrays_gather_maps_points*): the light that baked maps hold at the closest hits of a point's hemisphere rays, folded
// into one mean colour per point — one diffuse bounce of a light-map baker, on the device.  The rays, the lanes of a point and the mean are
// hemisphere_device.h's (point_lane, point_frame_live, hemisphere_dir, store_mean), the query is closest_hit (trace_device.h), the sample is the materials'
// (tex_sample) and the fold is the ordered one: 2^LP lanes a point, added in the order of the directions through __shfl.  The definition is include/nrays_abi.h (NraysGatherMapsParams).
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
    bool any = closest_hit<FEAT>(S, st, cnt, o, d, hit, is, node_id);
    if (any) any = hit.t <= P.max_toi;
    return gather_maps_contribution(any, is, node_id, cnt, P, M, node_map, cls);
}

// Point i of the chunk: its num_dirs rays, each through gather_maps_ray, folded in the order of the directions — f32 sum, then ONE division by (float)num_dirs;
// out_counts[2i], [2i + 1] count the mapped and the missed rays.  The two counts are per-lane integers: a ray's class goes through the shuffles
// beside its colour.  The frame is built once per point: what stays live across the traversal is the closest-hit
// query's own state, which fits (profiles/gather_maps_kres.txt: no scratch).
// A point whose flag bit 0 is clear is skipped: zeros, no traversal, neither its point nor its normal read.  NULL keys: key_base + i.
template <int FEAT, int LP>
__global__ void __launch_bounds__(kBlock, NRAYS_WAVES_PER_SIMD) k_gather_maps_points(DScene S, uint32_t n, const double* __restrict__ points, const double* __restrict__ normals,
                                                                                      const uint32_t* __restrict__ hit_flags, const unsigned long long* __restrict__ keys,
                                                                                      unsigned long long key_base, GatherMapsSpec P, GatherMapsTable M,
                                                                                      const int32_t* __restrict__ node_map, const double* __restrict__ dirs,
                                                                                      const double* __restrict__ rotations, float* __restrict__ out_rgb,
                                                                                      uint32_t* __restrict__ out_counts, uint32_t* spill) {
    __shared__ uint32_t lds_stack[kLdsStack * kBlock];
    Stack st; st.setup(lds_stack, spill, nullptr);
    Cnt cnt; cnt.zero();
    constexpr uint32_t kLanes = 1u << LP;
    const uint32_t k = P.num_dirs, slots = n << LP; // (n * num_dirs <= 2^22 and 2^LP <= num_dirs: batch_call.h's chunks)
    const bool rotate = P.num_rotations != 0u;
    const OcclusionSpec G{P.num_dirs, P.num_rotations, P.bias, 0.0};
    const GatherPoints in{points, normals, hit_flags, keys, key_base};
    for (uint32_t base = blockIdx.x * kBlock; base < slots; base += gridDim.x * kBlock) { // block-uniform trip count
        const PointLane L = point_lane<LP>(base, n, in);
        OccFrame f = neutral_frame();
        if (L.live) f = point_frame_live(in, L.i, G, rotations);
        f3 sum = F3(0.0f, 0.0f, 0.0f);
        uint32_t mapped = 0u, missed = 0u;
        for (uint32_t j0 = 0; j0 < k; j0 += kLanes) { // wave-uniform rounds
            const uint32_t j = j0 + L.sub;
            f3 c = F3(0.0f, 0.0f, 0.0f);
            uint32_t cls = kGatherDark;
            if (L.live && j < k) c = gather_maps_ray<FEAT>(S, st, cnt, f.o, hemisphere_dir(f, rotate, dirs, j), P, M, node_map, cls);
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
        if (L.i < n && L.sub == 0u) {
            store_mean(out_rgb, L.i, sum, k);
            if (out_counts) { out_counts[2 * (size_t)L.i] = mapped; out_counts[2 * (size_t)L.i + 1] = missed; }
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
