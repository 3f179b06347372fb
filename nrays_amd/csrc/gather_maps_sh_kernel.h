// gather_maps_sh_kernel.h — k_gather_maps_rays (nrays_gather_maps_sh_points*): a probe filled from baked maps, and what it sees of the geometry, from ONE traversal
// of its rays.  The rays and the lanes of a point are hemisphere_device.h's (point_lane, point_frame_live, hemisphere_dir), the query is closest_hit (trace_device.h) run once per ray, the
// contribution and its class are k_gather_maps_points' (gather_maps_contribution, max_toi filtering the finished query for them alone), and with DEPTH the distance is
// k_probe_depth_points', taken from the UNFILTERED query.  The definition is include/nrays_abi.h (nrays_gather_maps_sh_points_device).
// Nothing that depends on the order of a point's rays is folded here: the kernel stores c_ij (12 bytes a ray of one chunk) and, with DEPTH, rf (4 bytes a ray, a
// second plane of the same buffer) into the handle's workspace, and the unchanged k_gather_fold_sh (gather_sh_kernel.h) and k_probe_depth_fold (probe_depth_kernel.h)
// fold the two planes in the order of j.  What does not depend on it — the mapped and missed counts, the nearby and no-hit counts, the nearest (dist, j) — stays in the
// lane across its rounds and is folded through the lanes of the point ONCE (__shfl_xor), as k_probe_depth_points does.
// Templates and inline device code only: gather_maps_sh_inst.hip instantiates the kernel, point_batches.hip launches it through launch_gather_maps_rays.
#pragma once
#include "gather_maps_kernel.h"
#include "probe_depth_kernel.h"

namespace nrays {

// The depth side of a launch: kernel arguments (wave-uniform), read by the DEPTH = true permutations only.  out_counts, out_nearest, out_nearest_dir: each may be null.
struct GatherMapsDepth { double max_dist, near_dist; float* ray_rf; uint32_t* out_counts; double* out_nearest; uint32_t* out_nearest_dir; };

// Point i of the chunk: its num_dirs rays, each through ONE closest-hit query; ray_rgb[(i * num_dirs + j) * 3 ..] = c_ij for k_gather_fold_sh, and with DEPTH
// D.ray_rf[i * num_dirs + j] = rf for k_probe_depth_fold.  out_counts[2i], [2i + 1] (or null): the mapped and the missed rays, as k_gather_maps_points counts them;
// D.out_counts / out_nearest / out_nearest_dir: what k_probe_depth_points writes.  The rounds, the frame and the skipping are as in
// k_gather_maps_points.  DEPTH = false compiles the depth payload out: the registers of the query and the sample alone (profiles/gather_maps_sh_kres.txt).
// A point whose flag bit 0 is clear is skipped: no traversal, neither its point nor its normal read, nothing stored to the two planes (the folds do not read them);
// counts 0, 0 on both sides, nearest +inf, kDepthNoDir.  NULL keys: key_base + i.
template <int FEAT, int LP, bool DEPTH>
__global__ void __launch_bounds__(kBlock, NRAYS_WAVES_PER_SIMD) k_gather_maps_rays(DScene S, uint32_t n, const double* __restrict__ points, const double* __restrict__ normals,
                                                                                    const uint32_t* __restrict__ hit_flags, const unsigned long long* __restrict__ keys,
                                                                                    unsigned long long key_base, GatherMapsSpec P, GatherMapsTable M,
                                                                                    const int32_t* __restrict__ node_map, const double* __restrict__ dirs,
                                                                                    const double* __restrict__ rotations, float* __restrict__ ray_rgb,
                                                                                    uint32_t* __restrict__ out_counts, GatherMapsDepth D, uint32_t* spill) {
    __shared__ uint32_t lds_stack[kLdsStack * kBlock];
    Stack st; st.setup(lds_stack, spill, nullptr);
    Cnt cnt; cnt.zero();
    constexpr uint32_t kLanes = 1u << LP;
    const uint32_t k = P.num_dirs, slots = n << LP; // (n * num_dirs <= 2^22 and 2^LP <= num_dirs: batch_call.h's chunks)
    const bool rotate = P.num_rotations != 0u;
    const OcclusionSpec G{P.num_dirs, P.num_rotations, P.bias, 0.0};
    const GatherPoints in{points, normals, hit_flags, keys, key_base};
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    for (uint32_t base = blockIdx.x * kBlock; base < slots; base += gridDim.x * kBlock) { // block-uniform trip count
        const PointLane L = point_lane<LP>(base, n, in);
        OccFrame f = neutral_frame();
        if (L.live) f = point_frame_live(in, L.i, G, rotations);
        uint32_t mapped = 0u, missed = 0u, nearby = 0u, nohit = 0u, best_j = kDepthNoDir;
        double best = inf;
        for (uint32_t j0 = 0; j0 < k; j0 += kLanes) { // wave-uniform rounds
            const uint32_t j = j0 + L.sub;
            if (L.live && j < k) {
                const d3 d = hemisphere_dir(f, rotate, dirs, j);
                Hit hit; Isect is; uint32_t node_id;
                const bool any = closest_hit<FEAT>(S, st, cnt, f.o, d, hit, is, node_id);
                const size_t r = (size_t)L.i * k + j; // (< 2^22, or one point's)
                if constexpr (DEPTH) {
                    const double len = sqrt((d.x * d.x + d.y * d.y) + d.z * d.z);
                    const double dist = any ? hit.t * len : inf;
                    D.ray_rf[r] = (float)(dist < D.max_dist ? dist : D.max_dist);
                    nearby += dist < D.near_dist ? 1u : 0u; nohit += any ? 0u : 1u;
                    if (dist < best) { best = dist; best_j = j; } // (a lane's j only grow: the smallest j of its least dist)
                }
                uint32_t cls;
                const f3 c = gather_maps_contribution(any && hit.t <= P.max_toi, is, node_id, cnt, P, M, node_map, cls);
                ray_rgb[3 * r] = c.x; ray_rgb[3 * r + 1] = c.y; ray_rgb[3 * r + 2] = c.z;
                mapped += cls == kGatherMapped ? 1u : 0u; missed += cls == kGatherMissed ? 1u : 0u;
            }
        }
        if constexpr (LP != 0) {
#pragma unroll
            for (uint32_t m = kLanes >> 1; m != 0u; m >>= 1) { // the lanes of a point, reached by every lane of the wave
                mapped += (uint32_t)__shfl_xor((int)mapped, (int)m, (int)kLanes); missed += (uint32_t)__shfl_xor((int)missed, (int)m, (int)kLanes);
                if constexpr (DEPTH) {
                    nearby += (uint32_t)__shfl_xor((int)nearby, (int)m, (int)kLanes); nohit += (uint32_t)__shfl_xor((int)nohit, (int)m, (int)kLanes);
                    const double od = __shfl_xor(best, (int)m, (int)kLanes);
                    const uint32_t oj = (uint32_t)__shfl_xor((int)best_j, (int)m, (int)kLanes);
                    if (od < best || (od == best && oj < best_j)) { best = od; best_j = oj; }
                }
            }
        }
        if (L.i < n && L.sub == 0u) {
            if (out_counts) { out_counts[2 * (size_t)L.i] = mapped; out_counts[2 * (size_t)L.i + 1] = missed; }
            if constexpr (DEPTH) {
                if (D.out_counts) { D.out_counts[2 * (size_t)L.i] = nearby; D.out_counts[2 * (size_t)L.i + 1] = nohit; }
                if (D.out_nearest) D.out_nearest[L.i] = best;
                if (D.out_nearest_dir) D.out_nearest_dir[L.i] = best_j;
            }
        }
    }
}

// The arguments of one k_gather_maps_rays launch; the instantiations are compiled in gather_maps_sh_inst.hip.  `depth` null: the DEPTH = false permutations.
// false = no such permutation.
struct GatherMapsRaysLaunch {
    uint32_t grid; hipStream_t stream; const DScene* d; uint32_t n; GatherPoints in; GatherMapsSpec spec; const GatherMapsTable* maps; const int32_t* node_map; const double* dirs;
    const double* rotations; float* ray_rgb; uint32_t* out_counts; const GatherMapsDepth* depth; uint32_t* spill;
};
bool launch_gather_maps_rays(const GatherMapsRaysLaunch& a, int feat, int lp);

} // namespace nrays
