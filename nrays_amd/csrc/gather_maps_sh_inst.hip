// gather_maps_sh_inst.hip — the k_gather_maps_rays permutations (gather_maps_sh_kernel.h), in a translation unit of their own beside point_batches.hip, which launches
// them through launch_gather_maps_rays.  The permutations are k_gather_maps_points' — kFeatMesh for scenes of meshes only, kFeatAll otherwise, times the lanes per
// point of k_occlusion_points (2^0, 2^3, 2^6) — times DEPTH: with or without the payload of k_probe_depth_points.
#include <hip/hip_runtime.h>

#include "gather_maps_sh_kernel.h"

namespace nrays {

template <int FEAT, int LP, bool DEPTH>
static bool launch_if(const GatherMapsRaysLaunch& a, int feat, int lp) {
    if (feat != FEAT || lp != LP || (a.depth != nullptr) != DEPTH) return false;
    const GatherMapsDepth none{0.0, 0.0, nullptr, nullptr, nullptr, nullptr};
    hipLaunchKernelGGL((k_gather_maps_rays<FEAT, LP, DEPTH>), dim3(a.grid), dim3(kBlock), 0, a.stream, *a.d, a.n, a.in.points, a.in.normals, a.in.hit_flags, a.in.keys, a.in.key_base,
                       a.spec, *a.maps, a.node_map, a.dirs, a.rotations, a.ray_rgb, a.out_counts, a.depth ? *a.depth : none, a.spill);
    return true;
}
template <int FEAT, bool DEPTH>
static bool launch_if_lanes(const GatherMapsRaysLaunch& a, int feat, int lp) {
    return launch_if<FEAT, 0, DEPTH>(a, feat, lp) || launch_if<FEAT, 3, DEPTH>(a, feat, lp) || launch_if<FEAT, 6, DEPTH>(a, feat, lp);
}

bool launch_gather_maps_rays(const GatherMapsRaysLaunch& a, int feat, int lp) {
    return launch_if_lanes<kFeatAll, false>(a, feat, lp) || launch_if_lanes<kFeatMesh, false>(a, feat, lp) || launch_if_lanes<kFeatAll, true>(a, feat, lp) ||
           launch_if_lanes<kFeatMesh, true>(a, feat, lp);
}

} // namespace nrays
