// gather_maps_inst.hip — the k_gather_maps_points permutations (gather_maps_kernel.h), in a translation unit of their own beside point_batches.hip, which launches them
// through launch_gather_maps_points.  The permutations are nrays_cast_rays' — kFeatMesh for scenes of meshes only, kFeatAll otherwise — times the lanes per point of
// k_occlusion_points (2^0, 2^3, 2^6).
#include <hip/hip_runtime.h>

#include "gather_maps_kernel.h"

namespace nrays {

template <int FEAT, int LP>
static bool launch_if(const GatherMapsLaunch& a, int feat, int lp) {
    if (feat != FEAT || lp != LP) return false;
    hipLaunchKernelGGL((k_gather_maps_points<FEAT, LP>), dim3(a.grid), dim3(kBlock), 0, a.stream, *a.d, a.n, a.in.points, a.in.normals, a.in.hit_flags, a.in.keys, a.in.key_base,
                       a.spec, *a.maps, a.node_map, a.dirs, a.rotations, a.out_rgb, a.out_counts, a.spill);
    return true;
}

bool launch_gather_maps_points(const GatherMapsLaunch& a, int feat, int lp) {
    return launch_if<kFeatAll, 0>(a, feat, lp) || launch_if<kFeatAll, 3>(a, feat, lp) || launch_if<kFeatAll, 6>(a, feat, lp) ||
           launch_if<kFeatMesh, 0>(a, feat, lp) || launch_if<kFeatMesh, 3>(a, feat, lp) || launch_if<kFeatMesh, 6>(a, feat, lp);
}

} // namespace nrays
