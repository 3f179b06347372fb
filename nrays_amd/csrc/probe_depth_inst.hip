// probe_depth_inst.hip — the k_probe_depth_points and k_probe_depth_fold permutations (probe_depth_kernel.h), in a translation unit of their own beside
// point_batches.hip, which launches them through launch_probe_depth_points / launch_probe_depth_fold.  The trace's permutations are k_gather_maps_points' —
// kFeatMesh for scenes of meshes only, kFeatAll otherwise, times the lanes per point of k_occlusion_points (2^0, 2^3, 2^6); the fold's are the three resolutions.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "probe_depth_kernel.h"

namespace nrays {

template <int FEAT, int LP>
static bool launch_if(const ProbeDepthLaunch& a, int feat, int lp) {
    if (feat != FEAT || lp != LP) return false;
    hipLaunchKernelGGL((k_probe_depth_points<FEAT, LP>), dim3(a.grid), dim3(kBlock), 0, a.stream, *a.d, a.n, a.in.points, a.in.normals, a.in.hit_flags, a.in.keys, a.in.key_base,
                       a.spec, a.dirs, a.rotations, a.ray_out, a.out_counts, a.out_nearest, a.out_nearest_dir, a.spill);
    return true;
}

bool launch_probe_depth_points(const ProbeDepthLaunch& a, int feat, int lp) {
    return launch_if<kFeatAll, 0>(a, feat, lp) || launch_if<kFeatAll, 3>(a, feat, lp) || launch_if<kFeatAll, 6>(a, feat, lp) ||
           launch_if<kFeatMesh, 0>(a, feat, lp) || launch_if<kFeatMesh, 3>(a, feat, lp) || launch_if<kFeatMesh, 6>(a, feat, lp);
}

template <int R>
static bool launch_if(const ProbeDepthFoldLaunch& a, uint32_t res) {
    if (res != (uint32_t)R) return false;
    constexpr uint32_t kGroups = kDepthBlock / (uint32_t)(R * R);
    const uint32_t grid = std::min<uint32_t>((a.n + kGroups - 1u) / kGroups, kDepthMaxGrid);
    hipLaunchKernelGGL((k_probe_depth_fold<R>), dim3(grid), dim3(kDepthBlock), 0, a.stream, a.rays, a.n, a.in, OcclusionSpec{a.spec.num_dirs, a.spec.num_rotations, a.spec.bias, 0.0},
                       a.dirs, a.rotations, (float)a.spec.max_dist, a.out_moments);
    return true;
}

bool launch_probe_depth_fold(const ProbeDepthFoldLaunch& a, uint32_t res) { return launch_if<4>(a, res) || launch_if<8>(a, res) || launch_if<16>(a, res); }

} // namespace nrays
