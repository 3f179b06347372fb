// gather_inst.hip — the k_gather_points permutations (ray_batch_kernel.h), in a translation unit of their own: every one instantiates trace_chain, the
// expensive template, and compiles beside point_batches.hip (which launches them through launch_gather_points) instead of behind it.
// The permutations are launch_trace_rays's — kFeatMesh for scenes of opaque meshes, kFeatAll otherwise, the kernel that counts everything and skips nothing for
// no_elide scenes — times the lanes per point of k_occlusion_points (2^0, 2^3, 2^6).
#include <hip/hip_runtime.h>

#include "ray_batch_kernel.h"

namespace nrays {

template <bool STATS, int FEAT, int LP>
static bool launch_if(const GatherLaunch& a, bool stats, int feat, int lp) {
    if (stats != STATS || feat != FEAT || lp != LP) return false;
    hipLaunchKernelGGL((k_gather_points<STATS, FEAT, LP>), dim3(a.grid), dim3(kBlock), 0, a.stream, *a.d, a.n, a.in.points, a.in.normals, a.in.hit_flags, a.in.keys, a.in.key_base,
                       a.spec, a.dirs, a.rotations, a.out, a.ray_out, *a.qo, a.ctr, a.spill);
    return true;
}

bool launch_gather_points(const GatherLaunch& a, bool stats, int feat, int lp) {
    return launch_if<false, kFeatAll, 0>(a, stats, feat, lp) || launch_if<false, kFeatAll, 3>(a, stats, feat, lp) || launch_if<false, kFeatAll, 6>(a, stats, feat, lp) ||
           launch_if<false, kFeatMesh, 0>(a, stats, feat, lp) || launch_if<false, kFeatMesh, 3>(a, stats, feat, lp) || launch_if<false, kFeatMesh, 6>(a, stats, feat, lp) ||
           launch_if<true, kFeatAll, 0>(a, stats, feat, lp) || launch_if<true, kFeatAll, 3>(a, stats, feat, lp) || launch_if<true, kFeatAll, 6>(a, stats, feat, lp);
}

} // namespace nrays
