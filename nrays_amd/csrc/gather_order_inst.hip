// gather_order_inst.hip — the k_gather_pairs_ordered permutations (ray_batch_kernel.h): the trace of a reordered gather chunk, in a translation unit of its own
// for the reason gather_inst.hip has one (every permutation instantiates trace_chain, and this unit compiles beside that one and point_batches.hip, which launches it).  The
// permutations are launch_trace_rays's: kFeatMesh for scenes of opaque meshes, kFeatAll otherwise, the kernel that counts everything and skips nothing for no_elide scenes.
#include <hip/hip_runtime.h>

#include "ray_batch_kernel.h"

namespace nrays {

template <bool STATS, int FEAT>
static bool launch_if(const GatherPairsLaunch& a, bool stats, int feat) {
    if (stats != STATS || feat != FEAT) return false;
    hipLaunchKernelGGL((k_gather_pairs_ordered<STATS, FEAT>), dim3(a.grid), dim3(kBlock), 0, a.stream, *a.d, a.pairs, a.order, a.live, a.in, a.spec, a.dirs, a.rotations, a.ray_out,
                       *a.qo, a.ctr, a.spill);
    return true;
}

bool launch_gather_pairs_ordered(const GatherPairsLaunch& a, bool stats, int feat) {
    return launch_if<false, kFeatAll>(a, stats, feat) || launch_if<false, kFeatMesh>(a, stats, feat) || launch_if<true, kFeatAll>(a, stats, feat);
}

} // namespace nrays
