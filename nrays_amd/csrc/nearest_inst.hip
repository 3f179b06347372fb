// nearest_inst.hip — the k_nearest_points permutations (nearest_kernel.h) and the bound probe's kernel, in a translation unit of their own beside point_batches.hip, which
// launches them through launch_nearest_points / launch_nearest_bound.  The permutations are k_cast_rays': kFeatMesh for scenes of meshes only, kFeatAll otherwise.
#include <hip/hip_runtime.h>

#include "nearest_kernel.h"

namespace nrays {

template <int FEAT>
static bool launch_if(const NearestLaunch& a, int feat) {
    if (feat != FEAT) return false;
    hipLaunchKernelGGL((k_nearest_points<FEAT>), dim3(a.grid), dim3(kBlock), 0, a.stream, *a.d, a.n, a.points, a.max_dist, a.hit_flags, a.coord_bound, a.dist, a.node, a.point, a.normal, a.uv,
                       a.prim, a.flags, a.spill);
    return true;
}

// nrays_debug_nearest_bound: nearest_box_bound of point i against box j (6 f64 each, mins then maxs, narrowed to f32 as given) to out[i * boxes + j].
__global__ void __launch_bounds__(kBlock) k_nearest_bound(uint32_t n, uint32_t boxes, const double* __restrict__ points, const double* __restrict__ box, double* __restrict__ out) {
    const size_t total = (size_t)n * boxes;
    for (size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += (size_t)gridDim.x * kBlock) {
        const size_t i = t / boxes, j = t % boxes;
        const double* b = box + 6 * j;
        out[t] = nearest_box_bound(D3(points[3 * i], points[3 * i + 1], points[3 * i + 2]), (float)b[0], (float)b[1], (float)b[2], (float)b[3], (float)b[4], (float)b[5]);
    }
}

bool launch_nearest_points(const NearestLaunch& a, int feat) { return launch_if<kFeatAll>(a, feat) || launch_if<kFeatMesh>(a, feat); }

void launch_nearest_bound(uint32_t grid, hipStream_t stream, uint32_t n, uint32_t boxes, const double* points, const double* box, double* out) {
    hipLaunchKernelGGL(k_nearest_bound, dim3(grid), dim3(kBlock), 0, stream, n, boxes, points, box, out);
}

} // namespace nrays
