// light_points_inst.hip — the k_light_points permutations and k_light_rays (light_points_kernel.h), in a translation unit of their own beside point_batches.hip, which
// launches them through launch_light_points / launch_light_rays.  The permutations are k_occlusion_points': kFeatMesh for scenes of opaque meshes, kFeatAll otherwise,
// times 1, 8 or 64 lanes per point.
#include <hip/hip_runtime.h>

#include "light_points_kernel.h"

namespace nrays {

template <int FEAT, int LP>
static bool launch_if(const LightPointsLaunch& a, int feat, int lp) {
    if (feat != FEAT || lp != LP) return false;
    hipLaunchKernelGGL((k_light_points<FEAT, LP>), dim3(a.grid), dim3(kBlock), 0, a.stream, *a.d, a.n, a.points, a.normals, a.hit_flags, a.spec, a.tables, a.out_rgb, a.out_counts, a.spill);
    return true;
}

bool launch_light_points(const LightPointsLaunch& a, int feat, int lp) {
    return launch_if<kFeatAll, 0>(a, feat, lp) || launch_if<kFeatAll, 3>(a, feat, lp) || launch_if<kFeatAll, 6>(a, feat, lp) || launch_if<kFeatMesh, 0>(a, feat, lp) ||
           launch_if<kFeatMesh, 3>(a, feat, lp) || launch_if<kFeatMesh, 6>(a, feat, lp);
}

// nrays_debug_light_rays: the ray of (point i, light k) of the chunk, as k_light_points generates it, to out_*[(i * num_lights + k) ..]: origin and direction 3 f64
// each, t_max, and w (0 = the light is skipped).
__global__ void __launch_bounds__(kBlock) k_light_rays(uint32_t n, const double* __restrict__ points, const double* __restrict__ normals, LightSpec P, LightTables T,
                                                       double* __restrict__ out_origins, double* __restrict__ out_dirs, double* __restrict__ out_tmax, float* __restrict__ out_w) {
    const size_t rays = (size_t)n * P.num_lights;
    for (size_t r = (size_t)blockIdx.x * kBlock + threadIdx.x; r < rays; r += (size_t)gridDim.x * kBlock) {
        const size_t i = r / P.num_lights, k = r % P.num_lights;
        const d3 nm = D3(normals[3 * i], normals[3 * i + 1], normals[3 * i + 2]);
        const d3 q = D3(points[3 * i] + nm.x * P.bias, points[3 * i + 1] + nm.y * P.bias, points[3 * i + 2] + nm.z * P.bias);
        const LightRay lr = light_ray(q, nm, T, k, P);
        out_origins[3 * r] = lr.o.x; out_origins[3 * r + 1] = lr.o.y; out_origins[3 * r + 2] = lr.o.z;
        out_dirs[3 * r] = lr.d.x; out_dirs[3 * r + 1] = lr.d.y; out_dirs[3 * r + 2] = lr.d.z;
        out_tmax[r] = lr.t_max; out_w[r] = lr.w;
    }
}

void launch_light_rays(const LightRaysLaunch& a) {
    hipLaunchKernelGGL(k_light_rays, dim3(a.grid), dim3(kBlock), 0, a.stream, a.n, a.points, a.normals, a.spec, a.tables, a.out_origins, a.out_dirs, a.out_tmax, a.out_w);
}

} // namespace nrays
