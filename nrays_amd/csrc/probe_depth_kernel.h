// probe_depth_kernel.h — nrays_probe_depth_points*: what a probe sees of the geometry around it — per point an octahedral map of the mean and mean squared
// distance to the nearest surface (the visibility term of DDGI, read by k_irradiance_points<.., VIS = true>), the rays that end close by or nowhere, and the
// nearest hit.  The definition is include/nrays_abi.h (NraysProbeDepthParams), mirrored in numpy (nrays_amd.oct_texel / probe_depth_ref).
// Two kernels.  k_probe_depth_points: the rays and the lanes of a point are hemisphere_device.h's (point_lane, point_frame_live, hemisphere_dir: 2^LP lanes serve a
// point), the query is closest_hit (trace_device.h).  What does not depend on the order of the rays — the two counts and the nearest (dist, j), a lexicographic minimum — stays in
// the lane across its rounds and is folded through the lanes of the point ONCE, after the last round (__shfl_xor: log2 steps instead of the 2^LP steps a round of an ordered
// fold).  What does depend on it — the f32 sums of a texel — cannot go through lanes: the kernel stores rf, 4 bytes a ray of one chunk, into the handle's workspace, as
// the gather keeps a chunk's colours for k_gather_fold_sh.
// k_probe_depth_fold gives every (point, texel) a lane: R * R lanes serve a point, a tile is R * R directions; lane l rebuilds direction j0 + l (the one generator; no
// direction array exists), stores its texel and its rf to LDS, and every lane walks the tile in the order of j, adding the entries of ITS texel — one broadcast LDS read a
// step, a second one on a match.  The frame is built once per point.  2 KiB of LDS a workgroup, no scratch in either kernel (profiles/probe_depth_kres.txt).
// Templates and inline device code only: probe_depth_inst.hip instantiates both kernels, point_batches.hip launches them through launch_probe_depth_points / _fold.
#pragma once
#include "../../include/nrays_abi.h"
#include "ray_batch_kernel.h"

namespace nrays {

struct ProbeDepthSpec { uint32_t num_dirs, num_rotations; double bias, max_dist, near_dist; uint32_t res; };
constexpr uint32_t kDepthBlock = 256u;       // threads per workgroup of k_probe_depth_fold: one point at R = 16, four at R = 8, sixteen at R = 4
constexpr uint32_t kDepthMaxGrid = 1u << 16;
constexpr uint32_t kDepthNoDir = 0xffffffffu;

// One axis of the octahedral square: a in [-1, 1] -> its texel column in 0 .. R - 1; a NaN gives 0.
NR_DEV uint32_t oct_axis(double a, uint32_t R) {
    const double g = (a * 0.5 + 0.5) * (double)R;
    if (!(g > 0.0)) return 0u;
    const uint32_t t = (uint32_t)g; // (g <= R)
    return t < R - 1u ? t : R - 1u;
}
// The texel of direction (x, y, z), used as given, in the R x R octahedral map (include/nrays_abi.h: nrays_probe_depth_points_device, "texel"): the producer's for a
// ray's direction and the consumer's (irradiance_kernel.h) for the vector from a probe to a point.
NR_DEV uint32_t oct_texel(double x, double y, double z, uint32_t R) {
    const double s = (fabs(x) + fabs(y)) + fabs(z);
    double a = 0.0, b = 0.0;
    if (s > 0.0) { a = x / s; b = y / s; }
    if (z < 0.0) {
        const double a0 = a, b0 = b;
        a = (1.0 - fabs(b0)) * copysign(1.0, a0);
        b = (1.0 - fabs(a0)) * copysign(1.0, b0);
    }
    return oct_axis(b, R) * R + oct_axis(a, R);
}

// Point i of the chunk: its num_dirs rays, each through closest_hit (unbounded); ray_out[i * num_dirs + j] = rf, the clamped distance in f32, for
// k_probe_depth_fold.  out_counts[2i], [2i + 1]: the rays with dist < near_dist and the rays without a hit; out_nearest / out_nearest_dir: the least dist
// and the smallest j that has it.  Each of the three may be null.
// A point whose flag bit 0 is clear is skipped: no traversal, neither its point nor its normal read, nothing stored to ray_out (the fold does not read it);
// counts 0, 0, nearest +inf, kDepthNoDir.  NULL keys: key_base + i.
template <int FEAT, int LP>
__global__ void __launch_bounds__(kBlock, NRAYS_WAVES_PER_SIMD) k_probe_depth_points(DScene S, uint32_t n, const double* __restrict__ points, const double* __restrict__ normals,
                                                                                      const uint32_t* __restrict__ hit_flags, const unsigned long long* __restrict__ keys,
                                                                                      unsigned long long key_base, ProbeDepthSpec P, const double* __restrict__ dirs,
                                                                                      const double* __restrict__ rotations, float* __restrict__ ray_out,
                                                                                      uint32_t* __restrict__ out_counts, double* __restrict__ out_nearest,
                                                                                      uint32_t* __restrict__ out_nearest_dir, uint32_t* spill) {
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
        const double inf = __longlong_as_double(0x7ff0000000000000ll);
        uint32_t nearby = 0u, missed = 0u, best_j = kDepthNoDir;
        double best = inf;
        for (uint32_t j0 = 0; j0 < k; j0 += kLanes) { // wave-uniform rounds
            const uint32_t j = j0 + L.sub;
            if (L.live && j < k) {
                const d3 d = hemisphere_dir(f, rotate, dirs, j);
                Hit hit; Isect is; uint32_t node_id;
                const bool any = closest_hit<FEAT>(S, st, cnt, f.o, d, hit, is, node_id);
                const double len = sqrt((d.x * d.x + d.y * d.y) + d.z * d.z);
                const double dist = any ? hit.t * len : inf;
                ray_out[(size_t)L.i * k + j] = (float)(dist < P.max_dist ? dist : P.max_dist);
                nearby += dist < P.near_dist ? 1u : 0u; missed += any ? 0u : 1u;
                if (dist < best) { best = dist; best_j = j; } // (a lane's j only grow: the smallest j of its least dist)
            }
        }
        if constexpr (LP != 0) {
#pragma unroll
            for (uint32_t m = kLanes >> 1; m != 0u; m >>= 1) { // the lanes of a point: sums, and the minimum of (dist, j)
                nearby += (uint32_t)__shfl_xor((int)nearby, (int)m, (int)kLanes); missed += (uint32_t)__shfl_xor((int)missed, (int)m, (int)kLanes);
                const double od = __shfl_xor(best, (int)m, (int)kLanes);
                const uint32_t oj = (uint32_t)__shfl_xor((int)best_j, (int)m, (int)kLanes);
                if (od < best || (od == best && oj < best_j)) { best = od; best_j = oj; }
            }
        }
        if (L.i < n && L.sub == 0u) {
            if (out_counts) { out_counts[2 * (size_t)L.i] = nearby; out_counts[2 * (size_t)L.i + 1] = missed; }
            if (out_nearest) out_nearest[L.i] = best;
            if (out_nearest_dir) out_nearest_dir[L.i] = best_j;
        }
    }
}

// rays: rf of ray j of point i at i * num_dirs + j (k_probe_depth_points); out: n x R*R x 2 floats.  R * R lanes a point, kDepthBlock / (R * R) points a workgroup.
template <int R>
__global__ void __launch_bounds__(kDepthBlock) k_probe_depth_fold(const float* __restrict__ rays, uint32_t n, GatherPoints in, OcclusionSpec G, const double* __restrict__ dirs,
                                                                  const double* __restrict__ rotations, float max_dist, float* __restrict__ out) {
    constexpr uint32_t kGroup = R * R, kGroups = kDepthBlock / kGroup; // lanes per point = directions per tile; points per workgroup and round
    static_assert(R == 4 || R == 8 || R == 16, "a workgroup holds whole points");
    __shared__ uint32_t s_tex[kDepthBlock];
    __shared__ float s_rf[kDepthBlock];
    const uint32_t g = threadIdx.x / kGroup, lane = threadIdx.x % kGroup;
    const uint32_t k = G.num_dirs;
    const bool rotate = G.num_rotations != 0u;
    uint32_t* tex = s_tex + g * kGroup;
    float* rf = s_rf + g * kGroup;
    for (uint32_t base = blockIdx.x * kGroups; base < n; base += gridDim.x * kGroups) { // block-uniform trip count
        const uint32_t i = base + g;
        const bool live = i < n && gather_point_live(in, i); // (the same for all lanes of a point)
        OccFrame f = neutral_frame();
        if (live) f = point_frame_live(in, i, G, rotations);
        const float* src = rays + (size_t)i * k; // (dereferenced for live points only)
        float s1 = 0.0f, s2 = 0.0f;
        uint32_t cnt = 0u;
        for (uint32_t j0 = 0; j0 < k; j0 += kGroup) { // block-uniform trip count: the barriers below are reached by every thread
            const uint32_t m = k - j0 < kGroup ? k - j0 : kGroup; // directions of this tile
            if (live && lane < m) {
                const d3 d = hemisphere_dir(f, rotate, dirs, j0 + lane);
                tex[lane] = oct_texel(d.x, d.y, d.z, (uint32_t)R);
                rf[lane] = src[j0 + lane];
            }
            __syncthreads();
            if (live) {
#pragma unroll 8
                for (uint32_t jj = 0; jj < m; ++jj) {
                    if (tex[jj] == lane) { const float r = rf[jj]; s1 = s1 + r; s2 = s2 + r * r; ++cnt; }
                }
            }
            __syncthreads();
        }
        if (i < n) {
            float* o = out + ((size_t)i * kGroup + lane) * 2u;
            o[0] = cnt ? s1 / (float)cnt : max_dist;
            o[1] = cnt ? s2 / (float)cnt : max_dist * max_dist;
        }
    }
}

// The arguments of the two launches; the instantiations are compiled in probe_depth_inst.hip.  false = no such permutation.
struct ProbeDepthLaunch {
    uint32_t grid; hipStream_t stream; const DScene* d; uint32_t n; GatherPoints in; ProbeDepthSpec spec; const double* dirs; const double* rotations; float* ray_out;
    uint32_t* out_counts; double* out_nearest; uint32_t* out_nearest_dir; uint32_t* spill;
};
bool launch_probe_depth_points(const ProbeDepthLaunch& a, int feat, int lp);
struct ProbeDepthFoldLaunch { hipStream_t stream; uint32_t n; GatherPoints in; ProbeDepthSpec spec; const double* dirs; const double* rotations; const float* rays; float* out_moments; };
bool launch_probe_depth_fold(const ProbeDepthFoldLaunch& a, uint32_t res);

} // namespace nrays
