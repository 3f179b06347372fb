// gather_sh_kernel.h — the fold of nrays_gather_sh_points*: a chunk's finished ray colours (the handle's workspace, 12 bytes a ray, written by the unchanged
// k_gather_points / k_gather_pairs_ordered and the queue's rounds) projected onto the real spherical harmonics of bands 0 .. bands - 1 of each ray's direction.
// The value is DEFINED by include/nrays_abi.h (nrays_gather_sh_points_device) and mirrored in numpy (nrays_amd.sh_basis / sh_fold_ref): the basis in f64, left to
// right as written, nothing fused (-ffp-contract=off), rounded once to f32; then per accumulator acc = acc + y * colour in f32 in the order of j (the product
// rounded, then the sum) and one division by (float)num_dirs.
//
// The order of j is fixed, so the parallelism is over points and over the 3 C accumulators of a point (C = bands^2 <= 9): kShGroup = 32 lanes serve a point, lane
// a < 3 C owns accumulator (coefficient a / 3, channel a % 3) — its own output word, (i * C + c) * 3 + ch = i * 3 C + a, so a group's store is one coalesced
// run.  A tile is 32 directions: lane l rebuilds direction j0 + l through occlusion_dir (the one generator; no direction array exists), evaluates its C basis
// values and stores them as f32 to LDS, the group copies the tile's 96 colour floats (one contiguous run of the workspace) beside them, and then the owning lanes
// walk the tile: two LDS reads, one multiply, one add per direction.  The frame depends on the point only and is built once per point, before its tiles.
// LDS layout of a group: y[jj * 9 + c] (the tile's lane l writes at stride 9, coprime to the 32 banks: conflict-free; the walk reads C consecutive words, the
// lanes of one coefficient the same word: broadcast) and col[3 * jj + ch] (copied and read in order).  12 KiB a workgroup, no scratch (profiles/gather_sh_kres.txt).
// A skipped point (bit 0 of its flags clear) stores 3 C exact zeros and reads neither its point, its normal nor its colours.
#pragma once

#include "ray_batch_kernel.h"

namespace nrays {

constexpr uint32_t kShBlock = 256u;                  // threads per workgroup
constexpr uint32_t kShGroup = 32u;                   // lanes per point, and directions per tile
constexpr uint32_t kShGroups = kShBlock / kShGroup;  // points per workgroup and round
constexpr uint32_t kShMaxCoef = 9u;                  // bands <= 3
constexpr uint32_t kShMaxGrid = 1u << 16;
static_assert(3u * kShMaxCoef <= kShGroup, "a lane per accumulator");

// 1 / (2 sqrt(pi)), sqrt(3) / (2 sqrt(pi)), sqrt(15) / (2 sqrt(pi)), sqrt(5) / (4 sqrt(pi)), sqrt(15) / (4 sqrt(pi)): the nearest doubles (tests/test_gather_sh.py)
constexpr double kShK0 = 0.28209479177387814, kShK1 = 0.4886025119029199, kShK2 = 1.0925484305920792, kShK3 = 0.31539156525252005, kShK4 = 0.5462742152960396;

// The first C = bands^2 values of the real basis (no Condon-Shortley sign) at direction d, used as given (not normalised), to y[0 .. C).
NR_DEV void sh_basis_store(d3 d, uint32_t C, float* y) {
    y[0] = (float)kShK0;
    if (C < 4u) return;
    y[1] = (float)(kShK1 * d.y);
    y[2] = (float)(kShK1 * d.z);
    y[3] = (float)(kShK1 * d.x);
    if (C < 9u) return;
    y[4] = (float)((kShK2 * d.x) * d.y);
    y[5] = (float)((kShK2 * d.y) * d.z);
    y[6] = (float)(kShK3 * ((3.0 * d.z) * d.z - 1.0));
    y[7] = (float)((kShK2 * d.x) * d.z);
    y[8] = (float)(kShK4 * (d.x * d.x - d.y * d.y));
}

// rays: 3 * n * num_dirs floats, ray j of point i at 3 * (i * num_dirs + j); out: n * 3 C floats.  C is 1, 4 or 9.
__global__ void __launch_bounds__(kShBlock) k_gather_fold_sh(const float* __restrict__ rays, uint32_t n, GatherPoints in, OcclusionSpec G, const double* __restrict__ dirs,
                                                             const double* __restrict__ rotations, uint32_t C, float* __restrict__ out) {
    __shared__ float s_y[kShGroups][kShGroup * kShMaxCoef];
    __shared__ float s_col[kShGroups][kShGroup * 3u];
    const uint32_t g = threadIdx.x / kShGroup, lane = threadIdx.x % kShGroup;
    const uint32_t k = G.num_dirs, accs = 3u * C;
    const uint32_t c = lane / 3u, ch = lane - 3u * c;
    const bool rotate = G.num_rotations != 0u, owner = lane < accs;
    float* y = s_y[g];
    float* col = s_col[g];
    for (uint32_t base = blockIdx.x * kShGroups; base < n; base += gridDim.x * kShGroups) { // block-uniform trip count
        const uint32_t i = base + g;
        const bool live = i < n && gather_point_live(in, i); // (the same for all lanes of a point)
        OccFrame f = neutral_frame();
        if (live) f = point_frame_live(in, i, G, rotations);
        const float* src = rays + 3 * (size_t)i * k; // (dereferenced for live points only)
        float acc = 0.0f;
        for (uint32_t j0 = 0; j0 < k; j0 += kShGroup) { // block-uniform trip count: the barriers below are reached by every thread
            const uint32_t m = k - j0 < kShGroup ? k - j0 : kShGroup; // directions of this tile
            if (live) {
                if (lane < m) sh_basis_store(hemisphere_dir(f, rotate, dirs, j0 + lane), C, y + lane * kShMaxCoef);
                for (uint32_t t = lane; t < 3u * m; t += kShGroup) col[t] = src[3 * (size_t)j0 + t];
            }
            __syncthreads();
            if (live && owner) {
#pragma unroll 8
                for (uint32_t jj = 0; jj < m; ++jj) acc = acc + y[jj * kShMaxCoef + c] * col[3u * jj + ch];
            }
            __syncthreads();
        }
        if (i < n && owner) out[(size_t)i * accs + lane] = live ? acc / (float)k : 0.0f;
    }
}

} // namespace nrays
