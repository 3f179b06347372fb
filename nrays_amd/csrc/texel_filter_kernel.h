// texel_filter_kernel.h — the kernel of nrays_filter_texels* (texel_calls.hip launches it): one pass of a 5 x 5 a-trous (B3-spline) joint-bilateral filter over a
// width x height lattice of baked values, the weights taken from the texels' world points and normals.  The definition is the text above
// nrays_filter_texels_device in include/nrays_abi.h (f64 weights, f32 sums, tap order fixed; Python mirror: nrays_amd.filter_texels_ref).  The library is
// compiled with -ffp-contract=off and the definition relies on it: every product and every sum below is rounded on its own, nothing is fused.
//
//   k_filter_texels<CH>   a lane owns one lattice point, a workgroup of 256 lanes a block of kFilterTileX x kFilterTileY points of ONE residue class
//                         (x mod step, y mod step).  On the sub-lattice of a residue class the pass is a dense 5 x 5 filter, so the workgroup's taps are the
//                         (kFilterTileX + 4) x (kFilterTileY + 4) points of that sub-lattice around its block, the same tile at every step; the price of
//                         step > 1 is that the global loads of the stage are strided by `step` points (consecutive workgroups are the residues of one block
//                         column, so that they meet in the cache lines they share).  The stage puts the taps into LDS once, as planes per component —
//                         covered bit, p.x p.y p.z n.x n.y n.z (f64), the CH values (f32) — and not as records: a wave reads two rows of 32 consecutive
//                         words of one plane, 64 consecutive banks per 32-lane half for the f64 planes, conflict-free.  A point outside the lattice is
//                         staged as uncovered.  Then every lane walks its 25 taps in the order of the definition.
// Rejected by measurement (profiles/filter_rate.json): a dense block of the lattice with a halo of 2 * step — coalesced loads, but (32 + 4 step) x (8 + 4 step)
// staged points per 256 outputs; it ties at step 2 and takes 1.4 - 1.7 times as long at step 4.
// Uncovered points copy the CH words of values_in as integers, straight from memory; covered points take their own values from the tile.  With CH == 4 and
// both value arrays 16-byte aligned (`vec4`) a point's values are loaded and stored as one 128-bit word.
// Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nrays {

constexpr uint32_t kFilterBlock = 256u;      // threads per workgroup: four waves
constexpr uint32_t kFilterTileX = 32u;       // the block of one residue class a workgroup owns (tests/test_filter_texels_gpu.py reads both from here)
constexpr uint32_t kFilterTileY = 8u;
constexpr uint32_t kFilterHalo = 2u;         // taps reach two sub-lattice points to every side
constexpr uint32_t kFilterMaxStep = 64u;     // NRAYS_FILTER_MAX_STEP
constexpr uint32_t kFilterStageX = kFilterTileX + 2u * kFilterHalo, kFilterStageY = kFilterTileY + 2u * kFilterHalo;
constexpr uint32_t kFilterStagePoints = kFilterStageX * kFilterStageY; // 36 x 12 = 432: 20 736 B of f64 planes, 1 728 B per value plane, 1 728 B of covered bits
static_assert(kFilterTileX * kFilterTileY == kFilterBlock, "one lane per point of the block");

struct FilterLattice {
    uint32_t w, h, step;
    uint32_t tiles_x, tiles_y;   // blocks of a residue class per axis: ceil(ceil(w / step) / kFilterTileX), likewise y
    double r2;                   // pos_radius * pos_radius, the divisor of d2
    double normal_cos, normal_den; // normal_den = 1.0 - normal_cos
};

// grid: (tiles_x * step, tiles_y * step); blockIdx.x = tile * step + residue, likewise y.
template <int CH>
__global__ void __launch_bounds__(kFilterBlock) k_filter_texels(FilterLattice L, const uint32_t* __restrict__ flags_in, const double* __restrict__ points,
                                                                const double* __restrict__ normals, const float* __restrict__ values_in,
                                                                float* __restrict__ values_out, uint32_t vec4) {
    __shared__ double s_geo[6][kFilterStagePoints];
    __shared__ uint32_t s_val[CH][kFilterStagePoints];
    __shared__ uint32_t s_cov[kFilterStagePoints];
    const uint32_t step = L.step;
    const uint32_t rx = blockIdx.x % step, ry = blockIdx.y % step;
    const uint32_t tile_x = blockIdx.x / step, tile_y = blockIdx.y / step;
    // the block's first point in the lattice; every lane of an empty block leaves here, before the barrier
    const uint32_t x0 = rx + tile_x * kFilterTileX * step, y0 = ry + tile_y * kFilterTileY * step;
    if (x0 >= L.w || y0 >= L.h) return;
    const uint32_t* values_w = (const uint32_t*)values_in;

    for (uint32_t k = threadIdx.x; k < kFilterStagePoints; k += kFilterBlock) {
        const uint32_t sy = k / kFilterStageX, sx = k - sy * kFilterStageX;
        const int64_t x = (int64_t)x0 + ((int64_t)sx - (int64_t)kFilterHalo) * (int64_t)step;
        const int64_t y = (int64_t)y0 + ((int64_t)sy - (int64_t)kFilterHalo) * (int64_t)step;
        uint32_t cov = 0u;
        if (x >= 0 && x < (int64_t)L.w && y >= 0 && y < (int64_t)L.h) {
            const size_t i = (size_t)y * L.w + (size_t)x; // (w * h <= 2^24)
            cov = flags_in[i] & 1u;
            if (cov) {
#pragma unroll
                for (int c = 0; c < 3; ++c) { s_geo[c][k] = points[3 * i + c]; s_geo[3 + c][k] = normals[3 * i + c]; }
                bool done = false;
                if constexpr (CH == 4) if (vec4) {
                    const uint4 v = ((const uint4*)values_w)[i];
                    s_val[0][k] = v.x; s_val[1][k] = v.y; s_val[2][k] = v.z; s_val[3][k] = v.w;
                    done = true;
                }
                if (!done) {
#pragma unroll
                    for (int c = 0; c < CH; ++c) s_val[c][k] = values_w[(size_t)CH * i + c];
                }
            }
        }
        s_cov[k] = cov;
    }
    __syncthreads();

    const uint32_t lx = threadIdx.x % kFilterTileX, ly = threadIdx.x / kFilterTileX;
    const uint32_t x = x0 + lx * step, y = y0 + ly * step;
    if (x >= L.w || y >= L.h) return;
    const size_t i = (size_t)y * L.w + x;
    const uint32_t centre = (ly + kFilterHalo) * kFilterStageX + lx + kFilterHalo;
    uint32_t* out_w = (uint32_t*)values_out;
    if (!s_cov[centre]) { // uncovered: the words as they are
        if constexpr (CH == 4) if (vec4) { ((uint4*)out_w)[i] = ((const uint4*)values_w)[i]; return; }
#pragma unroll
        for (int c = 0; c < CH; ++c) out_w[(size_t)CH * i + c] = values_w[(size_t)CH * i + c];
        return;
    }
    const double px = s_geo[0][centre], py = s_geo[1][centre], pz = s_geo[2][centre];
    const double nx = s_geo[3][centre], ny = s_geo[4][centre], nz = s_geo[5][centre];
    float acc[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) acc[c] = 0.0f;
    float wsum = 0.0f;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
#pragma unroll
        for (int t = 0; t < 5; ++t) {
            const uint32_t k = (ly + (uint32_t)j) * kFilterStageX + lx + (uint32_t)t;
            const float kw = (float)((t == 0 || t == 4 ? 1 : t == 2 ? 6 : 4) * (j == 0 || j == 4 ? 1 : j == 2 ? 6 : 4));
            float w;
            if (j == 2 && t == 2) w = 36.0f;
            else {
                if (!s_cov[k]) continue;
                const double dx = s_geo[0][k] - px, dy = s_geo[1][k] - py, dz = s_geo[2][k] - pz;
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                const double wp = 1.0 - d2 / L.r2;
                if (!(wp > 0.0)) continue;
                const double cs = (nx * s_geo[3][k] + ny * s_geo[4][k]) + nz * s_geo[5][k];
                double wn = (cs - L.normal_cos) / L.normal_den;
                if (!(wn > 0.0)) continue;
                if (wn > 1.0) wn = 1.0;
                w = (kw * (float)wp) * (float)wn;
            }
#pragma unroll
            for (int c = 0; c < CH; ++c) acc[c] = acc[c] + w * __uint_as_float(s_val[c][k]);
            wsum = wsum + w;
        }
    }
    if constexpr (CH == 4) if (vec4) { ((float4*)values_out)[i] = make_float4(acc[0] / wsum, acc[1] / wsum, acc[2] / wsum, acc[3] / wsum); return; }
#pragma unroll
    for (int c = 0; c < CH; ++c) values_out[(size_t)CH * i + c] = acc[c] / wsum;
}

} // namespace nrays
