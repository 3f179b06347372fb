// texel_dilate_kernel.h — the kernels of nrays_dilate_texels* (texel_calls.hip launches them): every uncovered point of a width x height lattice takes the
// values of the nearest covered point inside a Euclidean disc of radius r, the smallest index among equals.  The definition is the text above
// nrays_dilate_texels_device in include/nrays_abi.h (integers only; Python mirror: nrays_amd.dilate_texels_ref).
//
// The definition is separable, and the two launches of one call are its two halves, on the caller's stream, nothing read back, no atomic:
//   k_dilate_rows   one lane per lattice point, a wave on 64 consecutive x of one row.  The nearest covered column within r <= 64 lies in the wave's own
//                   coverage ballot or in the ballot of one of the two neighbouring 64-column blocks: a count-leading-zeros to the left, a
//                   count-trailing-zeros to the right, the left one on a tie (the smaller index).  Per point one 16-bit word into the workspace: the
//                   signed dx to that column (0 = the point is covered itself), or kDilateNone.
//   k_dilate_cols   a workgroup owns 64 columns x T rows (T = 16 for r <= kDilateShortRadius, else 64: the halo of 2 r rows is loaded once per workgroup).  The dx words of rows
//                   [y0 - r, y0 + T + r) go into LDS, kDilateNone outside the lattice.  A lane whose point is uncovered walks |dy| = 0, 1, .. r outwards
//                   (the row above before the row below), keeps the minimum of (dx^2 + dy^2, index) as two integers compared lexicographically, and
//                   stops as soon as dy^2 exceeds the d2 it holds: nothing farther can win or tie.  Then out_source / out_flags, and the `channels`
//                   words of the source.  The minimum over a row is the row pass's word: a larger |dx| of the same row has a larger d2, and of the two
//                   columns at the same |dx| the left one has the smaller index.
// In-place `values` need no second buffer: only covered points are read, only uncovered points are written.  out_flags may alias flags_in: the row pass has
// finished with flags_in before k_dilate_cols starts, which reads and writes word i in lane i alone.
// Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nrays {

constexpr uint32_t kDilateBlock = 256u;        // threads per workgroup of both kernels: four waves
constexpr uint32_t kDilateWaves = kDilateBlock / 64u;
constexpr uint32_t kDilateMaxRadius = 64u;     // NRAYS_DILATE_MAX_RADIUS: one neighbouring 64-column block to either side suffices
constexpr uint32_t kDilateShortRadius = 8u;    // up to here k_dilate_cols takes 16 rows per workgroup, above it 64
constexpr int16_t kDilateNone = 0x7fff;        // no covered column within r in this row
constexpr uint32_t kDilateFilled = 4u;         // NRAYS_TEXEL_FILLED

struct DilateLattice { uint32_t w, h, r, col_blocks /* ceil(w / 64) */; };

__device__ __forceinline__ uint32_t dilate_rows_per_group(uint32_t r) { return r <= kDilateShortRadius ? 16u : 64u; }

// grid: ceil(h * col_blocks / 4) workgroups; wave `item` of the grid takes columns [64 * cb, 64 * cb + 64) of row y, item = y * col_blocks + cb.
__global__ void __launch_bounds__(kDilateBlock) k_dilate_rows(DilateLattice L, const uint32_t* __restrict__ flags_in, int16_t* __restrict__ dx_out) {
    const uint32_t lane = threadIdx.x & 63u, item = blockIdx.x * kDilateWaves + (threadIdx.x >> 6);
    if (item >= L.h * L.col_blocks) return; // (the whole wave)
    const uint32_t y = item / L.col_blocks, cb = item - y * L.col_blocks;
    const uint32_t x = cb * 64u + lane;
    const uint32_t* row = flags_in + (size_t)y * L.w;
    // the three ballots; a column outside the row is uncovered and is not read
    const bool in_row = x < L.w;
    const bool own = in_row && (row[x] & 1u);
    const bool left = cb > 0u && (row[x - 64u] & 1u);                 // (x - 64 < w: x < w or the block to the left is a full one)
    const bool right = x + 64u < L.w && (row[x + 64u] & 1u);
    const unsigned long long C = __ballot(own), Lm = __ballot(left), Rm = __ballot(right);
    uint32_t dl = 0xffffu, dr = 0xffffu;
    {
        const unsigned long long m = C & (~0ull >> (63u - lane)); // bits 0 .. lane
        if (m) dl = lane - (63u - (uint32_t)__clzll((long long)m));
        else if (Lm) dl = lane + 1u + (uint32_t)__clzll((long long)Lm);
    }
    {
        const unsigned long long m = C & (~0ull << lane);         // bits lane .. 63
        if (m) dr = (uint32_t)__ffsll((long long)m) - 1u - lane;
        else if (Rm) dr = 64u - lane + (uint32_t)__ffsll((long long)Rm) - 1u;
    }
    int16_t dx = kDilateNone;
    if (dl <= dr) { if (dl <= L.r) dx = (int16_t)(-(int32_t)dl); }
    else if (dr <= L.r) dx = (int16_t)dr;
    if (in_row) dx_out[(size_t)y * L.w + x] = dx;
}

// grid: (col_blocks, ceil(h / T)); dynamic LDS: (T + 2 r) * 64 int16.
__global__ void __launch_bounds__(kDilateBlock) k_dilate_cols(DilateLattice L, const int16_t* __restrict__ dx_in, const uint32_t* flags_in, uint32_t channels, uint32_t vec4,
                                                              float* values, int32_t* __restrict__ out_source, uint32_t* out_flags) {
    extern __shared__ __attribute__((aligned(16))) int16_t dilate_lds[];
    const uint32_t T = dilate_rows_per_group(L.r), r = L.r;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t x = blockIdx.x * 64u + lane, y0 = blockIdx.y * T;
    const bool in_row = x < L.w;
    // LDS row k holds lattice row y0 - r + k
    for (uint32_t k = wave; k < T + 2u * r; k += kDilateWaves) {
        const int32_t yy = (int32_t)(y0 + k) - (int32_t)r;
        int16_t v = kDilateNone;
        if (in_row && yy >= 0 && (uint32_t)yy < L.h) v = dx_in[(size_t)yy * L.w + x];
        dilate_lds[k * 64u + lane] = v;
    }
    __syncthreads();
    if (!in_row) return;
    uint32_t* values_w = (uint32_t*)values;
    for (uint32_t t = wave; t < T; t += kDilateWaves) {
        const uint32_t y = y0 + t;
        if (y >= L.h) break;
        const uint32_t i = y * L.w + x, centre = t + r; // (w * h <= 2^24)
        const int32_t own = dilate_lds[centre * 64u + lane];
        if (own == 0) { // covered: its own source
            if (out_source) out_source[i] = (int32_t)i;
            if (out_flags && out_flags != flags_in) out_flags[i] = flags_in[i];
            continue;
        }
        uint32_t best_d2 = r * r + 1u, best = 0u; // nothing found yet: a candidate at d2 = r^2 + 1 ties with this and loses, no index being below 0
        if (own != (int32_t)kDilateNone) { best_d2 = (uint32_t)(own * own); best = (uint32_t)((int32_t)i + own); }
        for (uint32_t k = 1u; k <= r && k * k <= best_d2; ++k) {
            const int32_t up = dilate_lds[(centre - k) * 64u + lane], down = dilate_lds[(centre + k) * 64u + lane];
            if (up != (int32_t)kDilateNone) {
                const uint32_t d2 = (uint32_t)(up * up) + k * k, idx = (uint32_t)((int32_t)(i - k * L.w) + up);
                if (d2 < best_d2 || (d2 == best_d2 && idx < best)) { best_d2 = d2; best = idx; }
            }
            if (down != (int32_t)kDilateNone) {
                const uint32_t d2 = (uint32_t)(down * down) + k * k, idx = (uint32_t)((int32_t)(i + k * L.w) + down);
                if (d2 < best_d2 || (d2 == best_d2 && idx < best)) { best_d2 = d2; best = idx; }
            }
        }
        const bool filled = best_d2 <= r * r;
        if (out_source) out_source[i] = filled ? (int32_t)best : -1;
        if (out_flags && (filled || out_flags != flags_in)) out_flags[i] = flags_in[i] | (filled ? kDilateFilled : 0u);
        if (values_w && filled) {
            if (vec4) ((uint4*)values_w)[i] = ((const uint4*)values_w)[best];
            else for (uint32_t c = 0; c < channels; ++c) values_w[(size_t)i * channels + c] = values_w[(size_t)best * channels + c];
        }
    }
}

} // namespace nrays
