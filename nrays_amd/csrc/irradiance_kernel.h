// irradiance_kernel.h — k_irradiance_points of nrays_irradiance_points*: per caller-supplied point and normal the irradiance from a regular grid of SH probes
// (what nrays_gather_sh_points* writes).  The value is DEFINED by include/nrays_abi.h (nrays_irradiance_points_device) and mirrored in numpy
// (nrays_amd.irradiance_points_ref): cell coordinates, facing factor and the basis at the normal in f64, weights and folds in f32, left to right as written,
// nothing fused (-ffp-contract=off), every division the correctly rounded one.
//
// One lane per point; the kernel strides by blocks.  A lane keeps its eight normalised weights and eight row offsets, then walks the 3 C accumulators one at a
// time: up to eight loads (a corner whose weight is 0 is not read), eight multiply-adds, and one update of e[ch] — it never holds a point's 27 coefficients,
// whether out_sh is wanted or not.  Lanes of a wave in surface order share cells, so a corner's load is mostly one address a wave and the grid's rows come from
// L2.  out_sh: a lane's 3 C words lie 12 C bytes from its neighbour's, so storing each accumulator as it is finished costs 64 lines a store instruction (0.75 ms
// for 2 M points at C = 9, against 0.21 ms without out_sh); the accumulators go to LDS instead (lane-major at the odd stride 3 C: conflict-free; 27 KiB a block at
// C = 9) and the block stores its points' words, which are one run of out_sh, coalesced (0.24 ms).  The 32-lanes-a-point layout of k_gather_fold_sh was measured
// too: 0.72 ms in surface order, though twice as fast as this one on shuffled points (profiles/irradiance_layouts_ab.json).  BANDS, the out_sh store and the
// facing factor are template parameters (launch_irradiance_points): the loops over c unroll and the a_c that a smaller C does not need are never computed.  No
// scratch (profiles/irradiance_kres.txt).
// VIS (nrays_irradiance_points_vis*): one more factor a corner, after the facing factor and the validity rule — Chebyshev's bound from the probe's two depth moments
// towards the point (probe_depth_kernel.h: oct_texel), cubed and held above G.floor: one 8-byte load a valid corner beside the corner's 12 C floats.  VIS = false is
// the kernel of nrays_irradiance_points*: the moments are not looked at.
// A skipped point (bit 0 of its flags clear) stores zeros and reads neither its point nor its normal.
#pragma once

#include "gather_sh_kernel.h"
#include "probe_depth_kernel.h"

namespace nrays {

// The checked grid as the kernel takes it: cell[a] = 0 where counts[a] == 1 (the header's rule), sh / valid the call's device addresses; bands is a template parameter.
// moments / res / floor / bias: NraysIrradianceVisibility's, read by the VIS permutations only (null and zeros otherwise).
struct IrradianceGrid { double origin[3], cell[3]; uint32_t counts[3]; const float* sh; const uint32_t* valid; float measure; const float* moments; uint32_t res; float floor; double bias; };
struct IrradianceLaunch { uint32_t grid; hipStream_t stream; uint32_t n; const double* points; const double* normals; const uint32_t* hit_flags; IrradianceGrid g;
                          float* out_rgb; float* out_sh; float* out_weight; };
// point_batches.hip: false = no such permutation.  bands 1 .. 3; want_sh: a.out_sh is stored; facing: NRAYS_IRRADIANCE_FACING; vis: a.g.moments are applied.
bool launch_irradiance_points(const IrradianceLaunch& a, uint32_t bands, bool want_sh, bool facing, bool vis);

constexpr double kShLobe0 = 3.141592653589793, kShLobe1 = 2.0943951023931953, kShLobe2 = 0.7853981633974483; // pi, 2 pi / 3, pi / 4

// a_c = (float)(A_band(c) * Y_c(n)), Y_c the nine expressions of sh_basis_store in f64, for c < C.
template <int C>
NR_DEV void irradiance_lobe(d3 n, float* a) {
    a[0] = (float)(kShLobe0 * kShK0);
    if (C < 4) return;
    a[1] = (float)(kShLobe1 * (kShK1 * n.y));
    a[2] = (float)(kShLobe1 * (kShK1 * n.z));
    a[3] = (float)(kShLobe1 * (kShK1 * n.x));
    if (C < 9) return;
    a[4] = (float)(kShLobe2 * ((kShK2 * n.x) * n.y));
    a[5] = (float)(kShLobe2 * ((kShK2 * n.y) * n.z));
    a[6] = (float)(kShLobe2 * (kShK3 * ((3.0 * n.z) * n.z - 1.0)));
    a[7] = (float)(kShLobe2 * ((kShK2 * n.x) * n.z));
    a[8] = (float)(kShLobe2 * (kShK4 * (n.x * n.x - n.y * n.y)));
}

template <int BANDS, bool WANT_SH, bool FACING, bool VIS>
__global__ void __launch_bounds__(kBlock) k_irradiance_points(uint32_t n, const double* __restrict__ points, const double* __restrict__ normals,
                                                              const uint32_t* __restrict__ hit_flags, IrradianceGrid G, float* __restrict__ out_rgb,
                                                              float* __restrict__ out_sh, float* __restrict__ out_weight) {
    constexpr int C = BANDS * BANDS, ACCS = 3 * C;
    __shared__ float s_sh[WANT_SH ? kBlock * ACCS : 1]; // out_sh of the block's points, lane-major at the odd stride ACCS: conflict-free
    for (uint32_t base = blockIdx.x * kBlock; base < n; base += gridDim.x * kBlock) { // block-uniform trip count (n <= 2^22: no overflow)
        const uint32_t i = base + threadIdx.x;
        const size_t i3 = 3 * (size_t)i;
        const bool inside = i < n;
        const bool live = inside && (!hit_flags || (hit_flags[i] & 1u));
        float w[8];
        uint32_t row[8];
        float wsum = 0.0f;
        d3 nm = D3(0.0, 0.0, 1.0);
        if (live) {
            const double p[3] = {points[i3], points[i3 + 1], points[i3 + 2]};
            nm = D3(normals[i3], normals[i3 + 1], normals[i3 + 2]);
            uint32_t lo[3], hi[3];
            float f[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const uint32_t c = G.counts[a];
                double g = 0.0;
                if (c != 1u) {
                    g = (p[a] - G.origin[a]) / G.cell[a];
                    const double top = (double)(c - 1u);
                    g = g > 0.0 ? (g < top ? g : top) : 0.0;
                }
                const uint32_t cap = (c > 2u ? c : 2u) - 2u, t = (uint32_t)g;
                lo[a] = t < cap ? t : cap;
                hi[a] = lo[a] + 1u < c - 1u ? lo[a] + 1u : c - 1u;
                f[a] = (float)(g - (double)lo[a]);
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const uint32_t ix = (k & 1) ? hi[0] : lo[0], iy = (k & 2) ? hi[1] : lo[1], iz = (k & 4) ? hi[2] : lo[2];
                const float X = (k & 1) ? f[0] : 1.0f - f[0], Y = (k & 2) ? f[1] : 1.0f - f[1], Z = (k & 4) ? f[2] : 1.0f - f[2];
                float wk = (X * Y) * Z;
                d3 q = D3(0.0, 0.0, 0.0); // the probe's position
                if (FACING || VIS) q = D3(G.origin[0] + (double)ix * G.cell[0], G.origin[1] + (double)iy * G.cell[1], G.origin[2] + (double)iz * G.cell[2]);
                if (FACING) {
                    const d3 v = D3(q.x - p[0], q.y - p[1], q.z - p[2]);
                    const double l2 = (v.x * v.x + v.y * v.y) + v.z * v.z;
                    const double c = (v.x * nm.x + v.y * nm.y) + v.z * nm.z;
                    const double t = l2 > 0.0 ? (c / sqrt(l2) + 1.0) * 0.5 : 1.0;
                    wk = wk * (float)(t * t + 0.2);
                }
                row[k] = (iz * G.counts[1] + iy) * G.counts[0] + ix; // (< 2^22)
                bool valid = true;
                if (G.valid && !(G.valid[row[k]] & 1u)) { wk = 0.0f; valid = false; }
                if (VIS && valid) {
                    const d3 v = D3((p[0] + nm.x * G.bias) - q.x, (p[1] + nm.y * G.bias) - q.y, (p[2] + nm.z * G.bias) - q.z);
                    const double l2 = (v.x * v.x + v.y * v.y) + v.z * v.z;
                    if (l2 > 0.0) {
                        const float* m = G.moments + ((size_t)row[k] * (G.res * G.res) + oct_texel(v.x, v.y, v.z, G.res)) * 2u;
                        const float m1 = m[0], m2 = m[1], df = (float)sqrt(l2);
                        if (df > m1) {
                            float var = m2 - m1 * m1;
                            var = var > 0.0f ? var : 0.0f;
                            const float diff = df - m1, den = var + diff * diff;
                            const float ch = den > 0.0f ? var / den : 0.0f, c3 = (ch * ch) * ch;
                            wk = wk * (c3 > G.floor ? c3 : G.floor);
                        }
                    }
                }
                w[k] = wk;
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) wsum = wsum + w[k];
        }
        if (out_weight && inside) out_weight[i] = wsum;
        const bool lit = wsum > 0.0f; // (false for a skipped point)
        float e[3] = {0.0f, 0.0f, 0.0f};
        if (lit) {
            float a[C];
            irradiance_lobe<C>(nm, a);
#pragma unroll
            for (int k = 0; k < 8; ++k) w[k] = w[k] / wsum;
#pragma unroll
            for (int c = 0; c < C; ++c) {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    float s = 0.0f;
#pragma unroll
                    for (int k = 0; k < 8; ++k)
                        if (w[k] != 0.0f) s = s + w[k] * G.sh[(size_t)row[k] * ACCS + (3 * c + ch)];
                    if (WANT_SH) s_sh[threadIdx.x * ACCS + (3 * c + ch)] = s;
                    e[ch] = e[ch] + a[c] * s;
                }
            }
        } else if (WANT_SH) {
#pragma unroll
            for (int t = 0; t < ACCS; ++t) s_sh[threadIdx.x * ACCS + t] = 0.0f;
        }
        if (WANT_SH) { // the block's points are consecutive: their out_sh words are one run, stored coalesced
            __syncthreads();
            const uint32_t words = (n - base < (uint32_t)kBlock ? n - base : (uint32_t)kBlock) * ACCS;
            float* dst = out_sh + (size_t)base * ACCS;
            for (uint32_t t = threadIdx.x; t < words; t += kBlock) dst[t] = s_sh[t];
            __syncthreads();
        }
        if (out_rgb && inside) {
            out_rgb[i3] = lit ? G.measure * e[0] : 0.0f; out_rgb[i3 + 1] = lit ? G.measure * e[1] : 0.0f; out_rgb[i3 + 2] = lit ? G.measure * e[2] : 0.0f;
        }
    }
}

} // namespace nrays
