// light_points_kernel.h — direct light at caller-supplied surface points from a caller-supplied table of point lights (nrays_light_points*): the occlusion kernel's
// sibling.  The rays of a point go towards the lights of a table instead of along the directions of one, each carries a Lambert weight, a light behind the surface
// (or behind its own emitter normal) costs nothing, and the result is a sum.  light_ray is the ONE generator: k_light_points traces what it builds and k_light_rays
// (nrays_debug_light_rays; light_points_inst.hip) stores it.  The arithmetic is DEFINED by include/nrays_abi.h (NraysPointLights) and mirrored in numpy (nrays_amd.light_rays): f64 + - * /
// and sqrt, f32 + *, every product evaluated left to right as written, nothing fused (-ffp-contract=off) — what material_compute (trace_device.h) does for a light of
// the scene, so that a Phong node of diffuse (1, 1, 1) gives the same bits through nrays_shade_points*.
// Templates and inline device code only: light_points_inst.hip instantiates k_light_points, holds k_light_rays, and point_batches.hip launches them through launch_light_points / launch_light_rays.
#pragma once
#include "hemisphere_device.h"
#include "primary_kernel.h"

namespace nrays {

struct LightSpec { uint32_t num_lights, inverse_square; double bias, offset, min_dist; };
// The tables of a chunk: positions num_lights x 3 f64, colors num_lights x 3 f32, emitter normals num_lights x 3 f64 or null (the lights shine every way).
struct LightTables { const double* positions; const float* colors; const double* normals; };
struct LightRay { d3 o, d; double t_max; float w; };

// The ray from q (the point moved along its normal nm by the bias) towards light k, and its weight; w == 0: the light is skipped and no ray exists — a light at q
// itself (d = 0, t_max = 0), one at or below the tangent plane, one whose emitter faces away.
NR_DEV LightRay light_ray(d3 q, d3 nm, const LightTables& T, size_t k, const LightSpec& P) {
    LightRay r;
    const d3 v = D3(T.positions[3 * k], T.positions[3 * k + 1], T.positions[3 * k + 2]) - q;
    const double nrm = sqrt((v.x * v.x + v.y * v.y) + v.z * v.z);
    r.o = q; r.d = D3(0.0, 0.0, 0.0); r.t_max = 0.0; r.w = 0.0f;
    if (!(nrm > 0.0)) return r;
    const d3 ldir = v / nrm;
    float cr = (float)((ldir.x * nm.x + ldir.y * nm.y) + ldir.z * nm.z);
    cr = cr > 0.0f ? cr : 0.0f;
    float ce = 1.0f;
    if (T.normals) { // (kernel argument: wave-uniform)
        ce = (float)(-((ldir.x * T.normals[3 * k] + ldir.y * T.normals[3 * k + 1]) + ldir.z * T.normals[3 * k + 2]));
        ce = ce > 0.0f ? ce : 0.0f;
    }
    float g = 1.0f;
    if (P.inverse_square) {
        const double d2 = nrm * nrm, m2 = P.min_dist * P.min_dist;
        g = (float)(1.0 / (d2 > m2 ? d2 : m2));
    }
    const float w = (cr * ce) * g;
    r.o = D3(q.x + ldir.x * P.offset, q.y + ldir.y * P.offset, q.z + ldir.z * P.offset);
    r.d = ldir;
    r.t_max = nrm - P.offset;
    r.w = w > 0.0f ? w : 0.0f;
    return r;
}

// Point i of the chunk: for light k = 0 .. num_lights - 1 in order, light_ray; a light with w > 0 is counted, and it is open when t_max <= 0 (nothing is traversed,
// filter (1, 1, 1)) or when Scene::intersects_ray (what k_intersects_rays runs) lets it through; an open light adds col * (filter * w) per channel to an f32 sum that
// starts at +0.  out_rgb[3i ..] = the sum; out_counts[2i] = the lights that got a ray, out_counts[2i + 1] = the open ones.
// 2^LP lanes serve a point: lane `sub` takes the lights k = sub (mod 2^LP), and after every round the 2^LP partial values and counts are added in the order of k through
// __shfl, every lane of the point keeping the same running sum — the sequential f32 sum, so the result does not depend on LP (k_occlusion_points' fold).  LP = 0 is
// lane = point: no shuffle, and light k is wave-uniform, so the compiler can fetch its row with scalar loads.
// Every lane of the wave runs every round to its end: a skipped light, a skipped point and a lane beyond the table only leave the traversal out (as in the other point
// kernels it sits in a branch that rejoins before the fold), never the round — the __shfl fold below is reached by all 64 lanes.
// A point whose flag bit 0 is clear is skipped: zeros, no traversal, neither its point nor its normal read.
template <int FEAT, int LP>
__global__ void __launch_bounds__(kBlock, NRAYS_WAVES_PER_SIMD) k_light_points(DScene S, uint32_t n, const double* __restrict__ points, const double* __restrict__ normals,
                                                                                const uint32_t* __restrict__ hit_flags, LightSpec P, LightTables T, float* __restrict__ out_rgb,
                                                                                uint32_t* __restrict__ out_counts, uint32_t* spill) {
    __shared__ uint32_t lds_stack[kLdsStack * kBlock];
    Stack st; st.setup(lds_stack, spill, nullptr);
    Cnt cnt; cnt.zero();
    constexpr uint32_t kLanes = 1u << LP;
    const uint32_t m = P.num_lights, slots = n << LP; // (n * num_lights <= 2^22 and 2^LP <= num_lights, or n == 1 .. 1024 with LP <= 6: batch_call.h's chunks)
    const GatherPoints in{points, normals, hit_flags, nullptr, 0ull};
    for (uint32_t base = blockIdx.x * kBlock; base < slots; base += gridDim.x * kBlock) { // block-uniform trip count
        const PointLane L = point_lane<LP>(base, n, in);
        const uint32_t i = L.i, sub = L.sub; const bool live = L.live;
        d3 q = D3(0.0, 0.0, 0.0), nm = D3(0.0, 0.0, 0.0);
        if (live) {
            const size_t i3 = 3 * (size_t)i;
            nm = D3(normals[i3], normals[i3 + 1], normals[i3 + 2]);
            q = D3(points[i3] + nm.x * P.bias, points[i3 + 1] + nm.y * P.bias, points[i3 + 2] + nm.z * P.bias);
        }
        f3 sum = F3(0.0f, 0.0f, 0.0f);
        uint32_t rays = 0u, open = 0u;
        for (uint32_t k0 = 0; k0 < m; k0 += kLanes) { // wave-uniform rounds
            const uint32_t k = k0 + sub;
            f3 c = F3(0.0f, 0.0f, 0.0f);
            uint32_t ray = 0u, lit = 0u;
            if (live && k < m) {
                const LightRay r = light_ray(q, nm, T, k, P);
                if (r.w > 0.0f) {
                    ray = 1u;
                    f3 filter = F3(1.0f, 1.0f, 1.0f);
                    bool blocked = false;
                    if (r.t_max > 0.0) { Hit hit; blocked = traverse<true, false, FEAT>(S, st, r.o, r.d, r.t_max, hit, filter, cnt); }
                    if (!blocked) {
                        lit = 1u;
                        c = F3(T.colors[3 * (size_t)k] * (filter.x * r.w), T.colors[3 * (size_t)k + 1] * (filter.y * r.w), T.colors[3 * (size_t)k + 2] * (filter.z * r.w));
                    }
                }
            }
            if constexpr (LP == 0) {
                if (lit) { sum.x += c.x; sum.y += c.y; sum.z += c.z; }
                rays += ray; open += lit;
            } else {
#pragma unroll
                for (uint32_t s = 0; s < kLanes; ++s) {
                    const float cx = __shfl(c.x, (int)s, (int)kLanes), cy = __shfl(c.y, (int)s, (int)kLanes), cz = __shfl(c.z, (int)s, (int)kLanes);
                    const uint32_t fl = (uint32_t)__shfl((int)(ray | (lit << 1)), (int)s, (int)kLanes);
                    if (fl & 2u) { sum.x += cx; sum.y += cy; sum.z += cz; }
                    rays += fl & 1u; open += fl >> 1;
                }
            }
        }
        if (i < n && sub == 0u) {
            out_rgb[3 * (size_t)i] = sum.x; out_rgb[3 * (size_t)i + 1] = sum.y; out_rgb[3 * (size_t)i + 2] = sum.z;
            if (out_counts) { out_counts[2 * (size_t)i] = rays; out_counts[2 * (size_t)i + 1] = open; }
        }
    }
}

// The arguments of one k_light_points launch and of one k_light_rays launch; the instantiations are compiled in light_points_inst.hip.  false = no such permutation.
struct LightPointsLaunch {
    uint32_t grid; hipStream_t stream; const DScene* d; uint32_t n; const double* points; const double* normals; const uint32_t* hit_flags; LightSpec spec; LightTables tables;
    float* out_rgb; uint32_t* out_counts; uint32_t* spill;
};
bool launch_light_points(const LightPointsLaunch& a, int feat, int lp);
struct LightRaysLaunch {
    uint32_t grid; hipStream_t stream; uint32_t n; const double* points; const double* normals; LightSpec spec; LightTables tables; double* out_origins; double* out_dirs;
    double* out_tmax; float* out_w;
};
void launch_light_rays(const LightRaysLaunch& a);

} // namespace nrays
