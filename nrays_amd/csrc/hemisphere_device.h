// hemisphere_device.h — the steps shared by the kernels that fire a hemisphere of rays from caller-supplied points (k_occlusion_points, k_gather_points,
// k_gather_pairs_ordered, k_gather_maps_points, k_gather_maps_rays, k_probe_depth_points, the folds k_gather_fold_sh and k_probe_depth_fold, the binning
// kernels of ray_order.hip and the probe k_occlusion_rays): which point and which of its lanes a thread serves (point_lane), the point's frame
// (neutral_frame, point_frame_live), ray j of it (hemisphere_dir, gather_pair_ray) and the mean (store_mean).  Steps, not a skeleton: every kernel keeps
// its own loop over rounds and its own fold, and calls what it needs.  A kernel takes a step only where its compiled code stays what it was with the
// step written out (profiles/point_steps_isa.txt): k_gather_points, whose registers are tight, writes its lane mapping, frame and mean out.
// The rays are DEFINED by include/nrays_abi.h (NraysOcclusionParams) and mirrored in numpy (nrays_amd.occlusion_rays): f64 + - * /, copysign and
// integer arithmetic only, every product evaluated left to right as written, nothing fused (-ffp-contract=off).  occlusion_frame / occlusion_dir are
// the one generator.  Inline device code only.
#pragma once
#include "../../include/nrays_abi.h"
#include "trace_device.h"

namespace nrays {

struct OcclusionSpec { uint32_t num_dirs, num_rotations; double bias, max_toi; };
struct OccFrame { d3 o, t, u, n; double c, s; };
// The points of a chunk (columns kPointPoints .. kPointKeys of batch_stage.h; batch_call.h: chunk_points) and the index of its first point in the call: what the
// launch structs of the point families carry, what the kernels of the reordered gather take as one argument and what the others build from their arguments.
struct GatherPoints { const double* points; const double* normals; const uint32_t* hit_flags; const unsigned long long* keys; unsigned long long key_base; };

// The branch-free orthonormal frame of Duff et al. 2017 around normal n (no singular normal), the biased origin, and the point's rotation
// (c, s) = rotations[rng_hash(key, kSaltOcclusion) % R]; R = 0: no table is read and occlusion_dir leaves (lx, ly) untouched.
NR_DEV OccFrame occlusion_frame(d3 p, d3 n, unsigned long long key, const OcclusionSpec& P, const double* __restrict__ rotations) {
    OccFrame f;
    const double s = copysign(1.0, n.z), a = -1.0 / (s + n.z), b = n.x * n.y * a;
    f.t = D3(1.0 + s * n.x * n.x * a, s * b, -s * n.x);
    f.u = D3(b, s + n.y * n.y * a, -n.y);
    f.n = n;
    f.o = D3(p.x + n.x * P.bias, p.y + n.y * P.bias, p.z + n.z * P.bias);
    f.c = 1.0; f.s = 0.0;
    if (P.num_rotations) {
        const size_t r = (size_t)(rng_hash(key, kSaltOcclusion) % (unsigned long long)P.num_rotations);
        f.c = rotations[2 * r]; f.s = rotations[2 * r + 1];
    }
    return f;
}
// Sample direction (lx, ly, lz) of the local frame (z = the normal) in world space.  Not normalised: the traversal uses directions as given.
NR_DEV d3 occlusion_dir(const OccFrame& f, bool rotate, double lx, double ly, double lz) {
    double x = lx, y = ly;
    if (rotate) { x = f.c * lx - f.s * ly; y = f.s * lx + f.c * ly; }
    return D3((x * f.t.x + y * f.u.x) + lz * f.n.x, (x * f.t.y + y * f.u.y) + lz * f.n.y, (x * f.t.z + y * f.u.z) + lz * f.n.z);
}
// Direction j of the table `dirs` in the frame.
NR_DEV d3 hemisphere_dir(const OccFrame& f, bool rotate, const double* dirs, size_t j) {
    return occlusion_dir(f, rotate, dirs[3 * j], dirs[3 * j + 1], dirs[3 * j + 2]);
}

// Bit 0 of a point's flags clear: the point is skipped — neither its point nor its normal is read.  NULL keys: key_base + i.
NR_DEV bool gather_point_live(const GatherPoints& in, size_t i) { return !in.hit_flags || (in.hit_flags[i] & 1u) != 0u; }
NR_DEV unsigned long long gather_point_key(const GatherPoints& in, size_t i) { return in.keys ? in.keys[i] : in.key_base + i; }

// 2^LP lanes serve a point: thread `base + threadIdx.x` of the chunk is lane `sub` of point i and takes the directions j = sub (mod 2^LP).  `live`: the
// point exists and is not skipped (the same for all lanes of a point).
struct PointLane { uint32_t i, sub; bool live; };
template <int LP>
NR_DEV PointLane point_lane(uint32_t base, uint32_t n, const GatherPoints& in) {
    static_assert(LP >= 0 && LP <= 6, "the lanes of a point share a wave");
    const uint32_t slot = base + threadIdx.x, i = slot >> LP, sub = slot & ((1u << LP) - 1u);
    const bool live = i < n && gather_point_live(in, i);
    return PointLane{i, sub, live};
}
// The frame of LIVE point i, and the frame of a lane without one (all zero, no rotation).  A kernel writes `OccFrame f = neutral_frame(); if (live) f =
// point_frame_live(..);` itself: with the branch inside a helper the compiler orders the frame's registers differently.
NR_DEV OccFrame point_frame_live(const GatherPoints& in, size_t i, const OcclusionSpec& G, const double* rotations) {
    const size_t i3 = 3 * i;
    return occlusion_frame(D3(in.points[i3], in.points[i3 + 1], in.points[i3 + 2]), D3(in.normals[i3], in.normals[i3 + 1], in.normals[i3 + 2]), gather_point_key(in, i), G, rotations);
}
NR_DEV OccFrame neutral_frame() {
    OccFrame f;
    f.o = f.t = f.u = f.n = D3(0.0, 0.0, 0.0); f.c = 1.0; f.s = 0.0;
    return f;
}
// Ray j of LIVE point i, exactly as every kernel here builds it.
NR_DEV void gather_pair_ray(const GatherPoints& in, uint32_t i, uint32_t j, const OcclusionSpec& G, const double* __restrict__ dirs, const double* __restrict__ rotations,
                            d3& o, d3& d) {
    const OccFrame f = point_frame_live(in, i, G, rotations);
    o = f.o; d = hemisphere_dir(f, G.num_rotations != 0u, dirs, j);
}

// out[3i ..] = sum / (float)k: ONE division a channel after the sum.
NR_DEV void store_mean(float* out, uint32_t i, f3 sum, uint32_t k) {
    const float fk = (float)k;
    out[3 * (size_t)i] = sum.x / fk; out[3 * (size_t)i + 1] = sum.y / fk; out[3 * (size_t)i + 2] = sum.z / fk;
}

} // namespace nrays
