// surface_texels_kernel.h — the kernels of nrays_surface_texels* (texel_calls.hip launches them): which triangle of a TriMesh node owns each point of a
// width x height lattice in uv space, and the surface record there.  The definition is the text above nrays_surface_texels_device in
// include/nrays_abi.h (f64 + - * /, sqrt and comparisons, left to right, nothing fused; Python mirror: nrays_amd.surface_texels_ref); the functions
// texel_coord .. texel_cover below restate it and are the only arithmetic both passes run, so that the resolve pass finds its owner covering again.
//
// Launches of one call, all on the caller's stream, nothing read back, no kernel waits for another workgroup:
//   (memset)         the owner words, one 64-bit word per lattice point, to all ones = uncovered
//   k_texel_count    one lane per triangle record of the node's BLAS range: the number of 8 x 8 lattice tiles its uv box touches (0 for another node's
//                    record, a degenerate triangle, a box beside the lattice)
//   k_texel_sums / k_texel_scan / k_texel_apply   exclusive prefix sum of the counts in place, 64 bits (ray_order.hip's three-launch scan, widened: a
//                    record has up to 2^22 tiles and a range up to 2^28 records); the total stays on the device
//   k_texel_owner    the items (record, tile) in scan order, 64 per wave and trip: every lane finds ITS item by bisection of the scanned counts, then the
//                    wave takes the 64 items one after the other with one lane per lattice point of the tile; a covering lane does
//                    atomicMin(owner, tri_id << 32 | record index).  The grid is fixed and strides over the device-side total with a 64-bit item index: a
//                    wave's trip count is total / (64 x waves) whatever the sizes of the triangles are, and no index can overflow.
//   k_texel_resolve  one lane per lattice point: the record of the owner word, its edge values again, the outputs.
// The owner word orders by the triangle's index in its mesh first: the smallest covering index wins whatever order the items run in.  The record
// index below it only picks ONE of the leaf references a pre-split triangle has (the smallest); they hold the same corners and uvs bit for bit.
// Device code only.
#pragma once
#include "trace_device.h"

namespace nrays {

constexpr uint32_t kTexelBlock = 256u;                                 // threads per workgroup of the kernels below
constexpr uint32_t kTexelScanItems = 16u, kTexelScanBlock = kTexelBlock * kTexelScanItems; // records per workgroup of the scan
constexpr uint32_t kTexelMaxRecords = 1u << 28;                        // scene_build.cpp refuses scenes with more triangle records
constexpr uint32_t kTexelMaxBlocks = kTexelMaxRecords / kTexelScanBlock; // 65 536 block sums; word [kTexelMaxBlocks] holds the total
constexpr uint32_t kTexelOwnerWgsPerCu = 4u;                           // k_texel_owner's grid: four waves per SIMD
constexpr unsigned long long kTexelUncovered = ~0ull;

struct TexelLattice { uint32_t w, h, centres, node; };
struct TexelXform { Xform m; uint32_t flags /* kInstIdentityRot, kInstNoXform */, flip; };
struct TexelOutputs { double* points; double* normals; double* uv; int32_t* node; int32_t* prim; uint32_t* flags; };

NR_DEV double texel_coord(uint32_t i, uint32_t n, uint32_t centres) {
    if (centres) return ((double)i + 0.5) / (double)n;
    return n > 1u ? (double)i / (double)(n - 1u) : 0.0;
}
// The watertight edge value: the endpoints in lexicographic order, the sign restored.
NR_DEV double texel_edge(double pu, double pv, double qu, double qv, double su, double sv) {
    const bool swapped = qu < pu || (qu == pu && qv < pv);
    if (swapped) { const double tu = pu, tv = pv; pu = qu; pv = qv; qu = tu; qv = tv; }
    const double e = (qu - pu) * (sv - pv) - (qv - pv) * (su - pu);
    return swapped ? -e : e;
}
struct TexelUv { double au, av, bu, bv, cu, cv; };
NR_DEV TexelUv texel_uv(const TriUv& t) { TexelUv r; r.au = t.uv[0]; r.av = t.uv[1]; r.bu = t.uv[2]; r.bv = t.uv[3]; r.cu = t.uv[4]; r.cv = t.uv[5]; return r; }
// area2 with its sign, or 0 for a triangle that covers nothing (degenerate, non-finite).
NR_DEV double texel_area2(const TexelUv& t) {
    const double area2 = (t.bu - t.au) * (t.cv - t.av) - (t.bv - t.av) * (t.cu - t.au);
    return (area2 != 0.0 && fabs(area2) <= kDblMax) ? area2 : 0.0; // (NaN fails both comparisons)
}
NR_DEV bool texel_cover(const TexelUv& t, double area2, double su, double sv, double& e0, double& e1, double& e2, double& sum) {
    const double ulo = fmin(t.au, fmin(t.bu, t.cu)), uhi = fmax(t.au, fmax(t.bu, t.cu)), vlo = fmin(t.av, fmin(t.bv, t.cv)), vhi = fmax(t.av, fmax(t.bv, t.cv));
    if (!(su >= ulo && su <= uhi && sv >= vlo && sv <= vhi)) return false;
    const double s = area2 > 0.0 ? 1.0 : -1.0;
    e0 = s * texel_edge(t.bu, t.bv, t.cu, t.cv, su, sv);
    e1 = s * texel_edge(t.cu, t.cv, t.au, t.av, su, sv);
    e2 = s * texel_edge(t.au, t.av, t.bu, t.bv, su, sv);
    sum = (e0 + e1) + e2;
    return e0 >= 0.0 && e1 >= 0.0 && e2 >= 0.0 && sum != 0.0;
}
// The lattice indices whose coordinate can lie in [lo, hi]: a superset with one index of margin on each side (the products below are off by a rounding,
// far less than an index), clamped IN F64 before the conversion — a uv of 3e38 or a negative one never reaches an integer.  false: none.
NR_DEV bool texel_range(double lo, double hi, uint32_t n, uint32_t centres, uint32_t& i0, uint32_t& i1) {
    double a, b;
    if (centres) { a = lo * (double)n - 0.5; b = hi * (double)n - 0.5; }
    else { a = lo * (double)(n - 1u); b = hi * (double)(n - 1u); }
    a = floor(a) - 1.0; b = ceil(b) + 1.0;
    const double top = (double)(n - 1u);
    if (!(b >= 0.0) || !(a <= top)) return false; // (a NaN fails both)
    a = a < 0.0 ? 0.0 : a; b = b > top ? top : b;
    i0 = (uint32_t)a; i1 = (uint32_t)b;
    return true;
}
struct TexelBox { uint32_t x0, x1, y0, y1; };
NR_DEV bool texel_box(const TexelUv& t, const TexelLattice& L, TexelBox& b) {
    const double ulo = fmin(t.au, fmin(t.bu, t.cu)), uhi = fmax(t.au, fmax(t.bu, t.cu)), vlo = fmin(t.av, fmin(t.bv, t.cv)), vhi = fmax(t.av, fmax(t.bv, t.cv));
    return texel_range(ulo, uhi, L.w, L.centres, b.x0, b.x1) && texel_range(vlo, vhi, L.h, L.centres, b.y0, b.y1);
}

// One lane per record of the range: the 8 x 8 tiles its box touches (at most 2048 x 2048).
__global__ void __launch_bounds__(kTexelBlock) k_texel_count(const TriRec* __restrict__ tris, const TriUv* __restrict__ uvs, uint32_t first, uint32_t n, TexelLattice L,
                                                             unsigned long long* __restrict__ counts) {
    const uint32_t i = blockIdx.x * kTexelBlock + threadIdx.x;
    if (i >= n) return;
    unsigned long long c = 0ull;
    if (tris[first + i].node_id == L.node) {
        const TexelUv t = texel_uv(uvs[first + i]);
        TexelBox b;
        if (texel_area2(t) != 0.0 && texel_box(t, L, b)) c = (unsigned long long)((b.x1 >> 3) - (b.x0 >> 3) + 1u) * (unsigned long long)((b.y1 >> 3) - (b.y0 >> 3) + 1u);
    }
    counts[i] = c;
}

// Exclusive prefix sum in place, three launches (ray_order.hip's k_bin_* with 64-bit sums; a thread owns 16 consecutive records).
__global__ void __launch_bounds__(kTexelBlock) k_texel_sums(const unsigned long long* __restrict__ in, uint32_t n, unsigned long long* __restrict__ block_sum) {
    __shared__ unsigned long long s_w[kTexelBlock / 64u];
    const uint32_t base = blockIdx.x * kTexelScanBlock + threadIdx.x * kTexelScanItems;
    unsigned long long sum = 0ull;
    for (uint32_t k = 0; k < kTexelScanItems; ++k) if (base + k < n) sum += in[base + k];
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off);
    if ((threadIdx.x & 63u) == 0u) s_w[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0u) block_sum[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}
__global__ void __launch_bounds__(1024) k_texel_scan(unsigned long long* block_sum, uint32_t nb, unsigned long long* total) { // one workgroup; nb <= kTexelMaxBlocks
    __shared__ unsigned long long s_sum[1024];
    const uint32_t per = (nb + 1023u) / 1024u, lo = min(nb, threadIdx.x * per), hi = min(nb, lo + per);
    unsigned long long sum = 0ull;
    for (uint32_t b = lo; b < hi; ++b) sum += block_sum[b];
    s_sum[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < 1024u; off <<= 1) { const unsigned long long v = threadIdx.x >= off ? s_sum[threadIdx.x - off] : 0ull; __syncthreads(); s_sum[threadIdx.x] += v; __syncthreads(); }
    unsigned long long run = s_sum[threadIdx.x] - sum;
    for (uint32_t b = lo; b < hi; ++b) { const unsigned long long v = block_sum[b]; block_sum[b] = run; run += v; }
    if (threadIdx.x == 1023u) *total = s_sum[1023];
}
__global__ void __launch_bounds__(kTexelBlock) k_texel_apply(unsigned long long* __restrict__ io, uint32_t n, const unsigned long long* __restrict__ block_base) {
    __shared__ unsigned long long s_t[kTexelBlock];
    const uint32_t base = blockIdx.x * kTexelScanBlock + threadIdx.x * kTexelScanItems;
    unsigned long long v[kTexelScanItems], sum = 0ull;
    for (uint32_t k = 0; k < kTexelScanItems; ++k) { v[k] = base + k < n ? io[base + k] : 0ull; sum += v[k]; }
    s_t[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < kTexelBlock; off <<= 1) { const unsigned long long q = threadIdx.x >= off ? s_t[threadIdx.x - off] : 0ull; __syncthreads(); s_t[threadIdx.x] += q; __syncthreads(); }
    unsigned long long run = block_base[blockIdx.x] + s_t[threadIdx.x] - sum;
    for (uint32_t k = 0; k < kTexelScanItems; ++k) { if (base + k < n) io[base + k] = run; run += v[k]; }
}

// The owner pass.  off[r] = items before record r (n >= 1 records, off[0] = 0), *total_p = all items.  Every lane of a wave stays to the end of a trip: the items
// are handed round by shuffles.
__global__ void __launch_bounds__(kTexelBlock) k_texel_owner(const TriRec* __restrict__ tris, const TriUv* __restrict__ uvs, uint32_t first, uint32_t n, TexelLattice L,
                                                             const unsigned long long* __restrict__ off, const unsigned long long* __restrict__ total_p,
                                                             unsigned long long* __restrict__ owner) {
    const unsigned long long total = *total_p;
    const uint32_t lane = threadIdx.x & 63u;
    const unsigned long long waves = (unsigned long long)gridDim.x * (kTexelBlock / 64u), wave = (unsigned long long)blockIdx.x * (kTexelBlock / 64u) + (threadIdx.x >> 6);
    for (unsigned long long base = wave * 64ull; base < total; base += waves * 64ull) { // wave-uniform trip count
        const unsigned long long g = base + lane;
        uint32_t rec = 0u, tile = 0u;
        if (g < total) { // the last record whose items start at or before g: it has items (the records behind it that have none start where the next one does)
            uint32_t lo = 0u, hi = n;
            while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (off[mid] <= g) lo = mid + 1u; else hi = mid; }
            rec = lo - 1u; // (lo >= 1: off[0] = 0 <= g)
            tile = (uint32_t)(g - off[rec]);
        }
        const uint32_t items = total - base < 64ull ? (uint32_t)(total - base) : 64u;
        for (uint32_t k = 0; k < items; ++k) {
            const uint32_t r = first + (uint32_t)__shfl((int)rec, (int)k), tl = (uint32_t)__shfl((int)tile, (int)k); // wave-uniform
            const TexelUv t = texel_uv(uvs[r]);
            const double area2 = texel_area2(t);
            TexelBox b;
            if (area2 == 0.0 || !texel_box(t, L, b)) continue; // (never: the record has items)
            const uint32_t ntx = (b.x1 >> 3) - (b.x0 >> 3) + 1u;
            const uint32_t x = (((b.x0 >> 3) + tl % ntx) << 3) + (lane & 7u), y = (((b.y0 >> 3) + tl / ntx) << 3) + (lane >> 3);
            if (x < b.x0 || x > b.x1 || y < b.y0 || y > b.y1) continue; // (x1 < w, y1 < h: the owner index stays inside the lattice)
            double e0, e1, e2, sum;
            if (!texel_cover(t, area2, texel_coord(x, L.w, L.centres), texel_coord(y, L.h, L.centres), e0, e1, e2, sum)) continue;
            atomicMin(&owner[(size_t)y * L.w + x], ((unsigned long long)tris[r].tri_id << 32) | (unsigned long long)r);
        }
    }
}

// The resolve pass: one lane per lattice point.  A NULL output is not stored.
__global__ void __launch_bounds__(kTexelBlock) k_texel_resolve(const TriRec* __restrict__ tris, const TriUv* __restrict__ uvs, TexelLattice L, TexelXform X,
                                                               const unsigned long long* __restrict__ owner, TexelOutputs out) {
    const uint32_t i = blockIdx.x * kTexelBlock + threadIdx.x;
    if (i >= L.w * L.h) return;
    const unsigned long long key = owner[i];
    d3 p = D3(0, 0, 0), nm = D3(0, 0, 0);
    double su = 0.0, sv = 0.0;
    int32_t node = -1, prim = -1;
    uint32_t flags = 0u;
    if (key != kTexelUncovered) {
        const uint32_t r = (uint32_t)key;
        const TriRec tr = tris[r];
        const TexelUv t = texel_uv(uvs[r]);
        su = texel_coord(i % L.w, L.w, L.centres); sv = texel_coord(i / L.w, L.h, L.centres);
        double e0 = 0.0, e1 = 0.0, e2 = 0.0, sum = 1.0;
        (void)texel_cover(t, texel_area2(t), su, sv, e0, e1, e2, sum); // (covers: the owner pass ran the same function on the same values)
        const double w0 = e0 / sum, w1 = e1 / sum, w2 = e2 / sum;
        const d3 a = D3(tr.v0[0], tr.v0[1], tr.v0[2]), b = D3(tr.v1[0], tr.v1[1], tr.v1[2]), c = D3(tr.v2[0], tr.v2[1], tr.v2[2]);
        p = D3((a.x * w0 + b.x * w1) + c.x * w2, (a.y * w0 + b.y * w1) + c.y * w2, (a.z * w0 + b.z * w1) + c.z * w2);
        nm = normalize(cross(b - a, c - a));
        if (!(X.flags & kInstNoXform)) {
            if (X.flags & kInstIdentityRot) p = p + X.m.t;
            else { p = rot(X.m, p) + X.m.t; nm = rot(X.m, nm); }
        }
        if (X.flip) nm = -nm;
        node = (int32_t)L.node; prim = (int32_t)(key >> 32); flags = 3u;
    }
    out.points[3 * (size_t)i] = p.x; out.points[3 * (size_t)i + 1] = p.y; out.points[3 * (size_t)i + 2] = p.z;
    if (out.normals) { out.normals[3 * (size_t)i] = nm.x; out.normals[3 * (size_t)i + 1] = nm.y; out.normals[3 * (size_t)i + 2] = nm.z; }
    if (out.uv) { out.uv[2 * (size_t)i] = su; out.uv[2 * (size_t)i + 1] = sv; }
    if (out.node) out.node[i] = node;
    if (out.prim) out.prim[i] = prim;
    out.flags[i] = flags;
}

} // namespace nrays
