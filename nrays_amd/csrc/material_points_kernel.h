// material_points_kernel.h — k_material_points of nrays_material_points*: per caller-supplied surface point the terms of its node's material without the lights —
// Material::ambiant, the diffuse reflectance kd ⊙ texture, the specular constants — and the node's own constants (alpha, refl_mix, refl_atenuation, refr_coeff).
// The value is DEFINED by include/nrays_abi.h (nrays_material_points_device) and mirrored in numpy (nrays_amd.material_points_ref).
//
// One lane per point; the kernel strides by blocks.  A lane reads its node index and flag word, then its node's ShadeRec (lanes in surface order share it: mostly
// one address a wave), then — only for a PHONG material with a texture at a point that carries a uv — its uv and the taps of tex_sample, the sampler every
// material of the library goes through.  The colour texture is fetched ONCE for out_ambient and out_diffuse together (phong_terms below; material_ambiant
// itself is left as the renders call it and serves the NORMAL and UV materials here), and not at all when neither is stored.  A point that is not live stores
// zeros and reads neither its normal nor its uv.  out_ambient and out_specular are one 16-byte store a lane, out_node two.  No LDS, no scratch, no traversal
// stack, no counters (profiles/material_kres.txt).
#pragma once

#include "trace_device.h"

namespace nrays {

struct MaterialLaunch {
    uint32_t grid; hipStream_t stream; const ShadeRec* shade; uint32_t n, num_nodes; const double* normals; const double* uvs; const int32_t* nodes; const uint32_t* hit_flags;
    float* out_ambient; float* out_diffuse; float* out_specular; double* out_node;
};
// ray_batches.hip, beside k_shade_points.
void launch_material_points(const MaterialLaunch& a);

// What a PHONG material gives a point: Material::ambiant (phong_material.rs:39-70) and diffuse_color.component_mul(tex_color) (phong_material.rs:120-121) from ONE
// sample of the colour texture.  The ambient half is material_ambiant's PHONG branch, term for term.
NR_DEV void phong_terms(const ShadeRec& m, bool has_uv, double u, double v, bool want_ambient, bool want_diffuse, f4& ambient, f3& diffuse) {
    Cnt cnt; // (tex_sample<false> counts nothing)
    f4 tc; tc.x = tc.y = tc.z = tc.w = 1.0f;
    if (has_uv && m.tex.texels && (want_ambient || want_diffuse)) tc = tex_sample<false>(m.tex, u, v, cnt);
    diffuse = F3(m.kd[0] * tc.x, m.kd[1] * tc.y, m.kd[2] * tc.z);
    if (!want_ambient) return;
    if (has_uv) {
        tc.w = 1.0f;
        if (m.alpha_tex.texels) tc.w = tex_sample<false>(m.alpha_tex, u, v, cnt).w;
        ambient.x = m.ka[0] * tc.x; ambient.y = m.ka[1] * tc.y; ambient.z = m.ka[2] * tc.z; ambient.w = 1.0f * tc.w;
    } else { ambient.x = m.ka[0]; ambient.y = m.ka[1]; ambient.z = m.ka[2]; ambient.w = 1.0f; }
}

// (aligned(4): the caller's arrays are arrays of floats and doubles; the target stores a dwordx4 at any dword address)
typedef float mp_f4v __attribute__((ext_vector_type(4), aligned(4)));
typedef double mp_d2v __attribute__((ext_vector_type(2), aligned(8)));

__global__ void __launch_bounds__(kBlock) k_material_points(const ShadeRec* __restrict__ shade, uint32_t n, uint32_t num_nodes, const double* __restrict__ normals,
                                                            const double* __restrict__ uvs, const int32_t* __restrict__ nodes, const uint32_t* __restrict__ hit_flags,
                                                            float* __restrict__ out_ambient, float* __restrict__ out_diffuse, float* __restrict__ out_specular,
                                                            double* __restrict__ out_node) {
    for (uint32_t base = blockIdx.x * kBlock; base < n; base += gridDim.x * kBlock) { // block-uniform trip count (n <= 2^22: no overflow)
        const uint32_t i = base + threadIdx.x;
        if (i >= n) continue;
        const int32_t node = nodes[i];
        const uint32_t hf = hit_flags ? hit_flags[i] : 3u;
        f4 amb, spec; amb.x = amb.y = amb.z = amb.w = 0.0f; spec = amb;
        f3 dif = F3(0.0f, 0.0f, 0.0f);
        double nd[4] = {0.0, 0.0, 0.0, 0.0};
        if ((hf & 1u) && node >= 0 && (uint32_t)node < num_nodes) {
            const ShadeRec& m = shade[node];
            const bool has_uv = uvs != nullptr && (hf & 2u) != 0u;
            const double u = has_uv ? uvs[2 * (size_t)i] : 0.0, v = has_uv ? uvs[2 * (size_t)i + 1] : 0.0;
            if (((m.flags >> 8) & 0xffu) == NRAYS_MAT_PHONG) {
                phong_terms(m, has_uv, u, v, out_ambient != nullptr, out_diffuse != nullptr, amb, dif);
                spec.x = m.ks[0]; spec.y = m.ks[1]; spec.z = m.ks[2]; spec.w = m.shininess;
            } else if (out_ambient) {
                Cnt cnt;
                Isect is;
                is.toi = 0.0; is.hit = true; is.has_uv = has_uv; is.u = u; is.v = v;
                is.n = D3(normals[3 * (size_t)i], normals[3 * (size_t)i + 1], normals[3 * (size_t)i + 2]);
                amb = material_ambiant<false>(m, is, cnt);
            }
            nd[0] = (double)m.alpha; nd[1] = (double)m.refl_mix; nd[2] = (double)m.refl_atenuation; nd[3] = m.refr_coeff;
        }
        if (out_ambient) { mp_f4v q; q.x = amb.x; q.y = amb.y; q.z = amb.z; q.w = amb.w; *(mp_f4v*)(out_ambient + 4 * (size_t)i) = q; }
        if (out_diffuse) { float* o = out_diffuse + 3 * (size_t)i; o[0] = dif.x; o[1] = dif.y; o[2] = dif.z; }
        if (out_specular) { mp_f4v q; q.x = spec.x; q.y = spec.y; q.z = spec.z; q.w = spec.w; *(mp_f4v*)(out_specular + 4 * (size_t)i) = q; }
        if (out_node) {
            mp_d2v a, b; a.x = nd[0]; a.y = nd[1]; b.x = nd[2]; b.y = nd[3];
            mp_d2v* o = (mp_d2v*)(out_node + 4 * (size_t)i);
            o[0] = a; o[1] = b;
        }
    }
}

} // namespace nrays
