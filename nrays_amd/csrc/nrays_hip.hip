// nrays_hip.hip — the handle behind the C ABI of include/nrays_abi.h: its lifetime (nrays_scene_create / _destroy), what it reports
// (stats, tile costs, the debug probes), the blocking renders, and the last error.  The frame path lives in frame_path.hip, the rounds
// over the continuation queue in bounce.hip, the caller batches in ray_batches.hip, point_batches.hip and texel_calls.hip (their driver: batch_call.cpp; their reorder: ray_order.hip), the staged path in wavefront.hip.
//   k_quantize_rgb8  a finished frame as 8-bit RGB (nrays_render_rgb8).
//   k_untile         un-permutes gathered multi-GPU tile buffers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/nrays_abi.h"
#include "device_types.h"
#include "primary_kernel.h"
#include "scene_build.h"
#include "scene_handle.h"
#include "trace_device.h"
#include "wavefront.h"

namespace nrays {

// Image::to_png quantisation (src/image.rs:66-76) of a finished frame: c * 255, clamped to [0, 255], truncated; NaN and
// negatives -> 0 (Rust's saturating `as u8`).  Same f32 operations as the host front-end's quantize_rgb8 (png_codec.cpp).
__global__ void k_quantize_rgb8(const float* __restrict__ rgb, uint8_t* __restrict__ out, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float v = rgb[i] * 255.0f;
    v = (v > 0.0f) ? v : 0.0f;
    v = v > 255.0f ? 255.0f : v;
    out[i] = (uint8_t)(uint32_t)v;
}

__global__ void k_untile(const float* __restrict__ gathered, float* __restrict__ out, uint32_t width, uint32_t height,
                         uint32_t band_rows, uint32_t owners, uint32_t rows_local) {
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t n = (size_t)width * height * 3;
    if (idx >= n) return;
    uint32_t c = (uint32_t)(idx % 3);
    size_t p = idx / 3;
    uint32_t i = (uint32_t)(p % width), j = (uint32_t)(p / width);
    uint32_t band = j / band_rows, owner = band % owners, lb = band / owners;
    uint32_t rl = lb * band_rows + (j % band_rows);
    out[idx] = gathered[((size_t)owner * rows_local + rl) * width * 3 + (size_t)i * 3 + c];
}

// =============================================================================================
// host side
// =============================================================================================
static thread_local std::string g_last_error;
static int fail(int status, const std::string& msg) { g_last_error = msg; return status; }
int set_last_error(int status, const std::string& msg) { return fail(status, msg); } // for the library's other translation units

int ensure_spill(const NraysScene* sc, uint32_t** region) {
    if (sc->facts.spill_entries && !*region) HIP_TRY(hipMalloc((void**)region, (size_t)kMaxGrid * kBlock * sc->facts.spill_entries * sizeof(uint32_t)));
    return NRAYS_OK;
}
int ensure_own_stream(NraysScene* sc) {
    if (!sc->buf.own_stream) HIP_TRY(hipStreamCreate(&sc->buf.own_stream));
    return NRAYS_OK;
}
int grow_device(void** buffer, size_t* have, size_t want, size_t elem) {
    if (want <= *have) return NRAYS_OK;
    if (*buffer) { (void)hipFree(*buffer); *buffer = nullptr; *have = 0; }
    HIP_TRY(hipMalloc(buffer, want * elem));
    *have = want;
    return NRAYS_OK;
}
int order_behind_stream(NraysScene* sc, hipStream_t prev, hipStream_t stream) {
    if (!sc->last.ev_switch) HIP_TRY(hipEventCreateWithFlags(&sc->last.ev_switch, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(sc->last.ev_switch, prev));
    HIP_TRY(hipStreamWaitEvent(stream, sc->last.ev_switch, 0));
    return NRAYS_OK;
}

// ---- scene creation, in phases (nrays_scene_create is the driver below) ---------------------------------------------------------------
// Every phase works on the handle `sc` whose sw (the switches) and facts.host (build_host_scene's result) are complete, and returns NRAYS_OK or an error
// that ends the creation.  The header of each names what it reads and what it sets.  Their order is the order of the HIP calls of a creation
// (tools/cold_probe.py and the bench's cold figure measure this path).

// NRAYS_BUILD_TIMES: where nrays_scene_create spends its time.
struct StageClock {
    bool on; std::chrono::steady_clock::time_point t;
    void mark(const char* what) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        fprintf(stderr, "  nrays_scene_create: %s %.2f ms\n", what, std::chrono::duration<double, std::milli>(now - t).count());
        t = now;
    }
};

// Device-built segments first (device-to-device), then the host-built part: the layout HostScene's refs address.
template <typename T>
static int upload_joined(NraysScene* sc, const std::vector<std::pair<const T*, size_t>>& segs, const std::vector<T>& v, const T** out) {
    *out = nullptr;
    size_t total = v.size();
    for (const auto& s : segs) total += s.second;
    if (total == 0) return NRAYS_OK;
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, total * sizeof(T)));
    sc->facts.allocs.push_back(p);
    sc->facts.scene_bytes += total * sizeof(T);
    size_t at = 0;
    for (const auto& s : segs) { if (s.second) HIP_TRY(hipMemcpy((T*)p + at, s.first, s.second * sizeof(T), hipMemcpyDeviceToDevice)); at += s.second; }
    if (!v.empty()) HIP_TRY(hipMemcpy((T*)p + at, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    *out = (const T*)p;
    return NRAYS_OK;
}
template <typename T>
static int upload(NraysScene* sc, const std::vector<T>& v, const T** out) { return upload_joined<T>(sc, {}, v, out); }

// Reads host.dev_blas (released or adopted here), host.nodes / tris / triuvs.  Sets d.nodes, d.tris, d.triuvs; facts.allocs, facts.scene_bytes.
static int upload_bvh_arrays(NraysScene* sc) {
    HostScene& h = sc->facts.host; DScene& d = sc->facts.d;
    if (h.dev_blas.size() == 1 && h.tris.empty() && h.triuvs.empty() && h.dev_blas[0].nodes && h.dev_blas[0].num_nodes + h.nodes.size() <= h.dev_blas[0].node_capacity) {
        // ONE device-built BLAS and nothing but TLAS nodes from the host (a single large mesh): the builder's arrays ARE the scene's arrays — the host
        // nodes go into the spare slots behind the BLAS; no second allocation, no copy and no release of gigabytes (0.2 s for the hairball stand-in)
        DeviceBlas& b = h.dev_blas[0];
        if (!h.nodes.empty() && hipMemcpy(b.nodes + b.num_nodes, h.nodes.data(), h.nodes.size() * sizeof(BvhNode), hipMemcpyHostToDevice) != hipSuccess)
            return fail(NRAYS_ERR_HIP, "upload of the TLAS nodes failed");
        d.nodes = b.nodes; d.tris = b.tris; d.triuvs = b.uvs;
        sc->facts.allocs.push_back(b.nodes); sc->facts.allocs.push_back(b.tris); sc->facts.allocs.push_back(b.uvs);
        sc->facts.scene_bytes += (b.num_nodes + h.nodes.size()) * sizeof(BvhNode) + b.num_refs * (sizeof(TriRec) + sizeof(TriUv));
        b.nodes = nullptr; b.tris = nullptr; b.uvs = nullptr;
        h.dev_blas.clear();
        return NRAYS_OK;
    }
    std::vector<std::pair<const BvhNode*, size_t>> nseg; std::vector<std::pair<const TriRec*, size_t>> tseg; std::vector<std::pair<const TriUv*, size_t>> useg;
    for (const DeviceBlas& b : h.dev_blas) { nseg.push_back({b.nodes, b.num_nodes}); tseg.push_back({b.tris, b.num_refs}); useg.push_back({b.uvs, b.num_refs}); }
    int rc = upload_joined(sc, nseg, h.nodes, &d.nodes);
    if (rc == NRAYS_OK) rc = upload_joined(sc, tseg, h.tris, &d.tris);
    if (rc == NRAYS_OK) rc = upload_joined(sc, useg, h.triuvs, &d.triuvs);
    if (rc != NRAYS_OK) return rc;
    for (DeviceBlas& b : h.dev_blas) free_device_blas(b);
    h.dev_blas.clear();
    return NRAYS_OK;
}

// The scene's small record arrays: ONE allocation and ONE copy (eight synchronous hipMalloc + hipMemcpy pairs before).
// Reads host.instances .. shadow_planes.  Sets the eight record pointers of d; facts.allocs, facts.scene_bytes.
static int upload_record_block(NraysScene* sc) {
    const HostScene& h = sc->facts.host; DScene& d = sc->facts.d;
    struct Part { const void* src; size_t bytes; const void** out; size_t at; };
    std::vector<Part> parts;
    size_t total = 0;
    auto add = [&](const auto& v, auto** out) {
        *out = nullptr;
        if (v.empty()) return;
        total = (total + 255u) & ~(size_t)255u;
        parts.push_back(Part{v.data(), v.size() * sizeof(v[0]), (const void**)out, total});
        total += v.size() * sizeof(v[0]);
    };
    add(h.instances, &d.instances); add(h.shadow_instances, &d.shadow_instances); add(h.links, &d.links); add(h.shadow_links, &d.shadow_links);
    add(h.node_aabbs, &d.node_aabbs); add(h.lights, &d.lights); add(h.planes, &d.planes); add(h.shadow_planes, &d.shadow_planes);
    if (!total) return NRAYS_OK;
    void* blk = nullptr;
    if (hipMalloc(&blk, total) != hipSuccess) return fail(NRAYS_ERR_OOM, "record allocation failed");
    sc->facts.allocs.push_back(blk); sc->facts.scene_bytes += total;
    std::vector<char> stage(total);
    for (const Part& pt : parts) { std::memcpy(stage.data() + pt.at, pt.src, pt.bytes); *pt.out = (const char*)blk + pt.at; }
    if (hipMemcpy(blk, stage.data(), total, hipMemcpyHostToDevice) != hipSuccess) return fail(NRAYS_ERR_HIP, "record upload failed");
    return NRAYS_OK;
}

// Nodes, triangles and uvs, the joined record block, the textures, the shading records (with the textures' device pointers patched in).
// Reads facts.host.  Sets every array pointer of facts.d except lds_blob and tiny (d is zeroed first); facts.allocs, facts.scene_bytes.
static int upload_scene_arrays(NraysScene* sc) {
    HostScene& h = sc->facts.host;
    std::memset(&sc->facts.d, 0, sizeof sc->facts.d);
    int rc = upload_bvh_arrays(sc);
    if (rc == NRAYS_OK) rc = upload_record_block(sc);
    if (rc != NRAYS_OK) return rc;
    std::vector<TextureRec> trecs;
    for (const HostTexture& t : h.textures) { // (the host copies of the texels stay until derive_scene_facts has looked at them)
        void* p = nullptr;
        if (hipMalloc(&p, t.bytes.size()) != hipSuccess) return fail(NRAYS_ERR_OOM, "texture allocation failed");
        sc->facts.allocs.push_back(p);
        sc->facts.scene_bytes += t.bytes.size();
        if (hipMemcpy(p, t.bytes.data(), t.bytes.size(), hipMemcpyHostToDevice) != hipSuccess) return fail(NRAYS_ERR_HIP, "texture upload failed");
        TextureRec r = t.rec; r.texels = p; trecs.push_back(r);
    }
    for (size_t i = 0; i < h.shade.size(); ++i) { // patch the device texel pointers into the per-node shading records
        if (h.shade_tex[i] >= 0) h.shade[i].tex.texels = trecs[h.shade_tex[i]].texels;
        if (h.shade_alpha_tex[i] >= 0) h.shade[i].alpha_tex.texels = trecs[h.shade_alpha_tex[i]].texels;
    }
    return upload(sc, h.shade, &sc->facts.d.shade);
}

// The elisions (trace_device.h: light_is_dark, shade_hit) need x * 0 == 0 for everything they skip: any non-finite light, material colour or float texel, or a
// negative shininess (0 * inf), switches them off for the scene (phong_material.rs:109-141, scene.rs:179-190 then produce NaN, and so do we).
static bool scene_is_finite(const HostScene& h) {
    bool finite = true;
    for (const LightRec& l : h.lights) { for (int a = 0; a < 3; ++a) finite = finite && std::isfinite(l.pos[a]) && std::isfinite(l.color[a]); finite = finite && std::isfinite(l.radius); }
    for (const ShadeRec& m : h.shade) {
        for (int a = 0; a < 3; ++a) finite = finite && std::isfinite(m.ka[a]) && std::isfinite(m.kd[a]) && std::isfinite(m.ks[a]);
        finite = finite && std::isfinite(m.shininess) && m.shininess >= 0.0f && std::isfinite(m.alpha) && std::isfinite(m.refl_mix) && std::isfinite(m.refl_atenuation) && std::isfinite(m.refr_coeff);
    }
    for (const HostTexture& t : h.textures) {
        if (t.rec.format != NRAYS_TEXEL_RGBA32F) continue;
        const float* f = (const float*)t.bytes.data();
        for (size_t i = 0, n = t.bytes.size() / sizeof(float); i < n && finite; ++i) finite = std::isfinite(f[i]);
    }
    for (int a = 0; a < 3; ++a) finite = finite && std::isfinite(h.background[a]);
    return finite;
}

// What follows from the scene and the switches alone: no HIP call except the query of the CU count.
// Reads facts.host, facts.device, sw.  Sets d.no_elide, d.incoherent, the roots, counts and background of d; facts.spill_entries, num_cus, features, noxform,
// park, light_lsl; the defaults that depend on the scene or on another switch: order.near_pixels, order.max_order_age, pipe.enabled, pipe.slots, pipe.lead_wgs, buf.count_rot.
static void derive_scene_facts(NraysScene* sc) {
    const HostScene& h = sc->facts.host; const Switches& sw = sc->sw; DScene& d = sc->facts.d;
    d.no_elide = (!scene_is_finite(h) || !sw.elide) ? 1u : 0u;
    // (such a scene's frames are rendered by the instrumented kernel, which does not decode the split entries of a cost-ordered list: no light-parallel / pixel-split tiles — light_lsl stays 0 below)
    d.closest_root = h.closest_root; d.shadow_root = h.shadow_root;
    d.num_planes = (uint32_t)h.planes.size(); d.num_lights = (uint32_t)h.lights.size();
    for (int a = 0; a < 3; ++a) d.background[a] = h.background[a];
    d.incoherent = h.any_incoherent && sw.node_quorum ? 1u : 0u; // quorum-ended node phases for hair-like meshes
    // worst-case stack use: up to 3 deferred siblings per level of TLAS + BLAS (max_bvh_depth bounds each),
    // one sentinel, the plane pseudo-leaves, a little slack; whatever exceeds the LDS part spills to HBM
    const uint32_t need = 6u * (uint32_t)(h.max_bvh_depth + 1) + (uint32_t)h.planes.size() + 9u; // + the bottom marker
    sc->facts.spill_entries = need > (uint32_t)kLdsStack ? need - (uint32_t)kLdsStack : 0u;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, sc->facts.device) == hipSuccess && cus > 0) sc->facts.num_cus = cus;
    const int f = sc->facts.features = h.features ? h.features : kFeatAll;
    // kFeatNoXform: scenes of TriMesh nodes only whose BLASes all sit in world space
    bool all = (f == 2 || f == 6 || f == 18 || f == 22) && !h.links.empty();
    for (const InstLink& l : h.links) all = all && (l.flags & kInstNoXform);
    for (const InstLink& l : h.shadow_links) all = all && (l.flags & kInstNoXform);
    sc->facts.noxform = all && sw.noxform;
    sc->facts.park = sw.park;
    // multi-light mesh scenes without double branching: 2, 4 or 8 lanes per pixel in a split tile
    if (d.no_elide) sc->facts.light_lsl = 0;
    else if ((f & kFeatMultiSample) && (f & kFeatMesh) && !(f & kFeatDouble) && h.lights.size() >= 2) { uint32_t l = 1; while (l < 3u && (2u << l) <= h.lights.size()) ++l; sc->facts.light_lsl = l; }
    else if (NR_PIXEL_SPLIT && !(f & kFeatMultiSample) && (f & kFeatMesh) && (f & kFeatAlphaShadow) && !(f & kFeatDouble)) sc->facts.light_lsl = 3; // pixel split: 8 pixels per part
    // Mesh scenes re-sort on every frame of a moving camera (age 0): the deep foliage chains of the sponza stand-in move between tiles with every pixel of camera motion, and a
    // frame that reuses an order a few frames old waits for tiles it started late — 1.20 ms against 1.145 with the previous frame's costs, 1.04 at rest
    // (profiles/r06_regimes_sweep.log).  Analytic scenes keep an order for 16 frames of a camera within two blocks (balls, moving: 0.0576 ms at 8 frames / 16 pixels,
    // 0.0565 at 16 / 64, 0.0550 with an order that is never refreshed; 0.049 at rest).
    sc->order.near_pixels = sw.near_pixels.value_or(h.any_mesh ? kNearPixels : 2.0 * kNearPixels);
    sc->order.max_order_age = sw.max_order_age.value_or(h.any_mesh ? 0u : 16u);
    sc->pipe.enabled = sw.pipeline;
    sc->pipe.slots = sw.pipe_depth == 3 ? 6 : 4; sc->buf.count_rot = sc->pipe.slots; // (depth 2: the rotation and the slots of the two-stream pipeline)
    sc->pipe.lead_wgs = sw.pipe_lead_wgs.value_or(sw.pipe_depth < 3);
}

// Small analytic scenes: one packed copy of the records for the kernels that read them from LDS (DScene::lds_blob).  Not when NRAYS_LDS_SCENE=0, for other
// scenes, or when the copy exceeds kLdsSceneBytes.  Reads facts.host, facts.features, sw.lds_scene.  Sets d.lds_blob, d.lds_bytes, d.lds_off; adds kFeatLdsScene to facts.features.
static int upload_lds_scene(NraysScene* sc) {
    const HostScene& h = sc->facts.host; DScene& d = sc->facts.d;
    d.lds_blob = nullptr; d.lds_bytes = 0;
    const int f = sc->facts.features;
    if (!(f == 1 || f == 5 || f == 17 || f == 21) || !sc->sw.lds_scene) return NRAYS_OK;
    std::vector<uint8_t> blob;
    auto section = [&](int k, const void* q, size_t n) { // 16-byte aligned sections
        blob.resize((blob.size() + 15u) & ~(size_t)15u);
        d.lds_off[k] = (uint32_t)blob.size();
        const uint8_t* b = (const uint8_t*)q;
        blob.insert(blob.end(), b, b + n);
    };
    section(kLdsNodes, h.nodes.data(), h.nodes.size() * sizeof(BvhNode));
    section(kLdsInstances, h.instances.data(), h.instances.size() * sizeof(Instance));
    section(kLdsShadowInstances, h.shadow_instances.data(), h.shadow_instances.size() * sizeof(Instance));
    section(kLdsLinks, h.links.data(), h.links.size() * sizeof(InstLink));
    section(kLdsShadowLinks, h.shadow_links.data(), h.shadow_links.size() * sizeof(InstLink));
    section(kLdsShade, h.shade.data(), h.shade.size() * sizeof(ShadeRec));
    section(kLdsNodeAabbs, h.node_aabbs.data(), h.node_aabbs.size() * sizeof(double));
    section(kLdsLights, h.lights.data(), h.lights.size() * sizeof(LightRec));
    section(kLdsPlanes, h.planes.data(), h.planes.size() * sizeof(int32_t));
    section(kLdsShadowPlanes, h.shadow_planes.data(), h.shadow_planes.size() * sizeof(int32_t));
    blob.resize((blob.size() + 15u) & ~(size_t)15u);
    if (blob.empty() || blob.size() > kLdsSceneBytes) return NRAYS_OK;
    std::vector<uint32_t> words(blob.size() / 4);
    std::memcpy(words.data(), blob.data(), blob.size());
    const int rc = upload(sc, words, &d.lds_blob);
    if (rc != NRAYS_OK) return rc;
    d.lds_bytes = (uint32_t)blob.size();
    sc->facts.features |= kFeatLdsScene;
    return NRAYS_OK;
}

// Opaque analytic scenes of at most kTinyLeaves TLAS leaves (planes included) with their records in LDS: one TinyLeaf per leaf of each TLAS for the
// stackless queries of the kFeatTinyScene kernels (trace_device.h: tiny_closest, tiny_shadow).  Pixels do not depend on it (NRAYS_TINY_SCENE=0: the TLAS walk, A/B).
// Reads facts.host, facts.features (after upload_lds_scene), sw.tiny_scene.  Sets d.tiny, d.tiny_n, d.tiny_shadow_n, facts.tiny.
static int upload_tiny_leaves(NraysScene* sc) {
    const HostScene& h = sc->facts.host; DScene& d = sc->facts.d;
    d.tiny = nullptr; d.tiny_n = d.tiny_shadow_n = 0u;
    const int f = sc->facts.features;
    if (!((f == (kFeatAnalytic | kFeatLdsScene) || f == (kFeatAnalytic | kFeatMultiSample | kFeatLdsScene)) && !h.instances.empty() &&
          h.instances.size() <= kTinyLeaves && h.shadow_instances.size() <= kTinyLeaves && sc->sw.tiny_scene)) return NRAYS_OK;
    std::vector<TinyLeaf> leaves;
    auto add = [&](const std::vector<Instance>& insts) {
        for (size_t k = 0; k < insts.size(); ++k) {
            const Instance& in = insts[k];
            TinyLeaf lf{};
            lf.kind = in.kind; lf.flags = in.flags; lf.node_id = in.node_id; lf.inst = (uint32_t)k;
            lf.radius = in.params[0];
            for (int a = 0; a < 3; ++a) lf.center[a] = in.trans[a];
            if (in.node_id >= 0 && 6 * (size_t)in.node_id + 6 <= h.node_aabbs.size())
                for (int a = 0; a < 6; ++a) lf.aabb[a] = h.node_aabbs[6 * (size_t)in.node_id + a];
            leaves.push_back(lf);
        }
    };
    add(h.instances); add(h.shadow_instances);
    const int rc = upload(sc, leaves, &d.tiny);
    if (rc != NRAYS_OK) return rc;
    d.tiny_n = (uint32_t)h.instances.size(); d.tiny_shadow_n = (uint32_t)h.shadow_instances.size();
    sc->facts.tiny = true;
    return NRAYS_OK;
}

// k_seed_costs: world AABBs of the nodes that can continue a chain (transparent / alpha-mapped / reflective), as f32.  A scene without such a node uploads nothing.
// Reads facts.host.  Sets facts.d_seed_boxes, facts.seed_boxes.
static int upload_seed_boxes(NraysScene* sc) {
    const HostScene& h = sc->facts.host;
    std::vector<float> boxes;
    for (size_t i = 0; i < h.shade.size() && boxes.size() < 6u * 2048u; ++i) {
        const ShadeRec& sr = h.shade[i];
        if (!(sr.alpha < 1.0f || h.shade_alpha_tex[i] >= 0 || sr.refl_mix != 0.0f)) continue;
        const double* b = h.node_aabbs.data() + 6 * i;
        bool finite = true;
        for (int a = 0; a < 6; ++a) finite = finite && std::isfinite(b[a]) && std::fabs(b[a]) < 1e30;
        if (!finite) continue;
        for (int a = 0; a < 6; ++a) boxes.push_back((float)b[a]);
    }
    // (scenes without such a node — opaque hair — get no guess: a frame in image order.  Their nodes' boxes priced by the chord a ray spends inside, round 6: hairball
    // cold frame 2.18 ms against 2.13 without — the order it buys is worth less than the two launches it costs: profiles/r06_regimes_sweep.log)
    const float* dptr = nullptr;
    const int rc = upload(sc, boxes, &dptr);
    if (rc != NRAYS_OK) return rc;
    sc->facts.d_seed_boxes = dptr; sc->facts.seed_boxes = (uint32_t)(boxes.size() / 6);
    return NRAYS_OK;
}

// The handle's own device state: the rotating counter sets, the cost meta words, the primary-kernel counter snapshot, and what a first frame would allocate
// (preallocate_first_frame, unless NRAYS_PREALLOC=0).  Reads sw.prealloc and what preallocate_first_frame reads.  Sets buf.d_counts_set, d_counters_set, d_counts,
// d_counters; order.d_cost_meta; ring.d_counters_primary; the first-frame buffers of buf, order, ring and last.
static int allocate_handle_state(NraysScene* sc, StageClock& clock) {
    for (int k = 0; k < NraysScene::kCountSets; ++k) {
        if (hipMalloc((void**)&sc->buf.d_counts_set[k], kNumCounts * sizeof(uint32_t)) != hipSuccess ||
            hipMalloc((void**)&sc->buf.d_counters_set[k], sizeof(DeviceCounters)) != hipSuccess)
            return fail(NRAYS_ERR_OOM, "counter allocation failed");
        if (hipMemset(sc->buf.d_counts_set[k], 0, kNumCounts * sizeof(uint32_t)) != hipSuccess ||
            hipMemset(sc->buf.d_counters_set[k], 0, sizeof(DeviceCounters)) != hipSuccess)
            return fail(NRAYS_ERR_HIP, "counter memset failed");
    }
    sc->buf.d_counts = sc->buf.d_counts_set[0]; sc->buf.d_counters = sc->buf.d_counters_set[0];
    if (hipMalloc((void**)&sc->order.d_cost_meta, 4 * sizeof(unsigned long long)) != hipSuccess || hipMemset(sc->order.d_cost_meta, 0, 4 * sizeof(unsigned long long)) != hipSuccess)
        return fail(NRAYS_ERR_OOM, "cost-meta allocation failed");
    clock.mark("records, switches, counters");
    if (hipMalloc((void**)&sc->ring.d_counters_primary, sizeof(DeviceCounters)) != hipSuccess)
        return fail(NRAYS_ERR_OOM, "counter allocation failed");
    // the stamps of timed pipelined frames (scene_handle.h: Ring::d_stamps): zeroed once, never cleared afterwards
    if (sc->sw.lean_stamps && (hipMalloc((void**)&sc->ring.d_stamps, (size_t)NraysScene::kRing * NraysScene::kStampBlock * sizeof(unsigned long long)) != hipSuccess ||
                               hipMemset(sc->ring.d_stamps, 0, (size_t)NraysScene::kRing * NraysScene::kStampBlock * sizeof(unsigned long long)) != hipSuccess))
        return fail(NRAYS_ERR_OOM, "stamp allocation failed");
    // (own_stream is created by the first entry point that needs it, ensure_own_stream(): a handle that is only ever rendered on the caller's streams leaves its
    // hardware queue to the internal streams of the pipelined frames — a stream that exists holds a queue, and a process has four)
    // (the ring's timing events are created by the first frame that records into a slot: 1 024 hipEventCreate cost 0.6 ms of every scene creation)
    clock.mark("stream + event ring");
    if (sc->sw.prealloc) preallocate_first_frame(sc);
    clock.mark("first-frame buffers");
    return NRAYS_OK;
}

} // namespace nrays

using namespace nrays;

extern "C" {

uint32_t nrays_abi_version(void) { return NRAYS_ABI_VERSION; }
const char* nrays_last_error(void) { return g_last_error.c_str(); }
uint32_t nrays_tile_rows(const NraysRenderParams* params) { return params ? tile_rows(params) : 0; }
uint64_t nrays_scene_device_bytes(const NraysScene* scene) { return scene ? scene->facts.scene_bytes : 0; }

// The driver: switches, host scene, then the phases above in the order of their HIP calls.
int nrays_scene_create(const NraysSceneDesc* desc, NraysScene** out_scene) {
    if (!desc || !out_scene) return fail(NRAYS_ERR_BAD_ARG, "null argument");
    *out_scene = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(NRAYS_ERR_NO_DEVICE, "no HIP device visible");
    NraysScene* sc = new (std::nothrow) NraysScene();
    if (!sc) return fail(NRAYS_ERR_OOM, "host allocation failed");
    auto bail = [&](int rc) { nrays_scene_destroy(sc); return rc; };
    if (hipGetDevice(&sc->facts.device) != hipSuccess) return bail(fail(NRAYS_ERR_HIP, "hipGetDevice failed"));
    sc->sw = read_switches();
    HostScene& h = sc->facts.host;
    std::string err;
    const auto t_create0 = std::chrono::steady_clock::now();
    StageClock clock{sc->sw.build_times, t_create0};
    int rc = build_host_scene(desc, sc->sw, h, err);
    clock.mark("build_host_scene (BLAS + TLAS builds)");
    if (rc != NRAYS_OK) return bail(fail(rc, err));
    const auto t_create1 = std::chrono::steady_clock::now();
    if ((rc = upload_scene_arrays(sc)) != NRAYS_OK) return bail(rc);
    clock.mark("uploads (nodes, triangles, records, textures)");
    if (sc->sw.build_times && h.tris.size() + h.dev_tris > 1000000)
        fprintf(stderr, "  nrays_scene_create: build_host_scene %.2f s, uploads %.2f s\n", std::chrono::duration<double>(t_create1 - t_create0).count(),
                std::chrono::duration<double>(std::chrono::steady_clock::now() - t_create1).count());
    derive_scene_facts(sc);
    if ((rc = upload_lds_scene(sc)) != NRAYS_OK || (rc = upload_tiny_leaves(sc)) != NRAYS_OK || (rc = upload_seed_boxes(sc)) != NRAYS_OK) return bail(rc);
    sc->facts.num_nodes = h.dev_nodes + h.nodes.size(); sc->facts.num_tris = h.dev_tris + h.tris.size();
    // release bulk host copies
    std::vector<BvhNode>().swap(h.nodes); std::vector<TriRec>().swap(h.tris); std::vector<TriUv>().swap(h.triuvs);
    for (HostTexture& t : h.textures) std::vector<uint8_t>().swap(t.bytes);
    if ((rc = allocate_handle_state(sc, clock)) != NRAYS_OK) return bail(rc);
    *out_scene = sc;
    return NRAYS_OK;
}

// Frees the handle group by group, behind its last work.
void nrays_scene_destroy(NraysScene* sc) {
    if (!sc) return;
    (void)hipSetDevice(sc->facts.device);
    if (sc->last.have) (void)hipStreamSynchronize(sc->last.stream); // (the compose of every pipelined frame is there or ordered before it, behind its trace)
    pipeline_release(sc); // pipe
    // facts
    for (void* p : sc->facts.allocs) (void)hipFree(p);
    for (DeviceBlas& b : sc->facts.host.dev_blas) free_device_blas(b); // a creation that failed between the build and the upload
    // buf (own_stream last, below)
    for (int k = 0; k < 2; ++k) if (sc->buf.queue[k].block) (void)hipFree(sc->buf.queue[k].block);
    for (int k = 0; k < NraysScene::kCountSets; ++k) {
        if (sc->buf.d_counts_set[k]) (void)hipFree(sc->buf.d_counts_set[k]);
        if (sc->buf.d_counters_set[k]) (void)hipFree(sc->buf.d_counters_set[k]);
    }
    for (void* q : {(void*)sc->buf.d_spill, (void*)sc->buf.d_fixed, (void*)sc->buf.d_frame, (void*)sc->buf.d_rgb8}) if (q) (void)hipFree(q);
    // order
    for (void* q : {(void*)sc->order.d_tile_cost, (void*)sc->order.d_tile_order, (void*)sc->order.d_order_len, (void*)sc->order.d_cost_stats, (void*)sc->order.d_cost_meta}) if (q) (void)hipFree(q);
    if (sc->order.h_cost_stats) (void)hipHostFree(sc->order.h_cost_stats);
    if (sc->order.ev_stats) (void)hipEventDestroy(sc->order.ev_stats);
    for (int k = 0; k < 2; ++k) if (sc->order.ev_rec[k]) (void)hipEventDestroy(sc->order.ev_rec[k]);
    // ring
    if (sc->ring.d_counters_primary) (void)hipFree(sc->ring.d_counters_primary);
    if (sc->ring.d_stamps) (void)hipFree(sc->ring.d_stamps);
    for (int k = 0; k < NraysScene::kRing; ++k)
        for (hipEvent_t e : {sc->ring.ev_begin[k], sc->ring.ev_pbegin[k], sc->ring.ev_pend[k], sc->ring.ev_end[k]}) if (e) (void)hipEventDestroy(e);
    // last
    if (sc->last.ev_switch) (void)hipEventDestroy(sc->last.ev_switch);
    wavefront_release(sc);
    trace_workspace_release(sc);
    if (sc->buf.own_stream) (void)hipStreamDestroy(sc->buf.own_stream);
    delete sc;
}

int nrays_render_device(NraysScene* scene, const NraysRenderParams* params, float* out_rgb_device, void* hip_stream) {
    return render_impl(scene, params, out_rgb_device, (hipStream_t)hip_stream, false);
}

int nrays_render_device_instrumented(NraysScene* scene, const NraysRenderParams* params, float* out_rgb_device, void* hip_stream) {
    return render_impl(scene, params, out_rgb_device, (hipStream_t)hip_stream, true);
}

int nrays_render_device_counted(NraysScene* scene, const NraysRenderParams* params, float* out_rgb_device, void* hip_stream, uint32_t flags) {
    if (flags & ~NRAYS_COUNT_AS_TIMED) return fail(NRAYS_ERR_BAD_ARG, "unknown count flags");
    return render_impl(scene, params, out_rgb_device, (hipStream_t)hip_stream, true, flags);
}

static void fill_counters(NraysStats* out, const DeviceCounters& c) {
    out->rays_reflection = c.rays_reflection; out->rays_refraction = c.rays_refraction; out->rays_shadow = c.rays_shadow;
    out->node_tests = c.node_tests; out->tri_tests = c.tri_tests; out->prim_tests = c.prim_tests;
    out->hit_records = c.hit_records; out->tex_samples = c.tex_samples; out->rays_primary_traced = c.rays_primary_traced; out->node_fetches = c.node_fetches;
}

int nrays_get_stats(NraysScene* sc, NraysStats* out) {
    if (!sc || !out) return fail(NRAYS_ERR_BAD_ARG, "null argument");
    std::memset(out, 0, sizeof *out);
    if (!sc->last.have) return NRAYS_OK;
    HIP_TRY(hipSetDevice(sc->facts.device));
    HIP_TRY(hipStreamSynchronize(sc->last.stream));
    DeviceCounters c;
    HIP_TRY(hipMemcpy(&c, sc->buf.d_counters, sizeof c, hipMemcpyDeviceToHost));
    out->rays_primary = sc->last.primary;
    fill_counters(out, c);
    out->generations = c.max_depth; out->instrumented = sc->last.instrumented ? 1u : 0u;
    out->reserved = c.max_chain_nodes; // instrumented renders: most AABB tests spent on one pixel's whole chain
    out->rays_shadow_elided = c.shadow_elided;
    // average the event timings of the frames recorded since the previous call (at most kRing)
    uint64_t first = sc->ring.frames_reported;
    if (sc->ring.frames_recorded - first > (uint64_t)NraysScene::kRing) first = sc->ring.frames_recorded - NraysScene::kRing;
    double sum_p = 0.0, sum_t = 0.0; uint64_t n = 0;
    // (timed pipelined frames left 100 MHz ticks instead of events — trace start, trace end, compose end: the whole array in one copy, behind the synchronisation above)
    std::vector<unsigned long long> stamps;
    for (uint64_t f = first; f < sc->ring.frames_recorded && stamps.empty(); ++f)
        if (sc->ring.timed_by[f % NraysScene::kRing] == NraysScene::Ring::kByStamps && sc->ring.d_stamps) {
            stamps.resize((size_t)NraysScene::kRing * NraysScene::kStampBlock);
            HIP_TRY(hipMemcpy(stamps.data(), sc->ring.d_stamps, stamps.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        }
    for (uint64_t f = first; f < sc->ring.frames_recorded; ++f) {
        int k = (int)(f % NraysScene::kRing);
        float ms_p = 0.f, ms_t = 0.f;
        if (sc->ring.timed_by[k] != NraysScene::Ring::kByEvents) { // a slot whose end is not later than its start is skipped, like an event pair that is not ready
            const unsigned long long* w = stamps.empty() ? nullptr : &stamps[(size_t)NraysScene::kStampBlock * (size_t)k];
            // the compose's end: its third word, or the latest of the words its rows shared (a handle uses one of the two for life, the other stays 0; stale ticks of a slot's earlier use are older and lose)
            unsigned long long end = w ? w[2] : 0ull;
            if (w && sc->sw.host_stamps) for (uint32_t j = 0; j < nrays::kStampWords; ++j) end = std::max(end, w[nrays::kStampHead + j]);
            if (sc->ring.timed_by[k] == NraysScene::Ring::kByStamps && w && w[1] > w[0] && end >= w[1]) { sum_p += (double)(w[1] - w[0]) * 1e-5; sum_t += (double)(end - w[0]) * 1e-5; ++n; }
            continue;
        }
        if (hipEventElapsedTime(&ms_p, sc->ring.ev_pbegin[k], sc->ring.ev_pend[k]) == hipSuccess &&
            hipEventElapsedTime(&ms_t, sc->ring.has_prepass[k] ? sc->ring.ev_begin[k] : sc->ring.ev_pbegin[k], sc->ring.single_launch[k] ? sc->ring.ev_pend[k] : sc->ring.ev_end[k]) == hipSuccess) { sum_p += ms_p; sum_t += ms_t; ++n; }
    }
    sc->ring.frames_reported = sc->ring.frames_recorded;
    if (n) { out->kernel_ms_primary = sum_p / (double)n; out->kernel_ms_total = sum_t / (double)n; }
    out->frames_timed = (uint32_t)n;
    if (c.overflow) return fail(NRAYS_ERR_QUEUE_OVERFLOW, "continuation-ray queue overflow: image is incomplete");
    return NRAYS_OK;
}

int nrays_get_tile_costs(NraysScene* sc, NraysTileCosts* out) {
    if (!sc || !out) return fail(NRAYS_ERR_BAD_ARG, "null argument");
    std::memset(out, 0, sizeof *out);
    if (!sc->last.have || !sc->order.d_tile_cost || !sc->order.cost_valid || sc->order.cost_tiles == 0) return fail(NRAYS_ERR_BAD_ARG, "no frame of this handle has recorded its tile costs");
    HIP_TRY(hipSetDevice(sc->facts.device));
    HIP_TRY(hipStreamSynchronize(sc->last.stream));
    std::vector<uint32_t> c(sc->order.cost_tiles);
    HIP_TRY(hipMemcpy(c.data(), sc->order.d_tile_cost, c.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    // The unit the schedule deals is a wave tile — or ONE PART of a tile the cost-ordered lists split: k_primary marks the record of a tile that ran in parts
    // (kCostSplit; the value is its most expensive part's cycles x 2^lsl, or x 3 for the pixel-split tiles of one-light frames).  max_cycles is the longest such
    // unit, sum_cycles what the waves spend: every part of a split tile counted (at its most expensive part's price: an upper bound).
    const uint32_t lsl = sc->order.cost_split_lsl;
    const bool multi = (sc->facts.features & kFeatMultiSample) != 0;
    for (uint32_t rec : c) {
        const uint32_t v = rec & kCostMask;
        uint64_t unit = v, n = 1;
        if (lsl && (rec & kCostSplit)) { unit = multi ? (uint64_t)(v >> lsl) : (uint64_t)(v / 3u); n = 1ull << lsl; }
        out->sum_cycles += unit * n * 16u; out->max_cycles = std::max<uint64_t>(out->max_cycles, unit * 16u);
    }
    out->tiles = c.size(); out->resident_waves = (uint64_t)sc->order.cost_grid * (kBlock / 64);
    if (sc->order.d_cost_meta) { // the recording launch about itself (DRender::cost_meta)
        unsigned long long m[4] = {0, 0, 0, 0};
        HIP_TRY(hipMemcpy(m, sc->order.d_cost_meta, sizeof m, hipMemcpyDeviceToHost));
        out->shader_clock_hz = m[3] ? (double)m[2] / ((double)m[3] * 1e-8) : 0.0;
    }
    {   // the recording launch between its events
        float ms = 0.0f;
        hipError_t e = hipErrorInvalidValue;
        if (sc->order.rec_events_valid) e = hipEventElapsedTime(&ms, sc->order.ev_rec[0], sc->order.ev_rec[1]);
        else if (sc->order.rec_slot >= 0 && sc->ring.ev_pbegin[sc->order.rec_slot] && sc->ring.ev_pend[sc->order.rec_slot]) e = hipEventElapsedTime(&ms, sc->ring.ev_pbegin[sc->order.rec_slot], sc->ring.ev_pend[sc->order.rec_slot]); // (the ring holds 256 timed frames)
        if (e == hipSuccess) out->kernel_ms = ms; else (void)hipGetLastError();
    }
    return NRAYS_OK;
}

#if defined(NR_PHASE_TIMING) || defined(NR_DEBUG_TILE_COSTS)
// Tuning builds only (tools/tile_costs.py): the per-wave-tile cycle counts (>> 4) of the last frame that recorded them.
int nrays_debug_tile_costs(NraysScene* sc, uint32_t* out, uint32_t capacity, uint32_t* out_count) {
    if (!sc || !sc->last.have || !sc->order.d_tile_cost) return NRAYS_ERR_BAD_ARG;
    HIP_TRY(hipStreamSynchronize(sc->last.stream));
    const uint32_t n = std::min(capacity, sc->order.tile_slots);
    HIP_TRY(hipMemcpy(out, sc->order.d_tile_cost, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    *out_count = n;
    return NRAYS_OK;
}
#endif
#ifdef NR_DEBUG_TILE_COSTS
// Tuning builds only (tools/tile_dump.py): k_seed_costs' guess of the last cold frame.
int nrays_debug_seed_costs(NraysScene* sc, uint32_t* out, uint32_t capacity, uint32_t* out_count) {
    if (!sc || !sc->last.have || !sc->order.d_seed_copy) return NRAYS_ERR_BAD_ARG;
    HIP_TRY(hipStreamSynchronize(sc->last.stream));
    const uint32_t n = std::min(capacity, sc->order.tile_slots);
    HIP_TRY(hipMemcpy(out, sc->order.d_seed_copy, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    *out_count = n;
    return NRAYS_OK;
}
// Tuning builds only (tools/wave_timeline.py): {kernel entry, first tile, exit, tiles} per wave of the last primary launch, 10 ns ticks.
int nrays_debug_wave_times(NraysScene* sc, uint32_t* out, uint32_t capacity_waves, uint32_t* out_waves) {
    if (!sc || !sc->last.have || !sc->order.d_wave_times) return NRAYS_ERR_BAD_ARG;
    HIP_TRY(hipStreamSynchronize(sc->last.stream));
    const uint32_t n = std::min<uint32_t>(capacity_waves, sc->order.dbg_grid * (kBlock / 64));
    HIP_TRY(hipMemcpy(out, sc->order.d_wave_times, (size_t)n * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    *out_waves = n;
    return NRAYS_OK;
}
// The second record per wave: {ticks in work tiles, ticks in tiles that traced nothing, ticks in background rows, work tiles | miss tiles << 8 | rows << 16 | longest work tile / 16 ticks << 24}.
int nrays_debug_wave_times2(NraysScene* sc, uint32_t* out, uint32_t capacity_waves, uint32_t* out_waves) {
    if (!sc || !sc->last.have || !sc->order.d_wave_times) return NRAYS_ERR_BAD_ARG;
    HIP_TRY(hipStreamSynchronize(sc->last.stream));
    const uint32_t n = std::min<uint32_t>(capacity_waves, sc->order.dbg_grid * (kBlock / 64));
    HIP_TRY(hipMemcpy(out, sc->order.d_wave_times + (size_t)kMaxGrid * (kBlock / 64) * 4, (size_t)n * 4 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    *out_waves = n;
    return NRAYS_OK;
}
#endif
#ifdef NR_PHASE_TIMING
// Tuning builds only (tools/phase_timing.py): wave / lane iteration counts of the node loops and the triangle loops.
int nrays_debug_counters(NraysScene* sc, unsigned long long out[16]) {
    if (!sc || !sc->last.have) return NRAYS_ERR_BAD_ARG;
    HIP_TRY(hipStreamSynchronize(sc->last.stream));
    DeviceCounters c;
    HIP_TRY(hipMemcpy(&c, sc->buf.d_counters, sizeof c, hipMemcpyDeviceToHost));
    for (int k = 0; k < 8; ++k) out[k] = c.dbg[k];
    for (int k = 0; k < 8; ++k) out[8 + k] = c.dbg2[k];
    return NRAYS_OK;
}
#endif

int nrays_get_primary_kernel_stats(NraysScene* sc, NraysStats* out) {
    if (!sc || !out) return fail(NRAYS_ERR_BAD_ARG, "null argument");
    std::memset(out, 0, sizeof *out);
    if (!sc->last.have || !sc->last.instrumented) return fail(NRAYS_ERR_BAD_ARG, "the last render was not instrumented");
    HIP_TRY(hipSetDevice(sc->facts.device));
    HIP_TRY(hipStreamSynchronize(sc->last.stream));
    DeviceCounters c;
    HIP_TRY(hipMemcpy(&c, sc->ring.d_counters_primary, sizeof c, hipMemcpyDeviceToHost));
    out->rays_primary = sc->last.primary_first_batch;
    fill_counters(out, c);
    out->rays_shadow_elided = c.shadow_elided;
    // single continuations (reflection OR refraction) are traced by the primary kernel itself (trace_chain); only the
    // second child of a double branch goes through the queue to k_bounce, after this snapshot was taken
    out->instrumented = 1;
    return NRAYS_OK;
}

// What the blocking renders report of the frame's continuation queue, once the frame is over.
static int check_overflow(NraysScene* sc) {
    if (!sc->facts.host.any_double_branch) return NRAYS_OK; // only scenes with a continuation queue can overflow it: the others skip the extra blocking copy
    unsigned int overflow = 0;
    HIP_TRY(hipMemcpy(&overflow, &sc->buf.d_counters->overflow, sizeof overflow, hipMemcpyDeviceToHost));
    if (overflow) return fail(NRAYS_ERR_QUEUE_OVERFLOW, "continuation-ray queue overflow: image is incomplete");
    return NRAYS_OK;
}

int nrays_render(NraysScene* sc, const NraysRenderParams* p, float* out_rgb) {
    if (!sc || !p || !out_rgb) return fail(NRAYS_ERR_BAD_ARG, "null argument");
    HIP_TRY(hipSetDevice(sc->facts.device));
    size_t floats = (size_t)tile_rows(p) * p->width * 3;
    int rc = grow_device((void**)&sc->buf.d_frame, &sc->buf.frame_floats, floats, sizeof(float));
    if (rc == NRAYS_OK) rc = ensure_own_stream(sc);
    if (rc == NRAYS_OK) rc = render_impl(sc, p, sc->buf.d_frame, sc->buf.own_stream, false);
    if (rc != NRAYS_OK) return rc;
    HIP_TRY(hipMemcpyAsync(out_rgb, sc->buf.d_frame, floats * sizeof(float), hipMemcpyDeviceToHost, sc->buf.own_stream));
    HIP_TRY(hipStreamSynchronize(sc->buf.own_stream));
    return check_overflow(sc);
}

int nrays_render_rgb8(NraysScene* sc, const NraysRenderParams* p, uint8_t* out_rgb8) {
    if (!sc || !p || !out_rgb8) return fail(NRAYS_ERR_BAD_ARG, "null argument");
    HIP_TRY(hipSetDevice(sc->facts.device));
    const size_t n = (size_t)tile_rows(p) * p->width * 3;
    int rc = grow_device((void**)&sc->buf.d_frame, &sc->buf.frame_floats, n, sizeof(float));
    if (rc == NRAYS_OK) rc = grow_device((void**)&sc->buf.d_rgb8, &sc->buf.rgb8_bytes, n, 1);
    if (rc == NRAYS_OK) rc = ensure_own_stream(sc);
    if (rc == NRAYS_OK) rc = render_impl(sc, p, sc->buf.d_frame, sc->buf.own_stream, false);
    if (rc != NRAYS_OK) return rc;
    if (n) {
        hipLaunchKernelGGL(k_quantize_rgb8, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, sc->buf.own_stream, sc->buf.d_frame, sc->buf.d_rgb8, n);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out_rgb8, sc->buf.d_rgb8, n, hipMemcpyDeviceToHost, sc->buf.own_stream));
    }
    HIP_TRY(hipStreamSynchronize(sc->buf.own_stream));
    return check_overflow(sc);
}

int nrays_debug_scene_flags(const NraysScene* sc, uint32_t out[2]) {
    if (!sc || !out) return fail(NRAYS_ERR_BAD_ARG, "null argument");
    out[0] = (uint32_t)sc->facts.host.features; out[1] = sc->facts.d.incoherent;
    return NRAYS_OK;
}

int nrays_debug_last_permutation(const NraysScene* sc, uint32_t out[6]) {
    if (!sc || !out) return fail(NRAYS_ERR_BAD_ARG, "null argument");
    for (int a = 0; a < 4; ++a) out[a] = sc->last.perm_launches ? sc->last.perm_last[a] : 0u;
    out[4] = sc->last.perm_launches; out[5] = sc->last.perm_mixed ? 1u : 0u;
    return NRAYS_OK;
}

int nrays_debug_pipeline_counts(const NraysScene* sc, uint64_t out[4]) {
    if (!sc || !out) return fail(NRAYS_ERR_BAD_ARG, "null argument");
    out[0] = sc->pipe.n_pipelined; out[1] = sc->pipe.n_direct; out[2] = sc->pipe.n_inflight_queries; out[3] = sc->pipe.n_slot_waits;
    return NRAYS_OK;
}

int nrays_debug_blas_build(const NraysMesh* mesh, uint32_t flags, NraysBlasDump* out) {
    if (!mesh || !out) return fail(NRAYS_ERR_BAD_ARG, "null argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(NRAYS_ERR_NO_DEVICE, "no HIP device visible");
    nrays::BlasProbe probe; std::string err;
    const int rc = nrays::build_blas_probe(mesh, nrays::read_switches(), (flags & 1u) != 0, (flags & 2u) == 0, probe, err);
    if (rc != NRAYS_OK) return fail(rc, err);
    out->num_nodes = (uint32_t)probe.nodes.size(); out->num_refs = (uint32_t)probe.tri_ids.size();
    out->root = probe.root; out->max_depth = probe.max_depth; out->hairy = probe.hairy ? 1u : 0u;
    if (probe.nodes.size() > out->node_capacity || probe.tri_ids.size() > out->ref_capacity) return fail(NRAYS_ERR_BAD_ARG, "dump buffers too small");
    if (!probe.nodes.empty()) { if (!out->nodes) return fail(NRAYS_ERR_BAD_ARG, "null node buffer"); std::memcpy(out->nodes, probe.nodes.data(), probe.nodes.size() * sizeof(nrays::BvhNode)); }
    if (!probe.tri_ids.empty()) { if (!out->tri_ids) return fail(NRAYS_ERR_BAD_ARG, "null reference buffer"); std::memcpy(out->tri_ids, probe.tri_ids.data(), probe.tri_ids.size() * 4u); }
    return NRAYS_OK;
}

int nrays_debug_node_aabb(NraysScene* sc, uint32_t node, double out[6]) {
    if (!sc || !out) return fail(NRAYS_ERR_BAD_ARG, "null argument");
    if (!sc->facts.d.node_aabbs || (size_t)node * 6 + 6 > sc->facts.host.node_aabbs.size()) return fail(NRAYS_ERR_BAD_ARG, "node index out of range");
    HIP_TRY(hipSetDevice(sc->facts.device));
    HIP_TRY(hipMemcpy(out, sc->facts.d.node_aabbs + 6 * (size_t)node, 6 * sizeof(double), hipMemcpyDeviceToHost));
    return NRAYS_OK;
}

// One array of the dump: `count` records of `elem` bytes from device memory into the caller's buffer.
static int dump_array(void* dst, const void* src, size_t count, size_t elem, const char* what) {
    if (count == 0) return NRAYS_OK;
    if (!dst) return fail(NRAYS_ERR_BAD_ARG, std::string("null dump buffer: ") + what);
    if (!src) return fail(NRAYS_ERR_HIP, std::string("the scene holds no device array: ") + what);
    HIP_TRY(hipMemcpy(dst, src, count * elem, hipMemcpyDeviceToHost));
    return NRAYS_OK;
}

int nrays_debug_scene_dump(NraysScene* sc, NraysSceneDump* out) {
    if (!sc || !out) return fail(NRAYS_ERR_BAD_ARG, "null argument");
    const HostScene& h = sc->facts.host; const DScene& d = sc->facts.d;
    // the counts of the uploaded arrays (the host copies of the records stay with the handle; the kernels' own words are d's)
    const size_t nodes = sc->facts.num_nodes, tris = sc->facts.num_tris, insts = h.instances.size(), sinsts = h.shadow_instances.size(), planes = d.num_planes, snodes = h.node_aabbs.size() / 6;
    out->num_nodes = (uint32_t)nodes; out->num_tris = (uint32_t)tris; out->num_instances = (uint32_t)insts; out->num_shadow_instances = (uint32_t)sinsts;
    out->num_planes = (uint32_t)planes; out->num_scene_nodes = (uint32_t)snodes;
    out->closest_root = d.closest_root; out->shadow_root = d.shadow_root;
    out->max_bvh_depth = h.max_bvh_depth; out->bounded = h.bounded ? 1u : 0u; out->dev_nodes = (uint32_t)h.dev_nodes; out->dev_tris = (uint32_t)h.dev_tris;
    for (int a = 0; a < 3; ++a) { out->bounds_mn[a] = h.bounds_mn[a]; out->bounds_mx[a] = h.bounds_mx[a]; }
    if (nodes > out->node_capacity || tris > out->tri_capacity || insts > out->instance_capacity || sinsts > out->shadow_instance_capacity || planes > out->plane_capacity ||
        snodes > out->scene_node_capacity) return fail(NRAYS_ERR_BAD_ARG, "dump buffers too small");
    HIP_TRY(hipSetDevice(sc->facts.device));
    int rc = dump_array(out->nodes, d.nodes, nodes, sizeof(BvhNode), "nodes");
    if (rc == NRAYS_OK) rc = dump_array(out->tris, d.tris, tris, sizeof(TriRec), "tris");
    if (rc == NRAYS_OK) rc = dump_array(out->instances, d.instances, insts, sizeof(Instance), "instances");
    if (rc == NRAYS_OK) rc = dump_array(out->shadow_instances, d.shadow_instances, sinsts, sizeof(Instance), "shadow_instances");
    if (rc == NRAYS_OK) rc = dump_array(out->links, d.links, insts, sizeof(InstLink), "links");
    if (rc == NRAYS_OK) rc = dump_array(out->shadow_links, d.shadow_links, sinsts, sizeof(InstLink), "shadow_links");
    if (rc == NRAYS_OK) rc = dump_array(out->planes, d.planes, planes, sizeof(int32_t), "planes");
    if (rc == NRAYS_OK) rc = dump_array(out->shadow_planes, d.shadow_planes, planes, sizeof(int32_t), "shadow_planes");
    if (rc == NRAYS_OK) rc = dump_array(out->node_aabbs, d.node_aabbs, snodes * 6, sizeof(double), "node_aabbs");
    return rc;
}

int nrays_untile_device(const float* gathered, float* out_rgb_device, uint32_t width, uint32_t height, uint32_t band_rows,
                        uint32_t band_owners, void* hip_stream) {
    if (!gathered || !out_rgb_device || width == 0 || height == 0 || band_rows == 0 || band_owners == 0)
        return fail(NRAYS_ERR_BAD_ARG, "bad untile arguments");
    NraysRenderParams p; std::memset(&p, 0, sizeof p);
    p.width = width; p.height = height; p.band_rows = band_rows; p.band_owners = band_owners;
    uint32_t rows_local = band_owners > 1 ? tile_rows(&p) : height;
    size_t n = (size_t)width * height * 3;
    hipLaunchKernelGGL(k_untile, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, gathered, out_rgb_device,
                       width, height, band_rows, band_owners, rows_local);
    HIP_TRY(hipGetLastError());
    return NRAYS_OK;
}

} // extern "C"
