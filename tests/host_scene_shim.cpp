// Flattens small scene descriptors with build_host_scene() on a machine without a GPU and reports, per HostScene member, its length and an FNV-1a digest
// (tests/test_host_scene.py compares them with tests/golden/host_scene_digests.json; tests/host_scene_main.cpp runs the same cases under the sanitizers).
// Linked with scene_build.cpp, bvh_build.cpp and switches.cpp; the three symbols they need from the device side are supplied here: hipMemcpy (never reached),
// free_device_blas and a deterministic FAKE build_blas_device — null arrays, one reference per triangle, 1 + triangles / 8 nodes, root = node_base, bounds = the
// f32 min / max of the parts' vertices, depth 3 — so that "device-built first, host-built shifted behind" and the pending local AABBs run without a device.
// Digests are taken field by field: NodeSurface and HostTexture carry padding that the builder does not write.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "scene_build.h"

namespace {

struct Fnv {
    uint64_t h = 1469598103934665603ull;
    void bytes(const void* p, size_t n) { const unsigned char* b = (const unsigned char*)p; for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; } }
    template <typename T> void add(const T& v) { bytes(&v, sizeof v); }
    template <typename T> void arr(const T* v, size_t n) { bytes(v, n * sizeof(T)); }
};

Fnv g_fake_calls; // what the fake device builder was asked for: options, bases, parts
size_t g_fake_count = 0;

} // namespace

namespace nrays {

int build_blas_device(const std::vector<DeviceMeshPart>& parts, const DeviceBuildOptions& o, int32_t node_base, uint32_t prim_base, DeviceBlas& out, std::string&) {
    Fnv& f = g_fake_calls;
    f.add(o.max_leaf); f.add(o.prim_cost); f.add(o.prim_cost_hairy); f.add(o.budget); f.add(o.budget_hairy); f.add(o.min_gain); f.add(o.min_gain_hairy); f.add(o.hairy_emptiness);
    f.add(o.presplit); f.add(o.debug_cap_div); f.add(o.split_grid_max); f.add(o.one_walk); f.add(o.debug_piece_cap); f.add(o.verbose); f.add(o.node_tail);
    f.add(node_base); f.add(prim_base);
    size_t tris = 0;
    for (int a = 0; a < 3; ++a) { out.mn[a] = std::numeric_limits<float>::infinity(); out.mx[a] = -std::numeric_limits<float>::infinity(); }
    for (const DeviceMeshPart& p : parts) {
        f.add(p.num_vertices); f.add(p.num_triangles); f.add(p.node_id); f.add((uint32_t)(p.uvs != nullptr));
        tris += p.num_triangles;
        for (uint32_t v = 0; v < p.num_vertices; ++v)
            for (int a = 0; a < 3; ++a) { const float x = (float)p.vertices[3 * (size_t)v + a]; out.mn[a] = std::min(out.mn[a], x); out.mx[a] = std::max(out.mx[a], x); }
    }
    out.nodes = nullptr; out.tris = nullptr; out.uvs = nullptr;
    out.num_triangles = tris; out.num_refs = tris; out.num_nodes = 1 + tris / 8; out.node_capacity = out.num_nodes;
    out.root = node_base; out.hairy = false; out.max_depth = 3;
    ++g_fake_count;
    return NRAYS_OK;
}
void free_device_blas(DeviceBlas& b) { b.nodes = nullptr; b.tris = nullptr; b.uvs = nullptr; b.num_nodes = 0; b.num_refs = 0; b.node_capacity = 0; }

} // namespace nrays

extern "C" hipError_t hipMemcpy(void*, const void*, size_t, hipMemcpyKind) { return hipErrorNotSupported; } // (build_blas_probe's device branch: not part of these cases)

namespace {
using namespace nrays;

// ---- the cases ---------------------------------------------------------------------------------------------------------
const double kRotA[3] = {0.3, -0.5, 0.2}, kRotB[3] = {0.0, 1.25, 0.0}; // the two rotations of the rotated cases (their half-angle sin / cos: host_scene_trig_bits)

struct Desc { // owns every array of a descriptor
    std::vector<NraysLight> lights; std::vector<NraysMaterial> materials; std::vector<NraysTexture> textures; std::vector<NraysMesh> meshes; std::vector<NraysNode> nodes;
    std::vector<std::vector<double>> verts, uvs; std::vector<std::vector<uint32_t>> idx; std::vector<std::vector<uint8_t>> texels;
    NraysSceneDesc d;
    Switches sw;
    const NraysSceneDesc* finish() {
        std::memset(&d, 0, sizeof d);
        d.background[0] = 0.25f; d.background[1] = 0.5f; d.background[2] = 0.75f;
        d.num_lights = (uint32_t)lights.size(); d.lights = lights.data(); d.num_materials = (uint32_t)materials.size(); d.materials = materials.data();
        d.num_textures = (uint32_t)textures.size(); d.textures = textures.data(); d.num_meshes = (uint32_t)meshes.size(); d.meshes = meshes.data();
        d.num_nodes = (uint32_t)nodes.size(); d.nodes = nodes.data();
        return &d;
    }
    void light(double x, double y, double z, double radius, uint32_t racsample) {
        NraysLight l; std::memset(&l, 0, sizeof l);
        l.pos[0] = x; l.pos[1] = y; l.pos[2] = z; l.radius = radius; l.racsample = racsample; l.color[0] = 1.0f; l.color[1] = 0.5f; l.color[2] = 0.25f;
        lights.push_back(l);
    }
    uint32_t material(uint32_t kind, int32_t tex = -1, int32_t alpha_tex = -1) {
        NraysMaterial m; std::memset(&m, 0, sizeof m);
        m.kind = kind; m.texture_id = tex; m.alpha_texture_id = alpha_tex; m.shininess = 12.5f;
        for (int a = 0; a < 3; ++a) { m.ambiant[a] = 0.125f * (float)(a + 1); m.diffuse[a] = 0.25f * (float)(a + 1); m.specular[a] = 0.0625f * (float)(a + 1); }
        materials.push_back(m);
        return (uint32_t)materials.size() - 1;
    }
    int32_t texture(uint32_t w, uint32_t h, uint32_t format, uint32_t interp, uint32_t overflow) {
        texels.emplace_back((size_t)w * h * (format == NRAYS_TEXEL_RGBA8 ? 4 : 16));
        for (size_t i = 0; i < texels.back().size(); ++i) texels.back()[i] = (uint8_t)(37u * i + 11u);
        NraysTexture t; std::memset(&t, 0, sizeof t);
        t.width = w; t.height = h; t.format = format; t.interp = interp; t.overflow = overflow; t.texels = texels.back().data();
        textures.push_back(t);
        return (int32_t)textures.size() - 1;
    }
    // a strip of `tris` triangles over tris + 2 vertices, every vertex used; f32-exact coordinates; `thin`: long diagonal slivers (hair-like)
    int32_t strip(uint32_t tris, bool with_uvs, double ox, bool thin = false) {
        std::vector<double> v, uv; std::vector<uint32_t> ix;
        if (thin) {
            for (uint32_t t = 0; t < tris; ++t) {
                const double x = ox + 0.5 * t;
                const double p[9] = {x, 0.0, 0.0, x + 8.0, 8.0, 8.0, x + 8.0, 8.0, 8.0625};
                v.insert(v.end(), p, p + 9);
                for (int k = 0; k < 3; ++k) { ix.push_back(3 * t + k); uv.push_back(0.125 * k); uv.push_back(0.25 * t); }
            }
        } else {
            for (uint32_t k = 0; k < tris + 2; ++k) { v.push_back(ox + 0.5 * (k / 2)); v.push_back((k & 1) ? 1.0 : 0.0); v.push_back(0.125 * (k % 3)); uv.push_back(0.25 * (k / 2)); uv.push_back((k & 1) ? 1.0 : 0.0); }
            for (uint32_t t = 0; t < tris; ++t) { ix.push_back(t); ix.push_back(t + 1); ix.push_back(t + 2); }
        }
        verts.push_back(v); uvs.push_back(uv); idx.push_back(ix);
        NraysMesh m; std::memset(&m, 0, sizeof m);
        m.num_vertices = (uint32_t)(v.size() / 3); m.num_triangles = tris; m.vertices = verts.back().data(); m.uvs = with_uvs ? uvs.back().data() : nullptr;
        m.indices = tris ? idx.back().data() : nullptr;
        meshes.push_back(m);
        return (int32_t)meshes.size() - 1;
    }
    NraysNode& node(uint32_t kind, uint32_t material_id, const double t[3], const double w[3], double p0 = 0.0, double p1 = 0.0, double p2 = 0.0, int32_t mesh = -1) {
        NraysNode n; std::memset(&n, 0, sizeof n);
        n.shape_kind = kind; n.solid = 1; n.params[0] = p0; n.params[1] = p1; n.params[2] = p2;
        for (int a = 0; a < 3; ++a) { n.translation[a] = t[a]; n.axis_angle[a] = w[a]; }
        n.alpha = 1.0f; n.refr_coeff = 1.0; n.material_id = material_id; n.mesh_id = mesh;
        nodes.push_back(n);
        return nodes.back();
    }
};

const double kZero[3] = {0, 0, 0};

void three_meshes(Desc& s, const double t[3], const double w[3]) { // opaque, opaque, alpha-textured under one isometry
    s.light(5, 6, 7, 0.0, 1);
    const int32_t rgba8 = s.texture(2, 2, NRAYS_TEXEL_RGBA8, 0, 1), rgbaf = s.texture(1, 3, NRAYS_TEXEL_RGBA32F, 1, 0);
    const uint32_t plain = s.material(NRAYS_MAT_PHONG), textured = s.material(NRAYS_MAT_PHONG, rgbaf), cutout = s.material(NRAYS_MAT_PHONG, -1, rgba8);
    s.node(NRAYS_SHAPE_TRIMESH, plain, t, w, 0, 0, 0, s.strip(5, false, 0.0));
    s.node(NRAYS_SHAPE_TRIMESH, textured, t, w, 0, 0, 0, s.strip(11, true, 4.0));
    s.node(NRAYS_SHAPE_TRIMESH, cutout, t, w, 0, 0, 0, s.strip(3, true, -3.0));
}

const char* const kCaseNames[] = {"empty", "analytic", "quad", "three_meshes", "no_triangles", "hair", "two_lights", "three_meshes_rotated", "mixed_device",
                                  "bad_index", "bad_vertex", "bad_uv", "bad_material_id", "bad_mesh_id", "bad_texture_id", "null_array"};
constexpr int kCases = (int)(sizeof kCaseNames / sizeof kCaseNames[0]);

const NraysSceneDesc* make_case(int c, Desc& s) {
    const double t1[3] = {1.0, 2.0, 3.0}, t2[3] = {-4.0, 0.5, 2.0}, t3[3] = {0.0, -7.0, 1.5};
    switch (c) {
    case 0: break;
    case 1: { // one of each analytic shape; the capsule is transparent and reflective (a reflection and a refraction at one hit)
        s.light(5, 6, 7, 0.0, 1);
        const uint32_t m = s.material(NRAYS_MAT_PHONG), nm = s.material(NRAYS_MAT_NORMAL), um = s.material(NRAYS_MAT_UV);
        s.node(NRAYS_SHAPE_BALL, m, t1, kRotA, 0.75);
        s.node(NRAYS_SHAPE_CUBOID, um, t2, kRotA, 0.5, 1.0, 1.5);
        s.node(NRAYS_SHAPE_CYLINDER, nm, t3, kRotB, 1.0, 0.25);
        NraysNode& cap = s.node(NRAYS_SHAPE_CAPSULE, m, t1, kRotB, 0.5, 0.25);
        cap.alpha = 0.5f; cap.refl_mix = 0.25f; cap.refl_atenuation = 0.25f; cap.refr_coeff = 1.5;
        s.node(NRAYS_SHAPE_CONE, um, t2, kZero, 1.0, 0.5).solid = 0;
        s.node(NRAYS_SHAPE_PLANE, m, t3, kZero, 0.0, 1.0, 0.0);
        break;
    }
    case 2: { // a two-triangle quad with uvs, untransformed
        s.light(5, 6, 7, 0.0, 1);
        s.node(NRAYS_SHAPE_TRIMESH, s.material(NRAYS_MAT_UV), kZero, kZero, 0, 0, 0, s.strip(2, true, 0.0));
        break;
    }
    case 3: three_meshes(s, t1, kZero); break;
    case 4: s.light(5, 6, 7, 0.0, 1); s.node(NRAYS_SHAPE_TRIMESH, s.material(NRAYS_MAT_PHONG), t1, kZero, 0, 0, 0, s.strip(0, false, 0.0)); break;
    case 5: s.light(5, 6, 7, 0.0, 1); s.node(NRAYS_SHAPE_TRIMESH, s.material(NRAYS_MAT_PHONG), kZero, kZero, 0, 0, 0, s.strip(70, false, 0.0, true)); break;
    case 6: s.light(5, 6, 7, 0.0, 1); s.light(-5, 6, 7, 0.5, 3); s.node(NRAYS_SHAPE_BALL, s.material(NRAYS_MAT_PHONG), t1, kZero, 0.75).refl_mix = 0.5f; break;
    case 7: three_meshes(s, t2, kRotA); break;
    case 8: { // meshes of 4 triangles and more go to the (fake) device builder: one alone in its group, two merged (one of them below the limit), one host-built, a ball
        s.sw.gpu_build_min = 4;
        s.light(5, 6, 7, 0.0, 1);
        const uint32_t m = s.material(NRAYS_MAT_PHONG);
        s.node(NRAYS_SHAPE_TRIMESH, m, t3, kZero, 0, 0, 0, s.strip(2, false, 9.0));
        s.node(NRAYS_SHAPE_TRIMESH, m, t1, kRotA, 0, 0, 0, s.strip(6, true, 0.0));
        s.node(NRAYS_SHAPE_BALL, m, t2, kRotB, 1.25);
        s.node(NRAYS_SHAPE_TRIMESH, m, t2, kRotB, 0, 0, 0, s.strip(5, false, 2.0));
        s.node(NRAYS_SHAPE_TRIMESH, m, t2, kRotB, 0, 0, 0, s.strip(3, false, -2.0));
        break;
    }
    case 9: case 10: case 11: { // a quad whose last index / one coordinate / one uv is refused
        s.light(5, 6, 7, 0.0, 1);
        s.node(NRAYS_SHAPE_TRIMESH, s.material(NRAYS_MAT_PHONG), kZero, kZero, 0, 0, 0, s.strip(2, true, 0.0));
        if (c == 9) s.idx.back()[5] = 4;
        if (c == 10) s.verts.back()[4] = 0.1;
        if (c == 11) s.uvs.back()[3] = 0.1;
        break;
    }
    case 12: s.material(NRAYS_MAT_PHONG); s.node(NRAYS_SHAPE_BALL, 1, t1, kZero, 0.75); break;
    case 13: s.node(NRAYS_SHAPE_TRIMESH, s.material(NRAYS_MAT_PHONG), t1, kZero, 0, 0, 0, 1); s.strip(2, false, 0.0); break;
    case 14: s.texture(1, 1, NRAYS_TEXEL_RGBA8, 0, 0); s.material(NRAYS_MAT_PHONG, 1); break;
    default: break;
    }
    const NraysSceneDesc* d = s.finish();
    if (c == 15) { s.d.num_lights = 1; s.d.lights = nullptr; }
    return d;
}

// ---- the report ----------------------------------------------------------------------------------------------------------
struct Report {
    std::string text = "{";
    void sep() { if (text.size() > 1) text += ", "; }
    void member(const char* name, size_t len, const Fnv& f) { char b[128]; snprintf(b, sizeof b, "\"%s\": [%zu, \"%016llx\"]", name, len, (unsigned long long)f.h); sep(); text += b; }
    void integer(const char* name, long long v) { char b[96]; snprintf(b, sizeof b, "\"%s\": %lld", name, v); sep(); text += b; }
    void string(const char* name, const std::string& v) { sep(); text += std::string("\"") + name + "\": \"" + v + "\""; } // (the messages hold no quote or backslash)
    template <typename T> void raw(const char* name, const std::vector<T>& v) { Fnv f; f.arr(v.data(), v.size()); member(name, v.size(), f); }
};

std::string run_case(int c) {
    Desc s;
    const NraysSceneDesc* d = make_case(c, s);
    g_fake_calls = Fnv(); g_fake_count = 0;
    HostScene hs; std::string err;
    const int rc = build_host_scene(d, s.sw, hs, err);
    Report r;
    r.integer("status", rc); r.string("err", err);
    if (rc != NRAYS_OK) return r.text + "}";
    {
        Fnv f;
        for (const BvhNode& n : hs.nodes) f.add(n.slot);
        r.member("nodes", hs.nodes.size(), f);
    }
    r.raw("tris", hs.tris); r.raw("triuvs", hs.triuvs);
    for (int which = 0; which < 2; ++which) {
        Fnv f;
        const std::vector<Instance>& v = which ? hs.shadow_instances : hs.instances;
        for (const Instance& in : v) { f.add(in.rot); f.add(in.trans); f.add(in.params); f.add(in.kind); f.add(in.flags); f.add(in.node_id); f.add(in.blas_root); }
        r.member(which ? "shadow_instances" : "instances", v.size(), f);
        Fnv g;
        const std::vector<InstLink>& l = which ? hs.shadow_links : hs.links;
        for (const InstLink& k : l) { g.add(k.blas_root); g.add(k.flags); }
        r.member(which ? "shadow_links" : "links", l.size(), g);
    }
    r.raw("planes", hs.planes); r.raw("shadow_planes", hs.shadow_planes);
    {
        Fnv f;
        for (const NodeRec& n : hs.node_recs) { f.add(n.refl_mix); f.add(n.refl_atenuation); f.add(n.alpha); f.add(n.material_id); f.add(n.refr_coeff); f.add(n.pad); }
        r.member("node_recs", hs.node_recs.size(), f);
    }
    {
        Fnv f;
        for (const ShadeRec& n : hs.shade) {
            f.add(n.refl_mix); f.add(n.refl_atenuation); f.add(n.alpha); f.add(n.flags); f.add(n.refr_coeff); f.add(n.ka); f.add(n.kd); f.add(n.ks); f.add(n.shininess);
            for (const ShadeTex* t : {&n.tex, &n.alpha_tex}) { f.add((uint32_t)(t->texels != nullptr)); f.add(t->width); f.add(t->height); f.add(t->mode); f.add(t->pad); }
            f.add(n.pad);
        }
        r.member("shade", hs.shade.size(), f);
    }
    r.raw("shade_tex", hs.shade_tex); r.raw("shade_alpha_tex", hs.shade_alpha_tex); r.raw("node_aabbs", hs.node_aabbs);
    {
        Fnv f;
        for (const NodeSurface& n : hs.surface) { f.add(n.first); f.add(n.count); f.add((uint32_t)n.mesh); f.add((uint32_t)n.has_uv); f.add((uint32_t)n.device_built); f.add(n.flags); f.add(n.rot); f.add(n.trans); }
        r.member("surface", hs.surface.size(), f);
    }
    {
        Fnv f;
        for (const MaterialRec& m : hs.materials) { f.add(m.kind); f.add(m.ka); f.add(m.kd); f.add(m.ks); f.add(m.shininess); f.add(m.tex); f.add(m.alpha_tex); f.add(m.pad); }
        r.member("materials", hs.materials.size(), f);
    }
    {
        Fnv f;
        for (const HostTexture& t : hs.textures) {
            f.add(t.rec.width); f.add(t.rec.height); f.add(t.rec.format); f.add(t.rec.interp); f.add(t.rec.overflow); f.add(t.rec.pad); f.add((uint32_t)(t.rec.texels != nullptr));
            f.add((uint64_t)t.bytes.size()); f.arr(t.bytes.data(), t.bytes.size());
        }
        r.member("textures", hs.textures.size(), f);
    }
    {
        Fnv f;
        for (const LightRec& l : hs.lights) { f.add(l.pos); f.add(l.radius); f.add(l.color); f.add(l.racsample); }
        r.member("lights", hs.lights.size(), f);
    }
    {
        Fnv f;
        for (const DeviceBlas& b : hs.dev_blas) { f.add((uint64_t)b.num_nodes); f.add((uint64_t)b.num_refs); f.add(b.root); f.add(b.mn); f.add(b.mx); f.add((uint32_t)b.hairy); f.add(b.max_depth); f.add((uint64_t)b.num_triangles); }
        r.member("dev_blas", hs.dev_blas.size(), f);
    }
    r.member("device_builds", g_fake_count, g_fake_calls);
    r.integer("closest_root", hs.closest_root); r.integer("shadow_root", hs.shadow_root);
    r.integer("flags", (hs.any_reflective ? 1 : 0) | (hs.any_transparent ? 2 : 0) | (hs.any_area_light ? 4 : 0) | (hs.any_double_branch ? 8 : 0) | (hs.any_incoherent ? 16 : 0) |
                           (hs.any_mesh ? 32 : 0) | (hs.bounded ? 64 : 0));
    r.integer("features", hs.features); r.integer("reflection_generations", hs.reflection_generations); r.integer("max_bvh_depth", hs.max_bvh_depth);
    r.integer("dev_nodes", (long long)hs.dev_nodes); r.integer("dev_tris", (long long)hs.dev_tris);
    {
        Fnv f; f.add(hs.background); f.add(hs.bounds_mn); f.add(hs.bounds_mx);
        r.member("background_bounds", 9, f);
    }
    return r.text + "}";
}

} // namespace

extern "C" {

int host_scene_cases() { return kCases; }
const char* host_scene_case_name(int c) { return c >= 0 && c < kCases ? kCaseNames[c] : nullptr; }

// The report of case c as one JSON object; returns its length, or -1 when `cap` is too small or there is no such case.
int host_scene_report(int c, char* out, size_t cap) {
    if (c < 0 || c >= kCases) return -1;
    const std::string r = run_case(c);
    if (r.size() + 1 > cap) return -1;
    std::memcpy(out, r.c_str(), r.size() + 1);
    return (int)r.size();
}

// Bit patterns of sin(a / 2), cos(a / 2) for the two rotation angles the rotated cases use: the libm results their goldens depend on.
int host_scene_trig_bits(uint64_t out[4]) {
    int k = 0;
    for (const double* w : {kRotA, kRotB}) {
        const double a = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
        static double (*volatile libm_sin)(double) = std::sin;
        static double (*volatile libm_cos)(double) = std::cos;
        const double s = libm_sin(a / 2.0), c = libm_cos(a / 2.0);
        std::memcpy(&out[k++], &s, 8); std::memcpy(&out[k++], &c, 8);
    }
    return k;
}

// Every case twice: the number of cases whose two reports differ (what tests/host_scene_main.cpp runs).
int host_scene_sweep(int* cases) {
    int bad = 0;
    for (int c = 0; c < kCases; ++c) if (run_case(c) != run_case(c)) ++bad;
    *cases = kCases;
    return bad;
}

} // extern "C"
