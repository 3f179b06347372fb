// tests/scene_dump_shim.cpp as a program of its own, for a build with -fsanitize=address,undefined (run by hand, on the host): a scene with two meshes under one rotated
// isometry (one of them transparent: three BLASes, two of them from the shim's fake device builder at a minimum of 16 triangles), a host-built mesh, a capsule and
// a plane is dumped through the size query and the fill, twice, and the two dumps compared.
//   g++ -std=c++17 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -I nrays_amd/csrc -pthread -o scene_dump_sweep \
//       tests/scene_dump_main.cpp tests/scene_dump_shim.cpp nrays_amd/csrc/scene_build.cpp nrays_amd/csrc/bvh_build.cpp nrays_amd/csrc/switches.cpp
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../include/nrays_abi.h"

extern "C" int scene_dump_host(const NraysSceneDesc* desc, uint32_t gpu_build_min, NraysSceneDump* out);
extern "C" const char* scene_dump_last_error();

namespace {

struct Dump {
    NraysSceneDump d;
    std::vector<float> nodes; std::vector<uint8_t> tris, inst, sinst; std::vector<int32_t> links, slinks, planes, splanes; std::vector<double> aabbs;
    int take(const NraysSceneDesc* desc) {
        std::memset(&d, 0, sizeof d);
        if (scene_dump_host(desc, 16, &d) != NRAYS_ERR_BAD_ARG) return 1; // sizes only
        nodes.resize(32u * d.num_nodes); tris.resize(48u * d.num_tris); inst.resize(136u * d.num_instances); sinst.resize(136u * d.num_shadow_instances);
        links.resize(2u * d.num_instances); slinks.resize(2u * d.num_shadow_instances); planes.resize(d.num_planes); splanes.resize(d.num_planes); aabbs.resize(6u * d.num_scene_nodes);
        d.node_capacity = d.num_nodes; d.tri_capacity = d.num_tris; d.instance_capacity = d.num_instances; d.shadow_instance_capacity = d.num_shadow_instances;
        d.plane_capacity = d.num_planes; d.scene_node_capacity = d.num_scene_nodes;
        d.nodes = nodes.data(); d.tris = tris.data(); d.instances = inst.data(); d.shadow_instances = sinst.data(); d.links = links.data(); d.shadow_links = slinks.data();
        d.planes = planes.data(); d.shadow_planes = splanes.data(); d.node_aabbs = aabbs.data();
        return scene_dump_host(desc, 16, &d) == NRAYS_OK ? 0 : 2;
    }
};

} // namespace

int main() {
    std::vector<std::vector<double>> verts; std::vector<std::vector<uint32_t>> idx;
    std::vector<NraysMesh> meshes; std::vector<NraysNode> nodes;
    NraysMaterial mat; std::memset(&mat, 0, sizeof mat); mat.kind = NRAYS_MAT_PHONG; mat.texture_id = -1; mat.alpha_texture_id = -1;
    NraysLight light; std::memset(&light, 0, sizeof light); light.pos[1] = 10.0; light.racsample = 1; light.color[0] = light.color[1] = light.color[2] = 1.0f;
    const uint32_t tri_counts[3] = {20, 17, 5};
    verts.reserve(3); idx.reserve(3);
    for (int m = 0; m < 3; ++m) { // strips of f32-exact vertices, side by side
        std::vector<double> v; std::vector<uint32_t> ix;
        for (uint32_t k = 0; k < tri_counts[m] + 2; ++k) { v.push_back(3.0 * m + 0.125 * (k / 2)); v.push_back((k & 1) ? 1.0 : 0.0); v.push_back(0.25 * (k % 3)); }
        for (uint32_t t = 0; t < tri_counts[m]; ++t) { ix.push_back(t); ix.push_back(t + 1); ix.push_back(t + 2); }
        verts.push_back(v); idx.push_back(ix);
        NraysMesh me; std::memset(&me, 0, sizeof me);
        me.num_vertices = tri_counts[m] + 2; me.num_triangles = tri_counts[m]; me.vertices = verts.back().data(); me.indices = idx.back().data();
        meshes.push_back(me);
    }
    auto node = [&](uint32_t kind, int32_t mesh, double tx, double wx, double wy, float alpha) {
        NraysNode n; std::memset(&n, 0, sizeof n);
        n.shape_kind = kind; n.solid = 1; n.params[0] = 0.75; n.params[1] = 0.5; n.translation[0] = tx; n.axis_angle[0] = wx; n.axis_angle[1] = wy;
        n.alpha = alpha; n.refr_coeff = 1.0; n.mesh_id = mesh;
        nodes.push_back(n);
    };
    node(NRAYS_SHAPE_TRIMESH, 0, 1.5, 2.221441469079183, 2.221441469079183, 1.0f);
    node(NRAYS_SHAPE_TRIMESH, 1, 1.5, 2.221441469079183, 2.221441469079183, 0.5f);
    node(NRAYS_SHAPE_TRIMESH, 2, 0.0, 0.0, 0.0, 1.0f);
    node(NRAYS_SHAPE_CAPSULE, -1, -2.0, 0.3, -0.5, 1.0f);
    node(NRAYS_SHAPE_PLANE, -1, 0.0, 0.0, 0.0, 1.0f);
    nodes.back().params[0] = 0.0; nodes.back().params[1] = 1.0;
    NraysSceneDesc d; std::memset(&d, 0, sizeof d);
    d.num_lights = 1; d.lights = &light; d.num_materials = 1; d.materials = &mat; d.num_meshes = 3; d.meshes = meshes.data(); d.num_nodes = (uint32_t)nodes.size(); d.nodes = nodes.data();
    Dump a, b;
    const int ra = a.take(&d), rb = b.take(&d);
    if (ra || rb) { std::printf("scene_dump sweep: dump failed (%d, %d): %s\n", ra, rb, scene_dump_last_error()); return 1; }
    // (bytes, not floats: a leaf ref read as a float is a NaN)
    const bool same = a.nodes.size() == b.nodes.size() && std::memcmp(a.nodes.data(), b.nodes.data(), a.nodes.size() * sizeof(float)) == 0 && a.tris == b.tris && a.inst == b.inst && a.sinst == b.sinst && a.links == b.links && a.slinks == b.slinks && a.planes == b.planes &&
                      a.splanes == b.splanes && std::memcmp(a.aabbs.data(), b.aabbs.data(), a.aabbs.size() * sizeof(double)) == 0;
    std::printf("scene_dump sweep: %u nodes (%u device-built), %u triangle records (%u), %u + %u instances, %u planes; two dumps %s\n", a.d.num_nodes, a.d.dev_nodes, a.d.num_tris,
                a.d.dev_tris, a.d.num_instances, a.d.num_shadow_instances, a.d.num_planes, same ? "equal" : "DIFFER");
    return same && a.d.dev_nodes && a.d.num_tris > a.d.dev_tris && a.d.num_planes == 1 ? 0 : 1;
}
