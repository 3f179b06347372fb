// The flattened scene of build_host_scene() on a machine without a GPU, in the field set of nrays_debug_scene_dump (include/nrays_abi.h: NraysSceneDump), for
// tests/scene_cover.py.  The descriptor comes straight from Python (nrays_amd.scene.SceneDescriptor.pointer()), so a scene is written once for this path and for the device's.
// Linked with scene_build.cpp, bvh_build.cpp and switches.cpp like tests/host_scene_shim.cpp, and like it supplies the three symbols they need from the device side:
// hipMemcpy (never reached), free_device_blas and a FAKE build_blas_device.  This fake returns real arrays in host memory — the host builder's tree over one box per
// triangle, child and leaf refs absolute from node_base / prim_base as the device builder leaves them, records in leaf order, bounds = the f32 min / max over the
// faces' vertices — so that "device-built first, host-built moved behind" (link_scene), single_bounds and the pending local AABBs run, and a walk from an instance's
// blas_root reaches the triangle records of either builder.  tests/scene_dump_main.cpp runs it under the sanitizers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "bvh_build.h"
#include "scene_build.h"

namespace nrays {

int build_blas_device(const std::vector<DeviceMeshPart>& parts, const DeviceBuildOptions& o, int32_t node_base, uint32_t prim_base, DeviceBlas& out, std::string& err) {
    std::vector<TriRec> recs; std::vector<PrimBounds> boxes;
    for (int a = 0; a < 3; ++a) { out.mn[a] = std::numeric_limits<float>::infinity(); out.mx[a] = -std::numeric_limits<float>::infinity(); }
    for (const DeviceMeshPart& p : parts)
        for (uint32_t t = 0; t < p.num_triangles; ++t) {
            TriRec r; PrimBounds b; float* vs[3] = {r.v0, r.v1, r.v2};
            for (int a = 0; a < 3; ++a) { b.mn[a] = std::numeric_limits<float>::infinity(); b.mx[a] = -std::numeric_limits<float>::infinity(); }
            for (int k = 0; k < 3; ++k) {
                const uint32_t vi = p.indices[3 * (size_t)t + k];
                if (vi >= p.num_vertices) return refuse_mesh(kMeshIndexRange, err);
                for (int a = 0; a < 3; ++a) { const float f = (float)p.vertices[3 * (size_t)vi + a]; vs[k][a] = f; b.mn[a] = std::min(b.mn[a], f); b.mx[a] = std::max(b.mx[a], f); }
            }
            for (int a = 0; a < 3; ++a) { out.mn[a] = std::min(out.mn[a], b.mn[a]); out.mx[a] = std::max(out.mx[a], b.mx[a]); }
            r.node_id = p.node_id; r.tri_id = t; r.pad = 0;
            recs.push_back(r); boxes.push_back(b);
        }
    BuiltBvh bvh = build_bvh(boxes, o.max_leaf);
    rebase_bvh(bvh, node_base, prim_base);
    out.num_nodes = bvh.nodes.size(); out.node_capacity = out.num_nodes; out.num_refs = bvh.order.size(); out.num_triangles = recs.size();
    out.nodes = out.num_nodes ? new BvhNode[out.num_nodes] : nullptr;
    out.tris = out.num_refs ? new TriRec[out.num_refs] : nullptr;
    out.uvs = nullptr;
    for (size_t i = 0; i < out.num_nodes; ++i) out.nodes[i] = bvh.nodes[i];
    for (size_t i = 0; i < out.num_refs; ++i) out.tris[i] = recs[bvh.order[i]];
    out.root = bvh.root; out.hairy = false; out.max_depth = bvh.max_depth;
    return NRAYS_OK;
}
void free_device_blas(DeviceBlas& b) {
    delete[] b.nodes; delete[] b.tris;
    b.nodes = nullptr; b.tris = nullptr; b.uvs = nullptr; b.num_nodes = 0; b.num_refs = 0; b.node_capacity = 0;
}

} // namespace nrays

extern "C" hipError_t hipMemcpy(void*, const void*, size_t, hipMemcpyKind) { return hipErrorNotSupported; } // (build_blas_probe's device branch: not reached from here)

namespace {
std::string g_error;
template <typename T> void put(void* dst, const std::vector<T>& v) { if (!v.empty()) std::memcpy(dst, v.data(), v.size() * sizeof(T)); }
} // namespace

extern "C" {

const char* scene_dump_last_error() { return g_error.c_str(); }

// build_host_scene(desc) with NRAYS_GPU_BUILD_MIN = gpu_build_min (0: the library's default) and every other switch at its default; the capacity contract of
// nrays_debug_scene_dump: too small a buffer fills in the sizes and the scalars and returns NRAYS_ERR_BAD_ARG.
int scene_dump_host(const NraysSceneDesc* desc, uint32_t gpu_build_min, NraysSceneDump* out) {
    using namespace nrays;
    if (!desc || !out) { g_error = "null argument"; return NRAYS_ERR_BAD_ARG; }
    Switches sw;
    if (gpu_build_min) sw.gpu_build_min = gpu_build_min;
    HostScene hs;
    int rc = build_host_scene(desc, sw, hs, g_error);
    struct Release { HostScene& h; ~Release() { for (DeviceBlas& b : h.dev_blas) free_device_blas(b); } } release{hs};
    if (rc != NRAYS_OK) return rc;
    std::vector<BvhNode> nodes; std::vector<TriRec> tris;
    for (const DeviceBlas& b : hs.dev_blas) { nodes.insert(nodes.end(), b.nodes, b.nodes + b.num_nodes); tris.insert(tris.end(), b.tris, b.tris + b.num_refs); }
    if (nodes.size() != hs.dev_nodes || tris.size() != hs.dev_tris) { g_error = "dev_nodes / dev_tris are not the device-built arrays' sizes"; return NRAYS_ERR_HIP; }
    nodes.insert(nodes.end(), hs.nodes.begin(), hs.nodes.end()); tris.insert(tris.end(), hs.tris.begin(), hs.tris.end());
    out->num_nodes = (uint32_t)nodes.size(); out->num_tris = (uint32_t)tris.size(); out->num_instances = (uint32_t)hs.instances.size();
    out->num_shadow_instances = (uint32_t)hs.shadow_instances.size(); out->num_planes = (uint32_t)hs.planes.size(); out->num_scene_nodes = (uint32_t)(hs.node_aabbs.size() / 6);
    out->closest_root = hs.closest_root; out->shadow_root = hs.shadow_root; out->max_bvh_depth = hs.max_bvh_depth; out->bounded = hs.bounded ? 1u : 0u;
    out->dev_nodes = (uint32_t)hs.dev_nodes; out->dev_tris = (uint32_t)hs.dev_tris;
    for (int a = 0; a < 3; ++a) { out->bounds_mn[a] = hs.bounds_mn[a]; out->bounds_mx[a] = hs.bounds_mx[a]; }
    if (hs.shadow_planes.size() != hs.planes.size() || hs.links.size() != hs.instances.size() || hs.shadow_links.size() != hs.shadow_instances.size()) {
        g_error = "parallel lists of different lengths"; return NRAYS_ERR_HIP;
    }
    if (out->num_nodes > out->node_capacity || out->num_tris > out->tri_capacity || out->num_instances > out->instance_capacity ||
        out->num_shadow_instances > out->shadow_instance_capacity || out->num_planes > out->plane_capacity || out->num_scene_nodes > out->scene_node_capacity) {
        g_error = "dump buffers too small"; return NRAYS_ERR_BAD_ARG;
    }
    put(out->nodes, nodes); put(out->tris, tris); put(out->instances, hs.instances); put(out->shadow_instances, hs.shadow_instances);
    put(out->links, hs.links); put(out->shadow_links, hs.shadow_links); put(out->planes, hs.planes); put(out->shadow_planes, hs.shadow_planes); put(out->node_aabbs, hs.node_aabbs);
    return NRAYS_OK;
}

} // extern "C"
