// The host compiler's build of build_blas_probe() (nrays_amd/csrc/scene_build.cpp) for tests/test_blas_cover.py: one mesh in, the host builder's BLAS out — the
// 128-byte nodes, the triangle behind every reference, root, depth and the hair-like flag — exactly what nrays_debug_blas_build dumps, without a device.
// Linked with scene_build.cpp, bvh_build.cpp and switches.cpp; the device side's three symbols are stubs that refuse (the host branch never reaches them).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "scene_build.h"

namespace nrays {

int build_blas_device(const std::vector<DeviceMeshPart>&, const DeviceBuildOptions&, int32_t, uint32_t, DeviceBlas&, std::string& err) { err = "no device in this build"; return NRAYS_ERR_UNSUPPORTED; }
void free_device_blas(DeviceBlas&) {}

} // namespace nrays

extern "C" hipError_t hipMemcpy(void*, const void*, size_t, hipMemcpyKind) { return hipErrorNotSupported; }

extern "C" {

// vertices: 3 f64 per vertex (f32-exact), indices: 3 per triangle.  Writes the nodes (32 floats each) and the triangle ids when they fit the capacities;
// info = {root, max_depth, hairy, num_nodes, num_refs}.  Returns the builder's status; `err` receives its message.
int blas_probe_shim_build(uint32_t num_vertices, const double* vertices, uint32_t num_triangles, const uint32_t* indices, int presplit, uint32_t node_capacity,
                          uint32_t ref_capacity, float* nodes, uint32_t* tri_ids, int32_t info[5], char* err, size_t err_capacity) {
    NraysMesh m; std::memset(&m, 0, sizeof m);
    m.num_vertices = num_vertices; m.num_triangles = num_triangles; m.vertices = vertices; m.indices = indices;
    nrays::BlasProbe p; std::string e;
    const int rc = nrays::build_blas_probe(&m, nrays::Switches{}, false, presplit != 0, p, e);
    if (err && err_capacity) std::snprintf(err, err_capacity, "%s", e.c_str());
    if (rc != NRAYS_OK) return rc;
    info[0] = p.root; info[1] = p.max_depth; info[2] = p.hairy ? 1 : 0; info[3] = (int32_t)p.nodes.size(); info[4] = (int32_t)p.tri_ids.size();
    if (p.nodes.size() <= node_capacity && !p.nodes.empty()) std::memcpy(nodes, p.nodes.data(), p.nodes.size() * sizeof(nrays::BvhNode));
    if (p.tri_ids.size() <= ref_capacity && !p.tri_ids.empty()) std::memcpy(tri_ids, p.tri_ids.data(), p.tri_ids.size() * sizeof(uint32_t));
    return rc;
}

} // extern "C"
