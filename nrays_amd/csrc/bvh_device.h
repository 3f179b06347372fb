// bvh_device.h — device-side BLAS build for large TriMesh groups (bvh_device.hip): triangle records, pre-splitting, the binned-SAH
// binary build, the 4-wide collapse in the host builder's depth-first layout and the leaf-ordered triangle copies all run on the
// GPU.  Same split rule, same arithmetic as bvh_build.cpp / scene_build.cpp (the tree is the one the host builder produces from
// the same references); replaces ncollide's BVT::new_balanced inside TriMesh::new (examples/loader3d.rs:695) like they do.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/nrays_abi.h"
#include "device_types.h"

namespace nrays {

struct DeviceMeshPart { // one TriMesh node of the group sharing a BLAS
    const double* vertices; // host, 3 * num_vertices
    const double* uvs;      // host, 2 * num_vertices, or null
    const uint32_t* indices; // host, 3 * num_triangles
    uint32_t num_vertices, num_triangles;
    uint32_t node_id;
};

struct DeviceBlas {
    BvhNode* nodes = nullptr; size_t num_nodes = 0; // device memory; child refs already absolute (node_base / prim_base applied)
    size_t node_capacity = 0;                        // nodes the allocation holds (>= num_nodes: room for the scene's host-built nodes behind them)
    TriRec* tris = nullptr; TriUv* uvs = nullptr; size_t num_refs = 0; // device memory, leaf order
    int32_t root = kEmptyChild;
    float mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0}; // local bounds of the triangles
    bool hairy = false;
    int max_depth = 0;
    size_t num_triangles = 0;
};

struct DeviceBuildOptions {
    int max_leaf = 8;
    float prim_cost = 1.0f, prim_cost_hairy = 0.7f;
    double budget = 1.0, budget_hairy = 5.0, min_gain = 1.0, min_gain_hairy = 0.02, hairy_emptiness = 0.9;
    bool presplit = true;
    int debug_cap_div = 1;    // NRAYS_DEBUG_BUILD_CAPS=n (tests): the builder's internal lists get 1 / n of their capacity, so that their overflow path — an error the caller answers with the host builder — runs
    uint32_t split_grid_max = 512; // NRAYS_SPLIT_GRID: most workgroups of k_presplit (each thread owns a 6.9 KB stack of frames)
    bool one_walk = true;     // NRAYS_PRESPLIT_ONE_WALK=0: pre-splitting walks twice instead of keeping the pieces of its last counting pass (A/B)
    uint32_t debug_piece_cap = 0; // NRAYS_DEBUG_PIECE_CAP=c (tests): c places per piece region — the regions overflow and the second walk takes over (0: sized by the budget)
    bool verbose = false;     // NRAYS_BUILD_TIMES: the builder's stage times on stderr
    size_t node_tail = 16384; // spare node slots behind the BLAS: a scene with ONE device-built BLAS adopts its arrays as they are (no second copy of GBs)
};

// Builds the BLAS of `parts` on the current device.  Returns NRAYS_OK or a negative NraysStatus with `err` set.
// node_base / prim_base: position of this BLAS's first node / first triangle slot in the scene's final arrays.
int build_blas_device(const std::vector<DeviceMeshPart>& parts, const DeviceBuildOptions& opt, int32_t node_base, uint32_t prim_base,
                      DeviceBlas& out, std::string& err);
void free_device_blas(DeviceBlas& b);

// Why either builder refuses a mesh; k_tri_records reports them as bits 0, 1, 2 of its error word, in this order.  Sets `err`, returns the status.
enum MeshError { kMeshIndexRange = 0, kMeshVertexInexact = 1, kMeshUvInexact = 2 };
inline int refuse_mesh(MeshError why, std::string& err) {
    static const char* const text[3] = {"triangle index out of range", "mesh vertex coordinate is not exactly representable in f32 (see DESIGN.md: f32-exact mesh storage)",
                                        "mesh uv is not exactly representable in f32"};
    err = text[why];
    return why == kMeshIndexRange ? NRAYS_ERR_BAD_ARG : NRAYS_ERR_UNSUPPORTED;
}

} // namespace nrays
