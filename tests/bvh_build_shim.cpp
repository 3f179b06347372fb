// The host compiler's build of nrays_amd/csrc/bvh_build.cpp (tests/test_stack_spill.py, tests/test_stack_spill_gpu.py): the 4-wide tree
// build_bvh returns over a list of primitive boxes, in the 128-byte node layout of device_types.h — what nrays_debug_blas_build dumps.
#include <cstdint>
#include <cstring>
#include <vector>

#include "bvh_build.h"

using namespace nrays;

extern "C" {

// boxes: n x {min x, y, z, max x, y, z}.  Writes up to node_capacity nodes (32 floats each) and the n entries of `order` (the primitive
// behind each leaf slot); info = {root, max_depth}.  Returns the number of nodes of the tree, whether they fitted or not.
uint32_t bvh_shim_build(uint32_t n, const float* boxes, int32_t max_leaf, float prim_cost, uint32_t node_capacity, float* nodes, uint32_t* order, int32_t info[2]) {
    std::vector<PrimBounds> pb(n);
    for (uint32_t i = 0; i < n; ++i)
        for (int a = 0; a < 3; ++a) { pb[i].mn[a] = boxes[6 * (size_t)i + a]; pb[i].mx[a] = boxes[6 * (size_t)i + 3 + a]; }
    const BuiltBvh b = build_bvh(pb, max_leaf, prim_cost);
    info[0] = b.root; info[1] = b.max_depth;
    if (b.nodes.size() <= node_capacity && !b.nodes.empty()) std::memcpy(nodes, b.nodes.data(), b.nodes.size() * sizeof(BvhNode));
    std::memcpy(order, b.order.data(), (size_t)n * sizeof(uint32_t));
    return (uint32_t)b.nodes.size();
}

} // extern "C"
