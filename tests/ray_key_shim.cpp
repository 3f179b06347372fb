// The host compiler's build of nrays_amd/csrc/ray_key.h (tests/test_ray_order.py, tests/test_ray_order_gpu.py): the frame and the keys
// of a batch exactly as the device code computes them.
#include <cstdint>

#include "ray_key.h"

using namespace nrays;

extern "C" {

// out = {K, B, doubles of a frame}
void ray_key_constants(int32_t out[3]) { out[0] = kRayKeyBits; out[1] = kRayBinBits; out[2] = kRayFrameDoubles; }

// The frame of n rays; box = the scene's bounding box {min xyz, max xyz}.  Merged in `parts` interleaved partial bounds, as a grid does.
void ray_key_frame(uint32_t n, const double* origins, const double* dirs, const double* box, uint32_t parts, double* frame) {
    if (parts == 0u) parts = 1u;
    RayBounds total; rk_bounds_init(total);
    for (uint32_t p = 0; p < parts; ++p) {
        RayBounds b; rk_bounds_init(b);
        for (uint32_t i = p; i < n; i += parts) rk_bounds_add(b, origins + 3 * (uint64_t)i, dirs + 3 * (uint64_t)i, box);
        rk_bounds_merge(total, b);
    }
    rk_frame_finish(total, box, frame);
}

void ray_key_keys(uint32_t n, const double* origins, const double* dirs, const double* frame, uint64_t* keys) {
    RayKeyFrame f; rk_frame_decode(frame, f);
    for (uint32_t i = 0; i < n; ++i) keys[i] = rk_key(f, origins + 3 * (uint64_t)i, dirs + 3 * (uint64_t)i);
}

uint32_t ray_key_octant(const double* frame, uint64_t key) { RayKeyFrame f; rk_frame_decode(frame, f); return rk_key_octant(f, key); }

} // extern "C"
