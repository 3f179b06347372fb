/* Test shim: the CPU oracle's Scene::trace (src/scene.rs:163-193) on caller-supplied rays, for tests/test_trace_rays*.py.
 * oracle/ exposes only whole frames and single queries; this unit includes its source as it is and adds one entry point. */
#include "../oracle/nrays_oracle.c"

/* out[3i..3i+2] = scene_trace(ray i, depth 0, max_depth); NULL refr / energy -> 1.0, NULL keys -> key i (the library's defaults). */
int trace_oracle_rays(const NraysSceneDesc* desc, uint32_t n, const double* origins, const double* dirs, const double* refr,
                      const float* energy, const uint64_t* keys, uint32_t max_depth, float* out) {
    OScene sc;
    int rc = oscene_build(&sc, desc);
    if (rc != NRAYS_OK) { oscene_free(&sc); return rc; }
    Counters cnt;
    memset(&cnt, 0, sizeof cnt);
    for (uint32_t i = 0; i < n; ++i) {
        RayWE r;
        r.ray.o = V(origins[3 * (size_t)i], origins[3 * (size_t)i + 1], origins[3 * (size_t)i + 2]);
        r.ray.d = V(dirs[3 * (size_t)i], dirs[3 * (size_t)i + 1], dirs[3 * (size_t)i + 2]);
        r.refr = refr ? refr[i] : 1.0;
        r.energy = energy ? energy[i] : 1.0f;
        r.key = keys ? keys[i] : (uint64_t)i;
        c3 c = scene_trace(&sc, &r, 0, max_depth, &cnt);
        out[3 * (size_t)i] = c.x; out[3 * (size_t)i + 1] = c.y; out[3 * (size_t)i + 2] = c.z;
    }
    oscene_free(&sc);
    return NRAYS_OK;
}
