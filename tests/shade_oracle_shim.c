/* Test shim: the CPU oracle's Material::compute (src/material.rs:8-16, src/phong_material.rs:72-151) on caller-supplied surface points, for
 * tests/test_shade_points*.py.  oracle/ exposes only whole frames and single queries; this unit includes its source as it is and adds one entry point. */
#include "../oracle/nrays_oracle.c"

/* out[4i..4i+3] = material(nodes[i]).compute(ray with dir view_dirs[i] and key i's, points[i], normals[i], uvs[i]) — the arrays and the skip rule of
 * nrays_shade_points: NULL uvs -> no point has a uv; hit_flags bit 0 clear, nodes[i] < 0 or >= the node count -> (0, 0, 0, 0); bit 1 -> the point
 * carries its uv; NULL hit_flags -> every point is shaded, with a uv exactly when uvs is there; NULL keys -> key i. */
int shade_oracle_points(const NraysSceneDesc* desc, uint32_t n, const double* points, const double* normals, const double* view_dirs, const double* uvs,
                        const int32_t* nodes, const uint32_t* hit_flags, const uint64_t* keys, float* out) {
    OScene sc;
    int rc = oscene_build(&sc, desc);
    if (rc != NRAYS_OK) { oscene_free(&sc); return rc; }
    Counters cnt;
    memset(&cnt, 0, sizeof cnt);
    for (uint32_t i = 0; i < n; ++i) {
        const size_t i3 = 3 * (size_t)i;
        const uint32_t hf = hit_flags ? hit_flags[i] : 3u;
        c4 c = {0.0f, 0.0f, 0.0f, 0.0f};
        if ((hf & 1u) && nodes[i] >= 0 && nodes[i] < sc.nnodes) {
            RayWE r;
            r.ray.o = V(0.0, 0.0, 0.0);
            r.ray.d = V(view_dirs[i3], view_dirs[i3 + 1], view_dirs[i3 + 2]);
            r.refr = 1.0; r.energy = 1.0f;
            r.key = keys ? keys[i] : (uint64_t)i;
            Inter in;
            in.toi = 0.0; in.prim = 0;
            in.normal = V(normals[i3], normals[i3 + 1], normals[i3 + 2]);
            in.has_uv = uvs && (hf & 2u);
            in.u = in.has_uv ? uvs[2 * (size_t)i] : 0.0; in.v = in.has_uv ? uvs[2 * (size_t)i + 1] : 0.0;
            c = material_compute(&sc, &desc->materials[sc.nodes[nodes[i]].d.material_id], &r, V(points[i3], points[i3 + 1], points[i3 + 2]), &in, &cnt);
        }
        out[4 * (size_t)i] = c.x; out[4 * (size_t)i + 1] = c.y; out[4 * (size_t)i + 2] = c.z; out[4 * (size_t)i + 3] = c.w;
    }
    oscene_free(&sc);
    return NRAYS_OK;
}
