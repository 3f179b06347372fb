/*
 * nrays_abi.h — C ABI of the MI355X-native replacement for nrays' per-pixel trace loop.
 *
 * This is the drop-in boundary for `scene::render` (reference src/scene.rs:29-36) and for the
 * construction surface that feeds it (`Scene::new` src/scene.rs:119, `SceneNode::new`
 * src/scene_node.rs:22-47, `Light::new` src/light.rs:16, `PhongMaterial::new`
 * src/phong_material.rs:19-26).  A host written in any language (the reference is Rust) fills
 * the POD descriptors below once per scene and calls `nrays_scene_create`; every later
 * `scene::render` becomes one `nrays_render` call.  INTEGRATION.md shows the Rust `extern "C"`
 * binding a maintainer would add.
 *
 * Rules of the boundary
 *   - plain C, `extern "C"`, POD structs only (`#[repr(C)]` on the Rust side), no exceptions;
 *   - the library copies everything it needs inside `nrays_scene_create`; the caller keeps
 *     ownership of every pointer it passes;
 *   - every entry point returns 0 (NRAYS_OK) or a negative NraysStatus; it never aborts
 *     (the reference panics / silently swallows thread panics, src/scene.rs:111 — not reproduced);
 *   - `nrays_last_error()` returns a thread-local, NUL-terminated description of the last failure.
 *
 * The same descriptors are consumed by the CPU oracle (oracle/nrays_oracle.c), which is test
 * infrastructure and is NOT part of this library.
 */
#ifndef NRAYS_ABI_H
#define NRAYS_ABI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever the exported surface grows or a struct changes: 3 = + nrays_debug_blas_build / NraysBlasDump, nrays_multi_get_timings / NraysMultiTimings (round 4); 4 = NraysStats::rays_shadow_elided (round 5); 5 = NraysStats::node_fetches, nrays_render_device_counted, NraysTileCosts::shader_clock_hz / kernel_ms (round 6); 6 = nrays_trace_rays_device / nrays_trace_rays /
 * nrays_intersects_rays_device (caller-supplied rays); 7 = nrays_debug_last_permutation.
 * Added after 7 WITHOUT a bump (plain functions over plain arrays, no struct): nrays_trace_rays_device_ex / nrays_trace_rays_ex /
 * nrays_intersects_rays_device_ex / nrays_debug_ray_order / nrays_cast_rays_device / nrays_cast_rays / nrays_shade_points_device /
 * nrays_shade_points / nrays_occlusion_points_device / nrays_occlusion_points / nrays_debug_occlusion_rays (their struct NraysOcclusionParams
 * is new with them and changes no other) / nrays_gather_points_device / nrays_gather_points (their struct NraysGatherParams likewise) / nrays_gather_points_device_ex / nrays_gather_points_ex / nrays_debug_gather_order / nrays_surface_texels_device / nrays_surface_texels / nrays_debug_surface_texels_passes / nrays_debug_pipeline_counts / nrays_dilate_texels_device / nrays_dilate_texels / nrays_filter_texels_device / nrays_filter_texels / nrays_gather_sh_points_device / nrays_gather_sh_points / nrays_debug_gather_sh_fold / nrays_gather_maps_points_device / nrays_gather_maps_points (their struct NraysGatherMapsParams likewise) / nrays_irradiance_points_device / nrays_irradiance_points (their struct NraysIrradianceGrid likewise) / nrays_probe_depth_points_device / nrays_probe_depth_points (their struct NraysProbeDepthParams likewise) / nrays_irradiance_points_vis_device / nrays_irradiance_points_vis (their struct NraysIrradianceVisibility likewise) / nrays_gather_maps_sh_points_device / nrays_gather_maps_sh_points (their struct NraysGatherDepthSpec likewise) / nrays_material_points_device / nrays_material_points / nrays_nearest_points_device / nrays_nearest_points / nrays_debug_nearest_bound / nrays_debug_scene_dump (its struct NraysSceneDump likewise) / nrays_light_points_device / nrays_light_points / nrays_debug_light_rays (their struct NraysPointLights likewise).  A caller that may meet an older version-7 library finds them by symbol lookup. */
#define NRAYS_ABI_VERSION 7

typedef enum NraysStatus {
    NRAYS_OK = 0,
    NRAYS_ERR_BAD_ARG = -1,        /* NULL pointer, ray_per_pixel == 0 (src/scene.rs:37), bad index */
    NRAYS_ERR_HIP = -2,            /* a HIP runtime call failed */
    NRAYS_ERR_OOM = -3,            /* host or device allocation failed */
    NRAYS_ERR_UNSUPPORTED = -4,    /* e.g. mesh vertices that are not f32-exact */
    NRAYS_ERR_NO_DEVICE = -5,      /* no gfx950 device visible to the process */
    NRAYS_ERR_QUEUE_OVERFLOW = -6, /* continuation-ray queue capacity exceeded */
    NRAYS_ERR_RCCL = -7            /* an RCCL call failed (multi-GPU entry points) */
} NraysStatus;

/* Shapes the loader can construct (examples/loader3d.rs:593-695). */
typedef enum NraysShapeKind {
    NRAYS_SHAPE_BALL = 0,     /* params[0] = radius                      (loader3d.rs:601) */
    NRAYS_SHAPE_CUBOID = 1,   /* params[0..2] = half extents             (loader3d.rs:612) */
    NRAYS_SHAPE_CYLINDER = 2, /* params[0] = half height, params[1] = radius, axis = local Y (:623) */
    NRAYS_SHAPE_CAPSULE = 3,  /* params[0] = half height, params[1] = radius               (:634) */
    NRAYS_SHAPE_CONE = 4,     /* params[0] = half height, params[1] = radius, apex at +Y   (:645) */
    NRAYS_SHAPE_PLANE = 5,    /* params[0..2] = unit normal, through the local origin      (:656) */
    NRAYS_SHAPE_TRIMESH = 6   /* mesh_id selects an NraysMesh                              (:695) */
} NraysShapeKind;

/* Material implementations that can cross the boundary (src/material.rs:6-17). */
typedef enum NraysMaterialKind {
    NRAYS_MAT_PHONG = 0,  /* src/phong_material.rs:9-152 */
    NRAYS_MAT_NORMAL = 1, /* src/normal_material.rs:5-22 */
    NRAYS_MAT_UV = 2      /* src/uv_material.rs:6-28 */
} NraysMaterialKind;

typedef enum NraysTexelFormat {
    NRAYS_TEXEL_RGBA8 = 0,  /* 4 x u8; sampled as `u8 as f32 / 255.0` (src/texture2d.rs:111-162) */
    NRAYS_TEXEL_RGBA32F = 1 /* 4 x f32, the reference's own in-memory form (Point4<f32>) */
} NraysTexelFormat;

typedef enum NraysInterpolation { NRAYS_INTERP_BILINEAR = 0, NRAYS_INTERP_NEAREST = 1 } NraysInterpolation;
typedef enum NraysOverflow { NRAYS_OVERFLOW_WRAP = 0, NRAYS_OVERFLOW_CLAMP = 1 } NraysOverflow;

/* src/light.rs:8-23.  `racsample` is already floor(sqrt(nsample)) (light.rs:20). */
typedef struct NraysLight {
    double pos[3];
    double radius;
    uint32_t racsample;
    float color[3];
} NraysLight;

/* src/texture2d.rs:10-76.  Row 0 is the BOTTOM row of the image: the Y flip of
 * texture2d.rs:99-107 has already been applied by whoever decoded the file, and so has the
 * depth/opacity decode of :109-177 (opaque -> (r,g,b,1); opacity map -> (1,1,1,a)). */
typedef struct NraysTexture {
    uint32_t width;
    uint32_t height;
    uint32_t format;   /* NraysTexelFormat */
    uint32_t interp;   /* NraysInterpolation */
    uint32_t overflow; /* NraysOverflow */
    uint32_t reserved;
    const void* texels; /* width*height texels, row-major, index y*width + x (texture2d.rs:204) */
} NraysTexture;

/* src/phong_material.rs:9-26 for PHONG; the colour fields are ignored for NORMAL / UV. */
typedef struct NraysMaterial {
    uint32_t kind; /* NraysMaterialKind */
    float ambiant[3];
    float diffuse[3];
    float specular[3];
    float shininess;
    int32_t texture_id;       /* index into textures, or -1 */
    int32_t alpha_texture_id; /* index into textures, or -1 */
} NraysMaterial;

/* ncollide3d TriMesh::new(points, indices, uvs) as called at examples/loader3d.rs:695.
 * Several meshes may alias the same `vertices` / `uvs` arrays (one SceneNode per OBJ group,
 * each holding the whole vertex array and only its faces, loader3d.rs:690-695). */
typedef struct NraysMesh {
    uint32_t num_vertices;
    uint32_t num_triangles;
    const double* vertices;  /* 3*num_vertices, local space; must be f32-exact (obj.rs:197-205 parses f32) */
    const double* uvs;       /* 2*num_vertices or NULL */
    const uint32_t* indices; /* 3*num_triangles */
} NraysMesh;

/* One SceneNode (src/scene_node.rs:8-47).  The transform is given as the loader builds it:
 * Isometry3::new(translation, axis_angle) (examples/loader3d.rs:546-552), i.e. `axis_angle` is a
 * scaled-axis rotation in RADIANS (|axis_angle| = angle), not Euler angles. */
typedef struct NraysNode {
    uint32_t shape_kind; /* NraysShapeKind */
    uint32_t solid;      /* 0/1, scene_node.rs:13 */
    double params[3];
    double translation[3];
    double axis_angle[3];
    float refl_mix;
    float refl_atenuation;
    float alpha;
    float reserved0;
    double refr_coeff;
    uint32_t material_id;
    int32_t mesh_id; /* for NRAYS_SHAPE_TRIMESH, else -1 */
} NraysNode;

/* Everything `Scene::new(nodes, lights, background)` receives (src/scene.rs:119-133). */
typedef struct NraysSceneDesc {
    float background[3];
    uint32_t num_lights;
    const NraysLight* lights;
    uint32_t num_materials;
    const NraysMaterial* materials;
    uint32_t num_textures;
    const NraysTexture* textures;
    uint32_t num_meshes;
    const NraysMesh* meshes;
    uint32_t num_nodes;
    const NraysNode* nodes;
} NraysSceneDesc;

/* Arguments of scene::render (src/scene.rs:29-36) plus extensions whose zero value preserves the
 * reference behaviour. */
typedef struct NraysRenderParams {
    uint32_t width;           /* resolution.x */
    uint32_t height;          /* resolution.y */
    uint32_t ray_per_pixel;   /* must be > 0 (scene.rs:37) */
    uint32_t max_depth;       /* 0 = energy rule only (scene.rs:204); else extra cap on trace depth.
                                 A hard safety cap of 64 generations always applies (unbounded
                                 refraction recursion in the reference, scene.rs:246). */
    double window_width;      /* AA jitter window in pixels (scene.rs:75) */
    double camera_eye[3];
    double inv_proj_view[16]; /* (P*V)^-1, COLUMN-major as nalgebra stores Matrix4 (loader3d.rs:77-79) */
    uint64_t seed;            /* counter-based RNG seed (reference RNG is OS-seeded, scene.rs:75) */
    /* Framebuffer tiling (multi-GPU): rows are grouped in bands of `band_rows`; band b is rendered
     * iff b % band_owners == band_owner.  band_rows == 0 renders the whole frame.  The output of a
     * tiled render is the compact buffer of the owner's bands in increasing order: nrays_tile_rows(params)
     * rows, the same for every owner.  The rows of it behind the owner's last real row — the part of a
     * ragged last band below the frame, and a whole band where the owner holds one band fewer than others —
     * are padding rows: every render writes them, as exactly +0.0 in every float (0 in nrays_render_rgb8). */
    uint32_t band_rows;
    uint32_t band_owner;
    uint32_t band_owners;
    uint32_t reserved;
} NraysRenderParams;

/* Counters of the last render of a scene (or of an oracle render).  A "ray" is one BVT query
 * (`world.best_first_search`, src/scene.rs:153,166). */
typedef struct NraysStats {
    uint64_t rays_primary;    /* scene.rs:89 */
    uint64_t rays_reflection; /* scene.rs:209 */
    uint64_t rays_refraction; /* scene.rs:246 */
    uint64_t rays_shadow;     /* scene.rs:153 */
    uint64_t node_tests;      /* AABB tests (TLAS + BLAS); filled by instrumented renders only */
    uint64_t tri_tests;       /* ray/triangle tests */
    uint64_t prim_tests;      /* analytic primitive / instance tests */
    uint64_t hit_records;     /* node + material records fetched at accepted hits */
    uint64_t tex_samples;     /* texture samples (4 taps each when bilinear) */
    uint32_t generations;     /* continuation generations executed */
    uint32_t instrumented;    /* 1 if the traversal counters above are valid */
    double kernel_ms_primary; /* mean GPU time of the primary kernel launch (HIP events on the render stream) */
    double kernel_ms_total;   /* mean GPU time of a whole render, first launch to last */
    uint32_t frames_timed;    /* renders averaged in the two figures above (since the previous get_stats): the events
                                 are recorded on every 4th render of a handle and on every instrumented one */
    uint32_t reserved;
    uint64_t rays_primary_traced; /* instrumented renders only: primary rays that went through a BVT query: rays_primary minus the ones whose wave tile was
                                     decided without one (outside the scene's screen bounds, or no ray of the tile passes the
                                     root of the BVT) — the pixels are the same, the reference would have queried for them */
    uint64_t rays_shadow_elided;  /* part of rays_shadow: shadow rays the reference traces although their result is multiplied by exactly 0 — light samples
                                     behind the surface (diffuse and specular coefficients both 0: phong_material.rs:109-141) and the samples of hits that
                                     contribute nothing of their own to the pixel (a fully transparent point: opacity-map texel 0 or node alpha 0; a perfect
                                     mirror: scene.rs:179-190).  Counted, so that rays_shadow stays the reference's number, but not traced by plain
                                     renders; instrumented renders trace them: 0 (NRAYS_COUNT_AS_TIMED: they skip them like a plain render and report them here) */
    uint64_t node_fetches;        /* instrumented renders only: 128-byte BVH node records fetched — ONE per wave for a visit in which every active lane sits on the same
                                     node with the same direction signs (the kernels read it through the scalar unit and broadcast), one per lane otherwise.
                                     node_fetches * 128 is the traversal's unique node traffic; node_tests * 32 counts a box per lane whoever fetched it */
} NraysStats;

/* Threading contract of a scene handle: the library is re-entrant on DISTINCT handles (any threads, any streams).
 * ONE handle must not be used by two threads at the same time (its calls must be serialised by the caller); its
 * renders execute in call order — a render enqueued on another stream than its predecessor is ordered behind it by
 * the library — because the handle owns per-frame device state (counters, continuation queues, per-camera scheduling state, tile
 * costs).  The environment switches NRAYS_MAX_PRIMARY / NRAYS_GRAB / NRAYS_LPT (tests and A/B runs) are read once,
 * by nrays_scene_create. */
typedef struct NraysScene NraysScene; /* opaque */

/* Builds the device-resident scene on the CURRENT HIP device of the calling thread: flattens the
 * nodes, builds the BVHs, uploads.  Replaces Scene::new + BVT::new_balanced (src/scene.rs:119-133). */
int nrays_scene_create(const NraysSceneDesc* desc, NraysScene** out_scene);

/* Replaces scene::render (src/scene.rs:29-116).  `out_rgb` is HOST memory, caller-allocated,
 * rows*width*3 floats, row-major, index (i + j*width)*3 (scene.rs:104), where rows = height for an
 * untiled render and nrays_tile_rows(params) for a tiled one.  Blocking. */
int nrays_render(NraysScene* scene, const NraysRenderParams* params, float* out_rgb);

/* The same frame as 8-bit RGB, quantised on the device exactly as Image::to_png does on the host (src/image.rs:66-76:
 * c * 255, clamped to [0, 255], truncated; NaN -> 0): what the loader3d front-end writes into its PNG, at a quarter of
 * the device-to-host bytes of nrays_render.  `out_rgb8` is HOST memory, rows*width*3 bytes, same indexing.  Blocking. */
int nrays_render_rgb8(NraysScene* scene, const NraysRenderParams* params, uint8_t* out_rgb8);

/* Same, but `out_rgb_device` is DEVICE memory on the scene's device and the work is enqueued on
 * `hip_stream` (a hipStream_t, NULL = default stream) without a final synchronisation unless the
 * scene needs host-side generation control (transparent scenes). */
int nrays_render_device(NraysScene* scene, const NraysRenderParams* params, float* out_rgb_device,
                        void* hip_stream);

/* As nrays_render_device, with the traversal counters of NraysStats collected (slower). */
int nrays_render_device_instrumented(NraysScene* scene, const NraysRenderParams* params,
                                     float* out_rgb_device, void* hip_stream);

/* As nrays_render_device_instrumented, with a choice of WHAT is counted.  flags = 0: the reference algorithm — every ray scene.rs / phong_material.rs trace is traced
 * and counted.  NRAYS_COUNT_AS_TIMED: the work of the PLAIN (timed) render of this scene — the shadow rays whose result is multiplied by exactly 0 are skipped as the
 * plain kernels skip them (and reported in rays_shadow_elided), so that node / triangle / hit / texture counts are those of the kernel whose time a roofline divides by
 * (bench.py: roofline_block).  Pixels are the same either way. */
#define NRAYS_COUNT_AS_TIMED 1u
int nrays_render_device_counted(NraysScene* scene, const NraysRenderParams* params, float* out_rgb_device, void* hip_stream, uint32_t flags);

/* Scene::trace (src/scene.rs:163-193) on n caller-supplied rays: out_rgb[3i..3i+2] = trace(ray i), with the reflection / refraction recursion,
 * the lights and the generation rules of a render.  Replaces direct calls of scene.trace (own camera models, light / AO baking, picking).
 *   origins, dirs  n x 3 doubles, xyz interleaved.  Directions are used as given: unit length is expected (every ray the reference builds is
 *                  normalised, scene.rs:87,200,236); the library does not normalise.
 *   refr           n doubles, RayWithEnergy::refr; NULL = 1.0 for every ray (RayWithEnergy::new, ray_with_energy.rs:11).
 *   energy         n floats, RayWithEnergy::energy; NULL = 1.0.
 *   keys           n RNG path keys (area-light sampling hashes them exactly as a render hashes a primary ray's); NULL = the key of ray i is i.
 *   max_depth      as NraysRenderParams::max_depth (0 = the energy rule only; the hard cap of 64 generations applies); the input rays are depth 0.
 *   out_rgb        n x 3 floats.
 * NULL scene / origins / dirs / out_rgb -> NRAYS_ERR_BAD_ARG; n == 0 -> NRAYS_OK without work; a continuation-queue overflow ->
 * NRAYS_ERR_QUEUE_OVERFLOW.  The rays are traced in chunks of at most 2^22 (results do not depend on it) with a workspace the handle owns
 * (allocated on first use, grown only when a chunk needs more, freed by nrays_scene_destroy).  A batch follows the handle's threading
 * contract and leaves what the handle reports about its renders (nrays_get_stats, nrays_get_primary_kernel_stats, nrays_get_tile_costs) and
 * its per-camera scheduling state untouched.
 * Every pointer is DEVICE memory on the scene's device and the work is enqueued on `hip_stream` (a hipStream_t, NULL = default stream)
 * without a final synchronisation unless the scene needs host-side generation control (transparent scenes). */
int nrays_trace_rays_device(NraysScene* scene, uint32_t n, const double* origins, const double* dirs, const double* refr, const float* energy,
                            const uint64_t* keys, uint32_t max_depth, float* out_rgb, void* hip_stream);

/* Same, every pointer HOST memory.  Blocking. */
int nrays_trace_rays(NraysScene* scene, uint32_t n, const double* origins, const double* dirs, const double* refr, const float* energy,
                     const uint64_t* keys, uint32_t max_depth, float* out_rgb);

/* Scene::intersects_ray (src/scene.rs:147-161), the transparent-shadow query, on n caller-supplied rays with max_toi[i]: out_lit[i] = 1 and
 * out_filter[3i..3i+2] = the colour filter where the reference returns Some(filter), out_lit[i] = 0 and out_filter = (0, 0, 0) where it
 * returns None.  origins / dirs n x 3 doubles, max_toi n doubles, out_filter n x 3 floats, out_lit n words; all DEVICE memory, enqueued on
 * `hip_stream` without synchronisation.  NULL arguments -> NRAYS_ERR_BAD_ARG; n == 0 -> NRAYS_OK. */
int nrays_intersects_rays_device(NraysScene* scene, uint32_t n, const double* origins, const double* dirs, const double* max_toi,
                                 float* out_filter, uint32_t* out_lit, void* hip_stream);

/* The three entry points above with `flags`.  flags == 0 IS the entry point without _ex: the same kernels with the same arguments.  Any bit
 * other than the ones below -> NRAYS_ERR_BAD_ARG.  Everything else of their contracts holds unchanged.
 *   NRAYS_RAYS_UNORDERED  a statement about the INPUT, like the coherent / incoherent hints of other ray-casting libraries: the rays come in
 *                         no useful order (baking, ambient occlusion, shuffled or gathered rays), so the library may trace them in an order
 *                         of its own.  It then computes a spatial key per ray on the device (origin cell, direction signs, direction cell, in
 *                         a frame fitted to each chunk), bins the rays of the chunk by it and traces them bin by bin; every result is written
 *                         to the slot of the ray it belongs to and is BIT-IDENTICAL to the unhinted call's — only the time changes.  The
 *                         inputs are not modified; the reorder is launches on the same stream, without read-back or synchronisation.  The
 *                         library cannot find incoherence out cheaply itself (that is reading the whole batch once more); under the hint it
 *                         still skips the reorder where the host can see that it does not pay (small batches).  NRAYS_RAY_REORDER=0 in the
 *                         environment of nrays_scene_create: never reorder; =2: reorder every hinted batch whatever its size. */
#define NRAYS_RAYS_UNORDERED 1u
int nrays_trace_rays_device_ex(NraysScene* scene, uint32_t n, const double* origins, const double* dirs, const double* refr, const float* energy,
                               const uint64_t* keys, uint32_t max_depth, float* out_rgb, uint32_t flags, void* hip_stream);
int nrays_trace_rays_ex(NraysScene* scene, uint32_t n, const double* origins, const double* dirs, const double* refr, const float* energy,
                        const uint64_t* keys, uint32_t max_depth, float* out_rgb, uint32_t flags);
int nrays_intersects_rays_device_ex(NraysScene* scene, uint32_t n, const double* origins, const double* dirs, const double* max_toi,
                                    float* out_filter, uint32_t* out_lit, uint32_t flags, void* hip_stream);

/* Scene::trace's closest-hit query (src/scene.rs:164-166, 262-283) with the record SceneNode::cast returns (src/scene_node.rs:51-54) on n
 * caller-supplied rays: WHICH node ray i meets first, where, with which normal and uv (picking, depth / normal / id passes, the first hop of
 * a baker that builds its own secondary rays).  The query is the one a render's shading runs: ties between nodes and triangles are broken
 * the same way and every accepted hit has passed the reference's exact AABB gates.
 *   origins, dirs  n x 3 doubles, xyz interleaved; directions are used as given (nrays_trace_rays_device).
 *   max_toi        n doubles, or NULL = unbounded.  The answer is that of the unbounded query if its toi <= max_toi[i] and a miss otherwise,
 *                  bit for bit (the bound filters the finished query; it never changes which hit wins).  +inf = unbounded, NaN = a miss.
 *   out_toi        n doubles, required.          out_node   n scene-node indices, required.
 *   out_normal     n x 3 doubles, world space.   out_uv     n x 2 doubles (zeros where the record carries none).
 *   out_prim       n: the triangle's index in its NraysMesh::indices (triangle t = indices[3t..3t+2]), -1 for an analytic shape.
 *   out_flags      n: the bits of NraysCastResult::flags — bit 0 = hit, bit 1 = the record carries uvs.
 *                  Each of these four may be NULL: that output is then not computed into memory at all (no store).
 * A miss writes out_node = -1, out_toi = +inf, zeros in out_normal and out_uv, out_prim = -1, out_flags = 0; a hit's toi is finite, so depth
 * compares and minima work on out_toi directly.
 *   flags          0 or NRAYS_RAYS_UNORDERED (same meaning, threshold and reorder as for the other batches; results bit-identical); any other
 *                  bit -> NRAYS_ERR_BAD_ARG.
 * NULL scene / origins / dirs / out_toi / out_node -> NRAYS_ERR_BAD_ARG; n == 0 -> NRAYS_OK without work.  Otherwise the contract of
 * nrays_intersects_rays_device: every pointer DEVICE memory on the scene's device, chunks of at most 2^22 rays, enqueued on `hip_stream`
 * without read-back or synchronisation, ordered behind the handle's previous work; what the handle reports about its renders and its
 * per-camera scheduling state stay untouched. */
int nrays_cast_rays_device(NraysScene* scene, uint32_t n, const double* origins, const double* dirs, const double* max_toi,
                           double* out_toi, int32_t* out_node, double* out_normal, double* out_uv, int32_t* out_prim,
                           uint32_t* out_flags, uint32_t flags, void* hip_stream);
/* Same, every pointer HOST memory.  Blocking. */
int nrays_cast_rays(NraysScene* scene, uint32_t n, const double* origins, const double* dirs, const double* max_toi,
                    double* out_toi, int32_t* out_node, double* out_normal, double* out_uv, int32_t* out_prim,
                    uint32_t* out_flags, uint32_t flags);

/* Material::compute (src/material.rs:8-16, src/phong_material.rs:72-151) on n caller-supplied surface points: the direct lighting of point i with
 * the material of scene node nodes[i] — the ambient term with the texture and opacity-map samples, per light Light::sample's jittered
 * positions, one transparent-shadow query per sample, the Phong diffuse and specular terms folded light after light.  It is the value
 * Scene::trace gets from `sn.material.compute(ray, &pt, &inter.normal, &uvs, self)`, on its own: no closest-hit traversal, no reflection, no
 * refraction (light-map and vertex bakers; the second step of nrays_cast_rays_device -> own shading; deferred shading of a camera's hits).
 *   out_rgba       n x 4 floats, the reference's Point4<f32>: the lit colour and, in w, the MATERIAL's alpha (the opacity-map sample, or 1) —
 *                  as compute returns it, before the node's alpha is multiplied in.
 *   points         n x 3 doubles, world space, used as given.
 *   normals        n x 3 doubles, used as given; unit length is expected, as the casts return it.
 *   view_dirs      n x 3 doubles, required: `ray.ray.dir`, the direction the viewer looks along, TOWARDS the surface.  It feeds the specular term;
 *                  nothing else of the ray is read.
 *   uvs            n x 2 doubles, or NULL = None for every point.
 *   nodes          n scene-node indices (the values out_node of nrays_cast_rays_device holds).  The node only selects the material; its alpha,
 *                  refl_mix and refr_coeff are not applied (that is Scene::trace's business).
 *   hit_flags      n words, or NULL: the bits of out_flags / NraysCastResult::flags.  Bit 0 clear = the point is skipped; bit 1 = the point carries
 *                  a uv (it has one only if `uvs` is non-NULL too).  NULL = every point is shaded, and carries a uv exactly when `uvs` is non-NULL.
 *   keys           n RNG path keys, or NULL = the key of point i is i (also across chunks).  Area lights hash the key exactly as the shading of a
 *                  traced ray with the same key does (nrays_trace_rays_device).
 *   flags          must be 0 (any bit -> NRAYS_ERR_BAD_ARG).  No reorder is offered: a baker's texels already come in surface order.
 * A point is SKIPPED when bit 0 of hit_flags[i] is clear, when nodes[i] < 0 or when nodes[i] >= the scene's node count: it writes (0, 0, 0, 0) and
 * reads no scene record, so the outputs of nrays_cast_rays_device can be passed on unfiltered, misses included.  Points, normals and view
 * directions are expected to be finite.
 * NULL scene / points / normals / view_dirs / nodes / out_rgba -> NRAYS_ERR_BAD_ARG; n == 0 -> NRAYS_OK without work.  Otherwise the contract of
 * nrays_cast_rays_device: every pointer DEVICE memory on the scene's device, chunks of at most 2^22 points, enqueued on `hip_stream` without
 * read-back or synchronisation, ordered behind the handle's previous work; what the handle reports about its renders and its per-camera
 * scheduling state stay untouched. */
int nrays_shade_points_device(NraysScene* scene, uint32_t n, const double* points, const double* normals, const double* view_dirs,
                              const double* uvs, const int32_t* nodes, const uint32_t* hit_flags, const uint64_t* keys, float* out_rgba,
                              uint32_t flags, void* hip_stream);
/* Same, every pointer HOST memory.  Blocking. */
int nrays_shade_points(NraysScene* scene, uint32_t n, const double* points, const double* normals, const double* view_dirs, const double* uvs,
                       const int32_t* nodes, const uint32_t* hit_flags, const uint64_t* keys, float* out_rgba, uint32_t flags);

/* Ambient occlusion at n caller-supplied surface points (a baker's texel centres, the hits of nrays_cast_rays_device): the library builds
 * num_dirs hemisphere rays per point ON THE DEVICE, runs Scene::intersects_ray (the transparent-shadow query of nrays_intersects_rays_device)
 * on each and writes ONE folded value per point — no ray, max_toi or per-ray result array exists anywhere.
 * The rays are defined exactly (f64 + - * /, copysign and integer arithmetic, every product evaluated left to right as written, nothing fused),
 * so that a caller can restate them bit for bit (Python: nrays_amd.occlusion_rays; the library's own: nrays_debug_occlusion_rays).  For point p
 * with normal n (used as given; unit length is expected, as the casts return it) and RNG key `key`:
 *   frame      sg = copysign(1.0, n.z), a = -1.0 / (sg + n.z), b = n.x * n.y * a,
 *              t = (1.0 + sg * n.x * n.x * a, sg * b, -sg * n.x), u = (b, sg + n.y * n.y * a, -n.y)   (Duff et al. 2017: no singular normal)
 *   rotation   r = hash(key, salt) % num_rotations with the library's counter-based hash and the salt 0x300 << 32, (c, s) = rotations[r];
 *              x = c * lx - s * ly, y = s * lx + c * ly.  num_rotations == 0: x = lx, y = ly, no table is read.
 *   ray j      origin p + n * bias per component; direction d = (x * t + y * u) + lz * n per component for (lx, ly, lz) = dirs[j], a direction of
 *              the local frame whose z axis is the normal.  d is not normalised (unit inputs give | |d| - 1 | <= 1e-15): directions are used as given.
 *   fold       sum = 0 (f32 rgb); for j = 0 .. num_dirs - 1 in order: sum += blocked ? 0 : filter, open += !blocked;
 *              out_filter[3i..3i+2] = sum / (float)num_dirs (one correctly rounded division per channel), out_open[i] = open.
 * The result is defined by this text and never by how the library assigns rays to lanes. */
/* (Declared as a struct plus a separate typedef, not in the one-statement typedef form of the structs above: tests/test_integration_rust.py lists those by that
 * form and by name, and so does NOT compare this struct with its Rust twin; tests/test_occlusion.py does, field for field, and with the ctypes one.) */
struct NraysOcclusionParams {
    uint32_t num_dirs;       /* 1 .. 1024 */
    uint32_t num_rotations;  /* 0 .. 1024; 0 = none */
    const double* dirs;      /* num_dirs x 3 */
    const double* rotations; /* num_rotations x 2 (cos, sin), or NULL when 0 */
    double bias;
    double max_toi;          /* > 0, +inf allowed */
};
typedef struct NraysOcclusionParams NraysOcclusionParams;
/*   points, normals  n x 3 doubles, world space, used as given.
 *   hit_flags        n words, or NULL: the bits of out_flags of nrays_cast_rays_device.  Bit 0 clear = the point is SKIPPED: out_filter (0, 0, 0), out_open 0,
 *                    no traversal, neither its point nor its normal read (they may hold anything) — the outputs of nrays_cast_rays_device pass on unfiltered.
 *   keys             n RNG keys, or NULL = the key of point i is i (also across chunks).  Only the rotation reads them.
 *   params           HOST memory (the struct); params->dirs and params->rotations are DEVICE memory here, like every other array.
 *   out_filter       n x 3 floats, required.      out_open   n words, or NULL (no store).
 *   flags            must be 0 (any bit -> NRAYS_ERR_BAD_ARG).
 * NULL scene / points / normals / params / params->dirs / out_filter, num_dirs outside 1 .. 1024, num_rotations > 1024 or > 0 with NULL rotations,
 * a NaN or <= 0 max_toi, a non-finite bias -> NRAYS_ERR_BAD_ARG; n == 0 -> NRAYS_OK without work.  Otherwise the contract of nrays_cast_rays_device:
 * every array DEVICE memory on the scene's device, chunks of at most max(1, 2^22 / num_dirs) points, enqueued on `hip_stream` without read-back or
 * synchronisation, ordered behind the handle's previous work; what the handle reports about its renders and its per-camera scheduling state stay
 * untouched. */
int nrays_occlusion_points_device(NraysScene* scene, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags,
                                  const uint64_t* keys, const NraysOcclusionParams* params, float* out_filter, uint32_t* out_open,
                                  uint32_t flags, void* hip_stream);
/* Same, every pointer (the two tables included) HOST memory.  Blocking. */
int nrays_occlusion_points(NraysScene* scene, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags,
                           const uint64_t* keys, const NraysOcclusionParams* params, float* out_filter, uint32_t* out_open, uint32_t flags);
/* Test probe: the ray generator of nrays_occlusion_points_device alone (the same device function), on HOST arrays, blocking: ray j of point i to
 * out_origins / out_dirs [(i * num_dirs + j) * 3 ..], n x num_dirs x 3 doubles each.  keys NULL: key i.  max_toi is checked and not used. */
int nrays_debug_occlusion_rays(NraysScene* scene, uint32_t n, const double* points, const double* normals, const uint64_t* keys,
                               const NraysOcclusionParams* params, double* out_origins, double* out_dirs);

/* Direct light at n caller-supplied surface points from a CALLER-SUPPLIED table of point lights — a baker's per-light layers, a light that moves, the virtual
 * point lights of instant radiosity (Keller 1997), a rig that is not in the scene description: the library builds the shadow ray of every (point, light) pair ON THE
 * DEVICE, weights it with Lambert's cosine (and, for an emitter with a normal, the emitter's; optionally the inverse-square falloff), runs Scene::intersects_ray (the
 * transparent-shadow query of nrays_intersects_rays_device) on it and writes ONE summed colour per point.  A light behind the surface costs nothing.  The scene's own
 * lights are not read.  The arithmetic is defined exactly — f64 + - * / and sqrt, f32 + *, every product evaluated left to right as written, nothing fused; what
 * Material::compute does for a light of the scene (phong_material.rs:106-147) — so that a caller can restate it bit for bit (Python: nrays_amd.light_rays; the
 * library's own: nrays_debug_light_rays).  Per point p with normal nm (used as given; unit length is expected), for light k = 0 .. num_lights - 1 in order, with L,
 * col, e row k of positions, colors, normals:
 *   origin     q = p + nm * bias per component.
 *   direction  v = L - q, nrm = sqrt((v.x * v.x + v.y * v.y) + v.z * v.z); !(nrm > 0): the light is skipped.  ldir = v / nrm (three divisions).
 *   weight     cr = (float)((ldir.x * nm.x + ldir.y * nm.y) + ldir.z * nm.z), cr = cr > 0 ? cr : 0;
 *              ce = 1.0f when normals is NULL, else (float)(-((ldir.x * e.x + ldir.y * e.y) + ldir.z * e.z)), clamped the same way;
 *              g = 1.0f without NRAYS_LIGHTS_INVERSE_SQUARE, else (float)(1.0 / max(nrm * nrm, min_dist * min_dist));
 *              w = (cr * ce) * g; !(w > 0): the light is skipped — no ray exists for it.
 *   ray        origin q + ldir * offset per component, direction ldir, t_max = nrm - offset.  !(t_max > 0): the light is open with filter (1, 1, 1) and nothing is
 *              traversed.  Otherwise Scene::intersects_ray with max_toi = t_max, exactly the query of nrays_intersects_rays_device.
 *   fold       sum = +0 (f32 rgb); a blocked light adds nothing, an open one adds col * (filter * w) per channel, in the order of k.  out_rgb[3i..3i+2] = sum (no
 *              division: lights add); out_counts[2i] = the lights that got as far as `ray`, out_counts[2i + 1] = how many of them were open.
 * The result is defined by this text and never by how the library assigns lights to lanes. */
/* (Struct plus separate typedef, as NraysOcclusionParams and for the same reason; tests/test_light_points.py compares it with its Rust and ctypes twins.) */
#define NRAYS_LIGHTS_INVERSE_SQUARE 1u
struct NraysPointLights {
    uint32_t num_lights;      /* 1 .. 4096 */
    uint32_t flags;           /* 0 or NRAYS_LIGHTS_INVERSE_SQUARE */
    const double* positions;  /* num_lights x 3, world space */
    const float* colors;      /* num_lights x 3 */
    const double* normals;    /* num_lights x 3 unit emitter normals (VPLs), or NULL = lights shine every way */
    double bias;              /* finite: the point is moved along its normal first */
    double offset;            /* finite, >= 0: the ray starts this far towards the light and ends this far before it (the reference's 0.001, phong_material.rs:109-112) */
    double min_dist;          /* finite, > 0 when INVERSE_SQUARE is set: the falloff's clamp; otherwise unread */
};
typedef struct NraysPointLights NraysPointLights;
/*   points, normals  n x 3 doubles, world space, used as given.
 *   hit_flags        n words, or NULL: the bits of out_flags of nrays_cast_rays_device / nrays_surface_texels_device.  Bit 0 clear = the point is SKIPPED: out_rgb
 *                    (0, 0, 0), out_counts (0, 0), no traversal, neither its point nor its normal read — those outputs pass in unfiltered.
 *   lights           HOST memory (the struct); its three tables are DEVICE memory here, like every other array.  Nothing is random: there are no keys.
 *   out_rgb          n x 3 floats, required.      out_counts   n x 2 words, or NULL (no store).
 *   flags            must be 0 (any bit -> NRAYS_ERR_BAD_ARG): neighbouring points send coherent rays towards one light, so no reorder is offered.
 * NULL scene / points / normals / lights / positions / colors / out_rgb, num_lights outside 1 .. 4096, an unknown bit in either flags word, a non-finite bias, a
 * negative or non-finite offset, under NRAYS_LIGHTS_INVERSE_SQUARE a min_dist that is not finite or not > 0 -> NRAYS_ERR_BAD_ARG before any HIP call; n == 0 ->
 * NRAYS_OK without work.  Otherwise the contract of nrays_occlusion_points_device: every array DEVICE memory on the scene's device, chunks of at most
 * max(1, 2^22 / num_lights) points, enqueued on `hip_stream` without read-back, synchronisation or workspace, ordered behind the handle's previous work; what the
 * handle reports about its renders and its per-camera scheduling state stay untouched. */
int nrays_light_points_device(NraysScene* scene, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags,
                              const NraysPointLights* lights, float* out_rgb, uint32_t* out_counts, uint32_t flags, void* hip_stream);
/* Same, every pointer (the three tables included) HOST memory.  Blocking. */
int nrays_light_points(NraysScene* scene, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags,
                       const NraysPointLights* lights, float* out_rgb, uint32_t* out_counts, uint32_t flags);
/* Test probe: the ray generator of nrays_light_points_device alone (the same device function), on HOST arrays, blocking: the ray of (point i, light k) to
 * out_origins / out_dirs [(i * num_lights + k) * 3 ..], out_tmax / out_w [i * num_lights + k].  w == 0 marks a skipped light; one with !(nrm > 0) has origin q,
 * direction (0, 0, 0) and t_max 0, every other skipped light the origin, direction and t_max of the text above. */
int nrays_debug_light_rays(NraysScene* scene, uint32_t n, const double* points, const double* normals, const NraysPointLights* lights,
                           double* out_origins, double* out_dirs, double* out_tmax, float* out_w);

/* The light arriving at n caller-supplied surface points from the rest of the scene — a light map's indirect term, a final gather: the library builds
 * num_dirs hemisphere rays per point ON THE DEVICE, runs Scene::trace (what nrays_trace_rays_device runs) on each and writes ONE mean colour per point — the
 * caller passes and receives per-point arrays only, and no ray, key or per-ray colour array exists anywhere except in double-branching scenes (below), where the
 * library keeps the ray colours of one chunk in the handle's workspace.  The result is defined by this text, so that a caller can restate it from existing parts:
 *   rays       ray j of point i is bit for bit the ray nrays_occlusion_points* builds from the same point, normal, key, dirs, rotations and bias: the same
 *              frame, the same rotation pick (salt 0x300 << 32), origin p + n * bias, the same direction.  Occlusion and gather with the same tables use the
 *              same rays; nrays_debug_occlusion_rays and Python's occlusion_rays serve both.
 *   trace      each ray is the depth-0 RayWithEnergy nrays_trace_rays_device loads: refr 1.0, energy = params->energy, weight 1, RNG key
 *              key_ij = hash(key_i, (0x301 << 32) + j) with the library's counter-based hash (Python: gather_ray_keys); the key is read only in scenes that
 *              sample an area light, as there.  c_ij = Scene::trace(ray) with params->max_depth.
 *   fold       sum = 0 (f32 rgb); for j = 0 .. num_dirs - 1 in order: sum += c_ij; out_rgb[3i..3i+2] = sum / (float)num_dirs (one correctly rounded division
 *              per channel).  The result never depends on how the library assigns rays to lanes: it equals, bit for bit, nrays_trace_rays_device on these
 *              rays and keys with energy params->energy, folded this way.
 *   double-branching scenes (one hit spawns both a reflection and a refraction): the second children go to the continuation queue as for
 *              nrays_trace_rays_device, PER RAY — ray j of point i is the queue's "pixel" i * num_dirs + j of its chunk, its queued chains are summed in
 *              2^-32 fixed point and added to ITS colour before the fold, exactly as that call does — so the fold above holds bit for bit there too.  These
 *              scenes alone keep per-ray memory in the handle's workspace between the trace and the fold (36 bytes a ray of one chunk, beside the queue);
 *              the caller still passes and receives per-point arrays only.  NRAYS_ERR_QUEUE_OVERFLOW applies as for nrays_trace_rays_device; the queue is
 *              sized by a chunk's rays with the same rule. */
/* (Struct plus separate typedef, as NraysOcclusionParams and for the same reason; tests/test_gather.py compares it with its Rust and ctypes twins.) */
struct NraysGatherParams {
    uint32_t num_dirs;       /* 1 .. 1024 */
    uint32_t num_rotations;  /* 0 .. 1024; 0 = none */
    const double* dirs;      /* num_dirs x 3, local frame, z = the normal */
    const double* rotations; /* num_rotations x 2 (cos, sin), or NULL when 0 */
    double bias;             /* finite */
    float energy;            /* RayWithEnergy::energy of every gathered ray; finite */
    uint32_t max_depth;      /* as nrays_trace_rays_device: 0 = the energy rule only, the cap of 64 generations applies */
};
typedef struct NraysGatherParams NraysGatherParams;
/*   points, normals  n x 3 doubles, world space, used as given (unit normals pointing to the side to gather on).
 *   hit_flags        n words, or NULL = every point is live: the bits of out_flags of nrays_cast_rays_device / nrays_surface_texels_device.  Bit 0 clear = the
 *                    point is SKIPPED: out_rgb (0, 0, 0), no traversal, neither its point nor its normal read (they may hold anything).
 *   keys             n RNG keys, or NULL = the key of point i is i (also across chunks).  The rotation pick and the rays' keys read them.
 *   params           HOST memory (the struct); params->dirs and params->rotations are DEVICE memory here, like every other array.
 *   out_rgb          n x 3 floats, required.
 *   flags            must be 0 (any bit -> NRAYS_ERR_BAD_ARG).
 * NULL scene / points / normals / params / params->dirs / out_rgb, num_dirs outside 1 .. 1024, num_rotations > 1024 or > 0 with NULL rotations, a non-finite
 * bias or energy -> NRAYS_ERR_BAD_ARG; n == 0 -> NRAYS_OK without work.  Otherwise the contract of nrays_occlusion_points_device: every array DEVICE memory on
 * the scene's device, chunks of at most max(1, 2^22 / num_dirs) points, the workspace owned by the handle, enqueued on `hip_stream` behind the handle's previous
 * work, without read-back or synchronisation unless the scene is double-branching (the queue's rounds are controlled from the host, as for
 * nrays_trace_rays_device); what the handle reports about its renders and its per-camera scheduling state stay untouched. */
int nrays_gather_points_device(NraysScene* scene, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags,
                               const uint64_t* keys, const NraysGatherParams* params, float* out_rgb, uint32_t flags, void* hip_stream);
/* Same, every pointer (the two tables included) HOST memory.  Blocking. */
int nrays_gather_points(NraysScene* scene, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags,
                        const uint64_t* keys, const NraysGatherParams* params, float* out_rgb, uint32_t flags);
/* The two entry points above with `flags` = 0 or NRAYS_RAYS_UNORDERED (any other bit -> NRAYS_ERR_BAD_ARG).  flags == 0 IS the entry point without _ex.  The hint
 * means what it means for the ray batches: a statement about the input — the points come in no order that keeps neighbouring rays together (a light map's texels
 * under many directions, gathered hits) — under which the library may trace the rays in an order of its own.  out_rgb is the value defined above, BIT FOR BIT,
 * for every scene kind, double-branching included: only the time changes.  The rule and the switch are those of the ray batches, applied to the call's
 * n * num_dirs rays: reordered from 2^19 rays, never under NRAYS_RAY_REORDER=0, always under =2; a hinted call that is not reordered runs the unhinted path.
 * A reordered chunk bins its (point, direction) pairs by the key of the ray batches (each ray rebuilt in registers), traces them bin by bin, and folds per point.
 * For that it holds, in the handle's workspace, 12 bytes of colour and 16 bytes of sort state per ray of ONE chunk (at most 2^22 rays) in every scene kind; the
 * caller's interface stays per point: no ray, key or per-ray colour array crosses it.  Launches on the same stream; no read-back beyond the one double-branching
 * scenes need anyway.  Everything else of the contracts above holds unchanged. */
int nrays_gather_points_device_ex(NraysScene* scene, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags,
                                  const uint64_t* keys, const NraysGatherParams* params, float* out_rgb, uint32_t flags, void* hip_stream);
int nrays_gather_points_ex(NraysScene* scene, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags,
                           const uint64_t* keys, const NraysGatherParams* params, float* out_rgb, uint32_t flags);

/* The gathered light of nrays_gather_points*_ex kept by DIRECTION: per point the projection of its rays' colours onto the real spherical harmonics of bands
 * 0 .. bands - 1 — 9 coefficients per channel at bands = 3 (Ramamoorthi and Hanrahan 2001) — instead of their mean.  An irradiance probe (a free point in space:
 * normal (0, 0, 1), bias 0, no rotations and a table of sphere directions reproduce the table's directions from the point itself) and a directional light map
 * (per texel) are this call.  The arguments, the rays, the ray keys, the trace, the double-branching rule, the chunks, the skipped points, the stream ordering
 * and the untouched render state are those of nrays_gather_points_device_ex / nrays_gather_points_ex; `flags` is 0 or NRAYS_RAYS_UNORDERED with the reorder rule
 * and NRAYS_RAY_REORDER as there.  Only the fold differs:
 *   bands      1, 2 or 3; C = bands * bands coefficients.
 *   out_sh     n x C x 3 floats, required: coefficient c, channel ch of point i at (i * C + c) * 3 + ch.
 *   basis      d = the direction of ray j of point i exactly as the gather builds it (NraysOcclusionParams above; NOT normalised).  In f64, left to right as
 *              written, nothing fused, with K0 = 0.28209479177387814, K1 = 0.4886025119029199, K2 = 1.0925484305920792, K3 = 0.31539156525252005,
 *              K4 = 0.5462742152960396 (the doubles nearest 1/(2 sqrt(pi)), sqrt(3)/(2 sqrt(pi)), sqrt(15)/(2 sqrt(pi)), sqrt(5)/(4 sqrt(pi)), sqrt(15)/(4 sqrt(pi))):
 *                Y0 = K0
 *                Y1 = K1 * d.y                 Y2 = K1 * d.z                              Y3 = K1 * d.x
 *                Y4 = (K2 * d.x) * d.y         Y5 = (K2 * d.y) * d.z                      Y6 = K3 * ((3.0 * d.z) * d.z - 1.0)
 *                Y7 = (K2 * d.x) * d.z         Y8 = K4 * (d.x * d.x - d.y * d.y)
 *              — the real basis without the Condon-Shortley sign (Python: sh_basis).
 *   fold       in f32: y = (float)Yc; acc[c][ch] = +0; for j = 0 .. num_dirs - 1 in order: acc[c][ch] = acc[c][ch] + y * colour_ij[ch] (the product rounded, then
 *              the sum); out = acc / (float)num_dirs (one correctly rounded division).  colour_ij is the finished colour nrays_trace_rays_device returns for that
 *              ray and key, the queued second children of double-branching scenes included (Python: sh_fold_ref).  The first 1 and 4 coefficient rows of a
 *              bands = 3 result are the bands = 1 and 2 results bit for bit.
 *   measure    none is applied: the caller multiplies by 4 pi for uniform sphere directions and by 2 pi for a uniform hemisphere.
 *   skipped    a point whose flag bit 0 is clear writes 3 C exact zeros; neither its point nor its normal is read, in the trace or in the fold.
 * The result never depends on lanes, tiles or the reorder.  bands outside 1 .. 3, NULL out_sh, an unknown flag bit and every bad argument of nrays_gather_points
 * -> NRAYS_ERR_BAD_ARG before any device work; n == 0 -> NRAYS_OK, out_sh untouched.
 * Workspace: EVERY scene kind keeps the ray colours of one chunk (12 bytes a ray, at most 2^22 rays = 48 MiB) in the handle's workspace between the trace and
 * the fold, which rebuilds each direction from (i, j); a reordered chunk adds its 16 bytes of sort state a ray and a double-branching scene its 24 bytes beside
 * the queue, as for nrays_gather_points*_ex.  The caller still passes and receives per-point arrays only: no ray, direction or per-ray colour array crosses
 * the interface.  The host form stages 60 + 12 C bytes a point. */
int nrays_gather_sh_points_device(NraysScene* scene, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags,
                                  const uint64_t* keys, const NraysGatherParams* params, uint32_t bands, float* out_sh, uint32_t flags, void* hip_stream);
/* Same, every pointer (the two tables included) HOST memory.  Blocking. */
int nrays_gather_sh_points(NraysScene* scene, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags,
                           const uint64_t* keys, const NraysGatherParams* params, uint32_t bands, float* out_sh, uint32_t flags);
/* Test probe: the fold kernel of nrays_gather_sh_points_device alone, on caller-supplied ray colours (n x num_dirs x 3 floats, ray j of point i at
 * (i * num_dirs + j) * 3; n * num_dirs <= 2^22: one chunk) with the points, normals, flags, keys, tables and bands of that call; nothing is traced and energy and
 * max_depth are not used.  keys NULL: key i.  out_kernel_ms, or NULL: the kernel's time between two HIP events of the probe's own.  All HOST memory (the tables
 * of params included).  Blocking.  Arguments are checked as by nrays_gather_sh_points; NULL ray_colours -> NRAYS_ERR_BAD_ARG. */
int nrays_debug_gather_sh_fold(NraysScene* scene, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const uint64_t* keys,
                               const NraysGatherParams* params, uint32_t bands, const float* ray_colours, float* out_sh, float* out_kernel_ms);

/* The CONSUMER of the probes nrays_gather_sh_points* writes: the irradiance at n caller-supplied points with normals from a regular GRID of SH probes — the
 * indirect term of whatever moves through a baked scene.  Per point the eight probes around it are blended (trilinear weights, optionally a facing factor that
 * holds down probes behind the surface, and a per-probe validity word that leaves out a probe inside a wall; which probes are valid is the caller's to decide, from the counts of nrays_probe_depth_points*)
 * and the blended coefficients are folded with the cosine lobe at the normal.  No ray is traced and the scene's geometry is not read: the handle gives the device,
 * the stream ordering and the staging arena.  The result is defined by this text; nothing is fused, every product and sum is rounded on its own and expressions
 * are evaluated left to right as written (Python: irradiance_points_ref).  With c_a = counts[a], for a live point p with normal n (f64, used as given):
 *   cell coordinate  per axis a: c_a == 1: g = 0.0 (and cell_a is taken as 0.0 below, whatever it holds).  Otherwise g = (p_a - origin_a) / cell_a, then
 *                    g = g > 0 ? (g < (double)(c_a - 1) ? g : (double)(c_a - 1)) : 0.0 — a NaN becomes 0, a point outside the grid takes the border's value.
 *                    i_a = min((uint32)g, max(c_a, 2) - 2);  f_a = (float)(g - (double)i_a).
 *   corners          k = 0 .. 7: d = (k & 1, (k >> 1) & 1, (k >> 2) & 1); the probe's index per axis is min(i_a + d_a, c_a - 1), its row
 *                    (index_z * counts[1] + index_y) * counts[0] + index_x.  In f32: w_k = (X * Y) * Z with X = d_x ? f_x : 1.0f - f_x, likewise Y and Z.
 *   facing           only with NRAYS_IRRADIANCE_FACING, in f64: q_a = origin_a + (double)index_a * cell_a;  v = q - p;  l2 = (v.x*v.x + v.y*v.y) + v.z*v.z;
 *                    c = (v.x*n.x + v.y*n.y) + v.z*n.z;  t = l2 > 0 ? (c / sqrt(l2) + 1.0) * 0.5 : 1.0;  w_k = w_k * (float)(t * t + 0.2) — a factor in
 *                    [0.2, 1.2] for a unit normal.
 *   validity         with valid != NULL and bit 0 of the corner probe's word clear: w_k = 0.
 *   normalisation    in f32: wsum = +0; for k = 0 .. 7 in order: wsum = wsum + w_k.  If !(wsum > 0): out_rgb (0, 0, 0), out_sh 3 C zeros, out_weight wsum as
 *                    computed.  Otherwise wn_k = w_k / wsum, one correctly rounded division each.
 *   interpolation    s[c][ch] = +0; for k = 0 .. 7 in order: a corner with wn_k == 0 is SKIPPED — its probe's row is not read, so a NaN in an invalid probe never
 *                    reaches a result —, otherwise s[c][ch] = s[c][ch] + wn_k * sh[row_k][c][ch].
 *   irradiance       Y_c(n): the nine expressions of nrays_gather_sh_points_device's basis at d = n, in f64.  a_c = (float)(A_band(c) * Y_c) with
 *                    A = 3.141592653589793, 2.0943951023931953, 0.7853981633974483 (pi, 2 pi / 3, pi / 4: the cosine lobe of Ramamoorthi and Hanrahan 2001) for
 *                    bands 0, 1, 2.  e[ch] = +0; for c = 0 .. C - 1 in order: e[ch] = e[ch] + a_c * s[c][ch].  out_rgb = measure * e.
 *   outputs          out_rgb n x 3, out_sh n x C x 3 (the interpolated coefficients s, laid out as nrays_gather_sh_points* lays them out), out_weight n (wsum).
 *                    Each may be NULL (no store); at least one of out_rgb and out_sh is required.
 *   skipped          a point whose hit_flags bit 0 is clear: zeros in every output; neither its point nor its normal is read.
 * The result never depends on how the library assigns points to lanes or chunks. */
#define NRAYS_IRRADIANCE_FACING 1u
/* (Struct plus separate typedef, as NraysGatherMapsParams and for the same reason; tests/test_irradiance.py compares it with its Rust and ctypes twins.) */
struct NraysIrradianceGrid {
    double origin[3];      /* position of probe (0, 0, 0); finite */
    double cell[3];        /* spacing per axis; finite and > 0 on every axis with counts > 1, ignored (any value) where counts == 1 */
    uint32_t counts[3];    /* probes per axis, each 1 .. 1024, product <= 2^22 */
    uint32_t bands;        /* 1, 2 or 3; C = bands * bands */
    const float* sh;       /* P x C x 3 floats, what nrays_gather_sh_points* writes: probe (ix, iy, iz) is row (iz * counts[1] + iy) * counts[0] + ix */
    const uint32_t* valid; /* P words or NULL = every probe valid; bit 0 clear = the probe is never read */
    float measure;         /* solid angle of the probes' sample table (4 pi for sphere_dirs); finite */
    uint32_t reserved;     /* must be 0 */
};
typedef struct NraysIrradianceGrid NraysIrradianceGrid;
/*   points, normals  n x 3 doubles, world space, used as given (unit normals).
 *   hit_flags        n words, or NULL = every point is live: the bits of out_flags of nrays_cast_rays_device / nrays_surface_texels_device.
 *   grid             HOST memory (the struct); grid->sh and grid->valid are DEVICE memory here, like every other array.  Nothing of the struct is read after the
 *                    call returns.
 *   flags            0 or NRAYS_IRRADIANCE_FACING.
 * NULL scene / points / normals / grid / grid->sh; out_rgb and out_sh both NULL; a count outside 1 .. 1024 or a product above 2^22; bands outside 1 .. 3; a
 * non-finite origin or measure; on an axis with counts > 1 a cell that is not finite and > 0; reserved != 0; an unknown flag bit -> NRAYS_ERR_BAD_ARG, before any
 * device work.  n == 0 -> NRAYS_OK, the outputs untouched.  Otherwise the contract of nrays_filter_texels_device, in chunks of at most 2^22 points: every array is
 * device memory on the scene's device, the call is enqueued on `hip_stream` behind the handle's previous work without read-back or synchronisation, and what the
 * handle reports about its renders and its per-camera scheduling state stay untouched.  Traffic: 48 bytes in (52 with hit_flags) and 12 + 12 C + 4 bytes out a
 * point as asked for; the corner rows come from the grid, which lanes in surface order share. */
int nrays_irradiance_points_device(NraysScene* scene, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags,
                                   const NraysIrradianceGrid* grid, float* out_rgb, float* out_sh, float* out_weight, uint32_t flags, void* hip_stream);
/* Same, every pointer (grid->sh and grid->valid included) HOST memory.  Blocking.  The grid's coefficients and validity words are staged with the tables, once
 * a call. */
int nrays_irradiance_points(NraysScene* scene, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags,
                            const NraysIrradianceGrid* grid, float* out_rgb, float* out_sh, float* out_weight, uint32_t flags);

/* The light that BAKED MAPS hold at the closest hits of the hemisphere rays of n caller-supplied surface points — one diffuse bounce of a light-map baker: the
 * library builds num_dirs rays per point ON THE DEVICE, finds each ray's closest hit, samples the light map of the node it hit at the hit's uv and writes ONE mean
 * colour per point.  Feeding a baked map back in (Python: bake_bounces) gathers the next bounce without a new scene, a host copy or a material that stands in for
 * the map.  No per-ray memory exists anywhere.  The result is defined by this text, so that a caller can restate it from existing parts:
 *   rays       ray j of point i is bit for bit the ray nrays_occlusion_points* / nrays_gather_points* build from the same point, normal, key, dirs, rotations and
 *              bias: the same frame, the same rotation pick (salt 0x300 << 32), origin p + n * bias, the same direction.  nrays_debug_occlusion_rays and Python's
 *              occlusion_rays serve this call too.  Only the rotation reads `keys`.
 *   query      each ray runs the closest-hit query of nrays_cast_rays_device (Scene::trace's first query, NOT Scene::intersects_ray): the ungated traversal, the
 *              winner checked against the exact gates, the gated repeat.  max_toi filters the FINISHED query (toi <= max_toi keeps the hit), as the per-ray bound
 *              of that call does.  Transparency is not looked at.
 *   c_ij       (f32 rgb) and its class:
 *                missed   no hit within max_toi: miss_rgb.
 *                mapped   a hit on node d with m = node_map[d] in [0, num_maps) whose record carries a uv (bit 1 of nrays_cast_rays_device's out_flags): x, y, z
 *                         of Texture2d::sample of maps[m] at the record's (u, v) (below); the sample's w is dropped.
 *                dark     every other hit: (+0, +0, +0).  A node_map entry outside [0, num_maps) counts as -1.  The side of the surface the ray arrives on is
 *                         not looked at.
 *   sample     the value the library's materials get from a texture (texture2d.rs:207-256), with maps[m].interp and .overflow honoured as given; format must be
 *              NRAYS_TEXEL_RGBA32F (what Python's bake_lightmap returns and lightmap_texture wraps), texel (x, y) at texels[4 * (y * width + x) ..], row 0 the
 *              BOTTOM row.  All f32, every product and sum rounded on its own, left to right as written (Python: lightmap_sample_ref):
 *                ux = (float)u, uy = (float)v
 *                NRAYS_OVERFLOW_CLAMP:  ux = ux > 0 ? (ux < 1 ? ux : 1) : 0          (a NaN becomes 0); likewise uy
 *                NRAYS_OVERFLOW_WRAP:   ux = copysign(ux - trunc(ux), ux)            (fmodf(ux, 1); inf gives NaN); if (ux < 0) ux = 1 + ux; likewise uy
 *                ux = ux * (float)(width - 1), uy = uy * (float)(height - 1)
 *                index(x) = 0 if !(x > 0), 2^32 - 1 if x >= 2^32, else trunc(x)      (Rust's `f32 as usize`)
 *                NRAYS_INTERP_NEAREST:  the texel at (min(index(round(ux)), width - 1), min(index(round(uy)), height - 1)), round = half away from zero.
 *                NRAYS_INTERP_BILINEAR: lx = min(index(floor(ux)), width - 1), hx = min(lx + 1, width - 1), ly, hy likewise;
 *                                       sx = ux - (float)lx, sy = uy - (float)ly;
 *                                       ul = texel(lx, hy), ur = texel(hx, hy), dl = texel(lx, ly), dr = texel(hx, ly); per channel
 *                                       ui = ul * (1 - sx) + ur * sx;  di = dl * (1 - sx) + dr * sx;  r = ui * sy + di * (1 - sy).
 *   fold       sum = +0 (f32 rgb); for j = 0 .. num_dirs - 1 in order: sum += c_ij; out_rgb[3i..3i+2] = sum / (float)num_dirs (one correctly rounded division per
 *              channel): the fold of nrays_gather_points.  The result never depends on how the library assigns rays to lanes.
 *   out_counts n x 2 words, or NULL (no store): the number of mapped and of missed rays of point i.
 *   skipped    a point whose hit_flags bit 0 is clear: out_rgb (0, 0, 0), out_counts 0, 0, no traversal, neither its point nor its normal read. */
#define NRAYS_GATHER_MAX_MAPS 16u
/* (Struct plus separate typedef, as NraysGatherParams and for the same reason; tests/test_gather_maps.py compares it with its Rust and ctypes twins.) */
struct NraysGatherMapsParams {
    uint32_t num_dirs;        /* 1 .. 1024 */
    uint32_t num_rotations;   /* 0 .. 1024; 0 = none */
    const double* dirs;       /* num_dirs x 3, local frame, z = the normal */
    const double* rotations;  /* num_rotations x 2 (cos, sin), or NULL when 0 */
    double bias;              /* finite */
    double max_toi;           /* > 0, +inf allowed */
    uint32_t num_maps;        /* 1 .. NRAYS_GATHER_MAX_MAPS */
    uint32_t num_nodes;       /* entries of node_map; must equal the scene's node count */
    const NraysTexture* maps; /* HOST array of num_maps records (always host, like this struct); their `texels` as the call says */
    const int32_t* node_map;  /* num_nodes entries: the map a node's surface reads, or -1 */
    float miss_rgb[3];        /* what a ray that leaves the scene brings; finite */
};
typedef struct NraysGatherMapsParams NraysGatherMapsParams;
/*   points, normals  n x 3 doubles, world space, used as given (unit normals pointing to the side to gather on).
 *   hit_flags        n words, or NULL = every point is live: the bits of out_flags of nrays_cast_rays_device / nrays_surface_texels_device.
 *   keys             n RNG keys, or NULL = the key of point i is i (also across chunks).
 *   params           HOST memory (the struct and its `maps` records); params->dirs, ->rotations, ->node_map and every map's texels are DEVICE memory here, like
 *                    every other array.  The records are copied into the kernel's arguments (16 x 24 bytes): nothing of them is read after the call returns.
 *   out_rgb          n x 3 floats, required.      out_counts   n x 2 words, or NULL.
 *   flags            must be 0 (any bit -> NRAYS_ERR_BAD_ARG).
 * NULL scene / points / normals / params / dirs / maps / node_map / out_rgb; num_dirs outside 1 .. 1024, num_rotations > 1024 or > 0 with NULL rotations; a
 * non-finite bias or miss_rgb, a NaN or <= 0 max_toi; num_maps outside 1 .. 16, num_nodes other than the scene's node count; a map with NULL texels, width or
 * height 0, a format other than NRAYS_TEXEL_RGBA32F or an unknown interp / overflow; flags != 0 -> NRAYS_ERR_BAD_ARG, before any device work.  n == 0 ->
 * NRAYS_OK, the outputs untouched.  Otherwise the contract of nrays_gather_points_device: chunks of at most max(1, 2^22 / num_dirs) points, enqueued on
 * `hip_stream` behind the handle's previous work, without read-back or synchronisation in ANY scene kind (nothing is queued here); what the handle reports
 * about its renders and its per-camera scheduling state stay untouched. */
int nrays_gather_maps_points_device(NraysScene* scene, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags,
                                    const uint64_t* keys, const NraysGatherMapsParams* params, float* out_rgb, uint32_t* out_counts,
                                    uint32_t flags, void* hip_stream);
/* Same, every pointer (the two tables, node_map and the maps' texels included) HOST memory.  Blocking.  The maps' texels are staged with the tables, once a call. */
int nrays_gather_maps_points(NraysScene* scene, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags,
                             const uint64_t* keys, const NraysGatherMapsParams* params, float* out_rgb, uint32_t* out_counts, uint32_t flags);

/* What a probe SEES of the geometry around it (Majercik et al. 2019, DDGI): per point a small octahedral map of the mean and the mean squared distance to the
 * nearest surface, the number of rays that end close by or nowhere, and the nearest hit.  The moments are what nrays_irradiance_points_vis* reads to hold down
 * a probe on the other side of a wall; the counts are what a caller decides a probe's validity with (a probe inside geometry sees surfaces at once in most
 * directions; Python: probe_valid_words); the nearest hit is what a caller moves a probe off a surface with.  Defined by this text:
 *   rays       ray j of point i is bit for bit the ray nrays_occlusion_points* builds: the same frame, rotation pick, origin and direction d (NOT normalised).
 *              A probe is a point with normal (0, 0, 1), bias 0 and no rotations.
 *   query      the closest-hit query of nrays_cast_rays_device, unbounded, as nrays_gather_maps_points* runs it.
 *   per ray    in f64, left to right, nothing fused: L = sqrt((d.x*d.x + d.y*d.y) + d.z*d.z);  dist = hit ? toi * L : +inf;
 *              r = dist < max_dist ? dist : max_dist;  rf = (float)r.
 *   texel      of a direction (x, y, z) at resolution R, in f64 (Python: oct_texel): s = (fabs(x) + fabs(y)) + fabs(z).  If !(s > 0): a = b = 0.0, otherwise
 *              a = x / s, b = y / s.  If z < 0, both from the OLD a and b: a' = (1.0 - fabs(b)) * copysign(1.0, a), b' = (1.0 - fabs(a)) * copysign(1.0, b).
 *              gx = (a * 0.5 + 0.5) * (double)R;  tx = gx > 0 ? min((uint32)gx, R - 1) : 0 (a NaN gives 0);  ty likewise from b;  t = ty * R + tx.  The octahedral
 *              map of the unit sphere; scaling a direction by a power of two does not change its texel.
 *   fold       per texel t of point i, in f32: s1 = s2 = +0, cnt = 0; for j = 0 .. num_dirs - 1 in order, if texel(d_ij) == t: s1 = s1 + rf;
 *              s2 = s2 + rf * rf (the product rounded, then the sum); cnt += 1.  out_moments[(i * R*R + t) * 2 + 0] = cnt ? s1 / (float)cnt : (float)max_dist,
 *              [.. + 1] = cnt ? s2 / (float)cnt : (float)max_dist * (float)max_dist; each division the correctly rounded one (Python: probe_depth_ref).
 *   out_counts n x 2 words, or NULL (no store): the rays of point i with dist < near_dist, and its rays with no hit at all.
 *   out_nearest      n doubles, or NULL: the minimum of dist over the rays of point i, +inf if none hit.
 *   out_nearest_dir  n words, or NULL: the smallest j that attains that minimum, 0xFFFFFFFF if none hit.
 *   skipped    a point whose hit_flags bit 0 is clear: (float)max_dist, (float)max_dist * (float)max_dist in every texel, counts 0, 0, nearest +inf and
 *              0xFFFFFFFF; no traversal, neither its point nor its normal read.
 * The result never depends on lanes, rounds or chunks. */
/* (Struct plus separate typedef, as NraysGatherMapsParams and for the same reason; tests/test_probe_depth.py compares it with its Rust and ctypes twins.) */
struct NraysProbeDepthParams {
    uint32_t num_dirs;        /* 1 .. 1024 */
    uint32_t num_rotations;   /* 0 .. 1024; 0 = none */
    const double* dirs;       /* num_dirs x 3, local frame, z = the normal */
    const double* rotations;  /* num_rotations x 2 (cos, sin), or NULL when 0 */
    double bias;              /* finite */
    double max_dist;          /* finite, > 0: distances are clamped to it, and an empty texel holds it */
    double near_dist;         /* finite, >= 0: out_counts[2i] counts the rays that end closer than this */
    uint32_t res;             /* R: 4, 8 or 16; R * R texels a point */
    uint32_t reserved;        /* must be 0 */
};
typedef struct NraysProbeDepthParams NraysProbeDepthParams;
/*   points, normals, hit_flags, keys   as for nrays_gather_maps_points_device.
 *   params           HOST memory (the struct); params->dirs and ->rotations are DEVICE memory here, like every other array.
 *   out_moments      n x R*R x 2 floats, required.   out_counts n x 2 words, out_nearest n doubles, out_nearest_dir n words: each may be NULL.
 *   flags            must be 0 (any bit -> NRAYS_ERR_BAD_ARG).
 * NULL scene / points / normals / params / dirs / out_moments; num_dirs outside 1 .. 1024, num_rotations > 1024 or > 0 with NULL rotations; a non-finite bias;
 * a max_dist that is not finite and > 0; a near_dist that is not finite and >= 0; res other than 4, 8 or 16; reserved != 0; flags != 0 -> NRAYS_ERR_BAD_ARG,
 * before any device work.  n == 0 -> NRAYS_OK, the outputs untouched.  Otherwise the contract of nrays_gather_maps_points_device: chunks of at most
 * max(1, 2^22 / num_dirs) points, enqueued on `hip_stream` behind the handle's previous work, without read-back or synchronisation in ANY scene kind; what the
 * handle reports about its renders and its per-camera scheduling state stay untouched.
 * Workspace: the per-texel sums depend on the order of j, so they are not folded through the lanes that trace: the handle's workspace keeps rf of ONE chunk
 * (4 bytes a ray, at most 2^22 rays = 16 MiB) between the trace and a fold that gives every (point, texel) a lane and rebuilds each direction from (i, j).  No
 * ray, direction or per-ray distance crosses the interface. */
int nrays_probe_depth_points_device(NraysScene* scene, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags,
                                    const uint64_t* keys, const NraysProbeDepthParams* params, float* out_moments, uint32_t* out_counts,
                                    double* out_nearest, uint32_t* out_nearest_dir, uint32_t flags, void* hip_stream);
/* Same, every pointer (the two tables included) HOST memory.  Blocking. */
int nrays_probe_depth_points(NraysScene* scene, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags,
                             const uint64_t* keys, const NraysProbeDepthParams* params, float* out_moments, uint32_t* out_counts,
                             double* out_nearest, uint32_t* out_nearest_dir, uint32_t flags);

/* A PROBE FILLED FROM BAKED MAPS, and what it sees of the geometry, from ONE traversal of its rays (post ABI 7): the spherical harmonics of the light that baked
 * maps hold at the closest hits of a point's rays — so a probe sees the bounced light the maps of its scene already hold —, and, when `depth` is given, the
 * outputs of nrays_probe_depth_points* from the same query (DDGI updates radiance and depth from one ray set).  Defined by this text from calls above:
 *   rays, query, c_ij, class   those of nrays_gather_maps_points_device under the same `params` (used unchanged): the same rays, the same closest-hit query, the
 *              same contribution c_ij and class per ray.  The query runs ONCE per ray, unbounded; params->max_toi filters the FINISHED query for c_ij and the
 *              class only.
 *   out_sh     n x bands^2 x 3 floats, required: the fold of nrays_gather_sh_points_device with colour_ij = c_ij — the same basis evaluated at the direction as
 *              generated (not normalised), rounded once to f32; per accumulator acc = acc + y * c in f32 in the order of j; ONE division by (float)num_dirs.  No
 *              measure is applied.  The first 1 and 4 coefficient rows of a 3-band result are the 1-band and 2-band results bit for bit.
 *   out_counts n x 2 words, or NULL (no store): the mapped and the missed rays of point i, as nrays_gather_maps_points_device counts them.
 *   depth      NULL: out_moments, out_depth_counts, out_nearest and out_nearest_dir must all be NULL.  Otherwise out_moments is required and the other three may be
 *              NULL, and the four hold exactly what nrays_probe_depth_points_device writes for the same points, hit_flags, keys, dirs, rotations and bias with
 *              max_dist, near_dist and res from `depth`.  dist comes from the UNFILTERED query: params->max_toi does not touch the depth side.
 *   skipped    a point whose hit_flags bit 0 is clear: out_sh 3 * bands^2 exact zeros, out_counts 0, 0, the depth outputs nrays_probe_depth_points_device's skipped
 *              values; no traversal, neither its point nor its normal read.
 * The result never depends on lanes, rounds or chunks. */
/* (Struct plus separate typedef, as NraysGatherMapsParams and for the same reason; tests/test_gather_maps_sh.py compares it with its Rust and ctypes twins.) */
struct NraysGatherDepthSpec {
    double max_dist;          /* finite, > 0: distances are clamped to it, and an empty texel holds it */
    double near_dist;         /* finite, >= 0: out_depth_counts[2i] counts the rays that end closer than this */
    uint32_t res;             /* R: 4, 8 or 16; R * R texels a point */
    uint32_t reserved;        /* must be 0 */
};
typedef struct NraysGatherDepthSpec NraysGatherDepthSpec;
/*   points, normals, hit_flags, keys, params   as for nrays_gather_maps_points_device (params and its `maps` records HOST memory; the tables, node_map and every
 *                    map's texels DEVICE memory here).
 *   bands            1 .. 3.          depth   HOST memory, or NULL.
 *   out_moments      n x R*R x 2 floats.   out_depth_counts n x 2 words, out_nearest n doubles, out_nearest_dir n words.
 *   flags            must be 0 (any bit -> NRAYS_ERR_BAD_ARG).
 * Every bad argument of nrays_gather_maps_points_device (out_sh in the place of out_rgb) and of nrays_probe_depth_points_device (depth's max_dist, near_dist and
 * res); bands outside 1 .. 3; depth->reserved != 0; a depth output without `depth`, or `depth` without out_moments; flags != 0 -> NRAYS_ERR_BAD_ARG, before any
 * device work.  n == 0 -> NRAYS_OK, the outputs untouched.  Otherwise the contract of nrays_gather_maps_points_device: chunks of at most max(1, 2^22 / num_dirs)
 * points, enqueued on `hip_stream` behind the handle's previous work, without read-back or synchronisation in ANY scene kind; what the handle reports about its
 * renders and its per-camera scheduling state stay untouched.
 * Workspace: the handle's workspace keeps c_ij of ONE chunk (12 bytes a ray) and, with `depth`, rf behind it (4 bytes a ray): at most 2^22 rays = 64 MiB, between
 * the trace and the two folds of the parent calls, which run unchanged: three launches a chunk, two without `depth`.  No ray, direction, per-ray colour or per-ray
 * distance crosses the interface. */
int nrays_gather_maps_sh_points_device(NraysScene* scene, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags,
                                       const uint64_t* keys, const NraysGatherMapsParams* params, uint32_t bands, float* out_sh, uint32_t* out_counts,
                                       const NraysGatherDepthSpec* depth, float* out_moments, uint32_t* out_depth_counts, double* out_nearest,
                                       uint32_t* out_nearest_dir, uint32_t flags, void* hip_stream);
/* Same, every pointer (the two tables, node_map and the maps' texels included) HOST memory.  Blocking. */
int nrays_gather_maps_sh_points(NraysScene* scene, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags,
                                const uint64_t* keys, const NraysGatherMapsParams* params, uint32_t bands, float* out_sh, uint32_t* out_counts,
                                const NraysGatherDepthSpec* depth, float* out_moments, uint32_t* out_depth_counts, double* out_nearest,
                                uint32_t* out_nearest_dir, uint32_t flags);

/* nrays_irradiance_points* with VISIBILITY: the value defined there with one step inserted per corner k, after the facing factor and the validity rule, for a
 * corner whose probe is valid (an invalid probe's moment row is never read, like its SH row).  With q the probe's position as the facing step computes it
 * (q_a = origin_a + (double)index_a * cell_a) and `texel` the function of nrays_probe_depth_points_device at R = vis->res:
 *   in f64: pb_a = p_a + n_a * bias;  v = pb - q;  l2 = (v.x*v.x + v.y*v.y) + v.z*v.z.  If l2 > 0: t = texel(v) (v is not normalised);  m1, m2 = the two floats
 *   of row row_k, texel t of vis->moments;  df = (float)sqrt(l2).  If df > m1, in f32 with every operation rounded on its own: var = m2 - m1 * m1;
 *   var = var > 0 ? var : 0;  diff = df - m1;  den = var + diff * diff;  ch = den > 0 ? var / den : 0;  c3 = (ch * ch) * ch;
 *   w_k = w_k * (c3 > floor ? c3 : floor) — Chebyshev's bound on the part of the probe's rays that reach as far as the point, cubed (DDGI).  Otherwise, and
 *   where l2 == 0, there is no factor.
 * Everything after that is unchanged: wsum, the normalisation, the corner with a zero weight that is skipped, interpolation, the lobe and the outputs.  Moments
 * larger than every distance (1e30) give nrays_irradiance_points* bit for bit (Python: irradiance_points_ref(visibility=...)). */
struct NraysIrradianceVisibility {
    const float* moments;  /* P x R*R x 2 floats, what nrays_probe_depth_points* writes at the grid's probes; rows as grid->sh */
    uint32_t res;          /* R: 4, 8 or 16 */
    float floor;           /* in [0, 1]: the least factor, so that a point no probe sees keeps some light (0: none) */
    double bias;           /* finite: the point is moved along its normal by this before its distance to a probe is taken */
};
typedef struct NraysIrradianceVisibility NraysIrradianceVisibility;
/* The arguments of nrays_irradiance_points_device plus `vis` (HOST memory; vis->moments DEVICE memory here).  flags: 0 or NRAYS_IRRADIANCE_FACING.  Every bad
 * argument of that call, and NULL vis or vis->moments, res other than 4, 8 or 16, a floor outside [0, 1] or NaN, a non-finite bias -> NRAYS_ERR_BAD_ARG before
 * any device work.  The rest of its contract holds unchanged. */
int nrays_irradiance_points_vis_device(NraysScene* scene, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags,
                                       const NraysIrradianceGrid* grid, const NraysIrradianceVisibility* vis, float* out_rgb, float* out_sh, float* out_weight,
                                       uint32_t flags, void* hip_stream);
/* Same, every pointer (grid->sh, grid->valid and vis->moments included) HOST memory.  Blocking.  The moments are staged with the grid, once a call. */
int nrays_irradiance_points_vis(NraysScene* scene, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags,
                                const NraysIrradianceGrid* grid, const NraysIrradianceVisibility* vis, float* out_rgb, float* out_sh, float* out_weight,
                                uint32_t flags);

/* The MATERIAL TERMS at n caller-supplied surface points, without the lights: what Material::ambiant (src/material.rs:7; Scene::intersects_ray calls it,
 * src/scene.rs:317) returns there, the diffuse reflectance `diffuse_color.component_mul(tex_color)` of phong_material.rs:120-121, the specular constants, and the
 * per-hit constants Scene::trace reads from the node.  nrays_shade_points* folds the first three with the lights into one colour; this call hands them out, so that
 * nrays_cast_rays* + this call is all an integrator of the caller's own needs on top of the library's traversal, a baker gets the albedo of a textured node
 * (Python: texel_albedo), and the irradiance of nrays_irradiance_points* becomes a colour (Python: indirect_points).  No ray is traced and no light is read.
 * The result is defined by this text (Python: material_points_ref), never by how the library assigns points to lanes or chunks.
 *   nodes          n scene-node indices, required (the values out_node of nrays_cast_rays_device holds).
 *   hit_flags      n words, or NULL: the bits of out_flags / NraysCastResult::flags.
 *   uvs            n x 2 doubles, or NULL; used as given, any double.
 *   normals        n x 3 doubles, used as given; may be NULL only when out_ambient is NULL (only the NORMAL material reads it).
 *   live           point i is LIVE when bit 0 of hit_flags[i] is set (or hit_flags == NULL) and 0 <= nodes[i] < the scene's node count.  It CARRIES A UV when
 *                  uvs != NULL and bit 1 of hit_flags[i] is set (or hit_flags == NULL) — nrays_shade_points_device's rule: the caller's word decides, the shape's
 *                  own uv bit is not looked at.  Below, m is the material of node nodes[i], (u, v) = uvs[2i], uvs[2i + 1], n = normals[3i .. 3i + 2].
 *   sample         sample(t, u, v) is Texture2d::sample of texture t exactly as written out under nrays_gather_maps_points_device (`sample`), with t's own interp
 *                  and overflow and either texel format: an NRAYS_TEXEL_RGBA32F texel is its four floats, a channel of an NRAYS_TEXEL_RGBA8 texel is
 *                  `u8 as f32 / 255.0`, the correctly rounded f32 quotient.  The colour texture is sampled ONCE for out_ambient and out_diffuse together, and not
 *                  at all when neither is asked for; the opacity map is sampled only for out_ambient.
 *   out_ambient    n x 4 floats, Material::ambiant(pt, normal, uv):
 *                    NRAYS_MAT_PHONG with a uv   tc = (1, 1, 1, 1); with a texture: tc = sample(texture, u, v), then tc.w = 1; with an opacity map:
 *                                                tc.w = sample(alpha, u, v).w; the result is (ka.x * tc.x, ka.y * tc.y, ka.z * tc.z, 1.0f * tc.w).
 *                    NRAYS_MAT_PHONG without     (ka.x, ka.y, ka.z, 1).
 *                    NRAYS_MAT_NORMAL            ((1.0f + (float)n.x) / 2.0f, (1.0f + (float)n.y) / 2.0f, (1.0f + (float)n.z) / 2.0f, 1).
 *                    NRAYS_MAT_UV                ((float)u, (float)v, 0, 1) with a uv, (0, 0, 0, 0) without.
 *   out_diffuse    n x 3 floats.  NRAYS_MAT_PHONG: (kd.x * t.x, kd.y * t.y, kd.z * t.z) with t = x, y, z of sample(texture, u, v) when the point carries a uv and
 *                  the material has a texture, else (1, 1, 1).  NRAYS_MAT_NORMAL / NRAYS_MAT_UV: (+0, +0, +0).
 *   out_specular   n x 4 floats.  NRAYS_MAT_PHONG: (ks.x, ks.y, ks.z, shininess).  Otherwise zeros.
 *   out_node       n x 4 doubles, for every material kind: ((double)alpha, (double)refl_mix, (double)refl_atenuation, refr_coeff) of node nodes[i].
 *   skipped        a point that is not live writes zeros into every output; neither its normal nor its uv is read, so the outputs of nrays_cast_rays_device pass
 *                  on unfiltered, misses included.
 *   Each output may be NULL (no store); at least one is required.
 *   flags          must be 0.
 * NULL scene / nodes; no output at all; NULL normals with out_ambient; any flag bit -> NRAYS_ERR_BAD_ARG, before any device work.  n == 0 -> NRAYS_OK, the outputs
 * untouched.  Otherwise the contract of nrays_irradiance_points_device: every array device memory on the scene's device, chunks of at most 2^22 points, one launch
 * a chunk enqueued on `hip_stream` behind the handle's previous work, without read-back, synchronisation or workspace; what the handle reports about its renders
 * and its per-camera scheduling state stay untouched.  Traffic: 4 bytes in for the node, 4 with hit_flags, 16 with uvs where a uv is read, 24 with normals where
 * out_ambient is asked for; 16 + 12 + 16 + 32 bytes out a point as asked for. */
int nrays_material_points_device(NraysScene* scene, uint32_t n, const double* normals, const double* uvs, const int32_t* nodes,
                                 const uint32_t* hit_flags, float* out_ambient, float* out_diffuse, float* out_specular, double* out_node,
                                 uint32_t flags, void* hip_stream);
/* Same, every pointer HOST memory.  Blocking. */
int nrays_material_points(NraysScene* scene, uint32_t n, const double* normals, const double* uvs, const int32_t* nodes,
                          const uint32_t* hit_flags, float* out_ambient, float* out_diffuse, float* out_specular, double* out_node, uint32_t flags);

/* The NEAREST SURFACE to n caller-supplied points: how far it is, where, and on which node and triangle — ncollide's PointQuery beside the RayCast the other
 * families restate.  The first six found outputs carry the names and layouts of nrays_cast_rays_device, so they pass unfiltered into nrays_shade_points*,
 * nrays_material_points*, nrays_occlusion_points*, nrays_gather_*_points* and nrays_irradiance_points* (out_point -> points, out_node -> nodes, out_flags -> hit_flags).
 * The result is defined by this text (Python: nearest_points_ref restates it bit for bit), never by the order the device visits anything in.  Every operation is an
 * f64 + - * / sqrt or comparison, evaluated left to right as written, nothing fused.  dot(a, b) = (a.x b.x + a.y b.y) + a.z b.z; a vector expression is applied
 * per component.
 *   candidates     every scene node.  For node k with rotation R (row-major, local -> world) and translation T, the query in local space is
 *                  pl = (R00 v.x + R10 v.y) + R20 v.z, ... (the transposed rows) with v = p - T; pl = p - T for a node whose axis_angle is zero; pl = p when the
 *                  translation is zero too.
 *   closest point  ql, in local space, by shape:
 *     TRIMESH      per triangle with corners a, b, c (f32 widened to f64), Ericson, Real-Time Collision Detection 5.1.5, tested in this order:
 *                    ab = b - a, ac = c - a, ap = pl - a, d1 = dot(ab, ap), d2 = dot(ac, ap);     d1 <= 0 and d2 <= 0:            (v, w) = (0, 0), ql = a
 *                    bp = pl - b, d3 = dot(ab, bp), d4 = dot(ac, bp);                             d3 >= 0 and d4 <= d3:           (v, w) = (1, 0), ql = b
 *                    vc = d1 d4 - d3 d2;                        vc <= 0 and d1 >= 0 and d3 <= 0:  v = d1 / (d1 - d3), w = 0, ql = a + ab v
 *                    cp = pl - c, d5 = dot(ab, cp), d6 = dot(ac, cp);                             d6 >= 0 and d5 <= d6:           (v, w) = (0, 1), ql = c
 *                    vb = d5 d2 - d1 d6;                        vb <= 0 and d2 >= 0 and d6 <= 0:  w = d2 / (d2 - d6), v = 0, ql = a + ac w
 *                    va = d3 d6 - d5 d4;       va <= 0 and d4 - d3 >= 0 and d5 - d6 >= 0:         w = (d4 - d3) / ((d4 - d3) + (d5 - d6)), v = 1 - w, ql = b + (c - b) w
 *                    otherwise den = (va + vb) + vc, v = vb / den, w = vc / den, ql = (a + ab v) + ac w, a candidate only if v >= 0, w >= 0 and (1 - v) - w >= 0.
 *                    One step beyond the book, for triangles whose corners are collinear (va, vb, vc are then rounding noise, and so were the tests above): in this
 *                    last branch the candidate competes with the three edge projections t1 = d1 / (d1 - d3) on AB, t2 = d2 / (d2 - d6) on AC,
 *                    t3 = (d4 - d3) / ((d4 - d3) + (d5 - d6)) on BC, each clamped as t >= 0 ? (t <= 1 ? t : 1) : 0, with ql = a + ab t1, a + ac t2, b + (c - b) t3
 *                    and (v, w) = (t1, 0), (0, t2), (1 - t3, t3); the smallest key wins, a later one only with a strictly smaller key.  Inside a real triangle
 *                    the interior candidate wins; on a collinear one an edge holds the true closest point.
 *     BALL         len = sqrt(dot(pl, pl)); ql = pl (r / len), nl = pl / len; len == 0: ql = (r, 0, 0), nl = (1, 0, 0).  Behind: len < r.
 *     CUBOID       g_k = h_k - |pl_k|.  All g_k >= 0 (inside or on it): the axis with the smallest g_k, the lowest among equals, moves to its face:
 *                  ql_k = copysign(h_k, pl_k), nl = copysign(1, pl_k) e_k; behind: all g_k > 0.  Otherwise ql_k = pl_k < -h_k ? -h_k : (pl_k > h_k ? h_k : pl_k)
 *                  and nl = (pl - ql) / sqrt(d2): at an edge or a corner the direction from that feature to the point.
 *     PLANE        the half-space's boundary: t = dot(nrm, pl), ql = pl - nrm t; behind: t < 0; nl = behind ? -nrm : nrm (the side cast_plane reports).
 *     CYLINDER, CAPSULE, CONE   surfaces of revolution about local y, the solids the casts intersect (the cone's apex at y = +hh, its base of radius r at -hh).
 *                  rho = sqrt(pl.x pl.x + pl.z pl.z), y = pl.y, (cx, cz) = rho == 0 ? (1, 0) : (pl.x / rho, pl.z / rho); the 2-D closest point (qr, qy) and
 *                  normal (nr, ny) lift to ql = (qr cx, qy, qr cz), nl = (nr cx, ny, nr cz).  Where no normal is named, (nr, ny) = (rho - qr, y - qy) / sqrt of their
 *                  squares' sum: the direction from the feature (a rim, the apex) to the point.
 *       CYLINDER   gs = r - rho, gc = hh - |y|.  Both >= 0: gs <= gc ? (qr, qy) = (r, y), normal (1, 0) : (qr, qy) = (rho, copysign(hh, y)), normal
 *                  (0, copysign(1, y)); behind: both > 0.  Otherwise qr = rho > r ? r : rho, qy = y clamped to [-hh, hh].
 *       CAPSULE    yc = y clamped to [-hh, hh], ey = y - yc, len = sqrt(rho rho + ey ey); normal (rho / len, ey / len), or (1, 0) for len == 0;
 *                  (qr, qy) = (nr r, yc + ny r); behind: len < r.
 *       CONE       up = y + hh, h2 = 2 hh.  Base: br = rho > r ? r : rho, db = (rho - br)^2 + up up.  Slant: t = (((rho - r) * -r + up h2) / (r r + h2 h2))
 *                  clamped to [0, 1], (sr, sy) = (r + -r t, -hh + h2 t), ds = (rho - sr)^2 + (y - sy)^2.  db <= ds: (qr, qy) = (br, -hh), else (sr, sy).
 *                  f = (rho - r) h2 + up r.  up >= 0 and f <= 0 (inside or on it): normal (0, -1) for the base, (h2, r) / sqrt(h2 h2 + r r) for the slant;
 *                  behind: up > 0 and f < 0.
 *   key            d2 = (dx dx + dy dy) + dz dz with dl = pl - ql, in local space.
 *   winner         the candidate with the smallest d2; among equal d2 the smallest node index, then the smallest triangle index in NraysMesh::indices (the leaf
 *                  references of a pre-split triangle are one triangle).
 *   max_dist       n doubles, or NULL = unbounded; +inf allowed; NaN or negative = a miss.  Found iff sqrt(d2) <= max_dist[i]: the unbounded answer, or a miss.
 *   hit_flags      n words or NULL; bit 0 clear: the point is skipped — the miss record, its coordinates are not read.
 *   found record   out_dist = sqrt(d2); out_point = R ql + T row-wise, ((R00 q.x + R01 q.y) + R02 q.z) + T.x, ..., = ql + T without a rotation, = ql without either;
 *                  out_node; out_prim = the triangle's index, -1 for an analytic shape; out_normal = the normal SceneNode::cast gives a ray arriving at that point
 *                  from p's side, in world space (R nl row-wise; nl without a rotation): for a triangle cr = cross(b - a, c - a), nl = cr / sqrt(dot(cr, cr)),
 *                  negated iff dot(pl - a, cr) < 0 (that is "behind"); for an analytic shape the nl above.  out_uv: for a mesh with uvs
 *                  (ua b0 + ub v) + uc w per coordinate with b0 = (1 - v) - w; for a ball the ball cast's uv of the world normal n,
 *                  (0.5 + atan2(n.z, n.x) / (2 pi), 0.5 - asin(n.y) / pi) — the one place outside + - * / sqrt: equal up to the math library; otherwise zeros.
 *                  out_flags: bit 0 = found, bit 1 = the record carries a uv, bit 2 = p lies behind the surface (the back of the triangle's winding, inside a
 *                  closed analytic shape, under a plane).
 *   miss record    out_dist = +inf, out_node = -1, out_prim = -1, zeros elsewhere, flags 0.  An empty scene gives a miss for every point.
 *   out_dist and out_node are required; the other five outputs may each be NULL (no store).  flags must be 0.
 * NULL scene / points / out_dist / out_node, or any flag bit -> NRAYS_ERR_BAD_ARG before any HIP call.  n == 0 -> NRAYS_OK without work.  Otherwise the contract of
 * nrays_cast_rays_device: every pointer device memory on the scene's device, chunks of at most 2^22 points enqueued on `hip_stream` behind the handle's previous
 * work, no read-back and no synchronisation; the handle's render statistics and per-camera scheduling state are untouched. */
int nrays_nearest_points_device(NraysScene* scene, uint32_t n, const double* points, const double* max_dist, const uint32_t* hit_flags, double* out_dist, int32_t* out_node,
                                double* out_point, double* out_normal, double* out_uv, int32_t* out_prim, uint32_t* out_flags, uint32_t flags, void* hip_stream);
/* Same, every pointer HOST memory.  Blocking. */
int nrays_nearest_points(NraysScene* scene, uint32_t n, const double* points, const double* max_dist, const uint32_t* hit_flags, double* out_dist, int32_t* out_node,
                         double* out_point, double* out_normal, double* out_uv, int32_t* out_prim, uint32_t* out_flags, uint32_t flags);

/* The surface of TriMesh node `node` at the points of a width x height lattice in its uv space — a light map's texels: for every lattice point
 * the triangle that owns it, the world position and normal there.  This is the baker's first step, in front of nrays_shade_points_device and
 * nrays_occlusion_points_device, which take the arrays written here unfiltered (out_node -> nodes, out_flags -> hit_flags, out_uv -> uvs); no
 * host copy of the mesh, no rasteriser and no upload is needed.
 * Every array holds width * height entries, lattice point (x, y) at index y * width + x; row 0 is the smallest v, the bottom row of NraysTexture.
 * The result is defined exactly (f64 + - * /, sqrt and comparisons only, every expression evaluated left to right as written, nothing fused), so
 * that a caller can restate it bit for bit (Python: nrays_amd.surface_texels_ref):
 *   lattice    su = width > 1 ? x / (width - 1) : 0.0, sv likewise from y and height: the points where Texture2d::sample reads texel (x, y)
 *              (texture2d.rs:225-233).  With NRAYS_TEXELS_CENTRES: su = (x + 0.5) / width, sv = (y + 0.5) / height.
 *   triangle   t of the node's NraysMesh with uv corners A, B, C (f32 widened to f64): area2 = (B.u - A.u) * (C.v - A.v) - (B.v - A.v) * (C.u - A.u).
 *              area2 == 0 or not finite: the triangle covers nothing.  s = area2 > 0 ? 1.0 : -1.0.
 *   edge       E(P, Q) at (su, sv): order the endpoints so that (P.u, P.v) <= (Q.u, Q.v) lexicographically;
 *              E = (Q.u - P.u) * (sv - P.v) - (Q.v - P.v) * (su - P.u); negated if the endpoints were swapped.  Two triangles that share an edge with
 *              bit-identical uv endpoints get exactly opposite values: no lattice point falls between them (but see the box under `coverage`).
 *   coverage   e0 = s * E(B, C), e1 = s * E(C, A), e2 = s * E(A, B), sum = (e0 + e1) + e2.  t covers the point iff (su, sv) lies in the triangle's uv
 *              box (min / max of the corners per axis, compared exactly — in exact arithmetic no restriction at all; it is what lets the library
 *              visit a triangle's own lattice points only) and e0 >= 0 && e1 >= 0 && e2 >= 0 && sum != 0.  Caveat: in f64 a point just OUTSIDE one
 *              triangle's box may get a rounded edge value >= 0 on the shared edge while the neighbour, whose box holds it, gets the opposite value
 *              < 0; such a point is then covered by neither.  It takes a point within a rounding of the edge's line and beyond the edge's own end.
 *   winner     the covering triangle with the smallest index t, whatever order the device visits triangles in; the leaf references a pre-split
 *              triangle has count as one triangle.  uvs are not wrapped: only triangles whose uvs reach a lattice point cover it.
 *   record     w0 = e0 / sum, w1 = e1 / sum, w2 = e2 / sum; local point p = (a * w0 + b * w1) + c * w2 per component (a, b, c the corners);
 *              world point R p + T with row k of R applied as (R[k][0] * p.x + R[k][1] * p.y) + R[k][2] * p.z — for a node whose axis_angle is zero
 *              p + T, and p itself when the translation is zero too.  Normal: cross(b - a, c - a) / its norm (the normal a ray arriving from that side
 *              gets from nrays_cast_rays), rotated by R the same way, negated with NRAYS_TEXELS_FLIP_NORMALS.  out_uv = (su, sv), the lattice point itself;
 *              out_prim = t; out_node = node; out_flags = 3 (bit 0 covered, bit 1 the record carries a uv: the bits of NraysCastResult::flags).
 *   uncovered  out_flags 0, out_node -1, out_prim -1, zeros elsewhere.
 * out_points and out_flags are required; out_normals, out_uv, out_node and out_prim may each be NULL: a NULL output is not stored at all.
 * NULL scene / out_points / out_flags, node >= the scene's node count, width or height outside 1 .. 16384, width * height > 2^24, an unknown
 * flag bit -> NRAYS_ERR_BAD_ARG; a node that is not a NRAYS_SHAPE_TRIMESH, or whose mesh has no uvs -> NRAYS_ERR_UNSUPPORTED.  Otherwise the
 * contract of nrays_cast_rays_device: every pointer DEVICE memory on the scene's device, enqueued on `hip_stream` without read-back or
 * synchronisation, ordered behind the handle's previous work, workspace owned by the handle; what the handle reports about its renders and
 * its per-camera scheduling state stay untouched. */
#define NRAYS_TEXELS_CENTRES      1u  /* lattice (x + 0.5) / W instead of x / (W - 1) */
#define NRAYS_TEXELS_FLIP_NORMALS 2u
int nrays_surface_texels_device(NraysScene* scene, uint32_t node, uint32_t width, uint32_t height, double* out_points, double* out_normals,
                                double* out_uv, int32_t* out_node, int32_t* out_prim, uint32_t* out_flags, uint32_t flags, void* hip_stream);
/* Same, every pointer HOST memory.  Blocking. */
int nrays_surface_texels(NraysScene* scene, uint32_t node, uint32_t width, uint32_t height, double* out_points, double* out_normals,
                         double* out_uv, int32_t* out_node, int32_t* out_prim, uint32_t* out_flags, uint32_t flags);
/* Timing probe: the two passes of nrays_surface_texels_device (owners: count, scan, one atomic per covering lane; resolve: the records) `repeats`
 * times on a stream of the handle, between HIP events of their own; every output is written to scratch memory.  out_ms: repeats x 2 floats HOST
 * memory, (owner pass, resolve pass) in milliseconds.  Blocking.  Statuses as above; repeats == 0 or NULL out_ms -> NRAYS_ERR_BAD_ARG. */
int nrays_debug_surface_texels_passes(NraysScene* scene, uint32_t node, uint32_t width, uint32_t height, uint32_t flags, uint32_t repeats, float* out_ms);

/* Gutter dilation of a baked light map: every lattice point that no triangle covers takes the values of the nearest covered point within `radius`, so
 * that Texture2d::sample with Bilinear, which reads the four lattice points around a uv, meets no unlit point at a chart's border (radius >= 2: the
 * diagonal neighbour of a border point lies at d2 = 2).  The baker's last step, behind nrays_shade_points_device / nrays_gather_points_device.
 * The lattice is width x height, point (x, y) at index i = y * width + x — the layout of nrays_surface_texels*.  The result is defined exactly, in
 * integers (Python: nrays_amd.dilate_texels_ref):
 *   covered     point i is covered iff bit 0 of flags_in[i] is set; every other bit is ignored (out_flags of nrays_surface_texels* passes in unfiltered).
 *   candidates  of an uncovered point (x, y): the covered points (x', y') with d2 = (x' - x)^2 + (y' - y)^2 <= radius * radius.  A Euclidean disc; no
 *               wrap-around at the lattice's borders.
 *   source      the candidate with the smallest d2, among equal d2 the one with the smallest index y' * width + x'.  A point with a source is FILLED.
 *               A covered point is its own source; an uncovered point without a candidate has source -1.
 *   values      optional, in place: `channels` (1 .. 4) floats per point, point i at values[i * channels ...].  For every filled point the `channels`
 *               32-bit words of its source are copied as bit patterns (NaN payloads, -0 and infinities pass unchanged).  Covered points and points
 *               with source -1 are not written at all.
 *   out_source  optional: int32 per point, the source index, the point's own index, or -1.
 *   out_flags   optional, may be the same pointer as flags_in: flags_in[i] for covered and unfilled points, flags_in[i] | NRAYS_TEXEL_FILLED for a
 *               filled point.  Bit 0 stays clear there: a filled point is not a surface point and must not be shaded.
 * The definition is separable, which is how the library computes it: per row the nearest covered column within `radius` (the left one on a tie), then
 * per column the minimum over dy in [-radius, radius] of dx(y + dy)^2 + dy^2 under the same tie rule.
 * NULL scene / flags_in, values, out_source and out_flags all NULL, values non-NULL with channels outside 1 .. 4, radius outside
 * 1 .. NRAYS_DILATE_MAX_RADIUS, width or height outside 1 .. 16384, width * height > 2^24, flags != 0 (reserved) -> NRAYS_ERR_BAD_ARG.  Otherwise the
 * contract of nrays_surface_texels_device: every pointer DEVICE memory on the scene's device, two launches enqueued on `hip_stream` without read-back
 * or synchronisation, ordered behind the handle's previous work, workspace owned by the handle (2 bytes per lattice point, grown only when needed); what
 * the handle reports about its renders and its per-camera scheduling state stay untouched. */
#define NRAYS_DILATE_MAX_RADIUS 64u
#define NRAYS_TEXEL_FILLED 4u
int nrays_dilate_texels_device(NraysScene* scene, uint32_t width, uint32_t height, const uint32_t* flags_in, uint32_t radius,
                               uint32_t channels, float* values, int32_t* out_source, uint32_t* out_flags, uint32_t flags, void* hip_stream);
/* Same, every pointer HOST memory.  Blocking. */
int nrays_dilate_texels(NraysScene* scene, uint32_t width, uint32_t height, const uint32_t* flags_in, uint32_t radius,
                        uint32_t channels, float* values, int32_t* out_source, uint32_t* out_flags, uint32_t flags);

/* Denoising of a baked light map: one pass of a 5 x 5 a-trous (B3-spline) joint-bilateral filter over the lattice, the step between
 * nrays_gather_points_device (a Monte-Carlo mean, noisy at few rays) and nrays_dilate_texels_device.  Neighbouring lattice points are averaged only where they
 * lie on the same piece of surface — close in the world, facing the same way —, never across a chart border, a gutter or a crease.
 * The lattice, the indexing i = y * width + x and "covered iff bit 0 of flags_in[i]" are those of nrays_dilate_texels*; points / normals (3 doubles per
 * lattice point) and flags_in are out_points / out_normals / out_flags of nrays_surface_texels*, unfiltered; values_in / values_out hold `channels`
 * (1 .. 4) floats per point, point i at [i * channels ...].  The result is defined exactly (Python: nrays_amd.filter_texels_ref); nothing is fused:
 * every product and every sum is rounded on its own.  For every COVERED point (x, y) with point p, normal n:
 *   taps        (i, j) for j = -2 .. 2 (outer loop) and i = -2 .. 2 (inner loop) at x' = x + i * step, y' = y + j * step, with point p', normal n', values v'.
 *               A tap outside the lattice or on an uncovered point is skipped.  No wrap-around.
 *   kernel      k = (float)(h[i + 2] * h[j + 2]), h = {1, 4, 6, 4, 1}: the integers 1 .. 36; the division by 256 is left to the normalisation.
 *   centre tap  (i = j = 0): w = 36, whatever its point and normal hold.  The weight sum is therefore never 0.
 *   other taps  in f64, left to right as written:
 *                 d2 = ((p'.x - p.x) * (p'.x - p.x) + (p'.y - p.y) * (p'.y - p.y)) + (p'.z - p.z) * (p'.z - p.z)
 *                 wp = 1.0 - d2 / (pos_radius * pos_radius)          skipped unless wp > 0 (a NaN skips; pos_radius = +inf gives wp = 1 for finite points)
 *                 c  = (n.x * n'.x + n.y * n'.y) + n.z * n'.z
 *                 wn = (c - normal_cos) / (1.0 - normal_cos)         skipped unless wn > 0; wn > 1 becomes 1.0
 *               then in f32:  w = (k * (float)wp) * (float)wn
 *   sum         in f32, in tap order, for each channel: acc = acc + w * v' (the product rounded, then the sum), wsum = wsum + w, both from +0;
 *               values_out = acc / wsum, one correctly rounded division per channel.
 * An UNCOVERED point: the `channels` words of values_in are copied to values_out as bit patterns (NaN payloads and -0 pass unchanged), so that the output
 * is a complete map which nrays_dilate_texels* can take next.  The result does not depend on how lanes and tiles are assigned.  A pass with
 * step = 1, 2, 4, ... after one another (two buffers) is the a-trous sequence: three passes reach 4 * 7 + 1 = 29 texels across.
 * NULL scene / flags_in / points / normals / values_in / values_out, values_out == values_in, channels outside 1 .. 4, step outside
 * 1 .. NRAYS_FILTER_MAX_STEP, width or height outside 1 .. 16384, width * height > 2^24, a NaN or <= 0 pos_radius, a normal_cos that is not in [-1, 1),
 * flags != 0 (reserved) -> NRAYS_ERR_BAD_ARG, checked before any device work.  Any other overlap of values_in and values_out is undefined.  Otherwise the contract of
 * nrays_dilate_texels_device: every pointer DEVICE memory on the scene's device, one launch enqueued on `hip_stream` without read-back or
 * synchronisation, ordered behind the handle's previous work; no workspace; what the handle reports about its renders and its per-camera scheduling
 * state stay untouched. */
#define NRAYS_FILTER_MAX_STEP 64u
int nrays_filter_texels_device(NraysScene* scene, uint32_t width, uint32_t height, const uint32_t* flags_in,
                               const double* points, const double* normals, uint32_t channels,
                               const float* values_in, float* values_out,
                               uint32_t step, double pos_radius, double normal_cos, uint32_t flags, void* hip_stream);
/* Same, every pointer HOST memory.  Blocking. */
int nrays_filter_texels(NraysScene* scene, uint32_t width, uint32_t height, const uint32_t* flags_in,
                        const double* points, const double* normals, uint32_t channels,
                        const float* values_in, float* values_out,
                        uint32_t step, double pos_radius, double normal_cos, uint32_t flags);

/* Test probe of the reorder: runs exactly the key and binning kernels of ONE hinted chunk (n <= 2^22) on n rays and returns
 *   out_keys   n keys (nrays_amd/csrc/ray_key.h), out_order  out_order[j] = index of the ray traced j-th (a permutation of 0..n-1),
 *   out_frame  NRAYS_RAY_FRAME_DOUBLES doubles: the quantisation frame the keys were computed in (layout: ray_key.h),
 *   out_info   {K: significant bits of a key, B: leading bits the binning orders by, 1 if a hinted batch of n rays on this handle would be
 *              reordered, 0}.  n == 0: out_info only.
 * All HOST memory.  Blocking. */
#define NRAYS_RAY_FRAME_DOUBLES 20
int nrays_debug_ray_order(NraysScene* scene, uint32_t n, const double* origins, const double* dirs, uint64_t* out_keys, uint32_t* out_order,
                          double* out_frame, uint32_t out_info[4]);

/* Test probe of the reordered gather: runs exactly the bounds, key and binning kernels of ONE reordered chunk of nrays_gather_points_device_ex
 * (n * num_dirs <= 2^22) on n points.  Pair i * num_dirs + j is ray j of point i.
 *   out_keys   n * num_dirs keys; the entries of a skipped point are left as the caller filled them,
 *   out_order  n * num_dirs words, of which the first out_info[3] are written: the original pair indices in trace order (the live pairs, each once),
 *   out_frame  NRAYS_RAY_FRAME_DOUBLES doubles: bit for bit the frame nrays_debug_ray_order computes from the live pairs' rays,
 *   out_info   {K, B, 1 if a hinted call of n * num_dirs rays on this handle would be reordered, the number of live pairs}.  n == 0: out_info only.
 * All HOST memory (the tables of params included).  Blocking.  Arguments are checked as by nrays_gather_points_ex; NULL outputs -> NRAYS_ERR_BAD_ARG. */
int nrays_debug_gather_order(NraysScene* scene, uint32_t n, const double* points, const double* normals, const uint32_t* hit_flags, const uint64_t* keys,
                             const NraysGatherParams* params, uint64_t* out_keys, uint32_t* out_order, double* out_frame, uint32_t out_info[4]);

/* Number of rows in the compact output buffer of a (possibly tiled) render. */
uint32_t nrays_tile_rows(const NraysRenderParams* params);

/* Un-permutes `band_owners` gathered compact tile buffers (concatenated in owner order, each
 * nrays_tile_rows*width*3 floats) into one row-major frame.  Device pointers. */
int nrays_untile_device(const float* gathered, float* out_rgb_device, uint32_t width, uint32_t height,
                        uint32_t band_rows, uint32_t band_owners, void* hip_stream);

/* Synchronises with the last render of `scene` and returns its counters; the kernel timings are
 * averaged over the renders issued since the previous call (at most 256). */
int nrays_get_stats(NraysScene* scene, NraysStats* out_stats);

/* Counters of the PRIMARY kernel alone (first sample batch) of the last instrumented render: its
 * primary rays, the shadow rays they spawned and the traversal work of both — the per-launch units
 * behind bench.py's roofline figure. */
int nrays_get_primary_kernel_stats(NraysScene* scene, NraysStats* out_stats);

/* Per-wave-tile cost of the last frame that recorded it (the first frames of a camera record the shader cycles every 8x8-pixel
 * wave tile took, for the cost-ordered work lists): the two numbers that bound a frame of the persistent kernel — it cannot end
 * before its LONGEST tile does (a pixel's chain of dependent traversals), nor before sum / resident_waves cycles have passed. */
typedef struct NraysTileCosts {
    uint64_t tiles;          /* wave tiles recorded */
    uint64_t sum_cycles;     /* shader cycles (s_memtime) the waves spend on them (every part of a tile the cost-ordered lists split counted) */
    uint64_t max_cycles;     /* the longest unit the schedule deals: a tile, or ONE PART of a split tile (light-parallel / pixel-split parts) */
    uint64_t resident_waves; /* waves of the persistent grid that rendered the frame */
    double shader_clock_hz;  /* the shader clock under this scene's load, MEASURED by the handle's instrumented launches (nrays_render_device_instrumented / _counted):
                                s_memtime over s_memrealtime (100 MHz), summed over the lifetimes of a sample of their waves; 0 before the first such launch */
    double kernel_ms;        /* duration of that launch (HIP events of its own around it).  max_cycles / shader_clock_hz and sum_cycles / resident_waves /
                                shader_clock_hz are fractions of kernel_ms: units and time come from the same launch */
} NraysTileCosts;
int nrays_get_tile_costs(NraysScene* scene, NraysTileCosts* out);

/* Probe of the two BVT queries of the path on caller-supplied rays — the device intersectors and traversals WITHOUT raygen and
 * shading around them, so that fixtures derived independently of this code base (tests/golden/kat_independent.npz) can be
 * checked against the HIP path directly.
 *   mode 0  Scene::trace's closest-hit query (src/scene.rs:164-166) + SceneNode::cast's record (src/scene_node.rs:51-54):
 *           flags bit 0 = hit, bit 1 = the record carries uvs; toi, world normal, uv, scene-node index.
 *   mode 1  Scene::intersects_ray (src/scene.rs:147-161) with `max_toi[i]`: flags bit 0 = blocked by an opaque node;
 *           normal[0..2] = the colour filter of the transparent nodes crossed (1, 1, 1 if none).
 * `origins` / `dirs`: n x 3 doubles, `max_toi`: n doubles (mode 1 only), `out`: n records; all HOST memory.  Blocking. */
typedef struct NraysCastResult {
    double toi;
    double normal[3];
    double uv[2];
    int32_t node_id;
    uint32_t flags;
} NraysCastResult;
int nrays_debug_cast_batch(NraysScene* scene, uint32_t mode, uint32_t n, const double* origins, const double* dirs,
                           const double* max_toi, NraysCastResult* out);

/* Probe of the f32 box culling ALONE (no scene handle): ONE node visit of the traversals per case, through the product's own device functions —
 * the f32 view of the ray, the f32 bound of the current best distance, the fetch of the node's planes, the four slab tests and the rule for
 * f32-zero direction components.  Case i: origin and direction (3 doubles each), the current best distance `best[i]` (kDblMax / max_toi / a hit's
 * toi), one box `boxes[6 i ..]` = {min x, y, z, max x, y, z} placed in child slot `slots[i]` (0..3) of a real 128-byte node whose other three
 * children are absent.  mode 0: the per-lane fetch, a case per lane; mode 1: the wave-uniform scalar fetch, a case per wave.
 * Out: `keys` n x 4 (entry distance of a child the ray may enter before `best`, +inf for a child it cannot), `bits` n (RayF::bits: 1 / 2 / 4 =
 * component x / y / z is zero in f32, 16 / 32 / 64 = negative), `inv32` n x 3 (the f32 reciprocals the device computed).  All HOST memory.
 * Blocking; runs on the current device's default stream. */
int nrays_debug_box_cull(uint32_t mode, uint32_t n, const double* origins, const double* dirs, const double* best, const float* boxes,
                         const uint32_t* slots, float* keys, uint32_t* bits, float* inv32);

/* Probe of the nearest-surface walk's box bound ALONE (no scene handle): the product's device function on `n` points x `boxes` boxes.  points n x 3 doubles;
 * box_bounds boxes x 6 doubles {min x, y, z, max x, y, z}, narrowed to f32 as a BVH node holds them; out[i * boxes + j] = a lower bound of the exact squared
 * distance from point i to box j (Python: nearest_box_bound_ref, bit for bit).  All HOST memory.  Blocking; runs on the current device's default stream. */
int nrays_debug_nearest_bound(uint32_t n, uint32_t boxes, const double* points, const double* box_bounds, double* out);

/* World AABB of scene node `node` as the device holds it: geometry.bounding_volume(&transform) of src/scene_node.rs:41 in the
 * reference's arithmetic; the kernels apply ncollide's exact ray / AABB test to it for every accepted hit (the reference only casts
 * a node whose AABB the ray passes, src/scene.rs:276).  out = {min x, y, z, max x, y, z}. */
int nrays_debug_node_aabb(NraysScene* scene, uint32_t node, double out[6]);

/* Test probe: the flattened scene as the kernels read it — both TLASes, every BLAS, both instance lists — copied back FROM DEVICE MEMORY
 * (tests/scene_cover.py validates it against the scene description).  The caller provides the buffers and their capacities in entries;
 * a call with a capacity too small fills in the num_* fields and the scalars and returns NRAYS_ERR_BAD_ARG ("dump buffers too small"),
 * as nrays_debug_blas_build does.  All HOST memory.  Blocking.
 *   nodes             num_nodes x 32 floats: the 128-byte 4-wide node of NraysBlasDump, child refs ABSOLUTE indices into this array
 *                     (TLAS leaves: ~((instance index << 3) | bits), bits 1 = untransformed, 2 = any-hit, 4 = mesh)
 *   tris              num_tris x 48 bytes: v0.xyz f32, node id u32, v1.xyz, triangle id u32, v2.xyz, 0
 *   instances /       num_instances / num_shadow_instances x 136 bytes, the TLAS's leaves in leaf order and the planes behind them:
 *   shadow_instances  f64 rot[9] at byte 0 (local -> world, row-major), f64 trans[3] at 72, f64 params[3] at 96, u32 kind at 120 (NraysShapeKind),
 *                     u32 flags at 124 (1 solid, 2 identity rotation, 4 any-hit, 8 has uvs, 16 untransformed, 32 no uv values, 64 hair-like),
 *                     i32 node_id at 128 (-1: a BLAS of several nodes), i32 blas_root at 132 (a node index, or a leaf ref < 0)
 *   links /           one {i32 blas_root, u32 flags} pair per instance of the list
 *   shadow_links
 *   planes /          num_planes indices into instances / shadow_instances
 *   shadow_planes
 *   node_aabbs        num_scene_nodes x 6 doubles (nrays_debug_node_aabb)
 * closest_root / shadow_root: a node index, a leaf ref, or INT32_MIN for an empty list.  bounds_mn / bounds_mx / bounded: the f32 box of the
 * closest-hit TLAS's leaves and whether the scene has no plane; max_bvh_depth; dev_nodes / dev_tris: how many leading entries of nodes /
 * tris the device builder made (the host-built ones were moved behind them) — these six are host bookkeeping. */
typedef struct NraysSceneDump {
    uint32_t num_nodes;
    uint32_t num_tris;
    uint32_t num_instances;
    uint32_t num_shadow_instances;
    uint32_t num_planes;
    uint32_t num_scene_nodes;
    uint32_t node_capacity;
    uint32_t tri_capacity;
    uint32_t instance_capacity;
    uint32_t shadow_instance_capacity;
    uint32_t plane_capacity;
    uint32_t scene_node_capacity;
    int32_t closest_root;
    int32_t shadow_root;
    int32_t max_bvh_depth;
    uint32_t bounded;
    uint32_t dev_nodes;
    uint32_t dev_tris;
    float bounds_mn[3];
    float bounds_mx[3];
    float* nodes;
    uint8_t* tris;
    uint8_t* instances;
    uint8_t* shadow_instances;
    int32_t* links;
    int32_t* shadow_links;
    int32_t* planes;
    int32_t* shadow_planes;
    double* node_aabbs;
} NraysSceneDump;
int nrays_debug_scene_dump(NraysScene* scene, NraysSceneDump* out);

/* How the library classified the scene's content (test probe): out[0] = the feature bits of the descriptor (1 analytic shapes, 2 meshes,
 * 4 some node may be non-opaque to shadow rays, 16 more than one light sample per hit; 15 / 31 when a node can both reflect and refract),
 * out[1] = 1 when a hair-like mesh makes the BVT queries end their node phases by quorum (NRAYS_NODE_QUORUM=0 in the environment of
 * nrays_scene_create turns that off).  out[0] is NOT the kernel a frame runs: the handle's switches, the frame's kind and its size choose
 * that per render — nrays_debug_last_permutation reports it. */
int nrays_debug_scene_flags(const NraysScene* scene, uint32_t out[2]);

/* The k_primary permutation the most recent render of this handle actually launched (test probe; host bookkeeping only, no device work):
 * out[0..3] = STATS, FEAT, PLAIN, OCC of its last k_primary launch — the template arguments listed in NR_PRIMARY_PERMUTATIONS of
 * nrays_amd/csrc/primary_kernel.h, after every fall-back to a more general kernel; out[4] = the number of k_primary launches of that
 * render (sample batches; 0 = no render yet, or the staged path rendered the frame: out[0..3] are then 0); out[5] = 1 when those
 * launches did not all run the same permutation (of a batched frame only the first batch can be a plain one). */
int nrays_debug_last_permutation(const NraysScene* scene, uint32_t out[6]);

/* How the frames of this handle were enqueued since it was created (test probe; host bookkeeping only, no device work): out[0] = frames
 * pipelined (trace on an internal stream, compose on the caller's), out[1] = frames on the direct path, out[2] = in-flight queries issued
 * (hipEventQuery / hipStreamQuery of the handle's previous work, asked to decide between the two), out[3] = waits for a staging slot's
 * last compose enqueued on a trace stream. */
int nrays_debug_pipeline_counts(const NraysScene* scene, uint64_t out[4]);

/* Test probe of `Scene::new`'s BVT construction for one TriMesh (src/scene.rs:119-133; ncollide's BVT::new_balanced inside TriMesh::new,
 * examples/loader3d.rs:695): builds the BLAS of `mesh` with the host builder (flags bit 0 clear) or the device builder (bit 0 set;
 * nrays_scene_create picks it for meshes from NRAYS_GPU_BUILD_MIN triangles, default 2 000), bit 1 = without triangle pre-splitting,
 * and copies it out: `nodes` = num_nodes x 32 floats (the 128-byte 4-wide node: planes by slot, child refs in slot 2, local
 * indices, depth-first order), `tri_ids` = the triangle index behind each of the num_refs leaf slots.  Both builders apply the same
 * split rule with the same arithmetic, so from the same references they return the same nodes.  The caller provides the buffers
 * (node_capacity / ref_capacity entries); all HOST memory.  Blocking. */
typedef struct NraysBlasDump {
    uint32_t num_nodes;
    uint32_t num_refs;
    int32_t root;      /* >= 0: node index, < 0: a single leaf */
    int32_t max_depth;
    uint32_t hairy;    /* the mesh was classified hair-like (aggressive pre-splitting, quorum-ended node phases) */
    uint32_t node_capacity;
    uint32_t ref_capacity;
    uint32_t pad;
    float* nodes;
    uint32_t* tri_ids;
} NraysBlasDump;
int nrays_debug_blas_build(const NraysMesh* mesh, uint32_t flags, NraysBlasDump* out);

/* Device bytes of the flattened scene (BVH nodes, triangle records, instance / shading records, textures): what
 * a frame must read at least once — the compulsory part of bench.py's roofline block. */
uint64_t nrays_scene_device_bytes(const NraysScene* scene);

void nrays_scene_destroy(NraysScene* scene);

/* ---------------------------------------------------------------------------------------------------------------
 * Multi-GPU: the framebuffer tiled over the GPUs of one node (replaces the thread partition of src/scene.rs:49-66).
 * The scene is replicated on every GPU, bands of 16 rows are dealt round-robin to the owners, every owner renders its
 * compact tile, ONE exchange (grouped RCCL send / receive over xGMI, every peer straight to owner 0) brings the tiles
 * to owner 0, which un-permutes them.  The frame is bit-identical for any number of owners.
 *
 *   one process, all GPUs (what a Rust caller of scene::render uses):
 *       nrays_comm_create_local(n, NULL, &comm); nrays_scene_set_create(&desc, comm, &set);
 *       nrays_render_multi(set, &params, frame);            // = scene::render on n GPUs
 *   one process per GPU (torch.distributed.run, MPI, ...): rank 0 calls nrays_comm_unique_id, ships the 128 bytes to
 *       the other ranks by its own means, every rank calls nrays_comm_create(id, n, rank, &comm) on ITS device, then
 *       nrays_scene_set_create / nrays_render_multi[_device] collectively; rank 0 receives the frame.
 * The band fields of NraysRenderParams are ignored (the set owns the partition). */
#define NRAYS_UNIQUE_ID_BYTES 128
typedef struct NraysComm NraysComm;         /* opaque */
typedef struct NraysSceneSet NraysSceneSet; /* opaque */

int nrays_comm_unique_id(uint8_t out_id[NRAYS_UNIQUE_ID_BYTES]);
int nrays_comm_create(const uint8_t id[NRAYS_UNIQUE_ID_BYTES], uint32_t num_ranks, uint32_t rank, NraysComm** out_comm);
/* `devices`: HIP device index of every owner, or NULL for owner o on device o % device_count.  Owners may share a
 * device (their tiles then move by device-to-device copies): a 1-GPU box can run the N-owner path. */
int nrays_comm_create_local(uint32_t num_owners, const int32_t* devices, NraysComm** out_comm);
uint32_t nrays_comm_owners(const NraysComm* comm);
void nrays_comm_destroy(NraysComm* comm); /* after every scene set that uses it */

int nrays_scene_set_create(const NraysSceneDesc* desc, NraysComm* comm, NraysSceneSet** out_set);
void nrays_scene_set_destroy(NraysSceneSet* set);
/* The per-GPU scene handles behind a set (owned by the set): for instrumented renders and per-GPU statistics of one
 * owner's tile (nrays_render_device_instrumented / nrays_get_stats with that owner's band parameters). */
uint32_t nrays_scene_set_num_local(const NraysSceneSet* set);
NraysScene* nrays_scene_set_local_scene(NraysSceneSet* set, uint32_t k, uint32_t* out_owner);

/* scene::render on the group; `out_rgb` is HOST memory (height*width*3 floats), filled on the process that drives
 * owner 0 (NULL elsewhere).  Blocking. */
int nrays_render_multi(NraysSceneSet* set, const NraysRenderParams* params, float* out_rgb);
/* Same with DEVICE memory on owner 0's GPU and no final synchronisation: consecutive calls form a depth-1 pipeline
 * (the tile render of frame k + 1 overlaps the exchange of frame k).  nrays_multi_sync waits for everything enqueued. */
int nrays_render_multi_device(NraysSceneSet* set, const NraysRenderParams* params, float* out_rgb_device);
int nrays_multi_sync(NraysSceneSet* set);
/* Counters of the last frame summed over the owners this process drives. */
int nrays_multi_get_stats(NraysSceneSet* set, NraysStats* out_stats);
/* Where a frame of the group spends its time on THIS process's first owner, averaged over the frames since the previous call
 * (HIP events on the owner's render / communication streams): the tile render (nrays_render_device), the exchange (owner 0: its own
 * tile copy + every receive; other owners: their send) and, on owner 0, the un-permute (k_untile).  The reference's analogue is the
 * join of its render threads, src/scene.rs:97-112. */
typedef struct NraysMultiTimings {
    double render_ms;
    double exchange_ms;
    double untile_ms;
    uint32_t frames;   /* frames averaged */
    uint32_t owner;    /* band owner the figures belong to */
} NraysMultiTimings;
int nrays_multi_get_timings(NraysSceneSet* set, NraysMultiTimings* out_timings);

const char* nrays_last_error(void);

uint32_t nrays_abi_version(void);

#ifdef __cplusplus
}
#endif

#endif /* NRAYS_ABI_H */
