// switches.h — every NRAYS_* environment switch the library reads, in one table.  Host only.
// read_switches() (switches.cpp) is the only place under csrc/ that reads the environment: nrays_scene_create calls it once and keeps
// the result in the handle (NraysScene::sw, never written afterwards — nothing in the frame path looks at the environment),
// nrays_debug_blas_build once per call, nrays_scene_set_create once per set.  Nothing is cached per process: tests and tools/build_sweep.py
// flip switches between two creations.  A member's default is the library's behaviour with the variable unset; switches.cpp holds each
// variable's name and parse rule, in the same order.  "=0: ..." switches are on unless the variable is set to 0.
#pragma once
#include <cstddef>
#include <cstdint>
#include <optional>

namespace nrays {

// Switches::host_time_proof: a call that comes within this many microseconds of the return of the handle's last pipelined call is pipelined without an in-flight query.
// Half the shortest gap between return and next entry that a caller which synchronises after every frame produced: 35.0 us, the least of 200 frames of the balls scene
// at 64 x 64 (the frame has to be enqueued, run and be seen finished in it; stream and device synchronisation alike, profiles/pipeline_host_ab.log) — the steady loop's
// own gap between calls is 0.1 - 0.4 us from ctypes, 3 - 6 us from bench.py.  A wrong "in flight" costs speed, never pixels.
constexpr double kInFlightProofUs = 17.5;

struct Switches {
    // ---- what the scene's kernels may skip or specialise (nrays_scene_create: derive_scene_facts and the optional tables) ----
    bool elide = true;                  // NRAYS_ELIDE=0: no hit or light sample is skipped for being multiplied by exactly 0 (A/B)
    bool node_quorum = true;            // NRAYS_NODE_QUORUM=0: every node phase runs until its last lane holds a leaf, hair-like meshes too (A/B)
    bool noxform = true;                // NRAYS_NOXFORM=0: the general permutations also when every BLAS sits in world space (A/B)
    bool park = true;                   // NRAYS_PARK=0: the three-wave multi-light kernels keep a hit's shading state in registers / scratch (A/B)
    bool lds_scene = true;              // NRAYS_LDS_SCENE=0: small analytic scenes read their records from HBM, not from a packed copy in LDS (A/B)
    bool tiny_scene = true;             // NRAYS_TINY_SCENE=0: the TLAS walk instead of the stackless queries of the kFeatTinyScene kernels (A/B)
    bool seed_enabled = true; uint32_t seed_rays = 1; // NRAYS_COST_SEED=0|1|4: k_seed_costs' first guess of a cold camera's tile costs — none, from a tile's centre ray, from four rays
    bool prealloc = true;               // NRAYS_PREALLOC=0: the first frame allocates its buffers, not nrays_scene_create (A/B)
    // ---- the frame path (frame_path.hip) ----
    uint64_t max_primary_per_launch = 32ull << 20; bool max_primary_forced = false; // NRAYS_MAX_PRIMARY=n: sample batching threshold; set at all, it forces batching (tests: several launches)
    int lane_log2_override = -1;        // NRAYS_LANE_LOG2=0..6: cap of the lanes per pixel of anti-aliased frames (A/B)
    uint32_t event_stride = 4;          // NRAYS_EVENT_STRIDE=n: the events behind NraysStats::kernel_ms_* on every n-th frame (and every instrumented one): three records cost ~6 us of an 85 us frame
    int grab_override = -1;             // NRAYS_GRAB=n: tiles per dequeue of the mesh kernels (A/B; pixels do not depend on it)
    bool lpt_enabled = true;            // NRAYS_LPT=0: mesh scenes run their tiles in image order
    bool cull_enabled = true;           // NRAYS_SCREEN_CULL=0: no wave tile is decided from the scene's screen bounds
    float light_split_factor = 1.0f;    // NRAYS_LIGHT_SPLIT=x: split threshold of light-parallel tiles in units of the frame's work per resident wave (0: never, < 0: every tile)
    int occ_override = -1;              // NRAYS_OCC=2|3: waves per SIMD of the alpha-shadow mesh kernels (A/B)
    int wavefront_mode = -1;            // NRAYS_WAVEFRONT=0|1: the staged path never / whenever the scene is eligible (unset: the library's rule, wavefront.hip)
    bool lpt_analytic = true;           // NRAYS_LPT_ANALYTIC=0: analytic scenes never switch to cost-ordered lists
    bool lpt_reuse = true;              // NRAYS_LPT_REUSE=0: mesh scenes re-sort their tiles every frame even when the camera rests
    bool near_reuse = true;             // NRAYS_NEAR_REUSE=0: only the very same camera reuses an order (A/B)
    float split_hyst = 0.5f;            // NRAYS_SPLIT_HYST=x: a tile that ran in parts stays split down to this fraction of the split threshold (k_tile_order)
    uint64_t host_times_from = 0;       // NRAYS_HOST_TIMES=n: render_impl prints where the host time of the handle's frames n .. n + 3 goes (1: its first frames)
    bool pipeline = true, pipeline_always = false; // NRAYS_PIPELINE=0|2: every frame on the direct path (A/B, tests) / every eligible frame pipelined, in flight or not (tests: no dependence on timing)
    int pipe_depth = 3;                 // NRAYS_PIPELINE_DEPTH=1|2|3: traces of the handle in flight at once = its internal streams
    std::optional<bool> pipe_lead_wgs;  // NRAYS_PIPELINE_LEAD_WGS=0|1: a pipelined trace keeps the lead + second workgroups of a direct frame, or runs its lists on one workgroup per CU (unset: by the depth)
    bool lean_stamps = true, lean_slots = true, lean_plan = false; // NRAYS_PIPELINE_LEAN=0: the host path of a pipelined frame as it was — event records on timed frames, a query of the slot's
                                        // compose per frame, the plan recomputed per call (A/B; =n: the sum of 1 device stamps, 2 one slot query per several frames, 4 the plan of an unchanged block; unset: 3 —
                                        // 1 + 2 separate from 0 by the three-widths rule, 4 does not: profiles/pipeline_host_ab.log)
    uint32_t stamp_words = 64;          // NRAYS_STAMP_WORDS=1|2|..|64: words the rows of a timed k_compose spread their exit ticks over (a power of two; tuning, with bit 1 of NRAYS_PIPELINE_HOST)
    bool host_stamps = false, host_time_proof = false, host_burst = false; // NRAYS_PIPELINE_HOST=n: the sum of 1 a kernel's exit ticks spread over kStampWords words of the frame's stamp block
                                        // instead of one shared word, 2 no in-flight query when the call comes within kInFlightProofUs of the return of the handle's last pipelined
                                        // call, 4 a burst that starts behind ONE plain direct frame orders only the internal stream that shares that frame's counter sets (A/B; unset: 0, the parent's path —
                                        // none of the three separates on bench.py by the three-widths rule: profiles/pipeline_host_ab.log)
    std::optional<double> near_pixels;  // NRAYS_NEAR_PIXELS=x: a camera within x pixels of an order's camera reuses the order (unset: by the scene)
    std::optional<uint32_t> max_order_age; // NRAYS_ORDER_AGE=n: frames of nearby cameras an order serves before it is re-sorted (unset: by the scene)
    bool lead_mode = true;              // NRAYS_LEAD_WGS=0: cost-ordered lists run on one workgroup per CU instead of lead + second workgroups
    double lone_factor = 1.5;           // NRAYS_LONE_FACTOR=x: cost-ordered lead / second lists when sum / max of the tile costs < x * SIMDs
    int lead_per_wg = 4;                // NRAYS_LEAD_PER_WG=1..64: long entries per lead workgroup
    int grid_wg_per_cu = 0;             // NRAYS_GRID_WG_PER_CU=n: caps the persistent grid at n workgroups per CU (tuning)
    // ---- caller-ray batches (batch_call.cpp, ray_order.hip) ----
    int ray_reorder = 1;                // NRAYS_RAY_REORDER=0|2: a batch called unordered is traced as it comes / always reordered (unset: by its size, reorder_pays)
    int occlusion_lanes = -1;           // NRAYS_OCCLUSION_LANES=0|3|6: log2 of the lanes that serve a point of nrays_occlusion_points* and of nrays_gather_points*, and by the lights of nrays_light_points* (unset: the most that the directions or lights fill; A/B, results identical)
    // ---- the staged path (wavefront.hip) ----
    uint64_t wf_max_paths = 64ull << 20; // NRAYS_WF_MAX_PATHS=n: (pixel, sample) paths per pass over a range of wave tiles
    bool wf_fuse = false;               // NRAYS_WF_FUSE=1: single-light scenes trace their shadow ray inside k_wf_shade instead of k_wf_shadow (A/B)
    bool wf_refill = true, wf_refill_aa = false; // NRAYS_WF_REFILL=0|2: the traversal stages never refill free lanes / also in anti-aliased frames
    // ---- multi-GPU sets (multi_gpu.cpp) ----
    std::optional<bool> multi_direct;   // NRAYS_MULTI_DIRECT=0|1: the exchange gathers + k_untile / lands straight in the frame (unset: the set's own default)
    // ---- scene build (scene_build.cpp, bvh_build.cpp, bvh_device.hip) ----
    bool build_times = false;           // NRAYS_BUILD_TIMES (present): the stages of nrays_scene_create and of both BLAS builders on stderr
    bool gpu_build = true;              // NRAYS_GPU_BUILD=0: every BLAS from the host builder
    size_t gpu_build_min = 2000;        // NRAYS_GPU_BUILD_MIN=n: triangles from which a BLAS is built on the device (crossover: profiles/r04_build_crossover.log)
    std::optional<double> presplit_budget, presplit_budget_hairy;   // NRAYS_PRESPLIT_BUDGET[_HAIRY]=x: extra references pre-splitting may add, per triangle (unset: NR_PRESPLIT_BUDGET[_HAIRY])
    std::optional<double> presplit_mingain, presplit_mingain_hairy; // NRAYS_PRESPLIT_MINGAIN[_HAIRY]=x: least gain of a split worth a reference (unset: NR_PRESPLIT_MINGAIN[_HAIRY])
    std::optional<float> prim_cost, prim_cost_hairy;                // NRAYS_PRIM_COST[_HAIRY]=x: a primitive test in units of a node visit, SAH leaf criterion (unset: NR_PRIM_COST[_HAIRY])
    std::optional<int> max_leaf;        // NRAYS_MAX_LEAF=n: triangles per leaf of a device-built BLAS (unset: NR_MAX_LEAF)
    uint32_t split_grid = 512;          // NRAYS_SPLIT_GRID=n: most workgroups of k_presplit (each thread owns a 6.9 KB stack of frames)
    bool presplit_one_walk = true;      // NRAYS_PRESPLIT_ONE_WALK=0: the device pre-split walks twice instead of keeping the pieces of its counting pass (A/B)
    // ---- debug (tests and tools) ----
    int debug_build_caps = 1;           // NRAYS_DEBUG_BUILD_CAPS=n (tests): the device builder's lists get 1 / n of their capacity, so that their overflow path runs
    uint32_t debug_piece_cap = 0;       // NRAYS_DEBUG_PIECE_CAP=c (tests): c places per piece region of the one-walk pre-split, so that the regions overflow (0: sized by the budget)
    bool debug_record_always = false;   // NRAYS_DEBUG_RECORD_ALWAYS (present; NR_DEBUG_TILE_COSTS builds): steady-state frames of analytic scenes record their tile costs (tools/tile_costs.py)
    uint32_t debug_wave_work = 0;       // NRAYS_DEBUG_WAVE_WORK=n (NR_DEBUG_TILE_COSTS builds): what the second word of a wave's time record holds (tools/wave_timeline.py)
};

Switches read_switches();

} // namespace nrays
