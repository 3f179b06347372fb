// scene_handle.h — the scene handle behind the C ABI (NraysScene) and what the library's translation units share
// around it.  Host only; frame_path.hip owns the megakernel path (k_primary), wavefront.hip the staged path, batch_call.cpp the
// caller batches' workspace and driver (their families: ray_batches.hip, point_batches.hip, texel_calls.hip; the reorder: ray_order.hip), nrays_hip.hip the handle's lifetime.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <string>
#include <vector>

#include "../../include/nrays_abi.h"
#include "device_types.h"
#include "scene_build.h"
#include "switches.h"

namespace nrays {

int set_last_error(int status, const std::string& msg); // nrays_hip.hip: sets nrays_last_error(), returns `status`
struct WavefrontState;                                   // wavefront.hip: buffers of the staged path, created on first use

// A failed HIP call ends the function: its status (out of memory told apart) and the call's text become the last error.
#define HIP_TRY(expr)                                                                                                                  \
    do {                                                                                                                               \
        hipError_t e_ = (expr);                                                                                                        \
        if (e_ != hipSuccess)                                                                                                          \
            return nrays::set_last_error(e_ == hipErrorOutOfMemory ? NRAYS_ERR_OOM : NRAYS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

struct QueueMem {
    RayQueue q;
    void* block = nullptr;
};

// A camera as the scheduler sees it (frame_path.hip: cam_snapshot): eye, unit rays through the four corners of the frame, the angle of a pixel,
// the distance to the scene's bounding box.
struct CamSnap { double eye[3] = {0, 0, 0}; double dir[4][3] = {}; double pix_angle = 0.0, depth = 1.0; bool valid = false; };

// What plan_frame (frame_path.hip) decides once per frame.  The phases read it; the header comment of each names what it may still change: grid, grab, R.lead_*, R.tile_order,
// R.tile_cost — and which group of the handle it writes.  Every phase reads sc->sw and sc->facts; none writes them.
struct FramePlan {
    uint32_t rows; uint64_t npix_local;    // rows and pixels of the local frame buffer
    uint64_t owned_rows;                   // rows of the image this frame owns (all of them, or its bands): what the ray counts are made of
    bool queued; uint32_t batch;           // the scene needs the HBM queue (double branching); samples per k_primary launch
    uint32_t lane_log2, bwl, bhl;          // log2 of the lanes per pixel of an anti-aliased frame, of the width / height of a scheduling unit's pixel block
    uint32_t tiles_x, tiles_y, ntiles;     // scheduling blocks of the frame; ntiles in units of four wave tiles
    bool banded; uint32_t win_units;       // the frame owns bands of rows only; scheduling blocks inside the window (DRender::win_*)
    int occ; uint32_t grid, grab;          // k_primary's OCC (0 or 3), its persistent grid, tiles per dequeue (0 = workgroup lists through LDS)
    bool timed; int slot;                  // this frame is timed (events or stamps of the ring), into this slot
    bool single_launch, staged;            // nothing follows the one k_primary launch; the staged path (wavefront.hip) renders the frame
    uint64_t sched_key, cam; CamSnap snap; // geometry key, camera hash and camera of the per-camera scheduling state (not filled for staged frames)
};

constexpr int kNumCounts = kMaxGenerations + 2 + 8; // queue round counters + 8 per-XCD work counters
constexpr int kMaxGrid = 2048;     // upper bound of the persistent grid (the launch uses CUs x waves/SIMD workgroups)

// Workspace of the caller batches (nrays_trace_rays* and every later family; batch_call.cpp): created on first use, grown
// only when a chunk needs more, freed with the handle.  It shares no device memory with the renders, so that a batch leaves their
// per-frame state (queues, counters, fixed-point sums, scheduling state) exactly as it found it.
constexpr uint32_t kTraceChunk = 1u << 22; // rays per chunk of a batch: bounds the queues and sums below for any batch size
constexpr int kTraceCountWords = kMaxGenerations + 3; // round counters 0..kMaxGenerations + 1, then the batch's queue-overflow word
struct TraceWorkspace {
    QueueMem queue[2];
    uint32_t queue_capacity = 0;
    long long* d_fixed = nullptr; size_t fixed_slots = 0; // left cleared by k_fold_fixed
    bool fixed_dirty = false;                               // rounds were enqueued and their k_fold_fixed was not (an error in between)
    uint32_t* d_counts = nullptr;                           // kTraceCountWords
    DeviceCounters* d_counters = nullptr;                   // sink of the kernels' ray-class counters (never reported)
    uint32_t* d_spill = nullptr;                            // traversal-stack spill region of the batch kernels
    void* d_stage = nullptr; size_t stage_bytes = 0;        // the blocking forms' staging arena: device copies of one chunk's host arrays (batch_stage.h lays them out)
    hipStream_t last_stream = nullptr; bool used = false;   // stream of the last batch (ordering, nrays_scene_destroy)
    // Batches the caller called unordered (NRAYS_RAYS_UNORDERED; ray_order.hip): created on the first such chunk, grown only when a chunk holds more rays
    uint64_t* d_ray_keys = nullptr; uint32_t* d_ray_rank = nullptr; uint32_t* d_ray_order = nullptr; size_t order_rays = 0; // per ray: key, place inside its bin, order[j] = ray traced j-th
    double* d_ray_frame = nullptr; double* d_ray_partial = nullptr; // the chunk's quantisation frame (ray_key.h) and the per-workgroup bounds it is reduced from
    uint32_t* d_ray_bins = nullptr; uint32_t* d_ray_scan = nullptr; // bin counts (+ one word: a gather chunk's total), scanned in place into bin starts; block sums of that scan
    // nrays_surface_texels* (surface_texels_kernel.h): the owner word of every lattice point, the scanned tile counts of the node's triangle records, the block sums of that scan + the total
    void* d_texel_owner = nullptr; size_t texel_owner_words = 0; void* d_texel_off = nullptr; size_t texel_off_words = 0; unsigned long long* d_texel_blocks = nullptr;
    // nrays_gather_points* in double-branching scenes and in every reordered chunk of the _ex forms: the colours of one chunk's rays (x 3), between k_gather_points /
    // k_gather_pairs_ordered, the queue's rounds and k_gather_fold
    void* d_gather_rays = nullptr; size_t gather_ray_floats = 0;
    // nrays_dilate_texels* (texel_dilate_kernel.h): per lattice point the 16-bit dx word the row pass leaves for the column pass
    void* d_dilate_dx = nullptr; size_t dilate_points = 0;
};

} // namespace nrays

using nrays::DeviceCounters; using nrays::DScene; using nrays::HostScene; using nrays::QueueMem;

// The handle, in parts: what is fixed when it is created (sw, facts), device memory that only grows (buf), and the bookkeeping of the frame path, one
// group per concern.  The phases of frame_path.hip name the group they own in their headers.
struct NraysScene {
    static constexpr int kCountSets = 6;  // counter sets a handle allocates (Buffers)
    static constexpr int kPipeStreams = 3, kPipeSlots = 2 * kPipeStreams; // the most a handle uses: the caller's stream + 3 fill a process's four hardware queues
    static constexpr int kRing = 256;     // slots of the event ring
    static constexpr int kStampBlock = (int)(nrays::kStampHead + nrays::kStampWords); // words of a ring slot's device stamps (Ring::d_stamps)

    nrays::Switches sw; // the environment's switches as nrays_scene_create found them: never written afterwards, never re-read in the frame path (switches.h)

    // Fixed when the handle is created (nrays_hip.hip: upload_scene_arrays, derive_scene_facts and the three optional tables).
    struct Facts {
        int device = 0;
        HostScene host;          // kept for counts only; bulk arrays are released after upload
        DScene d;
        std::vector<void*> allocs;
        uint64_t scene_bytes = 0; // device bytes of the uploaded scene arrays (BVH nodes, triangles, records, textures)
        size_t num_nodes = 0, num_tris = 0; // entries of d.nodes / d.tris, device-built and host-built together (nrays_debug_scene_dump)
        int num_cus = 256;
        int features = nrays::kFeatAll;
        bool park = true;     // kFeatPark permutations for the three-wave multi-light kernels (Switches::park)
        bool noxform = false; // every BLAS untransformed: the kFeatNoXform permutations of the mesh kernels render this scene
        bool tiny = false;    // opaque analytic scene of at most kTinyLeaves TLAS leaves: the kFeatTinyScene permutations render it (Switches::tiny_scene)
        uint32_t light_lsl = 0;     // light-parallel tiles: log2 of the lanes per pixel (0 = the scene is not eligible)
        uint32_t spill_entries = 0; // HBM stack entries per lane beyond the kLdsStack entries kept in LDS (0 = never needed)
        const float* d_seed_boxes = nullptr; uint32_t seed_boxes = 0; // k_seed_costs: world boxes of the nodes that can continue a chain
    } facts;

    // Device memory that only grows, and the indices that rotate through it.
    struct Buffers {
        QueueMem queue[2];
        uint32_t queue_capacity = 0;
        // Rotating sets: launch n uses set n mod count_rot and clears set (n + count_rot / 2) mod count_rot (frames likewise), count_rot = 2 x the streams
        // the handle's traces may run on (pipelined frames below; at least 4).  The launch whose set is cleared is the NEXT one on the clearing launch's own
        // stream, so no launch that can overlap this one reads or counts into the set being cleared; launches on the same stream are ordered among themselves.
        // (With three streams "clear n + 2" would be wrong: launch n + 2 runs on another stream and may have started.)
        int count_rot = 4;                               // 4 (pipeline depth 1, 2) or 6 (depth 3): fixed when the handle is created
        uint32_t* d_counts_set[kCountSets] = {};         // kNumCounts each
        DeviceCounters* d_counters_set[kCountSets] = {}; // per frame
        uint32_t* d_counts = nullptr;         // set used by the last launch
        DeviceCounters* d_counters = nullptr; // set used by the last frame
        uint64_t launch_index = 0, frame_index = 0;
        uint32_t* d_spill = nullptr;
        long long* d_fixed = nullptr; size_t fixed_slots = 0; // per-pixel fixed-point sums of the queued chains (double-branching scenes)
        bool fixed_dirty = false; // k_bounce rounds were enqueued and their k_fold_fixed was not (an error in between): cleared at the next frame's start
        float* d_frame = nullptr; size_t frame_floats = 0;
        uint8_t* d_rgb8 = nullptr; size_t rgb8_bytes = 0; // nrays_render_rgb8
        hipStream_t own_stream = nullptr;                 // the stream of the blocking entry points (ensure_own_stream)
    } buf;

    // The per-camera scheduling state (frame_path.hip: schedule_mesh, schedule_analytic, record_costs, ensure_tile_arrays).  No pixel depends on it.
    struct Order {
        // previous frame's wave-tile costs (k_primary) and the order derived from them (k_tile_order); valid for one
        // (width, rows, band) geometry at a time
        uint32_t* d_tile_cost = nullptr; uint32_t* d_tile_order = nullptr; uint32_t tile_slots = 0;
        hipEvent_t ev_rec[2] = {nullptr, nullptr}; bool rec_events_valid = false; int rec_slot = -1; // around the last primary launch that recorded tile costs (NraysTileCosts::kernel_ms)
        unsigned long long* d_cost_meta = nullptr; // DRender::cost_meta: start / end ticks and the measured clock of the launch that recorded d_tile_cost
        uint32_t* d_order_len = nullptr;           // light-parallel tiles: the lengths of the eight lists
        uint64_t cost_key = 0; bool cost_valid = false;
        uint32_t cost_tiles = 0, cost_grid = 0, cost_split_lsl = 0; // wave tiles / workgroups / log2 of a split tile's parts of the frame that recorded d_tile_cost last (nrays_get_tile_costs)
        // analytic scenes (workgroup lists): costs are recorded on the first frame of a camera, sorted once on the second, and
        // the order is then reused as long as the camera stays (the scene of a handle never changes)
        uint64_t cost_cam = 0, order_key = 0, order_cam = 0; bool order_valid = false; uint32_t order_age = 0;
        // ... and by cameras NEAR the one whose costs it was sorted from (frame_path.hip: cam_shift_px) for up to max_order_age frames, so that a moving camera does not
        // record and sort on every frame.  order_seeded: the order comes from k_seed_costs' guess, the next frame replaces it.
        nrays::CamSnap cost_snap, order_snap; bool order_seeded = false;
        double near_pixels = 16.0; uint32_t max_order_age = 8; // Switches::near_pixels / max_order_age, or the scene's defaults (derive_scene_facts)
        bool lone_known = false; uint64_t lone_key = 0, stats_key = 0; // the lead / second decision of the last sort that reported, and the geometry it belongs to
        // ... and the sort also reports the sum and the maximum of the costs: their ratio is the frame's parallelism, which
        // decides between cost-ordered lists with the long tiles on the first workgroup of each CU (few long tiles) and image-order
        // lists (many tiles: throughput)
#ifdef NR_DEBUG_TILE_COSTS
        uint32_t* d_wave_times = nullptr; uint32_t dbg_grid = 0; uint32_t* d_seed_copy = nullptr;
#endif
        unsigned long long* d_cost_stats = nullptr; unsigned long long* h_cost_stats = nullptr; hipEvent_t ev_stats = nullptr;
        bool stats_pending = false, lone_waves = false;
    } order;

    // Pipelined frames (frame_path.hip: pipeline_prepare, pipeline_compose): a frame enqueued while its predecessor is still in flight traces its window on one of up to three
    // library-owned non-blocking streams into a staging frame and is composed into `out` on the caller's stream (k_compose).  Slot s = launch
    // index mod slots: its stream (s mod Switches::pipe_depth), its staging rows, "traced" (recorded behind the trace) and "composed" (behind the compose that read the slot).
    struct Pipe {
        bool enabled = true;                    // Switches::pipeline, until the staging frames cannot be allocated: every frame on the direct path from then on
        // (twice as many slots as streams: with as many, the trace of frame k + depth waited for the compose of frame k, and a wait across queues costs 12 - 23 us on
        // this stack — the chain trace -> compose -> trace made the pipelined frame slower than the direct one; profiles/pipelined_frames_ab.log)
        int slots = 6;                          // 4 at depth 1 and 2, 6 at depth 3
        bool lead_wgs = false;                  // a pipelined trace keeps the lead + second workgroups of a direct frame (default at depth 1, 2) or runs its cost-ordered
                                                // lists on one workgroup per CU (default at depth 3: three grids share two wave slots per SIMD); Switches::pipe_lead_wgs overrides
        hipStream_t stream[kPipeStreams] = {};
        // A slot holds the rows [wr0, wr1) of the window only (the trace with DRender::no_rows writes nothing else; k_compose reads nothing else): the kernels get
        // `stage[s] - wr0 * width * 3`, which they address like `out`.  floats: floats allocated per slot; grown when a window needs more rows.
        float* stage[kPipeSlots] = {}; size_t floats = 0;
        uint32_t* spill[kPipeStreams] = {};     // a traversal-stack spill region per internal stream (spill_entries != 0): traces that overlap must not share buf.d_spill
        hipEvent_t ev_traced[kPipeSlots] = {}, ev_composed[kPipeSlots] = {};
        bool last_pipelined = false;            // the previous work of the handle was a pipelined frame: last.done is its "composed" event
        // Which composes the host knows to be over (Switches::lean_slots), in launch numbers (buf.launch_index of the frame's trace + 1; 0 = none).  Composes run in call order
        // on the caller's streams, each ordered behind its predecessor, so a compose seen finished proves every earlier one: a trace into a slot whose last compose is at or below
        // composed_seen needs neither a query nor a wait.  slot_launch[s]: the compose ev_composed[s] was last recorded behind; newest_launch: the handle's latest compose.
        uint64_t composed_seen = 0, newest_launch = 0, slot_launch[kPipeSlots] = {};
        // Switches::host_time_proof: when the handle's last pipelined call returned.  A call that arrives within kInFlightProofUs of it comes from a caller that did not wait for
        // that frame (frame_path.hip: pipeline_prepare), so it is pipelined without asking the device.
        std::chrono::steady_clock::time_point last_return{};
        // Switches::host_burst: the handle's only work since its last pipelined frame is ONE plain direct frame of render_impl (single launch, nothing recorded or sorted,
        // not instrumented / banded / staged), which was launch `burst_launch` (buf.launch_index before it).  Cleared by everything else that runs on the handle.
        bool burst_plain = false; uint64_t burst_launch = 0;
        // nrays_debug_pipeline_counts: host bookkeeping since the handle was created — frames pipelined, frames direct, in-flight queries issued, slot waits enqueued
        uint64_t n_pipelined = 0, n_direct = 0, n_inflight_queries = 0, n_slot_waits = 0;
    } pipe;

    // Ring of HIP event triples (frame begin, primary kernel begin/end, frame end) recorded on the render
    // stream; nrays_get_stats averages the frames recorded since its previous call.  Only every Switches::event_stride-th frame of a handle (and every
    // instrumented one) records them; the averages are over the sampled frames.
    struct Ring {
        hipEvent_t ev_begin[kRing] = {}, ev_pbegin[kRing] = {}, ev_pend[kRing] = {}, ev_end[kRing] = {};
        bool single_launch[kRing] = {};
        bool has_prepass[kRing] = {}; // the frame started with k_tile_order: ev_begin was recorded before it
        uint64_t frames_recorded = 0, frames_reported = 0, frames_total = 0;
        DeviceCounters* d_counters_primary = nullptr; // snapshot taken right after the primary kernel
        // A timed PIPELINED frame records none of the slot's events (three records cost its call 8 - 9 us): its trace and its compose leave 100 MHz ticks in the slot's four
        // words of d_stamps (DRender::stamp; allocated and zeroed with the handle, Switches::lean_stamps), which nrays_get_stats copies in one piece.  A slot's block is
        // kStampBlock words: the four of DRender::stamp, then kStampWords words the rows of k_compose spread their exit ticks over (Switches::host_stamps; their maximum counts).
        enum : uint8_t { kByEvents = 0, kByStamps = 1, kUntimed = 2 }; // kUntimed: the launch fell back to a kernel that does not stamp (tuning builds)
        uint8_t timed_by[kRing] = {};
        unsigned long long* d_stamps = nullptr; // kRing x kStampBlock words
    } ring;

    // The plan of the last parameter block (Switches::lean_plan): a call whose block and `instrumented` flag are the same bytes reuses `f` and `R` as plan_frame left them —
    // before the schedulers and pipeline_prepare changed anything — and recomputes only f.timed and f.slot.  What plan_frame reads of the handle (sw, facts) never changes.
    struct Plan {
        bool valid = false, instrumented = false;
        NraysRenderParams p;
        nrays::FramePlan f; nrays::DRender R;
    } plan;

    // The last render: what the next call orders itself behind, what nrays_get_stats and the probes report.
    struct Last {
        hipStream_t stream = nullptr;
        hipEvent_t done = nullptr;      // last event recorded by the previous render (one of the ring's events)
        hipEvent_t ev_switch = nullptr; // recorded on the previous render's stream when a render arrives on another one
        bool have = false, timed = true; // a render has run; it recorded `done`
        uint64_t primary = 0, primary_first_batch = 0;
        bool instrumented = false;
        // nrays_debug_last_permutation: the k_primary permutation(s) the most recent render launched (host bookkeeping of launch_primary(), no device work)
        uint32_t perm_last[4] = {0, 0, 0, 0}; // STATS, FEAT, PLAIN, OCC of the last launch
        uint32_t perm_launches = 0;           // k_primary launches of that render (0: none yet, or the staged path rendered it)
        bool perm_mixed = false;              // its launches did not all run the same permutation (sample batches: only the first can be plain)
    } last;

    nrays::WavefrontState* wf = nullptr;            // staged (wavefront) path: queues, chunk tables, sums (wavefront.hip)
    nrays::TraceWorkspace* tw = nullptr;            // caller-ray batches (nrays_trace_rays*), created on first use
};

namespace nrays {
// ---- what the translation units call of each other ----
// nrays_hip.hip.  ensure_spill: a traversal-stack spill region (the handle's, a pipeline stream's, the caller-ray workspace's), allocated on first use when the scene's trees are
// deeper than the LDS part of the stack (spill_entries != 0); *region stays null otherwise.  ensure_own_stream: the stream of the blocking entry points, created on first use.
// order_behind_stream: work enqueued on `stream` from here on runs behind what `prev` holds now (ev_switch recorded there and waited for: no host stall).
// grow_device: a device buffer that only grows — freed and re-allocated (contents not kept) when it holds fewer than `want` elements of `elem` bytes.
int ensure_spill(const NraysScene* sc, uint32_t** region);
int ensure_own_stream(NraysScene* sc);
int order_behind_stream(NraysScene* sc, hipStream_t prev, hipStream_t stream);
int grow_device(void** buffer, size_t* have, size_t want, size_t elem);
// frame_path.hip.  render_impl: one frame of `p` into d_out on `stream`.  tile_rows: rows of the local frame buffer (the image's, or this owner's bands).
// preallocate_first_frame: what a first frame would allocate (nrays_scene_create).  pipeline_release: the pipelined frames' streams, events and buffers (nrays_scene_destroy).
int render_impl(NraysScene* sc, const NraysRenderParams* p, float* d_out, hipStream_t stream, bool instrumented, uint32_t count_flags = 0u);
uint32_t tile_rows(const NraysRenderParams* p);
void preallocate_first_frame(NraysScene* sc);
void pipeline_release(NraysScene* sc);
constexpr double kNearPixels = 16.0; // (frame_path.hip: cam_shift_px; nrays_scene_create derives the handle's default from it)
void trace_workspace_release(NraysScene* sc); // batch_call.cpp: drains and frees the caller-ray workspace, if a batch ever ran
} // namespace nrays
