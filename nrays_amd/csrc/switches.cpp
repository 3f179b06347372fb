// switches.cpp — read_switches(): the library's one reader of the environment (switches.h).  One line per variable, in the order of
// struct Switches; an unset variable leaves the member's default.
#include "switches.h"

#include <algorithm>
#include <cstdlib>

namespace nrays {
namespace {

// The parse rules.  flag: atoi(value) != 0, so "=0" switches off; present: set at all, whatever the value; clamped / at_least: atoi / atoll, then the bounds.
void flag(const char* name, bool& v) { if (const char* e = getenv(name)) v = atoi(e) != 0; }
void flag(const char* name, std::optional<bool>& v) { if (const char* e = getenv(name)) v = atoi(e) != 0; }
bool present(const char* name) { return getenv(name) != nullptr; }
template <typename T> void integer(const char* name, T& v) { if (const char* e = getenv(name)) v = (T)atoi(e); }
template <typename T> void clamped(const char* name, T& v, int lo, int hi) { if (const char* e = getenv(name)) v = (T)std::max(lo, std::min(hi, atoi(e))); }
template <typename T> void at_least(const char* name, T& v, long long lo) { if (const char* e = getenv(name)) v = (T)std::max(lo, atoll(e)); } // 64-bit counts
template <typename T> void real(const char* name, T& v) { if (const char* e = getenv(name)) v = (T)atof(e); }
template <typename T> void real(const char* name, std::optional<T>& v) { if (const char* e = getenv(name)) v = (T)atof(e); }
constexpr int kIntMax = 0x7fffffff;

} // namespace

Switches read_switches() {
    Switches s;
    flag("NRAYS_ELIDE", s.elide);
    flag("NRAYS_NODE_QUORUM", s.node_quorum);
    flag("NRAYS_NOXFORM", s.noxform);
    flag("NRAYS_PARK", s.park);
    flag("NRAYS_LDS_SCENE", s.lds_scene);
    flag("NRAYS_TINY_SCENE", s.tiny_scene);
    if (const char* e = getenv("NRAYS_COST_SEED")) { s.seed_enabled = atoi(e) != 0; if (atoi(e) == 4) s.seed_rays = 4u; if (atoi(e) == 1) s.seed_rays = 1u; }
    flag("NRAYS_PREALLOC", s.prealloc);
    if (const char* e = getenv("NRAYS_MAX_PRIMARY")) { s.max_primary_per_launch = (uint64_t)std::max(1ll, atoll(e)); s.max_primary_forced = true; }
    clamped("NRAYS_LANE_LOG2", s.lane_log2_override, 0, 6);
    clamped("NRAYS_EVENT_STRIDE", s.event_stride, 1, kIntMax);
    clamped("NRAYS_GRAB", s.grab_override, 0, kIntMax);
    flag("NRAYS_LPT", s.lpt_enabled);
    flag("NRAYS_SCREEN_CULL", s.cull_enabled);
    real("NRAYS_LIGHT_SPLIT", s.light_split_factor);
    integer("NRAYS_OCC", s.occ_override);
    integer("NRAYS_WAVEFRONT", s.wavefront_mode);
    flag("NRAYS_LPT_ANALYTIC", s.lpt_analytic);
    flag("NRAYS_LPT_REUSE", s.lpt_reuse);
    flag("NRAYS_NEAR_REUSE", s.near_reuse);
    real("NRAYS_SPLIT_HYST", s.split_hyst);
    at_least("NRAYS_HOST_TIMES", s.host_times_from, 1);
    if (const char* e = getenv("NRAYS_PIPELINE")) { s.pipeline = atoi(e) != 0; s.pipeline_always = atoi(e) == 2; }
    clamped("NRAYS_PIPELINE_DEPTH", s.pipe_depth, 1, 3);
    flag("NRAYS_PIPELINE_LEAD_WGS", s.pipe_lead_wgs);
    if (const char* e = getenv("NRAYS_PIPELINE_LEAN")) { const int v = atoi(e); s.lean_stamps = (v & 1) != 0; s.lean_slots = (v & 2) != 0; s.lean_plan = (v & 4) != 0; }
    if (const char* e = getenv("NRAYS_STAMP_WORDS")) { const int v = std::max(1, std::min(64, atoi(e))); s.stamp_words = 1u; while ((int)(s.stamp_words * 2u) <= v) s.stamp_words *= 2u; }
    if (const char* e = getenv("NRAYS_PIPELINE_HOST")) { const int v = atoi(e); s.host_stamps = (v & 1) != 0; s.host_time_proof = (v & 2) != 0; s.host_burst = (v & 4) != 0; }
    real("NRAYS_NEAR_PIXELS", s.near_pixels);
    if (const char* e = getenv("NRAYS_ORDER_AGE")) s.max_order_age = (uint32_t)std::max(0, atoi(e));
    flag("NRAYS_LEAD_WGS", s.lead_mode);
    real("NRAYS_LONE_FACTOR", s.lone_factor);
    clamped("NRAYS_LEAD_PER_WG", s.lead_per_wg, 1, 64);
    clamped("NRAYS_GRID_WG_PER_CU", s.grid_wg_per_cu, 0, kIntMax);
    integer("NRAYS_RAY_REORDER", s.ray_reorder);
    integer("NRAYS_OCCLUSION_LANES", s.occlusion_lanes);
    at_least("NRAYS_WF_MAX_PATHS", s.wf_max_paths, 4096);
    flag("NRAYS_WF_FUSE", s.wf_fuse);
    if (const char* e = getenv("NRAYS_WF_REFILL")) { s.wf_refill = atoi(e) != 0; s.wf_refill_aa = atoi(e) == 2; }
    flag("NRAYS_MULTI_DIRECT", s.multi_direct);
    s.build_times = present("NRAYS_BUILD_TIMES");
    flag("NRAYS_GPU_BUILD", s.gpu_build);
    at_least("NRAYS_GPU_BUILD_MIN", s.gpu_build_min, 1);
    real("NRAYS_PRESPLIT_BUDGET", s.presplit_budget);
    real("NRAYS_PRESPLIT_BUDGET_HAIRY", s.presplit_budget_hairy);
    real("NRAYS_PRESPLIT_MINGAIN", s.presplit_mingain);
    real("NRAYS_PRESPLIT_MINGAIN_HAIRY", s.presplit_mingain_hairy);
    real("NRAYS_PRIM_COST", s.prim_cost);
    real("NRAYS_PRIM_COST_HAIRY", s.prim_cost_hairy);
    if (const char* e = getenv("NRAYS_MAX_LEAF")) s.max_leaf = atoi(e);
    clamped("NRAYS_SPLIT_GRID", s.split_grid, 1, kIntMax);
    flag("NRAYS_PRESPLIT_ONE_WALK", s.presplit_one_walk);
    clamped("NRAYS_DEBUG_BUILD_CAPS", s.debug_build_caps, 1, kIntMax);
    clamped("NRAYS_DEBUG_PIECE_CAP", s.debug_piece_cap, 1, kIntMax);
    s.debug_record_always = present("NRAYS_DEBUG_RECORD_ALWAYS");
    integer("NRAYS_DEBUG_WAVE_WORK", s.debug_wave_work);
    return s;
}

} // namespace nrays
