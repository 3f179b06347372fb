// batch_call.cpp — the caller-batch driver of batch_call.h: the handle's batch workspace (trace_workspace, trace_workspace_release), the ordering of a batch
// behind the handle's previous work (batch_begin / batch_end), batch_open / batch_close, the staging arena's copies, the chunked run, and the small helpers the
// families share (reorder_pays, check_ray_flags, chunk_order, launch_status, no_permutation, check_hemisphere, occlusion_lanes_log2).  Host only: no kernel, and the environment is switches.cpp's to read.
#include "batch_call.h"

#include <algorithm>
#include <cmath>
#include <new>
#include <string>

#include "ray_order.h"

namespace nrays {

static int trace_workspace(NraysScene* sc, TraceWorkspace** out) {
    if (!sc->tw) {
        sc->tw = new (std::nothrow) TraceWorkspace();
        if (!sc->tw) return set_last_error(NRAYS_ERR_OOM, "trace workspace");
    }
    TraceWorkspace* w = sc->tw;
    if (!w->d_counts) HIP_TRY(hipMalloc((void**)&w->d_counts, kTraceCountWords * sizeof(uint32_t)));
    if (!w->d_counters) HIP_TRY(hipMalloc((void**)&w->d_counters, sizeof(DeviceCounters)));
    { const int rs = ensure_spill(sc, &w->d_spill); if (rs != NRAYS_OK) return rs; }
    *out = w;
    return NRAYS_OK;
}
void trace_workspace_release(NraysScene* sc) {
    TraceWorkspace* w = sc->tw;
    if (!w) return;
    if (w->used) (void)hipStreamSynchronize(w->last_stream);
    for (int k = 0; k < 2; ++k) if (w->queue[k].block) (void)hipFree(w->queue[k].block);
    for (void* q : {(void*)w->d_fixed, (void*)w->d_counts, (void*)w->d_counters, (void*)w->d_spill, w->d_stage, w->d_texel_owner, w->d_texel_off, (void*)w->d_texel_blocks, w->d_gather_rays, w->d_dilate_dx}) if (q) (void)hipFree(q);
    ray_order_release(w);
    delete w;
    sc->tw = nullptr;
}
// The handle's threading contract: a batch on another stream than the handle's previous work (its last render, its last batch) is
// ordered behind it, and a render that follows on yet another stream is ordered behind the batch (frame_path.hip: order_behind_previous waits on ev_switch
// recorded on sc->last.stream when last_timed is false).  Nothing a render reports (counters, timings, tile costs) is touched.
static int batch_begin(NraysScene* sc, TraceWorkspace* w, hipStream_t stream) {
    const hipStream_t prev[2] = {sc->last.have ? sc->last.stream : stream, w->used ? w->last_stream : stream};
    for (int k = 0; k < 2; ++k) {
        if (prev[k] == stream || (k == 1 && prev[1] == prev[0])) continue;
        const int rc = order_behind_stream(sc, prev[k], stream);
        if (rc != NRAYS_OK) return rc;
    }
    return NRAYS_OK;
}
static void batch_end(NraysScene* sc, TraceWorkspace* w, hipStream_t stream) {
    w->last_stream = stream; w->used = true;
    if (sc->last.have) { sc->last.stream = stream; sc->last.timed = false; sc->pipe.last_pipelined = false; sc->pipe.burst_plain = false; }
}

int batch_open(BatchCall* b, NraysScene* sc, bool staged, hipStream_t caller_stream, const StageColumn* cols, int ncols, size_t cap, BatchEnsure ensure, const void* ensure_arg) {
    if (ncols > kStageMaxColumns) return set_last_error(NRAYS_ERR_BAD_ARG, "batch_open: more columns than a table holds");
    HIP_TRY(hipSetDevice(sc->facts.device));
    b->sc = sc; b->staged = staged; b->cols = cols; b->ncols = ncols; b->stream = caller_stream;
    int rc = trace_workspace(sc, &b->w);
    if (rc == NRAYS_OK && ensure) rc = ensure(b->w, ensure_arg);
    if (rc == NRAYS_OK && staged) {
        rc = grow_device(&b->w->d_stage, &b->w->stage_bytes, stage_layout(cols, ncols, cap, b->off), 1);
        if (rc == NRAYS_OK) rc = ensure_own_stream(sc);
        if (rc == NRAYS_OK) b->stream = sc->buf.own_stream;
    }
    if (rc == NRAYS_OK) rc = batch_begin(sc, b->w, b->stream);
    return rc;
}
void batch_close(const BatchCall& b) { batch_end(b.sc, b.w, b.stream); }

void batch_columns(const BatchCall& b, size_t c0, void** col) {
    for (int k = 0; k < b.ncols; ++k) {
        const StageColumn& c = b.cols[k];
        if (b.staged) col[k] = stage_present(c) ? (char*)b.w->d_stage + b.off[k] : nullptr;
        else col[k] = c.ptr && !c.table ? (char*)c.ptr + c0 * c.item_bytes : c.ptr;
    }
}
// The copies of one phase: tables, or the columns of direction `dir` for the nc items from c0 on.
static hipError_t stage_copy(const BatchCall& b, bool tables, uint8_t dir, size_t c0, size_t nc) {
    for (int k = 0; k < b.ncols; ++k) {
        const StageColumn& c = b.cols[k];
        if ((c.table != 0) != tables || !(c.dir & dir) || !stage_present(c)) continue;
        char* dev = (char*)b.w->d_stage + b.off[k];
        char* host = (char*)c.ptr + (tables ? 0 : c0 * c.item_bytes);
        const size_t bytes = c.item_bytes * (tables ? c.table_items : nc);
        const hipError_t e = dir == kStageIn ? hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, b.stream) : hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, b.stream);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
static int stage_status(hipError_t e, const char* what, const char* phase) {
    return e == hipSuccess ? NRAYS_OK : set_last_error(NRAYS_ERR_HIP, std::string(what) + phase + hipGetErrorString(e));
}
int batch_upload_tables(const BatchCall& b, const char* what) { return b.staged ? stage_status(stage_copy(b, true, kStageIn, 0, 0), what, " tables upload: ") : NRAYS_OK; }
int batch_upload(const BatchCall& b, size_t c0, size_t nc, const char* what) { return b.staged ? stage_status(stage_copy(b, false, kStageIn, c0, nc), what, " upload: ") : NRAYS_OK; }
int batch_download(const BatchCall& b, size_t c0, size_t nc, const char* what) { return b.staged ? stage_status(stage_copy(b, false, kStageOut, c0, nc), what, " read-back: ") : NRAYS_OK; }
int batch_drain(const BatchCall& b, int rc, const char* what) {
    if (!b.staged) return rc;
    const hipError_t es = hipStreamSynchronize(b.stream); // (always: the arena is reused by the next chunk and the next call, and the uploads read the caller's arrays)
    return rc != NRAYS_OK ? rc : stage_status(es, what, " read-back: ");
}

int batch_run(NraysScene* sc, bool staged, hipStream_t caller_stream, const StageColumn* cols, int ncols, uint32_t n, uint32_t chunk, const char* what, ChunkLaunch launch,
              BatchEnsure ensure, const void* ensure_arg) {
    BatchCall b;
    int rc = batch_open(&b, sc, staged, caller_stream, cols, ncols, std::min(n, chunk), ensure, ensure_arg);
    if (rc != NRAYS_OK) return rc;
    rc = batch_upload_tables(b, what);
    if (rc != NRAYS_OK) (void)batch_drain(b, rc, what);
    void* col[kStageMaxColumns];
    for (uint32_t c0 = 0; c0 < n && rc == NRAYS_OK; c0 += std::min<uint32_t>(n - c0, chunk)) { // (chunks keep the kernels' 32-bit item indices far from overflow)
        const uint32_t nc = std::min<uint32_t>(n - c0, chunk);
        batch_columns(b, c0, col);
        rc = batch_upload(b, c0, nc, what);
        if (rc == NRAYS_OK) rc = launch(b, nc, col, (unsigned long long)c0);
        if (rc == NRAYS_OK) rc = batch_download(b, c0, nc, what);
        rc = batch_drain(b, rc, what);
    }
    batch_close(b);
    return rc;
}

bool reorder_pays(const NraysScene* sc, uint32_t n) { return sc->sw.ray_reorder == 2 || (sc->sw.ray_reorder != 0 && n >= kReorderMinRays); }
int check_ray_flags(uint32_t flags) { return (flags & ~(uint32_t)NRAYS_RAYS_UNORDERED) ? set_last_error(NRAYS_ERR_BAD_ARG, "unknown ray-batch flag") : NRAYS_OK; }
int chunk_order(NraysScene* sc, TraceWorkspace* w, bool reorder, uint32_t n, const double* o, const double* d, hipStream_t stream, const uint32_t** order) {
    *order = nullptr;
    if (!reorder) return NRAYS_OK;
    int rc = ray_order_ensure(w, n);
    if (rc == NRAYS_OK) rc = ray_order_chunk(sc, w, n, o, d, stream);
    if (rc == NRAYS_OK) *order = w->d_ray_order;
    return rc;
}
int launch_status(const char* kernel) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? (int)NRAYS_OK : set_last_error(NRAYS_ERR_HIP, std::string(kernel) + ": " + hipGetErrorString(e));
}
int no_permutation(const char* kernel) { return set_last_error(NRAYS_ERR_UNSUPPORTED, std::string(kernel) + ": no such permutation"); }
int check_hemisphere(const char* struct_name, const double* dirs, uint32_t num_dirs, const double* rotations, uint32_t num_rotations, double bias, const char* with, bool with_finite) {
    auto bad = [&](const std::string& what) { return set_last_error(NRAYS_ERR_BAD_ARG, struct_name + what); }; // (a string is built for an error alone)
    if (!dirs) return set_last_error(NRAYS_ERR_BAD_ARG, "null argument");
    if (num_dirs < 1u || num_dirs > 1024u) return bad(": num_dirs must be in 1 .. 1024");
    if (num_rotations > 1024u || (num_rotations && !rotations)) return bad(": num_rotations > 1024, or rotations is NULL");
    if (!std::isfinite(bias) || !with_finite) return bad(with ? std::string(": bias and ") + with + " must be finite" : ": bias must be finite");
    return NRAYS_OK;
}
int occlusion_lanes_log2(const NraysScene* sc, uint32_t num_dirs) {
    int lp = 6;
    if (sc->sw.occlusion_lanes >= 0) lp = sc->sw.occlusion_lanes >= 6 ? 6 : (sc->sw.occlusion_lanes >= 3 ? 3 : 0);
    while (lp > 0 && (1u << lp) > num_dirs) lp -= 3;
    return lp;
}

} // namespace nrays
