// bvh_arena.h — where the working buffers of the device BLAS build (bvh_device.hip) lie in its three arenas, one per allocation phase.
// A carve function IS the layout of its phase: it takes the phase's pieces from an Arena, in order, into the phase's buffer struct.  build_impl runs it on a
// measuring arena (no base: take() only advances `used`) for the bytes to reserve, and again on the reserved arena for the pointers, so a size cannot
// disagree with the list of pieces.  Host code without HIP types: the builder's own records (Task, Node2, ...) come in through `Rec`, a struct of aliases;
// tests/build_arena_shim.cpp compiles this header with stand-ins of the sizes below, which bvh_device.hip asserts of the real ones.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "bvh_device.h"
#include "presplit_clip.h"

namespace nrays {

constexpr uint32_t kChunk = 1024;  // references per workgroup of the large-node kernels
constexpr uint32_t kSmall = 256;   // nodes up to this many references are finished by one wave in LDS
constexpr int kBinWords = 96 * 6;  // min (or max) words of one node's bins: [axis][bin][box xyz, centroid xyz]
constexpr uint32_t kHistShift = 13, kHistBins = 1u << (32 - kHistShift);
constexpr uint32_t kScanItems = 16u, kScanBlock = 256u * kScanItems; // exclusive_scan_u32: items a thread / a workgroup
constexpr size_t kTaskBytes = 64, kNode2Bytes = 56, kSplitInfoBytes = 20, kCountersBytes = 144, kSplitFrameBytes = 328, kPartDevBytes = 48, kTmp4Bytes = 128;
constexpr size_t kArenaTail[3] = {4096, 1u << 16, 4096}; // spare bytes behind the last piece of each phase

struct ArenaPiece { size_t at, bytes; bool null; };
struct Arena { // one allocation carved into 256-byte aligned pieces; without a base it measures
    char* base = nullptr; size_t size = 0, used = 0;
    std::vector<ArenaPiece>* log = nullptr; // tests: every piece handed out
    __attribute__((noinline)) char* take_bytes(size_t bytes) { // (one copy, not one per piece)
        used = (used + 255u) & ~(size_t)255u;
        const size_t at = used;
        used += bytes;
        char* p = base && used <= size ? base + at : nullptr;
        if (log) log->push_back(ArenaPiece{at, bytes, p == nullptr});
        return p;
    }
    template <typename T> T* take(size_t n) { return reinterpret_cast<T*>(take_bytes(n * sizeof(T))); }
};
template <typename Buffers, typename Sizes> size_t measure(void (*carve)(Arena&, const Sizes&, Buffers&), const Sizes& s) { Arena a; Buffers b; carve(a, s, b); return a.used; }

// ---- phase 1: inputs, triangle records, pre-split counts ----
struct Phase1Sizes {
    std::vector<size_t> uploads; // bytes of each distinct host array, in upload order
    size_t n, nparts, frame_count, scan_bytes, u_pieces;
    uint32_t nblocks_tri, split_grid, region_cap;
    bool may_split, one_walk;
};
inline Phase1Sizes phase1_sizes(std::vector<size_t> uploads, size_t n, size_t nparts, uint32_t nblocks_tri, const DeviceBuildOptions& opt) {
    Phase1Sizes s;
    s.uploads = std::move(uploads); s.n = n; s.nparts = nparts; s.nblocks_tri = nblocks_tri;
    s.split_grid = (uint32_t)std::min<size_t>(opt.split_grid_max, (n + 255) / 256);
    // the per-thread stacks of k_presplit (0.9 GB from 131 k triangles on) exist only if pre-splitting can run at all
    s.may_split = opt.presplit && n >= 64 && opt.budget > 0.0;
    s.frame_count = s.may_split ? (size_t)s.split_grid * 256u * (kSplitDepthMax + 1) : 1u;
    s.scan_bytes = ((n + 1 + kScanBlock - 1) / kScanBlock) * sizeof(uint32_t); // block sums of the prefix sum over the per-triangle reference counts (exclusive_scan_u32)
    // one-walk pre-splitting: the pieces of the last counting pass are kept (PieceList): 1.25 x the larger budget in all, dealt to the workgroups' regions (their triangles are
    // a uniform sample of the mesh); NRAYS_PRESPLIT_ONE_WALK=0: walk twice as before (A/B)
    s.one_walk = s.may_split && opt.one_walk;
    // (NRAYS_DEBUG_PIECE_CAP=c: c places per region — tests: the regions overflow and the second walk takes over)
    s.region_cap = !s.one_walk ? 0u : opt.debug_piece_cap ? opt.debug_piece_cap
                   : (uint32_t)((size_t)(1.25 * std::max(opt.budget, opt.budget_hairy) * (double)n) / s.split_grid + 1024u);
    s.u_pieces = (size_t)s.region_cap * s.split_grid;
    return s;
}
template <class Rec> struct Phase1Buffers {
    std::vector<char*> uploads; // device copies of Phase1Sizes::uploads
    TriRec* recs; TriUv* uvs; float* tbox;
    double* part_area; double* part_tri2;
    typename Rec::Counters* ctr;
    uint32_t* counts; uint32_t* offsets; uint32_t* hist;
    typename Rec::SplitFrame* frames;
    uint32_t* scan_tmp;
    typename Rec::PartDev* parts;
    float* piece_box = nullptr; uint32_t* piece_key = nullptr; float* piece_base_box = nullptr; uint32_t* piece_count = nullptr; // PieceList (one walk only)
    char* tail;
};
template <class Rec> void carve1(Arena& a, const Phase1Sizes& s, Phase1Buffers<Rec>& b) {
    // the upload pieces come FIRST and are consecutive: the staged upload of build_impl mirrors their layout in one host buffer
    for (size_t bytes : s.uploads) b.uploads.push_back(a.take<char>(bytes));
    b.recs = a.take<TriRec>(s.n); b.uvs = a.take<TriUv>(s.n); b.tbox = a.take<float>(6 * s.n);
    b.part_area = a.take<double>(s.nblocks_tri); b.part_tri2 = a.take<double>(s.nblocks_tri);
    b.ctr = a.take<typename Rec::Counters>(1);
    b.counts = a.take<uint32_t>(s.n + 1); b.offsets = a.take<uint32_t>(s.n + 1); b.hist = a.take<uint32_t>(kHistBins);
    b.frames = a.take<typename Rec::SplitFrame>(s.frame_count);
    b.scan_tmp = reinterpret_cast<uint32_t*>(a.take<char>(s.scan_bytes + 16));
    b.parts = a.take<typename Rec::PartDev>(s.nparts);
    if (s.one_walk) {
        b.piece_box = a.take<float>(6 * s.u_pieces); b.piece_key = a.take<uint32_t>(2 * s.u_pieces); b.piece_base_box = a.take<float>(6 * s.n); b.piece_count = a.take<uint32_t>(s.split_grid + 1u);
    }
    b.tail = a.take<char>(kArenaTail[0]);
}

// ---- phase 2: references, binary build ----
struct Phase2Sizes { uint32_t R; size_t max_t, max_c, small_cap; }; // references; most tasks / chunks of a level; most small subtrees
inline Phase2Sizes phase2_sizes(size_t nrefs, int debug_cap_div) {
    Phase2Sizes s;
    s.R = (uint32_t)nrefs;
    const size_t cap_div = (size_t)std::max(1, debug_cap_div);
    s.max_t = (s.R / (kSmall + 1u)) / cap_div + 2u; s.max_c = s.R / kChunk + s.max_t + 2u; s.small_cap = (s.R / 8u + 1024u) / cap_div + 1u;
    return s;
}
template <class Rec> struct Phase2Buffers {
    float* ref_box; uint32_t* ref_tri; uint32_t* order0; uint32_t* order1;
    typename Rec::Node2* node2;
    typename Rec::Task* tasks[2]; typename Rec::Task* small;
    uint32_t* gmn; uint32_t* gmx; uint32_t* gcnt;
    typename Rec::SplitInfo* split;
    uint32_t* chunk_base; uint32_t* chunk_task; uint32_t* chunk_off; uint32_t* scan_tmp; uint32_t* chunk_lefts; uint32_t* chunk_cnt;
    uint32_t* level2; // k_chunk_scan_next: {tasks, chunks} of the next level
    char* tail;
};
template <class Rec> void carve2(Arena& a, const Phase2Sizes& s, Phase2Buffers<Rec>& b) {
    b.ref_box = a.take<float>(6 * (size_t)s.R); b.ref_tri = a.take<uint32_t>(s.R);
    b.order0 = a.take<uint32_t>(s.R); b.order1 = a.take<uint32_t>(s.R);
    b.node2 = a.take<typename Rec::Node2>(s.R);
    b.tasks[0] = a.take<typename Rec::Task>(s.max_t); b.tasks[1] = a.take<typename Rec::Task>(s.max_t); b.small = a.take<typename Rec::Task>(s.small_cap);
    b.gmn = a.take<uint32_t>(s.max_t * kBinWords); b.gmx = a.take<uint32_t>(s.max_t * kBinWords); b.gcnt = a.take<uint32_t>(s.max_t * 96u);
    b.split = a.take<typename Rec::SplitInfo>(s.max_t); b.chunk_base = a.take<uint32_t>(s.max_t + 1);
    b.chunk_task = a.take<uint32_t>(s.max_c); b.chunk_off = a.take<uint32_t>(s.max_c); b.scan_tmp = a.take<uint32_t>(s.max_c); b.chunk_lefts = a.take<uint32_t>(s.max_c);
    b.chunk_cnt = a.take<uint32_t>(s.max_c * 96u);
    b.level2 = a.take<uint32_t>(2);
    b.tail = a.take<char>(kArenaTail[1]);
}

// ---- phase 3: collapse ----
struct Phase3Sizes { uint32_t nb; }; // binary nodes
template <class Rec> struct Phase3Buffers { typename Rec::Tmp4* tmp; char* tail; };
template <class Rec> void carve3(Arena& a, const Phase3Sizes& s, Phase3Buffers<Rec>& b) { b.tmp = a.take<typename Rec::Tmp4>(s.nb); b.tail = a.take<char>(kArenaTail[2]); }

} // namespace nrays
