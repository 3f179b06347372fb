// The arena layouts of the device BLAS build (nrays_amd/csrc/bvh_arena.h) on the host compiler, for tests/test_build_arena.py and tests/build_arena_main.cpp:
// the carve functions run on a measuring arena and on a real one (an address range reserved with mmap, never touched) with stand-ins for the builder's records.
#include <sys/mman.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "bvh_arena.h"

namespace {
using namespace nrays;

template <size_t N> struct Bytes { alignas(4) char b[N]; };
struct Rec { // stand-ins of the sizes bvh_device.hip asserts of its records
    using Task = Bytes<kTaskBytes>; using Node2 = Bytes<kNode2Bytes>; using SplitInfo = Bytes<kSplitInfoBytes>; using Counters = Bytes<kCountersBytes>;
    using SplitFrame = Bytes<kSplitFrameBytes>; using PartDev = Bytes<kPartDevBytes>; using Tmp4 = Bytes<kTmp4Bytes>;
};
static_assert(sizeof(Rec::SplitInfo) == 20 && sizeof(Rec::SplitFrame) == 328, "a stand-in has the size of its record");

struct Case { uint64_t n, nrefs, upload_bytes; uint32_t parts, one_walk, cap_div, piece_cap, nb; };

DeviceBuildOptions options(const Case& c) { DeviceBuildOptions o; o.one_walk = c.one_walk != 0; o.debug_cap_div = (int)c.cap_div; o.debug_piece_cap = c.piece_cap; return o; }
std::vector<size_t> uploads(const Case& c) { // three arrays a part, sizes from upload_bytes up
    std::vector<size_t> u;
    for (uint32_t k = 0; k < 3 * c.parts; ++k) u.push_back((size_t)c.upload_bytes + 24u * k);
    return u;
}
uint32_t tri_blocks(const Case& c) { return (uint32_t)((c.n + 255) / 256 + c.parts - 1); } // (every part rounds its own blocks up)

// Carves phase `phase` of the case twice — measuring, then on a reserved range of exactly the measured bytes — and returns the second run's pieces.
size_t carve(const Case& c, int phase, std::vector<ArenaPiece>& log) {
    const Phase1Sizes s1 = phase1_sizes(uploads(c), c.n, c.parts, tri_blocks(c), options(c));
    const Phase2Sizes s2 = phase2_sizes(c.nrefs, (int)c.cap_div);
    const Phase3Sizes s3{c.nb};
    const size_t total = phase == 1 ? measure(carve1<Rec>, s1) : phase == 2 ? measure(carve2<Rec>, s2) : measure(carve3<Rec>, s3);
    void* range = mmap(nullptr, total, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (range == MAP_FAILED) return 0;
    Arena a; a.base = (char*)range; a.size = total; a.log = &log;
    if (phase == 1) { Phase1Buffers<Rec> b; carve1<Rec>(a, s1, b); }
    else if (phase == 2) { Phase2Buffers<Rec> b; carve2<Rec>(a, s2, b); }
    else { Phase3Buffers<Rec> b; carve3<Rec>(a, s3, b); }
    munmap(range, total);
    return a.used == total ? total : 0;
}

// What the builder reserved before its layouts were carve functions: a hand-written sum, piece for piece, that had to match the take<>() calls.  Restated here as
// the upper bound of the measured totals.
template <typename T> size_t padded(size_t n) { return ((n * sizeof(T)) + 255u + 256u) & ~(size_t)255u; }
size_t former_bytes(const Case& c, int phase) {
    const Phase1Sizes s = phase1_sizes(uploads(c), c.n, c.parts, tri_blocks(c), options(c));
    const size_t n = (size_t)c.n;
    if (phase == 1) {
        size_t bytes1 = 0;
        for (size_t u : s.uploads) bytes1 += padded<char>(u);
        bytes1 += padded<TriRec>(n) + padded<TriUv>(n) + padded<float>(6 * n) + 2 * padded<double>(s.nblocks_tri) + padded<Rec::Counters>(1) + 2 * padded<uint32_t>(n + 1) +
                  padded<uint32_t>(kHistBins) + padded<Rec::SplitFrame>(s.frame_count) + padded<char>(s.scan_bytes) + padded<Rec::PartDev>(c.parts) + 4096;
        if (s.one_walk) bytes1 += padded<float>(6 * s.u_pieces) + padded<uint32_t>(2 * s.u_pieces) + padded<float>(6 * n) + padded<uint32_t>(s.split_grid + 1u);
        return bytes1;
    }
    if (phase == 2) {
        const uint32_t R = (uint32_t)c.nrefs;
        const size_t cap_div = (size_t)std::max(1, (int)c.cap_div);
        const size_t max_t = (R / (kSmall + 1u)) / cap_div + 2u, max_c = R / kChunk + max_t + 2u, small_cap = (R / 8u + 1024u) / cap_div + 1u;
        return padded<float>(6 * (size_t)R) + 3 * padded<uint32_t>(R) + padded<Rec::Node2>(R) + 2 * padded<Rec::Task>(max_t) + padded<Rec::Task>(small_cap) + 2 * padded<uint32_t>(max_t * kBinWords) +
               padded<uint32_t>(max_t * 96u) + padded<Rec::SplitInfo>(max_t) + padded<uint32_t>(max_t + 1) + 4 * padded<uint32_t>(max_c) + padded<uint32_t>(max_c * 96u) + (1u << 16);
    }
    return padded<Rec::Tmp4>(c.nb) + 4096;
}

bool sound(const Case& c, int phase) {
    std::vector<ArenaPiece> log;
    const size_t total = carve(c, phase, log);
    if (!total || log.empty() || total > former_bytes(c, phase)) return false;
    size_t end = 0;
    for (const ArenaPiece& p : log) {
        if (p.null || p.at % 256u || p.at < end || p.at + p.bytes > total) return false;
        end = p.at + p.bytes;
    }
    return true;
}

} // namespace

extern "C" {

// The pieces of one phase of a case, in carve order; returns their number (at most `cap` are written) and the measured total, 0 pieces when the two runs disagree.
int build_arena_pieces(const Case* c, int phase, uint64_t* at, uint64_t* bytes, uint32_t* null, int cap, uint64_t* total) {
    std::vector<ArenaPiece> log;
    *total = carve(*c, phase, log);
    if (!*total) return 0;
    for (int k = 0; k < (int)log.size() && k < cap; ++k) { at[k] = log[k].at; bytes[k] = log[k].bytes; null[k] = log[k].null; }
    return (int)log.size();
}
uint64_t build_arena_former_bytes(const Case* c, int phase) { return former_bytes(*c, phase); }
int build_arena_check(const Case* c, int phase) { return sound(*c, phase) ? 0 : -1; }

// The sweep of tests/test_build_arena.py in the shim itself (what tests/build_arena_main.cpp runs under the sanitizers): the number of unsound layouts.
uint64_t build_arena_sweep(uint64_t* cases) {
    uint64_t bad = 0; *cases = 0;
    for (uint64_t n : {1ull, 63ull, 64ull, 2000ull, 70000ull, 2880000ull})
        for (uint32_t parts : {1u, 270u})
            for (uint64_t up : {24ull, (1ull << 20) - 8, 1ull << 20, (1ull << 20) + 24})
                for (uint32_t one_walk : {1u, 0u})
                    for (uint32_t cap_div : {1u, 64u})
                        for (uint32_t piece_cap : {0u, 8u})
                            for (uint64_t nrefs : {n, 9 * n})
                                for (int phase = 1; phase <= 3; ++phase) {
                                    const Case c{n, nrefs, up, parts, one_walk, cap_div, piece_cap, (uint32_t)(nrefs > 1 ? nrefs - 1 : 1)};
                                    if (!sound(c, phase)) ++bad;
                                    ++*cases;
                                }
    return bad;
}

} // extern "C"
