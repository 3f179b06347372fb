// The host compiler's build of nrays_amd/csrc/batch_stage.h (tests/test_batch_stage.py; tests/batch_stage_main.cpp runs the same sweep as a program of its
// own, under the sanitizers): every family's column table exactly as the library fills it, and where stage_layout() puts the columns.
#include <cstdint>

#include "batch_stage.h"

using namespace nrays;

extern "C" {

enum { kFamTrace, kFamIntersects, kFamCast, kFamShade, kFamOcclusion, kFamGather, kFamGatherMaps, kFamSurfaceTexels, kFamDilate, kFamFilter, kFamRayProbe, kFamPointProbe,
       kFamShFoldProbe, kFamCastProbe, kFamOccRaysProbe, kFamCount };

// mask: bit k = the family's k-th optional array is given.  bands: 0 = nrays_gather_points, 1 .. 3 = nrays_gather_sh_points.
struct BatchStageCase { uint32_t family, mask, num_dirs, num_rotations, bands, channels, num_maps, map_w, map_h, num_nodes; };

// The number of optional arrays of a family (the bits of BatchStageCase::mask that count).
int batch_stage_optional(uint32_t family) {
    static const int opt[kFamCount] = {3, 0, 5, 3, 3, 2, 3, 4, 3, 0, 0, 2, 2, 1, 1};
    return family < kFamCount ? opt[family] : -1;
}

// Fills the table of a case: per column its offset for chunks of `cap` items, bytes, alignment and whether the blocking form copies it; *total = the arena's bytes.
// Returns the number of columns (at most kStageMaxColumns), or -1.
int batch_stage_table(const BatchStageCase* cs, uint64_t cap, uint64_t* off, uint64_t* bytes, uint32_t* align, uint32_t* present, uint64_t* total) {
    static double d8[4]; static float f4[4]; static uint32_t u4[4]; static int32_t i4[4]; static uint64_t u8[4]; // (never dereferenced: any non-null address)
    const uint32_t m = cs->mask;
    auto opt = [&](int bit, auto* p) -> decltype(p) { return (m >> bit) & 1u ? p : nullptr; };
    const double* rot = cs->num_rotations ? d8 : nullptr;
    StageColumn c[kStageMaxColumns];
    int n = -1;
    switch (cs->family) {
    case kFamTrace: n = trace_columns(c, d8, d8, opt(0, d8), opt(1, u8), opt(2, f4), f4); break;
    case kFamIntersects: n = intersects_columns(c, d8, d8, d8, f4, u4); break;
    case kFamCast: n = cast_columns(c, d8, d8, opt(0, d8), d8, i4, opt(1, d8), opt(2, d8), opt(3, i4), opt(4, u4)); break;
    case kFamShade: n = shade_columns(c, d8, d8, d8, opt(0, d8), i4, opt(1, u4), opt(2, u8), f4); break;
    case kFamOcclusion:
        point_columns(c, d8, cs->num_dirs, rot, cs->num_rotations, d8, d8, opt(0, u4), opt(1, u8));
        n = occlusion_columns(c, f4, opt(2, u4));
        break;
    case kFamGather: case kFamShFoldProbe:
        point_columns(c, d8, cs->num_dirs, rot, cs->num_rotations, d8, d8, opt(0, u4), opt(1, u8));
        n = gather_columns(c, f4, cs->bands ? 3u * cs->bands * cs->bands : 3u, cs->family == kFamShFoldProbe ? f4 : nullptr, cs->num_dirs);
        break;
    case kFamGatherMaps: {
        if (cs->num_maps > 16u) return -1;
        const void* texels[16]; size_t count[16];
        for (uint32_t k = 0; k < cs->num_maps; ++k) { texels[k] = f4; count[k] = (size_t)cs->map_w * cs->map_h; }
        point_columns(c, d8, cs->num_dirs, rot, cs->num_rotations, d8, d8, opt(0, u4), opt(1, u8));
        n = gather_maps_columns(c, f4, opt(2, u4), i4, cs->num_nodes, cs->num_maps, texels, count);
        break;
    }
    case kFamSurfaceTexels: n = surface_texel_columns(c, d8, opt(0, d8), opt(1, d8), opt(2, i4), opt(3, i4), u4); break;
    case kFamDilate: n = dilate_columns(c, u4, opt(0, f4), cs->channels, opt(1, i4), opt(2, u4)); break;
    case kFamFilter: n = filter_columns(c, d8, d8, f4, f4 + 1, cs->channels, u4); break;
    case kFamRayProbe: n = ray_columns(c, d8, d8); break;
    case kFamPointProbe: n = point_columns(c, d8, cs->num_dirs, rot, cs->num_rotations, d8, d8, opt(0, u4), opt(1, u8)); break;
    case kFamCastProbe: n = cast_probe_columns(c, d8, d8, opt(0, d8), u8, 56 /* sizeof(NraysCastResult) */); break;
    case kFamOccRaysProbe:
        point_columns(c, d8, cs->num_dirs, rot, cs->num_rotations, d8, d8, nullptr, opt(0, u8));
        n = occlusion_rays_columns(c, d8, d8, cs->num_dirs);
        break;
    default: return -1;
    }
    if (n < 0 || n > kStageMaxColumns) return -1;
    size_t o[kStageMaxColumns];
    *total = stage_layout(c, n, (size_t)cap, o);
    for (int k = 0; k < n; ++k) { off[k] = o[k]; bytes[k] = stage_column_bytes(c[k], (size_t)cap); align[k] = c[k].align; present[k] = stage_present(c[k]) ? 1u : 0u; }
    return n;
}

// 0 when the layout of the case is sound: every column starts at a multiple of its alignment, no two overlap, the last ends inside the total, and the total is at
// most the columns' bytes plus 15 bytes of padding a column.  Otherwise the number of the rule that broke (1 .. 4), or -1.
int batch_stage_check(const BatchStageCase* cs, uint64_t cap) {
    uint64_t off[kStageMaxColumns], bytes[kStageMaxColumns], total = 0, sum = 0; uint32_t align[kStageMaxColumns], present[kStageMaxColumns];
    const int n = batch_stage_table(cs, cap, off, bytes, align, present, &total);
    if (n < 0) return -1;
    for (int k = 0; k < n; ++k) {
        if (align[k] == 0u || off[k] % align[k]) return 1;
        for (int j = 0; j < n; ++j) if (j != k && bytes[j] && bytes[k] && off[j] < off[k] + bytes[k] && off[k] < off[j] + bytes[j]) return 2;
        if (off[k] + bytes[k] > total) return 3;
        sum += bytes[k];
    }
    return total > sum + 15u * (uint64_t)n ? 4 : 0;
}

// The whole sweep: every family, every subset of its optional arrays, cap in {1, 2, 3, 63, 64, 65, 4097}, num_dirs in {1, 16, 1024}, num_rotations in {0, 5, 1024},
// bands 0 .. 3, channels 1 .. 4, 1 and 16 maps of 1 x 1 and 3 x 5 texels.  Returns the number of unsound cases; *cases = the number swept.
uint64_t batch_stage_sweep(uint64_t* cases) {
    static const uint64_t caps[] = {1, 2, 3, 63, 64, 65, 4097};
    static const uint32_t dirs[] = {1, 16, 1024}, rots[] = {0, 5, 1024}, maps[] = {1, 16}, sides[][2] = {{1, 1}, {3, 5}};
    uint64_t bad = 0; *cases = 0;
    for (uint32_t fam = 0; fam < kFamCount; ++fam)
        for (uint32_t mask = 0; mask < (1u << batch_stage_optional(fam)); ++mask)
            for (uint64_t cap : caps)
                for (uint32_t nd : dirs) for (uint32_t nr : rots)
                    for (uint32_t bands = 0; bands <= 3; ++bands) for (uint32_t ch = 1; ch <= 4; ++ch)
                        for (uint32_t nm : maps) for (auto& wh : sides) {
                            const bool points = fam == kFamOcclusion || fam == kFamGather || fam == kFamGatherMaps || fam == kFamPointProbe || fam == kFamShFoldProbe || fam == kFamOccRaysProbe;
                            if (!points && (nd != 1 || nr != 0)) continue;                                  // (the parameter does not reach the family's table: once)
                            if (fam != kFamGather && fam != kFamShFoldProbe && bands != 0) continue;
                            if (fam == kFamShFoldProbe && bands == 0) continue;
                            if (fam != kFamDilate && fam != kFamFilter && ch != 1) continue;
                            if (fam != kFamGatherMaps && (nm != 1 || wh[0] != 1)) continue;
                            const BatchStageCase cs{fam, mask, nd, nr, bands, ch, nm, wh[0], wh[1], 7u};
                            ++*cases;
                            if (batch_stage_check(&cs, cap) != 0) ++bad;
                        }
    return bad;
}

} // extern "C"
