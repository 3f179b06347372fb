// The host compiler's build of the two column tables nrays_probe_depth_points* and nrays_irradiance_points_vis* add to nrays_amd/csrc/batch_stage.h
// (tests/test_probe_stage.py): each table exactly as the library fills it, and where stage_layout() puts its columns.  tests/batch_stage_shim.cpp holds the
// other families.
#include <cstdint>

#include "batch_stage.h"

using namespace nrays;

extern "C" {

enum { kFamProbeDepth, kFamIrradianceVis, kFamCount };

// mask: bit k = the family's k-th optional array is given.  probe_depth: hit_flags, keys, out_counts, out_nearest, out_nearest_dir.  irradiance_vis: grid valid,
// hit_flags, out_rgb, out_sh, out_weight.
struct ProbeStageCase { uint32_t family, mask, num_dirs, num_rotations, res, bands, probes; };

int probe_stage_optional(uint32_t family) { return family < kFamCount ? 5 : -1; }

// Per column its offset for chunks of `cap` items, bytes, alignment and whether the blocking form copies it; *total = the arena's bytes.  Returns the number of
// columns, or -1.
int probe_stage_table(const ProbeStageCase* cs, uint64_t cap, uint64_t* off, uint64_t* bytes, uint32_t* align, uint32_t* present, uint64_t* total) {
    static double d8[4]; static float f4[4]; static uint32_t u4[4]; static uint64_t u8[4]; // (never dereferenced: any non-null address)
    const uint32_t m = cs->mask;
    auto opt = [&](int bit, auto* p) -> decltype(p) { return (m >> bit) & 1u ? p : nullptr; };
    StageColumn c[kStageMaxColumns];
    int n = -1;
    switch (cs->family) {
    case kFamProbeDepth:
        point_columns(c, d8, cs->num_dirs, cs->num_rotations ? d8 : nullptr, cs->num_rotations, d8, d8, opt(0, u4), opt(1, u8));
        n = probe_depth_columns(c, f4, cs->res, opt(2, u4), opt(3, d8), opt(4, u4));
        break;
    case kFamIrradianceVis:
        irradiance_columns(c, f4, opt(0, u4), cs->probes, cs->bands * cs->bands, d8, d8, opt(1, u4), opt(2, f4), opt(3, f4), opt(4, f4));
        n = irradiance_vis_columns(c, f4, cs->probes, cs->res);
        break;
    default: return -1;
    }
    if (n < 0 || n > kStageMaxColumns) return -1;
    size_t o[kStageMaxColumns];
    *total = stage_layout(c, n, (size_t)cap, o);
    for (int k = 0; k < n; ++k) { off[k] = o[k]; bytes[k] = stage_column_bytes(c[k], (size_t)cap); align[k] = c[k].align; present[k] = stage_present(c[k]) ? 1u : 0u; }
    return n;
}

} // extern "C"
