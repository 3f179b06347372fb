"""The staging arena of the blocking caller-batch calls (nrays_amd/csrc/batch_stage.h), compiled by the host compiler (tests/batch_stage_shim.cpp): for every
family's column table — every subset of its optional arrays, chunk capacities around a wave and an odd large one, the table sizes the parameters allow —
every column starts at a multiple of its alignment, no two columns overlap, the last one ends inside the reported total, and the total carries no more than
15 bytes of padding a column.  One function computes the offsets and the total (stage_layout), so a size cannot disagree with a layout; this pins that function
and the tables.  No GPU.  tests/batch_stage_main.cpp runs the same sweep as a stand-alone program for the sanitizers."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_COLUMNS = 32
FAMILIES = ("trace", "intersects", "cast", "shade", "occlusion", "gather", "gather_maps", "surface_texels", "dilate", "filter", "ray_probe", "point_probe", "sh_fold_probe", "cast_probe",
            "occlusion_rays_probe")
POINT_FAMILIES = ("occlusion", "gather", "gather_maps", "point_probe", "sh_fold_probe", "occlusion_rays_probe")
CAPS = (1, 2, 3, 63, 64, 65, 4097)


class Case(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("family", "mask", "num_dirs", "num_rotations", "bands", "channels", "num_maps", "map_w", "map_h", "num_nodes")]


class StageShim:
    def __init__(self, directory):
        out = os.path.join(str(directory), "libbatch_stage_shim.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "nrays_amd", "csrc"), "-o", out,
                               os.path.join(ROOT, "tests", "batch_stage_shim.cpp")])
        self.lib = C.CDLL(out)
        self.lib.batch_stage_optional.restype = C.c_int
        self.lib.batch_stage_optional.argtypes = [C.c_uint32]
        self.lib.batch_stage_table.restype = C.c_int
        self.lib.batch_stage_table.argtypes = [C.POINTER(Case), C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                               C.POINTER(C.c_uint64)]
        self.lib.batch_stage_check.restype = C.c_int
        self.lib.batch_stage_check.argtypes = [C.POINTER(Case), C.c_uint64]
        self.lib.batch_stage_sweep.restype = C.c_uint64
        self.lib.batch_stage_sweep.argtypes = [C.POINTER(C.c_uint64)]

    def optional(self, family):
        return self.lib.batch_stage_optional(FAMILIES.index(family))

    def table(self, cap, family, mask=0, num_dirs=1, num_rotations=0, bands=0, channels=1, num_maps=1, map_w=1, map_h=1, num_nodes=7):
        """[(offset, bytes, align, present)] of the family's columns for chunks of `cap` items, and the arena's bytes."""
        cs = Case(FAMILIES.index(family), mask, num_dirs, num_rotations, bands, channels, num_maps, map_w, map_h, num_nodes)
        off, size = (C.c_uint64 * MAX_COLUMNS)(), (C.c_uint64 * MAX_COLUMNS)()
        align, present = (C.c_uint32 * MAX_COLUMNS)(), (C.c_uint32 * MAX_COLUMNS)()
        total = C.c_uint64()
        n = self.lib.batch_stage_table(C.byref(cs), cap, off, size, align, present, C.byref(total))
        assert 0 < n <= MAX_COLUMNS
        return [(off[k], size[k], align[k], present[k]) for k in range(n)], total.value


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return StageShim(tmp_path_factory.mktemp("batch_stage_shim"))


def _assert_sound(cols, total, what):
    for k, (off, size, align, _) in enumerate(cols):
        assert align in (8, 16) and off % align == 0, (what, k, "starts off its alignment")
        assert off + size <= total, (what, k, "ends beyond the total")
    spans = sorted((off, off + size) for off, size, _, _ in cols if size)
    for (_, end), (start, _) in zip(spans, spans[1:]):
        assert end <= start, (what, "two columns overlap")
    assert total <= sum(size for _, size, _, _ in cols) + 15 * len(cols), (what, "more padding than alignment can need")


def _variants(family):
    """The table sizes that reach the family's columns."""
    kw = [{}]
    if family in POINT_FAMILIES:
        kw = [dict(num_dirs=d, num_rotations=r) for d in (1, 16, 1024) for r in (0, 5, 1024)]
    if family == "gather":
        kw = [dict(v, bands=b) for v in kw for b in (0, 1, 2, 3)]
    if family == "sh_fold_probe":
        kw = [dict(v, bands=b) for v in kw for b in (1, 2, 3)]
    if family == "gather_maps":
        kw = [dict(v, num_maps=m, map_w=w, map_h=h) for v in kw for m in (1, 16) for (w, h) in ((1, 1), (3, 5))]
    if family in ("dilate", "filter"):
        kw = [dict(channels=c) for c in (1, 2, 3, 4)]
    return kw


@pytest.mark.parametrize("family", FAMILIES)
def test_every_layout_is_aligned_disjoint_and_inside_its_total(shim, family):
    swept = 0
    for mask, cap, kw in itertools.product(range(1 << shim.optional(family)), CAPS, _variants(family)):
        cols, total = shim.table(cap, family, mask=mask, **kw)
        _assert_sound(cols, total, (family, mask, cap, kw))
        swept += 1
    assert swept >= len(CAPS)


@pytest.mark.parametrize("family", FAMILIES)
def test_an_absent_array_is_not_copied_and_moves_nothing(shim, family):
    """The layout depends on the sizes alone: a missing optional array only switches its copies off."""
    bits = shim.optional(family)
    full, total = shim.table(65, family, mask=(1 << bits) - 1, num_rotations=5, bands=2 if family == "sh_fold_probe" else 0)
    for mask in range(1 << bits):
        cols, t = shim.table(65, family, mask=mask, num_rotations=5, bands=2 if family == "sh_fold_probe" else 0)
        if family != "dilate":  # (its value array has no width when it is absent)
            assert [c[:3] for c in cols] == [c[:3] for c in full] and t == total
        assert sum(1 for c in full if c[3]) - sum(1 for c in cols if c[3]) == bits - bin(mask).count("1")


def test_the_tables_are_what_the_calls_stage(shim):
    """Bytes an item, by hand from include/nrays_abi.h: a cast ray 24 + 24 + 8 in and 8 + 4 + 24 + 16 + 4 + 4 out; a gather_sh point of 3 bands 27 floats out; the value
    arrays of the texel calls on 16-byte boundaries; a record of the cast probe 56 bytes (NraysCastResult); the rays of the occlusion probe 24 bytes a direction, twice."""
    cols, _ = shim.table(3, "cast", mask=31)
    assert [c[1] // 3 for c in cols] == [24, 24, 8, 8, 4, 24, 16, 4, 4]
    cols, _ = shim.table(1, "gather", mask=3, num_dirs=16, num_rotations=5, bands=3)
    assert [c[1] for c in cols] == [16 * 24, 5 * 16, 24, 24, 4, 8, 27 * 4, 0]
    cols, _ = shim.table(1, "gather_maps", mask=7, num_dirs=1, num_maps=16, map_w=3, map_h=5)
    assert len(cols) == 9 + 16 and all(c[1:3] == (15 * 16, 16) for c in cols[9:]) and cols[8][1] == 7 * 4
    cols, _ = shim.table(3, "cast_probe", mask=1)
    assert [c[1] // 3 for c in cols] == [24, 24, 8, 56]
    cols, _ = shim.table(1, "occlusion_rays_probe", mask=1, num_dirs=16, num_rotations=5)
    assert [c[1] for c in cols] == [16 * 24, 5 * 16, 24, 24, 4, 8, 16 * 24, 16 * 24] and not cols[4][3]  # (the probe has no hit flags)
    for family, value_columns in (("dilate", (1,)), ("filter", (2, 3))):
        cols, _ = shim.table(63, family, mask=7 if family == "dilate" else 0, channels=3)
        assert all(cols[k][2] == 16 and cols[k][1] == 63 * 12 for k in value_columns)


def test_the_compiled_sweep_agrees(shim):
    """The same sweep in the shim itself (what tests/batch_stage_main.cpp runs under the sanitizers), and its checker is not vacuous."""
    cases = C.c_uint64()
    assert shim.lib.batch_stage_sweep(C.byref(cases)) == 0 and cases.value >= 5000
    assert shim.lib.batch_stage_check(C.byref(Case(99, 0, 1, 0, 0, 1, 1, 1, 1, 7)), 1) == -1  # (no such family)
