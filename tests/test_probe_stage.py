"""The column tables of nrays_probe_depth_points* and nrays_irradiance_points_vis* in the staging arena (nrays_amd/csrc/batch_stage.h), compiled by the host
compiler (tests/probe_stage_shim.cpp), under the four layout properties tests/test_batch_stage.py checks for the other families: every column starts at a
multiple of its alignment, no two columns overlap, the last one ends inside the reported total, and the total carries no more than 15 bytes of padding a
column — for every subset of the optional arrays, chunk capacities around a wave and an odd large one, and the table sizes the parameters allow.  No GPU."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_COLUMNS = 32
FAMILIES = ("probe_depth", "irradiance_vis")
CAPS = (1, 2, 3, 63, 64, 65, 4097)
RES = (4, 8, 16)


class Case(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("family", "mask", "num_dirs", "num_rotations", "res", "bands", "probes")]


class ProbeShim:
    def __init__(self, directory):
        out = os.path.join(str(directory), "libprobe_stage_shim.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-I", os.path.join(ROOT, "nrays_amd", "csrc"), "-o", out,
                               os.path.join(ROOT, "tests", "probe_stage_shim.cpp")])
        self.lib = C.CDLL(out)
        self.lib.probe_stage_optional.restype = C.c_int
        self.lib.probe_stage_optional.argtypes = [C.c_uint32]
        self.lib.probe_stage_table.restype = C.c_int
        self.lib.probe_stage_table.argtypes = [C.POINTER(Case), C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                               C.POINTER(C.c_uint64)]

    def optional(self, family):
        return self.lib.probe_stage_optional(FAMILIES.index(family))

    def table(self, cap, family, mask=0, num_dirs=1, num_rotations=0, res=8, bands=3, probes=1):
        """[(offset, bytes, align, present)] of the family's columns for chunks of `cap` items, and the arena's bytes."""
        cs = Case(FAMILIES.index(family), mask, num_dirs, num_rotations, res, bands, probes)
        off, size = (C.c_uint64 * MAX_COLUMNS)(), (C.c_uint64 * MAX_COLUMNS)()
        align, present = (C.c_uint32 * MAX_COLUMNS)(), (C.c_uint32 * MAX_COLUMNS)()
        total = C.c_uint64()
        n = self.lib.probe_stage_table(C.byref(cs), cap, off, size, align, present, C.byref(total))
        assert 0 < n <= MAX_COLUMNS
        return [(off[k], size[k], align[k], present[k]) for k in range(n)], total.value


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return ProbeShim(tmp_path_factory.mktemp("probe_stage_shim"))


def _assert_sound(cols, total, what):
    for k, (off, size, align, _) in enumerate(cols):
        assert align in (8, 16) and off % align == 0, (what, k, "starts off its alignment")
        assert off + size <= total, (what, k, "ends beyond the total")
    spans = sorted((off, off + size) for off, size, _, _ in cols if size)
    for (_, end), (start, _) in zip(spans, spans[1:]):
        assert end <= start, (what, "two columns overlap")
    assert total <= sum(size for _, size, _, _ in cols) + 15 * len(cols), (what, "more padding than alignment can need")


def _variants(family):
    if family == "probe_depth":
        return [dict(num_dirs=d, num_rotations=r, res=R) for d in (1, 16, 1024) for r in (0, 5, 1024) for R in RES]
    return [dict(res=R, bands=b, probes=p) for R in RES for b in (1, 2, 3) for p in (1, 7, 4097)]


@pytest.mark.parametrize("family", FAMILIES)
def test_every_layout_is_aligned_disjoint_and_inside_its_total(shim, family):
    swept = 0
    for mask, cap, kw in itertools.product(range(1 << shim.optional(family)), CAPS, _variants(family)):
        cols, total = shim.table(cap, family, mask=mask, **kw)
        _assert_sound(cols, total, (family, mask, cap, kw))
        swept += 1
    assert swept >= 32 * len(CAPS) * 9


@pytest.mark.parametrize("family", FAMILIES)
def test_an_absent_array_is_not_copied_and_moves_nothing(shim, family):
    """The layout depends on the sizes alone: a missing optional array only switches its copies off."""
    bits = shim.optional(family)
    full, total = shim.table(65, family, mask=(1 << bits) - 1, num_rotations=5, probes=7)
    for mask in range(1 << bits):
        cols, t = shim.table(65, family, mask=mask, num_rotations=5, probes=7)
        assert [c[:3] for c in cols] == [c[:3] for c in full] and t == total
        assert sum(1 for c in full if c[3]) - sum(1 for c in cols if c[3]) == bits - bin(mask).count("1")


def test_the_tables_are_what_the_calls_stage(shim):
    """Bytes an item, by hand from include/nrays_abi.h: a probe_depth point 24 + 24 + 4 + 8 in and 8 R^2 + 8 + 8 + 4 out behind the two tables; the visibility call is
    the irradiance call (grid 12 C and 4 bytes a probe, 24 + 24 + 4 in, 12 + 12 C + 4 out a point) plus 8 R^2 bytes a probe, a table like the grid's."""
    for R in RES:
        cols, _ = shim.table(3, "probe_depth", mask=31, num_dirs=16, num_rotations=5, res=R)
        assert [c[1] for c in cols] == [16 * 24, 5 * 16, 72, 72, 12, 24, 3 * 8 * R * R, 24, 24, 12]
        cols, _ = shim.table(3, "irradiance_vis", mask=31, res=R, bands=3, probes=7)
        assert [c[1] for c in cols] == [7 * 108, 7 * 4, 72, 72, 12, 36, 3 * 108, 12, 7 * 8 * R * R]
        wider, _ = shim.table(4097, "irradiance_vis", mask=31, res=R, bands=3, probes=7)
        assert [wider[k][1] for k in (0, 1, 8)] == [cols[k][1] for k in (0, 1, 8)]  # (tables: a call's, not a chunk's)
    assert shim.lib.probe_stage_table(C.byref(Case(9, 0, 1, 0, 8, 3, 1)), 1, None, None, None, None, None) == -1  # (no such family)
