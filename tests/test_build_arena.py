"""The three arenas of the device BLAS build (nrays_amd/csrc/bvh_arena.h), compiled by the host compiler (tests/build_arena_shim.cpp).  A carve function is the layout
of its phase: the builder runs it on a measuring arena for the bytes to reserve and again on the reserved one.  For triangle counts from 1 to the hairball's, 1 and 270
parts with upload arrays on both sides of the 1 MB staging limit, one walk on and off and the two debug caps: every piece starts 256-aligned, the pieces are disjoint and
in carve order, the last one ends inside the measured total, carving an arena of exactly that total hands out no null, and the total does not exceed what the builder
reserved when its sizes were hand-written sums (restated in the shim: former_bytes).  No GPU.  tests/build_arena_main.cpp runs the same sweep under the sanitizers."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_PIECES = 1024
NS = (1, 63, 64, 2000, 70000, 2880000)
UPLOADS = (24, (1 << 20) - 8, 1 << 20, (1 << 20) + 24)


class Case(C.Structure):
    _fields_ = [("n", C.c_uint64), ("nrefs", C.c_uint64), ("upload_bytes", C.c_uint64)] + [(n, C.c_uint32) for n in ("parts", "one_walk", "cap_div", "piece_cap", "nb")]


class ArenaShim:
    def __init__(self, directory):
        out = os.path.join(str(directory), "libbuild_arena_shim.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", os.path.join(ROOT, "nrays_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "build_arena_shim.cpp")])
        self.lib = C.CDLL(out)
        self.lib.build_arena_pieces.argtypes = [C.POINTER(Case), C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.c_int, C.POINTER(C.c_uint64)]
        self.lib.build_arena_former_bytes.restype = C.c_uint64
        self.lib.build_arena_former_bytes.argtypes = [C.POINTER(Case), C.c_int]
        self.lib.build_arena_check.argtypes = [C.POINTER(Case), C.c_int]
        self.lib.build_arena_sweep.restype = C.c_uint64
        self.lib.build_arena_sweep.argtypes = [C.POINTER(C.c_uint64)]

    def pieces(self, case, phase):
        """[(offset, bytes, null)] of the phase's pieces in carve order, the measured total and the former reservation."""
        at, size, null = (C.c_uint64 * MAX_PIECES)(), (C.c_uint64 * MAX_PIECES)(), (C.c_uint32 * MAX_PIECES)()
        total = C.c_uint64()
        n = self.lib.build_arena_pieces(C.byref(case), phase, at, size, null, MAX_PIECES, C.byref(total))
        assert 0 < n <= MAX_PIECES
        return [(at[k], size[k], null[k]) for k in range(n)], total.value, self.lib.build_arena_former_bytes(C.byref(case), phase)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return ArenaShim(tmp_path_factory.mktemp("build_arena_shim"))


def _case(n, nrefs, upload, parts, one_walk, cap_div, piece_cap):
    return Case(n, nrefs, upload, parts, one_walk, cap_div, piece_cap, max(nrefs - 1, 1))


@pytest.mark.parametrize("n", NS)
def test_every_layout_is_aligned_ordered_inside_its_total_and_no_larger_than_before(shim, n):
    swept = 0
    for parts, upload, one_walk, cap_div, piece_cap, nrefs in itertools.product((1, 270), UPLOADS, (1, 0), (1, 64), (0, 8), (n, 9 * n)):
        case = _case(n, nrefs, upload, parts, one_walk, cap_div, piece_cap)
        for phase in (1, 2, 3):
            what = (n, parts, upload, one_walk, cap_div, piece_cap, nrefs, phase)
            pieces, total, former = shim.pieces(case, phase)
            end = 0
            for k, (at, size, null) in enumerate(pieces):
                assert not null, (what, k, "a null piece from an arena of the measured size")
                assert at % 256 == 0, (what, k, "starts off its alignment")
                assert at >= end, (what, k, "overlaps the piece before it")
                end = at + size
            assert end <= total, (what, "the last piece ends beyond the total")
            assert total <= former, (what, "reserves more than the hand-written sum did")
            swept += 1
    assert swept == 2 * 4 * 2 * 2 * 2 * 2 * 3


def test_the_pieces_are_what_the_builder_carves(shim):
    """By hand from bvh_device.hip: the uploads first (three arrays a part) and consecutive; 13 more pieces in phase 1 (12 named buffers and the tail), 4 on top for the
    piece list of one walk; 20 pieces in phase 2, whose lists shrink with the debug divisor; the 4-wide nodes and the tail in phase 3."""
    pieces, _, _ = shim.pieces(_case(2000, 2000, 24, 270, 1, 1, 0), 1)
    assert len(pieces) == 3 * 270 + 13 + 4
    assert all(b[0] == (a[0] + a[1] + 255) // 256 * 256 for a, b in zip(pieces[:3 * 270 - 1], pieces[1:3 * 270]))
    assert len(shim.pieces(_case(2000, 2000, 24, 270, 0, 1, 0), 1)[0]) == 3 * 270 + 13
    assert len(shim.pieces(_case(63, 63, 24, 1, 1, 1, 0), 1)[0]) == 3 + 13  # (fewer than 64 triangles are never pre-split: no piece list)
    assert shim.pieces(_case(2000, 2000, 24, 1, 1, 1, 8), 1)[0][3 + 12][1] == 6 * 4 * 8 * 8  # 8 places in each of the 8 regions, 6 floats a piece
    full, _, _ = shim.pieces(_case(70000, 70000, 24, 1, 1, 1, 0), 2)
    tight, _, _ = shim.pieces(_case(70000, 70000, 24, 1, 1, 64, 0), 2)
    assert len(full) == len(tight) == 20 and full[0][1] == 70000 * 24 and full[4][1] == 70000 * 56
    assert full[5][1] == (70000 // 257 + 2) * 64 and tight[5][1] == (70000 // 257 // 64 + 2) * 64
    assert [p[1] for p in shim.pieces(_case(70000, 70000, 24, 1, 1, 1, 0), 3)[0]] == [69999 * 128, 4096]


def test_the_compiled_sweep_agrees(shim):
    """The same sweep in the shim itself (what tests/build_arena_main.cpp runs under the sanitizers), and its checker is not vacuous."""
    cases = C.c_uint64()
    assert shim.lib.build_arena_sweep(C.byref(cases)) == 0 and cases.value == len(NS) * 2 * 4 * 2 * 2 * 2 * 2 * 3
    assert shim.lib.build_arena_check(C.byref(Case(2000, 2000, 1 << 47, 1, 1, 1, 0, 1999)), 1) == -1  # (no such range can be reserved)
