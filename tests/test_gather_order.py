"""The reorder inside the gather call (nrays_gather_points_device_ex / nrays_gather_points_ex with NRAYS_RAYS_UNORDERED, the probe nrays_debug_gather_order;
nrays_amd.gather_points(unordered=True), gather_order), the parts that need no GPU: the header, the ctypes table and the Rust declarations, the statuses without a
scene, and the Python wrappers' checks and forwarding.  What the path computes is tests/test_gather_order_gpu.py's."""
import ctypes as C
import math
import re
import subprocess

import numpy as np
import pytest

import nrays_amd as nr
from nrays_amd import abi
from tests.test_gather import FFI, GPU_RS, HEADER, HEADER_TEXT, RUST_TYPES, _c_params, _good, _NoDevice, no_library  # noqa: F401  (no_library: a fixture)

_IN = ["NraysScene*", "uint32_t", "const double*", "const double*", "const uint32_t*", "const uint64_t*", "const NraysGatherParams*"]
EXPECTED = {"nrays_gather_points_device_ex": _IN + ["float*", "uint32_t", "void*"], "nrays_gather_points_ex": _IN + ["float*", "uint32_t"],
            "nrays_debug_gather_order": _IN + ["uint64_t*", "uint32_t*", "double*", "uint32_t"]}  # (out_info[4]: an array parameter, read here as its element type)
RUST = dict(RUST_TYPES, **{"uint64_t*": "*mut u64", "uint32_t*": "*mut u32", "double*": "*mut f64"})
CTYPES = {"NraysScene*": (C.c_void_p,), "uint32_t": (C.c_uint32,), "void*": (C.c_void_p,), "const NraysGatherParams*": (C.POINTER(abi.NraysGatherParams),),
          "const double*": (C.c_void_p, C.POINTER(C.c_double)), "const uint32_t*": (C.c_void_p, C.POINTER(C.c_uint32)), "const uint64_t*": (C.c_void_p, C.POINTER(C.c_uint64)),
          "float*": (C.c_void_p, C.POINTER(C.c_float)), "uint64_t*": (C.POINTER(C.c_uint64),), "uint32_t*": (C.POINTER(C.c_uint32),), "double*": (C.POINTER(C.c_double),)}


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_header_ctypes_and_rust_declare_the_same_function(name):
    want = EXPECTED[name]
    got = _c_params(name)
    if name == "nrays_debug_gather_order":
        assert re.search(r"uint32_t out_info\[4\]\s*\)\s*;", HEADER[HEADER.index("int nrays_debug_gather_order"):])
        got = got[:-1] + [got[-1].replace("out_info[4]", "").strip() or "uint32_t"]
    assert got == want
    assert name in abi.HIP_SYMBOLS and name in abi.POST_V7_SYMBOLS
    res, args = abi.HIP_SYMBOLS[name]
    assert res is C.c_int and len(args) == len(want)
    for a, t in zip(args[:-1] if name == "nrays_debug_gather_order" else args, want):
        assert a in CTYPES[t], (name, t, a)
    if name == "nrays_debug_gather_order":
        assert args[-1] is C.POINTER(C.c_uint32)
    m = re.search(r"pub fn %s\((.*?)\) -> c_int;" % name, FFI)
    assert m, "%s is not declared in gpu_ffi.rs" % name
    rust = [p.split(": ", 1)[1] for p in m.group(1).split(", ")]
    assert rust[:-1] == [RUST[t] for t in want[:-1]]
    assert rust[-1] == ("*mut u32" if name == "nrays_debug_gather_order" else RUST[want[-1]])


def test_the_ex_forms_take_the_argument_lists_of_the_calls_they_extend():
    for name in ("nrays_gather_points_device", "nrays_gather_points"):
        assert _c_params(name + "_ex") == _c_params(name)
        assert abi.HIP_SYMBOLS[name + "_ex"] == abi.HIP_SYMBOLS[name]
    assert "pub fn gather_points_unordered(" in GPU_RS and "nrays_gather_points_ex(" in GPU_RS and "nrays_gather_points_device_ex(" in GPU_RS
    assert "pub fn gather_points(" in GPU_RS and "nrays_gather_points(" in GPU_RS  # (the unhinted wrapper still calls the entry point without _ex)


def test_the_abi_version_is_still_7_and_the_symbols_are_exported(built):
    assert re.search(r"#define NRAYS_ABI_VERSION 7\b", HEADER) and abi.ABI_VERSION == 7 and abi.load_hip_lib().nrays_abi_version() == 7
    note = re.search(r"Added after 7 WITHOUT a bump.*?\*/", HEADER_TEXT, re.S).group(0)
    exported = subprocess.check_output(["nm", "-D", "--defined-only", abi.HIP_LIB_PATH]).decode()
    for name in EXPECTED:
        assert re.search(r"%s\b" % name, note), name
        assert (" T " + name + "\n") in exported, name
        assert getattr(abi.load_hip_lib(), name).argtypes == abi.HIP_SYMBOLS[name][1]
    assert re.search(r"#define NRAYS_RAYS_UNORDERED 1u", HEADER) and abi.RAYS_UNORDERED == 1


def test_without_a_scene_every_call_is_a_bad_arg(built):
    lib = abi.load_hip_lib()
    a = (C.c_double * 3)(0.0, 0.0, 1.0)
    out = (C.c_float * 3)(7.0, 7.0, 7.0)
    keys, order, frame, info = (C.c_uint64 * 1)(5), (C.c_uint32 * 1)(6), (C.c_double * abi.RAY_FRAME_DOUBLES)(), (C.c_uint32 * 4)(9, 9, 9, 9)
    adr = C.addressof
    params = abi.NraysGatherParams(1, 0, adr(a), None, 1e-3, 1.0, 0)
    for n in (0, 1):
        for flags in (0, 1, 2, 3, 1 << 31):
            assert lib.nrays_gather_points_ex(None, n, a, a, None, None, C.byref(params), out, flags) == abi.ERR_BAD_ARG
            assert lib.nrays_gather_points_device_ex(None, n, adr(a), adr(a), None, None, C.byref(params), adr(out), flags, None) == abi.ERR_BAD_ARG
        assert lib.nrays_debug_gather_order(None, n, a, a, None, None, C.byref(params), keys, order, frame, info) == abi.ERR_BAD_ARG
    assert lib.nrays_last_error() and list(out) == [7.0] * 3 and keys[0] == 5 and order[0] == 6 and list(info) == [9] * 4


def test_wrappers_reject_bad_arguments_before_any_library_call(no_library):
    import torch
    sc = _NoDevice()
    t3 = torch.zeros((4, 3), dtype=torch.float64)
    bad = [dict(points=np.zeros((4, 2))), dict(normals=None), dict(sample_dirs=np.zeros((0, 3))), dict(rotations=np.zeros((1025, 2))), dict(bias=math.nan), dict(energy=math.inf),
           dict(max_depth=-1), dict(hit_flags=np.ones(3, np.uint32)), dict(keys=np.zeros(5, np.uint64)), dict(normals=t3), dict(points=t3, normals=t3)]
    for kw in bad:
        with pytest.raises(ValueError):
            nr.gather_points(sc, unordered=True, **dict(_good(), **kw))
    for hint in (1, 0, None, "yes"):  # a flag word is not the keyword's type
        with pytest.raises(ValueError, match="unordered"):
            nr.gather_points(sc, unordered=hint, **_good())
    with pytest.raises(AssertionError, match="library was loaded"):  # a well-formed hinted call gets as far as the library
        nr.gather_points(sc, unordered=True, **_good())
    for kw in (dict(points=np.zeros((4, 2))), dict(sample_dirs=None), dict(hit_flags=np.ones(3, np.uint32)), dict(keys=np.zeros(5, np.uint64)), dict(bias=math.inf),
               dict(points=t3, normals=t3)):
        with pytest.raises(ValueError):
            nr.gather_order(sc, **dict(_good(), **kw))
    with pytest.raises(ValueError, match="one chunk"):
        nr.gather_order(sc, np.zeros((1 << 20, 3)), np.zeros((1 << 20, 3)), nr.hemisphere_dirs(5))
    with pytest.raises(AssertionError, match="library was loaded"):
        nr.gather_order(sc, rotations=nr.rotation_table(3), hit_flags=np.ones(4, np.uint32), keys=np.arange(4), **_good())
    from nrays_amd import scenefile
    import inspect
    for fn in (nr.gather_points, nr.gather_hits, nr.bake_indirect, nr.Scene.gather_points, nr.Scene.bake_indirect, scenefile.FileScene.gather_points,
               scenefile.FileScene.bake_indirect):
        last = list(inspect.signature(fn).parameters.values())[-1]
        assert last.name == "unordered" and last.default is False, fn


def test_unordered_is_forwarded_by_gather_hits_and_bake_indirect(no_library, monkeypatch):
    sc = _NoDevice()
    seen = []
    monkeypatch.setattr(nr.scene, "gather_points", lambda scene, points, normals, *a, **kw: seen.append((a, kw)) or np.zeros((len(points), 3), np.float32))
    o, d = np.zeros((4, 3)), np.tile([0.0, 0.0, 1.0], (4, 1))
    hits = nr.CastHits(toi=np.ones(4), node=np.zeros(4, np.int32), normal=np.tile([0.0, 0.0, -1.0], (4, 1)), uv=None, prim=None, flags=np.ones(4, np.uint32))
    L = nr.hemisphere_dirs(4)
    nr.gather_hits(sc, o, d, hits, L, None, 0.25, 0.5, 3, keys=np.arange(4), unordered=True)
    nr.gather_hits(sc, o, d, hits, L)
    assert seen[0][1]["unordered"] is True and not seen[1][1].get("unordered", False)
    assert seen[0][0][1:] == (None, 0.25, 0.5, 3)
    tx = nr.SurfaceTexels(points=np.zeros((6, 3)), normals=np.tile([0.0, 1.0, 0.0], (6, 1)), uv=None, node=None, prim=None, flags=np.ones(6, np.uint32))
    monkeypatch.setattr(nr.scene, "surface_texels", lambda *a, **kw: tx)
    del seen[:]
    assert nr.bake_indirect(sc, 0, 3, 2, L, unordered=True).shape == (2, 3, 3)
    assert nr.bake_indirect(sc, 0, 3, 2, L).shape == (2, 3, 3)
    assert nr.Scene([], []).bake_indirect(0, 3, 2, L, None, 1e-3, 1.0, 0, False, False, None, None, True).shape == (2, 3, 3)
    assert [bool(kw.get("unordered", False)) for _, kw in seen] == [True, False, True]
    assert all(np.array_equal(kw["hit_flags"], tx.flags) for _, kw in seen)
