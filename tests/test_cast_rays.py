"""Closest-hit queries on caller-supplied rays (nrays_cast_rays_device / nrays_cast_rays), the parts that need no GPU: the header, the ctypes
table and the Rust declarations agree on the two entry points, and nrays_amd.closest_hits checks its arguments before it touches the library."""
import os
import re

import numpy as np
import pytest

import nrays_amd as nr
from nrays_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nrays_abi.h")).read(), flags=re.S)
FFI = open(os.path.join(ROOT, "integration", "rust", "src", "gpu_ffi.rs")).read()
GPU_RS = open(os.path.join(ROOT, "integration", "rust", "src", "gpu.rs")).read()
# name -> the C parameter types the issue states, in order
EXPECTED = {
    "nrays_cast_rays_device": ["NraysScene*", "uint32_t", "const double*", "const double*", "const double*", "double*", "int32_t*", "double*", "double*", "int32_t*",
                               "uint32_t*", "uint32_t", "void*"],
    "nrays_cast_rays": ["NraysScene*", "uint32_t", "const double*", "const double*", "const double*", "double*", "int32_t*", "double*", "double*", "int32_t*", "uint32_t*",
                        "uint32_t"],
}
RUST_TYPES = {"NraysScene*": "*mut NraysScene", "uint32_t": "u32", "const double*": "*const f64", "double*": "*mut f64", "int32_t*": "*mut i32", "uint32_t*": "*mut u32",
              "void*": "*mut c_void"}


def _c_params(name):
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, HEADER, re.S)
    assert m, "%s is not declared in include/nrays_abi.h" % name
    out = []
    for p in m.group(1).split(","):
        t = re.sub(r"\s+", " ", p.strip())
        t = re.sub(r"\s*\w+$", "", t) if not t.endswith("*") else t  # drop the parameter's name
        out.append(re.sub(r"\s*\*\s*", "*", t))
    return out


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_header_ctypes_and_rust_declare_the_same_function(name):
    assert _c_params(name) == EXPECTED[name]
    assert name in abi.HIP_SYMBOLS and name in abi.POST_V7_SYMBOLS
    res, args = abi.HIP_SYMBOLS[name]
    assert res is abi.C.c_int and len(args) == len(EXPECTED[name])
    assert args[1] is abi.C.c_uint32 and args[11] is abi.C.c_uint32
    m = re.search(r"pub fn %s\((.*?)\) -> c_int;" % name, FFI)
    assert m, "%s is not declared in gpu_ffi.rs" % name
    assert [p.split(": ", 1)[1] for p in m.group(1).split(", ")] == [RUST_TYPES[t] for t in EXPECTED[name]]
    assert "%s(" % name in GPU_RS and "pub fn cast_rays(" in GPU_RS


def test_the_abi_version_did_not_move():
    assert re.search(r"#define NRAYS_ABI_VERSION 7\b", HEADER) and abi.ABI_VERSION == 7
    note = re.search(r"Added after 7 WITHOUT a bump.*?\*/", open(os.path.join(ROOT, "include", "nrays_abi.h")).read(), re.S).group(0)
    assert "nrays_cast_rays_device" in note and re.search(r"nrays_cast_rays\b", note)


class _NoScene:
    def device_handle(self):
        raise AssertionError("the scene was touched before the arguments were checked")


@pytest.fixture()
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(abi, "load_hip_lib", refuse)


def test_closest_hits_rejects_bad_arguments_before_any_library_call(no_library):
    import torch
    sc = _NoScene()
    o, d = np.zeros((4, 3)), np.tile([0.0, 0.0, 1.0], (4, 1))
    bad = [
        dict(origins=np.zeros((4, 2)), dirs=d),                              # not (n, 3)
        dict(origins=np.zeros(12), dirs=d),                                  # flat
        dict(origins=o, dirs=d[:3]),                                         # different numbers of rays
        dict(origins=None, dirs=d),
        dict(origins=o, dirs=d, max_toi=np.zeros((4, 1))),                   # max_toi not (n,)
        dict(origins=o, dirs=d, max_toi=np.zeros(5)),
        dict(origins=o.astype(np.int64), dirs=d),                            # not floating point
        dict(origins=o, dirs=d, max_toi=np.zeros(4, np.int32)),
        dict(origins=o, dirs=d, want=("normal", "depth")),                   # unknown output
        dict(origins=o, dirs=torch.zeros((4, 3), dtype=torch.float64)),      # numpy and torch mixed
        dict(origins=torch.zeros((4, 3), dtype=torch.float64), dirs=torch.zeros((4, 3), dtype=torch.float64)),  # torch tensors on the host
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            nr.closest_hits(sc, **kw)
    with pytest.raises(ValueError):
        nr.Scene([], []).cast_rays(np.zeros((4, 2)), d)
    # a well-formed call gets as far as the library
    with pytest.raises(AssertionError, match="library was loaded"):
        nr.closest_hits(sc, o, d, max_toi=np.ones(4), want=("prim",))


def test_the_result_names_its_outputs():
    assert nr.CastHits._fields == ("toi", "node", "normal", "uv", "prim", "flags")
    assert nr.scene.CAST_OUTPUTS == ("normal", "uv", "prim", "flags")
