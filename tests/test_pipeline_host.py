"""nrays_debug_pipeline_counts and the NRAYS_PIPELINE_HOST table entry, without a GPU (tests/test_pipeline_host_gpu.py runs them)."""
import ctypes as C
import os
import re

from nrays_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    with open(os.path.join(ROOT, *parts), encoding="utf-8") as f:
        return f.read()


def test_the_probe_refuses_null_arguments(built):
    lib = abi.load_hip_lib()
    assert lib.nrays_debug_pipeline_counts(None, None) == abi.ERR_BAD_ARG
    assert lib.nrays_debug_pipeline_counts(None, (C.c_uint64 * 4)()) == abi.ERR_BAD_ARG


def test_the_probe_came_without_an_abi_bump():
    assert "nrays_debug_pipeline_counts" in abi.HIP_SYMBOLS and "nrays_debug_pipeline_counts" in abi.POST_V7_SYMBOLS
    assert re.search(r"\bint nrays_debug_pipeline_counts\(const NraysScene\* scene, uint64_t out\[4\]\);", _read("include", "nrays_abi.h"))


def test_the_proof_window_is_half_the_measured_gap():
    """switches.h states the measured gap of a synchronising caller beside the constant that is half of it."""
    text = _read("nrays_amd", "csrc", "switches.h")
    gap = float(re.search(r"synchronises after every frame produced: ([0-9.]+) us", text).group(1))
    tau = float(re.search(r"constexpr double kInFlightProofUs = ([0-9.]+);", text).group(1))
    assert tau == gap / 2.0
