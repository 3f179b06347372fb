"""build_host_scene() (nrays_amd/csrc/scene_build.cpp) on the host compiler, without a device: tests/host_scene_shim.cpp flattens the smallest descriptors that reach each
branch of the builder — empty, every analytic shape, an untransformed quad, merged / opaque-shadow / per-node shadow BLASes, a mesh without triangles, a hair-like mesh
that is pre-split, an area light, a rotated group, device-built BLASes (a deterministic fake) in front of host-built ones, and the refusals — and reports each HostScene
member's length and FNV-1a digest plus the scalars.  They are compared with tests/golden/host_scene_digests.json, recorded from the builder before it was split into
phases (`python tests/test_host_scene.py --record` rewrites the file).  Rotated cases go through libm's sin / cos: the golden file holds the bit patterns of the half-angle
values it was recorded with, and only where this machine's differ are the rotated cases skipped.  No GPU.  tests/host_scene_main.cpp runs the cases under the sanitizers.

What the digests do NOT prove: that the recorded scene is a correct one.  They pin the builder to itself — a box one ulp too tight, or a node missing from the shadow side
of a grouping no case here has, is recorded and then defended.  Whether both TLASes hold and cover every node of a scene is tests/scene_cover.py's question, asked of a
dump and the scene description without any code of the builder's (tests/test_scene_cover.py here, tests/test_scene_cover_gpu.py on the device's arrays)."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "host_scene_digests.json")
CASES = ("empty", "analytic", "quad", "three_meshes", "no_triangles", "hair", "two_lights", "three_meshes_rotated", "mixed_device",
         "bad_index", "bad_vertex", "bad_uv", "bad_material_id", "bad_mesh_id", "bad_texture_id", "null_array")
ROTATED = ("analytic", "three_meshes_rotated", "mixed_device")
REFUSALS = {"bad_index": (-1, "triangle index out of range"),
            "bad_vertex": (-4, "mesh vertex coordinate is not exactly representable in f32 (see DESIGN.md: f32-exact mesh storage)"),
            "bad_uv": (-4, "mesh uv is not exactly representable in f32"), "bad_material_id": (-1, "bad material id"), "bad_mesh_id": (-1, "bad mesh id"),
            "bad_texture_id": (-1, "bad texture id"), "null_array": (-1, "null array with non-zero count")}


class SceneShim:
    def __init__(self, directory):
        out = os.path.join(str(directory), "libhost_scene_shim.so")
        csrc = os.path.join(ROOT, "nrays_amd", "csrc")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", csrc, "-fPIC", "-shared", "-pthread", "-o", out,
                               os.path.join(ROOT, "tests", "host_scene_shim.cpp")] + [os.path.join(csrc, f) for f in ("scene_build.cpp", "bvh_build.cpp", "switches.cpp")])
        self.lib = C.CDLL(out)
        self.lib.host_scene_case_name.restype = C.c_char_p
        self.lib.host_scene_report.argtypes = [C.c_int, C.c_char_p, C.c_size_t]
        assert tuple(self.lib.host_scene_case_name(c).decode() for c in range(self.lib.host_scene_cases())) == CASES

    def report(self, case):
        buf = C.create_string_buffer(8192)
        assert self.lib.host_scene_report(CASES.index(case), buf, len(buf)) > 0
        return json.loads(buf.value.decode())

    def trig_bits(self):
        out = (C.c_uint64 * 4)()
        assert self.lib.host_scene_trig_bits(out) == 4
        return ["%016x" % v for v in out]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return SceneShim(tmp_path_factory.mktemp("host_scene_shim"))


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("case", CASES)
def test_the_flattened_scene_is_the_recorded_one(shim, golden, case):
    if case in ROTATED and shim.trig_bits() != golden["trig_bits"]:
        pytest.skip("this machine's libm gives other sin / cos bits for the half angles than the one the goldens were recorded on")
    got = shim.report(case)
    assert got == golden["cases"][case]
    assert got == shim.report(case), "two runs differ"
    if case in REFUSALS:
        assert (got["status"], got["err"]) == REFUSALS[case]
    else:
        assert got["status"] == 0 and got["err"] == ""


def test_the_cases_reach_their_branches(shim, golden):
    """What the recorded scalars say about the cases themselves, by hand: flags = reflective 1, transparent 2, area light 4, double branch 8, incoherent 16, mesh 32, bounded 64."""
    g = golden["cases"]
    assert g["empty"]["features"] == 1 | 16 and g["empty"]["nodes"][0] == 0
    assert g["analytic"]["features"] == 15 and g["analytic"]["planes"][0] == 1 and g["analytic"]["flags"] == 1 | 2 | 8
    assert g["quad"]["nodes"][0] == 0 and g["quad"]["tris"][0] == 2 and g["quad"]["features"] == 2
    for name in ("three_meshes", "three_meshes_rotated"):  # closest: one merged BLAS; shadow: the two opaque meshes in one BLAS and the cut-out mesh in its own
        assert g[name]["instances"][0] == 1 and g[name]["shadow_instances"][0] == 2 and g[name]["tris"][0] == 19 + 16 + 3 and g[name]["features"] == 2 | 4
    assert g["no_triangles"]["instances"][0] == 0 and g["no_triangles"]["tris"][0] == 0
    assert g["hair"]["flags"] & 16 and g["hair"]["tris"][0] > 70
    assert g["two_lights"]["flags"] & 4 and g["two_lights"]["features"] & 16 and g["two_lights"]["lights"][0] == 2
    m = g["mixed_device"]
    assert m["device_builds"][0] == 2 and m["dev_tris"] == 6 + 8 and m["dev_nodes"] == 1 + 2 and m["tris"][0] == 2 and m["instances"][0] == 4


if __name__ == "__main__" and "--record" in sys.argv:
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        s = SceneShim(tmp)
        with open(GOLDEN, "w") as f:
            json.dump({"trig_bits": s.trig_bits(), "cases": {c: s.report(c) for c in CASES}}, f, indent=1, sort_keys=True)
            f.write("\n")
