"""Probes filled from baked maps with their depth from the same rays (nrays_gather_maps_sh_points_device / nrays_gather_maps_sh_points; nrays_amd.gather_maps_sh_points,
gather_maps_probes, bake_probe_grid_maps), the parts that need no GPU: the header, the ctypes table and the Rust declarations, NraysGatherDepthSpec's layout against the
C compiler's, what the three wrappers hand to the library (against the recording stand-in of tools/call_transcript.py), their argument checks, and the composition
the GPU tests restate the call with — sh_fold_ref of the contributions of tests/test_gather_maps.py — on synthetic per-ray records."""
import ctypes as C
import inspect
import math
import os
import re
import subprocess

import numpy as np
import pytest

import nrays_amd as nr
from nrays_amd import abi
from tests.test_gather import FFI, GPU_RS, HEADER, HEADER_TEXT, _NoDevice, _c_params, no_library  # noqa: F401  (no_library is a fixture)
from tests.test_gather_maps import BILINEAR_CLAMP, DARK, MAPPED, MISSED, contributions, fold_classes, random_map
from tests.test_occlusion_gpu import bits
from tools import call_transcript as ct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_IN = ["NraysScene*", "uint32_t", "const double*", "const double*", "const uint32_t*", "const uint64_t*", "const NraysGatherMapsParams*", "uint32_t", "float*", "uint32_t*",
       "const NraysGatherDepthSpec*", "float*", "uint32_t*", "double*", "uint32_t*", "uint32_t"]
EXPECTED = {"nrays_gather_maps_sh_points_device": _IN + ["void*"], "nrays_gather_maps_sh_points": _IN}
RUST_TYPES = {"NraysScene*": "*mut NraysScene", "uint32_t": "u32", "const double*": "*const f64", "const uint32_t*": "*const u32", "const uint64_t*": "*const u64",
              "const NraysGatherMapsParams*": "*const NraysGatherMapsParams", "const NraysGatherDepthSpec*": "*const NraysGatherDepthSpec", "float*": "*mut f32",
              "uint32_t*": "*mut u32", "double*": "*mut f64", "void*": "*mut c_void"}
STRUCT_FIELDS = [("max_dist", "double", "f64", C.c_double), ("near_dist", "double", "f64", C.c_double), ("res", "uint32_t", "u32", C.c_uint32),
                 ("reserved", "uint32_t", "u32", C.c_uint32)]
WANT_ALL = ("counts", "depth_counts", "nearest", "nearest_dir")


# ---- the surface --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_header_ctypes_and_rust_declare_the_same_function(name):
    assert _c_params(name) == EXPECTED[name]
    assert name in abi.HIP_SYMBOLS and name in abi.POST_V7_SYMBOLS
    res, args = abi.HIP_SYMBOLS[name]
    assert res is C.c_int and len(args) == len(EXPECTED[name]) and args[1] is C.c_uint32 and args[7] is C.c_uint32
    assert args[EXPECTED[name].index("const NraysGatherMapsParams*")] is C.POINTER(abi.NraysGatherMapsParams)
    assert args[EXPECTED[name].index("const NraysGatherDepthSpec*")] is C.POINTER(abi.NraysGatherDepthSpec)
    m = re.search(r"pub fn %s\((.*?)\) -> c_int;" % name, FFI)
    assert m, "%s is not declared in gpu_ffi.rs" % name
    assert [p.split(": ", 1)[1] for p in m.group(1).split(", ")] == [RUST_TYPES[t] for t in EXPECTED[name]]
    assert "pub fn gather_maps_sh_points(" in GPU_RS and "pub unsafe fn gather_maps_sh_points_device(" in GPU_RS
    assert "nrays_gather_maps_sh_points(" in GPU_RS and "nrays_gather_maps_sh_points_device(" in GPU_RS
    note = re.search(r"Added after 7 WITHOUT a bump.*?\*/", HEADER_TEXT, re.S).group(0)
    assert re.search(r"%s\b" % name, note)
    assert re.search(r"#define NRAYS_ABI_VERSION 7\b", HEADER) and abi.ABI_VERSION == 7


def test_the_depth_spec_is_the_same_in_the_header_ctypes_rust_and_the_c_compiler(tmp_path):
    m = re.search(r"struct NraysGatherDepthSpec \{(.*?)\};\s*typedef struct NraysGatherDepthSpec NraysGatherDepthSpec;", HEADER, re.S)
    assert m, "struct NraysGatherDepthSpec is not declared in include/nrays_abi.h (struct plus separate typedef)"
    c_fields = [re.sub(r"\s*\*\s*", "* ", f.strip()).rsplit(" ", 1) for f in m.group(1).split(";") if f.strip()]
    assert [(n, t) for t, n in c_fields] == [(n, t) for n, t, _, _ in STRUCT_FIELDS]
    r = re.search(r"#\[repr\(C\)\]\s*(?:#\[derive[^\]]*\]\s*)?pub struct NraysGatherDepthSpec \{(.*?)\n\}", FFI, re.S)
    assert r and re.findall(r"pub (\w+): ([^,]+),", r.group(1)) == [(n, t) for n, _, t, _ in STRUCT_FIELDS]
    assert [(n, t) for n, t in abi.NraysGatherDepthSpec._fields_] == [(n, t) for n, _, _, t in STRUCT_FIELDS]
    src = tmp_path / "layout.c"  # the layout, from the C compiler itself
    names = [n for n, _, _, _ in STRUCT_FIELDS]
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "nrays_abi.h"\nint main(void) {\n    printf("%zu", sizeof(NraysGatherDepthSpec));\n'
                   + "".join('    printf(" %%zu", offsetof(NraysGatherDepthSpec, %s));\n' % n for n in names) + '    printf("\\n");\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [C.sizeof(abi.NraysGatherDepthSpec)] + [getattr(abi.NraysGatherDepthSpec, n).offset for n in names]
    assert got == [24, 0, 8, 16, 20]


def test_the_symbols_are_exported_and_without_a_scene_every_call_is_a_bad_arg(built):
    lib = abi.load_hip_lib()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", abi.HIP_LIB_PATH]).decode()
    for name in EXPECTED:
        assert (" T " + name + "\n") in exported, name
        assert getattr(lib, name).argtypes == abi.HIP_SYMBOLS[name][1]
    assert lib.nrays_abi_version() == 7
    a = (C.c_double * 3)(0.0, 0.0, 1.0)
    sh, cnt, mo = (C.c_float * 3)(7.0, 7.0, 7.0), (C.c_uint32 * 2)(7, 7), (C.c_float * 32)(*([7.0] * 32))
    texels = (C.c_float * 4)(1.0, 1.0, 1.0, 1.0)
    rec = abi.NraysTexture(1, 1, abi.TEXEL_RGBA32F, abi.INTERP_BILINEAR, abi.OVERFLOW_CLAMP, 0, C.addressof(texels))
    nodes = (C.c_int32 * 1)(0)
    params = abi.NraysGatherMapsParams(1, 0, C.addressof(a), None, 0.0, math.inf, 1, 1, C.pointer(rec), C.addressof(nodes), (C.c_float * 3)(0, 0, 0))
    spec = abi.NraysGatherDepthSpec(1.0, 0.0, 4, 0)
    adr = C.addressof
    for n in (0, 1):
        assert lib.nrays_gather_maps_sh_points(None, n, a, a, None, None, C.byref(params), 1, sh, cnt, C.byref(spec), mo, None, None, None, 0) == abi.ERR_BAD_ARG
        assert lib.nrays_gather_maps_sh_points_device(None, n, adr(a), adr(a), None, None, C.byref(params), 1, adr(sh), adr(cnt), None, None, None, None, None, 0, None) == abi.ERR_BAD_ARG
    assert lib.nrays_last_error() and list(sh) == [7.0] * 3 and list(cnt) == [7, 7] and list(mo) == [7.0] * 32


def test_the_python_names_exist_and_the_methods_forward():
    assert nr.GatherMapsSh._fields == ("sh", "counts", "depth")
    sig = inspect.signature(nr.gather_maps_sh_points).parameters
    assert list(sig) == ["scene", "points", "normals", "sample_dirs", "maps", "node_map", "bands", "rotations", "bias", "max_toi", "miss", "hit_flags", "keys", "depth", "want"]
    assert sig["bands"].default == 3 and sig["bias"].default == 1e-3 and sig["max_toi"].default == math.inf and sig["depth"].default is None and sig["miss"].default == (0.0, 0.0, 0.0)
    assert list(inspect.signature(nr.gather_maps_probes).parameters)[:5] == ["scene", "positions", "sample_dirs", "maps", "node_map"]
    sig = inspect.signature(nr.bake_probe_grid_maps).parameters
    assert list(sig) == ["scene", "origin", "cell", "counts", "sample_dirs", "maps", "node_map", "bands", "miss", "visibility", "measure", "device"]
    assert sig["visibility"].default is None and sig["measure"].default == 4.0 * math.pi and sig["device"].default is None
    from nrays_amd import scenefile
    for cls in (nr.Scene, scenefile.FileScene):
        for name in ("gather_maps_sh_points", "gather_maps_probes", "bake_probe_grid_maps"):
            a, b = inspect.signature(getattr(cls, name)).parameters, inspect.signature(getattr(nr, name)).parameters
            assert list(a)[1:] == list(b)[1:] and [p.default for p in a.values()][1:] == [p.default for p in b.values()][1:], name


# ---- what the wrappers hand to the library: the recording stand-in -------------------------------------------------------------------------------------------
def _inputs(n=4):
    rng = np.random.RandomState(11)
    return dict(points=np.ascontiguousarray(rng.rand(n, 3)), normals=np.ascontiguousarray(rng.rand(n, 3)), sample_dirs=nr.hemisphere_dirs(4),
                maps=[np.ascontiguousarray(rng.rand(2, 3, 4), np.float32)], node_map=[0, -1])


def _record(fn, **kw):
    with ct.stand_in(abi) as rec:
        out = getattr(nr, fn)(ct.stub_scene(), **kw)
    assert len(rec.calls) == 1, [c[0] for c in rec.calls]  # one call into the library
    name, args, structs = rec.calls[0]
    assert len(args) == len(abi.HIP_SYMBOLS[name][1])
    return out, name, [None if a is None else a if isinstance(a, int) else ct._address(a) if not hasattr(a, "_obj") else "struct" for a in args], structs


def test_gather_maps_sh_points_hands_its_arguments_to_the_blocking_entry_point():
    a = _inputs()
    hf, keys, rot = np.ones(4, np.uint32), np.arange(4, dtype=np.uint64), nr.rotation_table(3)
    out, name, args, structs = _record("gather_maps_sh_points", **a, bands=2, rotations=rot, bias=0.25, max_toi=3.0, miss=(0.5, 0.25, 0.125), hit_flags=hf, keys=keys,
                                       depth=dict(res=4, max_dist=2.5, near_dist=0.5))
    assert name == "nrays_gather_maps_sh_points" and args[0] == ct.SCENE_HANDLE and args[1] == 4
    assert args[2:6] == [a["points"].ctypes.data, a["normals"].ctypes.data, hf.ctypes.data, keys.ctypes.data]
    assert args[6] == "struct" and args[7] == 2 and args[10] == "struct" and args[15] == 0
    p, d = structs[6], structs[10]
    assert (p["num_dirs"], p["num_rotations"], p["bias"], p["max_toi"], p["num_maps"], p["num_nodes"], p["miss_rgb"]) == (4, 3, 0.25, 3.0, 1, 2, [0.5, 0.25, 0.125])
    assert p["dirs"] == ("addr", a["sample_dirs"].ctypes.data) and p["rotations"] == ("addr", rot.ctypes.data) and p["node_map"][1]
    m = p["maps"][0]
    assert (m["width"], m["height"], m["format"], m["interp"], m["overflow"]) == (3, 2, abi.TEXEL_RGBA32F, abi.INTERP_BILINEAR, abi.OVERFLOW_CLAMP) and m["texels"] == ("addr", a["maps"][0].ctypes.data)
    assert d == dict(max_dist=2.5, near_dist=0.5, res=4, reserved=0)
    assert isinstance(out, nr.GatherMapsSh) and isinstance(out.depth, nr.ProbeDepth)
    assert args[8] == out.sh.ctypes.data and args[9] == out.counts.ctypes.data
    assert args[11:15] == [out.depth.moments.ctypes.data, out.depth.counts.ctypes.data, out.depth.nearest.ctypes.data, out.depth.nearest_dir.ctypes.data]
    assert (out.sh.shape, out.sh.dtype, out.counts.shape, out.counts.dtype) == ((4, 4, 3), np.float32, (4, 2), np.uint32)
    assert (out.depth.moments.shape, out.depth.moments.dtype, out.depth.counts.shape, out.depth.nearest.dtype, out.depth.nearest_dir.dtype) == ((4, 16, 2), np.float32, (4, 2), np.float64, np.uint32)


def test_depth_none_passes_a_null_spec_and_unwanted_outputs_are_null():
    a = _inputs()
    out, name, args, structs = _record("gather_maps_sh_points", **a)
    assert name == "nrays_gather_maps_sh_points" and args[7] == 3 and args[10] is None and args[11:15] == [None] * 4 and structs[10] is None
    assert args[4] is None and args[5] is None and structs[6]["rotations"] == ("addr", None) and structs[6]["max_toi"] == math.inf and structs[6]["bias"] == 1e-3
    assert out.depth is None and out.sh.shape == (4, 9, 3) and args[9] == out.counts.ctypes.data
    out, _, args, _ = _record("gather_maps_sh_points", **a, want=())
    assert out.counts is None and args[9] is None and args[8] == out.sh.ctypes.data
    out, _, args, structs = _record("gather_maps_sh_points", **a, depth=dict(max_dist=1.0), want=("nearest",))  # res 8 and near_dist 0 when left out
    assert structs[10] == dict(max_dist=1.0, near_dist=0.0, res=8, reserved=0) and out.depth.moments.shape == (4, 64, 2)
    assert args[9] is None and args[12] is None and args[14] is None and args[11] == out.depth.moments.ctypes.data and args[13] == out.depth.nearest.ctypes.data
    assert out.counts is None and out.depth.counts is None and out.depth.nearest_dir is None
    out, _, args, _ = _record("gather_maps_sh_points", **a, want=WANT_ALL)  # depth outputs wanted without depth settings: still NULL
    assert args[10] is None and args[11:15] == [None] * 4 and out.depth is None


def test_gather_maps_probes_is_the_point_form_with_the_z_normal():
    a = _inputs()
    L = nr.sphere_dirs(6)
    seen = {}
    real = nr.scene.gather_maps_sh_points
    try:
        nr.scene.gather_maps_sh_points = lambda *args: seen.update(args=args) or "result"
        assert nr.gather_maps_probes(ct.stub_scene(), a["points"], L, a["maps"], a["node_map"], 2, 3.0, (1, 2, 3), None, dict(max_dist=1.0), ("counts",)) == "result"
    finally:
        nr.scene.gather_maps_sh_points = real
    g = seen["args"]
    assert g[1] is a["points"] and np.array_equal(g[2], np.tile([0.0, 0.0, 1.0], (4, 1))) and g[3] is L and g[4] is a["maps"] and g[5] is a["node_map"]
    assert g[6:] == (2, None, 0.0, 3.0, (1, 2, 3), None, None, dict(max_dist=1.0), ("counts",))
    out, name, args, structs = _record("gather_maps_probes", positions=a["points"], sample_dirs=L, maps=a["maps"], node_map=a["node_map"], depth=dict(res=16, max_dist=2.0))
    assert name == "nrays_gather_maps_sh_points" and args[2] == a["points"].ctypes.data and structs[6]["bias"] == 0.0 and structs[6]["num_rotations"] == 0 and structs[6]["num_dirs"] == 6
    assert structs[10]["res"] == 16 and out.depth.moments.shape == (4, 256, 2)
    with pytest.raises(ValueError):
        nr.gather_maps_probes(ct.stub_scene(), np.zeros((4, 2)), L, a["maps"], a["node_map"])


def test_bake_probe_grid_maps_is_one_call_with_the_defaults_of_bake_probe_visibility():
    a = _inputs()
    L = nr.sphere_dirs(8)
    origin, cell, counts = (0.0, 1.0, 2.0), (0.5, 2.0, 1.0), (3, 1, 2)
    (grid, vis), name, args, structs = _record("bake_probe_grid_maps", origin=origin, cell=cell, counts=counts, sample_dirs=L, maps=a["maps"], node_map=a["node_map"], bands=2,
                                               miss=(0.5, 0.5, 0.5), visibility={})
    assert name == "nrays_gather_maps_sh_points" and args[1] == 6 and args[7] == 2
    d = structs[10]
    assert d["res"] == 8 and d["max_dist"] == 1.5 * math.sqrt(0.5 * 0.5 + 1.0 * 1.0) and d["near_dist"] == 0.2 * 0.5  # the axes with more than one probe
    assert structs[6]["miss_rgb"] == [0.5, 0.5, 0.5] and structs[6]["bias"] == 0.0 and structs[6]["max_toi"] == math.inf
    assert args[9] is None and args[13] is None and args[14] is None  # only what the bake reads is computed
    assert isinstance(grid, nr.ProbeGrid) and isinstance(vis, nr.ProbeVisibility)
    assert grid.sh.ctypes.data == args[8] and vis.moments.ctypes.data == args[11] and grid.sh.shape == (6, 4, 3) and vis.moments.shape == (6, 64, 2)
    assert (vis.res, vis.floor, vis.bias) == (8, 0.05, 0.0) and grid.measure == 4.0 * math.pi and grid.valid.shape == (6,) and grid.valid.dtype == np.uint32
    assert (grid.origin, grid.cell, grid.counts) == (origin, cell, counts)
    (grid, vis), _, args, structs = _record("bake_probe_grid_maps", origin=origin, cell=cell, counts=counts, sample_dirs=L, maps=a["maps"], node_map=a["node_map"], measure=2.0,
                                            visibility=dict(res=4, max_dist=3.0, near_dist=0.25, floor=0.5, bias=0.125, max_near_fraction=0.5))
    assert structs[10] == dict(max_dist=3.0, near_dist=0.25, res=4, reserved=0) and (vis.res, vis.floor, vis.bias) == (4, 0.5, 0.125) and grid.measure == 2.0 and args[7] == 3
    (grid, vis), _, args, structs = _record("bake_probe_grid_maps", origin=origin, cell=cell, counts=counts, sample_dirs=L, maps=a["maps"], node_map=a["node_map"])
    assert vis is None and grid.valid is None and args[10] is None and args[11:15] == [None] * 4 and args[9] is None


# ---- the wrappers check before any library call --------------------------------------------------------------------------------------------------------------
class _NoDeviceScene(_NoDevice):
    """A two-node scene whose device handle must never be asked for."""
    descriptor = ct.stub_scene().descriptor


def test_the_wrappers_reject_bad_arguments_before_any_library_call(no_library):
    import torch
    sc = _NoDeviceScene()
    a = _inputs()
    bad = [dict(bands=0), dict(bands=4), dict(bands=2.5), dict(bands=True), dict(bands=-1),
           dict(depth=dict(res=8)), dict(depth=dict(max_dist=None)), dict(depth=dict(max_dist=0.0)), dict(depth=dict(max_dist=math.inf)), dict(depth=dict(max_dist=math.nan)),
           dict(depth=dict(max_dist=1.0, res=5)), dict(depth=dict(max_dist=1.0, res=True)), dict(depth=dict(max_dist=1.0, res=8.5)), dict(depth=dict(max_dist=1.0, near_dist=-1e-9)),
           dict(depth=dict(max_dist=1.0, near_dist=math.inf)), dict(depth=dict(max_dist=1.0, floor=0.1)), dict(depth=(8, 1.0, 0.0)), dict(depth=8),
           dict(want=("moments",)), dict(want=("counts", "toi")),
           dict(points=np.zeros((4, 2))), dict(normals=np.zeros((5, 3))), dict(points=None), dict(hit_flags=np.ones(3, np.uint32)), dict(keys=np.zeros(5, np.uint64)),
           dict(keys=np.zeros(4, np.float64)), dict(sample_dirs=np.zeros((0, 3))), dict(sample_dirs=np.zeros((1025, 3))), dict(sample_dirs=np.zeros((4, 2))),
           dict(rotations=np.zeros((3, 3))), dict(bias=math.nan), dict(max_toi=0.0), dict(max_toi=math.nan), dict(miss=(0.0, math.inf, 0.0)), dict(miss=(0.0, 0.0)),
           dict(maps=[]), dict(maps=[np.zeros((3, 5, 3), np.float32)]), dict(maps=[np.zeros((3, 5, 4), np.float64)]), dict(maps=[torch.zeros((3, 5, 4), dtype=torch.float32)]),
           dict(node_map=[0]), dict(node_map=[0, 0, 0]), dict(node_map=None), dict(node_map={2: 0}), dict(normals=torch.zeros((4, 3), dtype=torch.float64))]
    for kw in bad:
        with pytest.raises(ValueError):
            nr.gather_maps_sh_points(sc, **dict(a, **kw))
    for ok in (dict(), dict(bands=1, depth=dict(res=16, max_dist=1.0, near_dist=0.0), want=()), dict(hit_flags=np.ones(4, np.uint32), keys=np.arange(4), rotations=nr.rotation_table(3))):
        with pytest.raises(AssertionError, match="library was loaded"):  # a well-formed call gets as far as the library
            nr.gather_maps_sh_points(sc, **dict(a, **ok))
    L = nr.sphere_dirs(4)
    probes = dict(positions=a["points"], sample_dirs=L, maps=a["maps"], node_map=a["node_map"])
    for kw in (dict(positions=np.zeros((4, 2))), dict(bands=4), dict(depth=dict(res=3, max_dist=1.0)), dict(maps=[])):
        with pytest.raises(ValueError):
            nr.gather_maps_probes(sc, **dict(probes, **kw))
    grid = dict(origin=(0, 0, 0), cell=(1.0, 1.0, 1.0), counts=(2, 2, 1), sample_dirs=L, maps=a["maps"], node_map=a["node_map"])
    for kw in (dict(counts=(0, 1, 1)), dict(cell=(0.0, 1.0, 1.0)), dict(bands=0), dict(visibility=8), dict(visibility=dict(resolution=8)), dict(visibility=dict(res=5)),
               dict(visibility=dict(max_dist=-1.0)), dict(visibility=dict(floor=1.5)), dict(visibility=dict(bias=math.nan)), dict(visibility=dict(max_near_fraction=1.5)),
               dict(counts=(1, 1, 1), visibility={}), dict(sample_dirs=np.zeros((4, 2))), dict(node_map=[0])):
        with pytest.raises(ValueError):
            nr.bake_probe_grid_maps(sc, **dict(grid, **kw))
    for ok in (dict(), dict(visibility={}), dict(counts=(1, 1, 1), visibility=dict(max_dist=2.0))):
        with pytest.raises(AssertionError, match="library was loaded"):
            nr.bake_probe_grid_maps(sc, **dict(grid, **ok))


# ---- the composition the GPU tests restate the call with, on synthetic per-ray records ---------------------------------------------------------------------------
def _synthetic(seed, n, k):
    """Per-ray closest-hit records without a scene: every class present, uvs beyond [0, 1], and unnormalised directions."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, k, 3)) * rng.uniform(0.5, 2.0, size=(n, k, 1))
    hit, has_uv = rng.random(n * k) < 0.7, rng.random(n * k) < 0.8
    node = rng.integers(0, 4, size=n * k)
    u, v = rng.uniform(-0.25, 1.25, size=n * k), rng.uniform(-0.25, 1.25, size=n * k)
    maps = [(random_map(seed + 1, 5, 3, 0.0, 3.0),) + BILINEAR_CLAMP, (random_map(seed + 2, 8, 8),) + (nr.Interpolation.Nearest, nr.Overflow.Wrap)]
    c, cls = contributions(hit, has_uv, node, u, v, maps, [0, 1, -1, 7], (0.25, 1.5, -0.5))
    return d, c.reshape(n, k, 3), cls.reshape(n, k)


@pytest.mark.parametrize("k", [1, 5, 64])
def test_the_restatement_has_the_band_prefix_property_and_counts_the_classes(k):
    n = 37
    d, c, cls = _synthetic(400 + k, n, k)
    assert c.dtype == np.float32 and all((cls == q).any() for q in (DARK, MAPPED, MISSED))
    full = nr.sh_fold_ref(d, c, 3)
    assert full.shape == (n, 9, 3) and full.dtype == np.float32
    assert np.array_equal(bits(nr.sh_fold_ref(d, c, 1)), bits(full[:, :1])) and np.array_equal(bits(nr.sh_fold_ref(d, c, 2)), bits(full[:, :4]))
    rgb, counts = fold_classes(c.reshape(-1, 3), cls.reshape(-1), n, k)
    assert np.array_equal(counts[:, 0], (cls == MAPPED).sum(axis=1)) and np.array_equal(counts[:, 1], (cls == MISSED).sum(axis=1)) and (counts.sum(axis=1) <= k).all()
    # band 0 is a constant basis: the first coefficient is the fold of fl(Y_0) * c_ij, the mean colour's sum scaled — but added in its own roundings
    y0 = np.float32(0.28209479177387814)
    acc = np.zeros((n, 3), np.float32)
    for j in range(k):
        acc = acc + y0 * c[:, j]
    assert np.array_equal(bits(full[:, 0]), bits(acc / np.float32(k)))


@pytest.mark.parametrize("k", [4, 16, 100])
def test_a_constant_contribution_folds_the_rounded_basis_times_the_colour(k):
    """What the furnace and open-sky GPU tests rely on: every ray bringing L gives out_sh[c] = the float32 fold over j of fl(Y_c(d_j)) * L."""
    n, L = 9, np.asarray((0.5, 0.25, 3.0), np.float32)
    pos = np.random.default_rng(7).uniform(-1.0, 1.0, size=(n, 3))
    _, d = nr.occlusion_rays(pos, np.tile([0.0, 0.0, 1.0], (n, 1)), nr.sphere_dirs(k), None, 0.0)
    assert np.array_equal(d, np.broadcast_to(nr.sphere_dirs(k), (n, k, 3)))  # the probe frame reproduces the table
    got = nr.sh_fold_ref(d, np.broadcast_to(L, (n, k, 3)).astype(np.float32), 3)
    y = nr.sh_basis(d, 3)
    assert y.dtype == np.float32
    acc = np.zeros((n, 9, 3), np.float32)
    for j in range(k):
        acc = acc + (y[:, j, :, None] * L[None, None, :]).astype(np.float32)
    assert np.array_equal(bits(got), bits(acc / np.float32(k)))
    assert np.array_equal(bits(got[1:]), bits(np.broadcast_to(got[:1], got[1:].shape)))  # the position does not enter
