"""Incoming light at caller-supplied points (nrays_gather_points_device / nrays_gather_points; nrays_amd.gather_points, gather_hits, bake_indirect,
gather_ray_keys), the parts that need no GPU: the header, the ctypes table and the Rust declarations, the struct's layout against the C compiler's, the
argument checks, the key mirror — and the expected values of three small scenes from the CPU oracle alone (the mirror's rays with the mirror's keys through
the oracle's Scene::trace, folded in numpy f32), which tests/test_gather_gpu.py imports."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import nrays_amd as nr
from nrays_amd import abi, math3d
from nrays_amd.scene import SALT_GATHER, _rng_hash
from tests.test_occlusion import _surface_points, quad_scene
from tests.test_shade_points import rich_analytic_scene, scattered_rays
from tests.test_trace_rays import build_shim, shim_trace
from tools import scenes_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_TEXT = open(os.path.join(ROOT, "include", "nrays_abi.h")).read()
HEADER = re.sub(r"/\*.*?\*/", "", HEADER_TEXT, flags=re.S)
FFI = open(os.path.join(ROOT, "integration", "rust", "src", "gpu_ffi.rs")).read()
GPU_RS = open(os.path.join(ROOT, "integration", "rust", "src", "gpu.rs")).read()
_IN = ["NraysScene*", "uint32_t", "const double*", "const double*", "const uint32_t*", "const uint64_t*", "const NraysGatherParams*", "float*", "uint32_t"]
EXPECTED = {"nrays_gather_points_device": _IN + ["void*"], "nrays_gather_points": _IN}
RUST_TYPES = {"NraysScene*": "*mut NraysScene", "uint32_t": "u32", "const double*": "*const f64", "const uint32_t*": "*const u32", "const uint64_t*": "*const u64",
              "const NraysGatherParams*": "*const NraysGatherParams", "float*": "*mut f32", "void*": "*mut c_void"}
STRUCT_FIELDS = [("num_dirs", "uint32_t", "u32", C.c_uint32), ("num_rotations", "uint32_t", "u32", C.c_uint32), ("dirs", "const double*", "*const f64", C.c_void_p),
                 ("rotations", "const double*", "*const f64", C.c_void_p), ("bias", "double", "f64", C.c_double), ("energy", "float", "f32", C.c_float),
                 ("max_depth", "uint32_t", "u32", C.c_uint32)]
SKY = (0.25, 0.5, 1.0)


# ---- shared with the GPU tests ------------------------------------------------------------------------------------------------------------------------
def fold(colours):
    """The fold of the definition on per-ray colours (n, k, 3) float32: f32 sum in the order of j, then one division by float32(k)."""
    n, k = colours.shape[:2]
    total = np.zeros((n, 3), np.float32)
    for j in range(k):
        total = total + colours[:, j].astype(np.float32)
    return total / np.float32(k)


_SHIM = []


def oracle_shim():
    """The oracle's Scene::trace on caller rays (tests/trace_oracle_shim.c), built once per process."""
    if not _SHIM:
        _SHIM.append(build_shim(tempfile.mkdtemp(prefix="gather_shim")))
    return _SHIM[0]


def _keys(seed, n):
    return np.random.default_rng(seed).integers(0, 2**63, size=n, dtype=np.int64).astype(np.uint64) * np.uint64(2) + np.uint64(1)


def _analytic_case():
    """rich_analytic_scene (tests/test_shade_points.py): reflective and half-transparent nodes.  320 surface points."""
    sc, _ = rich_analytic_scene()
    o, d = scattered_rays(np.random.default_rng(61), 1200)
    p, nm, _ = _surface_points(sc, o, d)
    assert len(p) >= 320
    sel = np.linspace(0, len(p) - 1, 320).astype(int)
    return dict(scene=sc, points=np.ascontiguousarray(p[sel]), normals=np.ascontiguousarray(nm[sel]), keys=_keys(62, 320))


def _quad_case():
    """The alpha-mapped quad scene (tests/test_shade_points_gpu.py): meshes, an opacity map and a colour texture.  320 surface points."""
    sc, cam = quad_scene()
    proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], 40, 40)
    o, d, _ = nr.camera_rays((40, 40), cam["eye"], proj, seed=9)
    p, nm, _ = _surface_points(sc, o, d)
    assert len(p) >= 320
    sel = np.linspace(0, len(p) - 1, 320).astype(int)
    return dict(scene=sc, points=np.ascontiguousarray(p[sel]), normals=np.ascontiguousarray(nm[sel]), keys=_keys(63, 320))


def _sky_case():
    """Points on an upward plane with nothing above it: every ray sees the background, whose partial sums j * (0.25, 0.5, 1.0), j <= 8, are exact in f32."""
    sc = nr.Scene([nr.SceneNode(su.default_material(), 0.0, 0.0, 1.0, 1.0, nr.Isometry3((0, 0, 0)), nr.Plane((0, 1, 0)))], [nr.Light((0.0, 5.0, 0.0), 0.0, 1, (1, 1, 1))], SKY)
    xz = np.random.default_rng(64).uniform(-20.0, 20.0, size=(97, 2))
    p = np.stack([xz[:, 0], np.zeros(97), xz[:, 1]], axis=1)
    return dict(scene=sc, points=p, normals=np.tile([0.0, 1.0, 0.0], (97, 1)), keys=_keys(65, 97))


_ORACLE = {}
_MAKERS = {"analytic": (_analytic_case, 16, (0, 1)), "quads": (_quad_case, 16, (0, 1)), "sky": (_sky_case, 8, (0,))}


def oracle_case(name):
    """Per scene, computed once and left unchanged: the arguments of gather_points and, per max_depth, what the CPU oracle expects — occlusion_rays() with
    gather_ray_keys() through the oracle's Scene::trace, folded in numpy f32.  c["rgb"][max_depth] (n, 3), c["ray_rgb"][max_depth] (n, k, 3)."""
    if name not in _ORACLE:
        make, k, depths = _MAKERS[name]
        c = make()
        c.update(sample_dirs=nr.hemisphere_dirs(k), rotations=nr.rotation_table(5), bias=1e-3, energy=1.0)
        ro, rd = nr.occlusion_rays(c["points"], c["normals"], c["sample_dirs"], c["rotations"], c["bias"], c["keys"])
        n = len(c["points"])
        rk = nr.gather_ray_keys(c["keys"], k)
        c["rgb"], c["ray_rgb"] = {}, {}
        for depth in depths:
            rgb = shim_trace(oracle_shim(), c["scene"], ro.reshape(-1, 3), rd.reshape(-1, 3), energy=np.full(n * k, c["energy"], np.float32), keys=rk.reshape(-1),
                             max_depth=depth).reshape(n, k, 3)
            c["ray_rgb"][depth], c["rgb"][depth] = rgb, fold(rgb)
        _ORACLE[name] = c
    return _ORACLE[name]


def call_args(c, max_depth):
    return dict({k: c[k] for k in ("points", "normals", "sample_dirs", "rotations", "bias", "energy", "keys")}, max_depth=max_depth)


# ---- the surface --------------------------------------------------------------------------------------------------------------------------------------------
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
    assert res is C.c_int and len(args) == len(EXPECTED[name]) and args[1] is C.c_uint32
    assert args[EXPECTED[name].index("const NraysGatherParams*")] is C.POINTER(abi.NraysGatherParams)
    m = re.search(r"pub fn %s\((.*?)\) -> c_int;" % name, FFI)
    assert m, "%s is not declared in gpu_ffi.rs" % name
    assert [p.split(": ", 1)[1] for p in m.group(1).split(", ")] == [RUST_TYPES[t] for t in EXPECTED[name]]
    assert "pub fn gather_points(" in GPU_RS and "pub unsafe fn gather_points_device(" in GPU_RS
    assert "nrays_gather_points(" in GPU_RS and "nrays_gather_points_device(" in GPU_RS


def test_the_params_struct_is_the_same_in_the_header_ctypes_rust_and_the_c_compiler(tmp_path):
    m = re.search(r"struct NraysGatherParams \{(.*?)\};\s*typedef struct NraysGatherParams NraysGatherParams;", HEADER, re.S)
    assert m, "struct NraysGatherParams is not declared in include/nrays_abi.h (struct plus separate typedef)"
    c_fields = [re.sub(r"\s*\*\s*", "* ", f.strip()).rsplit(" ", 1) for f in m.group(1).split(";") if f.strip()]
    assert [(n, t) for t, n in c_fields] == [(n, t) for n, t, _, _ in STRUCT_FIELDS]
    r = re.search(r"#\[repr\(C\)\]\s*(?:#\[derive[^\]]*\]\s*)?pub struct NraysGatherParams \{(.*?)\n\}", FFI, re.S)
    assert r and re.findall(r"pub (\w+): ([^,]+),", r.group(1)) == [(n, t) for n, _, t, _ in STRUCT_FIELDS]
    assert [(n, t) for n, t in abi.NraysGatherParams._fields_] == [(n, t) for n, _, _, t in STRUCT_FIELDS]
    # the layout, from the C compiler itself
    src = tmp_path / "layout.c"
    names = [n for n, _, _, _ in STRUCT_FIELDS]
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "nrays_abi.h"\nint main(void) {\n    printf("%zu", sizeof(NraysGatherParams));\n'
                   + "".join('    printf(" %%zu", offsetof(NraysGatherParams, %s));\n' % n for n in names) + '    printf("\\n");\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [C.sizeof(abi.NraysGatherParams)] + [getattr(abi.NraysGatherParams, n).offset for n in names]
    assert got == [40, 0, 4, 8, 16, 24, 32, 36]


def test_the_abi_version_is_still_7(built):
    assert re.search(r"#define NRAYS_ABI_VERSION 7\b", HEADER) and abi.ABI_VERSION == 7 and abi.load_hip_lib().nrays_abi_version() == 7
    note = re.search(r"Added after 7 WITHOUT a bump.*?\*/", HEADER_TEXT, re.S).group(0)
    exported = subprocess.check_output(["nm", "-D", "--defined-only", abi.HIP_LIB_PATH]).decode()
    for name in EXPECTED:
        assert re.search(r"%s\b" % name, note), name
        assert (" T " + name + "\n") in exported, name
        assert getattr(abi.load_hip_lib(), name).argtypes == abi.HIP_SYMBOLS[name][1]


def test_without_a_scene_every_call_is_a_bad_arg(built):
    """Without a scene nothing else is looked at; the other arguments one by one need a scene: tests/test_gather_gpu.py."""
    lib = abi.load_hip_lib()
    a = (C.c_double * 3)(0.0, 0.0, 1.0)
    out = (C.c_float * 3)(7.0, 7.0, 7.0)
    adr = C.addressof
    for params in (abi.NraysGatherParams(1, 0, adr(a), None, 1e-3, 1.0, 0), abi.NraysGatherParams(0, 0, None, None, math.nan, math.inf, 0)):
        for n in (0, 1):
            for flags in (0, 1):
                assert lib.nrays_gather_points(None, n, a, a, None, None, C.byref(params), out, flags) == abi.ERR_BAD_ARG
                assert lib.nrays_gather_points_device(None, n, adr(a), adr(a), None, None, C.byref(params), adr(out), flags, None) == abi.ERR_BAD_ARG
            assert lib.nrays_gather_points(None, n, None, None, None, None, None, None, 0) == abi.ERR_BAD_ARG
    assert lib.nrays_last_error() and list(out) == [7.0] * 3


# ---- the Python wrappers check before any library call ------------------------------------------------------------------------------------------------------
class _NoDevice:
    """A scene whose device handle must never be asked for: argument errors are raised first."""
    def device_handle(self):
        raise AssertionError("device touched before the arguments were checked")


@pytest.fixture()
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(abi, "load_hip_lib", refuse)


def _good(n=4):
    return dict(points=np.zeros((n, 3)), normals=np.tile([0.0, 1.0, 0.0], (n, 1)), sample_dirs=nr.hemisphere_dirs(4))


def test_gather_points_rejects_bad_arguments_before_any_library_call(no_library):
    import torch
    sc = _NoDevice()
    t3 = torch.zeros((4, 3), dtype=torch.float64)
    bad = [
        dict(points=np.zeros((4, 2))), dict(points=np.zeros(12)), dict(points=None), dict(normals=None), dict(normals=np.zeros((5, 3))),
        dict(points=np.zeros((4, 3), np.int64)), dict(normals=np.zeros((4, 3), np.int32)),
        dict(sample_dirs=None), dict(sample_dirs=np.zeros((0, 3))), dict(sample_dirs=np.zeros((1025, 3))), dict(sample_dirs=np.zeros((4, 2))), dict(sample_dirs=np.zeros(12)),
        dict(rotations=np.zeros((1025, 2))), dict(rotations=np.zeros((3, 3))), dict(rotations=np.zeros(4)),
        dict(bias=math.inf), dict(bias=math.nan), dict(energy=math.inf), dict(energy=-math.inf), dict(energy=math.nan), dict(energy=1e39),  # (1e39 is +inf as an f32)
        dict(max_depth=-1), dict(max_depth=1 << 32),
        dict(hit_flags=np.ones(3, np.uint32)), dict(hit_flags=np.ones(4, np.float32)), dict(keys=np.zeros(5, np.uint64)), dict(keys=np.zeros(4, np.float64)),
        dict(normals=t3),                                          # numpy and torch mixed
        dict(sample_dirs=torch.zeros((4, 3), dtype=torch.float64)),
        dict(keys=torch.zeros(4, dtype=torch.int64)),
        dict(points=t3, normals=t3),                               # torch tensors on the host
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            nr.gather_points(sc, **dict(_good(), **kw))
    with pytest.raises(ValueError):
        nr.Scene([], []).gather_points(np.zeros((4, 2)), _good()["normals"], _good()["sample_dirs"])
    with pytest.raises(AssertionError, match="library was loaded"):  # a well-formed call gets as far as the library
        nr.gather_points(sc, rotations=nr.rotation_table(3), energy=0.15, max_depth=3, hit_flags=np.ones(4, np.uint32), keys=np.arange(4), **_good())
    with pytest.raises(AssertionError, match="library was loaded"):
        nr.gather_points(sc, rotations=np.zeros((0, 2)), bias=0.0, energy=0.0, **_good())
    from nrays_amd import scenefile
    for cls in (nr.Scene, scenefile.FileScene):
        assert callable(cls.gather_points) and callable(cls.bake_indirect)
    with pytest.raises(ValueError):
        nr.bake_indirect(sc, 0, 0, 8, nr.hemisphere_dirs(4))  # an empty map: refused by surface_texels' own check, before the library


def test_gather_hits_refuses_incomplete_hits_and_flips_the_normals(no_library, monkeypatch):
    sc = _NoDevice()
    o, d = np.zeros((4, 3)), np.tile([0.0, 0.0, 1.0], (4, 1))
    normal = np.asarray([(0.0, 0.0, -1.0), (0.0, 0.0, 1.0), (0.6, 0.0, 0.8), (1.0, 0.0, 0.0)])
    full = nr.CastHits(toi=np.asarray([1.0, 2.0, 3.0, 4.0]), node=np.zeros(4, np.int32), normal=normal, uv=None, prim=None, flags=np.asarray([1, 3, 1, 0], np.uint32))
    L = nr.hemisphere_dirs(4)
    for name in ("normal", "flags"):
        with pytest.raises(ValueError, match=name):
            nr.gather_hits(sc, o, d, full._replace(**{name: None}), L)
    with pytest.raises(ValueError):
        nr.gather_hits(sc, o[:3], d, full, L)
    with pytest.raises(AssertionError, match="library was loaded"):  # uv and prim are not needed
        nr.gather_hits(sc, o, d, full, L)
    seen = {}
    monkeypatch.setattr(nr.scene, "gather_points", lambda scene, points, normals, *a, **kw: seen.update(points=points, normals=normals, a=a, kw=kw) or "result")
    assert nr.gather_hits(sc, o, d, full, L, None, 0.25, 0.5, 3, keys=np.arange(4)) == "result"
    assert np.array_equal(seen["points"], [(0, 0, 1), (0, 0, 2), (0, 0, 3), (0, 0, 0)])  # origins + dirs * toi, toi 0 at the miss: occlusion_hits' points
    assert np.array_equal(seen["normals"], [(0, 0, -1), (0, 0, -1), (-0.6, 0, -0.8), (1, 0, 0)])  # negated where n . d > 0
    assert seen["a"][1:] == (None, 0.25, 0.5, 3)
    assert np.array_equal(seen["kw"]["hit_flags"], full.flags) and np.array_equal(seen["kw"]["keys"], np.arange(4))


def test_gather_ray_keys_is_the_hash_of_the_point_key_and_the_ray_index():
    assert SALT_GATHER == 0x301 << 32
    m64 = 2**64 - 1

    def scalar(key, j):  # mix((key ^ salt * golden) + c), by hand
        z = ((key ^ (((SALT_GATHER + j) * 0x9E3779B97F4A7C15) & m64)) + 0xD1B54A32D192ED03) & m64
        z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & m64
        z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & m64
        return z ^ (z >> 31)
    keys = np.asarray([0, 1, 7, 2**63 + 5, m64], dtype=np.uint64)
    got = nr.gather_ray_keys(keys, 16)
    assert got.shape == (5, 16) and got.dtype == np.uint64
    for i, key in enumerate(keys.tolist()):
        for j in (0, 1, 2, 15):
            assert int(got[i, j]) == scalar(key, j), (key, j)
    assert len(np.unique(got)) == got.size  # differs per j and per key
    assert np.array_equal(nr.gather_ray_keys(keys, 1024)[:, :16], got)
    assert np.array_equal(nr.gather_ray_keys(np.arange(4), 3), _rng_hash(np.arange(4, dtype=np.uint64)[:, None].repeat(3, axis=1), np.uint64(SALT_GATHER) + np.arange(3, dtype=np.uint64)[None, :].repeat(4, axis=0)))
    assert not np.array_equal(got[:, 0], _rng_hash(keys, 0x300 << 32))  # not the rotation pick's salt
    for bad in (0, 1025):
        with pytest.raises(ValueError):
            nr.gather_ray_keys(keys, bad)
    with pytest.raises(ValueError):
        nr.gather_ray_keys(np.zeros(4), 4)
    with pytest.raises(ValueError):
        nr.gather_ray_keys(np.zeros((2, 2), np.uint64), 4)


# ---- the expected values from the oracle ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["analytic", "quads"])
def test_oracle_expectations(name):
    c = oracle_case(name)
    bg = np.asarray(c["scene"]._background, np.float32)
    assert c["points"].shape == (320, 3) and c["sample_dirs"].shape == (16, 3) and c["rotations"].shape == (5, 2)
    for depth in (0, 1):
        rgb, rays = c["rgb"][depth], c["ray_rgb"][depth]
        assert rgb.shape == (320, 3) and rgb.dtype == np.float32 and rays.shape == (320, 16, 3) and np.isfinite(rays).all()
        sky = (rays == bg).all(axis=2)
        assert 0.05 < sky.mean() < 0.95  # rays that see the background and rays that hit something
        mixed = ~(rgb == bg).all(axis=1) & (rgb != 0.0).any(axis=1)
        assert mixed.sum() >= 100  # means that are neither the background nor zero
    if name == "analytic":  # reflective / half-transparent nodes: the recursion matters
        assert (c["rgb"][0] != c["rgb"][1]).any()
    # another set of keys gives other rotations, so other rays
    ro, _ = nr.occlusion_rays(c["points"], c["normals"], c["sample_dirs"], c["rotations"], c["bias"], c["keys"])
    assert not np.array_equal(ro, nr.occlusion_rays(c["points"], c["normals"], c["sample_dirs"], c["rotations"], c["bias"], None)[1])


def test_open_sky_expectation_is_exactly_the_background():
    c = oracle_case("sky")
    assert c["sample_dirs"].shape == (8, 3) and (c["ray_rgb"][0] == np.asarray(SKY, np.float32)).all()
    assert np.array_equal(c["rgb"][0], np.tile(np.asarray(SKY, np.float32), (97, 1)))
