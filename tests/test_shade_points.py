"""Material::compute on caller-supplied surface points (nrays_shade_points_device / nrays_shade_points; nrays_amd.shade_points, shade_hits), the parts
that need no GPU: the header, the ctypes table and the Rust declarations agree on the two entry points, the argument checks of the library and of the
Python wrappers, and — on the CPU oracle alone (tests/shade_oracle_shim.c: its material_compute on caller points) — the premise of the GPU identity test:
on nodes that neither reflect nor refract, compute() at the closest hit IS Scene::trace's colour.  The scenes and the oracle wrapper are shared with
tests/test_shade_points_gpu.py."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import nrays_amd as nr
import oracle
from nrays_amd import abi, math3d
from tests.test_trace_rays import analytic_scene, build_shim, shim_trace
from tools import scenes_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_TEXT = open(os.path.join(ROOT, "include", "nrays_abi.h")).read()
HEADER = re.sub(r"/\*.*?\*/", "", HEADER_TEXT, flags=re.S)
FFI = open(os.path.join(ROOT, "integration", "rust", "src", "gpu_ffi.rs")).read()
GPU_RS = open(os.path.join(ROOT, "integration", "rust", "src", "gpu.rs")).read()
_INPUTS = ["NraysScene*", "uint32_t", "const double*", "const double*", "const double*", "const double*", "const int32_t*", "const uint32_t*", "const uint64_t*", "float*",
           "uint32_t"]
EXPECTED = {"nrays_shade_points_device": _INPUTS + ["void*"], "nrays_shade_points": _INPUTS}  # the C parameter types the issue states, in order
RUST_TYPES = {"NraysScene*": "*mut NraysScene", "uint32_t": "u32", "const double*": "*const f64", "const int32_t*": "*const i32", "const uint32_t*": "*const u32",
              "const uint64_t*": "*const u64", "float*": "*mut f32", "void*": "*mut c_void"}


# ---- shared with the GPU tests: the oracle on caller points, and the scenes -----------------------------------------------------------------
def build_shade_shim(directory):
    """Compiles tests/shade_oracle_shim.c with the oracle Makefile's flags and loads it."""
    out = os.path.join(str(directory), "libshade_oracle_shim.so")
    subprocess.check_call(["gcc", "-O3", "-std=c11", "-ffp-contract=off", "-fPIC", "-shared", "-o", out, os.path.join(ROOT, "tests", "shade_oracle_shim.c"), "-lm", "-lpthread"])
    lib = C.CDLL(out)
    dp = C.POINTER(C.c_double)
    lib.shade_oracle_points.restype = C.c_int
    lib.shade_oracle_points.argtypes = [C.POINTER(abi.NraysSceneDesc), C.c_uint32, dp, dp, dp, dp, C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                        C.POINTER(C.c_float)]
    return lib


def shim_shade(lib, scene, points, normals, view_dirs, nodes, uvs=None, hit_flags=None, keys=None):
    """The oracle's material.compute of every point, with the arrays and the skip rule of nrays_shade_points: (n, 4) float32."""
    f64 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
    p, nm, v, uv = f64(points), f64(normals), f64(view_dirs), f64(uvs)
    nd = np.ascontiguousarray(nodes, dtype=np.int32)
    hf = None if hit_flags is None else np.ascontiguousarray(hit_flags).astype(np.uint32)
    k = None if keys is None else np.ascontiguousarray(keys, dtype=np.uint64)
    out = np.empty((len(p), 4), dtype=np.float32)
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    rc = lib.shade_oracle_points(scene.descriptor.pointer(), len(p), ptr(p, C.c_double), ptr(nm, C.c_double), ptr(v, C.c_double), ptr(uv, C.c_double), ptr(nd, C.c_int32),
                                 ptr(hf, C.c_uint32), ptr(k, C.c_uint64), ptr(out, C.c_float))
    assert rc == 0, rc
    return out


def opaque(scene):
    """The scene with every node made opaque and non-reflective (refl 0 0, alpha 1): Scene::trace of a ray that hits is material.compute at the hit."""
    nodes = [nr.SceneNode(n.material, 0.0, 0.0, 1.0, n.refr_coeff, n.transform, n.geometry) for n in scene._nodes]
    return nr.Scene(nodes, scene._lights, scene._background)


def rich_analytic_scene():
    """analytic_scene()'s shapes (one node reflects AND refracts, the box refracts) with a cone, a cylinder and a capsule, one NormalMaterial and one
    UVMaterial node, under an area light of 2 samples per axis plus a point light."""
    sc, cam = analytic_scene(background=(0.25, 0.5, 0.75))
    red = nr.PhongMaterial((0.15, 0.05, 0.05), (0.9, 0.3, 0.2), (0.7, 0.7, 0.7), None, None, 30.0)
    iso = nr.Isometry3
    nodes = list(sc._nodes) + [
        nr.SceneNode(red, 0.2, 0.3, 1.0, 1.0, iso((-2.6, -0.5, 1.5), (0.0, 0.0, math.radians(20.0))), nr.Cone(0.7, 0.6)),
        nr.SceneNode(red, 0.0, 0.0, 0.6, 1.2, iso((2.8, -0.4, -0.5), (math.radians(30.0), 0.0, 0.0)), nr.Cylinder(0.8, 0.5)),
        nr.SceneNode(su.default_material(), 0.0, 0.0, 1.0, 1.0, iso((0.3, -0.6, -1.8)), nr.Capsule(0.4, 0.3)),
        nr.SceneNode(nr.NormalMaterial(), 0.0, 0.0, 1.0, 1.0, iso((-0.6, 1.6, 0.6)), nr.Ball(0.5)),
        nr.SceneNode(nr.UVMaterial(), 0.0, 0.0, 1.0, 1.0, iso((1.6, 1.9, 0.2)), nr.Ball(0.5))]
    lights = [nr.Light((2.0, 6.0, -4.0), 0.4, 4, (0.8, 0.8, 0.7)), nr.Light((-4.0, 3.0, -3.0), 0.0, 1, (0.3, 0.3, 0.4))]
    assert lights[0].racsample == 2
    return nr.Scene(nodes, lights, sc._background), cam


def scattered_rays(rng, n):
    """Arbitrary rays around the analytic scenes: from a shell around them towards points inside, plus rays that point away (misses)."""
    o = rng.normal(size=(n, 3))
    o *= rng.uniform(5.0, 9.0, size=(n, 1)) / np.sqrt((o * o).sum(axis=1))[:, None]
    o[:, 1] = np.abs(o[:, 1]) + 0.2  # above the plane
    t = rng.uniform(-2.5, 2.5, size=(n, 3)) - o
    d = t / np.sqrt((t * t).sum(axis=1))[:, None]
    away = np.arange(n) % 8 == 3
    d[away] = o[away] / np.sqrt((o[away] * o[away]).sum(axis=1))[:, None]
    return o, d


def odd_keys(rng, n):
    return rng.integers(0, 2**63, size=n, dtype=np.int64).astype(np.uint64) * np.uint64(2) + np.uint64(1)


# ---- the surface ----------------------------------------------------------------------------------------------------------------------------------
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
    assert res is C.c_int and len(args) == len(EXPECTED[name])
    assert args[1] is C.c_uint32 and args[10] is C.c_uint32
    m = re.search(r"pub fn %s\((.*?)\) -> c_int;" % name, FFI)
    assert m, "%s is not declared in gpu_ffi.rs" % name
    assert [p.split(": ", 1)[1] for p in m.group(1).split(", ")] == [RUST_TYPES[t] for t in EXPECTED[name]]
    assert "%s(" % name in GPU_RS and "pub fn shade_points(" in GPU_RS and "pub unsafe fn shade_points_device(" in GPU_RS


def test_the_abi_version_is_still_7(built):
    assert re.search(r"#define NRAYS_ABI_VERSION 7\b", HEADER) and abi.ABI_VERSION == 7 and abi.load_hip_lib().nrays_abi_version() == 7
    note = re.search(r"Added after 7 WITHOUT a bump.*?\*/", HEADER_TEXT, re.S).group(0)
    assert "nrays_shade_points_device" in note and re.search(r"nrays_shade_points\b", note)
    exported = subprocess.check_output(["nm", "-D", "--defined-only", abi.HIP_LIB_PATH]).decode()
    for name in EXPECTED:
        assert (" T " + name + "\n") in exported, name
        assert getattr(abi.load_hip_lib(), name).argtypes == abi.HIP_SYMBOLS[name][1]


def test_null_arguments_and_flags_are_bad_args(built):
    """Without a scene nothing else is looked at; the other arguments one by one need a scene: tests/test_shade_points_gpu.py."""
    lib = abi.load_hip_lib()
    a = (C.c_double * 3)(0.0, 0.0, 1.0)
    uv, node, hf, key, out = (C.c_double * 2)(), (C.c_int32 * 1)(0), (C.c_uint32 * 1)(3), (C.c_uint64 * 1)(1), (C.c_float * 4)(7.0, 7.0, 7.0, 7.0)
    adr = C.addressof
    for n in (0, 1):
        for flags in (0, 1):
            assert lib.nrays_shade_points(None, n, a, a, a, uv, node, hf, key, out, flags) == abi.ERR_BAD_ARG
            assert lib.nrays_shade_points(None, n, a, a, a, None, node, None, None, out, flags) == abi.ERR_BAD_ARG
            assert lib.nrays_shade_points_device(None, n, adr(a), adr(a), adr(a), adr(uv), adr(node), adr(hf), adr(key), adr(out), flags, None) == abi.ERR_BAD_ARG
    assert lib.nrays_last_error() and list(out) == [7.0] * 4


# ---- the Python wrappers check before any library call ----------------------------------------------------------------------------------------------
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
    z = np.zeros((n, 3))
    return dict(points=z, normals=np.tile([0.0, 1.0, 0.0], (n, 1)), view_dirs=np.tile([0.0, -1.0, 0.0], (n, 1)), nodes=np.zeros(n, np.int32))


def test_shade_points_rejects_bad_arguments_before_any_library_call(no_library):
    import torch
    sc = _NoDevice()
    t3 = torch.zeros((4, 3), dtype=torch.float64)
    bad = [
        dict(points=np.zeros((4, 2))),                               # not (n, 3)
        dict(points=np.zeros(12)),                                   # flat
        dict(normals=np.zeros((5, 3))),                              # different numbers of points
        dict(view_dirs=np.zeros((3, 3))),
        dict(view_dirs=np.zeros((4, 2))),
        dict(view_dirs=None), dict(nodes=None), dict(points=None), dict(normals=None),
        dict(nodes=np.zeros(5, np.int32)),
        dict(nodes=np.zeros((4, 1), np.int32)),
        dict(nodes=np.zeros(4, np.float64)),                         # not integers
        dict(uvs=np.zeros((4, 3))), dict(uvs=np.zeros(8)), dict(uvs=np.zeros((3, 2))),
        dict(uvs=np.zeros((4, 2), np.int32)),
        dict(hit_flags=np.ones(3, np.uint32)), dict(hit_flags=np.ones(4, np.float32)),
        dict(keys=np.zeros(5, np.uint64)), dict(keys=np.zeros(4, np.float64)),
        dict(points=np.zeros((4, 3), np.int64)), dict(normals=np.zeros((4, 3), np.int32)),
        dict(normals=t3),                                            # numpy and torch mixed
        dict(nodes=torch.zeros(4, dtype=torch.int32)),
        dict(points=t3, normals=t3, view_dirs=t3, nodes=torch.zeros(4, dtype=torch.int32)),  # torch tensors on the host
    ]
    for kw in bad:
        args = dict(_good(), **kw)
        with pytest.raises(ValueError):
            nr.shade_points(sc, **args)
    with pytest.raises(ValueError):
        nr.Scene([], []).shade_points(np.zeros((4, 2)), **{k: v for k, v in _good().items() if k != "points"})
    # a well-formed call gets as far as the library
    with pytest.raises(AssertionError, match="library was loaded"):
        nr.shade_points(sc, uvs=np.zeros((4, 2)), hit_flags=np.full(4, 3, np.uint32), keys=np.arange(4), **_good())


def test_shade_hits_refuses_incomplete_hits(no_library):
    sc = _NoDevice()
    o, d = np.zeros((4, 3)), np.tile([0.0, 0.0, 1.0], (4, 1))
    full = nr.CastHits(toi=np.ones(4), node=np.zeros(4, np.int32), normal=np.tile([0.0, 0.0, -1.0], (4, 1)), uv=np.zeros((4, 2)), prim=None,
                       flags=np.full(4, 3, np.uint32))
    for name in ("normal", "uv", "flags"):
        with pytest.raises(ValueError, match=name):
            nr.shade_hits(sc, o, d, full._replace(**{name: None}))
    with pytest.raises(ValueError):
        nr.shade_hits(sc, o[:3], d, full)
    with pytest.raises(ValueError):
        nr.shade_hits(sc, o[:3], d[:3], full)
    with pytest.raises(AssertionError, match="library was loaded"):  # prim is not needed
        nr.shade_hits(sc, o, d, full)
    assert nr.shade_points is nr.scene.shade_points and nr.shade_hits is nr.scene.shade_hits
    from nrays_amd import scenefile
    assert callable(nr.Scene.shade_points) and callable(scenefile.FileScene.shade_points)


# ---- the premise of the GPU identity test, on the oracle alone ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shims(tmp_path_factory):
    d = tmp_path_factory.mktemp("shade_shim")
    return build_shim(d), build_shade_shim(d)


def test_compute_at_the_closest_hit_is_trace_on_opaque_nodes(shims):
    """analytic_scene()'s shapes, every node opaque and non-reflective: material.compute at the hits of oracle.cast, viewed along the rays with the
    rays' keys, equals scene_trace of the same rays — obj.rgb * (1 - 0) + 0 * 0 with alpha 1 (scene.rs:179-190) — compared as values (-0 == +0)."""
    trace_lib, shade_lib = shims
    sc, cam = analytic_scene()
    sc = opaque(sc)
    w, h = 40, 30
    proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], w, h)
    o, d, k = nr.camera_rays((w, h), cam["eye"], proj, seed=5)
    so, sd = scattered_rays(np.random.default_rng(1), 800)
    o, d, k = np.concatenate([o, so]), np.concatenate([d, sd]), np.concatenate([k, odd_keys(np.random.default_rng(2), 800)])
    hit, rec = oracle.cast(sc.descriptor, o, d)
    assert 600 < hit.sum() < len(o) - 50 and set(rec[hit, 7].astype(int)) == {0, 1, 2, 3}
    toi = np.where(hit, rec[:, 0], 0.0)
    points = o + d * toi[:, None]
    flags = (hit.astype(np.uint32) | (np.where(rec[:, 4] != 0.0, 2, 0) * hit).astype(np.uint32))
    nodes = np.where(hit, rec[:, 7], -1).astype(np.int32)
    got = shim_shade(shade_lib, sc, points, rec[:, 1:4], d, nodes, uvs=rec[:, 5:7], hit_flags=flags, keys=k)
    ref = shim_trace(trace_lib, sc, o, d, keys=k)
    assert np.array_equal(got[hit, :3], ref[hit])
    assert (got[hit, 3] == 1.0).all() and (got[~hit] == 0.0).all()
    assert np.unique(ref[hit], axis=0).shape[0] > 100  # (lit, shadowed and specular points: not one flat colour)
