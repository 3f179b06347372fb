"""Ambient occlusion at caller-supplied points (nrays_occlusion_points_device / nrays_occlusion_points / nrays_debug_occlusion_rays; nrays_amd.occlusion_points,
occlusion_hits, occlusion_rays), the parts that need no GPU: the numpy mirror of the ray definition against the properties the definition promises, the
header, the ctypes table and the Rust declarations, the argument checks — and the expected values of two small scenes from the CPU oracle alone (the
mirror's rays through nrays_oracle_shadow, folded in numpy f32), which tests/test_occlusion_gpu.py imports."""
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
from nrays_amd.scene import SALT_OCCLUSION, _rng_hash
from tests.test_shade_points import rich_analytic_scene, scattered_rays

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_TEXT = open(os.path.join(ROOT, "include", "nrays_abi.h")).read()
HEADER = re.sub(r"/\*.*?\*/", "", HEADER_TEXT, flags=re.S)
FFI = open(os.path.join(ROOT, "integration", "rust", "src", "gpu_ffi.rs")).read()
GPU_RS = open(os.path.join(ROOT, "integration", "rust", "src", "gpu.rs")).read()
_IN = ["NraysScene*", "uint32_t", "const double*", "const double*", "const uint32_t*", "const uint64_t*", "const NraysOcclusionParams*", "float*", "uint32_t*", "uint32_t"]
EXPECTED = {"nrays_occlusion_points_device": _IN + ["void*"], "nrays_occlusion_points": _IN,
            "nrays_debug_occlusion_rays": ["NraysScene*", "uint32_t", "const double*", "const double*", "const uint64_t*", "const NraysOcclusionParams*", "double*", "double*"]}
RUST_TYPES = {"NraysScene*": "*mut NraysScene", "uint32_t": "u32", "const double*": "*const f64", "const uint32_t*": "*const u32", "const uint64_t*": "*const u64",
              "const NraysOcclusionParams*": "*const NraysOcclusionParams", "float*": "*mut f32", "uint32_t*": "*mut u32", "double*": "*mut f64", "void*": "*mut c_void"}
STRUCT_FIELDS = [("num_dirs", "uint32_t", "u32", C.c_uint32), ("num_rotations", "uint32_t", "u32", C.c_uint32), ("dirs", "const double*", "*const f64", C.c_void_p),
                 ("rotations", "const double*", "*const f64", C.c_void_p), ("bias", "double", "f64", C.c_double), ("max_toi", "double", "f64", C.c_double)]
EPS = 1e-15  # the issue's bound on the frame, d . n and |d|


# ---- shared with the GPU tests ------------------------------------------------------------------------------------------------------------------------
def fold(filters, lit):
    """The fold of the definition on per-ray results (n, k, 3) float32 / (n, k) bool: f32 sum in the order of j, blocked rays adding 0, then one division."""
    n, k = lit.shape
    total = np.zeros((n, 3), np.float32)
    for j in range(k):
        total = total + np.where(lit[:, j, None], filters[:, j].astype(np.float32), np.float32(0.0))
    return total / np.float32(k), lit.sum(axis=1).astype(np.uint32)


def unit_normals(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.sqrt((v * v).sum(axis=1))[:, None]


def quad_scene():
    from tests.test_shade_points_gpu import quad_scene as q  # (a scene builder only; nothing of that module runs here)
    return q()


def _surface_points(sc, o, d):
    """Points and outward (towards the ray's side) normals at the oracle's closest hits of the rays."""
    hit, rec = oracle.cast(sc.descriptor, o, d)
    o, d, rec = o[hit], d[hit], rec[hit]
    p = o + d * rec[:, 0:1]
    nm = rec[:, 1:4]
    facing = (nm[:, 0] * d[:, 0] + nm[:, 1] * d[:, 1]) + nm[:, 2] * d[:, 2]
    return np.ascontiguousarray(p), np.ascontiguousarray(np.where((facing > 0)[:, None], -nm, nm)), rec[:, 7].astype(int)


def _analytic_case():
    """rich_analytic_scene (tests/test_shade_points.py): half-transparent nodes, so that the filters are not only 0 and 1.  120 points x 8 directions, 5 rotations, +inf."""
    sc, _ = rich_analytic_scene()
    o, d = scattered_rays(np.random.default_rng(31), 400)
    p, nm, node = _surface_points(sc, o, d)
    assert len(p) >= 120
    keys = np.random.default_rng(32).integers(0, 2**63, size=120, dtype=np.int64).astype(np.uint64)
    return dict(scene=sc, points=p[:120], normals=nm[:120], keys=keys, sample_dirs=nr.hemisphere_dirs(8), rotations=nr.rotation_table(5), bias=1e-3, max_toi=math.inf)


def _quad_case():
    """The alpha-mapped quad scene (tests/test_shade_points_gpu.py): floor points under the occluder's opacity map.  100 points x 10 directions, no rotation, finite max_toi."""
    sc, cam = quad_scene()
    proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], 16, 16)
    o, d, _ = nr.camera_rays((16, 16), cam["eye"], proj, seed=1)
    p, nm, node = _surface_points(sc, o, d)
    sel = np.flatnonzero(node == 0)[:80].tolist() + np.flatnonzero(node == 1)[:20].tolist()
    assert len(sel) == 100
    return dict(scene=sc, points=p[sel], normals=nm[sel], keys=None, sample_dirs=nr.hemisphere_dirs(10, cosine=False), rotations=None, bias=1e-3, max_toi=3.0)


_ORACLE = {}


def oracle_case(name):
    """Per scene, computed once and left unchanged: the arguments of occlusion_points and what the CPU oracle expects — the mirror's rays (at most 2 000 over the
    two scenes) through nrays_oracle_shadow, folded in numpy f32."""
    if name not in _ORACLE:
        c = {"analytic": _analytic_case, "quads": _quad_case}[name]()
        ro, rd = nr.occlusion_rays(c["points"], c["normals"], c["sample_dirs"], c["rotations"], c["bias"], c["keys"])
        n, k = ro.shape[:2]
        filt, lit = np.zeros((n, k, 3), np.float32), np.zeros((n, k), bool)
        desc = c["scene"].descriptor
        for i in range(n):
            for j in range(k):
                f = oracle.shadow(desc, ro[i, j], rd[i, j], c["max_toi"])
                if f is not None:
                    filt[i, j], lit[i, j] = f, True
        c["filter"], c["open"] = fold(filt, lit)
        c["ray_filters"], c["ray_lit"] = filt, lit
        _ORACLE[name] = c
    return _ORACLE[name]


def call_args(c):
    return {k: c[k] for k in ("points", "normals", "sample_dirs", "rotations", "bias", "max_toi", "keys")}


# ---- the mirror against the definition's promises -------------------------------------------------------------------------------------------------------
SPECIAL_NORMALS = np.asarray([(0.0, 0.0, 1.0), (0.0, 0.0, -1.0), (1.0, 0.0, -0.0), (0.0, -1.0, 0.0), (0.6, 0.0, -0.8)])


def _normals():
    return np.concatenate([unit_normals(np.random.default_rng(7), 20000), SPECIAL_NORMALS])


def _frame(nm):
    """t and u of the definition, recovered from the mirror: the rays of the local x and y axes without rotation or bias."""
    _, d = nr.occlusion_rays(np.zeros_like(nm), nm, [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0)], None, 0.0)
    return d[:, 0], d[:, 1]


def test_frames_are_orthonormal_and_right_handed():
    nm = _normals()
    t, u = _frame(nm)
    dot = lambda a, b: (a * b).sum(axis=1)  # noqa: E731
    for a, b, want in ((t, t, 1.0), (u, u, 1.0), (t, u, 0.0), (t, nm, 0.0), (u, nm, 0.0)):
        assert float(np.abs(dot(a, b) - want).max()) <= EPS
    det = dot(np.cross(t, u), nm)
    assert float(np.abs(det - 1.0).max()) <= EPS
    assert np.isfinite(t).all() and np.isfinite(u).all()
    # the definition, spelled out once more on one normal
    nx, ny, nz = 0.6, 0.0, -0.8
    s, a = -1.0, -1.0 / (-1.0 + nz)
    assert t[-1].tolist() == [1.0 + s * nx * nx * a, s * (nx * ny * a), -s * nx] and u[-1].tolist() == [nx * ny * a, s + ny * ny * a, -ny]
    assert t[-3].tolist() == [0.0, 0.0, 1.0] and u[-3].tolist() == [0.0, -1.0, 0.0]  # (1, 0, -0.0): copysign reads the sign bit, s = -1


def test_direction_keeps_its_cosine_and_its_length():
    nm = _normals()
    L = np.concatenate([nr.hemisphere_dirs(16), nr.hemisphere_dirs(7, cosine=False)])
    keys = np.random.default_rng(8).integers(0, 2**63, size=len(nm), dtype=np.int64).astype(np.uint64)
    for rot in (None, nr.rotation_table(5)):
        o, d = nr.occlusion_rays(np.zeros_like(nm), nm, L, rot, 0.25, keys)
        assert o.shape == d.shape == (len(nm), len(L), 3)
        assert float(np.abs((d * nm[:, None, :]).sum(axis=2) - L[None, :, 2]).max()) <= EPS   # d . n = lz
        assert float(np.abs(np.sqrt((d * d).sum(axis=2)) - 1.0).max()) <= EPS                 # | |d| - 1 |
        assert np.array_equal(o, np.broadcast_to((nm * 0.25)[:, None, :], o.shape))           # p + n * bias, per component
    assert float(np.abs(np.sqrt((L * L).sum(axis=1)) - 1.0).max()) <= 2.3e-16 and (L[:, 2] > 0).all()


def test_rotation_index_is_the_hash_of_the_key():
    rng = np.random.default_rng(9)
    nm = unit_normals(rng, 500)
    keys = rng.integers(0, 2**63, size=500, dtype=np.int64).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    R = 5
    table = np.stack([np.arange(R) + 2.0, np.arange(R) * 0.5 - 1.0], axis=1)  # not rotations at all: any values are valid, and these identify their row
    t, u = _frame(nm)
    lx, ly = 0.75, -0.5
    _, d = nr.occlusion_rays(np.zeros_like(nm), nm, [(lx, ly, 0.0)], table, 0.0, keys)
    x, y = (d[:, 0] * t).sum(axis=1), (d[:, 0] * u).sum(axis=1)
    r = (_rng_hash(keys, SALT_OCCLUSION) % np.uint64(R)).astype(int)
    assert SALT_OCCLUSION == 0x300 << 32 and set(r) == set(range(R))
    c, s = table[r, 0], table[r, 1]
    assert float(np.abs(x - (c * lx - s * ly)).max()) <= 1e-14 and float(np.abs(y - (s * lx + c * ly)).max()) <= 1e-14
    # default keys: point i has key i
    _, d0 = nr.occlusion_rays(np.zeros_like(nm), nm, [(lx, ly, 0.0)], table, 0.0)
    _, d1 = nr.occlusion_rays(np.zeros_like(nm), nm, [(lx, ly, 0.0)], table, 0.0, np.arange(500))
    assert np.array_equal(d0, d1) and not np.array_equal(d0, d)
    # the hash itself, once, by hand: mix((key ^ salt * golden) + c)
    z = ((7 ^ ((SALT_OCCLUSION * 0x9E3779B97F4A7C15) & (2**64 - 1))) + 0xD1B54A32D192ED03) & (2**64 - 1)
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & (2**64 - 1)
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & (2**64 - 1)
    assert int(_rng_hash(np.asarray([7], np.uint64), SALT_OCCLUSION)[0]) == z ^ (z >> 31)


def test_no_rotations_leave_the_local_direction_untouched():
    nm = _normals()
    t, u = _frame(nm)
    L = np.asarray([(0.3, -0.4, 0.5), (-0.0, 0.0, 1.0)])
    for rot in (None, np.zeros((0, 2))):
        _, d = nr.occlusion_rays(np.zeros_like(nm), nm, L, rot, 0.0, np.arange(len(nm)) * 977)
        for j, (lx, ly, lz) in enumerate(L):
            assert np.array_equal(d[:, j], (lx * t + ly * u) + lz * nm)  # x = lx and y = ly exactly: no c * lx - s * ly in between
    ident = nr.occlusion_rays(np.zeros_like(nm), nm, L, [(1.0, 0.0)], 0.0)[1]
    assert np.array_equal(ident[:, 0], d[:, 0])  # (the identity rotation gives the same values here; -0.0 components are why R = 0 is not computed that way)


def test_table_builders():
    L = nr.hemisphere_dirs(64)
    assert L.shape == (64, 3) and L.dtype == np.float64 and abs(float(L[:, 2].mean()) - 2.0 / 3.0) < 0.01  # cosine-weighted: E[z] = 2/3
    assert abs(float(nr.hemisphere_dirs(64, cosine=False)[:, 2].mean()) - 0.5) < 0.01
    rot = nr.rotation_table(8)
    assert rot.shape == (8, 2) and np.allclose((rot * rot).sum(axis=1), 1.0) and rot[0].tolist() == [1.0, 0.0]
    for bad in (0, 1025):
        with pytest.raises(ValueError):
            nr.hemisphere_dirs(bad)
        with pytest.raises(ValueError):
            nr.rotation_table(bad)


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
    assert args[EXPECTED[name].index("const NraysOcclusionParams*")] is C.POINTER(abi.NraysOcclusionParams)
    m = re.search(r"pub fn %s\((.*?)\) -> c_int;" % name, FFI)
    assert m, "%s is not declared in gpu_ffi.rs" % name
    assert [p.split(": ", 1)[1] for p in m.group(1).split(", ")] == [RUST_TYPES[t] for t in EXPECTED[name]]
    assert "pub fn occlusion_points(" in GPU_RS and "pub unsafe fn occlusion_points_device(" in GPU_RS
    assert "nrays_occlusion_points(" in GPU_RS and "nrays_occlusion_points_device(" in GPU_RS


def test_the_params_struct_is_the_same_in_the_header_ctypes_and_rust():
    m = re.search(r"struct NraysOcclusionParams \{(.*?)\};\s*typedef struct NraysOcclusionParams NraysOcclusionParams;", HEADER, re.S)
    assert m, "struct NraysOcclusionParams is not declared in include/nrays_abi.h"
    c_fields = [re.sub(r"\s*\*\s*", "* ", f.strip()).rsplit(" ", 1) for f in m.group(1).split(";") if f.strip()]
    assert [(n, t) for t, n in c_fields] == [(n, t) for n, t, _, _ in STRUCT_FIELDS]
    r = re.search(r"#\[repr\(C\)\]\s*(?:#\[derive[^\]]*\]\s*)?pub struct NraysOcclusionParams \{(.*?)\n\}", FFI, re.S)
    assert r and re.findall(r"pub (\w+): ([^,]+),", r.group(1)) == [(n, t) for n, _, t, _ in STRUCT_FIELDS]
    assert [(n, t) for n, t in abi.NraysOcclusionParams._fields_] == [(n, t) for n, _, _, t in STRUCT_FIELDS]
    assert C.sizeof(abi.NraysOcclusionParams) == 40 and abi.NraysOcclusionParams.dirs.offset == 8 and abi.NraysOcclusionParams.max_toi.offset == 32


def test_the_abi_version_is_still_7(built):
    assert re.search(r"#define NRAYS_ABI_VERSION 7\b", HEADER) and abi.ABI_VERSION == 7 and abi.load_hip_lib().nrays_abi_version() == 7
    note = re.search(r"Added after 7 WITHOUT a bump.*?\*/", HEADER_TEXT, re.S).group(0)
    exported = subprocess.check_output(["nm", "-D", "--defined-only", abi.HIP_LIB_PATH]).decode()
    for name in EXPECTED:
        assert re.search(r"%s\b" % name, note), name
        assert (" T " + name + "\n") in exported, name
        assert getattr(abi.load_hip_lib(), name).argtypes == abi.HIP_SYMBOLS[name][1]


def test_without_a_scene_every_call_is_a_bad_arg(built):
    """Without a scene nothing else is looked at; the other arguments one by one need a scene: tests/test_occlusion_gpu.py."""
    lib = abi.load_hip_lib()
    a = (C.c_double * 3)(0.0, 0.0, 1.0)
    out, opened, rays = (C.c_float * 3)(7.0, 7.0, 7.0), (C.c_uint32 * 1)(7), (C.c_double * 3)(7.0, 7.0, 7.0)
    params = abi.NraysOcclusionParams(1, 0, C.addressof(a), None, 1e-3, math.inf)
    adr = C.addressof
    for n in (0, 1):
        for flags in (0, 1):
            assert lib.nrays_occlusion_points(None, n, a, a, None, None, C.byref(params), out, opened, flags) == abi.ERR_BAD_ARG
            assert lib.nrays_occlusion_points_device(None, n, adr(a), adr(a), None, None, C.byref(params), adr(out), adr(opened), flags, None) == abi.ERR_BAD_ARG
        assert lib.nrays_debug_occlusion_rays(None, n, a, a, None, C.byref(params), rays, rays) == abi.ERR_BAD_ARG
    assert lib.nrays_last_error() and list(out) == [7.0] * 3 and opened[0] == 7 and list(rays) == [7.0] * 3


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


def test_occlusion_points_rejects_bad_arguments_before_any_library_call(no_library):
    import torch
    sc = _NoDevice()
    t3 = torch.zeros((4, 3), dtype=torch.float64)
    bad = [
        dict(points=np.zeros((4, 2))), dict(points=np.zeros(12)), dict(points=None), dict(normals=None), dict(normals=np.zeros((5, 3))),
        dict(points=np.zeros((4, 3), np.int64)), dict(normals=np.zeros((4, 3), np.int32)),
        dict(sample_dirs=None), dict(sample_dirs=np.zeros((0, 3))), dict(sample_dirs=np.zeros((1025, 3))), dict(sample_dirs=np.zeros((4, 2))), dict(sample_dirs=np.zeros(12)),
        dict(rotations=np.zeros((1025, 2))), dict(rotations=np.zeros((3, 3))), dict(rotations=np.zeros(4)),
        dict(bias=math.inf), dict(bias=math.nan), dict(max_toi=0.0), dict(max_toi=-1.0), dict(max_toi=math.nan),
        dict(hit_flags=np.ones(3, np.uint32)), dict(hit_flags=np.ones(4, np.float32)), dict(keys=np.zeros(5, np.uint64)), dict(keys=np.zeros(4, np.float64)),
        dict(normals=t3),                                          # numpy and torch mixed
        dict(sample_dirs=torch.zeros((4, 3), dtype=torch.float64)),
        dict(points=t3, normals=t3),                               # torch tensors on the host
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            nr.occlusion_points(sc, **dict(_good(), **kw))
    with pytest.raises(ValueError):
        nr.Scene([], []).occlusion_points(np.zeros((4, 2)), _good()["normals"], _good()["sample_dirs"])
    with pytest.raises(AssertionError, match="library was loaded"):  # a well-formed call gets as far as the library
        nr.occlusion_points(sc, rotations=nr.rotation_table(3), max_toi=math.inf, hit_flags=np.ones(4, np.uint32), keys=np.arange(4), **_good())
    with pytest.raises(AssertionError, match="library was loaded"):
        nr.occlusion_points(sc, rotations=np.zeros((0, 2)), bias=0.0, max_toi=1e-300, **_good())


def test_occlusion_hits_refuses_incomplete_hits_and_flips_the_normals(no_library, monkeypatch):
    sc = _NoDevice()
    o, d = np.zeros((4, 3)), np.tile([0.0, 0.0, 1.0], (4, 1))
    normal = np.asarray([(0.0, 0.0, -1.0), (0.0, 0.0, 1.0), (0.6, 0.0, 0.8), (1.0, 0.0, 0.0)])
    full = nr.CastHits(toi=np.asarray([1.0, 2.0, 3.0, 4.0]), node=np.zeros(4, np.int32), normal=normal, uv=None, prim=None, flags=np.asarray([1, 3, 1, 0], np.uint32))
    L = nr.hemisphere_dirs(4)
    for name in ("normal", "flags"):
        with pytest.raises(ValueError, match=name):
            nr.occlusion_hits(sc, o, d, full._replace(**{name: None}), L)
    with pytest.raises(ValueError):
        nr.occlusion_hits(sc, o[:3], d, full, L)
    with pytest.raises(AssertionError, match="library was loaded"):  # uv and prim are not needed
        nr.occlusion_hits(sc, o, d, full, L)
    from nrays_amd import scenefile
    assert callable(nr.Scene.occlusion_points) and callable(scenefile.FileScene.occlusion_points) and nr.occlusion_points is nr.scene.occlusion_points
    seen = {}
    monkeypatch.setattr(nr.scene, "occlusion_points", lambda scene, points, normals, *a, **kw: seen.update(points=points, normals=normals, kw=kw) or "result")
    assert nr.occlusion_hits(sc, o, d, full, L, keys=np.arange(4)) == "result"
    assert np.array_equal(seen["points"], [(0, 0, 1), (0, 0, 2), (0, 0, 3), (0, 0, 0)])  # origins + dirs * toi, toi 0 at the miss
    assert np.array_equal(seen["normals"], [(0, 0, -1), (0, 0, -1), (-0.6, 0, -0.8), (1, 0, 0)])  # negated where n . d > 0
    assert np.array_equal(seen["kw"]["hit_flags"], full.flags) and np.array_equal(seen["kw"]["keys"], np.arange(4))


# ---- the expected values from the oracle ----------------------------------------------------------------------------------------------------------------
def test_oracle_expectations():
    a, q = oracle_case("analytic"), oracle_case("quads")
    assert a["ray_lit"].size + q["ray_lit"].size <= 2000
    for c in (a, q):
        n, k = c["ray_lit"].shape
        assert c["filter"].shape == (n, 3) and c["filter"].dtype == np.float32 and c["open"].dtype == np.uint32
        assert np.array_equal(c["open"], c["ray_lit"].sum(axis=1)) and 0 < c["open"].min() + 1 and c["open"].max() <= k
        assert (c["filter"] >= 0.0).all() and (c["filter"] <= 1.0).all()
        assert (c["filter"][c["open"] == 0] == 0.0).all()
        assert 0.2 < c["ray_lit"].mean() < 0.98  # (blocked and open rays both)
    # filters that are neither 0 nor 1: the analytic scene's half-transparent nodes, the quad scene's opacity map and colour texture
    for c in (a, q):
        f = c["ray_filters"][c["ray_lit"]]
        assert ((f > 0.0) & (f < 1.0)).any(axis=1).sum() >= 10
    # a fully open point of the analytic case: every filter (1, 1, 1), the mean exactly 1
    full = a["open"] == a["ray_lit"].shape[1]
    untouched = full & (a["ray_filters"] == 1.0).all(axis=(1, 2))
    assert untouched.any() and (a["filter"][untouched] == 1.0).all()
