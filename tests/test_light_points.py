"""Direct light at caller-supplied points from a caller-supplied table of point lights (nrays_light_points_device / nrays_light_points / nrays_debug_light_rays;
nrays_amd.light_points, light_hits, light_rays, light_points_ref, scene_point_lights, vpls_from_hits), the parts that need no GPU: the header, the ctypes table and
the Rust declarations, the argument checks, the numpy mirror of the ray definition against the properties the definition promises, the closed form of one light
over a plane — and the expected values of two small scenes from the CPU oracle alone (the mirror's rays through nrays_oracle_shadow, folded in numpy f32), which
tests/test_light_points_gpu.py imports."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import nrays_amd as nr
import oracle
from nrays_amd import abi
from tests.test_occlusion import SPECIAL_NORMALS, oracle_case, unit_normals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_TEXT = open(os.path.join(ROOT, "include", "nrays_abi.h")).read()
HEADER = re.sub(r"/\*.*?\*/", "", HEADER_TEXT, flags=re.S)
FFI = open(os.path.join(ROOT, "integration", "rust", "src", "gpu_ffi.rs")).read()
GPU_RS = open(os.path.join(ROOT, "integration", "rust", "src", "gpu.rs")).read()
_IN = ["NraysScene*", "uint32_t", "const double*", "const double*", "const uint32_t*", "const NraysPointLights*", "float*", "uint32_t*", "uint32_t"]
EXPECTED = {"nrays_light_points_device": _IN + ["void*"], "nrays_light_points": _IN,
            "nrays_debug_light_rays": ["NraysScene*", "uint32_t", "const double*", "const double*", "const NraysPointLights*", "double*", "double*", "double*", "float*"]}
RUST_TYPES = {"NraysScene*": "*mut NraysScene", "uint32_t": "u32", "const double*": "*const f64", "const uint32_t*": "*const u32",
              "const NraysPointLights*": "*const NraysPointLights", "float*": "*mut f32", "uint32_t*": "*mut u32", "double*": "*mut f64", "void*": "*mut c_void"}
STRUCT_FIELDS = [("num_lights", "uint32_t", "u32", C.c_uint32), ("flags", "uint32_t", "u32", C.c_uint32), ("positions", "const double*", "*const f64", C.c_void_p),
                 ("colors", "const float*", "*const f32", C.c_void_p), ("normals", "const double*", "*const f64", C.c_void_p), ("bias", "double", "f64", C.c_double),
                 ("offset", "double", "f64", C.c_double), ("min_dist", "double", "f64", C.c_double)]
UP = np.asarray([(0.0, 1.0, 0.0)])
F32_EPS = 2.0 ** -24  # half an ulp of a float32 in [1, 2): the relative error of one rounding


# ---- shared with the GPU tests ------------------------------------------------------------------------------------------------------------------------
def fold(colors, w, filters, open_):
    """The fold of the definition on per-(point, light) results: colors (m, 3) f32, w (n, m) f32, filters (n, m, 3) f32, open_ (n, m) bool -> the f32 sum in the
    order of k of col * (filter * w) over the open lights."""
    n, m = w.shape
    total = np.zeros((n, 3), np.float32)
    for k in range(m):
        c = colors[k][None, :] * (filters[:, k].astype(np.float32) * w[:, k, None])
        total = np.where(open_[:, k, None], total + c, total)
    return total


def oracle_lights(name):
    """Lights chosen so that every fate of a (point, light) pair is well represented (test_oracle_expectations asserts the shares): lights close above the quad
    scene's occluder or inside the analytic scene's shapes (blocked, or filtered by an opacity map or a half-transparent node), lights in the open, and lights
    below the floor (skipped: behind the surface).  Inverse-square falloff with a clamp that some of the pairs reach."""
    rng = np.random.default_rng({"analytic": 51, "quads": 52}[name])
    if name == "quads":
        pos = np.concatenate([rng.uniform((-0.9, 1.05, -0.9), (0.9, 1.7, 0.9), size=(6, 3)), rng.uniform((-4.5, 0.15, -4.5), (4.5, 0.9, 4.5), size=(3, 3)),
                              rng.uniform((-2.0, 2.5, -2.0), (2.0, 5.0, 2.0), size=(2, 3)), rng.uniform((-2.0, -3.0, -2.0), (2.0, -0.5, 2.0), size=(4, 3))])
    else:
        inside = np.asarray([(1.3, 0.0, 0.5), (1.2, 0.2, 0.4), (0.3, -0.6, -1.8), (-1.2, 0.0, 0.0), (0.2, 0.9, 1.8), (2.8, -0.4, -0.5)])
        pos = np.concatenate([inside, rng.uniform((-6.0, 2.0, -6.0), (6.0, 7.0, 6.0), size=(6, 3)), rng.uniform((-3.0, -4.0, -3.0), (3.0, -1.5, 3.0), size=(1, 3))])
    col = rng.uniform(0.1, 1.0, size=(len(pos), 3)).astype(np.float32)
    return nr.PointLights(pos, col, None, True, 0.25, 1e-3, 1e-3)


_ORACLE = {}


def light_oracle_case(name):
    """Per scene, computed once and left unchanged: the scene and points of tests/test_occlusion.py's oracle case, the lights, and what the CPU oracle expects —
    the mirror's rays with a weight (at most 1 900 per scene) through nrays_oracle_shadow, folded in numpy f32."""
    if name not in _ORACLE:
        base = oracle_case(name)
        c = dict(scene=base["scene"], points=base["points"], normals=base["normals"], lights=oracle_lights(name))
        ro, rd, t_max, w = nr.light_rays(c["points"], c["normals"], c["lights"])
        n, m = w.shape
        ray = w > 0
        open_, filt = ray.copy(), np.ones((n, m, 3), np.float32)
        desc = c["scene"].descriptor
        for i, k in zip(*np.nonzero(ray & (t_max > 0.0))):
            f = oracle.shadow(desc, ro[i, k], rd[i, k], t_max[i, k])
            open_[i, k] = f is not None
            if f is not None:
                filt[i, k] = f
        col = np.asarray(c["lights"].colors, np.float32)
        c.update(w=w, ray=ray, open=open_, ray_filters=filt, rgb=fold(col, w, filt, open_),
                 counts=np.stack([ray.sum(axis=1), open_.sum(axis=1)], axis=1).astype(np.uint32),
                 scale=(np.abs(col)[None, :, :] * (w * open_)[:, :, None].astype(np.float64)).sum(axis=1))  # sum over the open lights of |col_k| * w_k, per channel
        _ORACLE[name] = c
    return _ORACLE[name]


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
    assert args[EXPECTED[name].index("const NraysPointLights*")] is C.POINTER(abi.NraysPointLights)
    m = re.search(r"pub fn %s\((.*?)\) -> c_int;" % name, FFI)
    assert m, "%s is not declared in gpu_ffi.rs" % name
    assert [p.split(": ", 1)[1] for p in m.group(1).split(", ")] == [RUST_TYPES[t] for t in EXPECTED[name]]
    assert "pub fn light_points(" in GPU_RS and "pub unsafe fn light_points_device(" in GPU_RS
    assert "nrays_light_points(" in GPU_RS and "nrays_light_points_device(" in GPU_RS


def test_the_lights_struct_is_the_same_in_the_header_ctypes_and_rust():
    m = re.search(r"struct NraysPointLights \{(.*?)\};\s*typedef struct NraysPointLights NraysPointLights;", HEADER, re.S)
    assert m, "struct NraysPointLights is not declared in include/nrays_abi.h"
    c_fields = [re.sub(r"\s+", " ", re.sub(r"\s*\*\s*", "* ", f.strip())).rsplit(" ", 1) for f in m.group(1).split(";") if f.strip()]
    assert [(n, t) for t, n in c_fields] == [(n, t) for n, t, _, _ in STRUCT_FIELDS]
    r = re.search(r"#\[repr\(C\)\]\s*(?:#\[derive[^\]]*\]\s*)?pub struct NraysPointLights \{(.*?)\n\}", FFI, re.S)
    assert r and re.findall(r"pub (\w+): ([^,]+),", r.group(1)) == [(n, t) for n, _, t, _ in STRUCT_FIELDS]
    assert [(n, t) for n, t in abi.NraysPointLights._fields_] == [(n, t) for n, _, _, t in STRUCT_FIELDS]
    assert C.sizeof(abi.NraysPointLights) == 56 and abi.NraysPointLights.positions.offset == 8 and abi.NraysPointLights.min_dist.offset == 48
    assert re.search(r"#define NRAYS_LIGHTS_INVERSE_SQUARE 1u\b", HEADER) and abi.LIGHTS_INVERSE_SQUARE == 1 and abi.LIGHTS_MAX == 4096
    assert re.search(r"pub const NRAYS_LIGHTS_INVERSE_SQUARE: u32 = 1;", FFI)


def test_the_abi_version_is_still_7_and_the_symbols_are_exported(built):
    assert re.search(r"#define NRAYS_ABI_VERSION 7\b", HEADER) and abi.ABI_VERSION == 7 and abi.load_hip_lib().nrays_abi_version() == 7
    note = re.search(r"Added after 7 WITHOUT a bump.*?\*/", HEADER_TEXT, re.S).group(0)
    exported = subprocess.check_output(["nm", "-D", "--defined-only", abi.HIP_LIB_PATH]).decode()
    for name in EXPECTED:
        assert re.search(r"%s\b" % name, note), name
        assert (" T " + name + "\n") in exported, name
        assert getattr(abi.load_hip_lib(), name).argtypes == abi.HIP_SYMBOLS[name][1]


BAD_LIGHTS = [dict(positions=None), dict(colors=None), dict(num_lights=0), dict(num_lights=4097), dict(flags=2), dict(flags=3), dict(flags=1 << 31), dict(bias=math.inf),
              dict(bias=math.nan), dict(offset=-1e-9), dict(offset=math.inf), dict(offset=math.nan), dict(flags=1, min_dist=0.0), dict(flags=1, min_dist=-1.0),
              dict(flags=1, min_dist=math.inf), dict(flags=1, min_dist=math.nan)]


def lights_struct(pos, col, **kw):
    """An NraysPointLights over two ctypes / numpy tables with good settings, then `kw`."""
    adr = lambda a: None if a is None else (a.ctypes.data if isinstance(a, np.ndarray) else C.addressof(a))  # noqa: E731
    f = dict(num_lights=1, flags=0, positions=pos, colors=col, normals=None, bias=1e-3, offset=1e-3, min_dist=1.0)
    f.update(kw)
    return abi.NraysPointLights(f["num_lights"], f["flags"], adr(f["positions"]), adr(f["colors"]), adr(f["normals"]), f["bias"], f["offset"], f["min_dist"])


def test_without_a_scene_every_call_is_a_bad_arg(built):
    """Without a scene nothing else is looked at, whatever else is wrong; the other arguments one by one need a scene: tests/test_light_points_gpu.py."""
    lib = abi.load_hip_lib()
    a, col = (C.c_double * 3)(0.0, 0.0, 1.0), (C.c_float * 3)(1.0, 1.0, 1.0)
    out, counts = (C.c_float * 3)(7.0, 7.0, 7.0), (C.c_uint32 * 2)(7, 7)
    rays, tm, w = (C.c_double * 3)(7.0, 7.0, 7.0), (C.c_double * 1)(7.0), (C.c_float * 1)(7.0)
    adr = C.addressof
    for kw in [dict()] + BAD_LIGHTS:
        st = lights_struct(a, col, **kw)
        for n in (0, 1):
            for flags in (0, 1):
                assert lib.nrays_light_points(None, n, a, a, None, C.byref(st), out, counts, flags) == abi.ERR_BAD_ARG
                assert lib.nrays_light_points_device(None, n, adr(a), adr(a), None, C.byref(st), adr(out), adr(counts), flags, None) == abi.ERR_BAD_ARG
            assert lib.nrays_debug_light_rays(None, n, a, a, C.byref(st), rays, rays, tm, w) == abi.ERR_BAD_ARG
    assert lib.nrays_light_points(None, 1, a, a, None, None, out, counts, 0) == abi.ERR_BAD_ARG
    assert lib.nrays_last_error() and list(out) == [7.0] * 3 and list(counts) == [7, 7] and list(rays) == [7.0] * 3 and tm[0] == 7.0 and w[0] == 7.0


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


def _good(n=4, m=3):
    return dict(points=np.zeros((n, 3)), normals=np.tile([0.0, 1.0, 0.0], (n, 1)), lights=nr.PointLights(np.ones((m, 3)), np.ones((m, 3), np.float32)))


def test_light_points_rejects_bad_arguments_before_any_library_call(no_library):
    import torch
    sc = _NoDevice()
    t3 = torch.zeros((4, 3), dtype=torch.float64)
    L = _good()["lights"]
    bad = [
        dict(points=np.zeros((4, 2))), dict(points=np.zeros(12)), dict(points=None), dict(normals=None), dict(normals=np.zeros((5, 3))),
        dict(points=np.zeros((4, 3), np.int64)), dict(normals=np.zeros((4, 3), np.int32)),
        dict(lights=None), dict(lights=(L.positions, L.colors)), dict(lights=L._replace(positions=None)), dict(lights=L._replace(colors=None)),
        dict(lights=L._replace(positions=np.zeros((0, 3)))), dict(lights=L._replace(positions=np.zeros((4097, 3)), colors=np.zeros((4097, 3)))),
        dict(lights=L._replace(positions=np.zeros((3, 2)))), dict(lights=L._replace(positions=np.zeros(9))), dict(lights=L._replace(colors=np.zeros((2, 3)))),
        dict(lights=L._replace(colors=np.zeros((3, 4)))), dict(lights=L._replace(normals=np.zeros((2, 3)))), dict(lights=L._replace(positions=np.zeros((3, 3), "U1"))),
        dict(lights=L._replace(bias=math.inf)), dict(lights=L._replace(bias=math.nan)), dict(lights=L._replace(offset=-1.0)), dict(lights=L._replace(offset=math.inf)),
        dict(lights=L._replace(inverse_square=True, min_dist=0.0)), dict(lights=L._replace(inverse_square=True, min_dist=math.inf)),
        dict(lights=L._replace(inverse_square=True, min_dist=math.nan)),
        dict(hit_flags=np.ones(3, np.uint32)), dict(hit_flags=np.ones(4, np.float32)),
        dict(normals=t3),                                                      # numpy and torch mixed
        dict(lights=L._replace(positions=torch.ones((3, 3), dtype=torch.float64))),
        dict(points=t3, normals=t3),                                           # torch tensors on the host
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            nr.light_points(sc, **dict(_good(), **kw))
    with pytest.raises(ValueError):
        nr.Scene([], []).light_points(np.zeros((4, 2)), _good()["normals"], L)
    for mirror in (nr.light_rays, lambda *a: nr.light_points_ref(sc, *a)):
        with pytest.raises(ValueError):
            mirror(np.zeros((4, 2)), _good()["normals"], L)
        with pytest.raises(ValueError):
            mirror(np.zeros((4, 3)), _good()["normals"], L._replace(offset=-1.0))
    with pytest.raises(AssertionError, match="library was loaded"):  # a well-formed call gets as far as the library
        nr.light_points(sc, hit_flags=np.ones(4, np.uint32), want_counts=False, **_good())
    with pytest.raises(AssertionError, match="library was loaded"):  # min_dist is unread without the falloff; the tables may be lists
        nr.light_points(sc, np.zeros((4, 3)), _good()["normals"], nr.PointLights([(0, 1, 0)], [(1, 2, 3)], [(0, -1, 0)], False, math.nan, 0.0, 0.0))
    with pytest.raises(AssertionError, match="library was loaded"):
        nr.light_ray_probe(sc, **_good())


def test_light_hits_refuses_incomplete_hits_and_flips_the_normals(no_library, monkeypatch):
    sc = _NoDevice()
    o, d = np.zeros((4, 3)), np.tile([0.0, 0.0, 1.0], (4, 1))
    normal = np.asarray([(0.0, 0.0, -1.0), (0.0, 0.0, 1.0), (0.6, 0.0, 0.8), (1.0, 0.0, 0.0)])
    full = nr.CastHits(toi=np.asarray([1.0, 2.0, 3.0, 4.0]), node=np.zeros(4, np.int32), normal=normal, uv=None, prim=None, flags=np.asarray([1, 3, 1, 0], np.uint32))
    L = _good()["lights"]
    for name in ("normal", "flags"):
        with pytest.raises(ValueError, match=name):
            nr.light_hits(sc, o, d, full._replace(**{name: None}), L)
    with pytest.raises(ValueError):
        nr.light_hits(sc, o[:3], d, full, L)
    with pytest.raises(AssertionError, match="library was loaded"):  # uv and prim are not needed
        nr.light_hits(sc, o, d, full, L)
    from nrays_amd import scenefile
    assert callable(nr.Scene.light_points) and callable(scenefile.FileScene.light_points) and nr.light_points is nr.scene.light_points
    seen = {}
    monkeypatch.setattr(nr.scene, "light_points", lambda scene, points, normals, lights, **kw: seen.update(points=points, normals=normals, lights=lights, kw=kw) or "result")
    assert nr.light_hits(sc, o, d, full, L) == "result" and seen["lights"] is L
    assert np.array_equal(seen["points"], [(0, 0, 1), (0, 0, 2), (0, 0, 3), (0, 0, 0)])  # origins + dirs * toi, toi 0 at the miss
    assert np.array_equal(seen["normals"], [(0, 0, -1), (0, 0, -1), (-0.6, 0, -0.8), (1, 0, 0)])  # negated where n . d > 0
    assert np.array_equal(seen["kw"]["hit_flags"], full.flags)


# ---- the mirror against the definition's promises -------------------------------------------------------------------------------------------------------
def mirror_inputs(seed=7, n=3000, m=24):
    """Random unit normals plus the special ones, points in a box, lights around them with unit emitter normals."""
    rng = np.random.default_rng(seed)
    nm = np.concatenate([unit_normals(rng, n), SPECIAL_NORMALS])
    p = rng.uniform(-5.0, 5.0, size=(len(nm), 3))
    pos = rng.uniform(-8.0, 8.0, size=(m, 3))
    col = rng.uniform(0.0, 2.0, size=(m, 3)).astype(np.float32)
    return p, nm, pos, col, unit_normals(rng, m)


@pytest.mark.parametrize("emitters", [False, True])
@pytest.mark.parametrize("falloff", [False, True])
def test_mirror_direction_and_weight(emitters, falloff):
    p, nm, pos, col, en = mirror_inputs()
    bias, offset, min_dist = 0.37, 1e-3, 3.0  # (a clamp that a good part of the pairs reach)
    L = nr.PointLights(pos, col, en if emitters else None, falloff, min_dist, bias, offset)
    o, d, t_max, w = nr.light_rays(p, nm, L)
    n, m = len(p), len(pos)
    assert o.shape == d.shape == (n, m, 3) and t_max.shape == w.shape == (n, m) and o.dtype == d.dtype == t_max.dtype == np.float64 and w.dtype == np.float32
    length = np.sqrt((d * d).sum(axis=2))
    assert float(np.abs(length - 1.0).max()) <= 2 * 2.0 ** -52  # |ldir| within 2 ulp of 1
    q = (p + nm * bias)[:, None, :]
    v = pos[None, :, :] - q
    dist = np.sqrt((v * v).sum(axis=2))
    assert np.array_equal(t_max, np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]) - offset)
    assert np.array_equal(o, q + d * offset)
    # the f64 closed form: cos_r * cos_e / max(d^2, min_dist^2); five f32 roundings (cr, ce, g, two products), one to spare
    cos_r = np.maximum((v * nm[:, None, :]).sum(axis=2) / dist, 0.0)
    cos_e = np.maximum(-(v * en[None, :, :]).sum(axis=2) / dist, 0.0) if emitters else 1.0
    closed = cos_r * cos_e / (np.maximum(dist * dist, min_dist * min_dist) if falloff else 1.0)
    sure = closed > 1e-6  # (away from the clamp's edge at 0, where the cosine's own f64 rounding decides the sign)
    assert sure.mean() > (0.15 if emitters else 0.3)
    rel = np.abs(w[sure].astype(np.float64) - closed[sure]) / closed[sure]
    print("emitters %s falloff %s: max relative error of w %.3g (bound %.3g)" % (emitters, falloff, float(rel.max()), 6 * F32_EPS))
    assert float(rel.max()) <= 6 * F32_EPS
    assert (w >= 0).all() and np.isfinite(w).all()
    if falloff:
        assert ((dist < min_dist) & sure).sum() > 100 and ((dist > min_dist) & sure).sum() > 100  # both sides of the clamp


def test_mirror_skips_exactly_what_the_definition_skips():
    nm = np.concatenate([unit_normals(np.random.default_rng(3), 500), SPECIAL_NORMALS])
    n = len(nm)
    p = np.random.default_rng(4).uniform(-3.0, 3.0, size=(n, 3))
    bias = 0.25
    q = p + nm * bias
    t = np.cross(nm, np.roll(nm, 1, axis=1) + 0.5)  # some vector across the normal
    # per point its own lights (one point a call): in the tangent plane, below it, above it, and at q itself
    for i in range(0, n, 7):
        pos = np.stack([q[i] + nm[i] * 0.0 + np.asarray([0.0, 0.0, 0.0]), q[i] - 2.0 * nm[i], q[i] - 0.5 * nm[i] + t[i], q[i] + 2.0 * nm[i], q[i] + nm[i] + t[i]])
        en = np.stack([-nm[i], -nm[i], -nm[i], nm[i], -nm[i]])  # light 3 is above the point but its emitter faces away
        for emit in (None, en):
            o, d, t_max, w = nr.light_rays(p[i:i + 1], nm[i:i + 1], nr.PointLights(pos, np.ones((5, 3), np.float32), emit, False, 1.0, bias, 1e-3))
            assert w[0, 0] == 0 and np.array_equal(o[0, 0], q[i]) and (d[0, 0] == 0).all() and t_max[0, 0] == 0  # a light at q itself: !(nrm > 0)
            assert w[0, 1] == 0 and w[0, 2] == 0  # at or below the tangent plane
            assert (w[0, 3] > 0) == (emit is None)  # a back-facing emitter
            assert w[0, 4] > 0
            assert np.signbit(w[0, :4]).sum() == 0  # skipped is +0
    # exactly in the tangent plane, where the f64 dot is exactly 0: axis-aligned cases
    o, d, t_max, w = nr.light_rays(np.zeros((1, 3)), UP, nr.PointLights([(3.0, 0.0, 0.0), (0.0, 0.0, -2.0), (1.0, 1e-300, 0.0)], np.ones((3, 3)), None, False, 1.0, 0.0, 0.0))
    assert w[0, 0] == 0 and w[0, 1] == 0 and w[0, 2] == 0  # (the third: a positive f64 cosine that rounds to +0 in f32)
    assert np.array_equal(d[0, 0], [1.0, 0.0, 0.0]) and t_max[0, 0] == 3.0  # a skipped light still has the ray of the definition


def test_a_light_within_the_offset_is_open_without_a_ray():
    """t_max <= 0 (step 4): the weight stands, nothing is traversed, the filter is (1, 1, 1) — light_points_ref needs no scene for it."""
    class NoScene:
        def device_handle(self):
            raise AssertionError("nothing may be traced")
    L = nr.PointLights([(0.0, 0.05, 0.0), (0.0, 0.1, 0.0)], [(1.0, 2.0, 3.0), (0.5, 0.5, 0.5)], None, True, 0.5, 0.0, 0.1)
    o, d, t_max, w = nr.light_rays(np.zeros((1, 3)), UP, L)
    assert t_max[0, 0] < 0 and t_max[0, 1] == 0 and (w[0] == np.float32(4.0)).all()
    got = nr.light_points_ref(NoScene(), np.zeros((1, 3)), UP, L)
    assert np.array_equal(got.rgb, [[6.0, 10.0, 14.0]]) and got.counts.tolist() == [[2, 2]]
    skipped = nr.light_points_ref(NoScene(), np.full((1, 3), np.nan), np.full((1, 3), np.nan), L, hit_flags=[2])
    assert (skipped.rgb.view(np.uint32) == 0).all() and skipped.counts.tolist() == [[0, 0]]


def test_closed_form_of_one_light_over_a_plane():
    """One light at height h over the plane y = 0 with the inverse-square falloff and nothing in the way: out = col * h / d^3.  Seven f32 roundings (cr, g, the
    weight's two products, filter * w, col * that, and the +0 sum is exact) and the f64 work far below one f32 ulp: 8 * 2^-24 relative."""
    rng = np.random.default_rng(12)
    h, col = 2.5, np.asarray([0.9, 1.7, 0.3], np.float32)
    p = np.stack([rng.uniform(-6.0, 6.0, 100), np.zeros(100), rng.uniform(-6.0, 6.0, 100)], axis=1)
    nm = np.tile([0.0, 1.0, 0.0], (100, 1))
    L = nr.PointLights([(0.3, h, -0.2)], [col], None, True, 1e-3, 0.0, 1e-3)
    o, d, t_max, w = nr.light_rays(p, nm, L)
    out = fold(np.asarray(L.colors, np.float32), w, np.ones((100, 1, 3), np.float32), w > 0)
    dist = np.sqrt(((np.asarray(L.positions) - p) ** 2).sum(axis=1))
    want = col[None, :].astype(np.float64) * (h / dist ** 3)[:, None]
    rel = np.abs(out - want) / want
    print("closed form: max relative error %.3g (bound %.3g)" % (float(rel.max()), 8 * F32_EPS))
    assert float(rel.max()) <= 8 * F32_EPS and (t_max > 0).all()


# ---- the helpers equal their parts ----------------------------------------------------------------------------------------------------------------------------
def test_scene_point_lights_and_vpls_from_hits_equal_their_parts():
    lights = [nr.Light((2.0, 6.0, -4.0), 0.4, 4, (0.8, 0.8, 0.7)), nr.Light((-4.0, 3.0, -3.0), 0.0, 1, (0.3, 0.25, 0.4)), nr.Light((0.1, 0.2, 0.3), 0.0, 1, (1.0, 2.0, 3.0))]
    sc = nr.Scene([], lights)
    L = nr.scene_point_lights(sc, bias=0.0, offset=1e-3)
    assert np.array_equal(L.positions, [(-4.0, 3.0, -3.0), (0.1, 0.2, 0.3)]) and L.positions.dtype == np.float64  # the area light is left out
    assert np.array_equal(L.colors, np.asarray([(0.3, 0.25, 0.4), (1.0, 2.0, 3.0)], np.float32)) and L.colors.dtype == np.float32
    assert L.normals is None and L.inverse_square is False and L.bias == 0.0 and L.offset == 1e-3
    with pytest.raises(ValueError):
        nr.scene_point_lights(nr.Scene([], lights[:1]))
    # vpls_from_hits
    o = np.asarray([(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)])
    d = np.tile([0.0, 0.0, 1.0], (4, 1))
    normal = np.asarray([(0.0, 0.0, -1.0), (0.0, 0.0, 1.0), (0.6, 0.0, 0.8), (1.0, 0.0, 0.0)])
    hits = nr.CastHits(toi=np.asarray([1.0, 2.0, 3.0, math.inf]), node=np.asarray([0, 1, 2, -1], np.int32), normal=normal, uv=None, prim=None, flags=np.asarray([1, 3, 1, 0], np.uint32))
    diffuse = np.asarray([(0.5, 0.25, 1.0), (0.1, 0.2, 0.3), (1.0, 1.0, 1.0), (9.0, 9.0, 9.0)], np.float32)
    V = nr.vpls_from_hits(o, d, hits, diffuse, 0.3, inverse_square=True, min_dist=0.05)
    assert np.array_equal(V.positions, [(0, 0, 1), (1, 0, 2), (0, 1, 3)])  # origins + dirs * toi at the hits; the miss makes no light
    assert np.array_equal(V.normals, [(0, 0, -1), (0, 0, -1), (-0.6, 0, -0.8)])  # towards the side the ray came from
    assert V.colors.dtype == np.float32 and np.array_equal(V.colors, np.float32(0.3) * diffuse[:3])
    assert V.inverse_square is True and V.min_dist == 0.05 and V.bias == 1e-3 and V.offset == 1e-3
    with pytest.raises(ValueError):
        nr.vpls_from_hits(o, d, hits, diffuse[:3], 0.3)
    with pytest.raises(ValueError, match="normal"):
        nr.vpls_from_hits(o, d, hits._replace(normal=None), diffuse, 0.3)
    assert "closest_hits" in nr.vpls_from_hits.__doc__ and "material_hits" in nr.vpls_from_hits.__doc__ and "light_points" in nr.vpls_from_hits.__doc__


# ---- the expected values from the oracle ----------------------------------------------------------------------------------------------------------------
def test_oracle_expectations():
    for name in ("analytic", "quads"):
        c = light_oracle_case(name)
        n, m = c["w"].shape
        assert c["ray"].sum() <= 1900
        skipped, open_ = ~c["ray"], c["open"]
        blocked_or_filtered = c["ray"] & (~open_ | (c["ray_filters"] != 1.0).any(axis=2))
        clear = open_ & (c["ray_filters"] == 1.0).all(axis=2)
        shares = [float(x.mean()) for x in (skipped, blocked_or_filtered, clear)]
        print("%s: %d points x %d lights: skipped %.3f, blocked or filtered %.3f, open %.3f" % (name, n, m, *shares))
        assert min(shares) >= 0.25 and abs(sum(shares) - 1.0) < 1e-12
        assert (c["ray"] & ~open_).mean() > 0.05 and (open_ & (c["ray_filters"] != 1.0).any(axis=2)).mean() > 0.05  # blocked and filtered both
        assert c["rgb"].shape == (n, 3) and c["rgb"].dtype == np.float32 and c["counts"].dtype == np.uint32 and c["counts"].shape == (n, 2)
        assert (c["counts"][:, 1] <= c["counts"][:, 0]).all() and c["counts"][:, 0].max() <= m and (c["rgb"] >= 0).all()
        assert (c["rgb"][c["counts"][:, 1] == 0] == 0).all() and (c["rgb"][c["counts"][:, 1] > 0] > 0).all()
