"""Probe visibility (nrays_probe_depth_points* and nrays_irradiance_points_vis*; nrays_amd.probe_depth_points, probe_depth, oct_texel, probe_depth_ref,
ProbeVisibility, probe_valid_words, bake_probe_visibility, irradiance_points(visibility=)), the parts that need no GPU: the header, the ctypes table and the Rust
declarations, the two structs' layouts against the C compiler's, the argument checks, and the properties of the definitions on their numpy mirrors — which
tests/test_probe_depth_gpu.py and tests/test_irradiance_vis_gpu.py compare the device with bit for bit."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import nrays_amd as nr
from nrays_amd import abi
from tests.test_gather import FFI, GPU_RS, HEADER, HEADER_TEXT, _NoDevice, _c_params, no_library  # noqa: F401  (no_library is a fixture)
from tests.test_irradiance import random_grid, same, unit_vectors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_DEPTH = ["NraysScene*", "uint32_t", "const double*", "const double*", "const uint32_t*", "const uint64_t*", "const NraysProbeDepthParams*", "float*", "uint32_t*", "double*",
          "uint32_t*", "uint32_t"]
_VIS = ["NraysScene*", "uint32_t", "const double*", "const double*", "const uint32_t*", "const NraysIrradianceGrid*", "const NraysIrradianceVisibility*", "float*", "float*",
        "float*", "uint32_t"]
EXPECTED = {"nrays_probe_depth_points_device": _DEPTH + ["void*"], "nrays_probe_depth_points": _DEPTH,
            "nrays_irradiance_points_vis_device": _VIS + ["void*"], "nrays_irradiance_points_vis": _VIS}
RUST_TYPES = {"NraysScene*": "*mut NraysScene", "uint32_t": "u32", "const double*": "*const f64", "const uint32_t*": "*const u32", "const uint64_t*": "*const u64",
              "const NraysProbeDepthParams*": "*const NraysProbeDepthParams", "const NraysIrradianceGrid*": "*const NraysIrradianceGrid",
              "const NraysIrradianceVisibility*": "*const NraysIrradianceVisibility", "float*": "*mut f32", "uint32_t*": "*mut u32", "double*": "*mut f64", "void*": "*mut c_void"}
STRUCTS = {
    "NraysProbeDepthParams": ([("num_dirs", "uint32_t", "u32", C.c_uint32), ("num_rotations", "uint32_t", "u32", C.c_uint32), ("dirs", "const double*", "*const f64", C.c_void_p),
                               ("rotations", "const double*", "*const f64", C.c_void_p), ("bias", "double", "f64", C.c_double), ("max_dist", "double", "f64", C.c_double),
                               ("near_dist", "double", "f64", C.c_double), ("res", "uint32_t", "u32", C.c_uint32), ("reserved", "uint32_t", "u32", C.c_uint32)],
                              [56, 0, 4, 8, 16, 24, 32, 40, 48, 52]),
    "NraysIrradianceVisibility": ([("moments", "const float*", "*const f32", C.c_void_p), ("res", "uint32_t", "u32", C.c_uint32), ("floor", "float", "f32", C.c_float),
                                   ("bias", "double", "f64", C.c_double)], [24, 0, 8, 12, 16]),
}
RES = (4, 8, 16)


# ---- the surface --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_header_ctypes_and_rust_declare_the_same_function(name):
    assert _c_params(name) == EXPECTED[name]
    assert name in abi.HIP_SYMBOLS and name in abi.POST_V7_SYMBOLS
    res, args = abi.HIP_SYMBOLS[name]
    assert res is C.c_int and len(args) == len(EXPECTED[name]) and args[1] is C.c_uint32
    for c_type, struct in (("const NraysProbeDepthParams*", "NraysProbeDepthParams"), ("const NraysIrradianceVisibility*", "NraysIrradianceVisibility"),
                           ("const NraysIrradianceGrid*", "NraysIrradianceGrid")):
        if c_type in EXPECTED[name]:
            assert args[EXPECTED[name].index(c_type)] is C.POINTER(getattr(abi, struct))
    m = re.search(r"pub fn %s\((.*?)\) -> c_int;" % name, FFI)
    assert m, "%s is not declared in gpu_ffi.rs" % name
    assert [p.split(": ", 1)[1] for p in m.group(1).split(", ")] == [RUST_TYPES[t] for t in EXPECTED[name]]
    short = name[len("nrays_"):]
    assert ("pub unsafe fn %s(" if short.endswith("_device") else "pub fn %s(") % short in GPU_RS and name + "(" in GPU_RS
    note = re.search(r"Added after 7 WITHOUT a bump.*?\*/", HEADER_TEXT, re.S).group(0)
    assert re.search(r"%s\b" % name, note)


@pytest.mark.parametrize("struct", sorted(STRUCTS))
def test_the_structs_are_the_same_in_the_header_ctypes_rust_and_the_c_compiler(tmp_path, struct):
    fields, layout = STRUCTS[struct]
    m = re.search(r"struct %s \{(.*?)\};\s*typedef struct %s %s;" % (struct, struct, struct), HEADER, re.S)
    assert m, "struct %s is not declared in include/nrays_abi.h (struct plus separate typedef)" % struct
    c_fields = [re.sub(r"\s*\*\s*", "* ", f.strip()).rsplit(" ", 1) for f in m.group(1).split(";") if f.strip()]
    assert [(n, t) for t, n in c_fields] == [(n, t) for n, t, _, _ in fields]
    r = re.search(r"#\[repr\(C\)\]\s*(?:#\[derive[^\]]*\]\s*)?pub struct %s \{(.*?)\n\}" % struct, FFI, re.S)
    assert r and re.findall(r"pub (\w+): ([^,]+),", r.group(1)) == [(n, t) for n, _, t, _ in fields]
    ct = getattr(abi, struct)
    assert [(n, t) for n, t in ct._fields_] == [(n, t) for n, _, _, t in fields]
    src = tmp_path / "layout.c"  # the layout, from the C compiler itself
    names = [n for n, _, _, _ in fields]
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "nrays_abi.h"\nint main(void) {\n    printf("%%zu", sizeof(%s));\n' % struct
                   + "".join('    printf(" %%zu", offsetof(%s, %s));\n' % (struct, n) for n in names) + '    printf("\\n");\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [C.sizeof(ct)] + [getattr(ct, n).offset for n in names]
    assert got == layout


def test_the_symbols_are_exported_and_without_a_scene_every_call_is_a_bad_arg(built):
    lib = abi.load_hip_lib()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", abi.HIP_LIB_PATH]).decode()
    for name in EXPECTED:
        assert (" T " + name + "\n") in exported, name
        assert getattr(lib, name).argtypes == abi.HIP_SYMBOLS[name][1]
    assert abi.ABI_VERSION == 7 and lib.nrays_abi_version() == 7
    a = (C.c_double * 3)(0.0, 0.0, 1.0)
    mo, cnt, near, ndir = (C.c_float * 32)(*([7.0] * 32)), (C.c_uint32 * 2)(7, 7), (C.c_double * 1)(7.0), (C.c_uint32 * 1)(7)
    adr = C.addressof
    params = abi.NraysProbeDepthParams(1, 0, adr(a), None, 0.0, 1.0, 0.0, 4, 0)
    for n in (0, 1):
        assert lib.nrays_probe_depth_points(None, n, a, a, None, None, C.byref(params), mo, cnt, near, ndir, 0) == abi.ERR_BAD_ARG
        assert lib.nrays_probe_depth_points_device(None, n, adr(a), adr(a), None, None, C.byref(params), adr(mo), None, None, None, 0, None) == abi.ERR_BAD_ARG
    sh, rgb = (C.c_float * 3)(1.0, 1.0, 1.0), (C.c_float * 3)(7.0, 7.0, 7.0)
    grid = abi.NraysIrradianceGrid((C.c_double * 3)(0, 0, 0), (C.c_double * 3)(1, 1, 1), (C.c_uint32 * 3)(1, 1, 1), 1, adr(sh), None, 1.0, 0)
    vis = abi.NraysIrradianceVisibility(adr(mo), 4, 0.0, 0.0)
    for n in (0, 1):
        assert lib.nrays_irradiance_points_vis(None, n, a, a, None, C.byref(grid), C.byref(vis), rgb, None, None, 0) == abi.ERR_BAD_ARG
        assert lib.nrays_irradiance_points_vis_device(None, n, adr(a), adr(a), None, C.byref(grid), C.byref(vis), adr(rgb), None, None, 0, None) == abi.ERR_BAD_ARG
    assert lib.nrays_last_error() and list(mo) == [7.0] * 32 and list(rgb) == [7.0] * 3 and list(cnt) == [7, 7]


def test_the_python_names_exist_and_the_old_signatures_stand():
    import inspect
    for name in ("probe_depth_points", "probe_depth", "oct_texel", "probe_depth_ref", "probe_valid_words", "bake_probe_visibility"):
        assert callable(getattr(nr, name)), name
    assert nr.ProbeVisibility._fields == ("moments", "res", "floor", "bias")
    v = nr.ProbeVisibility(None, 8)
    assert v.floor == 0.05 and v.bias == 0.0
    assert nr.ProbeGrid._fields == ("origin", "cell", "counts", "sh", "valid", "measure")
    assert nr.ProbeDepth._fields == ("moments", "counts", "nearest", "nearest_dir")
    from nrays_amd import scenefile
    for cls in (nr.Scene, scenefile.FileScene):
        for name in ("probe_depth_points", "probe_depth", "bake_probe_visibility", "irradiance_points"):
            assert list(inspect.signature(getattr(cls, name)).parameters)[1:] == list(inspect.signature(getattr(nr, name)).parameters)[1:], name
    for fn in (nr.irradiance_points, nr.irradiance_points_ref):
        last = list(inspect.signature(fn).parameters.values())[-1]
        assert last.name == "visibility" and last.default is None
    assert list(inspect.signature(nr.irradiance_points).parameters)[:8] == ["scene", "points", "normals", "grid", "facing", "hit_flags", "want_sh", "want_weight"]
    sig = inspect.signature(nr.probe_depth_points).parameters
    assert list(sig)[:4] == ["scene", "points", "normals", "sample_dirs"] and sig["res"].default == 8 and sig["near_dist"].default == 0.0 and sig["bias"].default == 1e-3


# ---- the Python wrappers check before any library call ------------------------------------------------------------------------------------------------------
def _good(n=4):
    return dict(points=np.zeros((n, 3)), normals=np.tile([0.0, 1.0, 0.0], (n, 1)), sample_dirs=nr.sphere_dirs(4), max_dist=2.0)


def test_probe_depth_rejects_bad_arguments_before_any_library_call(no_library):
    import torch
    sc = _NoDevice()
    t3 = torch.zeros((4, 3), dtype=torch.float64)
    bad = [
        dict(points=np.zeros((4, 2))), dict(points=None), dict(normals=np.zeros((5, 3))), dict(points=np.zeros((4, 3), np.int64)),
        dict(sample_dirs=None), dict(sample_dirs=np.zeros((0, 3))), dict(sample_dirs=np.zeros((1025, 3))), dict(sample_dirs=np.zeros((4, 2))),
        dict(rotations=np.zeros((1025, 2))), dict(rotations=np.zeros((3, 3))), dict(bias=math.inf), dict(bias=math.nan),
        dict(res=0), dict(res=5), dict(res=32), dict(res=8.5), dict(res=True),
        dict(max_dist=None), dict(max_dist=0.0), dict(max_dist=-1.0), dict(max_dist=math.inf), dict(max_dist=math.nan),
        dict(near_dist=-1e-9), dict(near_dist=math.inf), dict(near_dist=math.nan),
        dict(want=("counts", "moments")), dict(want=("toi",)),
        dict(hit_flags=np.ones(3, np.uint32)), dict(hit_flags=np.ones(4, np.float32)), dict(keys=np.zeros(5, np.uint64)), dict(keys=np.zeros(4, np.float64)),
        dict(normals=t3), dict(points=t3, normals=t3),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            nr.probe_depth_points(sc, **dict(_good(), **kw))
    with pytest.raises(AssertionError, match="library was loaded"):  # a well-formed call gets as far as the library
        nr.probe_depth_points(sc, res=16, near_dist=0.5, rotations=nr.rotation_table(3), hit_flags=np.ones(4, np.uint32), keys=np.arange(4), want=(), **_good())
    for kw in (dict(positions=np.zeros((4, 2))), dict(max_dist=None), dict(res=3)):
        with pytest.raises(ValueError):
            nr.probe_depth(sc, **dict(dict(positions=np.zeros((4, 3)), sample_dirs=nr.sphere_dirs(4), max_dist=1.0), **kw))
    with pytest.raises(AssertionError, match="library was loaded"):
        nr.Scene([], []).probe_depth(np.zeros((4, 3)), nr.sphere_dirs(4), 4, 1.0)


def test_irradiance_points_rejects_a_bad_visibility_before_any_library_call(no_library):
    sc = _NoDevice()
    g = random_grid(1, (2, 1, 2))
    p, nm = np.zeros((3, 3)), np.tile([0.0, 0.0, 1.0], (3, 1))
    ok = np.ones((4, 64, 2), np.float32)
    bad = [ok, (ok, 8), nr.ProbeVisibility(None, 8), nr.ProbeVisibility(ok, 4), nr.ProbeVisibility(ok, 7), nr.ProbeVisibility(ok.astype(np.float64), 8),
           nr.ProbeVisibility(ok[:3], 8), nr.ProbeVisibility(ok, 8, floor=-0.1), nr.ProbeVisibility(ok, 8, floor=1.5), nr.ProbeVisibility(ok, 8, floor=math.nan),
           nr.ProbeVisibility(ok, 8, bias=math.inf), nr.ProbeVisibility(ok, 8, bias=math.nan), nr.ProbeVisibility(list(ok), 8)]
    for v in bad:
        with pytest.raises(ValueError):
            nr.irradiance_points(sc, p, nm, g, visibility=v)
        with pytest.raises(ValueError):
            nr.irradiance_points_ref(p, nm, g, visibility=v)
    with pytest.raises(AssertionError, match="library was loaded"):
        nr.irradiance_points(sc, p, nm, g, visibility=nr.ProbeVisibility(ok.reshape(-1), 8, 1.0, -0.5))
    with pytest.raises(AssertionError, match="library was loaded"):
        nr.irradiance_points(sc, p, nm, g)


def test_probe_valid_words_compares_in_integers():
    counts = np.array([[0, 9], [16, 0], [17, 0], [64, 64], [15, 3]], np.uint32)
    assert nr.probe_valid_words(counts, 64, 0.25).tolist() == [1, 1, 0, 0, 1] and nr.probe_valid_words(counts, 64, 0.25).dtype == np.uint32
    assert nr.probe_valid_words(counts, 64, 1.0).tolist() == [1] * 5 and nr.probe_valid_words(counts, 64, 0.0).tolist() == [1, 0, 0, 0, 0]
    assert nr.probe_valid_words(counts, 3, 0.34).tolist() == [1, 0, 0, 0, 0]  # floor(1.02) = 1 ray of 3
    for kw in (dict(num_dirs=0), dict(num_dirs=1025), dict(max_near_fraction=-0.1), dict(max_near_fraction=1.1), dict(max_near_fraction=math.nan)):
        with pytest.raises(ValueError):
            nr.probe_valid_words(counts, **dict(dict(num_dirs=64, max_near_fraction=0.25), **kw))
    with pytest.raises(ValueError):
        nr.probe_valid_words(counts[:, 0], 64)
    with pytest.raises(ValueError):
        nr.probe_valid_words(counts.astype(np.float32), 64)


# ---- the texel function ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", RES)
def test_oct_texel_reaches_every_texel_and_ignores_powers_of_two(R):
    d = np.random.default_rng(R).normal(size=(20000, 3))
    t = nr.oct_texel(d, R)
    assert t.dtype == np.uint32 and t.shape == (20000,) and sorted(set(t.tolist())) == list(range(R * R))
    for k in range(-20, 21):
        assert (nr.oct_texel(d * 2.0 ** k, R) == t).all(), k
    assert nr.oct_texel(d.reshape(100, 200, 3), R).shape == (100, 200)


@pytest.mark.parametrize("R", RES)
def test_oct_texel_on_the_axes_signed_zeros_zero_and_nan(R):
    h, top = R // 2, R - 1
    cases = [((1, 0, 0), (top, h)), ((-1, 0, 0), (0, h)), ((0, 1, 0), (h, top)), ((0, -1, 0), (h, 0)), ((0, 0, 1), (h, h)),
             ((0.0, 0.0, -1.0), (top, top)), ((-0.0, 0.0, -1.0), (0, top)), ((0.0, -0.0, -1.0), (top, 0)), ((-0.0, -0.0, -1.0), (0, 0)),  # the pole of the lower half: the sign of a zero picks the corner
             ((-0.0, -0.0, 1.0), (h, h)), ((1.0, 0.0, -0.0), (top, h)),                                                             # -0 is not < 0: the upper half
             ((0, 0, 0), (h, h)), ((-0.0, -0.0, -0.0), (h, h)), ((math.nan,) * 3, (h, h)), ((math.nan, 1.0, 1.0), (h, h)),             # s is not > 0 (or NaN): a = b = 0
             ((math.inf, 1.0, 1.0), (0, h)), ((1e308, 1e308, 1e308), (h, h))]                                                           # inf / inf is NaN -> 0; s overflows: a = b = 0
    for d, (tx, ty) in cases:
        assert int(nr.oct_texel(np.array(d, np.float64), R)) == ty * R + tx, d
    with pytest.raises(ValueError):
        nr.oct_texel(np.zeros((3, 2)), R)
    with pytest.raises(ValueError):
        nr.oct_texel(np.zeros((3, 3)), 5)


# ---- the fold -------------------------------------------------------------------------------------------------------------------------------------------------
def _rays(seed, n, k):
    d = np.random.default_rng(seed).normal(size=(n, k, 3))
    return d / np.sqrt((d * d).sum(axis=2))[..., None]


@pytest.mark.parametrize("R", RES)
def test_probe_depth_ref_constant_distance_and_empty_texels(R):
    d = _rays(3, 5, 100) * 0.5                       # |d| = 1/2 up to rounding; toi = 1 -> dist near 0.5
    n, k = d.shape[:2]
    # an exactly constant distance: directions along +-axes scaled by a power of two, toi a power of two
    axes = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], np.float64) * 0.25
    da = np.tile(axes[None], (2, 4, 1))              # (2, 24, 3)
    m, counts, nearest, ndir = nr.probe_depth_ref(da, np.full((2, 24), 8.0), np.ones((2, 24), bool), R, max_dist=64.0)
    tex = nr.oct_texel(da[0], R)
    hit_tex = np.zeros(R * R, bool); hit_tex[tex] = True
    assert (m[:, hit_tex, 0] == 2.0).all() and (m[:, hit_tex, 1].view(np.uint32) == (m[:, hit_tex, 0] * m[:, hit_tex, 0]).view(np.uint32)).all()
    assert (m[:, ~hit_tex, 0] == 64.0).all() and (m[:, ~hit_tex, 1] == 4096.0).all() and (~hit_tex).any()
    assert counts.tolist() == [[0, 0]] * 2 and nearest.tolist() == [2.0, 2.0] and ndir.tolist() == [0, 0]
    # the clamp and a max_dist that float32 rounds: the empty pair is float32(max_dist) and its float32 square
    md = 0.1
    m, counts, _, _ = nr.probe_depth_ref(da, np.full((2, 24), 8.0), np.ones((2, 24), bool), R, max_dist=md, near_dist=2.5)
    f = np.float32(md)
    assert (m[..., 0] == f).all() and (m[..., 1] == f * f).all() and counts.tolist() == [[24, 0]] * 2
    assert m.dtype == np.float32 and m.shape == (2, R * R, 2)
    m2 = nr.probe_depth_ref(d, np.ones((n, k)), np.ones((n, k), bool), R, max_dist=10.0)[0]
    assert np.isfinite(m2).all() and (m2[..., 1] >= 0).all()


def test_probe_depth_ref_counts_nearest_ties_misses_and_skipped_points():
    d = _rays(5, 4, 12)
    toi = np.full((4, 12), 3.0)
    hit = np.ones((4, 12), bool)
    d[0] = d[0, 0]                                    # point 0: twelve copies of one ray: a tie among all of them
    toi[1, 7] = toi[1, 3] = 0.5                       # point 1: the same least toi twice, on directions of different length
    d[1, 3] = d[1, 7] = (0.0, 0.0, 2.0)
    hit[2] = False; toi[2] = math.inf                 # point 2: nothing hit
    hit[3, ::2] = False; toi[3, ::2] = math.inf       # point 3: every other ray misses
    flags = np.array([1, 3, 1, 1], np.uint32)
    m, counts, nearest, ndir = nr.probe_depth_ref(d, toi, hit, 4, max_dist=8.0, near_dist=1.5, hit_flags=flags)
    assert ndir.tolist() == [0, 3, nr.scene.PROBE_NO_DIR, int(np.argmin(np.where(hit[3], toi[3] * np.sqrt((d[3] * d[3]).sum(axis=1)), math.inf)))]
    assert nearest[1] == 1.0 and nearest[2] == math.inf and ndir.dtype == np.uint32 and nearest.dtype == np.float64
    assert counts.tolist() == [[0, 0], [2, 0], [0, 12], [0, 6]] and counts.dtype == np.uint32
    assert (m[2, :, 0] == 8.0).all() and (m[2, :, 1] == 64.0).all()  # every ray is clamped to max_dist, and so is every empty texel
    # the flag words of closest_hits serve as `hit` (bit 0), and a skipped point is the empty record whatever its rays hold
    m_w = nr.probe_depth_ref(d, toi, np.where(hit, 3, 2).astype(np.uint32), 4, max_dist=8.0, near_dist=1.5, hit_flags=flags)
    assert all(same(a.astype(np.float32), b.astype(np.float32)) for a, b in zip(m_w, (m, counts, nearest, ndir)))
    d[1] = math.nan; toi[1] = math.nan
    m_s, c_s, n_s, d_s = nr.probe_depth_ref(d, toi, hit, 4, max_dist=0.1, near_dist=1.5, hit_flags=np.array([1, 2, 1, 1]))
    f = np.float32(0.1)
    assert (m_s[1, :, 0] == f).all() and (m_s[1, :, 1] == f * f).all() and c_s[1].tolist() == [0, 0] and n_s[1] == math.inf and d_s[1] == 0xFFFFFFFF
    # the order of j is the order of the sums: float32 addition is not associative
    big = np.array([[1.0e8, 1.0, -1.0e8, 1.0]])
    dz = np.tile([0.0, 0.0, 1.0], (1, 4, 1))
    a = nr.probe_depth_ref(dz, np.abs(big), np.ones((1, 4), bool), 4, max_dist=1e9)[0]
    t = int(nr.oct_texel(np.array([0.0, 0.0, 1.0]), 4))
    s = np.float32(0.0)
    for x in np.abs(big[0]).astype(np.float32):
        s = s + x
    assert a[0, t, 0] == s / np.float32(4.0)
    for kw in (dict(res=5), dict(max_dist=None), dict(max_dist=0.0), dict(max_dist=math.inf), dict(near_dist=-1.0), dict(tois=np.ones((1, 3))), dict(hit=np.ones((2, 4), bool))):
        with pytest.raises(ValueError):
            nr.probe_depth_ref(**dict(dict(ray_dirs=dz, tois=np.ones((1, 4)), hit=np.ones((1, 4), bool), res=4, max_dist=1.0), **kw))


# ---- the visibility factor on the mirror ----------------------------------------------------------------------------------------------------------------------
def _one_probe(moments, R, floor):
    g = nr.ProbeGrid((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (1, 1, 1), np.ones((1, 1, 3), np.float32), None, 1.0)
    return g, nr.ProbeVisibility(moments, R, floor, 0.0)


@pytest.mark.parametrize("R", RES)
@pytest.mark.parametrize("floor", [0.0, 0.25, 1.0])
def test_the_factor_lies_between_floor_and_one_and_never_grows_along_a_ray(R, floor):
    """One probe, one coefficient: the weight sum that comes back IS the factor (the trilinear weight of a lone probe is 1)."""
    rng = np.random.default_rng(R)
    m1 = rng.uniform(0.2, 3.0, size=(1, R * R)).astype(np.float32)
    m2 = (m1 * m1 + rng.uniform(0.0, 0.5, size=(1, R * R)).astype(np.float32)).astype(np.float32)
    m2[0, ::3] = (m1 * m1)[0, ::3]                     # zero variance in a third of the texels
    g, vis = _one_probe(np.stack([m1, m2], axis=2), R, floor)
    dirs = unit_vectors(R + 1, 40)
    steps = np.linspace(0.0, 6.0, 97)
    for d in dirs:
        p = d[None, :] * steps[:, None]
        nm = np.tile([0.0, 0.0, 1.0], (len(p), 1))
        _, _, w = nr.irradiance_points_ref(p, nm, g, visibility=vis)
        assert (w >= np.float32(floor)).all() and (w <= 1.0).all()
        assert w[0] == 1.0                             # l2 == 0: no factor
        assert (np.diff(w.astype(np.float64)) <= 0.0).all(), "the factor grew with the distance"
        t = int(nr.oct_texel(d, R))
        near = steps.astype(np.float32) <= m1[0, t]
        assert (w[near & (steps > 0)] == 1.0).all()    # not beyond the mean depth: no factor


def test_moments_beyond_every_distance_are_the_call_without_visibility():
    for counts, bands, facing in (((1, 1, 1), 1, False), ((2, 2, 2), 3, True), ((3, 1, 2), 2, False), ((3, 1, 2), 3, True)):
        g = random_grid(11, counts, bands)
        P = counts[0] * counts[1] * counts[2]
        valid = np.random.default_rng(12).integers(0, 2, size=P).astype(np.uint32)
        p = np.random.default_rng(13).uniform(-2.0, 3.0, size=(200, 3))
        nm = unit_vectors(14, 200)
        flags = np.random.default_rng(15).integers(0, 2, size=200).astype(np.uint32)
        for R in RES:
            for v in (None, valid):
                gg = g._replace(valid=v)
                vis = nr.ProbeVisibility(np.full((P, R * R, 2), 1e30, np.float32), R, 0.25, 0.01)
                a = nr.irradiance_points_ref(p, nm, gg, facing, flags)
                b = nr.irradiance_points_ref(p, nm, gg, facing, flags, visibility=vis)
                assert all(same(x, y) for x, y in zip(a, b))


def test_an_invalid_probes_moments_are_never_read():
    g = random_grid(21, (2, 2, 2), 2)
    valid = np.array([1, 0, 1, 1, 0, 1, 1, 0], np.uint32)
    mo = np.random.default_rng(22).uniform(0.1, 1.0, size=(8, 16, 2)).astype(np.float32)
    poisoned = mo.copy(); poisoned[valid == 0] = np.nan
    p = np.random.default_rng(23).uniform(-1.0, 1.5, size=(100, 3))
    nm = unit_vectors(24, 100)
    a = nr.irradiance_points_ref(p, nm, g._replace(valid=valid), True, visibility=nr.ProbeVisibility(mo, 4, 0.0, 0.0))
    b = nr.irradiance_points_ref(p, nm, g._replace(valid=valid), True, visibility=nr.ProbeVisibility(poisoned, 4, 0.0, 0.0))
    assert all(same(x, y) for x, y in zip(a, b)) and np.isfinite(a[0]).all()
    assert not same(a[0], nr.irradiance_points_ref(p, nm, g._replace(valid=valid), True)[0])  # and the factor is not vacuous
