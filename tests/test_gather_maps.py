"""Light gathered from baked maps at the rays' closest hits (nrays_gather_maps_points_device / nrays_gather_maps_points; nrays_amd.gather_maps_points,
gather_maps_hits, lightmap_sample_ref, bake_bounces), the parts that need no GPU: the header, the ctypes table and the Rust declarations, the struct's layout
against the C compiler's, the sample mirror against tests/texture_cases.py's independent restatement, the argument checks — and the expected values of one small
scene from the CPU oracle alone (the mirror's rays through oracle.cast, the mirror's sample, folded in numpy f32), which tests/test_gather_maps_gpu.py imports
together with the furnace scene."""
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
from tests import texture_cases as tc
from tests.test_gather import _NoDevice, _c_params, fold, no_library  # noqa: F401  (no_library is a fixture)
from tests.test_occlusion import _surface_points
from tools import scenes_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_TEXT = open(os.path.join(ROOT, "include", "nrays_abi.h")).read()
HEADER = re.sub(r"/\*.*?\*/", "", HEADER_TEXT, flags=re.S)
FFI = open(os.path.join(ROOT, "integration", "rust", "src", "gpu_ffi.rs")).read()
GPU_RS = open(os.path.join(ROOT, "integration", "rust", "src", "gpu.rs")).read()
_IN = ["NraysScene*", "uint32_t", "const double*", "const double*", "const uint32_t*", "const uint64_t*", "const NraysGatherMapsParams*", "float*", "uint32_t*", "uint32_t"]
EXPECTED = {"nrays_gather_maps_points_device": _IN + ["void*"], "nrays_gather_maps_points": _IN}
RUST_TYPES = {"NraysScene*": "*mut NraysScene", "uint32_t": "u32", "const double*": "*const f64", "const uint32_t*": "*const u32", "const uint64_t*": "*const u64",
              "const NraysGatherMapsParams*": "*const NraysGatherMapsParams", "float*": "*mut f32", "uint32_t*": "*mut u32", "void*": "*mut c_void"}
STRUCT_FIELDS = [("num_dirs", "uint32_t", "u32", C.c_uint32), ("num_rotations", "uint32_t", "u32", C.c_uint32), ("dirs", "const double*", "*const f64", C.c_void_p),
                 ("rotations", "const double*", "*const f64", C.c_void_p), ("bias", "double", "f64", C.c_double), ("max_toi", "double", "f64", C.c_double),
                 ("num_maps", "uint32_t", "u32", C.c_uint32), ("num_nodes", "uint32_t", "u32", C.c_uint32),
                 ("maps", "const NraysTexture*", "*const NraysTexture", C.POINTER(abi.NraysTexture)), ("node_map", "const int32_t*", "*const i32", C.c_void_p),
                 ("miss_rgb", "float", "[f32; 3]", C.c_float * 3)]
DARK, MAPPED, MISSED = 0, 1, 2
BILINEAR_CLAMP = (nr.Interpolation.Bilinear, nr.Overflow.ClampToEdges)


# ---- shared with the GPU tests ------------------------------------------------------------------------------------------------------------------------
def contributions(hit, has_uv, node, u, v, maps, node_map, miss):
    """The definition's c_ij and class per ray, from a closest-hit record: `maps` [(texels, interp, overflow)], `node_map` one integer per scene node."""
    hit, has_uv, node = np.asarray(hit, bool), np.asarray(has_uv, bool), np.asarray(node).astype(np.int64)
    node_map = np.asarray(node_map, np.int64)
    m = np.where(hit, node_map[np.where(hit, node, 0)], -1)
    m = np.where((m >= 0) & (m < len(maps)) & has_uv & hit, m, -1)
    c = np.zeros((len(hit), 3), np.float32)
    cls = np.where(hit, DARK, MISSED)
    c[~hit] = np.asarray(miss, np.float32)
    for i, (texels, interp, overflow) in enumerate(maps):
        sel = m == i
        if sel.any():
            c[sel] = nr.lightmap_sample_ref(texels, u[sel], v[sel], interp, overflow)[:, :3]
            cls[sel] = MAPPED
    return c, cls


def fold_classes(c, cls, n, k):
    """(out_rgb (n, 3) float32, out_counts (n, 2) uint32) of the definition from the n * k per-ray contributions."""
    cls = cls.reshape(n, k)
    return fold(c.reshape(n, k, 3)), np.stack([(cls == MAPPED).sum(axis=1), (cls == MISSED).sum(axis=1)], axis=1).astype(np.uint32)


def random_map(seed, w, h, lo=0.0, hi=1.0):
    return np.random.default_rng(seed).uniform(lo, hi, size=(h, w, 4)).astype(np.float32)


def mixed_scene():
    from tests.test_occlusion_gpu import _mixed  # (a scene builder only; nothing of that module runs here)
    return _mixed()


_ORACLE = {}


def oracle_case():
    """Computed once and left unchanged: 320 surface points of the quads with a ball and a capsule (four nodes), 16 directions, 5 rotations, two 8 x 8 maps with
    texels in [0, 1]; floor -> map 0, lace -> map 1, the ball -> -1, the capsule -> an entry out of range.  c["rgb"], c["counts"]: what the CPU oracle expects —
    the mirror's rays through oracle.cast, lightmap_sample_ref at its uv, folded in numpy f32; c["classes"] (n, k)."""
    if not _ORACLE:
        sc, cam, o, d = mixed_scene()
        p, nm, _ = _surface_points(sc, o, d)
        assert len(p) >= 320
        sel = np.linspace(0, len(p) - 1, 320).astype(int)
        keys = np.random.default_rng(71).integers(0, 2**63, size=320, dtype=np.int64).astype(np.uint64) * np.uint64(2) + np.uint64(1)
        c = dict(scene=sc, points=np.ascontiguousarray(p[sel]), normals=np.ascontiguousarray(nm[sel]), keys=keys, sample_dirs=nr.hemisphere_dirs(16),
                 rotations=nr.rotation_table(5), bias=1e-3, maps=[random_map(72, 8, 8), random_map(73, 8, 8)], node_map=[0, 1, -1, 7], miss=(0.25, 0.5, 1.0))
        ro, rd = nr.occlusion_rays(c["points"], c["normals"], c["sample_dirs"], c["rotations"], c["bias"], c["keys"])
        hit, rec = oracle.cast(sc.descriptor, ro.reshape(-1, 3), rd.reshape(-1, 3))
        con, cls = contributions(hit, rec[:, 4] != 0.0, rec[:, 7], rec[:, 5], rec[:, 6], [(m,) + BILINEAR_CLAMP for m in c["maps"]], c["node_map"], c["miss"])
        c["rgb"], c["counts"] = fold_classes(con, cls, 320, 16)
        c["classes"] = cls.reshape(320, 16)
        _ORACLE.update(c)
    return _ORACLE


def call_args(c):
    return {k: c[k] for k in ("points", "normals", "sample_dirs", "maps", "node_map", "rotations", "bias", "miss", "keys")}


# ---- the furnace: a closed unit cube that lights itself ------------------------------------------------------------------------------------------------
FURNACE_KA = (0.5, 0.25, 0.125)
FURNACE_ATLAS, FURNACE_CHART = 32, 8
_FACES = [  # (origin, e1, e2): v0 = o, v1 = o + e1, v2 = o + e1 + e2, v3 = o + e2; cross(e1, e2) points OUT of the cube
    ((0, 0, 0), (1, 0, 0), (0, 0, 1)),  # y = 0, the floor
    ((0, 1, 0), (0, 0, 1), (1, 0, 0)),  # y = 1, the top
    ((0, 0, 0), (0, 1, 0), (1, 0, 0)),  # z = 0
    ((0, 0, 1), (1, 0, 0), (0, 1, 0)),  # z = 1
    ((0, 0, 0), (0, 0, 1), (0, 1, 0)),  # x = 0
    ((1, 0, 0), (0, 1, 0), (0, 0, 1)),  # x = 1
]
FURNACE_FLOOR, FURNACE_TOP = 0, 1


def furnace_mesh(open_top=False):
    """The unit cube as one mesh of 12 triangles (10 without its top), wound so that the geometric normals point outwards (bake with flip_normals), six
    8 x 8-texel charts in a 32 x 32 atlas.  Chart c starts at texel (2 + 10 (c % 3), 2 + 10 (c // 3)); a face spans the uv square from half a texel before its
    first texel to half a texel after its last, so the 64 lattice points of a chart lie strictly inside the face, 1/16 of its side from the nearest edge."""
    pts, uvs, idx = [], [], []
    for c, (o, e1, e2) in enumerate(_FACES):
        if open_top and c == FURNACE_TOP:
            continue
        o, e1, e2 = (np.asarray(a, np.float64) for a in (o, e1, e2))
        x0, y0 = 2 + 10 * (c % 3), 2 + 10 * (c // 3)
        lo_u, hi_u, lo_v, hi_v = ((t - 0.5) / (FURNACE_ATLAS - 1) for t in (x0, x0 + FURNACE_CHART, y0, y0 + FURNACE_CHART))
        base = len(pts)
        pts += [o, o + e1, o + e1 + e2, o + e2]
        uvs += [(lo_u, lo_v), (hi_u, lo_v), (hi_u, hi_v), (lo_u, hi_v)]
        idx += [(base, base + 1, base + 2), (base, base + 2, base + 3)]
    return su.f32_exact(np.asarray(pts)), np.asarray(idx, np.uint32), su.f32_exact(np.asarray(uvs))


def furnace_scene(open_top=False):
    """One TriMesh node, Phong with ka = FURNACE_KA and no texture, NO lights: shade_points gives ka at every texel."""
    pts, idx, uvs = furnace_mesh(open_top)
    mat = nr.PhongMaterial(FURNACE_KA, (0.7, 0.7, 0.7), (0.3, 0.3, 0.3), None, None, 20.0)
    return nr.Scene([nr.SceneNode(mat, 0.0, 0.0, 1.0, 1.0, nr.Isometry3(), nr.TriMesh(pts, idx, uvs))], [], (0.0, 0.0, 0.0))


def furnace_chart_mask(face):
    """(32, 32) bool: the texels of one face's chart."""
    m = np.zeros((FURNACE_ATLAS, FURNACE_ATLAS), bool)
    x0, y0 = 2 + 10 * (face % 3), 2 + 10 * (face // 3)
    m[y0:y0 + FURNACE_CHART, x0:x0 + FURNACE_CHART] = True
    return m


def furnace_tables():
    return nr.hemisphere_dirs(16), nr.rotation_table(5)


# ---- the surface --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_header_ctypes_and_rust_declare_the_same_function(name):
    assert _c_params(name) == EXPECTED[name]
    assert name in abi.HIP_SYMBOLS and name in abi.POST_V7_SYMBOLS
    res, args = abi.HIP_SYMBOLS[name]
    assert res is C.c_int and len(args) == len(EXPECTED[name]) and args[1] is C.c_uint32
    assert args[EXPECTED[name].index("const NraysGatherMapsParams*")] is C.POINTER(abi.NraysGatherMapsParams)
    m = re.search(r"pub fn %s\((.*?)\) -> c_int;" % name, FFI)
    assert m, "%s is not declared in gpu_ffi.rs" % name
    assert [p.split(": ", 1)[1] for p in m.group(1).split(", ")] == [RUST_TYPES[t] for t in EXPECTED[name]]
    assert "pub fn gather_maps_points(" in GPU_RS and "pub unsafe fn gather_maps_points_device(" in GPU_RS
    assert "nrays_gather_maps_points(" in GPU_RS and "nrays_gather_maps_points_device(" in GPU_RS


def test_the_params_struct_is_the_same_in_the_header_ctypes_rust_and_the_c_compiler(tmp_path):
    m = re.search(r"struct NraysGatherMapsParams \{(.*?)\};\s*typedef struct NraysGatherMapsParams NraysGatherMapsParams;", HEADER, re.S)
    assert m, "struct NraysGatherMapsParams is not declared in include/nrays_abi.h (struct plus separate typedef)"
    c_fields = [re.sub(r"\[.*\]", "", re.sub(r"\s*\*\s*", "* ", f.strip())).rsplit(" ", 1) for f in m.group(1).split(";") if f.strip()]
    assert [(n, t) for t, n in c_fields] == [(n, t) for n, t, _, _ in STRUCT_FIELDS]
    assert re.search(r"float miss_rgb\[3\];", m.group(1))
    r = re.search(r"#\[repr\(C\)\]\s*(?:#\[derive[^\]]*\]\s*)?pub struct NraysGatherMapsParams \{(.*?)\n\}", FFI, re.S)
    assert r and re.findall(r"pub (\w+): ([^,]+),", r.group(1)) == [(n, t) for n, _, t, _ in STRUCT_FIELDS]
    assert [(n, t) for n, t in abi.NraysGatherMapsParams._fields_] == [(n, t) for n, _, _, t in STRUCT_FIELDS]
    assert re.search(r"#define NRAYS_GATHER_MAX_MAPS 16u\b", HEADER) and abi.GATHER_MAX_MAPS == 16 and re.search(r"pub const NRAYS_GATHER_MAX_MAPS: u32 = 16;", FFI)
    # the layout, from the C compiler itself
    src = tmp_path / "layout.c"
    names = [n for n, _, _, _ in STRUCT_FIELDS]
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "nrays_abi.h"\nint main(void) {\n    printf("%zu", sizeof(NraysGatherMapsParams));\n'
                   + "".join('    printf(" %%zu", offsetof(NraysGatherMapsParams, %s));\n' % n for n in names) + '    printf("\\n");\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [C.sizeof(abi.NraysGatherMapsParams)] + [getattr(abi.NraysGatherMapsParams, n).offset for n in names]
    assert got == [80, 0, 4, 8, 16, 24, 32, 40, 44, 48, 56, 64]


def test_the_symbols_are_exported_and_the_abi_version_is_still_7(built):
    assert re.search(r"#define NRAYS_ABI_VERSION 7\b", HEADER) and abi.ABI_VERSION == 7 and abi.load_hip_lib().nrays_abi_version() == 7
    note = re.search(r"Added after 7 WITHOUT a bump.*?\*/", HEADER_TEXT, re.S).group(0)
    exported = subprocess.check_output(["nm", "-D", "--defined-only", abi.HIP_LIB_PATH]).decode()
    for name in EXPECTED:
        assert re.search(r"%s\b" % name, note), name
        assert (" T " + name + "\n") in exported, name
        assert getattr(abi.load_hip_lib(), name).argtypes == abi.HIP_SYMBOLS[name][1]


def test_without_a_scene_every_call_is_a_bad_arg(built):
    lib = abi.load_hip_lib()
    a = (C.c_double * 3)(0.0, 0.0, 1.0)
    out = (C.c_float * 3)(7.0, 7.0, 7.0)
    cnt = (C.c_uint32 * 2)(7, 7)
    texels = (C.c_float * 4)(1.0, 1.0, 1.0, 1.0)
    rec = abi.NraysTexture(1, 1, abi.TEXEL_RGBA32F, abi.INTERP_BILINEAR, abi.OVERFLOW_CLAMP, 0, C.addressof(texels))
    nodes = (C.c_int32 * 1)(0)
    params = abi.NraysGatherMapsParams(1, 0, C.addressof(a), None, 1e-3, math.inf, 1, 1, C.pointer(rec), C.addressof(nodes), (C.c_float * 3)(0, 0, 0))
    for n in (0, 1):
        assert lib.nrays_gather_maps_points(None, n, a, a, None, None, C.byref(params), out, cnt, 0) == abi.ERR_BAD_ARG
        assert lib.nrays_gather_maps_points_device(None, n, C.addressof(a), C.addressof(a), None, None, C.byref(params), C.addressof(out), C.addressof(cnt), 0, None) == abi.ERR_BAD_ARG
    assert lib.nrays_last_error() and list(out) == [7.0] * 3 and list(cnt) == [7, 7]


# ---- the sample mirror against the independent restatement ---------------------------------------------------------------------------------------------------
def _same(a, b):
    """Bit patterns equal, any NaN equal to any NaN."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.parametrize("overflow", [tc.WRAP, tc.CLAMP])
@pytest.mark.parametrize("interp", [tc.BILINEAR, tc.NEAREST])
def test_lightmap_sample_ref_against_the_f64_restatement(interp, overflow):
    """Every texture and coordinate set of tests/texture_cases.py (±0, denormals, huge values, texel centres and ties with their f32 neighbours, random values;
    then the non-finite pairs): Nearest by bit pattern, Bilinear within that module's bound 4 * 2^-24 * max|texel| of the f64 blend of the same taps and weights."""
    assert (nr.Interpolation.Bilinear, nr.Interpolation.Nearest, nr.Overflow.Wrap, nr.Overflow.ClampToEdges) == (tc.BILINEAR, tc.NEAREST, tc.WRAP, tc.CLAMP)
    seen = 0
    for (w, h), tex in tc.TEXTURES.items():
        texels = tex["rgba32f"]
        bound = 4.0 * 2.0 ** -24 * float(np.abs(texels).max())
        for uv in (tc.pairs(w, h), tc.nonfinite_pairs()):
            want = tc.sample_ref(texels, interp, overflow, uv[:, 0], uv[:, 1])
            got = nr.lightmap_sample_ref(texels, uv[:, 0].astype(np.float64), uv[:, 1].astype(np.float64), interp, overflow)
            assert got.dtype == np.float32 and got.shape == (len(uv), 4)
            if interp == tc.NEAREST:
                assert _same(got, want.value.astype(np.float32)), (w, h)
            else:
                nan = np.isnan(want.value)
                assert np.array_equal(np.isnan(got), nan), (w, h)
                err = float(np.abs(np.where(nan, 0.0, got.astype(np.float64) - want.value)).max())
                assert err <= bound, (w, h, err, bound)
            seen += len(uv)
    assert seen > 2000
    # a texel centre is the texel itself, and the f64 coordinates of a hit record are rounded to f32 first
    t = tc.TEXTURES[(8, 8)]["rgba32f"]
    cu = tc.centre_values(8).astype(np.float64)[1:7]  # (without 0, where 1e-12 more is another f32, and 1, which Wrap folds to 0)
    assert _same(nr.lightmap_sample_ref(t, cu, cu[::-1].copy(), interp, overflow), t[np.arange(1, 7)[::-1], np.arange(1, 7)])
    assert _same(nr.lightmap_sample_ref(t, cu + 1e-12, cu, interp, overflow), nr.lightmap_sample_ref(t, cu, cu, interp, overflow))


def test_lightmap_sample_ref_defaults_and_checks():
    t = tc.TEXTURES[(3, 7)]["rgba32f"]
    u, v = np.asarray([0.3, 1.7, -0.2]), np.asarray([0.9, 0.1, 0.5])
    assert _same(nr.lightmap_sample_ref(t, u, v), nr.lightmap_sample_ref(t, u, v, nr.Interpolation.Bilinear, nr.Overflow.ClampToEdges))
    assert not _same(nr.lightmap_sample_ref(t, u, v), nr.lightmap_sample_ref(t, u, v, overflow=nr.Overflow.Wrap))
    for bad in (t.astype(np.float64), t[:, :, :3], t[0], tc.TEXTURES[(3, 7)]["rgba8"]):
        with pytest.raises(ValueError):
            nr.lightmap_sample_ref(bad, u, v)
    with pytest.raises(ValueError):
        nr.lightmap_sample_ref(t, u, v[:2])
    with pytest.raises(ValueError):
        nr.lightmap_sample_ref(t, u, v, interp=5)


# ---- the Python wrappers check before any library call ------------------------------------------------------------------------------------------------------
def _one_node_scene():
    return nr.Scene([nr.SceneNode(su.default_material(), 0.0, 0.0, 1.0, 1.0, nr.Isometry3((0, 0, 0)), nr.Plane((0, 1, 0)))], [], (0, 0, 0))


class _NoDeviceScene(_NoDevice):
    """A one-node scene whose device handle must never be asked for."""
    def __init__(self):
        self.descriptor = _one_node_scene().descriptor


def _good(n=4):
    return dict(points=np.zeros((n, 3)), normals=np.tile([0.0, 1.0, 0.0], (n, 1)), sample_dirs=nr.hemisphere_dirs(4), maps=[np.zeros((3, 5, 4), np.float32)], node_map=[0])


def test_gather_maps_points_rejects_bad_arguments_before_any_library_call(no_library):
    import torch
    sc = _NoDeviceScene()
    m = np.zeros((3, 5, 4), np.float32)
    bad = [
        dict(maps=[np.zeros((3, 5, 3), np.float32)]), dict(maps=[np.zeros((3, 5, 4), np.float64)]), dict(maps=[np.zeros((15, 4), np.float32)]),
        dict(maps=[np.zeros((0, 5, 4), np.float32)]), dict(maps=[np.zeros((3, 5, 4), np.uint8)]), dict(maps=[[[0.0] * 4]]), dict(maps=m), dict(maps=None), dict(maps=[]),
        dict(maps=[m] * 17), dict(maps=[nr.Texture2d(nr.ImageData(np.zeros((2, 2, 4), np.uint8)))]), dict(maps=[nr.Texture2d(nr.ImageData(m), 7, nr.Overflow.Wrap)]),
        dict(maps=[torch.zeros((3, 5, 4), dtype=torch.float32)]),  # numpy points, a tensor map
        dict(node_map=[0.0]), dict(node_map=["0"]), dict(node_map=[None]), dict(node_map=[True]), dict(node_map={0: 0.5}), dict(node_map={"a": 0}), dict(node_map={1: 0}),
        dict(node_map=[0, 0]), dict(node_map=[]), dict(node_map=None), dict(node_map="0"),
        dict(max_toi=math.nan), dict(max_toi=0.0), dict(max_toi=-1.0),
        dict(miss=(0.0, 0.0)), dict(miss=(0.0, math.inf, 0.0)), dict(miss=(math.nan, 0.0, 0.0)), dict(miss=(1e39, 0.0, 0.0)),
        dict(points=np.zeros((4, 2))), dict(normals=np.zeros((5, 3))), dict(sample_dirs=np.zeros((0, 3))), dict(sample_dirs=np.zeros((1025, 3))),
        dict(rotations=np.zeros((3, 3))), dict(bias=math.nan), dict(hit_flags=np.ones(3, np.uint32)), dict(keys=np.zeros(4, np.float64)),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            nr.gather_maps_points(sc, **dict(_good(), **kw))
    for ok in (dict(), dict(maps=[m] * 16, node_map=[15]), dict(node_map={0: 0}), dict(node_map={}), dict(node_map=[-1]), dict(node_map=[99]), dict(max_toi=2.0, miss=(1, 2, 3)),
               dict(maps=[nr.Texture2d(nr.ImageData(m), nr.Interpolation.Nearest, nr.Overflow.Wrap)]), dict(node_map=np.asarray([0], np.int32)), dict(want_counts=True)):
        with pytest.raises(AssertionError, match="library was loaded"):  # a well-formed call gets as far as the library
            nr.gather_maps_points(sc, **dict(_good(), **ok))
    from nrays_amd import scenefile
    for cls in (nr.Scene, scenefile.FileScene):
        assert callable(cls.gather_maps_points) and callable(cls.bake_bounces)
    with pytest.raises(ValueError):
        _one_node_scene().gather_maps_points(np.zeros((4, 3)), np.zeros((4, 3)), nr.hemisphere_dirs(4), [m], [0, 1])


def test_bake_bounces_rejects_bad_arguments_before_any_library_call(no_library):
    sc = _NoDeviceScene()
    L = nr.hemisphere_dirs(4)
    good = dict(node=0, width=8, height=6, sample_dirs=L, bounces=2, albedo=0.5 * np.ones(3))
    bad = [dict(dilate=1), dict(dilate=0), dict(dilate=65), dict(dilate=-1), dict(albedo=0.5), dict(albedo=(0.5, 0.5)), dict(albedo=np.ones((8, 6, 3))), dict(albedo=np.ones((6, 8, 4))),
           dict(albedo=("a", "b", "c")), dict(bounces=-1), dict(width=0), dict(sample_dirs=np.zeros((4, 2))), dict(miss=(1.0, math.nan, 0.0)), dict(bias=math.inf)]
    for kw in bad:
        with pytest.raises(ValueError):
            nr.bake_bounces(sc, **dict(good, **kw))
    for ok in (dict(), dict(albedo=np.ones((6, 8, 3))), dict(dilate=64), dict(bounces=0)):
        with pytest.raises(AssertionError, match="library was loaded"):
            nr.bake_bounces(sc, **dict(good, **ok))
    assert "denois" in nr.bake_bounces.__doc__


def test_gather_maps_hits_builds_the_points_of_occlusion_hits(no_library, monkeypatch):
    sc = _NoDeviceScene()
    o, d = np.zeros((4, 3)), np.tile([0.0, 0.0, 1.0], (4, 1))
    normal = np.asarray([(0.0, 0.0, -1.0), (0.0, 0.0, 1.0), (0.6, 0.0, 0.8), (1.0, 0.0, 0.0)])
    full = nr.CastHits(toi=np.asarray([1.0, 2.0, 3.0, 4.0]), node=np.zeros(4, np.int32), normal=normal, uv=None, prim=None, flags=np.asarray([1, 3, 1, 0], np.uint32))
    L, m = nr.hemisphere_dirs(4), np.zeros((2, 2, 4), np.float32)
    for name in ("normal", "flags"):
        with pytest.raises(ValueError, match=name):
            nr.gather_maps_hits(sc, o, d, full._replace(**{name: None}), L, [m], [0])
    with pytest.raises(AssertionError, match="library was loaded"):
        nr.gather_maps_hits(sc, o, d, full, L, [m], [0])
    seen = {}
    monkeypatch.setattr(nr.scene, "gather_maps_points", lambda scene, points, normals, *a, **kw: seen.update(points=points, normals=normals, a=a, kw=kw) or "result")
    assert nr.gather_maps_hits(sc, o, d, full, L, [m], [0], None, 0.25, 3.0, (1, 2, 3), keys=np.arange(4)) == "result"
    assert np.array_equal(seen["points"], [(0, 0, 1), (0, 0, 2), (0, 0, 3), (0, 0, 0)]) and np.array_equal(seen["normals"], [(0, 0, -1), (0, 0, -1), (-0.6, 0, -0.8), (1, 0, 0)])
    assert seen["a"][1:] == ([m], [0], None, 0.25, 3.0, (1, 2, 3)) and np.array_equal(seen["kw"]["hit_flags"], full.flags) and np.array_equal(seen["kw"]["keys"], np.arange(4))


# ---- the expected values from the oracle, and the furnace's rays -----------------------------------------------------------------------------------------------
def test_oracle_expectation_sees_all_three_classes():
    c = oracle_case()
    assert c["rgb"].shape == (320, 3) and c["rgb"].dtype == np.float32 and c["counts"].shape == (320, 2) and c["counts"].dtype == np.uint32
    cls = c["classes"]
    print("mapped %d, missed %d, dark %d of %d rays" % ((cls == MAPPED).sum(), (cls == MISSED).sum(), (cls == DARK).sum(), cls.size))
    assert (cls == MAPPED).sum() > 500 and (cls == MISSED).sum() > 500 and (cls == DARK).sum() > 50
    assert all(0.0 <= float(m.min()) and float(m.max()) <= 1.0 for m in c["maps"])
    mixed = ((c["counts"][:, 0] > 0) & (c["counts"][:, 1] > 0)).sum()
    assert mixed >= 50  # points whose mean blends map light and the sky


def test_furnace_rays_all_land_inside_the_cube():
    """Every hemisphere ray of every covered texel of the closed cube hits the cube, with a uv (checked with the CPU oracle): none escapes through an edge."""
    pts, idx, uvs = furnace_mesh()
    tx = nr.surface_texels_ref(pts, idx, uvs, None, FURNACE_ATLAS, FURNACE_ATLAS, flip_normals=True)
    live = (tx.flags & 1) != 0
    assert live.sum() == 6 * FURNACE_CHART ** 2
    assert np.array_equal(live.reshape(FURNACE_ATLAS, FURNACE_ATLAS), np.any([furnace_chart_mask(f) for f in range(6)], axis=0))
    inside = tx.points[live]
    assert (np.sort(np.minimum(inside, 1.0 - inside), axis=1)[:, 1] >= 1.0 / 16 - 1e-6).all()  # 1/16 from the nearest edge of its face
    assert (((0.5 - inside) * tx.normals[live]).sum(axis=1) > 0).all()  # the flipped normals point into the cube
    L, rot = furnace_tables()
    ro, rd = nr.occlusion_rays(inside, tx.normals[live], L, rot, 1e-3, np.flatnonzero(live).astype(np.uint64))
    hit, rec = oracle.cast(furnace_scene().descriptor, ro.reshape(-1, 3), rd.reshape(-1, 3))
    assert hit.all() and (rec[:, 4] != 0.0).all()
    # open top: the floor sees the sky
    otx = nr.surface_texels_ref(*furnace_mesh(open_top=True), None, FURNACE_ATLAS, FURNACE_ATLAS, flip_normals=True)
    floor = furnace_chart_mask(FURNACE_FLOOR).reshape(-1)
    assert ((otx.flags & 1) != 0).sum() == 5 * FURNACE_CHART ** 2 and ((otx.flags[floor] & 1) != 0).all()
    ro, rd = nr.occlusion_rays(otx.points[floor], otx.normals[floor], L, rot, 1e-3, np.flatnonzero(floor).astype(np.uint64))
    hit, _ = oracle.cast(furnace_scene(open_top=True).descriptor, ro.reshape(-1, 3), rd.reshape(-1, 3))
    assert (~hit.reshape(-1, 16)).any(axis=1).all()
