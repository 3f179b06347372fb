"""The surface of a mesh node at a light map's texels (nrays_surface_texels_device / nrays_surface_texels; nrays_amd.surface_texels, surface_texels_ref,
bake_lightmap): the parts that need no GPU — the lattice against the project's own texture sampler, the watertightness and the edge cases of the definition
on its numpy mirror, the ABI surface, and the checks the Python wrappers make before any library call.  The meshes below are shared with
tests/test_surface_texels_gpu.py, which holds the device to the mirror bit for bit."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import nrays_amd as nr
from nrays_amd import abi, math3d
from nrays_amd.scene import _texel_edge
from tests import texture_cases as tc
from tools import scenes_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_TEXT = open(os.path.join(ROOT, "include", "nrays_abi.h")).read()
HEADER = re.sub(r"/\*.*?\*/", "", HEADER_TEXT, flags=re.S)
FFI = open(os.path.join(ROOT, "integration", "rust", "src", "gpu_ffi.rs")).read()
GPU_RS = open(os.path.join(ROOT, "integration", "rust", "src", "gpu.rs")).read()
_OUT = ["NraysScene*", "uint32_t", "uint32_t", "uint32_t", "double*", "double*", "double*", "int32_t*", "int32_t*", "uint32_t*", "uint32_t"]
EXPECTED = {"nrays_surface_texels_device": _OUT + ["void*"], "nrays_surface_texels": _OUT,
            "nrays_debug_surface_texels_passes": ["NraysScene*", "uint32_t", "uint32_t", "uint32_t", "uint32_t", "uint32_t", "float*"]}
RUST_TYPES = {"NraysScene*": "*mut NraysScene", "uint32_t": "u32", "double*": "*mut f64", "int32_t*": "*mut i32", "uint32_t*": "*mut u32", "float*": "*mut f32",
              "void*": "*mut c_void"}
LATTICES = (False, True)  # centres
# The lattices on which tests/test_surface_texels_gpu.py compares the jittered grid with the casts: at least 95 % of their covered points are clear of every edge (asserted
# below).  Not 64 x 64 by x / (W - 1): its 252 border points lie ON the outline of the atlas, 6 % of the lattice.
CAST_LATTICES = (((64, 64), True), ((301, 173), False), ((301, 173), True))


# ---- meshes shared with the GPU tests ---------------------------------------------------------------------------------------------------------------------------
def quad():
    """The unit square of two triangles that share the diagonal u == v; uv = (x, y)."""
    p = su.f32_exact([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]])
    return p, np.asarray([[0, 1, 2], [0, 2, 3]], np.uint32), p[:, :2].copy()


def one_triangle():
    p = su.f32_exact([[0.5, 0.25, 1.0], [2.0, 0.5, 0.0], [1.0, 3.0, -0.5]])
    return p, np.asarray([[0, 1, 2]], np.uint32), su.f32_exact([[0.1, 0.05], [0.95, 0.2], [0.3, 0.9]])


@functools.lru_cache(maxsize=None)
def jittered_grid(scale=1.0, angle=0.0):
    """9 x 9 vertices, 128 triangles over the unit uv square, the interior vertices moved by up to 0.03 in uv (f32 uvs); optionally the atlas scaled about its centre
    and rotated.  The surface is a gentle height field over the unjittered grid (f32-exact), so that a ray along a triangle's normal from 1e-3 above it meets it first."""
    rng = np.random.default_rng(77)
    n = 9
    g = np.stack(np.meshgrid(np.arange(n) / (n - 1.0), np.arange(n) / (n - 1.0), indexing="ij"), -1).reshape(-1, 2)
    interior = ((g > 0) & (g < 1)).all(axis=1)
    uv = g + interior[:, None] * rng.uniform(-0.03, 0.03, size=g.shape)
    if scale != 1.0 or angle != 0.0:
        c, s = np.cos(angle), np.sin(angle)
        d = (uv - 0.5) * scale
        uv = 0.5 + np.stack([c * d[:, 0] - s * d[:, 1], s * d[:, 0] + c * d[:, 1]], -1)
    p = np.stack([4.0 * g[:, 0] - 2.0, 0.3 * np.sin(3.0 * g[:, 0]) * np.cos(2.0 * g[:, 1]), 4.0 * g[:, 1] - 2.0], -1)
    i, j = np.meshgrid(np.arange(n - 1), np.arange(n - 1), indexing="ij")
    a = (i * n + j).ravel()
    idx = np.concatenate([np.stack([a, a + n, a + n + 1], 1), np.stack([a, a + n + 1, a + 1], 1)]).astype(np.uint32)
    return su.f32_exact(p), idx, su.f32_exact(uv)


def covers_without_box(uvs, idx, width, height, centres):
    """Owner of every lattice point by the definition WITHOUT the uv-box condition — every triangle against every lattice point — or -1."""
    su_, sv_ = nr.texel_coords(width, centres)[None, :], nr.texel_coords(height, centres)[:, None]
    owner = np.full((height, width), -1, np.int64)
    with np.errstate(all="ignore"):
        for t in range(len(idx) - 1, -1, -1):
            (au, av), (bu, bv), (cu, cv) = ((float(uvs[v, 0]), float(uvs[v, 1])) for v in idx[t])
            area2 = np.float64(bu - au) * np.float64(cv - av) - np.float64(bv - av) * np.float64(cu - au)
            if area2 == 0.0 or not np.isfinite(area2):
                continue
            s = 1.0 if area2 > 0 else -1.0
            e0, e1, e2 = s * _texel_edge(bu, bv, cu, cv, su_, sv_), s * _texel_edge(cu, cv, au, av, su_, sv_), s * _texel_edge(au, av, bu, bv, su_, sv_)
            owner[(e0 >= 0) & (e1 >= 0) & (e2 >= 0) & (((e0 + e1) + e2) != 0)] = t
    return owner


# ---- the lattice is the sampler's ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(2, 2), (3, 5), (8, 8), (64, 33), (1, 4)])
def test_the_default_lattice_is_where_the_sampler_reads_each_texel(size):
    w, h = size
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    texels = np.zeros((h, w, 4), np.float32)
    texels[..., 0], texels[..., 1] = x, y
    u, v = np.meshgrid(nr.texel_coords(w), nr.texel_coords(h))
    x, y, u, v = x.ravel(), y.ravel(), u.ravel(), v.ravel()
    got = tc.sample_ref(texels, tc.NEAREST, tc.CLAMP, u, v).value
    assert np.array_equal(got[:, 0], x) and np.array_equal(got[:, 1], y)
    got = tc.sample_ref(texels, tc.NEAREST, tc.WRAP, u, v).value
    inner = (x < max(w - 1, 1)) & (y < max(h - 1, 1))  # (1.0 % 1.0 wraps the last column and row to texel 0; an axis of one texel has no last one to lose)
    assert inner.any() and np.array_equal(got[inner, 0], x[inner]) and np.array_equal(got[inner, 1], y[inner])
    mirror = nr.surface_texels_ref(*quad(), None, w, h)
    assert np.array_equal(mirror.uv, np.stack([u, v], -1)) and (mirror.flags == 3).all()  # the uv a texel is baked at is the uv it is sampled at


def test_the_centre_lattice_is_the_usual_one():
    assert np.array_equal(nr.texel_coords(4, True), [0.125, 0.375, 0.625, 0.875]) and np.array_equal(nr.texel_coords(1, True), [0.5])
    assert np.array_equal(nr.texel_coords(1), [0.0]) and np.array_equal(nr.texel_coords(3), [0.0, 0.5, 1.0])


# ---- watertightness -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("centres", LATTICES)
@pytest.mark.parametrize("size", [(2, 2), (7, 5), (64, 33), (257, 129)])
def test_the_quad_is_watertight_and_its_diagonal_goes_to_triangle_0(size, centres):
    w, h = size
    t = nr.surface_texels_ref(*quad(), None, w, h, centres=centres)
    assert (t.flags == 3).all() and (t.node == 0).all()
    on_diagonal = t.uv[:, 0] == t.uv[:, 1]
    assert (centres or on_diagonal.sum() >= 2) and (t.prim[on_diagonal] == 0).all()  # (x / (W - 1): at least the two corners)
    assert (t.prim[t.uv[:, 0] > t.uv[:, 1]] == 0).all() and (t.prim[t.uv[:, 0] < t.uv[:, 1]] == 1).all()
    # uv = (x, y): the point is the lattice point, up to the rounding of three weights (1.5 u each), three products and two sums of values <= 1: 6 u < 1e-15
    assert np.abs(t.points[:, :2] - t.uv).max() < 1e-15 and np.array_equal(t.normals, np.tile([0.0, 0.0, 1.0], (w * h, 1)))


@pytest.mark.parametrize("centres", LATTICES)
@pytest.mark.parametrize("size", [(64, 64), (301, 173)])
def test_the_jittered_grid_is_watertight(size, centres):
    p, idx, uv = jittered_grid()
    t, wts = nr.surface_texels_ref(p, idx, uv, None, *size, centres=centres, with_weights=True)
    assert (t.flags == 3).all() and t.prim.min() >= 0 and t.prim.max() < len(idx)
    assert np.abs(wts.sum(axis=1) - 1.0).max() <= 4e-16 and wts.min() >= 0.0
    # what tests/test_surface_texels_gpu.py compares with the casts: the texels clear of every edge are at least 95 % of the covered ones on these lattices
    if (size, centres) in CAST_LATTICES:
        assert (wts.min(axis=1) > 1e-9).sum() >= 0.95 * (t.flags == 3).sum()


@pytest.mark.parametrize("size", [(64, 64), (301, 173)])
def test_the_scaled_and_rotated_grid_is_watertight_inside_its_outline(size):
    p, idx, uv = jittered_grid(0.6, 0.3)
    t = nr.surface_texels_ref(p, idx, uv, None, *size)
    c, s = np.cos(0.3), np.sin(0.3)
    d = np.stack(np.meshgrid(nr.texel_coords(size[0]), nr.texel_coords(size[1])), -1).reshape(-1, 2) - 0.5
    back = np.stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1]], -1) / 0.6
    inside = (np.abs(back) < 0.5 - 1e-6).all(axis=1)  # strictly inside the outline (its f32 corners are within 1e-7 of the exact square)
    outside = (np.abs(back) > 0.5 + 1e-6).any(axis=1)
    assert inside.sum() > 0.3 * len(inside) and (t.flags[inside] == 3).all() and (t.flags[outside] == 0).all()
    assert (t.node[outside] == -1).all() and (t.prim[outside] == -1).all() and not t.points[outside].any() and not t.normals[outside].any() and not t.uv[outside].any()


@pytest.mark.parametrize("centres", LATTICES)
def test_the_uv_box_of_the_definition_excludes_nothing(centres):
    """The definition asks a lattice point to lie in the triangle's uv box; on these meshes every-triangle-against-every-point without the box gives the same owners."""
    for (p, idx, uv), size in ((quad(), (7, 5)), (quad(), (64, 33)), (one_triangle(), (5, 3)), (jittered_grid(), (64, 64)), (jittered_grid(0.6, 0.3), (61, 47))):
        t = nr.surface_texels_ref(p, idx, uv, None, *size, centres=centres)
        assert np.array_equal(t.prim.reshape(size[1], size[0]), covers_without_box(uv, idx, size[0], size[1], centres))


# ---- edge cases ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_degenerate_and_non_finite_triangles_cover_nothing():
    p = su.f32_exact([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [2, 2, 2]])
    inf, nan = np.inf, np.nan
    for uv5, tri in (([0.5, 0.5], [0, 2, 4]),      # a zero-area sliver along the diagonal, through lattice points
                     ([0.0, 0.0], [0, 4, 4]),      # a point
                     ([inf, 0.5], [0, 1, 4]), ([nan, 0.5], [0, 1, 4]), ([3e38, -3e38], [4, 1, 3])):  # area2 = inf, NaN, and 3e38 * 3e38 = inf
        uv = np.asarray([[0, 0], [1, 0], [1, 1], [0, 1], uv5], np.float64)
        t = nr.surface_texels_ref(p, [tri], uv, None, 9, 9)
        assert not t.flags.any() and (t.prim == -1).all() and (t.node == -1).all() and not t.points.any() and not t.uv.any(), (uv5, tri)
        both = nr.surface_texels_ref(p, [tri, [0, 1, 2], [0, 2, 3]], uv, None, 9, 9)  # ... and takes nothing from the triangles behind it
        assert (both.flags == 3).all() and (both.prim >= 1).all()


@pytest.mark.parametrize("centres", LATTICES)
def test_huge_uvs_cover_only_what_they_contain(centres):
    """A corner at +-3e38 with a finite area2: the box is clamped, and the lattice points covered are those an exact test finds."""
    p = su.f32_exact([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
    for far in ([3e38, 0.25], [-3e38, 0.75], [0.5, 3e38], [0.5, -3e38]):
        uv = su.f32_exact([[0.25, 0.25], [0.75, 0.5], far])
        if not np.isfinite((uv[1, 0] - uv[0, 0]) * (uv[2, 1] - uv[0, 1]) - (uv[1, 1] - uv[0, 1]) * (uv[2, 0] - uv[0, 0])):
            continue
        t = nr.surface_texels_ref(p, [[0, 1, 2]], uv, None, 16, 12, centres=centres)
        assert np.isfinite(t.points).all()
        from fractions import Fraction as F
        A, B, Cc = ([F(float(x)) for x in row] for row in uv)
        area = (B[0] - A[0]) * (Cc[1] - A[1]) - (B[1] - A[1]) * (Cc[0] - A[0])
        sgn = 1 if area > 0 else -1
        xs, ys = nr.texel_coords(16, centres), nr.texel_coords(12, centres)
        for y in range(12):
            for x in range(16):
                q = (F(float(xs[x])), F(float(ys[y])))
                e = [sgn * ((Q[0] - P[0]) * (q[1] - P[1]) - (Q[1] - P[1]) * (q[0] - P[0])) for P, Q in ((B, Cc), (Cc, A), (A, B))]
                if min(e) > 0:
                    assert t.flags[y * 16 + x] == 3, (far, x, y)
                elif min(e) < 0:
                    assert t.flags[y * 16 + x] == 0, (far, x, y)
    t = nr.surface_texels_ref(p, [[0, 1, 2]], su.f32_exact([[-5.0, -5.0], [-4.0, -5.0], [-5.0, -4.0]]), None, 16, 12)  # beside the lattice: uvs are not wrapped
    assert not t.flags.any()


def test_of_two_stacked_triangles_the_smaller_index_wins_in_either_order():
    p = su.f32_exact([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 5], [1, 0, 5], [0, 1, 5]])
    uv = su.f32_exact([[0, 0], [1, 0], [0, 1], [0, 0], [0.5, 0], [0, 0.5]])
    for order in ([[0, 1, 2], [3, 4, 5]], [[3, 4, 5], [0, 1, 2]]):
        t = nr.surface_texels_ref(p, order, uv, None, 9, 9)
        at = np.stack(np.meshgrid(nr.texel_coords(9), nr.texel_coords(9)), -1).reshape(-1, 2).sum(axis=1)  # (multiples of 1 / 8: exact)
        small, big = at <= 0.5, at <= 1.0
        assert np.array_equal(t.flags == 3, big) and small.sum() == 15
        assert (t.prim[small] == 0).all() and (t.prim[big & ~small] == (1 if order[0] == [3, 4, 5] else 0)).all()
        assert (t.points[small, 2] == (5.0 if order[0] == [3, 4, 5] else 0.0)).all()


def test_the_transform_and_the_flipped_normal():
    p, idx, uv = jittered_grid()
    iso = nr.Isometry3((0.5, -1.25, 2.0), (0.3, -0.7, 0.2))
    plain = nr.surface_texels_ref(p, idx, uv, None, 33, 17)
    moved = nr.surface_texels_ref(p, idx, uv, iso, 33, 17, flip_normals=True, node=3)
    R = math3d.rotation_from_axis_angle(iso.axis_angle)
    assert np.abs(R @ R.T - np.eye(3)).max() < 1e-15 and np.array_equal(math3d.rotation_from_axis_angle((0, 0, 0)), np.eye(3))
    assert np.array_equal(moved.prim, plain.prim) and (moved.node == 3).all() and np.array_equal(moved.uv, plain.uv)
    assert np.abs(moved.points - (plain.points @ R.T + iso.translation)).max() < 1e-14 and np.abs(moved.normals + plain.normals @ R.T).max() < 1e-15
    assert np.abs((plain.normals ** 2).sum(axis=1) - 1.0).max() < 1e-15
    shifted = nr.surface_texels_ref(p, idx, uv, nr.Isometry3((0.5, -1.25, 2.0)), 33, 17)
    assert np.array_equal(shifted.points, plain.points + np.asarray([0.5, -1.25, 2.0])) and np.array_equal(shifted.normals, plain.normals)


# ---- the surface of the ABI -----------------------------------------------------------------------------------------------------------------------------------------
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
    for c_type, ct in zip(EXPECTED[name], args):
        assert (ct is C.c_uint32) == (c_type == "uint32_t"), (c_type, ct)
    m = re.search(r"pub fn %s\((.*?)\) -> c_int;" % name, FFI)
    assert m, "%s is not declared in gpu_ffi.rs" % name
    assert [p.split(": ", 1)[1] for p in m.group(1).split(", ")] == [RUST_TYPES[t] for t in EXPECTED[name]]
    assert "pub fn surface_texels(" in GPU_RS and "pub unsafe fn surface_texels_device(" in GPU_RS
    assert "nrays_surface_texels(" in GPU_RS and "nrays_surface_texels_device(" in GPU_RS


def test_the_flag_constants_agree():
    for name, value, py in (("NRAYS_TEXELS_CENTRES", 1, abi.TEXELS_CENTRES), ("NRAYS_TEXELS_FLIP_NORMALS", 2, abi.TEXELS_FLIP_NORMALS)):
        assert re.search(r"#define %s\s+%du\b" % (name, value), HEADER) and py == value
        assert re.search(r"pub const %s: u32 = %d;" % (name, value), FFI)


def test_the_abi_version_is_still_7(built):
    assert re.search(r"#define NRAYS_ABI_VERSION 7\b", HEADER) and abi.ABI_VERSION == 7 and abi.load_hip_lib().nrays_abi_version() == 7
    note = re.search(r"Added after 7 WITHOUT a bump.*?\*/", HEADER_TEXT, re.S).group(0)
    exported = subprocess.check_output(["nm", "-D", "--defined-only", abi.HIP_LIB_PATH]).decode()
    for name in EXPECTED:
        assert re.search(r"%s\b" % name, note), name
        assert (" T " + name + "\n") in exported, name
        assert getattr(abi.load_hip_lib(), name).argtypes == abi.HIP_SYMBOLS[name][1]


def test_without_a_scene_every_call_is_a_bad_arg(built):
    """The one status that needs no device; the others need a scene: tests/test_surface_texels_gpu.py."""
    lib = abi.load_hip_lib()
    p, f, ms = (C.c_double * 3)(7.0, 7.0, 7.0), (C.c_uint32 * 1)(7), (C.c_float * 2)(7.0, 7.0)
    adr = C.addressof
    for flags in (0, 1, 2, 3, 4):
        assert lib.nrays_surface_texels(None, 0, 1, 1, p, None, None, None, None, f, flags) == abi.ERR_BAD_ARG
        assert lib.nrays_surface_texels_device(None, 0, 1, 1, adr(p), None, None, None, None, adr(f), flags, None) == abi.ERR_BAD_ARG
        assert lib.nrays_debug_surface_texels_passes(None, 0, 1, 1, flags, 1, ms) == abi.ERR_BAD_ARG
    assert lib.nrays_last_error() and list(p) == [7.0] * 3 and f[0] == 7 and list(ms) == [7.0, 7.0]


# ---- the Python wrappers check before any library call --------------------------------------------------------------------------------------------------------------
class _NoDevice:
    def device_handle(self):
        raise AssertionError("device touched before the arguments were checked")


@pytest.fixture()
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(abi, "load_hip_lib", refuse)


@pytest.mark.parametrize("kw", [dict(width=0), dict(height=0), dict(width=16385), dict(width=8192, height=4096), dict(node=-1), dict(want=("normals", "toi")), dict(device="cpu")])
def test_the_wrappers_reject_bad_arguments_before_any_library_call(no_library, kw):
    args = dict(node=0, width=4, height=4)
    args.update(kw)
    with pytest.raises(ValueError):
        nr.surface_texels(_NoDevice(), **args)
    if "want" not in kw:
        with pytest.raises(ValueError):
            nr.bake_lightmap(_NoDevice(), **args)
    if "width" in kw or "height" in kw:
        with pytest.raises(ValueError):
            nr.surface_texels_ref(*quad(), None, args["width"], args["height"])


def test_scene_and_filescene_carry_the_methods():
    from nrays_amd import scenefile
    for cls in (nr.Scene, scenefile.FileScene):
        assert callable(cls.surface_texels) and callable(cls.bake_lightmap)
    assert nr.SurfaceTexels._fields == ("points", "normals", "uv", "node", "prim", "flags")
