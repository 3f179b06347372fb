"""Gutter dilation of a baked light map (nrays_dilate_texels_device / nrays_dilate_texels; nrays_amd.dilate_texels, dilate_texels_ref, lightmap_texture): the
numpy mirror against a brute force written straight from the definition in include/nrays_abi.h, the hand cases of that definition, and the declarations at
every layer.  Nothing here needs a GPU; the device is held to the mirror, bit for bit, by tests/test_dilate_texels_gpu.py."""
import os
import re

import numpy as np
import pytest

import nrays_amd as nr
from nrays_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "nrays_abi.h")).read()
GPU_FFI = open(os.path.join(ROOT, "integration", "rust", "src", "gpu_ffi.rs")).read()
GPU_RS = open(os.path.join(ROOT, "integration", "rust", "src", "gpu.rs")).read()


def brute_force(flags, w, h, r, values=None):
    """The definition, O(n r^2): per uncovered point the covered points of the disc, the smallest (d2, index)."""
    f = np.asarray(flags, dtype=np.uint32).reshape(h, w)
    n = w * h
    source, out_flags = np.full(n, -1, np.int32), f.reshape(n).copy()
    out = None if values is None else np.array(values, copy=True)
    words = None if out is None else out.view(np.uint32).reshape(n, -1)
    before = None if words is None else words.copy()
    for y in range(h):
        for x in range(w):
            i = y * w + x
            if f[y, x] & 1:
                source[i] = i
                continue
            best = None
            for yy in range(max(0, y - r), min(h, y + r + 1)):
                for xx in range(max(0, x - r), min(w, x + r + 1)):
                    d2 = (xx - x) ** 2 + (yy - y) ** 2
                    if (f[yy, xx] & 1) and d2 <= r * r and (best is None or (d2, yy * w + xx) < best):
                        best = (d2, yy * w + xx)
            if best is not None:
                source[i] = best[1]
                out_flags[i] |= 4
                if words is not None:
                    words[i] = before[best[1]]
    return out, source, out_flags


def same(got, want):
    assert (got[0] is None) == (want[0] is None)
    if got[0] is not None:
        assert got[0].shape == want[0].shape and np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
    assert got[1].dtype == np.int32 and np.array_equal(got[1], want[1])
    assert got[2].dtype == np.uint32 and np.array_equal(got[2], want[2])


SPECIALS = np.asarray([0x7fc01234, 0xffc00001, 0x80000000, 0x7f800000, 0xff800000, 0x00000001, 0x807fffff], np.uint32).view(np.float32)  # NaNs with payloads, -0, +-inf, denormals


def random_values(rng, n, channels):
    v = rng.standard_normal((n, channels)).astype(np.float32)
    pick = rng.random((n, channels)) < 0.3
    v[pick] = SPECIALS[rng.integers(0, len(SPECIALS), int(pick.sum()))]
    return v


@pytest.mark.parametrize("coverage", [0.02, 0.10, 0.50, 0.90])
def test_the_mirror_equals_the_brute_force(coverage):
    rng = np.random.default_rng(int(coverage * 100))
    for _ in range(50):
        w, h, r, channels = int(rng.integers(1, 14)), int(rng.integers(1, 14)), int(rng.integers(1, 7)), int(rng.integers(1, 5))
        flags = ((rng.random(w * h) < coverage).astype(np.uint32) | (rng.integers(0, 4, w * h).astype(np.uint32) << 1))  # bit 0 = covered; bits 1, 2 noise
        values = random_values(rng, w * h, channels)
        kept = values.copy()
        same(nr.dilate_texels_ref(flags, w, h, r, values), brute_force(flags, w, h, r, values))
        assert np.array_equal(values.view(np.uint32), kept.view(np.uint32))  # the mirror returns a copy
        same(nr.dilate_texels_ref(flags.reshape(h, w), w, h, r), brute_force(flags, w, h, r))


def test_a_single_source_fills_exactly_the_disc():
    w = h = 15
    r, c = 5, 7
    flags = np.zeros(w * h, np.uint32)
    flags[c * w + c] = 3
    values = np.zeros((h, w, 2), np.float32)
    values[c, c] = (1.5, -2.5)
    v, source, out_flags = nr.dilate_texels_ref(flags, w, h, r, values)
    yy, xx = np.mgrid[0:h, 0:w]
    disc = (xx - c) ** 2 + (yy - c) ** 2 <= r * r
    assert np.array_equal(source.reshape(h, w) == c * w + c, disc) and (source.reshape(h, w)[~disc] == -1).all()
    assert source[(c + 4) * w + c + 3] == c * w + c and source[(c + 1) * w + c + 5] == -1  # offset (3, 4): d2 = 25, filled; (5, 1): d2 = 26, not
    assert np.array_equal(out_flags.reshape(h, w) == 4, disc & (flags.reshape(h, w) == 0)) and out_flags[c * w + c] == 3
    assert (v[disc] == (1.5, -2.5)).all() and not v[~disc].any()


@pytest.mark.parametrize("a,b,at", [((1, 2), (3, 2), (2, 2)), ((2, 1), (2, 3), (2, 2)), ((1, 1), (3, 3), (2, 2)), ((3, 1), (1, 3), (2, 2)), ((1, 2), (2, 1), (2, 2))],
                         ids=["left_right", "above_below", "diagonal", "antidiagonal", "row_vs_column"])
def test_of_two_equidistant_sources_the_smaller_index_wins(a, b, at):
    w = h = 5
    flags = np.zeros(w * h, np.uint32)
    ia, ib = a[1] * w + a[0], b[1] * w + b[0]
    flags[[ia, ib]] = 1
    _, source, _ = nr.dilate_texels_ref(flags, w, h, 3)
    assert source[at[1] * w + at[0]] == min(ia, ib)
    same(nr.dilate_texels_ref(flags, w, h, 3), brute_force(flags, w, h, 3))


def test_nothing_covered_and_everything_covered():
    w, h = 6, 4
    values = np.arange(w * h * 3, dtype=np.float32).reshape(w * h, 3)
    v, source, out_flags = nr.dilate_texels_ref(np.zeros(w * h, np.uint32), w, h, 64, values)
    assert (source == -1).all() and not out_flags.any() and np.array_equal(v, values)
    v, source, out_flags = nr.dilate_texels_ref(np.full(w * h, 3, np.uint32), w, h, 2, values)
    assert np.array_equal(source, np.arange(w * h)) and (out_flags == 3).all() and np.array_equal(v, values)


def test_only_bit_0_covers():
    flags = np.asarray([2, 3, 2], np.uint32)  # 2: uncovered, 3: covered
    v, source, out_flags = nr.dilate_texels_ref(flags, 3, 1, 1, np.asarray([1.0, 2.0, 3.0], np.float32))
    assert source.tolist() == [1, 1, 1] and out_flags.tolist() == [6, 3, 6] and v.tolist() == [2.0, 2.0, 2.0]


def test_the_mirror_is_quick_on_a_large_atlas():
    """Vectorised: a 1024^2 atlas of 16 x 16 charts with 4-texel gutters well inside a second (the Python loop per texel would take minutes)."""
    import time
    yy, xx = np.mgrid[0:1024, 0:1024]
    flags = (((xx % 20) < 16) & ((yy % 20) < 16)).astype(np.uint32) * 3
    t0 = time.perf_counter()
    _, source, out_flags = nr.dilate_texels_ref(flags, 1024, 1024, 8)
    assert time.perf_counter() - t0 < 10.0 and (source >= 0).all() and ((out_flags == 4) == (flags.reshape(-1) == 0)).all()


# ---- the declarations, layer by layer ----------------------------------------------------------------------------------------------------------------------------
_ARGS = ["NraysScene*", "uint32_t", "uint32_t", "const uint32_t*", "uint32_t", "uint32_t", "float*", "int32_t*", "uint32_t*", "uint32_t"]
EXPECTED = {"nrays_dilate_texels_device": _ARGS + ["void*"], "nrays_dilate_texels": _ARGS}


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_the_header_declares_the_entry_points(name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, HEADER)
    assert m, name
    types = [re.sub(r"\s*\w+$", "", a.strip()).replace(" *", "*") for a in m.group(1).split(",")]
    assert types == EXPECTED[name]
    assert name in abi.HIP_SYMBOLS and name in abi.POST_V7_SYMBOLS
    res, args = abi.HIP_SYMBOLS[name]
    assert len(args) == len(EXPECTED[name])


def test_constants_and_version():
    assert re.search(r"#define\s+NRAYS_DILATE_MAX_RADIUS\s+64u\b", HEADER) and re.search(r"#define\s+NRAYS_TEXEL_FILLED\s+4u\b", HEADER)
    assert (abi.DILATE_MAX_RADIUS, abi.TEXEL_FILLED) == (64, 4)
    assert re.search(r"#define\s+NRAYS_ABI_VERSION\s+7\b", HEADER) and abi.ABI_VERSION == 7


def test_the_library_exports_them(built):
    lib = abi.load_hip_lib()
    for name in EXPECTED:
        assert getattr(lib, name).argtypes == abi.HIP_SYMBOLS[name][1]
    import ctypes as C
    f, s = (C.c_uint32 * 1)(1), (C.c_int32 * 1)(7)
    assert lib.nrays_dilate_texels(None, 1, 1, f, 1, 0, None, s, None, 0) == abi.ERR_BAD_ARG and s[0] == 7  # the one status that needs no scene
    assert lib.nrays_dilate_texels_device(None, 1, 1, None, 1, 0, None, None, None, 0, None) == abi.ERR_BAD_ARG


def test_the_rust_side_declares_and_calls_them():
    for name in EXPECTED:
        assert re.search(r"pub fn %s\(" % name, GPU_FFI), name
        assert name + "(" in GPU_RS, name
    assert "pub fn dilate_texels(" in GPU_RS and "pub unsafe fn dilate_texels_device(" in GPU_RS
    assert "NRAYS_TEXEL_FILLED" in GPU_FFI and "NRAYS_DILATE_MAX_RADIUS" in GPU_FFI


# ---- the wrappers ---------------------------------------------------------------------------------------------------------------------------------------------------
class _NoDevice:
    def device_handle(self):
        raise AssertionError("device touched before the arguments were checked")


@pytest.fixture()
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(abi, "load_hip_lib", refuse)


@pytest.mark.parametrize("kw", [dict(radius=0), dict(radius=65), dict(width=0), dict(width=16385, height=1), dict(flags=np.zeros(15, np.uint32)),
                                dict(values=np.zeros((16, 5), np.float32)), dict(values=np.zeros(17, np.float32))])
def test_the_wrappers_reject_bad_arguments_before_any_library_call(no_library, kw):
    args = dict(flags=np.zeros(16, np.uint32), width=4, height=4, radius=2)
    args.update(kw)
    with pytest.raises(ValueError):
        nr.dilate_texels(_NoDevice(), **args)
    with pytest.raises(ValueError):
        nr.dilate_texels_ref(**args)


def test_the_bakers_take_dilate_and_the_methods_exist(monkeypatch):
    """bake_lightmap has `dilate` as a parameter; bake_indirect and its methods, whose positional parameters end with `unordered`, take it by keyword only.
    Neither reaches the library here: surface_texels, the two kernels' callers and dilate_texels are replaced."""
    from nrays_amd import scenefile
    import inspect
    for cls in (nr.Scene, scenefile.FileScene):
        assert callable(cls.dilate_texels)
        assert inspect.signature(cls.bake_lightmap).parameters["dilate"].default == 0
        assert list(inspect.signature(cls.bake_indirect).parameters)[-1] == "unordered"
    assert inspect.signature(nr.bake_lightmap).parameters["dilate"].default == 0
    for fn in (nr.bake_lightmap, nr.bake_indirect):
        assert "dilate >= 2" in fn.__doc__
    n, L = 6, nr.hemisphere_dirs(4)
    tx = nr.SurfaceTexels(points=np.zeros((n, 3)), normals=np.tile([0.0, 1.0, 0.0], (n, 1)), uv=np.zeros((n, 2)), node=np.zeros(n, np.int32), prim=None,
                          flags=np.asarray([3, 0, 3, 0, 0, 3], np.uint32))
    calls, wanted = [], []
    monkeypatch.setattr(nr.scene, "surface_texels", lambda *a, **kw: wanted.append(kw.get("want")) or tx)
    monkeypatch.setattr(nr.scene, "gather_points", lambda scene, points, *a, **kw: np.ones((len(points), 3), np.float32))
    monkeypatch.setattr(nr.scene, "shade_points", lambda scene, points, *a, **kw: np.ones((len(points), 4), np.float32))

    def fake_dilate(scene, flags, width, height, radius, values=None, want_source=False, device=None):
        calls.append((width, height, radius, values.shape))
        assert flags is tx.flags and values.flags.c_contiguous
        values[flags == 0] = 2.0  # in place
        return values, None, flags
    monkeypatch.setattr(nr.scene, "dilate_texels", fake_dilate)
    sc = _NoDevice()
    fake_self = type("S", (), {"device_handle": sc.device_handle})()
    for bake, args in ((nr.bake_indirect, (sc, 0, 3, 2, L)), (nr.Scene.bake_indirect, (fake_self, 0, 3, 2, L)), (scenefile.FileScene.bake_indirect, (fake_self, 0, 3, 2, L)),
                       (nr.bake_lightmap, (sc, 0, 3, 2)), (nr.Scene.bake_lightmap, (fake_self, 0, 3, 2)), (scenefile.FileScene.bake_lightmap, (fake_self, 0, 3, 2))):
        del calls[:]
        plain = bake(*args)
        assert not calls and (plain == 1.0).all() and np.array_equal(bake(*args, dilate=0), plain)  # 0 = off: nothing more is called
        n_texel_calls = len(wanted)
        got = bake(*args, dilate=3)
        assert calls == [(3, 2, 3, (n, plain.shape[-1]))] and got.shape == plain.shape == (2, 3, plain.shape[-1])
        assert (got.reshape(n, -1)[tx.flags == 0] == 2.0).all() and (got.reshape(n, -1)[tx.flags != 0] == 1.0).all()
        assert len(wanted) - n_texel_calls == (2 if "indirect" in bake.__name__ else 1)  # bake_indirect's keyword asks surface_texels for the flags once more ...
        if "indirect" in bake.__name__:
            assert wanted[-1] == ()                                                       # ... and for nothing else
        for bad in (-1, 65):
            with pytest.raises(ValueError):
                bake(*args, dilate=bad)
        assert len(calls) == 1


def test_lightmap_texture():
    rgba = np.arange(2 * 3 * 4, dtype=np.float64).reshape(2, 3, 4)
    t = nr.lightmap_texture(rgba)
    assert isinstance(t, nr.Texture2d) and t.interpol == nr.Interpolation.Bilinear and t.overflow == nr.Overflow.ClampToEdges
    assert t.data.format == abi.TEXEL_RGBA32F
    with pytest.raises(ValueError):
        nr.lightmap_texture(np.zeros((2, 3, 3), np.float32))
