"""Denoising of a baked light map (nrays_filter_texels_device / nrays_filter_texels; nrays_amd.filter_texels, filter_texels_ref, denoise_texels): the
vectorised numpy mirror against a plain per-texel loop written straight from the definition in include/nrays_abi.h, the hand cases of that definition,
what the filter is for (no leak between charts, the variance it removes), and the declarations at every layer.  Nothing here needs a GPU; the device is
held to the mirror, bit for bit, by tests/test_filter_texels_gpu.py."""
import math
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
F32, F64 = np.float32, np.float64
H = (1, 4, 6, 4, 1)


def per_texel_loop(flags, w, h, points, normals, values, step, pos_radius, normal_cos):
    """The definition, one texel and one tap at a time, in numpy scalars: float64 where it says f64, float32 where it says f32."""
    f = np.asarray(flags, dtype=np.uint32).reshape(-1)
    p, nm = np.asarray(points, F64).reshape(-1, 3), np.asarray(normals, F64).reshape(-1, 3)
    v = np.asarray(values, F32).reshape(w * h, -1)
    out = v.copy()
    r, cos = F64(pos_radius), F64(normal_cos)
    with np.errstate(all="ignore"):
        for y in range(h):
            for x in range(w):
                c0 = y * w + x
                if not f[c0] & 1:
                    continue
                acc, wsum = [F32(0.0)] * v.shape[1], F32(0.0)
                for j in range(-2, 3):
                    for i in range(-2, 3):
                        xx, yy = x + i * step, y + j * step
                        if not (0 <= xx < w and 0 <= yy < h) or not f[yy * w + xx] & 1:
                            continue
                        t = yy * w + xx
                        if i == 0 and j == 0:
                            wt = F32(36.0)
                        else:
                            k = F32(H[i + 2] * H[j + 2])
                            dx, dy, dz = p[t][0] - p[c0][0], p[t][1] - p[c0][1], p[t][2] - p[c0][2]
                            d2 = (dx * dx + dy * dy) + dz * dz
                            wp = F64(1.0) - d2 / (r * r)
                            if not wp > 0:
                                continue
                            c = (nm[c0][0] * nm[t][0] + nm[c0][1] * nm[t][1]) + nm[c0][2] * nm[t][2]
                            wn = (c - cos) / (F64(1.0) - cos)
                            if not wn > 0:
                                continue
                            if wn > 1:
                                wn = F64(1.0)
                            wt = (k * F32(wp)) * F32(wn)
                        acc = [a + wt * s for a, s in zip(acc, v[t])]
                        wsum = wsum + wt
                out[c0] = [a / wsum for a in acc]
    return out.reshape(np.shape(values))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(got, want):
    """Equal by bit pattern, NaN payloads included."""
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32
    assert np.array_equal(bits(got), bits(want)), int((bits(got) != bits(want)).sum())


SPECIALS = np.asarray([0x7fc01234, 0xffc00001, 0x80000000, 0x7f800000, 0xff800000, 0x00000001, 0x807fffff], np.uint32).view(np.float32)  # NaNs with payloads, -0, +-inf, denormals


def surface(rng, w, h, coverage, channels, special_share=0.0):
    """A jittered height field with jittered unit normals: every weight of the definition takes values in (0, 1), is clamped, and is skipped somewhere."""
    yy, xx = np.mgrid[0:h, 0:w]
    p = np.stack([xx * 0.1, rng.standard_normal((h, w)) * 0.05, yy * 0.1], -1) + rng.standard_normal((h, w, 3)) * 0.01
    nm = np.asarray([0.0, 1.0, 0.0]) + rng.standard_normal((h, w, 3)) * 0.6
    nm /= np.linalg.norm(nm, axis=-1, keepdims=True)
    flags = (rng.random(w * h) < coverage).astype(np.uint32) | (rng.integers(0, 4, w * h).astype(np.uint32) << 1)  # bit 0 = covered; bits 1, 2 noise
    v = rng.standard_normal((w * h, channels)).astype(np.float32)
    if special_share:
        pick = rng.random(v.shape) < special_share
        v[pick] = SPECIALS[rng.integers(0, len(SPECIALS), int(pick.sum()))]
    return flags, p.reshape(-1, 3), nm.reshape(-1, 3), v


@pytest.mark.parametrize("coverage", [0.0, 0.6, 1.0])
@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (17, 19), (33, 16)])
def test_the_mirror_equals_the_per_texel_loop(w, h, coverage):
    rng = np.random.default_rng(w * 100 + h + int(coverage * 10))
    for k, step in enumerate((1, 2, 3, 64)):
        channels = (1, 3, 4)[(k + w) % 3]
        flags, p, nm, v = surface(rng, w, h, coverage, channels, special_share=0.05 if k % 2 else 0.0)
        pos_radius, normal_cos = ((0.35 * step, 0.3), (math.inf, -1.0), (0.2 * step, -0.5), (1e3, 0.9))[k]
        kept = v.copy()
        got = nr.filter_texels_ref(flags, w, h, p, nm, v, step, pos_radius, normal_cos)
        same_bits(got, per_texel_loop(flags, w, h, p, nm, v, step, pos_radius, normal_cos))
        assert np.array_equal(bits(v), bits(kept)) and got is not v  # a new array
        unc = (flags & 1) == 0
        assert np.array_equal(bits(got)[unc], bits(v)[unc])
        same_bits(nr.filter_texels_ref(flags.reshape(h, w), w, h, p.reshape(h, w, 3), nm.reshape(h, w, 3), v.reshape(h, w, channels), step, pos_radius, normal_cos).reshape(-1, channels), got)


@pytest.mark.parametrize("channels", [1, 3, 4])
def test_every_channel_count_on_one_surface(channels):
    rng = np.random.default_rng(channels)
    flags, p, nm, v = surface(rng, 17, 19, 0.6, channels, special_share=0.02)
    for step in (1, 2):
        same_bits(nr.filter_texels_ref(flags, 17, 19, p, nm, v, step, 0.4, 0.2), per_texel_loop(flags, 17, 19, p, nm, v, step, 0.4, 0.2))
    c0 = nr.filter_texels_ref(flags, 17, 19, p, nm, np.ascontiguousarray(v[:, :1]), 1, 0.4, 0.2)
    same_bits(c0, np.ascontiguousarray(nr.filter_texels_ref(flags, 17, 19, p, nm, v, 1, 0.4, 0.2)[:, :1]))  # the channels do not mix


def test_a_step_larger_than_the_lattice_leaves_the_centre_tap():
    rng = np.random.default_rng(7)
    flags, p, nm, v = surface(rng, 20, 20, 0.8, 3, special_share=0.1)
    v[0] = (3.0e38, -3.0e38, 1e-45)  # 36 v overflows; a denormal
    flags[0] |= 1
    got = nr.filter_texels_ref(flags, 20, 20, p, nm, v, 64)
    with np.errstate(all="ignore"):
        want = np.where(((flags & 1) != 0)[:, None], (np.float32(0.0) + np.float32(36.0) * v) / np.float32(36.0), v)  # acc starts at +0: a -0 comes out as +0
    same_bits(got, want)
    assert np.isinf(got[0, :2]).all()
    same_bits(nr.filter_texels_ref(flags, 20, 20, p, nm, v, 20), want)  # x + 20 is the first point outside
    assert not np.array_equal(bits(nr.filter_texels_ref(flags, 20, 20, p, nm, v, 19)), bits(want))


def test_only_bit_0_covers():
    flags = np.asarray([2, 3, 2, 1, 6], np.uint32)  # covered: 1 and 3
    p, nm = np.zeros((5, 3)), np.tile([0.0, 1.0, 0.0], (5, 1))
    v = np.asarray([100.0, 1.0, 100.0, 3.0, 100.0], np.float32)
    got = nr.filter_texels_ref(flags, 5, 1, p, nm, v, 1)
    # texel 1: centre 36 * 1 and the tap at +2 (k = 6 * 1, wp = wn = 1): (36 + 18) / 42; texel 3: the tap at -2 first
    assert got.tolist() == [100.0, float(F32(F32(36.0) + F32(18.0)) / F32(42.0)), 100.0, float(F32(F32(6.0) + F32(108.0)) / F32(42.0)), 100.0]


def test_uncovered_texels_keep_their_words():
    rng = np.random.default_rng(3)
    flags, p, nm, v = surface(rng, 9, 7, 0.5, 4)
    unc = np.flatnonzero((flags & 1) == 0)
    words = np.asarray([0x7fc01234, 0xffc00001, 0x80000000, 0x7fa00001], np.uint32)  # quiet and signalling NaNs with payloads, -0
    v.view(np.uint32)[unc] = words
    got = nr.filter_texels_ref(flags, 9, 7, p, nm, v, 1, 0.5, 0.0)
    assert len(unc) > 5 and (bits(got)[unc] == words).all()
    assert np.isfinite(got[(flags & 1) != 0]).all()  # and nothing of them reaches a covered texel


def _two_charts(gap, second_normal):
    """Two 8 x 8 charts side by side in a 16 x 8 lattice: they touch in the lattice, the second lies `gap` away in the world with normal `second_normal`."""
    w, h = 16, 8
    yy, xx = np.mgrid[0:h, 0:w]
    right = xx >= 8
    p = np.stack([xx * 0.1 + right * gap, np.zeros((h, w)), yy * 0.1], -1)
    nm = np.where(right[..., None], np.asarray(second_normal, np.float64), np.asarray([0.0, 1.0, 0.0]))
    rng = np.random.default_rng(11)
    v = np.where(right[..., None], 10.0 + rng.random((h, w, 3)), rng.random((h, w, 3))).astype(np.float32)
    return w, h, right, p, nm, v


@pytest.mark.parametrize("case", ["far_apart", "right_angle"])
def test_nothing_leaks_between_two_charts_that_touch_in_the_lattice(case):
    pos_radius = 1.0
    if case == "far_apart":
        w, h, right, p, nm, v = _two_charts(100.0 * pos_radius, (0.0, 1.0, 0.0))
        kw = dict(pos_radius=pos_radius, normal_cos=-1.0)
    else:
        w, h, right, p, nm, v = _two_charts(0.0, (1.0, 0.0, 0.0))
        kw = dict(pos_radius=math.inf, normal_cos=0.5)
    flags = np.ones(w * h, np.uint32)
    out = v
    for step in (1, 2, 4):
        out = nr.filter_texels_ref(flags, w, h, p, nm, out, step, **kw)
        assert (out[~right] <= 1.0).all() and (out[right] >= 10.0).all(), step
    assert not np.array_equal(out, v)
    leaky = nr.filter_texels_ref(flags, w, h, p, nm, v, 1, math.inf, -1.0)  # the same map without the weights does blend
    assert (leaky[~right] > 1.0).any() and (leaky[right] < 10.0).any()


def test_one_pass_leaves_the_variance_of_a_b3_spline():
    """White noise on a fully covered plane, no position and no normal weight: the pass is the separable kernel h h^T / 256, which leaves
    (sum h^2 / (sum h)^2)^2 = (70 / 256)^2 of the variance.  Over the inner 192^2 — some 5 000 effectively independent samples of the output — a
    variance ratio has a standard error of about 2 %; 10 % is five of them."""
    n = 256
    rng = np.random.default_rng(2024)
    yy, xx = np.mgrid[0:n, 0:n]
    p = np.stack([xx * 1.0, np.zeros((n, n)), yy * 1.0], -1)
    nm = np.tile([0.0, 1.0, 0.0], (n * n, 1))
    v = rng.standard_normal((n, n, 1)).astype(np.float32)
    out = nr.filter_texels_ref(np.ones(n * n, np.uint32), n, n, p, nm, v, 1, math.inf, -1.0)
    inner = (slice(32, 224), slice(32, 224))
    ratio = float(out[inner].astype(np.float64).var() / v[inner].astype(np.float64).var())
    want = (70.0 / 256.0) ** 2
    print("variance ratio of one pass: %.4f, derived %.4f" % (ratio, want))
    assert abs(ratio - want) <= 0.10 * want
    for step in (2, 4):
        out = nr.filter_texels_ref(np.ones(n * n, np.uint32), n, n, p, nm, out, step, math.inf, -1.0)
    assert out[inner].astype(np.float64).var() < 0.01 * v[inner].astype(np.float64).var()


def test_the_mirror_is_quick_on_a_large_map():
    import time
    n = 1024
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:n, 0:n]
    flags = (((xx % 20) < 16) & ((yy % 20) < 16)).astype(np.uint32) * 3
    p = np.stack([xx * 0.01, np.zeros((n, n)), yy * 0.01], -1)
    nm = np.tile([0.0, 1.0, 0.0], (n * n, 1))
    v = rng.random((n * n, 3), dtype=np.float32)
    t0 = time.perf_counter()
    out = nr.filter_texels_ref(flags, n, n, p, nm, v, 2, 0.1, 0.5)
    assert time.perf_counter() - t0 < 30.0 and np.array_equal(out[flags.reshape(-1) == 0], v[flags.reshape(-1) == 0])


# ---- the declarations, layer by layer ----------------------------------------------------------------------------------------------------------------------------
_ARGS = ["NraysScene*", "uint32_t", "uint32_t", "const uint32_t*", "const double*", "const double*", "uint32_t", "const float*", "float*", "uint32_t", "double", "double", "uint32_t"]
EXPECTED = {"nrays_filter_texels_device": _ARGS + ["void*"], "nrays_filter_texels": _ARGS}


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_the_header_declares_the_entry_points(name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, HEADER)
    assert m, name
    types = [re.sub(r"\s*\w+$", "", a.strip()).replace(" *", "*") for a in m.group(1).split(",")]
    assert types == EXPECTED[name]
    assert name in abi.HIP_SYMBOLS and name in abi.POST_V7_SYMBOLS
    res, args = abi.HIP_SYMBOLS[name]
    assert len(args) == len(EXPECTED[name])
    assert re.search(r"WITHOUT a bump[^;]*?\b%s\b" % name, HEADER, re.S)


def test_constants_and_version():
    assert re.search(r"#define\s+NRAYS_FILTER_MAX_STEP\s+64u\b", HEADER) and abi.FILTER_MAX_STEP == 64
    assert re.search(r"#define\s+NRAYS_ABI_VERSION\s+7\b", HEADER) and abi.ABI_VERSION == 7


def test_the_library_exports_them(built):
    import ctypes as C
    lib = abi.load_hip_lib()
    for name in EXPECTED:
        assert getattr(lib, name).argtypes == abi.HIP_SYMBOLS[name][1]
    f, p, nm = (C.c_uint32 * 1)(1), (C.c_double * 3)(), (C.c_double * 3)()
    v, out = (C.c_float * 1)(2.0), (C.c_float * 1)(7.0)
    assert lib.nrays_filter_texels(None, 1, 1, f, p, nm, 1, v, out, 1, 1.0, 0.0, 0) == abi.ERR_BAD_ARG and out[0] == 7.0  # the one status that needs no scene
    assert lib.nrays_filter_texels_device(None, 1, 1, None, None, None, 1, None, None, 1, 1.0, 0.0, 0, None) == abi.ERR_BAD_ARG


def test_the_rust_side_declares_and_calls_them():
    for name in EXPECTED:
        assert re.search(r"pub fn %s\(" % name, GPU_FFI), name
        assert name + "(" in GPU_RS, name
    assert "pub fn filter_texels(" in GPU_RS and "pub unsafe fn filter_texels_device(" in GPU_RS
    assert "NRAYS_FILTER_MAX_STEP" in GPU_FFI


# ---- the wrappers ---------------------------------------------------------------------------------------------------------------------------------------------------
class _NoDevice:
    def device_handle(self):
        raise AssertionError("device touched before the arguments were checked")


@pytest.fixture()
def no_library(monkeypatch):
    def refuse():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(abi, "load_hip_lib", refuse)


def _good_args():
    return dict(flags=np.ones(16, np.uint32), width=4, height=4, points=np.zeros((16, 3)), normals=np.tile([0.0, 1.0, 0.0], (16, 1)), values=np.zeros((16, 3), np.float32),
                step=1, pos_radius=1.0, normal_cos=0.0)


@pytest.mark.parametrize("kw", [dict(step=0), dict(step=65), dict(values=np.zeros((16, 5), np.float32)), dict(pos_radius=math.nan), dict(pos_radius=0.0), dict(pos_radius=-1.0),
                                dict(normal_cos=1.0), dict(normal_cos=math.nan), dict(normal_cos=-1.5), dict(flags=np.ones(15, np.uint32)), dict(points=np.zeros((15, 3))),
                                dict(normals=np.zeros((16, 2))), dict(values=np.zeros(17, np.float32)), dict(width=0), dict(width=16385, height=1)])
def test_the_wrappers_reject_bad_arguments_before_any_library_call(no_library, kw):
    args = _good_args()
    args.update(kw)
    with pytest.raises(ValueError):
        nr.filter_texels(_NoDevice(), **args)
    with pytest.raises(ValueError):
        nr.filter_texels_ref(**args)
    tx = nr.SurfaceTexels(points=args["points"], normals=args["normals"], uv=None, node=None, prim=None, flags=args["flags"])
    if "step" not in kw:
        with pytest.raises(ValueError):
            nr.denoise_texels(_NoDevice(), tx, args["values"], 3, args["pos_radius"], args["normal_cos"], args["width"], args["height"])


def test_denoise_texels_checks_its_own_arguments(no_library):
    a = _good_args()
    tx = nr.SurfaceTexels(points=a["points"], normals=a["normals"], uv=None, node=None, prim=None, flags=a["flags"])
    for bad in (dict(passes=0), dict(passes=8), dict()):  # the last: (n, c) values without width and height
        with pytest.raises(ValueError):
            nr.denoise_texels(_NoDevice(), tx, a["values"], **bad)
    with pytest.raises(ValueError):
        nr.denoise_texels(_NoDevice(), tx._replace(normals=None), a["values"].reshape(4, 4, 3))


def test_the_methods_exist_and_the_bakers_name_the_recipe():
    from nrays_amd import scenefile
    import inspect
    for cls in (nr.Scene, scenefile.FileScene):
        assert list(inspect.signature(cls.filter_texels).parameters)[1:] == list(inspect.signature(nr.filter_texels).parameters)[1:]
        assert list(inspect.signature(cls.denoise_texels).parameters)[1:] == list(inspect.signature(nr.denoise_texels).parameters)[1:]
        assert list(inspect.signature(cls.bake_indirect).parameters)[-1] == "unordered"
    sig = inspect.signature(nr.filter_texels).parameters
    assert (sig["step"].default, sig["pos_radius"].default, sig["normal_cos"].default, sig["device"].default) == (1, math.inf, 0.0, None)
    assert inspect.signature(nr.denoise_texels).parameters["passes"].default == 3
    for fn in (nr.bake_lightmap, nr.bake_indirect):
        assert "denoise_texels(scene, tx, rgb" in fn.__doc__ and "dilate >= 2" in fn.__doc__
