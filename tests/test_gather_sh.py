"""Gathered light as spherical harmonics (nrays_gather_sh_points_device / nrays_gather_sh_points; nrays_amd.gather_sh_points, gather_probes, sphere_dirs, sh_basis,
sh_fold_ref, sh_irradiance) without a GPU: the declarations in the header, the ctypes table and the Rust binding; the basis' constants and orthonormality; the
sphere table as a quadrature; irradiance from the coefficients against the direct cosine integral; the f32 fold against an f64 accumulation; argument checks."""
import ctypes as C
import math

import numpy as np
import pytest

import nrays_amd as nr
from nrays_amd import abi
from nrays_amd.scene import SH_K
from tests.test_gather import FFI, GPU_RS, HEADER, HEADER_TEXT, RUST_TYPES, _c_params

_IN = ["NraysScene*", "uint32_t", "const double*", "const double*", "const uint32_t*", "const uint64_t*", "const NraysGatherParams*", "uint32_t", "float*", "uint32_t"]
EXPECTED = {"nrays_gather_sh_points_device": _IN + ["void*"], "nrays_gather_sh_points": _IN,
            "nrays_debug_gather_sh_fold": _IN[:8] + ["const float*", "float*", "float*"]}
RUST = dict(RUST_TYPES, **{"const float*": "*const f32"})
CTYPES = {"NraysScene*": (C.c_void_p,), "uint32_t": (C.c_uint32,), "const double*": (C.c_void_p, C.POINTER(C.c_double)), "const uint32_t*": (C.c_void_p, C.POINTER(C.c_uint32)),
          "const uint64_t*": (C.c_void_p, C.POINTER(C.c_uint64)), "const NraysGatherParams*": (C.POINTER(abi.NraysGatherParams),), "float*": (C.c_void_p, C.POINTER(C.c_float)),
          "const float*": (C.POINTER(C.c_float),), "void*": (C.c_void_p,)}


# ---- the surface --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_header_ctypes_and_rust_declare_the_same_function(name):
    assert _c_params(name) == EXPECTED[name]
    assert name in abi.HIP_SYMBOLS and name in abi.POST_V7_SYMBOLS
    res, args = abi.HIP_SYMBOLS[name]
    assert res is C.c_int and len(args) == len(EXPECTED[name])
    for a, t in zip(args, EXPECTED[name]):
        assert a in CTYPES[t], (a, t)
    m = __import__("re").search(r"pub fn %s\((.*?)\) -> c_int;" % name, FFI)
    assert m, "%s is not declared in gpu_ffi.rs" % name
    assert [p.split(": ", 1)[1] for p in m.group(1).split(", ")] == [RUST[t] for t in EXPECTED[name]]
    assert name in HEADER_TEXT.split("#define NRAYS_ABI_VERSION")[0]  # the "added after 7" list
    assert "#define NRAYS_ABI_VERSION 7" in HEADER


def test_the_rust_wrapper_and_the_python_names_exist():
    for text in ("pub fn gather_sh_points(", "pub fn gather_sh_points_unordered(", "pub unsafe fn gather_sh_points_device(", "nrays_gather_sh_points(", "nrays_gather_sh_points_device("):
        assert text in GPU_RS, text
    for name in ("gather_sh_points", "gather_probes", "sphere_dirs", "sh_basis", "sh_fold_ref", "sh_irradiance", "gather_sh_fold"):
        assert callable(getattr(nr, name)), name
    assert callable(nr.Scene.gather_sh_points) and callable(nr.Scene.gather_probes)
    from nrays_amd import scenefile
    assert callable(scenefile.FileScene.gather_sh_points) and callable(scenefile.FileScene.gather_probes)


def test_the_header_spells_the_constants_the_mirror_uses():
    for k in SH_K:
        assert repr(k) in HEADER_TEXT, k


# ---- the basis ----------------------------------------------------------------------------------------------------------------------------------------------
def test_the_five_constants_equal_their_closed_forms_exactly():
    rp = math.sqrt(math.pi)
    closed = (1.0 / (2.0 * rp), math.sqrt(3.0) / (2.0 * rp), math.sqrt(15.0) / (2.0 * rp), math.sqrt(5.0) / (4.0 * rp), math.sqrt(15.0) / (4.0 * rp))
    assert SH_K == closed


def _basis64(d):
    """The nine expressions in float64, unrounded (scene._sh_terms is what sh_basis rounds)."""
    from nrays_amd.scene import _sh_terms
    return np.stack(_sh_terms(d[..., 0], d[..., 1], d[..., 2], 9), axis=-1)


def test_sh_basis_is_the_nine_expressions_rounded_once_and_a_prefix_per_band():
    rng = np.random.default_rng(3)
    d = rng.normal(size=(200, 3)) * 3.0  # used as given: not normalised
    y = nr.sh_basis(d, 3)
    assert y.dtype == np.float32 and y.shape == (200, 9)
    K0, K1, K2, K3, K4 = SH_K
    x, yy, z = d[:, 0], d[:, 1], d[:, 2]
    want = np.stack([np.full(200, K0), K1 * yy, K1 * z, K1 * x, (K2 * x) * yy, (K2 * yy) * z, K3 * ((3.0 * z) * z - 1.0), (K2 * x) * z, K4 * (x * x - yy * yy)], axis=1).astype(np.float32)
    assert np.array_equal(y.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(nr.sh_basis(d, 1).view(np.uint32), y[:, :1].view(np.uint32)) and np.array_equal(nr.sh_basis(d, 2).view(np.uint32), y[:, :4].view(np.uint32))
    assert nr.sh_basis(d.reshape(10, 20, 3), 2).shape == (10, 20, 4)
    for bad in (0, 4, 2.5, True):
        with pytest.raises(ValueError):
            nr.sh_basis(d, bad)
    with pytest.raises(ValueError):
        nr.sh_basis(d[:, :2], 3)


def test_orthonormal_under_an_exact_quadrature():
    """8-point Gauss-Legendre in z times 16 uniform azimuths: exact for products of two of these polynomials (degree <= 4 in z, frequency <= 4 in phi)."""
    zs, ws = np.polynomial.legendre.leggauss(8)
    phi = (np.arange(16) + 0.5) * (2.0 * math.pi / 16)
    z, p = np.meshgrid(zs, phi, indexing="ij")
    r = np.sqrt(1.0 - z * z)
    d = np.stack([r * np.cos(p), r * np.sin(p), z], axis=-1).reshape(-1, 3)
    w = (np.broadcast_to(ws[:, None], z.shape) * (2.0 * math.pi / 16)).reshape(-1)
    Y = _basis64(d)
    dev = float(np.abs((Y * w[:, None]).T @ Y - np.eye(9)).max())
    print("orthonormality deviation %.3g" % dev)
    assert dev <= 1e-12


def test_sphere_dirs_is_a_quadrature_for_the_basis():
    d = nr.sphere_dirs(1024)
    assert d.shape == (1024, 3) and d.dtype == np.float64
    t = np.arange(1024) + 0.5
    z = 1.0 - 2.0 * t / 1024
    phi = t * (math.pi * (3.0 - math.sqrt(5.0)))
    assert np.array_equal(d, np.stack([np.sqrt(1.0 - z * z) * np.cos(phi), np.sqrt(1.0 - z * z) * np.sin(phi), z], axis=1))
    norm_dev = float(np.abs(np.sqrt((d * d).sum(axis=1)) - 1.0).max())
    Y = _basis64(d)
    dev = float(np.abs((4.0 * math.pi / 1024) * Y.T @ Y - np.eye(9)).max())
    print("sphere_dirs(1024): | |d| - 1 | <= %.3g, max |(4 pi / k) Y^T Y - I| = %.3g" % (norm_dev, dev))
    assert norm_dev <= 4e-16
    assert dev <= 1e-3
    for bad in (0, 1025):
        with pytest.raises(ValueError):
            nr.sphere_dirs(bad)
    assert nr.sphere_dirs(1).shape == (1, 3)


# ---- irradiance ---------------------------------------------------------------------------------------------------------------------------------------------
def test_irradiance_of_a_band_limited_radiance_against_the_direct_sum():
    """Radiance L(d) = sum_c a_c Y_c(d) per channel with random a (the constant term lifted so that the values are of size 2), projected with sh_fold_ref over
    sphere_dirs(1024); E(n) from the coefficients against (4 pi / k) sum_j max(0, n . d_j) L(d_j) at 50 normals."""
    rng = np.random.default_rng(11)
    k = 1024
    d = nr.sphere_dirs(k)
    a = rng.uniform(-0.3, 0.3, size=(9, 3))
    a[0] = rng.uniform(1.5, 2.5, size=3)
    L = _basis64(d) @ a  # (k, 3)
    sh = nr.sh_fold_ref(d[None], L[None].astype(np.float32), 3)
    assert sh.shape == (1, 9, 3) and sh.dtype == np.float32
    nm = rng.normal(size=(50, 3))
    nm /= np.sqrt((nm * nm).sum(axis=1))[:, None]
    got = nr.sh_irradiance(sh[0].astype(np.float64), nm)
    direct = (4.0 * math.pi / k) * (np.maximum(0.0, nm @ d.T) @ L)
    err = float(np.abs(got - direct).max())
    print("irradiance: max |sh - direct| = %.3g on values of size %.3g" % (err, float(np.abs(direct).mean())))
    assert got.shape == (50, 3)
    assert 1.0 < float(np.abs(direct).mean()) < 10.0
    assert err <= 2e-3
    # one coefficient set per normal, and torch tensors, give the same numbers
    assert np.array_equal(nr.sh_irradiance(np.broadcast_to(sh[0].astype(np.float64), (50, 9, 3)), nm), got)
    import torch
    tt = nr.sh_irradiance(torch.from_numpy(sh[0].astype(np.float64)), torch.from_numpy(nm))
    assert np.allclose(tt.numpy(), got, rtol=0, atol=1e-12)
    # a constant radiance: E = pi L whatever the normal
    const = np.zeros((1, 3)) + SH_K[0] * np.asarray([0.2, 0.5, 0.9])
    assert np.allclose(nr.sh_irradiance(const, nm[:4]), math.pi * np.asarray([0.2, 0.5, 0.9]), rtol=1e-14, atol=0)
    assert np.allclose(nr.sh_irradiance(const, nm[:4], measure=2.0 * math.pi), 0.5 * math.pi * np.asarray([0.2, 0.5, 0.9]), rtol=1e-14, atol=0)
    with pytest.raises(ValueError):
        nr.sh_irradiance(np.zeros((5, 3)), nm)
    with pytest.raises(ValueError):
        nr.sh_irradiance(sh[0], torch.from_numpy(nm))


# ---- the fold -----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 7, 64, 1024])
def test_fold_ref_against_an_f64_accumulation(k):
    """With u = 2^-24 and S = sum_j |y_j c_j| (y already f32, so each exact product is an f64): every product is rounded once (u S in all), the sequential sum of
    k terms is within (k - 1) u S of the sum of the rounded products (Higham, eq. 4.4, first order) and the division rounds once more: (k + 1) u S / k on the mean,
    taken as (k + 2) for the second-order terms and never above the 2 k u S / k = 2^-23 S per step pair that k = 1 allows."""
    rng = np.random.default_rng(k)
    d = rng.normal(size=(5, k, 3))
    col = rng.uniform(0.0, 4.0, size=(5, k, 3)).astype(np.float32)
    got = nr.sh_fold_ref(d, col, 3)
    y = nr.sh_basis(d, 3).astype(np.float64)
    terms = y[:, :, :, None] * col.astype(np.float64)[:, :, None, :]
    exact = terms.sum(axis=1) / k
    bound = min(k + 2, 2 * k) * 2.0 ** -24 * np.abs(terms).sum(axis=1) / k
    assert got.shape == (5, 9, 3) and got.dtype == np.float32
    assert (np.abs(got.astype(np.float64) - exact) <= bound).all()
    assert np.array_equal(nr.sh_fold_ref(d, col, 2).view(np.uint32), got[:, :4].view(np.uint32))
    assert np.array_equal(nr.sh_fold_ref(d, col, 1).view(np.uint32), got[:, :1].view(np.uint32))


def test_fold_ref_rounds_the_product_before_the_sum():
    """y * c is rounded to f32 before it is added: with y = K0 and colours chosen so that the exact product is not an f32, a fused or f64 accumulation differs."""
    d = np.zeros((1, 2, 3))
    d[..., 2] = 1.0
    col = np.asarray([[[1.0, 3.0, 1e8], [1e-8, 7.0, -1e8]]], np.float32)
    got = nr.sh_fold_ref(d, col, 1)[0, 0]
    y = np.float32(SH_K[0])
    want = ((np.float32(0) + y * col[0, 0]) + y * col[0, 1]) / np.float32(2)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    with pytest.raises(ValueError):
        nr.sh_fold_ref(d, col.astype(np.float64), 1)
    with pytest.raises(ValueError):
        nr.sh_fold_ref(d[:, :1], col, 1)


# ---- argument checks before any library call ----------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    def boom():
        raise AssertionError("the library must not be loaded for a rejected call")
    monkeypatch.setattr(abi, "load_hip_lib", boom)


def test_bad_arguments_are_rejected_before_any_library_call(no_library):
    p, nm, L = np.zeros((4, 3)), np.tile([0.0, 0.0, 1.0], (4, 1)), nr.sphere_dirs(8)
    for kw in (dict(bands=0), dict(bands=4), dict(bands=1.5), dict(unordered=1), dict(energy=math.inf), dict(bias=math.nan), dict(keys=np.zeros(3, np.uint64)),
               dict(hit_flags=np.zeros(5, np.uint32))):
        with pytest.raises(ValueError):
            nr.gather_sh_points(None, p, nm, L, **kw)
    with pytest.raises(ValueError):
        nr.gather_sh_points(None, p, nm[:3], L)
    with pytest.raises(ValueError):
        nr.gather_sh_points(None, p, nm, np.zeros((1025, 3)))
    with pytest.raises(ValueError):
        nr.gather_probes(None, np.zeros((4, 2)), L)
    with pytest.raises(ValueError):
        nr.gather_probes(None, p, L, bands=7)
    with pytest.raises(ValueError):
        nr.gather_sh_fold(None, p, nm, L, np.zeros((4, 7, 3), np.float32))
