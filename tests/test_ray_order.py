"""Reordering of caller-ray batches that come in no useful order (NRAYS_RAYS_UNORDERED: nrays_trace_rays_device_ex, nrays_trace_rays_ex,
nrays_intersects_rays_device_ex, nrays_debug_ray_order): the parts that need no GPU — the ABI surface, argument checks, and the key of
nrays_amd/csrc/ray_key.h compiled by the host compiler (tests/ray_key_shim.cpp): totality, the frame of a batch, and whether an order by
the key's leading bits is FINE enough.

The yardstick of "fine enough" is derived, not measured: 64 consecutive elements of a 1920-wide row-major grid cover exactly eight 8 x 8
tiles, so row-major order scores 8.0 tiles per wave by construction."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import nrays_amd as nr
from nrays_amd import abi, math3d
from tools import scenes_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("nrays_trace_rays_device_ex", "nrays_trace_rays_ex", "nrays_intersects_rays_device_ex", "nrays_debug_ray_order")
GRID_W, GRID_H = 1920, 1080
NO_BOX = np.asarray([-np.inf] * 3 + [np.inf] * 3)


# ---- the host build of ray_key.h ------------------------------------------------------------------------------------------------------

class KeyShim:
    def __init__(self, directory):
        out = os.path.join(str(directory), "libray_key_shim.so")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(ROOT, "nrays_amd", "csrc"), "-o", out,
                               os.path.join(ROOT, "tests", "ray_key_shim.cpp")])
        lib = C.CDLL(out)
        dp = C.POINTER(C.c_double)
        lib.ray_key_constants.argtypes = [C.POINTER(C.c_int32)]
        lib.ray_key_frame.argtypes = [C.c_uint32, dp, dp, dp, C.c_uint32, dp]
        lib.ray_key_keys.argtypes = [C.c_uint32, dp, dp, dp, C.POINTER(C.c_uint64)]
        lib.ray_key_octant.argtypes = [dp, C.c_uint64]
        lib.ray_key_octant.restype = C.c_uint32
        self.lib = lib
        c = (C.c_int32 * 3)()
        lib.ray_key_constants(c)
        self.K, self.B, self.frame_doubles = int(c[0]), int(c[1]), int(c[2])

    @staticmethod
    def _dp(a):
        return a.ctypes.data_as(C.POINTER(C.c_double))

    def frame(self, origins, dirs, box=NO_BOX, parts=1):
        o, d = np.ascontiguousarray(origins, np.float64), np.ascontiguousarray(dirs, np.float64)
        b = np.ascontiguousarray(box, np.float64)
        f = np.zeros(self.frame_doubles)
        self.lib.ray_key_frame(len(o), self._dp(o), self._dp(d), self._dp(b), parts, self._dp(f))
        return f

    def keys(self, origins, dirs, frame):
        o, d = np.ascontiguousarray(origins, np.float64), np.ascontiguousarray(dirs, np.float64)
        f = np.ascontiguousarray(frame, np.float64)
        k = np.zeros(len(o), np.uint64)
        self.lib.ray_key_keys(len(o), self._dp(o), self._dp(d), self._dp(f), k.ctypes.data_as(C.POINTER(C.c_uint64)))
        return k

    def octant(self, frame, key):
        f = np.ascontiguousarray(frame, np.float64)
        return int(self.lib.ray_key_octant(self._dp(f), int(key)))


@pytest.fixture(scope="module")
def keyshim(tmp_path_factory):
    return KeyShim(tmp_path_factory.mktemp("ray_key_shim"))


# ---- the two batches of the "fine enough" conditions and their score ------------------------------------------------------------------

def camera_batch():
    """(a) the 1920 x 1080 rays of balls_scene()'s camera, in image order."""
    _, cam = su.balls_scene(tex_size=(8, 4))
    proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], GRID_W, GRID_H)
    o, d, _ = nr.camera_rays((GRID_W, GRID_H), cam["eye"], proj)
    return o, d


def ao_batch(seed=1):
    """(b) origins on a 1920 x 1080 grid over a rectangle of the plane y = 0, directions cosine-distributed about +y."""
    rng = np.random.default_rng(seed)
    n = GRID_W * GRID_H
    gx, gz = np.meshgrid(np.arange(GRID_W), np.arange(GRID_H))
    o = np.stack([-8.0 + 16.0 * (gx.ravel() + 0.5) / GRID_W, np.zeros(n), -4.5 + 9.0 * (gz.ravel() + 0.5) / GRID_H], axis=1)
    r, phi = np.sqrt(rng.uniform(0.0, 1.0, n)), rng.uniform(0.0, 2.0 * np.pi, n)
    d = np.stack([r * np.cos(phi), np.sqrt(np.maximum(0.0, 1.0 - r * r)), r * np.sin(phi)], axis=1)
    return o, d


def tiles_per_wave(order):
    """Mean number of distinct 8 x 8 tiles of the 1920 x 1080 grid that 64 consecutive rays of `order` (grid indices) touch."""
    idx = np.asarray(order, dtype=np.int64)
    tile = (idx // GRID_W // 8) * (GRID_W // 8) + (idx % GRID_W) // 8
    n = len(tile) // 64 * 64
    t = np.sort(tile[:n].reshape(-1, 64), axis=1)
    return float((1 + (np.diff(t, axis=1) != 0).sum(axis=1)).mean())


def bin_orders(bins, rng):
    """Two orders by bin with different orders inside a bin: by index, and random."""
    by_index = np.argsort(bins, kind="stable")
    tie = rng.permutation(len(bins))
    return by_index, np.lexsort((tie, bins))


def test_row_major_scores_eight():
    assert tiles_per_wave(np.arange(GRID_W * GRID_H)) == 8.0


@pytest.mark.parametrize("batch,bound", [("camera", 8.0), ("ao", 16.0)])
def test_the_ordering_is_fine_enough(keyshim, batch, bound):
    o, d = camera_batch() if batch == "camera" else ao_batch()
    rng = np.random.default_rng(17)
    perm = rng.permutation(len(o))  # the shuffled batch: ray j of it is grid point perm[j]
    assert tiles_per_wave(perm) > 60.0
    so, sd = o[perm], d[perm]
    frame = keyshim.frame(so, sd)
    bins = keyshim.keys(so, sd, frame) >> np.uint64(keyshim.K - keyshim.B)
    for order in bin_orders(bins, rng):
        score = tiles_per_wave(perm[order])
        print("%s batch, shuffled and ordered by the leading %d key bits: %.2f tiles per wave (bound %.1f)" % (batch, keyshim.B, score, bound))
        assert score <= bound


def test_a_key_that_ignores_origins_would_fail(keyshim):
    """The bound of (b) separates: the same batch binned by its direction bits alone (every origin moved to one point) is as bad as shuffled."""
    o, d = ao_batch()
    frame = keyshim.frame(np.zeros_like(o), d)
    bins = keyshim.keys(np.zeros_like(o), d, frame) >> np.uint64(keyshim.K - keyshim.B)
    assert tiles_per_wave(np.argsort(bins, kind="stable")) > 16.0


# ---- the key ----------------------------------------------------------------------------------------------------------------------------

SPECIAL = [np.nan, np.inf, -np.inf, 0.0, -0.0, 1e308, -1e308, 5e-324, 1.0, -1.0]


def _special_rays():
    rng = np.random.default_rng(3)
    o = rng.choice(SPECIAL, size=(4000, 3))
    d = rng.choice(SPECIAL, size=(4000, 3))
    d[:10] = 0.0  # zero directions
    o[10:20] = 1e300  # far outside
    return o, d


def test_keys_are_total(keyshim):
    assert 0 < keyshim.B <= keyshim.K <= 64
    o, d = _special_rays()
    rng = np.random.default_rng(4)
    fo, fd = rng.uniform(-3, 3, (1000, 3)), rng.normal(size=(1000, 3))
    frames = [keyshim.frame(fo, fd), keyshim.frame(o, d), keyshim.frame(fo[:1], fd[:1]), keyshim.frame(fo[:0], fd[:0]),
              keyshim.frame(np.tile(fo[:1], (8, 1)), np.tile(fd[:1], (8, 1))),  # a frame of no extent
              keyshim.frame(fo, fd, box=[0, 0, 0, 0, 0, 0]), keyshim.frame(fo, fd, box=[1, 1, 1, -1, -1, -1]),
              keyshim.frame(np.asarray([[-1e308] * 3, [1e308] * 3]), fd[:2])]  # an extent that overflows
    for f in frames:
        assert np.all(np.isfinite(f[:14]))  # (f[14:] is the box as given)
        for oo, dd in ((o, d), (fo, fd)):
            k = keyshim.keys(oo, dd, f)
            assert int(k.max()) < 1 << keyshim.K
            assert np.array_equal(k, keyshim.keys(oo, dd, f))  # same inputs, same key
    # a frame the library never wrote still gives keys in range
    k = keyshim.keys(o, d, np.full(keyshim.frame_doubles, np.nan))
    assert int(k.max()) < 1 << keyshim.K


def test_non_finite_rays_do_not_poison_the_frame(keyshim):
    rng = np.random.default_rng(5)
    fo, fd = rng.uniform(-3, 3, (500, 3)), rng.normal(size=(500, 3))
    so, sd = _special_rays()
    with np.errstate(over="ignore"):
        l1 = np.abs(sd).sum(axis=1)
    dir_ok = np.isfinite(sd).all(axis=1) & np.isfinite(l1) & (l1 > 0)
    both = ~np.isfinite(so).all(axis=1) & ~dir_ok  # rays whose origin AND direction are unusable, mixed into the finite ones
    assert both.sum() > 100
    mo, md = np.concatenate([fo, so[both]]), np.concatenate([fd, sd[both]])
    perm = rng.permutation(len(mo))
    want = keyshim.frame(fo, fd)
    assert np.array_equal(keyshim.frame(mo[perm], md[perm]), want)
    assert np.array_equal(keyshim.frame(mo[perm], md[perm], parts=7), want)  # merged from partial bounds, in another order


def test_the_frame_is_clamped_to_the_scene_box(keyshim):
    rng = np.random.default_rng(6)
    fo, fd = rng.uniform(-3, 3, (500, 3)), rng.normal(size=(500, 3))
    fo[0] = (1e12, -1e12, 0.0)  # e.g. a ray that left for a plane far away
    f = keyshim.frame(fo, fd, box=[-2, -2, -2, 2, 2, 2])
    assert np.all(f[0:3] >= -2.0) and np.all(f[3:6] <= 2.0)


def test_a_direction_sign_changes_the_octant_field(keyshim):
    rng = np.random.default_rng(7)
    fo, fd = rng.uniform(-3, 3, (256, 3)), rng.normal(size=(256, 3))
    f = keyshim.frame(fo, fd)
    k0 = keyshim.keys(fo, fd, f)
    for axis in range(3):
        flipped = fd.copy()
        flipped[:, axis] = -flipped[:, axis]
        k1 = keyshim.keys(fo, flipped, f)
        for a, b in zip(k0[:64], k1[:64]):
            assert keyshim.octant(f, a) ^ keyshim.octant(f, b) == 1 << axis


# ---- ABI surface and argument checks ----------------------------------------------------------------------------------------------------

def test_new_symbols_are_exported_with_signatures(built):
    exported = subprocess.check_output(["nm", "-D", "--defined-only", abi.HIP_LIB_PATH]).decode()
    lib = abi.load_hip_lib()
    for name in NEW_SYMBOLS:
        assert (" T " + name) in exported, name
        res, args = abi.HIP_SYMBOLS[name]
        assert res is C.c_int
        assert getattr(lib, name).argtypes == args
    assert len(abi.HIP_SYMBOLS["nrays_trace_rays_device_ex"][1]) == 11
    assert len(abi.HIP_SYMBOLS["nrays_trace_rays_ex"][1]) == 10
    assert len(abi.HIP_SYMBOLS["nrays_intersects_rays_device_ex"][1]) == 9
    assert len(abi.HIP_SYMBOLS["nrays_debug_ray_order"][1]) == 8
    header = open(os.path.join(ROOT, "include", "nrays_abi.h")).read()
    assert "#define NRAYS_RAYS_UNORDERED 1u" in header and abi.RAYS_UNORDERED == 1
    assert "#define NRAYS_RAY_FRAME_DOUBLES %d" % abi.RAY_FRAME_DOUBLES in header
    assert abi.ABI_VERSION == 7 and lib.nrays_abi_version() == 7


def test_the_header_and_the_key_agree_on_the_frame_length(keyshim):
    assert keyshim.frame_doubles == abi.RAY_FRAME_DOUBLES


def test_null_arguments_and_unknown_flags_are_bad_args(built):
    lib = abi.load_hip_lib()
    o = (C.c_double * 3)(0.0, 0.0, 1.0)
    out = (C.c_float * 3)()
    lit = (C.c_uint32 * 1)()
    keys = (C.c_uint64 * 1)()
    order = (C.c_uint32 * 1)()
    frame = (C.c_double * abi.RAY_FRAME_DOUBLES)()
    info = (C.c_uint32 * 4)()
    fake = C.c_void_p(8)  # a non-NULL scene: the flag check comes before anything looks at it
    for n in (0, 1):
        for flags in (0, abi.RAYS_UNORDERED):
            assert lib.nrays_trace_rays_ex(None, n, o, o, None, None, None, 0, out, flags) == abi.ERR_BAD_ARG
            assert lib.nrays_trace_rays_device_ex(None, n, C.addressof(o), C.addressof(o), None, None, None, 0, C.addressof(out), flags, None) == abi.ERR_BAD_ARG
            assert lib.nrays_intersects_rays_device_ex(None, n, C.addressof(o), C.addressof(o), C.addressof(o), C.addressof(out), C.addressof(lit), flags, None) == abi.ERR_BAD_ARG
        for flags in (2, 3, 1 << 31):
            assert lib.nrays_trace_rays_ex(fake, n, o, o, None, None, None, 0, out, flags) == abi.ERR_BAD_ARG
            assert lib.nrays_trace_rays_device_ex(fake, n, C.addressof(o), C.addressof(o), None, None, None, 0, C.addressof(out), flags, None) == abi.ERR_BAD_ARG
            assert lib.nrays_intersects_rays_device_ex(fake, n, C.addressof(o), C.addressof(o), C.addressof(o), C.addressof(out), C.addressof(lit), flags, None) == abi.ERR_BAD_ARG
        assert lib.nrays_debug_ray_order(None, n, o, o, keys, order, frame, info) == abi.ERR_BAD_ARG
        assert lib.nrays_debug_ray_order(fake, n, None, o, keys, order, frame, info) == abi.ERR_BAD_ARG
        assert lib.nrays_debug_ray_order(fake, n, o, o, keys, order, frame, None) == abi.ERR_BAD_ARG
    assert lib.nrays_debug_ray_order(fake, (1 << 22) + 1, o, o, keys, order, frame, info) == abi.ERR_BAD_ARG  # more than a chunk
    assert lib.nrays_last_error()


class _NoDevice:
    """A scene whose device handle must never be asked for: argument errors are raised first."""
    def device_handle(self):
        raise AssertionError("device touched before the arguments were checked")


@pytest.mark.parametrize("kw", [
    dict(origins=np.zeros((4, 2)), dirs=np.zeros((4, 3))),
    dict(origins=np.zeros((4, 3)), dirs=np.zeros((5, 3))),
    dict(origins=np.zeros((4, 3), np.int64), dirs=np.zeros((4, 3))),
    dict(origins=np.zeros((4, 3)), dirs=np.zeros((4, 3)), refr=np.ones(3)),
    dict(origins=np.zeros((4, 3)), dirs=np.zeros((4, 3)), keys=np.zeros(4, np.float64)),
    dict(origins=np.zeros((4, 3)), dirs=np.zeros((4, 3)), max_depth=-1),
])
def test_hinted_trace_rays_checks_arguments_before_the_device(built, kw):
    with pytest.raises(ValueError):
        nr.trace_rays(_NoDevice(), unordered=True, **kw)


@pytest.mark.parametrize("kw", [
    dict(origins=np.zeros((4, 3)), dirs=np.zeros((4, 3)), max_toi=np.ones(5)),
    dict(origins=np.zeros((4, 3)), dirs=np.zeros((3, 3)), max_toi=np.ones(4)),
    dict(origins=np.zeros((4, 3)), dirs=np.zeros((4, 3)), max_toi=np.ones(4, np.int32)),
])
def test_hinted_intersects_rays_checks_arguments_before_the_device(built, kw):
    with pytest.raises(ValueError):
        nr.intersects_rays(_NoDevice(), unordered=True, **kw)


@pytest.mark.parametrize("kw", [
    dict(origins=np.zeros((4, 2)), dirs=np.zeros((4, 3))),
    dict(origins=np.zeros((4, 3)), dirs=np.zeros((5, 3))),
    dict(origins=np.zeros((4, 3), np.int64), dirs=np.zeros((4, 3))),
    dict(origins=np.zeros(((1 << 22) + 1, 3)), dirs=np.zeros(((1 << 22) + 1, 3))),
])
def test_ray_order_checks_arguments_before_the_device(built, kw):
    with pytest.raises(ValueError):
        nr.ray_order(_NoDevice(), **kw)
