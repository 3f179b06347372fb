"""Denoising of a baked light map on the GPU (nrays_filter_texels_device / nrays_filter_texels; texel_filter_kernel.h): the device against the numpy mirror of
the definition (nrays_amd.filter_texels_ref) by bit pattern — two NaNs count as equal whatever their payload — over lattices on both sides of the kernel's
tile seams at every step, every channel count, the 128-bit path and the word path, NaN values and non-finite points, the statuses, the host entry, a stream
shared with the baker's other calls, denoise_texels against three mirror passes on a real two-chart map, and the handle's render state."""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest

import nrays_amd as nr
from nrays_amd import abi, math3d
from tests.test_filter_texels import bits, surface
from tools import scenes_util as su

pytestmark = pytest.mark.gpu
STAT_FIELDS = ("rays_primary", "rays_reflection", "rays_refraction", "rays_shadow", "rays_shadow_elided", "rays_primary_traced", "generations")
# the block of one residue class that a workgroup owns: kFilterTileX x kFilterTileY of nrays_amd/csrc/texel_filter_kernel.h, read from there
_KERNEL_H = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nrays_amd", "csrc", "texel_filter_kernel.h")).read()
TILE_X, TILE_Y = (int(re.search(r"constexpr uint32_t kFilterTile%s = (\d+)u;" % a, _KERNEL_H).group(1)) for a in "XY")
SMALL = [(1, 1), (5, 3), (17, 19), (33, 16)]
STEPS = [1, 2, 3, 5, 64]


def lattices(step):
    """The small shapes, and the tile's extent in the lattice (TILE * step points) minus one, exactly, and plus one, in both axes; at step 64 that extent is
    2048 x 512, and the seams between workgroups are those between the residue classes and the sub-lattices of three to five points instead."""
    if step == 64:
        return SMALL + [(130, 67), (257, 129)]
    ex, ey = TILE_X * step, TILE_Y * step
    return SMALL + [(ex - 1, ey + 1), (ex, ey), (ex + 1, ey - 1), (2 * ex + 1, 2 * ey + 1)]


@functools.lru_cache(maxsize=None)
def any_scene():
    """The call needs a handle for its device and stream ordering; the scene's content plays no part."""
    from tests.test_surface_texels import quad
    p, idx, uv = quad()
    return nr.Scene([nr.SceneNode(nr.PhongMaterial((0.2, 0.2, 0.2), (0.5, 0.5, 0.5), (0.0, 0.0, 0.0)), 0.0, 0.0, 1.0, 1.0, nr.Isometry3(), nr.TriMesh(p, idx, uv))],
                    [nr.Light((1.0, 6.0, -2.0), 0.0, 1, (0.9, 0.9, 0.8))], (0.1, 0.2, 0.3))


def same(got, want, what=None):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, what
    ok = (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))
    assert ok.all(), (what, int((~ok).sum()), np.argwhere(~ok)[:5].tolist())


def device_call(flags, w, h, p, nm, v, step, pos_radius, normal_cos, scene=None):
    import torch
    f = torch.from_numpy(flags.view(np.int32)).cuda()
    tp, tn, tv = torch.from_numpy(p).cuda(), torch.from_numpy(nm).cuda(), torch.from_numpy(v).cuda()
    out = nr.filter_texels(scene or any_scene(), f, w, h, tp, tn, tv, step, pos_radius, normal_cos)
    torch.cuda.synchronize()
    assert out.data_ptr() != tv.data_ptr() and out.shape == tv.shape and out.dtype == torch.float32
    assert np.array_equal(bits(tv.cpu().numpy()), bits(v))  # the input is left alone
    return out.cpu().numpy()


WEIGHTS = ((0.35, 0.3), (math.inf, -1.0), (0.2, -0.5), (1e3, 0.9))  # (pos_radius per step, normal_cos): both weights at work, neither, tight, normals only


@pytest.mark.parametrize("step", STEPS)
def test_the_device_equals_the_mirror(gpu, step):
    for k, (w, h) in enumerate(lattices(step)):
        rng = np.random.default_rng(1000 * step + k)
        channels, coverage = (1, 3, 4)[k % 3], (0.8, 1.0, 0.6, 0.0)[(k // 3 + k) % 4] if k else 1.0
        flags, p, nm, v = surface(rng, w, h, coverage, channels, special_share=0.02 if k % 2 else 0.0)
        pos_radius, normal_cos = WEIGHTS[k % 4]
        pos_radius *= step
        want = nr.filter_texels_ref(flags, w, h, p, nm, v, step, pos_radius, normal_cos)
        got = device_call(flags, w, h, p, nm, v, step, pos_radius, normal_cos)
        same(got, want, (w, h, channels, coverage))
        unc = (flags & 1) == 0
        assert np.array_equal(bits(got)[unc], bits(v)[unc])  # uncovered texels: the words, NaN payloads and -0 included


@pytest.mark.parametrize("channels", [1, 2, 3, 4])
def test_every_channel_count_at_a_tile_seam(gpu, channels):
    w, h, step = 2 * TILE_X + 1, 2 * TILE_Y + 1, 2
    flags, p, nm, v = surface(np.random.default_rng(40 + channels), w, h, 0.7, channels, special_share=0.02)
    same(device_call(flags, w, h, p, nm, v, step, 0.6, 0.1), nr.filter_texels_ref(flags, w, h, p, nm, v, step, 0.6, 0.1))


def test_four_channels_take_the_same_values_aligned_or_not(gpu):
    """Four channels with both value arrays at 16-byte aligned addresses are loaded and stored as one 128-bit word, at any other address word by word."""
    import torch
    w, h, step = TILE_X + 5, TILE_Y + 3, 1
    flags, p, nm, v = surface(np.random.default_rng(5), w, h, 0.7, 4, special_share=0.02)
    want = nr.filter_texels_ref(flags, w, h, p, nm, v, step, 0.5, 0.2)
    f, tp, tn = torch.from_numpy(flags.view(np.int32)).cuda(), torch.from_numpy(p).cuda(), torch.from_numpy(nm).cuda()
    lib, handle, n = abi.load_hip_lib(), any_scene().device_handle(), w * h
    for shift_in, shift_out in ((0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (3, 1)):
        src, dst = torch.zeros(n * 4 + 4, dtype=torch.float32, device="cuda"), torch.full((n * 4 + 4,), 7.0, dtype=torch.float32, device="cuda")
        vin, vout = src[shift_in:shift_in + n * 4], dst[shift_out:shift_out + n * 4]
        vin.copy_(torch.from_numpy(v).cuda().reshape(-1))
        assert vin.data_ptr() % 16 == 4 * shift_in and vout.data_ptr() % 16 == 4 * shift_out
        assert lib.nrays_filter_texels_device(handle, w, h, f.data_ptr(), tp.data_ptr(), tn.data_ptr(), 4, vin.data_ptr(), vout.data_ptr(), step, 0.5, 0.2, 0, None) == abi.OK
        torch.cuda.synchronize()
        same(vout.cpu().numpy().reshape(n, 4), want, (shift_in, shift_out))
        assert bool((dst[:shift_out] == 7.0).all()) and bool((dst[shift_out + n * 4:] == 7.0).all())  # nothing written beside the array


def _plane(w, h, channels, seed):
    yy, xx = np.mgrid[0:h, 0:w]
    p = np.stack([xx * 0.1, np.zeros((h, w)), yy * 0.1], -1).reshape(-1, 3)
    nm = np.tile([0.0, 1.0, 0.0], (w * h, 1))
    v = np.random.default_rng(seed).random((w * h, channels), dtype=np.float32)
    return np.ones(w * h, np.uint32), p, nm, v


@pytest.mark.parametrize("step", [1, 3])
def test_a_nan_value_reaches_exactly_its_25_taps(gpu, step):
    w, h = 41, 23
    flags, p, nm, v = _plane(w, h, 3, 1)
    x0, y0 = 20, 11
    v[y0 * w + x0, 1] = np.nan
    want = nr.filter_texels_ref(flags, w, h, p, nm, v, step, math.inf, -1.0)
    got = device_call(flags, w, h, p, nm, v, step, math.inf, -1.0)
    same(got, want)
    yy, xx = np.mgrid[0:h, 0:w]
    reach = (np.abs(xx - x0) % step == 0) & (np.abs(xx - x0) <= 2 * step) & (np.abs(yy - y0) % step == 0) & (np.abs(yy - y0) <= 2 * step)
    assert reach.sum() == 25 - (10 if y0 + 2 * step >= h or y0 - 2 * step < 0 else 0)
    assert np.array_equal(np.isnan(got[:, 1]).reshape(h, w), reach) and np.array_equal(np.isnan(want[:, 1]).reshape(h, w), reach)
    assert not np.isnan(got[:, [0, 2]]).any()


@pytest.mark.parametrize("bad", [math.nan, math.inf, -math.inf])
def test_a_non_finite_point_at_a_centre_leaves_the_centre_tap(gpu, bad):
    w, h = 37, 11
    flags, p, nm, v = _plane(w, h, 4, 2)
    c = 5 * w + 18
    p[c, 0] = bad
    want = nr.filter_texels_ref(flags, w, h, p, nm, v, 1, 0.5, 0.0)
    got = device_call(flags, w, h, p, nm, v, 1, 0.5, 0.0)
    same(got, want)
    assert np.array_equal(bits(got[c]), bits((np.float32(0.0) + np.float32(36.0) * v[c]) / np.float32(36.0)))
    assert np.isfinite(got).all()


# ---- the entry points ---------------------------------------------------------------------------------------------------------------------------------------------
def test_the_host_entry_equals_the_device_entry(gpu):
    w, h, step = 2 * TILE_X + 3, TILE_Y + 2, 2
    for channels in (1, 3, 4):
        flags, p, nm, v = surface(np.random.default_rng(60 + channels), w, h, 0.7, channels, special_share=0.02)
        want = nr.filter_texels_ref(flags, w, h, p, nm, v, step, 0.7, 0.1)
        kept = v.copy()
        host = nr.filter_texels(any_scene(), flags, w, h, p, nm, v, step, 0.7, 0.1)
        assert isinstance(host, np.ndarray) and host is not v and np.array_equal(bits(v), bits(kept))
        same(host, want, "host")
        same(host, device_call(flags, w, h, p, nm, v, step, 0.7, 0.1), "host against device")
        grid = any_scene().filter_texels(flags.reshape(h, w), w, h, p.reshape(h, w, 3), nm.reshape(h, w, 3), v.reshape(h, w, channels), step, 0.7, 0.1)
        assert grid.shape == (h, w, channels)
        same(grid.reshape(-1, channels), want, "method, lattice-shaped arrays")
        moved = nr.filter_texels(any_scene(), flags, w, h, p, nm, v, step, 0.7, 0.1, device="cuda")  # numpy in, moved to the device
        same(moved.cpu().numpy(), want, "device=")


def test_statuses(gpu):
    import torch
    lib, handle = abi.load_hip_lib(), any_scene().device_handle()
    n = 16
    f, tp, tn = torch.ones(n, dtype=torch.int32, device="cuda"), torch.zeros((n, 3), dtype=torch.float64, device="cuda"), torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    vi, vo = torch.full((n, 4), 7.0, dtype=torch.float32, device="cuda"), torch.full((n, 4), 7.0, dtype=torch.float32, device="cuda")
    hf, hp, hn, hvi, hvo = np.ones(n, np.uint32), np.zeros((n, 3)), np.zeros((n, 3)), np.full((n, 4), 7.0, np.float32), np.full((n, 4), 7.0, np.float32)
    u32, f64, f32 = C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(C.c_float)

    def both(scene=True, w=4, h=4, flags_in=True, points=True, normals=True, ch=4, values_in=True, values_out=True, alias=False, step=1, r=1.0, cos=0.0, flags=0):
        a = lib.nrays_filter_texels_device(handle if scene else None, w, h, f.data_ptr() if flags_in else None, tp.data_ptr() if points else None, tn.data_ptr() if normals else None,
                                           ch, vi.data_ptr() if values_in else None, (vi if alias else vo).data_ptr() if values_out else None, step, r, cos, flags, None)
        b = lib.nrays_filter_texels(handle if scene else None, w, h, hf.ctypes.data_as(u32) if flags_in else None, hp.ctypes.data_as(f64) if points else None,
                                    hn.ctypes.data_as(f64) if normals else None, ch, hvi.ctypes.data_as(f32) if values_in else None,
                                    (hvi if alias else hvo).ctypes.data_as(f32) if values_out else None, step, r, cos, flags)
        assert a == b
        return a
    for kw in (dict(scene=False), dict(flags_in=False), dict(points=False), dict(normals=False), dict(values_in=False), dict(values_out=False), dict(alias=True), dict(ch=0), dict(ch=5),
               dict(step=0), dict(step=65), dict(step=0xffffffff), dict(w=0), dict(h=0), dict(w=16385, h=1), dict(w=1, h=16385), dict(w=8192, h=4096), dict(r=math.nan), dict(r=0.0),
               dict(r=-1.0), dict(r=-math.inf), dict(cos=1.0), dict(cos=1.5), dict(cos=-1.5), dict(cos=math.nan), dict(flags=1), dict(flags=0x80000000)):
        assert both(**kw) == abi.ERR_BAD_ARG, kw
        assert lib.nrays_last_error()
    torch.cuda.synchronize()
    for t in (vi, vo, hvi, hvo):  # a refused call writes nothing
        assert bool((t == 7.0).all())
    assert both() == abi.OK and both(step=64) == abi.OK and both(ch=1) == abi.OK and both(r=math.inf, cos=-1.0) == abi.OK and both(cos=0.999) == abi.OK
    torch.cuda.synchronize()
    assert bool((vo == 7.0).all()) and (hvo == 7.0).all() and bool((vi == 7.0).all())  # (36 * 7 + ...) / ... of a constant map is the constant


def test_on_a_stream_of_its_own_behind_surface_texels_and_gather_points(gpu):
    """surface_texels, gather_points and filter_texels enqueued back to back on a non-default stream, nothing synchronised in between."""
    import torch
    from tests.test_surface_texels_gpu import _bake_scene
    sc, _ = _bake_scene()
    w, h = 77, 41
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        tx = nr.surface_texels(sc, 0, w, h, flip_normals=True, want=("normals",), device="cuda")
        rgb = nr.gather_points(sc, tx.points, tx.normals, nr.hemisphere_dirs(8), None, 1e-3, 1.0, 0, hit_flags=tx.flags)
        out = sc.filter_texels(tx.flags, w, h, tx.points, tx.normals, rgb, 2, 0.3, 0.5)
    stream.synchronize()
    host = lambda t: t.cpu().numpy()  # noqa: E731
    flags = host(tx.flags).view(np.uint32)
    want = nr.filter_texels_ref(flags, w, h, host(tx.points), host(tx.normals), host(rgb), 2, 0.3, 0.5)
    assert 0 < (flags & 1).sum() < w * h and host(rgb).any()
    same(host(out), want, "stream")
    assert not np.array_equal(bits(want), bits(host(rgb)))


@functools.lru_cache(maxsize=None)
def two_chart_scene():
    """A floor quad and a wall quad that meet at a right angle along an edge, each with a uv chart of its own; a gutter between and around the charts."""
    pts = su.f32_exact([[0, 0, 0], [1, 0, 0], [1, 0, 1], [0, 0, 1], [1, 0, 0], [1, 1, 0], [1, 1, 1], [1, 0, 1]])
    uv = su.f32_exact([[0.05, 0.1], [0.45, 0.1], [0.45, 0.9], [0.05, 0.9], [0.55, 0.1], [0.95, 0.1], [0.95, 0.9], [0.55, 0.9]])
    idx = np.asarray([[0, 2, 1], [0, 3, 2], [4, 6, 5], [4, 7, 6]], np.uint32)
    m = nr.PhongMaterial((0.2, 0.2, 0.2), (0.9, 0.9, 0.9), (0.0, 0.0, 0.0))
    return nr.Scene([nr.SceneNode(m, 0.0, 0.0, 1.0, 1.0, nr.Isometry3(), nr.TriMesh(pts, idx, uv))], [nr.Light((0.2, 3.0, 0.4), 0.0, 1, (1.0, 1.0, 1.0))], (0.3, 0.4, 0.5))


@pytest.mark.parametrize("on_device", [False, True])
def test_denoise_texels_is_three_mirror_passes(gpu, on_device):
    import torch
    sc, (w, h) = two_chart_scene(), (48, 40)
    tx = nr.surface_texels(sc, 0, w, h, want=("normals",))
    covered = (tx.flags & 1) != 0
    left = (np.arange(w * h) % w) < w // 2
    assert 0.3 < covered.mean() < 0.9 and covered[left].any() and covered[~left].any()
    c = np.abs((tx.normals[covered & left][0] * tx.normals[covered & ~left][0]).sum())
    assert c < 1e-9  # the two charts are at a right angle
    rng = np.random.default_rng(9)
    v = np.where(left[:, None], rng.random((w * h, 3)), 10.0 + rng.random((w * h, 3))).astype(np.float32) * covered[:, None]
    want = v
    for step in (1, 2, 4):
        want = nr.filter_texels_ref(tx.flags, w, h, tx.points, tx.normals, want, step, 0.25, 0.5)
    if on_device:
        dtx = nr.surface_texels(sc, 0, w, h, want=("normals",), device="cuda")
        dv = torch.from_numpy(v).cuda()
        got = sc.denoise_texels(dtx, dv.view(h, w, 3), 3, 0.25, 0.5)
        torch.cuda.synchronize()
        assert got.shape == (h, w, 3) and got.data_ptr() != dv.data_ptr() and np.array_equal(bits(dv.cpu().numpy()), bits(v))
        got = got.cpu().numpy().reshape(-1, 3)
    else:
        got = nr.denoise_texels(sc, tx, v, 3, 0.25, 0.5, width=w, height=h)
        assert isinstance(got, np.ndarray) and got.shape == v.shape
    same(got, want)
    assert (got[covered & left] <= 1.0).all() and (got[covered & ~left] >= 10.0).all() and not got[~covered].any()  # nothing crossed the crease or the gutter
    assert got[covered & left].std() < 0.5 * v[covered & left].std()  # and the noise inside a chart went down
    one = nr.denoise_texels(sc, tx, v.reshape(h, w, 3), 1, 0.25, 0.5)
    same(one.reshape(-1, 3), nr.filter_texels_ref(tx.flags, w, h, tx.points, tx.normals, v, 1, 0.25, 0.5))


# ---- the handle ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_call_leaves_the_render_state_alone(gpu):
    import torch
    sc, cam = su.mesh_scene(alpha_mapped=True, rotate=True)
    w, h = 128, 72
    proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], w, h)
    first = nr.render(sc, (w, h), 1, 0.0, cam["eye"], proj)
    st1, perm1 = nr.get_stats(sc), nr.last_permutation(sc)
    flags, p, nm, v = surface(np.random.default_rng(3), 96, 48, 0.7, 4)
    want = nr.filter_texels_ref(flags, 96, 48, p, nm, v, 2, 0.6, 0.1)
    with torch.cuda.stream(torch.cuda.Stream()):  # after a render, on another stream
        got = nr.filter_texels(sc, torch.from_numpy(flags.view(np.int32)).cuda(), 96, 48, torch.from_numpy(p).cuda(), torch.from_numpy(nm).cuda(), torch.from_numpy(v).cuda(), 2, 0.6, 0.1)
        torch.cuda.current_stream().synchronize()
    same(got.cpu().numpy(), want, "after a render")
    same(nr.filter_texels(sc, flags, 96, 48, p, nm, v, 2, 0.6, 0.1), want, "host entry")
    assert nr.last_permutation(sc) == perm1
    second = nr.render(sc, (w, h), 1, 0.0, cam["eye"], proj)
    st2 = nr.get_stats(sc)
    assert np.array_equal(first.view(np.uint32), second.view(np.uint32)) and nr.last_permutation(sc) == perm1
    for fld in STAT_FIELDS:
        assert getattr(st1, fld) == getattr(st2, fld), fld
