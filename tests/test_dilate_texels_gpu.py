"""Gutter dilation of a baked light map on the GPU (nrays_dilate_texels_device / nrays_dilate_texels; texel_dilate_kernel.h): the device against the numpy
mirror of the definition (nrays_amd.dilate_texels_ref) — sources, flags and value bit patterns, exact equality everywhere — over lattices on both sides of
the wave and tile seams, the optional outputs, the statuses, the host entry, a stream shared with the baker's other calls, bake_lightmap / bake_indirect
with and without `dilate`, the handle's render state, and the case the feature exists for: a baked map sampled with Bilinear renders its quad to the
border in the baked colour."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import nrays_amd as nr
from nrays_amd import abi, math3d
from tests.test_dilate_texels import random_values
from tests.test_surface_texels import quad
from tools import scenes_util as su

pytestmark = pytest.mark.gpu
STAT_FIELDS = ("rays_primary", "rays_reflection", "rays_refraction", "rays_shadow", "rays_shadow_elided", "rays_primary_traced", "generations")
SENTINEL = np.asarray([0x5e5e5e5e], np.uint32).view(np.float32)[0]  # what uncovered texels hold before a call: it must survive where nothing is in reach
LATTICES = [(1, 1), (1, 37), (37, 1), (65, 3), (3, 65), (130, 67), (257, 129)]
RADII = [1, 2, 7, 64]  # 7 and 64 lie on either side of the radius at which k_dilate_cols takes 64 rows per workgroup instead of 16 (8 | 9: below)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def any_scene():
    """The call needs a handle for its device, stream ordering and workspace; the scene's content plays no part."""
    p, idx, uv = quad()
    return nr.Scene([nr.SceneNode(nr.PhongMaterial((0.2, 0.2, 0.2), (0.5, 0.5, 0.5), (0.0, 0.0, 0.0)), 0.0, 0.0, 1.0, 1.0, nr.Isometry3(), nr.TriMesh(p, idx, uv))],
                    [nr.Light((1.0, 6.0, -2.0), 0.0, 1, (0.9, 0.9, 0.8))], (0.1, 0.2, 0.3))


def coverages(w, h, r):
    """name -> bool (h, w): the coverage patterns of one lattice."""
    rng = np.random.default_rng(w * 1000 + h * 10 + r)
    yy, xx = np.mgrid[0:h, 0:w]
    out = {"none": np.zeros((h, w), bool), "all": np.ones((h, w), bool)}
    corners = np.zeros((h, w), bool)
    corners[[0, 0, h - 1, h - 1, h // 2], [0, w - 1, 0, w - 1, w // 2]] = True
    out["corners_centre"] = corners
    out["checkerboard"] = (xx + yy) % 2 == 0  # ties everywhere
    out["random_1"] = rng.random((h, w)) < 0.01
    out["random_50"] = rng.random((h, w)) < 0.5
    out["seam_columns"] = np.isin(xx, (63, 64, 127, 128)) & (yy % 5 == 0)  # the wave seams of the row pass
    out["seam_rows"] = np.isin(yy, (15, 16, 63, 64)) & (xx % 7 == 0)       # the tile seams of the column pass (16 and 64 rows)
    one = np.zeros((h, w), bool)
    one[h // 2, w // 4] = True  # a single source: points at distance exactly r are filled, points at d2 = r^2 + 1 are not
    out["single"] = one
    return out


def device_call(flags, w, h, r, values, want_source=True):
    import torch
    f = torch.from_numpy(flags.view(np.int32)).cuda()
    v = None if values is None else torch.from_numpy(values).cuda()
    got_v, got_s, got_f = nr.dilate_texels(any_scene(), f, w, h, r, values=v, want_source=want_source)
    torch.cuda.synchronize()
    assert got_f.dtype == torch.int32 and (got_v is None or got_v.data_ptr() == v.data_ptr())  # in place
    assert np.array_equal(f.cpu().numpy().view(np.uint32), flags)  # the input flags are left alone
    return (None if got_v is None else got_v.cpu().numpy(), None if got_s is None else got_s.cpu().numpy(), got_f.cpu().numpy().view(np.uint32))


def check(got, want, what):
    if want[0] is not None:
        assert got[0].shape == want[0].shape and np.array_equal(bits(got[0]), bits(want[0])), (what, "values", int((bits(got[0]) != bits(want[0])).sum()))
    assert np.array_equal(got[1], want[1]), (what, "source", int((got[1] != want[1]).sum()))
    assert np.array_equal(got[2], want[2]), (what, "flags", int((got[2] != want[2]).sum()))


def inputs(cov, channels, seed):
    """flags with noise in bits 1 and 2, values with NaN payloads, -0, infinities and denormals at covered texels and the sentinel at uncovered ones."""
    rng = np.random.default_rng(seed)
    n = cov.size
    flags = cov.reshape(n).astype(np.uint32) | (rng.integers(0, 2, n).astype(np.uint32) << 1)
    values = random_values(rng, n, channels)
    values[~cov.reshape(n)] = SENTINEL
    return flags, values


@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("w,h", LATTICES)
def test_the_device_equals_the_mirror(gpu, w, h, r):
    for k, (name, cov) in enumerate(coverages(w, h, r).items()):
        channels = (1, 3, 4)[k % 3]
        flags, values = inputs(cov, channels, k)
        want = nr.dilate_texels_ref(flags, w, h, r, values)
        got = device_call(flags, w, h, r, values.copy())
        check(got, want, (name, channels))
        keep = (want[2] & 4) == 0
        assert np.array_equal(bits(got[0])[keep], bits(values)[keep])  # covered and unfilled texels: not written
        assert (bits(got[0])[~cov.reshape(-1) & keep] == bits(SENTINEL)).all()
        if name == "single":
            x0, y0 = w // 4, h // 2
            if x0 + r < w:
                assert got[1][y0 * w + x0 + r] == y0 * w + x0 and (y0 + 1 >= h or got[1][(y0 + 1) * w + x0 + r] == -1)
            if y0 + r < h:
                assert got[1][(y0 + r) * w + x0] == y0 * w + x0 and (x0 + 1 >= w or got[1][(y0 + r) * w + x0 + 1] == -1)


@pytest.mark.parametrize("r", [8, 9, 33])
def test_both_sides_of_the_tile_height_switch(gpu, r):
    w, h = 130, 67
    for k, name in enumerate(("random_1", "checkerboard", "seam_rows", "single")):
        flags, values = inputs(coverages(w, h, r)[name], 4, k)
        check(device_call(flags, w, h, r, values.copy()), nr.dilate_texels_ref(flags, w, h, r, values), name)


def test_four_channels_take_the_same_values_aligned_or_not(gpu):
    """Four channels at a 16-byte aligned address are copied as one 128-bit word, at any other address word by word."""
    import torch
    w, h, r = 130, 67, 7
    flags, values = inputs(coverages(w, h, r)["random_1"], 4, 5)
    want = nr.dilate_texels_ref(flags, w, h, r, values)
    f = torch.from_numpy(flags.view(np.int32)).cuda()
    for shift in (0, 1, 2, 3):
        buf = torch.zeros(w * h * 4 + 4, dtype=torch.float32, device="cuda")
        v = buf[shift:shift + w * h * 4].view(w * h, 4)
        v.copy_(torch.from_numpy(values).cuda())
        assert v.data_ptr() % 16 == 4 * shift
        got, _, _ = nr.dilate_texels(any_scene(), f, w, h, r, values=v)
        assert got.data_ptr() == v.data_ptr() and np.array_equal(bits(got.cpu().numpy()), bits(want[0])), shift
        assert not buf[:shift].any() and not buf[shift + w * h * 4:].any()


# ---- the entry points ---------------------------------------------------------------------------------------------------------------------------------------------
def test_optional_outputs_aliasing_and_the_host_entry(gpu):
    import torch
    lib, handle = abi.load_hip_lib(), any_scene().device_handle()
    w, h, r, ch = 65, 33, 3, 3
    flags, values = inputs(coverages(w, h, r)["random_1"], ch, 9)
    n = w * h
    want = nr.dilate_texels_ref(flags, w, h, r, values)
    assert (want[1] == -1).any() and (want[2] & 4).any()

    def device(use_values, use_source, use_flags, alias=False):
        f = torch.from_numpy(flags.view(np.int32)).cuda()
        v = torch.from_numpy(values).cuda()
        s, of = torch.full((n,), -7, dtype=torch.int32, device="cuda"), torch.full((n,), -7, dtype=torch.int32, device="cuda")
        rc = lib.nrays_dilate_texels_device(handle, w, h, f.data_ptr(), r, ch if use_values else 0, v.data_ptr() if use_values else None, s.data_ptr() if use_source else None,
                                            (f if alias else of).data_ptr() if use_flags else None, 0, None)
        assert rc == abi.OK, lib.nrays_last_error()
        torch.cuda.synchronize()
        return v.cpu().numpy(), s.cpu().numpy(), (f if alias else of).cpu().numpy().view(np.uint32), f.cpu().numpy().view(np.uint32)

    for use in ((True, True, True), (False, True, True), (True, False, True), (True, True, False), (False, True, False), (True, False, False), (False, False, True)):
        v, s, of, f = device(*use)
        assert np.array_equal(bits(v), bits(want[0] if use[0] else values)), use   # a NULL output is not stored at all
        assert np.array_equal(s, want[1] if use[1] else np.full(n, -7, np.int32)), use
        assert np.array_equal(of, want[2] if use[2] else np.full(n, -7, np.int32).view(np.uint32)), use
        assert np.array_equal(f, flags), use
    v, s, of, f = device(True, True, True, alias=True)  # out_flags == flags_in
    assert np.array_equal(bits(v), bits(want[0])) and np.array_equal(s, want[1]) and np.array_equal(of, want[2])
    # the host entry, through the wrapper and with each output NULL in turn
    hv, hs, hf = nr.dilate_texels(any_scene(), flags, w, h, r, values=values.copy(), want_source=True)
    check((hv, hs, hf), want, "host")
    kept = values.copy()
    hv2, hs2, hf2 = any_scene().dilate_texels(flags.reshape(h, w), w, h, r, values=kept)
    assert hv2 is kept and hs2 is None and np.array_equal(bits(kept), bits(want[0])) and np.array_equal(hf2, want[2])
    _, hs3, hf3 = nr.dilate_texels(any_scene(), flags, w, h, r, want_source=True)
    assert np.array_equal(hs3, want[1]) and np.array_equal(hf3, want[2])
    src = np.full(n, -7, np.int32)
    assert lib.nrays_dilate_texels(handle, w, h, flags.ctypes.data_as(C.POINTER(C.c_uint32)), r, 0, None, src.ctypes.data_as(C.POINTER(C.c_int32)), None, 0) == abi.OK
    assert np.array_equal(src, want[1])
    own = flags.copy()  # the host entry with out_flags == flags_in
    p = own.ctypes.data_as(C.POINTER(C.c_uint32))
    assert lib.nrays_dilate_texels(handle, w, h, p, r, 0, None, None, p, 0) == abi.OK and np.array_equal(own, want[2])
    dv, ds, df = nr.dilate_texels(any_scene(), flags, w, h, r, values=values.copy(), want_source=True, device="cuda")  # numpy in, moved to the device
    check((dv.cpu().numpy(), ds.cpu().numpy(), df.cpu().numpy().view(np.uint32)), want, "device=")


def test_statuses(gpu):
    import torch
    lib, handle = abi.load_hip_lib(), any_scene().device_handle()
    f, v, s, of = (torch.full((16,), 7, dtype=torch.int32, device="cuda"), torch.full((16, 4), 7.0, dtype=torch.float32, device="cuda"),
                   torch.full((16,), 7, dtype=torch.int32, device="cuda"), torch.full((16,), 7, dtype=torch.int32, device="cuda"))
    hf, hv, hs, hof = np.full(16, 7, np.uint32), np.full((16, 4), 7.0, np.float32), np.full(16, 7, np.int32), np.full(16, 7, np.uint32)
    u32, i32, f32 = C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_float)

    def both(scene=True, w=4, h=4, flags_in=True, r=2, ch=4, values=True, source=True, out_flags=True, flags=0):
        a = lib.nrays_dilate_texels_device(handle if scene else None, w, h, f.data_ptr() if flags_in else None, r, ch, v.data_ptr() if values else None,
                                           s.data_ptr() if source else None, of.data_ptr() if out_flags else None, flags, None)
        b = lib.nrays_dilate_texels(handle if scene else None, w, h, hf.ctypes.data_as(u32) if flags_in else None, r, ch, hv.ctypes.data_as(f32) if values else None,
                                    hs.ctypes.data_as(i32) if source else None, hof.ctypes.data_as(u32) if out_flags else None, flags)
        assert a == b
        return a
    for kw in (dict(scene=False), dict(flags_in=False), dict(values=False, source=False, out_flags=False), dict(ch=0), dict(ch=5), dict(r=0), dict(r=65), dict(r=0xffffffff),
               dict(w=0), dict(h=0), dict(w=16385, h=1), dict(w=1, h=16385), dict(w=8192, h=4096), dict(flags=1), dict(flags=0x80000000)):
        assert both(**kw) == abi.ERR_BAD_ARG, kw
        assert lib.nrays_last_error()
    torch.cuda.synchronize()
    for t in (f, v, s, of, hf, hv, hs, hof):  # a refused call writes nothing
        assert bool((t == 7).all())
    assert both(values=False, ch=0) == abi.OK and both(values=False, ch=99) == abi.OK  # channels are read only with values
    assert both() == abi.OK and both(r=64) == abi.OK and both(r=1, ch=1) == abi.OK


def test_on_a_stream_of_its_own_behind_the_bakers_calls(gpu):
    """surface_texels, shade_points and dilate_texels enqueued back to back on a non-default stream, nothing synchronised in between."""
    import torch
    from tests.test_surface_texels_gpu import _bake_scene
    sc, _ = _bake_scene()
    w, h, r = 77, 41, 3
    tx = nr.surface_texels(sc, 0, w, h, flip_normals=True, want=("normals", "uv", "node"))
    lit = nr.shade_points(sc, tx.points, tx.normals, -tx.normals, tx.node, uvs=tx.uv, hit_flags=tx.flags)
    want = nr.dilate_texels_ref(tx.flags, w, h, r, lit)
    assert 0 < (want[2] & 4).sum() and (tx.flags == 0).any()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        dtx = nr.surface_texels(sc, 0, w, h, flip_normals=True, want=("normals", "uv", "node"), device="cuda")
        dlit = nr.shade_points(sc, dtx.points, dtx.normals, -dtx.normals, dtx.node, uvs=dtx.uv, hit_flags=dtx.flags)
        v, s, f = sc.dilate_texels(dtx.flags, w, h, r, values=dlit, want_source=True)
    stream.synchronize()
    check((v.cpu().numpy(), s.cpu().numpy(), f.cpu().numpy().view(np.uint32)), want, "stream")


# ---- bake_lightmap and bake_indirect ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [None, "cuda"])
def test_bake_with_dilate_is_the_bake_followed_by_the_mirror(gpu, device):
    from tests.test_surface_texels_gpu import OCCLUSION, _bake_scene
    sc, _ = _bake_scene()
    w, h = 77, 41
    flags = nr.surface_texels(sc, 0, w, h, flip_normals=True, want=()).flags
    host = lambda a: a.cpu().numpy() if device else a  # noqa: E731
    dirs = nr.hemisphere_dirs(8)
    for bake, args, kw in ((sc.bake_lightmap, (0, w, h), dict(occlusion=OCCLUSION, flip_normals=True)), (sc.bake_indirect, (0, w, h, dirs), dict(flip_normals=True))):
        plain = host(bake(*args, device=device, **kw))
        zero = host(bake(*args, device=device, dilate=0, **kw))
        assert np.array_equal(bits(plain), bits(zero)) and not plain[flags.reshape(h, w) == 0].any()  # 0 = off
        got = host(bake(*args, device=device, dilate=3, **kw))
        want = nr.dilate_texels_ref(flags, w, h, 3, plain)[0]
        assert got.shape == plain.shape and got.dtype == np.float32 and np.array_equal(bits(got), bits(want))
        assert not np.array_equal(bits(got), bits(plain))


def test_dilate_0_is_the_composition_the_bakes_were_before(gpu):
    from tests.test_surface_texels_gpu import _bake_scene
    sc, _ = _bake_scene()
    w, h = 77, 41
    tx = nr.surface_texels(sc, 0, w, h, want=("normals", "uv", "node"))
    lit = nr.shade_points(sc, tx.points, tx.normals, -tx.normals, tx.node, uvs=tx.uv, hit_flags=tx.flags).reshape(h, w, 4)
    ind = nr.gather_points(sc, tx.points, tx.normals, nr.hemisphere_dirs(8), None, 1e-3, 1.0, 0, hit_flags=tx.flags).reshape(h, w, 3)
    for device in (None, "cuda"):
        host = lambda a: a.cpu().numpy() if device else a  # noqa: E731
        assert np.array_equal(bits(host(nr.bake_lightmap(sc, 0, w, h, device=device, dilate=0))), bits(lit))
        assert np.array_equal(bits(host(nr.bake_indirect(sc, 0, w, h, nr.hemisphere_dirs(8), device=device, dilate=0))), bits(ind))


# ---- the handle ------------------------------------------------------------------------------------------------------------------------------------------------------
def test_a_call_leaves_the_render_state_alone(gpu):
    import torch
    sc, cam = su.mesh_scene(alpha_mapped=True, rotate=True)
    w, h = 128, 72
    proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], w, h)
    first = nr.render(sc, (w, h), 1, 0.0, cam["eye"], proj)
    st1, perm1 = nr.get_stats(sc), nr.last_permutation(sc)
    flags, values = inputs(coverages(96, 48, 5)["random_1"], 4, 3)
    want = nr.dilate_texels_ref(flags, 96, 48, 5, values)
    with torch.cuda.stream(torch.cuda.Stream()):  # after a render, on another stream
        got = nr.dilate_texels(sc, torch.from_numpy(flags.view(np.int32)).cuda(), 96, 48, 5, values=torch.from_numpy(values).cuda(), want_source=True)
        torch.cuda.current_stream().synchronize()
    check((got[0].cpu().numpy(), got[1].cpu().numpy(), got[2].cpu().numpy().view(np.uint32)), want, "after a render")
    check(nr.dilate_texels(sc, flags, 96, 48, 5, values=values.copy(), want_source=True), want, "host entry")
    assert nr.last_permutation(sc) == perm1
    second = nr.render(sc, (w, h), 1, 0.0, cam["eye"], proj)
    st2 = nr.get_stats(sc)
    assert np.array_equal(first.view(np.uint32), second.view(np.uint32)) and nr.last_permutation(sc) == perm1
    for fld in STAT_FIELDS:
        assert getattr(st1, fld) == getattr(st2, fld), fld


# ---- end to end: what the feature exists for ---------------------------------------------------------------------------------------------------------------------
U = 2.0 ** -24
BILINEAR_BOUND = 4.0 * U * (1.0 + 2.0 ** -20)  # tests/test_texture_sample.py derives it for taps and weights in [0, 1]; relative to the tap when all four taps are equal
AMBIENT = (0.3, 0.6, 0.9)  # not dyadic


def _lightmap_quad(ambient, texture=None):
    """A two-triangle unit quad turned in its own plane (so that the pixel rows meet its border at every phase), uvs spanning [0.25, 0.75]^2, no lights."""
    p, idx, _ = quad()
    uv = su.f32_exact(0.25 + 0.5 * p[:, :2])
    m = nr.PhongMaterial(ambient, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), texture, None, 1.0)
    return nr.Scene([nr.SceneNode(m, 0.0, 0.0, 1.0, 1.0, nr.Isometry3((0.0, 0.0, 0.0), (0.0, 0.0, 0.2)), nr.TriMesh(p, idx, uv))], [], (0.0, 0.0, 0.0))


def _render_with_map(rgba):
    sc = _lightmap_quad((1.0, 1.0, 1.0), nr.lightmap_texture(rgba))
    c, s = math.cos(0.2), math.sin(0.2)
    at = (0.5 * c - 0.5 * s, 0.5 * s + 0.5 * c, 0.0)  # the quad's centre
    eye = (at[0], at[1], 2.0)
    w = h = 64
    proj = math3d.inverse_projection(eye, at, 40.0, w, h)
    img = nr.render(sc, (w, h), 1, 0.0, eye, proj)
    o, d, _ = nr.camera_rays((w, h), eye, proj)
    mask = nr.closest_hits(sc, o, d, want=()).node.reshape(h, w) == 0
    return img, mask


def test_a_dilated_map_renders_its_quad_in_the_baked_colour_to_the_border(gpu):
    """bake (ambient c, no lights) -> texture -> render.  Every texel a Bilinear tap can reach holds f32(c) once the gutter is filled, so a pixel on the quad is
    the blend of four equal taps — within BILINEAR_BOUND of the tap, relatively — times the ambient 1.0, one more f32 rounding.  Without dilation the taps
    beside the chart are zeros and the border pixels come out darker by far more than that."""
    c32 = np.asarray(AMBIENT, np.float32)
    tol = c32.astype(np.float64) * ((1.0 + BILINEAR_BOUND) * (1.0 + U) - 1.0)
    baked = {d: nr.bake_lightmap(_lightmap_quad(AMBIENT), 0, 32, 32, dilate=d) for d in (0, 2)}
    covered = baked[0][..., 3] == 1.0
    assert covered.sum() == 16 * 16 and np.array_equal(bits(baked[0][covered][:, :3]), bits(np.tile(c32, (256, 1)))) and not baked[0][~covered].any()
    img, mask = _render_with_map(baked[2])
    assert 1000 < mask.sum() < 64 * 64 and not img[~mask].any()
    err = np.abs(img[mask].astype(np.float64) - c32.astype(np.float64))
    print("dilate=2: %d quad pixels, max |pixel - c| = %s, bound %s" % (mask.sum(), err.max(axis=0), tol))
    assert (err <= tol).all()
    dark, mask0 = _render_with_map(baked[0])
    assert np.array_equal(mask0, mask)
    below = (c32.astype(np.float64) - dark[mask].astype(np.float64)) > tol
    print("dilate=0: %d of %d quad pixels darker than the bound" % (below.any(axis=1).sum(), mask.sum()))
    assert below.any(axis=1).sum() >= 16 and not below.all()
