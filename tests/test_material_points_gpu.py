"""nrays_material_points_device / nrays_material_points on the GPU: every output is compared BIT FOR BIT with the numpy mirror material_points_ref (which
tests/test_material_points.py pins to the CPU oracle without a GPU), in the numpy (host) and the torch (device) form; the new kernel against the existing shading
(shade_points on a lightless twin, and under one light straight above); tex_sample with exact uvs against tests/texture_cases.py; sizes around a wave, past the
grid's stride and across the chunk seam; every combination of absent outputs between guard words; the handle's render state; texel_albedo and indirect_points."""
import ctypes as C
import itertools

import numpy as np
import pytest

import nrays_amd as nr
from nrays_amd import abi, math3d
from nrays_amd.marshal import CURRENT
from tests.test_gather_maps import FURNACE_ATLAS, FURNACE_KA, furnace_mesh, furnace_tables
from tests.test_irradiance import gamma, same as same32, unit_vectors
from tests.test_irradiance_vis_gpu import two_rooms
from tests.test_material_points import (ALL, MODE_IDS, MODES, WANTS, check_sampler, diffuse_points, diffuse_scene, lightless, material_args, mirror, same, same_terms,
                                        sampler_case, sampler_nodes, shade_args, skip_case, uv_variants)
from tests.test_shade_points import rich_analytic_scene, scattered_rays
from tests.test_shade_points_gpu import STAT_FIELDS, _camera, quad_scene
from tools import scenes_util as su

pytestmark = pytest.mark.gpu

WIDTH = {"ambient": 4, "diffuse": 3, "specular": 4, "node": 4}
_CASES = {}


def _quads():
    sc, cam = quad_scene()
    return (sc,) + _camera(cam, 64, 64, 9)[:2]


def _analytic():
    sc, _ = rich_analytic_scene()
    return (sc,) + scattered_rays(np.random.default_rng(21), 4096)


SCENES = {"quads": _quads, "analytic": _analytic}


def case(name):
    """Per scene, computed once and left unchanged: the scene, the closest hits of its rays through the blocking form as the arguments of material_points /
    shade_points (misses included), and the mirror's four outputs there."""
    if name not in _CASES:
        sc, o, d = SCENES[name]()
        hits = nr.closest_hits(sc, o, d)
        toi = np.where((hits.flags & 1) != 0, hits.toi, 0.0)
        a = dict(points=o + d * toi[:, None], normals=hits.normal, uvs=hits.uv, nodes=hits.node, hit_flags=hits.flags, view_dirs=d)
        _CASES[name] = dict(sc=sc, hits=hits, a=a, ref=mirror(sc, a, ALL))
    return _CASES[name]


def to_device(a):
    """The arrays of a point set as tensors on the GPU (flag words as int32, as closest_hits returns them on tensors); None stays None."""
    import torch
    signed = lambda v: v.view(np.int32) if v.dtype == np.uint32 else v  # noqa: E731
    return {k: None if v is None else torch.from_numpy(signed(np.ascontiguousarray(v))).cuda() for k, v in a.items()}


def device_terms(sc, a, want, stream=None):
    """material_points on torch tensors (on `stream` when given), copied back."""
    import torch
    t = to_device(material_args(a))
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            r = nr.material_points(sc, want=want, **t)
        stream.synchronize()
    else:
        r = nr.material_points(sc, want=want, **t)
    torch.cuda.synchronize()
    for name, out in zip(ALL, r):
        assert (out is None) == (name not in want)
        assert out is None or (out.dtype == (torch.float64 if name == "node" else torch.float32) and tuple(out.shape) == (len(a["nodes"]), WIDTH[name]))
    return nr.MaterialTerms(*(None if out is None else out.cpu().numpy() for out in r))


# ---- 1: the device against the mirror ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SCENES))
def test_equals_the_mirror_bit_for_bit(gpu, name):
    """All four outputs by bit pattern, both forms, at the closest hits as they come (misses included) and with the uv rule's variants: no uvs, flag bit 1 cleared on
    a third of the points, no flags."""
    c = case(name)
    sc, n = c["sc"], len(c["a"]["nodes"])
    live = (c["a"]["hit_flags"] & 1) != 0
    hit_nodes = set(c["a"]["nodes"][live].tolist())
    assert 0 < live.sum() < n and (hit_nodes == {0, 1} if name == "quads" else {sc._nodes[k].material.kind for k in hit_nodes} == {abi.MAT_PHONG, abi.MAT_NORMAL, abi.MAT_UV})
    for k, v in enumerate(uv_variants(c["a"], 7)):
        ref = c["ref"] if k == 0 else mirror(sc, v, ALL)
        assert same_terms(nr.material_points(sc, want=ALL, **material_args(v)), ref), k
        assert same_terms(device_terms(sc, v, ALL), ref), k
    assert same_terms(sc.material_hits(c["hits"], want=ALL), c["ref"])
    assert not c["ref"].ambient[~live].any() and c["ref"].node[live].any(axis=1).all()
    assert np.unique(c["ref"].diffuse[live], axis=0).shape[0] > (100 if name == "quads" else 3)


# ---- 2: the device against the existing shading -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SCENES))
def test_ambient_is_shade_points_on_the_lightless_twin(gpu, name):
    """Without lights Material::compute is Material::ambiant for all three kinds: k_material_points against material_compute as a render runs it, bit for bit."""
    c = case(name)
    dark = lightless(c["sc"])
    for k, v in enumerate(uv_variants(c["a"], 8)):
        assert same(nr.material_points(c["sc"], want=("ambient",), **material_args(v)).ambient, nr.shade_points(dark, **shade_args(v))), k


def test_diffuse_is_shade_points_under_one_light_straight_above(gpu):
    """diffuse_scene(): ka = ks = 0 and one white point light straight above the point: compute is kd * tex (dcoeff = 1, scoeff = -0, axpy with 1), as values."""
    sc, a = diffuse_scene(), diffuse_points()
    for v in (a, dict(a, uvs=None), dict(a, hit_flags=None)):
        got = nr.material_points(sc, want=("diffuse",), **material_args(v)).diffuse
        lit = nr.shade_points(sc, **shade_args(v))
        assert not np.isnan(lit).any() and np.array_equal(got, lit[:, :3])
        assert same(got, mirror(sc, v, ("diffuse",)).diffuse)
    assert np.unique(got, axis=0).shape[0] > 300  # (textured: not the three kd)


# ---- 3: tex_sample alone, with exact uvs ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,interp,overflow", MODES, ids=MODE_IDS)
def test_tex_sample_with_exact_uvs_against_texture_cases(gpu, fmt, interp, overflow):
    """The texture_cases pairs (boundaries, round-half ties, +-0, denormals, +-inf, NaN) straight through `uvs`: no mesh has to carry them.  The texture is colour
    texture and opacity map of a ka = 1 material, so out_ambient is the sample's four channels."""
    c = sampler_case(fmt, interp, overflow)
    sc = nr.Scene(sampler_nodes(fmt, interp, overflow), [], (0.0, 0.0, 0.0))
    n = len(c["nodes"])
    got = nr.material_points(sc, c["nodes"], np.tile([0.0, 0.0, 1.0], (n, 1)), c["uvs"], want=("ambient",)).ambient
    check_sampler(got, c, interp)
    assert same(got, nr.material_points_ref(sc._nodes, c["nodes"], np.zeros((n, 3)), c["uvs"], want=("ambient",)).ambient)


# ---- 4: sizes ---------------------------------------------------------------------------------------------------------------------------------------------------
STRIDE = 2048 * 256 + 257  # past kMaxGrid workgroups of 256 lanes: the stride loop's second pass
_BIG = []


def big_case():
    """STRIDE points of quad_scene()'s nodes — random nodes (some outside the scene), uvs and flags — and the mirror's outputs, computed once; a call of n points is
    checked against the first n rows."""
    if not _BIG:
        sc, _ = quad_scene()
        rng = np.random.default_rng(51)
        a = dict(nodes=rng.integers(-1, 3, STRIDE).astype(np.int32), normals=unit_vectors(52, STRIDE), uvs=rng.uniform(-2.0, 3.0, size=(STRIDE, 2)),
                 hit_flags=rng.integers(0, 4, STRIDE).astype(np.uint32))
        _BIG.append((sc, a, mirror(sc, a, ALL)))
    return _BIG[0]


def head(a, n):
    return {k: v[:n] for k, v in a.items()}


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, STRIDE])
def test_sizes_around_a_wave_a_workgroup_and_the_grid(gpu, n):
    sc, a, ref = big_case()
    want = nr.MaterialTerms(*(r[:n] for r in ref))
    assert same_terms(nr.material_points(sc, want=ALL, **head(a, n)), want)
    assert same_terms(device_terms(sc, head(a, n), ALL), want)


def test_the_chunk_seam(gpu):
    """2^22 + 65 points through the blocking form, two chunks: nodes without a texture, uvs given, only out_diffuse asked for — kd of the node, a table lookup."""
    sc, _ = rich_analytic_scene()
    n = (1 << 22) + 65
    rng = np.random.default_rng(53)
    nodes = rng.integers(0, len(sc._nodes), n).astype(np.int32)
    kd = np.asarray([m.diffuse_color if m.kind == abi.MAT_PHONG else (0.0, 0.0, 0.0) for m in (s.material for s in sc._nodes)], np.float32)
    t = nr.material_points(sc, nodes, uvs=rng.uniform(0.0, 1.0, size=(n, 2)), want=("diffuse",))
    assert t.ambient is None and t.specular is None and t.node is None
    assert same(t.diffuse, kd[nodes]) and len(np.unique(nodes[(1 << 22) - 3:])) > 3


GUARD = 4  # words of the output's own type in front of and behind it


def _guarded(form, n, name, wanted):
    """An output of n rows between guard words: (the whole buffer, the address of its first row or None).  Host: numpy; device: a tensor."""
    import torch
    dtype = np.float64 if name == "node" else np.float32
    whole = np.full(n * WIDTH[name] + 2 * GUARD, 7.0, dtype)
    if form == "device":
        whole = torch.from_numpy(whole).cuda()
        return whole, (whole.data_ptr() + GUARD * whole.element_size()) if wanted else None
    return whole, (C.cast(whole.ctypes.data + GUARD * whole.itemsize, C.POINTER(C.c_double if name == "node" else C.c_float)) if wanted else None)


@pytest.mark.parametrize("form", ["host", "device"])
def test_every_combination_of_absent_outputs_between_guard_words(gpu, form):
    """n = 257, raw calls: a NULL output is not stored, the others hold the mirror's bits, and the guard words in front of and behind every buffer — and the whole
    buffer of an output that was not passed — are untouched."""
    import torch
    sc, a, ref = big_case()
    n = 257
    lib, h = abi.load_hip_lib(), sc.device_handle()
    ins = head(a, n)
    if form == "device":
        t = to_device(ins)
        pin = [t[k].data_ptr() for k in ("normals", "uvs", "nodes", "hit_flags")]
    else:
        keep = [np.ascontiguousarray(ins[k]) for k in ("normals", "uvs", "nodes", "hit_flags")]
        pin = [nr.scene.np_ptr(x) for x in keep]
    for want in WANTS + [()]:
        bufs = {name: _guarded(form, n, name, name in want) for name in ALL}
        args = [h, n] + pin + [bufs[name][1] for name in ALL] + [0]
        rc = lib.nrays_material_points_device(*args, torch.cuda.current_stream().cuda_stream) if form == "device" else lib.nrays_material_points(*args)
        torch.cuda.synchronize()
        assert rc == (abi.OK if want else abi.ERR_BAD_ARG), want
        for name, r in zip(ALL, ref):
            whole = bufs[name][0].cpu().numpy() if form == "device" else bufs[name][0]
            assert (whole[:GUARD] == 7.0).all() and (whole[-GUARD:] == 7.0).all(), (want, name)
            body = whole[GUARD:-GUARD].reshape(n, WIDTH[name])
            assert same(body, r[:n]) if name in want else (body == 7.0).all(), (want, name)


@pytest.mark.parametrize("form", ["host", "device"])
def test_statuses(gpu, form):
    """Every BAD_ARG of the header with a scene in hand, outputs untouched; n == 0 is OK and touches nothing."""
    import torch
    sc, a, _ = big_case()
    lib, h = abi.load_hip_lib(), sc.device_handle()
    n = 8
    ins = head(a, n)
    if form == "device":
        t = to_device(ins)
        p = {k: t[k].data_ptr() for k in ins}
    else:
        keep = {k: np.ascontiguousarray(v) for k, v in ins.items()}
        p = {k: nr.scene.np_ptr(v) for k, v in keep.items()}

    def call(n_, normals, uvs, nodes, flags_, want, flag_bits):
        bufs = {name: _guarded(form, n, name, name in want) for name in ALL}
        args = [h, n_, normals, uvs, nodes, flags_] + [bufs[name][1] for name in ALL] + [flag_bits]
        rc = lib.nrays_material_points_device(*args, torch.cuda.current_stream().cuda_stream) if form == "device" else lib.nrays_material_points(*args)
        torch.cuda.synchronize()
        untouched = all(bool(((b[0].cpu().numpy() if form == "device" else b[0]) == 7.0).all()) for b in bufs.values())
        return rc, untouched
    assert call(n, p["normals"], p["uvs"], None, p["hit_flags"], ALL, 0) == (abi.ERR_BAD_ARG, True)             # NULL nodes
    assert call(n, p["normals"], p["uvs"], p["nodes"], p["hit_flags"], (), 0) == (abi.ERR_BAD_ARG, True)        # no output
    assert call(n, None, p["uvs"], p["nodes"], p["hit_flags"], ("ambient",), 0) == (abi.ERR_BAD_ARG, True)      # NULL normals with out_ambient
    assert call(n, None, p["uvs"], p["nodes"], p["hit_flags"], ALL, 0) == (abi.ERR_BAD_ARG, True)
    for bit in (1, 2, 1 << 31):
        assert call(n, p["normals"], p["uvs"], p["nodes"], p["hit_flags"], ALL, bit) == (abi.ERR_BAD_ARG, True)  # any flag bit
    assert call(0, p["normals"], p["uvs"], p["nodes"], p["hit_flags"], ALL, 0) == (abi.OK, True)                 # n == 0: nothing is touched
    assert call(n, None, None, p["nodes"], None, ("diffuse", "specular", "node"), 0)[0] == abi.OK                # everything optional absent


@pytest.mark.parametrize("form", ["host", "device"])
def test_skipped_points_are_exact_zeros_and_their_inputs_are_not_read(gpu, form):
    sc, _ = quad_scene()
    a, skipped = skip_case()
    got = nr.material_points(sc, want=ALL, **a) if form == "host" else device_terms(sc, a, ALL)
    assert same_terms(got, mirror(sc, a, ALL))
    for out in got:
        assert not out[skipped].view(np.uint32).any() and not np.isnan(out).any()


# ---- 5: the handle's render state -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SCENES))
def test_a_batch_leaves_the_render_state_alone(gpu, name):
    import torch
    c = case(name)
    sc, cam = (quad_scene if name == "quads" else rich_analytic_scene)()  # a fresh handle of the same scene
    w, h = 128, 72
    proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], w, h)
    first = nr.render(sc, (w, h), 1, 0.0, cam["eye"], proj)
    st1, perm1 = nr.get_stats(sc), nr.last_permutation(sc)
    assert same_terms(device_terms(sc, c["a"], ALL, stream=torch.cuda.Stream()), c["ref"])
    assert same_terms(nr.material_points(sc, want=ALL, **material_args(c["a"])), c["ref"])
    st_mid = nr.get_stats(sc)
    assert nr.last_permutation(sc) == perm1
    second = nr.render(sc, (w, h), 1, 0.0, cam["eye"], proj)
    st2 = nr.get_stats(sc)
    assert np.array_equal(first.view(np.uint32), second.view(np.uint32)) and nr.last_permutation(sc) == perm1
    for f in STAT_FIELDS:
        assert getattr(st1, f) == getattr(st_mid, f) == getattr(st2, f), f


# ---- 6: texel_albedo --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [None, "cuda"])
@pytest.mark.parametrize("fmt", ["rgba8", "rgba32f"])
def test_texel_albedo_of_a_nearest_texture_on_its_own_lattice_is_kd_times_the_texels(gpu, fmt, device):
    """A quad whose uvs are the identity (it spans the unit square of uv space and half a texel more on every side, so every lattice point lies inside it) with a
    W x H Nearest texture, at the W x H lattice: lattice point (x, y) reads texel (x, y), and the result is kd * texels exactly."""
    W, H = 7, 5
    rng = np.random.default_rng(61)
    texels = rng.integers(0, 256, size=(H, W, 4), dtype=np.uint8) if fmt == "rgba8" else rng.uniform(0.0, 1.0, size=(H, W, 4)).astype(np.float32)
    kd = (0.75, 0.3, 0.9)
    mat = nr.PhongMaterial((0.1, 0.1, 0.1), kd, (0.2, 0.2, 0.2), nr.Texture2d(nr.ImageData(texels), nr.Interpolation.Nearest, nr.Overflow.ClampToEdges), None, 10.0)
    mu, mv = 0.5 / (W - 1), 0.5 / (H - 1)
    uv = su.f32_exact([[-mu, -mv], [1 + mu, -mv], [1 + mu, 1 + mv], [-mu, 1 + mv]])
    pts = su.f32_exact(np.stack([uv[:, 0], np.zeros(4), uv[:, 1]], axis=1))
    sc = nr.Scene([nr.SceneNode(mat, 0.0, 0.0, 1.0, 1.0, nr.Isometry3(), nr.TriMesh(pts, np.asarray([[0, 2, 1], [0, 3, 2]], np.uint32), uv))], [], (0.0, 0.0, 0.0))
    got = sc.texel_albedo(0, W, H, device=device)
    if device:
        import torch
        assert torch.is_tensor(got) and got.dtype == torch.float32
        got = got.cpu().numpy()
    f32 = texels.astype(np.float32) / np.float32(255.0) if fmt == "rgba8" else texels
    assert got.shape == (H, W, 3) and got.dtype == np.float32
    assert same(got, np.asarray(kd, np.float32)[None, None, :] * f32[:, :, :3])
    # a lattice the quad covers only in part: zeros where no triangle covers a texel
    half = nr.Scene([nr.SceneNode(mat, 0.0, 0.0, 1.0, 1.0, nr.Isometry3(), nr.TriMesh(pts, np.asarray([[0, 2, 1]], np.uint32), uv))], [], (0.0, 0.0, 0.0))
    part = nr.texel_albedo(half, 0, W, H)
    covered = (nr.surface_texels(half, 0, W, H, want=()).flags & 1).reshape(H, W) != 0
    assert 0 < covered.sum() < W * H and not part[~covered].view(np.uint32).any() and same(part[covered], got[covered])


def test_bake_bounces_with_texel_albedo_is_bake_bounces_with_the_constant(gpu):
    """The closed furnace cube with kd = 0.5 and no texture: texel_albedo is 0.5 at every covered texel and +0 elsewhere, and bake_bounces with it equals
    bake_bounces(albedo=(0.5, 0.5, 0.5)) by bit pattern over the whole map (an uncovered texel's product is 0 either way and the dilation fills it)."""
    pts, idx, uvs = furnace_mesh()
    mat = nr.PhongMaterial(FURNACE_KA, (0.5, 0.5, 0.5), (0.3, 0.3, 0.3), None, None, 20.0)
    sc = nr.Scene([nr.SceneNode(mat, 0.0, 0.0, 1.0, 1.0, nr.Isometry3(), nr.TriMesh(pts, idx, uvs))], [], (0.0, 0.0, 0.0))
    L, rot = furnace_tables()
    N = FURNACE_ATLAS
    albedo = nr.texel_albedo(sc, 0, N, N, flip_normals=True)
    live = (nr.surface_texels(sc, 0, N, N, flip_normals=True, want=()).flags & 1).reshape(N, N) != 0
    assert live.sum() == 6 * 64 and (albedo[live] == np.float32(0.5)).all() and not albedo[~live].view(np.uint32).any()
    for B in (1, 2):
        a = nr.bake_bounces(sc, 0, N, N, L, B, albedo, rot, dilate=64, flip_normals=True)
        b = nr.bake_bounces(sc, 0, N, N, L, B, (0.5, 0.5, 0.5), rot, dilate=64, flip_normals=True)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and (a[..., :3] > np.asarray(FURNACE_KA, np.float32)).all()


# ---- 7: indirect_points -----------------------------------------------------------------------------------------------------------------------------------------
def two_rooms_textured_wall():
    """two_rooms() of tests/test_irradiance_vis_gpu.py with its dividing wall as a TriMesh box of the same extents that carries uvs and quad_scene()'s colour
    texture (the room's own kd, no ambient term)."""
    base = two_rooms()
    tex = quad_scene()[0]._nodes[0].material.texture
    mat = nr.PhongMaterial((0.0, 0.0, 0.0), (0.8, 0.7, 0.6), (0.0, 0.0, 0.0), tex, None, 20.0)
    lo, hi = np.asarray([-0.05, 0.0, -2.5]), np.asarray([0.05, 5.0, 2.5])
    corners = np.asarray([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for i, j, k in itertools.product((0, 1), repeat=3)])  # index 4 i + 2 j + k
    uv = np.stack([(corners[:, 2] + 2.5) / 5.0, corners[:, 1] / 5.0], axis=1)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]  # outward winding: -x, +x, -y, +y, -z, +z
    idx = np.asarray([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.uint32)
    wall = nr.SceneNode(mat, 0.0, 0.0, 1.0, 1.0, nr.Isometry3(), nr.TriMesh(su.f32_exact(corners), idx, su.f32_exact(uv)))
    return nr.Scene(list(base._nodes[:6]) + [wall], base._lights, base._background)


def wall_rays(n, seed):
    """Rays in room B towards the dividing wall: they end on its face x = 0.05, around the middles of the probe grid's cell faces."""
    rng = np.random.default_rng(seed)
    cy, cz = rng.integers(1, 4, size=n) + 0.0, rng.integers(-2, 2, size=n) + 0.5
    target = np.stack([np.full(n, 0.05), cy + rng.uniform(-0.2, 0.2, size=n), cz + rng.uniform(-0.2, 0.2, size=n)], axis=1)
    o = np.stack([rng.uniform(1.0, 3.0, size=n), rng.uniform(1.0, 4.0, size=n), rng.uniform(-1.5, 1.5, size=n)], axis=1)
    d = target - o
    return o, d / np.sqrt((d * d).sum(axis=1))[:, None]


def test_indirect_points_on_the_device_and_behind_a_wall(gpu):
    """The torch form equals the numpy form bit for bit, and both the expression on the mirrors, at the hits of rays in the two-room scene whose dividing wall is a
    textured node.  With visibility on, the points of tests/test_irradiance_vis_gpu.py behind that wall stay as dark relative to the plain lookup as that file asserts
    for the irradiance: the reflectance is one factor a point and channel in both, so the ratio is the irradiance's (within the four roundings of the two products
    on either side) and the ordering is unchanged."""
    import torch
    sc = two_rooms_textured_wall()
    k = next(k for k in range(64, 1025) if len(np.unique(nr.oct_texel(nr.sphere_dirs(k), 8))) == 64)
    L = nr.sphere_dirs(k)
    grid = nr.bake_probe_grid(sc, (-5.5, 0.5, -2.0), (1.0, 1.0, 1.0), (12, 5, 5), L, 3, device=CURRENT)
    vis, valid = nr.bake_probe_visibility(sc, grid, L, 8, max_dist=2.0, near_dist=0.2, floor=0.0)
    grid = grid._replace(valid=valid)
    g_np = grid._replace(sh=grid.sh.cpu().numpy(), valid=valid.cpu().numpy().view(np.uint32))
    v_np = vis._replace(moments=vis.moments.cpu().numpy())
    o, d = wall_rays(300, 710)
    so, sd = scattered_rays(np.random.default_rng(711), 300)  # and anywhere: other nodes, misses through no opening (closed rooms), rays from outside
    o, d = np.concatenate([o, so * 0.3 + np.asarray([0.0, 2.5, 0.0])]), np.concatenate([d, sd])
    hits = nr.closest_hits(sc, o, d)
    on_wall = (hits.node == 6) & (np.arange(len(o)) < 300)
    assert on_wall[:300].all() and (hits.flags[on_wall] == 3).all() and float(np.abs(hits.toi[on_wall] * d[on_wall, 0] + o[on_wall, 0] - 0.05).max()) < 1e-6
    p = o + d * np.where((hits.flags & 1) != 0, hits.toi, 0.0)[:, None]
    nm = np.where(((hits.normal * d).sum(axis=1) > 0)[:, None], -hits.normal, hits.normal)  # towards the side the ray came from
    args = dict(points=p, normals=nm, nodes=hits.node, uvs=hits.uv, hit_flags=hits.flags)
    dev = to_device(args)
    for kw_np, kw_t in ((dict(), dict()), (dict(facing=True), dict(facing=True)), (dict(visibility=v_np), dict(visibility=vis))):
        host = nr.indirect_points(sc, grid=g_np, **args, **kw_np)
        tens = sc.indirect_points(grid=grid, **dev, **kw_t)
        assert host.dtype == np.float32 and host.shape == (len(o), 3) and torch.is_tensor(tens) and tens.dtype == torch.float32
        dm = nr.material_points_ref(sc._nodes, hits.node, uvs=hits.uv, hit_flags=hits.flags, want=("diffuse",)).diffuse
        E = nr.irradiance_points_ref(p, nm, g_np, hit_flags=hits.flags, **kw_np)[0]
        assert same32(host, (dm * E) * nr.scene.INV_PI_F32) and same32(tens.cpu().numpy(), host)
    assert np.unique(dm[on_wall], axis=0).shape[0] > 100  # (the wall's texture, not one kd)
    # Behind the wall.  ON the wall's own far face the comparison of that file does not hold for the irradiance itself (the weights are normalised after the
    # visibility factor, and there the zero probes of room B are held down too), so it is made where that file makes it: at ITS points — the same generator and
    # seed: room B, within one cell of the wall, looking at it — which here carry the material of what they look at, the node and uv of the hit straight across.
    rng = np.random.default_rng(700)
    n = 300
    cy, cz = rng.integers(1, 4, size=n) + 0.0, rng.integers(-2, 2, size=n) + 0.5
    p = np.stack([rng.uniform(0.3, 0.45, size=n), cy + rng.uniform(-0.2, 0.2, size=n), cz + rng.uniform(-0.2, 0.2, size=n)], axis=1)
    nm = np.array([-1.0, 0.0, 0.0]) + rng.uniform(-0.2, 0.2, size=(n, 3))
    nm /= np.sqrt((nm * nm).sum(axis=1))[:, None]
    across = nr.closest_hits(sc, p, np.tile([-1.0, 0.0, 0.0], (n, 1)))
    assert (across.node == 6).all() and (across.flags == 3).all()
    args = dict(points=p, normals=nm, nodes=across.node, uvs=across.uv, hit_flags=across.flags)
    plain, seen = nr.indirect_points(sc, grid=g_np, **args), nr.indirect_points(sc, grid=g_np, visibility=v_np, **args)
    e_plain, e_seen = nr.irradiance_points(sc, p, nm, g_np), nr.irradiance_points(sc, p, nm, g_np, visibility=v_np)
    assert (plain > 0).all() and (e_plain > 0).all()
    ratio, e_ratio = seen.astype(np.float64) / plain.astype(np.float64), e_seen.astype(np.float64) / e_plain.astype(np.float64)
    print("light behind the wall, indirect_vis / indirect_plain per channel: median %.4g, max %.4g, min %.4g (plain median %.4g); the irradiance's own ratio: max %.4g"
          % (np.median(ratio), ratio.max(), ratio.min(), np.median(plain), e_ratio.max()))
    assert np.unique(nr.material_points(sc, across.node, uvs=across.uv, want=("diffuse",)).diffuse, axis=0).shape[0] > 100
    assert (seen >= 0).all() and (seen < plain).all()
    # one factor a point and channel: the ratio is the irradiance's, up to the two roundings of each product
    lit = e_seen != 0  # (a point whose probes are all held down to nothing is exactly dark in both)
    assert lit.any() and not seen[~lit].any() and float(np.abs(ratio[lit] / e_ratio[lit] - 1.0).max()) <= gamma(4)
