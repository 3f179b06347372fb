"""Material::compute on caller-supplied surface points (nrays_shade_points_device / nrays_shade_points; nrays_amd.shade_points, shade_hits) on the GPU:
bit for bit against Scene::trace where a node neither reflects nor refracts, against the oracle's material_compute (tests/shade_oracle_shim.c) on every
point, a scene with a non-finite light, the skip rule, sizes around a wave and across the chunk seam, the device path, and the handle's render state."""
import ctypes as C

import numpy as np
import pytest

import nrays_amd as nr
from nrays_amd import abi, math3d
from tests.test_shade_points import build_shade_shim, odd_keys, opaque, rich_analytic_scene, scattered_rays, shim_shade
from tools import scenes_util as su
from tools import standins

pytestmark = pytest.mark.gpu
TOL = 1e-4  # the project's HIP-versus-oracle bound (tests/test_trace_rays_gpu.py)
STAT_FIELDS = ("rays_primary", "rays_reflection", "rays_refraction", "rays_shadow", "rays_shadow_elided", "rays_primary_traced", "generations")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shade_shim(tmp_path_factory.mktemp("shade_shim_gpu"))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_values(a, b):
    """Equal as values (-0 == +0), NaN nowhere."""
    return a.shape == b.shape and bool(np.all(a == b))


# ---- scenes ---------------------------------------------------------------------------------------------------------------------------------------
def quad_scene():
    """A textured two-triangle floor quad (4 x 4 RGBA8, bilinear, wrap) under an occluder quad whose material carries an opacity map with texels 0, 0.5
    and 1 (and the colour texture): the floor's shadow rays are blocked, pass, or pick up a colour filter."""
    rng = np.random.default_rng(4)
    rgba = rng.integers(40, 256, size=(4, 4, 4), dtype=np.uint8)
    rgba[..., 3] = 255
    colour = nr.Texture2d(nr.ImageData(rgba), nr.Interpolation.Bilinear, nr.Overflow.Wrap)
    op = np.ones((4, 4, 4), np.float32)
    op[..., 3] = np.asarray([[0.0, 0.5, 1.0, 0.5], [1.0, 0.0, 0.5, 0.0], [0.5, 1.0, 0.0, 1.0], [0.0, 0.5, 0.5, 1.0]], np.float32)
    opacity = nr.Texture2d(nr.ImageData(op), nr.Interpolation.Nearest, nr.Overflow.Wrap)
    floor_m = nr.PhongMaterial((0.2, 0.2, 0.2), (0.9, 0.9, 0.9), (0.6, 0.6, 0.6), colour, None, 40.0)
    lace_m = nr.PhongMaterial((0.2, 0.15, 0.1), (0.8, 0.7, 0.6), (0.4, 0.4, 0.4), colour, opacity, 20.0)
    idx = np.asarray([[0, 2, 1], [0, 3, 2]], dtype=np.uint32)
    uv = np.asarray([[0.0, 0.0], [1.5, 0.0], [1.5, 1.5], [0.0, 1.5]])  # past 1: the wrap
    floor = su.f32_exact([[-2.5, 0.0, -2.5], [2.5, 0.0, -2.5], [2.5, 0.0, 2.5], [-2.5, 0.0, 2.5]])
    lace = su.f32_exact([[-1.25, 1.0, -1.25], [1.25, 1.0, -1.25], [1.25, 1.0, 1.25], [-1.25, 1.0, 1.25]])
    nodes = [nr.SceneNode(floor_m, 0.0, 0.0, 1.0, 1.0, nr.Isometry3(), nr.TriMesh(floor, idx, su.f32_exact(uv))),
             nr.SceneNode(lace_m, 0.0, 0.0, 1.0, 1.0, nr.Isometry3(), nr.TriMesh(lace, idx, su.f32_exact(uv / 1.5)))]
    return nr.Scene(nodes, [nr.Light((0.4, 5.0, 0.3), 0.0, 1, (1.0, 0.95, 0.9))], (0.1, 0.2, 0.3)), dict(eye=(0.3, 3.5, -5.0), at=(0.0, 0.0, 0.0), fovy=50.0)


def _camera(cam, w, h, seed):
    proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], w, h)
    return nr.camera_rays((w, h), cam["eye"], proj, seed=seed)


def _analytic():
    sc, _ = rich_analytic_scene()
    o, d = scattered_rays(np.random.default_rng(21), 4096)
    return sc, opaque(sc), o, d, odd_keys(np.random.default_rng(22), 4096)


def _hair():
    sc, cam = standins.hairball_scene(strands=400)
    return (sc, sc) + _camera(cam, 96, 96, 3)


def _quads():
    sc, cam = quad_scene()
    return (sc, sc) + _camera(cam, 64, 64, 9)


SCENES = {"analytic": _analytic, "hair": _hair, "quads": _quads}
_CASES = {}


def hit_arrays(o, d, hits):
    """The arguments shade_hits() builds from a numpy CastHits, for the oracle and for direct shade_points calls."""
    toi = np.where((hits.flags & 1) != 0, hits.toi, 0.0)
    step = d * toi[:, None]
    return dict(points=o + step, normals=hits.normal, view_dirs=d, nodes=hits.node, uvs=hits.uv, hit_flags=hits.flags)


def case(name):
    """Per scene, computed once and shared (nothing writes them): the scene as it is and its comparison variant for the identity test (every node opaque and
    non-reflective where the scene has others), rays, keys, the closest hits and shade_hits() on the scene as it is, through the blocking forms."""
    if name not in _CASES:
        full, ident, o, d, k = SCENES[name]()
        hits = nr.closest_hits(full, o, d)
        _CASES[name] = dict(full=full, ident=ident, o=o, d=d, k=k, hits=hits, args=hit_arrays(o, d, hits), shaded=nr.shade_hits(full, o, d, hits, keys=k))
    return _CASES[name]


def device_shade(sc, a, keys=None, stream=None):
    """shade_points on torch tensors (on `stream` when given), copied back."""
    import torch
    signed = lambda v: v.view(np.int32) if v.dtype == np.uint32 else v  # noqa: E731  (the flag words as closest_hits returns them on tensors)
    t = {k: None if v is None else torch.from_numpy(signed(np.ascontiguousarray(v))).cuda() for k, v in a.items()}
    tk = None if keys is None else torch.from_numpy(np.ascontiguousarray(keys).view(np.int64)).cuda()
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            r = nr.shade_points(sc, keys=tk, **t)
        stream.synchronize()
    else:
        r = nr.shade_points(sc, keys=tk, **t)
    torch.cuda.synchronize()
    assert r.dtype == torch.float32 and tuple(r.shape) == (len(a["points"]), 4)
    return r.cpu().numpy()


# ---- 1: bit identity with Scene::trace --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SCENES))
def test_equals_trace_where_a_node_neither_reflects_nor_refracts(gpu, name):
    """trace(ray) = obj.rgb * 1 on a node with refl_mix 0, alpha 1 and material alpha 1 (scene.rs:179-190): shade_hits at the closest hits gives trace_rays' colour."""
    c = case(name)
    sc, o, d, k = c["ident"], c["o"], c["d"], c["k"]
    if name == "hair":
        flags = (C.c_uint32 * 2)()
        abi.check(abi.load_hip_lib().nrays_debug_scene_flags(sc.device_handle(), flags))
        assert flags[0] == 2  # opaque meshes, one sample: trace_rays runs the single-sample kFeatMesh path, the new kernel the light loop
    hits = nr.closest_hits(sc, o, d)
    got = nr.shade_hits(sc, o, d, hits, keys=k)
    ref = nr.trace_rays(sc, o, d, keys=k)
    hit = (hits.flags & 1) != 0
    plain = np.asarray([n.refl_mix == 0.0 and n.alpha == 1.0 and getattr(n.material, "alpha", None) is None for n in sc._nodes])
    on = hit & plain[np.maximum(hits.node, 0)]
    if name == "quads":
        assert plain.tolist() == [True, False] and 500 < on.sum() and (hit & ~on).sum() > 200
    else:
        assert plain.all() and on.sum() > 1000 and (~hit).sum() > 100
    print("%s: %d points compared, %d differ" % (name, int(on.sum()), int((got[on, :3] != ref[on]).any(axis=1).sum())))
    assert got.dtype == np.float32 and got.shape == (len(o), 4)
    assert same_values(got[on, :3], ref[on])
    assert (got[on, 3] == 1.0).all()
    assert (bits(got[~hit]) == 0).all()
    assert np.unique(got[on, :3], axis=0).shape[0] > 50  # (not one flat colour)
    if name == "analytic":
        assert set(hits.node[hit]) == set(range(len(sc._nodes)))  # every shape kind and material kind is lit


# ---- 2: against the oracle everywhere ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SCENES))
def test_every_point_against_the_oracle(gpu, shim, name):
    c = case(name)
    got = c["shaded"]
    ref = shim_shade(shim, c["full"], keys=c["k"], **c["args"])
    err = np.abs(got - ref).max(axis=0)
    print("%s: max |hip - oracle| per channel %s over %d points" % (name, err, len(got)))
    assert float(err.max()) <= TOL
    hit = (c["hits"].flags & 1) != 0
    assert hit.sum() > 1000 and (bits(got[~hit]) == 0).all() and (ref[~hit] == 0.0).all()
    if name == "quads":
        lace = hit & (c["hits"].node == 1)
        assert lace.sum() > 200 and np.array_equal(bits(got[lace, 3]), bits(ref[lace, 3]))
        assert set(np.unique(got[lace, 3])) == {0.0, 0.5, 1.0}
        floor = hit & (c["hits"].node == 0)
        lit = np.unique(np.round(ref[floor, :3] / np.maximum(ref[floor, :3].max(axis=1, keepdims=True), 1e-6), 2), axis=0)
        assert len(lit) > 20  # (texture colours, full shadow and filtered light)
    if name == "analytic":
        assert any(n.refl_mix != 0.0 for n in c["full"]._nodes) and any(n.alpha != 1.0 for n in c["full"]._nodes)  # the scene as it is


# ---- 3: a non-finite scene ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["light", "texel"])
def test_non_finite_scene(gpu, shim, kind):
    """One light colour is +inf, or one colour texel (DScene::no_elide: the kernel that skips nothing): NaN and inf where the oracle puts them.  The light
    alone makes infinities (every lit point), the texel under a light behind the surface also inf * 0."""
    from tests.test_elision_gpu import _nonfinite_scene
    sc, cam = _nonfinite_scene(kind)
    o, d, k = _camera(cam, 104, 60, 0)
    hits = nr.closest_hits(sc, o, d)
    got = nr.shade_hits(sc, o, d, hits, keys=k)
    ref = shim_shade(shim, sc, keys=k, **hit_arrays(o, d, hits))
    assert np.isinf(ref).any() and (kind == "light" or np.isnan(ref).any())  # the case really produces non-finite colours
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref))
    assert np.array_equal(got[np.isinf(ref)], ref[np.isinf(ref)])
    fin = np.isfinite(ref)
    assert float(np.abs(got[fin] - ref[fin]).max()) <= TOL


# ---- 4: skipped points --------------------------------------------------------------------------------------------------------------------------------
def _pick(c, n, node=None):
    """The arguments of the first n hits of a case (on `node` when given), with their keys."""
    m = (c["hits"].flags & 1) != 0
    if node is not None:
        m &= c["hits"].node == node
    sel = np.flatnonzero(m)[:n]
    assert len(sel) == n
    return {k: np.ascontiguousarray(v[sel]) for k, v in c["args"].items()}, np.ascontiguousarray(c["k"][sel])


@pytest.mark.parametrize("form", ["host", "device"])
def test_skipped_points_are_zero_and_leave_their_neighbours_alone(gpu, form):
    c = case("analytic")
    sc = c["full"]
    shade = (lambda a, k: nr.shade_points(sc, keys=k, **a)) if form == "host" else (lambda a, k: device_shade(sc, a, keys=k))
    a, k = _pick(c, 130)
    base = shade(a, k)
    assert (base[:, 3] == 1.0).all() and (base[:, :3] > 0.0).any(axis=1).all()
    lanes = [0, 31, 63, 64]
    keep = np.setdiff1d(np.arange(130), lanes)
    without = shade({name: v[keep] for name, v in a.items()}, k[keep])
    assert np.array_equal(bits(without), bits(base[keep]))
    for turn in range(4):  # every kind of skip on every one of the lanes
        b = {name: v.copy() for name, v in a.items()}
        for j, lane in enumerate(lanes):
            kind = (j + turn) % 4
            if kind == 3:
                b["hit_flags"][lane] &= ~np.uint32(1)
            else:
                b["nodes"][lane] = (-1, len(sc._nodes), 2**31 - 1)[kind]
        got = shade(b, k)
        assert (bits(got[lanes]) == 0).all(), turn
        assert np.array_equal(bits(got[keep]), bits(base[keep])), turn


def test_no_flags_and_no_uvs_shade_without_the_texture(gpu, shim):
    """hit_flags = None with uvs = None: a textured node is lit with tex = 1, the oracle's answer for has_uv = 0 — and bit 1 clear says the same."""
    c = case("quads")
    sc = c["full"]
    a, k = _pick(c, 300, node=0)
    textured = nr.shade_points(sc, keys=k, **a)
    bare = dict(a, uvs=None, hit_flags=None)
    got = nr.shade_points(sc, keys=k, **bare)
    ref = shim_shade(shim, sc, keys=k, **bare)
    assert float(np.abs(got - ref).max()) <= TOL
    assert float(np.abs(got - textured).max()) > 0.05  # (the texture matters on this node)
    assert np.array_equal(bits(got), bits(nr.shade_points(sc, keys=k, **dict(a, hit_flags=a["hit_flags"] & ~np.uint32(2)))))
    assert np.array_equal(bits(got), bits(nr.shade_points(sc, keys=k, **dict(a, uvs=None))))  # bit 1 without uvs: no uv either
    assert np.array_equal(bits(textured), bits(nr.shade_points(sc, keys=k, **dict(a, hit_flags=None))))  # NULL flags with uvs: every point has its uv
    assert np.array_equal(bits(textured), bits(sc.shade_points(keys=k, **a)))  # Scene.shade_points


# ---- 5: sizes and paths ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, (1 << 22) + 17])
def test_sizes_device_path_pieces_and_default_keys(gpu, n):
    """The 4 096 points of the analytic case (area light: the keys matter), tiled to n.  Default keys: point i has key i, also across the chunk seam at 2^22."""
    import torch
    c = case("analytic")
    sc = c["full"]
    reps = -(-n // 4096)
    a = {name: np.ascontiguousarray(np.tile(v, (reps,) + (1,) * (v.ndim - 1))[:n]) for name, v in c["args"].items()}
    host = nr.shade_points(sc, **a)
    assert host.shape == (n, 4)
    dev = device_shade(sc, a, stream=torch.cuda.Stream())
    assert np.array_equal(bits(dev), bits(host))
    if n <= 64:
        assert np.array_equal(bits(device_shade(sc, a, keys=np.arange(n, dtype=np.uint64))), bits(host))
    else:  # (pieces under explicit keys against one call under the default keys)
        cuts = [0, n // 3, n // 3 + 1, n - 5, n]
        parts = [device_shade(sc, {name: v[p:q] for name, v in a.items()}, keys=np.arange(p, q, dtype=np.uint64)) for p, q in zip(cuts[:-1], cuts[1:])]
        assert np.array_equal(bits(np.concatenate(parts)), bits(host))
    if n > 4096:  # the same point under another key: the area light's samples move
        lit = (a["hit_flags"][:4096] & 1) != 0
        assert (bits(host[:4096][lit]) != bits(host[4096:8192][lit])).any()
        assert np.array_equal(bits(host[-17:]), bits(device_shade(sc, {name: v[-17:] for name, v in a.items()}, keys=np.arange(n - 17, n, dtype=np.uint64))))


def test_shade_hits_on_tensors_equals_the_host_form(gpu):
    import torch
    c = case("quads")
    sc = c["full"]
    to, td = torch.from_numpy(c["o"]).cuda(), torch.from_numpy(c["d"]).cuda()
    tk = torch.from_numpy(c["k"].view(np.int64)).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = nr.shade_hits(sc, to, td, nr.closest_hits(sc, to, td), keys=tk)
    s.synchronize()
    assert np.array_equal(bits(got.cpu().numpy()), bits(c["shaded"]))
    with pytest.raises(ValueError):
        nr.shade_hits(sc, to, td, c["hits"])  # tensors and arrays mixed


# ---- statuses -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "device"])
def test_statuses(gpu, form):
    import torch
    sc = case("analytic")["full"]
    lib = abi.load_hip_lib()
    a, k = _pick(case("analytic"), 16)
    a["hit_flags"] = a["hit_flags"].astype(np.uint32)
    arrays = dict(a, keys=k, out=np.full((16, 4), 7.0, np.float32))
    order = ("points", "normals", "view_dirs", "uvs", "nodes", "hit_flags", "keys", "out")
    if form == "device":
        held = {name: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v.view(np.int32) if v.dtype == np.uint32 else v).cuda() for name, v in arrays.items()}
        ptrs = {name: t.data_ptr() for name, t in held.items()}
    else:
        ct = {np.dtype(np.float64): C.c_double, np.dtype(np.int32): C.c_int32, np.dtype(np.uint32): C.c_uint32, np.dtype(np.uint64): C.c_uint64, np.dtype(np.float32): C.c_float}
        ptrs = {name: v.ctypes.data_as(C.POINTER(ct[v.dtype])) for name, v in arrays.items()}

    def call(n=16, flags=0, null=(), scene=True):
        p = [None if name in null else ptrs[name] for name in order]
        h = sc.device_handle() if scene else None
        if form == "device":
            rc = lib.nrays_shade_points_device(h, n, *p, flags, torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            return rc, held["out"].cpu().numpy()
        return lib.nrays_shade_points(h, n, *p, flags), arrays["out"]

    for flags in (1, 2, 1 << 31, 3):
        assert call(flags=flags)[0] == abi.ERR_BAD_ARG, flags
    for name in ("points", "normals", "view_dirs", "nodes", "out"):
        assert call(null=(name,))[0] == abi.ERR_BAD_ARG, name
    assert call(scene=False)[0] == abi.ERR_BAD_ARG
    rc, out = call(n=0)
    assert rc == abi.OK and (out == 7.0).all()  # without work; nothing so far wrote the output
    rc, out = call(null=("uvs", "hit_flags", "keys"))
    assert rc == abi.OK and np.array_equal(bits(out), bits(nr.shade_points(sc, **dict(a, uvs=None, hit_flags=None))))
    rc, out = call()
    assert rc == abi.OK and np.array_equal(bits(out), bits(nr.shade_points(sc, keys=k, **a)))


# ---- 6: the handle's state --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["analytic", "quads"])
def test_a_batch_leaves_the_render_state_alone(gpu, name):
    import torch
    c = case(name)
    sc, cam = SCENES_CAMERAS[name]()
    w, h = 128, 72
    proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], w, h)
    first = nr.render(sc, (w, h), 1, 0.0, cam["eye"], proj)
    st1, perm1 = nr.get_stats(sc), nr.last_permutation(sc)
    got = device_shade(sc, c["args"], keys=c["k"], stream=torch.cuda.Stream())
    assert np.array_equal(bits(got), bits(c["shaded"]))  # (a fresh handle of the same scene, after a render, on another stream)
    assert nr.last_permutation(sc) == perm1
    second = nr.render(sc, (w, h), 1, 0.0, cam["eye"], proj)
    st2 = nr.get_stats(sc)
    assert np.array_equal(first.view(np.uint32), second.view(np.uint32))
    assert nr.last_permutation(sc) == perm1
    for f in STAT_FIELDS:
        assert getattr(st1, f) == getattr(st2, f), f


SCENES_CAMERAS = {"analytic": rich_analytic_scene, "quads": quad_scene}
