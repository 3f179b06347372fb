"""Batched Scene::trace / Scene::intersects_ray on caller-supplied rays on the GPU (nrays_trace_rays*, nrays_intersects_rays_device): camera rays
against the oracle's frame and the library's own render, arbitrary rays against the oracle's scene_trace (tests/trace_oracle_shim.c), the device
path, chunking, the handle's render state, the shadow query and scenes with non-finite inputs."""
import ctypes as C

import numpy as np
import pytest

import nrays_amd as nr
import oracle
from nrays_amd import abi, math3d
from tests.test_trace_rays import analytic_scene, average_samples, build_shim, shim_trace
from tools import scenes_util as su
from tools import standins

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(tmp_path_factory.mktemp("trace_shim_gpu"))


def _glass_scene():
    """test_parity_gpu's double-branching scene (reflection AND refraction at one hit: the continuation queue)."""
    glass = nr.PhongMaterial((0.1, 0.1, 0.15), (0.6, 0.7, 0.9), (1, 1, 1), None, None, 80.0)
    iso = nr.Isometry3
    nodes = [nr.SceneNode(glass, 0.3, 0.4, 0.5, 1.3, iso((-1.2, 0, 0)), nr.Ball(1.0)),
             nr.SceneNode(glass, 0.3, 0.4, 0.5, 1.3, iso((1.2, 0, 0.5)), nr.Cuboid((0.7, 0.7, 0.7))),
             nr.SceneNode(su.default_material(), 0.25, 0.5, 1.0, 1.0, iso((0, -1.2, 0)), nr.Plane((0, 1, 0))),
             nr.SceneNode(nr.NormalMaterial(), 0.0, 0.0, 1.0, 1.0, iso((0, 0.3, 3.0)), nr.Ball(0.8))]
    return nr.Scene(nodes, [nr.Light((2.0, 6.0, -4.0), 0.0, 1, (1, 1, 1))]), dict(eye=(0.0, 2.0, -7.0), at=(0.0, 0.0, 0.0), fovy=45.0)


def _scene_flags(sc):
    out = (C.c_uint32 * 2)()
    abi.check(abi.load_hip_lib().nrays_debug_scene_flags(sc.device_handle(), out))
    return out[0]


CAMERA_CASES = {
    "balls": (lambda: su.balls_scene(), 96, 64, 1, 0.0),
    "primitives_area_light": (lambda: su.primitives_scene(light_radius=0.1, nsample=3), 80, 60, 2, 0.5),
    "double_branching": (_glass_scene, 96, 72, 1, 0.0),
    "sponza_standin": (lambda: standins.sponza_scene(), 96, 54, 1, 0.0),
    "hair_standin_mesh_kernel": (lambda: standins.hairball_scene(strands=400), 96, 96, 1, 0.0),
}


@pytest.mark.parametrize("case", sorted(CAMERA_CASES))
def test_camera_rays_round_trip(gpu, case):
    make, w, h, spp, window = CAMERA_CASES[case]
    sc, cam = make()
    if case.startswith("hair"):
        assert _scene_flags(sc) == 2  # opaque meshes, one light: the kFeatMesh kernel traces this batch
    proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], w, h)
    p = nr.make_params((w, h), spp, window, cam["eye"], proj, seed=3)
    ref, _ = oracle.render(sc.descriptor, p, num_threads=16)
    frame = nr.render(sc, (w, h), spp, window, cam["eye"], proj, seed=3)
    o, d, k = nr.camera_rays((w, h), cam["eye"], proj, ray_per_pixel=spp, window_width=window, seed=3)
    img = average_samples(nr.trace_rays(sc, o, d, keys=k), w, h, spp)
    assert float(np.abs(img - ref).max()) <= TOL
    assert float(np.abs(img - frame).max()) <= TOL


def _arbitrary_rays(rng, n):
    """Rays from inside the refractive ball of analytic_scene() (refr = its coefficient), from outside in every direction, and rays that miss."""
    dirs = rng.normal(size=(n, 3))
    dirs /= np.sqrt((dirs * dirs).sum(axis=1))[:, None]
    origins = rng.uniform(-4.0, 4.0, size=(n, 3))
    origins[:, 1] = rng.uniform(-1.0, 4.0, size=n)
    refr = np.ones(n)
    inside = np.arange(n) % 4 == 0
    v = rng.normal(size=(inside.sum(), 3))
    v *= (0.6 * rng.uniform(0.0, 1.0, size=(len(v), 1))) / np.sqrt((v * v).sum(axis=1))[:, None]
    origins[inside] = np.asarray([-1.2, 0.0, 0.0]) + v
    refr[inside] = 1.3
    miss = np.arange(n) % 4 == 1
    origins[miss] = rng.uniform(-3.0, 3.0, size=(miss.sum(), 3)) + np.asarray([0.0, 20.0, 0.0])
    dirs[miss] = np.asarray([0.0, 1.0, 0.0])
    energy = rng.uniform(0.0, 1.0, size=n).astype(np.float32)
    energy[::5] = rng.uniform(0.0, 0.1, size=len(energy[::5])).astype(np.float32)  # reflections cut (scene.rs:204)
    keys = rng.integers(0, 2**63, size=n, dtype=np.int64).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    return origins, dirs, refr, energy, keys, miss


@pytest.mark.parametrize("max_depth", [0, 1, 3])
def test_arbitrary_rays_against_the_oracle(gpu, shim, max_depth):
    bg = (0.25, 0.5, 0.75)
    sc, _ = analytic_scene(background=bg)
    o, d, r, e, k, miss = _arbitrary_rays(np.random.default_rng(11 + max_depth), 4096)
    got = nr.trace_rays(sc, o, d, refr=r, energy=e, keys=k, max_depth=max_depth)
    ref = shim_trace(shim, sc, o, d, refr=r, energy=e, keys=k, max_depth=max_depth)
    assert float(np.abs(got - ref).max()) <= TOL
    assert np.array_equal(got[miss], np.tile(np.asarray(bg, np.float32), (miss.sum(), 1)))
    assert np.abs(got[~miss] - np.asarray(bg, np.float32)).max() > 0.1  # (the others hit something)
    # the defaults: refr 1, energy 1, key i
    n = 512
    assert np.array_equal(nr.trace_rays(sc, o[:n], d[:n], max_depth=max_depth),
                          nr.trace_rays(sc, o[:n], d[:n], refr=np.ones(n), energy=np.ones(n, np.float32), keys=np.arange(n, dtype=np.uint64), max_depth=max_depth))


def _small_rays(n, seed=5):
    rng = np.random.default_rng(seed)
    o = np.tile(np.asarray([0.0, 2.0, -7.0]), (n, 1)) + rng.uniform(-0.5, 0.5, size=(n, 3))
    t = rng.uniform(-1.5, 1.5, size=(n, 3)) - o
    d = t / np.sqrt((t * t).sum(axis=1))[:, None]
    return o, d


@pytest.mark.parametrize("n", [1, 63, 64, 65, (1 << 22) + 17])
def test_device_path_equals_host_path(gpu, n):
    """torch tensors on a non-default stream: the host path's colours bit for bit; one call equals calls over pieces (chunks of 2^22 inside)."""
    import torch
    sc, _ = _glass_scene()
    sc = nr.Scene(sc._nodes, [nr.Light((2.0, 6.0, -4.0), 0.3, 2, (1, 1, 1))])  # area light: the keys matter
    o, d = _small_rays(n)
    host = nr.trace_rays(sc, o, d)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        dev = nr.trace_rays(sc, torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda())
        dev = dev.cpu().numpy()
    s.synchronize()
    assert np.array_equal(dev, host)
    if n > 64:
        cuts = [0, n // 3, n // 3 + 1, n - 5, n]
        parts = [nr.trace_rays(sc, o[a:b], d[a:b], keys=np.arange(a, b, dtype=np.uint64)) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
        assert np.array_equal(np.concatenate(parts), host)


def test_null_device_arguments(gpu):
    import torch
    sc, _ = _glass_scene()
    lib = abi.load_hip_lib()
    buf = torch.zeros(64, dtype=torch.float64, device="cuda")
    out = torch.zeros(64, dtype=torch.float32, device="cuda")
    h, p, q = sc.device_handle(), buf.data_ptr(), out.data_ptr()
    assert lib.nrays_trace_rays_device(h, 1, None, p, None, None, None, 0, q, None) == abi.ERR_BAD_ARG
    assert lib.nrays_trace_rays_device(h, 1, p, None, None, None, None, 0, q, None) == abi.ERR_BAD_ARG
    assert lib.nrays_trace_rays_device(h, 1, p, p, None, None, None, 0, None, None) == abi.ERR_BAD_ARG
    assert lib.nrays_intersects_rays_device(h, 1, p, p, None, q, q, None) == abi.ERR_BAD_ARG
    assert lib.nrays_intersects_rays_device(h, 1, p, p, p, None, q, None) == abi.ERR_BAD_ARG
    assert lib.nrays_trace_rays_device(h, 0, p, p, None, None, None, 0, q, None) == abi.OK


STAT_FIELDS = ("rays_primary", "rays_reflection", "rays_refraction", "rays_shadow", "rays_shadow_elided", "generations", "rays_primary_traced")


@pytest.mark.parametrize("make", [_glass_scene, lambda: standins.sponza_scene()], ids=["double_branching", "sponza_standin"])
def test_a_batch_leaves_the_render_state_alone(gpu, make):
    sc, cam = make()
    w, h = 128, 72
    proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], w, h)
    first = nr.render(sc, (w, h), 1, 0.0, cam["eye"], proj)
    st1 = nr.get_stats(sc)
    o, d = _small_rays(20000)
    nr.trace_rays(sc, o, d, max_depth=2)
    nr.intersects_rays(sc, o, d, np.full(len(o), 5.0))
    second = nr.render(sc, (w, h), 1, 0.0, cam["eye"], proj)
    st2 = nr.get_stats(sc)
    assert np.array_equal(first, second)
    for f in STAT_FIELDS:
        assert getattr(st1, f) == getattr(st2, f), f


def test_shadow_query_equals_the_probe_and_the_oracle(gpu):
    sc, _ = su.primitives_scene(light_radius=0.1, nsample=3)  # transparent box / cone / cylinder: colour filters
    rng = np.random.default_rng(2)
    n = 5000
    o = rng.uniform(-6.0, 6.0, size=(n, 3))
    t = rng.uniform(-2.5, 2.5, size=(n, 3)) - o
    d = t / np.sqrt((t * t).sum(axis=1))[:, None]
    max_toi = rng.uniform(0.5, 15.0, size=n)
    lit, filt = nr.intersects_rays(sc, o, d, max_toi)
    blocked, pfilt = nr.shadow_rays(sc, o, d, max_toi)
    assert np.array_equal(lit, ~blocked)
    assert 0 < lit.sum() < n
    assert np.array_equal(filt[lit], pfilt[lit].astype(np.float32))
    assert np.all(filt[~lit] == 0.0)
    assert (filt[lit] < 1.0).any()  # some lit rays cross a transparent node
    for i in range(0, n, 50):
        ref = oracle.shadow(sc.descriptor, o[i], d[i], max_toi[i])
        assert (ref is not None) == bool(lit[i]), i
        if ref is not None:
            assert float(np.abs(filt[i] - ref).max()) <= 1e-6, i


@pytest.mark.parametrize("kind", ["light", "shininess"])
def test_non_finite_scene(gpu, shim, kind):
    """A scene with a non-finite light / a negative shininess (as in test_elision_gpu): nothing may be skipped, NaN / inf appear where the
    oracle's scene_trace puts them."""
    from tests.test_elision_gpu import _nonfinite_scene
    sc, cam = _nonfinite_scene(kind)
    w, h = 104, 60
    proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], w, h)
    o, d, k = nr.camera_rays((w, h), cam["eye"], proj)
    got = nr.trace_rays(sc, o, d, keys=k)
    ref = shim_trace(shim, sc, o, d, keys=k)
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref))
    if kind == "light":
        assert (~np.isfinite(ref)).any()  # the case really produces non-finite colours
    fin = np.isfinite(ref)
    assert np.array_equal(got[np.isinf(ref)], ref[np.isinf(ref)])
    assert float(np.abs(got[fin] - ref[fin]).max()) <= TOL
