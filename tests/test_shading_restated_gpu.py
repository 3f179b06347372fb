"""The HIP shading and bounce code against the independent restatement of the reference (tests/shading_cases.py), inside the bound derived there:
nr.shade_points and nr.intersects_rays on sets A and B, nr.trace_rays on the probes, the slab and the lit mirror, nr.render on two small frames —
each by the default kernels and by the kernel that skips nothing (NRAYS_ELIDE=0, set before the scene is created), in the numpy (host-buffer)
and the torch (device, current stream) forms.  Nothing here reads the oracle."""
import functools

import numpy as np
import pytest

import nrays_amd as nr
from tests import shading_cases as sc
from tests.shading_cases import TRACE_CASES, report, shade_args

pytestmark = pytest.mark.gpu

ELIDE = pytest.mark.parametrize("elide", [None, "0"], ids=["default", "elide0"])
FORM = pytest.mark.parametrize("form", ["numpy", "torch"])


def _scene(world, elide, monkeypatch):
    if elide is not None:
        monkeypatch.setenv("NRAYS_ELIDE", elide)   # read when the handle is created
    scene = sc.build_scene(world)
    scene.device_handle()
    return scene


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def _call(fn, scene, form, **kw):
    """fn(scene, **kw) on numpy arrays, or on device tensors (the result copied back)."""
    if form == "numpy":
        return fn(scene, **kw)
    import torch
    out = fn(scene, **{k: (_dev(v) if isinstance(v, np.ndarray) else v) for k, v in kw.items()})
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy() for x in out) if isinstance(out, tuple) else out.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _expected_points(light_set):
    world = sc.world_b() if light_set == "filters" else sc.world_a(light_set)
    c = sc.points_set(light_set)
    return (world, c) + sc.expected_points(world, c)[:3]


@functools.lru_cache(maxsize=None)
def _expected_shadow_rays():
    world, c = _expected_points("filters")[:2]
    return sc.shadow_rays_set(world, c)


@functools.lru_cache(maxsize=None)
def _expected_trace(name):
    world, rays = TRACE_CASES[name]()
    return (world, rays) + sc.trace(world, *rays)


@ELIDE
@FORM
@pytest.mark.parametrize("light_set", ["one", "three", "area", "filters"])
def test_shade_points_is_the_restated_compute(gpu, monkeypatch, light_set, elide, form):
    world, c, want, err, keep = _expected_points(light_set)
    got = _call(nr.shade_points, _scene(world, elide, monkeypatch), form, **shade_args(c))
    assert got.dtype == np.float32 and got.shape == (len(c["points"]), 4)
    assert np.array_equal(got[:, 3].astype(np.float64), want[:, 3])
    assert report("%s %s %s" % (light_set, elide, form), sc.worst_ratio(got[:, :3], want[:, :3], err[:, :3], keep)) <= 1.0


@ELIDE
@FORM
def test_intersects_rays_is_the_restated_filter(gpu, monkeypatch, elide, form):
    world = _expected_points("filters")[0]
    o, d, mt, lit, filt, ferr, keep = _expected_shadow_rays()
    glit, gfilt = _call(nr.intersects_rays, _scene(world, elide, monkeypatch), form, origins=o, dirs=d, max_toi=mt)
    assert np.array_equal(glit[keep], lit[keep])
    assert report("filter %s %s" % (elide, form), sc.worst_ratio(gfilt, filt, ferr, keep)) <= 1.0


@ELIDE
@FORM
@pytest.mark.parametrize("name", ["probe", "quad_probe", "slab", "mirror"])
def test_trace_rays_is_the_restated_trace(gpu, monkeypatch, name, elide, form):
    world, (o, d, r, e, k), want, err = _expected_trace(name)
    got = _call(nr.trace_rays, _scene(world, elide, monkeypatch), form, origins=o, dirs=d, refr=r, energy=e, keys=k)
    assert got.dtype == np.float32 and got.shape == (len(o), 3)
    assert report("%s %s %s" % (name, elide, form), sc.worst_ratio(got, want, err)) <= 1.0


@ELIDE
@pytest.mark.parametrize("quad", [False, True], ids=["plane", "quad"])
def test_render_is_the_restated_trace_of_the_camera_rays(gpu, monkeypatch, quad, elide):
    world = sc.frame_world(quad)
    want, err = sc.expected_frame(world)
    proj = sc.frame_rays()[3]
    got = nr.render(_scene(world, elide, monkeypatch), sc.FRAME["resolution"], 1, 0.0, sc.FRAME["eye"], proj, seed=sc.FRAME["seed"])
    assert got.shape == want.shape
    assert report("frame %s %s" % (quad, elide), sc.worst_ratio(got, want, err)) <= 1.0
