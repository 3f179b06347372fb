"""Stackless closest-hit and shadow queries of tiny analytic scenes (kFeatTinyScene, trace_device.h: tiny_closest / tiny_shadow) against the
TLAS walk they replace (NRAYS_TINY_SCENE=0, read once per scene handle): frames, ray-class counters and caller-supplied rays must be
bit-identical — balls at every depth, exact ties between leaves (coincident and touching balls), rays along AABB faces and edges
(knife-edge gates), planes, the other shapes, several lights."""
import math
import os

import numpy as np
import pytest

import nrays_amd as nr
from nrays_amd import math3d
from tests.permutation_cases import TINY
from tools import scenes_util as su

pytestmark = pytest.mark.gpu

STAT_FIELDS = ("rays_primary", "rays_reflection", "rays_refraction", "rays_shadow", "rays_shadow_elided", "rays_primary_traced", "generations")


def _both(make, w, h, cam, max_depth=0, frames=2):
    """The same scene rendered by a handle with the stackless queries and by one without: (frame, stats) of each."""
    out = []
    old = os.environ.get("NRAYS_TINY_SCENE")
    try:
        for flag in ("1", "0"):
            os.environ["NRAYS_TINY_SCENE"] = flag
            sc = make()
            proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], w, h)
            for _ in range(frames):  # the second frame runs with the first one's tile costs (cost-ordered lists)
                img = nr.render(sc, (w, h), 1, 0.0, cam["eye"], proj, max_depth=max_depth)
            st = nr.get_stats(sc)
            out.append((img, {k: getattr(st, k) for k in STAT_FIELDS}))
            sc._release()
    finally:
        if old is None:
            os.environ.pop("NRAYS_TINY_SCENE", None)
        else:
            os.environ["NRAYS_TINY_SCENE"] = old
    return out


def _assert_same(make, w, h, cam, max_depth=0):
    (a, sa), (b, sb) = _both(make, w, h, cam, max_depth)
    assert a.shape == b.shape
    diff = a.view(np.uint32) != b.view(np.uint32)
    assert not diff.any(), "%d pixel components differ" % int(diff.sum())
    assert sa == sb


def _balls():
    return su.balls_scene(tex_size=(256, 128))[0]


BALLS_CAMERAS = {
    "balls": dict(eye=(0.0, 5.0, -10.0), at=(0.0, 0.0, 0.0), fovy=45.0),
    "balls_zoom": dict(eye=(0.0, 0.6, -6.0), at=(1.05, 0.0, 0.0), fovy=6.0),  # deep reflection chains between the balls
    "balls_side": dict(eye=(-12.0, 0.0, 0.0), at=(0.0, 0.0, 0.0), fovy=30.0),  # the balls one behind the other, rays in the plane y = 0
}


@pytest.mark.parametrize("max_depth", [0, 1, 2, 4])
@pytest.mark.parametrize("camera", sorted(BALLS_CAMERAS))
def test_balls_bit_identical(gpu, camera, max_depth):
    _assert_same(_balls, 160, 96, BALLS_CAMERAS[camera], max_depth)


def _ties():
    """Two coincident balls (every hit on them is an exact tie of toi: the smaller node id wins) and two touching balls (rays at the
    tangent point hit both at the same distance), reflective, with a plane below."""
    iso = nr.Isometry3
    mats = [nr.NormalMaterial(), nr.UVMaterial(), su.default_material()]
    nodes = [nr.SceneNode(mats[1], 0.3, 0.25, 1.0, 1.0, iso((0.0, 0.0, 0.0)), nr.Ball(1.0)),
             nr.SceneNode(mats[0], 0.3, 0.25, 1.0, 1.0, iso((0.0, 0.0, 0.0)), nr.Ball(1.0)),
             nr.SceneNode(mats[2], 0.2, 0.25, 1.0, 1.0, iso((2.0, 0.0, 0.0)), nr.Ball(1.0)),
             nr.SceneNode(mats[0], 0.2, 0.25, 1.0, 1.0, iso((4.0, 0.0, 0.0)), nr.Ball(1.0)),
             nr.SceneNode(mats[2], 0.2, 0.5, 1.0, 1.0, iso((0.0, -1.0, 0.0)), nr.Plane((0.0, 1.0, 0.0)))]
    return nr.Scene(nodes, [nr.Light((1.0, 8.0, -3.0), 0.0, 1, (1, 1, 1))], (0.2, 0.3, 0.4))


TIE_CAMERAS = {
    "front": dict(eye=(2.0, 1.0, -9.0), at=(2.0, 0.0, 0.0), fovy=40.0),
    "tangent": dict(eye=(1.0, 0.0, -8.0), at=(1.0, 0.0, 0.0), fovy=3.0),  # centre column: rays through the touching point (1, 0, 0)
    "edges": dict(eye=(1.0, 1.0, -8.0), at=(1.0, 1.0, 0.0), fovy=2.0),  # rays along the shared AABB edge x = 1, y = 1
    "grazing": dict(eye=(-8.0, 1.0, 0.0), at=(0.0, 1.0, 0.0), fovy=4.0),  # the AABB tops y = 1 seen edge-on
}


@pytest.mark.parametrize("camera", sorted(TIE_CAMERAS))
def test_ties_and_knife_edges_bit_identical(gpu, camera):
    _assert_same(_ties, 128, 96, TIE_CAMERAS[camera])


def _random_tiny(seed):
    """Up to 8 leaves (planes count): balls, cuboids, cylinders, capsules, cones, rotated or not, opaque, one or two lights."""
    rng = np.random.default_rng(seed)
    mats = [su.default_material(), nr.NormalMaterial(), nr.UVMaterial()]
    kinds = [lambda: nr.Ball(rng.uniform(0.4, 1.2)), lambda: nr.Cuboid(rng.uniform(0.3, 1.0, 3)),
             lambda: nr.Cylinder(rng.uniform(0.3, 1.0), rng.uniform(0.3, 0.9)), lambda: nr.Capsule(rng.uniform(0.3, 1.0), rng.uniform(0.2, 0.6)),
             lambda: nr.Cone(rng.uniform(0.4, 1.0), rng.uniform(0.3, 0.9))]
    n = int(rng.integers(2, 8))
    nodes = []
    for k in range(n):
        g = kinds[0]() if (seed % 2 == 0 or k < 2) else kinds[int(rng.integers(0, 5))]()
        pos = np.round(rng.uniform(-3.0, 3.0, 3) * 4.0) / 4.0  # quarter-unit grid: touching and aligned boxes occur
        ang = rng.uniform(-math.pi, math.pi, 3) * (rng.random() < 0.5)
        nodes.append(nr.SceneNode(mats[k % 3], float(rng.choice([0.0, 0.3])), 0.25, 1.0, 1.0, nr.Isometry3(pos, ang), g))
    if rng.random() < 0.5:
        nodes.append(nr.SceneNode(mats[0], 0.2, 0.5, 1.0, 1.0, nr.Isometry3((0.0, -3.5, 0.0)), nr.Plane((0.0, 1.0, 0.1))))
    lights = [nr.Light((0.0, 10.0, -2.0), 0.0, 1, (1, 1, 1))]
    if seed % 3 == 0:
        lights.append(nr.Light((-6.0, 4.0, -6.0), 0.0, 1, (0.5, 0.4, 0.3)))
    return nr.Scene(nodes, lights, (0.1, 0.1, 0.1))


@pytest.mark.parametrize("seed", range(8))
def test_random_tiny_scenes_bit_identical(gpu, seed):
    cam = dict(eye=(0.0, 3.0, -12.0), at=(0.0, 0.0, 0.0), fovy=50.0)
    _assert_same(lambda: _random_tiny(seed), 128, 96, cam)


def test_caller_supplied_rays_identical(gpu):
    rng = np.random.default_rng(5)
    n = 4096
    o = rng.uniform(-4.0, 4.0, size=(n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.sqrt((d * d).sum(axis=1))[:, None]
    t = rng.uniform(0.5, 12.0, size=n)
    res = []
    old = os.environ.get("NRAYS_TINY_SCENE")
    try:
        for flag in ("1", "0"):
            os.environ["NRAYS_TINY_SCENE"] = flag
            sc = _ties()
            col = nr.trace_rays(sc, o, d)
            lit, filt = nr.intersects_rays(sc, o, d, t)
            res.append((col, lit, filt))
            sc._release()
    finally:
        if old is None:
            os.environ.pop("NRAYS_TINY_SCENE", None)
        else:
            os.environ["NRAYS_TINY_SCENE"] = old
    (c1, l1, f1), (c0, l0, f0) = res
    assert np.array_equal(c1.view(np.uint32), c0.view(np.uint32))
    assert np.array_equal(l1, l0) and np.array_equal(f1.view(np.uint32), f0.view(np.uint32))


def test_switches_are_read_when_the_handle_is_created(gpu, monkeypatch):
    """A switch holds for a handle as nrays_scene_create found it, whatever the environment says afterwards: handle A is created with
    NRAYS_TINY_SCENE=0 and rendered after the variable is gone, handle B is created without it.  A never launches a kFeatTinyScene
    permutation, B always does, and all four frames are bit-identical (the smallest frame that runs such a permutation: 64 x 64, 1 spp)."""
    def three_balls():
        mat = su.default_material()
        nodes = [nr.SceneNode(mat, 0.0, 0.25, 1.0, 1.0, nr.Isometry3((x, 0.0, 0.0)), nr.Ball(0.8)) for x in (-2.0, 0.0, 2.0)]
        return nr.Scene(nodes, [nr.Light((1.0, 8.0, -3.0), 0.0, 1, (1, 1, 1))], (0.2, 0.3, 0.4))

    monkeypatch.setenv("NRAYS_TINY_SCENE", "0")
    a = three_balls()
    a.device_handle()
    monkeypatch.delenv("NRAYS_TINY_SCENE")
    b = three_balls()
    b.device_handle()
    cam = dict(eye=(0.0, 2.0, -8.0), at=(0.0, 0.0, 0.0), fovy=45.0)
    proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], 64, 64)
    frames = []
    for _ in range(2):
        for sc, tiny in ((a, 0), (b, TINY)):
            frames.append(nr.render(sc, (64, 64), 1, 0.0, cam["eye"], proj))
            (_, feat, _, _), launches, _ = nr.last_permutation(sc)
            assert launches == 1 and feat & TINY == tiny, (feat, launches)
    a._release()
    b._release()
    for f in frames[1:]:
        assert np.array_equal(f.view(np.uint32), frames[0].view(np.uint32))
    assert len(np.unique(frames[0].reshape(-1, 3), axis=0)) > 8  # (the balls are in the frame)
