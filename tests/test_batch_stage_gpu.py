"""The staging arena of the blocking caller-batch calls is one buffer shared by every family (nrays_amd/csrc/batch_call.cpp, batch_stage.h): on one handle the
blocking forms run in an order in which the arena grows, is reused at a smaller size under another layout, and grows again.  Every result equals, bit for
bit, the device form of the same call on a second handle of the same scene (the device forms are pinned to the oracle by the families' own tests), and the
batches leave the handle's frame state alone."""
import math

import numpy as np
import pytest

import nrays_amd as nr
from nrays_amd import math3d
from tests.test_occlusion import quad_scene
from tests.test_occlusion_gpu import bits, hit_points

pytestmark = pytest.mark.gpu


def _scene():
    """The UV-mapped floor quad of quad_scene() and a half-transparent ball standing on it."""
    q, cam = quad_scene()
    glass = nr.PhongMaterial((0.1, 0.1, 0.15), (0.6, 0.7, 0.9), (1, 1, 1), None, None, 80.0)
    ball = nr.SceneNode(glass, 0.0, 0.0, 0.5, 1.0, nr.Isometry3((0.9, 0.45, 0.2)), nr.Ball(0.45))
    return nr.Scene([q._nodes[0], ball], q._lights, q._background), cam


def _t(a):
    """A numpy argument as the tensor the device forms take (flag words int32, keys int64)."""
    import torch
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    a = a.view(np.int32) if a.dtype == np.uint32 else a.view(np.int64) if a.dtype == np.uint64 else a
    return torch.from_numpy(a).cuda()


def _same(host, device, what):
    """Bit for bit, whatever the form returned: arrays, tensors, tuples of them, None."""
    if isinstance(host, tuple):
        assert len(host) == len(device), what
        for k, (h, d) in enumerate(zip(host, device)):
            _same(h, d, "%s[%d]" % (what, k))
        return
    assert (host is None) == (device is None), what
    if host is None:
        return
    d = device.cpu().numpy() if hasattr(device, "cpu") else device
    assert host.shape == d.shape and np.array_equal(bits(host), bits(d)), what


def test_the_blocking_forms_share_one_arena(gpu):
    a, cam = _scene()  # blocking forms, in the order below
    b, _ = _scene()    # device forms
    rng = np.random.default_rng(17)
    o, d, _ = nr.camera_rays((13, 5), cam["eye"], math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], 13, 5), seed=2)
    assert len(o) == 65

    # 1. cast, 65 rays, every output: the arena's first size
    hits = nr.closest_hits(a, o, d)
    _same(tuple(hits), tuple(nr.closest_hits(b, _t(o), _t(d))), "cast")
    assert 0 < np.count_nonzero(hits.flags & 1) and np.count_nonzero(hits.node == 0) and np.count_nonzero(hits.node == 1)
    points, normals = hit_points(o, d, hits)
    keys = rng.integers(0, 2**63, size=65, dtype=np.int64).astype(np.uint64) * np.uint64(2) + np.uint64(1)

    # 2. gather_maps, 65 points x 16 directions, one 4 x 4 map, counts wanted: tables, texels and an 8-byte output column
    L16 = nr.hemisphere_dirs(16)
    lightmap = rng.random((4, 4, 4), dtype=np.float32)
    want = nr.gather_maps_points(a, points, normals, L16, [lightmap], {0: 0}, miss=(0.25, 0.5, 0.75), hit_flags=hits.flags, keys=keys, want_counts=True)
    got = nr.gather_maps_points(b, _t(points), _t(normals), L16, [lightmap], {0: 0}, miss=(0.25, 0.5, 0.75), hit_flags=_t(hits.flags), keys=_t(keys), want_counts=True)
    _same(want, got, "gather_maps")
    assert want[1][:, 0].max() > 0  # (some rays reached the map)

    # 3. filter_texels, 64 x 8, 4 channels: larger, with 16-byte aligned value columns
    w, h = 64, 8
    cover = (rng.random(w * h) < 0.8).astype(np.uint32)
    tp, tn = rng.standard_normal((w * h, 3)), rng.standard_normal((w * h, 3))
    tn /= np.linalg.norm(tn, axis=1)[:, None]
    values = rng.random((w * h, 4), dtype=np.float32)
    _same(nr.filter_texels(a, cover, w, h, tp, tn, values, step=2, pos_radius=3.0, normal_cos=-0.5),
          nr.filter_texels(b, cover, w, h, tp, tn, values, step=2, pos_radius=3.0, normal_cos=-0.5, device="cuda"), "filter")

    # 4. trace_rays, 1 ray: the smallest layout in the large arena
    _same(nr.trace_rays(a, o[32:33], d[32:33], max_depth=2), nr.trace_rays(b, _t(o[32:33]), _t(d[32:33]), max_depth=2), "trace")

    # 5. occlusion, 5 points x 1024 directions x 1024 rotations: the tables are larger than the points
    sel = np.flatnonzero(hits.flags & 1)[:5]
    L1k, R1k = nr.hemisphere_dirs(1024), nr.rotation_table(1024)
    want = nr.occlusion_points(a, points[sel], normals[sel], L1k, R1k, keys=keys[sel])
    got = nr.occlusion_points(b, _t(points[sel]), _t(normals[sel]), L1k, R1k, keys=_t(keys[sel]))
    _same(tuple(want), tuple(got), "occlusion")
    assert 0 < want.open.min() and want.open.max() <= 1024

    # 6. dilate, 64 x 8, radius 2, values and source: an in / out column, flags in and out apart
    want = nr.dilate_texels(a, cover, w, h, 2, values=values.copy(), want_source=True)
    got = nr.dilate_texels(b, cover, w, h, 2, values=values.copy(), want_source=True, device="cuda")
    _same(want, got, "dilate")
    assert np.count_nonzero(want[2] != cover)  # (something was filled)

    # 7. shade, 65 points, with uvs and keys: the arena grows again
    sa = dict(points=points, normals=normals, view_dirs=d, nodes=hits.node, uvs=hits.uv, hit_flags=hits.flags)
    _same(nr.shade_points(a, keys=keys, **sa), nr.shade_points(b, keys=_t(keys), **{k: _t(v) for k, v in sa.items()}), "shade")

    # 8. cast again, only toi and node wanted: the first layout with absent columns
    again = nr.closest_hits(a, o, d, want=())
    _same(tuple(again), tuple(nr.closest_hits(b, _t(o), _t(d), want=())), "cast, toi and node only")
    _same((again.toi, again.node), (hits.toi, hits.node), "cast repeated")

    # the batches left the frame state of their handle alone
    fresh, _ = _scene()
    proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], 96, 54)
    _same(nr.render(a, (96, 54), 1, 0.0, cam["eye"], proj), nr.render(fresh, (96, 54), 1, 0.0, cam["eye"], proj), "render")


def test_the_probes_share_the_arena_with_the_blocking_forms(gpu):
    """nrays_debug_cast_batch (both modes) and nrays_debug_occlusion_rays run through the driver and the arena like the blocking forms: on one handle, between blocking
    cast and occlusion calls of other layouts and sizes — a single item, a wave less and more than one item, more than one workgroup; 1 and 16 directions — every
    probe result equals, bit for bit, the same probe called alone on a fresh handle."""
    a, cam = _scene()
    rng = np.random.default_rng(23)
    words = lambda pair: (pair[0].astype(np.uint32), pair[1])  # noqa: E731  (the probes' wrappers return a bool mask and float64 records)
    for w, h in ((1, 1), (9, 7), (13, 5), (257, 1)):
        n = w * h
        o, d, _ = nr.camera_rays((w, h), cam["eye"], math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], w, h), seed=5)
        assert len(o) == n
        hits = nr.closest_hits(a, o, d)                      # blocking cast: nine columns
        probe = nr.cast_rays(a, o, d)                        # the probe, mode 0: four columns in the same arena
        _same(words(probe), words(nr.cast_rays(_scene()[0], o, d)), "cast probe, %d rays" % n)
        assert np.array_equal(probe[0], (hits.flags & 1) != 0) and np.array_equal(bits(probe[1][:, 0][probe[0]]), bits(hits.toi[probe[0]]))
        points, normals = hit_points(o, d, hits)
        normals[(hits.flags & 1) == 0] = (0.0, 0.0, 1.0)
        keys = rng.integers(0, 2**63, size=n, dtype=np.int64).astype(np.uint64)
        max_toi = rng.uniform(0.5, 6.0, size=n)
        for num_dirs in (1, 16):
            L, R = nr.hemisphere_dirs(num_dirs), nr.rotation_table(5)
            occ = nr.occlusion_points(a, points, normals, L, R, hit_flags=hits.flags, keys=keys)  # blocking occlusion: tables, points, two outputs
            rays = nr.occlusion_ray_probe(a, points, normals, L, R, keys=keys)                    # the probe: the same tables and points, 48 * num_dirs bytes a point out
            _same(rays, nr.occlusion_ray_probe(_scene()[0], points, normals, L, R, keys=keys), "occlusion probe, %d points x %d" % (n, num_dirs))
            _same(rays, nr.occlusion_rays(points, normals, L, R, 1e-3, keys=keys), "occlusion probe against the numpy mirror")
            shadow = nr.shadow_rays(a, o, d, max_toi)                                             # the probe, mode 1: max_toi staged
            _same(words(shadow), words(nr.shadow_rays(_scene()[0], o, d, max_toi)), "shadow probe, %d rays" % n)
            _same(tuple(occ), tuple(nr.occlusion_points(a, points, normals, L, R, hit_flags=hits.flags, keys=keys)), "occlusion repeated")
        _same(tuple(nr.closest_hits(a, o, d)), tuple(hits), "cast repeated")
