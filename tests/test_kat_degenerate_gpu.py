"""The HIP intersectors at DEGENERATE and NEAR-DEGENERATE rays against tests/golden/kat_degenerate.npz (60-digit mpmath on the shapes' convex
gauges, tests/golden/make_kat_degenerate.py): one scene per (shape, parameters, transform, solid) and all its rays in one call, 32 scenes.
Three paths meet the fixture:
  1. nr.cast_rays (nrays_debug_cast_batch, the record path) under the full checks of tests/test_kat_degenerate.py;
  2. Scene.cast_rays / closest_hits (nrays_cast_rays) equal to 1 by bit pattern in toi, normal and node;
  3. nr.shadow_rays on the opaque nodes, the record = 0 path (cast_ball without its square roots, cast_instance(..., false)): blocked with
     max_toi = 2 toi where the fixture says hit, not blocked with toi / 2 where toi > 0, never blocked on a miss.
The frame kernels are out of scope: raygen cannot deliver an exact zero component."""
import numpy as np
import pytest

import nrays_amd as nr
from tests import test_kat_degenerate as kd

pytestmark = pytest.mark.gpu


def other_paths(scene, rows, o, d, hit, out):
    h = scene.cast_rays(o, d)
    assert np.array_equal(h.node >= 0, hit) and np.array_equal((h.flags & 1) != 0, hit)
    assert np.array_equal(h.toi[hit].view(np.uint64), out[hit, 0].view(np.uint64)) and np.isinf(h.toi[~hit]).all()
    assert np.array_equal(np.ascontiguousarray(h.normal[hit]).view(np.uint64), np.ascontiguousarray(out[hit, 1:4]).view(np.uint64))
    assert np.array_equal(h.node[hit], out[hit, 7].astype(np.int32)) and (h.prim == -1).all()
    sure = np.array([kd.asserted(c) for c in rows])
    want, toi = rows[:, 17] != 0, rows[:, 18]
    blocked, _ = nr.shadow_rays(scene, o, d, np.where(want, 2.0 * toi, 1e30))
    assert np.array_equal(blocked[sure], want[sure]), np.nonzero(blocked[sure] != want[sure])
    far = sure & want & (toi > 0)
    blocked, _ = nr.shadow_rays(scene, o[far], d[far], 0.5 * toi[far])
    assert not blocked.any(), np.nonzero(blocked)


def test_hip_casts_against_the_degenerate_fixture(gpu):
    kd.check_fixture(lambda scene, o, d: nr.cast_rays(scene, o, d), "HIP", also=other_paths)


@pytest.mark.parametrize("cells,translation", [(4, (0.0, 0.0, 0.0)), (4, (7.0, -3.0, 11.0)), (32, (0.0, 0.0, 0.0)), (32, (7.0, -3.0, 11.0))])
def test_hip_rays_through_lattice_vertices_and_edge_midpoints_are_exact(gpu, cells, translation, monkeypatch, capfd):
    """4 x 4 quads: 32 triangles, the host builder; 32 x 32: 2 048, the device builder.  Every ray hits with exactly the integer toi and the
    smallest index among the tied triangles, on all three paths; a ray one unit beside the mesh misses."""
    monkeypatch.setenv("NRAYS_BUILD_TIMES", "1")
    o, d, toi, prim, normal = kd.lattice_rays(cells)
    want = np.isfinite(toi)
    assert want.sum() == 2 * (2 * cells - 1) ** 2 and (~want).sum() == 8
    scene = kd.lattice_scene(cells, translation)
    o = o + np.array(translation)
    hit, out = nr.cast_rays(scene, o, d)
    assert ("device BLAS build" in capfd.readouterr().err) == (cells == 32)
    assert np.array_equal(hit, want) and np.array_equal(out[hit, 0], toi[hit]) and (out[hit, 7] == 0).all()
    assert np.abs(out[hit, 1:4] - normal[hit]).max() <= 1e-15
    h = scene.cast_rays(o, d)
    assert np.array_equal(h.node >= 0, want) and np.array_equal(h.toi[want], toi[want]) and np.array_equal(h.prim, prim)
    assert np.array_equal(np.ascontiguousarray(h.normal[want]).view(np.uint64), np.ascontiguousarray(out[want, 1:4]).view(np.uint64))
    blocked, _ = nr.shadow_rays(scene, o, d, np.where(want, 16.0, 1e30))
    assert np.array_equal(blocked, want)
    blocked, _ = nr.shadow_rays(scene, o[want], d[want], np.full(want.sum(), 4.0))
    assert not blocked.any()
