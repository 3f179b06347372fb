"""nrays_irradiance_points_vis_device / nrays_irradiance_points_vis on the GPU: every result is compared BIT FOR BIT with the numpy mirror
irradiance_points_ref(visibility=...) (whose properties tests/test_probe_depth.py tests without a GPU) on random grids and moments; moments beyond every distance
give nrays_irradiance_points* bit for bit; the mechanism is pinned exactly where the variance is zero; and, end to end, two rooms divided by a thin wall with the
light in one of them: points behind the wall get less light with visibility than without, points in the open get the same."""
import itertools
import math

import numpy as np
import pytest

import nrays_amd as nr
from nrays_amd.marshal import CURRENT
from tests.test_irradiance import interior_points, random_grid, same, unit_vectors
from tests.test_irradiance_gpu import check, scene

pytestmark = pytest.mark.gpu

RES = (4, 8, 16)
N = 2 * 256 + 3  # two workgroups and three points


def random_moments(seed, P, R):
    """Mean depths around the grid's spacing and mean squares at or above their squares: a third of the texels with zero variance."""
    rng = np.random.default_rng(seed)
    m1 = rng.uniform(0.05, 1.2, size=(P, R * R)).astype(np.float32)
    m2 = (m1 * m1 + rng.uniform(0.0, 0.3, size=(P, R * R)).astype(np.float32)).astype(np.float32)
    m2[:, ::3] = (m1 * m1)[:, ::3]
    return np.stack([m1, m2], axis=2)


def points_for(grid, n, seed):
    """Inside the grid, exactly on probes, and outside every face."""
    p = interior_points(seed, grid, n)
    probes = nr.probe_grid_positions(grid.origin, grid.cell, grid.counts)
    rng = np.random.default_rng(seed + 1)
    p[::5] = probes[rng.integers(0, len(probes), size=len(p[::5]))]
    far = np.arange(3, n, 7)
    p[far, rng.integers(0, 3, size=len(far))] += rng.choice([-4.0, 4.0], size=len(far))
    return p


@pytest.mark.parametrize("R", RES)
@pytest.mark.parametrize("counts", [(1, 1, 1), (2, 2, 2), (3, 1, 2)])
def test_equals_the_mirror_bit_for_bit(gpu, counts, R):
    sc, _ = scene()
    P = counts[0] * counts[1] * counts[2]
    g0 = random_grid(200 + R, counts, 3 if R != 8 else 2)
    mo0 = random_moments(300 + R + P, P, R)
    p, nm = points_for(g0, N, 400 + R), unit_vectors(401 + R, N)
    flags = np.random.default_rng(402).integers(0, 2, size=N).astype(np.uint32) | np.uint32(4)
    live = (flags & 1) != 0
    ps, ns = np.where(live[:, None], p, 0.0), np.where(live[:, None], nm, 0.0)
    p[~live] = np.nan; nm[~live] = np.nan           # a skipped point's point and normal are not read
    held = 0
    for with_valid, facing, floor, bias in itertools.product((False, True), (False, True), (0.0, 0.25), (0.0, 0.01)):
        g, mo = g0, mo0
        if with_valid:                                # NaN in the SH row and the moment row of every invalid probe: never read
            valid = (np.random.default_rng(403 + P).uniform(size=P) < 0.6).astype(np.uint32) | np.uint32(8)
            valid[0] |= 1
            sh, mo = g0.sh.copy(), mo0.copy()
            sh[(valid & 1) == 0] = np.nan; mo[(valid & 1) == 0] = np.nan
            g = g0._replace(sh=sh, valid=valid)
        vis = nr.ProbeVisibility(mo, R, floor, bias)
        want = nr.irradiance_points_ref(ps, ns, g, facing, flags, visibility=vis)
        got = nr.irradiance_points(sc, p, nm, g, facing, flags, True, True, visibility=vis)
        check(got, want, (counts, R, with_valid, facing, floor, bias))
        assert np.isfinite(got.rgb).all() and (got.rgb[~live].view(np.uint32) == 0).all()
        plain = nr.irradiance_points_ref(ps, ns, g, facing, flags)
        held += int((want[2] != plain[2]).sum())
    assert held > 100                                 # the factor is at work in these cases
    three = np.flatnonzero(live)[:3]                  # three points, the method, rgb alone
    assert same(sc.irradiance_points(p[three], nm[three], g0, visibility=nr.ProbeVisibility(mo0, R)),
                nr.irradiance_points_ref(p[three], nm[three], g0, visibility=nr.ProbeVisibility(mo0, R))[0])


@pytest.mark.parametrize("R", RES)
def test_moments_beyond_every_distance_are_the_call_without_visibility(gpu, R):
    import torch
    sc, _ = scene()
    for counts, bands, facing in (((1, 1, 1), 1, False), ((2, 2, 2), 3, True), ((3, 1, 2), 2, False)):
        P = counts[0] * counts[1] * counts[2]
        g = random_grid(500 + R, counts, bands)
        g = g._replace(valid=(np.random.default_rng(501).uniform(size=P) < 0.7).astype(np.uint32))
        p, nm = points_for(g, N, 502), unit_vectors(503, N)
        vis = nr.ProbeVisibility(np.full((P, R * R, 2), 1e30, np.float32), R, 0.25, 0.01)
        plain = nr.irradiance_points(sc, p, nm, g, facing, None, True, True)
        got = nr.irradiance_points(sc, p, nm, g, facing, None, True, True, visibility=vis)
        check(got, plain, (counts, R))
        up = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
        dev = nr.irradiance_points(sc, up(p), up(nm), g._replace(sh=up(g.sh), valid=up(g.valid.view(np.int32))), facing, None, True, True,
                                   visibility=vis._replace(moments=up(vis.moments)))
        check(dev, plain, (counts, R, "device"))


def test_the_mechanism_where_the_variance_is_zero(gpu):
    """Probes that see nothing within max_dist = 1 hold (1, 1) in every texel: var == 0, so beyond distance 1 a probe's factor is the floor — exactly 0 here."""
    empty = nr.Scene([], [nr.Light((0.0, 5.0, 0.0), 0.0, 1, (1, 1, 1))], (0.0, 0.0, 0.0))
    sh = np.zeros((2, 9, 3), np.float32)
    sh[0] = np.random.default_rng(600).uniform(0.5, 1.0, size=(9, 3))
    sh[0, 1:] *= 0.05                                 # a positive irradiance at every normal
    g = nr.ProbeGrid((0.0, 0.0, 0.0), (4.0, 1.0, 1.0), (2, 1, 1), sh, None, 4.0 * math.pi)
    vis, valid = nr.bake_probe_visibility(empty, g, nr.sphere_dirs(256), 8, max_dist=1.0, near_dist=0.25, floor=0.0)
    assert vis.moments.shape == (2, 64, 2) and (vis.moments == 1.0).all() and valid.tolist() == [1, 1] and vis.floor == 0.0 and vis.res == 8
    sc, _ = scene()
    nm = unit_vectors(601, 4)
    beyond = np.array([(1.5, 0.0, 0.0), (2.0, 0.5, -0.5), (0.0, 1.0, 0.5), (0.9, 0.6, 0.0)])   # farther than 1 from probe 0 (and from probe 1, or not)
    got = nr.irradiance_points(sc, beyond, nm, g, visibility=vis, want_weight=True)
    plain = nr.irradiance_points(sc, beyond, nm, g)
    assert (got.rgb.view(np.uint32) == 0).all() and (plain > 0).all()
    check((got.rgb, None, got.weight), nr.irradiance_points_ref(beyond, nm, g, visibility=vis))
    g1 = g._replace(cell=(1.0, 1.0, 1.0))             # the two probes one apart: points within 1 of both
    vis1, _ = nr.bake_probe_visibility(empty, g1, nr.sphere_dirs(256), 8, max_dist=1.0, near_dist=0.25, floor=0.0)
    within = np.array([(0.5, 0.0, 0.0), (0.25, 0.4, 0.4), (0.75, -0.5, 0.25), (0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (0.5, 0.8, 0.0)])
    assert (np.sqrt(((within[:, None, :] - np.array([(0.0, 0, 0), (1.0, 0, 0)])[None]) ** 2).sum(axis=2)) <= 1.0).all()
    nm = unit_vectors(602, 6)
    check(nr.irradiance_points(sc, within, nm, g1, True, None, True, True, visibility=vis1), nr.irradiance_points(sc, within, nm, g1, True, None, True, True))


def two_rooms():
    """Two closed rooms, A (x < 0) and B (x > 0), divided by a cuboid wall 0.1 thick; one light, in A; no ambient term anywhere."""
    mat = nr.PhongMaterial((0.0, 0.0, 0.0), (0.8, 0.7, 0.6), (0.0, 0.0, 0.0), None, None, 20.0)
    node = lambda t, h: nr.SceneNode(mat, 0.0, 0.0, 1.0, 1.0, nr.Isometry3(t), nr.Cuboid(h))  # noqa: E731
    slabs = [((0, -0.25, 0), (6.5, 0.25, 3.0)), ((0, 5.25, 0), (6.5, 0.25, 3.0)), ((-6.25, 2.5, 0), (0.25, 3.0, 3.0)), ((6.25, 2.5, 0), (0.25, 3.0, 3.0)),
             ((0, 2.5, -2.75), (6.5, 3.0, 0.25)), ((0, 2.5, 2.75), (6.5, 3.0, 0.25)), ((0, 2.5, 0), (0.05, 2.5, 2.5))]
    return nr.Scene([node(t, h) for t, h in slabs], [nr.Light((-3.0, 2.5, 0.0), 0.0, 1, (3.0, 3.0, 3.0))], (0.0, 0.0, 0.0))


def test_end_to_end_a_wall_between_two_rooms(gpu):
    """The rooms' inner boxes are [-6, -0.05] and [0.05, 6] x [0, 5] x [-2.5, 2.5]; the probes sit one apart, the nearest 0.45 from the wall.  max_dist = 2 is a power
    of two, so a texel whose rays all reach it holds (2, 4) exactly, and the grid's cell diagonal sqrt(3) is shorter: a point with no surface within 2 lies within its
    eight probes' mean depth towards it, and gets no factor."""
    import torch
    sc = two_rooms()
    k = next(k for k in range(64, 1025) if len(np.unique(nr.oct_texel(nr.sphere_dirs(k), 8))) == 64)  # the fewest sphere directions that leave no texel of R = 8 empty
    assert len(np.unique(nr.oct_texel(nr.sphere_dirs(k - 1), 8))) < 64
    L = nr.sphere_dirs(k)
    grid = nr.bake_probe_grid(sc, (-5.5, 0.5, -2.0), (1.0, 1.0, 1.0), (12, 5, 5), L, 3, device=CURRENT)
    vis, valid = nr.bake_probe_visibility(sc, grid, L, 8, max_dist=2.0, near_dist=0.2, floor=0.0)
    assert torch.is_tensor(grid.sh) and torch.is_tensor(vis.moments) and torch.is_tensor(valid) and bool((valid == 1).all())
    sh, mo = grid.sh.cpu().numpy(), vis.moments.cpu().numpy()
    pos = nr.probe_grid_positions(grid.origin, grid.cell, grid.counts)
    assert (sh[pos[:, 0] > 0].view(np.uint32) == 0).all() and (np.abs(sh[pos[:, 0] < 0]).sum(axis=(1, 2)) > 0).all()  # the room-B probes are exact zeros
    grid = grid._replace(valid=valid)
    g_np, v_np = grid._replace(sh=sh, valid=valid.cpu().numpy().view(np.uint32)), vis._replace(moments=mo)
    rng = np.random.default_rng(700)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731

    def both(p, nm):
        plain = nr.irradiance_points(sc, up(p), up(nm), grid).cpu().numpy()
        seen = nr.irradiance_points(sc, up(p), up(nm), grid, visibility=vis).cpu().numpy()
        assert same(plain, nr.irradiance_points_ref(p, nm, g_np)[0]) and same(seen, nr.irradiance_points_ref(p, nm, g_np, visibility=v_np)[0])
        return plain, seen
    # room B, within one cell of the wall, around the middle of a cell's face, looking at the wall
    n = 300
    cy, cz = rng.integers(1, 4, size=n) + 0.0, rng.integers(-2, 2, size=n) + 0.5
    p = np.stack([rng.uniform(0.3, 0.45, size=n), cy + rng.uniform(-0.2, 0.2, size=n), cz + rng.uniform(-0.2, 0.2, size=n)], axis=1)
    nm = np.array([-1.0, 0.0, 0.0]) + rng.uniform(-0.2, 0.2, size=(n, 3))
    nm /= np.sqrt((nm * nm).sum(axis=1))[:, None]
    plain, seen = both(p, nm)
    ratio = seen.astype(np.float64) / plain.astype(np.float64)
    print("light behind the wall, E_vis / E_plain per channel: median %.4g, max %.4g, min %.4g (E_plain median %.4g)"
          % (np.median(ratio), ratio.max(), ratio.min(), np.median(plain)))
    assert (seen >= 0).all() and (seen < plain).all()
    # room A, no surface within max_dist: bit-identical
    p = np.stack([rng.uniform(-4.0, -2.05, size=n), rng.uniform(2.0, 3.0, size=n), rng.uniform(-0.5, 0.5, size=n)], axis=1)
    p[::10] = pos[(pos[:, 0] == -3.5) & (pos[:, 1] == 2.5) & (pos[:, 2] == 0.0)]  # and exactly on a probe
    plain, seen = both(p, unit_vectors(701, n))
    assert same(plain, seen) and (plain != 0).any()
