"""The CPU oracle against the independent restatement of the shading and bounce arithmetic (tests/shading_cases.py), inside a bound derived from
the reference's roundings — and the properties of the case sets themselves: every named single misreading of the reference, applied to the
restatement, moves some case by at least 100 x the bound.  No GPU.  The same cases run on the device in tests/test_shading_restated_gpu.py."""
import numpy as np
import pytest

import nrays_amd as nr
import oracle
from nrays_amd.scene import _rng_hash
from tests import shading_cases as sc
from tests.shading_cases import TRACE_CASES, report, shade_args
from tests.test_shade_points import build_shade_shim, shim_shade
from tests.test_trace_rays import build_shim, shim_trace


@pytest.fixture(scope="module")
def shims(tmp_path_factory):
    d = tmp_path_factory.mktemp("restated_shims")
    return build_shim(d), build_shade_shim(d)


# ---- tie-ins ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsample", sc.RACSAMPLE_NSAMPLES)
def test_racsample_is_the_floor_of_the_f32_square_root(nsample):
    want = {1: 1, 2: 1, 3: 1, 4: 2, 5: 2, 9: 3, 10: 3}[nsample]   # light.rs:20
    assert sc.racsample(nsample) == want == nr.Light((0, 0, 0), 0.1, nsample, (1, 1, 1)).racsample


def test_the_sample_positions_use_the_oracles_rng():
    """u = (hash(key, 0x1000 + dim) >> 11) * 2^-53 with key = hash(hash(seed, pixel), sample) is oracle.rng_u01."""
    for seed, pixel, sample, dim in ((0, 0, 0, 0), (7, 12345, 3, 2), (2 ** 63 + 5, 2 ** 40 + 1, 9, 1)):
        key = _rng_hash(_rng_hash(np.array([seed], np.uint64), pixel), sample)
        u = float((_rng_hash(key, 0x1000 + dim) >> np.uint64(11)).astype(np.float64)[0] * 2.0 ** -53)
        assert u == oracle.rng_u01(seed, pixel, sample, dim) and 0.0 <= u < 1.0
    area = sc.LIGHT_SETS["area"]
    pos = sc.light_positions(area, np.array([1, 3, 2 ** 63 + 1], np.uint64))
    assert pos[0].shape == (3, 4, 3) and pos[1].shape == (3, 1, 3)
    off = (pos[0] - np.asarray(area[0].pos)) / area[0].radius
    assert (off >= 0.0).all() and (off < 1.0).all() and len(np.unique(off)) == off.size
    assert np.array_equal(pos[1], np.tile(np.asarray(area[1].pos), (3, 1, 1)))


def test_the_case_sets_hold_their_edges():
    c = sc.points_set("one")
    n = len(c["points"])
    assert sc.N_RANDOM + 150 < n <= 2000 / 3 + 150 and c["directed"].sum() == 20 * len(sc.MATS)
    L = np.asarray(c["lights"][0].pos)
    ld = sc._unit(L - c["points"])
    dln = (ld * c["normals"]).sum(axis=1)[c["directed"]]
    for v in (0.0, sc.DENORM_MIN, -sc.DENORM_MIN, -1.0):
        assert (dln == v).any(), v
    e, a = np.float32(sc.ENERGY_ROUNDS), np.float32(sc.ATT_ROUNDS)
    assert (np.float32(e - a) > sc.F01) != (float(e) - float(a) > float(sc.F01))
    w = sc.world_b()
    smp = sc.light_samples(w, sc.points_set("filters")["points"], sc.points_set("filters")["keys"])
    crossings = np.concatenate([s[3].ravel() for s in smp])
    blocked = np.concatenate([(~s[2]).ravel() for s in smp])
    assert {0, 1, 2, 3} <= set(crossings.tolist()) and blocked.any() and not blocked.all()
    assert (smp[3][1][smp[3][2]] == 0.0).all() and smp[3][2].any()              # beyond the UVMaterial plane: lit, filter 0
    assert np.max([s[1].max() for s in smp]) > 0.5


# ---- the oracle against the restatement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("light_set", ["one", "three", "area"])
def test_oracle_compute_in_free_space(shims, light_set):
    world, c = sc.world_a(light_set), sc.points_set(light_set)
    want, err, keep, _ = sc.expected_points(world, c)
    assert keep.all()
    got = shim_shade(shims[1], sc.build_scene(world), **shade_args(c))
    assert np.array_equal(got[:, 3].astype(np.float64), want[:, 3])
    assert report("A " + light_set, sc.worst_ratio(got[:, :3], want[:, :3], err[:, :3])) <= 1.0


def test_oracle_compute_behind_filters(shims):
    world, c = sc.world_b(), sc.points_set("filters")
    want, err, keep, _ = sc.expected_points(world, c)
    scene = sc.build_scene(world)
    got = shim_shade(shims[1], scene, **shade_args(c))
    assert np.array_equal(got[:, 3].astype(np.float64), want[:, 3])
    assert report("B compute", sc.worst_ratio(got[:, :3], want[:, :3], err[:, :3], keep)) <= 1.0
    o, d, mt, lit, filt, ferr, fkeep = sc.shadow_rays_set(world, c)
    res = [oracle.shadow(scene.descriptor, o[i], d[i], mt[i]) for i in range(len(o))]
    olit = np.array([r is not None for r in res])
    ofilt = np.array([np.zeros(3) if r is None else r.astype(np.float64) for r in res])
    assert np.array_equal(olit[fkeep], lit[fkeep])
    assert report("B filter", sc.worst_ratio(ofilt, filt, ferr, fkeep)) <= 1.0


@pytest.mark.parametrize("name", ["probe", "quad_probe", "slab", "mirror"])
def test_oracle_trace(shims, name):
    world, rays = TRACE_CASES[name]()
    o, d, r, e, k = rays
    want, err = sc.trace(world, o, d, r, e, k)
    got = shim_trace(shims[0], sc.build_scene(world), o, d, refr=r, energy=e, keys=k)
    assert report("C " + name, sc.worst_ratio(got, want, err)) <= 1.0


@pytest.mark.parametrize("quad", [False, True])
def test_oracle_frame(quad):
    world = sc.frame_world(quad)
    want, err = sc.expected_frame(world)
    _, _, _, proj = sc.frame_rays()
    p = nr.make_params(sc.FRAME["resolution"], 1, 0.0, sc.FRAME["eye"], proj, seed=sc.FRAME["seed"])
    got, _ = oracle.render(sc.build_scene(world).descriptor, p, num_threads=2)
    assert len(np.unique(want.reshape(-1, 3).round(3), axis=0)) > 50                # the plane, the quad's surroundings and the ball are all in view
    assert report("C frame quad=%s" % quad, sc.worst_ratio(got, want, err)) <= 1.0


# ---- discriminating power: a property of the case sets (no oracle, no GPU) --------------------------------------------------------------------------
def _moved(mistake):
    """The worst |mistaken restatement - restatement| / bound over the case sets the mistake can touch."""
    worst = 0.0
    if mistake in ("max_before_lproj", "scoeff_unnormalised", "axpy_crossed", "max_before_cast"):
        for ls in ("one", "three", "area"):
            world, c = sc.world_a(ls), sc.points_set(ls)
            want, err, _, _ = sc.expected_points(world, c)
            bad = sc.expected_points(world, c, mistake)[0]
            worst = max(worst, sc.worst_ratio(bad[:, :3], want[:, :3], err[:, :3], finite=False))
    elif mistake in ("filter_without_node_alpha", "filter_alpha_first"):
        world, c = sc.world_b(), sc.points_set("filters")
        want, err, keep, _ = sc.expected_points(world, c)
        bad = sc.expected_points(world, c, mistake)[0]
        worst = sc.worst_ratio(bad[:, :3], want[:, :3], err[:, :3], keep, finite=False)
    else:
        for name in ("probe", "slab", "mirror"):
            world, (o, d, r, e, k) = TRACE_CASES[name]()
            want, err = sc.trace(world, o, d, r, e, k)
            worst = max(worst, sc.worst_ratio(sc.trace(world, o, d, r, e, k, mistake)[0], want, err, finite=False))
    return worst


@pytest.mark.parametrize("mistake", sc.MISTAKES)
def test_a_single_misreading_moves_some_case_by_100_bounds(mistake):
    moved = _moved(mistake)
    print("%s: %.1f x the bound" % (mistake, moved))
    assert moved >= 100.0


@pytest.mark.parametrize("identity", sc.IDENTITIES)
def test_two_named_rewritings_are_identities_and_stay_inside_the_bound(identity):
    """max(0.0) before or after `as f32`, and (1 - alpha) before or after the component product: the same real number (shading_cases' docstring)."""
    assert _moved(identity) <= 1.0
