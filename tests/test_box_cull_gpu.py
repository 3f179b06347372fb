"""The f32 box culling of the KERNELS against the reference's f64 ray / AABB test (tests/box_cull_cases.py holds the statement, the
restatements and the case sets; tests/test_box_cull.py shows the same on the CPU mirror).

nrays_debug_box_cull runs one node visit through the product's own device functions — make_rayf, best_f32, load_planes (mode 0) or
load_planes_uniform (mode 1), box_keys4, zero_axis_cull — and returns the four keys, RayF::bits and the three reciprocals.  Per class and
fetch mode: (a) every reciprocal within 1 ulp of the correctly rounded one (the premise of the error analysis), the cut-offs of inv_f32
applied as stated; (b) every key and the bits equal to the mirror's bit for bit, from the device's own reciprocals (packed fma rounded once,
fmaxf / fminf dropping a NaN, plane selection by address bit, the absent children's +inf); (c) the statement itself; and tightness on
the rays that clearly miss.  Then the traversals end to end on tiny axis-aligned meshes at the same edges, against the oracle's brute
force over all triangles (no BVT, tie rule D-2): hit / miss, node, triangle, toi and normal, through nrays_cast_rays, nrays_trace_rays
(NormalMaterial) and nrays_intersects_rays, in order and with NRAYS_RAYS_UNORDERED under NRAYS_RAY_REORDER=2 (the project's switch that
makes a small batch take the reordered path).  The caller-ray entry points never reach stream_device.h (only the staged frame path does,
whatever the batch size): its traversal meets the same meshes through a small staged frame, refilled and not, against the megakernel's."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import nrays_amd as nr
import oracle
from nrays_amd import abi
from tests import box_cull_cases as bc

pytestmark = pytest.mark.gpu
F32 = np.float32
NAMES = list(bc.CLASSES)
_probed = {}


def probed(name, mode):
    if (name, mode) not in _probed:
        c = bc.tightness_cases() if name == "tight" else bc.cases(name)
        _probed[(name, mode)] = bc.probe(mode, c)
    return _probed[(name, mode)]


@pytest.mark.parametrize("mode", [0, 1], ids=["lane_fetch", "uniform_fetch"])
@pytest.mark.parametrize("name", NAMES)
def test_reciprocals_keys_and_the_superset_statement(gpu, name, mode):
    c = bc.cases(name)
    n = len(c["o"])
    keys, bits, inv = probed(name, mode)
    # (a) the reciprocal: within 1 ulp where the device kept it; where it returned 0, a reciprocal within 1 ulp that inv_f32 cuts off exists
    # (a ray with all three components beyond 1e30 reports make_rayf's constant for x)
    x, r0 = bc.inv_exact(c["d"])
    cand = np.stack(bc.inv_candidates(c["d"]), axis=0)
    al = bc.all_long(c["d"], inv)
    assert (inv[al, 0] == bc.LONG_INV).all()
    inv = bc.inv_reported(c["d"], inv)
    kept = inv != 0
    with np.errstate(all="ignore"):
        worst = int(bc.ulps32(inv[kept], r0[kept]).max()) if kept.any() else 0
    print("%s mode %d: %d reciprocals kept, worst %d ulp from the correctly rounded one; %d axes unconstrained, %d rays with all three beyond 1e30" % (name, mode, kept.sum(), worst, (~kept).sum(), al.sum()))
    assert worst <= 1
    assert ((cand == 0).any(axis=0) | kept).all(), "inv_f32 returned 0 where no reciprocal within 1 ulp is cut off"
    assert ((cand != 0).any(axis=0) | ~kept).all(), "inv_f32 kept a reciprocal where every one within 1 ulp is cut off"
    # (b) keys and bits: the mirror on the device's own reciprocals
    mkeys, mbits = bc.mirror_keys(c["o"], c["d"], c["best"], c["box"], c["slot"], inv)
    assert np.array_equal(bits, mbits), np.flatnonzero(bits != mbits)[:5]
    same = bc.same_keys(keys, mkeys)
    assert same.all(), "%d keys differ from the mirror, first at case %d: %r vs %r" % ((~same).sum(), np.flatnonzero(~same.all(axis=1))[0],
                                                                                       keys[~same.all(axis=1)][0], mkeys[~same.all(axis=1)][0])
    other = np.ones((n, 4), bool)
    other[np.arange(n), c["slot"]] = False
    assert np.isposinf(keys[other]).all()                 # the three absent children
    k = keys[np.arange(n), c["slot"]]
    assert (np.isposinf(k) | (np.isfinite(k) & (k >= 0))).all()
    # (c) the statement
    bad = bc.violations(c, keys)
    print("%s mode %d: reference accepts %.2f %%, device %.2f %%" % (name, mode, 100 * c["ref"].mean(), 100 * np.isfinite(k).mean()))
    assert not len(bad), "%s: the reference accepts %d boxes the device culls, e.g. case %d" % (name, len(bad), bad[0])


@pytest.mark.parametrize("mode", [0, 1], ids=["lane_fetch", "uniform_fetch"])
def test_rays_that_clearly_miss_get_no_key(gpu, mode):
    """Tightness: a ray the exact test rejects even for the box grown by 2^-18 (|o_a| + max |b_a|) must get +inf (derivation: box_cull_cases)."""
    c = bc.tightness_cases()
    keys, bits, inv = probed("tight", mode)
    finite = np.isfinite(keys[np.arange(len(c["o"])), c["slot"]])
    print("tightness family mode %d: %d clear misses; reference accepts %.2f %%, device %.2f %%" % (mode, c["clear"].sum(), 100 * c["ref"].mean(), 100 * finite.mean()))
    print("  extra acceptance by relative push:", bc.extra_acceptance_by_push(c, finite))
    assert (bits & 7 == 0).all() and (inv != 0).all()
    assert not (c["clear"] & finite).any(), int((c["clear"] & finite).sum())
    assert not len(bc.violations(c, keys))


def test_recorded_margins_are_the_devices(gpu):
    """profiles/box_cull_margins.json (device accepts - reference accepts per class, quoted in DESIGN §3) was measured with this very probe: the
    figures are recorded, not bounds — this only says that the record is of these classes and that both fetch modes agree."""
    rec = json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "box_cull_margins.json")))
    assert set(rec["classes"]) == set(NAMES) | {"tight"}
    for name in NAMES + ["tight"]:
        assert bc.same_keys(probed(name, 0)[0], probed(name, 1)[0]).all(), name


# ---------------------------------------------------------------- the traversals, end to end ------------------------------------------------
BACKGROUND = (0.25, 0.5, 0.75)


def grid_mesh(shift):
    """54 axis-aligned triangles: 3 x 3 quads in each of the planes z = s, x = s, y = s (s = shift: 0 puts every plane into a coordinate
    plane), corners at multiples of 0.25 around (s, s, s) — every leaf box is flat and its triangles lie in its face; f32-exact at 1e5 too."""
    g = np.arange(-1, 3) * 0.5 - 0.25
    pts, idx = [], []
    for axis in range(3):
        base = len(pts)
        for i in range(4):
            for j in range(4):
                p = [0.0, 0.0, 0.0]
                p[(axis + 1) % 3], p[(axis + 2) % 3] = g[i], g[j]
                pts.append(p)
        for i in range(3):
            for j in range(3):
                a = base + 4 * i + j
                idx += [[a, a + 4, a + 5], [a, a + 5, a + 1]]
    pts = np.array(pts, F32) + F32(shift)
    assert np.array_equal(pts.astype(np.float64), np.array(pts, np.float64)) and len(idx) == 54
    return pts, np.array(idx, np.uint32)


PLACEMENTS = {"around_origin": (0.0, nr.Isometry3.identity), "at_1e5": (1e5, nr.Isometry3.identity),
              "rotated": (0.0, lambda: nr.Isometry3((0.37, -1.21, 2.05), (0.3, -0.5, 0.8)))}
_scenes = {}


def scenes(place):
    """(the mesh as ONE node, the same triangles as 54 one-triangle nodes — the oracle's brute force then names the triangle as the node,
    smallest index among equal distances (D-2) —, the mesh's corners, the node's rotation and translation)."""
    if place not in _scenes:
        shift, iso = PLACEMENTS[place]
        pts, idx = grid_mesh(shift)
        node = lambda p, i: nr.SceneNode(nr.NormalMaterial(), 0.0, 0.0, 1.0, 1.0, iso(), nr.TriMesh(p, i))  # noqa: E731
        lights = [nr.Light((0.0, 10.0, 0.0), 0.0, 1, (1, 1, 1))]
        one = nr.Scene([node(pts, idx)], lights, BACKGROUND)
        per_tri = nr.Scene([node(pts, idx[t:t + 1]) for t in range(len(idx))], lights, BACKGROUND)
        from nrays_amd import math3d
        R = np.array(math3d.rotation_from_axis_angle(iso().axis_angle), np.float64).reshape(3, 3)
        _scenes[place] = (one, per_tri, pts.astype(np.float64), R, np.array(iso().translation, np.float64))
    return _scenes[place]


def edge_rays(place, seed):
    """Rays from the classes, aimed at corners, edge points and interior points of the leaf boxes (= the grid's corners, points on its lines,
    points inside its quads): grazing from outside, from the coordinate origin, with zero components, with long and short directions."""
    rng = np.random.default_rng(seed)
    one, _, pts, R, T = scenes(place)
    n = 3072
    q = pts[rng.integers(0, len(pts), n)].copy()
    other = pts[rng.integers(0, len(pts), n)]
    w = np.where(rng.random(n) < 0.4, 0.0, rng.random(n))[:, None]
    q = q + w * (other - q)                                   # a corner, or a point of the segment between two corners
    q = q @ R.T + T                                           # (to world; a point near the corner is as good as the corner under a rotation)
    u = rng.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    kind = rng.integers(0, 6, n)
    axis = rng.integers(0, 3, n)
    u[kind == 1, axis[kind == 1]] = 0.0                        # a zero component: the ray stays in a plane through q parallel to a coordinate plane
    tiny = 10.0 ** rng.uniform(-36, -31, n) * np.where(rng.random(n) < 0.5, -1, 1)
    u[kind == 2, axis[kind == 2]] = tiny[kind == 2]           # a component that is zero in f32 only
    t = 10.0 ** rng.uniform(-1, 1.5, n)
    o = q - t[:, None] * u
    from0 = (kind == 3) & (np.abs(q).max(axis=1) > 0)
    o[from0] = 0.0                                            # from the coordinate origin
    d = np.where(from0[:, None], q, u)
    o = o + bc._nudge(rng, n, exact_share=0.3) * (np.abs(o) + np.abs(q)) * (~from0)[:, None]
    scale = np.ones(n)
    scale[kind == 4] = 10.0 ** rng.uniform(-12, 12, (kind == 4).sum())
    scale[kind == 5] = 10.0 ** rng.uniform(36, 38.3, (kind == 5).sum())
    d = np.clip(d * scale[:, None], -float(bc.FLT_MAX), float(bc.FLT_MAX))
    return np.ascontiguousarray(o), np.ascontiguousarray(d)


_expected = {}


def expected(place):
    """The oracle's brute force, once per placement: (rays, hit, toi, normal, triangle or -1 where the one-triangle nodes give another distance)."""
    if place not in _expected:
        one, per_tri, _, _, _ = scenes(place)
        o, d = edge_rays(place, 300 + sorted(PLACEMENTS).index(place))
        hit, out = oracle.cast(one.descriptor, o, d, bruteforce=True)
        thit, tout = oracle.cast(per_tri.descriptor, o, d, bruteforce=True)
        agree = (thit == hit) & (~hit | (tout[:, 0] == out[:, 0]))
        prim = np.where(hit & agree, tout[:, 7].astype(np.int64), -1)
        assert agree.mean() > 0.99, agree.mean()              # (the mesh's own AABB gates the one-node scene in addition: knife edges only)
        assert 0.25 < hit.mean() < 0.9, hit.mean()
        for a in (o, d, hit, out, prim):
            a.setflags(write=False)
        _expected[place] = (o, d, hit, out, prim)
    return _expected[place]


@pytest.fixture(params=[False, True], ids=["ordered", "unordered"])
def unordered(request, monkeypatch):
    if request.param:
        monkeypatch.setenv("NRAYS_RAY_REORDER", "2")          # read when a scene is created: the reorder then runs at any batch size
    return request.param


def fresh_scene(place):
    shift, iso = PLACEMENTS[place]
    pts, idx = grid_mesh(shift)
    return nr.Scene([nr.SceneNode(nr.NormalMaterial(), 0.0, 0.0, 1.0, 1.0, iso(), nr.TriMesh(pts, idx))], [nr.Light((0.0, 10.0, 0.0), 0.0, 1, (1, 1, 1))], BACKGROUND)


@pytest.mark.parametrize("place", sorted(PLACEMENTS))
def test_closest_hits_at_the_edges_equal_the_brute_force(gpu, place, unordered):
    o, d, hit, out, prim = expected(place)
    sc = fresh_scene(place)
    got = nr.closest_hits(sc, o, d, unordered=unordered)
    assert np.array_equal(got.node >= 0, hit), np.flatnonzero((got.node >= 0) != hit)[:5]
    assert np.array_equal(got.toi[hit], out[hit, 0]) and np.isposinf(got.toi[~hit]).all()
    assert (got.node[hit] == 0).all()
    known = hit & (prim >= 0)
    assert np.array_equal(got.prim[known], prim[known])
    assert np.abs(got.normal[hit] - out[hit, 1:4]).max() <= 1e-15
    print("%s: %d rays, %d hits, %d triangles named" % (place, len(o), hit.sum(), known.sum()))


@pytest.mark.parametrize("place", sorted(PLACEMENTS))
def test_traced_colours_at_the_edges_are_the_brute_forces_normals(gpu, place, unordered):
    """Scene::trace on a NormalMaterial mesh: (1 + n) / 2 in f32 of the closest hit's normal, the background for a miss."""
    o, d, hit, out, prim = expected(place)
    sc = fresh_scene(place)
    rgb = nr.trace_rays(sc, o, d, unordered=unordered)
    assert np.array_equal(rgb[~hit], np.broadcast_to(np.array(BACKGROUND, F32), rgb[~hit].shape))
    got_n = rgb[hit].astype(np.float64) * 2.0 - 1.0
    assert np.abs(got_n - out[hit, 1:4]).max() <= 2.0 ** -22   # f32 of the normal, one f32 sum, an exact halving


@pytest.mark.parametrize("place", sorted(PLACEMENTS))
def test_shadow_queries_with_max_toi_at_the_blocker(gpu, place, unordered):
    """Scene::intersects_ray blocks iff a hit has toi <= max_toi: max_toi exactly at the closest hit's distance, one f64 ulp below and above."""
    o, d, hit, out, prim = expected(place)
    sc = fresh_scene(place)
    toi = np.where(hit, out[:, 0], 1.0)
    for name, limit, blocked in (("at", toi, hit), ("below", np.nextafter(toi, -np.inf), np.zeros(len(o), bool)), ("above", np.nextafter(toi, np.inf), hit),
                                 ("unbounded", np.full(len(o), bc.DBL_MAX), hit)):
        if name == "below":
            limit = np.where(toi > 0.0, limit, -1.0)            # (below a distance of 0: nothing blocks)
        lit, _ = nr.intersects_rays(sc, np.array(o), np.array(d), np.array(limit), unordered=unordered)
        assert np.array_equal(~lit, blocked), (name, np.flatnonzero(~lit != blocked)[:5])


@pytest.mark.parametrize("refill", ["2", "0"], ids=["stream_device", "traverse"])
def test_staged_frames_of_the_meshes_equal_the_megakernel(gpu, monkeypatch, refill):
    """stream_device.h's traversal (the staged frame path with lane refill) on the same meshes: a camera ON a coordinate plane that holds
    triangles (rays with a zero component, origin coordinate 0), looking along the grid — the frame must be the megakernel's, pixel for pixel,
    and the oracle's within the north star's 1e-4."""
    from nrays_amd import math3d
    from tools import scenes_util as su
    cam = dict(eye=(0.0, 0.0, -4.0), at=(0.0, 0.0, 0.0), fovy=40.0)
    frames = {}
    for wf in ("0", "1"):
        monkeypatch.setenv("NRAYS_WAVEFRONT", wf)
        monkeypatch.setenv("NRAYS_WF_REFILL", refill)
        sc = fresh_scene("around_origin")
        p, _ = su.camera_params(cam, 64, 64)
        img = np.empty((64, 64, 3), F32)
        abi.check(abi.load_hip_lib().nrays_render(sc.device_handle(), C.byref(p), img.ctypes.data_as(C.POINTER(C.c_float))))
        frames[wf] = img
    assert np.array_equal(frames["0"], frames["1"])
    want, _ = oracle.render(sc.descriptor, p, 4)
    assert np.abs(frames["1"] - want).max() <= 1e-4
    assert (frames["1"] != np.array(BACKGROUND, F32)).any(axis=2).mean() > 0.05
