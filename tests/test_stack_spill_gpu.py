"""The traversal stack beyond its LDS slots, on the device (trace_device.h: Stack — the HBM half of push / pop, the wave_has_room ballot, the
ballot in pop, the column addressing and stride of the spill region, the sizing rule of derive_scene_facts, the region each launch is
given).  tests/stack_cases.py holds the ladder scenes and rays; tests/test_stack_spill.py proves on the CPU that in every scene and both
visiting orders a quarter of the rays hold 12 slots more than the LDS part while a tenth stay at 4, mixed inside every 64 consecutive rays.
The first test here shows that the tree of that proof IS the tree the library builds.  Then every query is held to the oracle's brute
force over all triangles (no BVT, no stack), in order and with NRAYS_RAYS_UNORDERED under NRAYS_RAY_REORDER=2; the composite calls to the
compositions their own test files pin them to; frames to the oracle's and to each other; overlapping pipelined traces — only scenes
without meshes are pipelined, so on ladders of cuboid plates, whose TLAS holds the chains — to the direct path's frames."""
import ctypes as C
import os

import numpy as np
import pytest

import nrays_amd as nr
import oracle
from nrays_amd import abi
from tests import stack_cases as sc
from tools import scenes_util as su

pytestmark = pytest.mark.gpu
F32 = np.float32
DBL_MAX = float(np.finfo(np.float64).max)
QUERY_SCENES = ("a_world", "a_translated", "a_rotated", "b_alpha", "c_tlas", "d_planes", "e_hair")
NORMAL_SCENES = ("a_world", "a_translated", "a_rotated", "c_tlas", "e_hair")   # every node a NormalMaterial
RAY_CLASSES = ("rays_primary", "rays_reflection", "rays_refraction", "rays_shadow")


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return sc.BuildShim(tmp_path_factory.mktemp("bvh_build_shim"))


@pytest.fixture(params=[False, True], ids=["ordered", "unordered"])
def unordered(request, monkeypatch):
    if request.param:
        monkeypatch.setenv("NRAYS_RAY_REORDER", "2")          # read when a scene is created: the reorder then runs at any batch size
    return request.param


def _flags(scene):
    out = (C.c_uint32 * 2)()
    abi.check(abi.load_hip_lib().nrays_debug_scene_flags(scene.device_handle(), out))
    return out[0], out[1]


def test_the_library_builds_the_tree_whose_reach_was_proved(gpu, shim):
    """nrays_debug_blas_build, host builder, pre-splitting as a scene applies it: node for node the shim's tree."""
    pts, idx, _, _ = sc.ladder()
    want = shim.build(pts, idx)
    v = np.ascontiguousarray(pts.astype(np.float64)); ix = np.ascontiguousarray(idx, np.uint32)
    m = abi.NraysMesh(len(v), len(ix), v.ctypes.data_as(C.POINTER(C.c_double)), None, ix.ctypes.data_as(C.POINTER(C.c_uint32)))
    cap = 12 * len(ix) + 64
    nodes = np.zeros((cap, 32), F32); tri = np.zeros(cap, np.uint32)
    d = abi.NraysBlasDump()
    d.node_capacity = cap; d.ref_capacity = cap
    d.nodes = nodes.ctypes.data_as(C.POINTER(C.c_float)); d.tri_ids = tri.ctypes.data_as(C.POINTER(C.c_uint32))
    abi.check(abi.load_hip_lib().nrays_debug_blas_build(C.byref(m), 0, C.byref(d)))
    assert d.hairy == 0 and d.num_refs == len(ix)                      # no rung was split
    assert (d.root, d.max_depth, d.num_nodes) == (want["root"], want["depth"], len(want["nodes"]))
    assert np.array_equal(nodes[:d.num_nodes].view(np.uint32), want["nodes"].view(np.uint32))
    assert np.array_equal(tri[:d.num_refs], want["tri"])
    assert sc.need(d.max_depth) > sc.lds_stack()


# ---------------------------------------------------------------- the queries against the brute force ------------------------------------------

@pytest.mark.parametrize("name", QUERY_SCENES)
def test_closest_hits_equal_the_brute_force(gpu, name, unordered):
    o, d, hit, out, prim = sc.expected(name)
    scene = sc.make_scene(name)
    got = nr.closest_hits(scene, o, d, unordered=unordered)
    if name == "e_hair":
        assert _flags(scene)[1] == 1                                   # quorum-ended node phases: parked lanes push their node
    if name == "d_planes":
        assert _flags(scene)[0] & 3 == 3                               # analytic shapes and meshes: plane pseudo-leaves below everything
    assert np.array_equal(got.node >= 0, hit), np.flatnonzero((got.node >= 0) != hit)[:5]
    assert np.array_equal(got.toi[hit], out[hit, 0]) and np.isposinf(got.toi[~hit]).all(), np.flatnonzero(hit & (got.toi != out[:, 0]))[:5]
    assert np.array_equal(got.node[hit], out[hit, 7].astype(np.int32))
    known = hit & (prim >= 0)
    assert np.array_equal(got.prim[known], prim[known]), np.flatnonzero(known & (got.prim != prim))[:5]
    assert np.abs(got.normal[hit] - out[hit, 1:4]).max() <= 1e-15
    print("%s: %d rays, %d hits, %d rungs named" % (name, len(o), hit.sum(), known.sum()))


@pytest.mark.parametrize("name", QUERY_SCENES)
def test_the_cast_probe_equals_the_brute_force(gpu, name):
    """nrays_debug_cast_batch mode 0: the closest-hit query with its deferred gates as shade_hit runs it."""
    o, d, hit, out, prim = sc.expected(name)
    ghit, gout = nr.cast_rays(sc.make_scene(name), o, d)
    assert np.array_equal(ghit, hit), np.flatnonzero(ghit != hit)[:5]
    assert np.array_equal(gout[hit, 0], out[hit, 0]) and np.array_equal(gout[hit, 7], out[hit, 7])
    assert np.abs(gout[hit, 1:4] - out[hit, 1:4]).max() <= 1e-15


@pytest.mark.parametrize("name", NORMAL_SCENES)
def test_traced_colours_are_the_brute_forces_normals(gpu, name, unordered):
    """Scene::trace on NormalMaterial nodes: (1 + n) / 2 in f32 of the closest hit's normal, the background for a miss."""
    o, d, hit, out, prim = sc.expected(name)
    rgb = nr.trace_rays(sc.make_scene(name), o, d, unordered=unordered)
    assert np.array_equal(rgb[~hit], np.broadcast_to(np.array(sc.BACKGROUND, F32), rgb[~hit].shape))
    got_n = rgb[hit].astype(np.float64) * 2.0 - 1.0
    assert np.abs(got_n - out[hit, 1:4]).max() <= 2.0 ** -22       # f32 of the normal, one f32 sum, an exact halving


def _limits(hit, out):
    toi = np.where(hit, out[:, 0], 1.0)
    below = np.where(toi > 0.0, np.nextafter(toi, -np.inf), -1.0)      # (below a distance of 0: nothing blocks)
    none = np.zeros(len(hit), bool)
    return (("at", toi, hit), ("below", below, none), ("above", np.nextafter(toi, np.inf), hit), ("unbounded", np.full(len(hit), DBL_MAX), hit))


@pytest.mark.parametrize("name", [n for n in QUERY_SCENES if n != "b_alpha"])
def test_shadow_queries_with_max_toi_at_the_blocker(gpu, name, unordered):
    """Every node is opaque: Scene::intersects_ray blocks iff the closest hit lies within max_toi — exactly at it, one f64 ulp below, one above,
    unbounded (the walk of the CPU proof); nrays_intersects_rays and nrays_debug_cast_batch mode 1."""
    o, d, hit, out, prim = sc.expected(name)
    scene = sc.make_scene(name)
    for what, limit, blocked in _limits(hit, out):
        lit, _ = nr.intersects_rays(scene, np.array(o), np.array(d), np.array(limit), unordered=unordered)
        assert np.array_equal(~lit, blocked), (what, np.flatnonzero(~lit != blocked)[:5])
        if not unordered:
            pblocked, _ = nr.shadow_rays(scene, o, d, limit)
            assert np.array_equal(pblocked, blocked), (what, np.flatnonzero(pblocked != blocked)[:5])


def test_a_transparent_ladder_filters_like_the_oracle(gpu, unordered):
    """Scene (b): alpha < 1, so a shadow ray collects the node's closest hit under the sentinel and nothing ends its walk early.  One transparent
    node means one factor: the filter is oracle.shadow's bit for bit, (1, 1, 1) where nothing lies within max_toi."""
    o, d, hit, out, prim = sc.expected("b_alpha")
    scene = sc.make_scene("b_alpha")
    desc = scene.descriptor
    assert _flags(scene)[0] & 4
    for what, limit, within in _limits(hit, out):
        want = np.ones((len(o), 3), F32)
        for i in np.flatnonzero(hit):
            f = oracle.shadow(desc, o[i], d[i], limit[i])
            assert f is not None
            want[i] = f
        assert ((want != 1).any(axis=1) == within).all(), what
        lit, filt = nr.intersects_rays(scene, np.array(o), np.array(d), np.array(limit), unordered=unordered)
        assert lit.all(), what
        assert np.array_equal(filt.view(np.uint32), want.view(np.uint32)), (what, np.flatnonzero((filt != want).any(axis=1))[:5])
        if not unordered:
            pblocked, pfilt = nr.shadow_rays(scene, o, d, limit)
            assert not pblocked.any() and np.array_equal(pfilt.astype(F32).view(np.uint32), want.view(np.uint32)), what


# ---------------------------------------------------------------- frames ----------------------------------------------------------------------

def _camera(name):
    """stack_cases.frame_camera: next to the first rung, across the ladder (tests/test_stack_spill.py: the primary rays' reach with f32 sort keys)."""
    return sc.frame_camera(name)


def _render(scene, p):
    img = np.empty((p.height, p.width, 3), F32)
    abi.check(abi.load_hip_lib().nrays_render(scene.device_handle(), C.byref(p), img.ctypes.data_as(C.POINTER(C.c_float))))
    st = nr.get_stats(scene)
    return img, tuple(getattr(st, k) for k in RAY_CLASSES)


@pytest.mark.parametrize("name", ["a_rotated", "b_alpha", "c_tlas", "d_planes", "e_hair"])
def test_frames_down_the_ladder_are_the_oracles(gpu, monkeypatch, name):
    """64 x 64, k_primary's stack and the staged path's: two thirds of the pixels walk the chain to its end on their primary ray, the others leave
    the scene at once (proved on the CPU with f32 sort keys).  The megakernel's frame within the north star's 1e-4 of the oracle's with the same
    ray classes; the staged path, with lane refill and without, bit-identical to the megakernel."""
    p, _ = su.camera_params(_camera(name), 64, 64)
    frames = {}
    for wf, refill in (("0", "2"), ("1", "2"), ("1", "0")):
        monkeypatch.setenv("NRAYS_WAVEFRONT", wf)
        monkeypatch.setenv("NRAYS_WF_REFILL", refill)
        scene = sc.make_scene(name)
        frames[(wf, refill)] = _render(scene, p)
    img, counts = frames[("0", "2")]
    want, ost = oracle.render(scene.descriptor, p, 4)
    err = float(np.abs(img - want).max())
    print("%s: max |hip - oracle| = %.3g, classes %s, %.2f of the pixels hit" % (name, err, counts, (want != np.array(sc.BACKGROUND, F32)).any(axis=2).mean()))
    assert err <= 1e-4
    assert counts == tuple(getattr(ost, k) for k in RAY_CLASSES)
    assert 0.1 < (want != np.array(sc.BACKGROUND, F32)).any(axis=2).mean() < 0.98
    for key in (("1", "2"), ("1", "0")):
        assert np.array_equal(frames[key][0].view(np.uint32), img.view(np.uint32)), key
        assert frames[key][1] == counts, key


def test_bounces_off_the_ladder_are_the_oracles_and_repeat(gpu):
    """Scene (f): the rungs reflect and refract, max_depth 2.  The eye stands in front of both kites, so the first rungs are hit at once and the
    refraction rays that go on from them (k_bounce's queries) start next to the first rung and walk the chain to its end as well (CPU proof).
    Within 1e-4 of the oracle, the same ray classes, and four renders of one handle identical."""
    p, _ = su.camera_params(_camera("f_bounce"), 64, 64, max_depth=2)
    scene = sc.make_scene("f_bounce")
    runs = [_render(scene, p) for _ in range(4)]
    want, ost = oracle.render(scene.descriptor, p, 4)
    err = float(np.abs(runs[0][0] - want).max())
    print("f_bounce: max |hip - oracle| = %.3g, classes %s" % (err, runs[0][1]))
    assert err <= 1e-4
    assert runs[0][1] == tuple(getattr(ost, k) for k in RAY_CLASSES) and runs[0][1][1] > 0 and runs[0][1][2] > 0
    for img, counts in runs[1:]:
        assert np.array_equal(img.view(np.uint32), runs[0][0].view(np.uint32)) and counts == runs[0][1]


# ---------------------------------------------------------------- an answer that depends on every entry ----------------------------------------

def test_a_shadow_ray_through_transparent_rungs_multiplies_every_one(gpu, unordered):
    """Scene (g): 121 one-triangle nodes, each transparent to shadow rays and tinted by powers of two.  The shadow TLAS is the chain (its walk
    passes the LDS part, tests/test_stack_spill.py), a BLAS's sentinel lies on top of it, and the filter is the product over EVERY rung the ray
    crosses within max_toi, exact in any order: an entry lost, doubled or taken from another lane changes it.  Bit for bit oracle.shadow's,
    unbounded and with max_toi at a multiple of the first hit's distance; closest hits name the rung as the node."""
    o, d, hit, out, prim = sc.expected("g_rungs")
    scene = sc.make_scene("g_rungs")
    desc = scene.descriptor
    assert _flags(scene)[0] & 7 == 6
    got = nr.closest_hits(scene, o, d, unordered=unordered)
    assert np.array_equal(got.node, np.where(hit, out[:, 7], -1).astype(np.int32)) and np.array_equal(got.toi[hit], out[hit, 0])
    rng = np.random.default_rng(77)
    first = np.where(hit, out[:, 0], 1.0)
    seen = set()
    for what, limit in (("unbounded", np.full(len(o), DBL_MAX)), ("a few rungs", first * rng.choice([1.0, 3.0, 70.0, 5000.0, 1e9], len(o)))):
        want = np.ones((len(o), 3), F32)
        for i in np.flatnonzero(hit):
            f = oracle.shadow(desc, o[i], d[i], limit[i])
            assert f is not None
            want[i] = f
        lit, filt = nr.intersects_rays(scene, np.array(o), np.array(d), np.array(limit), unordered=unordered)
        assert lit.all(), what
        assert np.array_equal(filt.view(np.uint32), want.view(np.uint32)), (what, np.flatnonzero((filt != want).any(axis=1))[:5])
        if not unordered:
            pblocked, pfilt = nr.shadow_rays(scene, o, d, limit)
            assert not pblocked.any() and np.array_equal(pfilt.astype(F32).view(np.uint32), want.view(np.uint32)), what
        seen |= set(map(tuple, want.tolist()))
    print("g_rungs: %d different filters, the darkest %g" % (len(seen), min(min(s) for s in seen)))
    assert len(seen) > 40 and min(min(s) for s in seen) < 2.0 ** -20     # (dozens of factors in one product)


# ---------------------------------------------------------------- the composite calls ---------------------------------------------------------
# Each sets up a Stack of its own.  Held to the bit-equalities of their own test files, as compositions of closest_hits / intersects_rays /
# trace_rays, which the tests above pin to the brute force; the points and directions are stack_cases.composite_case's (reach: test_stack_spill.py).

def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("name", ["a_rotated", "b_alpha"])
def test_occlusion_points_is_the_fold_of_intersects_rays(gpu, name):
    from tests.test_occlusion_gpu import reference
    p, nm, L, keys = sc.composite_case(name)
    scene = sc.make_scene(name)
    for max_toi in (float("inf"), 3.0):
        want_f, want_o = reference(scene, p, nm, L, None, 0.0, max_toi, keys)
        got = nr.occlusion_points(scene, p, nm, L, None, 0.0, max_toi, keys=keys)
        assert np.array_equal(_bits(got.filter), _bits(want_f)) and np.array_equal(got.open, want_o), max_toi
        assert want_o.sum() == want_o.size * len(L) if name == "b_alpha" else 0 < want_o.sum() < want_o.size * len(L)   # (a transparent ladder blocks nothing)
    if name == "b_alpha":
        assert ((want_f > 0.0) & (want_f < 1.0)).any()                     # the rungs' colour filters, not only open and blocked


@pytest.mark.parametrize("name,max_depth", [("a_rotated", 0), ("b_alpha", 1)])
def test_gather_points_and_gather_sh_points_are_folds_of_trace_rays(gpu, monkeypatch, name, max_depth):
    from tests.test_gather_gpu import ray_colours
    from tests.test_gather import fold
    monkeypatch.setenv("NRAYS_RAY_REORDER", "2")                            # (the hinted forms then reorder at this size too)
    p, nm, L, keys = sc.composite_case(name)
    scene = sc.make_scene(name)
    colours = ray_colours(scene, p, nm, L, None, 0.0, 1.0, max_depth, keys)
    bg = np.array(sc.BACKGROUND, F32)
    assert 0.2 < (colours == bg).all(axis=2).mean() < 0.9                   # rays that see the background and rays that hit
    want = fold(colours)
    for hinted in (False, True):
        got = nr.gather_points(scene, p, nm, L, None, 0.0, 1.0, max_depth, keys=keys, unordered=hinted)
        assert np.array_equal(_bits(got), _bits(want)), hinted
    _, rd = nr.occlusion_rays(p, nm, L, None, 0.0, keys)
    for bands in (1, 3):
        want_sh = nr.sh_fold_ref(rd, colours, bands)
        for hinted in (False, True):
            got = nr.gather_sh_points(scene, p, nm, L, None, 0.0, 1.0, max_depth, bands, keys=keys, unordered=hinted)
            assert np.array_equal(_bits(got), _bits(want_sh)), (bands, hinted)


def test_gather_maps_points_is_the_fold_of_closest_hits_and_the_sample_mirror(gpu):
    """The rungs carry uvs that name them (rung j: the strip u in [j / 128, (j + 1) / 128]): a wrong rung samples another texel."""
    from tests.test_gather_maps_gpu import reference, two_maps, with_mode
    p, nm, L, keys = sc.composite_case("a_rotated")
    scene = sc.make_scene("a_rotated")
    miss = (0.25, 1.5, -0.5)
    for max_toi in (float("inf"), 3.0):
        want_rgb, want_cnt, cls = reference(scene, p, nm, L, None, 0.0, max_toi, keys, with_mode(two_maps()), [1], miss)
        rgb, cnt = nr.gather_maps_points(scene, p, nm, L, two_maps(), [1], None, 0.0, max_toi, miss, keys=keys, want_counts=True)
        assert np.array_equal(_bits(rgb), _bits(want_rgb)) and np.array_equal(cnt, want_cnt), max_toi
        assert len(np.unique(cls)) >= 2 and len(np.unique(rgb, axis=0)) > 20


def test_shade_hits_is_trace_rays_on_an_opaque_phong_ladder(gpu):
    """trace(ray) = obj.rgb on a node that neither reflects nor refracts: shade_points at the closest hits gives trace_rays' colour.  The light
    stands next to the first rung, so Material::compute's shadow rays run back along the ladder from every rung that was hit; a quarter of them
    hold kLdsStack + 12 slots or more (tests/test_stack_spill.py).  Both sides are device traversals: this shows that k_shade_points' own Stack
    and region give what k_trace_rays' give, not that either is right — a fault both share shows in the tests against the brute force."""
    from tests.test_shade_points_gpu import same_values
    o, d, hit, out, prim = sc.expected("a_rotated")
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    scene = sc.phong_scene()
    hits = nr.closest_hits(scene, o, d)
    assert np.array_equal((hits.flags & 1) != 0, hit)
    got = nr.shade_hits(scene, o, d, hits)
    ref = nr.trace_rays(scene, o, d)
    assert same_values(got[hit, :3], ref[hit]) and (got[hit, 3] == 1.0).all() and (_bits(got[~hit]) == 0).all()
    assert len(np.unique(got[hit, :3], axis=0)) > 50                       # lit and shadowed points, not one flat colour


# ---------------------------------------------------------------- overlapping traces: a spill region each ------------------------------------

@pytest.mark.parametrize("depth", ["2", "3"])
def test_pipelined_frames_down_the_plates_are_the_direct_frames(gpu, depth):
    """NRAYS_PIPELINE=2: consecutive frames are traced on internal streams while their predecessors still run, two or three at a time, each with
    the spill region of its stream (pipe.spill[k]).  A pipelined frame's eye cannot stand next to the chain's deep end (stack_cases.plates_scene),
    so its primary rays stay inside the LDS part; the rays that go on through the half-transparent first plate (max_depth 2, inside the same
    trace kernel) hold kLdsStack + 12 slots or more behind a fifth of the pixels (tests/test_stack_spill.py, f32 sort keys).  Seven frames with
    pairwise different cameras, enqueued without a host synchronisation, bit for bit the direct path's (NRAYS_PIPELINE=0), the first of them
    within 1e-4 of the oracle with rays that went on; nrays_debug_pipeline_counts shows that they were pipelined.
    The hits' shadow rays run down the ladders through some eighty transparent plates each, past the LDS part by a few slots, and their filter
    has a factor per plate crossed.
    What this does not show: a build that hands every stream the region of stream 0 passes this test too.  Why is not established — frames
    this small may not overlap in time, and lanes that walk the same chain hold the same entries, so one trace overwriting another's changes
    little.  The test shows that frames whose traces use their spill regions are pipelined and equal the direct ones, no more."""
    import torch
    from tests.test_pipeline_depth_gpu import _enqueue, _fresh, _same, _settle
    lib = abi.load_hip_lib()
    w, h = sc.PLATES_SIZE
    frames = {}
    for pipeline in ("2", "0"):
        scene, cam = _fresh(sc.plates_scene, pipeline, depth)
        params = [su.camera_params(c, w, h, max_depth=2)[0] for c in sc.plates_cameras(7)]
        _settle(lib, scene, params[0], w, h)
        before = (C.c_uint64 * 4)(); abi.check(lib.nrays_debug_pipeline_counts(scene.device_handle(), before))
        outs = [torch.full((h, w, 3), -1.0, dtype=torch.float32, device="cuda") for _ in params]
        torch.cuda.synchronize()
        for p, o in zip(params, outs):
            _enqueue(lib, scene, p, o)
        torch.cuda.synchronize()
        after = (C.c_uint64 * 4)(); abi.check(lib.nrays_debug_pipeline_counts(scene.device_handle(), after))
        pipelined, direct = after[0] - before[0], after[1] - before[1]
        print("depth %s, NRAYS_PIPELINE=%s: %d frames pipelined, %d direct" % (depth, pipeline, pipelined, direct))
        assert (pipelined, direct) == ((len(params), 0) if pipeline == "2" else (0, len(params)))
        frames[pipeline] = [o.cpu().numpy() for o in outs]
        if pipeline == "0":
            want, ost = oracle.render(scene.descriptor, params[0], 4)
            assert np.abs(frames["0"][0] - want).max() <= 1e-4 and ost.rays_refraction > 0.3 * w * h
            assert 0.1 < (want != np.array(sc.BACKGROUND, F32)).any(axis=2).mean() < 0.5
        scene._release()
    for k in range(len(frames["0"])):
        _same(frames["2"][k], frames["0"][k], "frame %d" % k)
        for j in range(k):
            assert (frames["0"][k].view(np.uint32) != frames["0"][j].view(np.uint32)).any(), "frames %d and %d are the same picture" % (j, k)
