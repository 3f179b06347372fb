"""The traversal stack beyond its LDS slots, the part that needs no GPU: the ladder scenes of tests/stack_cases.py DO make a lane hold more
than kLdsStack entries.  The host builder (nrays_amd/csrc/bvh_build.cpp compiled by the host compiler, tests/bvh_build_shim.cpp) builds the
ladder's tree, stack_cases.simulate walks it in traverse()'s two visiting orders, and the conditions below are what keeps
tests/test_stack_spill_gpu.py from being vacuous: in every scene and in both orders a quarter of the rays go 12 slots beyond the LDS part,
a tenth stay at 4, every 64 consecutive rays mix both, and no ray exceeds the sizing rule of derive_scene_facts.  The oracle is checked
against itself on the same rays (BVT == brute force), and the measured reach is the record in profiles/stack_spill_reach.json."""
import json
import os

import numpy as np
import pytest

import nrays_amd as nr
import oracle
from tests import stack_cases as sc

F32 = np.float32


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return sc.BuildShim(tmp_path_factory.mktemp("bvh_build_shim"))


@pytest.fixture(scope="module")
def trees(shim):
    return sc.trees(shim)


@pytest.fixture(scope="module")
def tree(trees):
    return trees["ladder"]


# ---------------------------------------------------------------- the simulator itself -----------------------------------------------------------

def _hand_tree():
    """Six nodes, ten one-triangle leaves A .. J (triangle = its letter's index), every box [x0, x1] x [0, 1] x [0, 1]:
        node 0: A [10, 11]   node 1 [0, 9]   B [12, 13]   node 2 [20, 30]
        node 1: node 3 [0, 4]   node 4 [5, 9]
        node 2: I [20, 25]   J [26, 30]
        node 3: C [0, 1]   D [2, 3]   E [3.5, 4]
        node 4: F [5, 6]   node 5 [7, 9]
        node 5: G [7, 8]   H [8.5, 9]
    Every triangle sits in the corner y + z >= 1.5 of its box, except C's, which covers the rays' y = z = 0.25 at x = 0.5."""
    big = float(np.finfo(F32).max)
    leaf = lambda k: ~(k << 3)  # noqa: E731
    A, B, C_, D, E, F, G, H, I, J = range(10)
    spec = [[(10, 11, leaf(A)), (0, 9, 1), (12, 13, leaf(B)), (20, 30, 2)],
            [(0, 4, 3), (5, 9, 4)],
            [(20, 25, leaf(I)), (26, 30, leaf(J))],
            [(0, 1, leaf(C_)), (2, 3, leaf(D)), (3.5, 4, leaf(E))],
            [(5, 6, leaf(F)), (7, 9, 5)],
            [(7, 8, leaf(G)), (8.5, 9, leaf(H))]]
    nodes = np.zeros((6, 8, 4), F32)
    refs = np.full((6, 4), sc.EMPTY, np.int32)
    nodes[:, [0, 4, 3]] = big; nodes[:, [1, 6, 7]] = -big            # absent children: inverted boxes
    for n, children in enumerate(spec):
        for k, (x0, x1, ref) in enumerate(children):
            nodes[n, 0, k], nodes[n, 1, k] = x0, x1                  # x planes: slots 0 / 1
            nodes[n, 4, k] = nodes[n, 3, k] = 0.0                    # lower y, z: slots 4 / 3
            nodes[n, 6, k] = nodes[n, 7, k] = 1.0                    # upper y, z: slots 6 / 7
            refs[n, k] = ref
    nodes[:, 2] = refs.view(F32)
    mid = {A: 10.5, B: 12.5, C_: 0.5, D: 2.5, E: 3.75, F: 5.5, G: 7.5, H: 8.75, I: 22.0, J: 28.0}
    tris = np.array([[[mid[t], 1, 0.5], [mid[t], 0.5, 1], [mid[t], 1, 1]] for t in range(10)], np.float64)
    tris[C_] = [[0.5, 0, 0], [0.5, 1, 0], [0.5, 0, 1]]
    return dict(nodes=nodes.reshape(6, 32), tri=np.arange(10, dtype=np.uint32), root=0, depth=3), tris


def test_the_simulator_on_a_tree_worked_out_by_hand():
    """Heights include the bottom marker and the sentinel (2 slots).  With C's triangle out of the way (`miss`):
    closest order, ray +x from x = -1: node 0 sorts node 1 (entry 1), A (11), B (13), node 2 (21) and defers three -> 5; node 1 defers node 4 -> 6;
      node 3 defers E and D -> 8, the most: what follows (C, D, E, node 4 with node 5 deferred, F, node 5 with H deferred ...) stays below.
    closest order, ray -x from x = 40: node 0 sorts node 2 (10), B (27), A (29), node 1 (31) -> 5; node 2 defers I -> 6; after J, I, B, A the stack
      is empty and node 1 -> node 4 -> node 5 rebuild it to node 3, F, G -> 5: the most is 6.
    shadow order, ray +x: node 0 visits its last child node 2 and pushes A, node 1, B -> 5; node 2 pushes I -> 6; J, I, B; node 1 pushes node 3 -> 4
      (A, node 3); node 4 pushes F -> 5; node 5 pushes G -> 6; H, G, F; node 3 pushes C, D -> 5: the most is 6.
    shadow order, ray +x, distance bound 7.5: node 0 enters node 1 only -> 2; node 1 pushes node 3 -> 3; node 4 enters F only (node 5 starts at 8);
      node 3 pushes C, D -> 4.
    With C's triangle in the way the closest-order ray +x reaches its 8 before C is tested, finds C (triangle 2) and culls the rest; the
    any-hit shadow ray meets C last of all and has been at 6 by then; bounded by 1.4 it never reaches C's distance 1.5."""
    t, tris = _hand_tree()
    miss = tris.copy(); miss[2] = [[0.5, 1, 0.5], [0.5, 0.5, 1], [0.5, 1, 1]]
    fwd = (np.array([[-1.0, 0.25, 0.25]]), np.array([[1.0, 0.0, 0.0]]))
    back = (np.array([[40.0, 0.25, 0.25]]), np.array([[-1.0, 0.0, 0.0]]))
    run = lambda tr, ray, **kw: tuple(int(a[0]) for a in sc.simulate(t, tr, ray[0], ray[1], **kw))  # noqa: E731
    assert run(miss, fwd) == (8, -1)
    assert run(miss, back) == (6, -1)
    assert run(miss, fwd, shadow=True) == (6, -1)
    assert run(miss, fwd, shadow=True, limit=7.5) == (4, -1)
    assert run(tris, fwd) == (8, 2)
    assert run(tris, fwd, key32=True) == (8, 2)
    assert run(tris, fwd, shadow=True, any_hit=True) == (6, 2)
    assert run(tris, fwd, shadow=True, any_hit=True, limit=1.4) == (2, -1)   # node 0 -> node 1 -> node 3 -> C, one child in reach each time: nothing pushed
    assert run(tris, fwd, shadow=True, any_hit=False) == (6, 2)
    # a direction without a zero component meets the absent children's inverted boxes in the slab arithmetic: same walk, same heights
    tilt = (fwd[0], np.array([[1.0, 1e-9, -1e-9]]))
    assert run(miss, tilt) == (8, -1) and run(tris, tilt) == (8, 2) and run(miss, tilt, shadow=True) == (6, -1) and run(tris, tilt, shadow=True, any_hit=True) == (6, 2)
    # several rays at once keep their own stacks
    o = np.concatenate([fwd[0], back[0], fwd[0]]); d = np.concatenate([fwd[1], back[1], fwd[1]])
    h, f = sc.simulate(t, tris, o, d)
    assert h.tolist() == [8, 6, 8] and f.tolist() == [2, 2, 2]


# ---------------------------------------------------------------- the ladder and its tree ---------------------------------------------------------

def test_the_ladder_is_f32_exact_and_its_tree_a_deep_chain(tree):
    pts, idx, x, flipped = sc.ladder()
    assert 100 <= len(idx) <= 150 and 20 <= flipped.sum() <= len(idx) // 2
    assert np.abs(np.log2(np.abs(x))).max() <= 60
    L = sc.lds_stack()
    assert tree["root"] == 0 and sorted(tree["tri"].tolist()) == list(range(len(idx)))
    # three deferred children per level must be able to pass the LDS part by 12 slots; the sizing rule has to allocate HBM slots for this depth
    assert 3 * tree["depth"] + 2 >= L + 12, tree["depth"]
    assert sc.need(tree["depth"]) > L
    for name, make in sc.PLACEMENTS.items():
        R, T = sc.rotation(make())
        assert R[0, 1] == R[0, 2] == R[1, 0] == R[2, 0] == 0.0 and T[0] == 0.0, name   # x, up to 2^60, never reaches y and z
    print("ladder: %d rungs (%d flipped), %d nodes, depth %d, need %d slots, kLdsStack %d" % (len(idx), flipped.sum(), len(tree["nodes"]), tree["depth"], sc.need(tree["depth"]), L))


def _conditions(heights, L):
    """The four conditions on one scene and order; returns what fails."""
    bad = []
    if not (heights >= L + 12).mean() >= 0.25:
        bad.append("only %.3f of the rays reach %d slots" % ((heights >= L + 12).mean(), L + 12))
    if not (heights <= 4).mean() >= 0.10:
        bad.append("only %.3f of the rays stay at 4 slots" % (heights <= 4).mean())
    for i in range(0, len(heights), 64):
        b = heights[i:i + 64]
        if not ((b >= L + 12).any() and (b <= L - 4).any()):
            bad.append("rays %d .. %d do not mix LDS-only and HBM lanes" % (i, i + len(b) - 1))
            break
    return bad


@pytest.mark.parametrize("name", sc.SCENES)
def test_every_scene_reaches_the_hbm_slots_in_both_orders(trees, name):
    """Closest-hit order and shadow order (unbounded; ending at the first hit where the ladder is opaque), the sort on f64 keys and on keys
    rounded to f32 as the device holds them: the conditions hold either way."""
    L = sc.lds_stack()
    nodes, ladders = sc.scene_nodes(name)
    planes = sum(isinstance(n.geometry, nr.Plane) for n in nodes)
    for shadow in (False, True):
        for key32 in ((False, True) if not shadow else (False,)):   # (the shadow order does not sort)
            h = sc.reach(trees, name, shadow, key32=key32)
            assert len(h) == sc.N_RAYS and sc.N_RAYS % 256 != 0 and sc.N_RAYS > 8 * 256
            print("%s %s%s: %.3f at %d slots or more, %.3f beyond the LDS part, %.3f at 4 or fewer, most %d" % (
                name, "shadow" if shadow else "closest", " (f32 keys)" if key32 else "", (h >= L + 12).mean(), L + 12, (h > L).mean(), (h <= 4).mean(), h.max()))
            assert not _conditions(h, L), (name, shadow, key32, _conditions(h, L))
            assert h.max() <= sc.need(trees["ladder"]["depth"], planes), (h.max(), sc.need(trees["ladder"]["depth"], planes))   # the sizing rule against real use


def test_the_rung_per_node_scene_passes_the_lds_part_in_shadow_order(trees):
    """Scene (g), every rung a transparent node of its own: in closest-hit order its one shared BLAS is the ladder's tree and the conditions hold
    as above; its shadow TLAS (one instance per rung, leaves of one) keeps the long child in slot 0, which the shadow order visits last, so the
    stack passes the LDS part by a few slots only.  What it reaches: a quarter of the rays beyond kLdsStack, a tenth at 4, both in every 64."""
    L = sc.lds_stack()
    for key32 in (False, True):
        assert not _conditions(sc.reach(trees, "g_rungs", False, key32=key32), L)
    h = sc.reach(trees, "g_rungs", True)
    print("g_rungs shadow: %.3f beyond the LDS part, %.3f at 4 or fewer, most %d" % ((h > L).mean(), (h <= 4).mean(), h.max()))
    assert (h > L).mean() >= 0.25 and (h <= 4).mean() >= 0.10
    assert all((b > L).any() and (b <= L - 4).any() for b in (h[i:i + 64] for i in range(0, len(h), 64)))
    assert h.max() <= sc.need(max(t["depth"] for t in trees.values()))


def test_a_short_ladder_fails_the_conditions(shim):
    """The conditions bite: 40 rungs give a chain the LDS part holds."""
    pts, idx, x, flipped = sc.ladder(kmin=-20, kmax=19)
    t = shim.build(pts, idx)
    tris = pts.astype(np.float64)[idx.astype(np.int64)]
    o, d = sc.ladder_rays(x, flipped, 1)
    for shadow in (False, True):
        h = sc.simulate(t, tris, o, d, shadow=shadow, any_hit=shadow)[0]
        assert _conditions(h, sc.lds_stack()), (shadow, h.max())


# ---------------------------------------------------------------- the oracle alone ---------------------------------------------------------------

@pytest.mark.parametrize("name", sc.ALL_SCENES)
def test_the_oracles_bvt_agrees_with_its_brute_force(name):
    o, d, hit, out, prim = sc.expected(name)
    bhit, bout = oracle.cast(sc.make_scene(name).descriptor, o, d)
    cls = sc.ray_classes()
    for c, cname in enumerate(sc.CLASSES):
        m = cls == c
        assert np.array_equal(bhit[m], hit[m]) and np.array_equal(bout[m & hit], out[m & hit]), cname
    _, ladders = sc.scene_nodes(name)
    on_ladder = hit & np.isin(out[:, 7].astype(np.int64), [ni for ni, _ in ladders]) if ladders else hit
    shares = [float(on_ladder[cls == c].mean()) for c in range(4)]
    print("%s: hit share by class %s, %d distinct rungs hit, %d hits with their rung named" % (name, ["%.2f" % s for s in shares], len(set(prim[prim >= 0].tolist())), (prim >= 0).sum()))
    assert all(0.2 < s < 0.95 for s in shares), shares
    assert len(set(prim[prim >= 0].tolist())) >= 30
    assert (prim[on_ladder] >= 0).mean() > 0.99                # (a one-rung node's own AABB gates in addition: knife edges only)


def test_the_two_ladders_of_the_tlas_scene_do_not_shade_each_other():
    """Scene (c): a ray made for one ladder meets nothing else before it — the reach simulated in that ladder alone is the reach in the scene."""
    o, d, hit, out, prim = sc.expected("c_tlas")
    _, ladders = sc.scene_nodes("c_tlas")
    _, _, which = sc.scene_rays("c_tlas")
    node = out[:, 7].astype(np.int64)
    for k, (ni, _) in enumerate(ladders):
        assert (node[hit & (which == k)] == ni).all()
    assert all((hit & (which == k)).mean() > 0.1 for k in range(len(ladders)))


# ---------------------------------------------------------------- the record --------------------------------------------------------------------

def test_the_recorded_reach_is_of_these_cases(shim):
    """profiles/stack_spill_reach.json (python -m tests.stack_cases rewrites it; DESIGN §3 quotes it): same constants, same scenes, and shares
    within a hundredth of what this machine measures (a rotation's sine may move a ray across an edge elsewhere)."""
    rec = json.load(open(os.path.join(sc.ROOT, "profiles", "stack_spill_reach.json")))
    now = sc.reach_record(shim)
    for key in ("lds_stack", "rungs", "flipped", "rays", "tree_nodes", "tree_depth", "need", "slot_bins", "rungs_tlas_nodes", "rungs_tlas_depth"):
        assert rec[key] == now[key], key
    assert set(rec["scenes"]) == set(sc.ALL_SCENES)
    for name in sc.ALL_SCENES:
        for order in ("closest", "shadow"):
            a, b = rec["scenes"][name][order], now["scenes"][name][order]
            for key in ("rays_beyond_lds", "rays_12_beyond", "rays_at_most_4", "blocks_beyond_lds", "blocks_mixed"):
                assert abs(a[key] - b[key]) <= 0.01, (name, order, key, a[key], b[key])
    for name in sc.SCENES:
        for order in ("closest", "shadow"):
            a = rec["scenes"][name][order]
            assert a["rays_12_beyond"] >= 0.25 and a["rays_at_most_4"] >= 0.10 and a["blocks_mixed"] == 1.0 and a["blocks_beyond_lds"] == 1.0


@pytest.mark.parametrize("name", ["a_rotated", "b_alpha"])
def test_the_composite_calls_rays_reach_the_hbm_slots(trees, name):
    """The rays occlusion_points, gather_points, gather_sh_points and gather_maps_points build at the points of stack_cases.composite_case: four
    of six directions run down the ladder, two away from it.  The conditions of the ray classes hold for them too, in closest-hit order (the
    gathers) and in shadow order (occlusion)."""
    L = sc.lds_stack()
    for shadow, key32 in ((False, False), (False, True), (True, False)):     # (the shadow order does not sort)
        h = sc.composite_reach(trees, name, shadow, key32=key32)
        print("%s composite rays, %s%s: %.3f at %d slots or more, %.3f at 4 or fewer, most %d" % (name, "shadow" if shadow else "closest", " (f32 keys)" if key32 else "", (h >= L + 12).mean(), L + 12, (h <= 4).mean(), h.max()))
        assert len(h) == 516 * 6 and not _conditions(h, L), _conditions(h, L)


def _frame_conditions(heights, size, L):
    """A frame's lanes are pixels of 8 x 8 packets, not consecutive rays: a quarter of the pixels at kLdsStack + 12 slots or more, a tenth at 4 or
    fewer, and packets that hold both kinds (they lie along the border between the two: eight at least)."""
    w, rows = size
    deep, shallow = (heights >= L + 12).reshape(rows, w), (heights <= L - 4).reshape(rows, w)
    packets = lambda m: m.reshape(rows // 8, 8, w // 8, 8).any(axis=(1, 3))  # noqa: E731
    return deep.mean() >= 0.25 and (heights <= 4).mean() >= 0.10 and (packets(deep) & packets(shallow)).sum() >= 8


@pytest.mark.parametrize("name", ["a_rotated", "b_alpha", "c_tlas", "d_planes", "e_hair", "f_bounce"])
def test_the_frames_primary_rays_reach_the_hbm_slots(trees, name):
    """The 64 x 64 frames of tests/test_stack_spill_gpu.py (k_primary and the staged path): their primary rays, walked with the sort keys rounded to
    f32 as the device holds them.  From an eye some units away every ray stays below kLdsStack under that rule (asserted: the camera must stand
    next to the first rung).  Scene (f) at max_depth 2: the rays that go on from the first hit in the same direction — what a refraction ray
    does up to its bend — start next to the first rung too (the eye of that scene stands in front of both kites) and hold kLdsStack + 12 slots or more."""
    L = sc.lds_stack()
    for key32 in (True, False):
        h, found, lo, ld = sc.frame_reach(trees, name, key32=key32)
        print("%s frame%s: %.3f of the pixels at %d slots or more, %.3f at 4 or fewer, most %d; %.2f hit, %d rungs" % (
            name, " (f32 keys)" if key32 else "", (h >= L + 12).mean(), L + 12, (h <= 4).mean(), h.max(), (found >= 0).mean(), len(set(found[found >= 0].tolist()))))
        assert _frame_conditions(h, sc.FRAME_SIZE, L)
        assert 0.1 < (found >= 0).mean() < 0.9 and len(set(found[found >= 0].tolist())) >= (1 if name == "f_bounce" else 4)
    pts, idx, _, _ = sc.ladder()
    tris = pts.astype(np.float64)[idx.astype(np.int64)]
    far = lo + np.array([6.0, 0.0, 0.0])                                      # the same directions from six units in front: what does NOT reach
    assert sc.simulate(trees["ladder"], tris, far, ld, key32=True)[0].max() <= L
    if name == "f_bounce":
        m = found >= 0
        toi = np.array([sc._tri_toi(tris[t:t + 1, 0], tris[t:t + 1, 1], tris[t:t + 1, 2], lo[i:i + 1], ld[i:i + 1])[0] for i, t in zip(np.flatnonzero(m), found[m])])
        on = lo[m] + ld[m] * (toi * (1.0 + 2.0 ** -40))[:, None]
        h2 = sc.simulate(trees["ladder"], tris, on, ld[m], key32=True)[0]
        print("f_bounce: rays going on from the first hit: %.3f at %d slots or more, most %d" % ((h2 >= L + 12).mean(), L + 12, h2.max()))
        assert (h2 >= L + 12).mean() >= 0.9


def test_shade_points_shadow_rays_reach_the_hbm_slots(trees):
    """The shadow rays Material::compute casts in stack_cases.phong_scene(), from the closest hits of scene a_rotated's rays to the light next to
    the first rung: an opaque rung ends such a ray, so fewer go deep than in the ray classes — a fifth at kLdsStack + 12 slots or more."""
    L = sc.lds_stack()
    h = sc.shade_shadow_reach(trees)
    print("shade_points' shadow rays: %.3f at %d slots or more, %.3f beyond the LDS part, most %d" % ((h >= L + 12).mean(), L + 12, (h > L).mean(), h.max()))
    assert (h >= L + 12).mean() >= 0.2 and (h <= 4).mean() >= 0.10


def test_the_plates_frame_walks_its_tlas_beyond_the_lds_part(shim):
    """The scene of the pipelined frames (no meshes: two ladders of 121 half-transparent cuboid plates, the TLAS holds both chains), walked with the
    sort keys rounded to f32, for the first and the last camera of the consecutive frames.  The primary rays stay inside the LDS part (asserted:
    the eye is nine units away).  The rays that go on from the first plate's back hold kLdsStack + 12 slots or more: a tenth of the frame's
    pixels at least, a twentieth behind each ladder, in 8 x 8 packets that also hold pixels of the background."""
    L = sc.lds_stack()
    w, rows = sc.PLATES_SIZE
    for cam in (sc.plates_cameras(7)[0], sc.plates_cameras(7)[-1]):
        tree, h, onward, found = sc.plates_reach(shim, key32=True, cam=cam)
        deep = onward >= L + 12
        per_ladder = [float((deep & (found // 121 == k)).mean()) for k in range(len(sc.PLATES_OFFSETS))]
        print("plates: TLAS depth %d; primary rays %d slots at most; rays that go on: %.3f of the pixels at %d slots or more (by ladder %s), most %d" % (
            tree["depth"], h.max(), deep.mean(), L + 12, per_ladder, onward.max()))
        assert h.max() <= L + 8
        assert 0.10 <= deep.mean() <= 0.45 and min(per_ladder) >= 0.05
        assert sc.need(tree["depth"]) > L and onward.max() <= sc.need(tree["depth"])
        packets = lambda m: m.reshape(rows // 8, 8, w // 8, 8).any(axis=(1, 3))  # noqa: E731
        assert (packets(deep.reshape(rows, w)) & packets((found < 0).reshape(rows, w))).sum() >= 8


def test_the_plates_shadow_rays_pass_the_lds_part(shim):
    """The shadow rays of the plates' frame (to a light far down each ladder, through transparent nodes only): most of them (half at least is asked) hold more than
    kLdsStack slots — the shadow order keeps the long child for last, so it is a few slots only, as in scene (g) — and its filter, a factor per
    plate crossed, depends on every entry it pops."""
    L = sc.lds_stack()
    h = sc.plates_shadow_reach(shim)
    print("plates' shadow rays: %d hits x %d lights, %.3f beyond the LDS part, most %d" % (h.shape[0], h.shape[1], (h > L).mean(), h.max()))
    assert h.shape[0] > 0.2 * sc.PLATES_SIZE[0] * sc.PLATES_SIZE[1] and (h > L).mean() >= 0.5
