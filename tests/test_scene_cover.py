"""Both TLASes of a flattened scene, from the host builder: tests/scene_cover.py (the statements S1 .. S8) on the dumps tests/scene_dump_shim.cpp takes of the named
scenes of tests/scene_cover_cases.py — bare roots, shapes resting on the coordinate planes in every rotation of a named set, a merged group with a member's faces at the
planes, a scene where device-built (here: the shim's fake builder) and host-built BLASes, an untransformed group, planes, a mesh without triangles and never-opaque
nodes coexist, and 300 instances in TLASes several levels deep.  tests/test_scene_cover_gpu.py runs the same on the device's own arrays and adds rays.  No GPU.

Then nine edits of a DUMP, each of which the validator must name by the statement it breaks.  Every edit is made consistent with the statements checked before the
one it aims at (an any-hit flag is set in the instance, its link and its leaf tag, so that S2 holds and S6 has to see it).  Two of them say something about the
product: a leaf box moved INWARD by one f32 step still contains its node's reference AABB and geometry, because world_box rounds outward and then steps once more — S7
and S8 cannot see one step, S3 does where the face is an extreme of its parent; two steps are S7's."""
import copy

import numpy as np
import pytest

from tests import scene_cover as sv
from tests import scene_cover_cases as cc

F32 = np.float32


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return cc.HostDump(tmp_path_factory.mktemp("scene_dump_shim"))


_dumps = {}


def dump_of(host, name):
    if name not in _dumps:
        _dumps[name] = host.dump(cc.case(name)[1], cc.build_min(name))
    return copy.deepcopy(_dumps[name])


def validated(host, name, dump=None):
    nodes, _, ref = cc.case(name)
    return sv.validate(dump if dump is not None else dump_of(host, name), nodes, ref)


@pytest.mark.parametrize("name", cc.NAMES)
def test_both_tlases_hold_and_cover_every_node(host, name):
    rep = validated(host, name)
    print(sv.line(name, rep))
    assert not rep["violations"]


def test_the_scenes_are_what_their_names_say(host):
    d = dump_of(host, "empty")
    assert d["closest_root"] == d["shadow_root"] == sv.EMPTY and len(d["nodes"]) == 0
    for name in ("one_ball", "one_triangle"):
        d = dump_of(host, name)
        assert d["closest_root"] < 0 and d["shadow_root"] < 0 and len(d["nodes"]) == 0 and len(d["instances"]) == 1
    rep = validated(host, "resting")
    assert rep["instances"] == [5 * len(cc.ROTATIONS) + 1] * 2 and len(cc.ROTATIONS) == 36
    nodes = cc.case("resting")[0]
    named = [n for n in nodes if n.geometry.kind == sv.CAPSULE and n.transform.axis_angle == cc.CAPSULE_ROTATION]
    assert len(named) == 1 and named[0].geometry.params[:2] == (cc.CAPSULE_HALF_HEIGHT, cc.CAPSULE_RADIUS)
    ref = cc.case("resting")[2]
    assert (np.abs(ref[:-1, :3]) <= 1e-15).all()                       # every minimum of every resting shape within 1e-15 of its coordinate plane
    # merged: one BLAS of three nodes for closest hits; for shadow rays an any-hit BLAS of the opaque node and one BLAS per transparent node
    d, rep = dump_of(host, "merged"), validated(host, "merged")
    assert (np.abs(cc.case("merged")[2][0, :3]) <= 1e-15).all()
    inst, sinst = (np.frombuffer(d[k].tobytes(), sv.INSTANCE) for k in ("instances", "shadow_instances"))
    assert rep["under"][0] == {0: [0, 1, 2]} and inst[0]["node_id"] == -1
    assert sorted(rep["under"][1].values()) == [[0], [1], [2]]
    assert sorted((int(i["node_id"]), bool(i["flags"] & sv.INST_ANY_HIT)) for i in sinst) == [(0, True), (1, False), (2, False)]
    # mixed: both builders, the rebase, an untransformed group, two planes
    d, rep = dump_of(host, "mixed"), validated(host, "mixed")
    assert 0 < d["dev_nodes"] < len(d["nodes"]) - sum(rep["tlas_nodes"]) and 0 < d["dev_tris"] < len(d["tris"]) and len(d["planes"]) == 2 and not d["bounded"]
    inst = np.frombuffer(d["instances"].tobytes(), sv.INSTANCE)
    assert ((inst["flags"] & sv.INST_NO_XFORM != 0) & (inst["kind"] == sv.TRIMESH)).sum() == 1
    rep = validated(host, "many")
    assert min(rep["tlas_depth"]) >= 3 and rep["instances"] == [300, 300]


def test_too_small_a_buffer_reports_the_sizes(host):
    from nrays_amd import abi
    import ctypes as C
    d = abi.NraysSceneDump()
    scene = cc.case("mixed")[1]
    assert host.lib.scene_dump_host(scene.descriptor.pointer(), cc.GPU_BUILD_MIN, C.byref(d)) == abi.ERR_BAD_ARG
    full = dump_of(host, "mixed")
    assert (d.num_nodes, d.num_tris, d.num_instances, d.num_shadow_instances, d.num_planes, d.num_scene_nodes) == (
        len(full["nodes"]), len(full["tris"]), len(full["instances"]), len(full["shadow_instances"]), 2, len(cc.case("mixed")[0]))
    assert d.closest_root == full["closest_root"] and d.dev_nodes == full["dev_nodes"]


@pytest.mark.parametrize("name", cc.RAY_SCENES)
def test_the_face_rays_rarely_meet_two_nodes_at_one_distance(name):
    """The rays of tests/test_scene_cover_gpu.py, by the oracle alone: a few thousand a scene, every (step, component) pair at every scene, at most 1 % of them with two
    nodes at the same toi (those are compared on hit and toi only), hits and misses both present, and a ray one step below its distance never blocked."""
    e = cc.expected(name)
    n = len(e["o"])
    print("%s: %d rays, %.1f %% hit, %.1f %% hit the node they were aimed at, %d with two nodes at one distance, %.1f %% blocked at the hit's distance" % (
        name, n, 100 * e["hit"].mean(), 100 * (e["node"] == e["aimed"]).mean(), e["tie"].sum(), 100 * e["blocked"]["at"].mean()))
    assert 2000 <= n <= 5000 and e["tie"].mean() <= 0.01
    assert 0.1 < e["hit"].mean() and (e["node"] == e["aimed"]).sum() >= 30
    assert not e["blocked"]["below"].any() and np.array_equal(e["blocked"]["at"], e["blocked"]["above"]) and e["blocked"]["at"].any()
    in_plane = (e["d"][np.arange(n), e["face"] % 3] == 0.0)
    assert in_plane.sum() >= n // 8 and (np.abs(e["d"][np.arange(n), e["face"] % 3]) == 1e-300).sum() >= n // 5


# ---- the mutants -------------------------------------------------------------------------------------------------------------------

def refs_of(d):
    return d["nodes"].view(np.int32)[:, 8:12]


def box_columns(k):
    """Columns of child k's six faces in a node's 32 floats: lower x, y, z, upper x, y, z."""
    return [4 * s + k for s in sv.LO + sv.HI]


def instances(d, key):
    return d[key].view(sv.INSTANCE).reshape(-1)


def leaf_slot(d, tlas_nodes, index):
    """(node, child) of the TLAS leaf of instance `index`."""
    refs = refs_of(d)
    for n in tlas_nodes:
        for k in range(4):
            r = int(refs[n, k])
            if r < 0 and r != sv.EMPTY and (~r & 0xffffffff) >> 3 == index:
                return n, k
    raise KeyError(index)


def expect(host, name, dump, statement):
    with pytest.raises(sv.Violation) as e:
        validated(host, name, dump)
    print(e.value)
    assert e.value.statement == statement, e.value


def extreme_leaf_face(d, tlas_nodes, want_leaf):
    """A (node, child, column, inward step) whose face alone is the extreme of the node's children on that side: moving it inward changes the node's union."""
    refs, nodes = refs_of(d), d["nodes"]
    for n in tlas_nodes:
        real = [k for k in range(4) if refs[n, k] != sv.EMPTY]
        for k in real:
            if (refs[n, k] < 0) != want_leaf:
                continue
            for j, col in enumerate(box_columns(k)):
                others = [nodes[n, box_columns(o)[j]] for o in real if o != k]
                v = nodes[n, col]
                if others and (v < min(others) if j < 3 else v > max(others)):
                    return n, k, col, F32(np.inf) if j < 3 else F32(-np.inf)
    raise AssertionError("no such face")


def test_a_leaf_box_moved_inward_by_one_step(host):
    d = dump_of(host, "mixed")
    rep = validated(host, "mixed")
    n, k, col, toward = extreme_leaf_face(d, rep["tlas_node_ids"][0][1:], True)       # (below the root: the root's own union is compared with the bounds)
    d["nodes"][n, col] = np.nextafter(d["nodes"][n, col], toward)
    expect(host, "mixed", d, "S3")


def test_a_bare_roots_box_two_steps_inward_leaves_the_reference_aabb_outside(host):
    """One step inward is what world_box's extra step pays for; the second one is missing from the box."""
    d = dump_of(host, "one_ball")
    one = d["bounds_mn"].copy()
    one[0] = np.nextafter(one[0], F32(np.inf))
    d["bounds_mn"] = one
    validated(host, "one_ball", copy.deepcopy(d))
    two = one.copy()
    two[0] = np.nextafter(two[0], F32(np.inf))
    d["bounds_mn"] = two
    expect(host, "one_ball", d, "S7")


def test_an_inner_box_shrunk_by_one_step(host):
    d = dump_of(host, "many")
    rep = validated(host, "many")
    n, k, col, toward = extreme_leaf_face(d, rep["tlas_node_ids"][1], False)
    inner = int(refs_of(d)[n, k])
    assert inner >= 0
    d["nodes"][n, col] = np.nextafter(d["nodes"][n, col], toward)
    expect(host, "many", d, "S3")


def test_a_shadow_instance_removed(host):
    """The instance leaves the list, its leaf becomes an absent child, later leaves and the planes are renumbered; the leaf is one whose box lies strictly inside the
    union of its siblings, so the tree is still a well-formed TLAS (S1 .. S4 hold) — of one node too few."""
    d = dump_of(host, "mixed")
    rep = validated(host, "mixed")
    tlas = rep["tlas_node_ids"][1]
    refs, nodes = refs_of(d), d["nodes"]
    n_leaf = len(d["shadow_instances"]) - len(d["shadow_planes"])
    found = None
    for index in range(n_leaf):
        n, k = leaf_slot(d, tlas, index)
        sib = [o for o in range(4) if o != k and refs[n, o] != sv.EMPTY]
        if not sib:
            continue
        mine = nodes[n, box_columns(k)]
        rest = np.stack([nodes[n, box_columns(o)] for o in sib])
        if (mine[:3] > rest[:, :3].min(axis=0)).all() and (mine[3:] < rest[:, 3:].max(axis=0)).all():
            found = (index, n, k)
            break
    assert found, "no shadow leaf strictly inside its siblings' union"
    index, n, k = found
    nodes[n, box_columns(k)[:3]] = sv.FLT_MAX
    nodes[n, box_columns(k)[3:]] = -sv.FLT_MAX
    refs[n, k] = sv.EMPTY
    for m in tlas:
        for c in range(4):
            r = int(refs[m, c])
            if r < 0 and r != sv.EMPTY:
                v = ~r & 0xffffffff
                if v >> 3 > index:
                    refs[m, c] = ~(((v >> 3) - 1) << 3 | (v & 7))
    d["shadow_instances"] = np.delete(d["shadow_instances"], index, axis=0)
    d["shadow_links"] = np.delete(d["shadow_links"], index, axis=0)
    d["shadow_planes"] = d["shadow_planes"] - 1
    expect(host, "mixed", d, "S6")


def test_any_hit_on_the_half_transparent_node(host):
    d = dump_of(host, "merged")
    inst = instances(d, "shadow_instances")
    index = int(np.flatnonzero(inst["node_id"] == 1)[0])           # the alpha = 0.5 member
    assert cc.case("merged")[0][1].alpha == 0.5
    inst["flags"][index] |= sv.INST_ANY_HIT
    d["shadow_links"][index, 1] |= sv.INST_ANY_HIT
    n, k = leaf_slot(d, [d["shadow_root"]], index)
    refs_of(d)[n, k] = ~((~int(refs_of(d)[n, k]) & 0xffffffff) | sv.LEAF_ANY_HIT)
    expect(host, "merged", d, "S6")


def test_the_tag_bits_of_a_leaf_cleared(host):
    d = dump_of(host, "merged")
    refs = refs_of(d)
    n = d["shadow_root"]
    k = [c for c in range(4) if refs[n, c] != sv.EMPTY and ~int(refs[n, c]) & 7][0]
    refs[n, k] = ~((~int(refs[n, k]) & 0xffffffff) & ~7)
    expect(host, "merged", d, "S2")


def test_two_links_swapped(host):
    d = dump_of(host, "mixed")
    inst = instances(d, "instances")
    a, b = [int(i) for i in np.flatnonzero(inst["kind"] == sv.TRIMESH)[:2]]
    assert tuple(d["links"][a]) != tuple(d["links"][b])
    d["links"][[a, b]] = d["links"][[b, a]]
    expect(host, "mixed", d, "S2")


def test_a_plane_index_off_by_one(host):
    d = dump_of(host, "mixed")
    d["planes"][0] -= 1
    expect(host, "mixed", d, "S4")


def test_host_built_refs_left_unrebased(host):
    """What link_scene adds to everything the host built when device-built BLASes take the front of the arrays, taken away again from the host-built BLASes: their
    nodes' child and leaf refs, and the roots in the instances and links that name them (the TLASes stay, or S1 would speak first)."""
    d = dump_of(host, "mixed")
    rep = validated(host, "mixed")
    dn, dt = d["dev_nodes"], d["dev_tris"]
    tlas = set(rep["tlas_node_ids"][0]) | set(rep["tlas_node_ids"][1])

    def back(r):
        r = int(r)
        if r == sv.EMPTY:
            return r
        if r >= 0:
            return r - dn if r >= dn else r
        v = ~r & 0xffffffff
        return ~(((v >> 3) - dt) << 3 | (v & 7)) if v >> 3 >= dt else r
    refs = refs_of(d)
    moved = 0
    for n in range(dn, len(refs)):
        if n not in tlas:
            for k in range(4):
                moved += back(refs[n, k]) != refs[n, k]
                refs[n, k] = back(refs[n, k])
    for ikey, lkey in (("instances", "links"), ("shadow_instances", "shadow_links")):
        inst = instances(d, ikey)
        for i in np.flatnonzero(inst["kind"] == sv.TRIMESH):
            moved += back(inst["blas_root"][i]) != inst["blas_root"][i]
            inst["blas_root"][i] = back(inst["blas_root"][i])
            d[lkey][i, 0] = inst["blas_root"][i]
    assert moved > 2
    expect(host, "mixed", d, "S5")


def test_a_merged_instance_named_after_its_first_node(host):
    d = dump_of(host, "merged")
    inst = instances(d, "instances")
    assert inst["node_id"][0] == -1
    inst["node_id"][0] = 0
    expect(host, "merged", d, "S5")
