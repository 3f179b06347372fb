"""Both TLASes of a flattened scene AS THE KERNELS READ THEM: tests/scene_cover.py (S1 .. S8) on nrays_debug_scene_dump, which copies the nodes, triangle records, instance
lists, links, plane lists and node AABBs back from device memory — the named scenes of tests/scene_cover_cases.py, `mixed` created under NRAYS_GPU_BUILD_MIN=16 so that
BLASes of the device builder and of the host builder coexist, a device-built BLAS feeds a node's local AABB and link_scene's rebase runs.

Then rays at every face of every node's reference AABB in `resting`, `merged` and `mixed` (scene_cover_cases.face_rays: in the face's plane and one f64 step beside it,
the direction's component on that axis 0, +-1e-300, +-2^-60 or ordinary), through nrays_cast_rays and nrays_intersects_rays (max_toi at the hit, one f64 step below and
above), in order and with NRAYS_RAYS_UNORDERED under NRAYS_RAY_REORDER=2, against the oracle's brute force: hit, toi, node, blocked.  Rays on which the oracle names two
nodes at one distance are compared on hit and toi only; they are at most 1 % of a scene's rays (tests/test_scene_cover.py checks that share without a GPU)."""
import numpy as np
import pytest

import nrays_amd as nr
from tests import scene_cover as sv
from tests import scene_cover_cases as cc

pytestmark = pytest.mark.gpu


def fresh_scene(name, monkeypatch):
    """A scene of its own (the switches are read when it is created); `mixed` with the device builder taking meshes from 16 triangles."""
    if cc.build_min(name):
        monkeypatch.setenv("NRAYS_GPU_BUILD_MIN", str(cc.build_min(name)))
    sc = nr.Scene(cc.case(name)[0], cc.lights(), cc.BACKGROUND)
    sc.device_handle()
    return sc


@pytest.mark.parametrize("name", cc.NAMES)
def test_the_devices_arrays_hold_and_cover_every_node(gpu, monkeypatch, name):
    nodes, _, ref = cc.case(name)
    sc = fresh_scene(name, monkeypatch)
    d = cc.device_dump(sc)
    rep = sv.validate(d, nodes, ref)
    print(sv.line(name, rep), " dev_nodes %d dev_tris %d of %d nodes %d triangle records" % (d["dev_nodes"], d["dev_tris"], len(d["nodes"]), len(d["tris"])))
    assert not rep["violations"]
    if name == "mixed":                                      # both builders, and the rebase between them
        assert 0 < d["dev_nodes"] < len(d["nodes"]) - sum(rep["tlas_nodes"]) and 0 < d["dev_tris"] < len(d["tris"])
    if name == "many":
        assert min(rep["tlas_depth"]) >= 3


def test_too_small_a_buffer_reports_the_sizes(gpu, monkeypatch):
    import ctypes as C
    from nrays_amd import abi
    sc = fresh_scene("merged", monkeypatch)
    d = abi.NraysSceneDump()
    assert abi.load_hip_lib().nrays_debug_scene_dump(sc.device_handle(), C.byref(d)) == abi.ERR_BAD_ARG
    assert b"too small" in abi.load_hip_lib().nrays_last_error()
    assert (d.num_instances, d.num_shadow_instances, d.num_planes, d.num_scene_nodes, d.num_tris) == (1, 3, 0, 3, 20 + 24 + 17 + 20 + 24 + 17)


@pytest.fixture(params=[False, True], ids=["ordered", "unordered"])
def unordered(request, monkeypatch):
    if request.param:
        monkeypatch.setenv("NRAYS_RAY_REORDER", "2")          # read when a scene is created: the reorder then runs at any batch size
    return request.param


@pytest.mark.parametrize("name", cc.RAY_SCENES)
def test_rays_at_the_faces_of_the_reference_aabbs(gpu, monkeypatch, name, unordered):
    e = cc.expected(name)
    o, d, hit, tie = e["o"], e["d"], e["hit"], e["tie"]
    print("%s: %d rays, %.1f %% hit, %.1f %% hit the node they were aimed at, %d with two nodes at one distance" % (
        name, len(o), 100 * hit.mean(), 100 * (e["node"] == e["aimed"]).mean(), tie.sum()))
    assert tie.mean() <= 0.01
    sc = fresh_scene(name, monkeypatch)
    got = nr.closest_hits(sc, np.array(o), np.array(d), unordered=unordered, want=())
    assert np.array_equal(got.node >= 0, hit), np.flatnonzero((got.node >= 0) != hit)[:5]
    other = hit & (got.toi != e["toi"])
    assert not other.any(), "%d of %d hits at another distance than the brute force's, e.g. ray %d (aimed at node %d face %d): %r, brute force %r on node %d" % (
        other.sum(), hit.sum(), np.flatnonzero(other)[0], e["aimed"][other][0], e["face"][other][0], got.toi[other][0], e["toi"][other][0], e["node"][other][0])
    assert np.isposinf(got.toi[~hit]).all()
    sure = hit & ~tie
    assert np.array_equal(got.node[sure], e["node"][sure]), np.flatnonzero(sure & (got.node != e["node"]))[:5]
    for limit in ("at", "below", "above"):
        lit, _ = nr.intersects_rays(sc, np.array(o), np.array(d), np.array(e["limits"][limit]), unordered=unordered)
        blocked = e["blocked"][limit]
        assert np.array_equal(~lit[~tie], blocked[~tie]), (limit, np.flatnonzero(~tie & (~lit != blocked))[:5])
