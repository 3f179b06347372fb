"""Every BLAS of the HOST builder covers its triangles (tests/blas_cover.py states the property: shape, nesting, cover), pre-split pieces included, on a
machine without a GPU: tests/blas_probe_shim.cpp is build_blas_probe(mesh, Switches{}, device = false, presplit) compiled with g++ like
tests/host_scene_shim.cpp.  tests/test_device_build_gpu.py compares the device builder with this one, and both clip, box and rate pre-split pieces with the
one header presplit_clip.h: only a property that needs no second builder can see a mistake in it.

  - every case mesh, with and without pre-splitting (run with -s for the report lines: references, samples, worst slack, seconds);
  - a second build of the shim with -DNR_PRESPLIT_EXACT_BELOW=512 sends the meshes of more than 512 triangles through presplit()'s threshold path (the
    sample's heap, split_rec under std::async), which the library takes from 400 000 triangles; the library's own build keeps that value
    (tests/test_host_scene.py's digests);
  - build_bvh alone (tests/bvh_build_shim.cpp; the TLAS's case with max_leaf 1): rules 1 and 2, and every primitive's box inside all boxes of its path;
  - mutants of a valid dump, each reported under its rule;
  - mutants of the builder: a copy of presplit_clip.h with ONE textual substitution and a copy of scene_build.cpp (which includes it by its quoted
    name) in tmp_path, the shim compiled against them; each must leave seam samples uncovered:
      poly_box rounding to nearest; poly_box skipping the polygon's last vertex; the upper half clipped at mid + 1e-3 * ext (1e-7 * ext is swallowed by
      the f32 rounding of the boxes: no gap).
    Readings that SURVIVE, and are therefore not on the list: dropping the extra ulp (clip_next_up(clip_round_up(..)) -> clip_round_up(..)) — it is
    insurance against the rounding of the clip's own intersection points, a few 2^-53 that the outward f32 rounding already swallows, so no sample
    reaches it; and `<` for `<=` in clip_half — it only decides which half keeps a vertex lying exactly on the plane, which generic meshes do not have."""
import ctypes as C
import os
import subprocess
import time

import numpy as np
import pytest

from tests import blas_cover as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nrays_amd", "csrc")
CLIP = os.path.join(CSRC, "presplit_clip.h")

BUILDER_MUTANTS = {
    "box_rounds_to_nearest": ("const float dn = clip_next_down(clip_round_down(lo)), up = clip_next_up(clip_round_up(hi));", "const float dn = (float)lo, up = (float)hi;"),
    "box_skips_last_vertex": ("for (int k = 0; k < p.n; ++k) { lo = ", "for (int k = 0; k + 1 < p.n; ++k) { lo = "),
    "upper_half_clipped_late": ("!clip_half(poly, axis, mid, false, hi)", "!clip_half(poly, axis, mid + 1e-3 * (double)ext, false, hi)"),
}


def _compile(out, scene_build, flags=()):
    """Starts g++ on the probe shim; the caller waits."""
    return subprocess.Popen(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", CSRC, "-fPIC", "-shared", "-pthread", *flags,
                             "-o", out, os.path.join(ROOT, "tests", "blas_probe_shim.cpp"), scene_build, os.path.join(CSRC, "bvh_build.cpp"), os.path.join(CSRC, "switches.cpp")])


class Probe:
    def __init__(self, path):
        self.lib = C.CDLL(path)

    def build(self, pts, idx, presplit):
        p64 = np.ascontiguousarray(np.asarray(pts, np.float32).astype(np.float64)); idx = np.ascontiguousarray(idx, np.uint32)
        cap = 12 * len(idx) + 64
        nodes = np.zeros((cap, 32), np.float32); tri = np.zeros(cap, np.uint32)
        info = (C.c_int32 * 5)(); err = C.create_string_buffer(256)
        rc = self.lib.blas_probe_shim_build(C.c_uint32(len(p64)), p64.ctypes.data_as(C.c_void_p), C.c_uint32(len(idx)), idx.ctypes.data_as(C.c_void_p), C.c_int(int(presplit)),
                                            C.c_uint32(cap), C.c_uint32(cap), nodes.ctypes.data_as(C.c_void_p), tri.ctypes.data_as(C.c_void_p), info, err, C.c_size_t(len(err)))
        assert rc == 0, err.value
        assert info[3] <= cap and info[4] <= cap
        return dict(nodes=nodes[:info[3]].copy(), tri=tri[:info[4]].copy(), root=info[0], depth=info[1], hairy=info[2])


@pytest.fixture(scope="module")
def shims(tmp_path_factory):
    """All compilations of this module at once: the shim, the shim with the low threshold, one shim per mutant of presplit_clip.h, and build_bvh's shim."""
    d = tmp_path_factory.mktemp("blas_probe")
    text = open(CLIP).read(); scene_build = open(os.path.join(CSRC, "scene_build.cpp")).read()
    jobs = {"heap": _compile(str(d / "probe.so"), os.path.join(CSRC, "scene_build.cpp")),
            "threshold": _compile(str(d / "probe512.so"), os.path.join(CSRC, "scene_build.cpp"), ["-DNR_PRESPLIT_EXACT_BELOW=512"])}
    paths = {"heap": str(d / "probe.so"), "threshold": str(d / "probe512.so")}
    for name, (old, new) in BUILDER_MUTANTS.items():
        assert text.count(old) == 1, (name, "the text to replace occurs %d times in presplit_clip.h" % text.count(old))
        mutated = text.replace(old, new)
        assert mutated != text, name
        m = d / name; m.mkdir()
        (m / "presplit_clip.h").write_text(mutated); (m / "scene_build.cpp").write_text(scene_build)
        paths[name] = str(m / "probe.so")
        jobs[name] = _compile(paths[name], str(m / "scene_build.cpp"))
    paths["bvh"] = str(d / "bvh.so")
    jobs["bvh"] = subprocess.Popen(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-I", CSRC, "-fPIC", "-shared", "-pthread", "-o", paths["bvh"],
                                    os.path.join(ROOT, "tests", "bvh_build_shim.cpp"), os.path.join(CSRC, "bvh_build.cpp")])
    for name, j in jobs.items():
        assert j.wait() == 0, name
    out = {k: Probe(v) for k, v in paths.items() if k != "bvh"}
    out["bvh"] = C.CDLL(paths["bvh"])
    return out


@pytest.fixture(scope="module")
def meshes():
    m = bc.case_meshes()
    m["hair10k"] = bc.hair10k()
    return m


def _seam_every(idx):
    return max(1, len(idx) // 1200)  # all triangles of the small meshes; of the larger ones about 1 200, spread over the mesh


def _check(name, probe, pts, idx, presplit):
    t0 = time.time()
    d = probe.build(pts, idx, presplit)
    rep = bc.validate(d, pts, idx, presplit, seam_every=_seam_every(idx))
    print(bc.line(name, rep, time.time() - t0))
    assert bc.clean(rep), bc.line(name, rep)
    return d, rep


CASES = ("hair800", "hairball", "slivers", "sheet", "copies", "hair64", "hair255", "hair256", "hair257", "fat_soup", "hair10k")


@pytest.mark.parametrize("presplit", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_host_blas_covers_its_triangles(shims, meshes, case, presplit):
    pts, idx = meshes[case]
    d, rep = _check("%s%s" % (case, " pre-split" if presplit else ""), shims["heap"], pts, idx, presplit)
    if not presplit:
        assert len(d["tri"]) == len(idx)
    elif case.startswith("hair"):  # the hair-like meshes must really be pre-split, with seams to sample
        assert d["hairy"] == 1 and len(d["tri"]) > 4 * len(idx) and rep["seam"] > 0
    elif case == "copies":
        assert len(d["tri"]) == len(idx)  # a right triangle fills half of its box: nothing to gain, nothing split


@pytest.mark.parametrize("case", ["hair800", "hairball", "slivers", "fat_soup", "hair10k"])
def test_host_threshold_path_covers_its_triangles(shims, meshes, case):
    """presplit() above kExactBelow triangles: the threshold from a sample's heap, then split_rec over all triangles under std::async."""
    pts, idx = meshes[case]
    assert len(idx) > 512
    d, _ = _check("%s threshold" % case, shims["threshold"], pts, idx, True)
    if case == "hair800":  # the sample's threshold is not the whole mesh's: other references than the heap's, which shows that the other path ran
        assert len(d["tri"]) != len(shims["heap"].build(pts, idx, True)["tri"])
        assert d["hairy"] == 1 and len(d["tri"]) > 4 * len(idx)


# ---- build_bvh alone ---------------------------------------------------------------------------------------------------------------

def _bvh(lib, boxes, max_leaf):
    boxes = np.ascontiguousarray(boxes, np.float32); n = len(boxes)
    cap = 2 * n + 4
    nodes = np.zeros((cap, 32), np.float32); order = np.zeros(n, np.uint32); info = (C.c_int32 * 2)()
    lib.bvh_shim_build.restype = C.c_uint32
    got = lib.bvh_shim_build(C.c_uint32(n), boxes.ctypes.data_as(C.c_void_p), C.c_int32(max_leaf), C.c_float(0.0), C.c_uint32(cap), nodes.ctypes.data_as(C.c_void_p),
                             order.ctypes.data_as(C.c_void_p), info)
    assert got <= cap
    return dict(nodes=nodes[:got].copy(), tri=order, root=info[0], depth=info[1])


def _box_sets():
    rng = np.random.default_rng(3)
    def rand(n):
        c = rng.uniform(-1, 1, (n, 3)); h = rng.uniform(0.0, 0.2, (n, 3))
        return np.concatenate([c - h, c + h], axis=1).astype(np.float32)
    sets = {"random%d" % n: rand(n) for n in (1, 2, 4, 5, 300)}
    sets["coincident"] = np.tile(rand(1), (37, 1))
    p = rng.uniform(-1, 1, (90, 3)).astype(np.float32)
    sets["zero_extent"] = np.concatenate([p, p], axis=1)
    sets["flat"] = rand(120); sets["flat"][:, [1, 4]] = 0.5
    return sets


@pytest.mark.parametrize("max_leaf", [1, 8])
def test_build_bvh_trees_are_well_formed_and_hold_their_boxes(shims, max_leaf):
    for name, boxes in _box_sets().items():
        d = _bvh(shims["bvh"], boxes, max_leaf)
        n = len(boxes)
        shape, nesting, depth, lv = bc.walk(d["nodes"], d["root"], n, (boxes[:, :3].min(axis=0), boxes[:, 3:].max(axis=0)))
        assert (shape, nesting) == (0, 0) and depth == d["depth"], (name, shape, nesting, depth, d["depth"])
        assert sorted(d["tri"].tolist()) == list(range(n)), name
        assert (lv["count"] <= max_leaf).all(), name
        leaf_of = np.repeat(np.arange(len(lv["first"])), lv["count"])  # the leaves tile [0, n): slot k belongs to leaf leaf_of[k]
        b = boxes[d["tri"]].astype(np.float64)
        assert (b[:, :3] >= lv["lo"][leaf_of]).all() and (b[:, 3:] <= lv["hi"][leaf_of]).all(), name  # inside the intersection = inside every box of the path


# ---- mutants of a dumped tree ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def valid(shims, meshes):
    pts, idx = meshes["hair256"]
    d = shims["heap"].build(pts, idx, True)
    rep = bc.validate(d, pts, idx, True)
    assert bc.clean(rep)
    return d, rep, pts, idx


def _mutant(valid):
    d, rep, pts, idx = valid
    return dict(nodes=d["nodes"].copy(), tri=d["tri"].copy(), root=d["root"], depth=d["depth"]), rep["leaves"], pts, idx


def _slot(nodes, node, plane_slot, k):
    return nodes.reshape(-1, 8, 4)[node, plane_slot, k:k + 1]  # a view of one plane of child k


def test_mutant_leaf_plane_one_ulp_inward_is_a_cover_violation(valid):
    """A triangle's corner (a grid sample) that lies ON a face of the only region holding it: that face moved one f32 ulp inward uncovers it."""
    m, lv, pts, idx = _mutant(valid)
    V = np.asarray(pts, np.float32)[idx.astype(np.int64)].astype(np.float64)
    regions = {}  # triangle -> leaves
    for l, (f, c) in enumerate(zip(lv["first"], lv["count"])):
        for t in m["tri"][f:f + c]:
            regions.setdefault(int(t), set()).add(l)
    found = None
    for t, ls in regions.items():
        for p in V[t]:
            holding = [l for l in ls if (p >= lv["lo"][l]).all() and (p <= lv["hi"][l]).all()]
            if len(holding) != 1:
                continue
            l = holding[0]
            for ax in range(3):
                if p[ax] == lv["hi"][l][ax]: found = (l, ax, True)
                elif p[ax] == lv["lo"][l][ax]: found = (l, ax, False)
            if found: break
        if found: break
    assert found, "no corner on a face of its only region"
    l, ax, upper = found
    plane = _slot(m["nodes"], lv["node"][l], (bc.HI if upper else bc.LO)[ax], lv["slot"][l])
    plane[0] = np.nextafter(plane[0], np.float32(-np.inf if upper else np.inf))
    rep = bc.validate(m, pts, idx, True)
    assert rep["cover"] >= 1 and rep["shape"] == 0 and rep["nesting"] == 0, bc.line("plane inward", rep)
    assert 0 < rep["worst_slack"] < 1e-6  # one f32 ulp of a coordinate of order 1


def test_mutant_reference_to_another_subtrees_triangle_is_a_cover_violation(valid):
    m, lv, pts, idx = _mutant(valid)
    assert m["tri"][0] != m["tri"][-1]
    m["tri"][0] = m["tri"][-1]  # first and last leaf in depth-first order: under different children of the root
    rep = bc.validate(m, pts, idx, True)
    assert rep["cover"] >= 1 and rep["shape"] == 0 and rep["nesting"] == 0, bc.line("foreign reference", rep)


def test_mutant_child_redirected_to_a_sibling_is_a_shape_violation(valid):
    m, lv, pts, idx = _mutant(valid)
    refs = m["nodes"].reshape(-1, 8, 4)[m["root"], bc.CHILD].view(np.int32)
    assert refs[0] >= 0 and refs[1] >= 0
    refs[0] = refs[1]
    rep = bc.validate(m, pts, idx, True)
    assert rep["shape"] >= 1, bc.line("redirected child", rep)


def test_mutant_child_box_past_its_parent_is_a_nesting_violation(valid):
    m, lv, pts, idx = _mutant(valid)
    n3 = m["nodes"].reshape(-1, 8, 4)
    child = int(n3[m["root"], bc.CHILD].view(np.int32)[0])
    assert child >= 0
    n3[child, bc.HI[0], 0] = np.nextafter(n3[m["root"], bc.HI[0], 0], np.float32(np.inf))  # one ulp past the box the root holds for this node
    rep = bc.validate(m, pts, idx, True)
    assert rep["nesting"] >= 1 and rep["shape"] == 0 and rep["cover"] == 0, bc.line("grown child", rep)


def test_mutant_leaf_count_reduced_is_a_shape_violation(valid):
    m, lv, pts, idx = _mutant(valid)
    l = int(np.nonzero(lv["count"] >= 2)[0][0])
    ref = _slot(m["nodes"], lv["node"][l], bc.CHILD, lv["slot"][l]).view(np.int32)
    assert ~int(ref[0]) == (int(lv["first"][l]) << 3) | (int(lv["count"][l]) - 1)
    ref[0] = ~((int(lv["first"][l]) << 3) | (int(lv["count"][l]) - 2))
    rep = bc.validate(m, pts, idx, True)
    assert rep["shape"] >= 1 and rep["nesting"] == 0, bc.line("short leaf", rep)


# ---- mutants of the builder --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mutant", sorted(BUILDER_MUTANTS))
def test_mutant_of_the_clip_header_leaves_seam_samples_uncovered(shims, meshes, mutant):
    pts, idx = meshes["hair800"]
    d = shims[mutant].build(pts, idx, True)
    assert d["hairy"] == 1 and len(d["tri"]) > 4 * len(idx)
    rep = bc.validate(d, pts, idx, True)
    print(bc.line(mutant, rep))
    assert rep["uncovered_seam"] > 0 and rep["cover"] > 0, bc.line(mutant, rep)
