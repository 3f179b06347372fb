"""Probes filled from baked maps with their depth from the same rays (nrays_gather_maps_sh_points_device / nrays_gather_maps_sh_points; nrays_amd.gather_maps_sh_points,
gather_maps_probes, bake_probe_grid_maps) on the GPU.  Every comparison is by bit pattern and covers every point: out_sh and out_counts against the restatement from
parts that existed before — occlusion_rays -> closest_hits -> contributions / lightmap_sample_ref -> sh_fold_ref (tests/test_gather_maps_sh.py pins it without a GPU) —,
the four depth outputs against probe_depth_points on the same inputs; a finite max_toi, every number of lanes per point, sizes around a wave, the chunk seam, skipped
points, another stream, the open sky, the furnace, the statuses, the handle's render state, and a grid baked end to end."""
import ctypes as C
import math

import numpy as np
import pytest

import nrays_amd as nr
from nrays_amd import abi, math3d
from nrays_amd.marshal import CURRENT
from tests.test_gather_maps import DARK, FURNACE_ATLAS, MAPPED, MISSED, contributions, fold_classes, furnace_scene
from tests.test_gather_maps_gpu import NODE_MAPS, two_maps, with_mode
from tests.test_irradiance_vis_gpu import two_rooms
from tests.test_occlusion_gpu import SCENES, STAT_FIELDS, bits, case
from tests.test_probe_depth_gpu import same_depth, scene as depth_scene, seven_points
from tests.test_shade_points import rich_analytic_scene
from tests.test_shade_points_gpu import quad_scene

pytestmark = pytest.mark.gpu
MISS = (0.25, 1.5, -0.5)
MIXED_MAP = [0, 1, -1, 1]


def restate(sc, points, normals, L, rot, bias, max_toi, keys, maps, node_map, miss, bands):
    """The definition, from parts that existed before: the mirror's rays through closest_hits (uv and flags), the contributions of the mirror's sample, folded by
    sh_fold_ref in the order of j; the counts by fold_classes.  `maps`: [(texels, interp, overflow)].  Returns (sh, counts, classes (n, k))."""
    ro, rd = nr.occlusion_rays(points, normals, L, rot, bias, keys)
    n, k = ro.shape[:2]
    h = nr.closest_hits(sc, ro.reshape(-1, 3), rd.reshape(-1, 3), None if max_toi == math.inf else np.full(n * k, max_toi), want=("uv", "flags"))
    c, cls = contributions((h.flags & 1) != 0, (h.flags & 2) != 0, h.node, h.uv[:, 0], h.uv[:, 1], maps, node_map, miss)
    return nr.sh_fold_ref(rd, c.reshape(n, k, 3), bands), fold_classes(c, cls, n, k)[1], cls.reshape(n, k)


def to_host(out):
    """A GatherMapsSh of tensors as numpy arrays, words as uint32."""
    def one(a):
        if a is None or not hasattr(a, "cpu"):
            return a
        a = a.cpu().numpy()
        return a.view(np.uint32) if a.dtype == np.int32 else a
    return nr.GatherMapsSh(one(out.sh), one(out.counts), None if out.depth is None else nr.ProbeDepth(*(one(a) for a in out.depth)))


def device_call(sc, points, normals, L, maps, node_map, bands=3, rot=None, bias=1e-3, max_toi=math.inf, miss=(0.0, 0.0, 0.0), hit_flags=None, keys=None, depth=None,
                want=nr.scene.GATHER_MAPS_SH_OUTPUTS, stream=None):
    """gather_maps_sh_points on torch tensors (on `stream` when given), copied back."""
    import torch
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    tp, tn = up(points), up(normals)
    thf = None if hit_flags is None else up(np.ascontiguousarray(hit_flags, dtype=np.uint32).view(np.int32))
    tk = None if keys is None else up(np.ascontiguousarray(keys, dtype=np.uint64).view(np.int64))
    tm = [up(m) if isinstance(m, np.ndarray) else m for m in maps]
    run = lambda: nr.gather_maps_sh_points(sc, tp, tn, L, tm, node_map, bands, rot, bias, max_toi, miss, thf, tk, depth, want)  # noqa: E731
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            out = run()
        stream.synchronize()
    else:
        out = run()
    torch.cuda.synchronize()
    assert out.sh.dtype == torch.float32 and tuple(out.sh.shape) == (len(points), bands * bands, 3)
    return to_host(out)


def same_sh(got, want, where=""):
    """Two GatherMapsSh (or (sh, counts)) by bit pattern, every point."""
    assert got[0].dtype == np.float32 and got[0].shape == want[0].shape, where
    assert np.array_equal(bits(got[0]), bits(want[0])), ("sh", where, int((bits(got[0]) != bits(want[0])).any(axis=(1, 2)).sum()))
    if want[1] is not None:
        assert got[1].dtype == np.uint32 and np.array_equal(got[1], want[1]), ("counts", where)
    if len(want) > 2 and want[2] is not None:
        same_depth(got[2], want[2], where)


# ---- 1: out_sh and out_counts are the fold of the parts that existed -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [5, 64])
@pytest.mark.parametrize("name", ["quads", "mixed", "analytic"])
def test_sh_equals_the_restatement_bit_for_bit(gpu, name, k):
    c = case(name)
    sc = c["scene"]
    maps, L, rot = with_mode(two_maps()), nr.hemisphere_dirs(k), nr.rotation_table(5)
    seen = {MAPPED: 0, MISSED: 0, DARK: 0}
    for node_map in NODE_MAPS[name][:2]:
        assert len(node_map) == len(sc._nodes)
        want3, want_cnt, cls = restate(sc, c["points"], c["normals"], L, rot, 1e-3, math.inf, c["keys"], maps, node_map, MISS, 3)
        for bands in (1, 2, 3):
            want = want3 if bands == 3 else restate(sc, c["points"], c["normals"], L, rot, 1e-3, math.inf, c["keys"], maps, node_map, MISS, bands)[0]
            got = nr.gather_maps_sh_points(sc, c["points"], c["normals"], L, two_maps(), node_map, bands, rot, 1e-3, math.inf, MISS, keys=c["keys"])
            bad = int((bits(got.sh) != bits(want)).any(axis=(1, 2)).sum() + (got.counts != want_cnt).any(axis=1).sum())
            print("%s %s k = %d bands = %d: %d points differ; mapped %d, missed %d of %d rays" % (name, node_map, k, bands, bad, (cls == MAPPED).sum(), (cls == MISSED).sum(), cls.size))
            assert got.depth is None and got.sh.shape == (320, bands * bands, 3)
            same_sh(got, (want, want_cnt), (name, node_map, k, bands))
            assert np.array_equal(bits(got.sh), bits(want3[:, :bands * bands]))  # the first rows of the 3-band result
        for q in seen:
            seen[q] += int((cls == q).sum())
    print(name, k, seen)
    assert seen[MISSED] > 100 and (seen[MAPPED] > 100 or name == "analytic") and seen[DARK] > 0  # (most analytic records carry no uv)


# ---- 2: the depth outputs are the existing call's ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [4, 8, 16])
@pytest.mark.parametrize("name", ["room", "cube"])
def test_depth_outputs_equal_probe_depth_points_and_leave_sh_alone(gpu, name, res):
    sc = depth_scene(name)
    p, nm, flags, keys = seven_points(name)
    L, rot = nr.sphere_dirs(100), nr.rotation_table(3)
    node_map = [0] * len(sc._nodes)
    for near_dist in (0.0, 1.25):
        want = nr.probe_depth_points(sc, p, nm, L, res, 2.5, near_dist, rot, 1e-3, flags, keys)
        got = nr.gather_maps_sh_points(sc, p, nm, L, two_maps(), node_map, 3, rot, 1e-3, math.inf, MISS, flags, keys, dict(res=res, max_dist=2.5, near_dist=near_dist))
        same_depth(got.depth, want, (name, res, near_dist))
        plain = nr.gather_maps_sh_points(sc, p, nm, L, two_maps(), node_map, 3, rot, 1e-3, math.inf, MISS, flags, keys)
        same_sh(got, (plain.sh, plain.counts), (name, res, near_dist))
        assert plain.depth is None and (bits(got.sh[6]) == 0).all() and got.counts[6].tolist() == [0, 0]  # the skipped point
        assert int(got.depth.counts[:, 1].sum()) == int(got.counts[:, 1].sum())  # unbounded: a missed ray is a ray without a hit
    only = nr.gather_maps_sh_points(sc, p, nm, L, two_maps(), node_map, 1, rot, 1e-3, math.inf, MISS, flags, keys, dict(res=res, max_dist=2.5), want=())
    assert only.counts is None and only.depth.counts is None and only.depth.nearest is None and only.depth.nearest_dir is None
    assert np.array_equal(bits(only.depth.moments), bits(nr.probe_depth_points(sc, p, nm, L, res, 2.5, 0.0, rot, 1e-3, flags, keys, want=()).moments))


# ---- 3: max_toi filters the colours and the classes, never the depth ---------------------------------------------------------------------------------------------------
def test_a_finite_max_toi_turns_far_hits_into_misses_and_leaves_the_depth_alone(gpu):
    c = case("mixed")
    sc, L, rot, maps = c["scene"], nr.hemisphere_dirs(16), nr.rotation_table(5), two_maps()
    depth = dict(res=8, max_dist=3.0, near_dist=0.75)
    want_depth = nr.probe_depth_points(sc, c["points"], c["normals"], L, 8, 3.0, 0.75, rot, 1e-3, None, c["keys"])
    far = nr.gather_maps_sh_points(sc, c["points"], c["normals"], L, maps, MIXED_MAP, 3, rot, 1e-3, math.inf, MISS, keys=c["keys"], depth=depth)
    same_depth(far.depth, want_depth, "inf")
    changed = 0
    for max_toi in (1.5, 0.4):
        sh, cnt, _ = restate(sc, c["points"], c["normals"], L, rot, 1e-3, max_toi, c["keys"], with_mode(maps), MIXED_MAP, MISS, 3)
        got = nr.gather_maps_sh_points(sc, c["points"], c["normals"], L, maps, MIXED_MAP, 3, rot, 1e-3, max_toi, MISS, keys=c["keys"], depth=depth)
        same_sh(got, (sh, cnt), max_toi)
        same_depth(got.depth, want_depth, max_toi)
        assert (got.counts[:, 1] >= far.counts[:, 1]).all()
        changed += int((got.counts[:, 1] > far.counts[:, 1]).sum())
        assert (got.counts[:, 1] >= got.depth.counts[:, 1]).all() and (got.counts[:, 1] > got.depth.counts[:, 1]).any()  # the depth side still sees those hits
    assert changed > 50  # the bound did turn hits into misses


# ---- 4: lanes per point ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [5, 64, 100])
def test_every_number_of_lanes_per_point_gives_the_same_bits(gpu, k, monkeypatch):
    c = case("mixed")
    L, rot, maps, n = nr.hemisphere_dirs(k), nr.rotation_table(5), two_maps(), 257
    p, nm, keys = c["points"][:n], c["normals"][:n], c["keys"][:n]
    depth = dict(res=8, max_dist=3.0, near_dist=0.75)
    args = (L, maps, MIXED_MAP, 3, rot, 1e-3, math.inf, MISS, None, keys)
    want = nr.gather_maps_sh_points(c["scene"], p, nm, *args, depth)
    sh, cnt, _ = restate(c["scene"], p, nm, L, rot, 1e-3, math.inf, keys, with_mode(maps), MIXED_MAP, MISS, 3)
    same_sh(want, (sh, cnt, nr.probe_depth_points(c["scene"], p, nm, L, 8, 3.0, 0.75, rot, 1e-3, None, keys)), "default")
    assert 0 < cnt[:, 0].sum() < n * k
    for lanes in ("0", "3", "6"):
        monkeypatch.setenv("NRAYS_OCCLUSION_LANES", lanes)  # read when the handle is created
        sc = SCENES["mixed"]()[0]
        same_sh(nr.gather_maps_sh_points(sc, p, nm, *args, depth), want, lanes)
        same_sh(nr.gather_maps_sh_points(sc, p, nm, *args), (want.sh, want.counts), lanes)  # and the permutations without the depth payload


# ---- 5: sizes and the seam --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_sizes_around_a_wave(gpu, n):
    c = case("mixed")
    sc, L, rot, maps = c["scene"], nr.hemisphere_dirs(16), nr.rotation_table(5), two_maps()
    p, nm = c["points"][:n], c["normals"][:n]
    got = nr.gather_maps_sh_points(sc, p, nm, L, maps, MIXED_MAP, 2, rot, miss=(1, 2, 3), depth=dict(res=4, max_dist=2.0, near_dist=0.5))  # default keys
    sh, cnt, _ = restate(sc, p, nm, L, rot, 1e-3, math.inf, None, with_mode(maps), MIXED_MAP, (1, 2, 3), 2)
    assert got.sh.shape == (n, 4, 3) and got.counts.shape == (n, 2) and got.depth.moments.shape == (n, 16, 2)
    same_sh(got, (sh, cnt, nr.probe_depth_points(sc, p, nm, L, 4, 2.0, 0.5, rot)), n)
    dev = device_call(sc, p, nm, L, maps, MIXED_MAP, 2, rot, miss=(1, 2, 3), keys=np.arange(n, dtype=np.uint64), depth=dict(res=4, max_dist=2.0, near_dist=0.5))
    same_sh(dev, got, ("device", n))


def test_default_keys_continue_across_the_chunk_seam(gpu):
    """num_dirs = 1024: a chunk holds 4096 points, so point 4096 of n = 4097 is the first of a second chunk.  One call under the default keys against the same call in
    two pieces under explicit keys."""
    c = case("quads")
    sc, L, rot, maps, node_map = c["scene"], nr.hemisphere_dirs(1024), nr.rotation_table(5), two_maps(), [0, 1]
    n = 4097
    reps = -(-n // 320)
    p, nm = (np.ascontiguousarray(np.tile(a, (reps, 1))[:n]) for a in (c["points"], c["normals"]))
    depth = dict(res=4, max_dist=4.0, near_dist=1.0)
    got = nr.gather_maps_sh_points(sc, p, nm, L, maps, node_map, 3, rot, miss=MISS, depth=depth)
    parts = [nr.gather_maps_sh_points(sc, p[a:b], nm[a:b], L, maps, node_map, 3, rot, miss=MISS, keys=np.arange(a, b, dtype=np.uint64), depth=depth) for a, b in ((0, 4090), (4090, n))]
    cat = lambda f: np.concatenate([f(q) for q in parts])  # noqa: E731
    same_sh(got, (cat(lambda q: q.sh), cat(lambda q: q.counts), nr.ProbeDepth(*(cat(lambda q, i=i: q.depth[i]) for i in range(4)))), "seam")
    assert (got.counts.sum(axis=1) <= 1024).all() and got.counts[:, 0].sum() > 0
    assert np.array_equal(p[256], p[4096]) and not np.array_equal(bits(got.sh[256]), bits(got.sh[4096]))  # the same point under another key: another rotation
    same_depth(nr.ProbeDepth(*(a[4000:] for a in got.depth)), nr.probe_depth_points(sc, p[4000:], nm[4000:], L, 4, 4.0, 1.0, rot, keys=np.arange(4000, n, dtype=np.uint64)), "tail")


# ---- 6: skipped points --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("k", [4, 16])
def test_skipped_points_hold_the_defined_values_and_leave_their_neighbours_alone(gpu, form, k):
    c = case("mixed")
    sc, L, rot, maps = c["scene"], nr.hemisphere_dirs(k), nr.rotation_table(5), two_maps()
    depth = dict(res=4, max_dist=0.1, near_dist=0.05)  # a max_dist that float32 rounds
    if form == "host":
        run = lambda p, nm, hf, keys: nr.gather_maps_sh_points(sc, p, nm, L, maps, MIXED_MAP, 3, rot, miss=(1.0, 2.0, 3.0), hit_flags=hf, keys=keys, depth=depth)  # noqa: E731
    else:
        run = lambda p, nm, hf, keys: device_call(sc, p, nm, L, maps, MIXED_MAP, 3, rot, miss=(1.0, 2.0, 3.0), hit_flags=hf, keys=keys, depth=depth)  # noqa: E731
    n = 130
    p, nm, keys = c["points"][:n].copy(), c["normals"][:n].copy(), c["keys"][:n]
    base = run(p, nm, None, keys)
    assert base.counts.sum() > 0
    lanes = [0, 31, 63, 64, 129]
    keep = np.setdiff1d(np.arange(n), lanes)
    hf = np.full(n, 1, np.uint32)
    hf[lanes] = [0, 2, 0xfffffffe, 0, 2]  # bit 0 clear, whatever else is set
    p[lanes], nm[lanes] = np.nan, np.nan
    p[lanes[1]] = np.inf
    got = run(p, nm, hf, keys)
    f = np.float32(0.1)

    def skipped(o, idx):
        assert (bits(o.sh[idx]) == 0).all() and (o.counts[idx] == 0).all()
        assert (o.depth.moments[idx, :, 0] == f).all() and (o.depth.moments[idx, :, 1] == f * f).all() and (o.depth.counts[idx] == 0).all()
        assert (o.depth.nearest[idx] == math.inf).all() and (o.depth.nearest_dir[idx] == 0xFFFFFFFF).all()
    skipped(got, lanes)
    pick = lambda o, idx: (o.sh[idx], o.counts[idx], nr.ProbeDepth(*(a[idx] for a in o.depth)))  # noqa: E731
    same_sh(pick(got, keep), pick(base, keep), (form, k))
    skipped(run(p, nm, np.zeros(n, np.uint32), keys), np.arange(n))  # every point skipped


# ---- 7: the device form on another stream, and the free-point form ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["quads", "mixed"])
def test_the_device_form_on_another_stream_and_gather_maps_probes(gpu, name):
    import torch
    c = case(name)
    sc = c["scene"]
    L, rot, maps, node_map = nr.hemisphere_dirs(7), nr.rotation_table(4), two_maps(), NODE_MAPS[name][0]
    depth = dict(res=8, max_dist=3.0, near_dist=0.5)
    host = nr.gather_maps_sh_points(sc, c["points"], c["normals"], L, maps, node_map, 3, rot, 1e-3, 4.0, MISS, keys=c["keys"], depth=depth)
    dev = device_call(sc, c["points"], c["normals"], L, maps, node_map, 3, rot, 1e-3, 4.0, MISS, keys=c["keys"], depth=depth, stream=torch.cuda.Stream())
    same_sh(dev, host, name)
    same_sh(sc.gather_maps_sh_points(c["points"], c["normals"], L, maps, node_map, 3, rot, 1e-3, 4.0, MISS, keys=c["keys"], depth=depth), host, "method")
    S = nr.sphere_dirs(33)
    pos = c["points"] + 0.05 * c["normals"]
    nz = np.tile([0.0, 0.0, 1.0], (len(pos), 1))
    want = nr.gather_maps_sh_points(sc, pos, nz, S, maps, node_map, 2, None, 0.0, 4.0, MISS, depth=depth)
    same_sh(nr.gather_maps_probes(sc, pos, S, maps, node_map, 2, 4.0, MISS, depth=depth), want, "probes")
    same_sh(sc.gather_maps_probes(pos, S, maps, node_map, 2, 4.0, MISS, depth=depth), want, "probes, method")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        t = nr.gather_maps_probes(sc, torch.from_numpy(pos).cuda(), S, [torch.from_numpy(m).cuda() for m in maps], node_map, 2, 4.0, MISS, depth=depth)
    s.synchronize()
    assert t.counts.dtype == torch.int32 and t.depth.nearest.dtype == torch.float64
    same_sh(to_host(t), want, "probes, device")
    sh, cnt, _ = restate(sc, pos, nz, S, None, 0.0, 4.0, None, with_mode(maps), node_map, MISS, 2)
    same_sh(want, (sh, cnt), "probes, restated")


# ---- 8: the open sky and the furnace ------------------------------------------------------------------------------------------------------------------------------------
def test_open_sky_folds_the_miss_colour(gpu):
    from tests.test_gather import _sky_case
    c = _sky_case()
    k = 8
    L, rot = nr.hemisphere_dirs(k), nr.rotation_table(5)
    got = nr.gather_maps_sh_points(c["scene"], c["points"], c["normals"], L, two_maps(), [0], 3, rot, miss=MISS, keys=c["keys"], depth=dict(res=4, max_dist=2.0))
    rd = nr.occlusion_rays(c["points"], c["normals"], L, rot, 1e-3, c["keys"])[1]
    sky = np.broadcast_to(np.asarray(MISS, np.float32), rd.shape).copy()
    assert np.array_equal(bits(got.sh), bits(nr.sh_fold_ref(rd, sky, 3)))
    assert (got.counts == [0, k]).all() and (got.depth.counts == [0, k]).all() and (got.depth.nearest == math.inf).all() and (got.depth.moments == [2.0, 4.0]).all()


def test_furnace_a_probe_in_a_closed_cube_of_constant_maps(gpu):
    sc = furnace_scene()
    L_rgb = np.asarray((0.5, 0.25, 3.0), np.float32)
    m = np.empty((FURNACE_ATLAS, FURNACE_ATLAS, 4), np.float32)
    m[..., :3], m[..., 3] = L_rgb, 1.0
    tex = nr.Texture2d(nr.ImageData(m), nr.Interpolation.Nearest, nr.Overflow.ClampToEdges)
    pos = np.array([(0.5, 0.5, 0.5), (0.3, 0.6, 0.45), (0.7, 0.2, 0.8)], np.float64)  # the centre first
    for k in (64, 100):
        S = nr.sphere_dirs(k)
        got = nr.gather_maps_probes(sc, pos, S, [tex], [0], 3, miss=(9.0, 9.0, 9.0), depth=dict(res=8, max_dist=2.0))
        rd = np.broadcast_to(S, (len(pos), k, 3))
        want = nr.sh_fold_ref(rd, np.broadcast_to(L_rgb, rd.shape).copy(), 3)
        assert np.array_equal(bits(got.sh), bits(want))
        assert (got.counts == [k, 0]).all() and (got.depth.counts[:, 1] == 0).all()  # every ray counts as mapped
        assert (got.depth.nearest < 1.0).all() and (got.depth.nearest > 0.0).all()


# ---- 9: statuses ------------------------------------------------------------------------------------------------------------------------------------------------------
OUTS = ("out_sh", "out_counts", "out_moments", "out_depth_counts", "out_nearest", "out_nearest_dir")


def _raw_call(sc, form, n, arrays, params, bands=3, depth=(1.0, 0.25, 4, 0), flags=0, null=(), scene=True):
    """One library call with host or device pointers: (status, the six outputs as numpy arrays).  params: the fields of NraysGatherMapsParams with the tables as arrays and
    maps [(texels or None, width, height, format, interp, overflow)]; depth: (max_dist, near_dist, res, reserved) or None."""
    import torch
    lib = abi.load_hip_lib()
    h = sc.device_handle() if scene else None
    f64 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64)  # noqa: E731
    tables = dict(dirs=f64(params["dirs"]), rotations=f64(params["rotations"]), node_map=None if params["node_map"] is None else np.ascontiguousarray(params["node_map"], dtype=np.int32))
    texels = [None if m[0] is None else np.ascontiguousarray(m[0], dtype=np.float32) for m in (params["maps"] or [])]
    if form == "device":
        held = {k: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v.view(np.int32) if v.dtype == np.uint32 else v).cuda() for k, v in arrays.items()}
        tables = {k: None if v is None else torch.from_numpy(v).cuda() for k, v in tables.items()}
        texels = [None if t is None else torch.from_numpy(t).cuda() for t in texels]
        adr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        ptrs = {k: adr(t) for k, t in held.items()}
    else:
        ct = {np.dtype(np.float64): C.c_double, np.dtype(np.uint32): C.c_uint32, np.dtype(np.uint64): C.c_uint64, np.dtype(np.float32): C.c_float}
        adr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        ptrs = {k: v.ctypes.data_as(C.POINTER(ct[v.dtype])) for k, v in arrays.items()}
    recs = None
    if params["maps"] is not None:
        recs = (abi.NraysTexture * max(1, len(params["maps"])))()
        for r, t, (_, w, hh, fmt, interp, overflow) in zip(recs, texels, params["maps"]):
            r.width, r.height, r.format, r.interp, r.overflow, r.texels = w, hh, fmt, interp, overflow, adr(t)
    st = abi.NraysGatherMapsParams(params["num_dirs"], params["num_rotations"], adr(tables["dirs"]), adr(tables["rotations"]), params["bias"], params["max_toi"],
                                   params["num_maps"], params["num_nodes"], None if recs is None else C.cast(recs, C.POINTER(abi.NraysTexture)), adr(tables["node_map"]),
                                   (C.c_float * 3)(*params["miss"]))
    spec = None if depth is None else C.byref(abi.NraysGatherDepthSpec(*depth))
    a = {k: None if k in null else v for k, v in ptrs.items()}
    args = [a["points"], a["normals"], a["hit_flags"], a["keys"], None if "params" in null else C.byref(st), bands, a["out_sh"], a["out_counts"], spec, a["out_moments"],
            a["out_depth_counts"], a["out_nearest"], a["out_nearest_dir"], flags]
    if form == "device":
        rc = lib.nrays_gather_maps_sh_points_device(h, n, *args, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        back = lambda t: t.cpu().numpy().view(np.uint32) if t.dtype == torch.int32 else t.cpu().numpy()  # noqa: E731
        return rc, [back(held[k]) for k in OUTS]
    return lib.nrays_gather_maps_sh_points(h, n, *args), [arrays[k] for k in OUTS]


def _raw_setup(n=16, k=8, R=3):
    c = case("mixed")
    arrays = dict(points=c["points"][:n].copy(), normals=c["normals"][:n].copy(), hit_flags=np.ones(n, np.uint32), keys=c["keys"][:n].copy(),
                  out_sh=np.full((n, 9, 3), 7.0, np.float32), out_counts=np.full((n, 2), 7, np.uint32), out_moments=np.full((n, 16, 2), 7.0, np.float32),
                  out_depth_counts=np.full((n, 2), 7, np.uint32), out_nearest=np.full(n, 7.0, np.float64), out_nearest_dir=np.full(n, 7, np.uint32))
    a, b = two_maps()
    rec = lambda m: (m, m.shape[1], m.shape[0], abi.TEXEL_RGBA32F, abi.INTERP_BILINEAR, abi.OVERFLOW_CLAMP)  # noqa: E731
    params = dict(num_dirs=k, num_rotations=R, dirs=nr.hemisphere_dirs(k), rotations=nr.rotation_table(R), bias=1e-3, max_toi=math.inf, num_maps=2, num_nodes=4,
                  maps=[rec(a), rec(b)], node_map=MIXED_MAP, miss=(0.5, 0.25, 2.0))
    return c, arrays, params


@pytest.mark.parametrize("form", ["host", "device"])
def test_statuses(gpu, form):
    c, arrays, params = _raw_setup()
    sc = c["scene"]
    a, b = two_maps()
    untouched = lambda outs: all((o == 7).all() for o in outs)  # noqa: E731
    call = lambda **kw: _raw_call(sc, form, kw.pop("n", 16), arrays, dict(params, **kw.pop("p", {})), **kw)  # noqa: E731
    want = nr.gather_maps_sh_points(sc, arrays["points"], arrays["normals"], params["dirs"], [a, b], MIXED_MAP, 3, params["rotations"], miss=params["miss"], keys=arrays["keys"],
                                    depth=dict(res=4, max_dist=1.0, near_dist=0.25))
    rec = lambda m, **kw: tuple(dict(zip(("t", "w", "h", "f", "i", "o"), (m, m.shape[1], m.shape[0], abi.TEXEL_RGBA32F, abi.INTERP_BILINEAR, abi.OVERFLOW_CLAMP)), **kw).values())  # noqa: E731
    bad = [dict(flags=f) for f in (1, 2, 1 << 31, 3)] + [dict(null=(name,)) for name in ("points", "normals", "params", "out_sh")] + [dict(scene=False)]
    bad += [dict(bands=q) for q in (0, 4, 9, 0xFFFFFFFF)]
    bad += [dict(depth=d) for d in ((1.0, 0.25, 4, 1), (1.0, 0.25, 4, 0xFFFFFFFF), (1.0, 0.25, 0, 0), (1.0, 0.25, 5, 0), (1.0, 0.25, 32, 0), (0.0, 0.25, 4, 0), (-1.0, 0.25, 4, 0),
                                    (math.inf, 0.25, 4, 0), (math.nan, 0.25, 4, 0), (1.0, -1.0, 4, 0), (1.0, math.inf, 4, 0), (1.0, math.nan, 4, 0))]
    bad += [dict(null=("out_moments",))]                                                              # a spec without its required output
    depth_outs = OUTS[2:]
    bad += [dict(depth=None, null=tuple(q for q in depth_outs if q != keep)) for keep in depth_outs]  # a depth output without a spec, each of the four
    bad += [dict(depth=None)]                                                                         # ... and all four
    bad += [dict(p=q) for q in (dict(dirs=None), dict(maps=None), dict(node_map=None), dict(num_dirs=0), dict(num_dirs=1025), dict(num_rotations=1025), dict(rotations=None),
                                dict(bias=math.inf), dict(bias=math.nan), dict(miss=(math.inf, 0.0, 0.0)), dict(miss=(0.0, math.nan, 0.0)), dict(max_toi=math.nan), dict(max_toi=0.0),
                                dict(max_toi=-1.0), dict(num_maps=0), dict(num_maps=17), dict(num_nodes=3), dict(num_nodes=5), dict(maps=[rec(a), rec(b, t=None)]),
                                dict(maps=[rec(a, w=0), rec(b)]), dict(maps=[rec(a), rec(b, h=0)]), dict(maps=[rec(a, f=abi.TEXEL_RGBA8), rec(b)]), dict(maps=[rec(a), rec(b, i=2)]),
                                dict(maps=[rec(a, o=2), rec(b)]))]
    for kw in bad:
        for n in (16, 0):
            rc, outs = call(n=n, **dict(kw))
            assert rc == abi.ERR_BAD_ARG, (kw, n)
            assert untouched(outs), (kw, n)  # checked before any device work
    rc, outs = call(n=0)
    assert rc == abi.OK and untouched(outs)  # n == 0: the outputs untouched
    rc, outs = call(n=0, depth=None, null=depth_outs)
    assert rc == abi.OK and untouched(outs)
    rc, outs = call()
    assert rc == abi.OK
    same_sh((outs[0], outs[1], nr.ProbeDepth(*outs[2:])), want, form)
    for o in outs[1:]:
        o[...] = 7
    rc, outs = call(null=("out_counts", "out_depth_counts", "out_nearest", "out_nearest_dir", "hit_flags", "keys"), p=dict(num_rotations=0, rotations=None))  # the optional ones
    none = nr.gather_maps_sh_points(sc, arrays["points"], arrays["normals"], params["dirs"], [a, b], MIXED_MAP, 3, None, miss=params["miss"], depth=dict(res=4, max_dist=1.0, near_dist=0.25))
    assert rc == abi.OK and np.array_equal(bits(outs[0]), bits(none.sh)) and np.array_equal(bits(outs[2]), bits(none.depth.moments))
    assert all((o == 7).all() for o in (outs[1], outs[3], outs[4], outs[5]))  # nothing was stored there
    for o in outs:
        o[...] = 7
    rc, outs = call(depth=None, null=depth_outs, bands=2)
    assert rc == abi.OK and np.array_equal(bits(outs[0].reshape(-1)[:16 * 12].reshape(16, 4, 3)), bits(want.sh[:, :4])) and np.array_equal(outs[1], want.counts)
    assert untouched(outs[2:])


# ---- 10: the handle's state ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["analytic", "quads"])
def test_a_batch_leaves_the_render_state_alone(gpu, name):
    import torch
    c = case(name)
    sc, cam = {"analytic": rich_analytic_scene, "quads": quad_scene}[name]()
    L, rot, maps, node_map = nr.hemisphere_dirs(16), nr.rotation_table(5), two_maps(), NODE_MAPS[name][0]
    depth = dict(res=8, max_dist=3.0, near_dist=0.5)
    want = nr.gather_maps_sh_points(c["scene"], c["points"], c["normals"], L, maps, node_map, 3, rot, miss=(1, 1, 1), keys=c["keys"], depth=depth)
    w, h = 128, 72
    proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], w, h)
    first = nr.render(sc, (w, h), 1, 0.0, cam["eye"], proj)
    st1, perm1 = nr.get_stats(sc), nr.last_permutation(sc)
    got = device_call(sc, c["points"], c["normals"], L, maps, node_map, 3, rot, miss=(1, 1, 1), keys=c["keys"], depth=depth, stream=torch.cuda.Stream())
    same_sh(got, want, name)  # (a fresh handle of the same scene, after a render, on another stream)
    assert nr.last_permutation(sc) == perm1
    second = nr.render(sc, (w, h), 1, 0.0, cam["eye"], proj)
    st2 = nr.get_stats(sc)
    assert np.array_equal(first.view(np.uint32), second.view(np.uint32))
    assert nr.last_permutation(sc) == perm1
    for fld in STAT_FIELDS:
        assert getattr(st1, fld) == getattr(st2, fld), fld


# ---- 11: end to end -----------------------------------------------------------------------------------------------------------------------------------------------------
def two_rooms_with_a_panel():
    """The two rooms of tests/test_irradiance_vis_gpu.py — cuboids, which carry no light map — with one mesh node that can: a 4 x 4 panel lying 1/64 above the floor of
    the lit room, facing up, its uv square the unit square.  (scene, the panel's node index)."""
    base = two_rooms()
    y = 0.015625  # (a float32: mesh vertices must be)
    pts = np.array([(-5.0, y, -2.0), (-1.0, y, -2.0), (-1.0, y, 2.0), (-5.0, y, 2.0)], np.float64)
    uvs = np.array([(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)], np.float64)
    idx = np.array([(0, 2, 1), (0, 3, 2)], np.uint32)  # cross(e1, e2) points up
    mat = nr.PhongMaterial((0.0, 0.0, 0.0), (0.8, 0.7, 0.6), (0.0, 0.0, 0.0), None, None, 20.0)
    nodes = list(base._nodes) + [nr.SceneNode(mat, 0.0, 0.0, 1.0, 1.0, nr.Isometry3(), nr.TriMesh(pts, idx, uvs))]
    return nr.Scene(nodes, base._lights, base._background), len(nodes) - 1


@pytest.mark.parametrize("device", [None, CURRENT])
def test_end_to_end_a_grid_baked_from_a_light_map(gpu, device):
    import torch
    sc, panel = two_rooms_with_a_panel()
    to_np = lambda t: (t.cpu().numpy().view(np.uint32) if t.dtype == torch.int32 else t.cpu().numpy()) if torch.is_tensor(t) else t  # noqa: E731
    base = nr.bake_lightmap(sc, panel, 16, 16, device=device, dilate=2)
    assert float(to_np(base)[..., :3].max()) > 0.0  # the panel is lit
    L = nr.sphere_dirs(128)
    origin, cell, counts = (-5.5, 0.5, -2.0), (1.0, 1.0, 1.0), (12, 5, 5)
    settings = dict(res=8, max_dist=2.0, near_dist=0.2, floor=0.0)
    grid, vis = nr.bake_probe_grid_maps(sc, origin, cell, counts, L, [base], {panel: 0}, 3, (0.0, 0.0, 0.0), settings, device=device)
    assert torch.is_tensor(grid.sh) == (device is not None) and torch.is_tensor(vis.moments) == (device is not None)
    plain = nr.bake_probe_grid(sc, origin, cell, counts, L, 3, device=device)
    want_vis, want_valid = nr.bake_probe_visibility(sc, plain, L, 8, max_dist=2.0, near_dist=0.2, floor=0.0)
    assert np.array_equal(bits(to_np(vis.moments)), bits(to_np(want_vis.moments))) and np.array_equal(to_np(grid.valid), to_np(want_valid))
    assert (vis.res, vis.floor, vis.bias) == (want_vis.res, want_vis.floor, want_vis.bias) and to_np(grid.valid).dtype == np.uint32
    pos = nr.probe_grid_positions(origin, cell, counts)
    probes = nr.gather_maps_probes(sc, pos if device is None else torch.from_numpy(pos).cuda(), L, [base], {panel: 0}, 3)
    sh = to_np(grid.sh)
    assert np.array_equal(bits(sh), bits(to_np(probes.sh))) and sh.shape == (300, 9, 3)
    mapped = to_np(probes.counts)[:, 0]
    assert (mapped[pos[:, 0] > 0] == 0).all() and (mapped[pos[:, 0] < 0] > 0).all()  # the probes of the lit room see the panel, the others cannot
    assert (sh[pos[:, 0] > 0].view(np.uint32) == 0).all() and (np.abs(sh[pos[:, 0] < 0]).sum(axis=(1, 2)) > 0).all()
    # ... and the consumer runs on the result
    rng = np.random.default_rng(900)
    p = np.stack([rng.uniform(-5.0, 5.0, size=200), rng.uniform(0.5, 4.5, size=200), rng.uniform(-2.0, 2.0, size=200)], axis=1)
    nm = np.tile([0.0, -1.0, 0.0], (200, 1))  # looking down at the panel
    up = (lambda a: a) if device is None else (lambda a: torch.from_numpy(a).cuda())  # noqa: E731
    rgb = to_np(nr.irradiance_points(sc, up(p), up(nm), grid, visibility=vis))
    g_np = grid._replace(sh=sh, valid=to_np(grid.valid))
    assert np.array_equal(bits(rgb), bits(nr.irradiance_points_ref(p, nm, g_np, visibility=vis._replace(moments=to_np(vis.moments)))[0]))
    assert np.isfinite(rgb).all() and (rgb[p[:, 0] < -1.0] > 0).any()
