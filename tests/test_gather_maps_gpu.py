"""Light gathered from baked maps at the rays' closest hits (nrays_gather_maps_points_device / nrays_gather_maps_points; nrays_amd.gather_maps_points,
gather_maps_hits, bake_bounces) on the GPU: the fused outputs against the parts that existed before — occlusion_rays -> closest_hits -> lightmap_sample_ref -> the
numpy f32 fold — bit for bit, every number of lanes per point, sizes around a wave and across the chunk seam, maps of one row or column and every sampling mode,
max_toi and miss, skipped points, the device form, the statuses, the handle's render state, the CPU oracle's expectation (tests/test_gather_maps.py), and the
furnace: a closed cube that lights itself, whose bounces are a geometric series."""
import ctypes as C
import math

import numpy as np
import pytest

import nrays_amd as nr
from nrays_amd import abi, math3d
from tests.test_gather_maps import (BILINEAR_CLAMP, DARK, FURNACE_ATLAS, FURNACE_FLOOR, FURNACE_KA, MAPPED, MISSED, call_args, contributions, fold_classes, furnace_chart_mask,
                                    furnace_scene, furnace_tables, oracle_case, random_map)
from tests.test_occlusion_gpu import SCENES, STAT_FIELDS, bits, case
from tests.test_shade_points import rich_analytic_scene
from tests.test_shade_points_gpu import quad_scene

pytestmark = pytest.mark.gpu
ORACLE_TOL = 1e-4  # the project's bound per channel against the CPU oracle
NODE_MAPS = {"quads": ([0, 1], [1, -1], [-1, 16]), "mixed": ([0, 1, -1, 99], [1, 0, 0, -5]), "analytic": ([0, 1, -1, 99, 0, 1, 0, 1, 0], [-1] * 9)}
_MAPS = []


def two_maps():
    """A 5 x 3 and an 8 x 8 map of random float32 texels, values above 1 and a negative one among them.  Computed once, never written."""
    if not _MAPS:
        a, b = random_map(81, 5, 3, 0.0, 3.0), random_map(82, 8, 8, 0.0, 1.5)
        a[1, 2, 1] = -0.75
        assert (a > 1.0).any() and (b > 1.0).any() and (a < 0.0).any()
        _MAPS.extend([a, b])
    return list(_MAPS)


def with_mode(maps, mode=BILINEAR_CLAMP):
    return [(m,) + tuple(mode) for m in maps]


def reference(sc, points, normals, L, rot, bias, max_toi, keys, maps, node_map, miss):
    """The definition, from parts that existed before: the mirror's rays through closest_hits (uv and flags), the mirror's sample, folded in numpy f32 in the order
    of j.  `maps`: [(texels, interp, overflow)].  Returns (rgb, counts, classes (n, k))."""
    ro, rd = nr.occlusion_rays(points, normals, L, rot, bias, keys)
    n, k = ro.shape[:2]
    h = nr.closest_hits(sc, ro.reshape(-1, 3), rd.reshape(-1, 3), None if max_toi == math.inf else np.full(n * k, max_toi), want=("uv", "flags"))
    c, cls = contributions((h.flags & 1) != 0, (h.flags & 2) != 0, h.node, h.uv[:, 0], h.uv[:, 1], maps, node_map, miss)
    rgb, counts = fold_classes(c, cls, n, k)
    return rgb, counts, cls.reshape(n, k)


def textures(maps):
    """[(texels, interp, overflow)] as gather_maps_points takes them: arrays for the default mode, Texture2d otherwise."""
    return [m if (i, o) == BILINEAR_CLAMP else nr.Texture2d(nr.ImageData(m), i, o) for m, i, o in maps]


def device_gather(sc, points, normals, L, maps, node_map, rot=None, bias=1e-3, max_toi=math.inf, miss=(0.0, 0.0, 0.0), hit_flags=None, keys=None, stream=None,
                  map_tensors=True):
    """gather_maps_points on torch tensors (on `stream` when given), copied back: (rgb, counts uint32)."""
    import torch
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    tp, tn = up(points), up(normals)
    thf = None if hit_flags is None else up(np.ascontiguousarray(hit_flags, dtype=np.uint32).view(np.int32))
    tk = None if keys is None else up(np.ascontiguousarray(keys, dtype=np.uint64).view(np.int64))
    tm = [up(m) if map_tensors and isinstance(m, np.ndarray) else m for m in maps]
    run = lambda: nr.gather_maps_points(sc, tp, tn, L, tm, node_map, rot, bias, max_toi, miss, hit_flags=thf, keys=tk, want_counts=True)  # noqa: E731
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            rgb, counts = run()
        stream.synchronize()
    else:
        rgb, counts = run()
    torch.cuda.synchronize()
    assert rgb.dtype == torch.float32 and tuple(rgb.shape) == (len(points), 3) and counts.dtype == torch.int32 and tuple(counts.shape) == (len(points), 2)
    return rgb.cpu().numpy(), counts.cpu().numpy().view(np.uint32)


# ---- 1: the fused outputs are the fold of the parts that existed -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["quads", "mixed", "analytic"])
def test_equals_the_fold_of_closest_hits_and_the_sample_mirror_bit_for_bit(gpu, name):
    c = case(name)
    sc = c["scene"]
    maps = with_mode(two_maps())
    miss = (0.25, 1.5, -0.5)
    seen = {MAPPED: 0, MISSED: 0, DARK: 0}
    for node_map in NODE_MAPS[name]:
        assert len(node_map) == len(sc._nodes)
        for k in (1, 2, 7, 16):
            L = nr.hemisphere_dirs(k)
            for R in (0, 5):
                rot = nr.rotation_table(R) if R else None
                want_rgb, want_cnt, cls = reference(sc, c["points"], c["normals"], L, rot, 1e-3, math.inf, c["keys"], maps, node_map, miss)
                rgb, cnt = nr.gather_maps_points(sc, c["points"], c["normals"], L, two_maps(), node_map, rot, 1e-3, math.inf, miss, keys=c["keys"], want_counts=True)
                bad = int((bits(rgb) != bits(want_rgb)).any(axis=1).sum() + (cnt != want_cnt).any(axis=1).sum())
                print("%s %s k = %d R = %d: %d points differ; mapped %d, missed %d of %d rays" % (name, node_map, k, R, bad, (cls == MAPPED).sum(), (cls == MISSED).sum(), cls.size))
                assert rgb.dtype == np.float32 and cnt.dtype == np.uint32 and cnt.shape == (320, 2)
                assert np.array_equal(bits(rgb), bits(want_rgb)) and np.array_equal(cnt, want_cnt)
                for q in seen:
                    seen[q] += int((cls == q).sum())
    print(name, seen)
    if name == "analytic":  # most records carry no uv there (dark whatever the node's entry says), and the second node map makes every hit dark
        assert seen[DARK] > 1000 and seen[MISSED] > 1000 and seen[MAPPED] > 0
    else:
        assert seen[MAPPED] > 1000 and seen[MISSED] > 1000 and seen[DARK] > 0  # no class passes empty


# ---- 2: lanes per point ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [7, 64])
def test_every_number_of_lanes_per_point_gives_the_same_bits(gpu, k, monkeypatch):
    c = case("mixed")
    L, rot, maps, node_map, miss = nr.hemisphere_dirs(k), nr.rotation_table(5), two_maps(), [0, 1, -1, 1], (0.5, 0.25, 2.0)
    n = 257
    p, nm, keys = c["points"][:n], c["normals"][:n], c["keys"][:n]
    want = nr.gather_maps_points(c["scene"], p, nm, L, maps, node_map, rot, miss=miss, keys=keys, want_counts=True)
    ref_rgb, ref_cnt, _ = reference(c["scene"], p, nm, L, rot, 1e-3, math.inf, keys, with_mode(maps), node_map, miss)
    assert np.array_equal(bits(want[0]), bits(ref_rgb)) and np.array_equal(want[1], ref_cnt) and 0 < ref_cnt[:, 0].sum() < n * k
    for lanes in ("0", "3", "6"):
        monkeypatch.setenv("NRAYS_OCCLUSION_LANES", lanes)  # read when the handle is created
        sc = SCENES["mixed"]()[0]
        got = nr.gather_maps_points(sc, p, nm, L, maps, node_map, rot, miss=miss, keys=keys, want_counts=True)
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1]), lanes


# ---- 3: sizes and seams ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_sizes_around_a_wave(gpu, n):
    c = case("mixed")
    L, rot, maps, node_map = nr.hemisphere_dirs(16), nr.rotation_table(5), two_maps(), [0, 1, -1, 1]
    p, nm = c["points"][:n], c["normals"][:n]
    rgb, cnt = nr.gather_maps_points(c["scene"], p, nm, L, maps, node_map, rot, miss=(1, 2, 3), want_counts=True)  # default keys
    want_rgb, want_cnt, _ = reference(c["scene"], p, nm, L, rot, 1e-3, math.inf, None, with_mode(maps), node_map, (1, 2, 3))
    assert rgb.shape == (n, 3) and cnt.shape == (n, 2)
    assert np.array_equal(bits(rgb), bits(want_rgb)) and np.array_equal(cnt, want_cnt)
    d_rgb, d_cnt = device_gather(c["scene"], p, nm, L, maps, node_map, rot, miss=(1, 2, 3), keys=np.arange(n, dtype=np.uint64))
    assert np.array_equal(bits(d_rgb), bits(rgb)) and np.array_equal(d_cnt, cnt)


def test_default_keys_continue_across_the_chunk_seam(gpu):
    """num_dirs = 1024: a chunk holds 4096 points, so point 4096 of n = 4097 is the first of a second chunk.  One call under the default keys against the same
    call in two pieces under explicit keys."""
    c = case("quads")
    L, rot, maps, node_map = nr.hemisphere_dirs(1024), nr.rotation_table(5), two_maps(), [0, 1]
    n = 4097
    reps = -(-n // 320)
    p, nm = (np.ascontiguousarray(np.tile(a, (reps, 1))[:n]) for a in (c["points"], c["normals"]))
    rgb, cnt = nr.gather_maps_points(c["scene"], p, nm, L, maps, node_map, rot, miss=(0.5, 0.5, 0.5), want_counts=True)
    parts = [nr.gather_maps_points(c["scene"], p[a:b], nm[a:b], L, maps, node_map, rot, miss=(0.5, 0.5, 0.5), keys=np.arange(a, b, dtype=np.uint64), want_counts=True)
             for a, b in ((0, 4090), (4090, n))]
    assert np.array_equal(bits(rgb), bits(np.concatenate([r for r, _ in parts]))) and np.array_equal(cnt, np.concatenate([q for _, q in parts]))
    assert (cnt.sum(axis=1) <= 1024).all() and cnt[:, 0].sum() > 0
    r256, r4096 = (nr.occlusion_rays(p[i:i + 1], nm[i:i + 1], L, rot, 1e-3, np.asarray([i], np.uint64))[1] for i in (256, 4096))
    assert np.array_equal(p[256], p[4096]) and not np.array_equal(r256, r4096)  # the same point under another key: another rotation, so the keys matter
    dev = device_gather(c["scene"], p[4000:], nm[4000:], L, maps, node_map, rot, miss=(0.5, 0.5, 0.5), keys=np.arange(4000, n, dtype=np.uint64))
    assert np.array_equal(bits(dev[0]), bits(rgb[4000:])) and np.array_equal(dev[1], cnt[4000:])


# ---- 4: map edges and modes ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (6, 1), (1, 6)])
def test_maps_of_one_row_or_column(gpu, shape):
    """width - 1 = 0 or height - 1 = 0: the scaled coordinate is 0 and both taps are the one row / column."""
    c = case("quads")
    L, rot = nr.hemisphere_dirs(16), nr.rotation_table(5)
    m = random_map(90 + shape[0], shape[0], shape[1], 0.0, 2.0)
    for mode in ((nr.Interpolation.Bilinear, nr.Overflow.ClampToEdges), (nr.Interpolation.Nearest, nr.Overflow.Wrap)):
        maps = [(m,) + mode]
        want_rgb, want_cnt, cls = reference(c["scene"], c["points"], c["normals"], L, rot, 1e-3, math.inf, c["keys"], maps, [0, 0], (0, 0, 0))
        rgb, cnt = nr.gather_maps_points(c["scene"], c["points"], c["normals"], L, textures(maps), [0, 0], rot, keys=c["keys"], want_counts=True)
        assert (cls == MAPPED).sum() > 200
        assert np.array_equal(bits(rgb), bits(want_rgb)) and np.array_equal(cnt, want_cnt)


@pytest.mark.parametrize("overflow", [nr.Overflow.Wrap, nr.Overflow.ClampToEdges])
@pytest.mark.parametrize("interp", [nr.Interpolation.Bilinear, nr.Interpolation.Nearest])
def test_every_sampling_mode_equals_the_mirror(gpu, interp, overflow):
    """The quads' uvs run to 1.5 on the floor: Wrap and ClampToEdges differ there."""
    c = case("quads")
    L, rot = nr.hemisphere_dirs(16), nr.rotation_table(5)
    maps = with_mode(two_maps(), (interp, overflow))
    # points under the lace looking up see the lace; flipped normals on the lace look down at the floor, whose uvs pass 1
    p, nm = np.concatenate([c["points"], c["points"]]), np.concatenate([c["normals"], -c["normals"]])
    keys = np.concatenate([c["keys"], c["keys"]])
    want_rgb, want_cnt, cls = reference(c["scene"], p, nm, L, rot, 1e-3, math.inf, keys, maps, [0, 1], (0.1, 0.2, 0.3))
    rgb, cnt = nr.gather_maps_points(c["scene"], p, nm, L, textures(maps), [0, 1], rot, miss=(0.1, 0.2, 0.3), keys=keys, want_counts=True)
    assert (cls == MAPPED).sum() > 500
    assert np.array_equal(bits(rgb), bits(want_rgb)) and np.array_equal(cnt, want_cnt)
    d_rgb, d_cnt = device_gather(c["scene"], p, nm, L, textures(maps), [0, 1], rot, miss=(0.1, 0.2, 0.3), keys=keys, map_tensors=False)
    assert np.array_equal(bits(d_rgb), bits(rgb)) and np.array_equal(d_cnt, cnt)
    if (interp, overflow) != BILINEAR_CLAMP:  # the mode is honoured: the default mode gives other values
        other = nr.gather_maps_points(c["scene"], p, nm, L, two_maps(), [0, 1], rot, miss=(0.1, 0.2, 0.3), keys=keys)
        assert (bits(other) != bits(rgb)).any()


# ---- 5: max_toi and miss ---------------------------------------------------------------------------------------------------------------------------------------
def test_a_finite_max_toi_turns_far_hits_into_misses(gpu):
    c = case("mixed")
    L, rot, maps, node_map, miss = nr.hemisphere_dirs(16), nr.rotation_table(5), two_maps(), [0, 1, -1, 1], (4.0, 5.0, 6.0)
    far = reference(c["scene"], c["points"], c["normals"], L, rot, 1e-3, math.inf, c["keys"], with_mode(maps), node_map, miss)
    changed = 0
    for max_toi in (1.5, 0.4):
        want_rgb, want_cnt, cls = reference(c["scene"], c["points"], c["normals"], L, rot, 1e-3, max_toi, c["keys"], with_mode(maps), node_map, miss)
        rgb, cnt = nr.gather_maps_points(c["scene"], c["points"], c["normals"], L, maps, node_map, rot, 1e-3, max_toi, miss, keys=c["keys"], want_counts=True)
        assert np.array_equal(bits(rgb), bits(want_rgb)) and np.array_equal(cnt, want_cnt)
        assert (cnt[:, 1] >= far[1][:, 1]).all()
        changed += int((cnt[:, 1] > far[1][:, 1]).sum())
    assert changed > 50  # the bound did turn hits into misses


def test_open_sky_is_the_miss_colour_exactly(gpu):
    """Points on a plane with nothing above it: every ray misses, and sum of k equal values divided by k is the value (k = 8, powers of two)."""
    from tests.test_gather import _sky_case
    c = _sky_case()
    L, miss = nr.hemisphere_dirs(8), (0.25, 0.5, 1.0)
    rgb, cnt = nr.gather_maps_points(c["scene"], c["points"], c["normals"], L, two_maps(), [0], nr.rotation_table(5), miss=miss, keys=c["keys"], want_counts=True)
    assert np.array_equal(bits(rgb), bits(np.tile(np.asarray(miss, np.float32), (97, 1)))) and (cnt == [0, 8]).all()
    alone = nr.gather_maps_points(c["scene"], c["points"], c["normals"], L, two_maps(), [0], nr.rotation_table(5), miss=miss, keys=c["keys"])  # out_counts NULL
    assert np.array_equal(bits(alone), bits(rgb))


# ---- 6: skipped points -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("k", [4, 16])
def test_skipped_points_are_zero_and_leave_their_neighbours_alone(gpu, form, k):
    c = case("mixed")
    sc = c["scene"]
    L, rot, maps, node_map, miss = nr.hemisphere_dirs(k), nr.rotation_table(5), two_maps(), [0, 1, -1, 1], (1.0, 2.0, 3.0)
    if form == "host":
        run = lambda p, nm, hf, keys: nr.gather_maps_points(sc, p, nm, L, maps, node_map, rot, miss=miss, hit_flags=hf, keys=keys, want_counts=True)  # noqa: E731
    else:
        run = lambda p, nm, hf, keys: device_gather(sc, p, nm, L, maps, node_map, rot, miss=miss, hit_flags=hf, keys=keys)  # noqa: E731
    n = 130
    p, nm, keys = c["points"][:n].copy(), c["normals"][:n].copy(), c["keys"][:n]
    base_rgb, base_cnt = run(p, nm, None, keys)
    assert base_cnt.sum() > 0
    lanes = [0, 31, 63, 64, 129]
    keep = np.setdiff1d(np.arange(n), lanes)
    hf = np.full(n, 1, np.uint32)
    hf[lanes] = [0, 2, 0xfffffffe, 0, 2]  # bit 0 clear, whatever else is set
    p[lanes], nm[lanes] = np.nan, np.nan
    p[lanes[1]] = np.inf
    rgb, cnt = run(p, nm, hf, keys)
    assert (bits(rgb[lanes]) == 0).all() and (cnt[lanes] == 0).all()
    assert np.array_equal(bits(rgb[keep]), bits(base_rgb[keep])) and np.array_equal(cnt[keep], base_cnt[keep])
    rgb, cnt = run(p, nm, np.zeros(n, np.uint32), keys)  # every point skipped
    assert (bits(rgb) == 0).all() and (cnt == 0).all()


# ---- 7: the device form, gather_maps_hits ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["quads", "mixed"])
def test_the_device_form_on_another_stream_and_gather_maps_hits(gpu, name):
    import torch
    c = case(name)
    sc, o, d = c["scene"], c["o"], c["d"]
    L, rot, maps, node_map, miss = nr.hemisphere_dirs(7), nr.rotation_table(4), two_maps(), NODE_MAPS[name][0], (0.5, 1.0, 0.25)
    host = nr.gather_maps_points(sc, c["points"], c["normals"], L, maps, node_map, rot, 1e-3, 4.0, miss, keys=c["keys"], want_counts=True)
    dev = device_gather(sc, c["points"], c["normals"], L, maps, node_map, rot, 1e-3, 4.0, miss, keys=c["keys"], stream=torch.cuda.Stream())
    assert np.array_equal(bits(dev[0]), bits(host[0])) and np.array_equal(dev[1], host[1])
    assert np.array_equal(bits(sc.gather_maps_points(c["points"], c["normals"], L, maps, node_map, rot, 1e-3, 4.0, miss, keys=c["keys"])), bits(host[0]))  # Scene's method
    as_dict = {i: m for i, m in enumerate(node_map) if 0 <= m < 2}
    assert np.array_equal(bits(nr.gather_maps_points(sc, c["points"], c["normals"], L, maps, as_dict, rot, 1e-3, 4.0, miss, keys=c["keys"])), bits(host[0]))
    want = nr.gather_maps_hits(sc, o, d, c["hits"], L, maps, node_map, rot, 1e-3, 4.0, miss, want_counts=True)
    hit = (c["hits"].flags & 1) != 0
    assert hit.sum() > 300 and (bits(want[0][~hit]) == 0).all() and (want[1][~hit] == 0).all() and want[1][hit, 0].sum() > 0
    to, td = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = nr.gather_maps_hits(sc, to, td, nr.closest_hits(sc, to, td), L, [torch.from_numpy(m).cuda() for m in maps], node_map, rot, 1e-3, 4.0, miss, want_counts=True)
    s.synchronize()
    assert np.array_equal(bits(got[0].cpu().numpy()), bits(want[0])) and np.array_equal(got[1].cpu().numpy().view(np.uint32), want[1])
    with pytest.raises(ValueError):
        nr.gather_maps_hits(sc, to, td, c["hits"], L, maps, node_map)  # tensors and arrays mixed


# ---- 8: statuses -----------------------------------------------------------------------------------------------------------------------------------------------
def _raw_call(sc, form, n, arrays, params, flags=0, null=(), scene=True):
    """One library call with host or device pointers; returns (status, out_rgb, out_counts) as numpy arrays.  params: num_dirs, num_rotations, dirs, rotations, bias,
    max_toi, num_maps, num_nodes, maps [(texels or None, width, height, format, interp, overflow)] or None, node_map or None, miss."""
    import torch
    lib = abi.load_hip_lib()
    order = ("points", "normals", "hit_flags", "keys", "params", "out_rgb", "out_counts")
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
    ptrs["params"] = C.byref(st)
    args = [None if k in null else ptrs[k] for k in order]
    if form == "device":
        rc = lib.nrays_gather_maps_points_device(h, n, *args, flags, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc, held["out_rgb"].cpu().numpy(), held["out_counts"].cpu().numpy().view(np.uint32)
    return lib.nrays_gather_maps_points(h, n, *args, flags), arrays["out_rgb"], arrays["out_counts"]


def _raw_setup(n=16, k=8, R=3):
    c = case("mixed")
    arrays = dict(points=c["points"][:n].copy(), normals=c["normals"][:n].copy(), hit_flags=np.ones(n, np.uint32), keys=c["keys"][:n].copy(),
                  out_rgb=np.full((n, 3), 7.0, np.float32), out_counts=np.full((n, 2), 7, np.uint32))
    a, b = two_maps()
    rec = lambda m: (m, m.shape[1], m.shape[0], abi.TEXEL_RGBA32F, abi.INTERP_BILINEAR, abi.OVERFLOW_CLAMP)  # noqa: E731
    params = dict(num_dirs=k, num_rotations=R, dirs=nr.hemisphere_dirs(k), rotations=nr.rotation_table(R), bias=1e-3, max_toi=math.inf, num_maps=2, num_nodes=4,
                  maps=[rec(a), rec(b)], node_map=[0, 1, -1, 1], miss=(0.5, 0.25, 2.0))
    return c, arrays, params


@pytest.mark.parametrize("form", ["host", "device"])
def test_statuses(gpu, form):
    c, arrays, params = _raw_setup()
    sc = c["scene"]
    a, b = two_maps()
    call = lambda **kw: _raw_call(sc, form, kw.pop("n", 16), arrays, dict(params, **kw.pop("p", {})), **kw)  # noqa: E731
    want = nr.gather_maps_points(sc, arrays["points"], arrays["normals"], params["dirs"], [a, b], params["node_map"], params["rotations"], miss=params["miss"], keys=arrays["keys"],
                                 want_counts=True)
    for flags in (1, 2, 1 << 31, 3):
        assert call(flags=flags)[0] == abi.ERR_BAD_ARG, flags
    for name in ("points", "normals", "params", "out_rgb"):
        assert call(null=(name,))[0] == abi.ERR_BAD_ARG, name
    assert call(scene=False)[0] == abi.ERR_BAD_ARG
    rec = lambda m, **kw: tuple(dict(zip(("t", "w", "h", "f", "i", "o"), (m, m.shape[1], m.shape[0], abi.TEXEL_RGBA32F, abi.INTERP_BILINEAR, abi.OVERFLOW_CLAMP)), **kw).values())  # noqa: E731
    bad_params = [dict(dirs=None), dict(maps=None), dict(node_map=None), dict(num_dirs=0), dict(num_dirs=1025), dict(num_rotations=1025), dict(rotations=None),
                  dict(bias=math.inf), dict(bias=-math.inf), dict(bias=math.nan), dict(miss=(math.inf, 0.0, 0.0)), dict(miss=(0.0, math.nan, 0.0)), dict(miss=(0.0, 0.0, -math.inf)),
                  dict(max_toi=math.nan), dict(max_toi=0.0), dict(max_toi=-1.0), dict(max_toi=-math.inf),
                  dict(num_maps=0), dict(num_maps=17), dict(num_nodes=3), dict(num_nodes=5), dict(num_nodes=0),
                  dict(maps=[rec(a), rec(b, t=None)]), dict(maps=[rec(a, w=0), rec(b)]), dict(maps=[rec(a), rec(b, h=0)]), dict(maps=[rec(a, f=abi.TEXEL_RGBA8), rec(b)]),
                  dict(maps=[rec(a, f=2), rec(b)]), dict(maps=[rec(a), rec(b, i=2)]), dict(maps=[rec(a, o=2), rec(b)])]
    for p in bad_params:
        rc, rgb, cnt = call(p=p)
        assert rc == abi.ERR_BAD_ARG, p
        assert (rgb == 7.0).all() and (cnt == 7).all(), p  # checked before any device work
    rc, rgb, cnt = call(n=0)
    assert rc == abi.OK and (rgb == 7.0).all() and (cnt == 7).all()  # the outputs untouched
    assert call(n=0, flags=1)[0] == abi.ERR_BAD_ARG and call(n=0, p=dict(num_maps=0))[0] == abi.ERR_BAD_ARG
    rc, rgb, cnt = call(null=("out_counts",))
    assert rc == abi.OK and np.array_equal(bits(rgb), bits(want[0])) and (cnt == 7).all()  # nothing was stored there
    rc, rgb, cnt = call()
    assert rc == abi.OK and np.array_equal(bits(rgb), bits(want[0])) and np.array_equal(cnt, want[1])
    rc, rgb, cnt = call(p=dict(num_maps=1))  # one map: node 1's and 3's entry 1 is out of range now and counts as -1
    one = nr.gather_maps_points(sc, arrays["points"], arrays["normals"], params["dirs"], [a], [0, -1, -1, -1], params["rotations"], miss=params["miss"], keys=arrays["keys"], want_counts=True)
    assert rc == abi.OK and np.array_equal(bits(rgb), bits(one[0])) and np.array_equal(cnt, one[1])
    rc, rgb, cnt = call(p=dict(num_rotations=0, rotations=None), null=("hit_flags", "keys"))  # no rotation: a NULL table is fine; default keys, every point live
    none = nr.gather_maps_points(sc, arrays["points"], arrays["normals"], params["dirs"], [a, b], params["node_map"], None, miss=params["miss"], want_counts=True)
    assert rc == abi.OK and np.array_equal(bits(rgb), bits(none[0])) and np.array_equal(cnt, none[1])


# ---- 9: the handle's state -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["analytic", "quads"])
def test_a_batch_leaves_the_render_state_alone(gpu, name):
    import torch
    c = case(name)
    sc, cam = {"analytic": rich_analytic_scene, "quads": quad_scene}[name]()
    L, rot, maps, node_map = nr.hemisphere_dirs(16), nr.rotation_table(5), two_maps(), NODE_MAPS[name][0]
    want = nr.gather_maps_points(c["scene"], c["points"], c["normals"], L, maps, node_map, rot, miss=(1, 1, 1), keys=c["keys"], want_counts=True)
    w, h = 128, 72
    proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], w, h)
    first = nr.render(sc, (w, h), 1, 0.0, cam["eye"], proj)
    st1, perm1 = nr.get_stats(sc), nr.last_permutation(sc)
    rgb, cnt = device_gather(sc, c["points"], c["normals"], L, maps, node_map, rot, miss=(1, 1, 1), keys=c["keys"], stream=torch.cuda.Stream())
    assert np.array_equal(bits(rgb), bits(want[0])) and np.array_equal(cnt, want[1])  # (a fresh handle of the same scene, after a render, on another stream)
    assert nr.last_permutation(sc) == perm1
    second = nr.render(sc, (w, h), 1, 0.0, cam["eye"], proj)
    st2 = nr.get_stats(sc)
    assert np.array_equal(first.view(np.uint32), second.view(np.uint32))
    assert nr.last_permutation(sc) == perm1
    for fld in STAT_FIELDS:
        assert getattr(st1, fld) == getattr(st2, fld), fld


# ---- 10: the oracle's expectation -----------------------------------------------------------------------------------------------------------------------------
def test_against_the_cpu_oracle(gpu):
    """A hit uv that differs from the oracle's in its last f64 bit moves an 8 x 8 sample by at most 2^-24 * 7: far inside the bound."""
    c = oracle_case()
    rgb, cnt = nr.gather_maps_points(c["scene"], want_counts=True, **call_args(c))
    err = float(np.abs(rgb - c["rgb"]).max())
    print("max |hip - oracle| %.3g (bound %.3g); counts differ at %d of %d points" % (err, ORACLE_TOL, int((cnt != c["counts"]).any(axis=1).sum()), len(cnt)))
    assert np.array_equal(cnt, c["counts"])
    assert err <= ORACLE_TOL


# ---- 11: the furnace -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [None, "cuda"])
def test_furnace_the_bounces_of_a_closed_cube_are_a_geometric_series(gpu, device):
    """A closed cube with ambient ka and no lights, albedo 1/2, nothing escaping: L_0 = ka everywhere, every bounce halves it, so B bounces give
    ka * (1 - 0.5^(B + 1)) / (1 - 0.5).  Tolerance per bounce (relative): 4 roundings of the bilinear blend, k - 1 of the fold, one each for the division, the
    albedo product and the sum: B * (k + 6) * 2^-24, k = 16."""
    sc = furnace_scene()
    L, rot = furnace_tables()
    N = FURNACE_ATLAS
    to_np = lambda t: t.cpu().numpy() if device else t  # noqa: E731
    tx = nr.surface_texels(sc, 0, N, N, flip_normals=True, want=("normals",))
    live = (tx.flags & 1) != 0
    assert live.sum() == 6 * 64
    base = to_np(nr.bake_lightmap(sc, 0, N, N, flip_normals=True, device=device, dilate=64))
    assert np.array_equal(base[..., :3], np.broadcast_to(np.asarray(FURNACE_KA, np.float32), (N, N, 3))) and (base[..., 3] == 1.0).all()  # the whole atlas is filled
    rgb, cnt = nr.gather_maps_points(sc, tx.points, tx.normals, L, [base], {0: 0}, rot, hit_flags=tx.flags, want_counts=True)
    assert (cnt[live] == [16, 0]).all() and (cnt[~live] == 0).all()  # every ray of every live texel lands on the map
    ka = np.asarray(FURNACE_KA, np.float64)
    for B in (0, 1, 3):
        got = to_np(nr.bake_bounces(sc, 0, N, N, L, B, (0.5, 0.5, 0.5), rot, dilate=64, flip_normals=True, device=device))
        assert got.shape == (N, N, 4) and got.dtype == np.float32 and (got[..., 3] == 1.0).all()
        if B == 0:
            assert np.array_equal(bits(got), bits(base))
            continue
        want = ka * (1.0 - 0.5 ** (B + 1)) / (1.0 - 0.5)
        rel = float(np.abs(got.reshape(-1, 4)[live][:, :3].astype(np.float64) / want - 1.0).max())
        tol = B * (16 + 6) * 2.0 ** -24
        print("B = %d (%s): max relative error %.3g, bound %.3g" % (B, device or "host", rel, tol))
        assert rel <= tol
    per_texel = np.full((N, N, 3), 0.5)
    assert np.array_equal(bits(to_np(nr.bake_bounces(sc, 0, N, N, L, 1, per_texel, rot, dilate=64, flip_normals=True, device=device))),
                          bits(to_np(sc.bake_bounces(0, N, N, L, 1, (0.5, 0.5, 0.5), rot, dilate=64, flip_normals=True, device=device))))


def test_furnace_with_an_open_top_the_sky_reaches_a_texel_once(gpu):
    sc = furnace_scene(open_top=True)
    L, rot = furnace_tables()
    N, miss, albedo = FURNACE_ATLAS, (1.0, 1.0, 1.0), np.float32(0.5)
    tx = nr.surface_texels(sc, 0, N, N, flip_normals=True, want=("normals",))
    live = (tx.flags & 1) != 0
    floor = furnace_chart_mask(FURNACE_FLOOR).reshape(-1)
    assert live.sum() == 5 * 64 and live[floor].all()
    l0 = nr.bake_bounces(sc, 0, N, N, L, 0, (0.5, 0.5, 0.5), rot, miss=miss, dilate=64, flip_normals=True)
    b1 = nr.bake_bounces(sc, 0, N, N, L, 1, (0.5, 0.5, 0.5), rot, miss=miss, dilate=64, flip_normals=True)
    b2 = nr.bake_bounces(sc, 0, N, N, L, 2, (0.5, 0.5, 0.5), rot, miss=miss, dilate=64, flip_normals=True)
    l1 = (b1 - l0).reshape(-1, 4)[:, :3]
    dark1 = (nr.bake_bounces(sc, 0, N, N, L, 1, (0.5, 0.5, 0.5), rot, miss=(0, 0, 0), dilate=64, flip_normals=True) - l0).reshape(-1, 4)[:, :3]
    assert (l1[floor] > 0.0).all() and (l1[floor] > dark1[floor]).all()  # the floor sees the sky in its first bounce

    def loop(second_miss):
        """bake_bounces' two bounces from the calls themselves, the second with `second_miss`."""
        level, total = l0.reshape(-1, 4).copy(), l0.reshape(-1, 4).copy()
        for m in (miss, second_miss):
            rgb = nr.gather_maps_points(sc, tx.points, tx.normals, L, [level.reshape(N, N, 4)], {0: 0}, rot, miss=m, hit_flags=tx.flags)
            nxt = total.copy()
            nxt[:, :3] = albedo * rgb
            level = nr.dilate_texels(sc, tx.flags, N, N, 64, values=nxt)[0]
            total[:, :3] = total[:, :3] + level[:, :3]
        return total.reshape(N, N, 4)
    assert np.array_equal(bits(b2), bits(loop((0.0, 0.0, 0.0))))
    wrong = loop(miss)
    assert (wrong.reshape(-1, 4)[floor][:, :3] > b2.reshape(-1, 4)[floor][:, :3]).all()  # the sky counted twice is brighter: not what bake_bounces computes
