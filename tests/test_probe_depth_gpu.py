"""nrays_probe_depth_points_device / nrays_probe_depth_points on the GPU: moments, counts, nearest and nearest_dir are compared BIT FOR BIT with the mirror built
from parts that existed before — occlusion_rays() -> closest_hits() -> probe_depth_ref() (whose properties tests/test_probe_depth.py tests without a GPU) — in an
analytic room and on a transformed cube mesh, at points in open space, inside a solid, exactly on a surface and skipped, for every resolution, direction counts
around the lane counts and the tile sizes of the fold, every forced number of lanes a point, across a chunk seam, and on another stream."""
import math

import numpy as np
import pytest

import nrays_amd as nr
from tests.test_occlusion_gpu import bits
from tools import scenes_util as su

pytestmark = pytest.mark.gpu

RES = (4, 8, 16)
NUM_DIRS = (1, 5, 64, 100, 1024)


def room_scene():
    """A closed room of six cuboid slabs (inner box [-3, 3] x [0, 4] x [-3, 3]) with a ball and a SOLID cuboid block in it: analytic shapes only."""
    mat = su.default_material()
    node = lambda t, g, solid=False: nr.SceneNode(mat, 0.0, 0.0, 1.0, 1.0, nr.Isometry3(t), g, None, solid)  # noqa: E731
    slabs = [((0, -0.25, 0), (3.5, 0.25, 3.5)), ((0, 4.25, 0), (3.5, 0.25, 3.5)), ((-3.25, 2, 0), (0.25, 2.5, 3.5)), ((3.25, 2, 0), (0.25, 2.5, 3.5)),
             ((0, 2, -3.25), (3.5, 2.5, 0.25)), ((0, 2, 3.25), (3.5, 2.5, 0.25))]
    nodes = [node(t, nr.Cuboid(h)) for t, h in slabs] + [node((1.0, 1.0, -0.5), nr.Ball(0.75)), node((-1.5, 0.5, 1.0), nr.Cuboid((0.5, 0.5, 0.5)), True)]
    return nr.Scene(nodes, [nr.Light((0.0, 3.5, 0.0), 0.0, 1, (1, 1, 1))], (0.0, 0.0, 0.0))


def cube_mesh_scene():
    """Twelve triangles: a unit cube mesh under a rotation and a translation — the mesh permutation (kFeatMesh) and the instance transform."""
    v = np.array([(x, y, z) for x in (-0.5, 0.5) for y in (-0.5, 0.5) for z in (-0.5, 0.5)], np.float64)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    idx = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.uint32)
    mesh = nr.SceneNode(su.default_material(), 0.0, 0.0, 1.0, 1.0, nr.Isometry3((0.5, 1.0, -0.25), (0.3, -0.4, 0.5)), nr.TriMesh(v, idx))
    return nr.Scene([mesh], [nr.Light((0.0, 5.0, 0.0), 0.0, 1, (1, 1, 1))], (0.0, 0.0, 0.0))


def seven_points(name):
    """In open space (twice), inside a solid, exactly on a surface, with non-axis normals, and one skipped point that holds NaNs."""
    s = 1.0 / math.sqrt(3.0)
    if name == "room":
        p = [(0.0, 2.0, 0.0), (-1.0, 3.0, -2.0), (-1.5, 0.5, 1.0), (2.0, 0.0, 2.0), (1.0, 1.75, -0.5), (0.5, 1.0, 1.5), (math.nan,) * 3]
    else:
        p = [(0.5, 1.0, -0.25), (3.0, 1.0, 0.0), (0.6, 0.9, -0.2), (0.5, 3.0, -0.25), (-2.0, -1.0, 1.5), (0.5, 1.0, 4.0), (math.nan,) * 3]
    nm = [(0.0, 0.0, 1.0), (s, s, s), (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), (0.6, 0.0, -0.8), (-s, s, -s), (math.nan,) * 3]
    flags = np.array([1, 3, 1, 1, 7, 1, 2], np.uint32)
    keys = np.array([11, 5, 2 ** 40 + 1, 7, 9, 2 ** 63 + 3, 1], np.uint64)
    return np.array(p, np.float64), np.array(nm, np.float64), flags, keys


_SCENES = {}


def scene(name):
    if name not in _SCENES:
        _SCENES[name] = room_scene() if name == "room" else cube_mesh_scene()
    return _SCENES[name]


def mirror(sc, p, nm, flags, keys, L, rot, bias, R, max_dist, near_dist):
    """The definition from parts that existed before: the mirror's rays through closest_hits, folded by probe_depth_ref.  A skipped point's rays are not traced."""
    live = np.ones(len(p), bool) if flags is None else (flags & 1) != 0
    ps, ns = np.where(live[:, None], p, 0.0), np.where(live[:, None], nm, [0.0, 0.0, 1.0])
    ro, rd = nr.occlusion_rays(ps, ns, L, rot, bias, keys)
    n, k = ro.shape[:2]
    hits = nr.closest_hits(sc, ro.reshape(-1, 3), rd.reshape(-1, 3), want=("flags",))
    return nr.probe_depth_ref(rd, hits.toi.reshape(n, k), hits.flags.reshape(n, k), R, max_dist, near_dist, flags)


def same_depth(got, want, where=""):
    for name, a, b in zip(nr.ProbeDepth._fields, got, want):
        a = a.cpu().numpy() if hasattr(a, "cpu") else a
        a = a.view(np.uint32) if a.dtype == np.int32 else a
        assert a.dtype == b.dtype and a.shape == b.shape, (name, where, a.dtype, a.shape)
        assert np.array_equal(bits(a), bits(b)), (name, where, int((bits(a) != bits(b)).sum()))


@pytest.mark.parametrize("k", NUM_DIRS)
@pytest.mark.parametrize("name", ["room", "cube"])
def test_equals_the_mirror_bit_for_bit(gpu, name, k):
    sc = scene(name)
    p, nm, flags, keys = seven_points(name)
    L, rot = (nr.sphere_dirs(k), nr.rotation_table(3))
    seen_near = seen_miss = seen_hit = 0
    for R in RES:
        for near_dist in (0.0, 1.25):
            want = mirror(sc, p, nm, flags, keys, L, rot, 1e-3, R, 2.5, near_dist)
            got = nr.probe_depth_points(sc, p, nm, L, R, 2.5, near_dist, rot, 1e-3, flags, keys)
            print("%s k = %d R = %d near %g: counts %s nearest_dir %s" % (name, k, R, near_dist, got.counts.tolist(), got.nearest_dir.tolist()))
            same_depth(got, want, (name, k, R, near_dist))
            f = np.float32(2.5)
            assert (got.moments[6, :, 0] == f).all() and (got.moments[6, :, 1] == f * f).all() and got.counts[6].tolist() == [0, 0]
            assert got.nearest[6] == math.inf and got.nearest_dir[6] == 0xFFFFFFFF
            if near_dist == 0.0:
                assert (got.counts[:, 0] == 0).all()
            seen_near += int(got.counts[:, 0].sum()); seen_miss += int(got.counts[:, 1].sum()); seen_hit += int((got.counts[:6, 1] < k).sum())
    assert seen_near > 0 and seen_hit > 0 and (seen_miss > 0 or name == "room")  # (the room is closed: nothing misses there)
    if name == "room":
        d = nr.probe_depth_points(sc, p, nm, L, 8, 2.5, 1.25, rot, 1e-3, flags, keys)
        assert d.counts[2].tolist() == [k, 0] and d.nearest[2] == 0.0 and d.nearest_dir[2] == 0  # inside the solid block: every ray ends at once
    # the outputs that are not asked for are not computed, and the moments do not depend on them
    only = nr.probe_depth_points(sc, p, nm, L, 4, 2.5, 0.0, rot, 1e-3, flags, keys, want=())
    assert only.counts is None and only.nearest is None and only.nearest_dir is None
    assert np.array_equal(bits(only.moments), bits(mirror(sc, p, nm, flags, keys, L, rot, 1e-3, 4, 2.5, 0.0)[0]))


def test_probes_at_free_points_are_points_with_the_z_normal(gpu):
    sc = scene("room")
    pos = seven_points("room")[0][:6]
    L = nr.sphere_dirs(100)
    got = sc.probe_depth(pos, L, 8, 3.0, 0.5)
    nz = np.tile([0.0, 0.0, 1.0], (6, 1))
    same_depth(got, mirror(sc, pos, nz, None, None, L, None, 0.0, 8, 3.0, 0.5))
    rd = nr.occlusion_rays(pos, nz, L, None, 0.0)[1]
    assert np.array_equal(bits(rd), bits(np.broadcast_to(L, rd.shape)))  # that frame reproduces the table


@pytest.mark.parametrize("k", [5, 64, 100])
def test_every_number_of_lanes_per_point_gives_the_same_bits(gpu, k, monkeypatch):
    p, nm, flags, keys = seven_points("room")
    L, rot = nr.sphere_dirs(k), nr.rotation_table(3)
    want = nr.probe_depth_points(scene("room"), p, nm, L, 8, 2.5, 1.25, rot, 1e-3, flags, keys)
    for lanes in ("0", "3", "6"):
        monkeypatch.setenv("NRAYS_OCCLUSION_LANES", lanes)  # read when the handle is created
        same_depth(nr.probe_depth_points(room_scene(), p, nm, L, 8, 2.5, 1.25, rot, 1e-3, flags, keys), want, lanes)
    for lanes in ("0", "6"):
        monkeypatch.setenv("NRAYS_OCCLUSION_LANES", lanes)
        pc, nc, fc, kc = seven_points("cube")
        same_depth(nr.probe_depth_points(cube_mesh_scene(), pc, nc, L, 16, 2.5, 1.25, rot, 1e-3, fc, kc),
                   nr.probe_depth_points(scene("cube"), pc, nc, L, 16, 2.5, 1.25, rot, 1e-3, fc, kc), lanes)


def test_a_chunk_seam_changes_nothing(gpu):
    """num_dirs = 1024: a chunk holds 4096 probes, so probe 4096 of n = 4097 is the first of a second chunk.  The positions repeat with period 7, and a probe reads no
    key (no rotations): every probe must be its residue's result."""
    sc = nr.Scene([nr.SceneNode(su.default_material(), 0.0, 0.0, 1.0, 1.0, nr.Isometry3((0.25, 0.0, -0.5)), nr.Ball(1.0))], [nr.Light((0.0, 5.0, 0.0), 0.0, 1, (1, 1, 1))],
                  (0.0, 0.0, 0.0))
    seven = np.array([(0.25, 0.0, -0.5), (2.0, 0.0, 0.0), (0.0, 3.0, 0.0), (-1.5, -1.5, 1.0), (0.25, 1.0, -0.5), (0.0, 0.0, 6.0), (1.0, 0.5, -0.25)], np.float64)
    n = 4097
    pos = np.ascontiguousarray(np.tile(seven, (-(-n // 7), 1))[:n])
    L = nr.sphere_dirs(1024)
    got = sc.probe_depth(pos, L, 4, 4.0, 1.0)
    same_depth(tuple(a[:7] for a in got), mirror(sc, seven, np.tile([0.0, 0.0, 1.0], (7, 1)), None, None, L, None, 0.0, 4, 4.0, 1.0))
    for a in got:
        assert np.array_equal(bits(a), bits(a[np.arange(n) % 7])), "a probe differs from its residue's"
    assert got.counts[:7, 0].sum() > 0 and got.counts[:7, 1].sum() > 0 and (got.nearest_dir[:7] != 0xFFFFFFFF).all()


def test_the_device_form_on_another_stream_equals_the_blocking_form(gpu):
    import torch
    sc = scene("room")
    p, nm, flags, keys = seven_points("room")
    L, rot = nr.sphere_dirs(100), nr.rotation_table(3)
    want = nr.probe_depth_points(sc, p, nm, L, 8, 2.5, 1.25, rot, 1e-3, flags, keys)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    tp, tn, tf, tk = up(p), up(nm), up(flags.view(np.int32)), up(keys.view(np.int64))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = nr.probe_depth_points(sc, tp, tn, L, 8, 2.5, 1.25, rot, 1e-3, tf, tk)
    s.synchronize()
    assert got.moments.dtype == torch.float32 and got.counts.dtype == torch.int32 and got.nearest.dtype == torch.float64 and got.nearest_dir.dtype == torch.int32
    same_depth(got, want)
    same_depth(nr.probe_depth_points(sc, tp, tn, up(L), 8, 2.5, 1.25, up(rot), 1e-3, tf, tk), want)  # the tables as tensors, torch's current stream
    torch.cuda.synchronize()


def test_statuses(gpu):
    import ctypes as C
    from nrays_amd import abi
    sc = scene("room")
    lib, h = abi.load_hip_lib(), sc.device_handle()
    a = (C.c_double * 3)(0.0, 2.0, 0.0)
    nz = (C.c_double * 3)(0.0, 0.0, 1.0)
    mo = (C.c_float * 32)(*([7.0] * 32))
    adr = C.addressof
    good = dict(num_dirs=1, num_rotations=0, dirs=adr(nz), rotations=None, bias=0.0, max_dist=1.0, near_dist=0.0, res=4, reserved=0)
    call = lambda n=1, flags=0, out=mo, pts=a, **kw: lib.nrays_probe_depth_points(h, n, pts, nz, None, None, C.byref(abi.NraysProbeDepthParams(**dict(good, **kw))), out, None, None,  # noqa: E731
                                                                                None, flags)
    bad = [dict(res=0), dict(res=5), dict(res=32), dict(max_dist=0.0), dict(max_dist=-1.0), dict(max_dist=math.inf), dict(max_dist=math.nan), dict(near_dist=-1.0),
           dict(near_dist=math.inf), dict(near_dist=math.nan), dict(reserved=1), dict(bias=math.nan), dict(num_dirs=0), dict(num_dirs=1025), dict(dirs=None),
           dict(num_rotations=2), dict(flags=1), dict(out=None), dict(pts=None)]
    for kw in bad:
        for n in (0, 1):
            assert call(n=n, **kw) == abi.ERR_BAD_ARG, kw
    assert list(mo) == [7.0] * 32
    assert call(n=0) == abi.OK and list(mo) == [7.0] * 32  # n == 0: the outputs untouched
    assert call() == abi.OK and list(mo) != [7.0] * 32
