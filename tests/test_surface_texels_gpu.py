"""The surface of a mesh node at a light map's texels on the GPU (nrays_surface_texels_device / nrays_surface_texels; surface_texels_kernel.h): the device against
the numpy mirror of the definition bit for bit (nrays_amd.surface_texels_ref), every way the owner pass splits its work, pre-split triangles, merged BLASes,
agreement with the closest-hit query, the downstream calls fed unfiltered, bake_lightmap, the NULL outputs, the statuses, and the handle's render state."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import nrays_amd as nr
from nrays_amd import abi, math3d
from tests.test_surface_texels import CAST_LATTICES, LATTICES, jittered_grid, one_triangle, quad
from tools import scenes_util as su

pytestmark = pytest.mark.gpu
STAT_FIELDS = ("rays_primary", "rays_reflection", "rays_refraction", "rays_shadow", "rays_shadow_elided", "rays_primary_traced", "generations")
FIELDS = nr.SurfaceTexels._fields
SKEW = nr.Isometry3((0.75, -1.5, 2.25), (0.4, -0.9, 0.3))  # a rotation about a skew axis, and a translation


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same_bits(got, want, fields=FIELDS):
    for k in fields:
        g, w = np.asarray(getattr(got, k)), np.asarray(getattr(want, k))
        assert g.shape == w.shape and np.array_equal(bits(g), bits(w)), (k, int((bits(g) != bits(w)).sum()))


def material():
    return nr.PhongMaterial((0.2, 0.2, 0.2), (0.9, 0.8, 0.7), (0.5, 0.5, 0.5), su.checker_texture(64, 8), None, 30.0)


LIGHTS = (nr.Light((1.0, 6.0, -2.0), 0.0, 1, (0.9, 0.9, 0.8)), nr.Light((-3.0, 4.0, 3.0), 0.5, 4, (0.4, 0.5, 0.6)))  # one point light, one area light


def scene_of(*meshes, lights=LIGHTS[:1]):
    """One node per (points, indices, uvs[, isometry]) tuple."""
    nodes = [nr.SceneNode(material(), 0.0, 0.0, 1.0, 1.0, (m[3] if len(m) > 3 else nr.Isometry3()), nr.TriMesh(m[0], m[1], m[2])) for m in meshes]
    return nr.Scene(nodes, list(lights), (0.1, 0.2, 0.3))


# ---- 1, 2: bit equality -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flip", (False, True))
@pytest.mark.parametrize("centres", LATTICES)
@pytest.mark.parametrize("mesh,size", [("triangle", (4, 4)), ("triangle", (5, 3)), ("quad", (7, 5)), ("quad", (1, 1)), ("quad", (1, 4)), ("quad", (64, 33))])
def test_simple_shapes_equal_the_mirror_bit_for_bit(gpu, mesh, size, centres, flip):
    m = one_triangle() if mesh == "triangle" else quad()
    got = nr.surface_texels(scene_of(m), 0, *size, centres=centres, flip_normals=flip)
    want = nr.surface_texels_ref(*m, None, *size, centres=centres, flip_normals=flip)
    assert (want.flags == 3).any() and got.flags.dtype == np.uint32
    same_bits(got, want)


@pytest.mark.parametrize("centres", LATTICES)
@pytest.mark.parametrize("size", [(64, 64), (301, 173)])
def test_the_jittered_grid_equals_the_mirror(gpu, size, centres):
    m = jittered_grid()
    same_bits(nr.surface_texels(scene_of(m), 0, *size, centres=centres), nr.surface_texels_ref(*m, None, *size, centres=centres))
    shifted = nr.Isometry3((0.75, -1.5, 2.25))  # identity rotation: p + t, still bit for bit
    same_bits(nr.surface_texels(scene_of(m + (shifted,)), 0, *size, centres=centres), nr.surface_texels_ref(*m, shifted, *size, centres=centres))
    got, want = nr.surface_texels(scene_of(m + (SKEW,)), 0, *size, centres=centres), nr.surface_texels_ref(*m, SKEW, *size, centres=centres)
    same_bits(got, want, ("uv", "node", "prim", "flags"))
    M = max(1.0, float(np.abs(want.points).max()))
    err_p, err_n = float(np.abs(got.points - want.points).max()), float(np.abs(got.normals - want.normals).max())
    print("rotated grid %s centres=%s: |dp| %.3g (M %.3g), |dn| %.3g" % (size, centres, err_p, M, err_n))
    assert err_p <= 1e-13 * M and err_n <= 1e-13 * M


# ---- 3: every way the work is split ---------------------------------------------------------------------------------------------------------------------------------
def _small_triangles(n, seed):
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.02, 0.98, size=(n, 1, 2))
    uv = su.f32_exact((c + rng.uniform(-0.02, 0.02, size=(n, 3, 2))).reshape(-1, 2))
    p = su.f32_exact(np.concatenate([uv * 4.0 - 2.0, rng.uniform(-1.0, 1.0, size=(3 * n, 1))], axis=1))
    return p, np.arange(3 * n, dtype=np.uint32).reshape(n, 3), uv


def _with_big(small, first):
    """`small` and ONE triangle whose uv box is the whole lattice (and more), declared first or last."""
    p, idx, uv = small
    bp, buv = su.f32_exact([[-9, 5, -9], [9, 5, -9], [-9, 5, 9]]), su.f32_exact([[0, 0], [2, 0], [0, 2]])
    if first:
        return np.concatenate([bp, p]), np.concatenate([[[0, 1, 2]], idx + 3]).astype(np.uint32), np.concatenate([buv, uv])
    n = len(p)
    return np.concatenate([p, bp]), np.concatenate([idx, [[n, n + 1, n + 2]]]).astype(np.uint32), np.concatenate([uv, buv])


def _sweep_items():
    """Items one sweep of k_texel_owner's grid takes: 4 workgroups per CU, 4 waves each, 64 items per wave and trip (surface_texels_kernel.h)."""
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count * 4 * 4 * 64


@pytest.mark.parametrize("path", ["many_tiles_big_last", "many_tiles_big_first", "scan_blocks", "grid_stride"])
def test_every_way_of_splitting_the_work_equals_the_mirror(gpu, path):
    """many_tiles: one record of 64 x 64 tiles beside 3 000 records of one to four; big_last: the small ones win where they cover, big_first: the big one wins everywhere.
    scan_blocks: more records than three workgroups of the scan hold (4 096 each).  grid_stride: more items than one sweep of the owner pass's fixed grid, so its waves take
    a second trip."""
    if path.startswith("many_tiles"):
        first = path.endswith("first")
        m, size = _with_big(_small_triangles(3000, 5), first), (512, 512)
    elif path == "scan_blocks":
        m, size = _with_big(_small_triangles(9000, 6), False), (512, 512)
        assert len(m[1]) > 2 * 4096
    else:
        side = 2048
        corners = [[[0, 0], [2, 0], [0, 2]], [[1, 1], [-1, 1], [1, -1]]]
        k = 1 + -(-_sweep_items() // ((side // 8) ** 2))  # triangles whose box is the whole lattice: 256 x 256 tiles each
        uv = su.f32_exact(np.concatenate([np.asarray(corners[i % 2], np.float64) * (1.0 + 0.01 * (i // 2)) for i in range(k)]))
        p = su.f32_exact(np.concatenate([uv, np.repeat(np.arange(k, dtype=np.float64), 3)[:, None]], axis=1))
        m, size = (p, np.arange(3 * k, dtype=np.uint32).reshape(k, 3), uv), (side, side)
        assert k * (side // 8) ** 2 > _sweep_items()
    got, want = nr.surface_texels(scene_of(m), 0, *size), nr.surface_texels_ref(*m, None, *size)
    same_bits(got, want)
    if path.startswith("many_tiles"):
        big = 0 if first else len(m[1]) - 1
        assert (want.flags == 3).all()
        assert (want.prim == big).all() if first else (0 < (want.prim == big).sum() < want.prim.size and len(np.unique(want.prim)) > 2000)


# ---- 4: several leaf references to one triangle ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sliver_mesh():
    """2 304 triangles with an atlas of their own: 2 048 small ones and 256 long thin slivers across the whole mesh, which the builders pre-split."""
    p, idx, uv = _small_triangles(2048, 8)
    rng = np.random.default_rng(9)
    k = 256
    a = rng.uniform(0.0, 1.0, size=(k, 2))
    d = rng.normal(size=(k, 2)); d /= np.sqrt((d * d).sum(axis=1))[:, None]
    suv = np.stack([a - 0.6 * d, a + 0.6 * d, a + 0.6 * d + 0.004 * d[:, ::-1] * [1, -1]], axis=1).reshape(-1, 2)
    suv = su.f32_exact(suv)
    sp = su.f32_exact(np.concatenate([suv * 4.0 - 2.0, rng.uniform(-1.0, 1.0, size=(k, 1)).repeat(3, axis=0)], axis=1))
    return np.concatenate([p, sp]), np.concatenate([idx, np.arange(3 * k, dtype=np.uint32).reshape(k, 3) + len(p)]).astype(np.uint32), np.concatenate([uv, suv])


def _num_refs(mesh, device):
    p, idx, uv = mesh
    m = abi.NraysMesh(len(p), len(idx), p.ctypes.data_as(C.POINTER(C.c_double)), uv.ctypes.data_as(C.POINTER(C.c_double)), idx.ctypes.data_as(C.POINTER(C.c_uint32)))
    cap = 16 * len(idx)
    nodes, tri = np.zeros((cap, 32), np.float32), np.zeros(cap, np.uint32)
    d = abi.NraysBlasDump()
    d.node_capacity = cap; d.ref_capacity = cap
    d.nodes = nodes.ctypes.data_as(C.POINTER(C.c_float)); d.tri_ids = tri.ctypes.data_as(C.POINTER(C.c_uint32))
    abi.check(abi.load_hip_lib().nrays_debug_blas_build(C.byref(m), 1 if device else 0, C.byref(d)))
    assert set(tri[:d.num_refs].tolist()) == set(range(len(idx)))
    return d.num_refs


@pytest.mark.parametrize("builder", ["device", "host"])
def test_a_pre_split_triangle_counts_once(gpu, monkeypatch, builder):
    mesh = _sliver_mesh()
    assert len(mesh[1]) >= 2000 and _num_refs(mesh, builder == "device") > len(mesh[1])
    if builder == "host":
        monkeypatch.setenv("NRAYS_GPU_BUILD", "0")
    want = nr.surface_texels_ref(*mesh, None, 256, 192)
    assert len(np.unique(want.prim[want.prim >= 2048])) > 200  # the slivers own lattice points
    same_bits(nr.surface_texels(scene_of(mesh), 0, 256, 192), want)


# ---- 5: a BLAS that merges nodes; nodes without a surface to sample -------------------------------------------------------------------------------------------------
def test_a_merged_blas_yields_only_the_nodes_own_triangles(gpu):
    q, g = quad(), jittered_grid()
    lifted = (su.f32_exact(g[0] + np.asarray([0.0, 2.0, 0.0])),) + g[1:]
    ball = nr.SceneNode(nr.NormalMaterial(), 0.0, 0.0, 1.0, 1.0, nr.Isometry3((5.0, 0.0, 0.0)), nr.Ball(0.5))
    bare = nr.SceneNode(material(), 0.0, 0.0, 1.0, 1.0, SKEW, nr.TriMesh(q[0], q[1], None))
    sc = scene_of(q + (SKEW,), lifted + (SKEW,))  # two mesh nodes under one isometry: one BLAS, TriRec::node_id tells them apart
    sc = nr.Scene(sc._nodes + [ball, bare], list(LIGHTS[:1]), (0.1, 0.2, 0.3))
    for node, m in ((1, lifted), (0, q)):
        got, want = nr.surface_texels(sc, node, 61, 47), nr.surface_texels_ref(*m, SKEW, 61, 47, node=node)
        same_bits(got, want, ("uv", "node", "prim", "flags"))
        assert (got.node[got.flags == 3] == node).all() and got.prim.max() == len(m[1]) - 1
        assert np.abs(got.points - want.points).max() <= 1e-13 * max(1.0, np.abs(want.points).max()) and np.abs(got.normals - want.normals).max() <= 1e-13
    for node in (2, 3):
        with pytest.raises(abi.NraysError) as e:
            nr.surface_texels(sc, node, 8, 8)
        assert e.value.status == abi.ERR_UNSUPPORTED


# ---- 6: the casts find what the texels hold -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iso", [None, SKEW], ids=["plain", "skew"])
@pytest.mark.parametrize("size,centres", CAST_LATTICES)
def test_the_closest_hit_query_finds_the_texels(gpu, size, centres, iso):
    m = jittered_grid()
    sc = scene_of(m + ((iso,) if iso else ()))
    tx = nr.surface_texels(sc, 0, *size, centres=centres)
    _, wts = nr.surface_texels_ref(*m, iso, *size, centres=centres, with_weights=True)
    take = (tx.flags == 3) & (wts.min(axis=1) > 1e-9)  # (edge texels may belong to either neighbour)
    assert take.sum() >= 0.95 * (tx.flags == 3).sum()
    p, n = tx.points[take], tx.normals[take]
    hits = nr.closest_hits(sc, p + n * 1e-3, -n)
    dn, dt, duv = np.abs(hits.normal - n).max(), np.abs(hits.toi - 1e-3).max(), np.abs(hits.uv - tx.uv[take]).max()
    print("casts %s centres=%s %s: %d of %d compared, |dn| %.3g, |dtoi| %.3g, |duv| %.3g" % (size, centres, "skew" if iso else "plain", take.sum(), (tx.flags == 3).sum(), dn, dt, duv))
    assert np.array_equal(hits.node, tx.node[take]) and np.array_equal(hits.prim, tx.prim[take]) and (hits.flags == 3).all()
    assert dn <= 1e-15 and dt <= 1e-12 and duv <= 1e-12


# ---- 7: the downstream calls, unfiltered ------------------------------------------------------------------------------------------------------------------------------
def _bake_scene():
    """The jittered grid (untransformed) with holes in its atlas (every fifth triangle left out), under an occluder quad, one point and one area light."""
    p, idx, uv = jittered_grid()
    keep = np.arange(len(idx)) % 5 != 0
    q = quad()
    roof = (su.f32_exact(q[0][:, [0, 2, 1]] * 1.5 + [-0.75, 1.5, -0.75]), q[1], q[2])
    return scene_of((p, np.ascontiguousarray(idx[keep]), uv), roof, lights=LIGHTS), (p, np.ascontiguousarray(idx[keep]), uv)


OCCLUSION = (nr.hemisphere_dirs(8), nr.rotation_table(5), 1e-3, math.inf)


@pytest.mark.parametrize("size", [(64, 64), (77, 41)])
def test_shading_and_occlusion_take_the_device_arrays_unfiltered(gpu, size):
    sc, m = _bake_scene()
    got, want = nr.surface_texels(sc, 0, *size, flip_normals=True), nr.surface_texels_ref(*m, None, *size, flip_normals=True)  # (the grid's triangles face down: flipped, they face the lights)
    same_bits(got, want)
    covered = want.flags == 3
    assert 0.5 < covered.mean() < 0.95 and (want.normals[covered, 1] > 0).all()
    lit = [nr.shade_points(sc, t.points, t.normals, -t.normals, t.node, uvs=t.uv, hit_flags=t.flags) for t in (got, want)]
    assert np.array_equal(bits(lit[0]), bits(lit[1])) and not lit[0][~covered].any() and (lit[0][covered, :3] > 0).any()
    occ = [nr.occlusion_points(sc, t.points, t.normals, *OCCLUSION, hit_flags=t.flags) for t in (got, want)]
    assert np.array_equal(bits(occ[0].filter), bits(occ[1].filter)) and np.array_equal(occ[0].open, occ[1].open)
    assert not occ[0].filter[~covered].any() and not occ[0].open[~covered].any() and occ[0].open[covered].min() < occ[0].open[covered].max() <= 8


@pytest.mark.parametrize("occlusion", [None, OCCLUSION], ids=["lit", "lit_x_occlusion"])
def test_bake_lightmap_is_the_composition(gpu, occlusion):
    import torch
    sc, m = _bake_scene()
    w, h = 77, 41
    tx = nr.surface_texels(sc, 0, w, h)
    want = nr.shade_points(sc, tx.points, tx.normals, -tx.normals, tx.node, uvs=tx.uv, hit_flags=tx.flags)
    if occlusion:
        want[:, :3] = want[:, :3] * nr.occlusion_points(sc, tx.points, tx.normals, *occlusion, hit_flags=tx.flags).filter
    want = want.reshape(h, w, 4)
    got = nr.bake_lightmap(sc, 0, w, h, occlusion=occlusion)
    assert got.shape == (h, w, 4) and got.dtype == np.float32 and np.array_equal(bits(got), bits(want))
    assert not got[tx.flags.reshape(h, w) == 0].any() and (got[tx.flags.reshape(h, w) == 3, 3] == 1.0).all()
    dev = sc.bake_lightmap(0, w, h, occlusion=occlusion, device="cuda")
    assert dev.is_cuda and dev.dtype == torch.float32 and np.array_equal(bits(dev.cpu().numpy()), bits(want))
    flipped = nr.bake_lightmap(sc, 0, w, h, occlusion=occlusion, centres=True, flip_normals=True)  # the underside: lit by neither light from above
    assert flipped.shape == (h, w, 4) and not np.array_equal(flipped, got)


# ---- 8: the interface -----------------------------------------------------------------------------------------------------------------------------------------------
def test_every_optional_output_may_be_null(gpu):
    import torch
    sc = scene_of(jittered_grid() + (SKEW,))
    w, h = 37, 29
    full = nr.surface_texels(sc, 0, w, h)
    for leave in nr.scene.TEXEL_OUTPUTS:
        want_names = tuple(k for k in nr.scene.TEXEL_OUTPUTS if k != leave)
        for device in (None, "cuda"):
            got = nr.surface_texels(sc, 0, w, h, want=want_names, device=device)
            assert getattr(got, leave) is None
            for k in (f for f in FIELDS if f != leave):
                v, ref = getattr(got, k), getattr(full, k)
                v = (v.cpu().numpy() if device else v).view(ref.dtype)  # (flags: int32 tensors, uint32 arrays)
                assert np.array_equal(bits(v), bits(ref)), (leave, k, device)
    only = nr.surface_texels(sc, 0, w, h, want=(), device="cuda")
    assert only.normals is None and only.prim is None and np.array_equal(bits(only.points.cpu().numpy()), bits(full.points)) and only.flags.dtype == torch.int32


def test_statuses(gpu):
    import torch
    lib = abi.load_hip_lib()
    sc = scene_of(quad())
    h = sc.device_handle()
    p, f = np.full((16, 3), 7.0), np.full(16, 7, np.uint32)
    dp, df = torch.full((16, 3), 7.0, dtype=torch.float64, device="cuda"), torch.full((16,), 7, dtype=torch.int32, device="cuda")
    pp, fp = p.ctypes.data_as(C.POINTER(C.c_double)), f.ctypes.data_as(C.POINTER(C.c_uint32))

    def both(node, w, hh, points, flags_out, flags):
        a = lib.nrays_surface_texels(h, node, w, hh, pp if points else None, None, None, None, None, fp if flags_out else None, flags)
        b = lib.nrays_surface_texels_device(h, node, w, hh, dp.data_ptr() if points else None, None, None, None, None, df.data_ptr() if flags_out else None, flags, None)
        assert a == b
        return a
    assert both(0, 4, 4, True, True, 0) == abi.OK and both(0, 4, 4, True, True, 3) == abi.OK
    p[:], f[:] = 7.0, 7
    dp[:], df[:] = 7.0, 7
    for args in ((0, 4, 4, False, True, 0), (0, 4, 4, True, False, 0), (1, 4, 4, True, True, 0), (0, 0, 4, True, True, 0), (0, 4, 0, True, True, 0), (0, 16385, 1, True, True, 0),
                 (0, 1, 16385, True, True, 0), (0, 8192, 4096, True, True, 0), (0, 4, 4, True, True, 4), (0, 4, 4, True, True, 0x80000001)):
        assert both(*args) == abi.ERR_BAD_ARG, args
        assert lib.nrays_last_error()
    torch.cuda.synchronize()
    assert (p == 7.0).all() and (f == 7).all() and bool((dp == 7.0).all()) and bool((df == 7).all())  # a refused call writes nothing
    ms = np.zeros(2, np.float32)
    assert lib.nrays_debug_surface_texels_passes(h, 0, 4, 4, 0, 0, ms.ctypes.data_as(C.POINTER(C.c_float))) == abi.ERR_BAD_ARG
    assert lib.nrays_debug_surface_texels_passes(h, 0, 4, 4, 0, 1, None) == abi.ERR_BAD_ARG
    assert nr.surface_texels_passes(sc, 0, 16, 16, repeats=2).shape == (2, 2)
    empty = scene_of((quad()[0], np.zeros((0, 3), np.uint32), quad()[2]))  # a mesh without triangles: every point uncovered
    t = nr.surface_texels(empty, 0, 5, 4)
    assert not t.flags.any() and (t.node == -1).all() and (t.prim == -1).all() and not t.points.any()


def test_a_call_leaves_the_render_state_alone(gpu):
    import torch
    sc, cam = su.mesh_scene(alpha_mapped=True, rotate=True)  # node 0: the textured torus, in a BLAS with the floor; node 2 is half transparent (its records exist twice)
    pts, idx, uvs = su.torus_mesh()
    iso = sc._nodes[0].transform
    want = nr.surface_texels_ref(pts, idx, uvs, iso, 96, 48)
    w, h = 128, 72
    proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], w, h)
    first = nr.render(sc, (w, h), 1, 0.0, cam["eye"], proj)
    st1, perm1 = nr.get_stats(sc), nr.last_permutation(sc)
    with torch.cuda.stream(torch.cuda.Stream()):  # after a render, on another stream
        got = nr.surface_texels(sc, 0, 96, 48, device="cuda")
        torch.cuda.current_stream().synchronize()
    assert np.array_equal(got.prim.cpu().numpy(), want.prim) and np.array_equal(got.flags.cpu().numpy().astype(np.uint32), want.flags)
    assert np.abs(got.points.cpu().numpy() - want.points).max() <= 1e-13 * max(1.0, np.abs(want.points).max())
    assert nr.last_permutation(sc) == perm1
    second = nr.render(sc, (w, h), 1, 0.0, cam["eye"], proj)
    st2 = nr.get_stats(sc)
    assert np.array_equal(first.view(np.uint32), second.view(np.uint32)) and nr.last_permutation(sc) == perm1
    for fld in STAT_FIELDS:
        assert getattr(st1, fld) == getattr(st2, fld), fld
