"""Incoming light at caller-supplied points (nrays_gather_points_device / nrays_gather_points; nrays_amd.gather_points, gather_hits, bake_indirect) on the
GPU: the fused mean against the fold of trace_rays on the very same rays and keys bit for bit — every scene kind, an area light, every number of lanes per
point —, the double-branching scene within the rounding of a sequential f32 sum, the CPU oracle's expectation (tests/test_gather.py), sizes around a wave and
across the chunk seam, the device path, gather_hits, bake_indirect, skipped points, the statuses, and the handle's render state."""
import ctypes as C
import math

import numpy as np
import pytest

import nrays_amd as nr
from nrays_amd import abi, math3d
from tests.test_gather import SKY, call_args, fold, oracle_case
from tests.test_occlusion import quad_scene
from tests.test_occlusion_gpu import SCENES, STAT_FIELDS, bits, case, hit_points
from tests.test_shade_points import rich_analytic_scene
from tests.test_trace_rays_gpu import _glass_scene
from tools import scenes_util as su

pytestmark = pytest.mark.gpu
ORACLE_TOL = 1e-4  # the project's GPU-against-oracle bound per channel; a mean of k such values keeps it


def scene_flags(sc):
    out = (C.c_uint32 * 2)()
    abi.check(abi.load_hip_lib().nrays_debug_scene_flags(sc.device_handle(), out))
    return out[0]


def ray_colours(sc, points, normals, L, rot, bias, energy, max_depth, keys):
    """The parts that existed before: the mirror's rays through trace_rays with the mirror's keys, (n, k, 3) float32."""
    ro, rd = nr.occlusion_rays(points, normals, L, rot, bias, keys)
    n, k = ro.shape[:2]
    rk = nr.gather_ray_keys(np.arange(n, dtype=np.uint64) if keys is None else keys, k)
    return nr.trace_rays(sc, ro.reshape(-1, 3), rd.reshape(-1, 3), energy=np.full(n * k, energy, np.float32), keys=rk.reshape(-1), max_depth=max_depth).reshape(n, k, 3)


def reference(sc, points, normals, L, rot, bias, energy, max_depth, keys):
    """The definition: those colours folded in numpy f32 in the order of j and divided by float32(k)."""
    return fold(ray_colours(sc, points, normals, L, rot, bias, energy, max_depth, keys))


def device_gather(sc, points, normals, L, rot=None, bias=1e-3, energy=1.0, max_depth=0, hit_flags=None, keys=None, stream=None):
    """gather_points on torch tensors (on `stream` when given), copied back."""
    import torch
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    tp, tn = up(points), up(normals)
    thf = None if hit_flags is None else up(np.ascontiguousarray(hit_flags, dtype=np.uint32).view(np.int32))
    tk = None if keys is None else up(np.ascontiguousarray(keys, dtype=np.uint64).view(np.int64))
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            r = nr.gather_points(sc, tp, tn, L, rot, bias, energy, max_depth, hit_flags=thf, keys=tk)
        stream.synchronize()
    else:
        r = nr.gather_points(sc, tp, tn, L, rot, bias, energy, max_depth, hit_flags=thf, keys=tk)
    torch.cuda.synchronize()
    assert r.dtype == torch.float32 and tuple(r.shape) == (len(points), 3)
    return r.cpu().numpy()


# ---- 1: bit-identity with the parts that existed ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SCENES))
def test_equals_the_fold_of_trace_rays_bit_for_bit(gpu, name):
    c = case(name)
    sc = c["scene"]
    # "analytic" has a node that reflects AND refracts: its second children go through the queue, per ray; the others fold inside the kernel
    assert ((scene_flags(sc) & 8) != 0) == (name == "analytic")
    if name == "hair":
        assert (scene_flags(sc) & ~16) == 2  # opaque meshes only: the kFeatMesh kernels
    bg = np.asarray(sc._background, np.float32)
    seen_sky, seen_hit, by_depth = 0, 0, {}
    for k in (1, 2, 7, 16):
        L = nr.hemisphere_dirs(k)
        for R in (0, 5):
            rot = nr.rotation_table(R) if R else None
            for max_depth in (0, 1):
                for energy in (1.0, 0.15):
                    rays = ray_colours(sc, c["points"], c["normals"], L, rot, 1e-3, energy, max_depth, c["keys"])
                    want = fold(rays)
                    got = nr.gather_points(sc, c["points"], c["normals"], L, rot, 1e-3, energy, max_depth, keys=c["keys"])
                    bad = int((bits(got) != bits(want)).any(axis=1).sum())
                    sky = (rays == bg).all(axis=2)
                    print("%s k = %d R = %d max_depth = %d energy = %g: %d points differ; %d of %d rays see the background" % (name, k, R, max_depth, energy, bad, int(sky.sum()), sky.size))
                    assert got.dtype == np.float32 and got.shape == (320, 3)
                    assert np.array_equal(bits(got), bits(want))
                    seen_sky += int(sky.sum())
                    seen_hit += int((~sky).sum())
                    if k == 16 and R == 5 and energy == 1.0:
                        by_depth[max_depth] = got
    assert seen_sky > 1000 and seen_hit > 1000  # rays that see the background and rays that hit
    if name in ("analytic", "mixed"):  # reflective or half-transparent nodes: the recursion is traced
        assert (bits(by_depth[0]) != bits(by_depth[1])).any()


# ---- 2: an area light reads the per-ray keys -------------------------------------------------------------------------------------------------------------
def test_area_light_reads_the_ray_keys(gpu):
    sc, cam = su.primitives_scene(light_radius=0.1, nsample=3)
    assert (scene_flags(sc) & 8) == 0  # (no queue; the light's radius makes every shaded hit hash its ray's key)
    proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], 40, 30)
    o, d, _ = nr.camera_rays((40, 30), cam["eye"], proj, seed=2)
    hits = nr.closest_hits(sc, o, d, want=("normal", "flags"))
    p, nm = hit_points(o, d, hits)
    sel = np.flatnonzero((hits.flags & 1) != 0)
    sel = sel[np.linspace(0, len(sel) - 1, 320).astype(int)]
    p, nm = np.ascontiguousarray(p[sel]), np.ascontiguousarray(nm[sel])
    keys = case("analytic")["keys"]
    L, rot = nr.hemisphere_dirs(16), nr.rotation_table(5)
    for k_, max_depth in ((16, 0), (16, 1), (7, 0)):
        want = reference(sc, p, nm, L[:k_], rot, 1e-3, 1.0, max_depth, keys)
        got = nr.gather_points(sc, p, nm, L[:k_], rot, 1e-3, 1.0, max_depth, keys=keys)
        print("area light k = %d max_depth = %d: %d points differ" % (k_, max_depth, int((bits(got) != bits(want)).any(axis=1).sum())))
        assert np.array_equal(bits(got), bits(want))
    # other keys, same rotation table: without rotations the rays are the same, only the light samples move
    a = nr.gather_points(sc, p, nm, L, None, 1e-3, 1.0, 0, keys=keys)
    b = nr.gather_points(sc, p, nm, L, None, 1e-3, 1.0, 0, keys=keys + np.uint64(2))
    assert (bits(a) != bits(b)).any()
    assert np.array_equal(bits(b), bits(reference(sc, p, nm, L, None, 1e-3, 1.0, 0, keys + np.uint64(2))))


# ---- 3: lanes per point ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["analytic", "mixed"])
@pytest.mark.parametrize("k", [16, 20, 64, 70])
def test_every_number_of_lanes_per_point_gives_the_same_values(gpu, k, name, monkeypatch):
    """A point gets 8 or 64 lanes (k >= 8, k >= 64), on a forced handle any of 1, 8, 64; k = 20 and 70 leave a partial last round.  All of them are the sequential
    fold: through the wave's shuffles ("mixed") and, where the queue runs, through the per-ray colours ("analytic")."""
    c = case(name)
    L, rot = nr.hemisphere_dirs(k), nr.rotation_table(5)
    n = 257
    p, nm, keys = c["points"][:n], c["normals"][:n], c["keys"][:n]
    want = reference(c["scene"], p, nm, L, rot, 1e-3, 1.0, 1, keys)
    got = nr.gather_points(c["scene"], p, nm, L, rot, 1e-3, 1.0, 1, keys=keys)
    assert np.array_equal(bits(got), bits(want))
    for lanes in ("0", "3", "6"):
        monkeypatch.setenv("NRAYS_OCCLUSION_LANES", lanes)  # read when the handle is created
        sc = SCENES[name]()[0]
        got = nr.gather_points(sc, p, nm, L, rot, 1e-3, 1.0, 1, keys=keys)
        assert np.array_equal(bits(got), bits(want)), lanes


# ---- 4: double-branching scenes --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [7, 16, 64])
def test_double_branching_scene_within_the_rounding_of_the_fold(gpu, k):
    """The queue path.  Bound, per channel, against the f64 mean m64 of the per-ray trace_rays colours c_ij (themselves f32 values), for ANY way of adding the
    queued second children's fixed-point sums to a point — per ray before the fold, or per point after it:
      * a sequential f32 sum of k terms, in any association, is within (k - 1) u S of the exact sum, S = sum_j |c_ij|, u = 2^-24 (Higham, Accuracy and Stability
        of Numerical Algorithms, eq. 4.4, first order);
      * each c_ij is itself one f32 rounding of first pass + queued part; adding those pieces elsewhere moves a term by at most u |c_ij|, u S in all; the
        fixed-point quantum 2^-32 per queued chain is far below that;
      * the division rounds once more: u S / k after dividing.
    Together (k - 1 + 1 + 1) u S / k = (k + 1) u S / k <= (k + 2) u S / k, plus one u absolute for values near zero: |got - m64| <= (k + 2) 2^-24 S / k + 2^-24.
    The library adds the queued sums per RAY, as trace_rays does, so the value is in fact the plain fold bit for bit; that is asserted as well."""
    sc, cam = _glass_scene()
    assert (scene_flags(sc) & 8) != 0  # a node reflects AND refracts: the continuation queue runs
    proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], 40, 30)
    o, d, _ = nr.camera_rays((40, 30), cam["eye"], proj, seed=4)
    hits = nr.closest_hits(sc, o, d, want=("normal", "flags"))
    p, nm = hit_points(o, d, hits)
    sel = np.flatnonzero((hits.flags & 1) != 0)
    sel = sel[np.linspace(0, len(sel) - 1, 320).astype(int)]
    p, nm = np.ascontiguousarray(p[sel]), np.ascontiguousarray(nm[sel])
    keys = case("analytic")["keys"]
    L, rot = nr.hemisphere_dirs(k), nr.rotation_table(5)
    for max_depth in (0, 2):
        rays = ray_colours(sc, p, nm, L, rot, 1e-3, 1.0, max_depth, keys).astype(np.float64)
        m64 = rays.sum(axis=1) / k
        bound = (k + 2) * 2.0 ** -24 * np.abs(rays).sum(axis=1) / k + 2.0 ** -24
        got = nr.gather_points(sc, p, nm, L, rot, 1e-3, 1.0, max_depth, keys=keys)  # (NRAYS_ERR_QUEUE_OVERFLOW would raise)
        err = np.abs(got.astype(np.float64) - m64)
        print("glass k = %d max_depth = %d: max |got - m64| / bound = %.3g; %d of %d values differ from the plain fold" %
              (k, max_depth, float((err / bound).max()), int((bits(got) != bits(fold(rays.astype(np.float32)))).sum()), got.size))
        assert (err <= bound).all()
        assert np.array_equal(bits(got), bits(fold(rays.astype(np.float32))))
        dev = device_gather(sc, p, nm, L, rot, 1e-3, 1.0, max_depth, keys=keys)
        assert np.array_equal(bits(dev), bits(got))  # fixed-point sums: reproducible
    assert (np.abs(rays - np.asarray(sc._background, np.float64)).max(axis=2) > 1e-3).any()


# ---- 5: the oracle's expectation -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_depth", [0, 1])
@pytest.mark.parametrize("name", ["analytic", "quads"])
def test_against_the_cpu_oracle(gpu, name, max_depth):
    c = oracle_case(name)
    got = nr.gather_points(c["scene"], **call_args(c, max_depth))
    err = float(np.abs(got - c["rgb"][max_depth]).max())
    print("%s max_depth = %d: max |hip - oracle| %.3g (bound %.3g)" % (name, max_depth, err, ORACLE_TOL))
    assert err <= ORACLE_TOL


def test_open_sky_is_exactly_the_background(gpu):
    c = oracle_case("sky")
    got = nr.gather_points(c["scene"], **call_args(c, 0))
    assert np.array_equal(bits(got), bits(c["rgb"][0])) and np.array_equal(got, np.tile(np.asarray(SKY, np.float32), (len(got), 1)))
    assert np.array_equal(bits(device_gather(c["scene"], c["points"], c["normals"], c["sample_dirs"], c["rotations"], keys=c["keys"])), bits(got))


# ---- 6: sizes and forms ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, (1 << 22) // 16 + 17])
def test_sizes_pieces_default_keys_and_the_device_path(gpu, n):
    """The 320 points of the analytic case tiled to n, k = 16 with 5 rotations (the keys matter).  Default keys: point i has key i, also across the chunk seam at
    2^22 / 16 points.  The host form against the device form on a stream of its own."""
    import torch
    c = case("analytic")
    sc = c["scene"]
    L, rot = nr.hemisphere_dirs(16), nr.rotation_table(5)
    reps = -(-n // 320)
    p, nm = (np.ascontiguousarray(np.tile(a, (reps, 1))[:n]) for a in (c["points"], c["normals"]))
    host = nr.gather_points(sc, p, nm, L, rot, 1e-3, 1.0, 1)
    assert host.shape == (n, 3) and host.dtype == np.float32
    dev = device_gather(sc, p, nm, L, rot, 1e-3, 1.0, 1, stream=torch.cuda.Stream())
    assert np.array_equal(bits(dev), bits(host))
    if n <= 64:
        assert np.array_equal(bits(device_gather(sc, p, nm, L, rot, 1e-3, 1.0, 1, keys=np.arange(n, dtype=np.uint64))), bits(host))
    else:  # (pieces under explicit keys against one call under the default keys)
        cuts = [0, n // 3, n // 3 + 1, n - 5, n]
        parts = [device_gather(sc, p[a:b], nm[a:b], L, rot, 1e-3, 1.0, 1, keys=np.arange(a, b, dtype=np.uint64)) for a, b in zip(cuts[:-1], cuts[1:])]
        assert np.array_equal(bits(np.concatenate(parts)), bits(host))
    if n <= 320:  # against the definition, under the default keys
        assert np.array_equal(bits(host), bits(reference(sc, p, nm, L, rot, 1e-3, 1.0, 1, None)))
    if n > 640:  # the same point under another key: another rotation somewhere; and the keys continue across the seam
        assert (bits(host[:320]) != bits(host[320:640])).any()
        tail = device_gather(sc, p[-17:], nm[-17:], L, rot, 1e-3, 1.0, 1, keys=np.arange(n - 17, n, dtype=np.uint64))
        assert np.array_equal(bits(tail), bits(host[-17:]))


@pytest.mark.parametrize("name", ["quads", "tiny"])
def test_gather_hits_on_tensors_equals_the_numpy_form(gpu, name):
    import torch
    c = case(name)
    sc, o, d = c["scene"], c["o"], c["d"]
    L, rot = nr.hemisphere_dirs(7), nr.rotation_table(4)
    want = nr.gather_hits(sc, o, d, c["hits"], L, rot, 1e-3, 1.0, 1)
    hit = (c["hits"].flags & 1) != 0
    assert hit.sum() > 300 and (name != "tiny" or (~hit).sum() > 50)  # (the tiny scene's camera sees the sky)
    assert (bits(want[~hit]) == 0).all() and (want[hit] != 0.0).any()
    p, nm = hit_points(o, d, c["hits"])
    direct = nr.gather_points(sc, p, nm, L, rot, 1e-3, 1.0, 1, hit_flags=c["hits"].flags)
    assert np.array_equal(bits(want), bits(direct))
    to, td = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = nr.gather_hits(sc, to, td, nr.closest_hits(sc, to, td), L, rot, 1e-3, 1.0, 1)
    s.synchronize()
    assert np.array_equal(bits(got.cpu().numpy()), bits(want))
    assert np.array_equal(bits(sc.gather_points(p, nm, L, rot, 1e-3, 1.0, 1, hit_flags=c["hits"].flags)), bits(want))  # Scene.gather_points
    with pytest.raises(ValueError):
        nr.gather_hits(sc, to, td, c["hits"], L)  # tensors and arrays mixed


def test_bake_indirect_is_gather_points_on_surface_texels(gpu):
    import torch
    sc, _ = quad_scene()
    L, rot = nr.hemisphere_dirs(16), nr.rotation_table(5)
    for node in (0, 1):
        tx = nr.surface_texels(sc, node, 8, 8, want=("normals",))
        assert (tx.flags & 1).sum() > 16
        want = nr.gather_points(sc, tx.points, tx.normals, L, rot, 1e-3, 1.0, 1, hit_flags=tx.flags)
        got = nr.bake_indirect(sc, node, 8, 8, L, rot, 1e-3, 1.0, 1)
        assert got.shape == (8, 8, 3) and got.dtype == np.float32 and np.array_equal(bits(got.reshape(64, 3)), bits(want))
        assert (bits(got.reshape(64, 3)[(tx.flags & 1) == 0]) == 0).all() and (got != 0.0).any()
        dev = sc.bake_indirect(node, 8, 8, L, rot, 1e-3, 1.0, 1, device=torch.device("cuda", torch.cuda.current_device()))
        torch.cuda.synchronize()
        assert tuple(dev.shape) == (8, 8, 3) and np.array_equal(bits(dev.cpu().numpy()), bits(got))


# ---- 7: skipped points -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mixed", "analytic"])
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("k", [4, 16])
def test_skipped_points_are_zero_and_leave_their_neighbours_alone(gpu, form, k, name):
    """k = 4: a lane per point; k = 16: eight lanes per point.  Alternating flags, NaN points and normals behind the cleared ones.  "mixed" folds inside the kernel;
    "analytic" is double-branching: a skipped point's zeros go through the per-ray colours (a buffer the calls before it have used) and k_gather_fold."""
    c = case(name)
    sc = c["scene"]
    L, rot = nr.hemisphere_dirs(k), nr.rotation_table(5)
    if form == "host":
        run = lambda p, nm, hf, keys: nr.gather_points(sc, p, nm, L, rot, 1e-3, 1.0, 1, hit_flags=hf, keys=keys)  # noqa: E731
    else:
        run = lambda p, nm, hf, keys: device_gather(sc, p, nm, L, rot, 1e-3, 1.0, 1, hit_flags=hf, keys=keys)  # noqa: E731
    n = 130
    p, nm, keys = c["points"][:n].copy(), c["normals"][:n].copy(), c["keys"][:n]
    base = run(p, nm, None, keys)
    assert (base != 0.0).any(axis=1).sum() > n // 2
    assert np.array_equal(bits(run(p, nm, np.full(n, 3, np.uint32), keys)), bits(base))
    skipped = np.arange(n) % 2 == 1
    hf = np.where(skipped, np.asarray([0, 2, 0xfffffffe, 0], np.uint32)[(np.arange(n) // 2) % 4], 1).astype(np.uint32)  # bit 0 clear, whatever else is set
    p[skipped], nm[skipped] = np.nan, np.nan
    p[1] = np.inf
    got = run(p, nm, hf, keys)
    assert (bits(got[skipped]) == 0).all()
    assert np.array_equal(bits(got[~skipped]), bits(base[~skipped]))
    assert (bits(run(p, nm, np.zeros(n, np.uint32), keys)) == 0).all()  # every point skipped


# ---- 8: statuses -----------------------------------------------------------------------------------------------------------------------------------------
def _raw_call(sc, form, n, arrays, params, flags=0, null=(), scene=True):
    """One library call with host or device pointers; returns (status, out_rgb) as numpy arrays."""
    import torch
    lib = abi.load_hip_lib()
    order = ("points", "normals", "hit_flags", "keys", "params", "out_rgb")
    h = sc.device_handle() if scene else None
    if form == "device":
        held = {k: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v.view(np.int32) if v.dtype == np.uint32 else v).cuda() for k, v in arrays.items()}
        tables = {k: None if params[k] is None else torch.from_numpy(np.ascontiguousarray(params[k], dtype=np.float64)).cuda() for k in ("dirs", "rotations")}
        adr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        ptrs = {k: adr(t) for k, t in held.items()}
    else:
        ct = {np.dtype(np.float64): C.c_double, np.dtype(np.uint32): C.c_uint32, np.dtype(np.uint64): C.c_uint64, np.dtype(np.float32): C.c_float}
        tables = {k: None if params[k] is None else np.ascontiguousarray(params[k], dtype=np.float64) for k in ("dirs", "rotations")}
        adr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        ptrs = {k: v.ctypes.data_as(C.POINTER(ct[v.dtype])) for k, v in arrays.items()}
    st = abi.NraysGatherParams(params["num_dirs"], params["num_rotations"], adr(tables["dirs"]), adr(tables["rotations"]), params["bias"], params["energy"], params["max_depth"])
    ptrs["params"] = C.byref(st)
    args = [None if k in null else ptrs[k] for k in order]
    if form == "device":
        rc = lib.nrays_gather_points_device(h, n, *args, flags, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc, held["out_rgb"].cpu().numpy()
    return lib.nrays_gather_points(h, n, *args, flags), arrays["out_rgb"]


@pytest.mark.parametrize("form", ["host", "device"])
def test_statuses(gpu, form):
    c = case("analytic")
    sc, n, k, R = c["scene"], 16, 8, 3
    arrays = dict(points=c["points"][:n].copy(), normals=c["normals"][:n].copy(), hit_flags=np.ones(n, np.uint32), keys=c["keys"][:n].copy(), out_rgb=np.full((n, 3), 7.0, np.float32))
    params = dict(num_dirs=k, num_rotations=R, dirs=nr.hemisphere_dirs(k), rotations=nr.rotation_table(R), bias=1e-3, energy=1.0, max_depth=1)
    call = lambda **kw: _raw_call(sc, form, kw.pop("n", n), arrays, dict(params, **kw.pop("p", {})), **kw)  # noqa: E731
    for flags in (1, 2, 1 << 31, 3):
        assert call(flags=flags)[0] == abi.ERR_BAD_ARG, flags
    for name in ("points", "normals", "params", "out_rgb"):
        assert call(null=(name,))[0] == abi.ERR_BAD_ARG, name
    assert call(scene=False)[0] == abi.ERR_BAD_ARG
    bad_params = [dict(dirs=None), dict(num_dirs=0), dict(num_dirs=1025), dict(num_rotations=1025), dict(rotations=None), dict(bias=math.inf), dict(bias=-math.inf),
                  dict(bias=math.nan), dict(energy=math.inf), dict(energy=-math.inf), dict(energy=math.nan)]
    for p in bad_params:
        assert call(p=p)[0] == abi.ERR_BAD_ARG, p
    rc, out = call(n=0)
    assert rc == abi.OK and (out == 7.0).all()  # without work; nothing so far wrote the output
    assert call(n=0, flags=1)[0] == abi.ERR_BAD_ARG and call(n=0, p=dict(num_dirs=0))[0] == abi.ERR_BAD_ARG
    want = nr.gather_points(sc, arrays["points"], arrays["normals"], params["dirs"], params["rotations"], 1e-3, 1.0, 1, keys=arrays["keys"])
    rc, out = call()
    assert rc == abi.OK and np.array_equal(bits(out), bits(want))
    rc, out = call(null=("hit_flags", "keys"), p=dict(num_rotations=0, rotations=None))  # every point live, key i; no rotation: a NULL table is fine
    assert rc == abi.OK and np.array_equal(bits(out), bits(nr.gather_points(sc, arrays["points"], arrays["normals"], params["dirs"], None, 1e-3, 1.0, 1)))


# ---- 9: the handle's state -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["analytic", "glass"])
def test_a_batch_leaves_the_render_state_alone(gpu, name):
    import torch
    make = {"analytic": rich_analytic_scene, "glass": _glass_scene}[name]
    c = case("analytic")  # (points near the glass scene's shapes too: both scenes sit around the origin)
    L, rot = nr.hemisphere_dirs(16), nr.rotation_table(5)
    w, h = 128, 72

    def frames_and_stats(sc, cam, batch):
        proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], w, h)
        first = nr.render(sc, (w, h), 1, 0.0, cam["eye"], proj)
        st1, perm = nr.get_stats(sc), nr.last_permutation(sc)
        got = device_gather(sc, c["points"], c["normals"], L, rot, 1e-3, 1.0, 2, keys=c["keys"], stream=torch.cuda.Stream()) if batch else None
        assert nr.last_permutation(sc) == perm
        second = nr.render(sc, (w, h), 1, 0.0, cam["eye"], proj)
        assert nr.last_permutation(sc) == perm
        return first, second, st1, nr.get_stats(sc), got

    plain = frames_and_stats(*make(), batch=False)
    mixed = frames_and_stats(*make(), batch=True)
    other, _ = make()
    assert np.array_equal(bits(mixed[4]), bits(nr.gather_points(other, c["points"], c["normals"], L, rot, 1e-3, 1.0, 2, keys=c["keys"])))  # (after a render, on another stream)
    assert (mixed[4] != 0.0).any()
    for a, b in zip(plain[:2], mixed[:2]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    for st_plain, st_mixed in zip(plain[2:4], mixed[2:4]):
        for fld in STAT_FIELDS:
            assert getattr(st_plain, fld) == getattr(st_mixed, fld), fld
