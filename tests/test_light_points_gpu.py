"""Direct light at caller-supplied points from a caller-supplied table of point lights (nrays_light_points_device / nrays_light_points; nrays_amd.light_points,
light_hits) on the GPU: the library's own rays and weights against the numpy mirror bit for bit (nrays_debug_light_rays), the fused outputs against the fold of
intersects_rays on those very rays bit for bit under every number of lanes per point, the CPU oracle's expectation (tests/test_light_points.py), shade_points on a
scene whose materials make the two definitions the same arithmetic, sizes around a wave and across the chunk seam, skipped points, the NULL output, the device
path, light_hits, the statuses, the handle's render state, and one physical picture."""
import ctypes as C
import math

import numpy as np
import pytest

import nrays_amd as nr
from nrays_amd import abi, math3d
from tests.test_light_points import BAD_LIGHTS, F32_EPS, fold, light_oracle_case, lights_struct
from tests.test_occlusion import SPECIAL_NORMALS, unit_normals
from tests.test_occlusion_gpu import SCENES, STAT_FIELDS, bits, case, hit_points
from tests.test_shade_points import rich_analytic_scene
from tools import scenes_util as su

pytestmark = pytest.mark.gpu
LIGHT_COUNTS = (1, 7, 8, 9, 63, 64, 65, 200)  # one lane a point below 8 lights, 8 lanes below 64, 64 lanes from there; full and partial rounds of each


def case_lights(name, m, seed=0):
    """m lights in and around the scene's 320 surface points (inside its shapes too: blocked and filtered pairs), emitter normals and falloff on every other count."""
    c = case(name)
    rng = np.random.default_rng(1000 * seed + m)
    lo, hi = c["points"].min(axis=0), c["points"].max(axis=0)
    pad = 0.35 * (hi - lo) + 0.5
    pos = rng.uniform(lo - pad, hi + pad, size=(m, 3))
    col = rng.uniform(-0.2, 1.5, size=(m, 3)).astype(np.float32)  # (a negative channel: the sum is no sum of magnitudes)
    en = unit_normals(rng, m) if m % 2 else None
    return nr.PointLights(pos, col, en, m % 3 == 0, 0.5, 1e-3, 1e-3)


_REFS = {}


def reference(name, m):
    """light_points_ref at the scene's 320 points under case_lights(name, m): computed once and shared, nothing writes it."""
    if (name, m) not in _REFS:
        c = case(name)
        L = case_lights(name, m)
        _REFS[name, m] = (L, nr.light_points_ref(c["scene"], c["points"], c["normals"], L))
    return _REFS[name, m]


def device_light(sc, points, normals, lights, hit_flags=None, want_counts=True, stream=None):
    """light_points on torch tensors (on `stream` when given), copied back: (rgb, counts uint32 or None)."""
    import torch
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    tp, tn = up(points), up(normals)
    thf = None if hit_flags is None else up(np.ascontiguousarray(hit_flags, dtype=np.uint32).view(np.int32))
    run = lambda: nr.light_points(sc, tp, tn, lights, hit_flags=thf, want_counts=want_counts)  # noqa: E731
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            r = run()
        stream.synchronize()
    else:
        r = run()
    torch.cuda.synchronize()
    assert r.rgb.dtype == torch.float32 and tuple(r.rgb.shape) == (len(points), 3)
    assert r.counts is None or (r.counts.dtype == torch.int32 and tuple(r.counts.shape) == (len(points), 2))
    return r.rgb.cpu().numpy(), None if r.counts is None else r.counts.cpu().numpy().view(np.uint32)


def same(got, want):
    return np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(got[1], want[1])


# ---- 1: the library's rays and weights are the mirror's ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("emitters", [False, True])
@pytest.mark.parametrize("falloff", [False, True])
def test_probe_rays_equal_the_mirror_bit_for_bit(gpu, emitters, falloff):
    """The check that finds a contracted or reordered operation: every double and every float of every (point, light) pair, by bit pattern."""
    c = case("analytic")
    rng = np.random.default_rng(11)
    nm = np.concatenate([c["normals"], unit_normals(rng, 3000), SPECIAL_NORMALS])
    p = np.concatenate([c["points"], rng.uniform(-50.0, 50.0, size=(len(nm) - len(c["points"]), 3))])
    m = 11
    pos = rng.uniform(-8.0, 8.0, size=(m, 3))
    pos[0] = p[5]  # with bias 0: a light at the point itself
    pos[1] = p[6] + np.cross(nm[6], (0.3, 0.5, 0.7))  # (about) in a tangent plane
    col = rng.uniform(0.0, 2.0, size=(m, 3)).astype(np.float32)
    en = unit_normals(rng, m) if emitters else None
    for bias in (0.0, 0.37):
        for offset in (0.0, 1e-3):
            L = nr.PointLights(pos, col, en, falloff, 3.0, bias, offset)
            mirror = nr.light_rays(p, nm, L)
            probe = nr.light_ray_probe(c["scene"], p, nm, L)
            differ = [int((bits(a) != bits(b)).sum()) for a, b in zip(mirror, probe)]
            print("emitters %s falloff %s bias %g offset %g: origins / dirs / t_max / w differ at %s of %d pairs; %d skipped" % (emitters, falloff, bias, offset, differ, mirror[3].size, int((mirror[3] == 0).sum())))
            assert differ == [0, 0, 0, 0]
            assert 0.15 < (mirror[3] > 0).mean() < 0.7  # skipped and kept pairs both
            if bias == 0.0:
                assert mirror[3][5, 0] == 0 and (mirror[1][5, 0] == 0).all() and mirror[2][5, 0] == 0


# ---- 2: the fused outputs are the fold of intersects_rays on those rays, whatever the lanes ------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SCENES))
def test_equals_the_restatement_bit_for_bit_under_every_lane_form(gpu, name, monkeypatch):
    c = case(name)
    seen = np.zeros(3, np.int64)
    for m in LIGHT_COUNTS:
        L, want = reference(name, m)
        got = nr.light_points(c["scene"], c["points"], c["normals"], L)
        bad = int((bits(got.rgb) != bits(want.rgb)).any(axis=1).sum() + (got.counts != want.counts).any(axis=1).sum())
        print("%s m = %d: %d points differ; pairs %d, with a ray %d, open %d" % (name, m, bad, 320 * m, int(want.counts[:, 0].sum()), int(want.counts[:, 1].sum())))
        assert got.rgb.dtype == np.float32 and got.counts.dtype == np.uint32 and got.counts.shape == (320, 2)
        assert same(got, want)
        seen += (320 * m - int(want.counts[:, 0].sum()), int(want.counts[:, 0].sum() - want.counts[:, 1].sum()), int(want.counts[:, 1].sum()))
    assert (seen > 1000).all()  # skipped, blocked and open pairs, all three
    for lanes in ("0", "3", "6"):
        monkeypatch.setenv("NRAYS_OCCLUSION_LANES", lanes)  # read when the handle is created
        fresh = SCENES[name]()[0]
        for m in LIGHT_COUNTS:
            L, want = reference(name, m)
            assert same(nr.light_points(fresh, c["points"], c["normals"], L), want), (lanes, m)


# ---- 3: the oracle's expectation ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["analytic", "quads"])
def test_against_the_cpu_oracle(gpu, name):
    """The counts exactly; per channel (6 + m) * 2^-24 * sum over the open lights of |col_k| * w_k: 4 for the filter (DESIGN §3's derived bound for a bilinear
    sample), 2 for the two products, m for the f32 sum of m terms."""
    c = light_oracle_case(name)
    m = c["w"].shape[1]
    got = nr.light_points(c["scene"], c["points"], c["normals"], c["lights"])
    bound = (6 + m) * F32_EPS * c["scale"]
    err = np.abs(got.rgb.astype(np.float64) - c["rgb"].astype(np.float64))
    print("%s: max |hip - oracle| %.3g, max err / bound %.3g; counts differ at %d of %d points" % (name, float(err.max()), float((err / np.maximum(bound, 1e-300)).max()),
                                                                                              int((got.counts != c["counts"]).any(axis=1).sum()), len(c["counts"])))
    assert np.array_equal(got.counts, c["counts"])
    assert (err <= bound).all()


# ---- 4: shade_points on a scene where the two definitions are the same arithmetic ----------------------------------------------------------------------------
def lambert_scene():
    """rich_analytic_scene's shapes (three of them half-transparent) with one Phong material of ambient 0, diffuse (1, 1, 1), specular 0 and no texture on every
    node, under three lights of radius 0."""
    base, cam = rich_analytic_scene()
    white = nr.PhongMaterial((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), None, None, 1.0)
    nodes = [nr.SceneNode(white, n.refl_mix, n.refl_atenuation, n.alpha, n.refr_coeff, n.transform, n.geometry) for n in base._nodes]
    lights = [nr.Light((2.0, 6.0, -4.0), 0.0, 1, (0.8, 0.8, 0.7)), nr.Light((-4.0, 3.0, -3.0), 0.0, 1, (0.3, 0.25, 0.4)), nr.Light((0.5, 0.4, 3.5), 0.0, 1, (1.0, 0.5, 0.25))]
    return nr.Scene(nodes, lights, base._background), cam


def test_equals_shade_points_where_the_definitions_coincide(gpu):
    sc, _ = lambert_scene()
    c = case("analytic")  # (the same shapes: its surface points lie on this scene's surfaces)
    hits = c["hits"]
    sel = np.flatnonzero((hits.flags & 1) != 0)
    sel = sel[np.linspace(0, len(sel) - 1, 320).astype(int)]
    assert np.array_equal(hit_points(c["o"], c["d"], hits)[0][sel], c["points"])
    nodes = hits.node[sel]
    L = nr.scene_point_lights(sc, bias=0.0, offset=1e-3)
    assert len(L.positions) == 3
    got = nr.light_points(sc, c["points"], c["normals"], L)
    shaded = nr.shade_points(sc, c["points"], c["normals"], np.ascontiguousarray(c["d"][sel]), nodes)
    bad = int((bits(got.rgb) != bits(shaded[:, :3])).any(axis=1).sum())
    print("light_points against shade_points: %d of 320 points differ; lit points %d, lights with a ray %d, open %d" % (bad, int((got.rgb > 0).any(axis=1).sum()), int(got.counts[:, 0].sum()), int(got.counts[:, 1].sum())))
    assert np.array_equal(bits(got.rgb), bits(np.ascontiguousarray(shaded[:, :3])))
    assert (got.rgb > 0).any(axis=1).sum() > 100 and 0 < got.counts[:, 1].sum() < got.counts[:, 0].sum() < 3 * 320


# ---- 5: sizes ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_sizes_around_a_wave(gpu, n):
    c = case("mixed")
    L, want = reference("mixed", 9)
    got = nr.light_points(c["scene"], c["points"][:n], c["normals"][:n], L)
    assert got.rgb.shape == (n, 3) and got.counts.shape == (n, 2) and same(got, (want.rgb[:n], want.counts[:n]))
    assert same(device_light(c["scene"], c["points"][:n], c["normals"][:n], L), (want.rgb[:n], want.counts[:n]))


@pytest.mark.parametrize("form", ["host", "device"])
def test_across_the_chunk_seam(gpu, form):
    """1 024 lights: chunks of 2^22 / 1024 = 4 096 points; 4 096 + 65 points, and the restatement at the points on both sides of the seam and at both ends."""
    c = case("tiny")
    sc = c["scene"]
    n = 4096 + 65
    reps = -(-n // 320)
    p = np.ascontiguousarray(np.tile(c["points"], (reps, 1))[:n])
    nm = np.ascontiguousarray(np.tile(c["normals"], (reps, 1))[:n])
    L = case_lights("tiny", 1024)
    got = tuple(nr.light_points(sc, p, nm, L)) if form == "host" else device_light(sc, p, nm, L)
    assert got[0].shape == (n, 3) and got[1].shape == (n, 2)
    near = np.concatenate([np.arange(0, 8), np.arange(4096 - 24, 4096 + 24), np.arange(n - 8, n)])
    want = nr.light_points_ref(sc, p[near], nm[near], L)
    assert same((got[0][near], got[1][near]), want)
    assert 0 < want.counts[:, 1].sum() < want.counts[:, 0].sum() < len(near) * 1024
    assert same((got[0][320:640], got[1][320:640]), (got[0][:320], got[1][:320]))  # the same points, another place in the chunk
    assert same((got[0][4096:4161], got[1][4096:4161]), (got[0][256:321], got[1][256:321]))  # ... and in the second chunk (4096 = 12 * 320 + 256)


# ---- 6: options ---------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["host", "device"])
@pytest.mark.parametrize("m", [4, 16, 70])
def test_skipped_points_are_zero_and_leave_their_neighbours_alone(gpu, form, m):
    """m = 4: a lane per point; 16: eight lanes; 70: sixty-four."""
    c = case("mixed")
    sc = c["scene"]
    L = case_lights("mixed", m, seed=3)
    if form == "host":
        run = lambda p, nm, hf: tuple(nr.light_points(sc, p, nm, L, hit_flags=hf))  # noqa: E731
    else:
        run = lambda p, nm, hf: device_light(sc, p, nm, L, hit_flags=hf)  # noqa: E731
    n = 130
    p, nm = c["points"][:n].copy(), c["normals"][:n].copy()
    base = run(p, nm, None)
    assert base[1][:, 1].sum() > 0
    lanes = [0, 31, 63, 64, 129]
    keep = np.setdiff1d(np.arange(n), lanes)
    assert same(run(p[keep], nm[keep], np.full(len(keep), 3, np.uint32)), (base[0][keep], base[1][keep]))
    hf = np.full(n, 1, np.uint32)
    hf[lanes] = [0, 2, 0xfffffffe, 0, 2]  # bit 0 clear, whatever else is set
    p[lanes], nm[lanes] = np.nan, np.nan
    p[lanes[1]] = np.inf
    f, k = run(p, nm, hf)
    assert (bits(f[lanes]) == 0).all() and (k[lanes] == 0).all()
    assert same((f[keep], k[keep]), (base[0][keep], base[1][keep]))
    f, k = run(p, nm, np.zeros(n, np.uint32))  # every point skipped
    assert (bits(f) == 0).all() and (k == 0).all()


GUARD = 64  # floats / words of 7 on either side of an output


def _raw_call(sc, form, n, arrays, lights, call_flags=0, null=(), scene=True, **kw):
    """One library call with host or device pointers on guarded outputs; `kw` replaces fields of the struct (positions=None / colors=None: a NULL table).  Returns
    (status, out_rgb with its guards, out_counts with its guards)."""
    import torch
    lib = abi.load_hip_lib()
    order = ("points", "normals", "hit_flags", "lights", "out_rgb", "out_counts")
    h = sc.device_handle() if scene else None
    tables = dict(positions=np.ascontiguousarray(lights.positions, np.float64), colors=np.ascontiguousarray(lights.colors, np.float32),
                  normals=None if lights.normals is None else np.ascontiguousarray(lights.normals, np.float64))
    if form == "device":
        held = {k: torch.from_numpy(v.view(np.int32) if v.dtype == np.uint32 else v).cuda() for k, v in arrays.items()}
        dev_tables = {k: None if v is None else torch.from_numpy(v).cuda() for k, v in tables.items()}
        adr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        inner = {"out_rgb": lambda t: t.data_ptr() + 4 * GUARD, "out_counts": lambda t: t.data_ptr() + 4 * GUARD}
        ptrs = {k: inner.get(k, adr)(t) for k, t in held.items()}
        tab = {k: adr(t) for k, t in dev_tables.items()}
    else:
        ct = {np.dtype(np.float64): C.c_double, np.dtype(np.uint32): C.c_uint32, np.dtype(np.float32): C.c_float}
        ptrs = {k: C.cast(v.ctypes.data + (4 * GUARD if k.startswith("out_") else 0), C.POINTER(ct[v.dtype])) for k, v in arrays.items()}
        tab = {k: None if v is None else v.ctypes.data for k, v in tables.items()}
    f = dict(num_lights=len(tables["positions"]), flags=abi.LIGHTS_INVERSE_SQUARE if lights.inverse_square else 0, bias=lights.bias, offset=lights.offset, min_dist=lights.min_dist)
    f.update(kw)
    for k in ("positions", "colors"):
        if k in kw:
            tab[k] = None
    st = abi.NraysPointLights(f["num_lights"], f["flags"], tab["positions"], tab["colors"], tab["normals"], f["bias"], f["offset"], f["min_dist"])
    ptrs["lights"] = C.byref(st)
    args = [None if k in null else ptrs[k] for k in order]
    if form == "device":
        rc = lib.nrays_light_points_device(h, n, *args, call_flags, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc, held["out_rgb"].cpu().numpy(), held["out_counts"].cpu().numpy().view(np.uint32)
    return lib.nrays_light_points(h, n, *args, call_flags), arrays["out_rgb"], arrays["out_counts"]


def _raw_setup(n=16, m=9):
    c = case("analytic")
    arrays = dict(points=c["points"][:n].copy(), normals=c["normals"][:n].copy(), hit_flags=np.ones(n, np.uint32),
                  out_rgb=np.full(3 * n + 2 * GUARD, 7.0, np.float32), out_counts=np.full(2 * n + 2 * GUARD, 7, np.uint32))
    L, want = reference("analytic", m)
    return c, arrays, L, (want.rgb[:n], want.counts[:n])


@pytest.mark.parametrize("form", ["host", "device"])
def test_out_counts_may_be_null_and_nothing_is_stored_beside_the_outputs(gpu, form):
    c, arrays, L, want = _raw_setup()
    n = 16
    rc, f, k = _raw_call(c["scene"], form, n, arrays, L, null=("out_counts",))
    assert rc == abi.OK and np.array_equal(bits(f[GUARD:-GUARD].reshape(n, 3)), bits(want[0])) and (k == 7).all()  # nothing was stored there
    assert (f[:GUARD] == 7.0).all() and (f[-GUARD:] == 7.0).all()
    rc, f, k = _raw_call(c["scene"], form, n, arrays, L)
    assert rc == abi.OK and same((f[GUARD:-GUARD].reshape(n, 3), k[GUARD:-GUARD].reshape(n, 2)), want)
    assert (f[:GUARD] == 7.0).all() and (f[-GUARD:] == 7.0).all() and (k[:GUARD] == 7).all() and (k[-GUARD:] == 7).all()
    rc, f, k = _raw_call(c["scene"], form, n, arrays, L, null=("hit_flags",))
    assert rc == abi.OK and same((f[GUARD:-GUARD].reshape(n, 3), k[GUARD:-GUARD].reshape(n, 2)), want)
    got = nr.light_points(c["scene"], arrays["points"], arrays["normals"], L, want_counts=False)
    assert got.counts is None and np.array_equal(bits(got.rgb), bits(want[0]))


@pytest.mark.parametrize("form", ["host", "device"])
def test_statuses(gpu, form):
    c, arrays, L, want = _raw_setup()
    sc = c["scene"]
    call = lambda **kw: _raw_call(sc, form, kw.pop("n", 16), arrays, L, **kw)  # noqa: E731
    for flags in (1, 2, 1 << 31, 3):
        assert call(call_flags=flags)[0] == abi.ERR_BAD_ARG, flags
    for name in ("points", "normals", "lights", "out_rgb"):
        assert call(null=(name,))[0] == abi.ERR_BAD_ARG, name
    assert call(scene=False)[0] == abi.ERR_BAD_ARG
    for bad in BAD_LIGHTS:
        assert call(**bad)[0] == abi.ERR_BAD_ARG, bad
        assert call(n=0, **bad)[0] == abi.ERR_BAD_ARG, bad
    rc, f, k = call(n=0)
    assert rc == abi.OK and (f == 7.0).all() and (k == 7).all()  # without work; nothing so far wrote the outputs
    assert call(n=0, call_flags=1)[0] == abi.ERR_BAD_ARG
    assert L.inverse_square and call(min_dist=math.nan)[0] == abi.ERR_BAD_ARG and call(flags=0, min_dist=math.nan)[0] == abi.OK  # min_dist is unread without the falloff
    # the probe's checks
    lib = abi.load_hip_lib()
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    p, nm = arrays["points"], arrays["normals"]
    pos, col = np.ascontiguousarray(L.positions), np.ascontiguousarray(L.colors, np.float32)
    ro, rd, tm, w = np.full((16, 9, 3), 7.0), np.full((16, 9, 3), 7.0), np.full((16, 9), 7.0), np.full((16, 9), 7.0, np.float32)
    st = lights_struct(pos, col, num_lights=9)
    good = [sc.device_handle(), 16, p.ctypes.data_as(dp), nm.ctypes.data_as(dp), C.byref(st), ro.ctypes.data_as(dp), rd.ctypes.data_as(dp), tm.ctypes.data_as(dp), w.ctypes.data_as(fp)]
    for i in (0, 2, 3, 4, 5, 6, 7, 8):
        assert lib.nrays_debug_light_rays(*[None if j == i else a for j, a in enumerate(good)]) == abi.ERR_BAD_ARG, i
    for bad in BAD_LIGHTS:
        bst = lights_struct(pos, col, **dict(dict(num_lights=9), **bad))
        assert lib.nrays_debug_light_rays(*[C.byref(bst) if j == 4 else a for j, a in enumerate(good)]) == abi.ERR_BAD_ARG, bad
    assert lib.nrays_debug_light_rays(*[0 if j == 1 else a for j, a in enumerate(good)]) == abi.OK and (ro == 7.0).all()
    assert lib.nrays_debug_light_rays(*good) == abi.OK
    mirror = nr.light_rays(p, nm, nr.PointLights(pos, col, None, False, 1.0, 1e-3, 1e-3))
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(mirror, (ro, rd, tm, w)))


@pytest.mark.parametrize("name", ["quads", "tiny"])
def test_light_hits_on_tensors_on_a_stream_equals_the_numpy_form(gpu, name):
    import torch
    c = case(name)
    sc, o, d = c["scene"], c["o"], c["d"]
    L = case_lights(name, 20, seed=5)
    want = nr.light_hits(sc, o, d, c["hits"], L)
    hit = (c["hits"].flags & 1) != 0
    assert hit.sum() > 300 and (name != "tiny" or (~hit).sum() > 50)  # (the tiny scene's camera sees the sky)
    assert (bits(want.rgb[~hit]) == 0).all() and (want.counts[~hit] == 0).all() and want.counts[hit, 1].sum() > 0
    p, nm = hit_points(o, d, c["hits"])
    assert same(nr.light_points(sc, p, nm, L, hit_flags=c["hits"].flags), want)
    assert same(sc.light_points(p, nm, L, hit_flags=c["hits"].flags), want)  # Scene.light_points
    to, td = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        got = nr.light_hits(sc, to, td, nr.closest_hits(sc, to, td), L)
    s.synchronize()
    assert same((got.rgb.cpu().numpy(), got.counts.cpu().numpy().view(np.uint32)), want)
    with pytest.raises(ValueError):
        nr.light_hits(sc, to, td, c["hits"], L)  # tensors and arrays mixed


def test_vpls_light_the_points_through_the_chain_of_the_docstring(gpu):
    """closest_hits -> material_hits -> vpls_from_hits -> light_points, against the restatement: emitter normals and falloff from real hits.  The paths come from the
    side, under the mixed scene's occluder quad, and land on the floor, the ball and the capsule; what they leave there lights the points the camera sees."""
    c = case("mixed")
    sc = c["scene"]
    rng = np.random.default_rng(6)
    o = np.tile((0.3, 0.7, -5.0), (400, 1))
    t = rng.uniform((-2.0, 0.0, -2.0), (2.0, 0.9, 2.0), size=(400, 3)) - o
    d = t / np.sqrt((t * t).sum(axis=1))[:, None]
    hits = nr.closest_hits(sc, o, d)
    diffuse = nr.material_hits(sc, hits, want=("diffuse",)).diffuse
    vpls = nr.vpls_from_hits(o, d, hits, diffuse, 0.05, inverse_square=True, min_dist=0.1)
    assert 100 < len(vpls.positions) < 400 and vpls.normals.shape == vpls.positions.shape and len(np.unique(hits.node[(hits.flags & 1) != 0])) >= 3
    got = nr.light_points(sc, c["points"], c["normals"], vpls)
    assert same(got, nr.light_points_ref(sc, c["points"], c["normals"], vpls))
    assert (got.rgb > 0).any(axis=1).mean() > 0.25 and 0 < got.counts[:, 1].sum() < got.counts[:, 0].sum() < 0.6 * 320 * len(vpls.positions)


@pytest.mark.parametrize("name", ["analytic", "quads"])
def test_a_batch_leaves_the_render_state_alone(gpu, name):
    import torch
    from tests.test_occlusion import quad_scene
    c = case(name)
    sc, cam = {"analytic": rich_analytic_scene, "quads": quad_scene}[name]()
    L, want = reference(name, 9)
    w, h = 128, 72
    proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], w, h)
    first = nr.render(sc, (w, h), 1, 0.0, cam["eye"], proj)
    st1, perm1 = nr.get_stats(sc), nr.last_permutation(sc)
    got = device_light(sc, c["points"], c["normals"], L, stream=torch.cuda.Stream())
    assert same(got, want)  # (a fresh handle of the same scene, after a render, on another stream)
    assert nr.last_permutation(sc) == perm1
    second = nr.render(sc, (w, h), 1, 0.0, cam["eye"], proj)
    st2 = nr.get_stats(sc)
    assert np.array_equal(first.view(np.uint32), second.view(np.uint32))
    assert nr.last_permutation(sc) == perm1
    for fld in STAT_FIELDS:
        assert getattr(st1, fld) == getattr(st2, fld), fld


# ---- 7: one physical picture ----------------------------------------------------------------------------------------------------------------------------------
def test_one_physical_picture(gpu):
    """A floor at y = 0, an opaque disc (a flat cylinder) at height 1 over the origin, a half-transparent quad at height 1 beside it, one light straight above."""
    grey = su.default_material()
    idx = np.asarray([[0, 2, 1], [0, 3, 2]], dtype=np.uint32)
    floor = su.f32_exact([[-6.0, 0.0, -6.0], [6.0, 0.0, -6.0], [6.0, 0.0, 6.0], [-6.0, 0.0, 6.0]])
    pane = su.f32_exact([[2.0, 1.0, -1.0], [4.0, 1.0, -1.0], [4.0, 1.0, 1.0], [2.0, 1.0, 1.0]])
    nodes = [nr.SceneNode(grey, 0.0, 0.0, 1.0, 1.0, nr.Isometry3(), nr.TriMesh(floor, idx, None)),
             nr.SceneNode(grey, 0.0, 0.0, 1.0, 1.0, nr.Isometry3((0.0, 1.0, 0.0)), nr.Cylinder(0.05, 1.0)),
             nr.SceneNode(grey, 0.0, 0.0, 0.5, 1.0, nr.Isometry3(), nr.TriMesh(pane, idx, None))]
    sc = nr.Scene(nodes, [nr.Light((0.0, 8.0, 0.0), 0.0, 1, (1.0, 1.0, 1.0))])  # (the scene's own light is not read)
    col = np.asarray([0.9, 1.7, 0.3], np.float32)
    L = nr.PointLights([(0.0, 8.0, 0.0)], [col], None, True, 0.1, 1e-3, 1e-3)
    rng = np.random.default_rng(21)
    r, a = rng.uniform(0.0, 0.6, 40), rng.uniform(0.0, 2.0 * math.pi, 40)
    under_disc = np.stack([r * np.cos(a), np.zeros(40), r * np.sin(a)], axis=1)
    under_pane = np.stack([rng.uniform(2.6, 3.0, 40), np.zeros(40), rng.uniform(-0.5, 0.5, 40)], axis=1)  # (the light is at x = 0: the shadow moves outwards by 1/7)
    in_the_open = np.stack([rng.uniform(-5.0, -2.0, 40), np.zeros(40), rng.uniform(-5.0, 5.0, 40)], axis=1)
    p = np.concatenate([under_disc, under_pane, in_the_open, in_the_open])
    nm = np.tile([0.0, 1.0, 0.0], (160, 1))
    nm[120:] = (0.0, -1.0, 0.0)  # the floor's underside: lit from behind
    got = nr.light_points(sc, p, nm, L)
    ro, rd, t_max, w = nr.light_rays(p, nm, L)
    lit, filt = nr.intersects_rays(sc, np.ascontiguousarray(ro[:120, 0]), np.ascontiguousarray(rd[:120, 0]), np.ascontiguousarray(t_max[:120, 0]))
    assert not lit[:40].any() and lit[40:].all() and (filt[40:80] < 1.0).all() and (filt[40:80] > 0.0).all() and (filt[80:120] == 1.0).all()
    assert (bits(got.rgb[:40]) == 0).all() and (got.counts[:40] == (1, 0)).all()
    assert np.array_equal(bits(got.rgb[40:80]), bits(col[None, :] * (filt[40:80] * w[40:80, 0, None]))) and (got.counts[40:80] == (1, 1)).all()
    assert np.array_equal(bits(got.rgb[80:120]), bits(col[None, :] * w[80:120, 0, None])) and (got.counts[80:120] == (1, 1)).all()
    assert (bits(got.rgb[120:]) == 0).all() and (got.counts[120:] == (0, 0)).all() and (w[120:] == 0).all()
    # the closed form in the open: col * h / d^3 with h and d from the biased point, within the CPU test's 8 * 2^-24
    q = p[80:120] + nm[80:120] * 1e-3
    dist = np.sqrt(((np.asarray(L.positions) - q) ** 2).sum(axis=1))
    want = col[None, :].astype(np.float64) * ((8.0 - 1e-3) / dist ** 3)[:, None]
    assert float((np.abs(got.rgb[80:120] - want) / want).max()) <= 8 * F32_EPS
    assert same(got, fold_reference(sc, p, nm, L))


def fold_reference(sc, p, nm, L):
    """light_points_ref, spelled with tests/test_light_points.py's fold: the restatement's own parts once more."""
    ro, rd, t_max, w = nr.light_rays(p, nm, L)
    ray = w > 0
    open_, filt = ray.copy(), np.ones(w.shape + (3,), np.float32)
    lit, f = nr.intersects_rays(sc, np.ascontiguousarray(ro[ray]), np.ascontiguousarray(rd[ray]), np.ascontiguousarray(t_max[ray]))
    open_[ray], filt[ray] = lit, f
    return fold(np.asarray(L.colors, np.float32), w, filt, open_), np.stack([ray.sum(axis=1), open_.sum(axis=1)], axis=1).astype(np.uint32)
