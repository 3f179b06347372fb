"""Reordering of caller-ray batches that come in no useful order, on the GPU (NRAYS_RAYS_UNORDERED; nrays_amd/csrc/ray_order.hip): the hinted
calls give the unhinted calls' results BIT FOR BIT on every kernel of the batch path, the probe's frame and keys equal the host compiler's,
its order is a permutation sorted by the leading key bits and fine enough by the derived yardstick of tests/test_ray_order.py.
Every handle is created under NRAYS_RAY_REORDER=2 (reorder whatever the size) unless a test says otherwise."""
import ctypes as C

import numpy as np
import pytest

import nrays_amd as nr
from nrays_amd import abi, math3d
from tests.test_ray_order import GRID_H, GRID_W, KeyShim, ao_batch, camera_batch, tiles_per_wave
from tests.test_trace_rays import analytic_scene, build_shim, shim_trace
from tests.test_trace_rays_gpu import CAMERA_CASES, STAT_FIELDS, TOL, _arbitrary_rays, _glass_scene, _small_rays
from tools import scenes_util as su
from tools import standins

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def reorder_always(monkeypatch):
    monkeypatch.setenv("NRAYS_RAY_REORDER", "2")  # read when a handle is created


@pytest.fixture(scope="module")
def keyshim(tmp_path_factory):
    return KeyShim(tmp_path_factory.mktemp("ray_key_shim_gpu"))


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(tmp_path_factory.mktemp("trace_shim_order_gpu"))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _orders(o, d, k, seed):
    """The batch in image order, shuffled, and all equal to one ray."""
    perm = np.random.default_rng(seed).permutation(len(o))
    one = len(o) // 3
    return {"image": (o, d, k), "shuffled": (o[perm], d[perm], k[perm]),
            "one_ray": (np.tile(o[one], (len(o), 1)), np.tile(d[one], (len(o), 1)), k)}


@pytest.mark.parametrize("case", sorted(CAMERA_CASES))
def test_hinted_equals_unhinted_bit_for_bit(gpu, case):
    make, w, h, spp, window = CAMERA_CASES[case]
    sc, cam = make()
    proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], w, h)
    o, d, k = nr.camera_rays((w, h), cam["eye"], proj, ray_per_pixel=spp, window_width=window, seed=3)
    assert nr.ray_order(sc, o, d)[3][2]  # this handle reorders a hinted batch of this size
    rng = np.random.default_rng(21)
    refr, energy = rng.uniform(1.0, 1.4, len(o)), rng.uniform(0.2, 1.0, len(o)).astype(np.float32)
    for name, (oo, dd, kk) in _orders(o, d, k, 5).items():
        plain = nr.trace_rays(sc, oo, dd, keys=kk)
        assert np.array_equal(bits(nr.trace_rays(sc, oo, dd, keys=kk, unordered=True)), bits(plain)), name
        assert np.array_equal(bits(nr.trace_rays(sc, oo, dd, unordered=True)), bits(nr.trace_rays(sc, oo, dd))), name
        assert np.array_equal(bits(nr.trace_rays(sc, oo, dd, refr=refr, energy=energy, keys=kk, max_depth=2, unordered=True)),
                              bits(nr.trace_rays(sc, oo, dd, refr=refr, energy=energy, keys=kk, max_depth=2))), name
        if name == "image":
            assert np.abs(plain - plain[0]).max() > 0.05  # (the batch really sees the scene)
        toi = rng.uniform(0.5, 30.0, len(oo))
        lit0, f0 = nr.intersects_rays(sc, oo, dd, toi)
        lit1, f1 = nr.intersects_rays(sc, oo, dd, toi, unordered=True)
        assert np.array_equal(lit0, lit1) and np.array_equal(bits(f0), bits(f1)), name


def test_non_finite_rays_mixed_in(gpu):
    sc, cam = su.balls_scene()
    w, h = 96, 64
    proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], w, h)
    o, d, k = nr.camera_rays((w, h), cam["eye"], proj)
    o, d = o.copy(), d.copy()
    rng = np.random.default_rng(8)
    special = np.asarray([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e308])
    rows = rng.choice(len(o), 600, replace=False)
    o[rows[:200]] = rng.choice(special, (200, 3))
    d[rows[200:400]] = rng.choice(special, (200, 3))
    o[rows[400:]] = rng.choice(special, (200, 3)); d[rows[400:]] = rng.choice(special, (200, 3))
    perm = rng.permutation(len(o))
    o, d, k = o[perm], d[perm], k[perm]
    assert np.array_equal(bits(nr.trace_rays(sc, o, d, keys=k, unordered=True)), bits(nr.trace_rays(sc, o, d, keys=k)))
    toi = np.full(len(o), 20.0)
    lit0, f0 = nr.intersects_rays(sc, o, d, toi)
    lit1, f1 = nr.intersects_rays(sc, o, d, toi, unordered=True)
    assert np.array_equal(lit0, lit1) and np.array_equal(bits(f0), bits(f1))
    keys, order, frame, _ = nr.ray_order(sc, o, d)
    assert np.array_equal(np.sort(order), np.arange(len(o))) and np.all(np.isfinite(frame[:14]))


def test_non_finite_scene_hinted(gpu):
    """The <true, kFeatAll> kernel: a scene with a non-finite light."""
    from tests.test_elision_gpu import _nonfinite_scene
    sc, cam = _nonfinite_scene("light")
    w, h = 104, 60
    proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], w, h)
    o, d, k = nr.camera_rays((w, h), cam["eye"], proj)
    perm = np.random.default_rng(9).permutation(len(o))
    o, d, k = o[perm], d[perm], k[perm]
    plain = nr.trace_rays(sc, o, d, keys=k)
    assert (~np.isfinite(plain)).any()
    assert np.array_equal(bits(nr.trace_rays(sc, o, d, keys=k, unordered=True)), bits(plain))


@pytest.mark.parametrize("max_depth", [0, 1, 3])
def test_arbitrary_rays_against_the_oracle_hinted(gpu, shim, max_depth):
    sc, _ = analytic_scene(background=(0.25, 0.5, 0.75))
    o, d, r, e, k, _ = _arbitrary_rays(np.random.default_rng(11 + max_depth), 4096)
    got = nr.trace_rays(sc, o, d, refr=r, energy=e, keys=k, max_depth=max_depth, unordered=True)
    ref = shim_trace(shim, sc, o, d, refr=r, energy=e, keys=k, max_depth=max_depth)
    assert float(np.abs(got - ref).max()) <= TOL


@pytest.mark.parametrize("n", [1, 63, 64, 65, (1 << 22) + 17])
def test_sizes_streams_and_inputs(gpu, n):
    """Hinted equals unhinted for every size (two chunks at 2^22 + 17); the device path on a non-default stream with torch tensors equals the
    host path; the input tensors are unchanged after the call."""
    import torch
    sc, _ = _glass_scene()
    sc = nr.Scene(sc._nodes, [nr.Light((2.0, 6.0, -4.0), 0.3, 2, (1, 1, 1))])  # area light: the keys matter
    o, d = _small_rays(n)
    plain = nr.trace_rays(sc, o, d)
    host = nr.trace_rays(sc, o, d, unordered=True)
    assert np.array_equal(bits(host), bits(plain))
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        to, td = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
        keep_o, keep_d = to.clone(), td.clone()
        dev = nr.trace_rays(sc, to, td, unordered=True)
        toi = torch.full((n,), 5.0, dtype=torch.float64, device="cuda")
        lit1, f1 = nr.intersects_rays(sc, to, td, toi, unordered=True)
        lit0, f0 = nr.intersects_rays(sc, to, td, toi)
        same_inputs = bool(torch.equal(to, keep_o)) and bool(torch.equal(td, keep_d))
        dev, lit0, lit1, f0, f1 = dev.cpu().numpy(), lit0.cpu().numpy(), lit1.cpu().numpy(), f0.cpu().numpy(), f1.cpu().numpy()
    s.synchronize()
    assert same_inputs
    assert np.array_equal(bits(dev), bits(host))
    assert np.array_equal(lit0, lit1) and np.array_equal(bits(f0), bits(f1))


def _floor_scene():
    """A slab whose top face is the plane y = 0 under the AO batch of tests/test_ray_order.py, and a few balls on it."""
    iso, mat = nr.Isometry3, su.default_material()
    nodes = [nr.SceneNode(mat, 0.0, 0.0, 1.0, 1.0, iso((0.0, -0.5, 0.0)), nr.Cuboid((10.0, 0.5, 6.0)))]
    nodes += [nr.SceneNode(mat, 0.0, 0.0, 1.0, 1.0, iso((x, 0.7, z)), nr.Ball(0.7)) for x, z in ((-5.0, -2.0), (0.0, 1.0), (4.0, -1.0), (6.5, 3.0))]
    return nr.Scene(nodes, [nr.Light((2.0, 9.0, -4.0), 0.0, 1, (1, 1, 1))])


@pytest.mark.parametrize("batch,bound", [("camera", 8.0), ("ao", 16.0)])
def test_probe_against_the_host_key_and_the_yardstick(gpu, keyshim, batch, bound):
    if batch == "camera":
        (sc, _), (o, d) = su.balls_scene(), camera_batch()
    else:
        sc, (o, d) = _floor_scene(), ao_batch()
    perm = np.random.default_rng(17).permutation(len(o))
    so, sd = o[perm], d[perm]
    keys, order, frame, (K, B, reordered) = nr.ray_order(sc, so, sd)
    assert (K, B) == (keyshim.K, keyshim.B) and reordered
    assert np.array_equal(np.sort(order), np.arange(len(o), dtype=np.uint32))  # a permutation
    box = frame[14:20]
    assert np.all(np.isfinite(box)) and np.all(box[:3] <= box[3:])
    want = keyshim.frame(so, sd, box=box)
    assert np.array_equal(frame.view(np.uint64), want.view(np.uint64))           # the device's frame, bit for bit
    assert np.array_equal(keys, keyshim.keys(so, sd, frame))                     # ... and its keys
    lead = (keys >> np.uint64(K - B))[order]
    assert np.all(lead[1:] >= lead[:-1])                                         # sorted by the leading B bits
    score = tiles_per_wave(perm[order])
    print("%s batch, shuffled, in the device's order: %.2f tiles per wave (bound %.1f)" % (batch, score, bound))
    assert score <= bound
    # the hinted trace of the same arrays (2 M rays in one chunk): bit-identical
    assert np.array_equal(bits(nr.trace_rays(sc, so, sd, unordered=True)), bits(nr.trace_rays(sc, so, sd)))


def test_probe_small_and_degenerate(gpu, keyshim):
    sc, _ = su.balls_scene()
    for n in (1, 63, 64, 65, 1000):
        o, d = _small_rays(n)
        keys, order, frame, _ = nr.ray_order(sc, o, d)
        assert np.array_equal(np.sort(order), np.arange(n))
        assert np.array_equal(keys, keyshim.keys(o, d, frame))
        assert np.array_equal(frame.view(np.uint64), keyshim.frame(o, d, box=frame[14:20]).view(np.uint64))
    o, d = _small_rays(1)
    o, d = np.tile(o, (5000, 1)), np.tile(d, (5000, 1))  # every ray in one bin
    keys, order, frame, _ = nr.ray_order(sc, o, d)
    assert np.array_equal(np.sort(order), np.arange(5000)) and len(np.unique(keys)) == 1


@pytest.mark.parametrize("make", [_glass_scene, lambda: standins.sponza_scene()], ids=["double_branching", "sponza_standin"])
def test_a_hinted_batch_leaves_the_render_state_alone(gpu, make):
    sc, cam = make()
    w, h = 128, 72
    proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], w, h)
    first = nr.render(sc, (w, h), 1, 0.0, cam["eye"], proj)
    st1 = nr.get_stats(sc)
    o, d = _small_rays(20000)
    nr.trace_rays(sc, o, d, max_depth=2, unordered=True)
    nr.intersects_rays(sc, o, d, np.full(len(o), 5.0), unordered=True)
    nr.ray_order(sc, o, d)
    second = nr.render(sc, (w, h), 1, 0.0, cam["eye"], proj)
    st2 = nr.get_stats(sc)
    assert np.array_equal(first, second)
    for f in STAT_FIELDS:
        assert getattr(st1, f) == getattr(st2, f), f


def _would_reorder(sc, n):
    info = (C.c_uint32 * 4)()
    o = np.zeros((max(n, 1), 3))
    d = np.tile(np.asarray([0.0, 0.0, 1.0]), (max(n, 1), 1))
    keys, order, frame = np.zeros(max(n, 1), np.uint64), np.zeros(max(n, 1), np.uint32), np.zeros(abi.RAY_FRAME_DOUBLES)
    dp = C.POINTER(C.c_double)
    abi.check(abi.load_hip_lib().nrays_debug_ray_order(sc.device_handle(), n, o.ctypes.data_as(dp), d.ctypes.data_as(dp), keys.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                       order.ctypes.data_as(C.POINTER(C.c_uint32)), frame.ctypes.data_as(dp), info))
    return int(info[2])


def test_the_switch_and_the_threshold(gpu, monkeypatch):
    monkeypatch.setenv("NRAYS_RAY_REORDER", "0")
    sc, _ = su.balls_scene()
    assert [_would_reorder(sc, n) for n in (0, 1, 64, 1 << 21, 1 << 22)] == [0, 0, 0, 0, 0]
    o, d = _small_rays(3000)
    assert np.array_equal(bits(nr.trace_rays(sc, o, d, unordered=True)), bits(nr.trace_rays(sc, o, d)))
    monkeypatch.delenv("NRAYS_RAY_REORDER")
    sc, _ = su.balls_scene()
    assert _would_reorder(sc, 64) == 0 and _would_reorder(sc, 1 << 21) == 1
    monkeypatch.setenv("NRAYS_RAY_REORDER", "2")
    sc, _ = su.balls_scene()
    assert _would_reorder(sc, 64) == 1 and _would_reorder(sc, 1) == 1


def test_flags_zero_is_the_plain_entry_point(gpu):
    import torch
    sc, _ = _glass_scene()
    o, d = _small_rays(5000)
    to, td = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    lib, h = abi.load_hip_lib(), sc.device_handle()
    out0, out1 = torch.zeros((5000, 3), dtype=torch.float32, device="cuda"), torch.zeros((5000, 3), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    abi.check(lib.nrays_trace_rays_device(h, 5000, to.data_ptr(), td.data_ptr(), None, None, None, 0, out0.data_ptr(), stream))
    abi.check(lib.nrays_trace_rays_device_ex(h, 5000, to.data_ptr(), td.data_ptr(), None, None, None, 0, out1.data_ptr(), 0, stream))
    torch.cuda.synchronize()
    assert np.array_equal(bits(out0.cpu().numpy()), bits(out1.cpu().numpy()))
    assert lib.nrays_trace_rays_device_ex(h, 5000, to.data_ptr(), td.data_ptr(), None, None, None, 0, out1.data_ptr(), 2, stream) == abi.ERR_BAD_ARG
