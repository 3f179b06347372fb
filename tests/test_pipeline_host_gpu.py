"""What sits above the three enqueues of a pipelined frame (NRAYS_PIPELINE_HOST, read once per scene handle; 0 = the path as it was), one bit per part:
  1  spread stamps   the rows of a timed k_compose leave their exit ticks in several words of the frame's stamp block, nrays_get_stats takes the latest;
  2  time proof      a call that comes right behind the return of the handle's last pipelined call is pipelined without an in-flight query;
  4  burst start     the first pipelined frame behind ONE plain direct frame orders only the internal stream that shares that frame's counter sets.
Pixels are compared bit for bit with the direct path (NRAYS_PIPELINE=0); cameras drift by 2e-5 of the viewing distance per frame, so a frame that lands in the
wrong slot or order shows; nrays_debug_pipeline_counts tells how the frames were enqueued.  Small frames: a few seconds in all."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import nrays_amd as nr
from nrays_amd import abi
from tools import scenes_util as su

pytestmark = pytest.mark.gpu

FRAMES = 40
HOST = ["0", "1", "2", "4", None]  # nothing, each part alone, the library's default
HOST_IDS = ["host0", "stamps", "time_proof", "burst_start", "default"]
CASES = [("balls", (160, 96)), ("balls", (173, 111)), ("spheres", (128, 96))]  # 173 x 111 is not whole in wave tiles; the spheres walk the TLAS with the LDS / HBM stack
CASE_IDS = ["%s_%dx%d" % ((c[0],) + c[1]) for c in CASES]
KRING = 256  # scene_handle.h: NraysScene::kRing


def _spheres():
    """300 reflecting balls."""
    rng = np.random.RandomState(7)
    mats = [nr.NormalMaterial(), su.default_material()]
    nodes = [nr.SceneNode(mats[k & 1], 0.3, 0.25, 1.0, 1.0, nr.Isometry3(tuple(float(x) for x in rng.uniform(-3.0, 3.0, 3))), nr.Ball(float(rng.uniform(0.15, 0.45))))
             for k in range(300)]
    return nr.Scene(nodes, [nr.Light((4.0, 12.0, -9.0), 0.0, 1, (1, 1, 1))], (0.2, 0.3, 0.4)), dict(eye=(2.0, 6.0, -30.0), at=(0.0, 0.0, 0.0), fovy=45.0)


SCENES = {"balls": lambda: su.balls_scene(tex_size=(256, 128)), "spheres": _spheres}


class _env:
    """A scene handle reads its switches when it is created.  A value of None leaves the variable unset."""
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _fresh(make, pipeline, host=None, stride=None, lean=None):
    with _env(NRAYS_PIPELINE=pipeline, NRAYS_PIPELINE_HOST=host, NRAYS_EVENT_STRIDE=stride, NRAYS_PIPELINE_LEAN=lean, NRAYS_STAMP_WORDS=None):
        sc, cam = make()
        sc.device_handle()
    return sc, cam


def _drift(cam, n, step=2e-5):
    eye0 = np.array(cam["eye"], dtype=np.float64); at = np.array(cam["at"], dtype=np.float64)
    d = step * np.linalg.norm(eye0 - at) * np.array([1.0, 0.3, 0.0])
    return [dict(cam, eye=tuple(eye0 + k * d)) for k in range(n)]


def _enqueue(lib, sc, p, out):
    abi.check(lib.nrays_render_device(sc.device_handle(), C.byref(p), C.c_void_p(out.data_ptr()), None))


def _settle(lib, sc, p, w, h):
    import torch
    o = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    for _ in range(4):
        _enqueue(lib, sc, p, o)
    torch.cuda.synchronize()
    nr.get_stats(sc)  # drains the timing ring: the averages that follow are over the frames that follow


def _counts(lib, sc):
    """(frames pipelined, frames direct, in-flight queries, slot waits) since the handle was created."""
    c = (C.c_uint64 * 4)()
    abi.check(lib.nrays_debug_pipeline_counts(sc.device_handle(), c))
    return np.array(list(c), dtype=np.int64)


def _same(a, b, what):
    diff = a.view(np.uint32) != b.view(np.uint32)
    assert not diff.any(), "%s: %d pixel components differ" % (what, int(diff.sum()))


_direct = {}


def _direct_frames(lib, scene, w, h):
    """The FRAMES drifting frames of a scene on the direct path: rendered once, shared, never changed."""
    import torch
    if (scene, w, h) not in _direct:
        sc, cam = _fresh(SCENES[scene], "0")
        params = [su.camera_params(c, w, h)[0] for c in _drift(cam, FRAMES)]
        _settle(lib, sc, params[0], w, h)
        outs = [torch.full((h, w, 3), -1.0, dtype=torch.float32, device="cuda") for _ in params]
        for p, o in zip(params, outs):
            _enqueue(lib, sc, p, o)
        torch.cuda.synchronize()
        frames = [o.cpu().numpy() for o in outs]
        for f in frames:
            f.setflags(write=False)
        c = _counts(lib, sc)
        assert c[0] == 0 and c[1] == 4 + FRAMES and c[2] == 0 and c[3] == 0, c  # (NRAYS_PIPELINE=0: nothing is pipelined, nothing is asked)
        _direct[(scene, w, h)] = frames
        sc._release()
    return _direct[(scene, w, h)]


@pytest.mark.parametrize("pipeline", ["1", "2"], ids=["in_flight", "always"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("host", HOST, ids=HOST_IDS)
def test_frames_back_to_back_equal_the_direct_path(gpu, host, case, pipeline):
    """40 drifting frames enqueued back to back, each into its own buffer: frame k is the direct path's frame k, bit for bit."""
    import torch
    lib = abi.load_hip_lib()
    scene, (w, h) = case
    want = _direct_frames(lib, scene, w, h)
    sc, cam = _fresh(SCENES[scene], pipeline, host)
    params = [su.camera_params(c, w, h)[0] for c in _drift(cam, FRAMES)]
    _settle(lib, sc, params[0], w, h)
    outs = [torch.full((h, w, 3), -1.0, dtype=torch.float32, device="cuda") for _ in params]
    before = _counts(lib, sc)
    for p, o in zip(params, outs):
        _enqueue(lib, sc, p, o)
    torch.cuda.synchronize()
    c = _counts(lib, sc) - before
    print("%s %dx%d pipeline %s host %s: pipelined %d, direct %d, in-flight queries %d, slot waits %d" % ((scene, w, h, pipeline, host) + tuple(c)))
    assert c[0] + c[1] == FRAMES
    if pipeline == "2":  # every eligible frame, in flight or not, and nothing asked: only the frames that record or sort the drifting camera's tile costs go direct
        assert c[0] >= FRAMES - 8 and c[2] == 0, c
    for k, o in enumerate(outs):
        _same(o.cpu().numpy(), want[k], "frame %d" % k)
    sc._release()


@pytest.mark.parametrize("host", ["2", None], ids=["time_proof", "default"])
def test_a_caller_that_waits_for_every_frame_is_never_pipelined(gpu, host):
    """40 frames, a host synchronisation after each: all of them on the direct path, with the time proof on."""
    import torch
    lib = abi.load_hip_lib()
    w, h = 160, 96
    sc, cam = _fresh(SCENES["balls"], "1", host)
    p = su.camera_params(cam, w, h)[0]
    _settle(lib, sc, p, w, h)
    out = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    for _ in range(6):  # (the handle's last call before the loop is a pipelined one)
        _enqueue(lib, sc, p, out)
    torch.cuda.synchronize()
    before = _counts(lib, sc)
    for _ in range(FRAMES):
        _enqueue(lib, sc, p, out)
        torch.cuda.synchronize()
    c = _counts(lib, sc) - before
    assert c[0] == 0 and c[1] == FRAMES, c
    sc._release()


@pytest.mark.parametrize("host", ["2", "0"], ids=["time_proof", "host0"])
def test_a_back_to_back_loop_is_pipelined(gpu, host):
    """40 frames of a resting camera back to back: with the time proof at least 36 are pipelined on fewer in-flight queries than frames; without it every pipelined frame was asked for."""
    import torch
    lib = abi.load_hip_lib()
    w, h = 173, 111
    sc, cam = _fresh(SCENES["balls"], "1", host)
    p = su.camera_params(cam, w, h)[0]
    _settle(lib, sc, p, w, h)
    out = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    before = _counts(lib, sc)
    for _ in range(FRAMES):
        _enqueue(lib, sc, p, out)
    torch.cuda.synchronize()
    c = _counts(lib, sc) - before
    print("host %s: pipelined %d, direct %d, in-flight queries %d, slot waits %d" % ((host,) + tuple(c)))
    assert c[0] + c[1] == FRAMES
    if host == "2":
        assert c[0] >= 36 and c[2] < FRAMES, c
    else:
        assert c[2] == FRAMES, c  # (one query per eligible call)
    sc._release()


@pytest.mark.parametrize("host", ["4", None], ids=["burst_start", "default"])
def test_a_burst_starts_behind_one_plain_direct_frame(gpu, host):
    """After a host synchronisation, behind matmuls that keep the caller's stream busy: frame 1 goes direct (its predecessor is over), frames 2 .. 5 are pipelined —
    the traces of 2 and 3 run before frame 1 has even started, frame 4's waits for it — and every one of them is the direct path's frame."""
    import torch
    lib = abi.load_hip_lib()
    w, h = 173, 111
    want = _direct_frames(lib, "balls", w, h)
    sc, cam = _fresh(SCENES["balls"], "1", host)
    params = [su.camera_params(c, w, h)[0] for c in _drift(cam, FRAMES)]
    _settle(lib, sc, params[0], w, h)
    outs = [torch.full((h, w, 3), -1.0, dtype=torch.float32, device="cuda") for _ in range(10)]
    a = torch.ones((4096, 4096), dtype=torch.float32, device="cuda")

    def busy():
        b = a
        for _ in range(6):
            b = (b @ b) * (1.0 / 4096.0)
    torch.cuda.synchronize()
    busy()
    for k in range(5):  # behind matmuls as well, so that the handle's last work before the burst is a pipelined frame
        _enqueue(lib, sc, params[k], outs[k])
    torch.cuda.synchronize()
    before = _counts(lib, sc)
    busy()
    for k in range(5, 10):
        _enqueue(lib, sc, params[k], outs[k])
    torch.cuda.synchronize()
    c = _counts(lib, sc) - before
    assert c[0] == 4 and c[1] == 1, c
    for k in range(10):
        _same(outs[k].cpu().numpy(), want[k], "frame %d" % k)
    sc._release()


@pytest.mark.parametrize("host", ["0", "7"], ids=["host0", "host7"])
def test_plan_reuse_is_off_by_default_and_still_right(gpu, host):
    """NRAYS_PIPELINE_LEAN=7 (the plan of an unchanged parameter block reused: no longer the default) renders cameras A A B B A A as the direct path does."""
    import torch
    lib = abi.load_hip_lib()
    w, h = 173, 111
    want = _direct_frames(lib, "balls", w, h)
    sc, cam = _fresh(SCENES["balls"], "2", host, lean="7")
    params = [su.camera_params(c, w, h)[0] for c in _drift(cam, 2)]
    _settle(lib, sc, params[0], w, h)
    seq = [0, 0, 1, 1, 0, 0]
    outs = [torch.full((h, w, 3), -1.0, dtype=torch.float32, device="cuda") for _ in seq]
    for k, o in zip(seq, outs):
        _enqueue(lib, sc, params[k], o)
    torch.cuda.synchronize()
    for n, (k, o) in enumerate(zip(seq, outs)):
        _same(o.cpu().numpy(), want[k], "step %d (camera %d)" % (n, k))
    sc._release()


def _check_timing(st, timed, wall_ms, what):
    """The bounds of test_pipeline_lean_gpu.py."""
    print("%s: frames_timed %d (want %d), kernel_ms_primary %.5f, kernel_ms_total %.5f, wall %.3f ms" % (what, st.frames_timed, timed, st.kernel_ms_primary, st.kernel_ms_total, wall_ms))
    assert st.frames_timed == timed, what
    assert 0.0 < st.kernel_ms_primary <= st.kernel_ms_total, what
    assert st.kernel_ms_total <= wall_ms, what
    assert st.kernel_ms_total > st.kernel_ms_primary, what + ": no timed frame was pipelined"


@pytest.mark.parametrize("stride", ["1", "3"], ids=["stride1", "stride3"])
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_spread_stamps_time_the_frame(gpu, case, stride):
    """16 drifting frames after the settle frames, one nrays_get_stats: every timed frame is counted and 0 < kernel_ms_primary <= kernel_ms_total <= wall time."""
    import torch
    lib = abi.load_hip_lib()
    scene, (w, h) = case
    sc, cam = _fresh(SCENES[scene], "2", "1", stride)
    params = [su.camera_params(c, w, h)[0] for c in _drift(cam, 16)]
    _settle(lib, sc, params[0], w, h)
    out = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    timed = sum(1 for k in range(16) if (4 + k) % int(stride) == 0)  # (the handle has rendered its four settle frames)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for p in params:
        _enqueue(lib, sc, p, out)
    torch.cuda.synchronize()
    wall_ms = (time.perf_counter() - t0) * 1e3
    _check_timing(nr.get_stats(sc), timed, wall_ms, "%s %dx%d stride %s" % (scene, w, h, stride))
    sc._release()


def test_spread_stamps_across_a_ring_wrap(gpu):
    """300 frames at stride 1, past the ring's 256 slots: the averages after frame 40 and after frame 300 (every slot in its second use) obey the same bounds —
    the ticks a slot's words keep from its earlier use are older and must lose."""
    import torch
    lib = abi.load_hip_lib()
    w, h = 64, 48
    sc, cam = _fresh(SCENES["balls"], "2", "1", "1")
    eye0 = np.array(cam["eye"], dtype=np.float64); at = np.array(cam["at"], dtype=np.float64)
    cam = dict(cam, eye=tuple(at + 3.0 * (eye0 - at)))  # far enough for a window of less than half the frame's blocks: the frames are pipelined
    params = [su.camera_params(c, w, h)[0] for c in _drift(cam, 300, step=2e-6)]
    _settle(lib, sc, params[0], w, h)
    out = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    for first, last, timed in ((0, 40, 40), (40, 300, KRING)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for p in params[first:last]:
            _enqueue(lib, sc, p, out)
        torch.cuda.synchronize()
        wall_ms = (time.perf_counter() - t0) * 1e3
        _check_timing(nr.get_stats(sc), timed, wall_ms, "frames %d..%d" % (first, last))
    sc._release()
