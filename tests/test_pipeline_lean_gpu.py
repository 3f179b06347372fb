"""The lean host path of a pipelined frame (NRAYS_PIPELINE_LEAN, read once per scene handle; 0 = the path as it was) against what it replaces:
  stamps      a timed pipelined frame records no events — its trace and its compose leave clock ticks in the handle's ring of device stamps, and
              nrays_get_stats averages them with the event-timed frames (direct, instrumented, cost-recording) of the same interval;
  slot proof  a trace is launched into a staging slot without a query when a compose at or after the slot's last one has been seen finished;
  plan reuse  a call with the parameter block of the call before it reuses that call's plan.
NRAYS_PIPELINE=2 pipelines every eligible frame, in flight or not, so nothing depends on how fast the host enqueues; cameras drift by a fraction of a
pixel, so the window stays what it is; four settle frames come first (the helpers' style of test_pipeline_depth_gpu.py).  Pixels are compared bit for
bit with the direct path (NRAYS_PIPELINE=0); the timings are only bounded: 0 < kernel_ms_primary <= kernel_ms_total <= wall time of the loop."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import nrays_amd as nr
from nrays_amd import abi
from tools import scenes_util as su

pytestmark = pytest.mark.gpu

STAT_FIELDS = ("rays_primary", "rays_reflection", "rays_refraction", "rays_shadow", "rays_shadow_elided")
LEAN = [None, "0"]  # the library's default (all three parts), and the host path of the parent
CASES = [("balls", (173, 111)), ("spheres", (256, 144))]
SLOT_FRAMES = 2 * 6 + 4  # the six staging slots wrap twice, and then some
KRING = 256              # scene_handle.h: NraysScene::kRing


def _spheres():
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


def _fresh(make, pipeline, lean=None, stride=None):
    with _env(NRAYS_PIPELINE=pipeline, NRAYS_PIPELINE_LEAN=lean, NRAYS_EVENT_STRIDE=stride):
        sc, cam = make()
        sc.device_handle()
    return sc, cam


def _drift(cam, n, step=2e-5):
    eye0 = np.array(cam["eye"], dtype=np.float64); at = np.array(cam["at"], dtype=np.float64)
    d = step * np.linalg.norm(eye0 - at) * np.array([1.0, 0.3, 0.0])
    return [dict(cam, eye=tuple(eye0 + k * d)) for k in range(n)]


def _enqueue(lib, sc, p, out, instrumented=False):
    fn = lib.nrays_render_device_instrumented if instrumented else lib.nrays_render_device
    abi.check(fn(sc.device_handle(), C.byref(p), C.c_void_p(out.data_ptr()), None))


def _settle(lib, sc, p, w, h):
    import torch
    o = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    for _ in range(4):
        _enqueue(lib, sc, p, o)
    torch.cuda.synchronize()
    nr.get_stats(sc)  # drains the timing ring: the averages that follow are over the frames that follow


def _same(a, b, what):
    diff = a.view(np.uint32) != b.view(np.uint32)
    assert not diff.any(), "%s: %d pixel components differ" % (what, int(diff.sum()))


def _check_timing(st, timed, wall_ms, what, pipelined=True):
    print("%s: frames_timed %d (want %d), kernel_ms_primary %.5f, kernel_ms_total %.5f, wall %.3f ms" % (what, st.frames_timed, timed, st.kernel_ms_primary, st.kernel_ms_total, wall_ms))
    assert st.frames_timed == timed, what
    assert 0.0 < st.kernel_ms_primary <= st.kernel_ms_total, what
    assert st.kernel_ms_total <= wall_ms, what
    if pipelined:  # (a direct frame's total is its trace; a pipelined one's ends with its compose)
        assert st.kernel_ms_total > st.kernel_ms_primary, what + ": no timed frame was pipelined"


@pytest.mark.parametrize("every_third_instrumented", [False, True], ids=["plain", "every_third_instrumented"])
@pytest.mark.parametrize("stride", ["1", None], ids=["stride1", "default_stride"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s_%dx%d" % ((c[0],) + c[1]))
@pytest.mark.parametrize("lean", LEAN, ids=["lean", "lean0"])
def test_stamped_frames_are_timed(gpu, lean, case, stride, every_third_instrumented):
    """16 drifting frames after the settle frames, one nrays_get_stats: every timed frame of the interval is counted, whether its slot holds events or stamps."""
    import torch
    lib = abi.load_hip_lib()
    scene, (w, h) = case
    sc, cam = _fresh(SCENES[scene], "2", lean, stride)
    params = [su.camera_params(c, w, h)[0] for c in _drift(cam, 16)]
    _settle(lib, sc, params[0], w, h)
    out = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    n_stride = int(stride or 4)
    timed = 0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k, p in enumerate(params):
        instrumented = every_third_instrumented and k % 3 == 2
        timed += 1 if (instrumented or (4 + k) % n_stride == 0) else 0  # (the handle has rendered its four settle frames)
        _enqueue(lib, sc, p, out, instrumented)
    torch.cuda.synchronize()
    wall_ms = (time.perf_counter() - t0) * 1e3
    st = nr.get_stats(sc)
    _check_timing(st, timed, wall_ms, "%s %dx%d" % (scene, w, h))
    sc._release()


@pytest.mark.parametrize("lean", LEAN, ids=["lean", "lean0"])
def test_ring_wrap_keeps_stale_stamps_out(gpu, lean):
    """300 frames at stride 1, past the ring's 256 slots: the averages after frame 40 and after frame 300 (the latter over the ring's 256 newest frames,
    every slot in its second use) obey the same bounds — a slot's stamps of its earlier use must not leak into them."""
    import torch
    lib = abi.load_hip_lib()
    w, h = 64, 48
    sc, cam = _fresh(SCENES["balls"], "2", lean, "1")
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


_direct = {}


def _direct_frames(lib, scene, w, h):
    """The SLOT_FRAMES drifting frames of a scene on the direct path: rendered once, shared, never changed."""
    import torch
    if (scene, w, h) not in _direct:
        sc, cam = _fresh(SCENES[scene], "0")
        params = [su.camera_params(c, w, h)[0] for c in _drift(cam, SLOT_FRAMES)]
        _settle(lib, sc, params[0], w, h)
        outs = [torch.full((h, w, 3), -1.0, dtype=torch.float32, device="cuda") for _ in params]
        for p, o in zip(params, outs):
            _enqueue(lib, sc, p, o)
        torch.cuda.synchronize()
        frames = [o.cpu().numpy() for o in outs]
        for f in frames:
            f.setflags(write=False)
        _direct[(scene, w, h)] = (frames, {k: getattr(nr.get_stats(sc), k) for k in STAT_FIELDS})
        sc._release()
    return _direct[(scene, w, h)]


@pytest.mark.parametrize("how", ["back_to_back", "sync_every_fifth", "behind_matmuls"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s_%dx%d" % ((c[0],) + c[1]))
@pytest.mark.parametrize("lean", LEAN, ids=["lean", "lean0"])
def test_slots_are_reused_only_behind_their_compose(gpu, lean, case, how):
    """SLOT_FRAMES drifting frames into ONE buffer, a device-to-device copy on the caller's stream after each call (copy k must be frame k): back to back; with
    a host synchronisation after every fifth call (the slot's compose is then proved by a newer one); behind large matmuls on the caller's stream (no compose
    has finished while the host enqueues: the fall-back query and the wait run)."""
    import torch
    lib = abi.load_hip_lib()
    scene, (w, h) = case
    want, want_fields = _direct_frames(lib, scene, w, h)
    sc, cam = _fresh(SCENES[scene], "2", lean)
    params = [su.camera_params(c, w, h)[0] for c in _drift(cam, SLOT_FRAMES)]
    _settle(lib, sc, params[0], w, h)
    outs = [torch.full((h, w, 3), -1.0, dtype=torch.float32, device="cuda") for _ in params]
    shared = torch.full((h, w, 3), -1.0, dtype=torch.float32, device="cuda")
    a = torch.ones((4096, 4096), dtype=torch.float32, device="cuda") if how == "behind_matmuls" else None
    torch.cuda.synchronize()
    if a is not None:
        for _ in range(6):
            a = (a @ a) * (1.0 / 4096.0)
    for k, (p, o) in enumerate(zip(params, outs)):
        _enqueue(lib, sc, p, shared)
        o.copy_(shared, non_blocking=True)  # the current (null) stream: the one the frames are enqueued on
        if how == "sync_every_fifth" and k % 5 == 4:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    fields = {k: getattr(nr.get_stats(sc), k) for k in STAT_FIELDS}
    for k, o in enumerate(outs):
        _same(o.cpu().numpy(), want[k], "frame %d" % k)
    assert fields == want_fields
    sc._release()


_fresh_direct = {}


def _fresh_direct_frame(lib, key, p, w, h, instrumented=False):
    """Frame `p` of a fresh balls handle on the direct path (and, instrumented, its counters): rendered once per key, shared, never changed."""
    import torch
    if key not in _fresh_direct:
        sc, _ = _fresh(SCENES["balls"], "0")
        o = torch.full((h, w, 3), -1.0, dtype=torch.float32, device="cuda")
        _enqueue(lib, sc, p, o, instrumented)
        torch.cuda.synchronize()
        s = nr.get_stats(sc)
        img = o.cpu().numpy(); img.setflags(write=False)
        _fresh_direct[key] = (img, {k: getattr(s, k) for k in STAT_FIELDS + ("node_tests", "prim_tests", "rays_primary_traced")})
        sc._release()
    return _fresh_direct[key]


@pytest.mark.parametrize("lean", LEAN, ids=["lean", "lean0"])
def test_a_changed_parameter_block_is_planned_anew(gpu, lean):
    """One handle renders cameras A, B, A, A, B; then A with max_depth 1 instead of 4, with another seed, at another resolution, each followed by A itself;
    then an instrumented A after a plain A.  Every frame is the frame of a fresh handle on the direct path, the instrumented frame's counters are that handle's."""
    import torch
    lib = abi.load_hip_lib()
    w, h = 173, 111
    sc, cam = _fresh(SCENES["balls"], "2", lean)
    cam_b = _drift(cam, 2, step=3e-5)[1]

    def block(c, size=(w, h), **kw):
        return su.camera_params(c, size[0], size[1], **dict(dict(max_depth=4), **kw))[0]
    seq = [("A", block(cam), (w, h), False), ("B", block(cam_b), (w, h), False), ("A", block(cam), (w, h), False), ("A", block(cam), (w, h), False), ("B", block(cam_b), (w, h), False),
           ("A", block(cam), (w, h), False), ("A depth 1", block(cam, max_depth=1), (w, h), False),
           ("A", block(cam), (w, h), False), ("A seed 9", block(cam, seed=9), (w, h), False),
           ("A", block(cam), (w, h), False), ("A 256x144", block(cam, size=(256, 144)), (256, 144), False),
           ("A", block(cam), (w, h), False), ("A instrumented", block(cam), (w, h), True)]
    _settle(lib, sc, seq[0][1], w, h)
    outs = [torch.full((sh, sw, 3), -1.0, dtype=torch.float32, device="cuda") for _, _, (sw, sh), _ in seq]
    torch.cuda.synchronize()
    for (_, p, _, instrumented), o in zip(seq, outs):
        _enqueue(lib, sc, p, o, instrumented)
    torch.cuda.synchronize()
    s = nr.get_stats(sc)
    counters = {k: getattr(s, k) for k in STAT_FIELDS + ("node_tests", "prim_tests", "rays_primary_traced")}
    for k, ((name, p, (sw, sh), instrumented), o) in enumerate(zip(seq, outs)):
        want, want_counters = _fresh_direct_frame(lib, name, p, sw, sh, instrumented)
        _same(o.cpu().numpy(), want, "step %d (%s)" % (k, name))
    assert counters == want_counters  # (the sequence ends with the instrumented frame)
    depth1, full = _fresh_direct_frame(lib, "A depth 1", None, w, h)[0], _fresh_direct_frame(lib, "A", None, w, h)[0]
    assert (depth1 != full).any() and (_fresh_direct_frame(lib, "B", None, w, h)[0] != full).any()  # (the blocks do differ in what they render)
    sc._release()
