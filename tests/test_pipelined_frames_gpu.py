"""Pipelined frames of one handle (frame_path.hip: pipeline_prepare / pipeline_compose — a frame enqueued while its predecessor is in flight traces its window on an
internal stream and is composed into `out` on the caller's stream, k_compose) against the direct path (NRAYS_PIPELINE=0, read once per scene
handle): every frame bit for bit, `out` written in the caller's stream order, the counters, and everything that has to order itself behind
frames in flight.  NRAYS_PIPELINE=2 pipelines every eligible frame whether its predecessor has finished or not, so that the cases do not
depend on how fast the host enqueues; NRAYS_PIPELINE=1 (the default) is run beside it.
Scenes: balls (the stackless tiny-scene kernel), `spheres` (300 reflecting balls without a plane: a kernel that walks the TLAS with its LDS /
HBM traversal stack while two traces overlap), and primitives, which is never pipelined (double branching, and its plane makes the window the
whole frame): for it the cases check that the switch changes nothing.  Whether frames WERE pipelined is read from nrays_get_stats: a timed
pipelined frame's kernel_ms_total runs from its trace to the end of its compose, a direct one-launch frame's equals kernel_ms_primary."""
import ctypes as C
import os

import numpy as np
import pytest

import nrays_amd as nr
from nrays_amd import abi
from tools import scenes_util as su

pytestmark = pytest.mark.gpu

STAT_FIELDS = ("rays_primary", "rays_reflection", "rays_refraction", "rays_shadow", "rays_shadow_elided")
def _spheres():
    rng = np.random.RandomState(7)
    mats = [nr.NormalMaterial(), su.default_material()]
    nodes = [nr.SceneNode(mats[k & 1], 0.3, 0.25, 1.0, 1.0, nr.Isometry3(tuple(float(x) for x in rng.uniform(-3.0, 3.0, 3))), nr.Ball(float(rng.uniform(0.15, 0.45))))
             for k in range(300)]
    return nr.Scene(nodes, [nr.Light((4.0, 12.0, -9.0), 0.0, 1, (1, 1, 1))], (0.2, 0.3, 0.4)), dict(eye=(2.0, 6.0, -30.0), at=(0.0, 0.0, 0.0), fovy=45.0)


SCENES = {"balls": lambda: su.balls_scene(tex_size=(256, 128)), "primitives": lambda: su.primitives_scene(0.0, 1), "spheres": _spheres}
PIPELINED = ("balls", "spheres")  # the scenes whose resting / nearby frames are eligible
SIZES = [(1920, 1080), (173, 111)]


class _mode:
    """A scene handle reads NRAYS_PIPELINE when it is created."""
    def __init__(self, flag):
        self.flag = flag

    def __enter__(self):
        self.old = os.environ.get("NRAYS_PIPELINE")
        os.environ["NRAYS_PIPELINE"] = self.flag

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop("NRAYS_PIPELINE", None)
        else:
            os.environ["NRAYS_PIPELINE"] = self.old


def _fresh(make, flag):
    with _mode(flag):
        sc, cam = make()
        sc.device_handle()
    return sc, cam


def _moving(cam, n):
    """The camera path of tests/test_regimes_gpu.py: a nearby camera every frame (orders reused, costs recorded and re-sorted on the way)."""
    eye0 = np.array(cam["eye"], dtype=np.float64); at = np.array(cam["at"], dtype=np.float64)
    step = 2e-3 * np.linalg.norm(eye0 - at) * np.array([1.0, 0.3, 0.0])
    return [dict(cam, eye=tuple(eye0 + k * step)) for k in range(n)]


def _enqueue(lib, sc, p, out, stream=None):
    abi.check(lib.nrays_render_device(sc.device_handle(), C.byref(p), C.c_void_p(out.data_ptr()), C.c_void_p(stream) if stream else None))


def _frames(sc, params, w, h, stream=None):
    """The frames of `params` enqueued back to back without a host synchronisation, each into a buffer of its own."""
    import torch
    lib = abi.load_hip_lib()
    outs = [torch.full((h, w, 3), -1.0, dtype=torch.float32, device="cuda") for _ in params]
    torch.cuda.synchronize()
    for p, o in zip(params, outs):
        _enqueue(lib, sc, p, o, stream)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


def _same(a, b, what):
    diff = a.view(np.uint32) != b.view(np.uint32)
    assert not diff.any(), "%s: %d pixel components differ" % (what, int(diff.sum()))


@pytest.mark.parametrize("flag", ["2", "1"])
@pytest.mark.parametrize("path", ["resting", "moving"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("scene", sorted(SCENES))
def test_back_to_back_frames_are_the_direct_frames(gpu, scene, size, path, flag):
    w, h = size
    n = 12 if path == "resting" else 24  # (the moving path crosses a recording and a sorting frame, which drop to the direct path)
    results = []
    for f in (flag, "0"):
        sc, cam = _fresh(SCENES[scene], f)
        cams = [cam] * n if path == "resting" else _moving(cam, n)
        params = [su.camera_params(c, w, h)[0] for c in cams]
        frames = _frames(sc, params, w, h)
        st = nr.get_stats(sc)
        results.append((frames, {k: getattr(st, k) for k in STAT_FIELDS}, nr.last_permutation(sc)))
        # frames 0, 4, 8, ... are timed; frame 0 is the cold one (direct), the others rest or are nearby cameras
        assert st.frames_timed >= 3
        if f == "2" and scene in PIPELINED:
            assert st.kernel_ms_total > st.kernel_ms_primary, "no timed frame was pipelined"
        if f == "0" and scene in PIPELINED and path == "resting":
            assert st.kernel_ms_total == st.kernel_ms_primary  # direct one-launch frames: the same pair of events
        sc._release()
    (a, sa, pa), (b, sb, pb) = results
    if scene == "spheres":
        assert not (pa[0][1] & 256) and pa[0][1] & 1  # an analytic kernel with the traversal stack, not the stackless one
    for k in range(n):
        _same(a[k], b[k], "frame %d" % k)
    assert sa == sb       # ray classes and rays_shadow_elided of the last frame
    assert pa == pb       # the trace launch is the frame's launch


@pytest.mark.parametrize("flag", ["2", "1"])
def test_out_is_written_in_stream_order(gpu, flag):
    """A device-to-device copy of `out` enqueued on the caller's stream after EACH of 8 frames with 8 different cameras: copy k is frame k."""
    import torch
    lib = abi.load_hip_lib()
    w, h = 640, 360
    copies = []
    for f in (flag, "0"):
        sc, cam = _fresh(SCENES["balls"], f)
        eye0 = np.array(cam["eye"], dtype=np.float64)
        for _ in range(4):  # the scheduling state of the first camera settles
            nr.render(sc, (w, h), 1, 0.0, cam["eye"], su.camera_params(cam, w, h)[1])
        params = [su.camera_params(dict(cam, eye=tuple(eye0 + 0.01 * k * np.array([1.0, 0.5, 0.2]))), w, h)[0] for k in range(8)]
        out = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        snaps = [torch.empty_like(out) for _ in params]
        torch.cuda.synchronize()
        for p, s in zip(params, snaps):
            _enqueue(lib, sc, p, out)
            s.copy_(out, non_blocking=True)  # the current (null) stream: the one the frames were enqueued on
        torch.cuda.synchronize()
        copies.append([s.cpu().numpy() for s in snaps])
        sc._release()
    for k in range(8):
        _same(copies[0][k], copies[1][k], "copy %d" % k)
    assert any((copies[1][k] != copies[1][0]).any() for k in range(1, 8))  # (the cameras do differ)


@pytest.mark.parametrize("flag", ["2", "1"])
def test_caller_streams(gpu, flag):
    """The null stream, a blocking and a non-blocking stream of the caller, and the same `out` rendered from two streams alternately."""
    import torch
    lib = abi.load_hip_lib()
    hip = C.CDLL("libamdhip64.so")
    w, h = 480, 270
    blocking = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(blocking)) == 0
    nonblocking = torch.cuda.Stream()
    try:
        ref_sc, cam = _fresh(SCENES["balls"], "0")
        eye0 = np.array(cam["eye"], dtype=np.float64)
        params = [su.camera_params(dict(cam, eye=tuple(eye0 + 0.02 * k * np.array([1.0, 0.0, 0.3]))), w, h)[0] for k in range(10)]
        want = _frames(ref_sc, params, w, h)
        ref_sc._release()
        for name, streams in (("null", [None]), ("blocking", [blocking.value]), ("non-blocking", [nonblocking.cuda_stream]),
                              ("alternating", [blocking.value, nonblocking.cuda_stream])):
            sc, _ = _fresh(SCENES["balls"], flag)
            out = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            for k, p in enumerate(params):  # every frame into the SAME buffer: the last one must be what is left
                _enqueue(lib, sc, p, out, streams[k % len(streams)])
            torch.cuda.synchronize()
            _same(out.cpu().numpy(), want[-1], "%s stream(s), last frame" % name)
            got = [torch.zeros_like(out) for _ in params]
            torch.cuda.synchronize()  # (the fills run on torch's current stream, which a non-blocking caller stream is not ordered behind)
            for k, p in enumerate(params):  # and frame by frame (the handle is settled by now: resting / nearby cameras)
                _enqueue(lib, sc, p, got[k], streams[k % len(streams)])
            torch.cuda.synchronize()
            for k in range(len(params)):
                _same(got[k].cpu().numpy(), want[k], "%s stream(s), frame %d" % (name, k))
            sc._release()
    finally:
        torch.cuda.synchronize()
        hip.hipStreamDestroy(blocking)


@pytest.mark.parametrize("flag", ["2", "1"])
def test_other_entry_points_order_themselves_behind_frames_in_flight(gpu, flag):
    """An instrumented render and nrays_trace_rays_device issued while frames are in flight give their usual results, and so do the frames after them."""
    import torch
    lib = abi.load_hip_lib()
    w, h = 640, 360
    res = []
    for f in (flag, "0"):
        sc, cam = _fresh(SCENES["balls"], f)
        p, proj = su.camera_params(cam, w, h)
        o_np, d_np, _ = nr.camera_rays((64, 36), cam["eye"], su.camera_params(cam, 64, 36)[1])
        ro, rd = torch.from_numpy(o_np).cuda(), torch.from_numpy(d_np).cuda()
        outs = [torch.zeros((h, w, 3), dtype=torch.float32, device="cuda") for _ in range(16)]
        torch.cuda.synchronize()
        for o in outs[:8]:
            _enqueue(lib, sc, p, o)
        rays = nr.trace_rays(sc, ro, rd, max_depth=0)                       # frames in flight
        for o in outs[8:12]:
            _enqueue(lib, sc, p, o)
        instr = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda")
        abi.check(lib.nrays_render_device_instrumented(sc.device_handle(), C.byref(p), C.c_void_p(instr.data_ptr()), None))
        ist = nr.get_stats(sc)
        for o in outs[12:]:
            _enqueue(lib, sc, p, o)
        torch.cuda.synchronize()
        st = nr.get_stats(sc)
        res.append(([o.cpu().numpy() for o in outs], rays.cpu().numpy(), instr.cpu().numpy(),
                    {k: getattr(ist, k) for k in STAT_FIELDS + ("node_tests", "prim_tests", "rays_primary_traced")}, {k: getattr(st, k) for k in STAT_FIELDS}))
        sc._release()
    (fa, ra, ia, isa, sa), (fb, rb, ib, isb, sb) = res
    for k in range(16):
        _same(fa[k], fb[k], "frame %d" % k)
        _same(fa[k], ia, "frame %d against the instrumented one" % k)
    _same(ra, rb, "traced rays"); _same(ia, ib, "instrumented frame")
    assert isa == isb and sa == sb


@pytest.mark.parametrize("flag", ["2", "1"])
def test_destroy_with_frames_in_flight(gpu, flag):
    import torch
    lib = abi.load_hip_lib()
    w, h = 1920, 1080
    ref_sc, cam = _fresh(SCENES["balls"], "0")
    p, _ = su.camera_params(cam, w, h)
    want = _frames(ref_sc, [p] * 2, w, h)[-1]
    ref_sc._release()
    sc, _ = _fresh(SCENES["balls"], flag)
    outs = [torch.zeros((h, w, 3), dtype=torch.float32, device="cuda") for _ in range(10)]
    for o in outs:
        _enqueue(lib, sc, p, o)
    sc._release()  # returns with every frame finished: the buffers are the caller's again
    for k, o in enumerate(outs):
        _same(o.cpu().numpy(), want, "frame %d of the destroyed handle" % k)
    sc2, _ = _fresh(SCENES["balls"], flag)
    for k, f in enumerate(_frames(sc2, [p] * 6, w, h)):
        _same(f, want, "frame %d of the following handle" % k)
    sc2._release()
