"""Pipeline depth (NRAYS_PIPELINE_DEPTH = 1, 2, 3: how many traces of one handle may be in flight, each on an internal stream of its own; read
once per scene handle) against the direct path (NRAYS_PIPELINE=0): every frame bit for bit, the counters of the last frame, and everything that
has to order itself behind three frames in flight.  What the depths differ in is what overlapping launches may not share: staging slots
(2 x depth, at least 4; a slot holds the rows of the window only), counter sets (launch n uses set n mod 2 x depth and clears the set of the next
launch on its own stream), a traversal-stack spill region per stream.  NRAYS_PIPELINE=2 pipelines every eligible frame whether its predecessor
has finished or not, so no case depends on how fast the host enqueues; the assertions are on pixels and counters, never on timing.
Scenes: balls (the stackless tiny-scene kernel) and `spheres` (300 reflecting balls: a kernel that walks the TLAS with its LDS / HBM traversal
stack while up to three traces overlap)."""
import ctypes as C
import os

import numpy as np
import pytest

import nrays_amd as nr
from nrays_amd import abi
from tools import scenes_util as su

pytestmark = pytest.mark.gpu

STAT_FIELDS = ("rays_primary", "rays_reflection", "rays_refraction", "rays_shadow", "rays_shadow_elided")
DEPTHS = ["1", "2", "3"]
SIZES = [(1920, 1080), (173, 111)]  # the second is not whole in wave tiles (16 x 16 pixels), and its rows are not whole in 16-byte chunks
FRAMES = 2 * 6 + 3 + 1              # slots (6 at depth 3) and counter sets (6) wrap twice, and then some


def _spheres():
    rng = np.random.RandomState(7)
    mats = [nr.NormalMaterial(), su.default_material()]
    nodes = [nr.SceneNode(mats[k & 1], 0.3, 0.25, 1.0, 1.0, nr.Isometry3(tuple(float(x) for x in rng.uniform(-3.0, 3.0, 3))), nr.Ball(float(rng.uniform(0.15, 0.45))))
             for k in range(300)]
    return nr.Scene(nodes, [nr.Light((4.0, 12.0, -9.0), 0.0, 1, (1, 1, 1))], (0.2, 0.3, 0.4)), dict(eye=(2.0, 6.0, -30.0), at=(0.0, 0.0, 0.0), fovy=45.0)


SCENES = {"balls": lambda: su.balls_scene(tex_size=(256, 128)), "spheres": _spheres}


class _env:
    """A scene handle reads its switches when it is created."""
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _fresh(make, pipeline, depth):
    with _env(NRAYS_PIPELINE=pipeline, NRAYS_PIPELINE_DEPTH=depth):
        sc, cam = make()
        sc.device_handle()
    return sc, cam


def _drift(cam, n, step=2e-5):
    """n pairwise different cameras so close to each other that the window of blocks that can see the scene stays what it is (a frame whose window
    changes records its tile costs on the direct path): frame 0 is `cam` itself, the whole path moves the view by a fraction of a pixel."""
    eye0 = np.array(cam["eye"], dtype=np.float64); at = np.array(cam["at"], dtype=np.float64)
    d = step * np.linalg.norm(eye0 - at) * np.array([1.0, 0.3, 0.0])
    return [dict(cam, eye=tuple(eye0 + k * d)) for k in range(n)]


def _enqueue(lib, sc, p, out):
    abi.check(lib.nrays_render_device(sc.device_handle(), C.byref(p), C.c_void_p(out.data_ptr()), None))


def _settle(lib, sc, p, w, h):
    """Four frames of the first camera: its tile costs recorded, sorted, the order decided — the frames after them are eligible."""
    import torch
    o = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    for _ in range(4):
        _enqueue(lib, sc, p, o)


def _same(a, b, what):
    diff = a.view(np.uint32) != b.view(np.uint32)
    assert not diff.any(), "%s: %d pixel components differ" % (what, int(diff.sum()))


def _stats(sc):
    st = nr.get_stats(sc)
    return st, {k: getattr(st, k) for k in STAT_FIELDS}


@pytest.mark.parametrize("one_buffer", [False, True], ids=["separate_buffers", "one_buffer_and_copies"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("scene", sorted(SCENES))
@pytest.mark.parametrize("depth", DEPTHS)
def test_consecutive_frames_are_the_direct_frames(gpu, depth, scene, size, one_buffer):
    """FRAMES consecutive frames with pairwise different cameras, enqueued without a host synchronisation: into buffers of their own, or all into one
    buffer with a device-to-device copy enqueued on the caller's stream after each call (copy k must be frame k); then the last frame's counters."""
    import torch
    lib = abi.load_hip_lib()
    w, h = size
    results = []
    for pipeline in ("2", "0"):
        sc, cam = _fresh(SCENES[scene], pipeline, depth)
        params = [su.camera_params(c, w, h)[0] for c in _drift(cam, FRAMES)]
        _settle(lib, sc, params[0], w, h)
        nr.get_stats(sc)  # (drains the timing ring: the averages below are over the frames that follow)
        outs = [torch.full((h, w, 3), -1.0, dtype=torch.float32, device="cuda") for _ in params]
        shared = torch.full((h, w, 3), -1.0, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for p, o in zip(params, outs):
            if one_buffer:
                _enqueue(lib, sc, p, shared)
                o.copy_(shared, non_blocking=True)  # the current (null) stream: the one the frames are enqueued on
            else:
                _enqueue(lib, sc, p, o)
        torch.cuda.synchronize()
        st, fields = _stats(sc)
        assert st.frames_timed >= 3
        if pipeline == "2":
            assert st.kernel_ms_total > st.kernel_ms_primary, "no timed frame was pipelined"
        results.append(([o.cpu().numpy() for o in outs], fields, nr.last_permutation(sc)))
        sc._release()
    (a, sa, pa), (b, sb, pb) = results
    for k in range(FRAMES):
        _same(a[k], b[k], "frame %d" % k)
    for k in range(FRAMES):  # the cameras do differ: a frame taken from another slot would show
        for j in range(k):
            assert (b[k].view(np.uint32) != b[j].view(np.uint32)).any(), "frames %d and %d are the same picture" % (j, k)
    assert sa == sb  # every ray class and rays_shadow_elided of the last frame
    assert pa == pb  # the trace launch is the frame's launch


@pytest.mark.parametrize("depth", DEPTHS)
def test_pipelined_direct_pipelined_with_frames_in_flight(gpu, depth):
    """Direct work between pipelined frames, three and more frames in flight at each switch: an instrumented render, a batch of caller rays, a camera
    jump (its first frames record and sort their tile costs on the direct path) and the way back.  Every frame, the batch, the instrumented
    frame's counters and the last frame's counters are those of a handle that renders everything on the direct path."""
    import torch
    lib = abi.load_hip_lib()
    w, h = 960, 540
    res = []
    for pipeline in ("2", "0"):
        sc, cam = _fresh(SCENES["balls"], pipeline, depth)
        near = _drift(cam, 8)
        eye0 = np.array(cam["eye"], dtype=np.float64); at = np.array(cam["at"], dtype=np.float64)
        far = _drift(dict(cam, eye=tuple(at + 1.6 * (eye0 - at) + np.array([0.5, 0.0, 0.0]))), 8)
        pn = [su.camera_params(c, w, h)[0] for c in near]
        pf = [su.camera_params(c, w, h)[0] for c in far]
        o_np, d_np, _ = nr.camera_rays((64, 36), cam["eye"], su.camera_params(cam, 64, 36)[1])
        ro, rd = torch.from_numpy(o_np).cuda(), torch.from_numpy(d_np).cuda()
        _settle(lib, sc, pn[0], w, h)
        seq = pn[:5] + ["instrumented"] + pn[3:8] + ["rays"] + pn[:5] + pf + pf[:4] + pn[:6]
        outs = [torch.full((h, w, 3), -1.0, dtype=torch.float32, device="cuda") for _ in seq]
        torch.cuda.synchronize()
        rays = ist = None
        for what, o in zip(seq, outs):
            if what == "instrumented":
                abi.check(lib.nrays_render_device_instrumented(sc.device_handle(), C.byref(pn[5]), C.c_void_p(o.data_ptr()), None))
                s = nr.get_stats(sc)
                ist = {k: getattr(s, k) for k in STAT_FIELDS + ("node_tests", "prim_tests", "rays_primary_traced")}
            elif what == "rays":
                rays = nr.trace_rays(sc, ro, rd, max_depth=0)
                o.zero_()
            else:
                _enqueue(lib, sc, what, o)
        torch.cuda.synchronize()
        _, fields = _stats(sc)
        res.append(([o.cpu().numpy() for o in outs], rays.cpu().numpy(), ist, fields))
        sc._release()
    (fa, ra, isa, sa), (fb, rb, isb, sb) = res
    for k in range(len(fa)):
        _same(fa[k], fb[k], "step %d of the sequence" % k)
    _same(ra, rb, "traced rays")
    assert isa == isb and sa == sb


@pytest.mark.parametrize("depth", DEPTHS)
def test_window_grows_with_frames_in_flight(gpu, depth):
    """A distant camera (a window of a few block rows), then a close one (many more rows: the staging rows are re-allocated while frames of the
    handle are in flight), then the distant one again (fewer rows than allocated)."""
    import torch
    lib = abi.load_hip_lib()
    w, h = 1280, 720
    res = []
    for pipeline in ("2", "0"):
        sc, cam = _fresh(SCENES["balls"], pipeline, depth)
        eye0 = np.array(cam["eye"], dtype=np.float64); at = np.array(cam["at"], dtype=np.float64)
        far = [su.camera_params(c, w, h)[0] for c in _drift(dict(cam, eye=tuple(at + 4.0 * (eye0 - at))), 7)]
        close = [su.camera_params(c, w, h)[0] for c in _drift(dict(cam, eye=tuple(at + 1.3 * (eye0 - at))), 7)]
        seq = far + close + far
        outs = [torch.full((h, w, 3), -1.0, dtype=torch.float32, device="cuda") for _ in seq]
        torch.cuda.synchronize()
        for p, o in zip(seq, outs):
            _enqueue(lib, sc, p, o)
        torch.cuda.synchronize()
        _, fields = _stats(sc)
        res.append(([o.cpu().numpy() for o in outs], fields))
        sc._release()
    (fa, sa), (fb, sb) = res
    for k in range(len(fa)):
        _same(fa[k], fb[k], "frame %d" % k)
    assert (fb[0] != fb[7]).any()  # (the two cameras do differ)
    assert sa == sb


@pytest.mark.parametrize("scene", sorted(SCENES))
@pytest.mark.parametrize("depth", DEPTHS)
def test_destroy_with_three_frames_in_flight(gpu, depth, scene):
    import torch
    lib = abi.load_hip_lib()
    w, h = 1920, 1080
    ref_sc, cam = _fresh(SCENES[scene], "0", depth)
    params = [su.camera_params(c, w, h)[0] for c in _drift(cam, 9)]
    _settle(lib, ref_sc, params[0], w, h)
    want = [torch.zeros((h, w, 3), dtype=torch.float32, device="cuda") for _ in params]
    for p, o in zip(params, want):
        _enqueue(lib, ref_sc, p, o)
    torch.cuda.synchronize()
    ref_sc._release()
    sc, _ = _fresh(SCENES[scene], "2", depth)
    _settle(lib, sc, params[0], w, h)
    outs = [torch.zeros((h, w, 3), dtype=torch.float32, device="cuda") for _ in params]
    for p, o in zip(params, outs):
        _enqueue(lib, sc, p, o)
    sc._release()  # returns with every frame finished: the buffers are the caller's again
    for k, o in enumerate(outs):
        _same(o.cpu().numpy(), want[k].cpu().numpy(), "frame %d of the destroyed handle" % k)
    sc2, _ = _fresh(SCENES[scene], "2", depth)  # and a handle created afterwards is none the worse for it
    _settle(lib, sc2, params[0], w, h)
    again = [torch.zeros((h, w, 3), dtype=torch.float32, device="cuda") for _ in params[:4]]
    for p, o in zip(params, again):
        _enqueue(lib, sc2, p, o)
    torch.cuda.synchronize()
    for k, o in enumerate(again):
        _same(o.cpu().numpy(), want[k].cpu().numpy(), "frame %d of the following handle" % k)
    sc2._release()
