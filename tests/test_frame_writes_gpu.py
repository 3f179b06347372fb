"""Every frame writes every float of its target and nothing beside it — on the direct path above all, the one bench.py times: it renders one
camera into one device buffer frame after frame, and "a resting camera reuses a work order, never a pixel".  A float that frame k does not
write holds frame k - 1's value in every other frame test of the suite (they render into the handle's own frame or into one reused buffer),
and for a resting camera that value is the right one.  Here every call gets a guarded buffer that was poisoned just before it
(tests/frame_writes.py): a quiet NaN with a payload, -1.0, or the frame of another camera.  For every frame of every case:
  (a) the guards are intact;  (b) no poison is left in the frame (and no NaN: the scenes are finite);  (c) the frame is bit-identical under
  the three poisons;  (d) it is bit-identical to the first frame of a fresh handle of the same scene and switches, itself rendered under a
  poison (a moving camera's frames: to the settled frame of that camera on a fresh handle);  and once per case  (e) the first frame is within
  1e-4 of the oracle (the north-star tolerance of BASELINE.json) with the oracle's ray classes.
Padding rows of a tiled frame hold exactly +0.0 (include/nrays_abi.h: NraysRenderParams::band_rows).
Every handle is created inside the case's environment (the library reads its switches in nrays_scene_create).  Cases about the direct path
run under NRAYS_PIPELINE=0 — and once with the switch unset, where a caller that synchronises after every frame must stay direct too — and
ask nrays_debug_pipeline_counts that every frame was direct.  Sizes: 173 x 111 (width * 3 no multiple of 4: the scalar row writers; ragged in
8 x 8 wave tiles and 16 x 16 blocks), 164 x 92 (the 16-byte row writers; ragged rows), 160 x 120 (whole tiles)."""
import ctypes as C

import numpy as np
import pytest

import nrays_amd as nr
import oracle
from nrays_amd import abi
from tests import frame_writes as fw
from tests import permutation_cases as pc
from tests.test_screen_cull_gpu import CAMERAS
from tools import scenes_util as su, standins

pytestmark = pytest.mark.gpu
CLASSES = ("rays_primary", "rays_reflection", "rays_refraction", "rays_shadow")
SWITCHES = ("NRAYS_PIPELINE", "NRAYS_LPT_ANALYTIC", "NRAYS_LEAD_WGS", "NRAYS_LDS_SCENE", "NRAYS_TINY_SCENE", "NRAYS_SCREEN_CULL", "NRAYS_MAX_PRIMARY",
            "NRAYS_LIGHT_SPLIT", "NRAYS_LPT", "NRAYS_GRID_WG_PER_CU", "NRAYS_OCC", "NRAYS_WAVEFRONT", "NRAYS_WF_MAX_PATHS", "NRAYS_WF_REFILL")
RAGGED, VECTOR, WHOLE = (173, 111), (164, 92), (160, 120)
ALIGNMENTS = [pytest.param(False, id="aligned"), pytest.param(True, id="plus4")]
MESH_FAR = dict(eye=(3.0, 14.0, -45.0), at=(0.0, 0.0, 0.0), fovy=40.0)  # the far camera of tests/test_screen_cull_gpu.py

SCENES = {
    "balls": lambda: su.balls_scene(tex_size=(256, 128)),
    "double": lambda: pc.double_scene(lights=2),
    "primitives": lambda: su.primitives_scene(0.0, 1),
    "analytic": lambda: pc.analytic_scene(),
    "sponza1": lambda: standins.sponza_scene(detail=0.2),
    "sponza8": lambda: standins.sponza_scene(detail=0.2, n_lights=8),
    "hair": lambda: standins.hairball_scene(strands=300),
    "mesh": lambda: (su.mesh_scene()[0], MESH_FAR),
}
_SCENES, _ORACLE, _STALE, _SETTLED = {}, {}, {}, {}


# ---- scenes, handles, references (each computed once, shared, never written) ----------------------------------------------------------------
def _scene(name):
    """(Scene, camera) of SCENES[name], built once; _fresh() gives it a new handle."""
    if name not in _SCENES:
        _SCENES[name] = SCENES[name]()
    return _SCENES[name]


def _fresh(monkeypatch, name, env):
    """A new handle of the scene, created with exactly the switches of `env` (NRAYS_PIPELINE=0 unless env says otherwise; None: unset)."""
    env = dict({"NRAYS_PIPELINE": "0"}, **env)
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        assert k in SWITCHES
        if v is not None:
            monkeypatch.setenv(k, v)
    sc, cam = _scene(name)
    sc._release()
    sc.device_handle()
    return sc, cam


def _key(p):
    return bytes(p)


def _plain(lib, sc, p, address):
    abi.check(lib.nrays_render_device(sc.device_handle(), C.byref(p), C.c_void_p(address), None))


def _instrumented(lib, sc, p, address):
    abi.check(lib.nrays_render_device_instrumented(sc.device_handle(), C.byref(p), C.c_void_p(address), None))


def _counted(flags):
    def call(lib, sc, p, address):
        abi.check(lib.nrays_render_device_counted(sc.device_handle(), C.byref(p), C.c_void_p(address), None, flags))
    return call


def _oracle(name, p):
    key = (name, _key(p))
    if key not in _ORACLE:
        img, st = oracle.render(_scene(name)[0].descriptor, p, 16)
        _ORACLE[key] = (img, {k: int(getattr(st, k)) for k in CLASSES})
    return _ORACLE[key]


def _other(cam):
    return dict(cam, eye=(cam["eye"][0] * 1.25 + 1.5, cam["eye"][1] * 1.25 + 0.5, cam["eye"][2]))


def _stale(monkeypatch, name, cam, w, h, kw):
    """The frame of ANOTHER camera of the scene with the same size and tiling, on the device: what a caller's buffer holds."""
    import torch
    p, _ = su.camera_params(_other(cam), w, h, **kw)
    key = (name, _key(p))
    if key not in _STALE:
        lib = abi.load_hip_lib()
        sc, _ = _fresh(monkeypatch, name, {})
        out = torch.zeros((int(lib.nrays_tile_rows(C.byref(p))), w, 3), dtype=torch.float32, device="cuda")
        _plain(lib, sc, p, out.data_ptr())
        torch.cuda.synchronize()
        _STALE[key] = out
    return _STALE[key]


def _counts(lib, sc):
    c = (C.c_uint64 * 4)()
    abi.check(lib.nrays_debug_pipeline_counts(sc.device_handle(), c))
    return int(c[0]), int(c[1])


def _checked(buf, kind, what):
    """(a), (b) and the padding rows of the buffer after a call; the frame."""
    rep = buf.check(kind)
    assert rep.problems() == [], (what, rep.problems())
    bad = np.flatnonzero(~np.isfinite(rep.frame.reshape(-1)))
    assert bad.size == 0, (what, "not finite at frame index %d" % int(bad[0]))
    return rep.frame


def _same(a, b, what):
    d = fw.first_difference(a, b)
    assert d is None, (what, "frame index %d: 0x%08X against 0x%08X" % d)


def _sequence(monkeypatch, name, env, params, buf, kind, stale, call, direct):
    """The frames of `params` in order on a fresh handle, each into the buffer poisoned with `kind` just before, the host waiting after each."""
    import torch
    lib = abi.load_hip_lib()
    sc, _ = _fresh(monkeypatch, name, env)
    before = _counts(lib, sc)
    frames, first = [], None
    # With pipelining allowed the library asks whether the caller's stream is idle (hipStreamQuery), and the poison's own fill would be in flight on it
    idle_stream = "NRAYS_PIPELINE" in env and env["NRAYS_PIPELINE"] is None
    for k, p in enumerate(params):
        buf.poison(kind, stale)
        if idle_stream:
            torch.cuda.synchronize()
        call(lib, sc, p, buf.address)
        torch.cuda.synchronize()
        frames.append(_checked(buf, kind, (kind, "frame %d" % k)))
        if k == 0:
            st = nr.get_stats(sc)
            first = {c: int(getattr(st, c)) for c in CLASSES}
    after = _counts(lib, sc)
    if direct:
        assert (after[0] - before[0], after[1] - before[1]) == (0, len(params)), (before, after)
    return frames, first


def _settled(monkeypatch, name, p):
    """A moving camera's reference: the third frame of that camera on a handle of its own (tests/test_regimes_gpu.py), under a poison too."""
    key = (name, _key(p))
    if key not in _SETTLED:
        buf = fw.DeviceBuffer(fw.Layout.of_params(abi.load_hip_lib(), p), False)
        _SETTLED[key] = _sequence(monkeypatch, name, {}, [p] * 3, buf, "neg", None, _plain, True)[0][-1]
    return _SETTLED[key]


def _case(monkeypatch, name, env, size, misaligned, kw=None, frames=8, moving=0, call=_plain, direct=True):
    """`frames` frames of the scene's camera at rest, then `moving` frames of a camera that moves 2e-3 of its distance per frame: (a) - (e)."""
    lib = abi.load_hip_lib()
    kw = dict(kw or {})
    w, h = size
    cam = _scene(name)[1]
    if "camera" in kw:
        cam = kw.pop("camera")
    eye0, at = np.array(cam["eye"], dtype=np.float64), np.array(cam["at"], dtype=np.float64)
    step = 2e-3 * np.linalg.norm(eye0 - at) * np.array([1.0, 0.3, 0.0])
    cams = [cam] * frames + [dict(cam, eye=tuple(eye0 + k * step)) for k in range(1, moving + 1)]
    params = [su.camera_params(c, w, h, **kw)[0] for c in cams]
    stale = _stale(monkeypatch, name, cam, w, h, kw)
    want_moving = [_settled(monkeypatch, name, p) for p in params[frames:]]
    buf = fw.DeviceBuffer(fw.Layout.of_params(lib, params[0]), misaligned)
    assert buf.address % 16 == (4 if misaligned else 0)
    got, first = {}, None
    for kind in fw.POISONS:
        got[kind], st = _sequence(monkeypatch, name, env, params, buf, kind, stale, call, direct)
        first = first or st
        assert st == first, (kind, st, first)
    for k in range(len(params)):
        _same(got["nan"][k], got["neg"][k], "frame %d, nan against neg" % k)                                   # (c)
        _same(got["nan"][k], got["stale"][k], "frame %d, nan against stale" % k)
        _same(got["nan"][k], got["nan"][0] if k < frames else want_moving[k - frames], "frame %d against a fresh handle's" % k)  # (d)
    ref, counts = _oracle(name, params[0])                                                                      # (e)
    assert np.abs(got["nan"][0] - ref).max() <= 1e-4
    assert first == counts
    return got["nan"]


# ---- balls: a resting camera through cold, recording and cost-ordered lists -------------------------------------------------------------------
BALLS_CAMERAS = ["bench view", "scene in a corner", "scene cut by the frame edge", "scene behind the camera", "eye inside the bounding box"]


@pytest.mark.parametrize("misaligned", ALIGNMENTS)
@pytest.mark.parametrize("size", [RAGGED, VECTOR, WHOLE], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("camera", BALLS_CAMERAS)
def test_balls_plain_frames(gpu, monkeypatch, camera, size, misaligned):
    _case(monkeypatch, "balls", {}, size, misaligned, dict(camera=CAMERAS[camera]))


@pytest.mark.parametrize("size,misaligned", [(RAGGED, True), (VECTOR, False)], ids=["173x111-plus4", "164x92-aligned"])
@pytest.mark.parametrize("camera", BALLS_CAMERAS)
def test_balls_anti_aliased_frames(gpu, monkeypatch, camera, size, misaligned):
    _case(monkeypatch, "balls", {}, size, misaligned, dict(camera=CAMERAS[camera], spp=4, window=1.0, seed=9))


@pytest.mark.parametrize("camera", BALLS_CAMERAS)
def test_balls_sixteen_samples_window_edge_inside_a_chunk(gpu, monkeypatch, camera):
    """Sixteen lanes per pixel: a wave tile is 2 x 2 pixels, so the window's edge is no multiple of four pixels and 16-byte chunks of the row
    writers straddle it (tile_device.h: the float-by-float branch)."""
    _case(monkeypatch, "balls", {}, VECTOR, False, dict(camera=CAMERAS[camera], spp=16, window=2.5, seed=11))


@pytest.mark.parametrize("size,misaligned", [(RAGGED, True), (VECTOR, False)], ids=["173x111-plus4", "164x92-aligned"])
@pytest.mark.parametrize("switch", ["NRAYS_LPT_ANALYTIC", "NRAYS_LEAD_WGS", "NRAYS_LDS_SCENE", "NRAYS_TINY_SCENE", "NRAYS_SCREEN_CULL"])
def test_balls_with_a_switch_off(gpu, monkeypatch, switch, size, misaligned):
    _case(monkeypatch, "balls", {switch: "0"}, size, misaligned, dict(camera=CAMERAS["bench view"]))


@pytest.mark.parametrize("misaligned", ALIGNMENTS)
@pytest.mark.parametrize("size", [RAGGED, VECTOR], ids=lambda s: "%dx%d" % s)
def test_a_synchronising_caller_stays_direct_with_the_pipeline_switch_unset(gpu, monkeypatch, size, misaligned):
    """NRAYS_PIPELINE unset (pipelining allowed): the host waits after every frame — and after the poison's fill, which is work on the
    caller's stream like a frame —, so no frame finds its stream busy."""
    _case(monkeypatch, "balls", {"NRAYS_PIPELINE": None}, size, misaligned, dict(camera=CAMERAS["bench view"]))


# ---- double branching: k_primary, the k_bounce rounds, then k_fold_fixed's read-modify-write ----------------------------------------------------
@pytest.mark.parametrize("misaligned", ALIGNMENTS)
@pytest.mark.parametrize("batches", [1, 3], ids=["one batch", "three batches"])
@pytest.mark.parametrize("name", ["double", "primitives"])
def test_double_branching_frames(gpu, monkeypatch, name, batches, misaligned):
    """Three batches: spp = 3 with a primary-ray budget of one sample per launch (tests/test_parity_gpu.py).  Only the first batch may write;
    the later ones, the folds and k_resolve work in place."""
    if batches == 1:
        _case(monkeypatch, name, {}, (96, 72), misaligned, dict(max_depth=5), frames=4)
    else:
        _case(monkeypatch, name, {"NRAYS_MAX_PRIMARY": str(96 * 72)}, (96, 72), misaligned, dict(max_depth=5, spp=3, window=1.0, seed=3), frames=4)


# ---- meshes: at rest, then moving (reused and aged orders) ------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,misaligned", [(RAGGED, True), (VECTOR, False)], ids=["173x111-plus4", "164x92-aligned"])
@pytest.mark.parametrize("name", ["sponza1", "sponza8", "hair", "mesh"])
def test_mesh_frames_at_rest_and_moving(gpu, monkeypatch, name, size, misaligned):
    _case(monkeypatch, name, {}, size, misaligned, frames=6, moving=6)


@pytest.mark.parametrize("name,env", [("sponza8", {"NRAYS_LIGHT_SPLIT": "-1"}), ("sponza8", {"NRAYS_LIGHT_SPLIT": "0"}), ("sponza1", {"NRAYS_LIGHT_SPLIT": "-1"}),
                                      ("sponza8", {"NRAYS_LPT": "0"}), ("sponza8", {"NRAYS_GRID_WG_PER_CU": "1"}), ("sponza8", {"NRAYS_OCC": "3"})],
                         ids=["every tile in light parts", "no tile in parts", "one light: pixel parts", "no cost order", "one workgroup per CU", "three waves"])
def test_mesh_frames_with_a_switch(gpu, monkeypatch, name, env):
    """(The moving frames' references are shared with the case above: a switch changes the schedule, never a pixel.)"""
    _case(monkeypatch, name, env, VECTOR, False, frames=6, moving=6)


# ---- bands: an owner's compact buffer, its padding rows exactly +0.0 --------------------------------------------------------------------------
BANDS = [dict(band_rows=16, band_owners=3, band_owner=0), dict(band_rows=16, band_owners=3, band_owner=1), dict(band_rows=16, band_owners=3, band_owner=2),
         dict(band_rows=1, band_owners=2, band_owner=1)]
BAND_IDS = ["16 rows, owner 0 of 3 (ragged band)", "16 rows, owner 1 of 3", "16 rows, owner 2 of 3", "1 row, owner 1 of 2"]


@pytest.mark.parametrize("misaligned", ALIGNMENTS)
@pytest.mark.parametrize("bands", BANDS, ids=BAND_IDS)
@pytest.mark.parametrize("name", ["balls", "sponza8"])
def test_band_tiles(gpu, monkeypatch, name, bands, misaligned):
    lay = fw.Layout.of_params(abi.load_hip_lib(), su.camera_params(_scene(name)[1], RAGGED[0], RAGGED[1], **bands)[0])
    rows_and_padding = {0: (48, 1), 1: (48, 16), 2: (48, 16)}[bands["band_owner"]] if bands["band_rows"] == 16 else (56, 1)  # of 111 rows
    assert (lay.rows, lay.pad_rows) == rows_and_padding
    _case(monkeypatch, name, {}, RAGGED, misaligned, bands, frames=4)


# ---- the staged path --------------------------------------------------------------------------------------------------------------------------
STAGED = [("sponza1", {}, {}, VECTOR), ("sponza8", {}, {}, RAGGED), ("hair", {}, {}, RAGGED), ("hair", {}, dict(spp=4, window=1.0, seed=3), VECTOR),
          ("hair", {"NRAYS_WF_MAX_PATHS": "4096"}, dict(spp=4, window=1.0, seed=3), (120, 80)), ("sponza8", {}, dict(band_rows=16, band_owners=3, band_owner=2), RAGGED)]


@pytest.mark.parametrize("refill", ["2", "0"], ids=["refill", "norefill"])
@pytest.mark.parametrize("name,env,kw,size", STAGED, ids=["sponza 1 light", "sponza 8 lights", "hair", "hair spp 4", "hair in several passes", "sponza owner 2 of 3"])
def test_staged_frames(gpu, monkeypatch, name, env, kw, size, refill):
    _case(monkeypatch, name, dict(env, NRAYS_WAVEFRONT="1", NRAYS_WF_REFILL=refill), size, refill == "0", kw, frames=3)


# ---- other entry points -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["balls", "sponza8"])
@pytest.mark.parametrize("entry", ["instrumented", "counted 0", "counted as timed"])
def test_instrumented_and_counted_frames(gpu, monkeypatch, entry, name):
    call = {"instrumented": _instrumented, "counted 0": _counted(0), "counted as timed": _counted(abi.COUNT_AS_TIMED)}[entry]
    for size, misaligned in ((RAGGED, True), (VECTOR, False)):
        frames = _case(monkeypatch, name, {}, size, misaligned, frames=3, call=call)
        plain = _case(monkeypatch, name, {}, size, misaligned, frames=1)
        _same(frames[0], plain[0], "%s against the plain frame" % entry)


# ---- pipelined frames: the trace aside, k_compose into the caller's buffer --------------------------------------------------------------------
@pytest.mark.parametrize("misaligned", ALIGNMENTS)
@pytest.mark.parametrize("size", [RAGGED, VECTOR], ids=lambda s: "%dx%d" % s)
def test_pipelined_frames(gpu, monkeypatch, size, misaligned):
    """NRAYS_PIPELINE=2, six frames back to back without a synchronisation, a guarded buffer each: both branches of k_compose."""
    import torch
    lib = abi.load_hip_lib()
    w, h = size
    cam = CAMERAS["bench view"]
    p, _ = su.camera_params(cam, w, h)
    stale = _stale(monkeypatch, "balls", cam, w, h, {})
    lay = fw.Layout.of_params(lib, p)
    want = _sequence(monkeypatch, "balls", {}, [p], fw.DeviceBuffer(lay, misaligned), "nan", None, _plain, True)[0][0]  # the direct frame
    got = {}
    for kind in fw.POISONS:
        sc, _ = _fresh(monkeypatch, "balls", {"NRAYS_PIPELINE": "2"})
        bufs = [fw.DeviceBuffer(lay, misaligned) for _ in range(6)]
        for b in bufs:
            b.poison(kind, stale)
        torch.cuda.synchronize()
        for b in bufs:
            _plain(lib, sc, p, b.address)
        torch.cuda.synchronize()
        pipelined, direct = _counts(lib, sc)
        assert pipelined + direct == 6 and pipelined >= 1, (pipelined, direct)
        got[kind] = [_checked(b, kind, (kind, "frame %d" % k)) for k, b in enumerate(bufs)]
    for k in range(6):
        _same(got["nan"][k], got["neg"][k], "frame %d, nan against neg" % k)
        _same(got["nan"][k], got["stale"][k], "frame %d, nan against stale" % k)
        _same(got["nan"][k], want, "frame %d against the direct frame" % k)
    ref, _ = _oracle("balls", p)
    assert np.abs(want - ref).max() <= 1e-4


# ---- host buffers -----------------------------------------------------------------------------------------------------------------------------
def _quantise(f):
    """Image::to_png's rule as tests/test_frontend_gpu.py states it: c * 255, clamped to [0, 255], truncated."""
    v = f * np.float32(255.0)
    v = np.where(v > 0, v, np.float32(0.0))
    return np.minimum(v, np.float32(255.0)).astype(np.uint8)


@pytest.mark.parametrize("misaligned", ALIGNMENTS)
@pytest.mark.parametrize("kw", [dict(), dict(band_rows=16, band_owners=3, band_owner=2)], ids=["untiled", "owner 2 of 3"])
def test_host_buffers(gpu, monkeypatch, kw, misaligned):
    """nrays_render and nrays_render_rgb8 into guarded host allocations: guards in floats and in bytes, the device frame's content."""
    lib = abi.load_hip_lib()
    w, h = RAGGED
    cam = CAMERAS["bench view"]
    p, _ = su.camera_params(cam, w, h, **kw)
    lay = fw.Layout.of_params(lib, p)
    want = _sequence(monkeypatch, "balls", {}, [p], fw.DeviceBuffer(lay, misaligned), "nan", None, _plain, True)[0][0]
    stale = _stale(monkeypatch, "balls", cam, w, h, kw).cpu().numpy()
    sc, _ = _fresh(monkeypatch, "balls", {})
    floats, bytes_ = fw.HostBuffer(lay, misaligned), fw.HostBuffer(lay, misaligned, np.uint8)
    for kind in fw.POISONS:
        for k in range(2):
            floats.poison(kind, stale)
            abi.check(lib.nrays_render(sc.device_handle(), C.byref(p), C.cast(C.c_void_p(floats.address), C.POINTER(C.c_float))))
            _same(_checked(floats, kind, ("nrays_render", kind, k)), want, ("nrays_render", kind, k))
    seen = {}
    for kind in ("nan", "neg"):
        bytes_.poison(kind)
        abi.check(lib.nrays_render_rgb8(sc.device_handle(), C.byref(p), C.cast(C.c_void_p(bytes_.address), C.POINTER(C.c_uint8))))
        rep = bytes_.check(kind)
        assert rep.problems() == [], ("nrays_render_rgb8", kind, rep.problems())
        seen[kind] = rep.frame
        _same(rep.frame, _quantise(want), ("nrays_render_rgb8", kind))
    _same(seen["nan"], seen["neg"], "nrays_render_rgb8, nan against neg")


# ---- caller batches that share bounce.hip -----------------------------------------------------------------------------------------------------
_BATCHES = {}


def _batch(monkeypatch, name):
    """Rays of the scene's camera that hit something, and the hit points with their normals: 257 of each, computed once."""
    if name not in _BATCHES:
        from nrays_amd import math3d
        sc, cam = _fresh(monkeypatch, name, {})
        o, d, _ = nr.camera_rays((40, 30), cam["eye"], math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], 40, 30))
        hits = nr.closest_hits(sc, o, d, want=("normal", "flags"))
        sel = np.flatnonzero((hits.flags & 1) != 0)
        assert len(sel) >= 257
        sel = sel[np.linspace(0, len(sel) - 1, 257).astype(int)]
        o, d = np.ascontiguousarray(o[sel]), np.ascontiguousarray(d[sel])
        nm = hits.normal[sel]
        facing = (nm * d).sum(axis=1) > 0
        _BATCHES[name] = (o, d, np.ascontiguousarray(o + d * hits.toi[sel][:, None]), np.ascontiguousarray(np.where(facing[:, None], -nm, nm)))
    return _BATCHES[name]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
@pytest.mark.parametrize("name", ["double", "analytic"])
@pytest.mark.parametrize("entry", ["trace_rays", "gather_points"])
def test_caller_batches(gpu, monkeypatch, entry, name, n):
    """nrays_trace_rays_device / nrays_gather_points_device write n x 3 floats: k_trace_rays or the gather kernel, then — in the double-branching
    scene — the k_bounce rounds and k_fold_fixed on the caller's colours."""
    import torch
    lib = abi.load_hip_lib()
    depth = 5 if name == "double" else 0
    o, d, pts, nms = (a[:n] for a in _batch(monkeypatch, name))
    sc, _ = _fresh(monkeypatch, name, {})
    h = sc.device_handle()
    L, rot = nr.hemisphere_dirs(8), nr.rotation_table(3)
    if entry == "trace_rays":
        want = nr.trace_rays(sc, o, d, max_depth=depth)                                  # the host form
        held = [torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()]

        def call(address):
            abi.check(lib.nrays_trace_rays_device(h, n, held[0].data_ptr(), held[1].data_ptr(), None, None, None, depth, address, None))
    else:
        want = nr.gather_points(sc, pts, nms, L, rot, 1e-3, 1.0, depth)
        held = [torch.from_numpy(pts).cuda(), torch.from_numpy(nms).cuda(), torch.from_numpy(L).cuda(), torch.from_numpy(rot).cuda()]
        gp = abi.NraysGatherParams(len(L), len(rot), held[2].data_ptr(), held[3].data_ptr(), 1e-3, 1.0, depth)

        def call(address):
            abi.check(lib.nrays_gather_points_device(h, n, held[0].data_ptr(), held[1].data_ptr(), None, None, C.byref(gp), address, 0, None))
    assert np.isfinite(want).all() and (want != 0).any()
    for misaligned in (False, True):
        buf = fw.DeviceBuffer(fw.Layout(1, n), misaligned)
        got = {}
        for kind in ("nan", "neg"):
            buf.poison(kind)
            call(buf.address)
            torch.cuda.synchronize()
            got[kind] = _checked(buf, kind, (entry, kind, misaligned)).reshape(n, 3)
        _same(got["nan"], got["neg"], "nan against neg")
        _same(got["nan"], np.ascontiguousarray(want, dtype=np.float32), "against the host form")
