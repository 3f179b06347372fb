#!/usr/bin/env python
"""Rays per second of nrays_trace_rays_device (caller-supplied rays) beside nrays_render_device of the same frame.

  (a) balls 1080p camera rays in image order (pixel-major, as camera_rays() gives them)
  (b) the same rays shuffled (incoherent order)
  (c) sponza stand-in 1080p camera rays, then AO-style cosine-weighted rays from their first hits (normal side, 1e-3 off the surface),
      timed as one batch (camera + AO) and the AO rays alone

Each batch and each frame: warm-up, then 20 launches timed by HIP events around all of them.  The render's value_traced is bench.py's
figure (rays that went through a BVT query per second, from an instrumented frame counted as the timed kernel traces).

  python tools/trace_rays_rate.py [--out profiles/trace_rays_rate.json] [--reps 20] [--quick]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAST_DTYPE = np.dtype([("toi", "<f8"), ("normal", "<f8", 3), ("uv", "<f8", 2), ("node_id", "<i4"), ("flags", "<u4")])


def _time(fn, reps, warmup=3):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps  # ms per launch


def _batch(sc, o, d, reps, keys=None):
    import torch
    import nrays_amd as nr
    to, td = torch.from_numpy(np.ascontiguousarray(o)).cuda(), torch.from_numpy(np.ascontiguousarray(d)).cuda()
    tk = None if keys is None else torch.from_numpy(keys.astype(np.int64)).cuda()
    ms = _time(lambda: nr.trace_rays(sc, to, td, keys=tk), reps)
    return {"rays": int(len(o)), "ms": round(ms, 4), "mrays_per_s": round(len(o) / (ms * 1e-3) / 1e6, 2)}


def _render(sc, p, reps):
    import torch
    import nrays_amd as nr
    from nrays_amd import abi
    lib = abi.load_hip_lib()
    out = torch.empty((p.height, p.width, 3), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ms = _time(lambda: abi.check(lib.nrays_render_device(sc.device_handle(), C.byref(p), C.c_void_p(out.data_ptr()), stream)), reps)
    abi.check(lib.nrays_render_device_counted(sc.device_handle(), C.byref(p), C.c_void_p(out.data_ptr()), stream, abi.COUNT_AS_TIMED))
    st = nr.get_stats(sc)
    traced = int(st.rays_traced()) - int(st.rays_shadow_elided)
    npx = p.width * p.height
    return {"ms": round(ms, 4), "primary_mrays_per_s": round(npx / (ms * 1e-3) / 1e6, 2),
            "rays_traced_per_frame": traced, "value_traced": round(traced / (ms * 1e-3) / 1e6, 2)}


def _first_hits(sc, o, d):
    """Closest hits of the camera rays (nrays_debug_cast_batch mode 0, blocking): AO rays from each hit, cosine-weighted about the normal."""
    from nrays_amd import abi
    n = len(o)
    res = np.zeros(n, dtype=CAST_DTYPE)
    abi.check(abi.load_hip_lib().nrays_debug_cast_batch(sc.device_handle(), 0, n, o.ctypes.data_as(C.POINTER(C.c_double)), d.ctypes.data_as(C.POINTER(C.c_double)),
                                                        None, res.ctypes.data_as(C.POINTER(abi.NraysCastResult))))
    hit = (res["flags"] & 1) != 0
    pt = o[hit] + d[hit] * res["toi"][hit][:, None]
    nrm = res["normal"][hit]
    nrm = nrm / np.linalg.norm(nrm, axis=1)[:, None]
    nrm = np.where(((nrm * d[hit]).sum(axis=1) > 0.0)[:, None], -nrm, nrm)  # the side the camera ray came from
    rng = np.random.default_rng(0)
    u1, u2 = rng.uniform(size=len(pt)), rng.uniform(size=len(pt))
    r, phi = np.sqrt(u1), 2.0 * np.pi * u2
    local = np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(np.maximum(0.0, 1.0 - u1))], axis=1)
    a = np.where(np.abs(nrm[:, 0:1]) > 0.9, np.asarray([[0.0, 1.0, 0.0]]), np.asarray([[1.0, 0.0, 0.0]]))
    t = np.cross(a, nrm)
    t /= np.linalg.norm(t, axis=1)[:, None]
    b = np.cross(nrm, t)
    dirs = local[:, 0:1] * t + local[:, 1:2] * b + local[:, 2:3] * nrm
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    return pt + nrm * 1e-3, dirs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trace_rays_rate.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="320x180 instead of 1920x1080 (a rehearsal of the tool, not a measurement)")
    a = ap.parse_args()
    import torch
    import nrays_amd as nr
    from nrays_amd import math3d
    from tools import scenes_util as su
    from tools import standins
    assert torch.cuda.is_available(), "the rate tool measures the GPU; there is nothing to measure without one"
    torch.cuda.set_device(0)
    w, h = (320, 180) if a.quick else (1920, 1080)
    res = {"tool": "tools/trace_rays_rate.py", "resolution": [w, h], "reps": a.reps, "device": torch.cuda.get_device_name(0), "workloads": {}}

    sc, cam = su.balls_scene()
    proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], w, h)
    o, d, k = nr.camera_rays((w, h), cam["eye"], proj)
    res["workloads"]["a_balls_image_order"] = _batch(sc, o, d, a.reps, k)
    perm = np.random.default_rng(1).permutation(len(o))
    res["workloads"]["b_balls_shuffled"] = _batch(sc, o[perm], d[perm], a.reps, k[perm])
    res["workloads"]["balls_render_device"] = _render(sc, nr.make_params((w, h), 1, 0.0, cam["eye"], proj), a.reps)
    del sc

    sc, cam = standins.sponza_scene()
    proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], w, h)
    o, d, k = nr.camera_rays((w, h), cam["eye"], proj)
    ao_o, ao_d = _first_hits(sc, o, d)
    res["workloads"]["c_sponza_camera_plus_ao"] = dict(_batch(sc, np.concatenate([o, ao_o]), np.concatenate([d, ao_d]), a.reps),
                                                       camera_rays=int(len(o)), ao_rays=int(len(ao_o)))
    res["workloads"]["c_sponza_camera_only"] = _batch(sc, o, d, a.reps, k)
    res["workloads"]["c_sponza_ao_only"] = _batch(sc, ao_o, ao_d, a.reps)
    res["workloads"]["sponza_render_device"] = _render(sc, nr.make_params((w, h), 1, 0.0, cam["eye"], proj), a.reps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
