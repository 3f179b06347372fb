#!/usr/bin/env python
"""(GPU box) The flagship loop (balls 1920x1080, 200 frames back to back) through the probe: frames pipelined / direct, in-flight queries, slot waits
(nrays_debug_pipeline_counts; NRAYS_PIPELINE_HOST is taken from the environment).

  python tools/pipeline_counts.py
"""
import ctypes as C, os, sys, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from nrays_amd import abi
from tools import scenes_util as su
torch.cuda.set_device(0)
lib = abi.load_hip_lib()
sc, cam = su.balls_scene()
h = sc.device_handle()
w, hh = 1920, 1080
p, _ = su.camera_params(cam, w, hh)
out = torch.empty((hh, w, 3), dtype=torch.float32, device="cuda")
def counts():
    c = (C.c_uint64 * 4)(); abi.check(lib.nrays_debug_pipeline_counts(h, c)); return list(c)
for _ in range(24): abi.check(lib.nrays_render_device(h, C.byref(p), C.c_void_p(out.data_ptr()), None))
torch.cuda.synchronize()
for steps in (200, 20):
    b = counts()
    for _ in range(steps): abi.check(lib.nrays_render_device(h, C.byref(p), C.c_void_p(out.data_ptr()), None))
    torch.cuda.synchronize()
    a = counts()
    print(json.dumps({"host": os.environ.get("NRAYS_PIPELINE_HOST", "default"), "steps": steps, "pipelined": a[0] - b[0], "direct": a[1] - b[1], "inflight_queries": a[2] - b[2], "slot_waits": a[3] - b[3]}))
