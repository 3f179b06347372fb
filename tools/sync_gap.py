#!/usr/bin/env python
"""(GPU box) Shortest gap between the return of one nrays_render_device and the entry of the next for a caller that synchronises after every frame: balls, 64x64, least of 200 —
switches.h: kInFlightProofUs is half of it — and the gaps of a loop that does not synchronise, 1920x1080.

  python tools/sync_gap.py
"""
import ctypes as C, os, sys, time, json
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from nrays_amd import abi
from tools import scenes_util as su
torch.cuda.set_device(0)
lib = abi.load_hip_lib()
sc, cam = su.balls_scene()
h = sc.device_handle()
w = hh = 64
p, _ = su.camera_params(cam, w, hh)
out = torch.empty((hh, w, 3), dtype=torch.float32, device="cuda")
fn = lib.nrays_render_device
ptr = C.c_void_p(out.data_ptr()); ref = C.byref(p)
for _ in range(8):
    fn(h, ref, ptr, None); torch.cuda.synchronize()
cs = torch.cuda.current_stream()
for mode in ("torch.cuda.synchronize", "torch current_stream().synchronize"):
    hip = cs if mode.endswith(".synchronize") and "current" in mode else None
    gaps = []; t_ret = None
    for _ in range(201):
        t_in = time.perf_counter()
        fn(h, ref, ptr, None)
        t_out = time.perf_counter()
        if t_ret is not None: gaps.append((t_in - t_ret) * 1e6)
        t_ret = t_out
        if hip is None: torch.cuda.synchronize()
        else: hip.synchronize()
    gaps.sort()
    print(json.dumps({"sync": mode, "frames": len(gaps), "gap_us_min": round(gaps[0], 2), "gap_us_p10": round(gaps[len(gaps)//10], 2), "gap_us_median": round(gaps[len(gaps)//2], 2)}))
# the steady (unsynchronised) loop's own gap between calls, 1920x1080
w, hh = 1920, 1080
p, _ = su.camera_params(cam, w, hh)
out = torch.empty((hh, w, 3), dtype=torch.float32, device="cuda"); ptr = C.c_void_p(out.data_ptr()); ref = C.byref(p)
for _ in range(30): fn(h, ref, ptr, None)
gaps = []; t_ret = None
for _ in range(201):
    t_in = time.perf_counter(); fn(h, ref, ptr, None); t_out = time.perf_counter()
    if t_ret is not None: gaps.append((t_in - t_ret) * 1e6)
    t_ret = t_out
torch.cuda.synchronize(); gaps.sort()
print(json.dumps({"sync": "none (back to back, 1920x1080)", "gap_us_min": round(gaps[0], 2), "gap_us_median": round(gaps[len(gaps)//2], 2), "gap_us_p90": round(gaps[len(gaps)*9//10], 2), "gap_us_max": round(gaps[-1], 2)}))
