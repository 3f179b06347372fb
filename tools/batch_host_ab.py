"""One process of the host-time A/B of the caller-batch call path (profiles/batch_driver_host_ab.log): the library NRAYS_HIP_LIB names (or the tree's).

  NRAYS_HIP_LIB=<parent build>/libnrays_hip.so python tools/batch_host_ab.py parent ; python tools/batch_host_ab.py change   (alternate, five each)
  Prints one line: label, us per device-form cast call of 64 rays,
us per device-form gather call of 64 points x 16 directions (2000 back-to-back calls each, one sync at the end), ms of one blocking trace of 2^20 rays,
and the host's share of the two loops (the time until the calls had returned)."""
import ctypes as C
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import nrays_amd as nr
from nrays_amd import abi, math3d
from tests.test_batch_stage_gpu import _scene, _t
from tests.test_occlusion_gpu import hit_points

label, calls = sys.argv[1], 2000
torch.cuda.set_device(0)
lib = abi.load_hip_lib()
sc, cam = _scene()
h = sc.device_handle()
o, d, _ = nr.camera_rays((8, 8), cam["eye"], math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], 8, 8), seed=2)
hits = nr.closest_hits(sc, o, d)
p, nm = hit_points(o, d, hits)
to, td, tp, tn, tf = _t(o), _t(d), _t(p), _t(nm), _t(hits.flags)
toi = torch.empty(64, dtype=torch.float64, device="cuda"); node = torch.empty(64, dtype=torch.int32, device="cuda")
rgb = torch.empty((64, 3), dtype=torch.float32, device="cuda")
L = torch.from_numpy(nr.hemisphere_dirs(16)).cuda()
gp = abi.NraysGatherParams(16, 0, L.data_ptr(), None, 1e-3, 1.0, 0)
stream = torch.cuda.current_stream().cuda_stream
cast = lambda: lib.nrays_cast_rays_device(h, 64, to.data_ptr(), td.data_ptr(), None, toi.data_ptr(), node.data_ptr(), None, None, None, None, 0, stream)  # noqa: E731
gather = lambda: lib.nrays_gather_points_device(h, 64, tp.data_ptr(), tn.data_ptr(), tf.data_ptr(), None, C.byref(gp), rgb.data_ptr(), 0, stream)  # noqa: E731
out, enq = [], []
for fn in (cast, gather):
    for _ in range(200):  # warm: workspace, code objects
        abi.check(fn())
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    enq.append((time.perf_counter() - t0) / calls * 1e6)  # the host's share: the calls have returned, the device has not finished
    torch.cuda.synchronize()
    out.append((time.perf_counter() - t0) / calls * 1e6)
n = 1 << 20
o2, d2, _ = nr.camera_rays((1024, 1024), cam["eye"], math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], 1024, 1024), seed=3)
nr.trace_rays(sc, o2[:4096], d2[:4096])  # warm
t0 = time.perf_counter()
nr.trace_rays(sc, o2, d2)
out.append((time.perf_counter() - t0) * 1e3)
print("%-7s cast_device_64 %8.3f us/call   gather_device_64x16 %8.3f us/call   trace_blocking_2^20 %8.3f ms   (host enqueue alone: cast %6.3f, gather %6.3f us/call)" % (label, out[0], out[1], out[2], enq[0], enq[1]), flush=True)
