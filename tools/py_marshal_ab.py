"""One process of the host-time A/B of the Python batch wrappers (profiles/py_marshal_host_ab.log): us per wrapper call over 2 000 calls after 200 warm-up calls.

  python tools/py_marshal_ab.py LABEL numpy|torch [--tree DIR]      (DIR: the checkout whose nrays_amd is timed, e.g. a git worktree of the parent; default: this one)

  numpy: the stand-in library of tools/call_transcript.py, so only the Python layer is timed (no GPU): closest_hits (64 rays), shade_points (64 points),
         gather_points (64 points x 16 directions).
  torch: the real library (NRAYS_HIP_LIB, or the tree's) on CUDA tensors, as tools/batch_host_ab.py does: the time until the calls have returned, and the time with
         one sync at the end: closest_hits (64), gather_points (64 x 16), surface_texels (8 x 8, device="cuda").
Run parent and change alternately, five processes each, in one session.  Then

  python tools/py_marshal_ab.py verdict LOG

reads the lines and prints, per figure, both medians, the parent's spread (max - min of its five runs) and whether the change's median <= the parent's median + that spread."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
label, form = sys.argv[1], sys.argv[2]
if label == "verdict":
    import re
    import statistics
    runs = {}
    for line in open(form):
        m = re.match(r"(parent|change) +(numpy|torch) ", line)
        if m:
            for key, val in re.findall(r"(\S+)=([\d.]+)", line):
                runs.setdefault("%s.%s" % (m.group(2), key), {}).setdefault(m.group(1), []).append(float(val))
    ok = True
    for key, r in runs.items():
        pm, cm, spread = statistics.median(r["parent"]), statistics.median(r["change"]), max(r["parent"]) - min(r["parent"])
        ok &= cm <= pm + spread
        print("verdict %-36s parent median %8.3f (n=%d, spread %6.3f)   change median %8.3f (n=%d)   %s" % (key, pm, len(r["parent"]), spread, cm, len(r["change"]),
                                                                                                            "ok" if cm <= pm + spread else "MISS"))
    sys.exit(0 if ok else 1)
sys.path.insert(0, sys.argv[4] if len(sys.argv) > 4 and sys.argv[3] == "--tree" else ROOT)
import numpy as np

import nrays_amd as nr  # the timed tree's; tools and tests below are this tree's
sys.path[0] = ROOT
from nrays_amd import math3d
from tools import call_transcript as ct

WARM, CALLS = 200, 2000


def timed(fn, sync=None):
    for _ in range(WARM):
        fn()
    if sync:
        sync()
    t0 = time.perf_counter()
    for _ in range(CALLS):
        fn()
    returned = (time.perf_counter() - t0) / CALLS * 1e6
    if sync:
        sync()
    return returned, (time.perf_counter() - t0) / CALLS * 1e6


if form == "numpy":
    rng = np.random.RandomState(3)
    sc = ct.stub_scene()
    o, d, v = (np.ascontiguousarray(rng.rand(64, 3)) for _ in range(3))
    nodes, L = np.zeros(64, np.int32), nr.hemisphere_dirs(16)
    with ct.stand_in(nr.abi) as rec:
        us = [timed(fn)[0] for fn in (lambda: nr.closest_hits(sc, o, d), lambda: nr.shade_points(sc, o, d, v, nodes), lambda: nr.gather_points(sc, o, d, L))]
        del rec.calls[:]
    print("%-7s numpy  closest_hits_64=%.3f   shade_points_64=%.3f   gather_points_64x16=%.3f   us/call" % (label, us[0], us[1], us[2]), flush=True)
else:
    import torch
    from tests.test_batch_stage_gpu import _scene, _t
    from tests.test_occlusion_gpu import hit_points
    torch.cuda.set_device(0)
    sc, cam = _scene()
    o, d, _ = nr.camera_rays((8, 8), cam["eye"], math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], 8, 8), seed=2)
    hits = nr.closest_hits(sc, o, d)
    p, nm = hit_points(o, d, hits)
    to, td, tp, tn, tf, L = _t(o), _t(d), _t(p), _t(nm), _t(hits.flags), _t(nr.hemisphere_dirs(16))
    r = [timed(fn, torch.cuda.synchronize) for fn in (lambda: nr.closest_hits(sc, to, td), lambda: nr.gather_points(sc, tp, tn, L, hit_flags=tf),
                                                      lambda: nr.surface_texels(sc, 0, 8, 8, device="cuda"))]
    print("%-7s torch  returned.closest_hits_64=%.3f   returned.gather_points_64x16=%.3f   returned.surface_texels_8x8=%.3f   synced.closest_hits_64=%.3f   "
          "synced.gather_points_64x16=%.3f   synced.surface_texels_8x8=%.3f   us/call" % (label, r[0][0], r[1][0], r[2][0], r[0][1], r[1][1], r[2][1]), flush=True)
