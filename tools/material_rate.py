#!/usr/bin/env python
"""Rate of material_points() (nrays_material_points_device: per point the terms of its node's material without the lights) and of indirect_points() on the first
hits of the sponza stand-in's 1080p camera rays (about 2 M points), beside shade_points() and irradiance_points() on the same points in the same run.  Points in
surface order (the camera's scan order) and shuffled; and 16 384 of them.  All calls are interleaved in one process: every figure is the median of `rounds`
timings of `reps` back-to-back calls between two events on one stream, reported with its spread; the copy bandwidth of the same run (a device-to-device copy of
1 GiB, read + written bytes) gives the traffic floor.

The expectations are written into the output file BEFORE the first timing; the finished file reports MET or MISSED beside the measured values:

  python tools/material_rate.py [--out profiles/material_rate.json] [--reps 10] [--quick]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.irradiance_rate import _copy_gbs, _hit_inputs  # noqa: E402
from tools.trace_rays_rate import _time  # noqa: E402

EXPECTATION = {
    "a": "material_points(want=(ambient, diffuse)) is cheaper than shade_points on the same points in the same run: it is that call's first texture fetch without any "
         "shadow ray (shade_hits stood at 0.70 - 0.79 ms in profiles/irradiance_rate.json / shade_points_rate.json; the comparison is with this run's own figure)",
    "b": "indirect_points costs no more than irradiance_points + material_points(want=(diffuse,)) + two element-wise torch products timed separately: it is exactly "
         "those",
    "c": "no threshold: the fraction of the traffic floor at the run's measured copy bandwidth — 24 bytes in (uv 16, node 4, flags 4) and 12 out a point for the "
         "diffuse term alone, 24 more in (the normal) and 16 more out with the ambient term — for surface order and shuffled"}
FLOOR_DIFFUSE, FLOOR_BOTH = 24 + 12, 24 + 12 + 24 + 16
GRID = (32, 16, 32)


def _row(sc, inp, reps, rounds, gbs):
    import torch
    import nrays_amd as nr
    p, nm = inp["points"], inp["normals"]
    n = p.shape[0]
    lo, hi = p.min(dim=0).values.cpu().numpy(), p.max(dim=0).values.cpu().numpy()
    origin, cell = tuple(float(x) for x in lo), tuple(float(x) for x in (hi - lo) / (np.asarray(GRID) - 1))
    sh = torch.from_numpy(np.random.default_rng(3).uniform(0.0, 1.0, size=(GRID[0] * GRID[1] * GRID[2], 9, 3)).astype(np.float32)).cuda()
    grid = nr.ProbeGrid(origin, cell, GRID, sh)
    d0 = nr.material_points(sc, inp["nodes"], None, inp["uvs"], inp["flags"], want=("diffuse",)).diffuse
    e0 = nr.irradiance_points(sc, p, nm, grid, hit_flags=inp["flags"])
    fns = {
        "material_ambient_diffuse": lambda: nr.material_points(sc, inp["nodes"], nm, inp["uvs"], inp["flags"], want=("ambient", "diffuse")),
        "material_diffuse": lambda: nr.material_points(sc, inp["nodes"], None, inp["uvs"], inp["flags"], want=("diffuse",)),
        "material_all_four": lambda: nr.material_points(sc, inp["nodes"], nm, inp["uvs"], inp["flags"], want=("ambient", "diffuse", "specular", "node")),
        "shade_points": lambda: nr.shade_points(sc, p, nm, inp["view"], inp["nodes"], inp["uvs"], inp["flags"]),
        "irradiance_points": lambda: nr.irradiance_points(sc, p, nm, grid, hit_flags=inp["flags"]),
        "two_products": lambda: (d0 * e0) * nr.scene.INV_PI_F32,
        "indirect_points": lambda: nr.indirect_points(sc, p, nm, inp["nodes"], grid, inp["uvs"], inp["flags"]),
    }
    ms = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            ms[name].append(_time(fn, reps, warmup=1))
    row = {"points": int(n), "rounds": rounds, "reps": reps}
    for name, v in ms.items():
        row[name] = {"ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    med = lambda name: row[name]["ms"]  # noqa: E731
    floor = lambda bytes_: n * bytes_ / (gbs * 1e9) * 1e3  # noqa: E731  (ms)
    row["material_ambient_diffuse"]["expectation_a"] = "MET" if med("material_ambient_diffuse") < med("shade_points") else "MISSED"
    parts = med("irradiance_points") + med("material_diffuse") + med("two_products")
    row["indirect_points"]["sum_of_its_parts_ms"] = round(parts, 4)
    row["indirect_points"]["expectation_b"] = "MET" if med("indirect_points") <= parts else "MISSED"
    for name, bytes_ in (("material_diffuse", FLOOR_DIFFUSE), ("material_ambient_diffuse", FLOOR_BOTH)):
        row[name]["floor_ms"] = round(floor(bytes_), 4)
        row[name]["fraction_of_floor"] = round(floor(bytes_) / med(name), 4)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "material_rate.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="320x180 instead of 1920x1080 (a rehearsal of the tool, not a measurement)")
    args = ap.parse_args()
    out = {"expectation": EXPECTATION, "status": "expectations written before the first run; no measurement yet"}

    def write():
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    write()
    import torch
    from tools import standins
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    w, h = (320, 180) if args.quick else (1920, 1080)
    sc, cam = standins.sponza_scene()
    sc.device_handle()
    inp = _hit_inputs(sc, cam, w, h)
    n = inp["points"].shape[0]
    perm = torch.from_numpy(np.random.default_rng(11).permutation(n)).cuda()
    shuffled = {k: v[perm].contiguous() for k, v in inp.items()}
    sub = torch.from_numpy(np.linspace(0, n - 1, min(16384, n)).astype(np.int64)).cuda()
    subset = {k: v[sub].contiguous() for k, v in inp.items()}
    gbs = _copy_gbs()
    del out["status"]
    out.update({"device": torch.cuda.get_device_name(0), "scene": "sponza stand-in, first hits of the camera rays", "resolution": [w, h],
                "copy_bandwidth_gb_s": round(gbs, 1), "floor_bytes_per_point": {"diffuse": FLOOR_DIFFUSE, "ambient_diffuse": FLOOR_BOTH}})
    out["surface_order"] = _row(sc, inp, args.reps, args.rounds, gbs)
    out["shuffled"] = _row(sc, shuffled, args.reps, args.rounds, gbs)
    out["subset_16384"] = _row(sc, subset, args.reps * 4, args.rounds, gbs)
    verdicts = [v2[key] for v in out.values() if isinstance(v, dict) for v2 in v.values() if isinstance(v2, dict) for key in ("expectation_a", "expectation_b") if key in v2]
    out["met"], out["missed"] = verdicts.count("MET"), verdicts.count("MISSED")
    write()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
