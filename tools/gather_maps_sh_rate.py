#!/usr/bin/env python
"""Rates of probes filled from baked maps (nrays_gather_maps_sh_points_device) on the sponza stand-in, every node reading one shared 1024 x 1024 map.

gather_maps_probes() with and without its depth side for 4 096 probes x 1 024 sphere directions and 16 384 probes x 64 directions at R = 8, on lattices over the
bounding box of the camera's first hits, beside existing calls timed in the same run on the same rays: closest_hits() on the rays given as arrays (uv and flags),
gather_maps_points() (the same query and sample, folded to a mean in the lanes), probe_depth() and gather_probes(max_depth=0) (Scene::trace on the rays: direct
light).  With --parent-lib, gather_maps_points and probe_depth of a library built from the parent commit are timed in a child process under NRAYS_HIP_LIB on the
same inputs.  Every figure is the median of `rounds` timings of `reps` back-to-back calls between two events on one stream; the calls of a row are interleaved
round by round.

The expectations were written before the first run; the JSON reports MET or MISSED beside the measured values:

  python tools/gather_maps_sh_rate.py [--out profiles/gather_maps_sh_rate.json] [--reps 10] [--parent-lib PATH] [--quick]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.irradiance_rate import _hit_inputs  # noqa: E402
from tools.trace_rays_rate import _time  # noqa: E402

EXPECTATION = {
    "a": "with depth, the fused call is cheaper than a depth-less call of its own plus probe_depth on the same probes: one traversal replaces two, and the depth side adds 4 "
         "bytes a ray stored and one more fold over them",
    "b": "without depth, the call is no dearer than probe_depth on the same rays — both run the same query, store per-ray floats (12 bytes against 4) and fold them (27 "
         "accumulators a probe against 64 texels) — and it is cheaper than gather_probes(max_depth=0), whose rays run Scene::trace with its shadow rays",
    "c": "gather_maps_points and probe_depth of this tree equal those of a library built from the parent commit, timed in the same run, within the larger of the two "
         "rows' own spread (max_ms - min_ms): splitting gather_maps_ray into the query and the contribution changes no instruction of k_gather_maps_points"}
RES = 8
MAP_SIDE = 1024
SHARED_ROWS = ("gather_maps_points", "probe_depth")  # the calls the parent library has too


def _stats(v):
    return {"ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def _inputs(sc, lo, hi, counts, k):
    import torch
    import nrays_amd as nr
    cell = tuple(float(x) for x in (hi - lo) / (np.asarray(counts) + 1))
    origin = tuple(float(x) for x in lo + np.asarray(cell))  # the lattice strictly inside the box
    pos = torch.from_numpy(nr.probe_grid_positions(origin, cell, counts)).cuda()
    nz = torch.zeros_like(pos)
    nz[:, 2] = 1.0
    texels = torch.from_numpy(np.random.default_rng(17).uniform(0.0, 1.0, size=(MAP_SIDE, MAP_SIDE, 4)).astype(np.float32)).cuda()
    return dict(pos=pos, nz=nz, tl=torch.from_numpy(nr.sphere_dirs(k)).cuda(), maps=[texels], node_map=[0] * int(sc.descriptor.desc.num_nodes),
                max_dist=1.5 * float(np.sqrt(sum(c * c for c in cell))), near_dist=0.2 * min(cell), cell=cell)


def _shared_fns(sc, a):
    import nrays_amd as nr
    return {"gather_maps_points": lambda: nr.gather_maps_points(sc, a["pos"], a["nz"], a["tl"], a["maps"], a["node_map"], None, 0.0, want_counts=True),
            "probe_depth": lambda: nr.probe_depth(sc, a["pos"], a["tl"], RES, a["max_dist"], a["near_dist"])}


def _run(fns, reps, rounds):
    ms = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            ms[name].append(_time(fn, reps, warmup=1))
    return {name: _stats(v) for name, v in ms.items()}


def _row(sc, lo, hi, counts, k, reps, rounds, shared_only):
    import nrays_amd as nr
    a = _inputs(sc, lo, hi, counts, k)
    n = a["pos"].shape[0]
    fns = _shared_fns(sc, a)
    if shared_only:
        return _run(fns, reps, rounds)
    depth = dict(res=RES, max_dist=a["max_dist"], near_dist=a["near_dist"])
    ro = a["pos"][:, None, :].expand(n, k, 3).reshape(n * k, 3).contiguous()
    rd = a["tl"][None, :, :].expand(n, k, 3).reshape(n * k, 3).contiguous()
    fns.update({"fused_with_depth": lambda: nr.gather_maps_probes(sc, a["pos"], a["tl"], a["maps"], a["node_map"], 3, depth=depth),
                "fused_without_depth": lambda: nr.gather_maps_probes(sc, a["pos"], a["tl"], a["maps"], a["node_map"], 3),
                "closest_hits": lambda: nr.closest_hits(sc, ro, rd, want=("uv", "flags")),
                "gather_probes_depth_0": lambda: nr.gather_probes(sc, a["pos"], a["tl"], 3, max_depth=0)})
    got = fns["fused_with_depth"]()
    want = fns["probe_depth"]()
    row = {"probes": int(n), "lattice": list(counts), "dirs": int(k), "rays": int(n * k), "res": RES, "bands": 3, "max_dist": round(a["max_dist"], 4), "rounds": rounds, "reps": reps,
           "mapped_share": round(float(got.counts[:, 0].sum().item()) / (n * k), 4), "missed_share": round(float(got.counts[:, 1].sum().item()) / (n * k), 4),
           "depth_outputs_equal_probe_depth": bool(all(bool((x == y).all().item()) for x, y in zip(got.depth, want)))}
    row.update(_run(fns, reps, rounds))
    med = lambda name: row[name]["ms"]  # noqa: E731
    row["depthless_plus_probe_depth_ms"] = round(med("fused_without_depth") + med("probe_depth"), 4)
    row["ns_per_ray_fused_with_depth"] = round(med("fused_with_depth") * 1e6 / (n * k), 4)
    row["expectation_a"] = "MET" if med("fused_with_depth") < med("fused_without_depth") + med("probe_depth") else "MISSED"
    row["expectation_b"] = "MET" if med("fused_without_depth") <= med("probe_depth") and med("fused_without_depth") < med("gather_probes_depth_0") else "MISSED"
    return row


def _setup(quick):
    import torch
    from tools import standins
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    w, h = (320, 180) if quick else (1920, 1080)
    sc, cam = standins.sponza_scene()
    sc.device_handle()
    p = _hit_inputs(sc, cam, w, h)["points"]
    return sc, p.min(dim=0).values.cpu().numpy(), p.max(dim=0).values.cpu().numpy(), (w, h)


def _shapes(quick, reps):
    """(lattice, directions, reps): 4 096 x 1 024 and 16 384 x 64."""
    return (((8, 4, 8), 64, reps), ((8, 8, 8), 16, reps)) if quick else (((16, 16, 16), 1024, max(1, reps // 2)), ((32, 16, 32), 64, reps * 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gather_maps_sh_rate.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libnrays_hip.so built from the parent commit: its gather_maps_points and probe_depth are timed in a child process")
    ap.add_argument("--shared-only", action="store_true", help="(the child process) time the calls the parent library has and print them as one JSON line")
    ap.add_argument("--quick", action="store_true", help="320x180 first hits and small lattices (a rehearsal of the tool, not a measurement)")
    args = ap.parse_args()
    sc, lo, hi, (w, h) = _setup(args.quick)
    shapes = _shapes(args.quick, args.reps)
    name_of = lambda counts, k: "probes_%d_dirs_%d" % (np.prod(counts), k)  # noqa: E731
    if args.shared_only:
        print("SHARED_ROWS " + json.dumps({name_of(c, k): _row(sc, lo, hi, c, k, reps, args.rounds, True) for c, k, reps in shapes}))
        return
    import torch
    out = {"device": torch.cuda.get_device_name(0), "scene": "sponza stand-in, one shared %d x %d map" % (MAP_SIDE, MAP_SIDE), "resolution": [w, h], "expectation": EXPECTATION}
    for c, k, reps in shapes:
        out[name_of(c, k)] = _row(sc, lo, hi, c, k, reps, args.rounds, False)
    verdicts = [out[name_of(c, k)][e] for c, k, _ in shapes for e in ("expectation_a", "expectation_b")]
    if args.parent_lib:
        env = dict(os.environ, NRAYS_HIP_LIB=os.path.abspath(args.parent_lib))
        cmd = [sys.executable, os.path.abspath(__file__), "--shared-only", "--reps", str(args.reps), "--rounds", str(args.rounds)] + (["--quick"] if args.quick else [])
        text = subprocess.check_output(cmd, env=env, timeout=600).decode()
        parent = json.loads([ln for ln in text.splitlines() if ln.startswith("SHARED_ROWS ")][-1][len("SHARED_ROWS "):])
        for c, k, _ in shapes:
            row, theirs = out[name_of(c, k)], parent[name_of(c, k)]
            row["parent_library"], row["expectation_c"] = theirs, {}
            for name in SHARED_ROWS:
                spread = max(row[name]["max_ms"] - row[name]["min_ms"], theirs[name]["max_ms"] - theirs[name]["min_ms"])
                row["expectation_c"][name] = {"ms": row[name]["ms"], "parent_ms": theirs[name]["ms"], "spread_ms": round(spread, 4),
                                              "verdict": "MET" if abs(row[name]["ms"] - theirs[name]["ms"]) <= spread else "MISSED"}
                verdicts.append(row["expectation_c"][name]["verdict"])
    else:
        out["parent_library"] = "not measured (no --parent-lib)"
    out["met"], out["missed"] = verdicts.count("MET"), verdicts.count("MISSED")
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
