#!/usr/bin/env python
"""Rates of the probe-visibility pair on the sponza stand-in.

(a) probe_depth() (nrays_probe_depth_points_device: sphere rays built in registers, the closest-hit query, 4 bytes a ray kept for a per-texel fold) for 4 096 probes x
    1 024 directions and 16 384 probes x 64 directions at R = 8, on lattices over the bounding box of the camera's first hits, beside the parts a caller had before:
    building the rays with torch, closest_hits() on them given as arrays (toi and flags only), and a torch scatter-fold (index_add_ of r, r^2 and 1 per texel).
(b) irradiance_points(visibility=) (nrays_irradiance_points_vis_device) at the first hits of the 1080p camera rays against a 32 x 16 x 32 grid, beside the call
    without visibility, with the facing factor, with out_sh, with both, and — with --parent-lib, in a child process under NRAYS_HIP_LIB — beside irradiance_points of a
    library built from the parent commit on the same points.
(c) the rows without visibility beside the committed profiles/irradiance_rate.json (surface_order_small_32x16x32), which the parent's kernel wrote.
Every figure is the median of `rounds` timings of `reps` back-to-back calls between two events on one stream.

The expectations were written before the first run; the JSON reports MET or MISSED beside the measured values:

  python tools/probe_depth_rate.py [--out profiles/probe_depth_rate.json] [--reps 10] [--parent-lib PATH] [--quick]
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
    "a": "probe_depth is no dearer than closest_hits (toi, flags) alone on the same rays given as arrays, in both rows: the traversal is the same device code on the "
         "same rays in the same lanes (64 lanes a probe = consecutive rays of an array), the fused call reads 48 bytes a PROBE instead of 48 bytes a RAY, stores 4 bytes a "
         "ray instead of 16, and its fold walks 4 bytes a ray out of the L2 / Infinity Cache; its registers (203 - 210 against k_cast_rays' 182 - 195) leave the "
         "occupancy at 2 waves a SIMD",
    "b": "visibility costs less over the plain call than the facing factor and out_sh together do: per corner one 8-byte load from a 16 MiB table and a dozen f32 "
         "operations behind an f64 octahedral projection, against a square root and a division per corner plus 108 more bytes stored a point",
    "c": "the rows without visibility equal profiles/irradiance_rate.json (surface_order_small_32x16x32, written by the parent's kernel) within that file's own "
         "run-to-run spread (its max_ms - min_ms of the row, around its median): the VIS = false permutations have the parent's registers row for row "
         "(profiles/probe_depth_kres.txt)"}
RES = 8
GRID = (32, 16, 32)
PLAIN_ROWS = {"plain": dict(), "out_sh": dict(want_sh=True), "flags": dict(flags=True), "facing": dict(facing=True), "facing_out_sh": dict(facing=True, want_sh=True)}
FILE_ROWS = {"plain": "bands_3", "out_sh": "bands_3_out_sh", "flags": "bands_3_flags"}  # the rows profiles/irradiance_rate.json has


def _stats(v):
    return {"ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def _torch_texel(d, R):
    """oct_texel() with torch on the device (f64, the header's operations)."""
    import torch
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    s = (x.abs() + y.abs()) + z.abs()
    some = s > 0
    den = torch.where(some, s, torch.ones_like(s))
    a, b = torch.where(some, x / den, torch.zeros_like(x)), torch.where(some, y / den, torch.zeros_like(y))
    one = torch.ones_like(a)
    a2 = torch.where(z < 0, (1.0 - b.abs()) * torch.copysign(one, a), a)
    b2 = torch.where(z < 0, (1.0 - a.abs()) * torch.copysign(one, b), b)
    tx = ((a2 * 0.5 + 0.5) * R).clamp(min=0.0).long().clamp(max=R - 1)
    ty = ((b2 * 0.5 + 0.5) * R).clamp(min=0.0).long().clamp(max=R - 1)
    return ty * R + tx


def _torch_fold(rd, toi, flags, n, k, R, max_dist):
    """What a caller did with torch after closest_hits: distances, clamp, texels, and a scatter of r, r^2 and 1 per (probe, texel) — index_add_, in no fixed order."""
    import torch
    L = torch.sqrt((rd[:, 0] * rd[:, 0] + rd[:, 1] * rd[:, 1]) + rd[:, 2] * rd[:, 2])
    dist = torch.where((flags & 1) != 0, toi * L, torch.full_like(toi, float("inf")))
    r = dist.clamp(max=max_dist).float()
    at = _torch_texel(rd, R) + torch.arange(n, device=rd.device).repeat_interleave(k) * (R * R)
    s1 = torch.zeros(n * R * R, dtype=torch.float32, device=rd.device).index_add_(0, at, r)
    s2 = torch.zeros_like(s1).index_add_(0, at, r * r)
    cnt = torch.zeros_like(s1).index_add_(0, at, torch.ones_like(r))
    some = cnt > 0
    return torch.stack([torch.where(some, s1 / cnt.clamp(min=1.0), torch.full_like(s1, max_dist)), torch.where(some, s2 / cnt.clamp(min=1.0), torch.full_like(s1, max_dist * max_dist))],
                       dim=1).view(n, R * R, 2)


def _torch_build_rays(pos, tl):
    n, k = pos.shape[0], tl.shape[0]
    return pos[:, None, :].expand(n, k, 3).reshape(n * k, 3).contiguous(), tl[None, :, :].expand(n, k, 3).reshape(n * k, 3).contiguous()


def _depth_row(sc, lo, hi, counts, k, reps, rounds):
    import torch
    import nrays_amd as nr
    cell = tuple(float(x) for x in (hi - lo) / (np.asarray(counts) + 1))
    origin = tuple(float(x) for x in lo + np.asarray(cell))  # the lattice strictly inside the box
    pos = torch.from_numpy(nr.probe_grid_positions(origin, cell, counts)).cuda()
    n = pos.shape[0]
    max_dist = 1.5 * float(np.sqrt(sum(c * c for c in cell)))
    tl = torch.from_numpy(nr.sphere_dirs(k)).cuda()
    ro, rd = _torch_build_rays(pos, tl)
    hits = nr.closest_hits(sc, ro, rd, want=("flags",))
    fns = {"fused": lambda: nr.probe_depth(sc, pos, tl, RES, max_dist, 0.2 * min(cell)),
           "fused_moments_only": lambda: nr.probe_depth(sc, pos, tl, RES, max_dist, 0.0, want=()),
           "closest_hits": lambda: nr.closest_hits(sc, ro, rd, want=("flags",)),
           "torch_build_rays": lambda: _torch_build_rays(pos, tl),
           "torch_scatter_fold": lambda: _torch_fold(rd, hits.toi, hits.flags, n, k, RES, max_dist)}
    ms = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            ms[name].append(_time(fn, reps, warmup=1))
    got = nr.probe_depth(sc, pos, tl, RES, max_dist, 0.2 * min(cell))
    want = _torch_fold(rd, hits.toi, hits.flags, n, k, RES, max_dist)
    row = {"probes": int(n), "lattice": list(counts), "dirs": int(k), "rays": int(n * k), "res": RES, "max_dist": round(max_dist, 4), "rounds": rounds, "reps": reps,
           "missed_share": round(float(got.counts[:, 1].sum().item()) / (n * k), 4), "near_share": round(float(got.counts[:, 0].sum().item()) / (n * k), 4),
           "max_abs_difference_from_the_torch_scatter": float((got.moments - want).abs().max().item())}
    for name, v in ms.items():
        row[name] = _stats(v)
    med = lambda name: row[name]["ms"]  # noqa: E731
    row["parts_with_torch_ms"] = round(med("torch_build_rays") + med("closest_hits") + med("torch_scatter_fold"), 4)
    row["ns_per_ray_fused"] = round(med("fused") * 1e6 / (n * k), 4)
    row["expectation_a"] = "MET" if med("fused") <= med("closest_hits") else "MISSED"
    return row


def _grid_for(p, rng_seed=3):
    import torch
    import nrays_amd as nr
    lo, hi = p.min(dim=0).values.cpu().numpy(), p.max(dim=0).values.cpu().numpy()
    origin, cell = tuple(float(x) for x in lo), tuple(float(x) for x in (hi - lo) / (np.asarray(GRID) - 1))
    P = GRID[0] * GRID[1] * GRID[2]
    sh = torch.from_numpy(np.random.default_rng(rng_seed).uniform(0.0, 1.0, size=(P, 9, 3)).astype(np.float32)).cuda()
    return nr.ProbeGrid(origin, cell, GRID, sh), P, cell


def _plain_rows(sc, inp, reps, rounds):
    """The calls every library has (no visibility), on the first hits: {row: stats}."""
    import nrays_amd as nr
    p, nm = inp["points"], inp["normals"]
    grid, _, _ = _grid_for(p)
    fns = {name: (lambda kw=kw: nr.irradiance_points(sc, p, nm, grid, facing=kw.get("facing", False), hit_flags=inp["flags"] if kw.get("flags") else None,
                                                     want_sh=kw.get("want_sh", False))) for name, kw in PLAIN_ROWS.items()}
    ms = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            ms[name].append(_time(fn, reps, warmup=1))
    return {name: _stats(v) for name, v in ms.items()}


def _vis_rows(sc, inp, reps, rounds):
    import torch
    import nrays_amd as nr
    p, nm = inp["points"], inp["normals"]
    grid, P, cell = _grid_for(p)
    rng = np.random.default_rng(5)  # synthetic moments around the cell size: the factor is live for a share of the corners, as behind real walls
    m1 = rng.uniform(0.2, 1.5, size=(P, RES * RES)).astype(np.float32) * np.float32(min(cell))
    m2 = m1 * m1 * rng.uniform(1.0, 1.3, size=m1.shape).astype(np.float32)
    vis = nr.ProbeVisibility(torch.from_numpy(np.stack([m1, m2], axis=2)).cuda(), RES, 0.05, 0.0)
    fns = {"vis": lambda: nr.irradiance_points(sc, p, nm, grid, visibility=vis),
           "vis_facing": lambda: nr.irradiance_points(sc, p, nm, grid, facing=True, visibility=vis),
           "vis_facing_out_sh": lambda: nr.irradiance_points(sc, p, nm, grid, facing=True, want_sh=True, visibility=vis)}
    ms = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            ms[name].append(_time(fn, reps, warmup=1))
    held = nr.irradiance_points(sc, p, nm, grid, visibility=vis, want_weight=True).weight
    plain = nr.irradiance_points(sc, p, nm, grid, want_weight=True).weight
    rows = {name: _stats(v) for name, v in ms.items()}
    rows["share_of_points_whose_weight_the_factor_changed"] = round(float((held != plain).float().mean().item()), 4)
    return rows


def _setup(quick):
    import torch
    from tools import standins
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    w, h = (320, 180) if quick else (1920, 1080)
    sc, cam = standins.sponza_scene()
    sc.device_handle()
    return sc, _hit_inputs(sc, cam, w, h), (w, h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "probe_depth_rate.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None, help="libnrays_hip.so built from the parent commit: its irradiance_points is timed in a child process on the same points")
    ap.add_argument("--plain-only", action="store_true", help="(the child process) time the calls without visibility and print them as one JSON line")
    ap.add_argument("--quick", action="store_true", help="320x180 instead of 1920x1080 and small lattices (a rehearsal of the tool, not a measurement)")
    args = ap.parse_args()
    sc, inp, (w, h) = _setup(args.quick)
    if args.plain_only:
        print("PLAIN_ROWS " + json.dumps(_plain_rows(sc, inp, args.reps, args.rounds)))
        return
    import torch
    p = inp["points"]
    lo, hi = p.min(dim=0).values.cpu().numpy(), p.max(dim=0).values.cpu().numpy()
    out = {"device": torch.cuda.get_device_name(0), "scene": "sponza stand-in", "resolution": [w, h], "expectation": EXPECTATION}
    shapes = (((8, 4, 8), 64), ((8, 8, 8), 16)) if args.quick else (((16, 16, 16), 1024), ((32, 16, 32), 64))
    out["probes_%d_dirs_%d" % (np.prod(shapes[0][0]), shapes[0][1])] = _depth_row(sc, lo, hi, shapes[0][0], shapes[0][1], max(1, args.reps // 2), args.rounds)
    out["probes_%d_dirs_%d" % (np.prod(shapes[1][0]), shapes[1][1])] = _depth_row(sc, lo, hi, shapes[1][0], shapes[1][1], args.reps * 2, args.rounds)
    irr = {"points": int(p.shape[0]), "grid": list(GRID), "res": RES, "rounds": args.rounds, "reps": args.reps}
    irr.update(_plain_rows(sc, inp, args.reps, args.rounds))
    irr.update(_vis_rows(sc, inp, args.reps, args.rounds))
    med = lambda name: irr[name]["ms"]  # noqa: E731
    irr["visibility_over_plain_ms"] = round(med("vis") - med("plain"), 4)
    irr["facing_and_out_sh_over_plain_ms"] = round(med("facing_out_sh") - med("plain"), 4)
    irr["expectation_b"] = "MET" if med("vis") - med("plain") < med("facing_out_sh") - med("plain") else "MISSED"
    if args.parent_lib:
        env = dict(os.environ, NRAYS_HIP_LIB=os.path.abspath(args.parent_lib))
        cmd = [sys.executable, os.path.abspath(__file__), "--plain-only", "--reps", str(args.reps), "--rounds", str(args.rounds)] + (["--quick"] if args.quick else [])
        text = subprocess.check_output(cmd, env=env, timeout=600).decode()
        irr["parent_library"] = json.loads([ln for ln in text.splitlines() if ln.startswith("PLAIN_ROWS ")][-1][len("PLAIN_ROWS "):])
        irr["plain_over_parent_library"] = {name: round(med(name) / irr["parent_library"][name]["ms"], 4) for name in PLAIN_ROWS}
    else:
        irr["parent_library"] = "not measured (no --parent-lib)"
    committed = os.path.join(ROOT, "profiles", "irradiance_rate.json")
    if os.path.exists(committed) and not args.quick:
        ref = json.load(open(committed))["surface_order_small_32x16x32"]
        irr["expectation_c"] = {}
        for name, theirs in FILE_ROWS.items():
            r = ref[theirs]
            spread = r["max_ms"] - r["min_ms"]
            irr["expectation_c"][name] = {"file_ms": r["ms"], "file_spread_ms": round(spread, 4), "ms": med(name),
                                          "verdict": "MET" if abs(med(name) - r["ms"]) <= spread else "MISSED"}
    out["irradiance_first_hits"] = irr
    verdicts = [out[k]["expectation_a"] for k in out if k.startswith("probes_")] + [irr["expectation_b"]] + [v["verdict"] for v in irr.get("expectation_c", {}).values()]
    out["met"], out["missed"] = verdicts.count("MET"), verdicts.count("MISSED")
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
