#!/usr/bin/env python
"""Rate of irradiance_points() (nrays_irradiance_points_device: per point the eight probes around it blended, folded with the cosine lobe at the normal) on the
first hits of the sponza stand-in's 1080p camera rays (about 2 M points), beside the same lookup written with torch ops on the same tensors — index_select of the
eight corners, the weights and the folds — and beside shade_points() on the same points.  Grids over the points' bounding box: 32 x 16 x 32 probes (1.7 MB of
coefficients at 3 bands: L2-resident) and 128 x 64 x 128 (113 MB: beyond the L2).  Points in surface order (the camera's scan order) and shuffled; and 16 384 of
them.  Every row with 3 bands and with 1 band, with and without out_sh.  Every figure is the median of `rounds` timings of `reps` back-to-back calls between two
events on one stream; the copy bandwidth of the same run (a device-to-device copy of 1 GiB, read + written bytes) gives the traffic floor.

The expectations were written before the first run; the JSON reports MET or MISSED beside the measured values:

  python tools/irradiance_rate.py [--out profiles/irradiance_rate.json] [--reps 10] [--quick]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.trace_rays_rate import _time  # noqa: E402

EXPECTATION = {
    "a": "every row is cheaper than the same lookup written with torch ops (index_select of the 8 corners plus the weights and the folds, on the same tensors): the "
         "torch form writes and re-reads 8 gathered blocks of 12 C bytes a point and a dozen temporaries, the kernel reads 48 bytes and writes 12 (+ 12 C with out_sh)",
    "b": "the surface-order rows with the small grid are cheaper than shade_points on the same points, measured in the same run: a lookup with no traversal should "
         "undercut direct lighting with shadow rays",
    "c": "no threshold: the fraction of the traffic floor — 60 bytes a point (48 in, 12 out), 4 more where flags are passed — at the run's measured copy bandwidth"}
GRIDS = {"small_32x16x32": (32, 16, 32), "large_128x64x128": (128, 64, 128)}
FLOOR_BYTES = 60


def _hit_inputs(sc, cam, w, h):
    """The first hits of the camera rays as device tensors: points, normals on the camera's side, and what shade_points takes beside them."""
    import torch
    import nrays_amd as nr
    from nrays_amd import math3d
    proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], w, h)
    o, d, _ = nr.camera_rays((w, h), cam["eye"], proj)
    to, td = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    hits = nr.closest_hits(sc, to, td, want=("normal", "uv", "flags"))
    hit = (hits.flags & 1) != 0
    tp = (to + td * hits.toi[:, None])[hit].contiguous()
    nm, view = hits.normal[hit], td[hit].contiguous()
    tn = torch.where((((nm[:, 0] * view[:, 0] + nm[:, 1] * view[:, 1]) + nm[:, 2] * view[:, 2]) > 0)[:, None], -nm, nm).contiguous()
    return dict(points=tp, normals=tn, view=view, nodes=hits.node[hit].contiguous(), uvs=hits.uv[hit].contiguous(), flags=hits.flags[hit].contiguous())


def _torch_lookup(p, nm, origin, cell, counts, sh, measure):
    """The lookup as a caller wrote it with torch: f64 cell coordinates, f32 weights, index_select of the eight corners, the two folds (no facing, every probe valid)."""
    import torch
    from nrays_amd.restated import SH_COSINE_LOBE, _sh_terms
    top = (counts - 1).to(torch.float64)
    g = torch.minimum(((p - origin) / cell).clamp(min=0.0), top)
    i = torch.minimum(g.floor().long(), (counts - 2).clamp(min=0))
    f = (g - i.to(torch.float64)).float()
    hi = torch.minimum(i + 1, counts - 1)
    w, rows = [], []
    for k in range(8):
        d = (k & 1, (k >> 1) & 1, (k >> 2) & 1)
        idx = [hi[:, a] if d[a] else i[:, a] for a in range(3)]
        X, Y, Z = (f[:, a] if d[a] else 1.0 - f[:, a] for a in range(3))
        w.append((X * Y) * Z)
        rows.append((idx[2] * counts[1] + idx[1]) * counts[0] + idx[0])
    wsum = torch.zeros_like(w[0])
    for k in range(8):
        wsum = wsum + w[k]
    s = torch.zeros((p.shape[0],) + tuple(sh.shape[1:]), dtype=torch.float32, device=p.device)
    for k in range(8):
        s = s + (w[k] / wsum)[:, None, None] * sh.index_select(0, rows[k])
    C_ = sh.shape[1]
    Y = _sh_terms(nm[:, 0], nm[:, 1], nm[:, 2], C_)
    band = (0, 1, 1, 1, 2, 2, 2, 2, 2)
    e = torch.zeros((p.shape[0], 3), dtype=torch.float32, device=p.device)
    for c in range(C_):
        e = e + (SH_COSINE_LOBE[band[c]] * Y[c]).float()[:, None] * s[:, c, :]
    return measure * e, s


def _copy_gbs():
    import torch
    a = torch.empty(1 << 28, dtype=torch.float32, device="cuda")
    b = torch.empty_like(a)
    ms = sorted(_time(lambda: b.copy_(a), 5, warmup=2) for _ in range(5))[2]
    return 2.0 * a.numel() * 4 / (ms * 1e-3) / 1e9


def _row(sc, inp, counts, reps, rounds, gbs, with_shade):
    import torch
    import nrays_amd as nr
    p, nm = inp["points"], inp["normals"]
    n = p.shape[0]
    lo, hi = p.min(dim=0).values.cpu().numpy(), p.max(dim=0).values.cpu().numpy()
    origin, cell = tuple(float(x) for x in lo), tuple(float(x) for x in (hi - lo) / (np.asarray(counts) - 1))
    P = counts[0] * counts[1] * counts[2]
    sh3 = torch.from_numpy(np.random.default_rng(3).uniform(0.0, 1.0, size=(P, 9, 3)).astype(np.float32)).cuda()
    t_origin, t_cell, t_counts = (torch.tensor(v, dtype=dt, device="cuda") for v, dt in ((origin, torch.float64), (cell, torch.float64), (counts, torch.int64)))
    row = {"points": int(n), "grid": list(counts), "rounds": rounds, "reps": reps}
    fns = {}
    for bands in (3, 1):
        sh = sh3[:, :bands * bands].contiguous()
        grid = nr.ProbeGrid(origin, cell, counts, sh)
        fns["bands_%d" % bands] = lambda grid=grid: nr.irradiance_points(sc, p, nm, grid)
        fns["bands_%d_out_sh" % bands] = lambda grid=grid: nr.irradiance_points(sc, p, nm, grid, want_sh=True)
        fns["bands_%d_flags" % bands] = lambda grid=grid: nr.irradiance_points(sc, p, nm, grid, hit_flags=inp["flags"])
        fns["torch_bands_%d" % bands] = lambda sh=sh: _torch_lookup(p, nm, t_origin, t_cell, t_counts, sh, 4.0 * math.pi)
        got = nr.irradiance_points(sc, p, nm, grid, want_sh=True)
        want = _torch_lookup(p, nm, t_origin, t_cell, t_counts, sh, 4.0 * math.pi)
        row["bands_%d_max_abs_difference_from_torch" % bands] = float((got.rgb - want[0]).abs().max().item())
        del got, want
    if with_shade:
        fns["shade_points"] = lambda: nr.shade_points(sc, p, nm, inp["view"], inp["nodes"], inp["uvs"], inp["flags"])
    ms = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            ms[name].append(_time(fn, reps, warmup=1))
    for name, v in ms.items():
        row[name] = {"ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    med = lambda name: row[name]["ms"]  # noqa: E731
    floor = lambda bytes_: n * bytes_ / (gbs * 1e9) * 1e3  # noqa: E731  (ms)
    for bands in (3, 1):
        for suffix, extra in (("", 0), ("_out_sh", 12 * bands * bands), ("_flags", 4)):
            name = "bands_%d%s" % (bands, suffix)
            row[name]["expectation_a"] = "MET" if med(name) < med("torch_bands_%d" % bands) else "MISSED"
            row[name]["floor_ms"] = round(floor(FLOOR_BYTES + (4 if suffix == "_flags" else 0)), 4)
            row[name]["fraction_of_floor"] = round(floor(FLOOR_BYTES + (4 if suffix == "_flags" else 0)) / med(name), 4)
            if suffix == "_out_sh":
                row[name]["fraction_of_floor_with_the_sh_store"] = round(floor(FLOOR_BYTES + extra) / med(name), 4)
            if with_shade:
                row[name]["expectation_b"] = "MET" if med(name) < med("shade_points") else "MISSED"
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "irradiance_rate.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="320x180 instead of 1920x1080 (a rehearsal of the tool, not a measurement)")
    args = ap.parse_args()
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
    out = {"device": torch.cuda.get_device_name(0), "scene": "sponza stand-in, first hits of the camera rays", "resolution": [w, h], "expectation": EXPECTATION,
           "copy_bandwidth_gb_s": round(gbs, 1), "floor_bytes_per_point": FLOOR_BYTES}
    for gname, counts in GRIDS.items():
        out["surface_order_" + gname] = _row(sc, inp, counts, args.reps, args.rounds, gbs, gname.startswith("small"))
        out["shuffled_" + gname] = _row(sc, shuffled, counts, args.reps, args.rounds, gbs, False)
        out["subset_16384_" + gname] = _row(sc, subset, counts, args.reps * 4, args.rounds, gbs, False)
    verdicts = [v2[key] for v in out.values() if isinstance(v, dict) for v2 in v.values() if isinstance(v2, dict) for key in ("expectation_a", "expectation_b") if key in v2]
    out["met"], out["missed"] = verdicts.count("MET"), verdicts.count("MISSED")
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
