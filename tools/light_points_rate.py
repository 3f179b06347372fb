#!/usr/bin/env python
"""Rate of light_points() (nrays_light_points_device: per point the shadow rays towards a caller-supplied table of point lights, built, weighted, traced and summed on
the device) on the sponza stand-in: the first hits of its 1080p camera rays (about 2 M points) against 16 lights spread through the hall, and 16 384 of those hits
against 256 virtual point lights made by vpls_from_hits().  Beside it, in the same run on the same points: intersects_rays() alone on the n x m rays of the definition
handed over as arrays (skipped pairs included: a caller without the fused call traces them), and the parts a caller has today — a torch ray build, intersects_rays(),
a torch weight and fold.  Every leg with and without emitter normals.  All legs are interleaved in one process: every figure is the median of `rounds` timings of
`reps` back-to-back calls between two events on one stream, reported with its spread.

The expectations are written into the output file BEFORE the first timing; the finished file reports MET or MISSED beside the measured values:

  python tools/light_points_rate.py [--out profiles/light_points_rate.json] [--reps 5] [--quick]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.irradiance_rate import _hit_inputs  # noqa: E402
from tools.trace_rays_rate import _time  # noqa: E402

EXPECTATION = {
    "a": "the fused call is no dearer than intersects_rays alone on the same n x m rays handed over as arrays (the definition's rays, skipped pairs included): it "
         "traces fewer rays and reads 52 bytes a point instead of 56 a ray",
    "b": "the fused call is cheaper than the parts a caller has today, timed as one sequence: a torch ray build, intersects_rays, a torch weight and fold",
    "c": "no threshold: with emitter normals the time falls roughly with the share of pairs that get a ray; both shares and both times are reported"}


def unit_normals(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.sqrt((v * v).sum(axis=1))[:, None]


def _torch_rays(p, nm, pos, en, falloff, min_dist, bias, offset):
    """The rays and weights of the definition as a caller writes them with torch (n x m rows; not meant to match bit for bit)."""
    import torch
    q = (p + nm * bias)[:, None, :]
    v = pos[None, :, :] - q
    nrm = torch.sqrt((v * v).sum(dim=2))
    ldir = v / nrm[..., None]
    w = (ldir * nm[:, None, :]).sum(dim=2).float().clamp(min=0.0)
    if en is not None:
        w = w * (-(ldir * en[None, :, :]).sum(dim=2)).float().clamp(min=0.0)
    if falloff:
        w = w * (1.0 / torch.clamp(nrm * nrm, min=min_dist * min_dist)).float()
    return (q + ldir * offset).reshape(-1, 3), ldir.reshape(-1, 3), (nrm - offset).reshape(-1), w


def _torch_fold(col, w, lit, filt):
    """sum over the lights of col * (filter * w) where the ray got through and has a weight."""
    import torch
    n, m = w.shape
    c = col[None, :, :] * (filt.reshape(n, m, 3) * w[..., None])
    return torch.where((lit.reshape(n, m) & (w > 0))[..., None], c, torch.zeros_like(c)).sum(dim=1)


def _case(sc, inp, lights, reps, rounds):
    import torch
    import nrays_amd as nr
    p, nm, flags = inp["points"], inp["normals"], inp["flags"]
    n, m = int(p.shape[0]), int(lights.positions.shape[0])
    row = {"points": n, "lights": m, "pairs": n * m, "rounds": rounds, "reps": reps}
    for label, L in (("all_ways", lights._replace(normals=None)), ("emitter_normals", lights)):
        pos, col, en = L.positions, L.colors, L.normals
        args = (L.inverse_square, L.min_dist, L.bias, L.offset)
        ro, rd, tm, w = _torch_rays(p, nm, pos, en, *args)
        lit0, filt0 = nr.intersects_rays(sc, ro, rd, tm)

        def parts():
            o, d, t, ww = _torch_rays(p, nm, pos, en, *args)
            lit, filt = nr.intersects_rays(sc, o, d, t)
            return _torch_fold(col, ww, lit, filt)
        fns = {"light_points": lambda: nr.light_points(sc, p, nm, L, hit_flags=flags),
               "intersects_rays_alone": lambda: nr.intersects_rays(sc, ro, rd, tm),
               "torch_ray_build": lambda: _torch_rays(p, nm, pos, en, *args),
               "torch_weight_and_fold": lambda: _torch_fold(col, w, lit0, filt0),
               "parts_in_sequence": parts}
        ms = {name: [] for name in fns}
        for _ in range(rounds):
            for name, fn in fns.items():
                ms[name].append(_time(fn, reps, warmup=1))
        leg = {name: {"ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for name, v in ms.items()}
        counts = nr.light_points(sc, p, nm, L, hit_flags=flags).counts.long().sum(dim=0)
        fused = nr.light_points(sc, p, nm, L, hit_flags=flags).rgb
        leg["share_of_pairs_with_a_ray"] = round(float(counts[0]) / (n * m), 4)
        leg["share_of_pairs_open"] = round(float(counts[1]) / (n * m), 4)
        leg["max_abs_difference_to_the_torch_parts"] = float((fused - parts()).abs().max())
        med = lambda name: leg[name]["ms"]  # noqa: E731
        leg["light_points"]["mrays_with_a_ray_per_s"] = round(float(counts[0]) / med("light_points") / 1e3, 1)
        leg["light_points"]["expectation_a"] = "MET" if med("light_points") <= med("intersects_rays_alone") else "MISSED"
        leg["light_points"]["expectation_b"] = "MET" if med("light_points") < med("parts_in_sequence") else "MISSED"
        row[label] = leg
        del ro, rd, tm, w, lit0, filt0
        torch.cuda.empty_cache()
    a, e = row["all_ways"], row["emitter_normals"]
    row["expectation_c"] = {"time_ratio_emitters_to_all_ways": round(e["light_points"]["ms"] / a["light_points"]["ms"], 4),
                            "ray_share_ratio_emitters_to_all_ways": round(e["share_of_pairs_with_a_ray"] / a["share_of_pairs_with_a_ray"], 4)}
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "light_points_rate.json"))
    ap.add_argument("--reps", type=int, default=5)
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
    import nrays_amd as nr
    from tools import standins
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    w, h = (320, 180) if args.quick else (1920, 1080)
    sc, cam = standins.sponza_scene()
    sc.device_handle()
    inp = _hit_inputs(sc, cam, w, h)
    n = inp["points"].shape[0]
    rng = np.random.default_rng(17)
    lo, hi = inp["points"].min(dim=0).values.cpu().numpy(), inp["points"].max(dim=0).values.cpu().numpy()
    # 16 lights spread through the hall: a jittered 4 x 2 x 2 lattice inside the box of the visible surface
    cells = np.stack(np.meshgrid(np.arange(4), np.arange(2), np.arange(2), indexing="ij"), axis=-1).reshape(-1, 3)
    pos = lo + (hi - lo) * (0.15 + 0.7 * (cells + rng.uniform(0.25, 0.75, size=cells.shape)) / np.asarray([4.0, 2.0, 2.0]))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    hall = nr.PointLights(up(pos), up(rng.uniform(0.2, 1.0, size=(16, 3)).astype(np.float32)), up(unit_normals(rng, 16)), True, 0.1, 1e-3, 1e-3)
    # 256 virtual point lights: the first hits of rays leaving the first light in every direction
    d = torch.from_numpy(unit_normals(rng, 640)).cuda()
    o = up(np.tile(pos[0], (640, 1)))
    hits = nr.closest_hits(sc, o, d)
    vpls = nr.vpls_from_hits(o, d, hits, nr.material_hits(sc, hits, want=("diffuse",)).diffuse, 1.0 / 256.0, inverse_square=True, min_dist=0.1)
    vpls = vpls._replace(positions=vpls.positions[:256].contiguous(), colors=vpls.colors[:256].contiguous(), normals=vpls.normals[:256].contiguous())
    assert vpls.positions.shape[0] == 256, "fewer than 256 of 640 rays from the light hit the hall"
    sub = torch.from_numpy(np.linspace(0, n - 1, min(16384, n)).astype(np.int64)).cuda()
    subset = {k: v[sub].contiguous() for k, v in inp.items()}
    del out["status"]
    out.update({"device": torch.cuda.get_device_name(0), "scene": "sponza stand-in, first hits of the camera rays", "resolution": [w, h]})
    out["hits_x_16_lights"] = _case(sc, inp, hall, args.reps, args.rounds)
    write()
    out["16384_hits_x_256_vpls"] = _case(sc, subset, vpls, args.reps * 4, args.rounds)
    verdicts = [leg["light_points"][key] for case in (out["hits_x_16_lights"], out["16384_hits_x_256_vpls"]) for leg in (case["all_ways"], case["emitter_normals"])
                for key in ("expectation_a", "expectation_b")]
    out["met"], out["missed"] = verdicts.count("MET"), verdicts.count("MISSED")
    write()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
