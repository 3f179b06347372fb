#!/usr/bin/env python
"""Rate of nearest_points() (nrays_nearest_points_device: per point the nearest surface of the scene, by a distance-pruned walk of both BVH levels) on the sponza
stand-in, beside closest_hits() on as many rays from the same points and beside the same query written with torch over all triangles in chunks.  Inputs: the first
hits of the 1080p camera rays (about 2 M) pushed 0.25 of a probe cell along their normals, with max_dist of one cell and unbounded; the positions of a 32 x 16 x 32
probe lattice over the scene's box; 16 384 of the hits.  All calls are interleaved in one process: every figure is the median of `rounds` timings of `reps`
back-to-back calls between two events on one stream, reported with its spread.

The expectations are written into the output file BEFORE the first timing; the finished file reports MET or MISSED beside the measured values:

  python tools/nearest_rate.py [--out profiles/nearest_rate.json] [--reps 5] [--quick]
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
    "a": "nearest_points on 16 384 points is cheaper than the same query written with torch over all triangles in chunks (every point against every triangle, float64)",
    "b": "nearest_points with max_dist of one probe cell costs no more than closest_hits on as many rays from the same points (towards the surface they came from): the "
         "bound keeps the walk as local as a short ray's",
    "c": "no threshold: the share of the walk's node fetches that were stale (popped after the bound had shrunk below their box) would need an instrumented build; "
         "it is reported as not counted unless one exists"}
GRID = (32, 16, 32)


def _world_triangles(sc):
    """Every triangle of the scene in world space, (m, 3, 3) float64 on the device (the stand-in's nodes do not move)."""
    import torch
    tris = []
    for nd in sc._nodes:
        g = nd.geometry
        assert nd.transform.axis_angle == (0.0, 0.0, 0.0) and nd.transform.translation == (0.0, 0.0, 0.0)
        tris.append(np.asarray(g.points, np.float64)[np.asarray(g.indices, np.int64)])
    return torch.from_numpy(np.concatenate(tris)).cuda()


def _torch_nearest(p, tris, chunk=1024):
    """The squared distance from every point to its nearest triangle as a caller wrote it with torch: the three clamped edge projections and the plane projection where it
    falls inside, every point against every triangle, `chunk` triangles at a time."""
    import torch
    best = torch.full((p.shape[0],), float("inf"), dtype=torch.float64, device=p.device)
    P = p[:, None, :]
    dot = lambda a, b: (a * b).sum(dim=-1)  # noqa: E731
    for t0 in range(0, tris.shape[0], chunk):
        a, b, c = (tris[None, t0:t0 + chunk, k, :] for k in range(3))
        d2 = None
        for u, v in ((a, b), (b, c), (c, a)):
            e, w = v - u, P - u
            t = (dot(e, w) / dot(e, e).clamp(min=1e-300)).clamp(0.0, 1.0)
            r = w - e * t[..., None]
            k = dot(r, r)
            d2 = k if d2 is None else torch.minimum(d2, k)
        ab, ac, ap = b - a, c - a, P - a
        n = torch.linalg.cross(ab, ac)
        nn = dot(n, n).clamp(min=1e-300)
        d00, d01, d11, d20, d21 = dot(ab, ab), dot(ab, ac), dot(ac, ac), dot(ap, ab), dot(ap, ac)
        den = d00 * d11 - d01 * d01
        v, w = (d11 * d20 - d01 * d21) / den, (d00 * d21 - d01 * d20) / den
        inside = (v >= 0) & (w >= 0) & (v + w <= 1)
        plane = dot(ap, n) ** 2 / nn
        d2 = torch.where(inside, torch.minimum(d2, plane), d2)
        best = torch.minimum(best, d2.min(dim=1).values)
    return best


def _stats(v):
    return {"ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nearest_rate.json"))
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
    hits, nm = inp["points"], inp["normals"]
    lo, hi = hits.min(dim=0).values, hits.max(dim=0).values
    cell = ((hi - lo) / (torch.tensor(GRID, dtype=torch.float64, device=hits.device) - 1)).cpu().numpy()
    step = float(cell.max())
    pushed = (hits + nm * (0.25 * step)).contiguous()
    back = (-nm).contiguous()
    n = pushed.shape[0]
    md = torch.full((n,), step, dtype=torch.float64, device=hits.device)
    lattice = torch.from_numpy(nr.probe_grid_positions(tuple(lo.cpu().numpy()), tuple(cell), GRID)).cuda()
    sub = torch.from_numpy(np.linspace(0, n - 1, min(16384, n)).astype(np.int64)).cuda()
    p16, b16, md16 = pushed[sub].contiguous(), back[sub].contiguous(), md[sub].contiguous()
    tris = _world_triangles(sc)
    # what is timed is also checked once: the bounded answer is the unbounded one or a miss, and the torch form finds the same distances
    full, bounded = nr.nearest_points(sc, p16), nr.nearest_points(sc, p16, md16)
    found = bounded.node >= 0
    assert torch.equal(bounded.dist[found], full.dist[found]) and bool((full.dist[~found] > step).all())
    ref = _torch_nearest(p16, tris).sqrt()
    worst = float((ref - full.dist).abs().max())
    assert worst <= 1e-9 * float(hi.abs().max()), worst
    fns = {
        "nearest_bounded_hits": lambda: nr.nearest_points(sc, pushed, md),
        "nearest_unbounded_hits": lambda: nr.nearest_points(sc, pushed),
        "nearest_dist_node_only_bounded": lambda: nr.nearest_points(sc, pushed, md, want=()),
        "closest_hits_same_points": lambda: nr.closest_hits(sc, pushed, back),
        "nearest_lattice": lambda: nr.nearest_points(sc, lattice),
        "closest_hits_lattice": lambda: nr.closest_hits(sc, lattice, back[:lattice.shape[0]].contiguous()),
        "nearest_bounded_16384": lambda: nr.nearest_points(sc, p16, md16),
        "nearest_unbounded_16384": lambda: nr.nearest_points(sc, p16),
        "closest_hits_16384": lambda: nr.closest_hits(sc, p16, b16),
    }
    ms = {name: [] for name in fns}
    torch_ms = []
    for _ in range(args.rounds):
        for name, fn in fns.items():
            ms[name].append(_time(fn, args.reps, warmup=1))
        torch_ms.append(_time(lambda: _torch_nearest(p16, tris), 1, warmup=0))
    del out["status"]
    out.update({"device": torch.cuda.get_device_name(0), "scene": "sponza stand-in, %d triangles" % tris.shape[0], "resolution": [w, h], "points": int(n), "lattice": list(GRID),
                "probe_cell": round(step, 4), "rounds": args.rounds, "reps": args.reps, "found_within_a_cell": round(float(found.double().mean()), 4),
                "torch_form_max_abs_difference": worst})
    for name, v in ms.items():
        out[name] = _stats(v)
        out[name]["mpoints_per_s"] = round((lattice.shape[0] if "lattice" in name else 16384 if "16384" in name else n) / out[name]["ms"] / 1e3, 1)
    out["torch_all_triangles_16384"] = _stats(torch_ms)
    out["expectation_a"] = "MET" if out["nearest_unbounded_16384"]["ms"] < out["torch_all_triangles_16384"]["ms"] else "MISSED"
    out["expectation_b"] = "MET" if out["nearest_bounded_hits"]["ms"] <= out["closest_hits_same_points"]["ms"] else "MISSED"
    out["expectation_b_16384"] = "MET" if out["nearest_bounded_16384"]["ms"] <= out["closest_hits_16384"]["ms"] else "MISSED"
    out["expectation_c"] = "not counted: no instrumented build of k_nearest_points exists"
    write()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
