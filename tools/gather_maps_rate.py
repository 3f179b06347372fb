#!/usr/bin/env python
"""Rate of gather_maps_points() (nrays_gather_maps_points_device: hemisphere rays built in registers, the closest-hit query, a light-map sample at the hit's uv,
one mean colour per point) on the sponza stand-in, beside the parts a caller had before: building the rays with torch, closest_hits() on them given as arrays
(node, uv and flags only), sampling one map and folding with torch — and beside gather_points(max_depth=0), which also shades every hit and traces its shadow rays.
One shared 1024 x 1024 float32 map for every node.  Inputs: the first hits of the 1080p camera rays x 16 directions (about 2 M points, 33 M rays), and 16 384 of
them x 64 directions.  Every figure is the median of `rounds` timings of `reps` back-to-back calls between two events on one stream.

The expectations were written before the first run; the JSON reports MET or MISSED beside the measured values:

  python tools/gather_maps_rate.py [--out profiles/gather_maps_rate.json] [--reps 20] [--quick]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.trace_rays_rate import _first_hit_points, _time, _torch_occlusion_rays  # noqa: E402

EXPECTATION = {
    "a": "gather_maps_points is no dearer than closest_hits (node, uv, flags) alone on the same rays given as arrays, in both rows: the traversal is the same device "
         "code on the same rays in the same lanes (8 or 64 lanes a point = consecutive rays of an array), the fused call reads 56 bytes a POINT instead of 48 bytes "
         "a RAY and stores 12 bytes a point instead of 40 bytes a ray, and adds per mapped ray four 16-byte texel fetches from a 16 MiB map that stays in the L2 / "
         "Infinity Cache, and a shuffle fold; its registers (198 - 203 against 182 - 195) leave the occupancy at 2 waves a SIMD as for k_cast_rays",
    "b": "gather_maps_points is cheaper than gather_points(max_depth=0) on the same points and tables, in both rows: that call runs the same closest-hit query and "
         "then Material::compute at every hit, a shadow ray per light included"}
MAP_SIZE = 1024


def _torch_sample_fold(texels, uv, flags, n, k, miss):
    """What a caller did with torch after closest_hits: Bilinear / ClampToEdges sample of one map at the hits' uv (the header's f32 operations), miss colour at the
    misses, the sequential f32 fold over j and one division."""
    import torch
    h, w = texels.shape[0], texels.shape[1]
    ux = uv[:, 0].float().clamp(0.0, 1.0) * float(w - 1)
    uy = uv[:, 1].float().clamp(0.0, 1.0) * float(h - 1)
    lx, ly = ux.floor().long().clamp(max=w - 1), uy.floor().long().clamp(max=h - 1)
    hx, hy = (lx + 1).clamp(max=w - 1), (ly + 1).clamp(max=h - 1)
    sx, sy = (ux - lx.float())[:, None], (uy - ly.float())[:, None]
    ul, ur, dl, dr = texels[hy, lx, :3], texels[hy, hx, :3], texels[ly, lx, :3], texels[ly, hx, :3]
    ui = ul * (1.0 - sx) + ur * sx
    di = dl * (1.0 - sx) + dr * sx
    c = ui * sy + di * (1.0 - sy)
    hit, has_uv = (flags & 1) != 0, (flags & 2) != 0
    c = torch.where((hit & has_uv)[:, None], c, torch.zeros_like(c))
    c = torch.where(hit[:, None], c, miss[None, :]).view(n, k, 3)
    tot = torch.zeros((n, 3), dtype=torch.float32, device=c.device)
    for j in range(k):
        tot = tot + c[:, j]
    return tot / float(k)


def _input(sc, tp, tn, keys, k, reps, rounds=5):
    import torch
    import nrays_amd as nr
    n = tp.shape[0]
    L, rot = nr.hemisphere_dirs(k), nr.rotation_table(8)
    tl, tr = torch.from_numpy(L).cuda(), torch.from_numpy(rot).cuda()
    tk = torch.from_numpy(keys.astype(np.int64)).cuda()
    texels = torch.from_numpy(np.random.default_rng(7).uniform(0.0, 1.0, size=(MAP_SIZE, MAP_SIZE, 4)).astype(np.float32)).cuda()
    node_map = [0] * int(sc.descriptor.desc.num_nodes)
    miss = (0.25, 0.5, 1.0)
    tmiss = torch.tensor(miss, dtype=torch.float32, device="cuda")
    ro, rd = _torch_occlusion_rays(tp, tn, L, rot, 1e-3, keys)
    hits = nr.closest_hits(sc, ro, rd, want=("uv", "flags"))
    fns = {"fused": lambda: nr.gather_maps_points(sc, tp, tn, tl, [texels], node_map, tr, 1e-3, miss=miss, keys=tk),
           "closest_hits": lambda: nr.closest_hits(sc, ro, rd, want=("uv", "flags")),
           "torch_build_rays": lambda: _torch_occlusion_rays(tp, tn, L, rot, 1e-3, keys),
           "torch_sample_fold": lambda: _torch_sample_fold(texels, hits.uv, hits.flags, n, k, tmiss),
           "gather_points_depth_0": lambda: nr.gather_points(sc, tp, tn, tl, tr, 1e-3, 1.0, 0, keys=tk)}
    ms = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            ms[name].append(_time(fn, reps, warmup=1))
    got, counts = nr.gather_maps_points(sc, tp, tn, tl, [texels], node_map, tr, 1e-3, miss=miss, keys=tk, want_counts=True)
    want = _torch_sample_fold(texels, hits.uv, hits.flags, n, k, tmiss)
    row = {"points": int(n), "dirs": int(k), "rays": int(n * k), "map": [MAP_SIZE, MAP_SIZE], "rounds": rounds, "reps": reps,
           "mapped_share": round(float(counts[:, 0].sum().item()) / (n * k), 4), "missed_share": round(float(counts[:, 1].sum().item()) / (n * k), 4),
           "points_whose_bits_differ_from_the_torch_restatement": int((got.view(torch.int32) != want.view(torch.int32)).any(dim=1).sum().item())}
    for name, v in ms.items():
        row[name] = {"ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    med = lambda name: row[name]["ms"]  # noqa: E731
    row["parts_with_torch_ms"] = round(med("torch_build_rays") + med("closest_hits") + med("torch_sample_fold"), 4)
    row["ns_per_ray_fused"] = round(med("fused") * 1e6 / (n * k), 4)
    row["expectation_a"] = "MET" if med("fused") <= med("closest_hits") else "MISSED"
    row["expectation_b"] = "MET" if med("fused") < med("gather_points_depth_0") else "MISSED"
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gather_maps_rate.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="320x180 instead of 1920x1080 (a rehearsal of the tool, not a measurement)")
    args = ap.parse_args()
    import torch
    from tools import standins
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    w, h = (320, 180) if args.quick else (1920, 1080)
    sc, cam = standins.sponza_scene()
    sc.device_handle()
    tp, tn, keys = _first_hit_points((sc, cam), w, h)
    n = tp.shape[0]
    sub = torch.from_numpy(np.linspace(0, n - 1, min(16384, n)).astype(np.int64)).cuda()
    out = {"device": torch.cuda.get_device_name(0), "scene": "sponza stand-in, one shared %d x %d float32 map for every node" % (MAP_SIZE, MAP_SIZE), "resolution": [w, h],
           "expectation": EXPECTATION,
           "first_hits_16_dirs": _input(sc, tp, tn, keys, 16, max(1, args.reps // 4)),
           "subset_16384_points_64_dirs": _input(sc, tp[sub].contiguous(), tn[sub].contiguous(), keys[sub.cpu().numpy()], 64, args.reps)}
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
