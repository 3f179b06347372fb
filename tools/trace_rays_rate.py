#!/usr/bin/env python
"""Rays per second of nrays_trace_rays_device (caller-supplied rays) beside nrays_render_device of the same frame.

  (a) balls 1080p camera rays in image order (pixel-major, as camera_rays() gives them)
  (b) the same rays shuffled (incoherent order)
  (c) sponza stand-in 1080p camera rays, then AO-style cosine-weighted rays from their first hits (normal side, 1e-3 off the surface),
      timed as one batch (camera + AO) and the AO rays alone
  (d) the sponza camera rays shuffled, the AO rays shuffled

Each batch and each frame: warm-up, then 20 launches timed by HIP events around all of them.  The render's value_traced is bench.py's
figure (rays that went through a BVT query per second, from an instrumented frame counted as the timed kernel traces).

Every batch is timed as it comes ("ms") and with the caller's hint that it comes in no useful order ("hinted_ms": unordered=True, the
library bins the rays by a spatial key first; left out when the library under NRAYS_HIP_LIB is older than the hint).  --coherence adds two
CPU figures per batch and order (as given / in the order the reorder probe returns): "tiles_per_wave", the mean number of distinct
8 x 8-pixel tiles the 64 consecutive rays of a wave come from (an AO ray counts for the pixel whose camera ray spawned it), and
"one_octant_waves", the share of waves whose 64 rays share their direction signs.  --sweep times the shuffled camera rays of both scenes
for n = 2^10 .. 2^22 hinted and unhinted with every hinted batch reordered (NRAYS_RAY_REORDER=2): the threshold of DESIGN §5b.

The AO rays are built on the device from the camera rays' closest hits (nrays_cast_rays_device through closest_hits()).  Each scene also gets
a row "closest hits, camera rays": closest_hits() of the camera rays in order, shuffled, and shuffled under the hint, beside the wall time of
the blocking test probe nrays_debug_cast_batch on the same rays (upload, kernel, 64-byte records back).  --cast times these rows only.

--shade times, and nothing else: on the sponza stand-in and on its 8-light variant, closest_hits() of the camera rays runs once, then shade_hits()
at those hits (nrays_shade_points_device alone: the direct lighting without the closest-hit traversal) is timed beside trace_rays() of the same rays
and closest_hits() itself — in alternating rounds, each of --reps launches between events, so that the spread of a figure is known; "ms" is the
median round.  A library without the entry point (an older one under NRAYS_HIP_LIB) gets the trace_rays and closest_hits figures only, and
--beside FILE copies the workloads of such an earlier run into this run's JSON under "beside".

--occlusion times, and nothing else, the leg e_sponza_occlusion: ambient occlusion at the first hits of the sponza stand-in's camera rays with 16 directions
a point, and at a 16 384-point subset of them with 64.  The fused call (occlusion_points(): rays built in registers, one folded value per point) stands
beside what the library offered before on the very same rays — the rays of the definition built with torch on the device, intersects_rays() on them unhinted
and with unordered=True, and the torch fold of the per-ray results, timed apart — and beside itself on handles forced to one lane per point and to 8 / 64 lanes
per point (NRAYS_OCCLUSION_LANES).  Alternating rounds, each of a few launches between events: min, median and max of every leg.

--texels times, and nothing else, the leg g_surface_texels: surface_texels() (nrays_surface_texels_device) of a grid mesh of about 500 k triangles with an atlas
of its own at 1024^2 and 4096^2 lattice points, and of a two-triangle quad at 4096^2 (one triangle = half the atlas: the owner pass must not care) — the whole call,
its owner and resolve passes between events of their own (nrays_debug_surface_texels_passes), shade_points() on the same texels, and for the 1024^2 lattice of the
grid the numpy mirror surface_texels_ref() on the host, which is what a caller without the entry point does (plus the upload, not counted).

--texels --dilate (or --dilate alone: that leg and nothing else, into profiles/dilate_rate.json) times the leg i_dilate_texels: dilate_texels()
(nrays_dilate_texels_device) with four float channels on the surface_texels() flags of an atlas of 64 x 64 quad charts with gutters between them
(tools/scenes_util.py: atlas_quads_mesh) at 1024^2 and 4096^2, radius 2, 8 and 64 — beside surface_texels() on the same lattice, beside what a caller paid
before (`radius` passes of an 8-neighbour fill written with torch ops on the same device tensors; time only, its values differ by definition) and beside
the traffic floor: the bytes the call must move over the 6.29 TB/s a float4 copy reaches.  The expectation, written before the first run, is judged in the
JSON: cheaper than the torch passes in every row, and at radius <= 8 cheaper than surface_texels().

--filter (that leg and nothing else, into profiles/filter_rate.json) times the leg j_filter_texels: filter_texels() (nrays_filter_texels_device) with three float
channels at steps 1, 2 and 4 and the three-pass denoise_texels() on the surface_texels() result of the --texels sine-surface grid (100 % covered) and of the
--dilate atlas of 64 x 64 quad charts (gutters), at 1024^2 and 4096^2 — beside a torch restatement of one pass (25 shifted slices with the same weights; time
only), beside the traffic floor ((52 + 8 * channels) bytes per texel over the 6.29 TB/s a float4 copy reaches), beside gather_points() with 16 directions on
the same texels divided by 16 — what one more direction costs.  The expectations, written into the JSON before the first run, are judged per row: every pass
cheaper than its torch restatement, and three passes cheaper than one more gathered direction.

--gather-sh (that leg and nothing else, into profiles/gather_sh_rate.json) times the leg k_gather_sh: gather_sh_points() (nrays_gather_sh_points_device) at bands
1 / 2 / 3, hinted and unhinted, beside gather_points() on the same input — the gather leg's two inputs and 4 096 probes on a grid in the hall under
sphere_dirs(1024) —, the fold kernel alone (nrays_debug_gather_sh_fold, HIP events of its own) on the input's first chunk, the torch restatement of the fold
on the same per-ray colours, and the fold's traffic floor (12 bytes a ray plus the outputs over the 6.29 TB/s a float4 copy reaches).  The expectations are
written to the file before the first run and judged in it.
--gather times, and nothing else, the leg h_sponza_gather: the incoming light (gather_points(): Scene::trace on hemisphere rays built in registers, one mean
colour per point) at the same two inputs as --occlusion — 16 directions at every first hit, 64 at a 16 384-point subset — beside what a caller did before it: the
same rays built with torch on the device, trace_rays() on them with the keys of gather_ray_keys() unhinted and with unordered=True, and the torch fold of the
per-ray colours, each timed apart — beside itself under the hint (fused_unordered: gather_points(unordered=True), the reorder inside the call, in the same rounds)
— and beside itself on handles forced to one lane per point and to 8 / 64 lanes per point (NRAYS_OCCLUSION_LANES).  The same
two inputs are then timed on the stand-in with a ball that reflects and refracts in the hall: a double-branching scene, where the call keeps a chunk's ray colours
and runs the continuation queue per ray.  Alternating rounds, each of a few launches between events: min, median and max of every leg.

  python tools/trace_rays_rate.py [--out profiles/trace_rays_rate.json] [--reps 20] [--quick] [--coherence] [--sweep] [--cast] [--shade [--beside FILE]] [--occlusion] [--gather] [--texels] [--dilate] [--filter] [--gather-sh]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CAST_DTYPE = np.dtype([("toi", "<f8"), ("normal", "<f8", 3), ("uv", "<f8", 2), ("node_id", "<i4"), ("flags", "<u4")])


def _time(fn, reps, warmup=3):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps  # ms per launch


def _has_hint():
    from nrays_amd import abi
    return hasattr(abi.load_hip_lib(), "nrays_trace_rays_device_ex")


def _coherence(pix, d, width, order=None):
    """(tiles per wave, share of one-octant waves) of the rays in `order` (None: as given); pix = the pixel a ray belongs to."""
    idx = np.arange(len(pix)) if order is None else np.asarray(order, dtype=np.int64)
    n = len(idx) // 64 * 64
    if n == 0:
        return None
    p = np.asarray(pix, dtype=np.int64)[idx[:n]]
    tile = (p // width // 8) * ((width + 7) // 8) + (p % width) // 8
    t = np.sort(tile.reshape(-1, 64), axis=1)
    tiles = float((1 + (np.diff(t, axis=1) != 0).sum(axis=1)).mean())
    sign = np.signbit(d[idx[:n]])
    octant = (sign[:, 0] * 1 + sign[:, 1] * 2 + sign[:, 2] * 4).reshape(-1, 64)
    return {"tiles_per_wave": round(tiles, 2), "one_octant_waves": round(float((octant.min(axis=1) == octant.max(axis=1)).mean()), 4)}


def _batch(sc, o, d, reps, keys=None, pix=None, width=0):
    import torch
    import nrays_amd as nr
    o, d = np.ascontiguousarray(o), np.ascontiguousarray(d)
    to, td = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    tk = None if keys is None else torch.from_numpy(keys.astype(np.int64)).cuda()
    ms = _time(lambda: nr.trace_rays(sc, to, td, keys=tk), reps)
    out = {"rays": int(len(o)), "ms": round(ms, 4), "mrays_per_s": round(len(o) / (ms * 1e-3) / 1e6, 2)}
    if _has_hint():
        hms = _time(lambda: nr.trace_rays(sc, to, td, keys=tk, unordered=True), reps)
        out.update(hinted_ms=round(hms, 4), hinted_mrays_per_s=round(len(o) / (hms * 1e-3) / 1e6, 2))
    if pix is not None:
        out["as_given"] = _coherence(pix, d, width)
        if _has_hint() and len(o) <= 1 << 22:
            out["reordered"] = _coherence(pix, d, width, nr.ray_order(sc, o, d)[1])
    return out


def _sweep(sc, o, d, k, reps):
    """Shuffled camera rays, the first n of them: unhinted and hinted ms for n = 2^10 .. 2^22 (every hinted batch reordered)."""
    rows = []
    for lg in range(10, 23):
        n = min(1 << lg, len(o))
        r = _batch(sc, o[:n], d[:n], reps, k[:n])
        rows.append({"n": n, "ms": r["ms"], "hinted_ms": r.get("hinted_ms")})
        if n == len(o):
            break
    return rows


def _render(sc, p, reps):
    import torch
    import nrays_amd as nr
    from nrays_amd import abi
    lib = abi.load_hip_lib()
    out = torch.empty((p.height, p.width, 3), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    ms = _time(lambda: abi.check(lib.nrays_render_device(sc.device_handle(), C.byref(p), C.c_void_p(out.data_ptr()), stream)), reps)
    abi.check(lib.nrays_render_device_counted(sc.device_handle(), C.byref(p), C.c_void_p(out.data_ptr()), stream, abi.COUNT_AS_TIMED))
    st = nr.get_stats(sc)
    traced = int(st.rays_traced()) - int(st.rays_shadow_elided)
    npx = p.width * p.height
    return {"ms": round(ms, 4), "primary_mrays_per_s": round(npx / (ms * 1e-3) / 1e6, 2),
            "rays_traced_per_frame": traced, "value_traced": round(traced / (ms * 1e-3) / 1e6, 2)}


def _first_hits(sc, o, d):
    """AO rays from the closest hits of the camera rays (closest_hits on the device: toi, node and normal only), cosine-weighted about the
    normal on the side the camera ray came from, and the index of the camera ray each came from.  Built with torch on the GPU; returned as
    numpy arrays, which the batches and the coherence figures take."""
    import torch
    import nrays_amd as nr
    to, td = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    r = nr.closest_hits(sc, to, td, want=("normal",))
    hit = r.node >= 0
    to, td = to[hit], td[hit]
    pt = to + td * r.toi[hit][:, None]
    nrm = r.normal[hit]
    nrm = nrm / torch.linalg.norm(nrm, dim=1)[:, None]
    nrm = torch.where(((nrm * td).sum(dim=1) > 0.0)[:, None], -nrm, nrm)  # the side the camera ray came from
    gen = torch.Generator(device="cuda").manual_seed(0)
    u1 = torch.rand(len(pt), dtype=torch.float64, device="cuda", generator=gen)
    u2 = torch.rand(len(pt), dtype=torch.float64, device="cuda", generator=gen)
    rad, phi = torch.sqrt(u1), 2.0 * np.pi * u2
    local = torch.stack([rad * torch.cos(phi), rad * torch.sin(phi), torch.sqrt(torch.clamp(1.0 - u1, min=0.0))], dim=1)
    ey, ex = torch.tensor([[0.0, 1.0, 0.0]], dtype=torch.float64, device="cuda"), torch.tensor([[1.0, 0.0, 0.0]], dtype=torch.float64, device="cuda")
    a = torch.where(torch.abs(nrm[:, 0:1]) > 0.9, ey, ex)
    t = torch.linalg.cross(a.expand_as(nrm), nrm)
    t = t / torch.linalg.norm(t, dim=1)[:, None]
    b = torch.linalg.cross(nrm, t)
    dirs = local[:, 0:1] * t + local[:, 1:2] * b + local[:, 2:3] * nrm
    dirs = dirs / torch.linalg.norm(dirs, dim=1)[:, None]
    return (pt + nrm * 1e-3).cpu().numpy(), dirs.cpu().numpy(), torch.nonzero(hit)[:, 0].cpu().numpy()


def _closest_hits_row(sc, o, d, perm, reps):
    """closest hits, camera rays: closest_hits() on device tensors in order, shuffled and shuffled under the hint (every output, and toi + node
    alone), beside the blocking probe nrays_debug_cast_batch on the same host arrays (wall clock: it uploads, runs and copies 64-byte records back)."""
    import torch
    import nrays_amd as nr
    from nrays_amd import abi
    n = len(o)
    rate = lambda ms: round(n / (ms * 1e-3) / 1e6, 2)  # noqa: E731
    row = {"rays": int(n)}
    so, sd = np.ascontiguousarray(o[perm]), np.ascontiguousarray(d[perm])
    for name, (ho, hd), kw in (("in_order", (o, d), {}), ("shuffled", (so, sd), {}), ("shuffled_hinted", (so, sd), dict(unordered=True))):
        to, td = torch.from_numpy(np.ascontiguousarray(ho)).cuda(), torch.from_numpy(np.ascontiguousarray(hd)).cuda()
        ms = _time(lambda: nr.closest_hits(sc, to, td, **kw), reps)
        ms2 = _time(lambda: nr.closest_hits(sc, to, td, want=(), **kw), reps)
        row[name] = {"ms": round(ms, 4), "mrays_per_s": rate(ms), "toi_node_only_ms": round(ms2, 4), "toi_node_only_mrays_per_s": rate(ms2)}
    res = np.zeros(n, dtype=CAST_DTYPE)
    dp = C.POINTER(C.c_double)
    lib, oo, dd = abi.load_hip_lib(), np.ascontiguousarray(o), np.ascontiguousarray(d)
    probe = lambda: abi.check(lib.nrays_debug_cast_batch(sc.device_handle(), 0, n, oo.ctypes.data_as(dp), dd.ctypes.data_as(dp), None,  # noqa: E731
                                                         res.ctypes.data_as(C.POINTER(abi.NraysCastResult))))
    probe()
    t0 = time.perf_counter()
    for _ in range(max(1, reps // 4)):
        probe()
    ms = (time.perf_counter() - t0) * 1e3 / max(1, reps // 4)
    row["blocking_probe_in_order"] = {"ms": round(ms, 4), "mrays_per_s": rate(ms)}
    return row


def _shade_row(sc, o, d, k, reps, rounds=5):
    """shade_hits() at the closest hits of the rays, beside trace_rays() of the same rays and closest_hits() itself: device tensors, alternating rounds."""
    import torch
    import nrays_amd as nr
    from nrays_amd import abi
    to, td = torch.from_numpy(np.ascontiguousarray(o)).cuda(), torch.from_numpy(np.ascontiguousarray(d)).cuda()
    tk = torch.from_numpy(k.astype(np.int64)).cuda()
    hits = nr.closest_hits(sc, to, td)
    fns = {"trace_rays": lambda: nr.trace_rays(sc, to, td, keys=tk), "closest_hits": lambda: nr.closest_hits(sc, to, td)}
    if hasattr(abi.load_hip_lib(), "nrays_shade_points_device"):
        fns["shade_hits"] = lambda: nr.shade_hits(sc, to, td, hits, keys=tk)
    ms = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            ms[name].append(_time(fn, reps))
    row = {"rays": int(len(o)), "hits": int((hits.node >= 0).sum().item()), "rounds": rounds}
    for name, v in ms.items():
        row[name] = {"ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    return row


OCCLUSION_MAX_TOI = 0.5  # the occlusion leg's radius (the stand-in is a closed hall about 7 units long: no ray gets out of it)


def _first_hit_points(sc, w, h):
    """The first hits of the scene's camera rays as device tensors (points, normals on the camera's side) and their keys: the inputs of the occlusion and gather legs."""
    import torch
    import nrays_amd as nr
    from nrays_amd import math3d
    cam = sc[1]
    proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], w, h)
    o, d, keys = nr.camera_rays((w, h), cam["eye"], proj)
    to, td = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    hits = nr.closest_hits(sc[0], to, td, want=("normal", "flags"))
    hit = (hits.flags & 1) != 0
    tp = (to + td * hits.toi[:, None])[hit].contiguous()
    nm = hits.normal[hit]
    tn = torch.where((((nm[:, 0] * td[hit][:, 0] + nm[:, 1] * td[hit][:, 1]) + nm[:, 2] * td[hit][:, 2]) > 0)[:, None], -nm, nm).contiguous()
    return tp, tn, keys[hit.cpu().numpy()]


def _torch_occlusion_rays(tp, tn, L, rot, bias, keys):
    """nrays_amd.occlusion_rays() with torch on the device: the same element-wise f64 operations (the rotation index comes from the host: torch has no uint64
    arithmetic).  Returns (origins, dirs) as (n * k, 3) tensors, point-major."""
    import torch
    from nrays_amd.scene import SALT_OCCLUSION, _rng_hash
    n, k = tp.shape[0], len(L)
    tl = torch.from_numpy(np.ascontiguousarray(L)).cuda()
    nx, ny, nz = tn[:, 0:1], tn[:, 1:2], tn[:, 2:3]
    s = torch.copysign(torch.ones_like(nz), nz)
    a = -1.0 / (s + nz)
    b = nx * ny * a
    t = (1.0 + s * nx * nx * a, s * b, -s * nx)
    u = (b, s + ny * ny * a, -ny)
    lx, ly, lz = tl[None, :, 0], tl[None, :, 1], tl[None, :, 2]
    r = torch.from_numpy((_rng_hash(keys, SALT_OCCLUSION) % np.uint64(len(rot))).astype(np.int64)).cuda()
    tr = torch.from_numpy(np.ascontiguousarray(rot)).cuda()
    c_r, s_r = tr[r, 0:1], tr[r, 1:2]
    x, y = c_r * lx - s_r * ly, s_r * lx + c_r * ly
    dirs = torch.stack([(x * t[q] + y * u[q]) + lz * tn[:, q:q + 1] for q in range(3)], dim=2)
    origins = (tp + tn * bias)[:, None, :].expand(n, k, 3)
    return origins.reshape(n * k, 3).contiguous(), dirs.reshape(n * k, 3).contiguous()


def _occlusion_input(scenes, tp, tn, keys, k, reps, rounds=5):
    """One input of the occlusion leg: n points, k directions, 8 rotations.  scenes: {"auto" | "lanes_1" | "lanes_8" | "lanes_64": handle}."""
    import torch
    import nrays_amd as nr
    n = tp.shape[0]
    L, rot = nr.hemisphere_dirs(k), nr.rotation_table(8)
    tl, tr = torch.from_numpy(L).cuda(), torch.from_numpy(rot).cuda()
    tk = torch.from_numpy(keys.astype(np.int64)).cuda()
    ro, rd = _torch_occlusion_rays(tp, tn, L, rot, 1e-3, keys)
    tmax = torch.full((n * k,), OCCLUSION_MAX_TOI, dtype=torch.float64, device="cuda")
    sc = scenes["auto"]
    lit, filt = nr.intersects_rays(sc, ro, rd, tmax)

    def torch_fold():
        f = filt.view(n, k, 3)
        tot = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
        for j in range(k):
            tot = tot + f[:, j]
        return tot / float(k), lit.view(n, k).sum(dim=1)

    fns = {"fused": lambda: nr.occlusion_points(sc, tp, tn, tl, tr, 1e-3, OCCLUSION_MAX_TOI, keys=tk),
           "intersects_rays": lambda: nr.intersects_rays(sc, ro, rd, tmax),
           "intersects_rays_unordered": lambda: nr.intersects_rays(sc, ro, rd, tmax, unordered=True),
           "torch_fold": torch_fold}
    for name, other in scenes.items():
        if name != "auto":
            fns["fused_" + name] = lambda other=other: nr.occlusion_points(other, tp, tn, tl, tr, 1e-3, OCCLUSION_MAX_TOI, keys=tk)
    ms = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            ms[name].append(_time(fn, reps, warmup=1))
    got, (want_f, want_o) = nr.occlusion_points(sc, tp, tn, tl, tr, 1e-3, OCCLUSION_MAX_TOI, keys=tk), torch_fold()
    row = {"points": int(n), "dirs": int(k), "rays": int(n * k), "max_toi": OCCLUSION_MAX_TOI, "rounds": rounds, "reps": reps, "open_share": round(float(lit.float().mean().item()), 4),
           "points_that_differ_from_the_torch_fold": int(((got.filter != want_f).any(dim=1) | (got.open != want_o)).sum().item())}
    for name, v in ms.items():
        row[name] = {"ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    return row


def _occlusion_leg(w, h, reps):
    import torch
    from tools import standins
    scenes = {}
    for name, lanes in (("auto", None), ("lanes_1", "0"), ("lanes_8", "3"), ("lanes_64", "6")):
        os.environ.pop("NRAYS_OCCLUSION_LANES", None)
        if lanes is not None:
            os.environ["NRAYS_OCCLUSION_LANES"] = lanes  # read when a handle is created
        scenes[name], cam = standins.sponza_scene()
        scenes[name].device_handle()
    os.environ.pop("NRAYS_OCCLUSION_LANES", None)
    tp, tn, keys = _first_hit_points((scenes["auto"], cam), w, h)
    n = tp.shape[0]
    sub = torch.from_numpy(np.linspace(0, n - 1, min(16384, n)).astype(np.int64)).cuda()
    pick = lambda names: {k: scenes[k] for k in names}  # noqa: E731
    return {"first_hits_16_dirs": _occlusion_input(pick(("auto", "lanes_1", "lanes_8")), tp, tn, keys, 16, max(1, reps // 4)),
            "subset_16384_points_64_dirs": _occlusion_input(pick(("auto", "lanes_1", "lanes_8", "lanes_64")), tp[sub].contiguous(), tn[sub].contiguous(), keys[sub.cpu().numpy()], 64, reps)}


def _gather_input(scenes, tp, tn, keys, k, reps, rounds=5):
    """One input of the gather leg: n points, k directions, 8 rotations, energy 1, max_depth 0.  scenes: {"auto" | "lanes_1" | "lanes_8" | "lanes_64": handle}."""
    import torch
    import nrays_amd as nr
    n = tp.shape[0]
    L, rot = nr.hemisphere_dirs(k), nr.rotation_table(8)
    tl, tr = torch.from_numpy(L).cuda(), torch.from_numpy(rot).cuda()
    tk = torch.from_numpy(keys.astype(np.int64)).cuda()
    rk = torch.from_numpy(nr.gather_ray_keys(keys, k).reshape(-1).view(np.int64)).cuda()
    ro, rd = _torch_occlusion_rays(tp, tn, L, rot, 1e-3, keys)
    sc = scenes["auto"]
    rgb = nr.trace_rays(sc, ro, rd, keys=rk)

    def torch_fold():
        c = rgb.view(n, k, 3)
        tot = torch.zeros((n, 3), dtype=torch.float32, device="cuda")
        for j in range(k):
            tot = tot + c[:, j]
        return tot / float(k)

    fns = {"fused": lambda: nr.gather_points(sc, tp, tn, tl, tr, 1e-3, 1.0, 0, keys=tk),
           "fused_unordered": lambda: nr.gather_points(sc, tp, tn, tl, tr, 1e-3, 1.0, 0, keys=tk, unordered=True),
           "torch_build_rays": lambda: _torch_occlusion_rays(tp, tn, L, rot, 1e-3, keys),
           "trace_rays": lambda: nr.trace_rays(sc, ro, rd, keys=rk),
           "trace_rays_unordered": lambda: nr.trace_rays(sc, ro, rd, keys=rk, unordered=True),
           "torch_fold": torch_fold}
    for name, other in scenes.items():
        if name != "auto":
            fns["fused_" + name] = lambda other=other: nr.gather_points(other, tp, tn, tl, tr, 1e-3, 1.0, 0, keys=tk)
    ms = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            ms[name].append(_time(fn, reps, warmup=1))
    got, want = nr.gather_points(sc, tp, tn, tl, tr, 1e-3, 1.0, 0, keys=tk), torch_fold()
    hinted = nr.gather_points(sc, tp, tn, tl, tr, 1e-3, 1.0, 0, keys=tk, unordered=True)
    row = {"points": int(n), "dirs": int(k), "rays": int(n * k), "energy": 1.0, "max_depth": 0, "rounds": rounds, "reps": reps,
           "points_that_differ_from_the_torch_fold": int((got != want).any(dim=1).sum().item()),
           "points_whose_hinted_bits_differ": int((hinted.view(torch.int32) != got.view(torch.int32)).any(dim=1).sum().item())}
    for name, v in ms.items():
        row[name] = {"ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    return row


def _glass_sponza():
    """The stand-in with a ball in the middle of the hall that reflects AND refracts: a double-branching scene, whose gather keeps per-ray colours and runs the queue."""
    import nrays_amd as nr
    from tools import standins
    sc, cam = standins.sponza_scene()
    glass = nr.PhongMaterial((0.1, 0.1, 0.15), (0.6, 0.7, 0.9), (1, 1, 1), None, None, 80.0)
    ball = nr.SceneNode(glass, 0.3, 0.4, 0.5, 1.3, nr.Isometry3(cam["at"]), nr.Ball(30.0))
    return nr.Scene(list(sc._nodes) + [ball], sc._lights, sc._background), cam


def _gather_leg(w, h, reps):
    import torch
    from tools import standins
    scenes = {}
    for name, lanes in (("auto", None), ("lanes_1", "0"), ("lanes_8", "3"), ("lanes_64", "6")):
        os.environ.pop("NRAYS_OCCLUSION_LANES", None)
        if lanes is not None:
            os.environ["NRAYS_OCCLUSION_LANES"] = lanes  # read when a handle is created
        scenes[name], cam = standins.sponza_scene()
        scenes[name].device_handle()
    os.environ.pop("NRAYS_OCCLUSION_LANES", None)
    pick = lambda names: {k: scenes[k] for k in names}  # noqa: E731
    out = {}
    for leg, group, cam_ in (("sponza", None, cam), ("sponza_glass_ball_double_branching",) + _glass_sponza()):
        tp, tn, keys = _first_hit_points((scenes["auto"] if group is None else group, cam_), w, h)
        n = tp.shape[0]
        sub = torch.from_numpy(np.linspace(0, n - 1, min(16384, n)).astype(np.int64)).cuda()
        many = pick(("auto", "lanes_1", "lanes_8")) if group is None else {"auto": group}
        few = pick(("auto", "lanes_1", "lanes_8", "lanes_64")) if group is None else {"auto": group}
        out[leg] = {"first_hits_16_dirs": _gather_input(many, tp, tn, keys, 16, max(1, reps // 4)),
                    "subset_16384_points_64_dirs": _gather_input(few, tp[sub].contiguous(), tn[sub].contiguous(), keys[sub.cpu().numpy()], 64, reps)}
    return out


GATHER_SH_EXPECTATION = {
    "a": "gather_sh_points(bands = 3, unordered=True) within 5 % of gather_points(unordered=True) on the same input: the trace costs about 1.6 ns a ray (52.4 ms / 33 M rays, "
         "profiles/gather_order_rate.json); a fold at 10 % of its traffic floor — the low end of what dilate / filter reach — costs about 0.02 ns a ray, 1.3 % of the trace; "
         "clearing and storing the ray colours adds less than that",
    "b": "the fold alone (k_gather_fold_sh between two HIP events of nrays_debug_gather_sh_fold) is cheaper than its torch restatement (basis from the ray directions, "
         "sequential f32 fold over j) in every row",
    "c": "the fold alone as a share of its traffic floor (12 bytes a ray plus the outputs over the 6.29 TB/s a float4 copy reaches) is recorded; no threshold"}


def _gather_sh_input(sc, tp, tn, keys, L, rot, bias, reps, rounds=3):
    """One input of the gather-sh leg: n points under the table L (energy 1, max_depth 0).  Whole calls on device tensors; the fold alone and its torch restatement
    on the input's first chunk (at most 2^22 rays: what one launch of the fold sees)."""
    import torch
    import nrays_amd as nr
    from nrays_amd.scene import SH_K
    n, k = tp.shape[0], len(L)
    tl = torch.from_numpy(L).cuda()
    tr = None if rot is None else torch.from_numpy(rot).cuda()
    tk = torch.from_numpy(keys.astype(np.int64)).cuda()
    fns = {"gather_points": lambda: nr.gather_points(sc, tp, tn, tl, tr, bias, 1.0, 0, keys=tk),
           "gather_points_unordered": lambda: nr.gather_points(sc, tp, tn, tl, tr, bias, 1.0, 0, keys=tk, unordered=True)}
    for bands in (1, 2, 3):
        fns["gather_sh_bands_%d" % bands] = lambda bands=bands: nr.gather_sh_points(sc, tp, tn, tl, tr, bias, 1.0, 0, bands, keys=tk)
        fns["gather_sh_bands_%d_unordered" % bands] = lambda bands=bands: nr.gather_sh_points(sc, tp, tn, tl, tr, bias, 1.0, 0, bands, keys=tk, unordered=True)
    # the first chunk, on the host for the probe and on the device for the restatement
    nc = min(n, max(1, (1 << 22) // k))
    hp, hn, hk = tp[:nc].cpu().numpy(), tn[:nc].cpu().numpy(), np.ascontiguousarray(keys[:nc]).astype(np.uint64)
    ro, rd = nr.occlusion_rays(hp, hn, L, rot, bias, hk)
    rk = nr.gather_ray_keys(hk, k).reshape(-1)
    t_rd = torch.from_numpy(rd).cuda()
    colours = nr.trace_rays(sc, torch.from_numpy(ro.reshape(-1, 3)).cuda(), t_rd.view(-1, 3), keys=torch.from_numpy(rk.view(np.int64)).cuda()).view(nc, k, 3)
    h_colours = colours.cpu().numpy()
    K0, K1, K2, K3, K4 = SH_K

    def torch_fold():
        x, y, z = t_rd[..., 0], t_rd[..., 1], t_rd[..., 2]
        Y = torch.stack([torch.full_like(x, K0), K1 * y, K1 * z, K1 * x, (K2 * x) * y, (K2 * y) * z, K3 * ((3.0 * z) * z - 1.0), (K2 * x) * z, K4 * (x * x - y * y)], dim=-1).float()
        acc = torch.zeros((nc, 9, 3), dtype=torch.float32, device="cuda")
        for j in range(k):
            acc = acc + Y[:, j, :, None] * colours[:, j, None, :]
        return acc / float(k)

    ms = {name: [] for name in fns}
    ms["torch_fold_bands_3_first_chunk"], fold_ms = [], {1: [], 2: [], 3: []}
    for _ in range(rounds):
        for name, fn in fns.items():
            ms[name].append(_time(fn, reps, warmup=1))
        ms["torch_fold_bands_3_first_chunk"].append(_time(torch_fold, max(1, reps // 2), warmup=1))
        for bands in fold_ms:
            nr.gather_sh_fold(sc, hp, hn, L, h_colours, rot, bias, bands, keys=hk)  # (warm)
            fold_ms[bands].append(min(nr.gather_sh_fold(sc, hp, hn, L, h_colours, rot, bias, bands, keys=hk, want_ms=True)[1] for _ in range(max(2, reps))))
    got = nr.gather_sh_points(sc, tp[:nc], tn[:nc], tl, tr, bias, 1.0, 0, 3, keys=tk[:nc])
    hinted = nr.gather_sh_points(sc, tp[:nc], tn[:nc], tl, tr, bias, 1.0, 0, 3, keys=tk[:nc], unordered=True)
    alone = torch.from_numpy(nr.gather_sh_fold(sc, hp, hn, L, h_colours, rot, bias, 3, keys=hk)).cuda()
    row = {"points": int(n), "dirs": int(k), "rays": int(n * k), "energy": 1.0, "max_depth": 0, "rounds": rounds, "reps": reps, "first_chunk_points": int(nc),
           "first_chunk_values_whose_bits_differ_hinted": int((hinted.view(torch.int32) != got.view(torch.int32)).sum().item()),
           "first_chunk_values_whose_bits_differ_from_the_fold_alone": int((alone.view(torch.int32) != got.view(torch.int32)).sum().item()),
           "first_chunk_values_that_differ_from_the_torch_fold": int((torch_fold() != got).sum().item())}
    for name, v in ms.items():
        row[name] = {"ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    for bands, v in fold_ms.items():
        floor_ms = (12.0 * nc * k + 12.0 * bands * bands * nc) / HBM_COPY_BYTES_PER_S * 1e3
        med = float(np.median(v))
        row["fold_alone_bands_%d_first_chunk" % bands] = {"ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "how": "the least of max(2, reps) probe calls per round; median of the rounds",
                                                          "traffic_floor_ms": round(floor_ms, 5), "share_of_floor": round(floor_ms / med, 4) if med > 0 else None,
                                                          "ns_per_ray": round(med * 1e6 / (nc * k), 5)}
    a = row["gather_sh_bands_3_unordered"]["ms"] / row["gather_points_unordered"]["ms"]
    row["expectation"] = {"a_bands_3_hinted_over_gather_points_hinted": round(a, 4), "a": "MET" if a <= 1.05 else "MISSED",
                          "b": "MET" if row["fold_alone_bands_3_first_chunk"]["ms"] < row["torch_fold_bands_3_first_chunk"]["ms"] else "MISSED",
                          "c_share_of_floor_bands_3": row["fold_alone_bands_3_first_chunk"]["share_of_floor"]}
    return row


def _gather_sh_leg(w, h, reps, path):
    import torch
    import nrays_amd as nr
    from tools import standins
    out = {"expectation_written_before_the_first_run": GATHER_SH_EXPECTATION,
           "inputs": "first_hits_16_dirs / subset_16384_points_64_dirs: the gather leg's (8 rotations, bias 1e-3); probes_4096_sphere_1024: a 16^3 grid over the middle half of the "
                     "first hits' bounding box, sphere_dirs(1024), normal (0, 0, 1), bias 0, no rotations"}
    with open(path, "w") as f:  # the expectation is on file before anything is timed
        json.dump({"workloads": {"k_gather_sh": out}}, f, indent=1)
    sc, cam = standins.sponza_scene()
    tp, tn, keys = _first_hit_points((sc, cam), w, h)
    n = tp.shape[0]
    sub = torch.from_numpy(np.linspace(0, n - 1, min(16384, n)).astype(np.int64)).cuda()
    rot = nr.rotation_table(8)
    out["first_hits_16_dirs"] = _gather_sh_input(sc, tp, tn, keys, nr.hemisphere_dirs(16), rot, 1e-3, max(1, reps // 4))
    out["subset_16384_points_64_dirs"] = _gather_sh_input(sc, tp[sub].contiguous(), tn[sub].contiguous(), keys[sub.cpu().numpy()], nr.hemisphere_dirs(64), rot, 1e-3, reps)
    lo, hi = tp.min(dim=0).values.cpu().numpy(), tp.max(dim=0).values.cpu().numpy()
    g = (np.arange(16) + 0.5) / 16.0 * 0.5 + 0.25
    grid = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3) * (hi - lo) + lo
    up = np.tile([0.0, 0.0, 1.0], (len(grid), 1))
    out["probes_4096_sphere_1024"] = _gather_sh_input(sc, torch.from_numpy(grid).cuda(), torch.from_numpy(up).cuda(), np.arange(len(grid), dtype=np.uint64), nr.sphere_dirs(1024), None, 0.0,
                                                      max(1, reps // 4))
    return out


def _texels_row(sc, mesh, size, reps, mirror, rounds=5):
    import torch
    import nrays_amd as nr
    w, h = size
    dev = torch.device("cuda", torch.cuda.current_device())
    tx = nr.surface_texels(sc, 0, w, h, want=("normals", "uv", "node"), device=dev)
    view = -tx.normals
    fns = {"surface_texels": lambda: nr.surface_texels(sc, 0, w, h, want=("normals", "uv", "node"), device=dev),
           "shade_points": lambda: nr.shade_points(sc, tx.points, tx.normals, view, tx.node, uvs=tx.uv, hit_flags=tx.flags)}
    ms = {name: [] for name in fns}
    for _ in range(rounds):  # alternating rounds, each timed by events around `reps` launches after a warm-up
        for name, fn in fns.items():
            ms[name].append(_time(fn, reps, warmup=2))
    nr.surface_texels_passes(sc, 0, w, h, repeats=3)
    passes = nr.surface_texels_passes(sc, 0, w, h, repeats=rounds * reps)
    row = {"triangles": int(len(mesh[1])), "lattice": [w, h], "points": w * h, "covered_share": round(float((tx.flags != 0).float().mean().item()), 4), "rounds": rounds, "reps": reps}
    for name, v in ms.items():
        row[name] = {"ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    for k, name in enumerate(("owner_pass", "resolve_pass")):
        row[name] = {"ms": round(float(np.median(passes[:, k])), 4), "min_ms": round(float(passes[:, k].min()), 4), "max_ms": round(float(passes[:, k].max()), 4)}
    if mirror:
        t0 = time.perf_counter()
        ref = nr.surface_texels_ref(mesh[0], mesh[1], mesh[2], None, w, h)
        row["numpy_mirror_host"] = {"ms": round((time.perf_counter() - t0) * 1e3, 1), "runs": 1}
        row["points_that_differ_from_the_mirror"] = int((tx.flags.cpu().numpy().astype(np.uint32) != ref.flags).sum() + (tx.points.cpu().numpy() != ref.points).any(axis=1).sum())
    return row


def _texels_leg(reps, quick):
    import nrays_amd as nr
    from tools import scenes_util as su
    from tools import standins
    n = 64 if quick else 500
    p, uv, idx = standins._surface(lambda u, v: np.stack([8.0 * u - 4.0, 0.5 * np.sin(6.0 * u) * np.cos(5.0 * v), 8.0 * v - 4.0], -1), n, n)  # 2 n^2 triangles, the atlas = the unit square
    grid = (su.f32_exact(p), idx, su.f32_exact(uv))
    quad = (su.f32_exact([[-4, 0, -4], [4, 0, -4], [4, 0, 4], [-4, 0, 4]]), np.asarray([[0, 2, 1], [0, 3, 2]], np.uint32), su.f32_exact([[0, 0], [1, 0], [1, 1], [0, 1]]))
    mat = nr.PhongMaterial((0.2, 0.2, 0.2), (0.9, 0.9, 0.9), (0.5, 0.5, 0.5), su.checker_texture(64, 8), None, 40.0)
    scene = lambda m: nr.Scene([nr.SceneNode(mat, 0.0, 0.0, 1.0, 1.0, nr.Isometry3(), nr.TriMesh(*m[:2], m[2]))], [nr.Light((1.0, 6.0, -2.0), 0.0, 1, (1.0, 1.0, 1.0))], (0, 0, 0))  # noqa: E731
    small, large = ((128, 128), (512, 512)) if quick else ((1024, 1024), (4096, 4096))
    sg, sq = scene(grid), scene(quad)
    return {"grid_small_lattice": _texels_row(sg, grid, small, reps, True), "grid_large_lattice": _texels_row(sg, grid, large, max(1, reps // 4), False),
            "quad_large_lattice": _texels_row(sq, quad, large, max(1, reps // 4), False)}


def _torch_fill(values, covered, passes):
    """What a caller without dilate_texels() writes: `passes` rounds of an 8-neighbour fill with torch ops (each round, an unfilled texel takes the first
    filled neighbour in a fixed order).  Not the library's definition — compared for its time only."""
    import torch
    import torch.nn.functional as F
    h, w = covered.shape
    v, m = values.clone(), covered.clone()
    for _ in range(passes):
        vp = F.pad(v.permute(2, 0, 1)[None], (1, 1, 1, 1))[0]
        mp = F.pad(m[None, None].to(torch.uint8), (1, 1, 1, 1))[0, 0].bool()
        nv, nm = v.clone(), m.clone()
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if dy == 0 and dx == 0:
                    continue
                take = mp[1 + dy:h + 1 + dy, 1 + dx:w + 1 + dx] & ~nm
                nv = torch.where(take[..., None], vp[:, 1 + dy:h + 1 + dy, 1 + dx:w + 1 + dx].permute(1, 2, 0), nv)
                nm = nm | take
        v, m = nv, nm
    return v


HBM_COPY_BYTES_PER_S = 6.29e12  # MI355X, measured with a float4 copy


def _dilate_row(sc, size, radius, reps, rounds=5):
    import torch
    import nrays_amd as nr
    w, h = size
    n = w * h
    dev = torch.device("cuda", torch.cuda.current_device())
    tx = nr.surface_texels(sc, 0, w, h, want=(), device=dev)
    covered = (tx.flags & 1) != 0
    values = torch.rand((n, 4), dtype=torch.float32, device=dev) * covered[:, None]
    work = values.clone()

    def dilate():
        work.copy_(values)  # (the call is in place; the copy is timed apart and subtracted)
        nr.dilate_texels(sc, tx.flags, w, h, radius, values=work)
    fns = {"copy_of_the_values": lambda: work.copy_(values), "copy_and_dilate_texels": dilate,
           "surface_texels": lambda: nr.surface_texels(sc, 0, w, h, want=("normals", "uv", "node"), device=dev)}
    ms = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            ms[name].append(_time(fn, reps, warmup=2))
    torch_reps = 1 if radius * n > 1 << 26 else 3
    grid_values, grid_covered = values.view(h, w, 4), covered.view(h, w)
    ms["torch_passes"] = [_time(lambda: _torch_fill(grid_values, grid_covered, radius), torch_reps, warmup=1) for _ in range(2)]
    _, source, out_flags = nr.dilate_texels(sc, tx.flags, w, h, radius, values=work, want_source=True)
    filled = int(((out_flags & 4) != 0).sum().item())
    floor_bytes = 4 * n + 2 * n + 2 * n + 4 * n + 2 * 16 * filled  # flags read, dx written and read, out_flags written, four floats read and written per filled texel
    row = {"lattice": [w, h], "points": n, "radius": radius, "channels": 4, "covered_share": round(float(covered.float().mean().item()), 4),
           "filled_share": round(filled / n, 4), "left_unfilled_share": round(float((source < 0).float().mean().item()), 4), "rounds": rounds, "reps": reps, "torch_reps": torch_reps}
    for name, v in ms.items():
        row[name] = {"ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    t = row["copy_and_dilate_texels"]["ms"] - row["copy_of_the_values"]["ms"]
    row["dilate_texels"] = {"ms": round(t, 4), "how": "copy_and_dilate_texels - copy_of_the_values (medians)"}
    row["traffic_floor"] = {"bytes": floor_bytes, "ms": round(floor_bytes / HBM_COPY_BYTES_PER_S * 1e3, 4), "share_of_it_reached": round(floor_bytes / HBM_COPY_BYTES_PER_S * 1e3 / t, 3) if t > 0 else None}
    row["expectation"] = {"cheaper_than_the_torch_passes": "MET" if t < row["torch_passes"]["ms"] else "MISSED"}
    if radius <= 8:
        row["expectation"]["cheaper_than_surface_texels"] = "MET" if t < row["surface_texels"]["ms"] else "MISSED"
    return row


def _dilate_leg(reps, quick):
    import nrays_amd as nr
    from tools import scenes_util as su
    mesh = su.atlas_quads_mesh(16 if quick else 64)
    mat = nr.PhongMaterial((0.2, 0.2, 0.2), (0.9, 0.9, 0.9), (0.5, 0.5, 0.5), None, None, 40.0)
    sc = nr.Scene([nr.SceneNode(mat, 0.0, 0.0, 1.0, 1.0, nr.Isometry3(), nr.TriMesh(*mesh[:2], mesh[2]))], [nr.Light((1.0, 6.0, -2.0), 0.0, 1, (1.0, 1.0, 1.0))], (0, 0, 0))
    small, large = ((128, 128), (512, 512)) if quick else ((1024, 1024), (4096, 4096))
    out = {"expectation_written_before_the_first_run": "dilate_texels cheaper than `radius` torch passes in every row; at radius <= 8 cheaper than surface_texels on the same lattice",
           "atlas": "64 x 64 quad charts, each 0.75 of its atlas cell (tools/scenes_util.py: atlas_quads_mesh)"}
    for name, size, rp in (("small_lattice", small, reps), ("large_lattice", large, max(1, reps // 4))):
        for radius in (2, 8, 64):
            out["%s_r%d" % (name, radius)] = _dilate_row(sc, size, radius, rp)
    return out


def _torch_filter(cov, p, nm, v, step, pos_radius, normal_cos):
    """What a caller without filter_texels() writes: one pass of the same filter as 25 shifted slices of the padded lattice, with torch ops on the same device
    tensors (cov (h, w) bool, p / nm (h, w, 3) float64, v (h, w, c) float32).  Compared for its time only."""
    import torch
    import torch.nn.functional as F
    h, w = cov.shape
    pad = 2 * step
    padded = lambda t: F.pad(t.permute(2, 0, 1), (pad, pad, pad, pad))  # noqa: E731
    pp, nn, vv = padded(p), padded(nm), padded(v)
    cc = F.pad(cov[None].to(torch.uint8), (pad, pad, pad, pad))[0].bool()
    pc, nc = p.permute(2, 0, 1), nm.permute(2, 0, 1)
    acc, wsum = torch.zeros_like(vv[:, pad:pad + h, pad:pad + w]), torch.zeros((h, w), dtype=torch.float32, device=v.device)
    taps = (1.0, 4.0, 6.0, 4.0, 1.0)
    for j in range(-2, 3):
        for i in range(-2, 3):
            ys, xs = pad + j * step, pad + i * step
            if i == 0 and j == 0:
                wt = cov.float() * 36.0
            else:
                d = pp[:, ys:ys + h, xs:xs + w] - pc
                wp = 1.0 - (d * d).sum(0) / (pos_radius * pos_radius)
                wn = (((nc * nn[:, ys:ys + h, xs:xs + w]).sum(0) - normal_cos) / (1.0 - normal_cos)).clamp(max=1.0)
                take = cc[ys:ys + h, xs:xs + w] & cov & (wp > 0) & (wn > 0)
                wt = torch.where(take, (taps[i + 2] * taps[j + 2]) * wp.float() * wn.float(), torch.zeros_like(wsum))
            acc = acc + wt[None] * vv[:, ys:ys + h, xs:xs + w]
            wsum = wsum + wt
    return torch.where(cov[..., None], (acc / wsum[None]).permute(1, 2, 0), v)


FILTER_EXPECTATION = ("every filter_texels pass cheaper than its torch restatement on the same device tensors; the three passes of denoise_texels cheaper than one more "
                      "gathered direction (gather_points with 16 directions on the same texels / 16) on the same lattice — if they are not, adding rays beats filtering")


def _filter_row(sc, size, reps, rounds=5, channels=3):
    import torch
    import nrays_amd as nr
    w, h = size
    n = w * h
    dev = torch.device("cuda", torch.cuda.current_device())
    tx = nr.surface_texels(sc, 0, w, h, want=("normals",), device=dev)
    covered = (tx.flags & 1) != 0
    values = torch.rand((n, channels), dtype=torch.float32, device=dev) * covered[:, None]
    pos_radius, normal_cos = 16.0 * 8.0 / w, 0.5  # both meshes span 8 world units over the atlas: 16 texels of reach
    dirs = nr.hemisphere_dirs(16)
    fns = {"filter_step_%d" % s: (lambda s=s: nr.filter_texels(sc, tx.flags, w, h, tx.points, tx.normals, values, s, pos_radius, normal_cos)) for s in (1, 2, 4)}
    fns["denoise_3_passes"] = lambda: nr.denoise_texels(sc, tx, values, 3, pos_radius, normal_cos, w, h)
    ms = {name: [] for name in fns}
    for _ in range(rounds):  # alternating rounds, each timed by events around `reps` launches after a warm-up
        for name, fn in fns.items():
            ms[name].append(_time(fn, reps, warmup=2))
    grid = (covered.view(h, w), tx.points.view(h, w, 3), tx.normals.view(h, w, 3), values.view(h, w, channels))
    torch_reps = 1 if n > 1 << 22 else 3
    for s in (1, 2, 4):
        ms["torch_step_%d" % s] = [_time(lambda: _torch_filter(*grid, s, pos_radius, normal_cos), torch_reps, warmup=1) for _ in range(2)]
    gather_reps = 1 if n > 1 << 22 else 2
    ms["gather_points_16_dirs"] = [_time(lambda: nr.gather_points(sc, tx.points, tx.normals, dirs, None, 1e-3, 1.0, 0, hit_flags=tx.flags), gather_reps, warmup=1) for _ in range(2)]
    floor_ms = (52 + 8 * channels) * n / HBM_COPY_BYTES_PER_S * 1e3
    row = {"lattice": [w, h], "points": n, "channels": channels, "covered_share": round(float(covered.float().mean().item()), 4), "pos_radius": pos_radius, "normal_cos": normal_cos,
           "rounds": rounds, "reps": reps, "torch_reps": torch_reps, "gather_reps": gather_reps}
    for name, v in ms.items():
        row[name] = {"ms": round(float(np.median(v)), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    row["one_more_gathered_direction"] = {"ms": round(row["gather_points_16_dirs"]["ms"] / 16.0, 4), "how": "gather_points_16_dirs / 16"}
    row["traffic_floor"] = {"bytes": (52 + 8 * channels) * n, "ms": round(floor_ms, 4),
                            "share_of_it_reached": {"step_%d" % s: round(floor_ms / row["filter_step_%d" % s]["ms"], 3) for s in (1, 2, 4)}}
    row["expectation"] = {"step_%d_cheaper_than_its_torch_restatement" % s: "MET" if row["filter_step_%d" % s]["ms"] < row["torch_step_%d" % s]["ms"] else "MISSED" for s in (1, 2, 4)}
    row["expectation"]["three_passes_cheaper_than_one_more_gathered_direction"] = "MET" if row["denoise_3_passes"]["ms"] < row["one_more_gathered_direction"]["ms"] else "MISSED"
    return row


def _filter_leg(reps, quick, path):
    import nrays_amd as nr
    from tools import scenes_util as su
    from tools import standins
    out = {"expectation_written_before_the_first_run": FILTER_EXPECTATION,
           "inputs": "sine_grid: the --texels grid mesh, 100 % covered; atlas: 64 x 64 quad charts, each 0.75 of its atlas cell (tools/scenes_util.py: atlas_quads_mesh)"}
    with open(path, "w") as f:  # the expectation is on file before anything is timed
        json.dump({"workloads": {"j_filter_texels": out}}, f, indent=1)
    n = 64 if quick else 500
    p, uv, idx = standins._surface(lambda u, v: np.stack([8.0 * u - 4.0, 0.5 * np.sin(6.0 * u) * np.cos(5.0 * v), 8.0 * v - 4.0], -1), n, n)
    meshes = {"sine_grid": (su.f32_exact(p), idx, su.f32_exact(uv)), "atlas": su.atlas_quads_mesh(16 if quick else 64)}
    mat = nr.PhongMaterial((0.2, 0.2, 0.2), (0.9, 0.9, 0.9), (0.5, 0.5, 0.5), None, None, 40.0)
    scene = lambda m: nr.Scene([nr.SceneNode(mat, 0.0, 0.0, 1.0, 1.0, nr.Isometry3(), nr.TriMesh(*m[:2], m[2]))], [nr.Light((1.0, 6.0, -2.0), 0.0, 1, (1.0, 1.0, 1.0))], (0.2, 0.3, 0.4))  # noqa: E731
    small, large = ((128, 128), (512, 512)) if quick else ((1024, 1024), (4096, 4096))
    for name, m in meshes.items():
        sc = scene(m)
        for tag, size, rp in (("small_lattice", small, reps), ("large_lattice", large, max(1, reps // 4))):
            out["%s_%s" % (name, tag)] = _filter_row(sc, size, rp)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="default: profiles/trace_rays_rate.json; with --occlusion profiles/occlusion_rate.json, with --gather profiles/gather_rate.json")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="320x180 instead of 1920x1080 (a rehearsal of the tool, not a measurement)")
    ap.add_argument("--coherence", action="store_true", help="add the CPU coherence figures of every batch, as given and reordered")
    ap.add_argument("--sweep", action="store_true", help="time the shuffled camera rays for n = 2^10 .. 2^22 with every hinted batch reordered, nothing else")
    ap.add_argument("--cast", action="store_true", help="time the closest-hit rows of both scenes, nothing else")
    ap.add_argument("--shade", action="store_true", help="time shade_hits beside trace_rays and closest_hits on the sponza stand-in with 1 and 8 lights, nothing else")
    ap.add_argument("--beside", default=None, help="with --shade: the JSON of an earlier run (another library), copied into this one under 'beside'")
    ap.add_argument("--occlusion", action="store_true", help="time occlusion_points beside intersects_rays on the same rays and the torch fold (leg e_sponza_occlusion), nothing else")
    ap.add_argument("--gather", action="store_true", help="time gather_points beside building the rays with torch, trace_rays on them and the torch fold (leg h_sponza_gather), nothing else")
    ap.add_argument("--gather-sh", action="store_true", help="time gather_sh_points at bands 1 / 2 / 3 beside gather_points, the fold kernel alone, its torch restatement and its traffic floor (leg k_gather_sh, into profiles/gather_sh_rate.json), nothing else")
    ap.add_argument("--texels", action="store_true", help="time surface_texels, its two passes, shade_points on its texels and the numpy mirror (leg g_surface_texels), nothing else")
    ap.add_argument("--dilate", action="store_true", help="time dilate_texels beside surface_texels, the torch passes a caller wrote before and the traffic floor (leg i_dilate_texels, into profiles/dilate_rate.json); alone: nothing else")
    ap.add_argument("--filter", action="store_true", help="time filter_texels and denoise_texels beside a torch restatement, the traffic floor, and one more gathered direction (leg j_filter_texels, into profiles/filter_rate.json), nothing else")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "gather_sh_rate.json" if a.gather_sh else "filter_rate.json" if a.filter else "dilate_rate.json" if a.dilate and not a.texels else "surface_texels_rate.json" if a.texels else "occlusion_rate.json" if a.occlusion else "gather_rate.json" if a.gather else "trace_rays_rate.json")
    if a.sweep:
        os.environ["NRAYS_RAY_REORDER"] = "2"  # read when a handle is created
    import torch
    import nrays_amd as nr
    from nrays_amd import math3d
    from tools import scenes_util as su
    from tools import standins
    assert torch.cuda.is_available(), "the rate tool measures the GPU; there is nothing to measure without one"
    torch.cuda.set_device(0)
    w, h = (320, 180) if a.quick else (1920, 1080)
    res = {"tool": "tools/trace_rays_rate.py", "resolution": [w, h], "reps": a.reps, "device": torch.cuda.get_device_name(0),
           "library": "/".join((os.environ.get("NRAYS_HIP_LIB") or "nrays_amd/lib/libnrays_hip.so").split("/")[-2:]), "workloads": {}}

    if a.gather_sh:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        leg = dict(res, workloads={"k_gather_sh": _gather_sh_leg(w, h, a.reps, a.out)})
        with open(a.out, "w") as f:
            json.dump(leg, f, indent=1)
        print(json.dumps(leg))
        return

    if a.filter:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        leg = dict(res, workloads={"j_filter_texels": _filter_leg(a.reps, a.quick, a.out)})
        with open(a.out, "w") as f:
            json.dump(leg, f, indent=1)
        print(json.dumps(leg))
        return

    if a.dilate:
        leg = dict(res, workloads={"i_dilate_texels": _dilate_leg(a.reps, a.quick)})
        path = a.out if not a.texels else os.path.join(ROOT, "profiles", "dilate_rate.json")
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(leg, f, indent=1)
        print(json.dumps(leg))
        if not a.texels:
            return

    if a.texels:
        res["workloads"]["g_surface_texels"] = _texels_leg(a.reps, a.quick)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res))
        return

    if a.gather:
        res["workloads"]["h_sponza_gather"] = _gather_leg(w, h, a.reps)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res))
        return

    if a.occlusion:
        res["workloads"]["e_sponza_occlusion"] = _occlusion_leg(w, h, a.reps)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res))
        return

    if a.shade:
        for name, lights in (("f_sponza_shade_hits_camera_rays", 1), ("f_sponza_8_lights_shade_hits_camera_rays", 8)):
            sc, cam = standins.sponza_scene(n_lights=lights)
            proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], w, h)
            o, d, k = nr.camera_rays((w, h), cam["eye"], proj)
            res["workloads"][name] = _shade_row(sc, o, d, k, a.reps)
            del sc
        if a.beside:
            with open(a.beside) as f:
                other = json.load(f)
            res["beside"] = {"library": other["library"], "workloads": other["workloads"]}
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res))
        return

    sc, cam = su.balls_scene()
    proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], w, h)
    o, d, k = nr.camera_rays((w, h), cam["eye"], proj)
    perm = np.random.default_rng(1).permutation(len(o))
    pix = np.arange(len(o)) if a.coherence else None
    coh = lambda p: dict(pix=p, width=w) if a.coherence else {}  # noqa: E731
    res["workloads"]["e_balls_closest_hits_camera_rays"] = None if a.sweep else _closest_hits_row(sc, o, d, perm, a.reps)
    if a.sweep:
        res["sweep"] = {"balls_shuffled": _sweep(sc, o[perm], d[perm], k[perm], a.reps)}
    elif not a.cast:
        res["workloads"]["a_balls_image_order"] = _batch(sc, o, d, a.reps, k, **coh(pix))
        res["workloads"]["b_balls_shuffled"] = _batch(sc, o[perm], d[perm], a.reps, k[perm], **coh(perm))
        res["workloads"]["balls_render_device"] = _render(sc, nr.make_params((w, h), 1, 0.0, cam["eye"], proj), a.reps)
    del sc

    sc, cam = standins.sponza_scene()
    proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], w, h)
    o, d, k = nr.camera_rays((w, h), cam["eye"], proj)
    res["workloads"]["e_sponza_closest_hits_camera_rays"] = None if a.sweep else _closest_hits_row(sc, o, d, perm, a.reps)
    if a.sweep:
        res["sweep"]["sponza_shuffled"] = _sweep(sc, o[perm], d[perm], k[perm], a.reps)
    elif not a.cast:
        ao_o, ao_d, ao_pix = _first_hits(sc, o, d)
        ao_perm = np.random.default_rng(2).permutation(len(ao_o))
        res["workloads"]["c_sponza_camera_plus_ao"] = dict(_batch(sc, np.concatenate([o, ao_o]), np.concatenate([d, ao_d]), a.reps, **coh(np.concatenate([np.arange(len(o)), ao_pix]))),
                                                           camera_rays=int(len(o)), ao_rays=int(len(ao_o)))
        res["workloads"]["c_sponza_camera_only"] = _batch(sc, o, d, a.reps, k, **coh(pix))
        res["workloads"]["c_sponza_ao_only"] = _batch(sc, ao_o, ao_d, a.reps, **coh(ao_pix))
        res["workloads"]["d_sponza_camera_shuffled"] = _batch(sc, o[perm], d[perm], a.reps, k[perm], **coh(perm))
        res["workloads"]["d_sponza_ao_shuffled"] = _batch(sc, ao_o[ao_perm], ao_d[ao_perm], a.reps, **coh(ao_pix[ao_perm]))
        res["workloads"]["sponza_render_device"] = _render(sc, nr.make_params((w, h), 1, 0.0, cam["eye"], proj), a.reps)
    res["workloads"] = {k_: v for k_, v in res["workloads"].items() if v is not None}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
