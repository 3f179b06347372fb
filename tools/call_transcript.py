"""What the Python batch wrappers hand to the library, as a transcript without addresses (tests/test_call_transcript.py, tests/golden/call_transcript_*.json).

  python tools/call_transcript.py numpy|torch OUT.json [--tree DIR]     (DIR: the checkout whose nrays_amd is recorded; default: this one)

abi.load_hip_lib is replaced by a stand-in whose every attribute records its call and returns abi.OK, so no kernel runs and `numpy` needs no GPU.  Every public
wrapper and probe of nrays_amd.scene runs over a fixed list of small cases on a stub scene.  A record holds the entry point, its scalar arguments, and for every
pointer the NAME of the argument or result whose memory it is ("other": memory of neither, a converted copy or an upload; null: absent), the same for the fields
of a params struct and of its NraysTexture records, and the name, dtype and shape of what came back.  `torch` runs the tensor forms, the device= forms and the
calls that upload numpy arguments, on real CUDA tensors."""
import contextlib
import ctypes as C
import json
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE_HANDLE = 0x5CE0E0


class Recorder:
    """The stand-in library: any attribute is an entry point that records (name, args, the params struct's fields as they were during the call)."""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args, [_struct_fields(a._obj) if hasattr(a, "_obj") and isinstance(a._obj, C.Structure) else None for a in args]))
            return 0
        return entry


@contextlib.contextmanager
def stand_in(abi):
    rec, real = Recorder(), abi.load_hip_lib
    abi.load_hip_lib = lambda: rec
    try:
        yield rec
    finally:
        abi.load_hip_lib = real


def stub_scene():
    return types.SimpleNamespace(device_handle=lambda: SCENE_HANDLE, descriptor=types.SimpleNamespace(desc=types.SimpleNamespace(num_nodes=2)))


def _address(a):
    if a is None or isinstance(a, int):
        return a
    if isinstance(a, C.c_void_p):
        return a.value
    if isinstance(a, C.Array):
        return C.addressof(a)
    return C.cast(a, C.c_void_p).value  # a typed pointer; byref() of a scalar is not one


def _is_pointer_type(t):
    return t is C.c_void_p or (isinstance(t, type) and issubclass(t, C._Pointer))


def _struct_fields(s):
    """A params struct as a dict: scalars as they are, addresses raw under ("addr", value) for _resolve, the NraysTexture records expanded."""
    out = {}
    for name, t in s._fields_:
        v = getattr(s, name)
        if t is C.c_void_p:
            out[name] = ("addr", v)
        elif _is_pointer_type(t):
            out[name] = [_struct_fields(v[i]) for i in range(s.num_maps)] if v else None
        elif isinstance(v, C.Array):
            out[name] = list(v)
        else:
            out[name] = v
    return out


def _addr_of(x):
    return x.data_ptr() if hasattr(x, "data_ptr") else x.ctypes.data


def _named_arrays(prefix, x, out):
    """Every array or tensor with at least one element inside `x`, as (name, address)."""
    if x is None or isinstance(x, (int, float, str, bool)):
        return
    if hasattr(x, "_fields"):
        for f in x._fields:
            _named_arrays("%s.%s" % (prefix, f) if prefix else f, getattr(x, f), out)
    elif isinstance(x, (list, tuple)):
        for i, e in enumerate(x):
            _named_arrays("%s[%d]" % (prefix, i), e, out)
    elif hasattr(x, "shape") and int(np.prod(tuple(x.shape))) > 0:
        out.append((prefix, _addr_of(x)))
    elif hasattr(x, "data") and hasattr(x.data, "pixels"):  # a Texture2d
        out.append((prefix, _addr_of(x.data.pixels)))


def _describe(prefix, x):
    if hasattr(x, "_fields"):
        return {f: _describe(f, getattr(x, f)) for f in x._fields}
    if isinstance(x, (list, tuple)):
        return [_describe("%s[%d]" % (prefix, i), e) for i, e in enumerate(x)]
    if hasattr(x, "shape"):
        return {"type": type(x).__module__.split(".")[0], "dtype": str(x.dtype), "shape": list(x.shape)}
    return x


def _resolve(v, names):
    if isinstance(v, tuple) and v and v[0] == "addr":
        return None if not v[1] else names.get(v[1], "other")
    if isinstance(v, dict):
        return {k: _resolve(e, names) for k, e in v.items()}
    if isinstance(v, list):
        return [_resolve(e, names) for e in v]
    return v


def run_case(nr, label, fn, args):
    """One wrapper call under the stand-in: {"case", "calls": [...], "returned" | "raises"}."""
    record = {"case": label}
    inputs = []
    for k, v in args.items():
        _named_arrays(k, v, inputs)
    with stand_in(nr.abi) as rec:
        try:
            result = getattr(nr.scene, fn)(stub_scene(), **args)
        except Exception as e:  # a refusal is part of the behaviour
            record["raises"] = "%s: %s" % (type(e).__name__, e)
            result = None
    results = []
    _named_arrays("result", result, results)
    names = {}
    for name, addr in results + inputs:  # (an input wins over a result that is the same memory)
        names[addr] = name
    names[SCENE_HANDLE] = "scene"
    record["calls"] = []
    for entry, cargs, structs in rec.calls:
        types_ = nr.abi.HIP_SYMBOLS[entry][1]
        out = []
        for i, (a, t, s) in enumerate(zip(cargs, types_, structs)):
            if s is not None:
                out.append(_resolve(s, names))
            elif "_device" in entry and i == len(cargs) - 1:
                out.append("stream")
            elif _is_pointer_type(t):
                addr = None if a is None else (_address(a) if not hasattr(a, "_obj") else -1)
                out.append(None if addr is None else names.get(addr, "other"))
            else:
                out.append(a)
        assert len(cargs) == len(types_), (entry, len(cargs), len(types_))
        record["calls"].append({"entry": entry, "args": out})
    if "raises" not in record:
        record["returned"] = _describe("result", result)
    return record


def cases(nr, form):
    """The fixed list: (label, wrapper, arguments).  Arrays conform (float64 / float32 / int32 / uint32 / uint64, C-contiguous) unless the label says otherwise."""
    n, f8, f4 = 4, np.float64, np.float32
    rng = np.random.RandomState(7)
    P, N, D, V = (np.ascontiguousarray(rng.rand(n, 3), f8) for _ in range(4))
    toi, refr, energy = np.ones(n, f8), np.ones(n, f8), np.ones(n, f4)
    keys, hf, nodes, uvs = np.arange(n, dtype=np.uint64), np.ones(n, np.uint32), np.zeros(n, np.int32), np.ascontiguousarray(rng.rand(n, 2), f8)
    L, R3, R0 = nr.hemisphere_dirs(4), nr.rotation_table(3), np.zeros((0, 2), f8)
    m0 = np.ascontiguousarray(rng.rand(2, 2, 4), f4)
    w = h = 4
    tf, tp, tn, tv = np.ones(w * h, np.uint32), np.ascontiguousarray(rng.rand(w * h, 3), f8), np.tile([0.0, 1.0, 0.0], (w * h, 1)), np.ascontiguousarray(rng.rand(w * h, 3), f4)
    wide = np.ascontiguousarray(rng.rand(w * h, 6), f4)

    if form == "numpy":
        T = lambda a: a  # noqa: E731
    else:
        import torch
        signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}

        def T(a):
            return torch.from_numpy(a.view(signed.get(a.dtype, a.dtype))).cuda()
    out = []

    def add(label, fn, **kw):
        out.append(("%s/%s" % (fn, label), fn, kw))

    tables = dict(sample_dirs=T(L))
    pts = dict(points=T(P), normals=T(N))
    tx = nr.SurfaceTexels(points=T(tp), normals=T(tn), uv=None, node=None, prim=None, flags=T(tf))

    # rays
    add("plain", "trace_rays", origins=T(P), dirs=T(D))
    add("all columns, unordered", "trace_rays", origins=T(P), dirs=T(D), refr=T(refr), energy=T(energy), keys=T(keys), max_depth=2, unordered=True)
    add("plain", "closest_hits", origins=T(P), dirs=T(D))
    add("max_toi, want=(), unordered", "closest_hits", origins=T(P), dirs=T(D), max_toi=T(toi), unordered=True, want=())
    add("want=(uv, flags)", "closest_hits", origins=T(P), dirs=T(D), want=("uv", "flags"))
    # points
    add("plain", "shade_points", points=T(P), normals=T(N), view_dirs=T(V), nodes=T(nodes))
    add("uvs, hit_flags, keys", "shade_points", points=T(P), normals=T(N), view_dirs=T(V), nodes=T(nodes), uvs=T(uvs), hit_flags=T(hf), keys=T(keys))
    add("plain", "occlusion_points", **pts, **tables)
    add("3 rotations, hit_flags, keys, max_toi", "occlusion_points", **pts, **tables, rotations=T(R3), bias=0.25, max_toi=3.0, hit_flags=T(hf), keys=T(keys))
    add("0 rotations", "occlusion_points", **pts, **tables, rotations=T(R0))
    for fn in ("gather_points", "gather_sh_points"):
        add("plain", fn, **pts, **tables)
        add("3 rotations, hit_flags, keys, unordered", fn, **pts, **tables, rotations=T(R3), bias=0.25, energy=0.5, max_depth=3, hit_flags=T(hf), keys=T(keys), unordered=True)
        add("0 rotations", fn, **pts, **tables, rotations=T(R0))
    add("bands=2", "gather_sh_points", **pts, **tables, bands=2)
    add("plain", "gather_probes", positions=T(P), sample_dirs=T(L))
    add("bands=1, keys, ordered", "gather_probes", positions=T(P), sample_dirs=T(L), bands=1, keys=T(keys), unordered=False)
    add("plain", "gather_maps_points", **pts, **tables, maps=[T(m0)], node_map=[0, -1])
    add("3 rotations, hit_flags, keys, counts, dict", "gather_maps_points", **pts, **tables, maps=[T(m0)], node_map={1: 0}, rotations=T(R3), bias=0.25, max_toi=3.0,
        miss=(0.5, 0.25, 0.125), hit_flags=T(hf), keys=T(keys), want_counts=True)
    add("0 rotations, Texture2d, clamped node_map", "gather_maps_points", **pts, **tables, rotations=T(R0),
        maps=[nr.Texture2d(nr.ImageData(m0), nr.Interpolation.Nearest, nr.Overflow.Wrap)], node_map=[99, -7])
    # texels
    dev = None if form == "numpy" else "cuda"
    add("full", "surface_texels", node=1, width=w, height=h, device=dev)
    add("want=(), centres, flipped", "surface_texels", node=0, width=w, height=h, centres=True, flip_normals=True, want=(), device=dev)
    add("want=(uv, prim)", "surface_texels", node=0, width=w, height=h, want=("uv", "prim"), device=dev)
    add("flags only", "dilate_texels", flags=T(tf), width=w, height=h, radius=2)
    add("values, source", "dilate_texels", flags=T(tf), width=w, height=h, radius=3, values=T(tv), want_source=True)
    add("values (h, w, c)", "dilate_texels", flags=T(tf), width=w, height=h, radius=1, values=T(tv.reshape(h, w, 3).copy()))
    add("plain", "filter_texels", flags=T(tf), width=w, height=h, points=T(tp), normals=T(tn), values=T(tv))
    add("step, radius, cos", "filter_texels", flags=T(tf), width=w, height=h, points=T(tp), normals=T(tn), values=T(tv), step=2, pos_radius=1.5, normal_cos=0.5)

    if form == "numpy":
        # the converted-copy paths, and the probes (numpy only)
        add("float32 origins", "trace_rays", origins=P.astype(f4), dirs=D)
        add("float32 dirs", "closest_hits", origins=P, dirs=D.astype(f4))
        add("int64 nodes, int64 hit_flags, int64 keys", "shade_points", points=P, normals=N, view_dirs=V, nodes=nodes.astype(np.int64), hit_flags=hf.astype(np.int64),
            keys=keys.astype(np.int64))
        add("float32 points", "occlusion_points", points=P.astype(f4), normals=N, sample_dirs=L)
        add("float32 points, list tables", "gather_points", points=P.astype(f4), normals=N, sample_dirs=L.tolist(), rotations=R3.tolist())
        add("float32 normals", "gather_sh_points", points=P, normals=N.astype(f4), sample_dirs=L)
        add("float32 positions", "gather_probes", positions=P.astype(f4), sample_dirs=L)
        add("float32 points, non-contiguous map", "gather_maps_points", points=P.astype(f4), normals=N, sample_dirs=L, maps=[np.asfortranarray(m0)], node_map=[0, 0])
        add("non-contiguous values", "dilate_texels", flags=tf, width=w, height=h, radius=2, values=wide[:, ::2])
        add("float64 values, int64 flags", "dilate_texels", flags=tf.astype(np.int64), width=w, height=h, radius=2, values=tv.astype(f8))
        add("non-contiguous values, int32 flags", "filter_texels", flags=tf.astype(np.int32), width=w, height=h, points=tp, normals=tn, values=wide[:, ::2])
        add("plain", "occlusion_ray_probe", points=P, normals=N, sample_dirs=L)
        add("3 rotations, keys", "occlusion_ray_probe", points=P, normals=N, sample_dirs=L, rotations=R3, bias=0.25, keys=keys)
        colours = np.ascontiguousarray(rng.rand(n, 4, 3), f4)
        add("plain", "gather_sh_fold", points=P, normals=N, sample_dirs=L, ray_colours=colours)
        add("3 rotations, hit_flags, keys, ms", "gather_sh_fold", points=P, normals=N, sample_dirs=L, ray_colours=colours, rotations=R3, bands=2, hit_flags=hf, keys=keys, want_ms=True)
        add("plain", "ray_order", origins=P, dirs=D)
        add("plain", "gather_order", points=P, normals=N, sample_dirs=L)
        add("3 rotations, hit_flags, keys", "gather_order", points=P, normals=N, sample_dirs=L, rotations=R3, bias=0.25, hit_flags=hf, keys=keys)
    else:
        # calls that upload: no blocking form (intersects_rays), ping-pong on the device (denoise_texels), numpy tables next to tensor points, device= with numpy arguments
        txn = nr.SurfaceTexels(points=tp, normals=tn, uv=None, node=None, prim=None, flags=tf)
        add("plain", "intersects_rays", origins=T(P), dirs=T(D), max_toi=T(toi))
        add("unordered", "intersects_rays", origins=T(P), dirs=T(D), max_toi=T(toi), unordered=True)
        add("numpy in", "intersects_rays", origins=P, dirs=D, max_toi=toi)
        add("numpy in, unordered", "intersects_rays", origins=P, dirs=D, max_toi=toi, unordered=True)
        add("3 passes", "denoise_texels", tx=tx, values=T(tv), width=w, height=h)
        add("1 pass, (h, w, c)", "denoise_texels", tx=tx, values=T(tv.reshape(h, w, 3).copy()), passes=1, pos_radius=1.5, normal_cos=0.5)
        add("numpy in, 2 passes", "denoise_texels", tx=txn, values=tv, passes=2, width=w, height=h)
        add("numpy tables", "occlusion_points", **pts, sample_dirs=L, rotations=R3)
        add("numpy tables", "gather_points", **pts, sample_dirs=L, rotations=R3)
        add("numpy tables", "gather_sh_points", **pts, sample_dirs=L, rotations=R0)
        add("numpy tables, numpy map", "gather_maps_points", **pts, sample_dirs=L, maps=[m0], node_map=[0, -1], want_counts=True)
        add("device=, numpy flags and values", "dilate_texels", flags=tf, width=w, height=h, radius=2, values=tv, want_source=True, device="cuda")
        add("device=, tensors", "dilate_texels", flags=T(tf), width=w, height=h, radius=2, values=T(tv), device="cuda")
        add("device=, numpy in", "filter_texels", flags=tf, width=w, height=h, points=tp, normals=tn, values=tv, device="cuda")
        add("device=, tensors", "filter_texels", flags=T(tf), width=w, height=h, points=T(tp), normals=T(tn), values=T(tv), device="cuda")
        # the converted-copy path of tensors: non-contiguous ones
        tw = T(wide)
        add("non-contiguous origins", "trace_rays", origins=T(np.ascontiguousarray(rng.rand(n, 6)))[:, ::2], dirs=T(D))
        add("non-contiguous points", "shade_points", points=T(np.ascontiguousarray(rng.rand(n, 6)))[:, ::2], normals=T(N), view_dirs=T(V), nodes=T(nodes))
        add("non-contiguous points", "gather_points", points=T(np.ascontiguousarray(rng.rand(n, 6)))[:, ::2], normals=T(N), sample_dirs=T(L))
        add("non-contiguous values", "dilate_texels", flags=T(tf), width=w, height=h, radius=2, values=tw[:, ::2])
        add("non-contiguous values", "filter_texels", flags=T(tf), width=w, height=h, points=T(tp), normals=T(tn), values=tw[:, ::2])
        # refusals that the driver words
        add("host tensors", "gather_points", points=torch.from_numpy(P), normals=torch.from_numpy(N), sample_dirs=L)
        add("mixed", "shade_points", points=T(P), normals=N, view_dirs=T(V), nodes=T(nodes))
        add("float32 tensor", "closest_hits", origins=T(P).float(), dirs=T(D))
    if form == "numpy":
        import torch
        add("mixed", "shade_points", points=P, normals=torch.from_numpy(N), view_dirs=V, nodes=nodes)
        add("mixed values", "dilate_texels", flags=tf, width=w, height=h, radius=2, values=torch.from_numpy(tv))
        add("host tensors", "occlusion_points", points=torch.from_numpy(P), normals=torch.from_numpy(N), sample_dirs=L)
    return out


def transcript(nr, form):
    return [run_case(nr, label, fn, args) for label, fn, args in cases(nr, form)]


if __name__ == "__main__":
    form, path = sys.argv[1], sys.argv[2]
    sys.path.insert(0, sys.argv[4] if len(sys.argv) > 4 and sys.argv[3] == "--tree" else ROOT)
    import nrays_amd
    with open(path, "w") as f:
        json.dump(transcript(nrays_amd, form), f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d cases -> %s" % (len(json.load(open(path))), path))
