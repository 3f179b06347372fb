"""How an argument of a batch call becomes an address: the one place that knows the numpy form and the torch form of the caller-batch wrappers of scene.py.

A wrapper validates shapes and settings, declares its columns and outputs, and makes one call:

    b = Batch((("origins", origins, F64), ("dirs", dirs, F64), ("keys", keys, U64)), (("rgb", (n, 3), F32),))
    b.call(scene, "nrays_trace_rays", n, *b.pin, max_depth, *b.pout)

A column is (name, value or None, kind[, upload]); an output is (name, shape, kind[, wanted]).  The form follows the lead (first) column: numpy arrays -> the
blocking entry point `name` on host memory; torch tensors on a GPU -> `name + "_device"` on torch.cuda.current_stream().  `device=` asks for the torch form with
numpy arguments (every column is converted as numpy would and moved there); a column marked `upload` (a table) may be numpy next to tensors.  Batch checks
or converts every column, refuses mixtures and host tensors, allocates the wanted outputs, and keeps everything alive while it lives.  Nothing here loads the
library before every column has passed.

Below the driver: the names scene.py (the calls) and restated.py (the numpy restatements) both need."""
import collections
import ctypes as C
import math

import numpy as np

from . import abi

F64, F32, I32, U32, U64 = range(5)  # kinds: float64; float32; int32 (numpy integers clipped); uint32 flag words (torch: int32 / uint32); uint64 keys (torch: int64 / uint64)
CURRENT = "current"                 # device=CURRENT: numpy arguments go to torch.cuda.current_device(); tensors stay where they are
_NP = (np.float64, np.float32, np.int32, np.uint32, np.uint64)
_DTYPE = tuple(np.dtype(t) for t in _NP)
_CTYPE = tuple(C.POINTER(c) for c in (C.c_double, C.c_float, C.c_int32, C.c_uint32, C.c_uint64))
_POINTER = dict({d.char: c for d, c in zip(_DTYPE, _CTYPE)}, Q=_CTYPE[U64])
_ndarray = np.ndarray
_SIGNED = {U32: np.int32, U64: np.int64}  # torch.from_numpy takes the unsigned kinds as their signed twins
_MIXED = "torch tensors and numpy arrays cannot be mixed in one call"
_torch = None


def _torch_kinds():
    """(torch, per kind the dtypes a tensor may have, per kind the dtype of an output tensor), built once: older torch has no uint32 / uint64."""
    global _torch
    if _torch is None:
        import torch
        either = lambda signed, name: tuple(d for d in (signed, getattr(torch, name, None)) if d is not None)  # noqa: E731
        _torch = (torch, ((torch.float64,), (torch.float32,), (torch.int32,), either(torch.int32, "uint32"), either(torch.int64, "uint64")),
                  (torch.float64, torch.float32, torch.int32, torch.int32, torch.int64))
    return _torch


def np_ptr(a):
    """The typed ctypes pointer of a numpy array of one of the five kinds (None stays None)."""
    return None if a is None else a.ctypes.data_as(_POINTER[a.dtype.char])


def _np_addr(a):
    return None if a is None else a.ctypes.data


def _tensor_ptr(t):
    return None if t is None else t.data_ptr()


def upload(a, device):
    """A numpy array as a tensor on `device`."""
    return _torch_kinds()[0].from_numpy(a).to(device)


def _np_column(name, a, kind):
    if kind <= F32:
        return _np_floats(name, a, _NP[kind])
    return _np_keys(a) if kind == U64 else _np_ints(name, a, _NP[kind])


class Batch:
    """The marshalled arguments of one batch call.  `ins`: the columns as contiguous arrays or tensors of their kind (None where absent), the caller's own memory
    where it conformed; `outs`: the allocated outputs (None where not wanted; flag words uint32 in numpy, int32 in torch); `pin` / `pout`: what the entry point takes
    for them; `ptr(x)`: the same for any array of this form; `addr(x)`: its address as an integer, for a params struct.  `device`: None in the numpy form."""

    def __init__(self, cols, outs, device=None, texels=False):
        lead = cols[0] if cols else None
        lead_t = lead is not None and _is_tensor(lead[1])
        if not lead_t and device is None:
            self.device, self.ptr, self.addr = None, np_ptr, _np_addr
            self.ins, self.pin, self.outs, self.pout = ins, pin, out, pout = [], [], [], []
            for c in cols:
                a, kind, p = c[1], c[2], None
                if a is not None:
                    if type(a) is not _ndarray or a.dtype != _DTYPE[kind] or not a.flags.c_contiguous:  # (a conforming array is passed as it is)
                        if _is_tensor(a):
                            raise ValueError("%s: %s" % (c[0], _MIXED) if texels else _MIXED)
                        a = _np_column(c[0], a, kind)
                    if len(c) < 4 or not c[3]:  # (a table goes into a params struct through addr())
                        p = a.ctypes.data_as(_CTYPE[kind])
                ins.append(a)
                pin.append(p)
            for o in outs:
                a = p = None
                if len(o) < 4 or o[3]:
                    a = np.empty(o[1], _NP[o[2]])
                    p = a.ctypes.data_as(_CTYPE[o[2]])
                out.append(a)
                pout.append(p)
            return
        torch, in_dtypes, out_dtypes = _torch_kinds()
        if lead_t:
            dev = lead[1].device
            if dev.type != "cuda":
                raise ValueError("%s must be on a GPU, got %s" % (lead[0], dev) if texels else "torch tensors must be on the GPU, %s is on %s" % (lead[0], dev))
            if device is not None and device is not CURRENT and torch.device(device).index not in (None, dev.index):
                raise ValueError("%s is on %s, device is %s" % (lead[0], dev, device))
        else:  # numpy arguments on their way to a GPU: converted as the numpy form converts them, before the device is touched
            for c in cols:
                if _is_tensor(c[1]):
                    raise ValueError("%s: %s" % (c[0], _MIXED) if texels else _MIXED)
            cols = [(c[0], None if c[1] is None else _np_column(c[0], c[1], c[2]), c[2]) for c in cols]
            dev = torch.device("cuda", torch.cuda.current_device()) if device is CURRENT else torch.device(device)
            if dev.type != "cuda":
                raise ValueError("device must be a GPU, got %s" % dev)
        ins = []
        for c in cols:
            name, t, kind = c[0], c[1], c[2]
            if t is not None:
                if not _is_tensor(t):
                    if lead_t:
                        if len(c) < 4 or not c[3]:
                            raise ValueError("%s: %s" % (name, _MIXED))
                        t = _np_column(name, t, kind)
                    t = torch.from_numpy(t.view(_SIGNED[kind]) if kind in _SIGNED else t).to(dev)
                    if not ins:
                        dev = t.device  # (the lead's: "cuda" has become "cuda:0")
                if t.dtype not in in_dtypes[kind]:
                    raise ValueError("%s must be %s, got %s" % (name, " or ".join(str(d) for d in in_dtypes[kind]), t.dtype))
                if t.device != dev:
                    raise ValueError("%s is on %s, origins on %s" % (name, t.device, dev))
                t = t.contiguous()
            ins.append(t)
        self.device, self.ins = dev, ins
        self.outs = [torch.empty(o[1], dtype=out_dtypes[o[2]], device=dev) if len(o) < 4 or o[3] else None for o in outs]
        self.ptr = self.addr = _tensor_ptr
        self.pin, self.pout = [_tensor_ptr(x) for x in ins], [_tensor_ptr(x) for x in self.outs]

    def call(self, scene, name, *args, ex=False):
        """lib.<name>(handle, *args) in the numpy form, lib.<name>_device(handle, *args, stream) on the tensors' GPU in the torch form; `ex`: the _ex symbol."""
        lib = abi.load_hip_lib()
        if self.device is None:
            abi.check(getattr(lib, name + "_ex" if ex else name)(scene.device_handle(), *args))
            return
        cuda = _torch[0].cuda
        with cuda.device(self.device):
            abi.check(getattr(lib, name + ("_device_ex" if ex else "_device"))(scene.device_handle(), *args, cuda.current_stream().cuda_stream))


# ---- what scene.py and restated.py share: small checkers, bounds, the texture modes and the texel record --------------------------------------------------------

def _is_tensor(x):
    return type(x).__module__.split(".")[0] == "torch"


def _n_of(origins, dirs, names=("origins", "dirs")):
    """Number of rays of an (n, 3) origins / directions pair (numpy arrays or torch tensors), checked before any device work."""
    for name, a in zip(names, (origins, dirs)):
        if a is None:
            raise ValueError("%s is required" % name)
        if len(a.shape) != 2 or a.shape[1] != 3:
            raise ValueError("%s must have shape (n, 3), got %s" % (name, tuple(a.shape)))
    if origins.shape[0] != dirs.shape[0]:
        raise ValueError("%s and %s hold %d and %d rays" % (names[0], names[1], origins.shape[0], dirs.shape[0]))
    n = int(origins.shape[0])
    if n >= 1 << 32:
        raise ValueError("at most 2^32 - 1 rays per call")
    return n


def _check_vec(name, a, n):
    if a is not None and (len(a.shape) != 1 or a.shape[0] != n):
        raise ValueError("%s must have shape (%d,), got %s" % (name, n, tuple(a.shape)))


def _np_floats(name, a, dtype):
    a = np.asarray(a)
    if not np.issubdtype(a.dtype, np.floating):
        raise ValueError("%s must be floating point, got %s" % (name, a.dtype))
    return np.ascontiguousarray(a, dtype=dtype)


def _np_keys(keys):
    k = np.asarray(keys)
    if not np.issubdtype(k.dtype, np.integer):
        raise ValueError("keys must be integers, got %s" % k.dtype)
    return np.ascontiguousarray(k.astype(np.uint64, copy=False))


def _check_rows(name, a, n, cols):
    if len(a.shape) != 2 or a.shape[0] != n or a.shape[1] != cols:
        raise ValueError("%s must have shape (%d, %d), got %s" % (name, n, cols, tuple(a.shape)))


def _np_ints(name, a, dtype):
    """An integer numpy array as `dtype`: int32 keeps out-of-range node indices out of range (clipped), uint32 keeps the low 32 bits (flag words)."""
    a = np.asarray(a)
    if not np.issubdtype(a.dtype, np.integer):
        raise ValueError("%s must be integers, got %s" % (name, a.dtype))
    if dtype == np.int32 and a.dtype != np.int32:
        a = np.clip(a, -(1 << 31), (1 << 31) - 1)
    return np.ascontiguousarray(a.astype(dtype, copy=False))


OCCLUSION_MAX_TABLE = 1024


def _occlusion_tables(sample_dirs, rotations, bias, max_toi):
    """The two tables as contiguous float64 numpy arrays (or the torch tensors they came as), checked against NraysOcclusionParams' bounds."""
    def table(name, a, cols, lo):
        if not _is_tensor(a):
            a = np.asarray(a)
            if not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
                raise ValueError("%s must be numbers, got %s" % (name, a.dtype))
            a = np.ascontiguousarray(a, dtype=np.float64)
        if len(a.shape) != 2 or a.shape[1] != cols or not lo <= a.shape[0] <= OCCLUSION_MAX_TABLE:
            raise ValueError("%s must have shape (%d .. %d, %d), got %s" % (name, lo, OCCLUSION_MAX_TABLE, cols, tuple(a.shape)))
        return a
    if sample_dirs is None:
        raise ValueError("sample_dirs is required")
    L = table("sample_dirs", sample_dirs, 3, 1)
    rot = None if rotations is None else table("rotations", rotations, 2, 0)
    if rot is not None and rot.shape[0] == 0:
        rot = None
    bias, max_toi = float(bias), float(max_toi)
    if not math.isfinite(bias):
        raise ValueError("bias must be finite")
    if not max_toi > 0.0:
        raise ValueError("max_toi must be > 0 (inf allowed)")
    return L, rot, bias, max_toi


PointLights = collections.namedtuple("PointLights", ("positions", "colors", "normals", "inverse_square", "min_dist", "bias", "offset"), defaults=(None, False, 1e-3, 1e-3, 1e-3))
PointLights.__doc__ = """A table of point lights for light_points (NraysPointLights): `positions` (m, 3) float64, world space; `colors` (m, 3) float32; `normals` (m, 3) float64 unit
emitter normals (virtual point lights: vpls_from_hits()) or None: the lights shine every way; 1 <= m <= 4096.  `inverse_square`: the weight falls with
1 / max(d^2, min_dist^2).  `bias`: a lit point is moved along its normal by this first.  `offset`: the shadow ray starts this far towards the light and ends this far
before it."""


def _point_lights(lights):
    """The checks of NraysPointLights that need no library: (positions, colors, normals or None — contiguous numpy arrays of their kinds, or the torch tensors they came
    as —, flags, bias, offset, min_dist)."""
    if not isinstance(lights, tuple) or len(lights) != 7:
        raise ValueError("lights must be a PointLights(positions, colors, normals, inverse_square, min_dist, bias, offset)")
    positions, colors, normals, inverse_square, min_dist, bias, offset = lights

    def table(name, a, dtype):
        if a is None:
            raise ValueError("lights.%s is required" % name)
        if not _is_tensor(a):
            a = np.asarray(a)
            if not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
                raise ValueError("lights.%s must be numbers, got %s" % (name, a.dtype))
            a = np.ascontiguousarray(a, dtype=dtype)
        if len(a.shape) != 2 or a.shape[1] != 3 or not 1 <= a.shape[0] <= abi.LIGHTS_MAX:
            raise ValueError("lights.%s must have shape (1 .. %d, 3), got %s" % (name, abi.LIGHTS_MAX, tuple(a.shape)))
        return a
    pos, col = table("positions", positions, np.float64), table("colors", colors, np.float32)
    en = None if normals is None else table("normals", normals, np.float64)
    if col.shape[0] != pos.shape[0] or (en is not None and en.shape[0] != pos.shape[0]):
        raise ValueError("lights: positions, colors and normals must hold the same number of rows")
    bias, offset, min_dist = float(bias), float(offset), float(min_dist)
    if not math.isfinite(bias):
        raise ValueError("lights.bias must be finite")
    if not (math.isfinite(offset) and offset >= 0.0):
        raise ValueError("lights.offset must be finite and >= 0")
    if inverse_square and not (math.isfinite(min_dist) and min_dist > 0.0):
        raise ValueError("lights.min_dist must be finite and > 0 with inverse_square")
    return pos, col, en, abi.LIGHTS_INVERSE_SQUARE if inverse_square else 0, bias, offset, min_dist


SH_MAX_BANDS = 3


def _sh_bands(bands):
    if isinstance(bands, bool) or int(bands) != bands or not 1 <= int(bands) <= SH_MAX_BANDS:
        raise ValueError("bands must be 1, 2 or 3, got %r" % (bands,))
    return int(bands)


ProbeGrid = collections.namedtuple("ProbeGrid", ("origin", "cell", "counts", "sh", "valid", "measure"), defaults=(None, 4.0 * math.pi))
ProbeGrid.__doc__ = """A regular grid of SH probes (NraysIrradianceGrid): probe (ix, iy, iz) sits at origin + (ix, iy, iz) * cell and is row (iz * counts[1] + iy) * counts[0] + ix
of `sh` ((P, bands^2, 3) float32, what gather_probes returns at probe_grid_positions()); `valid` (P,) integers or None: bit 0 clear = the probe is never read;
`measure`: the solid angle of the probes' sample table."""


def _probe_lattice(origin, cell, counts):
    """origin, cell and counts of a ProbeGrid as tuples of plain numbers, checked against NraysIrradianceGrid's bounds."""
    vec = []
    for name, v in (("origin", origin), ("cell", cell), ("counts", counts)):
        v = np.asarray(v).reshape(-1)
        if v.shape != (3,) or not (np.issubdtype(v.dtype, np.integer) if name == "counts" else np.issubdtype(v.dtype, np.number)) or v.dtype == np.bool_:
            raise ValueError("grid.%s must be three %s" % (name, "integers" if name == "counts" else "numbers"))
        vec.append(v)
    origin, cell, counts = tuple(float(x) for x in vec[0]), tuple(float(x) for x in vec[1]), tuple(int(x) for x in vec[2])
    if not all(math.isfinite(x) for x in origin):
        raise ValueError("grid.origin must be finite")
    if not all(1 <= c <= abi.IRRADIANCE_MAX_COUNT for c in counts) or counts[0] * counts[1] * counts[2] > abi.IRRADIANCE_MAX_PROBES:
        raise ValueError("grid.counts must be in 1 .. %d with a product <= 2^22, got %s" % (abi.IRRADIANCE_MAX_COUNT, counts))
    if not all(c == 1 or (math.isfinite(x) and x > 0.0) for c, x in zip(counts, cell)):
        raise ValueError("grid.cell must be finite and > 0 on every axis with more than one probe, got %s" % (cell,))
    return origin, cell, counts


def _probe_grid(grid):
    """The checks of NraysIrradianceGrid that need no library: (origin, cell, counts, bands, sh, valid, measure) with plain Python numbers, sh a float32 array or
    tensor (P, bands^2, 3), valid None or integers of P words."""
    if not isinstance(grid, tuple) or len(grid) != 6:
        raise ValueError("grid must be a ProbeGrid(origin, cell, counts, sh, valid, measure)")
    origin, cell, counts, sh, valid, measure = grid
    origin, cell, counts = _probe_lattice(origin, cell, counts)
    probes = counts[0] * counts[1] * counts[2]
    if sh is None or not (_is_tensor(sh) or isinstance(sh, np.ndarray)):
        raise ValueError("grid.sh must be a float32 numpy array or torch tensor")
    coefs = sh.shape[-2] if len(sh.shape) >= 2 else 0
    if str(sh.dtype).split(".")[-1] != "float32" or coefs not in (1, 4, 9) or sh.shape[-1] != 3 or int(np.prod(tuple(sh.shape))) != probes * coefs * 3:
        raise ValueError("grid.sh must be float32 of shape (%d, 1 | 4 | 9, 3), got %s %s" % (probes, tuple(sh.shape), sh.dtype))
    if valid is not None:
        if not _is_tensor(valid):
            valid = np.asarray(valid)
            if valid.dtype == np.bool_:
                valid = valid.astype(np.uint32)
            if not np.issubdtype(valid.dtype, np.integer):
                raise ValueError("grid.valid must be integers, got %s" % valid.dtype)
        if int(np.prod(tuple(valid.shape))) != probes:
            raise ValueError("grid.valid must hold one word per probe (%d), got shape %s" % (probes, tuple(valid.shape)))
        valid = valid.reshape(-1)
    measure = float(measure)
    if not math.isfinite(measure) or abs(measure) > float(np.finfo(np.float32).max):
        raise ValueError("grid.measure must be a finite float32")
    return origin, cell, counts, {1: 1, 4: 2, 9: 3}[coefs], sh.reshape(probes, coefs, 3), valid, measure


ProbeVisibility = collections.namedtuple("ProbeVisibility", ("moments", "res", "floor", "bias"), defaults=(0.05, 0.0))
ProbeVisibility.__doc__ = """The depth moments of a ProbeGrid's probes (NraysIrradianceVisibility): `moments` (P, res^2, 2) float32, what probe_depth() returns at the grid's
probe_grid_positions(), rows as grid.sh; `res` 4, 8 or 16; `floor` in [0, 1]: the least visibility factor; `bias`: a point is moved along its normal by this before
its distance to a probe is taken."""


def _depth_res(res):
    if isinstance(res, bool) or int(res) != res or int(res) not in abi.PROBE_DEPTH_RES:
        raise ValueError("res must be 4, 8 or 16, got %r" % (res,))
    return int(res)


def _probe_visibility(vis, probes):
    """The checks of NraysIrradianceVisibility that need no library: (moments (P, res^2, 2) float32 array or tensor, res, floor, bias) with plain Python numbers."""
    if not isinstance(vis, tuple) or len(vis) != 4:
        raise ValueError("visibility must be a ProbeVisibility(moments, res, floor, bias)")
    moments, res, floor, bias = vis
    res = _depth_res(res)
    if moments is None or not (_is_tensor(moments) or isinstance(moments, np.ndarray)):
        raise ValueError("visibility.moments must be a float32 numpy array or torch tensor")
    if str(moments.dtype).split(".")[-1] != "float32" or int(np.prod(tuple(moments.shape))) != probes * res * res * 2:
        raise ValueError("visibility.moments must be float32 of shape (%d, %d, 2), got %s %s" % (probes, res * res, tuple(moments.shape), moments.dtype))
    floor, bias = float(floor), float(bias)
    if not 0.0 <= floor <= 1.0:
        raise ValueError("visibility.floor must be in [0, 1], got %r" % floor)
    if not math.isfinite(bias):
        raise ValueError("visibility.bias must be finite")
    return moments.reshape(probes, res * res, 2), res, floor, bias


class Interpolation:
    Bilinear = abi.INTERP_BILINEAR
    Nearest = abi.INTERP_NEAREST


class Overflow:
    Wrap = abi.OVERFLOW_WRAP
    ClampToEdges = abi.OVERFLOW_CLAMP


TEXEL_OUTPUTS = ("normals", "uv", "node", "prim")  # the optional outputs of surface_texels, in the order of nrays_surface_texels_device's arguments
SurfaceTexels = collections.namedtuple("SurfaceTexels", ("points",) + TEXEL_OUTPUTS + ("flags",))
TEXELS_MAX_SIDE, TEXELS_MAX_POINTS = 16384, 1 << 24


MATERIAL_OUTPUTS = ("ambient", "diffuse", "specular", "node")  # the outputs of material_points, in the order of nrays_material_points_device's arguments
MaterialTerms = collections.namedtuple("MaterialTerms", MATERIAL_OUTPUTS)
NEAREST_OUTPUTS = ("point", "normal", "uv", "prim", "flags")  # the optional outputs of nearest_points, in the order of nrays_nearest_points_device's arguments
NearestHits = collections.namedtuple("NearestHits", ("dist", "node") + NEAREST_OUTPUTS)  # closest_hits' record with `dist` for `toi`, plus `point`
NEAREST_BEHIND = 4  # flag bit 2 of a nearest-surface record: the query point lies behind the surface
MaterialTerms.__doc__ = """What material_points returns: `ambient` (n, 4) float32, Material::ambiant; `diffuse` (n, 3) float32, kd * texture; `specular` (n, 4) float32, (ks, shininess);
`node` (n, 4) float64, the node's (alpha, refl_mix, refl_atenuation, refr_coeff).  None for what was not asked for."""


def _material_args(node_ids, normals, uvs, hit_flags, want):
    """The checks material_points and material_points_ref share: (n, want as a tuple)."""
    if node_ids is None:
        raise ValueError("nodes is required")
    if len(node_ids.shape) != 1:
        raise ValueError("nodes must have shape (n,), got %s" % (tuple(node_ids.shape),))
    if not _is_tensor(node_ids) and not np.issubdtype(np.asarray(node_ids).dtype, np.integer):
        raise ValueError("nodes must be integers, got %s" % np.asarray(node_ids).dtype)
    n = int(node_ids.shape[0])
    if n >= 1 << 32:
        raise ValueError("at most 2^32 - 1 points per call")
    if isinstance(want, str):
        raise ValueError("want must be a sequence of names, got %r" % (want,))
    want = tuple(want)
    for name in want:
        if name not in MATERIAL_OUTPUTS:
            raise ValueError("want: unknown output %r (one of %s)" % (name, ", ".join(MATERIAL_OUTPUTS)))
    if not want:
        raise ValueError("want: at least one of %s" % ", ".join(MATERIAL_OUTPUTS))
    if normals is None and "ambient" in want:
        raise ValueError("normals is required for the ambient term (the Normal material reads it)")
    if normals is not None:
        _check_rows("normals", normals, n, 3)
    if uvs is not None:
        _check_rows("uvs", uvs, n, 2)
    _check_vec("hit_flags", hit_flags, n)
    return n, want


def _texel_lattice(width, height):
    width, height = int(width), int(height)
    if not (1 <= width <= TEXELS_MAX_SIDE and 1 <= height <= TEXELS_MAX_SIDE and width * height <= TEXELS_MAX_POINTS):
        raise ValueError("width and height must be in 1 .. %d and width * height <= 2^24, got %d x %d" % (TEXELS_MAX_SIDE, width, height))
    return width, height


def _dilate_args(flags, width, height, radius, values):
    """Checks shared by dilate_texels and dilate_texels_ref: (width, height, radius, channels); channels 0 without values."""
    width, height = _texel_lattice(width, height)
    radius = int(radius)
    if not 1 <= radius <= abi.DILATE_MAX_RADIUS:
        raise ValueError("radius must be in 1 .. %d, got %d" % (abi.DILATE_MAX_RADIUS, radius))
    n = width * height
    if int(np.prod(tuple(flags.shape))) != n:
        raise ValueError("flags must hold width * height = %d words, got shape %s" % (n, tuple(flags.shape)))
    channels = 0
    if values is not None:
        size = int(np.prod(tuple(values.shape)))
        channels = size // n
        if channels * n != size or not 1 <= channels <= 4:
            raise ValueError("values must hold 1 .. 4 floats per lattice point (%d points), got shape %s" % (n, tuple(values.shape)))
    return width, height, radius, channels


def _filter_args(flags, width, height, points, normals, values, step, pos_radius, normal_cos):
    """Checks shared by filter_texels, filter_texels_ref and denoise_texels: (width, height, step, pos_radius, normal_cos, channels)."""
    width, height = _texel_lattice(width, height)
    step, pos_radius, normal_cos = int(step), float(pos_radius), float(normal_cos)
    if not 1 <= step <= abi.FILTER_MAX_STEP:
        raise ValueError("step must be in 1 .. %d, got %d" % (abi.FILTER_MAX_STEP, step))
    if not pos_radius > 0.0:
        raise ValueError("pos_radius must be > 0 (math.inf: no position weight), got %r" % pos_radius)
    if not -1.0 <= normal_cos < 1.0:
        raise ValueError("normal_cos must be in [-1, 1), got %r" % normal_cos)
    n = width * height
    for name, a, per in (("flags", flags, 1), ("points", points, 3), ("normals", normals, 3)):
        if a is None:
            raise ValueError("%s is required" % name)
        if int(np.prod(tuple(a.shape))) != n * per:
            raise ValueError("%s must hold %d x width * height = %d words, got shape %s" % (name, per, n * per, tuple(a.shape)))
    if values is None:
        raise ValueError("values is required")
    size = int(np.prod(tuple(values.shape)))
    channels = size // n
    if channels * n != size or not 1 <= channels <= 4:
        raise ValueError("values must hold 1 .. 4 floats per lattice point (%d points), got shape %s" % (n, tuple(values.shape)))
    return width, height, step, pos_radius, normal_cos, channels
