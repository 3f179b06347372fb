"""The library's definitions restated in plain numpy, bit for bit where their docstrings say so: the references the tests compare the device against, and the
sample tables and camera rays that feed the calls of scene.py.  Nothing here touches the library or a GPU.  scene.py re-exports every name."""
import math

import numpy as np

from . import abi
from .marshal import (NEAREST_BEHIND, NearestHits, OCCLUSION_MAX_TABLE, Interpolation, MaterialTerms, Overflow, SurfaceTexels, _check_vec, _dilate_args, _filter_args, _is_tensor, _n_of, _np_floats, _np_keys,
                      _depth_res, _material_args, _np_ints, _occlusion_tables, _point_lights, _probe_grid, _probe_lattice, _probe_visibility, _sh_bands, _texel_lattice)

SALT_OCCLUSION = 0x300 << 32  # kSaltOcclusion (csrc/trace_device.h)
SALT_GATHER = 0x301 << 32  # kSaltGather (csrc/trace_device.h)


_U64 = (1 << 64) - 1
def _rng_mix(z):
    z = z ^ (z >> np.uint64(30))
    z = z * np.uint64(0xbf58476d1ce4e5b9)
    z = z ^ (z >> np.uint64(27))
    z = z * np.uint64(0x94d049bb133111eb)
    return z ^ (z >> np.uint64(31))


def _rng_hash(key, salt):
    """The library's counter-based RNG on uint64 arrays: mix((key ^ salt * golden) + c), wrapping.  `salt`: an int or a uint64 array."""
    with np.errstate(over="ignore"):
        if isinstance(salt, np.ndarray):
            s = salt.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        else:
            s = np.uint64((int(salt) * 0x9E3779B97F4A7C15) & _U64)
        return _rng_mix((np.asarray(key, dtype=np.uint64) ^ s) + np.uint64(0xD1B54A32D192ED03))


def camera_rays(resolution, camera_eye, projection, ray_per_pixel=1, window_width=0.0, seed=0):
    """The rays scene::render traces (src/scene.rs:67-89), for trace_rays: returns (origins (n, 3) float64, dirs (n, 3) float64,
    keys (n,) uint64) with n = width * height * ray_per_pixel, pixel-major (pixel i + j * width) with the samples innermost.
    Same f64 operations in the same order as a render: jitter (window_width), NDC, unprojection by the column-major inverse
    projection-view matrix, v / sqrt(x^2 + y^2 + z^2); key = hash(hash(hash(seed, pixel), sample), path salt).  Averaging the traced
    colours of a pixel's samples in order (f32 sum, then / ray_per_pixel) gives render()'s pixel."""
    from .math3d import column_major16
    w, h, spp = int(resolution[0]), int(resolution[1]), int(ray_per_pixel)
    if w <= 0 or h <= 0 or spp <= 0:
        raise ValueError("empty resolution or ray_per_pixel <= 0")
    M = [float(x) for x in column_major16(projection)]
    eye0 = [float(x) for x in camera_eye]
    pix = np.repeat(np.arange(w * h, dtype=np.uint64), spp)
    s = np.tile(np.arange(spp, dtype=np.uint64), w * h)
    i = (pix % np.uint64(w)).astype(np.float64)
    j = (pix // np.uint64(w)).astype(np.float64)
    pkey = _rng_hash(np.full(pix.shape, int(seed) & _U64, dtype=np.uint64), pix)
    skey = _rng_hash(pkey, s)
    ox, oy = i, j
    if float(window_width) != 0.0:  # scene.rs:74-76
        u0 = (_rng_hash(skey, 0x1000) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
        u1 = (_rng_hash(skey, 0x1001) >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)
        ox = ox + (u0 - 0.5) * float(window_width)
        oy = oy + (u1 - 0.5) * float(window_width)
    dx = (ox / float(w) - 0.5) * 2.0
    dy = -(oy / float(h) - 0.5) * 2.0
    hv = [M[r] * dx + M[4 + r] * dy + M[8 + r] * -1.0 + M[12 + r] * 1.0 for r in range(4)]
    v = [hv[a] / hv[3] - eye0[a] for a in range(3)]
    nrm = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    dirs = np.stack([v[0] / nrm, v[1] / nrm, v[2] / nrm], axis=1)
    origins = np.empty_like(dirs)
    origins[:] = eye0
    keys = _rng_hash(skey, 2)  # RNG_SALT_PATH
    return origins, dirs, keys


def hemisphere_dirs(k, cosine=True):
    """k sample directions of the local frame of occlusion_points (z = the normal), (k, 3) float64, unit length, z > 0: a golden-angle spiral,
    cosine-weighted (the mean filter then IS the cosine-weighted ambient term) or uniform over the hemisphere.  A convenience: any values are valid."""
    k = int(k)
    if k < 1 or k > OCCLUSION_MAX_TABLE:
        raise ValueError("k must be in 1 .. %d" % OCCLUSION_MAX_TABLE)
    u = (np.arange(k, dtype=np.float64) + 0.5) / k
    z = np.sqrt(1.0 - u) if cosine else 1.0 - u
    r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    phi = np.arange(k, dtype=np.float64) * (math.pi * (3.0 - math.sqrt(5.0)))
    d = np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)
    return d / np.sqrt((d * d).sum(axis=1))[:, None]


def rotation_table(m):
    """m rotations about the normal, evenly spaced, as the (m, 2) float64 table of (cos, sin) pairs occlusion_points picks from per point."""
    m = int(m)
    if m < 1 or m > OCCLUSION_MAX_TABLE:
        raise ValueError("m must be in 1 .. %d" % OCCLUSION_MAX_TABLE)
    a = np.arange(m, dtype=np.float64) * (2.0 * math.pi / m)
    return np.stack([np.cos(a), np.sin(a)], axis=1)


def sphere_dirs(k):
    """k directions spread over the whole sphere, (k, 3) float64 — a probe's sample table for gather_probes(): Fibonacci points, with t = i + 0.5:
    z = 1 - 2 t / k, r = sqrt(1 - z^2), phi = t * pi (3 - sqrt 5), direction (r cos phi, r sin phi, z).  A convenience: any values are valid."""
    k = int(k)
    if k < 1 or k > OCCLUSION_MAX_TABLE:
        raise ValueError("k must be in 1 .. %d" % OCCLUSION_MAX_TABLE)
    t = np.arange(k, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * t / k
    r = np.sqrt(1.0 - z * z)
    phi = t * (math.pi * (3.0 - math.sqrt(5.0)))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)


def occlusion_rays(points, normals, sample_dirs, rotations=None, bias=1e-3, keys=None):
    """The numpy mirror of the rays nrays_occlusion_points* builds on the device, bit for bit (include/nrays_abi.h: NraysOcclusionParams — f64 + - * /,
    copysign and integer arithmetic, products left to right).  Returns (origins (n, k, 3), dirs (n, k, 3)) float64: ray j of point i at [i, j].
    `keys` (n,) integers, default arange(n): only the rotation pick reads them."""
    n = _n_of(points, normals, ("points", "normals"))
    _check_vec("keys", keys, n)
    L, rot, bias, _ = _occlusion_tables(sample_dirs, rotations, bias, math.inf)
    if _is_tensor(points) or _is_tensor(normals) or _is_tensor(L) or _is_tensor(rot) or _is_tensor(keys):
        raise ValueError("occlusion_rays takes numpy arrays")
    p, nm = _np_floats("points", points, np.float64), _np_floats("normals", normals, np.float64)
    k = np.arange(n, dtype=np.uint64) if keys is None else _np_keys(keys)
    nx, ny, nz = nm[:, 0], nm[:, 1], nm[:, 2]
    with np.errstate(all="ignore"):
        s = np.copysign(1.0, nz)
        a = -1.0 / (s + nz)
        b = nx * ny * a
        t = (1.0 + s * nx * nx * a, s * b, -s * nx)
        u = (b, s + ny * ny * a, -ny)
        lx, ly, lz = (np.broadcast_to(L[:, c], (n, len(L))) for c in range(3))
        if rot is None:
            x, y = lx, ly
        else:
            r = (_rng_hash(k, SALT_OCCLUSION) % np.uint64(len(rot))).astype(np.int64)
            c_r, s_r = rot[r, 0][:, None], rot[r, 1][:, None]
            x, y = c_r * lx - s_r * ly, s_r * lx + c_r * ly
        dirs = np.stack([(x * t[q][:, None] + y * u[q][:, None]) + lz * nm[:, q][:, None] for q in range(3)], axis=2)
        o = p + nm * bias
    origins = np.ascontiguousarray(np.broadcast_to(o[:, None, :], dirs.shape))
    return origins, np.ascontiguousarray(dirs)


def light_rays(points, normals, lights):
    """The numpy mirror of the shadow rays and weights nrays_light_points* builds on the device, bit for bit (include/nrays_abi.h: NraysPointLights — f64 + - * / and
    sqrt, f32 *, products left to right).  `lights`: a PointLights of numpy tables.  Returns (origins (n, m, 3) float64, dirs (n, m, 3) float64, t_max (n, m) float64,
    w (n, m) float32): the ray of (point i, light k) at [i, k]; w == 0 marks a skipped light — one at the biased point itself has origin q, direction 0 and t_max 0, every
    other skipped light the origin, direction and t_max of the definition."""
    n = _n_of(points, normals, ("points", "normals"))
    pos, col, en, flags, bias, offset, min_dist = _point_lights(lights)
    if _is_tensor(points) or _is_tensor(normals) or _is_tensor(pos) or _is_tensor(col) or _is_tensor(en):
        raise ValueError("light_rays takes numpy arrays")
    p, nm = _np_floats("points", points, np.float64), _np_floats("normals", normals, np.float64)
    zero = np.float32(0.0)
    with np.errstate(all="ignore"):
        q = (p + nm * bias)[:, None, :]
        v = pos[None, :, :] - q
        vx, vy, vz = v[..., 0], v[..., 1], v[..., 2]
        nrm = np.sqrt((vx * vx + vy * vy) + vz * vz)
        there = nrm > 0.0
        ldir = v / nrm[..., None]
        lx, ly, lz = ldir[..., 0], ldir[..., 1], ldir[..., 2]
        cr = ((lx * nm[:, None, 0] + ly * nm[:, None, 1]) + lz * nm[:, None, 2]).astype(np.float32)
        cr = np.where(cr > zero, cr, zero)
        ce = np.ones_like(cr)
        if en is not None:
            ce = (-((lx * en[None, :, 0] + ly * en[None, :, 1]) + lz * en[None, :, 2])).astype(np.float32)
            ce = np.where(ce > zero, ce, zero)
        g = np.ones_like(cr)
        if flags & abi.LIGHTS_INVERSE_SQUARE:
            g = (1.0 / np.maximum(nrm * nrm, min_dist * min_dist)).astype(np.float32)
        w = (cr * ce) * g
        w = np.where(there & (w > zero), w, zero).astype(np.float32)
        origins = np.where(there[..., None], q + ldir * offset, np.broadcast_to(q, ldir.shape))
        dirs = np.where(there[..., None], ldir, 0.0)
        t_max = np.where(there, nrm - offset, 0.0)
    return np.ascontiguousarray(origins), np.ascontiguousarray(dirs), np.ascontiguousarray(t_max), np.ascontiguousarray(w)


def gather_ray_keys(keys, k):
    """The RNG keys of the rays gather_points traces: (n, k) uint64, entry [i, j] = hash(keys[i], (0x301 << 32) + j) — ray j of the point whose key is keys[i]
    (include/nrays_abi.h: NraysGatherParams).  With occlusion_rays() it restates gather_points from trace_rays."""
    k = int(k)
    if k < 1 or k > OCCLUSION_MAX_TABLE:
        raise ValueError("k must be in 1 .. %d" % OCCLUSION_MAX_TABLE)
    if _is_tensor(keys):
        raise ValueError("gather_ray_keys takes a numpy array")
    keys = _np_keys(keys)
    if keys.ndim != 1:
        raise ValueError("keys must have shape (n,), got %s" % (keys.shape,))
    salts = np.uint64(SALT_GATHER) + np.arange(k, dtype=np.uint64)
    return _rng_hash(np.broadcast_to(keys[:, None], (len(keys), k)), np.broadcast_to(salts[None, :], (len(keys), k)).copy())


# 1/(2 sqrt(pi)), sqrt(3)/(2 sqrt(pi)), sqrt(15)/(2 sqrt(pi)), sqrt(5)/(4 sqrt(pi)), sqrt(15)/(4 sqrt(pi)): the nearest doubles, as the header spells them
SH_K = (0.28209479177387814, 0.4886025119029199, 1.0925484305920792, 0.31539156525252005, 0.5462742152960396)
SH_COSINE_LOBE = (math.pi, 2.0 * math.pi / 3.0, math.pi / 4.0)  # A_l of Ramamoorthi and Hanrahan 2001, bands 0 .. 2


def _sh_terms(x, y, z, C):
    """The first C basis values at (x, y, z), each an array like x: the nine expressions of the header, left to right as written (numpy or torch, any dtype)."""
    K0, K1, K2, K3, K4 = SH_K
    Y = [K0 + 0.0 * x]
    if C >= 4:
        Y += [K1 * y, K1 * z, K1 * x]
    if C >= 9:
        Y += [(K2 * x) * y, (K2 * y) * z, K3 * ((3.0 * z) * z - 1.0), (K2 * x) * z, K4 * (x * x - y * y)]
    return Y


def sh_basis(dirs, bands=3):
    """The numpy mirror of the basis of nrays_gather_sh_points*: (..., 3) float64 directions, used as given -> (..., bands^2) float32 — the real spherical
    harmonics without the Condon-Shortley sign, evaluated in float64 left to right as the header writes them and rounded once."""
    bands = _sh_bands(bands)
    if _is_tensor(dirs):
        raise ValueError("sh_basis takes a numpy array")
    d = np.asarray(dirs, dtype=np.float64)
    if d.ndim < 1 or d.shape[-1] != 3:
        raise ValueError("dirs must have shape (..., 3), got %s" % (d.shape,))
    with np.errstate(all="ignore"):
        return np.stack(_sh_terms(d[..., 0], d[..., 1], d[..., 2], bands * bands), axis=-1).astype(np.float32)


def sh_fold_ref(ray_dirs, ray_colours, bands=3):
    """The numpy mirror of the fold of nrays_gather_sh_points*: ray_dirs (n, k, 3) float64 (occlusion_rays()' directions), ray_colours (n, k, 3) float32 (what
    trace_rays returns for them) -> (n, bands^2, 3) float32: acc = acc + float32(Y_c) * colour in float32 in the order of j, then acc / float32(k)."""
    d, col = np.asarray(ray_dirs, dtype=np.float64), np.asarray(ray_colours)
    if col.dtype != np.float32:
        raise ValueError("ray_colours must be float32, got %s" % col.dtype)
    if d.ndim != 3 or d.shape[2] != 3 or d.shape[1] < 1 or col.shape != d.shape:
        raise ValueError("ray_dirs and ray_colours must both have shape (n, k >= 1, 3), got %s and %s" % (d.shape, col.shape))
    y = sh_basis(d, bands)
    acc = np.zeros((d.shape[0], y.shape[2], 3), np.float32)
    with np.errstate(all="ignore"):
        for j in range(d.shape[1]):
            acc = acc + y[:, j, :, None] * col[:, j, None, :]
        return acc / np.float32(d.shape[1])


def sh_irradiance(sh, normals, measure=4.0 * math.pi):
    """The irradiance E(n) = measure * sum_lm A_l sh_lm Y_lm(n) with A = pi, 2 pi / 3, pi / 4 (Ramamoorthi and Hanrahan 2001) from the coefficients gather_sh_points /
    gather_probes return: sh (..., C, 3) with C = 1, 4 or 9, normals (..., 3) unit vectors whose leading shape broadcasts against sh's -> (..., 3).  `measure`: the
    solid angle the sample table covers — 4 pi for sphere_dirs (the default), 2 pi for a uniform hemisphere.  Plain numpy or torch arithmetic, no kernel."""
    C = sh.shape[-2] if len(sh.shape) >= 2 else 0
    if C not in (1, 4, 9) or sh.shape[-1] != 3 or normals.shape[-1] != 3:
        raise ValueError("sh must have shape (..., 1 | 4 | 9, 3) and normals (..., 3), got %s and %s" % (tuple(sh.shape), tuple(normals.shape)))
    if _is_tensor(sh) != _is_tensor(normals):
        raise ValueError("torch tensors and numpy arrays cannot be mixed in one call")
    Y = _sh_terms(normals[..., 0], normals[..., 1], normals[..., 2], C)
    band = (0, 1, 1, 1, 2, 2, 2, 2, 2)
    e = None
    for c in range(C):
        term = (SH_COSINE_LOBE[band[c]] * Y[c])[..., None] * sh[..., c, :]
        e = term if e is None else e + term
    return measure * e


def probe_grid_positions(origin, cell, counts):
    """The positions of a ProbeGrid's probes, (P, 3) float64 in the grid's row order (x fastest, then y, then z): origin + index * cell, one product and one sum
    per axis — the q of nrays_irradiance_points_device's facing factor, bit for bit."""
    origin, cell, counts = _probe_lattice(origin, cell, counts)
    axes = [origin[a] + np.arange(counts[a], dtype=np.float64) * (cell[a] if counts[a] > 1 else 0.0) for a in range(3)]
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return np.ascontiguousarray(np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], axis=1))


def oct_texel(dirs, res):
    """The numpy mirror of the texel function of nrays_probe_depth_points* (include/nrays_abi.h): (..., 3) float64 directions, used as given -> (...) uint32 texel
    indices ty * res + tx of the res x res octahedral map.  Scaling a direction by a power of two does not change its texel; a zero or NaN direction gives the
    middle texel (res / 2, res / 2)."""
    R = _depth_res(res)
    if _is_tensor(dirs):
        raise ValueError("oct_texel takes a numpy array")
    d = np.asarray(dirs, dtype=np.float64)
    if d.ndim < 1 or d.shape[-1] != 3:
        raise ValueError("dirs must have shape (..., 3), got %s" % (d.shape,))
    x, y, z = d[..., 0], d[..., 1], d[..., 2]

    def axis(a):
        g = (a * 0.5 + 0.5) * float(R)
        pos = g > 0.0
        return np.where(pos, np.minimum(np.where(pos, g, 0.0).astype(np.int64), R - 1), 0)
    with np.errstate(all="ignore"):
        s = (np.abs(x) + np.abs(y)) + np.abs(z)
        some = s > 0.0
        den = np.where(some, s, 1.0)
        a, b = np.where(some, x / den, 0.0), np.where(some, y / den, 0.0)
        below = z < 0.0
        a, b = (np.where(below, (1.0 - np.abs(b)) * np.copysign(1.0, a), a), np.where(below, (1.0 - np.abs(a)) * np.copysign(1.0, b), b))
        return (axis(b) * R + axis(a)).astype(np.uint32)


PROBE_NO_DIR = 0xFFFFFFFF  # nearest_dir of a point none of whose rays hit


def probe_depth_ref(ray_dirs, tois, hit, res=8, max_dist=None, near_dist=0.0, hit_flags=None):
    """The numpy mirror of the fold of nrays_probe_depth_points*, bit for bit: ray_dirs (n, k, 3) float64 (occlusion_rays()' directions), tois (n, k) float64 and
    hit (n, k) booleans or flag words with bit 0 (closest_hits' toi and flags for those rays) -> (moments (n, res^2, 2) float32, counts (n, 2) uint32, nearest (n,)
    float64, nearest_dir (n,) uint32).  dist = toi * |d| in float64 (+inf at a miss), clamped to max_dist and rounded to float32; per texel of oct_texel(d) the
    float32 sums of rf and rf * rf in the order of j over the count, or (max_dist, max_dist^2) where no ray fell.  hit_flags (n,): bit 0 clear skips a point."""
    R = _depth_res(res)
    if max_dist is None:
        raise ValueError("max_dist is required")
    max_dist, near_dist = float(max_dist), float(near_dist)
    if not (math.isfinite(max_dist) and max_dist > 0.0):
        raise ValueError("max_dist must be finite and > 0")
    if not (math.isfinite(near_dist) and near_dist >= 0.0):
        raise ValueError("near_dist must be finite and >= 0")
    d, toi, hit = np.asarray(ray_dirs, dtype=np.float64), np.asarray(tois, dtype=np.float64), np.asarray(hit)
    if d.ndim != 3 or d.shape[2] != 3 or d.shape[1] < 1 or toi.shape != d.shape[:2] or hit.shape != d.shape[:2]:
        raise ValueError("ray_dirs must have shape (n, k >= 1, 3), tois and hit (n, k), got %s, %s and %s" % (d.shape, toi.shape, hit.shape))
    n, k = toi.shape
    _check_vec("hit_flags", hit_flags, n)
    hit = hit if hit.dtype == np.bool_ else (hit.astype(np.uint64) & np.uint64(1)) != 0
    live = np.ones(n, bool) if hit_flags is None else (np.asarray(hit_flags).astype(np.uint64) & np.uint64(1)) != 0
    hit = hit & live[:, None]
    f32 = np.float32
    with np.errstate(all="ignore"):
        L = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
        dist = np.where(hit, toi * L, math.inf)
        rf = np.where(dist < max_dist, dist, max_dist).astype(f32)
        tex = oct_texel(d, R).astype(np.int64)
        s1, s2, cnt = np.zeros((n, R * R), f32), np.zeros((n, R * R), f32), np.zeros((n, R * R), np.int64)
        rows = np.arange(n)[live]
        for j in range(k):
            at = (rows, tex[rows, j])
            r = rf[rows, j]
            s1[at] = s1[at] + r
            s2[at] = s2[at] + r * r
            cnt[at] += 1
        some = cnt > 0
        fc = np.where(some, cnt, 1).astype(f32)
        moments = np.stack([np.where(some, s1 / fc, f32(max_dist)), np.where(some, s2 / fc, f32(max_dist) * f32(max_dist))], axis=2).astype(f32)
        counts = np.stack([((dist < near_dist) & live[:, None]).sum(axis=1), (~hit & live[:, None]).sum(axis=1)], axis=1).astype(np.uint32)
        nearest = dist.min(axis=1)
        nearest_dir = np.where(nearest < math.inf, np.argmin(dist, axis=1), PROBE_NO_DIR).astype(np.uint32)
    return moments, counts, nearest, nearest_dir


def irradiance_points_ref(points, normals, grid, facing=False, hit_flags=None, visibility=None):
    """The numpy mirror of nrays_irradiance_points*, bit for bit (include/nrays_abi.h: NraysIrradianceGrid — cell coordinates, the facing factor and the basis at
    the normal in float64, weights and folds in float32, every product and sum rounded on its own, left to right as the header writes them).  `grid`: a ProbeGrid of
    numpy arrays.  `visibility`: a ProbeVisibility of numpy arrays — the mirror of nrays_irradiance_points_vis*: per valid corner the Chebyshev factor from the probe's
    depth moments towards the point —, or None.  Returns (rgb (n, 3), sh (n, bands^2, 3), weight (n,)) float32: the three outputs of the call."""
    origin, cell, counts, bands, sh, valid, measure = _probe_grid(grid)
    vis = None if visibility is None else _probe_visibility(visibility, counts[0] * counts[1] * counts[2])
    if vis is not None and _is_tensor(vis[0]):
        raise ValueError("irradiance_points_ref takes numpy arrays")
    n = _n_of(points, normals, ("points", "normals"))
    _check_vec("hit_flags", hit_flags, n)
    if any(_is_tensor(a) for a in (points, normals, hit_flags, sh, valid)):
        raise ValueError("irradiance_points_ref takes numpy arrays")
    p, nm = _np_floats("points", points, np.float64), _np_floats("normals", normals, np.float64)
    live = np.ones(n, bool) if hit_flags is None else (np.asarray(hit_flags).astype(np.uint64) & np.uint64(1)) != 0
    C_ = bands * bands
    f32, one = np.float32, np.float32(1.0)
    cell = tuple(cell[a] if counts[a] > 1 else 0.0 for a in range(3))
    if valid is not None:
        valid = (np.asarray(valid).astype(np.uint64) & np.uint64(1)) != 0
    with np.errstate(all="ignore"):
        lo, hi, f = [], [], []
        for a in range(3):
            c = counts[a]
            if c == 1:
                g = np.zeros(n, np.float64)
            else:
                g = (p[:, a] - origin[a]) / cell[a]
                top = float(c - 1)
                g = np.where(g > 0.0, np.where(g < top, g, top), 0.0)
            i = np.minimum(g.astype(np.int64), max(c, 2) - 2)
            lo.append(i)
            hi.append(np.minimum(i + 1, c - 1))
            f.append((g - i.astype(np.float64)).astype(f32))
        w, rows = np.zeros((8, n), f32), np.zeros((8, n), np.int64)
        for k in range(8):
            d = (k & 1, (k >> 1) & 1, (k >> 2) & 1)
            idx = [hi[a] if d[a] else lo[a] for a in range(3)]
            X, Y, Z = (f[a] if d[a] else one - f[a] for a in range(3))
            wk = (X * Y) * Z
            if facing:
                v = [(origin[a] + idx[a].astype(np.float64) * cell[a]) - p[:, a] for a in range(3)]
                l2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
                c = (v[0] * nm[:, 0] + v[1] * nm[:, 1]) + v[2] * nm[:, 2]
                t = np.where(l2 > 0.0, (c / np.sqrt(l2) + 1.0) * 0.5, 1.0)
                wk = wk * (t * t + 0.2).astype(f32)
            rows[k] = (idx[2] * counts[1] + idx[1]) * counts[0] + idx[0]
            if valid is not None:
                wk = np.where(valid[rows[k]], wk, f32(0.0))
            if vis is not None:
                moments, R, floor, vbias = vis
                v = [(p[:, a] + nm[:, a] * vbias) - (origin[a] + idx[a].astype(np.float64) * cell[a]) for a in range(3)]
                l2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]
                m = moments[rows[k], oct_texel(np.stack(v, axis=1), R).astype(np.int64)]
                m1, m2, df = m[:, 0], m[:, 1], np.sqrt(l2).astype(f32)
                var = m2 - m1 * m1
                var = np.where(var > 0, var, f32(0.0))
                diff = df - m1
                den = var + diff * diff
                ch = np.where(den > 0, var / np.where(den > 0, den, one), f32(0.0))
                c3 = (ch * ch) * ch
                held = (l2 > 0.0) & (df > m1) & (True if valid is None else valid[rows[k]])
                wk = np.where(held, wk * np.where(c3 > f32(floor), c3, f32(floor)), wk).astype(f32)
            w[k] = wk
        wsum = np.zeros(n, f32)
        for k in range(8):
            wsum = wsum + w[k]
        lit = live & (wsum > 0)
        wn = w / np.where(lit, wsum, one)[None, :]
        s = np.zeros((n, C_, 3), f32)
        for k in range(8):
            use = lit & (wn[k] != 0)
            s[use] = s[use] + wn[k][use, None, None] * sh[rows[k][use]]
        Yn = _sh_terms(nm[:, 0], nm[:, 1], nm[:, 2], C_)
        Yn[0] = np.full(n, SH_K[0])
        band = (0, 1, 1, 1, 2, 2, 2, 2, 2)
        e = np.zeros((n, 3), f32)
        for c in range(C_):
            a_c = (SH_COSINE_LOBE[band[c]] * Yn[c]).astype(f32)
            e = e + a_c[:, None] * s[:, c, :]
        rgb = np.where(lit[:, None], f32(measure) * e, f32(0.0)).astype(f32)
    return rgb, s, np.where(live, wsum, f32(0.0)).astype(f32)


def texel_coords(n, centres=False):
    """The n lattice coordinates of one axis of surface_texels: x / (n - 1), where Texture2d::sample reads texel x (0.0 for n == 1), or the usual texel
    centres (x + 0.5) / n.  float64, one correctly rounded division each."""
    x = np.arange(n, dtype=np.float64)
    if centres:
        return (x + 0.5) / float(n)
    return x / float(n - 1) if n > 1 else np.zeros(1, dtype=np.float64)


def _texel_edge(pu, pv, qu, qv, su, sv):
    swapped = qu < pu or (qu == pu and qv < pv)
    if swapped:
        pu, pv, qu, qv = qu, qv, pu, pv
    e = (qu - pu) * (sv - pv) - (qv - pv) * (su - pu)
    return -e if swapped else e


def surface_texels_ref(points, indices, uvs, transform, width, height, centres=False, flip_normals=False, node=0, with_weights=False):
    """The numpy mirror of nrays_surface_texels_device's definition (include/nrays_abi.h), bit for bit: what surface_texels() returns for a scene node `node`
    whose geometry is TriMesh(points, indices, uvs) (coordinates and uvs exactly representable in float32, as a scene requires) under the Isometry3
    `transform` (None: the identity; the rotation is math3d.rotation_from_axis_angle's).  Every operation is a float64 + - * /, sqrt or comparison in the
    order the header writes it.  Returns SurfaceTexels of numpy arrays (flags uint32); with_weights=True: (texels, (n, 3) float64 barycentric weights
    w0, w1, w2, zeros where uncovered)."""
    from . import math3d
    width, height = _texel_lattice(width, height)
    P = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    I = np.asarray(indices).reshape(-1, 3).astype(np.int64)
    UV = np.asarray(uvs, dtype=np.float64).reshape(-1, 2)
    su, sv = texel_coords(width, centres), texel_coords(height, centres)
    n = width * height
    owner = np.full((height, width), -1, dtype=np.int64)
    pts, nrm, wts = np.zeros((height, width, 3)), np.zeros((height, width, 3)), np.zeros((height, width, 3))
    axis_angle = (0.0, 0.0, 0.0) if transform is None else tuple(transform.axis_angle)
    trans = (0.0, 0.0, 0.0) if transform is None else tuple(transform.translation)
    identity = axis_angle == (0.0, 0.0, 0.0)
    noxform = identity and trans == (0.0, 0.0, 0.0)
    R = math3d.rotation_from_axis_angle(axis_angle)
    rot = lambda x, y, z: [(float(R[k, 0]) * x + float(R[k, 1]) * y) + float(R[k, 2]) * z for k in range(3)]  # noqa: E731
    with np.errstate(all="ignore"):
        for t in range(len(I)):
            (au, av), (bu, bv), (cu, cv) = ((float(UV[v, 0]), float(UV[v, 1])) for v in I[t])
            area2 = np.float64(bu - au) * np.float64(cv - av) - np.float64(bv - av) * np.float64(cu - au)
            if area2 == 0.0 or not np.isfinite(area2):
                continue
            # the lattice points inside the triangle's uv box, by exact comparisons (the coordinates of an axis ascend)
            x0, x1 = int(np.searchsorted(su, min(au, bu, cu), "left")), int(np.searchsorted(su, max(au, bu, cu), "right"))
            y0, y1 = int(np.searchsorted(sv, min(av, bv, cv), "left")), int(np.searchsorted(sv, max(av, bv, cv), "right"))
            if x0 >= x1 or y0 >= y1:
                continue
            s = 1.0 if area2 > 0.0 else -1.0
            gu, gv = su[None, x0:x1], sv[y0:y1, None]
            e0, e1, e2 = s * _texel_edge(bu, bv, cu, cv, gu, gv), s * _texel_edge(cu, cv, au, av, gu, gv), s * _texel_edge(au, av, bu, bv, gu, gv)
            total = (e0 + e1) + e2
            win = (e0 >= 0.0) & (e1 >= 0.0) & (e2 >= 0.0) & (total != 0.0) & (owner[y0:y1, x0:x1] < 0)  # (ascending t: the smallest covering index wins)
            if not win.any():
                continue
            w0, w1, w2 = (e0 / total)[win], (e1 / total)[win], (e2 / total)[win]
            a, b, c = (P[v] for v in I[t])
            p = [(float(a[k]) * w0 + float(b[k]) * w1) + float(c[k]) * w2 for k in range(3)]
            ab, ac = [float(b[k]) - float(a[k]) for k in range(3)], [float(c[k]) - float(a[k]) for k in range(3)]
            cr = [ab[1] * ac[2] - ab[2] * ac[1], ab[2] * ac[0] - ab[0] * ac[2], ab[0] * ac[1] - ab[1] * ac[0]]
            norm = np.sqrt(np.float64(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]))
            nm = [float(np.float64(x) / norm) for x in cr]
            if not noxform:
                if identity:
                    p = [p[k] + trans[k] for k in range(3)]
                else:
                    p = [q + trans[k] for k, q in enumerate(rot(*p))]
                    nm = rot(*nm)
            if flip_normals:
                nm = [-x for x in nm]
            own = owner[y0:y1, x0:x1]; own[win] = t
            for k in range(3):
                pts[y0:y1, x0:x1, k][win] = p[k]
                nrm[y0:y1, x0:x1, k][win] = nm[k]
            wts[y0:y1, x0:x1, 0][win], wts[y0:y1, x0:x1, 1][win], wts[y0:y1, x0:x1, 2][win] = w0, w1, w2
    covered = (owner >= 0).reshape(n)
    uv = np.stack(np.broadcast_arrays(su[None, :], sv[:, None]), axis=-1).reshape(n, 2) * covered[:, None]
    out = SurfaceTexels(points=pts.reshape(n, 3), normals=nrm.reshape(n, 3), uv=np.ascontiguousarray(uv), node=np.where(covered, int(node), -1).astype(np.int32),
                        prim=owner.reshape(n).astype(np.int32), flags=np.where(covered, 3, 0).astype(np.uint32))
    return (out, wts.reshape(n, 3)) if with_weights else out


def dilate_texels_ref(flags, width, height, radius, values=None):
    """The numpy mirror of nrays_dilate_texels_device's definition (include/nrays_abi.h), bit for bit: what dilate_texels() returns, as
    (values, source int32 (n,), flags uint32 (n,)); `values` is a dilated COPY of the argument (None without one), the arguments stay as they are.
    Integers only.  Written the separable way: per row the nearest covered column (running maximum / minimum of the covered column indices, the left
    one on a tie), then rings |dy| = 1, 2, .. radius over the points that are still open — uncovered, and dy^2 not above the d2 they hold — so that the
    cost follows the gutters' area and depth, not radius x the lattice."""
    flags = np.asarray(flags)
    if not np.issubdtype(flags.dtype, np.integer):
        raise ValueError("flags must be integers, got %s" % flags.dtype)
    w, h, r, channels = _dilate_args(flags, width, height, radius, None if values is None else np.asarray(values))
    n, none = w * h, 1 << 20
    f = flags.astype(np.uint32, copy=False).reshape(h, w)
    cov = (f & np.uint32(1)) != 0
    x = np.arange(w, dtype=np.int64)[None, :]
    dl = x - np.maximum.accumulate(np.where(cov, x, -none), axis=1)
    dr = np.minimum.accumulate(np.where(cov, x, none)[:, ::-1], axis=1)[:, ::-1] - x
    dx = np.where(dl <= dr, -dl, dr)
    dx = np.where(np.minimum(dl, dr) <= r, dx, none).reshape(n)  # per point: the row pass's word
    i = np.arange(n, dtype=np.int64)
    y = i // w
    have = dx != none
    best_d2 = np.where(have, dx * dx, r * r + 1)
    best = np.where(have, i + dx, -1)
    active = np.flatnonzero(~cov.reshape(n))
    for k in range(1, r + 1):
        active = active[best_d2[active] >= k * k]
        if active.size == 0:
            break
        for sign in (-1, 1):  # the row above first: on equal (d2, index) nothing changes, and the comparison below is lexicographic anyway
            yy = y[active] + sign * k
            a = active[(yy >= 0) & (yy < h)]
            j = a + sign * k * w
            d = dx[j]
            keep = d != none
            a, j, d = a[keep], j[keep], d[keep]
            d2, idx = d * d + k * k, j + d
            better = (d2 < best_d2[a]) | ((d2 == best_d2[a]) & (idx < best[a]))
            a = a[better]
            best_d2[a], best[a] = d2[better], idx[better]
    filled = ~cov.reshape(n) & (best >= 0)
    out_flags = f.reshape(n) | np.where(filled, np.uint32(abi.TEXEL_FILLED), np.uint32(0))
    out_values = None
    if values is not None:
        v = np.asarray(values)
        if v.dtype != np.float32:
            raise ValueError("values must be float32, got %s" % v.dtype)
        out_values = np.array(v, order="C", copy=True)
        words = out_values.view(np.uint32).reshape(n, channels)
        words[filled] = words[best[filled]]
    return out_values, best.astype(np.int32), out_flags.astype(np.uint32)


def lightmap_sample_ref(texels, u, v, interp=Interpolation.Bilinear, overflow=Overflow.ClampToEdges):
    """The numpy float32 mirror of the sample nrays_gather_maps_points* takes from a map, bit for bit (include/nrays_abi.h: NraysGatherMapsParams — the value the
    library's materials get from a texture, Texture2d::sample): `texels` (height, width, 4) float32, row 0 = the bottom row; `u`, `v` (n,) coordinates (the float64
    uv of a hit record, converted to float32 first).  Every product and sum is a float32 operation of its own, in the header's order.  Returns (n, 4) float32."""
    t = np.asarray(texels)
    if t.ndim != 3 or t.shape[2] != 4 or t.dtype != np.float32 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError("texels must be a (height, width, 4) float32 array")
    if interp not in (Interpolation.Bilinear, Interpolation.Nearest) or overflow not in (Overflow.Wrap, Overflow.ClampToEdges):
        raise ValueError("unknown interp or overflow")
    F = np.float32
    h, w = t.shape[0], t.shape[1]
    with np.errstate(all="ignore"):
        c = [np.atleast_1d(np.asarray(a)).astype(F) for a in (u, v)]
        if c[0].shape != c[1].shape or c[0].ndim != 1:
            raise ValueError("u and v must have the same shape (n,)")
        for q in range(2):
            x = c[q]
            if overflow == Overflow.ClampToEdges:
                x = np.where(x > F(0), np.where(x < F(1), x, F(1)), F(0)).astype(F)
            else:
                x = np.copysign(x - np.trunc(x), x).astype(F)
                x = np.where(x < F(0), F(1) + x, x).astype(F)
            c[q] = x * F((w, h)[q] - 1)
        ux, uy = c
        index = lambda x: np.where(x > F(0), np.minimum(np.trunc(np.where(x > F(0), x, F(0))).astype(np.float64), 4294967295.0), 0.0).astype(np.int64)  # noqa: E731
        if interp == Interpolation.Nearest:
            rnd = lambda x: np.where(np.abs(x) < F(8388608.0), np.copysign(np.floor(np.abs(x.astype(np.float64)) + 0.5), x), x).astype(F)  # noqa: E731
            return np.ascontiguousarray(t[np.minimum(index(rnd(uy)), h - 1), np.minimum(index(rnd(ux)), w - 1)])
        lx, ly = np.minimum(index(np.floor(ux)), w - 1), np.minimum(index(np.floor(uy)), h - 1)
        hx, hy = np.minimum(lx + 1, w - 1), np.minimum(ly + 1, h - 1)
        sx, sy = (ux - lx.astype(F))[:, None], (uy - ly.astype(F))[:, None]
        ul, ur, dl, dr = t[hy, lx], t[hy, hx], t[ly, lx], t[ly, hx]
        ui = ul * (F(1) - sx) + ur * sx
        di = dl * (F(1) - sx) + dr * sx
        return np.ascontiguousarray((ui * sy + di * (F(1) - sy)).astype(F))


def _texture_sample_ref(tex, u, v):
    """Texture2d::sample of a scene's Texture2d at float64 (u, v): lightmap_sample_ref on its texels, an RGBA8 channel being `u8 as f32 / 255.0`, one correctly rounded
    float32 division."""
    px = tex.data.pixels
    if px.dtype == np.uint8:
        px = px.astype(np.float32) / np.float32(255.0)
    return lightmap_sample_ref(px, u, v, tex.interpol, tex.overflow)


def material_points_ref(nodes, node_ids, normals=None, uvs=None, hit_flags=None, want=("ambient", "diffuse")):
    """The numpy mirror of nrays_material_points*, bit for bit (include/nrays_abi.h: nrays_material_points_device), over `nodes`, the SceneNode list a Scene is made
    from: per point the terms of the material of nodes[node_ids[i]] — Material::ambiant, kd * texture, (ks, shininess) — and the node's own constants.  Every float32
    step is a numpy float32 operation of its own, in the header's order; the texture sample is lightmap_sample_ref.  `node_ids` (n,) integers, `normals` (n, 3),
    `uvs` (n, 2) or None, `hit_flags` (n,) integers or None, `want` as for material_points.  Returns MaterialTerms of numpy arrays, None for what was not asked for."""
    if any(_is_tensor(a) for a in (node_ids, normals, uvs, hit_flags)):
        raise ValueError("material_points_ref takes numpy arrays")
    node_ids = np.asarray(node_ids)
    n, want = _material_args(node_ids, None if normals is None else np.asarray(normals), None if uvs is None else np.asarray(uvs),
                             None if hit_flags is None else np.asarray(hit_flags), want)
    ids = _np_ints("nodes", node_ids, np.int32).astype(np.int64)
    F = np.float32
    hf = np.full(n, 3, np.uint64) if hit_flags is None else np.asarray(hit_flags).astype(np.uint64)
    live = ((hf & np.uint64(1)) != 0) & (ids >= 0) & (ids < len(nodes))
    has_uv = ((hf & np.uint64(2)) != 0) if uvs is not None else np.zeros(n, bool)
    uv = None if uvs is None else _np_floats("uvs", uvs, np.float64)
    nm = None if normals is None else _np_floats("normals", normals, np.float64)
    amb, dif, spec, nd = np.zeros((n, 4), F), np.zeros((n, 3), F), np.zeros((n, 4), F), np.zeros((n, 4), np.float64)
    with np.errstate(all="ignore"):
        for k in np.unique(ids[live]):
            node, at = nodes[int(k)], live & (ids == k)
            m = node.material
            nd[at] = (float(F(node.alpha)), float(F(node.refl_mix)), float(F(node.refl_atenuation)), node.refr_coeff)
            if m.kind == abi.MAT_NORMAL:
                if "ambient" in want:
                    amb[at, :3] = (F(1.0) + nm[at].astype(F)) / F(2.0)
                    amb[at, 3] = F(1.0)
                continue
            if m.kind == abi.MAT_UV:
                with_uv = at & has_uv
                if "ambient" in want and with_uv.any():
                    amb[with_uv, :2] = uv[with_uv].astype(F)
                    amb[with_uv, 3] = F(1.0)
                continue
            ka, kd = np.asarray(m.ambiant_color, F), np.asarray(m.diffuse_color, F)
            spec[at] = np.asarray(m.specular_color + (m.shininess,), F)
            with_uv, without = at & has_uv, at & ~has_uv
            tc = np.ones((int(with_uv.sum()), 4), F)
            if with_uv.any() and m.texture is not None and ("ambient" in want or "diffuse" in want):
                tc = _texture_sample_ref(m.texture, uv[with_uv, 0], uv[with_uv, 1])
            dif[with_uv] = kd[None, :] * tc[:, :3]
            dif[without] = kd * F(1.0)
            if "ambient" in want:
                w = np.ones(len(tc), F)
                if with_uv.any() and m.alpha is not None:
                    w = _texture_sample_ref(m.alpha, uv[with_uv, 0], uv[with_uv, 1])[:, 3]
                amb[with_uv, :3] = ka[None, :] * tc[:, :3]
                amb[with_uv, 3] = F(1.0) * w
                amb[without, :3] = ka
                amb[without, 3] = F(1.0)
    out = dict(ambient=amb, diffuse=dif, specular=spec, node=nd)
    return MaterialTerms(*(out[name] if name in want else None for name in MaterialTerms._fields))


FILTER_TAPS = (1, 4, 6, 4, 1)  # the B3 spline; a tap's kernel weight is the product of two of them, 1 .. 36


def filter_texels_ref(flags, width, height, points, normals, values, step=1, pos_radius=math.inf, normal_cos=0.0):
    """The numpy mirror of nrays_filter_texels_device's definition (include/nrays_abi.h), bit for bit: what filter_texels() returns, a new float32 array in
    the shape of `values`.  Vectorised: every tap (i, j) is one pair of shifted slices of the lattice, the taps in the definition's order, a skipped tap
    leaving acc and wsum as they are (np.where, not a weight of 0: 0 * inf would be a NaN).  f64 where the definition says f64, float32 arrays where it
    says f32; numpy rounds every operation on its own."""
    flags, values = np.asarray(flags), np.asarray(values)
    if not np.issubdtype(flags.dtype, np.integer):
        raise ValueError("flags must be integers, got %s" % flags.dtype)
    if values.dtype != np.float32:
        raise ValueError("values must be float32, got %s" % values.dtype)
    points, normals = _np_floats("points", points, np.float64), _np_floats("normals", normals, np.float64)
    w, h, step, pos_radius, normal_cos, channels = _filter_args(flags, width, height, points, normals, values, step, pos_radius, normal_cos)
    cov = (flags.astype(np.uint32, copy=False).reshape(h, w) & np.uint32(1)) != 0
    p, nm, v = points.reshape(h, w, 3), normals.reshape(h, w, 3), np.ascontiguousarray(values).reshape(h, w, channels)
    acc, wsum = np.zeros((h, w, channels), np.float32), np.zeros((h, w), np.float32)
    r2, cos, den = np.float64(pos_radius) * np.float64(pos_radius), np.float64(normal_cos), np.float64(1.0) - np.float64(normal_cos)
    with np.errstate(all="ignore"):
        for j in range(-2, 3):
            for i in range(-2, 3):
                dx, dy = i * step, j * step
                xa, xb, ya, yb = max(0, -dx), min(w, w - dx), max(0, -dy), min(h, h - dy)
                if xa >= xb or ya >= yb:
                    continue  # every tap of this offset lies outside the lattice
                D, S = (slice(ya, yb), slice(xa, xb)), (slice(ya + dy, yb + dy), slice(xa + dx, xb + dx))
                if i == 0 and j == 0:
                    take, wt = cov, np.full((h, w), 36.0, np.float32)
                else:
                    take = cov[D] & cov[S]
                    d = p[S] - p[D]
                    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                    wp = np.float64(1.0) - d2 / r2
                    c = (nm[D][..., 0] * nm[S][..., 0] + nm[D][..., 1] * nm[S][..., 1]) + nm[D][..., 2] * nm[S][..., 2]
                    wn = (c - cos) / den
                    take = take & (wp > 0.0) & (wn > 0.0)
                    wn = np.where(wn > 1.0, np.float64(1.0), wn)
                    wt = (np.float32(FILTER_TAPS[i + 2] * FILTER_TAPS[j + 2]) * wp.astype(np.float32)) * wn.astype(np.float32)
                acc[D] = np.where(take[..., None], acc[D] + wt[..., None] * v[S], acc[D])
                wsum[D] = np.where(take, wsum[D] + wt, wsum[D])
        res = acc / wsum[..., None]
    out = v.copy()  # uncovered points: the words as they are
    out[cov] = res[cov]
    return out.reshape(values.shape)


# ---- the nearest surface to caller-supplied points (include/nrays_abi.h: nrays_nearest_points_device) ------------------------------------------------------------

NEAREST_MARGIN = 2.0 ** -38  # the cull's margin is NEAREST_MARGIN * (bound + scale2): DESIGN, "Nearest-surface queries"


def nearest_box_bound_ref(points, boxes):
    """The numpy mirror of the device's nearest_box_bound (nearest_kernel.h), bit for bit: a lower bound of the exact squared distance from each of the (n, 3) float64
    `points` to each of the (m, 6) `boxes` {min x, y, z, max x, y, z}, narrowed to float32 as a BVH node holds them.  Per axis the gap max(mn - p, p - mx, 0), the
    squares summed left to right, capped at DBL_MAX, scaled by 1 - 2^-50; below 1e-290 the bound is 0.  Returns (n, m) float64."""
    P = np.asarray(points, np.float64).reshape(-1, 1, 3)
    B = np.asarray(boxes, np.float64).reshape(1, -1, 6).astype(np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        g = np.fmax(np.fmax(B[..., :3] - P, P - B[..., 3:]), 0.0)
        s = np.fmin((g[..., 0] * g[..., 0] + g[..., 1] * g[..., 1]) + g[..., 2] * g[..., 2], np.finfo(np.float64).max)
        b = s * (1.0 - 2.0 ** -50)
    return np.where(b < 1e-290, 0.0, b)


def nearest_margin_ref(bound, scale2):
    """The margin the walk grants a box bound: NEAREST_MARGIN * (bound + scale2), scale2 = (max |p_k| + the scene's coordinate bound)^2."""
    with np.errstate(all="ignore"):
        return NEAREST_MARGIN * (np.asarray(bound, np.float64) + scale2)


def nearest_skips_ref(bound, margin, best):
    """Whether the walk skips a box: iff bound - margin > best.  Equal values are visited (the tie-break); a NaN skips nothing."""
    with np.errstate(all="ignore"):
        return np.asarray(bound, np.float64) - margin > best


def _dot3(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _d2_of(p, q):
    e = p - q
    return (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]


def tri_closest_ref(a, b, c, p):
    """Ericson's closest point on a triangle as the header writes it, element-wise over broadcastable (..., 3) float64 arrays: (v, w, q, region), region 0 .. 6 =
    vertex A, vertex B, edge AB, vertex C, edge AC, edge BC, interior."""
    a, b, c, p = np.broadcast_arrays(*(np.asarray(x, np.float64) for x in (a, b, c, p)))
    with np.errstate(all="ignore"):
        ab, ac, ap = b - a, c - a, p - a
        d1, d2 = _dot3(ab, ap), _dot3(ac, ap)
        bp = p - b
        d3, d4 = _dot3(ab, bp), _dot3(ac, bp)
        vc = d1 * d4 - d3 * d2
        cp = p - c
        d5, d6 = _dot3(ab, cp), _dot3(ac, cp)
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        den = (va + vb) + vc
        tests = [(d1 <= 0.0) & (d2 <= 0.0), (d3 >= 0.0) & (d4 <= d3), (vc <= 0.0) & (d1 >= 0.0) & (d3 <= 0.0), (d6 >= 0.0) & (d5 <= d6),
                 (vb <= 0.0) & (d2 >= 0.0) & (d6 <= 0.0), (va <= 0.0) & ((d4 - d3) >= 0.0) & ((d5 - d6) >= 0.0)]
        region = np.full(d1.shape, 6, np.int64)
        for k in range(5, -1, -1):
            region = np.where(tests[k], k, region)
        vab, wac, wbc = d1 / (d1 - d3), d2 / (d2 - d6), (d4 - d3) / ((d4 - d3) + (d5 - d6))
        vi, wi = vb / den, vc / den
        one, zero = np.ones_like(d1), np.zeros_like(d1)
        # the last branch: the interior point, if its weights are in range, against the three clamped edge projections (strict <, in the order AB, AC, BC)
        clamp01 = lambda t: np.where(t >= 0.0, np.where(t <= 1.0, t, 1.0), 0.0)  # noqa: E731
        qi = (a + ab * vi[..., None]) + ac * wi[..., None]
        best = np.where((vi >= 0.0) & (wi >= 0.0) & ((1.0 - vi) - wi >= 0.0), _d2_of(p, qi), np.inf)
        t1, t2, t3 = clamp01(vab), clamp01(wac), clamp01(wbc)
        for t, qe, ve, we in ((t1, a + ab * t1[..., None], t1, zero), (t2, a + ac * t2[..., None], zero, t2), (t3, b + (c - b) * t3[..., None], 1.0 - t3, t3)):
            e = _d2_of(p, qe)
            take = e < best
            best, qi, vi, wi = np.where(take, e, best), np.where(take[..., None], qe, qi), np.where(take, ve, vi), np.where(take, we, wi)
        v = np.choose(region, [zero, one, vab, zero, zero, 1.0 - wbc, vi])
        w = np.choose(region, [zero, zero, zero, one, wac, wbc, wi])
        r = region[..., None]
        q = np.where(r == 0, a, np.where(r == 1, b, np.where(r == 2, a + ab * vab[..., None], np.where(r == 3, c, np.where(
            r == 4, a + ac * wac[..., None], np.where(r == 5, b + (c - b) * wbc[..., None], qi))))))
    return v, w, q, region


def _clamp(x, lo, hi):
    return np.where(x < lo, lo, np.where(x > hi, hi, x))


def nearest_shape_ref(kind, params, pl):
    """An analytic shape's closest point to the (n, 3) local points `pl` as the header defines it: (ql, nl, behind)."""
    pl = np.asarray(pl, np.float64).reshape(-1, 3)
    p0, p1, p2 = (float(x) for x in params)
    x, y, z = pl[:, 0], pl[:, 1], pl[:, 2]
    with np.errstate(all="ignore"):
        if kind == abi.SHAPE_BALL:
            ln = np.sqrt((x * x + y * y) + z * z)
            at0 = (ln == 0.0)[:, None]
            q = np.where(at0, np.array([p0, 0.0, 0.0]), pl * (p0 / ln)[:, None])
            nl = np.where(at0, np.array([1.0, 0.0, 0.0]), pl / ln[:, None])
            return q, nl, ln < p0
        if kind == abi.SHAPE_CUBOID:
            h = np.array([p0, p1, p2])
            g = h - np.abs(pl)
            inside = (g >= 0.0).all(axis=1)
            ax = np.where((g[:, 0] <= g[:, 1]) & (g[:, 0] <= g[:, 2]), 0, np.where(g[:, 1] <= g[:, 2], 1, 2))
            on = np.arange(3)[None, :] == ax[:, None]
            qi, ni = np.where(on, np.copysign(h, pl), pl), np.where(on, np.copysign(1.0, pl), 0.0)
            qo = _clamp(pl, -h, h)
            no = (pl - qo) / np.sqrt(_d2_of(pl, qo))[:, None]
            return np.where(inside[:, None], qi, qo), np.where(inside[:, None], ni, no), inside & (g > 0.0).all(axis=1)
        if kind == abi.SHAPE_PLANE:
            nrm = np.array([p0, p1, p2])
            t = _dot3(np.broadcast_to(nrm, pl.shape), pl)
            behind = t < 0.0
            return pl - nrm * t[:, None], np.where(behind[:, None], -nrm, nrm), behind
        hh, r = p0, p1
        rho = np.sqrt(x * x + z * z)
        cx, cz = np.where(rho == 0.0, 1.0, x / rho), np.where(rho == 0.0, 0.0, z / rho)
        if kind == abi.SHAPE_CYLINDER:
            gs, gc = r - rho, hh - np.abs(y)
            named = (gs >= 0.0) & (gc >= 0.0)
            side = gs <= gc
            qr, qy = np.where(named, np.where(side, r, rho), np.where(rho > r, r, rho)), np.where(named, np.where(side, y, np.copysign(hh, y)), _clamp(y, -hh, hh))
            nr, ny = np.where(side, 1.0, 0.0), np.where(side, 0.0, np.copysign(1.0, y))
            behind = (gs > 0.0) & (gc > 0.0)
        elif kind == abi.SHAPE_CAPSULE:
            yc = _clamp(y, -hh, hh)
            ey = y - yc
            ln = np.sqrt(rho * rho + ey * ey)
            nr, ny = np.where(ln == 0.0, 1.0, rho / ln), np.where(ln == 0.0, 0.0, ey / ln)
            qr, qy = nr * r, yc + ny * r
            named, behind = np.ones(len(pl), bool), ln < r
        elif kind == abi.SHAPE_CONE:
            up, h2 = y + hh, 2.0 * hh
            br = np.where(rho > r, r, rho)
            e0 = rho - br
            db = e0 * e0 + up * up
            t = _clamp(((rho - r) * -r + up * h2) / (r * r + h2 * h2), 0.0, 1.0)
            sr, sy = r + -r * t, -hh + h2 * t
            e1, e2 = rho - sr, y - sy
            ds = e1 * e1 + e2 * e2
            f = (rho - r) * h2 + up * r
            base = db <= ds
            qr, qy = np.where(base, br, sr), np.where(base, -hh, sy)
            behind, named = (up > 0.0) & (f < 0.0), (up >= 0.0) & (f <= 0.0)
            ln = np.sqrt(h2 * h2 + r * r)
            nr, ny = np.where(base, 0.0, h2 / ln), np.where(base, -1.0, r / ln)
        else:
            raise ValueError("nearest_shape_ref: not an analytic shape kind: %r" % (kind,))
        er, ey = rho - qr, y - qy
        ln = np.sqrt(er * er + ey * ey)
        nr, ny = np.where(named, nr, er / ln), np.where(named, ny, ey / ln)
        return np.stack([qr * cx, qy, qr * cz], axis=1), np.stack([nr * cx, ny, nr * cz], axis=1), behind


def _nearest_frame(transform):
    from . import math3d
    aa = (0.0, 0.0, 0.0) if transform is None else tuple(transform.axis_angle)
    T = np.array((0.0, 0.0, 0.0) if transform is None else tuple(transform.translation), np.float64)
    identity = aa == (0.0, 0.0, 0.0)
    return math3d.rotation_from_axis_angle(aa), T, identity, identity and not T.any()


def nearest_local_ref(transform, p):
    """The query points in a node's local space, with the header's shortcuts: R^T (p - T) in inv_rot's order, p - T without a rotation, p without either."""
    R, T, identity, noxform = _nearest_frame(transform)
    p = np.asarray(p, np.float64).reshape(-1, 3)
    if noxform:
        return p
    v = p - T
    if identity:
        return v
    return np.stack([(R[0, k] * v[:, 0] + R[1, k] * v[:, 1]) + R[2, k] * v[:, 2] for k in range(3)], axis=1)


def _nearest_world(transform, q, nl):
    R, T, identity, noxform = _nearest_frame(transform)
    if noxform:
        return q, nl
    if identity:
        return q + T, nl
    rot = lambda a: np.stack([(R[k, 0] * a[:, 0] + R[k, 1] * a[:, 1]) + R[k, 2] * a[:, 2] for k in range(3)], axis=1)  # noqa: E731
    return rot(q) + T, rot(nl)


def _mesh_arrays(g):
    P = np.asarray(g.points, np.float64).astype(np.float32).astype(np.float64)
    I = np.asarray(g.indices).reshape(-1, 3).astype(np.int64)
    UV = None if g.uvs is None else np.asarray(g.uvs, np.float64).astype(np.float32).astype(np.float64)
    return P, I, UV


def nearest_node_d2_ref(node, points, block=1 << 21):
    """The keys of one scene node: (d2 (n,) float64, tri (n,) int64) — the smallest key over the node's triangles with the smallest triangle index among equals
    (-1 and d2 NaN for a mesh without triangles), or the analytic shape's key with tri -1.  A NaN key is no candidate."""
    g = node.geometry
    pl = nearest_local_ref(node.transform, points)
    n = len(pl)
    with np.errstate(all="ignore"):
        if g.kind != abi.SHAPE_TRIMESH:
            q, _, _ = nearest_shape_ref(g.kind, g.params, pl)
            return _d2_of(pl, q), np.full(n, -1, np.int64)
        P, I, _ = _mesh_arrays(g)
        best, tri = np.full(n, np.nan), np.full(n, -1, np.int64)
        pstep = max(1, min(n, 8192))
        tstep = max(1, block // pstep)
        for p0 in range(0, n, pstep):
            pp = pl[p0:p0 + pstep, None, :]
            for t0 in range(0, len(I), tstep):
                T = I[t0:t0 + tstep]
                _, _, q, _ = tri_closest_ref(P[T[:, 0]][None], P[T[:, 1]][None], P[T[:, 2]][None], pp)
                d2 = _d2_of(pp, q)
                d2c = np.where(np.isnan(d2), np.inf, d2)
                k = np.argmin(d2c, axis=1)  # (the first of equals: the smallest index)
                rows = np.arange(len(k))
                cand, valid = d2[rows, k], ~np.isnan(d2[rows, k])
                cur, curt = best[p0:p0 + pstep], tri[p0:p0 + pstep]
                take = valid & ((curt < 0) | (cand < cur))
                cur[take], curt[take] = cand[take], (k + t0)[take]
        return best, tri


def nearest_points_ref(nodes, points, max_dist=None, hit_flags=None):
    """The numpy mirror of nrays_nearest_points*, bit for bit (include/nrays_abi.h: nrays_nearest_points_device), by brute force over `nodes`, the SceneNode list a Scene
    is made from: every node and every triangle is a candidate, in ascending order, a later one winning only with a strictly smaller key.  `points` (n, 3) float64;
    `max_dist` (n,) or None; `hit_flags` (n,) integers or None.  Returns NearestHits of numpy arrays (flags uint32).  The ball's uv goes through numpy's arctan2 and
    arcsin: equal to the device's up to the math library; everything else is + - * / sqrt."""
    P = np.ascontiguousarray(np.asarray(points, np.float64).reshape(-1, 3))
    n = len(P)
    md = np.full(n, np.inf) if max_dist is None else np.asarray(max_dist, np.float64).reshape(n)
    with np.errstate(invalid="ignore"):
        live = md >= 0.0
    if hit_flags is not None:
        live &= (np.asarray(hit_flags).astype(np.uint64) & np.uint64(1)) != 0
    idx = np.nonzero(live)[0]
    Q = P[idx]
    m = len(Q)
    bd2, bnode, btri = np.full(m, np.inf), np.full(m, -1, np.int64), np.full(m, -1, np.int64)
    with np.errstate(all="ignore"):
        for k, node in enumerate(nodes):
            d2, tri = nearest_node_d2_ref(node, Q)
            take = ~np.isnan(d2) & ((bnode < 0) | (d2 < bd2))
            bd2[take], bnode[take], btri[take] = d2[take], k, tri[take]
        dist = np.sqrt(bd2)
        found = (bnode >= 0) & (dist <= md[idx])
        out = NearestHits(dist=np.full(n, np.inf), node=np.full(n, -1, np.int32), point=np.zeros((n, 3)), normal=np.zeros((n, 3)), uv=np.zeros((n, 2)),
                          prim=np.full(n, -1, np.int32), flags=np.zeros(n, np.uint32))
        for k in np.unique(bnode[found]):
            node, at = nodes[int(k)], found & (bnode == k)
            g, rows = node.geometry, idx[at]
            pl = nearest_local_ref(node.transform, Q[at])
            flags = np.full(len(rows), 1, np.uint32)
            if g.kind == abi.SHAPE_TRIMESH:
                V, I, UV = _mesh_arrays(g)
                T = I[btri[at]]
                a, b, c = V[T[:, 0]], V[T[:, 1]], V[T[:, 2]]
                v, w, q, _ = tri_closest_ref(a, b, c, pl)
                cr = np.cross(b - a, c - a)  # (each component x y' - y x': two products and a difference, as cross())
                behind = _dot3(pl - a, cr) < 0.0
                nl = cr / np.sqrt(_dot3(cr, cr))[:, None]
                nl = np.where(behind[:, None], -nl, nl)
                out.prim[rows] = btri[at]
                if UV is not None:
                    b0 = (1.0 - v) - w
                    out.uv[rows] = (UV[T[:, 0]] * b0[:, None] + UV[T[:, 1]] * v[:, None]) + UV[T[:, 2]] * w[:, None]
                    flags |= np.uint32(2)
            else:
                q, nl, behind = nearest_shape_ref(g.kind, g.params, pl)
            wp, wn = _nearest_world(node.transform, q, nl)
            if g.kind == abi.SHAPE_BALL:
                out.uv[rows] = np.stack([0.5 + np.arctan2(wn[:, 2], wn[:, 0]) / (math.pi * 2.0), 0.5 - np.arcsin(wn[:, 1]) / math.pi], axis=1)
                flags |= np.uint32(2)
            out.dist[rows], out.node[rows], out.point[rows], out.normal[rows] = dist[at], k, wp, wn
            out.flags[rows] = flags | np.where(behind, np.uint32(NEAREST_BEHIND), np.uint32(0))
    return out
