"""The arithmetic past the closest hit, restated from the reference's sources alone, and the case sets the shading tests share.

Tests only.  The restatement was written from
  src/phong_material.rs:39-151   PhongMaterial::ambiant and ::compute
  src/normal_material.rs         (1 + normal as f32) / 2, w = 1
  src/uv_material.rs             (u as f32, v as f32, 0, 1); without a uv the origin, w = 0
  src/material.rs                the default compute() IS ambiant()
  src/scene.rs:147-252, 304-339  intersects_ray and its cost function; trace, trace_reflection, trace_refraction
  src/ray_with_energy.rs         refr f64, energy f32, both 1.0 for a camera ray
  src/light.rs:16-24             racsample = sqrt(nsample as f32) as usize
without reading the shading or bounce code of oracle/nrays_oracle.c or nrays_amd/csrc/trace_device.h (only the project's own RNG definition and the
key salts of continuation rays, which are inputs here, were taken from the oracle: light 0x200 + index, reflection 0x100, refraction 0x101).  It is float64 numpy and rounds to f32 only where the reference's types
round AND a later step amplifies the rounding: `dot_ldir_norm as f32` before max(0.0); `scoeff as f32` before powf; shininess and every colour as
the f32 they are stored as; `ray.energy - attenuation`; the comparisons energy > 0.1, alpha != 1.0, alpha < 1.0, !mix.is_zero() (alpha = obj.w *
sn.alpha is an f32 product); and the transparent-shadow filter, which is evaluated in f32 as written.  Everything else stays in float64 and
bound() pays for it.

What is NOT restated because it is this project's own definition and therefore an input: where an area light's samples lie (tied to
oracle.rng_u01 by one CPU assertion) and the keys of continuation rays.  What is elementary and not under test: the hit of a ray with an infinite
plane, an axis-aligned horizontal quad, and a ball (hits()).

Worlds are lists of Surf (plane / quad / ball) with Mat materials; build_scene() makes the nrays_amd scene of a world.  Case sets:
  A  compute() in free space: one tiny far ball per material, ~800 points per light set (three light sets), directed edges for every material;
  B  the same behind one, two and three transparent surfaces, an opaque blocker, and the shadow rays themselves;
  C  the direction probe: 35 probes (mix, alpha) x refr_coeff in one scene, a plane (or a textured quad) through the centre of a non-solid
     NormalMaterial ball of radius 50: every continuation leaves the centre radially and the ball's colour (1 - dir) / 2 reads its DIRECTION back;
     the slab (two planes, carried refr / energy), the lit mirror (non-unit reflected directions seen by a specular term), and two 16 x 12 frames.

The bound (see bound_compute / trace's error recursion), with U = 2^-24:
  K, compute:    16 roundings on the longest path (+ 5 per transparent crossing in set B: up to 31)       per channel K * U * sum|terms|
  K, blend:      9 per level of Scene::trace, propagated through the recursion; + 2 U for a NormalMaterial colour
  P, powf:       2 ulp — no accuracy table for powf ships with the ROCm installation (searched share/, include/ and the device library's
                 headers for "ulp"), so the issue's fallback is used              per specular term (shininess + P) * 2^-23 * |term|
  filter alone:  5 roundings per crossing
  Set  what                              K        worst |error| / bound: oracle (CPU)   device (MI355X)
  A    shade_points, three light sets    16       0.166 (2.7 U sum|terms|)              0.166
  B    shade_points behind filters       16 - 31  0.074                                 0.074
  B    intersects_rays' filter           5 - 15   0 (bit-equal, lit mask equal)         0 (bit-equal, lit mask equal)
  C    probes, slab, lit mirror          9 / level  0.130                               0.130
  C    the two 16 x 12 frames            9 / level  0.117                               0.117
(the device figures are the same with NRAYS_ELIDE=0 and in the numpy and torch forms; the derived bound is 16 - 31 units of U * sum|terms| for
compute and about 11 - 20 U per unit of colour for a traced ray, against the 1e-4 = 1678 U of the oracle-parity tests.)
Dropped random cases: set B drops a random point when one of its shadow rays passes within 1e-6 of an edge (or the diagonal) of a quad: 0 of
them at the committed seed (asserted < 2 %); no directed case is ever dropped (asserted).

Two of the issue's nine "named single mistakes" are identities in real numbers and cannot move a result by more than a rounding:
max(0) on either side of the f32 cast (rounding is monotone and fixes 0; only the sign of a zero differs, which no later step sees) and
(1 - alpha) applied before or after the component product (multiplication commutes).  They are kept, asserted to stay INSIDE the bound
(tests/test_shading_restated.py), and each has a neighbour that is a real misreading and must be caught by 100 x the bound: the clamped dot
also feeding the mirrored direction, and (1 - alpha) taken from the material's w without the node's alpha.
"""
import collections

import numpy as np

import nrays_amd as nr
from nrays_amd import math3d
from nrays_amd.scene import _rng_hash

F32 = np.float32
U = 2.0 ** -24
P_POWF = 2.0
K_COMPUTE = 16
K_CROSSING = 5
K_BLEND = 9
SEED = 0x5AADE
DENORM_MIN = float(np.array([1], np.uint32).view(F32)[0])
FLT_MIN = float(np.finfo(F32).tiny)
F01 = F32(0.1)

MISTAKES = ("swap_n1_n2", "reflect_normalised", "tangent_n1_over_n2", "max_before_lproj", "scoeff_unnormalised", "axpy_crossed",
            "filter_without_node_alpha", "blend_one_minus_mix_on_refl", "energy_ge")
IDENTITIES = ("max_before_cast", "filter_alpha_first")


def f32(x):
    """The value after `as f32`, as float64."""
    return np.asarray(x, dtype=np.float64).astype(F32).astype(np.float64)


def _unit(v):
    v = np.asarray(v, dtype=np.float64)
    return v / np.sqrt((v * v).sum(axis=-1, keepdims=True))


def _dot(a, b):
    return (a * b).sum(axis=-1)


# ---------------------------------------------------------------------------------------------------------------- materials, surfaces, worlds
class Mat:
    """kind 'phong' | 'normal' | 'uv'.  tex: the one RGBA8 texel of a 1 x 1 colour texture or None; alpha_tex: the one alpha byte of a 1 x 1
    opacity map or None (a 1 x 1 texture samples to its texel exactly, `u8 as f32 / 255.0`, in every mode)."""

    def __init__(self, kind="phong", ka=(0, 0, 0), kd=(0, 0, 0), ks=(0, 0, 0), shininess=1.0, tex=None, alpha_tex=None):
        self.kind = kind
        self.ka, self.kd, self.ks = f32(ka), f32(kd), f32(ks)
        self.shininess = float(f32(shininess))
        self.tex, self.alpha_tex = tex, alpha_tex
        self.texel = None if tex is None else (np.asarray(tex, np.uint8).astype(F32) / F32(255.0)).astype(np.float64)
        self.alpha_w = None if alpha_tex is None else float(F32(alpha_tex) / F32(255.0))

    def to_nr(self):
        if self.kind == "normal":
            return nr.NormalMaterial()
        if self.kind == "uv":
            return nr.UVMaterial()
        one = lambda rgba: nr.Texture2d(nr.ImageData(np.asarray(rgba, np.uint8).reshape(1, 1, 4)), nr.Interpolation.Nearest, nr.Overflow.Wrap)  # noqa: E731
        tex = None if self.tex is None else one(self.tex)
        alpha = None if self.alpha_tex is None else one((255, 255, 255, self.alpha_tex))
        return nr.PhongMaterial(tuple(self.ka), tuple(self.kd), tuple(self.ks), tex, alpha, self.shininess)


class Surf:
    """shape 'plane' (unit normal n through p0), 'quad' (y = p0.y, x in [lo.x, hi.x], z in [lo.z, hi.z], two triangles with uvs),
    'ball' (centre p0, radius r; never solid)."""

    def __init__(self, shape, mat, p0=(0, 0, 0), n=(0, 1, 0), r=0.0, lo=None, hi=None, mix=0.0, att=0.0, alpha=1.0, coeff=1.0):
        self.shape, self.mat = shape, mat
        self.p0, self.n, self.r = np.asarray(p0, np.float64), np.asarray(n, np.float64), float(r)
        self.lo, self.hi = lo, hi
        self.mix, self.att, self.alpha, self.coeff = float(f32(mix)), float(f32(att)), float(f32(alpha)), float(coeff)
        self.has_uv = shape == "quad"  # (a ball has a uv too, but only a NormalMaterial is ever put on one here)

    def to_nr(self):
        if self.shape == "plane":
            geom, iso = nr.Plane(tuple(self.n)), nr.Isometry3(tuple(self.p0))
        elif self.shape == "ball":
            geom, iso = nr.Ball(self.r), nr.Isometry3(tuple(self.p0))
        else:
            (x0, z0), (x1, z1), y = self.lo, self.hi, self.p0[1]
            pts = np.array([[x0, y, z0], [x1, y, z0], [x1, y, z1], [x0, y, z1]], np.float64)
            assert np.array_equal(pts, pts.astype(F32).astype(np.float64))
            uvs = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float64)
            geom, iso = nr.TriMesh(pts, np.array([[0, 1, 2], [0, 2, 3]], np.uint32), uvs), nr.Isometry3()
        return nr.SceneNode(self.mat.to_nr(), self.mix, self.att, self.alpha, self.coeff, iso, geom)


World = collections.namedtuple("World", "surfs lights background")
LightSpec = collections.namedtuple("LightSpec", "pos radius nsample color")


def racsample(nsample):
    """light.rs:20: ((nsample as f32).sqrt()) as usize."""
    return int(np.sqrt(F32(nsample)))


def build_scene(world):
    lights = [nr.Light(tuple(l.pos), l.radius, l.nsample, tuple(l.color)) for l in world.lights]
    return nr.Scene([s.to_nr() for s in world.surfs], lights, tuple(world.background))


# ---------------------------------------------------------------------------------------------------------------- elementary hits (not under test)
def hits(surf, o, d):
    """(t, facing normal, margin) of rays with one surface: t = inf where there is no hit; margin = distance of a quad's plane crossing from its
    nearest edge or diagonal (inf for the other shapes)."""
    n = len(o)
    inf = np.full(n, np.inf)
    with np.errstate(divide="ignore", invalid="ignore"):
        if surf.shape == "ball":
            oc = o - surf.p0
            a, b, c = _dot(d, d), _dot(oc, d), _dot(oc, oc) - surf.r * surf.r
            disc = b * b - a * c
            ok = disc >= 0.0
            sq = np.sqrt(np.where(ok, disc, 0.0))
            inside = c <= 0.0
            t = np.where(inside, (-b + sq) / a, (-b - sq) / a)
            ok &= t >= 0.0
            pt = o + d * np.where(ok, t, 0.0)[:, None]
            nrm = (pt - surf.p0) / surf.r
            nrm = np.where(inside[:, None], -nrm, nrm)
            return np.where(ok, t, np.inf), nrm, inf
        s = _dot(o - surf.p0, surf.n)
        den = _dot(d, surf.n)
        t = -s / den
        ok = (den != 0.0) & (t >= 0.0)
        nrm = np.where((s < 0.0)[:, None], -surf.n, surf.n) * np.ones((n, 1))
        margin = inf
        if surf.shape == "quad":
            pt = o + d * np.where(ok, t, 0.0)[:, None]
            (x0, z0), (x1, z1) = surf.lo, surf.hi
            x, z = pt[:, 0], pt[:, 2]
            ok &= (x > x0) & (x < x1) & (z > z0) & (z < z1)
            w, h = x1 - x0, z1 - z0
            diag = np.abs((x - x0) * h - (z - z0) * w) / np.hypot(w, h)
            inner = np.minimum(np.minimum(x - x0, x1 - x), np.minimum(z - z0, z1 - z))
            outer = np.hypot(np.maximum(np.maximum(x0 - x, x - x1), 0.0), np.maximum(np.maximum(z0 - z, z - z1), 0.0))
            near = (den != 0.0) & (t >= 0.0)
            margin = np.where(near, np.where(ok, np.minimum(inner, diag), outer), np.inf)
        return np.where(ok, t, np.inf), nrm, margin


def closest(world, o, d):
    best_t, best_n, best_s = np.full(len(o), np.inf), np.zeros((len(o), 3)), np.full(len(o), -1)
    for i, s in enumerate(world.surfs):
        t, nrm, _ = hits(s, o, d)
        take = t < best_t
        best_t, best_s = np.where(take, t, best_t), np.where(take, i, best_s)
        best_n = np.where(take[:, None], nrm, best_n)
    return best_t, best_n, best_s


# ---------------------------------------------------------------------------------------------------------------- the restatement
def ambiant(mat, normal, has_uv, uv=None):
    """Material::ambiant: (n, 4).  has_uv: (n,) bool."""
    n = len(normal)
    has_uv = np.broadcast_to(np.asarray(has_uv, bool), (n,))
    out = np.ones((n, 4))
    if mat.kind == "normal":      # normal_material.rs:9-14
        out[:, :3] = (1.0 + f32(normal)) / 2.0
        return out
    if mat.kind == "uv":          # uv_material.rs:10-20
        out[:] = 0.0
        if uv is not None:
            out[:, 0], out[:, 1] = np.where(has_uv, f32(uv[:, 0]), 0.0), np.where(has_uv, f32(uv[:, 1]), 0.0)
        out[:, 3] = np.where(has_uv, 1.0, 0.0)
        return out
    tex = np.ones((n, 4))         # phong_material.rs:39-70
    if mat.texel is not None:
        tex[:, :3] = mat.texel[:3]      # tex_color.w = 1.0
    if mat.alpha_w is not None:
        tex[:, 3] = mat.alpha_w
    tex = np.where(has_uv[:, None], tex, 1.0)
    out[:, :3] = mat.ka * tex[:, :3]
    out[:, 3] = tex[:, 3]
    return out


def shadow_filter(rgb, alpha, mistake=None):
    """scene.rs:322-331 over the crossings of one ray IN ORDER, in f32: rgb (k, n, 3) and alpha (k, n) as f32 values, `crossed` where a
    surface is crossed at all is folded into alpha = nan (no crossing).  Returns (lit (n,), filter (n, 3))."""
    k, n = alpha.shape
    filt = np.ones((n, 3), F32)
    lit = np.ones(n, bool)
    for i in range(k):
        a = alpha[i].astype(F32)
        there = ~np.isnan(a)
        lit &= ~(there & ~(a < F32(1.0)))
        one_minus = (F32(1.0) - a)[:, None]
        if mistake == "filter_alpha_first":
            new = filt * (rgb[i].astype(F32) * one_minus)
        else:
            new = (filt * rgb[i].astype(F32)) * one_minus
        filt = np.where((there & (a < F32(1.0)))[:, None], new, filt).astype(F32)
    return lit, np.where(lit[:, None], filt, F32(0.0)).astype(np.float64)


def shadow(world, o, d, maxtoi, mistake=None):
    """Scene::intersects_ray (scene.rs:147-161, 304-339).  Returns lit, filter, number of transparent crossings, quad margin."""
    n = len(o)
    rgb, alpha = np.zeros((len(world.surfs), n, 3)), np.full((len(world.surfs), n), np.nan)
    margin = np.full(n, np.inf)
    for i, s in enumerate(world.surfs):
        t, nrm, m = hits(s, o, d)
        crossed = t <= maxtoi
        margin = np.minimum(margin, m)
        col = ambiant(s.mat, nrm, s.has_uv, np.zeros((n, 2)))
        a = col[:, 3].astype(F32) if mistake == "filter_without_node_alpha" else col[:, 3].astype(F32) * F32(s.alpha)
        rgb[i] = col[:, :3].astype(F32)
        alpha[i] = np.where(crossed, a, np.nan)
    lit, filt = shadow_filter(rgb, alpha, mistake)
    ncross = (~np.isnan(alpha) & (alpha < 1.0)).sum(axis=0)
    return lit, filt, ncross, margin


def light_positions(lights, keys):
    """Per light (n, racsample^2, 3): pos + u * radius, u from this project's RNG, an INPUT of the restatement."""
    keys = np.asarray(keys, np.uint64)
    out = []
    for li, l in enumerate(lights):
        ns = racsample(l.nsample) ** 2
        pos = np.tile(np.asarray(l.pos, np.float64), (len(keys), ns, 1))
        if l.radius != 0.0:
            lkey = _rng_hash(keys, 0x200 + li)
            for k in range(ns):
                sk = _rng_hash(lkey, k)
                u = np.stack([(_rng_hash(sk, 0x1000 + dim) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53 for dim in range(3)], axis=1)
                pos[:, k] = pos[:, k] + u * l.radius
        out.append(pos)
    return out


def shadow_rays_of(point, positions):
    """phong_material.rs:109-112: per light (origin, dir, maxtoi) of shape (n, ns, ...)."""
    out = []
    for pos in positions:
        ld = pos - point[:, None, :]
        dist = np.sqrt(_dot(ld, ld))
        ld = ld / dist[..., None]
        out.append((point[:, None, :] + ld * 0.001, ld, dist - 0.001))
    return out


def light_samples(world, point, keys, mistake=None):
    """The INPUTS of compute(): per light (positions, filters, lit, crossings, margin)."""
    positions = light_positions(world.lights, keys)
    out = []
    for pos, (o, d, mt) in zip(positions, shadow_rays_of(point, positions)):
        n, ns = mt.shape
        lit, filt, nc, mg = shadow(world, o.reshape(-1, 3), d.reshape(-1, 3), mt.reshape(-1), mistake)
        out.append((pos, filt.reshape(n, ns, 3), lit.reshape(n, ns), nc.reshape(n, ns), mg.reshape(n, ns)))
    return out


def compute(mat, lights, samples, point, normal, view, has_uv, uv=None, mistake=None):
    """Material::compute.  Returns colour (n, 3), alpha (n,), sum|terms| (n, 3), and the powf allowance (n, 3) =
    sum over specular terms of (shininess + P) * 2^-23 * |term|."""
    n = len(normal)
    has_uv = np.broadcast_to(np.asarray(has_uv, bool), (n,))
    if mat.kind != "phong":       # material.rs:8-16
        a = ambiant(mat, normal, has_uv, uv)
        return a[:, :3], a[:, 3], np.abs(a[:, :3]), np.zeros((n, 3))
    tex = np.ones((n, 3))
    if mat.texel is not None:
        tex = np.where(has_uv[:, None], mat.texel[:3], 1.0)
    alpha = np.ones(n) if mat.alpha_w is None else np.where(has_uv, mat.alpha_w, 1.0)
    res = mat.ka * tex
    sumabs, powabs = np.abs(res), np.zeros((n, 3))
    for l, smp in zip(lights, samples):
        pos, filt, lit = smp[0], smp[1], smp[2]
        acc, accabs, accpow = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
        lc = f32(l.color)
        for k in range(pos.shape[1]):
            ldir = pos[:, k] - point
            ldir = ldir / np.sqrt(_dot(ldir, ldir))[:, None]
            dln = _dot(ldir, normal)
            dcoeff = f32(np.maximum(dln, 0.0)) if mistake == "max_before_cast" else np.maximum(f32(dln), 0.0)
            if mistake == "max_before_lproj":
                dln = np.maximum(dln, 0.0)
            diffuse = (mat.kd * tex) * dcoeff[:, None]
            r = -ldir + (normal * dln[:, None]) * 2.0
            rldir = r if mistake == "scoeff_unnormalised" else r / np.sqrt(_dot(r, r))[:, None]
            scoeff = f32(-_dot(rldir, view))
            shines = scoeff > 0.0
            with np.errstate(over="ignore"):   # (only a mistaken restatement overflows)
                specular = mat.ks * np.where(shines, np.power(np.where(shines, scoeff, 1.0), mat.shininess), 0.0)[:, None]
            on = lit[:, k][:, None]
            acc = acc + np.where(on, lc * (filt[:, k] * (diffuse + specular)), 0.0)
            accabs = accabs + np.where(on, np.abs(lc * filt[:, k]) * (np.abs(diffuse) + np.abs(specular)), 0.0)
            accpow = accpow + np.where(on, np.abs(lc * filt[:, k] * specular), 0.0)
        rs = racsample(l.nsample)
        w = float(F32(1.0) / F32(rs * rs))                   # res.axpy(1.0 / (r * r) as f32, &acc, 1.0): self = a * x + b * self
        res = acc + w * res if mistake == "axpy_crossed" else w * acc + res
        sumabs = sumabs + w * accabs
        powabs = powabs + w * accpow * ((mat.shininess + P_POWF) * 2.0 ** -23)
    return res, alpha, sumabs, powabs


def bound_compute(sumabs, powabs, crossings=0):
    """The largest |f32 result - restatement| a faithful evaluation can show, per channel.

    The reference evaluates in f32; the restatement in f64 from the same f32 inputs.  Every f32 operation is correctly rounded: a relative
    error of at most U = 2^-24 of its result, and every partial result is at most sum|terms| (the sum of the absolute values of the ambient term
    and of every light sample's diffuse and specular terms, with their weights).  So the difference is at most K * U * sum|terms| to first order,
    K = the number of roundings on the longest path of phong_material.rs:102-150:
        dot_ldir_norm as f32          2   (the cast, and one more because two faithful f64 evaluations of the dot may round to neighbours)
        Kd * tex, * dcoeff            2   (the specular path Ks * powf is shorter: 1, its powf is paid separately below)
        diffuse + specular            1
        filter *, light.color *       2
        acc + ...                     4   (racsample^2 = 4 samples at most in these cases)
        1 / (r * r) as f32, a * acc   2
        res + ... per light           3   (three lights at most; the ambient product's own rounding is on a shorter path)
                                     16
    Behind filters the filter itself is an f32 chain whose ORDER is the tree's, not the ray's: per crossing Ka * tex, w * alpha, 1 - alpha,
    filter * rgb, * (1 - alpha) = 5 more.  powf: its f32 argument may move by one ulp (2^-23 relative), which the exponent multiplies by the
    shininess, and its result carries P ulp: (shininess + P) * 2^-23 of each specular term (that is powabs).  1e-30 absorbs denormal products."""
    return (K_COMPUTE + K_CROSSING * crossings) * U * sumabs + powabs + 1e-30


def bound_filter(filt, ncross):
    return K_CROSSING * np.maximum(ncross, 1)[:, None] * U * np.abs(filt) + 1e-30


def trace(world, o, d, refr, energy, keys, mistake=None, depth=0):
    """Scene::trace (scene.rs:163-252).  Returns (colour (n, 3), bound (n, 3)).  The bound follows the recursion: a NormalMaterial colour is
    2 U (the normal's cast and the sum 1 + n; / 2 is exact), a Phong colour bound_compute, and a level's blend
        alpha = obj.w * sn.alpha, 1 - mix, obj * (1 - mix), refl * mix, +, * alpha, 1 - alpha, refr * (1 - alpha), +   = 9 roundings (K_BLEND)
    of results no larger than S = |obj| |1 - mix| |alpha| + |refl| |mix| |alpha| + |refr| |1 - alpha|, plus the children's bounds with the
    weights they are blended with."""
    n = len(o)
    col, err = np.zeros((n, 3)), np.zeros((n, 3))
    if n == 0:
        return col, err
    assert depth < 64
    t, nrm, sid = closest(world, o, d)
    miss = sid < 0
    col[miss] = f32(world.background)
    energy = np.asarray(energy, F32)
    for si in np.unique(sid[~miss]):
        s = world.surfs[si]
        ix = np.nonzero(sid == si)[0]
        oo, dd, nn, rr, ee, kk = o[ix], d[ix], nrm[ix], refr[ix], energy[ix], keys[ix]
        pt = oo + dd * t[ix][:, None]
        smp = light_samples(world, pt, kk) if s.mat.kind == "phong" else []
        crossings = max([int(x[3].max()) for x in smp] + [0])
        obj, w, sumabs, powabs = compute(s.mat, world.lights, smp, pt, nn, dd, s.has_uv, np.zeros((len(ix), 2)), mistake)
        eobj = 2.0 * U * np.ones_like(obj) if s.mat.kind == "normal" else bound_compute(sumabs, powabs, crossings)
        mix = float(s.mix)
        # trace_reflection, scene.rs:196-218
        refl, erefl = np.zeros_like(obj), np.zeros_like(obj)
        go = (ee >= F01) if mistake == "energy_ge" else (ee > F01)
        if mix != 0.0 and go.any():
            g = np.nonzero(go)[0]
            rdir = dd[g] - (nn[g] * _dot(dd[g], nn[g])[:, None]) * 2.0
            if mistake == "reflect_normalised":
                rdir = _unit(rdir)
            refl[g], erefl[g] = trace(world, pt[g] + rdir * 0.001, rdir, rr[g], ee[g] - F32(s.att), _rng_hash(kk[g], 0x100), mistake, depth + 1)
        alpha = (w.astype(F32) * F32(s.alpha)).astype(np.float64)
        one_mix = f32(1.0 - mix)
        obj_color = obj * one_mix + refl * ((1.0 - mix) if mistake == "blend_one_minus_mix_on_refl" else mix)
        # trace_refraction, scene.rs:221-252
        refc, erefc = np.zeros_like(obj), np.zeros_like(obj)
        g = np.nonzero(alpha != 1.0)[0]
        if len(g):
            first = rr[g] == 1.0
            n1, n2 = np.where(first, 1.0, s.coeff), np.where(first, s.coeff, 1.0)
            if mistake == "swap_n1_n2":
                n1, n2 = n2, n1
            along = nn[g] * _dot(dd[g], nn[g])[:, None]
            tangent = dd[g] - along
            ratio = n1 / n2 if mistake == "tangent_n1_over_n2" else n2 / n1
            ndir = _unit(along + tangent * ratio[:, None])
            refc[g], erefc[g] = trace(world, pt[g] + ndir * 0.001, ndir, n2, ee[g], _rng_hash(kk[g], 0x101), mistake, depth + 1)
        a = alpha[:, None]
        blended = np.where(a == 1.0, obj_color, obj_color * a + refc * (1.0 - a))
        S = np.abs(obj) * abs(one_mix) * np.abs(a) + np.abs(refl) * abs(mix) * np.abs(a) + np.abs(refc) * np.abs(1.0 - a)
        col[ix] = blended
        err[ix] = K_BLEND * U * S + eobj * abs(one_mix) * np.abs(a) + erefl * abs(mix) * np.abs(a) + erefc * np.abs(1.0 - a)
    return col, err


# ---------------------------------------------------------------------------------------------------------------- case set A and B
_GREY = dict(ka=(0.125, 0.0625, 0.1), kd=(0.7, 0.5, 0.9), ks=(0.6, 0.8, 0.4))
MATS = [Mat(shininess=s, **_GREY) for s in (0.0, 0.5, 1.0, 17.0, 300.0, 2000.0)] + [
    Mat(ka=(0.1, 0.1, 0.1), kd=(0.9, 0.8, 0.7), ks=(0, 0, 0), shininess=40.0),                        # no_specular
    Mat(ka=(0.05, 0.1, 0.15), kd=(0, 0, 0), ks=(1.0, 0.9, 0.8), shininess=5.0),                       # no diffuse
    Mat(ka=(0.2, 0.3, 0.1), kd=(0.8, 0.6, 0.9), ks=(0.5, 0.5, 0.5), shininess=9.0, tex=(51, 204, 119, 255), alpha_tex=102),  # needs a uv
    Mat("normal"), Mat("uv")]
TEXTURED = 8
LIGHT_SETS = {
    "one": [LightSpec((1.0, 5.0, -2.0), 0.0, 1, (0.9, 0.8, 0.7))],
    "three": [LightSpec((1.0, 5.0, -2.0), 0.0, 1, (0.9, 0.2, 0.1)), LightSpec((-4.0, 3.0, 3.0), 0.0, 1, (0.1, 0.7, 0.3)),
              LightSpec((0.0, -60.0, 0.0), 0.0, 1, (0.4, 0.4, 0.9))],                                  # the third is below every surface
    "area": [LightSpec((2.0, 6.0, -4.0), 0.4, 4, (0.8, 0.8, 0.7)), LightSpec((-4.0, 3.0, -3.0), 0.0, 1, (0.3, 0.3, 0.4))],
}
N_RANDOM = 480
RACSAMPLE_NSAMPLES = (1, 2, 3, 4, 5, 9, 10)


def _far_balls():
    return [Surf("ball", m, p0=(1000.0 + 10.0 * i, 1000.0, 1000.0), r=1e-3) for i, m in enumerate(MATS)]


def _directed(L):
    """(point, normal, view) relative to a point light at L; the light direction of every one is exactly (0, 1, 0) unless stated."""
    L = np.asarray(L, np.float64)
    p = L - np.array([0.0, 4.0, 0.0])
    t, m = DENORM_MIN, FLT_MIN
    ob = np.array([0.6, 0.8, 0.0])
    rows = [
        (p, (1, 0, 0), (0, 1, 0)),                  # n.l exactly 0; the mirrored light is -l: scoeff exactly 1 with no diffuse term
        (p, (1, 0, 0), (-0.6, -0.8, 0)),            # n.l exactly 0; scoeff < 0
        (p, (1, t, 0), (0.6, 0.8, 0)),              # n.l = +1 ulp of f32 around 0
        (p, (1, -t, 0), (0.6, 0.8, 0)),             # n.l = -1 ulp
        (p, (1, m, 0), (0.6, 0.8, 0)), (p, (1, -m, 0), (0.6, 0.8, 0)),
        (L + np.array([0.0, 4.0, 0.0]), (0, 1, 0), (0, 1, 0)),    # the light exactly behind: l = -n; mirrored l = n ... scoeff = -1
        (L + np.array([0.0, 4.0, 0.0]), (0, 1, 0), (0, -1, 0)),   # ... and scoeff = +1: a specular term from a light behind the surface
        (p, (0, 1, 0), (1, 0, 0)),                  # scoeff exactly 0
        (p, (0, 1, 0), (1, -t, 0)),                 # scoeff the smallest positive f32 (with shininess 0 the whole specular colour)
        (p, (0, 1, 0), (1, -m, 0)),                 # scoeff the smallest positive normal f32
        (p, (0, 1, 0), (1, t, 0)),                  # scoeff the largest negative f32
        (p, ob, -(2.0 * ob * ob[1] - np.array([0.0, 1.0, 0.0]))),   # the view along the mirrored light: scoeff -> 1
        (p, ob * 0.5, (0.28, -0.96, 0)), (p, ob * 2.0, (0.28, -0.96, 0)),          # normals that are not unit
        (p, ob, np.array([0.28, -0.96, 0]) * 0.5), (p, ob, np.array([0.28, -0.96, 0]) * 2.0),   # views that are not unit
        (p, ob * 2.0, np.array([-0.6, -0.64, 0.48]) * 0.5),
        (p, (0, 1, 0), (0.6, 0.8, 0)), (p, ob, (0.8, 0.6, 0)),                    # the normal faces away from the viewer
    ]
    return [np.array([np.asarray(x, np.float64) for x in r]) for r in rows]


def points_set(light_set, seed=SEED, n_random=N_RANDOM):
    """The points of set A / B for one light set: dict of the shade_points arguments plus `directed` (mask)."""
    lights = LIGHT_SETS[light_set]
    rng = np.random.default_rng(seed + len(light_set))
    nm = len(MATS)
    p = rng.uniform((-3.0, -1.0, -3.0), (3.0, 2.0, 3.0), size=(n_random, 3))
    nrm, view = _unit(rng.normal(size=(n_random, 3))), _unit(rng.normal(size=(n_random, 3)))
    if light_set == "three":   # every normal faces up: the light below is behind every surface
        nrm[:, 1] = np.abs(nrm[:, 1]) + 0.3
        nrm = _unit(nrm)
    scale = np.where(np.arange(n_random) % 7 == 3, 0.5, np.where(np.arange(n_random) % 7 == 5, 2.0, 1.0))[:, None]
    nrm, view = nrm * scale, view * scale[::-1]
    node = np.arange(n_random) % nm
    ed = _directed(lights[0].pos)
    ep = np.array([e[0] for e in ed for _ in range(nm)])
    en = np.array([e[1] for e in ed for _ in range(nm)])
    ev = np.array([e[2] for e in ed for _ in range(nm)])
    enode = np.tile(np.arange(nm), len(ed))
    points, normals, views = np.concatenate([p, ep]), np.concatenate([nrm, en]), np.concatenate([view, ev])
    nodes = np.concatenate([node, enode]).astype(np.int32)
    n = len(points)
    # scoeff <= |view|: a view twice the unit length raised to a shininess above 17 leaves f32's range, so those materials get it halved instead
    steep = np.array([m.kind == "phong" and m.shininess > 17.0 for m in MATS])[nodes] & ((views * views).sum(axis=1) > 1.5)
    views = np.where(steep[:, None], views * 0.25, views)
    uvs = np.random.default_rng(seed + 7).uniform(-1.0, 2.0, size=(n, 2))
    has_uv = (nodes == TEXTURED) | ((nodes == len(MATS) - 1) & (np.arange(n) % 2 == 0))    # the textured material, and half of the UV material's points
    flags = (1 | np.where(has_uv, 2, 0)).astype(np.uint32)
    keys = np.random.default_rng(seed + 11).integers(0, 2 ** 63, size=n, dtype=np.int64).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    directed = np.arange(n) >= n_random
    return dict(points=points, normals=normals, views=views, nodes=nodes, uvs=uvs, has_uv=has_uv, flags=flags, keys=keys, directed=directed, lights=lights)


def world_a(light_set):
    return World(_far_balls(), LIGHT_SETS[light_set], (0.0, 0.0, 0.0))


LIGHTS_B = [LightSpec((1.0, 7.0, 2.0), 0.0, 1, (0.9, 0.8, 0.7)),       # above the three horizontal filters
            LightSpec((-2.0, 2.5, 1.0), 0.0, 1, (0.2, 0.5, 0.3)),      # below them all: never filtered
            LightSpec((-1.0, 5.0, -1.0), 0.5, 4, (0.6, 0.6, 0.9)),     # area light between the quad and the NormalMaterial plane
            LightSpec((12.0, 1.0, 0.0), 0.0, 1, (0.7, 0.7, 0.7))]      # beyond the UVMaterial plane: lit, with a filter of exactly 0
LIGHT_SETS["filters"] = LIGHTS_B


def world_b():
    """The far balls of set A, then: a transparent Phong Plane (no uv: Ka, w = 1), a textured quad whose colour exceeds 1 (Ka 1.5 x texel)
    with an opacity texel, a NormalMaterial plane, a UVMaterial plane without uvs (w = 0: fully transparent, rgb 0), an opaque blocker."""
    glass = Mat(ka=(0.9, 0.7, 0.5))
    quad = Mat(ka=(1.5, 0.75, 1.25), tex=(255, 204, 153, 255), alpha_tex=102)
    solid = Mat(ka=(0.3, 0.3, 0.3))
    return World(_far_balls() + [
        Surf("plane", glass, p0=(0, 3.25, 0), n=(0, -1, 0), alpha=0.5),
        Surf("quad", quad, p0=(0, 4.0, 0), lo=(-3.0, -2.5), hi=(1.5, 2.5), alpha=0.75),
        Surf("plane", Mat("normal"), p0=(0, 6.0, 0), n=(0, -1, 0), alpha=0.625),
        Surf("plane", Mat("uv"), p0=(8.0, 0, 0), n=(-1, 0, 0), alpha=1.0),
        Surf("quad", solid, p0=(0, 3.5, 0), lo=(1.75, -2.0), hi=(4.0, 3.0), alpha=1.0)], LIGHTS_B, (0.0, 0.0, 0.0))


def expected_points(world, c, mistake=None):
    """The restatement on a points set: colour+alpha (n, 4), bound (n, 4), keep mask (the input rule), samples."""
    n = len(c["points"])
    smp = light_samples(world, c["points"], c["keys"], mistake)
    margin = np.min([s[4].min(axis=1) for s in smp], axis=0)
    crossings = np.max([s[3].max(axis=1) for s in smp], axis=0)
    keep = ~(margin < 1e-6)
    assert keep[c["directed"]].all(), "a directed case lies on a quad's edge"
    assert (~keep).sum() < 0.02 * n
    col, err = np.zeros((n, 4)), np.zeros((n, 4))
    for mi, mat in enumerate(MATS):
        ix = np.nonzero(c["nodes"] == mi)[0]
        sub = [tuple(a[ix] for a in s) for s in smp]
        rgb, alpha, sumabs, powabs = compute(mat, world.lights, sub, c["points"][ix], c["normals"][ix], c["views"][ix], c["has_uv"][ix], c["uvs"][ix], mistake)
        col[ix, :3], col[ix, 3] = rgb, alpha
        err[ix, :3] = bound_compute(sumabs, powabs, crossings[ix][:, None])
    return col, err, keep, smp


def shadow_rays_set(world, c):
    """Set B's shadow rays themselves: origins, dirs, max_toi (m, ...), and the restatement's lit, filter, bound, keep."""
    positions = light_positions(world.lights, c["keys"])
    rays = shadow_rays_of(c["points"], positions)
    o = np.concatenate([r[0].reshape(-1, 3) for r in rays])
    d = np.concatenate([r[1].reshape(-1, 3) for r in rays])
    mt = np.concatenate([r[2].reshape(-1) for r in rays])
    directed = np.concatenate([np.repeat(c["directed"], r[2].shape[1]) for r in rays])
    lit, filt, nc, margin = shadow(world, o, d, mt)
    keep = ~(margin < 1e-6)
    assert keep[directed].all() and (~keep).sum() < 0.02 * len(o)
    return o, d, mt, lit, filt, bound_filter(filt, nc), keep


# ---------------------------------------------------------------------------------------------------------------- case set C
MIX_ALPHA = ((0.0, 0.25), (0.5, 1.0), (0.3, 0.4), (1.0, 0.0), (0.25, 0.5), (-0.0, 1.0), (0.3, 1.5))
COEFFS = (1.0, 0.7, 1.3, 1.5, 4.0)
CALLER_REFR = (1.0, 1.5, float(np.nextafter(1.0, 2.0)))
ENERGIES = (1.0, float(F01), float(np.nextafter(F01, F32(1.0))), 0.05)
ATTENUATION = 0.45
BALL_R = 50.0
PROBE_STEP = 200.0
N_DIRS = 28


def _rounding_energy():
    """(energy, attenuation) for which `energy - attenuation` in f32 and in exact arithmetic fall on different sides of `> 0.1f`: the exact
    difference lies less than half an ulp above 0.1f and rounds down to it."""
    att = F32(0.00123)
    for _ in range(64):
        e = F32(float(F01) + float(att))
        for _ in range(8):
            if (F32(e - att) > F01) != (float(e) - float(att) > float(F01)):
                return float(e), float(att)
            e = np.nextafter(e, F32(1.0))
        att = np.nextafter(att, F32(1.0))
    raise AssertionError("no such energy")


ENERGY_ROUNDS, ATT_ROUNDS = _rounding_energy()


def probe_world(quad=False):
    """35 probes, probe i centred on (0, 200 i, 0): a surface through the centre with normal +y, Kd = Ks = 0 (obj is the ambient colour exactly;
    the quad: Ka x texel, with an opacity texel of 0 for (mix, alpha) = (1, 0) — the mesh kernel's transparent-hit elision — else 255), inside a
    non-solid NormalMaterial ball of radius 50 (mix 0, alpha 1).  No lights."""
    surfs = []
    for i, ((mix, alpha), coeff) in enumerate([(ma, c) for ma in MIX_ALPHA for c in COEFFS]):
        c = (0.0, PROBE_STEP * i, 0.0)
        if quad:
            transparent = (mix, alpha) == (1.0, 0.0)
            mat = Mat(ka=(0.8, 0.4, 0.6), tex=(102, 255, 51, 255), alpha_tex=0 if transparent else 255)
            node_alpha = 1.0 if transparent else alpha
            surfs.append(Surf("quad", mat, p0=c, lo=(-3.0, -2.0), hi=(5.0, 6.0), mix=mix, att=ATTENUATION, alpha=node_alpha, coeff=coeff))
        else:
            surfs.append(Surf("plane", Mat(ka=(0.3, 0.6, 0.2)), p0=c, n=(0, 1, 0), mix=mix, att=ATTENUATION, alpha=alpha, coeff=coeff))
        surfs.append(Surf("ball", Mat("normal"), p0=c, r=BALL_R))
    return World(surfs, [], (0.1, 0.2, 0.3))


def probe_rays(n_probes=len(MIX_ALPHA) * len(COEFFS), seed=SEED):
    """Rays aimed at each probe's centre from inside its ball: (origins, dirs, refr, energy, keys).  Per probe and caller refr: N_DIRS random
    directions from the upper hemisphere, normal incidence (tangent exactly 0), grazing incidence (1e-6 rad), two obliques; per probe and other
    energy: 6 directions with refr 1.0 and 1.5."""
    rng = np.random.default_rng(seed)
    fixed = np.array([[0.0, -1.0, 0.0], [np.cos(1e-6), -np.sin(1e-6), 0.0], [0.6, -0.8, 0.0], [-0.48, -0.6, 0.64]])
    o, d, r, e = [], [], [], []
    for i in range(n_probes):
        c = np.array([0.0, PROBE_STEP * i, 0.0])
        for refr in CALLER_REFR:
            dirs = _unit(rng.normal(size=(N_DIRS, 3)))
            dirs[:, 1] = -np.abs(dirs[:, 1])
            dirs = np.concatenate([dirs, fixed])
            dist = rng.uniform(5.0, 40.0, size=(len(dirs), 1))
            o.append(c - dirs * dist); d.append(dirs); r.append(np.full(len(dirs), refr)); e.append(np.ones(len(dirs)))
        for en in ENERGIES[1:] + (ENERGY_ROUNDS,):
            dirs = _unit(rng.normal(size=(6, 3)))
            dirs[:, 1] = -np.abs(dirs[:, 1])
            o.append(c - dirs * 20.0); d.append(dirs); r.append(np.where(np.arange(6) % 2 == 0, 1.0, 1.5)); e.append(np.full(6, en))
    o, d, r, e = np.concatenate(o), np.concatenate(d), np.concatenate(r), np.concatenate(e).astype(F32)
    return o, d, r, e, np.arange(len(o), dtype=np.uint64)


def slab_world():
    """Two parallel planes (refr_coeff 1.5 above 1.3, alpha 0.5 each, both reflecting) inside one ball: the second refraction is decided by the
    refr the first continuation carries, the reflections between the planes by the energy it carries (the lower plane's attenuation is the one
    for which ENERGY_ROUNDS - attenuation rounds across 0.1f: the upper plane, met from below, reflects once more or not)."""
    return World([Surf("plane", Mat(ka=(0.3, 0.6, 0.2)), p0=(0, 0, 0), n=(0, 1, 0), mix=0.3, att=ATTENUATION, alpha=0.5, coeff=1.5),
                  Surf("plane", Mat(ka=(0.7, 0.2, 0.5)), p0=(0, -2.0, 0), n=(0, 1, 0), mix=0.25, att=ATT_ROUNDS, alpha=0.5, coeff=1.3),
                  Surf("ball", Mat("normal"), p0=(0, 0, 0), r=BALL_R)], [], (0.1, 0.2, 0.3))


def slab_rays(seed=SEED + 1, n=40):
    rng = np.random.default_rng(seed)
    o, d, r, e = [], [], [], []
    for refr in CALLER_REFR:
        for en in ENERGIES + (ENERGY_ROUNDS, 0.56, 0.4):
            dirs = _unit(rng.normal(size=(n, 3)))
            dirs[:, 1] = -np.abs(dirs[:, 1]) - 0.05
            dirs = np.concatenate([_unit(dirs), [[0.0, -1.0, 0.0]]])
            o.append(rng.uniform(-3.0, 3.0, size=(len(dirs), 3)) * (1, 0, 1) - dirs * rng.uniform(4.0, 30.0, size=(len(dirs), 1)))
            d.append(dirs); r.append(np.full(len(dirs), refr)); e.append(np.full(len(dirs), en))
    o, d, r, e = np.concatenate(o), np.concatenate(d), np.concatenate(r), np.concatenate(e).astype(F32)
    return o, d, r, e, np.arange(len(o), dtype=np.uint64)


def mirror_world():
    """A half mirror (Kd = Ks = 0) under a lit Phong ceiling whose normal faces down, shininess 2: a reflected ray's direction is the view of the
    ceiling's specular term, so the LENGTH of the unnormalised reflected direction (the caller's rays are 0.5 x and 2 x unit here) is observable."""
    return World([Surf("plane", Mat(ka=(0.3, 0.6, 0.2)), p0=(0, 0, 0), n=(0, 1, 0), mix=0.5, att=ATTENUATION, alpha=1.0, coeff=1.0),
                  Surf("plane", Mat(ka=(0.1, 0.1, 0.1), kd=(0.5, 0.6, 0.7), ks=(0.9, 0.8, 0.7), shininess=2.0), p0=(0, 10.0, 0), n=(0, -1, 0)),
                  Surf("ball", Mat("normal"), p0=(0, 0, 0), r=BALL_R)],
                 [LightSpec((1.0, 4.0, -2.0), 0.0, 1, (0.9, 0.9, 0.8)), LightSpec((-3.0, 6.0, 1.0), 0.3, 4, (0.3, 0.4, 0.5))], (0.1, 0.2, 0.3))


def mirror_rays(seed=SEED + 2, n=60):
    rng = np.random.default_rng(seed)
    dirs = _unit(rng.normal(size=(n, 3)))
    dirs[:, 1] = -np.abs(dirs[:, 1]) - 0.3
    dirs = _unit(dirs)
    o = rng.uniform(-2.0, 2.0, size=(n, 3)) * (1, 0, 1) - dirs * rng.uniform(3.0, 9.0, size=(n, 1))
    scale = np.where(np.arange(n) % 3 == 0, 0.5, np.where(np.arange(n) % 3 == 1, 2.0, 1.0))[:, None]
    keys = np.random.default_rng(seed + 1).integers(0, 2 ** 63, size=n, dtype=np.int64).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    return o, dirs * scale, np.ones(n), np.ones(n, F32), keys


FRAME = dict(resolution=(16, 12), eye=(3.0, 20.0, -25.0), at=(0.5, 0.0, 1.0), fovy=50.0, seed=3)


def frame_world(quad):
    """Probe 12 ((mix, alpha) = (0.3, 0.4), refr_coeff 1.3: both continuations) alone, at the origin, for a render from inside the ball."""
    w = probe_world(quad)
    s, b = w.surfs[2 * 12], w.surfs[2 * 12 + 1]
    s.p0, b.p0 = np.zeros(3), np.zeros(3)
    return World([s, b], [], w.background)


def frame_rays():
    w, h = FRAME["resolution"]
    proj = math3d.inverse_projection(FRAME["eye"], FRAME["at"], FRAME["fovy"], w, h)
    o, d, k = nr.camera_rays((w, h), FRAME["eye"], proj, seed=FRAME["seed"])
    return o, d, k, proj


def expected_frame(world):
    """scene.rs:71-94 at one ray per pixel: the pixel is the traced colour (0 + c, / 1.0: exact).  No ray may pass within 1e-6 of a quad's edge."""
    o, d, k, _ = frame_rays()
    for s in world.surfs:
        assert not (hits(s, o, d)[2] < 1e-6).any()
    col, err = trace(world, o, d, np.ones(len(o)), np.ones(len(o), F32), k)
    w, h = FRAME["resolution"]
    return col.reshape(h, w, 3), err.reshape(h, w, 3)


def worst_ratio(got, want, err, keep=None, finite=True):
    """max |got - want| / bound over the kept cases.  `finite`: every value under test must be finite (a mistaken restatement may overflow;
    its overflowed values are left out, so a mistake has to show in a finite value)."""
    got = np.asarray(got, np.float64)
    if finite:
        assert np.isfinite(got).all()
    with np.errstate(invalid="ignore", over="ignore"):
        ratio = np.abs(got - want) / err
    ratio = np.where(np.isfinite(got), ratio, 0.0)
    if keep is not None:
        ratio = ratio[keep]
    return float(ratio.max())


TRACE_CASES = {"probe": lambda: (probe_world(False), probe_rays()), "quad_probe": lambda: (probe_world(True), probe_rays()),
               "slab": lambda: (slab_world(), slab_rays()), "mirror": lambda: (mirror_world(), mirror_rays())}


def shade_args(c):
    """The arguments of shade_points (and of the oracle's shim) for a points set."""
    return dict(points=c["points"], normals=c["normals"], view_dirs=c["views"], nodes=c["nodes"], uvs=c["uvs"], hit_flags=c["flags"], keys=c["keys"])


def report(name, ratio):
    """Prints a figure before it is asserted on."""
    print("%s: worst |error| / bound = %.4f" % (name, ratio))
    return ratio
