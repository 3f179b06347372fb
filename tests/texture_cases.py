"""Texture2d::sample (texture2d.rs:207-256) restated in numpy, and the table of textures and coordinates the texture tests share.

Tests only; nothing here comes from oracle/ or from the product package.

sample_ref() follows the reference statement by statement in f32:
  * `coords.x as f32`;
  * ClampToEdges: nalgebra's `clamp(val, min, max) = if val > min { if val < max { val } else { max } } else { min }` — a NaN
    compares false and becomes `min` (0.0), -0.0 becomes +0.0; Wrap: `% 1.0` is np.fmod(x, 1) (sign of x), then `1.0 + x` if x < 0;
  * times `(dim - 1) as f32`;
  * `as usize` is Rust's saturating cast: negative and NaN -> 0;
  * the ONE deviation of the project (DESIGN D-6): every tap index is clamped to dim - 1 (the reference indexes past the row / panics);
  * Nearest: f32::round, half away from zero;
  * Bilinear: taps (low, high) per axis, shift = x - (low as f32) in f32.
It returns the taps, the f32 weights and the blend of those taps and weights evaluated in f64 (the f32 blend of the code under test is
compared with that value inside a derived bound; see tests/test_texture_sample.py).

Textures: 1x1, 1x5, 5x1, 2x2, 3x7, 8x8, 257x3 (width x height), each as RGBA8 bytes and as the RGBA32F array texel_ref(bytes).  Every channel
is a multiple of 17 (= 255 / 15).  r, g, b are the three base-16 digits of a hashed permutation of the texel index, so any two texels of a
texture differ by >= 17/255 in some channel; alpha is (x + 4 y + hash) mod 16, so that a texel differs in alpha from all its eight
neighbours and a texture of 64 or more texels (8x8, 257x3) holds exactly 0.0 and exactly 1.0 next to values in between (the alpha-only observables
see nothing but this channel).  Both properties are asserted at import: a wrong tap moves a result by far more than any rounding.
"""
import numpy as np

F32 = np.float32
BILINEAR, NEAREST = 0, 1      # NraysInterp   (the values of nrays_amd.Interpolation, asserted by the tests)
WRAP, CLAMP = 0, 1            # NraysOverflow (nrays_amd.Overflow)
SIZES = ((1, 1), (1, 5), (5, 1), (2, 2), (3, 7), (8, 8), (257, 3))  # (width, height)
MAX_PAIRS = 4096
SEED = 0x7E57CA5E
MIN_SEPARATION = 16.0 / 255.0


# ----------------------------------------------------------------------------------------------- textures
def _mix(z):
    """splitmix64 finaliser on python ints."""
    z &= (1 << 64) - 1
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & ((1 << 64) - 1)
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & ((1 << 64) - 1)
    return z ^ (z >> 31)


def texel_ref(b):
    """`u8 as f32 / 255.0` (texture2d.rs:111-162)."""
    return np.asarray(b).astype(F32) / F32(255.0)


def texture_bytes(width, height):
    """(height, width, 4) uint8, row 0 first (ImageData's layout: texel (x, y) at [y, x])."""
    h0 = _mix(SEED ^ (width << 20) ^ height)
    mul, add, a0 = (h0 | 1) & 4095, (h0 >> 12) & 4095, (h0 >> 24) & 15
    out = np.zeros((height, width, 4), np.uint8)
    for y in range(height):
        for x in range(width):
            p = ((y * width + x) * mul + add) & 4095  # odd multiplier: a permutation of 0 .. 4095 (width * height <= 4096)
            out[y, x] = (17 * (p & 15), 17 * ((p >> 4) & 15), 17 * ((p >> 8) & 15), 17 * ((x + 4 * y + a0) & 15))
    return out


def _check_texture(b):
    h, w, _ = b.shape
    assert w * h <= 4096
    flat = texel_ref(b).reshape(-1, 4).astype(np.float64)
    if len(flat) > 1:
        d = np.abs(flat[:, None, :] - flat[None, :, :]).max(axis=2)
        d[np.arange(len(flat)), np.arange(len(flat))] = 1.0
        assert d.min() >= MIN_SEPARATION, (w, h, d.min())          # two distinct texels: some channel apart
    a = flat.reshape(h, w, 4)[:, :, 3]
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if (dx or dy):
                ys, xs = np.mgrid[0:h, 0:w]
                y2, x2 = ys + dy, xs + dx
                ok = (y2 >= 0) & (y2 < h) & (x2 >= 0) & (x2 < w)
                assert (np.abs(a[ys[ok], xs[ok]] - a[y2[ok], x2[ok]]) >= MIN_SEPARATION).all(), (w, h, dx, dy)  # alpha: the eight neighbours
    if w * h >= 64:
        assert (a == 0.0).any() and (a == 1.0).any() and ((a > 0.0) & (a < 1.0)).any()


TEXTURES = {}  # (width, height) -> {"rgba8": uint8 (h, w, 4), "rgba32f": float32 (h, w, 4)}
for _w, _h in SIZES:
    _b = texture_bytes(_w, _h)
    _check_texture(_b)
    TEXTURES[(_w, _h)] = {"rgba8": _b, "rgba32f": texel_ref(_b)}
FORMATS = ("rgba8", "rgba32f")


# ----------------------------------------------------------------------------------------------- coordinates
_INF = F32(np.inf)
DENORM_MIN = np.array([1], np.uint32).view(F32)[0]
FLT_MIN = np.finfo(F32).tiny
BASE_VALUES = np.array([
    0.0, -0.0, 1.0, np.nextafter(F32(1), F32(0)), np.nextafter(F32(1), F32(2)), 0.5, 0.25,
    DENORM_MIN, -DENORM_MIN, FLT_MIN, -FLT_MIN,
    F32(-1e-8),                                    # 1 + ux rounds to 1.0f
    -0.25, -1.0, -1.75, 1.25, 2.0, 7.0, -3.0,
    8388607.5, 16777216.0, F32(1e30), F32(-1e30)], dtype=F32)
assert F32(1) + F32(-1e-8) == F32(1)
NONFINITE_VALUES = np.array([np.inf, -np.inf, np.nan], dtype=F32)
RANDOM_VALUES = np.random.default_rng(SEED).uniform(-2.0, 3.0, 200).astype(F32)


def boundary_values(n):
    """For a dimension n > 1 and every k: the f32 nearest to k / (n - 1) (a texel centre: the floor of the scaled coordinate changes there) and to
    (k + 0.5) / (n - 1) (a tie of Nearest), each with its two f32 neighbours.  Returns (values, exact): `exact` marks the values whose f32 product
    with (n - 1) IS k or k + 0.5; every k has one among its three (asserted)."""
    vals, exact = [], []
    m = F32(n - 1)
    for k in range(n):
        for target in ((float(k),) if k == n - 1 else (float(k), k + 0.5)):
            c = F32(target / (n - 1))
            trio = [np.nextafter(c, -_INF), c, np.nextafter(c, _INF)]
            ex = [bool(x * m == F32(target)) for x in trio]
            assert any(ex), (n, target)
            vals += trio
            exact += ex
    return np.array(vals, F32), np.array(exact)


def axis_values(n):
    """Every finite coordinate value of one axis of dimension n, each bit pattern once (-0.0 and 0.0 are two)."""
    v = np.concatenate([BASE_VALUES, boundary_values(n)[0] if n > 1 else np.zeros(0, F32), RANDOM_VALUES]).astype(F32)
    _, first = np.unique(v.view(np.uint32), return_index=True)
    return v[np.sort(first)]


def centre_values(n):
    """One coordinate per texel k of a dimension n whose f32 product with (n - 1) is exactly k."""
    if n == 1:
        return np.zeros(1, F32)
    vals, exact = boundary_values(n)
    scaled = vals * F32(n - 1)
    return np.array([vals[exact & (scaled == F32(k))][0] for k in range(n)], F32)


def pairs(width, height):
    """(n, 2) f32: the u values of `width` paired with the v values of `height` by a fixed-seed shuffle (the shorter list repeats):
    every value of each axis at least once, no full product.  A shuffle almost never puts BOTH coordinates on a texel centre, so for the
    textures of up to 64 texels the centres of all their texels follow (there a Bilinear sample is one texel exactly: the alpha values 0 and 1)."""
    rng = np.random.default_rng(SEED ^ (width << 16) ^ height)
    u, v = axis_values(width), axis_values(height)
    n = max(len(u), len(v))
    u, v = np.resize(rng.permutation(u), n), np.resize(rng.permutation(v), n)
    out = np.stack([u, v], axis=1).astype(F32)
    if width * height <= 64:
        cu, cv = np.meshgrid(centre_values(width), centre_values(height))
        out = np.concatenate([out, np.stack([cu.ravel(), cv.ravel()], axis=1).astype(F32)])
    assert len(out) <= MAX_PAIRS
    return out


def nonfinite_pairs(with_nan=True):
    """(n, 2) f32: +inf, -inf (and NaN) on one axis against finite values and against each other on the other axis, both ways round."""
    nf = NONFINITE_VALUES if with_nan else NONFINITE_VALUES[:2]
    others = np.concatenate([np.array([0.0, 0.25, 1.0, -0.75, 0.6], F32), nf])
    out = [(a, b) for a in nf for b in others] + [(b, a) for a in nf for b in others[:5]]
    return np.array(out, dtype=F32)


# ----------------------------------------------------------------------------------------------- the reference
class Sample:
    """taps: Nearest (x, y); Bilinear (low_x, high_x, low_y, high_y) — int64 arrays, clamped to dim - 1 (D-6).
    weights: Bilinear (shift_x, 1 - shift_x, shift_y, 1 - shift_y) as f32 arrays, None for Nearest.
    value: (n, 4) float64 — the selected texel, or the f64 blend of the f32 taps with the f32 weights."""

    def __init__(self, taps, weights, value):
        self.taps, self.weights, self.value = taps, weights, value


def _overflow(x, overflow):
    if overflow == CLAMP:
        return np.where(x > F32(0), np.where(x < F32(1), x, F32(1)), F32(0)).astype(F32)  # na::clamp: NaN -> 0.0
    with np.errstate(invalid="ignore"):
        r = np.fmod(x, F32(1)).astype(F32)                                                # inf % 1 = NaN
    return np.where(r < F32(0), F32(1) + r, r).astype(F32)


def _as_usize(x):
    """Rust's `f32 as usize`: truncation, saturating; NaN and negative values -> 0."""
    x = np.asarray(x, np.float64)
    return np.where(x > 0.0, np.minimum(np.trunc(np.where(np.isnan(x), 0.0, x)), 2.0 ** 62), 0.0).astype(np.int64)


def _round_half_away(x):
    """f32::round.  |x| + 0.5 is exact in f64 for every f32 below 2^52."""
    x64 = np.asarray(x, np.float64)
    return np.where(np.abs(x64) < 2.0 ** 52, np.copysign(np.floor(np.abs(x64) + 0.5), x64), x64).astype(F32)


def sample_ref(texels, interp, overflow, u, v):
    """Texture2d::sample for arrays of coordinates.  texels: (height, width, 4) uint8 or float32."""
    texels = np.asarray(texels)
    t32 = texel_ref(texels) if texels.dtype == np.uint8 else texels.astype(F32)
    h, w, _ = t32.shape
    t64 = t32.astype(np.float64)
    ux = _overflow(np.atleast_1d(np.asarray(u)).astype(F32), overflow)
    uy = _overflow(np.atleast_1d(np.asarray(v)).astype(F32), overflow)
    ux = (ux * F32(w - 1)).astype(F32)
    uy = (uy * F32(h - 1)).astype(F32)
    if interp == NEAREST:
        x = np.minimum(_as_usize(_round_half_away(ux)), w - 1)
        y = np.minimum(_as_usize(_round_half_away(uy)), h - 1)
        return Sample((x, y), None, t64[y, x])
    low_x, low_y = _as_usize(np.floor(ux)), _as_usize(np.floor(uy))
    with np.errstate(invalid="ignore"):
        sx = (ux - low_x.astype(F32)).astype(F32)
        sy = (uy - low_y.astype(F32)).astype(F32)
        wx, wy = (F32(1) - sx).astype(F32), (F32(1) - sy).astype(F32)
    lx, hx = np.minimum(low_x, w - 1), np.minimum(low_x + 1, w - 1)
    ly, hy = np.minimum(low_y, h - 1), np.minimum(low_y + 1, h - 1)
    ul, ur, dr, dl = t64[hy, lx], t64[hy, hx], t64[ly, hx], t64[ly, lx]
    sx64, wx64, sy64, wy64 = (a.astype(np.float64)[:, None] for a in (sx, wx, sy, wy))
    with np.errstate(invalid="ignore"):
        ui = ul * wx64 + ur * sx64
        di = dl * wx64 + dr * sx64
        value = ui * sy64 + di * wy64
    return Sample((lx, hx, ly, hy), (sx, wx, sy, wy), value)
