"""tex_sample() / tex_at() of nrays_amd/csrc/trace_device.h on the device, in every mode and at their edges, against the independent numpy restatement
of Texture2d::sample (tests/texture_cases.py: sample_ref) — no oracle in between.

How exact coordinates reach the sampler: one TriMesh per texture of the table, one small triangle per (u, v) case, laid out on a grid in the plane
z = 0 with f32-exact vertices; the three vertices of a triangle carry the SAME uv (c_u, c_v) and one ray goes down -z through the point of the triangle
whose barycentric coordinates are (1/2, 1/4, 1/4).  The device interpolates c b0 + c b1 + c b2 in f64 and tex_sample casts the sum to f32: for an
f32-exact c the f64 error is far below half an f32 ulp, so the sampled coordinate IS c (-0.0 stays -0.0).  Every test first reads the device's own
uv through the cast probe and asserts exactly that, and that every ray hits its own triangle: a condition on the inputs, not on the sampler.

Bounds (u = 2^-24; texels, weights, alpha and colours in [0, 1]; the device code is built with -ffp-contract=off (__graft_entry__.py: HIP_FLAGS), and the bounds hold
with contraction too: a fused multiply-add only removes a rounding):
  sample     Nearest: bit equality.  Bilinear: |f32 blend - f64 blend of the reference's f32 taps and weights| <= 4 u (1 + 2^-20), derived in
             tests/test_texture_sample.py (two levels of fl(fl(a w) + fl(b s)), w = fl(1 - s) shared with the reference): SAMPLE.
  colour     Scene::trace with ka = 1, kd = ks = 0, no light, alpha 1, no reflection: rgb = fl(1 tex) (exact), own weight 1 (1 - 0) = 1, 0 + rgb: no rounding
             after the sample.  Bound: SAMPLE (Nearest: bit equality).
  filter     Scene::intersects_ray: alpha = fl(w 1) (exact); lit iff alpha < 1; filter = fl(fl(1 1) fl(1 - alpha)): ONE rounding of a value <= 1, and
             d(1 - w)/dw = -1 passes the sample's error on unchanged.  Bound: SAMPLE + u (Nearest: fl(1 - w) exactly).  Where the f64 blend lies within
             SAMPLE of 1 the f32 blend may legitimately land on either side of 1.0: there both outcomes of `alpha < 1` are accepted (the filter, if any,
             still has to be 1 - w within the bound); everywhere else lit == (w < 1).
  blend      Scene::trace with the alpha-only material over the background bg, the refraction ray traced (refr_coeff 1: straight on, it hits nothing):
             own term fl(ka fl(a (1 - 0))) = a (ka = 1: exact, counted as one rounding for any ka <= 1), refraction weight fl(1 - a), fl(bg fl(1 - a)),
             and the sum of the two terms: at most FOUR roundings of values <= 1, and |d/da (ka a + bg (1 - a))| = |ka - bg| <= 1.  Bound: SAMPLE + 4 u
             (Nearest: 4 u).  Exactly bg where a == 0 (the elided hit — trace_device.h: FULLY TRANSPARENT — and 0 + bg 1) and exactly ka where a == 1 (no
             refraction ray, ka 1).
A wrong tap moves a result by >= 16/255 = 0.06 (texture_cases: texel separation), five orders of magnitude above these bounds.
"""
import functools

import numpy as np
import pytest

import nrays_amd as nr
from nrays_amd import abi
from tests import texture_cases as tc

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
SAMPLE = 4.0 * U * (1.0 + 2.0 ** -20)
BG = (0.25, 0.5, 0.75)
MODES = [(f, i, o) for f in tc.FORMATS for i in (tc.BILINEAR, tc.NEAREST) for o in (tc.WRAP, tc.CLAMP)]
MODE_IDS = ["%s-%s-%s" % (f, "nearest" if i else "bilinear", "clamp" if o else "wrap") for f, i, o in MODES]
COLS, ROW_PITCH = 64, 80  # triangles per grid row; rows between two textures' blocks (the largest block has 28 rows)


class _Layout:
    """The meshes, rays and case coordinates of the seven textures: `uv` (n, 2) f32, `node` (n,), `first[t] : first[t + 1]` the rays of texture t."""

    def __init__(self, uv_of):
        self.meshes, uv, node, org, self.first = [], [], [], [], [0]
        for t, size in enumerate(tc.SIZES):
            c = uv_of(size)
            n = len(c)
            i = np.arange(n)
            x0, y0 = (i % COLS).astype(np.float64), (t * ROW_PITCH + i // COLS).astype(np.float64)
            assert (i // COLS).max() < ROW_PITCH
            pts = np.zeros((n, 3, 3))
            pts[:, :, 0], pts[:, :, 1] = x0[:, None], y0[:, None]
            pts[:, 1, 0] += 0.5
            pts[:, 2, 1] += 0.5
            # A NaN coordinate cannot be a mesh uv (nrays_scene_create refuses it) but it reaches the sampler all the same: the vertices carry +inf there and the ray
            # goes through the middle of the edge v0 v1 — barycentric (1/2, 1/2, 0) — so the device's inf 1/2 + inf 1/2 + inf 0 is NaN (an infinite coordinate
            # on the other axis of such a case becomes NaN with it, a finite one stays itself: c 1/2 + c 1/2 + c 0).
            nan_row = np.isnan(c).any(axis=1)
            mesh_uv = np.where(np.isnan(c), np.float32(np.inf), c)
            c = np.where(nan_row[:, None] & ~np.isfinite(c), np.float32(np.nan), c).astype(np.float32)
            self.meshes.append((pts.reshape(-1, 3), np.arange(3 * n, dtype=np.uint32).reshape(n, 3), np.repeat(mesh_uv.astype(np.float64), 3, axis=0)))
            org.append(np.stack([x0 + np.where(nan_row, 0.25, 0.125), y0 + np.where(nan_row, 0.0, 0.125), np.ones(n)], axis=1))  # else (1/2, 1/4, 1/4): exact dyadic weights
            uv.append(c)
            node.append(np.full(n, t))
            self.first.append(self.first[-1] + n)
        self.uv, self.node, self.origins = np.concatenate(uv).astype(np.float32), np.concatenate(node), np.concatenate(org)
        self.dirs = np.tile(np.asarray([0.0, 0.0, -1.0]), (len(self.uv), 1))
        self.max_toi = np.full(len(self.uv), 2.0)  # beyond the plane


@functools.lru_cache(maxsize=None)
def _layout(nonfinite=False):
    return _Layout((lambda size: tc.nonfinite_pairs()) if nonfinite else (lambda size: tc.pairs(*size)))


@functools.lru_cache(maxsize=None)
def _reference(fmt, interp, overflow, nonfinite=False):
    """(n, 4) f64: sample_ref over the layout's cases, computed once per mode and shared by the tests."""
    L = _layout(nonfinite)
    out = [tc.sample_ref(tc.TEXTURES[size][fmt], interp, overflow, L.uv[a:b, 0], L.uv[a:b, 1]).value
           for size, a, b in zip(tc.SIZES, L.first[:-1], L.first[1:])]
    out = np.concatenate(out)
    out.setflags(write=False)
    return out


def _scene(L, fmt, interp, overflow, role):
    """Seven nodes side by side, one per texture; role "colour": the texture is the material's colour texture, "alpha": its opacity map."""
    nodes = []
    for size, (pts, idx, uvs) in zip(tc.SIZES, L.meshes):
        tex = nr.Texture2d(nr.ImageData(tc.TEXTURES[size][fmt]), interp, overflow)
        mat = nr.PhongMaterial((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), tex if role == "colour" else None, tex if role == "alpha" else None, 1.0)
        nodes.append(nr.SceneNode(mat, 0.0, 0.0, 1.0, 1.0, nr.Isometry3(), nr.TriMesh(pts, idx, uvs)))
    return nr.Scene(nodes, [], BG)


def _check_inputs(sc, L):
    """Every ray hits its own triangle (toi 1, its node) and the device's interpolated uv, cast to f32, is the case's coordinate bit for bit."""
    hit, out = nr.cast_rays(sc, L.origins, L.dirs)
    assert hit.all()
    assert float(np.abs(out[:, 0] - 1.0).max()) <= 1e-12
    assert np.array_equal(out[:, 7], L.node) and (out[:, 4] == 1.0).all()
    got = out[:, 5:7].astype(np.float32)
    ok = ~np.isnan(L.uv)
    assert np.array_equal(got.view(np.uint32)[ok], L.uv.view(np.uint32)[ok])
    assert np.isnan(got[~ok]).all()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _worst(got, ref):
    return float(np.abs(got.astype(np.float64) - ref).max()) if len(got) else 0.0


@pytest.mark.parametrize("fmt,interp,overflow", MODES, ids=MODE_IDS)
def test_colour_texture_through_trace(gpu, monkeypatch, fmt, interp, overflow):
    monkeypatch.setenv("NRAYS_RAY_REORDER", "2")  # read when the handle is created: a batch called unordered is reordered whatever its size
    L = _layout()
    sc = _scene(L, fmt, interp, overflow, "colour")
    _check_inputs(sc, L)
    got = nr.trace_rays(sc, L.origins, L.dirs, max_depth=0)
    ref = _reference(fmt, interp, overflow)[:, :3]
    worst = _worst(got, ref)
    print("colour: worst |device - reference| = %.4g (bound %.4g)" % (worst, 0.0 if interp == tc.NEAREST else SAMPLE))
    if interp == tc.NEAREST:
        assert np.array_equal(_bits(got), _bits(ref))
    else:
        assert worst <= SAMPLE
    again = nr.trace_rays(sc, L.origins, L.dirs, max_depth=0, unordered=True)
    assert np.array_equal(_bits(again), _bits(got))


@pytest.mark.parametrize("fmt,interp,overflow", MODES, ids=MODE_IDS)
def test_alpha_texture_through_intersects_ray(gpu, fmt, interp, overflow):
    L = _layout()
    sc = _scene(L, fmt, interp, overflow, "alpha")
    _check_inputs(sc, L)
    lit, filt = nr.intersects_rays(sc, L.origins, L.dirs, L.max_toi)
    blocked, pfilt = nr.shadow_rays(sc, L.origins, L.dirs, L.max_toi)
    assert np.array_equal(lit, ~blocked)                                   # the two entry points agree bit for bit
    assert np.array_equal(_bits(filt[lit]), _bits(pfilt[lit]))
    assert np.all(filt[~lit] == 0.0)
    w = _reference(fmt, interp, overflow)[:, 3]
    sample = 0.0 if interp == tc.NEAREST else SAMPLE
    near = (np.abs(w - 1.0) <= sample) & (w != 1.0)                        # the f32 blend may round onto either side of 1.0 (module docstring)
    assert np.array_equal(lit[~near], (w < 1.0)[~near])
    assert 0 < lit.sum() < len(lit)
    exp = np.repeat((1.0 - w)[:, None], 3, axis=1)
    worst = _worst(filt[lit], exp[lit])
    print("filter: worst |device - reference| = %.4g (bound %.4g), %d cases within the sample bound of 1" % (worst, sample + (0.0 if interp == tc.NEAREST else U), int(near.sum())))
    if interp == tc.NEAREST:
        assert np.array_equal(_bits(filt[lit]), _bits(np.repeat((np.float32(1.0) - w.astype(np.float32))[:, None], 3, axis=1)[lit]))  # fl(1 - w), w a texel
    else:
        assert worst <= sample + U


@pytest.mark.parametrize("fmt,interp,overflow", MODES, ids=MODE_IDS)
def test_alpha_texture_through_the_blend_and_the_transparent_hit_elision(gpu, fmt, interp, overflow):
    L = _layout()
    sc = _scene(L, fmt, interp, overflow, "alpha")
    _check_inputs(sc, L)
    # max_depth 1: the smallest positive depth limit — the refraction ray of the hit (depth 0 < 1) is traced, nothing deeper (0 means no limit)
    got = nr.trace_rays(sc, L.origins, L.dirs, max_depth=1)
    a = _reference(fmt, interp, overflow)[:, 3]
    bg = np.asarray(BG, np.float64)
    exp = a[:, None] * 1.0 + bg[None, :] * (1.0 - a[:, None])
    bound = (0.0 if interp == tc.NEAREST else SAMPLE) + 4.0 * U
    worst = _worst(got, exp)
    zero, one = a == 0.0, a == 1.0
    print("blend: worst |device - reference| = %.4g (bound %.4g), %d cases of a == 0, %d of a == 1" % (worst, bound, int(zero.sum()), int(one.sum())))
    assert worst <= bound
    t8 = tc.SIZES.index((8, 8))
    in8 = slice(L.first[t8], L.first[t8 + 1])
    assert zero[in8].any() and one[in8].any() and (~zero[in8] & ~one[in8]).any()  # the 8x8 texture: texels of exactly 0 and 1 next to others
    assert np.array_equal(_bits(got[zero]), _bits(np.tile(np.asarray(BG, np.float32), (int(zero.sum()), 1))))  # the elided hit: exactly the background
    assert np.array_equal(_bits(got[one]), _bits(np.ones((int(one.sum()), 3), np.float32)))                    # opaque: exactly ka


def test_non_finite_uvs(gpu):
    """nrays_scene_create refuses a NaN uv (a mesh uv must be f32-exact: `(double)(float)x == x` fails for NaN) and accepts +-inf; a hit on an edge of a
    triangle with an infinite uv interpolates inf 0 = NaN, so the sampler sees NaN too (_Layout).  ClampToEdges turns +-inf into 1 / 0 and, as nalgebra's
    clamp, a NaN into 0.0; under Wrap `inf % 1.0` and `NaN % 1.0` are NaN, the saturating cast selects tap 0 and, for Bilinear, the NaN weights make every
    channel NaN: the device must return NaN exactly where the reference's arithmetic does, and the reference's texel elsewhere."""
    bad = nr.Scene([nr.SceneNode(nr.PhongMaterial((1, 1, 1), (0, 0, 0), (0, 0, 0), None, None, 1.0), 0.0, 0.0, 1.0, 1.0, nr.Isometry3(),
                                 nr.TriMesh([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 1, 2]], [[0.5, 0.5], [float("nan"), 0.5], [0.5, 0.5]]))], [], BG)
    with pytest.raises(abi.NraysError) as e:
        bad.device_handle()
    assert e.value.status == abi.ERR_UNSUPPORTED and "mesh uv is not exactly representable in f32" in str(e.value)

    L = _layout(True)
    assert (~np.isfinite(L.uv)).any(axis=1).all() and np.isnan(L.uv).any() and np.isinf(L.uv).any()
    for fmt, interp, overflow in MODES:
        ref = _reference(fmt, interp, overflow, True)
        nan = np.isnan(ref)
        assert nan.any() == (interp == tc.BILINEAR and overflow == tc.WRAP)
        sc = _scene(L, fmt, interp, overflow, "colour")
        _check_inputs(sc, L)
        got = nr.trace_rays(sc, L.origins, L.dirs, max_depth=0)
        assert np.array_equal(np.isnan(got), nan[:, :3]), (fmt, interp, overflow)
        fin = ~nan[:, :3]
        if interp == tc.NEAREST:
            assert np.array_equal(_bits(got), _bits(ref[:, :3])), (fmt, interp, overflow)
        else:
            assert _worst(got[fin], ref[:, :3][fin]) <= SAMPLE, (fmt, interp, overflow)
        sa = _scene(L, fmt, interp, overflow, "alpha")
        lit, filt = nr.intersects_rays(sa, L.origins, L.dirs, L.max_toi)
        w = ref[:, 3]
        with np.errstate(invalid="ignore"):
            near = (np.abs(w - 1.0) <= SAMPLE) & (w != 1.0)
            assert np.array_equal(lit[~near], (w < 1.0)[~near]), (fmt, interp, overflow)  # a NaN alpha is not < 1: blocked, as in the reference
        assert not lit.any() or _worst(filt[lit], np.repeat((1.0 - w[lit])[:, None], 3, axis=1)) <= SAMPLE + U, (fmt, interp, overflow)
