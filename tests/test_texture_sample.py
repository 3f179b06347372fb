"""The oracle's tex_sample (oracle/nrays_oracle.c) against the independent numpy restatement of Texture2d::sample (tests/texture_cases.py): every
texture of the table in both texel formats, Bilinear / Nearest x Wrap / ClampToEdges, over the whole coordinate table and the non-finite group.

Bounds (u = 2^-24, the unit roundoff of f32; texels and weights lie in [0, 1]; a subnormal product loses at most 2^-150, ignored):

  Nearest   no arithmetic follows the tap: bit equality with the selected texel (for RGBA8 that texel is texel_ref = `u8 as f32 / 255.0`).

  Bilinear  the code under test evaluates, in f32 and without contraction (oracle/Makefile and __graft_entry__.py: HIP_FLAGS both pass -ffp-contract=off; see the last
            line for a build that contracts), with s = shift and w = fl(1 - s) — the SAME f32 weights the reference blend uses:
              U = fl(fl(ul w_x) + fl(ur s_x)),  D likewise,  R = fl(fl(U s_y) + fl(D w_y)).
            One lerp of exact inputs a, b: fl(fl(a w) + fl(b s)) = (a w (1 + d1) + b s (1 + d2)) (1 + d3), |d| <= u, so its error is at most
            (a w + b s) (2 u + u^2) <= (w + s) (2 u + u^2) <= (1 + u) (2 u + u^2), because w = fl(1 - s) <= (1 - s) (1 + u): E1 <= 2 u + 3 u^2 + u^3.
            The second lerp takes U, D with errors <= E1 and values <= 1 + u + E1: it passes on E1 (s_y + w_y) <= E1 (1 + u) and adds at most
            (1 + u + E1) (1 + u) (2 u + u^2) of its own.  Sum: 4 u + 15 u^2 + O(u^3) < 4 u (1 + 2^-20).
            A fused multiply-add (a w + fl(b s) in one rounding) only removes a rounding from each lerp: the bound holds with contraction too.
            BILINEAR_BOUND = 4 * 2^-24 * (1 + 2^-20) = 2.3842e-07 — against the f64 blend of the reference's f32 taps and f32 weights.
"""
import numpy as np
import pytest

import nrays_amd as nr
import oracle
from tests import texture_cases as tc

U = 2.0 ** -24
BILINEAR_BOUND = 4.0 * U * (1.0 + 2.0 ** -20)

MODES = [(f, i, o) for f in tc.FORMATS for i in (tc.BILINEAR, tc.NEAREST) for o in (tc.WRAP, tc.CLAMP)]
MODE_IDS = ["%s-%s-%s" % (f, "nearest" if i else "bilinear", "clamp" if o else "wrap") for f, i, o in MODES]


def test_the_table_uses_the_abi_constants():
    assert (tc.BILINEAR, tc.NEAREST) == (nr.Interpolation.Bilinear, nr.Interpolation.Nearest)
    assert (tc.WRAP, tc.CLAMP) == (nr.Overflow.Wrap, nr.Overflow.ClampToEdges)


def _oracle_samples(texels, interp, overflow, uv):
    t = nr.Texture2d(nr.ImageData(texels), interp, overflow)
    return np.stack([oracle.tex_sample(t, float(u), float(v)) for u, v in uv])


def _compare(got, ref, interp, what):
    """Returns the worst |got - ref| over the finite reference values; NaN exactly where the reference's arithmetic gives NaN."""
    assert np.array_equal(np.isnan(got), np.isnan(ref.value)), what
    fin = ~np.isnan(ref.value)
    if interp == tc.NEAREST:
        assert fin.all(), what
        assert np.array_equal(got.view(np.uint32), ref.value.astype(np.float32).view(np.uint32)), what
        return 0.0
    err = np.abs(got.astype(np.float64) - ref.value)[fin]
    worst = float(err.max()) if err.size else 0.0
    assert worst <= BILINEAR_BOUND, (what, worst)
    return worst


@pytest.mark.parametrize("fmt,interp,overflow", MODES, ids=MODE_IDS)
def test_oracle_tex_sample_equals_the_reference(fmt, interp, overflow):
    worst = 0.0
    for size in tc.SIZES:
        texels = tc.TEXTURES[size][fmt]
        uv = tc.pairs(*size)
        ref = tc.sample_ref(texels, interp, overflow, uv[:, 0], uv[:, 1])
        worst = max(worst, _compare(_oracle_samples(texels, interp, overflow, uv), ref, interp, (size, fmt)))
    print("worst |oracle - f64 blend| = %.4g (bound %.4g)" % (worst, BILINEAR_BOUND))


@pytest.mark.parametrize("fmt,interp,overflow", MODES, ids=MODE_IDS)
def test_oracle_tex_sample_on_non_finite_coordinates(fmt, interp, overflow):
    """+-inf and NaN: the casts saturate (NaN -> tap 0), na::clamp turns a NaN into 0.0, `inf % 1.0` is NaN; NaN where the reference's arithmetic gives NaN."""
    uv = tc.nonfinite_pairs()
    worst, nans = 0.0, 0
    for size in tc.SIZES:
        texels = tc.TEXTURES[size][fmt]
        ref = tc.sample_ref(texels, interp, overflow, uv[:, 0], uv[:, 1])
        worst = max(worst, _compare(_oracle_samples(texels, interp, overflow, uv), ref, interp, (size, fmt)))
        nans += int(np.isnan(ref.value).any(axis=1).sum())
    assert (nans > 0) == (interp == tc.BILINEAR and overflow == tc.WRAP)  # only the weights of `inf % 1.0` are NaN; Nearest selects tap 0, the clamp returns 0 or 1
    print("worst |oracle - f64 blend| = %.4g, %d NaN samples" % (worst, nans))


def test_reference_known_answers():
    """The restatement itself, on values worked out by hand (2x2 texture: texel (x, y) at [y, x])."""
    px = np.array([[[0, 0, 0, 255], [255, 0, 0, 255]], [[0, 255, 0, 255], [255, 255, 255, 51]]], dtype=np.uint8)
    s = tc.sample_ref(px, tc.BILINEAR, tc.WRAP, [0.5, 1.25, 1.0, -0.0], [0.5, -0.75, 1.0, 0.0])
    assert np.allclose(s.value, [(0.5, 0.5, 0.25, 0.8), (0.25, 0.25, 0.0625, 0.95), (0, 0, 0, 1), (0, 0, 0, 1)], atol=1e-7)
    assert [int(a[0]) for a in s.taps] == [0, 1, 0, 1]
    s = tc.sample_ref(px, tc.NEAREST, tc.WRAP, [0.5, 0.49999997, 0.6], [0.0, 0.0, 0.4])  # round half AWAY from zero: 0.5 -> 1
    assert [int(x) for x in s.taps[0]] == [1, 0, 1] and [int(y) for y in s.taps[1]] == [0, 0, 0]
    s = tc.sample_ref(px, tc.BILINEAR, tc.CLAMP, [7.0, -3.0, np.nan], [9.0, 0.0, np.nan])
    assert np.allclose(s.value, [(1, 1, 1, 0.2), (0, 0, 0, 1), (0, 0, 0, 1)])
    s = tc.sample_ref(px, tc.NEAREST, tc.WRAP, [np.inf, np.nan], [1.0 - 2.0 ** -24, -np.inf])  # NaN -> tap 0
    assert [int(x) for x in s.taps[0]] == [0, 0] and [int(y) for y in s.taps[1]] == [1, 0]
