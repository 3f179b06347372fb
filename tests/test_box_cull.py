"""The f32 box culling as a SUPERSET of the reference's f64 ray / AABB test, on the CPU mirror of trace_device.h (tests/box_cull_cases.py):
the mirror's fma, the two conditions that keep the classes honest, the statement at three reciprocals per axis, tightness, and the
mutants — each single change of the arithmetic must break the statement in a class named here.  The kernels themselves meet the same
cases in tests/test_box_cull_gpu.py, where every key must equal this mirror's bit for bit."""
import fractions
import itertools

import numpy as np
import pytest

from tests import box_cull_cases as bc

F32 = np.float32
NAMES = list(bc.CLASSES)


def _f32_of_fraction(fr):
    """Correctly rounded (ties to even) f32 of a rational, in integers."""
    if fr == 0:
        return F32(0.0)
    sign, fr = (-1.0 if fr < 0 else 1.0), abs(fr)
    e = fr.numerator.bit_length() - fr.denominator.bit_length()
    if fractions.Fraction(2) ** e > fr:
        e -= 1
    e = max(e, -126)                      # denormals: the spacing of the smallest normal binade
    q = fr / fractions.Fraction(2) ** (e - 23)
    m, rem = divmod(q.numerator, q.denominator)
    if 2 * rem > q.denominator or (2 * rem == q.denominator and m & 1):
        m += 1
    with np.errstate(over="ignore"):
        return F32(sign * float(m) * 2.0 ** (e - 23))


def test_mirror_fma_is_rounded_once():
    """fma32 against the rational value rounded once, on random operands, on sums that land on f32 ties (where "product and sum in f64, then
    cast" rounds twice and goes wrong) and in the f32 denormals."""
    rng = np.random.default_rng(7)
    a = (rng.normal(size=4000) * 10.0 ** rng.uniform(-3, 3, 4000)).astype(F32)
    b = (rng.normal(size=4000) * 10.0 ** rng.uniform(-3, 3, 4000)).astype(F32)
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1.0 + rng.normal(size=4000) * 10.0 ** rng.uniform(-8, 0, 4000))).astype(F32)
    # a * b = 2^-24 - 2^-70 exactly, c = 1 + 2^-23: the sum lies 2^-70 BELOW the tie between 1 + 2^-23 and 1 + 2^-22 and rounds down; the f64 sum
    # drops the 2^-70, lands on the tie, and the cast rounds it to even = up.  Mirrored for the other sign, and two sums in the f32 denormals.
    a = np.concatenate([a, [F32(1.0 + 2.0 ** -23)] * 2, [F32(1e-20), F32(3e-39)]]).astype(F32)
    b = np.concatenate([b, [F32((1.0 - 2.0 ** -23) * 2.0 ** -24), F32(-(1.0 - 2.0 ** -23) * 2.0 ** -24)], [F32(1.1e-19), F32(0.3)]]).astype(F32)
    c = np.concatenate([c, [F32(1.0 + 2.0 ** -23), F32(-1.0 - 2.0 ** -23)], [F32(1e-39), F32(-1e-40)]]).astype(F32)
    got = bc.fma32(a, b, c)
    Fr = fractions.Fraction
    want = np.array([_f32_of_fraction(Fr(float(x)) * Fr(float(y)) + Fr(float(z))) for x, y, z in zip(a, b, c)], F32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    twice = (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F32)
    assert (twice.view(np.uint32) != want.view(np.uint32)).any(), "no operand set separates one rounding from two"


def test_mirror_special_values():
    """-inf / +inf addends of an unconstrained axis, fmax / fmin dropping a NaN (an origin so far that o32 * inv32 overflows: -p + e = NaN)."""
    inf = F32(np.inf)
    assert bc.fma32(F32(3.0), F32(0.0), -inf) == -inf and bc.fma32(F32(-bc.FLT_MAX), F32(0.0), inf) == inf
    o, d = np.array([[1e12, 0.5, 0.5]]), np.array([[1e-29, 0.0, 0.0]])
    box = np.array([[0, 0, 0, 2e12, 1, 1]], F32)
    keys, bits = bc.mirror_keys(o, d, [bc.DBL_MAX], box, [0], bc.inv_candidates(d)[1])
    assert bits[0] == 6 and np.isfinite(keys[0, 0]) and np.isinf(keys[0, 1:]).all()


@pytest.mark.parametrize("name", NAMES)
def test_classes_are_split_by_the_reference_and_settled_by_f64(name):
    """The two conditions: the f64 reference accepts 20 % .. 80 % of a class, and the exact predicate disagrees with it on <= 1 %."""
    c = bc.cases(name)
    acc, dis = c["ref"].mean(), (c["ref"] != c["exact"]).mean()
    print("%s: %d cases, reference accepts %.1f %%, near an f64 tie %.1f %%, exact verdict differs on %.3f %%" % (name, len(c["ref"]), 100 * acc, 100 * c["tie"].mean(), 100 * dis))
    assert 0.2 <= acc <= 0.8
    assert dis <= 0.01


def test_classes_cover_octants_slots_and_their_special_values():
    for name in NAMES:
        c = bc.cases(name)
        octant = ((c["d"] < 0) * np.array([1, 2, 4])).sum(axis=1)
        for s in range(4):
            assert len(np.unique(octant[c["slot"] == s])) == 8, (name, s)
    c = bc.cases("zero_origin")
    assert ((c["o"] == 0).sum(axis=1) == 3).sum() > 1000 and ((c["o"] == 0).sum(axis=1) == 1).sum() > 1000
    for a in range(3):       # a face in the coordinate plane of a zero origin coordinate, both sides, both signs of the direction
        for side in (0, 3):
            f = (c["o"][:, a] == 0) & (c["box"][:, a + side] == 0)
            assert (f & (c["d"][:, a] > 0)).sum() > 50 and (f & (c["d"][:, a] < 0)).sum() > 50 and (f & (c["d"][:, a] == 0)).sum() > 50
    c = bc.cases("tiny_dir")
    x = np.abs(c["d"].astype(F32))
    assert ((c["d"] == 0).any(axis=1)).sum() > 500 and ((x > 0) & (x < np.finfo(F32).tiny)).any(axis=1).sum() > 500
    assert (x == F32(1e-30)).any(axis=1).sum() > 100 and (x == np.nextafter(F32(1e-30), F32(0))).any() and (x == np.nextafter(F32(1e-30), F32(1))).any()
    assert (np.abs(c["d"]).max(axis=1) >= 0.1).all()      # an ordinary component in every direction (box_cull_cases: what a class must satisfy)
    c = bc.cases("dir_huge")
    assert (np.abs(c["d"]) == float(bc.FLT_MAX)).any(axis=1).sum() > 1000 and (np.abs(c["d"]) <= float(bc.FLT_MAX)).all()
    c = bc.cases("dir_length")
    assert np.linalg.norm(c["d"], axis=1).min() < 1e-11 and np.linalg.norm(c["d"], axis=1).max() > 1e12
    c = bc.cases("best_entry")
    with np.errstate(over="ignore"):
        down = c["best"].astype(F32).astype(np.float64) < c["best"]
    assert 0.2 < down[c["best"] < 1e300].mean() < 0.8 and (c["best"] == bc.DBL_MAX).sum() > 1000 and ((c["best"] > 0) & (c["best"] < 1e-300)).sum() > 1000


def _union_of_violations(c, combos=None, **kw):
    cand = bc.inv_candidates(c["d"], long_fix=kw.get("long_fix", True))
    bad = set()
    for pick in combos or RECIPROCALS:
        inv = np.stack([cand[pick[a]][:, a] for a in range(3)], axis=1)
        keys, _ = bc.mirror_keys(c["o"], c["d"], c["best"], c["box"], c["slot"], inv, **kw)
        bad |= set(bc.violations(c, keys).tolist())
    return bad


RECIPROCALS = list(itertools.product(range(3), repeat=3))   # per axis: one ulp below, the correctly rounded reciprocal, one ulp above


@pytest.mark.parametrize("name", NAMES)
def test_mirror_is_a_superset_at_three_reciprocals_per_axis(name):
    """The statement for ANY reciprocal within 1 ulp of the correctly rounded one: all 27 combinations of the three candidates per axis."""
    c = bc.cases(name)
    bad = _union_of_violations(c)
    assert not bad, "%s: the reference accepts %d boxes the f32 test culls, e.g. case %d" % (name, len(bad), min(bad))


def test_mirror_is_tight():
    """A ray the exact test rejects even for the box grown by 2^-18 (|o_a| + max |b_a|) gets +inf (box_cull_cases: the derivation)."""
    c = bc.tightness_cases()
    n = len(c["ref"])
    assert c["clear"].mean() > 0.3 and (~c["clear"] & ~c["ref"]).mean() > 0.05   # both kinds of miss are there: clear ones and ones inside the growth
    assert (np.abs(c["d"]) >= 1e-3).all() and (np.abs(c["d"]) <= 1.0).all() and np.abs(c["o"]).max() <= 1e6 and np.abs(c["box"]).max() <= 1e6
    for pick in ((0, 0, 0), (1, 1, 1), (2, 2, 2), (0, 1, 2), (2, 0, 1)):
        cand = bc.inv_candidates(c["d"])
        inv = np.stack([cand[pick[a]][:, a] for a in range(3)], axis=1)
        keys, _ = bc.mirror_keys(c["o"], c["d"], c["best"], c["box"], c["slot"], inv)
        finite = np.isfinite(keys[np.arange(n), c["slot"]])
        assert not (c["clear"] & finite).any(), int((c["clear"] & finite).sum())
        assert not len(bc.violations(c, keys))
    print("tightness family: reference accepts %.2f %%, mirror %.2f %%; extra acceptance by relative push: %s" % (100 * c["ref"].mean(), 100 * finite.mean(), bc.extra_acceptance_by_push(c, finite)))


# (mutant, the class that must catch it).  Counts are printed; the seeds are fixed, so they are reproducible.
MUTANTS = [
    ("the absolute margin e absent", dict(e_scale=0.0), "far_origin"),
    ("e = 2^-24 |p| instead of 2^-21 |p|", dict(e_scale=2.0 ** -24), "far_origin"),
    ("kSlack = 1", dict(kslack=1.0), "zero_origin"),
    ("zero_axis_cull's margin = 0", dict(zero_margin=False), "tiny_dir"),
    ("entry and exit planes swapped", dict(swap=True), "ordinary"),
    ("1e30 directions handed to the zero-axis rule again (the parent commit)", dict(long_fix=False), "dir_huge"),
    # the neighbours that take the place of the two identities below
    ("best_f32's factor on the wrong side (1 - 2^-19)", dict(best_factor=1.0 - 2.0 ** -19), "best_entry"),
    ("best_f32's factor = 1 together with kSlack = 1", dict(best_factor=1.0, kslack=1.0), "best_entry"),
    ("the zero-axis rule with <= / >= and no margin (round 1's bug: a face in the origin's coordinate plane)", dict(zero_strict=True, zero_margin=False), "zero_origin"),
]


@pytest.mark.parametrize("what,kw,where", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_every_single_change_breaks_the_statement_in_a_named_class(what, kw, where):
    counts = {name: len(_union_of_violations(bc.cases(name), combos=((0, 0, 0), (1, 1, 1), (2, 2, 2)), **kw)) for name in NAMES}
    print("%s: %s" % (what, ", ".join("%s %d" % kv for kv in counts.items())))
    assert counts[where] > 0, (what, where, counts)


def test_the_three_mutants_that_stay_inside_the_statement():
    """best_f32's factor = 1 alone, the zero-axis rule with <= / >= alone, and fmaxf(..., 0) dropped break nothing, and cannot:
    * kSlack multiplies f = min(..., tbest), so tbest * kSlack >= (float)best * (1 + 1.4e-6) > best (1 - 2^-24)(1 + 1.4e-6) > best: the factor of
      best_f32 is a second line behind kSlack.  It shows once kSlack is gone (the pair above: more violations in best_entry than kSlack = 1 alone).
    * zero_axis_cull's margin m >= 2^-22 |o32| is four f32 ulps of o32, so o32 + m > o32 >= mn wherever the reference accepts (fl is monotonic, mn
      is an f32): `<` and `<=` cannot differ.  They differ once the margin is gone: the neighbour above.
    * without the clamp n only gets smaller, so n <= f * kSlack holds more often: the clamp is what makes "a negative f never passes" true (trace_device.h),
      i.e. tightness.  Its loss shows on the boxes that lie wholly BEHIND the origin: the product culls them, the mutant accepts them, with a negative key."""
    for kw in (dict(best_factor=1.0), dict(zero_strict=True), dict(clamp0=False)):
        for name in NAMES:
            assert not _union_of_violations(bc.cases(name), combos=((0, 0, 0), (1, 1, 1), (2, 2, 2)), **kw), (kw, name)
    c = bc.cases("best_entry")
    alone = len(_union_of_violations(c, combos=((1, 1, 1),), kslack=1.0))
    both = len(_union_of_violations(c, combos=((1, 1, 1),), kslack=1.0, best_factor=1.0))
    assert both > alone, (alone, both)
    c = bc.cases("ordinary")
    n, inv = len(c["o"]), bc.inv_candidates(c["d"])[1]
    mn, mx = c["box"][:, :3].astype(np.float64), c["box"][:, 3:].astype(np.float64)
    with np.errstate(all="ignore"):
        behind = (np.maximum((mn - c["o"]) / c["d"], (mx - c["o"]) / c["d"]).min(axis=1) < -1e-3) & ~c["ref"]
    product = np.isfinite(bc.mirror_keys(c["o"], c["d"], c["best"], c["box"], c["slot"], inv)[0][np.arange(n), c["slot"]])
    mutant = bc.mirror_keys(c["o"], c["d"], c["best"], c["box"], c["slot"], inv, clamp0=False)[0][np.arange(n), c["slot"]]
    print("fmaxf(..., 0) dropped: %d boxes behind the origin, the product accepts %d of them, the mutant %d" % (behind.sum(), (behind & product).sum(), (behind & np.isfinite(mutant)).sum()))
    assert behind.sum() > 1000 and not (behind & product).any() and (behind & np.isfinite(mutant)).sum() > 1000 and (mutant[behind & np.isfinite(mutant)] < 0).all()


def test_the_parent_commits_rule_for_long_directions_fails_on_the_mirror():
    """What this class found: with components beyond ~1e37.9 the reciprocal is an f32 denormal; where the device's rcp returns 0 for it, the axis was
    handed to zero_axis_cull — the rule for a ray PARALLEL to the slab — and boxes the reference accepts were culled.  Unflushed, the denormal
    reciprocal's lost bits still break the relative-error premise on a few cases."""
    c = bc.cases("dir_huge")
    out = {}
    for flush in (False, True):
        bad = set()
        for inv in bc.inv_candidates(c["d"], long_fix=False, flush=flush):
            keys, _ = bc.mirror_keys(c["o"], c["d"], c["best"], c["box"], c["slot"], inv, long_fix=False)
            bad |= set(bc.violations(c, keys).tolist())
        out[flush] = len(bad)
    print("dir_huge, parent arithmetic: %d violations with a denormal reciprocal kept, %d with it flushed to 0, of %d accepted" % (out[False], out[True], c["ref"].sum()))
    assert out[True] > 1000 and out[False] > 0
