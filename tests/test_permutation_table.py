"""The permutation table (tests/permutation_cases.py) against the list it stands for and against the oracle — no GPU needed.

1. The set of permutations the table claims to reach EQUALS the X(g, s, f, p, o) items parsed out of NR_PRIMARY_PERMUTATIONS
   (csrc/primary_kernel.h): a permutation added without a case, or a case left behind by a removed permutation, fails here.
2. The groups are 0 .. kPrimaryGroups - 1 and the build compiles one unit per group.
3. Every scene gives its specialised code something to do.  The conditions are evaluated on the ORACLE's frame and ray counts, so they hold
   for what the kernels are later compared with (tests/test_permutations_gpu.py):
     - at least half of the pixels differ from the background;
     - shadow rays, and reflection or refraction rays (trace_chain iterates), in every case;
     - bit 4: shadow rays are filtered by the non-opaque node — the frame differs from the same scene with that node opaque, and shadow
       rays from the floor (which fills the frame) to the first light arrive dimmed, neither blocked nor untouched; scenes without bit 4 (and without double branching) spawn no refraction ray at all, which is what "every node opaque" means to the oracle;
     - bit 16: more than one shadow ray per shaded hit.  Every ray has at most one hit, so rays_shadow > rays_primary + rays_reflection +
       rays_refraction is sufficient (and is what is asserted);
     - 15 / 31: reflection AND refraction rays;
     - tiny scenes: a plane among the leaves, and one case with exactly kTinyLeaves leaves;
     - every untransformed (bit 64) case has a sibling with one rotated BLAS that expects the same permutation without bit 64;
     - at least a third of the frame sizes are whole neither in 8 x 8 wave tiles nor in 16 x 16 blocks.
"""
import collections
import re

import numpy as np
import pytest

import nrays_amd as nr
from tests import permutation_cases as pc


def test_parser_reads_the_header():
    perms = pc.parse_permutations()
    assert len(perms) == len(set(perms)) > 0, "duplicate X(...) items"
    tuples = [t for _, t in perms]
    assert len(tuples) == len(set(tuples)), "one permutation in two groups"
    assert (0, (True, 31, False, 0)) in perms and (0, (False, 31, False, 0)) in perms  # the two full kernels every build holds
    # the X( count of the macro's text is the parser's count: nothing was silently dropped
    text = open(pc.PRIMARY_KERNEL_H).read()
    body = text[text.index("#define NR_PRIMARY_PERMUTATIONS(X)"):text.index("constexpr int kPrimaryGroups")]
    assert len(re.findall(r"\bX\(\d", body)) == len(perms)


def test_table_equals_the_list():
    want = {t for _, t in pc.parse_permutations()}
    have = pc.listed_permutations()
    assert have == want, "permutations without a case: %s; cases without a permutation: %s" % (sorted(want - have), sorted(have - want))
    per = collections.Counter(c.expect for c in pc.CASES if c.listed)
    assert all(n == 1 for n in per.values()), "two cases stand for one permutation: %s" % [t for t, n in per.items() if n > 1]
    # fall-backs and switch-offs end in a kernel of the list too
    assert {c.expect for c in pc.CASES if not c.listed} <= want
    assert len({c.name for c in pc.CASES}) == len(pc.CASES)


def test_groups_and_build_units():
    import __graft_entry__ as g
    groups = {grp for grp, _ in pc.parse_permutations()}
    n = pc.parse_group_count()
    assert groups == set(range(n))
    assert g.PRIMARY_GROUPS == n, "build_hip compiles %d primary units, primary_kernel.h names %d groups" % (g.PRIMARY_GROUPS, n)
    inst = open(pc.PRIMARY_KERNEL_H.replace("primary_kernel.h", "primary_inst.hip")).read()
    assert "NR_PRIMARY_PERMUTATIONS(X)" in inst
    decl = set(re.findall(r"bool launch_primary_group(\d+)\(", open(pc.PRIMARY_KERNEL_H).read()))
    assert decl == {str(k) for k in range(n)}
    hip = open(pc.PRIMARY_KERNEL_H.replace("primary_kernel.h", "frame_path.hip")).read()
    assert set(re.findall(r"launch_primary_group(\d+)\(a,", hip)) == decl, "launch_primary() does not ask every group"


def test_expected_tuples_follow_the_selection_rules():
    """The table's own consistency: what a case expects is what its scene content, switches and frame kind select by the rules written in
    permutation_cases.py's docstring (independent of the library: a typo in the table fails here, a typo in the library on the GPU)."""
    for c in pc.CASES:
        stats, feat, plain, occ = c.expect
        if c.kind == "instrumented":
            assert c.expect == (True, 31, False, 0)
            continue
        sc, _ = c.build()
        kinds = {type(n.geometry) for n in sc._nodes}
        content = (pc.ANALYTIC if kinds - {nr.TriMesh} else 0) | (pc.MESH if nr.TriMesh in kinds else 0)
        transparent = any(n.alpha < 1.0 or getattr(n.material, "alpha", None) is not None for n in sc._nodes)
        content |= pc.ALPHA if transparent else 0
        if any(n.alpha < 1.0 and n.refl_mix != 0.0 for n in sc._nodes):
            content = 15
        if not (len(sc._lights) == 1 and sc._lights[0].racsample == 1):
            content |= pc.MULTI
        want = content
        env = c.env
        if content in (1, 5, 17, 21) and env.get("NRAYS_LDS_SCENE") != "0":
            want |= pc.LDS
            if content in (1, 17) and len(sc._nodes) <= pc.TINY_LEAVES and env.get("NRAYS_TINY_SCENE") != "0":
                want |= pc.TINY
        world = all(n.transform.translation == (0.0, 0.0, 0.0) and n.transform.axis_angle == (0.0, 0.0, 0.0) for n in sc._nodes)
        if content in (2, 6, 18, 22) and world and env.get("NRAYS_NOXFORM") != "0":
            want |= pc.NOXFORM
        spp, window = pc.FRAME_KINDS[c.kind]
        one_lane = spp == 1
        want_occ = 3 if (env.get("NRAYS_OCC") == "3" and content in (6, 7, 22, 23) and one_lane) else 0
        if want_occ == 3 and content in (6, 22) and env.get("NRAYS_PARK") != "0":
            want |= pc.PARK
        is_plain = spp == 1 and window == 0.0 and not any(l.radius != 0.0 for l in sc._lights)
        want_plain = is_plain and (content & 3) != 3 and content not in (15, 31)  # mixed and double-branching scenes have general kernels only
        assert (stats, feat, plain, occ) == (False, want, want_plain, want_occ), c.name
        if content in (6, 7, 22, 23):
            assert "NRAYS_OCC" in env, "%s: the library would choose OCC by the frame's size" % c.name


@pytest.mark.parametrize("case", pc.CASES, ids=[c.name for c in pc.CASES])
def test_scene_exercises_its_permutation(case):
    img, cnt, background = pc.oracle_frame(case)
    w, h = case.size
    assert img.shape == (h, w, 3)
    covered = (np.abs(img - np.asarray(background, np.float32)).max(axis=2) > 0).mean()
    assert covered >= 0.5, "only %.0f %% of the pixels differ from the background" % (100 * covered)
    assert cnt["rays_primary"] == w * h * pc.FRAME_KINDS[case.kind][0]
    assert cnt["rays_shadow"] > 0
    assert cnt["rays_reflection"] > 0 or cnt["rays_refraction"] > 0
    feat = case.expect[1]
    double = (feat & 15) == 15
    if double:
        assert cnt["rays_reflection"] > 0 and cnt["rays_refraction"] > 0
    elif feat & pc.ALPHA:
        twin, twin_cnt, _ = pc.oracle_frame(case, opaque_twin=True)
        assert cnt["rays_refraction"] > 0 and twin_cnt["rays_refraction"] == 0
        assert (np.abs(twin - img).max(axis=2) > 0).sum() >= 64, "the non-opaque node changes nothing visible"
        assert pc.filtered_floor_shadows(case) >= 4, "no shadow ray from the floor to the light is filtered by the non-opaque node"
    else:
        assert cnt["rays_refraction"] == 0, "a scene of opaque nodes refracts nothing"
    if feat & pc.MULTI:
        assert cnt["rays_shadow"] > cnt["rays_primary"] + cnt["rays_reflection"] + cnt["rays_refraction"]
    if feat & pc.TINY:
        sc, _ = case.build()
        assert any(isinstance(n.geometry, nr.Plane) for n in sc._nodes) and len(sc._nodes) <= pc.TINY_LEAVES


def test_table_wide_conditions():
    tiny = [c for c in pc.CASES if c.expect[1] & pc.TINY]
    assert any(len(c.build()[0]._nodes) == pc.TINY_LEAVES for c in tiny), "no tiny scene with exactly kTinyLeaves leaves"
    assert any(len(c.build()[0]._nodes) < pc.TINY_LEAVES for c in tiny)
    for c in pc.CASES:
        if c.expect[1] & pc.NOXFORM:
            _, feat, plain, occ = c.expect
            sib = [s for s in pc.CASES if s.builder is c.builder and s.kwargs.get("rotate") and s.expect == (False, feat - pc.NOXFORM, plain, occ)]
            assert sib, "%s has no rotated sibling that expects no bit 64" % c.name
    odd = [c for c in pc.CASES if c.size[0] % 8 or c.size[1] % 8]
    assert 3 * len(odd) >= len(pc.CASES)
    assert all(not (c.size[0] % 16 == 0 and c.size[1] % 16 == 0) for c in odd)
    assert all(100 <= c.size[0] <= 200 and 80 <= c.size[1] <= 150 for c in pc.CASES)  # the table stays cheap
