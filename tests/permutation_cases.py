"""The k_primary permutation table: one case per item of NR_PRIMARY_PERMUTATIONS (nrays_amd/csrc/primary_kernel.h) plus the frames that
have no exact permutation and must fall back to a named more general kernel.  Plain module, no fixtures: tests/test_permutation_table.py
checks it on any machine (against the parsed list, and every scene against the oracle's view of it), tests/test_permutations_gpu.py
renders it and asks the library which permutation ran (nrays_debug_last_permutation).

What selects a permutation (nrays_hip.hip: nrays_scene_create; frame_path.hip: plan_frame, render_impl, launch_primary):
  scene content   1 analytic shapes, 2 meshes with triangles, 4 some node not opaque to shadow rays, 16 unless exactly one light with one
                  sample; a node that both reflects and refracts makes it 15 (31 with bit 16)             scene_build.cpp
  handle          + 32 analytic-only and the records fit LDS (NRAYS_LDS_SCENE=0: off); + 256 additionally opaque with <= 8 leaves in each
                  TLAS (NRAYS_TINY_SCENE=0: off); + 64 mesh-only with every BLAS untransformed (NRAYS_NOXFORM=0: off);
                  + 128 for 6 / 22 at OCC = 3 (NRAYS_PARK=0: off)
  frame           PLAIN = one sample, no window, no area light;  OCC = 3 for 6 / 7 / 22 / 23 scenes above a size threshold or with
                  NRAYS_OCC=3 (only frames with one lane per pixel: one sample per pixel);  nrays_render_device_instrumented = (true, 31, false, 0)
"""
import os
import re

import nrays_amd as nr
from tools import scenes_util as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRIMARY_KERNEL_H = os.path.join(ROOT, "nrays_amd", "csrc", "primary_kernel.h")
SWITCHES = ("NRAYS_LDS_SCENE", "NRAYS_TINY_SCENE", "NRAYS_NOXFORM", "NRAYS_PARK", "NRAYS_OCC")  # read once by nrays_scene_create
# bits of FEAT (csrc/device_types.h: Features)
ANALYTIC, MESH, ALPHA, DOUBLE, MULTI, LDS, NOXFORM, PARK, TINY = 1, 2, 4, 8, 16, 32, 64, 128, 256
TINY_LEAVES = 8  # csrc/device_types.h: kTinyLeaves


# ---- the list in the header -------------------------------------------------------------------------------------------------------------
def parse_permutations(path=PRIMARY_KERNEL_H):
    """[(group, (stats, feat, plain, occ)), ...] of the X(g, s, f, p, o) items of NR_PRIMARY_PERMUTATIONS, in the header's order."""
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith("#define NR_PRIMARY_PERMUTATIONS(X)"))
    body = []
    for l in lines[start:]:
        body.append(l.rstrip().rstrip("\\"))
        if not l.rstrip().endswith("\\"):
            break
    text = re.sub(r"/\*.*?\*/", " ", " ".join(body)[len("#define NR_PRIMARY_PERMUTATIONS(X)"):], flags=re.S)
    items = re.findall(r"X\(\s*(\d+)\s*,\s*(true|false)\s*,\s*(\d+)\s*,\s*(true|false)\s*,\s*(\d+)\s*\)", text)
    assert re.sub(r"X\([^()]*\)", "", text).strip() == "", "NR_PRIMARY_PERMUTATIONS holds something that is not an X(g, s, f, p, o) item"
    return [(int(g), (s == "true", int(f), p == "true", int(o))) for g, s, f, p, o in items]


def parse_group_count(path=PRIMARY_KERNEL_H):
    return int(re.search(r"constexpr\s+int\s+kPrimaryGroups\s*=\s*(\d+)\s*;", open(path).read()).group(1))


# ---- scenes (tools/scenes_util.py style: small dyadic numbers, the same descriptor feeds the library and the oracle) ----------------------
def _lights(n, area):
    """area = 0: point lights; 2: the first light is a disc sampled 2 x 2 (bit 16 by itself); 1: a disc with ONE sample (no bit 16, but
    no plain frame either: the sample is drawn with the frame's RNG)."""
    first = nr.Light((2.0, 8.0, -4.0), 0.5 if area else 0.0, {0: 1, 1: 1, 2: 4}[area], (1, 1, 1))
    return [first, nr.Light((-5.0, 6.0, -3.0), 0.0, 1, (0.5, 0.375, 0.25))][:n]


def analytic_scene(transparent=False, lights=1, leaves=8, area=0, opaque_twin=False):
    """A reflective plane and `leaves` - 1 shapes of every analytic kind on and above it.  transparent: the box floating over the others is
    glass (alpha 0.375: its shadow on the plane and the balls is filtered, rays through it refract; no reflection on it, so no double
    branching).  opaque_twin: the same scene with that box opaque."""
    iso = nr.Isometry3
    white = su.default_material()
    glass = nr.PhongMaterial((0.0, 0.0, 0.125), (0.25, 0.25, 1.0), (1, 1, 1), None, None, 100.0)
    red = nr.PhongMaterial((0.125, 0.0, 0.0), (1.0, 0.25, 0.25), (1, 1, 1), None, None, 50.0)
    box_alpha = 0.375 if (transparent and not opaque_twin) else 1.0
    nodes = [
        nr.SceneNode(white, 0.25, 0.5, 1.0, 1.0, iso((0.0, -1.0, 0.0)), nr.Plane((0.0, 1.0, 0.0))),
        nr.SceneNode(nr.UVMaterial(), 0.25, 0.25, 1.0, 1.0, iso((-2.25, 0.0, 0.0)), nr.Ball(1.0)),
        nr.SceneNode(glass if transparent else red, 0.0, 0.0, box_alpha, 1.25, iso((0.25, 1.75, -0.5), (0.25, 0.5, 0.0)), nr.Cuboid((1.0, 0.25, 1.0))),
        nr.SceneNode(nr.NormalMaterial(), 0.25, 0.25, 1.0, 1.0, iso((2.25, -0.25, 0.5)), nr.Ball(0.75)),
        nr.SceneNode(white, 0.0, 0.0, 1.0, 1.0, iso((0.0, -0.5, -1.5)), nr.Cylinder(0.5, 0.5)),
        nr.SceneNode(red, 0.0, 0.0, 1.0, 1.0, iso((-1.25, -0.5, -2.5)), nr.Cone(0.5, 0.5)),
        nr.SceneNode(nr.NormalMaterial(), 0.0, 0.0, 1.0, 1.0, iso((1.5, -0.25, -2.25), (0.0, 0.0, 0.5)), nr.Capsule(0.5, 0.25)),  # (no uvs on a capsule: a UVMaterial would make it transparent)
        nr.SceneNode(white, 0.5, 0.25, 1.0, 1.0, iso((0.0, -0.25, 2.0)), nr.Ball(0.75)),
    ]
    for k in range(max(0, leaves - len(nodes))):
        nodes.append(nr.SceneNode(nr.NormalMaterial(), 0.0, 0.0, 1.0, 1.0, iso((-3.0 + 1.5 * k, -0.5, 3.5)), nr.Ball(0.5)))
    cam = dict(eye=(0.0, 4.0, -9.0), at=(0.0, 0.0, 0.0), fovy=45.0, floor_y=-1.0)
    return nr.Scene(nodes[:leaves], _lights(lights, area), (0.25, 0.375, 0.5)), cam


def mesh_scene(alpha=False, lights=1, rotate=False, ball=False, area=0, opaque_twin=False):
    """Textured torus, a large reflective floor, a quad wall between the first light and the torus; every TriMesh sits in world space
    (identity isometry) unless rotate, which turns the torus' BLAS.  alpha: the wall is alpha-mapped and slightly transparent (filtered
    shadows, refraction continuations); opaque_twin: the same scene with an opaque wall.  ball: one analytic ball (a mixed scene)."""
    pts, idx, uvs = su.torus_mesh(32, 16)
    tex_mat = nr.PhongMaterial((0.25, 0.25, 0.25), (1, 1, 1), (0.5, 0.5, 0.5), su.checker_texture(64, 8), None, 60.0)
    floor_mat = nr.PhongMaterial((0.125, 0.125, 0.125), (0.75, 0.75, 0.75), (1, 1, 1), None, None, 100.0)
    see_through = alpha and not opaque_twin
    wall_mat = nr.PhongMaterial((0.125, 0.25, 0.125), (0.25, 1.0, 0.25), (1, 1, 1), su.checker_texture(32, 4),
                                su.checker_texture(32, 6, alpha_holes=True) if see_through else None, 60.0)
    here = nr.Isometry3()
    fl = su.f32_exact([[-30, -1.25, -30], [30, -1.25, -30], [30, -1.25, 30], [-30, -1.25, 30]])
    fl_uv = su.f32_exact([[0, 0], [3, 0], [3, 3], [0, 3]])
    quad = [[0, 2, 1], [0, 3, 2]]
    wl = su.f32_exact([[-2.5, -1.0, -3.0], [2.5, -1.0, -3.0], [2.5, 2.0, -3.0], [-2.5, 2.0, -3.0]])
    wl_uv = su.f32_exact([[0, 0], [2, 0], [2, 1], [0, 1]])
    nodes = [
        nr.SceneNode(tex_mat, 0.0, 0.0, 1.0, 1.0, nr.Isometry3((0.0, 0.0, 0.0), (0.0, 0.25, 0.125)) if rotate else here, nr.TriMesh(pts, idx, uvs)),
        nr.SceneNode(floor_mat, 0.25, 0.5, 1.0, 1.0, here, nr.TriMesh(fl, quad, fl_uv)),
        nr.SceneNode(wall_mat, 0.0, 0.0, 0.875 if see_through else 1.0, 1.25, here, nr.TriMesh(wl, quad, wl_uv)),
    ]
    if ball:
        nodes.append(nr.SceneNode(su.default_material(), 0.25, 0.25, 1.0, 1.0, nr.Isometry3((2.75, 0.25, 0.5)), nr.Ball(0.75)))
    cam = dict(eye=(0.5, 6.0, -8.0), at=(0.0, 0.0, 0.0), fovy=40.0, floor_y=-1.25)
    return nr.Scene(nodes, _lights(lights, area), (0.5, 0.625, 0.75)), cam


def double_scene(lights=1, area=0):
    """A glass ball that reflects AND refracts (double branching: the continuation queue), a mirror ball, a glass box, a small torus mesh,
    a reflective plane."""
    iso = nr.Isometry3
    white = su.default_material()
    glass = nr.PhongMaterial((0.0, 0.0, 0.125), (0.25, 0.25, 1.0), (1, 1, 1), None, None, 100.0)
    pts, idx, uvs = su.torus_mesh(16, 8, 0.75, 0.25)
    nodes = [
        nr.SceneNode(glass, 0.25, 0.5, 0.5, 1.25, iso((-1.25, 0.0, 0.0)), nr.Ball(1.0)),
        nr.SceneNode(white, 0.5, 0.25, 1.0, 1.0, iso((1.25, 0.0, 0.5)), nr.Ball(0.75)),
        nr.SceneNode(glass, 0.0, 0.0, 0.375, 1.5, iso((0.25, 1.0, 1.75)), nr.Cuboid((0.5, 0.5, 0.5))),
        nr.SceneNode(nr.UVMaterial(), 0.0, 0.0, 1.0, 1.0, iso((0.5, -0.5, -1.5), (0.5, 0.0, 0.25)), nr.TriMesh(pts, idx, uvs)),
        nr.SceneNode(white, 0.25, 0.5, 1.0, 1.0, iso((0.0, -1.25, 0.0)), nr.Plane((0.0, 1.0, 0.0))),
    ]
    cam = dict(eye=(0.0, 2.5, -7.0), at=(0.0, 0.0, 0.0), fovy=45.0, floor_y=-1.25)
    return nr.Scene(nodes, _lights(lights, area), (0.25, 0.375, 0.5)), cam


# ---- frames -----------------------------------------------------------------------------------------------------------------------------
# kind -> (samples per pixel, window width, is a plain frame unless the scene has an area light)
FRAME_KINDS = {
    "plain": (1, 0.0),         # one sample, no window
    "window": (1, 1.0),        # a general frame with one lane per pixel (the only general frames that can run at OCC = 3, besides area lights)
    "aa": (3, 1.0),            # anti-aliased: two lanes per pixel
    "area": (1, 0.0),          # one sample, no window, but the scene's first light is a disc: general
    "instrumented": (1, 0.0),  # nrays_render_device_instrumented
}
SIZES = [(160, 120), (150, 100), (173, 111), (164, 92), (128, 96), (157, 119)]  # four of six are whole neither in 8 x 8 wave tiles nor in 16 x 16 blocks


class Case:
    def __init__(self, name, expect, builder, kwargs, kind, env, listed, size):
        self.name, self.expect, self.builder, self.kwargs, self.kind, self.env, self.listed, self.size = name, expect, builder, dict(kwargs), kind, dict(env), listed, size
        assert kind in FRAME_KINDS and all(k in SWITCHES for k in env)
        assert (kind == "area") == bool(kwargs.get("area", 0)), name
        self.max_depth = 5 if builder is double_scene else 0  # bounds the ray tree of double-branching nodes (0: the energy rule alone)

    def build(self, opaque_twin=False):
        """(scene, camera).  The library reads the switches when the handle is created: create it inside environment()."""
        return self.builder(**dict(self.kwargs, opaque_twin=True)) if opaque_twin else self.builder(**self.kwargs)

    def params(self, cam):
        spp, window = FRAME_KINDS[self.kind]
        return su.camera_params(cam, self.size[0], self.size[1], spp=spp, window=window, seed=7, max_depth=self.max_depth)[0]

    def oracle_key(self, opaque_twin=False):
        spp, window = FRAME_KINDS[self.kind]
        return (self.builder.__name__, tuple(sorted(self.kwargs.items())), spp, window, self.size, opaque_twin)

    def environment(self):
        return _Environment(self.env)

    def __repr__(self):
        return self.name


class _Environment:
    """The five switches exactly as the case names them (the others unset), restored on exit."""

    def __init__(self, env):
        self.env = env

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in SWITCHES}
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        return False


def _build_table():
    cases = []

    def add(expect, builder, kwargs, kind, env=None, listed=True):
        stats, feat, plain, occ = expect
        name = "%s%d_%s_occ%d_%s%s" % ("stats" if stats else "feat", feat, "plain" if plain else "general", occ, kind, "" if listed else "_fallback")
        while any(c.name == name for c in cases):
            name += "_b"
        cases.append(Case(name, (bool(stats), feat, bool(plain), occ), builder, kwargs, kind, env or {}, listed, SIZES[len(cases) % len(SIZES)]))

    # group 0: the full kernels.  15 / 31 / 3 / 19 exist only as general kernels: their plain frames fall back to them
    add((True, 31, False, 0), double_scene, dict(lights=2), "instrumented")
    add((False, 31, False, 0), double_scene, dict(lights=2), "aa")
    add((False, 31, False, 0), double_scene, dict(lights=1, area=2), "area", listed=False)
    add((False, 31, False, 0), double_scene, dict(lights=2), "plain", listed=False)
    add((False, 15, False, 0), double_scene, dict(lights=1), "window")
    add((False, 15, False, 0), double_scene, dict(lights=1), "plain", listed=False)
    add((False, 3, False, 0), mesh_scene, dict(ball=True, rotate=True), "window")
    add((False, 3, False, 0), mesh_scene, dict(ball=True), "plain", listed=False)
    add((False, 19, False, 0), mesh_scene, dict(ball=True, lights=2), "aa")
    add((False, 19, False, 0), mesh_scene, dict(ball=True, lights=2, rotate=True), "plain", listed=False)

    # groups 1, 2 and 7: analytic scenes.  Records in LDS unless NRAYS_LDS_SCENE=0; the opaque ones are tiny scenes unless they have more than
    # TINY_LEAVES leaves or NRAYS_TINY_SCENE=0
    general = {1: "window", 5: "area", 17: "aa", 21: "window"}
    for base, transparent, lights in ((1, False, 1), (5, True, 1), (17, False, 2), (21, True, 2)):
        for lds in (True, False):
            env, kw = ({} if lds else {"NRAYS_LDS_SCENE": "0"}), dict(transparent=transparent, lights=lights)
            if lds and base == 1:
                kw["leaves"] = TINY_LEAVES + 2  # too many leaves for the stackless queries
            if lds and base == 17:
                env["NRAYS_TINY_SCENE"] = "0"   # few enough leaves, switched off
            feat = base + (LDS if lds else 0)
            add((False, feat, True, 0), analytic_scene, kw, "plain", env)
            kind = general[base] if lds else {"window": "aa", "aa": "window", "area": "window"}[general[base]]
            add((False, feat, False, 0), analytic_scene, dict(kw, area=1) if kind == "area" else kw, kind, env)
    add((False, 1 + LDS + TINY, True, 0), analytic_scene, dict(leaves=TINY_LEAVES), "plain")
    add((False, 1 + LDS + TINY, False, 0), analytic_scene, dict(leaves=5), "window")
    add((False, 1 + LDS + TINY, False, 0), analytic_scene, dict(leaves=TINY_LEAVES, area=1), "area", listed=False)
    add((False, 17 + LDS + TINY, True, 0), analytic_scene, dict(leaves=TINY_LEAVES, lights=2), "plain")
    add((False, 17 + LDS + TINY, False, 0), analytic_scene, dict(leaves=6, lights=1, area=2), "area")
    add((False, 17 + LDS + TINY, False, 0), analytic_scene, dict(leaves=TINY_LEAVES, lights=2), "aa", listed=False)

    # groups 3 and 4: mesh scenes at two waves per SIMD (NRAYS_OCC=2 where the library would otherwise choose by the frame's size).
    # rotate=True is the sibling of every untransformed scene: one rotated BLAS, no bit 64
    general = {2: "window", 6: "aa", 18: "area", 22: "window"}
    for base, alpha, lights in ((2, False, 1), (6, True, 1), (18, False, 2), (22, True, 2)):
        for noxform in (False, True):
            env = {"NRAYS_OCC": "2"} if alpha else {}
            feat = base + (NOXFORM if noxform else 0)
            kw = dict(alpha=alpha, lights=lights, rotate=not noxform)
            add((False, feat, True, 0), mesh_scene, kw, "plain", env)
            kind = general[base] if noxform else {"window": "aa", "aa": "window", "area": "aa"}[general[base]]
            add((False, feat, False, 0), mesh_scene, dict(kw, lights=1, area=2) if kind == "area" else kw, kind, env)
    add((False, 2, True, 0), mesh_scene, dict(), "plain", {"NRAYS_NOXFORM": "0"}, listed=False)  # untransformed, switched off
    add((False, 22, False, 0), mesh_scene, dict(alpha=True, lights=2), "aa", {"NRAYS_NOXFORM": "0", "NRAYS_OCC": "2"}, listed=False)
    for base, lights, kind in ((7, 1, "aa"), (23, 2, "window")):
        add((False, base, False, 0), mesh_scene, dict(alpha=True, lights=lights, ball=True, rotate=True), kind, {"NRAYS_OCC": "2"})
        add((False, base, False, 0), mesh_scene, dict(alpha=True, lights=lights, ball=True), "plain", {"NRAYS_OCC": "2"}, listed=False)

    # groups 5 and 6: the three-wave builds (NRAYS_OCC=3), parked shading state unless NRAYS_PARK=0
    for noxform in (False, True):
        for base, lights in ((6, 1), (22, 2)):
            for park in (True, False):
                env = {"NRAYS_OCC": "3"} if park else {"NRAYS_OCC": "3", "NRAYS_PARK": "0"}
                feat = base + (NOXFORM if noxform else 0) + (PARK if park else 0)
                kw = dict(alpha=True, lights=lights, rotate=not noxform)
                add((False, feat, True, 3), mesh_scene, kw, "plain", env)
                kind = "area" if (base == 22 and park) else "window"
                add((False, feat, False, 3), mesh_scene, dict(kw, lights=1, area=2) if kind == "area" else kw, kind, env)
    for base, lights in ((7, 1), (23, 2)):
        add((False, base, False, 3), mesh_scene, dict(alpha=True, lights=lights, ball=True), "window", {"NRAYS_OCC": "3"})
        add((False, base, False, 3), mesh_scene, dict(alpha=True, lights=lights, ball=True, rotate=True), "plain", {"NRAYS_OCC": "3", "NRAYS_PARK": "0"}, listed=False)
    # an anti-aliased frame has several lanes per pixel: NRAYS_OCC=3 does not apply to it
    add((False, 22, False, 0), mesh_scene, dict(alpha=True, lights=2, rotate=True), "aa", {"NRAYS_OCC": "3"}, listed=False)
    return cases


CASES = _build_table()


def listed_permutations():
    """The permutations the table claims to reach exactly (not as a fall-back)."""
    return {c.expect for c in CASES if c.listed}


# ---- the oracle's view of a case (what the conditions of tests/test_permutation_table.py are evaluated on) --------------------------------
_ORACLE_FRAMES = {}


def oracle_frame(case, opaque_twin=False):
    """(image, {ray class: count}, background) of the case's frame by the CPU oracle; cases that share scene, frame kind and size share it."""
    key = case.oracle_key(opaque_twin)
    if key not in _ORACLE_FRAMES:
        import oracle
        sc, cam = case.build(opaque_twin)
        img, st = oracle.render(sc.descriptor, case.params(cam), 8)
        counts = {k: int(getattr(st, k)) for k in ("rays_primary", "rays_reflection", "rays_refraction", "rays_shadow")}
        _ORACLE_FRAMES[key] = (img, counts, sc._background)
    return _ORACLE_FRAMES[key]


_FLOOR_SHADOWS = {}


def filtered_floor_shadows(case):
    """Shadow rays from a grid of points just above the floor (it fills the frame) to the first light, by the oracle's Scene::intersects_ray:
    how many arrive dimmed by a non-opaque node (neither blocked nor untouched)."""
    import numpy as np
    import oracle
    key = (case.builder.__name__, tuple(sorted(case.kwargs.items())))
    if key in _FLOOR_SHADOWS:
        return _FLOOR_SHADOWS[key]
    sc, cam = case.build()
    light = np.asarray(sc._lights[0].pos)
    n = 0
    for x in np.arange(-5.0, 5.5, 0.5):
        for z in np.arange(-5.0, 5.5, 0.5):
            o = np.array([x, cam["floor_y"] + 1.0 / 64.0, z])
            d = light - o
            f = oracle.shadow(sc.descriptor, o, d / np.linalg.norm(d), float(np.linalg.norm(d)))
            n += 1 if (f is not None and float(f.min()) < 1.0) else 0
    _FLOOR_SHADOWS[key] = n
    return n
