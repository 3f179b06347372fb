"""The named scenes of tests/test_scene_cover.py (host: tests/scene_dump_shim.cpp) and tests/test_scene_cover_gpu.py (the device's arrays: nrays_debug_scene_dump), written
once for both, and the two ways of taking a dump in the field set tests/scene_cover.py validates.

Where a box face of the TLAS can fall short of the reference's AABB: world_box (scene_build.cpp) forms wc - wh and wc + wh in f64 and rounds outward to f32; the reference
forms the same face through OTHER f64 sums (a support point mapped and translated; R c + t and |R| h summed in another order; a member of a merged group from its own
centre).  Where the face lies at a coordinate plane of the world the terms cancel, an f32 step of the RESULT is as small as the result itself, and only a margin relative
to the TERMS covers the difference.  So the `resting` shapes are translated by -aabb_min(their AABB at zero translation): the reference's minima then sit at +-0 or a few
1e-16 from it on every axis, for every rotation of ROTATIONS (quarter, half, eighth, sixth and twelfth turns about the axes and diagonals: many exact zeros and equal
entries in R).  `merged` does the same with the first member of a group of three meshes sharing one rotated isometry."""
import ctypes as C
import math
import os
import subprocess

import numpy as np

import nrays_amd as nr
from nrays_amd import abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
BACKGROUND = (0.25, 0.5, 0.75)
GPU_BUILD_MIN = 16                       # `mixed`: meshes of 16 triangles and more go to the device builder (on the host: the shim's fake one)
NAMES = ("empty", "one_ball", "one_triangle", "resting", "merged", "mixed", "many")

AXES = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 1, 1), (0, 1, 1))
ANGLES = (90.0, -90.0, 180.0, 45.0, 60.0, 30.0)
ROTATIONS = tuple(tuple(c * math.radians(a) / math.sqrt(sum(axis)) for c in axis) for axis in AXES for a in ANGLES)
# The capsule of the issue's experiment: turned by pi about (1, 1, 0) / sqrt 2 and resting on x = 0, world_box's min x came out at +4.44e-16, above the reference's 0.0.
CAPSULE_HALF_HEIGHT, CAPSULE_RADIUS = 0.7458903193473816, 1.9824098348617554
CAPSULE_ROTATION = (2.221441469079183, 2.221441469079183, 0.0)
assert CAPSULE_ROTATION in ROTATIONS


def lights():
    return [nr.Light((3.0, 30.0, 5.0), 0.0, 1, (1, 1, 1))]


def phong(alpha_map=None):
    return nr.PhongMaterial((0.2, 0.3, 0.4), (0.5, 0.5, 0.5), (0.1, 0.1, 0.1), None, alpha_map, 20.0)


def node(geometry, iso=None, material=None, alpha=1.0):
    return nr.SceneNode(material or nr.NormalMaterial(), 0.0, 0.0, alpha, 1.0, iso or nr.Isometry3.identity(), geometry, None, True)


def f32_exact(a):
    return np.asarray(a, F32).astype(np.float64)


def soup(rng, tris, centre, half=(1.0, 1.0, 1.0)):
    """`tris` random triangles inside centre +- half, f32-exact, with uvs per vertex."""
    pts = f32_exact(np.asarray(centre) + rng.uniform(-1.0, 1.0, (3 * tris, 3)) * np.asarray(half))
    return pts, np.arange(3 * tris, dtype=np.uint32).reshape(-1, 3), f32_exact(rng.uniform(0.0, 1.0, (3 * tris, 2)))


def alpha_map():
    texels = np.full((4, 4, 4), 255, np.uint8)
    texels[::2, 1::2, 3] = 64
    return nr.Texture2d(nr.ImageData(texels))


def resting_on_the_planes(make_node):
    """make_node(translation) -> SceneNode.  The node translated by -aabb_min of its reference AABB at zero translation."""
    import oracle
    at_zero = oracle.node_aabb(nr.Scene([make_node((0.0, 0.0, 0.0))], lights(), BACKGROUND).descriptor, 0)
    return make_node(tuple(-at_zero[:3]))


def resting_nodes():
    rng = np.random.default_rng(41)
    out = []
    for w in ROTATIONS:
        p = f32_exact(rng.uniform(0.4, 2.0, 10))
        if w == CAPSULE_ROTATION:
            p[8:] = CAPSULE_HALF_HEIGHT, CAPSULE_RADIUS       # (elsewhere every capsule has its own size: turned about its own axis, equal ones would coincide)
        shapes = (nr.Ball(p[0]), nr.Cuboid(p[1:4]), nr.Cylinder(p[4], p[5]), nr.Capsule(p[8], p[9]), nr.Cone(p[6], p[7]))
        for g in shapes:
            out.append(resting_on_the_planes(lambda t, g=g: node(g, nr.Isometry3(t, w))))
    return out


def merged_nodes():
    """Three meshes under one rotated isometry: opaque, alpha = 0.5, alpha-mapped with uvs; disjoint local boxes; 20 + 24 + 17 triangles.  The half turn about
    (1, 1, 0) maps local (x, y, z) to world (y, x, -z) up to the rounding of R, and the first member spans the group's local box at its lower x and y faces and on z: the
    three world minima of the merged BLAS are faces of the first member, formed from the union's centre by world_box and from the member's own by the reference.
    (Whether the two sums then differ is a matter of the vertices' last bits: against world_box before its margin, 17 of the 24 seeds 40 .. 63 gave a box that left
    the first member's reference AABB outside by 4.4e-16 on one face; 41 is one of them.)"""
    rng = np.random.default_rng(41)
    w = CAPSULE_ROTATION
    a, b, c = soup(rng, 20, (0, 0, 0)), soup(rng, 24, (3, 0, 0), (1.0, 0.5, 0.5)), soup(rng, 17, (0, 3, 0), (0.5, 1.0, 0.5))
    first = resting_on_the_planes(lambda t: node(nr.TriMesh(a[0], a[1]), nr.Isometry3(t, w), phong()))
    iso = first.transform
    return [first, node(nr.TriMesh(b[0], b[1]), nr.Isometry3(iso.translation, iso.axis_angle), phong(), alpha=0.5),
            node(nr.TriMesh(c[0], c[1], c[2]), nr.Isometry3(iso.translation, iso.axis_angle), phong(alpha_map()))]


def mixed_nodes():
    rng = np.random.default_rng(47)
    out = merged_nodes()
    for tris, centre in ((4, (-6, 0, 0)), (6, (-6, 3, 0))):            # a second group, untransformed: kInstNoXform, host-built beside the device-built ones
        p, i, _ = soup(rng, tris, centre)
        out.append(node(nr.TriMesh(p, i), nr.Isometry3.identity(), phong()))
    out += resting_nodes()[::7]
    out.append(node(nr.Plane((0.0, 1.0, 0.0)), nr.Isometry3((0.0, -9.0, 0.0), (0.0, 0.0, 0.0)), phong()))
    out.append(node(nr.Plane((1.0, 0.0, 0.25)), nr.Isometry3((-12.0, 0.0, 0.0), (0.0, 0.3, 0.0)), phong(), alpha=0.5))
    out.append(node(nr.TriMesh(np.zeros((3, 3)), np.zeros((0, 3), np.uint32)), nr.Isometry3((1.0, 2.0, 3.0), ROTATIONS[5]), phong()))   # no triangles
    p, i, _ = soup(rng, 8, (6, 0, 0))
    out.append(node(nr.TriMesh(p, i), nr.Isometry3((0.5, 0.25, -1.0), ROTATIONS[9]), nr.UVMaterial()))                                   # UV material, no uvs: never opaque
    p, i, _ = soup(rng, 20, (6, 4, 0))
    out.append(node(nr.TriMesh(p, i), nr.Isometry3((0.0, 1.0, 2.0), ROTATIONS[16]), phong(), alpha=1.5))                                 # device-built, alone: single_bounds
    return out


def many_nodes():
    rng = np.random.default_rng(53)
    out = []
    for k in range(300):
        iso = nr.Isometry3(tuple(f32_exact(rng.uniform(-20.0, 20.0, 3))), ROTATIONS[int(rng.integers(len(ROTATIONS)))])
        what = k % 3
        if what == 0:
            out.append(node(nr.Ball(f32_exact(rng.uniform(0.2, 1.0))), iso, phong(), alpha=1.0 if k % 2 else 0.5))
        elif what == 1:
            out.append(node(nr.Cuboid(f32_exact(rng.uniform(0.2, 1.0, 3))), iso))
        else:
            p, i, _ = soup(rng, 1, (0, 0, 0))
            out.append(node(nr.TriMesh(p, i), iso, phong(), alpha=1.0 if k % 4 else 0.25))
    return out


def scene_nodes(name):
    if name == "empty":
        return []
    if name == "one_ball":
        return [node(nr.Ball(0.75), nr.Isometry3((1.0, 2.0, 3.0), ROTATIONS[3]))]
    if name == "one_triangle":
        return [node(nr.TriMesh(f32_exact([[0, 0, 0], [1, 0, 0], [0, 1, 0.5]]), np.asarray([[0, 1, 2]], np.uint32)), nr.Isometry3((1.0, 2.0, 3.0), ROTATIONS[4]))]
    if name == "resting":
        return resting_nodes() + [node(nr.Plane((0.0, 1.0, 0.0)), nr.Isometry3((0.0, -40.0, 0.0), (0.0, 0.0, 0.0)), phong())]
    return dict(merged=merged_nodes, mixed=mixed_nodes, many=many_nodes)[name]()


_made = {}


def case(name):
    """(nodes, Scene for the descriptor and the oracle, the reference's AABBs nodes x 6), made once and left unchanged."""
    if name not in _made:
        import oracle
        nodes = scene_nodes(name)
        scene = nr.Scene(nodes, lights(), BACKGROUND)
        ref = np.asarray([oracle.node_aabb(scene.descriptor, i) for i in range(len(nodes))], np.float64).reshape(-1, 6)
        ref.setflags(write=False)
        _made[name] = (nodes, scene, ref)
    return _made[name]


def build_min(name):
    return GPU_BUILD_MIN if name == "mixed" else 0


# ---- taking a dump ------------------------------------------------------------------------------------------------------------------

def take_dump(call):
    """call(pointer to NraysSceneDump) -> status, under the capacity contract of nrays_debug_scene_dump: once for the sizes, once for the arrays.  Returns the dict
    tests/scene_cover.py validates."""
    d = abi.NraysSceneDump()
    rc = call(C.byref(d))
    sizes = (d.num_nodes, d.num_tris, d.num_instances, d.num_shadow_instances, d.num_planes, d.num_scene_nodes)
    assert rc == (abi.ERR_BAD_ARG if any(sizes) else abi.OK), rc
    arrays = dict(nodes=np.zeros((d.num_nodes, 32), F32), tris=np.zeros((d.num_tris, 48), np.uint8), instances=np.zeros((d.num_instances, 136), np.uint8),
                  shadow_instances=np.zeros((d.num_shadow_instances, 136), np.uint8), links=np.zeros((d.num_instances, 2), np.int32),
                  shadow_links=np.zeros((d.num_shadow_instances, 2), np.int32), planes=np.zeros(d.num_planes, np.int32), shadow_planes=np.zeros(d.num_planes, np.int32),
                  node_aabbs=np.zeros((d.num_scene_nodes, 6), np.float64))
    d.node_capacity, d.tri_capacity, d.instance_capacity, d.shadow_instance_capacity, d.plane_capacity, d.scene_node_capacity = sizes
    for key, a in arrays.items():
        setattr(d, key, a.ctypes.data_as(dict(abi.NraysSceneDump._fields_)[key]) if a.size else None)
    rc = call(C.byref(d))
    assert rc == abi.OK, rc
    assert (d.num_nodes, d.num_tris, d.num_instances, d.num_shadow_instances, d.num_planes, d.num_scene_nodes) == sizes
    out = dict(arrays)
    out.update(closest_root=d.closest_root, shadow_root=d.shadow_root, max_bvh_depth=d.max_bvh_depth, bounded=bool(d.bounded), dev_nodes=d.dev_nodes, dev_tris=d.dev_tris,
               bounds_mn=np.asarray(d.bounds_mn[:], F32), bounds_mx=np.asarray(d.bounds_mx[:], F32))
    return out


class HostDump:
    """tests/scene_dump_shim.cpp, compiled as tests/test_host_scene.py compiles its shim.  scene_build: another scene_build.cpp to build against (an earlier commit's)."""

    def __init__(self, directory, scene_build=None):
        out = os.path.join(str(directory), "libscene_dump_shim.so")
        csrc = os.path.join(ROOT, "nrays_amd", "csrc")
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", csrc, "-fPIC", "-shared", "-pthread", "-o", out,
                               os.path.join(ROOT, "tests", "scene_dump_shim.cpp"), scene_build or os.path.join(csrc, "scene_build.cpp")] +
                              [os.path.join(csrc, f) for f in ("bvh_build.cpp", "switches.cpp")])
        self.lib = C.CDLL(out)
        self.lib.scene_dump_host.argtypes = [C.POINTER(abi.NraysSceneDesc), C.c_uint32, C.POINTER(abi.NraysSceneDump)]
        self.lib.scene_dump_last_error.restype = C.c_char_p

    def dump(self, scene, gpu_build_min=0):
        return take_dump(lambda d: self.lib.scene_dump_host(scene.descriptor.pointer(), gpu_build_min, d))


def device_dump(scene):
    """The device's own arrays of a created scene."""
    lib = abi.load_hip_lib()
    return take_dump(lambda d: lib.nrays_debug_scene_dump(scene.device_handle(), d))


# ---- rays at the faces of the reference AABBs ---------------------------------------------------------------------------------------------
# For every face of every bounded node's reference AABB: rays through the point where the node touches that face, starting in the face's plane or one f64 step to
# either side of it, their direction component on the face's axis 0, +-1e-300, +-2^-60 or ordinary.  A ray IN the plane with a zero component passes the reference's
# slab test on that axis by its origin alone (min <= o <= max), one step outside it does not: the node is cast or not on the strength of the last bit, and the f32
# TLAS box in front of it has to let through everything that the exact gate behind it then decides.
RAY_SCENES = ("resting", "merged", "mixed")
COMPONENTS = (0.0, 1e-300, -1e-300, 2.0 ** -60, -2.0 ** -60, None, None)   # None: ordinary (twice: as often as the zero and tiny ones together would be too rare)
STEPS = (0, -1, 1)
RAYS_PER_FACE = dict(resting=3, merged=168, mixed=21)                   # of the 21 (step, component) pairs, dealt in turn; merged: 8 aims around the point for each


def touch_point(n, axis, sign):
    """Where node n touches the face `sign` (-1 lower, +1 upper) of its world AABB on `axis`, in plain float64 (an aim, not a claim)."""
    from tests import scene_cover as sv
    g = n.geometry
    R = np.asarray(sv.rotation(n.transform.axis_angle), np.float64).reshape(3, 3)
    t = np.asarray(n.transform.translation, np.float64)
    e = np.zeros(3); e[axis] = sign
    if g.kind == sv.TRIMESH:
        v = np.asarray(g.points, np.float64)[np.unique(np.asarray(g.indices, np.int64))] @ R.T + t
        return v[np.argmax(v[:, axis] * sign)]
    if g.kind == sv.BALL:
        return t + e * g.params[0]
    dl = R.T @ e
    if g.kind == sv.CUBOID:
        p = np.where(dl >= 0, 1.0, -1.0) * np.asarray(g.params)
    else:
        hh, r = g.params[0], g.params[1]
        rad = np.asarray([dl[0], 0.0, dl[2]])
        rad = rad / np.linalg.norm(rad) * r if np.linalg.norm(rad) > 0 else rad
        up = np.asarray([0.0, math.copysign(hh, dl[1]), 0.0])
        if g.kind == sv.CYLINDER:
            p = rad + up
        elif g.kind == sv.CAPSULE:
            p = up + dl * r
        else:
            base, apex = rad + np.asarray([0.0, -hh, 0.0]), np.asarray([0.0, hh, 0.0])
            p = base if base @ dl >= apex @ dl else apex
    return R @ p + t


def face_rays(name):
    """(origins, dirs, node aimed at, face 0..5) of scene `name`."""
    from tests import scene_cover as sv
    nodes, _, ref = case(name)
    rng = np.random.default_rng(600 + NAMES.index(name))
    pairs = [(s, c) for s in STEPS for c in range(len(COMPONENTS))]
    O, D, N, F = [], [], [], []
    turn = 0
    for i, n in enumerate(nodes):
        if n.geometry.kind == sv.PLANE or (n.geometry.kind == sv.TRIMESH and len(n.geometry.indices) == 0):
            continue
        for face in range(6):
            axis, sign = face % 3, (-1.0 if face < 3 else 1.0)
            q0 = touch_point(n, axis, sign)
            for _ in range(RAYS_PER_FACE[name]):
                step, comp = pairs[turn % len(pairs)]
                turn += 1
                q = q0.copy()
                q[axis] = ref[i, face]
                if step:
                    q[axis] = np.nextafter(q[axis], step * np.inf)
                # Every ray comes out of the octant in which the resting nodes lie (all components <= 0, the tiny ones aside).  A ray from anywhere else enters that
                # octant through a coordinate plane, where every node with a flat face in it is met at ONE distance: a third of `resting`'s rays then had two nodes at
                # the same toi.  From inside the octant a ray in such a plane meets each flat face at the face's own far edge.
                u = rng.normal(size=3); u = -np.abs(u) / np.linalg.norm(u)
                if COMPONENTS[comp] is not None:
                    u[axis] = 0.0
                    u /= np.linalg.norm(u)
                    u[axis] = COMPONENTS[comp]
                o = q - 10.0 ** rng.uniform(1.3, 1.6) * u             # from 20 .. 40 away: outside every bounded node (a ray from inside solids meets them all at 0)
                if COMPONENTS[comp] is not None and abs(COMPONENTS[comp]) < 1e-100:
                    o[axis] = q[axis]                                   # in the plane (or the step beside it), to the last bit
                O.append(o); D.append(u); N.append(i); F.append(face)
    return np.ascontiguousarray(O), np.ascontiguousarray(D), np.asarray(N), np.asarray(F)


_expected = {}


def expected(name):
    """The oracle's answers, once per scene: o, d, hit, toi, node (brute force over all nodes and triangles), tie (the brute force names another node when the nodes
    are listed in reverse: two nodes at the same distance, tie rule D-2 takes the smaller index), and per limit of Scene::intersects_ray — at the hit's distance, one
    f64 step below, one above — the limits and whether the ray is blocked."""
    if name not in _expected:
        import oracle
        nodes, scene, _ = case(name)
        o, d, aimed, face = face_rays(name)
        hit, out = oracle.cast(scene.descriptor, o, d, bruteforce=True)
        rhit, rout = oracle.cast(nr.Scene(nodes[::-1], lights(), BACKGROUND).descriptor, o, d, bruteforce=True)
        node = np.where(hit, out[:, 7].astype(np.int64), -1)
        assert np.array_equal(hit, rhit) and np.array_equal(out[hit, 0], rout[hit, 0])
        tie = hit & (len(nodes) - 1 - rout[:, 7].astype(np.int64) != node)
        toi = np.where(hit, out[:, 0], 1.0)
        limits = dict(at=toi, below=np.where(toi > 0.0, np.nextafter(toi, -np.inf), -1.0), above=np.nextafter(toi, np.inf))
        blocked = {k: np.asarray([oracle.shadow(scene.descriptor, o[i], d[i], lim[i]) is None for i in range(len(o))]) for k, lim in limits.items()}
        e = dict(o=o, d=d, aimed=aimed, face=face, hit=hit, toi=out[:, 0].copy(), node=node, tie=tie, limits=limits, blocked=blocked)
        for v in list(e.values()) + list(limits.values()) + list(blocked.values()):
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _expected[name] = e
    return _expected[name]
