"""Do both TLASes of a flattened scene hold and cover every node of the scene?  A check of a DUMP (the field set of nrays_debug_scene_dump: tests/scene_dump_shim.cpp
on the host, the device's own arrays on the GPU) against the Python scene description, which shares no code with the builder (nrays_amd/csrc/scene_build.cpp:
analytic_instances, mesh_groups, mesh_group_blas, world_box, append_tlas, link_scene).  numpy, math and fractions only.

validate(dump, nodes, ref_aabbs) raises Violation on the first statement that does not hold; Violation.statement names it:

S1 shape       per TLAS: child refs in range, an absent child is kEmptyChild with the inverted box and nothing else is, no node visited twice, depth <= max_bvh_depth, every
               instance in front of the planes is a leaf exactly once, a single instance is a bare leaf root, an empty list an empty root
S2 tags        the three low bits of a leaf ref are the instance's (mesh 4, any-hit 2, untransformed mesh 1); links[i] == (blas_root, flags) of instance i, both lists
S3 nesting     an inner child's box == the union of that node's children's boxes, exactly; the closest root's union == bounds_mn / bounds_mx; bounded iff no plane
S4 planes      planes / shadow_planes index exactly the plane nodes, each once, behind the TLAS leaves, with the node's parameters; no plane inside a TLAS
S5 closest     every non-plane analytic node is exactly one instance (node_id, kind, params, R, t); every triangle of every mesh node is reached under exactly one instance,
               by a walk from blas_root through the dumped nodes to the triangle records (pre-split pieces included) as the set of (node_id, tri_id), with the mesh's own
               vertices; a mesh without triangles is in no instance; node_id == -1 iff the BLAS holds several nodes; the nodes under an instance have bit-equal translation
               and axis-angle, which are the instance's; triangle refs stay below 2^28 and inside the arrays (link_scene's rebase by dev_nodes / dev_tris)
S6 shadow      the same partition; kInstAnyHit iff EVERY node under the instance is opaque; a non-opaque mesh node is alone in its instance, node_id >= 0; an all-opaque
               group shares one BLAS root between the two lists
S7 reference   the instance's f32 box (its parent's slots; the scene bounds for a bare root) contains node_aabbs[node] for every node under it, in both lists, on all six
               faces, compared as doubles without a tolerance; node_aabbs == ref_aabbs (the oracle's node_aabb) bit for bit — except for a mesh without triangles,
               which is under no instance and never cast: ncollide has no AABB for an empty BVT, the builder stores NaNs and the oracle a point
S8 geometry    the eight corners of a node's local box — a mesh's f32 bounds, the cuboid's own box, the bounding cylinder's of cylinder and cone, the capsule's, the ball's
               (unrotated) — mapped by the instance's STORED rot and trans in rational arithmetic, lie inside the instance's box.  No tolerance.

"Opaque" is restated here from Scene::intersects_ray's rule (src/scene.rs:322-331: a hit blocks iff ambiant().w * node.alpha >= 1) and the materials' ambiant()
(NormalMaterial w = 1; UVMaterial w = 1 with uvs and 0 without; PhongMaterial w = the alpha map's sample where the shape carries uvs and a map is set, else 1):
a node is opaque iff its w is 1 whatever the hit and alpha >= 1.  A sampled alpha map never counts as identically 1.  Analytic shapes with uvs: ball, cuboid."""
import math
from fractions import Fraction

import numpy as np

EMPTY = -2**31
LO, HI, CHILD = (0, 4, 3), (1, 6, 7), 2          # slots of a 128-byte node: lower / upper planes for x, y, z; child refs
FLT_MAX = float(np.finfo(np.float32).max)
BALL, CUBOID, CYLINDER, CAPSULE, CONE, PLANE, TRIMESH = range(7)
MAT_PHONG, MAT_NORMAL, MAT_UV = range(3)
INST_ANY_HIT, INST_NO_XFORM = 4, 16
LEAF_NO_XFORM, LEAF_ANY_HIT, LEAF_MESH = 1, 2, 4
INSTANCE = np.dtype([("rot", "<f8", 9), ("trans", "<f8", 3), ("params", "<f8", 3), ("kind", "<u4"), ("flags", "<u4"), ("node_id", "<i4"), ("blas_root", "<i4")])
assert INSTANCE.itemsize == 136
SIDES = (("closest", "instances", "links", "planes", "closest_root"), ("shadow", "shadow_instances", "shadow_links", "shadow_planes", "shadow_root"))


class Violation(AssertionError):
    def __init__(self, statement, text):
        super().__init__("%s: %s" % (statement, text))
        self.statement = statement


def need(ok, statement, text, *args):
    if not ok:
        raise Violation(statement, text % args if args else text)


# ---- the scene description, restated ------------------------------------------------------------------------------------------------

def rotation(axis_angle):
    """Isometry3::new's rotation matrix through the unit quaternion (cos(a / 2), axis sin(a / 2)), row-major: nalgebra's from_scaled_axis and to_rotation_matrix,
    in plain doubles, sin and cos from libm separately."""
    x, y, z = (float(v) for v in axis_angle)
    angle = math.sqrt(x * x + y * y + z * z)
    if angle == 0.0:
        return (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
    s, w = math.sin(angle / 2.0), math.cos(angle / 2.0)
    i, j, k = x / angle * s, y / angle * s, z / angle * s
    ww, ii, jj, kk = w * w, i * i, j * j, k * k
    ij, wk, wj, ik, jk, wi = i * j * 2.0, w * k * 2.0, w * j * 2.0, i * k * 2.0, j * k * 2.0, w * i * 2.0
    return (ww + ii - jj - kk, ij - wk, wj + ik, wk + ij, ww - ii + jj - kk, jk - wi, ik - wj, wi + jk, ww - ii - jj + kk)


def has_uv(node):
    g = node.geometry
    return g.uvs is not None if g.kind == TRIMESH else g.kind in (BALL, CUBOID)


def opaque(node):
    m = node.material
    if m.kind == MAT_NORMAL:
        w_is_one = True
    elif m.kind == MAT_UV:
        w_is_one = has_uv(node)
    else:
        w_is_one = m.alpha is None or not has_uv(node)
    return w_is_one and np.float32(node.alpha) >= np.float32(1.0)


def same_bits(a, b):
    return np.asarray(a, np.float64).tobytes() == np.asarray(b, np.float64).tobytes()


def mesh_local_box(geometry):
    """The f32 min / max over the vertices the faces use."""
    used = np.asarray(geometry.points, np.float64)[np.asarray(geometry.indices, np.int64).ravel()].astype(np.float32)
    return used.min(axis=0), used.max(axis=0)


def local_box(kind, params, geometry=None):
    """(centre, half extent) of the local box of S8 as Fractions."""
    if kind == TRIMESH:
        mn, mx = mesh_local_box(geometry)
        lo, hi = [Fraction(float(v)) for v in mn], [Fraction(float(v)) for v in mx]
        return [(a + b) / 2 for a, b in zip(lo, hi)], [(b - a) / 2 for a, b in zip(lo, hi)]
    p = [abs(Fraction(float(v))) for v in params]
    zero = [Fraction(0)] * 3
    if kind == BALL:
        return zero, [p[0], p[0], p[0]]
    if kind == CUBOID:
        return zero, p
    if kind == CAPSULE:
        return zero, [p[1], p[0] + p[1], p[1]]
    return zero, [p[1], p[0], p[1]]                   # cylinder, cone: half height along y, radius across


# ---- the dumped trees ----------------------------------------------------------------------------------------------------------------

def child_boxes(nodes):
    n = np.asarray(nodes, np.float32).reshape(-1, 8, 4)
    lo = np.stack([n[:, s, :] for s in LO], axis=2).astype(np.float64)      # node x child x axis
    hi = np.stack([n[:, s, :] for s in HI], axis=2).astype(np.float64)
    return lo, hi, n[:, CHILD, :].view(np.int32).astype(np.int64)


def walk_tlas(dump, side):
    """S1 and S2 of one TLAS.  Returns leaf_box: instance index -> (lo, hi) of its slot in its parent (the scene bounds for a bare root), the inner nodes visited and
    the depth of the deepest (root node = 0)."""
    name, inst_key, link_key, plane_key, root_key = side
    inst, root = dump[inst_key], int(dump[root_key])
    n_leaf = len(inst) - len(dump[plane_key])
    lo, hi, refs = dump["_boxes"]
    n_nodes = len(refs)
    need(n_leaf >= 0, "S1", "%s: more planes than instances", name)
    bounds = (np.asarray(dump["bounds_mn"], np.float64), np.asarray(dump["bounds_mx"], np.float64))
    leaf_box, visited, deepest = {}, [], 0

    def check_tag(ref, where):
        v = ~ref & 0xffffffff
        idx, bits = v >> 3, v & 7
        need(idx < n_leaf, "S1", "%s: %s is a leaf for instance %d of %d in front of the planes", name, where, idx, n_leaf)
        need(idx not in leaf_box, "S1", "%s: instance %d is a leaf twice", name, idx)
        i = inst[idx]
        mesh = int(i["kind"]) == TRIMESH
        want = (LEAF_MESH if mesh else 0) | (LEAF_ANY_HIT if int(i["flags"]) & INST_ANY_HIT else 0) | (LEAF_NO_XFORM if mesh and int(i["flags"]) & INST_NO_XFORM else 0)
        need(bits == want, "S2", "%s: %s carries the tag bits %d, instance %d says %d", name, where, bits, idx, want)
        return idx

    if n_leaf == 0:
        need(root == EMPTY, "S1", "%s: an empty list with the root %d", name, root)
    elif n_leaf == 1:
        need(root < 0 and root != EMPTY, "S1", "%s: a single instance, but the root %d is no bare leaf", name, root)
        leaf_box[check_tag(root, "the root")] = bounds
    else:
        need(0 <= root < n_nodes, "S1", "%s: root %d of %d nodes", name, root, n_nodes)
        seen = set()
        front = [(root, 0)]
        while front:
            node, depth = front.pop()
            need(node not in seen, "S1", "%s: node %d is visited twice", name, node)
            need(depth <= int(dump["max_bvh_depth"]), "S1", "%s: node %d at depth %d, max_bvh_depth %d", name, node, depth, int(dump["max_bvh_depth"]))
            seen.add(node); visited.append(node)
            deepest = max(deepest, depth)
            present = 0
            for k in range(4):
                ref = int(refs[node, k])
                inverted = (lo[node, k] == FLT_MAX).all() and (hi[node, k] == -FLT_MAX).all()
                need((ref == EMPTY) == bool(inverted), "S1", "%s: node %d child %d: ref %d with %s box", name, node, k, ref, "the inverted" if inverted else "a real")
                if ref == EMPTY:
                    continue
                present += 1
                if ref >= 0:
                    need(ref < n_nodes, "S1", "%s: node %d child %d = %d of %d nodes", name, node, k, ref, n_nodes)
                    front.append((ref, depth + 1))
                else:
                    leaf_box[check_tag(ref, "node %d child %d" % (node, k))] = (lo[node, k].copy(), hi[node, k].copy())
            need(present > 0, "S1", "%s: node %d has no child", name, node)
    missing = [i for i in range(n_leaf) if i not in leaf_box]
    need(not missing, "S1", "%s: instances %s are in no leaf", name, missing[:5])
    links = np.asarray(dump[link_key], np.int64).reshape(-1, 2)
    need(len(links) == len(inst), "S2", "%s: %d links for %d instances", name, len(links), len(inst))
    for i in range(len(inst)):
        want = (int(inst[i]["blas_root"]), int(inst[i]["flags"]))
        need((int(links[i, 0]), int(links[i, 1]) & 0xffffffff) == want, "S2", "%s: links[%d] = %s, the instance says %s", name, i, tuple(links[i]), want)
    return leaf_box, visited, deepest


def check_nesting(dump, side, visited):
    name, root = side[0], int(dump[side[4]])
    lo, hi, refs = dump["_boxes"]

    def union(node):
        real = refs[node] != EMPTY
        return lo[node][real].min(axis=0), hi[node][real].max(axis=0)
    for node in visited:
        for k in range(4):
            ref = int(refs[node, k])
            if ref >= 0:
                u_lo, u_hi = union(ref)
                need((u_lo == lo[node, k]).all() and (u_hi == hi[node, k]).all(), "S3", "%s: node %d child %d: box %s %s, the union of node %d's children is %s %s", name, node, k,
                     lo[node, k], hi[node, k], ref, u_lo, u_hi)
    if name == "closest" and root >= 0:
        u_lo, u_hi = union(root)
        need((u_lo == np.asarray(dump["bounds_mn"], np.float64)).all() and (u_hi == np.asarray(dump["bounds_mx"], np.float64)).all(), "S3",
             "the closest root's union %s %s is not the scene bounds %s %s", u_lo, u_hi, dump["bounds_mn"], dump["bounds_mx"])


def check_planes(dump, nodes, side):
    name, inst, planes = side[0], dump[side[1]], [int(p) for p in dump[side[3]]]
    n_leaf = len(inst) - len(planes)
    want = [i for i, n in enumerate(nodes) if n.geometry.kind == PLANE]
    need(sorted(planes) == list(range(n_leaf, len(inst))), "S4", "%s: planes %s do not index the %d instances behind the %d leaves", name, planes, len(planes), n_leaf)
    need(sorted(int(inst[p]["node_id"]) for p in planes) == want, "S4", "%s: the plane instances name the nodes %s, the scene's planes are %s", name, [int(inst[p]["node_id"]) for p in planes], want)
    for p in planes:
        i, n = inst[p], nodes[int(inst[p]["node_id"])]
        need(int(i["kind"]) == PLANE and same_bits(i["params"], n.geometry.params) and same_bits(i["trans"], n.transform.translation) and same_bits(i["rot"], rotation(n.transform.axis_angle)),
             "S4", "%s: plane instance %d is not node %d", name, p, int(i["node_id"]))
    for k in range(n_leaf):
        need(int(inst[k]["kind"]) != PLANE, "S4", "%s: instance %d, a plane, is inside the TLAS", name, k)
    if name == "closest":
        need(bool(dump["bounded"]) == (not want), "S3", "bounded = %s with %d planes", bool(dump["bounded"]), len(want))


def walk_blas(dump, root, where):
    """The (node_id, tri_id) pairs and the records reached from a BLAS root."""
    lo, hi, refs = dump["_boxes"]
    tris = dump["tris"]
    n_nodes, n_tris = len(refs), len(tris)
    records, seen = [], set()

    def leaf(ref):
        v = ~ref & 0xffffffff
        first, count = v >> 3, (v & 7) + 1
        need(first < 2**28 and first + count <= n_tris, "S5", "%s: leaf ref %d names the records [%d, %d) of %d", where, ref, first, first + count, n_tris)
        records.extend(range(first, first + count))
    need(root != EMPTY, "S5", "%s: an empty BLAS", where)
    if root < 0:
        leaf(root)
        return records
    front = [(root, 0)]
    while front:
        node, depth = front.pop()
        need(0 <= node < n_nodes, "S5", "%s: BLAS node %d of %d", where, node, n_nodes)
        need(node not in seen, "S5", "%s: BLAS node %d is visited twice", where, node)
        need(depth <= int(dump["max_bvh_depth"]), "S5", "%s: BLAS node %d at depth %d, max_bvh_depth %d", where, node, depth, int(dump["max_bvh_depth"]))
        seen.add(node)
        for k in range(4):
            ref = int(refs[node, k])
            if ref == EMPTY:
                continue
            if ref >= 0:
                front.append((ref, depth + 1))
            else:
                leaf(ref)
    return records


def check_membership(dump, nodes, side, statement):
    """S5 / S6's partition.  Returns under: instance index -> sorted node ids."""
    name, inst = side[0], dump[side[1]]
    n_leaf = len(inst) - len(dump[side[3]])
    tris = dump["tris"]
    tri_node, tri_id = tris[:, 3].astype(np.int64), tris[:, 7].astype(np.int64)
    verts = tris[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]].view(np.float32)
    owner = {}                                       # scene node -> instance
    under = {}
    for k in range(n_leaf):
        i = inst[k]
        kind, nid = int(i["kind"]), int(i["node_id"])
        where = "%s instance %d" % (name, k)
        if kind != TRIMESH:
            need(0 <= nid < len(nodes), statement, "%s: node_id %d of %d nodes", where, nid, len(nodes))
            n = nodes[nid]
            need(n.geometry.kind == kind and kind != PLANE, statement, "%s: kind %d, node %d is a %d", where, kind, nid, n.geometry.kind)
            need(same_bits(i["params"], n.geometry.params), statement, "%s: params %s, node %d has %s", where, i["params"], nid, n.geometry.params)
            need(same_bits(i["trans"], n.transform.translation) and same_bits(i["rot"], rotation(n.transform.axis_angle)), statement, "%s: not the isometry of node %d", where, nid)
            need(nid not in owner, statement, "%s: node %d is also instance %d", where, nid, owner.get(nid, -1))
            owner[nid] = k; under[k] = [nid]
            continue
        recs = np.asarray(walk_blas(dump, int(i["blas_root"]), where), np.int64)
        pairs = set(zip(tri_node[recs].tolist(), tri_id[recs].tolist()))
        members = sorted(set(p[0] for p in pairs))
        for m in members:
            need(0 <= m < len(nodes) and nodes[m].geometry.kind == TRIMESH, statement, "%s: a triangle record names node %d, no mesh", where, m)
            need(m not in owner, statement, "%s: triangles of node %d are also under instance %d", where, m, owner.get(m, -1))
            owner[m] = k
            g = nodes[m].geometry
            want = set((m, t) for t in range(len(g.indices)))
            got = set(p for p in pairs if p[0] == m)
            need(got == want, statement, "%s: %d of node %d's %d triangles are reached (%d unknown ids)", where, len(got & want), m, len(want), len(got - want))
            need(same_bits(i["trans"], nodes[m].transform.translation) and same_bits(i["rot"], rotation(nodes[m].transform.axis_angle)), statement,
                 "%s: node %d has another isometry than the instance", where, m)
            need(same_bits(nodes[m].transform.axis_angle, nodes[members[0]].transform.axis_angle), statement, "%s: nodes %d and %d differ in their axis-angle", where, m, members[0])
        sel = recs
        want_v = np.stack([np.asarray(nodes[a].geometry.points, np.float64)[np.asarray(nodes[a].geometry.indices, np.int64)[b]].astype(np.float32).ravel()
                           for a, b in zip(tri_node[sel].tolist(), tri_id[sel].tolist())])
        need(np.array_equal(verts[sel].view(np.uint32), want_v.view(np.uint32)), statement, "%s: a triangle record does not hold its triangle's vertices", where)
        need((nid == -1) == (len(members) > 1), statement, "%s: node_id %d with %d nodes in the BLAS", where, nid, len(members))
        need(nid == -1 or nid == members[0], statement, "%s: node_id %d, the BLAS holds node %d", where, nid, members[0])
        under[k] = members
    for m, n in enumerate(nodes):
        k = n.geometry.kind
        inside = m in owner
        should = k != PLANE and not (k == TRIMESH and len(n.geometry.indices) == 0)
        need(inside == should, statement, "%s: node %d (kind %d) is in %s", name, m, k, "no instance" if should else "instance %d" % owner.get(m, -1))
    return under


def check_shadow_flags(dump, nodes, under_c, under_s):
    inst_c, inst_s = dump["instances"], dump["shadow_instances"]
    for k, members in under_s.items():
        i = inst_s[k]
        all_opaque = all(opaque(nodes[m]) for m in members)
        need(bool(int(i["flags"]) & INST_ANY_HIT) == all_opaque, "S6", "shadow instance %d (nodes %s): kInstAnyHit %s, the nodes are %s", k, members,
             bool(int(i["flags"]) & INST_ANY_HIT), "all opaque" if all_opaque else "not all opaque")
        for m in members:
            if nodes[m].geometry.kind == TRIMESH and not opaque(nodes[m]):
                need(members == [m] and int(i["node_id"]) == m, "S6", "shadow instance %d: the non-opaque mesh node %d shares it with %s (node_id %d)", k, m, members, int(i["node_id"]))
    for k, members in under_c.items():
        if int(inst_c[k]["kind"]) == TRIMESH and all(opaque(nodes[m]) for m in members):
            twin = [s for s, ms in under_s.items() if ms == members]
            need(len(twin) == 1 and int(inst_s[twin[0]]["blas_root"]) == int(inst_c[k]["blas_root"]), "S6",
                 "the all-opaque group %s: closest BLAS root %d, shadow %s", members, int(inst_c[k]["blas_root"]), [int(inst_s[s]["blas_root"]) for s in twin])


def check_reference_cover(dump, nodes, ref_aabbs, sides_under):
    aabbs = np.ascontiguousarray(np.asarray(dump["node_aabbs"], np.float64).reshape(-1, 6))
    ref = np.ascontiguousarray(np.asarray(ref_aabbs, np.float64).reshape(-1, 6))
    need(aabbs.shape == ref.shape == (len(nodes), 6), "S7", "%d node_aabbs, %d reference AABBs, %d nodes", len(aabbs), len(ref), len(nodes))
    # (a mesh without triangles is under no instance and is never cast; the reference has no AABB for it — ncollide's TriMesh takes it from the root of an empty BVT)
    cast = np.asarray([not (n.geometry.kind == TRIMESH and len(n.geometry.indices) == 0) for n in nodes], bool)
    diff = np.flatnonzero((aabbs.view(np.uint64) != ref.view(np.uint64)).any(axis=1) & cast)
    need(not len(diff), "S7", "node_aabbs differs from the reference's AABB at the nodes %s", diff[:5])
    worst, faces, bad = 0.0, 0, []
    for name, leaf_box, under in sides_under:
        for k, members in under.items():
            b_lo, b_hi = leaf_box[k]
            for m in members:
                gap = np.concatenate([b_lo - aabbs[m, :3], aabbs[m, 3:] - b_hi])          # > 0: the box is too tight on that face
                faces += 6
                if (gap > 0).any():
                    bad.append((name, k, m, int(np.argmax(gap)), float(gap.max())))
                    worst = max(worst, float(gap.max()))
    need(not bad, "S7", "%d of %d instance boxes do not contain their node's reference AABB (largest gap %.3g), e.g. %s instance %d node %d face %d by %.3g",
         len(bad), faces // 6, worst, *(bad[0] if bad else ("", 0, 0, 0, 0.0)))
    return faces


def check_geometry_cover(dump, nodes, sides_under):
    corners, bad = 0, []
    for name, leaf_box, under, inst in sides_under:
        for k, members in under.items():
            i = inst[k]
            ball = int(i["kind"]) == BALL
            R = [Fraction(float(v)) for v in i["rot"]]
            if ball:
                R = [Fraction(int(a == b)) for a in range(3) for b in range(3)]
            t = [Fraction(float(v)) for v in i["trans"]]
            b_lo, b_hi = ([Fraction(float(v)) for v in leaf_box[k][0]], [Fraction(float(v)) for v in leaf_box[k][1]])
            for m in members:
                c, h = local_box(int(i["kind"]), i["params"], nodes[m].geometry)
                for sx in (-1, 1):
                    for sy in (-1, 1):
                        for sz in (-1, 1):
                            p = [c[0] + sx * h[0], c[1] + sy * h[1], c[2] + sz * h[2]]
                            corners += 1
                            for a in range(3):
                                w = R[3 * a] * p[0] + R[3 * a + 1] * p[1] + R[3 * a + 2] * p[2] + t[a]
                                if not b_lo[a] <= w <= b_hi[a]:
                                    bad.append((name, k, m, sx, sy, sz, float(w), a, float(b_lo[a]), float(b_hi[a]), float(max(b_lo[a] - w, w - b_hi[a]))))
    need(not bad, "S8", "%d of %d corners of local boxes lie outside their instance's box (furthest by %.3g), e.g. %s instance %d node %d: the corner (%d, %d, %d) maps to %.17g on axis %d, "
         "outside [%.9g, %.9g] by %.3g", len(bad), corners, max([b[-1] for b in bad] or [0.0]), *(bad[0] if bad else ("", 0, 0, 0, 0, 0, 0.0, 0, 0.0, 0.0, 0.0)))
    return corners


def validate(dump, nodes, ref_aabbs, collect=False):
    """dump: dict with the arrays and scalars of NraysSceneDump (scene_cover_cases.as_dict); nodes: the scene's SceneNode list; ref_aabbs: nodes x 6, the reference's AABBs.
    Returns a report (counts of what was checked).  collect=True: the statements after S1 / S2 all run, and the report's "violations" lists the first of each that failed
    instead of raising it (what the builder before a fix is shown with)."""
    nodes = list(nodes)
    dump = dict(dump)
    dump["_boxes"] = child_boxes(dump["nodes"])
    for key in ("instances", "shadow_instances"):
        dump[key] = np.frombuffer(np.ascontiguousarray(dump[key]).tobytes(), INSTANCE)
    dump["tris"] = np.ascontiguousarray(dump["tris"]).view(np.uint32).reshape(-1, 12)
    violations = []

    def run(fn, *args):
        try:
            return fn(*args)
        except Violation as v:
            if not collect:
                raise
            violations.append(v)
            return None
    walked = [walk_tlas(dump, side) for side in SIDES]                       # S1, S2: everything below rests on them
    for side, (_, visited, _) in zip(SIDES, walked):
        run(check_nesting, dump, side, visited)
        run(check_planes, dump, nodes, side)
    under_c = run(check_membership, dump, nodes, SIDES[0], "S5")
    under_s = run(check_membership, dump, nodes, SIDES[1], "S6")
    report = dict(violations=violations, tlas_nodes=[len(v) for _, v, _ in walked], tlas_node_ids=[sorted(v) for _, v, _ in walked], tlas_depth=[d for _, _, d in walked],
                  instances=[len(dump["instances"]), len(dump["shadow_instances"])], faces=0, corners=0)
    if under_c is None or under_s is None:
        return report
    run(check_shadow_flags, dump, nodes, under_c, under_s)
    boxes = [("closest", walked[0][0], under_c), ("shadow", walked[1][0], under_s)]
    report["under"] = [under_c, under_s]
    report["faces"] = run(check_reference_cover, dump, nodes, ref_aabbs, boxes) or 0
    report["corners"] = run(check_geometry_cover, dump, nodes, [b + (dump[s[1]],) for b, s in zip(boxes, SIDES)]) or 0
    return report


def line(name, report):
    """One line for the test log."""
    bad = "; ".join(str(v) for v in report["violations"])
    return "%-12s TLAS nodes %3d + %3d  instances %3d + %3d  faces %5d  corners %5d  %s" % (name, *report["tlas_nodes"], *report["instances"], report["faces"], report["corners"],
                                                                                          bad if bad else "S1-S8 hold")
