"""Host-side mirror of the reference's scene-model surface, flattened into the C-ABI descriptors.

Same names, argument order and meaning as the reference constructors:
  Light.new            src/light.rs:16-23
  PhongMaterial.new    src/phong_material.rs:19-35;  NormalMaterial / UVMaterial  src/{normal,uv}_material.rs
  Texture2d / ImageData src/texture2d.rs:10-76
  SceneNode.new        src/scene_node.rs:22-47
  Scene.new / lights / set_background   src/scene.rs:119-145
  render               src/scene.rs:29-36
The geometry classes stand in for the ncollide3d shapes the loader constructs
(examples/loader3d.rs:601-695).  Nothing here computes pixels: `render` calls the HIP library
through the C ABI (include/nrays_abi.h) and fails loudly if it is missing.
"""
import collections
import ctypes as C
import functools
import inspect
import math

import numpy as np

from . import abi


# ----------------------------------------------------------------------------- geometry ----
class Ball:
    kind = abi.SHAPE_BALL

    def __init__(self, radius):
        self.params = (float(radius), 0.0, 0.0)


class Cuboid:
    kind = abi.SHAPE_CUBOID

    def __init__(self, half_extents):
        self.params = tuple(float(x) for x in half_extents)


class Cylinder:
    kind = abi.SHAPE_CYLINDER

    def __init__(self, half_height, radius):
        self.params = (float(half_height), float(radius), 0.0)


class Capsule:
    kind = abi.SHAPE_CAPSULE

    def __init__(self, half_height, radius):
        self.params = (float(half_height), float(radius), 0.0)


class Cone:
    kind = abi.SHAPE_CONE

    def __init__(self, half_height, radius):
        self.params = (float(half_height), float(radius), 0.0)


class Plane:
    """Plane::new(Unit::new_normalize(n)) — loader3d.rs:656 (parse_plane normalises, :863-867)."""
    kind = abi.SHAPE_PLANE

    def __init__(self, normal):
        n = np.asarray(normal, dtype=np.float64)
        n = n / np.linalg.norm(n)
        self.params = tuple(float(x) for x in n)


class TriMesh:
    """TriMesh::new(points, indices, uvs) — loader3d.rs:695."""
    kind = abi.SHAPE_TRIMESH

    def __init__(self, points, indices, uvs=None):
        self.points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        self.indices = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1, 3)
        self.uvs = None if uvs is None else np.ascontiguousarray(uvs, dtype=np.float64).reshape(-1, 2)
        if self.uvs is not None and len(self.uvs) != len(self.points):
            raise ValueError("uvs must have one entry per vertex")
        if len(self.indices) and int(self.indices.max()) >= len(self.points):
            raise ValueError("triangle index out of range")
        self.params = (0.0, 0.0, 0.0)


class Isometry3:
    """Isometry3::new(translation, axis_angle): `axis_angle` is a scaled-axis rotation in radians."""

    def __init__(self, translation=(0.0, 0.0, 0.0), axis_angle=(0.0, 0.0, 0.0)):
        self.translation = tuple(float(x) for x in translation)
        self.axis_angle = tuple(float(x) for x in axis_angle)

    @staticmethod
    def new(translation, axis_angle):
        return Isometry3(translation, axis_angle)

    @staticmethod
    def identity():
        return Isometry3()


# ----------------------------------------------------------------------------- textures ----
class ImageData:
    """RGBA texels, row 0 = bottom row (the Y flip of texture2d.rs:99-107 already applied)."""

    def __init__(self, pixels, dims=None):
        arr = np.ascontiguousarray(pixels)
        if arr.dtype == np.uint8:
            self.format = abi.TEXEL_RGBA8
        else:
            arr = np.ascontiguousarray(arr, dtype=np.float32)
            self.format = abi.TEXEL_RGBA32F
        if arr.ndim != 3 or arr.shape[2] != 4:
            raise ValueError("texels must be H x W x 4")
        if dims is not None and (int(dims[0]), int(dims[1])) != (arr.shape[1], arr.shape[0]):
            raise ValueError("dims mismatch")
        if arr.shape[0] < 1 or arr.shape[1] < 1:
            raise ValueError("empty texture")
        self.pixels = arr
        self.dims = (arr.shape[1], arr.shape[0])

    @staticmethod
    def from_image_rows(rows_top_first, opacity=False):
        """Decode of texture2d.rs:99-177 for an 8-bit image given top row first: flips Y, expands depth
        1/3/4 to RGBA with the reference's opaque / opacity conventions.  (Depth 2 multiplies two
        channels in f32 and therefore yields an RGBA32F image.)"""
        img = np.asarray(rows_top_first)
        if img.dtype != np.uint8:
            raise ValueError("8-bit image expected")
        if img.ndim == 2:
            img = img[:, :, None]
        img = img[::-1]
        h, w, d = img.shape
        if d == 2:
            r = img[:, :, 0].astype(np.float32) / np.float32(255.0)
            g = img[:, :, 1].astype(np.float32) / np.float32(255.0)
            out = np.ones((h, w, 4), dtype=np.float32)
            if opacity:
                out[:, :, 3] = g * r
            else:
                out[:, :, 0] = out[:, :, 1] = out[:, :, 2] = r * g
            return ImageData(out)
        out = np.full((h, w, 4), 255, dtype=np.uint8)
        if opacity:
            out[:, :, 3] = img[:, :, 3] if d == 4 else img[:, :, 0]
        elif d == 1:
            out[:, :, 0] = out[:, :, 1] = out[:, :, 2] = img[:, :, 0]
        else:
            out[:, :, :3] = img[:, :, :3]
        return ImageData(out)


class Interpolation:
    Bilinear = abi.INTERP_BILINEAR
    Nearest = abi.INTERP_NEAREST


class Overflow:
    Wrap = abi.OVERFLOW_WRAP
    ClampToEdges = abi.OVERFLOW_CLAMP


class Texture2d:
    def __init__(self, data, interpolation=Interpolation.Bilinear, overflow=Overflow.Wrap):
        self.data = data
        self.interpol = interpolation
        self.overflow = overflow

    @staticmethod
    def new(data, interpolation, overflow):
        return Texture2d(data, interpolation, overflow)


# ----------------------------------------------------------------------------- materials ---
class PhongMaterial:
    kind = abi.MAT_PHONG

    def __init__(self, ambiant_color, diffuse_color, specular_color, texture=None, alpha=None, shininess=100.0):
        self.ambiant_color = tuple(float(x) for x in ambiant_color)
        self.diffuse_color = tuple(float(x) for x in diffuse_color)
        self.specular_color = tuple(float(x) for x in specular_color)
        self.texture = texture
        self.alpha = alpha
        self.shininess = float(shininess)

    @staticmethod
    def new(ambiant_color, diffuse_color, specular_color, texture, alpha, shininess):
        return PhongMaterial(ambiant_color, diffuse_color, specular_color, texture, alpha, shininess)


class NormalMaterial:
    kind = abi.MAT_NORMAL
    texture = None
    alpha = None

    @staticmethod
    def new():
        return NormalMaterial()


class UVMaterial:
    kind = abi.MAT_UV
    texture = None
    alpha = None

    @staticmethod
    def new():
        return UVMaterial()


# ----------------------------------------------------------------------------- lights ------
class Light:
    def __init__(self, pos, radius, nsample, color):
        self.pos = tuple(float(x) for x in pos)
        self.radius = float(radius)
        self.racsample = int(np.sqrt(np.float32(nsample)))  # light.rs:20
        self.color = tuple(float(x) for x in color)

    @staticmethod
    def new(pos, radius, nsample, color):
        return Light(pos, radius, nsample, color)


# ----------------------------------------------------------------------------- scene node --
class SceneNode:
    def __init__(self, material, refl_mix, refl_atenuation, alpha, refr_coeff, transform, geometry, nmap=None,
                 solid=False):
        if nmap is not None:
            # scene_node.rs:60-74 is dead code in the reference (the loader always passes None).
            raise NotImplementedError("nmap is never constructed by the reference loader and is out of scope")
        self.material = material
        self.refl_mix = float(refl_mix)
        self.refl_atenuation = float(refl_atenuation)
        self.alpha = float(alpha)
        self.refr_coeff = float(refr_coeff)
        self.transform = transform
        self.geometry = geometry
        self.solid = bool(solid)

    @staticmethod
    def new(material, refl_mix, refl_atenuation, alpha, refr_coeff, transform, geometry, nmap, solid):
        return SceneNode(material, refl_mix, refl_atenuation, alpha, refr_coeff, transform, geometry, nmap, solid)


# ----------------------------------------------------------------------------- flattening --
class SceneDescriptor:
    """Owns the ctypes arrays behind an NraysSceneDesc (and keeps the numpy buffers alive)."""

    def __init__(self, nodes, lights, background):
        self._keep = []
        tex_index, textures = {}, []
        mat_index, materials = {}, []
        mesh_index, meshes = {}, []

        def tex_id(tex):
            if tex is None:
                return -1
            key = (id(tex.data), tex.interpol, tex.overflow)
            if key not in tex_index:
                t = abi.NraysTexture()
                t.width, t.height = tex.data.dims
                t.format, t.interp, t.overflow = tex.data.format, tex.interpol, tex.overflow
                t.texels = tex.data.pixels.ctypes.data
                self._keep.append(tex.data.pixels)
                tex_index[key] = len(textures)
                textures.append(t)
            return tex_index[key]

        def mat_id(mat):
            if id(mat) not in mat_index:
                m = abi.NraysMaterial()
                m.kind = mat.kind
                if mat.kind == abi.MAT_PHONG:
                    m.ambiant[:] = mat.ambiant_color
                    m.diffuse[:] = mat.diffuse_color
                    m.specular[:] = mat.specular_color
                    m.shininess = mat.shininess
                m.texture_id = tex_id(mat.texture)
                m.alpha_texture_id = tex_id(mat.alpha)
                mat_index[id(mat)] = len(materials)
                materials.append(m)
                self._keep.append(mat)
            return mat_index[id(mat)]

        def mesh_id(geom):
            if id(geom) not in mesh_index:
                m = abi.NraysMesh()
                m.num_vertices, m.num_triangles = len(geom.points), len(geom.indices)
                m.vertices = geom.points.ctypes.data_as(C.POINTER(C.c_double))
                m.uvs = geom.uvs.ctypes.data_as(C.POINTER(C.c_double)) if geom.uvs is not None else None
                m.indices = geom.indices.ctypes.data_as(C.POINTER(C.c_uint32))
                mesh_index[id(geom)] = len(meshes)
                meshes.append(m)
                self._keep.append(geom)
            return mesh_index[id(geom)]

        cnodes = (abi.NraysNode * max(1, len(nodes)))()
        for i, n in enumerate(nodes):
            c = cnodes[i]
            c.shape_kind = n.geometry.kind
            c.solid = 1 if n.solid else 0
            c.params[:] = n.geometry.params
            c.translation[:] = n.transform.translation
            c.axis_angle[:] = n.transform.axis_angle
            c.refl_mix, c.refl_atenuation, c.alpha = n.refl_mix, n.refl_atenuation, n.alpha
            c.refr_coeff = n.refr_coeff
            c.material_id = mat_id(n.material)
            c.mesh_id = mesh_id(n.geometry) if n.geometry.kind == abi.SHAPE_TRIMESH else -1
        clights = (abi.NraysLight * max(1, len(lights)))()
        for i, l in enumerate(lights):
            clights[i].pos[:] = l.pos
            clights[i].radius = l.radius
            clights[i].racsample = l.racsample
            clights[i].color[:] = l.color
        self._nodes, self._lights = cnodes, clights
        self._materials = (abi.NraysMaterial * max(1, len(materials)))(*materials)
        self._textures = (abi.NraysTexture * max(1, len(textures)))(*textures)
        self._meshes = (abi.NraysMesh * max(1, len(meshes)))(*meshes)
        d = abi.NraysSceneDesc()
        d.background[:] = tuple(float(x) for x in background)
        d.num_lights, d.lights = len(lights), self._lights
        d.num_materials, d.materials = len(materials), self._materials
        d.num_textures, d.textures = len(textures), self._textures
        d.num_meshes, d.meshes = len(meshes), self._meshes
        d.num_nodes, d.nodes = len(nodes), self._nodes
        self.desc = d

    def pointer(self):
        return C.byref(self.desc)


def _dilate_keyword(bake):
    """bake_indirect and its two methods take their arguments by position up to `unordered`, their last parameter, and callers and tests rely on that
    order (tests/test_gather_order.py).  The gutter radius `dilate` that bake_lightmap takes as an ordinary parameter is therefore added AROUND them, as a
    keyword-only option: inspect.signature() shows the positional parameters as they were, the docstring names the keyword.  dilate=0 calls the baker and
    nothing else.  Otherwise the map it returns is dilated in place by dilate_texels() on the flags of one more surface_texels() call (no optional
    output: a small fraction of the gather's time), on the same stream."""
    sig = inspect.signature(bake)

    @functools.wraps(bake)
    def with_dilate(*args, dilate=0, **kw):
        radius = _dilate_radius(dilate)
        out = bake(*args, **kw)
        if radius == 0:
            return out
        bound = sig.bind(*args, **kw)
        bound.apply_defaults()
        a, scene = bound.arguments, bound.args[0]
        flags = surface_texels(scene, a["node"], a["width"], a["height"], a["centres"], a["flip_normals"], want=(), device=a["device"]).flags
        return _bake_dilate(scene, flags, out.reshape(-1, out.shape[-1]), a["width"], a["height"], radius).reshape(out.shape)
    return with_dilate


class Scene:
    """Scene::new(nodes, lights, background) — src/scene.rs:119-133.  The device-resident scene (BVHs
    included) is created on first render on the current HIP device and reused afterwards."""

    def __init__(self, nodes, lights, background=(1.0, 1.0, 1.0)):
        self._nodes = list(nodes)
        self._lights = list(lights)
        self._background = tuple(float(x) for x in background)
        self._descriptor = None
        self._handle = None

    @staticmethod
    def new(nodes, lights, background):
        return Scene(nodes, lights, background)

    def lights(self):
        return self._lights

    def set_background(self, background):
        self._background = tuple(float(x) for x in background)
        self._release()
        self._descriptor = None

    @property
    def descriptor(self):
        if self._descriptor is None:
            self._descriptor = SceneDescriptor(self._nodes, self._lights, self._background)
        return self._descriptor

    def device_handle(self):
        if self._handle is None:
            lib = abi.load_hip_lib()
            h = C.c_void_p()
            abi.check(lib.nrays_scene_create(self.descriptor.pointer(), C.byref(h)))
            self._handle = h
        return self._handle

    def cast_rays(self, origins, dirs, max_toi=None, unordered=False, want=("normal", "uv", "prim", "flags")):
        """The closest hits of caller-supplied rays on this scene: closest_hits(self, ...)."""
        return closest_hits(self, origins, dirs, max_toi, unordered, want)

    def shade_points(self, points, normals, view_dirs, nodes, uvs=None, hit_flags=None, keys=None):
        """The direct lighting of caller-supplied surface points of this scene: shade_points(self, ...)."""
        return shade_points(self, points, normals, view_dirs, nodes, uvs, hit_flags, keys)

    def occlusion_points(self, points, normals, sample_dirs, rotations=None, bias=1e-3, max_toi=math.inf, hit_flags=None, keys=None):
        """Ambient occlusion at caller-supplied surface points of this scene: occlusion_points(self, ...)."""
        return occlusion_points(self, points, normals, sample_dirs, rotations, bias, max_toi, hit_flags, keys)

    def gather_points(self, points, normals, sample_dirs, rotations=None, bias=1e-3, energy=1.0, max_depth=0, hit_flags=None, keys=None, unordered=False):
        """The incoming light at caller-supplied surface points of this scene: gather_points(self, ...)."""
        return gather_points(self, points, normals, sample_dirs, rotations, bias, energy, max_depth, hit_flags, keys, unordered)

    def gather_sh_points(self, points, normals, sample_dirs, rotations=None, bias=1e-3, energy=1.0, max_depth=0, bands=3, hit_flags=None, keys=None, unordered=False):
        """The incoming light at caller-supplied points of this scene as spherical harmonics: gather_sh_points(self, ...)."""
        return gather_sh_points(self, points, normals, sample_dirs, rotations, bias, energy, max_depth, bands, hit_flags, keys, unordered)

    def gather_probes(self, positions, sample_dirs, bands=3, energy=1.0, max_depth=0, keys=None, unordered=True):
        """Irradiance probes at free points of this scene: gather_probes(self, ...)."""
        return gather_probes(self, positions, sample_dirs, bands, energy, max_depth, keys, unordered)

    @_dilate_keyword
    def bake_indirect(self, node, width, height, sample_dirs, rotations=None, bias=1e-3, energy=1.0, max_depth=0, centres=False, flip_normals=False, keys=None,
                      device=None, unordered=False):
        """The indirect term of a light map of mesh node `node`: bake_indirect(self, node, ...); `dilate=` as there, by keyword."""
        return bake_indirect(self, node, width, height, sample_dirs, rotations, bias, energy, max_depth, centres, flip_normals, keys, device, unordered)

    def gather_maps_points(self, points, normals, sample_dirs, maps, node_map, rotations=None, bias=1e-3, max_toi=math.inf, miss=(0.0, 0.0, 0.0), hit_flags=None,
                           keys=None, want_counts=False):
        """The light of baked maps at the closest hits of the hemisphere rays of caller-supplied points of this scene: gather_maps_points(self, ...)."""
        return gather_maps_points(self, points, normals, sample_dirs, maps, node_map, rotations, bias, max_toi, miss, hit_flags, keys, want_counts)

    def bake_bounces(self, node, width, height, sample_dirs, bounces, albedo, rotations=None, bias=1e-3, miss=(0.0, 0.0, 0.0), dilate=2, flip_normals=False, keys=None,
                     device=None):
        """The multi-bounce light map of mesh node `node`: bake_bounces(self, node, ...)."""
        return bake_bounces(self, node, width, height, sample_dirs, bounces, albedo, rotations, bias, miss, dilate, flip_normals, keys, device)

    def surface_texels(self, node, width, height, centres=False, flip_normals=False, want=("normals", "uv", "node", "prim"), device=None):
        """The surface of mesh node `node` at a light map's texels: surface_texels(self, node, ...)."""
        return surface_texels(self, node, width, height, centres, flip_normals, want, device)

    def bake_lightmap(self, node, width, height, occlusion=None, centres=False, flip_normals=False, keys=None, device=None, dilate=0):
        """A light map of mesh node `node`: bake_lightmap(self, node, ...)."""
        return bake_lightmap(self, node, width, height, occlusion, centres, flip_normals, keys, device, dilate)

    def dilate_texels(self, flags, width, height, radius, values=None, want_source=False, device=None):
        """Gutter dilation of a light map on this scene's GPU: dilate_texels(self, flags, ...)."""
        return dilate_texels(self, flags, width, height, radius, values, want_source, device)

    def filter_texels(self, flags, width, height, points, normals, values, step=1, pos_radius=math.inf, normal_cos=0.0, device=None):
        """One pass of the edge-aware light-map filter on this scene's GPU: filter_texels(self, flags, ...)."""
        return filter_texels(self, flags, width, height, points, normals, values, step, pos_radius, normal_cos, device)

    def denoise_texels(self, tx, values, passes=3, pos_radius=math.inf, normal_cos=0.0, width=None, height=None):
        """A baked light map denoised on this scene's GPU: denoise_texels(self, tx, values, ...)."""
        return denoise_texels(self, tx, values, passes, pos_radius, normal_cos, width, height)

    def _release(self):
        if self._handle is not None:
            abi.load_hip_lib().nrays_scene_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass


def make_params(resolution, ray_per_pixel, window_width, camera_eye, projection, max_depth=0, seed=0,
                band_rows=0, band_owner=0, band_owners=1):
    """Packs the arguments of scene::render (src/scene.rs:29-36) into NraysRenderParams."""
    from .math3d import column_major16
    p = abi.NraysRenderParams()
    p.width, p.height = int(resolution[0]), int(resolution[1])
    p.ray_per_pixel = int(ray_per_pixel)
    p.max_depth = int(max_depth)
    p.window_width = float(window_width)
    p.camera_eye[:] = tuple(float(x) for x in camera_eye)
    p.inv_proj_view[:] = tuple(column_major16(projection))
    p.seed = int(seed)
    p.band_rows, p.band_owner, p.band_owners = int(band_rows), int(band_owner), int(band_owners)
    return p


def render(scene, resolution, ray_per_pixel, window_width, camera_eye, projection, max_depth=0, seed=0):
    """scene::render (src/scene.rs:29-116): returns the image as an (H, W, 3) float32 array, row 0 = top.
    Blocking; pixels are computed by the HIP kernels behind nrays_render."""
    if ray_per_pixel <= 0:
        raise ValueError("ray_per_pixel must be > 0")  # assert!(ray_per_pixel > 0), scene.rs:37
    lib = abi.load_hip_lib()
    p = make_params(resolution, ray_per_pixel, window_width, camera_eye, projection, max_depth, seed)
    out = np.empty((p.height, p.width, 3), dtype=np.float32)
    abi.check(lib.nrays_render(scene.device_handle(), C.byref(p), out.ctypes.data_as(C.POINTER(C.c_float))))
    return out


def cast_rays(scene, origins, dirs):
    """The closest-hit query of Scene::trace (src/scene.rs:164-166) on caller-supplied rays, by the HIP traversal and
    intersectors alone (nrays_debug_cast_batch).  Returns (hit mask, (n, 8) array of toi, nx, ny, nz, has_uv, u, v, node) —
    the layout of oracle.cast."""
    o = np.ascontiguousarray(origins, dtype=np.float64).reshape(-1, 3)
    d = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
    n = len(o)
    res = (abi.NraysCastResult * max(n, 1))()
    abi.check(abi.load_hip_lib().nrays_debug_cast_batch(scene.device_handle(), 0, n, o.ctypes.data_as(C.POINTER(C.c_double)),
                                                        d.ctypes.data_as(C.POINTER(C.c_double)), None, res))
    out = np.zeros((n, 8), dtype=np.float64)
    hit = np.zeros(n, dtype=bool)
    for i in range(n):
        r = res[i]
        hit[i] = bool(r.flags & 1)
        out[i] = (r.toi, r.normal[0], r.normal[1], r.normal[2], 1.0 if r.flags & 2 else 0.0, r.uv[0], r.uv[1], r.node_id)
    return hit, out


def shadow_rays(scene, origins, dirs, max_toi):
    """Scene::intersects_ray (src/scene.rs:147-161) on caller-supplied rays by the HIP shadow traversal: returns
    (blocked mask, (n, 3) colour filters)."""
    o = np.ascontiguousarray(origins, dtype=np.float64).reshape(-1, 3)
    d = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
    t = np.ascontiguousarray(max_toi, dtype=np.float64).reshape(-1)
    n = len(o)
    res = (abi.NraysCastResult * max(n, 1))()
    abi.check(abi.load_hip_lib().nrays_debug_cast_batch(scene.device_handle(), 1, n, o.ctypes.data_as(C.POINTER(C.c_double)),
                                                        d.ctypes.data_as(C.POINTER(C.c_double)), t.ctypes.data_as(C.POINTER(C.c_double)), res))
    blocked = np.array([bool(res[i].flags & 1) for i in range(n)])
    filt = np.array([[res[i].normal[0], res[i].normal[1], res[i].normal[2]] for i in range(n)], dtype=np.float64).reshape(n, 3)
    return blocked, filt


def get_stats(scene):
    st = abi.NraysStats()
    abi.check(abi.load_hip_lib().nrays_get_stats(scene.device_handle(), C.byref(st)))
    return st


def last_permutation(scene):
    """Test probe (nrays_debug_last_permutation): the k_primary permutation the handle's most recent render launched, as
    ((stats, feat, plain, occ), launches, mixed) — the template arguments of csrc/primary_kernel.h: NR_PRIMARY_PERMUTATIONS."""
    out = (C.c_uint32 * 6)()
    abi.check(abi.load_hip_lib().nrays_debug_last_permutation(scene.device_handle(), out))
    return (bool(out[0]), int(out[1]), bool(out[2]), int(out[3])), int(out[4]), bool(out[5])


# ---- caller-supplied rays: Scene::trace / Scene::intersects_ray (src/scene.rs:147-193) in batches ----------------------------------------

def _is_tensor(x):
    return type(x).__module__.split(".")[0] == "torch"


def _n_of(origins, dirs, names=("origins", "dirs")):
    """Number of rays of an (n, 3) origins / directions pair (numpy arrays or torch tensors), checked before any device work."""
    for name, a in zip(names, (origins, dirs)):
        if a is None:
            raise ValueError("%s is required" % name)
        if len(a.shape) != 2 or a.shape[1] != 3:
            raise ValueError("%s must have shape (n, 3), got %s" % (name, tuple(a.shape)))
    if origins.shape[0] != dirs.shape[0]:
        raise ValueError("%s and %s hold %d and %d rays" % (names[0], names[1], origins.shape[0], dirs.shape[0]))
    n = int(origins.shape[0])
    if n >= 1 << 32:
        raise ValueError("at most 2^32 - 1 rays per call")
    return n


def _check_vec(name, a, n):
    if a is not None and (len(a.shape) != 1 or a.shape[0] != n):
        raise ValueError("%s must have shape (%d,), got %s" % (name, n, tuple(a.shape)))


def _np_floats(name, a, dtype):
    a = np.asarray(a)
    if not np.issubdtype(a.dtype, np.floating):
        raise ValueError("%s must be floating point, got %s" % (name, a.dtype))
    return np.ascontiguousarray(a, dtype=dtype)


def _np_keys(keys):
    k = np.asarray(keys)
    if not np.issubdtype(k.dtype, np.integer):
        raise ValueError("keys must be integers, got %s" % k.dtype)
    return np.ascontiguousarray(k.astype(np.uint64, copy=False))


def _torch_args(named, device):
    """Checks dtypes and the device of torch arguments: (name, tensor or None, allowed dtypes) -> contiguous tensors."""
    out = []
    for name, t, dtypes in named:
        if t is None:
            out.append(None)
            continue
        if not _is_tensor(t):
            raise ValueError("%s: torch tensors and numpy arrays cannot be mixed in one call" % name)
        if t.dtype not in dtypes:
            raise ValueError("%s must be %s, got %s" % (name, " or ".join(str(d) for d in dtypes), t.dtype))
        if t.device != device:
            raise ValueError("%s is on %s, origins on %s" % (name, t.device, device))
        out.append(t.contiguous())
    return out


def trace_rays(scene, origins, dirs, refr=None, energy=None, keys=None, max_depth=0, unordered=False):
    """Scene::trace (src/scene.rs:163-193) on n caller-supplied rays: the colour of each, with the reflection / refraction recursion
    and the lights of a render.  `origins`, `dirs`: (n, 3); `refr` (n,) refraction index of the medium the ray is in (default 1.0),
    `energy` (n,) (default 1.0), `keys` (n,) RNG path keys for area-light sampling (default: ray i has key i); directions are used as
    given (unit length expected).  `max_depth` as in render().
    `unordered=True` (NRAYS_RAYS_UNORDERED) says that the rays come in no useful order — AO / baking rays, shuffled or gathered rays: the
    library may then bin them by a spatial key and trace them in that order.  The colours are bit-identical either way; only the time changes.
    numpy arrays -> nrays_trace_rays (blocking), (n, 3) float32 numpy array.  torch tensors on the scene's GPU (float64, energy float32,
    keys int64 / uint64) -> nrays_trace_rays_device on torch.cuda.current_stream(), (n, 3) float32 tensor."""
    n = _n_of(origins, dirs)
    for name, a in (("refr", refr), ("energy", energy), ("keys", keys)):
        _check_vec(name, a, n)
    if int(max_depth) < 0 or int(max_depth) >= 1 << 32:
        raise ValueError("max_depth must be in [0, 2^32)")
    lib = abi.load_hip_lib()
    if _is_tensor(origins):
        import torch
        if origins.device.type != "cuda":
            raise ValueError("torch tensors must be on the GPU, origins is on %s" % origins.device)
        keys_dt = tuple(d for d in (torch.int64, getattr(torch, "uint64", None)) if d is not None)
        o, d, r, e, k = _torch_args((("origins", origins, (torch.float64,)), ("dirs", dirs, (torch.float64,)), ("refr", refr, (torch.float64,)),
                                     ("energy", energy, (torch.float32,)), ("keys", keys, keys_dt)), origins.device)
        out = torch.empty((n, 3), dtype=torch.float32, device=origins.device)
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        with torch.cuda.device(origins.device):
            stream = torch.cuda.current_stream().cuda_stream
            if unordered:
                abi.check(lib.nrays_trace_rays_device_ex(scene.device_handle(), n, ptr(o), ptr(d), ptr(r), ptr(e), ptr(k), int(max_depth), ptr(out),
                                                         abi.RAYS_UNORDERED, stream))
            else:
                abi.check(lib.nrays_trace_rays_device(scene.device_handle(), n, ptr(o), ptr(d), ptr(r), ptr(e), ptr(k), int(max_depth), ptr(out), stream))
        return out
    if any(_is_tensor(a) for a in (dirs, refr, energy, keys)):
        raise ValueError("torch tensors and numpy arrays cannot be mixed in one call")
    o, d = _np_floats("origins", origins, np.float64), _np_floats("dirs", dirs, np.float64)
    r = None if refr is None else _np_floats("refr", refr, np.float64)
    e = None if energy is None else _np_floats("energy", energy, np.float32)
    k = None if keys is None else _np_keys(keys)
    out = np.empty((n, 3), dtype=np.float32)
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    if unordered:
        abi.check(lib.nrays_trace_rays_ex(scene.device_handle(), n, ptr(o, C.c_double), ptr(d, C.c_double), ptr(r, C.c_double), ptr(e, C.c_float),
                                          ptr(k, C.c_uint64), int(max_depth), ptr(out, C.c_float), abi.RAYS_UNORDERED))
    else:
        abi.check(lib.nrays_trace_rays(scene.device_handle(), n, ptr(o, C.c_double), ptr(d, C.c_double), ptr(r, C.c_double), ptr(e, C.c_float),
                                       ptr(k, C.c_uint64), int(max_depth), ptr(out, C.c_float)))
    return out


def intersects_rays(scene, origins, dirs, max_toi, unordered=False):
    """Scene::intersects_ray (src/scene.rs:147-161) on n caller-supplied rays, through nrays_intersects_rays_device: returns
    (lit mask, (n, 3) float32 colour filters) — lit where the reference returns Some(filter); the filter is (0, 0, 0) elsewhere.
    numpy arrays in -> numpy out (blocking); torch tensors on the GPU (float64) -> tensors (bool, float32) on torch.cuda.current_stream().
    `unordered=True`: as for trace_rays (nrays_intersects_rays_device_ex with NRAYS_RAYS_UNORDERED); the results are bit-identical."""
    n = _n_of(origins, dirs)
    _check_vec("max_toi", max_toi, n)
    lib = abi.load_hip_lib()
    import torch
    if _is_tensor(origins):
        if origins.device.type != "cuda":
            raise ValueError("torch tensors must be on the GPU, origins is on %s" % origins.device)
        o, d, t = _torch_args((("origins", origins, (torch.float64,)), ("dirs", dirs, (torch.float64,)), ("max_toi", max_toi, (torch.float64,))), origins.device)
        device, host = origins.device, False
    else:
        if any(_is_tensor(a) for a in (dirs, max_toi)):
            raise ValueError("torch tensors and numpy arrays cannot be mixed in one call")
        on = _np_floats("origins", origins, np.float64)
        dn, tn = _np_floats("dirs", dirs, np.float64), _np_floats("max_toi", max_toi, np.float64)
        device, host = torch.device("cuda", torch.cuda.current_device()), True
        o, d, t = (torch.from_numpy(a).to(device) for a in (on, dn, tn))
    filt = torch.empty((n, 3), dtype=torch.float32, device=device)
    lit = torch.empty((n,), dtype=torch.int32, device=device)
    with torch.cuda.device(device):
        stream = torch.cuda.current_stream().cuda_stream
        if unordered:
            abi.check(lib.nrays_intersects_rays_device_ex(scene.device_handle(), n, o.data_ptr(), d.data_ptr(), t.data_ptr(), filt.data_ptr(), lit.data_ptr(),
                                                          abi.RAYS_UNORDERED, stream))
        else:
            abi.check(lib.nrays_intersects_rays_device(scene.device_handle(), n, o.data_ptr(), d.data_ptr(), t.data_ptr(), filt.data_ptr(), lit.data_ptr(), stream))
    if host:
        return lit.cpu().numpy() != 0, filt.cpu().numpy()
    return lit != 0, filt


CAST_OUTPUTS = ("normal", "uv", "prim", "flags")  # the optional outputs of closest_hits, in the order of nrays_cast_rays_device's arguments
CastHits = collections.namedtuple("CastHits", ("toi", "node") + CAST_OUTPUTS)


def closest_hits(scene, origins, dirs, max_toi=None, unordered=False, want=CAST_OUTPUTS):
    """Scene::trace's closest-hit query (src/scene.rs:164-166, 262-283) with SceneNode::cast's record on n caller-supplied rays, through
    nrays_cast_rays_device / nrays_cast_rays: WHICH node each ray meets first, where, with which normal and uv (picking, depth / normal / id
    passes, the first hop of a baker).  Also `scene.cast_rays(origins, dirs, ...)` on Scene and FileScene.  (The module-level `cast_rays`
    is the older wrapper of the test probe nrays_debug_cast_batch.)
    `origins`, `dirs`: (n, 3), directions used as given; `max_toi` (n,) or None: the unbounded answer where its toi <= max_toi[i], a miss
    otherwise (NaN: a miss).  `unordered=True`: as for trace_rays; the results are bit-identical.  `want`: which of "normal", "uv", "prim",
    "flags" to compute into memory.
    Returns CastHits(toi (n,) f64, node (n,) i32, normal (n, 3) f64, uv (n, 2) f64, prim (n,) i32, flags (n,)), None for what was not wanted.
    A miss has node -1, toi +inf, zeros, prim -1, flags 0; flags bit 0 = hit, bit 1 = the record carries uvs; prim = the triangle's index in
    its mesh, -1 for an analytic shape.
    numpy arrays -> nrays_cast_rays (blocking), numpy arrays (flags uint32).  torch tensors on the scene's GPU (float64) ->
    nrays_cast_rays_device on torch.cuda.current_stream(), tensors (flags int32)."""
    n = _n_of(origins, dirs)
    _check_vec("max_toi", max_toi, n)
    want = tuple(want)
    for name in want:
        if name not in CAST_OUTPUTS:
            raise ValueError("want: unknown output %r (one of %s)" % (name, ", ".join(CAST_OUTPUTS)))
    flags = abi.RAYS_UNORDERED if unordered else 0
    shapes = {"toi": (n,), "node": (n,), "normal": (n, 3), "uv": (n, 2), "prim": (n,), "flags": (n,)}
    if _is_tensor(origins):
        import torch
        if origins.device.type != "cuda":
            raise ValueError("torch tensors must be on the GPU, origins is on %s" % origins.device)
        o, d, t = _torch_args((("origins", origins, (torch.float64,)), ("dirs", dirs, (torch.float64,)), ("max_toi", max_toi, (torch.float64,))), origins.device)
        dtypes = {"toi": torch.float64, "node": torch.int32, "normal": torch.float64, "uv": torch.float64, "prim": torch.int32, "flags": torch.int32}
        out = {k: torch.empty(shapes[k], dtype=dtypes[k], device=origins.device) if k in ("toi", "node") or k in want else None for k in CastHits._fields}
        ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
        lib = abi.load_hip_lib()
        with torch.cuda.device(origins.device):
            abi.check(lib.nrays_cast_rays_device(scene.device_handle(), n, ptr(o), ptr(d), ptr(t), *[ptr(out[k]) for k in CastHits._fields], flags,
                                                 torch.cuda.current_stream().cuda_stream))
        return CastHits(**out)
    if any(_is_tensor(a) for a in (dirs, max_toi)):
        raise ValueError("torch tensors and numpy arrays cannot be mixed in one call")
    o, d = _np_floats("origins", origins, np.float64), _np_floats("dirs", dirs, np.float64)
    t = None if max_toi is None else _np_floats("max_toi", max_toi, np.float64)
    dtypes = {"toi": np.float64, "node": np.int32, "normal": np.float64, "uv": np.float64, "prim": np.int32, "flags": np.uint32}
    ctypes_of = {np.float64: C.c_double, np.int32: C.c_int32, np.uint32: C.c_uint32}
    out = {k: np.empty(shapes[k], dtype=dtypes[k]) if k in ("toi", "node") or k in want else None for k in CastHits._fields}
    ptr = lambda a, ct: None if a is None else a.ctypes.data_as(C.POINTER(ct))  # noqa: E731
    lib = abi.load_hip_lib()
    abi.check(lib.nrays_cast_rays(scene.device_handle(), n, ptr(o, C.c_double), ptr(d, C.c_double), ptr(t, C.c_double),
                                  *[ptr(out[k], ctypes_of[dtypes[k]]) for k in CastHits._fields], flags))
    return CastHits(**out)


def _check_rows(name, a, n, cols):
    if len(a.shape) != 2 or a.shape[0] != n or a.shape[1] != cols:
        raise ValueError("%s must have shape (%d, %d), got %s" % (name, n, cols, tuple(a.shape)))


def _np_ints(name, a, dtype):
    """An integer numpy array as `dtype`: int32 keeps out-of-range node indices out of range (clipped), uint32 keeps the low 32 bits (flag words)."""
    a = np.asarray(a)
    if not np.issubdtype(a.dtype, np.integer):
        raise ValueError("%s must be integers, got %s" % (name, a.dtype))
    if dtype == np.int32 and a.dtype != np.int32:
        a = np.clip(a, -(1 << 31), (1 << 31) - 1)
    return np.ascontiguousarray(a.astype(dtype, copy=False))


def shade_points(scene, points, normals, view_dirs, nodes, uvs=None, hit_flags=None, keys=None):
    """Material::compute (src/material.rs:8-16, src/phong_material.rs:72-151) on n caller-supplied surface points, through
    nrays_shade_points_device / nrays_shade_points: the direct lighting of each point with the material of scene node nodes[i] — ambient term,
    texture and opacity map, the lights' samples with one transparent-shadow query each, Phong — without a closest-hit traversal and without
    reflection or refraction.  Also `scene.shade_points(...)` on Scene and FileScene; shade_hits() feeds it from closest_hits().
    `points`, `normals`, `view_dirs`: (n, 3), used as given (unit normals; view_dirs = the direction the viewer looks along, towards the surface:
    it feeds the specular term).  `nodes` (n,) integers: the node only selects the material; its alpha / refl_mix / refr_coeff are not applied.
    `uvs` (n, 2) or None (no point has a uv).  `hit_flags` (n,) integers or None: the flag words of closest_hits — bit 0 clear: the point is
    skipped, bit 1: it carries a uv; None: every point is shaded and has a uv exactly when `uvs` is given.  `keys` (n,) RNG path keys for
    area-light sampling (default: point i has key i), hashed as for a traced ray with the same key.
    Returns (n, 4) float32: the lit colour and the material's alpha (the opacity-map sample, or 1).  A skipped point — flag bit 0 clear, node
    < 0 or >= the scene's node count — is (0, 0, 0, 0), so the result of closest_hits can be passed on unfiltered.
    numpy arrays -> nrays_shade_points (blocking), numpy array.  torch tensors on the scene's GPU (float64; nodes int32; hit_flags int32 /
    uint32; keys int64 / uint64) -> nrays_shade_points_device on torch.cuda.current_stream(), tensor."""
    n = _n_of(points, normals, ("points", "normals"))
    for name, a in (("view_dirs", view_dirs), ("nodes", nodes)):
        if a is None:
            raise ValueError("%s is required" % name)
    _check_rows("view_dirs", view_dirs, n, 3)
    if uvs is not None:
        _check_rows("uvs", uvs, n, 2)
    for name, a in (("nodes", nodes), ("hit_flags", hit_flags), ("keys", keys)):
        _check_vec(name, a, n)
    if _is_tensor(points):
        import torch
        if points.device.type != "cuda":
            raise ValueError("torch tensors must be on the GPU, points is on %s" % points.device)
        f64 = (torch.float64,)
        keys_dt = tuple(d for d in (torch.int64, getattr(torch, "uint64", None)) if d is not None)
        flags_dt = tuple(d for d in (torch.int32, getattr(torch, "uint32", None)) if d is not None)
        p, nm, v, uv, nd, hf, k = _torch_args((("points", points, f64), ("normals", normals, f64), ("view_dirs", view_dirs, f64), ("uvs", uvs, f64),
                                               ("nodes", nodes, (torch.int32,)), ("hit_flags", hit_flags, flags_dt), ("keys", keys, keys_dt)), points.device)
        out = torch.empty((n, 4), dtype=torch.float32, device=points.device)
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        lib = abi.load_hip_lib()
        with torch.cuda.device(points.device):
            abi.check(lib.nrays_shade_points_device(scene.device_handle(), n, ptr(p), ptr(nm), ptr(v), ptr(uv), ptr(nd), ptr(hf), ptr(k), ptr(out), 0,
                                                    torch.cuda.current_stream().cuda_stream))
        return out
    if any(_is_tensor(a) for a in (normals, view_dirs, nodes, uvs, hit_flags, keys)):
        raise ValueError("torch tensors and numpy arrays cannot be mixed in one call")
    p, nm, v = _np_floats("points", points, np.float64), _np_floats("normals", normals, np.float64), _np_floats("view_dirs", view_dirs, np.float64)
    uv = None if uvs is None else _np_floats("uvs", uvs, np.float64)
    nd = _np_ints("nodes", nodes, np.int32)
    hf = None if hit_flags is None else _np_ints("hit_flags", hit_flags, np.uint32)
    k = None if keys is None else _np_keys(keys)
    out = np.empty((n, 4), dtype=np.float32)
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    lib = abi.load_hip_lib()
    abi.check(lib.nrays_shade_points(scene.device_handle(), n, ptr(p, C.c_double), ptr(nm, C.c_double), ptr(v, C.c_double), ptr(uv, C.c_double),
                                     ptr(nd, C.c_int32), ptr(hf, C.c_uint32), ptr(k, C.c_uint64), ptr(out, C.c_float), 0))
    return out


def shade_hits(scene, origins, dirs, hits, keys=None):
    """The direct lighting of the closest hits of caller-supplied rays: shade_points() at the hits of `hits = closest_hits(scene, origins, dirs)`
    (a CastHits with normal, uv and flags), viewed along the rays.  The points are origins + dirs * toi — two separate element-wise operations,
    the unfused `ray.o + ray.d * toi` of Scene::trace, with toi 0 at the misses — so that on a node that neither reflects nor refracts the colour
    is trace_rays()'s, bit for bit.  Misses come back as (0, 0, 0, 0).  `keys` as for trace_rays.  (n, 4) float32, numpy or torch as the inputs."""
    n = _n_of(origins, dirs)
    for name in ("normal", "uv", "flags"):
        if getattr(hits, name) is None:
            raise ValueError("shade_hits: hits.%s is None (closest_hits must be asked for normal, uv and flags)" % name)
    _check_vec("hits.toi", hits.toi, n)
    if _is_tensor(origins) != _is_tensor(hits.toi):
        raise ValueError("torch tensors and numpy arrays cannot be mixed in one call")
    if _is_tensor(origins):
        import torch
        toi = torch.where((hits.flags & 1) != 0, hits.toi, torch.zeros_like(hits.toi))
    else:
        toi = np.where((np.asarray(hits.flags) & 1) != 0, hits.toi, 0.0)
    step = dirs * toi[:, None]
    points = origins + step
    return shade_points(scene, points, hits.normal, dirs, hits.node, uvs=hits.uv, hit_flags=hits.flags, keys=keys)


# ---- ambient occlusion at caller-supplied points: the hemisphere rays are built on the device (include/nrays_abi.h: NraysOcclusionParams) ----------

Occlusion = collections.namedtuple("Occlusion", ("filter", "open"))
SALT_OCCLUSION = 0x300 << 32  # kSaltOcclusion (csrc/trace_device.h)
OCCLUSION_MAX_TABLE = 1024


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


def _occlusion_tables(sample_dirs, rotations, bias, max_toi):
    """The two tables as contiguous float64 numpy arrays (or the torch tensors they came as), checked against NraysOcclusionParams' bounds."""
    def table(name, a, cols, lo):
        if not _is_tensor(a):
            a = np.asarray(a)
            if not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
                raise ValueError("%s must be numbers, got %s" % (name, a.dtype))
            a = np.ascontiguousarray(a, dtype=np.float64)
        if len(a.shape) != 2 or a.shape[1] != cols or not lo <= a.shape[0] <= OCCLUSION_MAX_TABLE:
            raise ValueError("%s must have shape (%d .. %d, %d), got %s" % (name, lo, OCCLUSION_MAX_TABLE, cols, tuple(a.shape)))
        return a
    if sample_dirs is None:
        raise ValueError("sample_dirs is required")
    L = table("sample_dirs", sample_dirs, 3, 1)
    rot = None if rotations is None else table("rotations", rotations, 2, 0)
    if rot is not None and rot.shape[0] == 0:
        rot = None
    bias, max_toi = float(bias), float(max_toi)
    if not math.isfinite(bias):
        raise ValueError("bias must be finite")
    if not max_toi > 0.0:
        raise ValueError("max_toi must be > 0 (inf allowed)")
    return L, rot, bias, max_toi


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


def occlusion_ray_probe(scene, points, normals, sample_dirs, rotations=None, bias=1e-3, keys=None):
    """Test probe (nrays_debug_occlusion_rays): the rays as the library's own generator — the device function k_occlusion_points traces — builds them,
    in occlusion_rays()' layout.  numpy arrays, blocking."""
    n = _n_of(points, normals, ("points", "normals"))
    _check_vec("keys", keys, n)
    L, rot, bias, _ = _occlusion_tables(sample_dirs, rotations, bias, math.inf)
    p, nm = _np_floats("points", points, np.float64), _np_floats("normals", normals, np.float64)
    k = None if keys is None else _np_keys(keys)
    o, d = np.empty((n, len(L), 3), np.float64), np.empty((n, len(L), 3), np.float64)
    params = abi.NraysOcclusionParams(len(L), 0 if rot is None else len(rot), L.ctypes.data, None if rot is None else rot.ctypes.data, bias, math.inf)
    dp = C.POINTER(C.c_double)
    abi.check(abi.load_hip_lib().nrays_debug_occlusion_rays(scene.device_handle(), n, p.ctypes.data_as(dp), nm.ctypes.data_as(dp),
                                                            None if k is None else k.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(params),
                                                            o.ctypes.data_as(dp), d.ctypes.data_as(dp)))
    return o, d


def occlusion_points(scene, points, normals, sample_dirs, rotations=None, bias=1e-3, max_toi=math.inf, hit_flags=None, keys=None):
    """Ambient occlusion at n caller-supplied surface points, through nrays_occlusion_points_device / nrays_occlusion_points: per point the library
    builds len(sample_dirs) hemisphere rays ON THE DEVICE (occlusion_rays() restates them bit for bit), runs Scene::intersects_ray — the query of
    intersects_rays() — with `max_toi` on each and folds them in order: Occlusion(filter (n, 3) float32 — the mean colour filter, a blocked ray counting as
    black —, open (n,) — the rays that got through).  No ray or per-ray result is ever in memory.  Also `scene.occlusion_points(...)` on Scene and FileScene;
    occlusion_hits() feeds it from closest_hits().
    `points`, `normals`: (n, 3), used as given (unit normals, pointing to the side to sample).  `sample_dirs` (k, 3), 1 <= k <= 1024: directions of the local
    frame whose z axis is the normal (hemisphere_dirs()).  `rotations` (R, 2) (cos, sin) pairs, R <= 1024, or None: point i turns its directions about the
    normal by entry hash(keys[i]) % R (rotation_table()).  `bias`: the rays start at point + normal * bias.  `hit_flags` (n,) integers or None: the flag words
    of closest_hits — bit 0 clear: the point is skipped (zeros; its point and normal may hold anything).  `keys` (n,) integers, default: point i has key i.
    numpy arrays -> nrays_occlusion_points (blocking), numpy arrays (open uint32).  torch tensors on the scene's GPU (float64; hit_flags int32 / uint32; keys
    int64 / uint64; the tables tensors or anything numpy takes) -> nrays_occlusion_points_device on torch.cuda.current_stream(), tensors (open int32)."""
    n = _n_of(points, normals, ("points", "normals"))
    for name, a in (("hit_flags", hit_flags), ("keys", keys)):
        _check_vec(name, a, n)
    L, rot, bias, max_toi = _occlusion_tables(sample_dirs, rotations, bias, max_toi)
    if _is_tensor(points):
        import torch
        if points.device.type != "cuda":
            raise ValueError("torch tensors must be on the GPU, points is on %s" % points.device)
        f64 = (torch.float64,)
        keys_dt = tuple(d for d in (torch.int64, getattr(torch, "uint64", None)) if d is not None)
        flags_dt = tuple(d for d in (torch.int32, getattr(torch, "uint32", None)) if d is not None)
        L, rot = (t if t is None or _is_tensor(t) else torch.from_numpy(t).to(points.device) for t in (L, rot))
        p, nm, hf, k, L, rot = _torch_args((("points", points, f64), ("normals", normals, f64), ("hit_flags", hit_flags, flags_dt), ("keys", keys, keys_dt),
                                            ("sample_dirs", L, f64), ("rotations", rot, f64)), points.device)
        filt = torch.empty((n, 3), dtype=torch.float32, device=points.device)
        opened = torch.empty((n,), dtype=torch.int32, device=points.device)
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        params = abi.NraysOcclusionParams(L.shape[0], 0 if rot is None else rot.shape[0], ptr(L), ptr(rot), bias, max_toi)
        lib = abi.load_hip_lib()
        with torch.cuda.device(points.device):
            abi.check(lib.nrays_occlusion_points_device(scene.device_handle(), n, ptr(p), ptr(nm), ptr(hf), ptr(k), C.byref(params), ptr(filt), ptr(opened), 0,
                                                        torch.cuda.current_stream().cuda_stream))
        return Occlusion(filt, opened)
    if any(_is_tensor(a) for a in (normals, hit_flags, keys, L, rot)):
        raise ValueError("torch tensors and numpy arrays cannot be mixed in one call")
    p, nm = _np_floats("points", points, np.float64), _np_floats("normals", normals, np.float64)
    hf = None if hit_flags is None else _np_ints("hit_flags", hit_flags, np.uint32)
    k = None if keys is None else _np_keys(keys)
    filt, opened = np.empty((n, 3), dtype=np.float32), np.empty((n,), dtype=np.uint32)
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    params = abi.NraysOcclusionParams(len(L), 0 if rot is None else len(rot), L.ctypes.data, None if rot is None else rot.ctypes.data, bias, max_toi)
    lib = abi.load_hip_lib()
    abi.check(lib.nrays_occlusion_points(scene.device_handle(), n, ptr(p, C.c_double), ptr(nm, C.c_double), ptr(hf, C.c_uint32), ptr(k, C.c_uint64), C.byref(params),
                                         ptr(filt, C.c_float), ptr(opened, C.c_uint32), 0))
    return Occlusion(filt, opened)


def _hit_points(name, origins, dirs, hits):
    """The surface points and the normals facing the rays of `hits = closest_hits(scene, origins, dirs)`, as occlusion_hits() builds them."""
    n = _n_of(origins, dirs)
    for field in ("normal", "flags"):
        if getattr(hits, field) is None:
            raise ValueError("%s: hits.%s is None (closest_hits must be asked for normal and flags)" % (name, field))
    _check_vec("hits.toi", hits.toi, n)
    _check_rows("hits.normal", hits.normal, n, 3)
    if _is_tensor(origins) != _is_tensor(hits.toi) or _is_tensor(origins) != _is_tensor(dirs) or _is_tensor(origins) != _is_tensor(hits.normal):
        raise ValueError("torch tensors and numpy arrays cannot be mixed in one call")
    nm = hits.normal
    if _is_tensor(origins):
        import torch
        toi = torch.where((hits.flags & 1) != 0, hits.toi, torch.zeros_like(hits.toi))
        where = torch.where
    else:
        toi = np.where((np.asarray(hits.flags) & 1) != 0, hits.toi, 0.0)
        where = np.where
    step = dirs * toi[:, None]
    points = origins + step
    facing = (nm[:, 0] * dirs[:, 0] + nm[:, 1] * dirs[:, 1]) + nm[:, 2] * dirs[:, 2]
    return points, where((facing > 0)[:, None], -nm, nm)


def occlusion_hits(scene, origins, dirs, hits, sample_dirs, rotations=None, bias=1e-3, max_toi=math.inf, keys=None):
    """Ambient occlusion at the closest hits of caller-supplied rays: occlusion_points() at the hits of `hits = closest_hits(scene, origins, dirs)` (a
    CastHits with normal and flags), on the side the rays came from.  The points are origins + dirs * toi — two separate element-wise operations, with toi 0
    at the misses, as in shade_hits() —; a normal is negated where (nx * dx + ny * dy) + nz * dz > 0.  Misses come back as zeros.  numpy or torch as the
    inputs."""
    points, normals = _hit_points("occlusion_hits", origins, dirs, hits)
    return occlusion_points(scene, points, normals, sample_dirs, rotations, bias, max_toi, hit_flags=hits.flags, keys=keys)


# ---- incoming light at caller-supplied points (include/nrays_abi.h: nrays_gather_points_device) ------------------------------------------------------------

SALT_GATHER = 0x301 << 32  # kSaltGather (csrc/trace_device.h)


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


def _gather_settings(energy, max_depth):
    energy = float(energy)
    if not math.isfinite(energy) or abs(energy) > float(np.finfo(np.float32).max):
        raise ValueError("energy must be a finite float32")
    if int(max_depth) < 0 or int(max_depth) >= 1 << 32:
        raise ValueError("max_depth must be in [0, 2^32)")
    return energy, int(max_depth)


def gather_points(scene, points, normals, sample_dirs, rotations=None, bias=1e-3, energy=1.0, max_depth=0, hit_flags=None, keys=None, unordered=False):
    """The light arriving at n caller-supplied surface points from the rest of the scene — a light map's indirect term —, through nrays_gather_points_device /
    nrays_gather_points: per point the library builds the len(sample_dirs) hemisphere rays of occlusion_points() ON THE DEVICE (the same rays bit for bit:
    occlusion_rays()), runs Scene::trace — the query of trace_rays() — on each and folds the colours in order: (n, 3) float32, the mean.  It equals trace_rays
    on occlusion_rays() with keys gather_ray_keys() and the given energy, summed over j in float32 and divided by float32(k), bit for bit.  No ray
    or per-ray colour is ever in the caller's memory (the library keeps a chunk's ray colours only in scenes where one hit both reflects and refracts).
    Also `scene.gather_points(...)` on Scene and FileScene; gather_hits() feeds it from closest_hits(), bake_indirect() from surface_texels().
    `points`, `normals`, `sample_dirs`, `rotations`, `bias`, `hit_flags`, `keys`: as for occlusion_points.  `energy`: RayWithEnergy::energy of every gathered
    ray (1.0: a primary ray's; less ends the reflection / refraction recursion earlier).  `max_depth` as in render().
    `unordered=True` (nrays_gather_points_device_ex / nrays_gather_points_ex with NRAYS_RAYS_UNORDERED): the rays of neighbouring points do not stay together,
    so the library may bin a chunk's (point, direction) pairs on the device and trace them bin by bin, as trace_rays(unordered=True) does with rays from memory.
    The result is bit-identical; a chunk then keeps 28 bytes a ray in the handle's workspace.  False calls the entry points without _ex.
    numpy arrays -> nrays_gather_points (blocking), a numpy array.  torch tensors on the scene's GPU (float64; hit_flags int32 / uint32; keys int64 / uint64;
    the tables tensors or anything numpy takes) -> nrays_gather_points_device on torch.cuda.current_stream(), a tensor."""
    if not isinstance(unordered, (bool, np.bool_)):
        raise ValueError("unordered must be True or False, got %r" % (unordered,))
    n = _n_of(points, normals, ("points", "normals"))
    for name, a in (("hit_flags", hit_flags), ("keys", keys)):
        _check_vec(name, a, n)
    L, rot, bias, _ = _occlusion_tables(sample_dirs, rotations, bias, math.inf)
    energy, max_depth = _gather_settings(energy, max_depth)
    if _is_tensor(points):
        import torch
        if points.device.type != "cuda":
            raise ValueError("torch tensors must be on the GPU, points is on %s" % points.device)
        f64 = (torch.float64,)
        keys_dt = tuple(d for d in (torch.int64, getattr(torch, "uint64", None)) if d is not None)
        flags_dt = tuple(d for d in (torch.int32, getattr(torch, "uint32", None)) if d is not None)
        L, rot = (t if t is None or _is_tensor(t) else torch.from_numpy(t).to(points.device) for t in (L, rot))
        p, nm, hf, k, L, rot = _torch_args((("points", points, f64), ("normals", normals, f64), ("hit_flags", hit_flags, flags_dt), ("keys", keys, keys_dt),
                                            ("sample_dirs", L, f64), ("rotations", rot, f64)), points.device)
        rgb = torch.empty((n, 3), dtype=torch.float32, device=points.device)
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        params = abi.NraysGatherParams(L.shape[0], 0 if rot is None else rot.shape[0], ptr(L), ptr(rot), bias, energy, max_depth)
        lib = abi.load_hip_lib()
        with torch.cuda.device(points.device):
            if unordered:
                abi.check(lib.nrays_gather_points_device_ex(scene.device_handle(), n, ptr(p), ptr(nm), ptr(hf), ptr(k), C.byref(params), ptr(rgb), abi.RAYS_UNORDERED,
                                                            torch.cuda.current_stream().cuda_stream))
            else:
                abi.check(lib.nrays_gather_points_device(scene.device_handle(), n, ptr(p), ptr(nm), ptr(hf), ptr(k), C.byref(params), ptr(rgb), 0,
                                                         torch.cuda.current_stream().cuda_stream))
        return rgb
    if any(_is_tensor(a) for a in (normals, hit_flags, keys, L, rot)):
        raise ValueError("torch tensors and numpy arrays cannot be mixed in one call")
    p, nm = _np_floats("points", points, np.float64), _np_floats("normals", normals, np.float64)
    hf = None if hit_flags is None else _np_ints("hit_flags", hit_flags, np.uint32)
    k = None if keys is None else _np_keys(keys)
    rgb = np.empty((n, 3), dtype=np.float32)
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    params = abi.NraysGatherParams(len(L), 0 if rot is None else len(rot), L.ctypes.data, None if rot is None else rot.ctypes.data, bias, energy, max_depth)
    lib = abi.load_hip_lib()
    if unordered:
        abi.check(lib.nrays_gather_points_ex(scene.device_handle(), n, ptr(p, C.c_double), ptr(nm, C.c_double), ptr(hf, C.c_uint32), ptr(k, C.c_uint64), C.byref(params),
                                             ptr(rgb, C.c_float), abi.RAYS_UNORDERED))
    else:
        abi.check(lib.nrays_gather_points(scene.device_handle(), n, ptr(p, C.c_double), ptr(nm, C.c_double), ptr(hf, C.c_uint32), ptr(k, C.c_uint64), C.byref(params),
                                          ptr(rgb, C.c_float), 0))
    return rgb


def gather_hits(scene, origins, dirs, hits, sample_dirs, rotations=None, bias=1e-3, energy=1.0, max_depth=0, keys=None, unordered=False):
    """The incoming light at the closest hits of caller-supplied rays: gather_points() at the hits of `hits = closest_hits(scene, origins, dirs)` (a CastHits
    with normal and flags), on the side the rays came from — the points and normals of occlusion_hits(), built the same way.  Misses come back as zeros.
    numpy or torch as the inputs.  `unordered`: as for gather_points."""
    points, normals = _hit_points("gather_hits", origins, dirs, hits)
    return gather_points(scene, points, normals, sample_dirs, rotations, bias, energy, max_depth, hit_flags=hits.flags, keys=keys, unordered=unordered)


# ---- gathered light kept by direction: spherical harmonics per point, irradiance probes (include/nrays_abi.h: nrays_gather_sh_points_device) ----------------

# 1/(2 sqrt(pi)), sqrt(3)/(2 sqrt(pi)), sqrt(15)/(2 sqrt(pi)), sqrt(5)/(4 sqrt(pi)), sqrt(15)/(4 sqrt(pi)): the nearest doubles, as the header spells them
SH_K = (0.28209479177387814, 0.4886025119029199, 1.0925484305920792, 0.31539156525252005, 0.5462742152960396)
SH_MAX_BANDS = 3
SH_COSINE_LOBE = (math.pi, 2.0 * math.pi / 3.0, math.pi / 4.0)  # A_l of Ramamoorthi and Hanrahan 2001, bands 0 .. 2


def _sh_bands(bands):
    if isinstance(bands, bool) or int(bands) != bands or not 1 <= int(bands) <= SH_MAX_BANDS:
        raise ValueError("bands must be 1, 2 or 3, got %r" % (bands,))
    return int(bands)


def _sh_terms(x, y, z, C):
    """The first C basis values at (x, y, z), each an array like x: the nine expressions of the header, left to right as written (numpy or torch, any dtype)."""
    K0, K1, K2, K3, K4 = SH_K
    Y = [K0 + 0.0 * x]
    if C >= 4:
        Y += [K1 * y, K1 * z, K1 * x]
    if C >= 9:
        Y += [(K2 * x) * y, (K2 * y) * z, K3 * ((3.0 * z) * z - 1.0), (K2 * x) * z, K4 * (x * x - y * y)]
    return Y


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


def _gather_sh_call(scene, points, normals, sample_dirs, rotations, bias, energy, max_depth, bands, hit_flags, keys, unordered):
    if not isinstance(unordered, (bool, np.bool_)):
        raise ValueError("unordered must be True or False, got %r" % (unordered,))
    bands = _sh_bands(bands)
    n = _n_of(points, normals, ("points", "normals"))
    for nm_, a in (("hit_flags", hit_flags), ("keys", keys)):
        _check_vec(nm_, a, n)
    L, rot, bias, _ = _occlusion_tables(sample_dirs, rotations, bias, math.inf)
    energy, max_depth = _gather_settings(energy, max_depth)
    flags = abi.RAYS_UNORDERED if unordered else 0
    C_ = bands * bands
    if _is_tensor(points):
        import torch
        if points.device.type != "cuda":
            raise ValueError("torch tensors must be on the GPU, points is on %s" % points.device)
        f64 = (torch.float64,)
        keys_dt = tuple(d for d in (torch.int64, getattr(torch, "uint64", None)) if d is not None)
        flags_dt = tuple(d for d in (torch.int32, getattr(torch, "uint32", None)) if d is not None)
        L, rot = (t if t is None or _is_tensor(t) else torch.from_numpy(t).to(points.device) for t in (L, rot))
        p, nm, hf, k, L, rot = _torch_args((("points", points, f64), ("normals", normals, f64), ("hit_flags", hit_flags, flags_dt), ("keys", keys, keys_dt),
                                            ("sample_dirs", L, f64), ("rotations", rot, f64)), points.device)
        sh = torch.empty((n, C_, 3), dtype=torch.float32, device=points.device)
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        params = abi.NraysGatherParams(L.shape[0], 0 if rot is None else rot.shape[0], ptr(L), ptr(rot), bias, energy, max_depth)
        with torch.cuda.device(points.device):
            abi.check(abi.load_hip_lib().nrays_gather_sh_points_device(scene.device_handle(), n, ptr(p), ptr(nm), ptr(hf), ptr(k), C.byref(params), bands, ptr(sh), flags,
                                                                       torch.cuda.current_stream().cuda_stream))
        return sh
    if any(_is_tensor(a) for a in (normals, hit_flags, keys, L, rot)):
        raise ValueError("torch tensors and numpy arrays cannot be mixed in one call")
    p, nm = _np_floats("points", points, np.float64), _np_floats("normals", normals, np.float64)
    hf = None if hit_flags is None else _np_ints("hit_flags", hit_flags, np.uint32)
    k = None if keys is None else _np_keys(keys)
    sh = np.empty((n, C_, 3), dtype=np.float32)
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    params = abi.NraysGatherParams(len(L), 0 if rot is None else len(rot), L.ctypes.data, None if rot is None else rot.ctypes.data, bias, energy, max_depth)
    abi.check(abi.load_hip_lib().nrays_gather_sh_points(scene.device_handle(), n, ptr(p, C.c_double), ptr(nm, C.c_double), ptr(hf, C.c_uint32), ptr(k, C.c_uint64),
                                                        C.byref(params), bands, ptr(sh, C.c_float), flags))
    return sh


def gather_sh_points(scene, points, normals, sample_dirs, rotations=None, bias=1e-3, energy=1.0, max_depth=0, bands=3, hit_flags=None, keys=None, unordered=False):
    """gather_points() that keeps WHERE the light came from, through nrays_gather_sh_points_device / nrays_gather_sh_points: the same rays, keys and traces, folded
    on the device into the projection onto the real spherical harmonics of bands 0 .. bands - 1 of each ray's direction: (n, bands^2, 3) float32 — a directional
    light map's texels, or irradiance probes (gather_probes()).  It equals sh_fold_ref(occlusion_rays()' directions, trace_rays' colours under gather_ray_keys())
    bit for bit; no measure is applied (sh_irradiance() takes it).  Every scene kind keeps a chunk's ray colours (12 bytes a ray) in the handle's workspace;
    no ray, direction or per-ray colour is ever in the caller's memory.  Arguments and numpy / torch forms: as for gather_points; `unordered=True` passes
    NRAYS_RAYS_UNORDERED (bit-identical values).  Also `scene.gather_sh_points(...)` on Scene and FileScene."""
    return _gather_sh_call(scene, points, normals, sample_dirs, rotations, bias, energy, max_depth, bands, hit_flags, keys, unordered)


def gather_probes(scene, positions, sample_dirs, bands=3, energy=1.0, max_depth=0, keys=None, unordered=True):
    """Irradiance probes at free points in space: gather_sh_points() with normals (0, 0, 1), bias 0 and no rotations — that frame reproduces `sample_dirs`
    (sphere_dirs()) bit for bit as world directions and the origin is the position itself.  (n, bands^2, 3) float32; sh_irradiance(probes, normals) lights a
    surface from them.  A probe's rays share an origin and nothing else, hence `unordered=True` by default.  numpy or torch as `positions`."""
    if len(positions.shape) != 2 or positions.shape[1] != 3:
        raise ValueError("positions must have shape (n, 3), got %s" % (tuple(positions.shape),))
    if _is_tensor(positions):
        import torch
        normals = torch.zeros_like(positions)
    else:
        normals = np.zeros((len(positions), 3), np.float64)
    normals[:, 2] = 1.0
    return _gather_sh_call(scene, positions, normals, sample_dirs, None, 0.0, energy, max_depth, bands, None, keys, unordered)


def gather_sh_fold(scene, points, normals, sample_dirs, ray_colours, rotations=None, bias=1e-3, bands=3, hit_flags=None, keys=None, want_ms=False):
    """Test probe (nrays_debug_gather_sh_fold): the fold kernel of gather_sh_points alone on caller-supplied per-ray colours (n, k, 3) float32, one chunk
    (n * k <= 2^22).  numpy arrays, blocking: (n, bands^2, 3) float32; `want_ms`: also the kernel's time between two HIP events, in milliseconds."""
    bands = _sh_bands(bands)
    n = _n_of(points, normals, ("points", "normals"))
    for nm_, a in (("hit_flags", hit_flags), ("keys", keys)):
        _check_vec(nm_, a, n)
    L, rot, bias, _ = _occlusion_tables(sample_dirs, rotations, bias, math.inf)
    if any(_is_tensor(a) for a in (points, normals, hit_flags, keys, L, rot, ray_colours)):
        raise ValueError("gather_sh_fold takes numpy arrays")
    col = np.ascontiguousarray(ray_colours, dtype=np.float32)
    if col.shape != (n, len(L), 3):
        raise ValueError("ray_colours must have shape (%d, %d, 3), got %s" % (n, len(L), col.shape))
    p, nm = _np_floats("points", points, np.float64), _np_floats("normals", normals, np.float64)
    hf = None if hit_flags is None else _np_ints("hit_flags", hit_flags, np.uint32)
    k = None if keys is None else _np_keys(keys)
    sh, ms = np.empty((n, bands * bands, 3), dtype=np.float32), C.c_float(0.0)
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    params = abi.NraysGatherParams(len(L), 0 if rot is None else len(rot), L.ctypes.data, None if rot is None else rot.ctypes.data, bias, 1.0, 0)
    abi.check(abi.load_hip_lib().nrays_debug_gather_sh_fold(scene.device_handle(), n, ptr(p, C.c_double), ptr(nm, C.c_double), ptr(hf, C.c_uint32), ptr(k, C.c_uint64),
                                                            C.byref(params), bands, ptr(col, C.c_float), ptr(sh, C.c_float), C.byref(ms) if want_ms else None))
    return (sh, float(ms.value)) if want_ms else sh


# ---- the surface of a mesh node at a light map's texels (include/nrays_abi.h: nrays_surface_texels_device) ---------------------------------------------

TEXEL_OUTPUTS = ("normals", "uv", "node", "prim")  # the optional outputs of surface_texels, in the order of nrays_surface_texels_device's arguments
SurfaceTexels = collections.namedtuple("SurfaceTexels", ("points",) + TEXEL_OUTPUTS + ("flags",))
TEXELS_MAX_SIDE, TEXELS_MAX_POINTS = 16384, 1 << 24


def _texel_lattice(width, height):
    width, height = int(width), int(height)
    if not (1 <= width <= TEXELS_MAX_SIDE and 1 <= height <= TEXELS_MAX_SIDE and width * height <= TEXELS_MAX_POINTS):
        raise ValueError("width and height must be in 1 .. %d and width * height <= 2^24, got %d x %d" % (TEXELS_MAX_SIDE, width, height))
    return width, height


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


def surface_texels(scene, node, width, height, centres=False, flip_normals=False, want=TEXEL_OUTPUTS, device=None):
    """The surface of TriMesh node `node` of the scene at the points of a width x height lattice in its uv space — a light map's texels — through
    nrays_surface_texels_device / nrays_surface_texels: per lattice point the triangle that owns it, the world point and normal there.  The baker's first
    step: the arrays pass unfiltered into shade_points (nodes=node, hit_flags=flags, uvs=uv) and occlusion_points (hit_flags=flags); bake_lightmap() does.
    Also `scene.surface_texels(node, ...)` on Scene and FileScene.  surface_texels_ref() restates the result bit for bit.
    Lattice point (x, y) is entry y * width + x and lies at u = x / (width - 1), v = y / (height - 1) — where the scene's own Texture2d::sample reads texel
    (x, y); row 0 is the smallest v, the bottom row of a texture.  `centres=True`: u = (x + 0.5) / width instead.  A point on a shared edge goes to the
    triangle with the smaller index; none falls between two triangles whose edge has the same uv endpoints.  uvs are not wrapped into [0, 1].
    `want`: which of "normals", "uv", "node", "prim" to compute into memory.  Returns SurfaceTexels(points (n, 3) f64, normals (n, 3) f64 (negated with
    flip_normals), uv (n, 2) f64 — the lattice point —, node (n,) i32, prim (n,) i32 — the triangle's index in its mesh —, flags (n,): 3 where covered),
    None for what was not wanted.  An uncovered point has flags 0, node -1, prim -1 and zeros.
    `device=None` -> nrays_surface_texels (blocking), numpy arrays (flags uint32).  `device`: a torch device of the scene's GPU -> nrays_surface_texels_device
    on torch.cuda.current_stream(), tensors there (flags int32)."""
    width, height = _texel_lattice(width, height)
    node = int(node)
    if node < 0:
        raise ValueError("node must be >= 0")
    want = tuple(want)
    for name in want:
        if name not in TEXEL_OUTPUTS:
            raise ValueError("want: unknown output %r (one of %s)" % (name, ", ".join(TEXEL_OUTPUTS)))
    flags = (abi.TEXELS_CENTRES if centres else 0) | (abi.TEXELS_FLIP_NORMALS if flip_normals else 0)
    n = width * height
    shapes = {"points": (n, 3), "normals": (n, 3), "uv": (n, 2), "node": (n,), "prim": (n,), "flags": (n,)}
    wanted = lambda k: k in ("points", "flags") or k in want  # noqa: E731
    if device is not None:
        import torch
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("device must be a GPU, got %s" % device)
        dtypes = {"points": torch.float64, "normals": torch.float64, "uv": torch.float64, "node": torch.int32, "prim": torch.int32, "flags": torch.int32}
        out = {k: torch.empty(shapes[k], dtype=dtypes[k], device=device) if wanted(k) else None for k in SurfaceTexels._fields}
        ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
        lib = abi.load_hip_lib()
        with torch.cuda.device(device):
            abi.check(lib.nrays_surface_texels_device(scene.device_handle(), node, width, height, *[ptr(out[k]) for k in SurfaceTexels._fields], flags,
                                                      torch.cuda.current_stream().cuda_stream))
        return SurfaceTexels(**out)
    dtypes = {"points": np.float64, "normals": np.float64, "uv": np.float64, "node": np.int32, "prim": np.int32, "flags": np.uint32}
    ctypes_of = {np.float64: C.c_double, np.int32: C.c_int32, np.uint32: C.c_uint32}
    out = {k: np.empty(shapes[k], dtype=dtypes[k]) if wanted(k) else None for k in SurfaceTexels._fields}
    ptr = lambda a, ct: None if a is None else a.ctypes.data_as(C.POINTER(ct))  # noqa: E731
    lib = abi.load_hip_lib()
    abi.check(lib.nrays_surface_texels(scene.device_handle(), node, width, height, *[ptr(out[k], ctypes_of[dtypes[k]]) for k in SurfaceTexels._fields], flags))
    return SurfaceTexels(**out)


def surface_texels_passes(scene, node, width, height, centres=False, flip_normals=False, repeats=1):
    """Timing probe (nrays_debug_surface_texels_passes): the owner pass and the resolve pass of surface_texels, `repeats` times between events of their own.
    (repeats, 2) float32, milliseconds."""
    width, height = _texel_lattice(width, height)
    ms = np.zeros((int(repeats), 2), dtype=np.float32)
    flags = (abi.TEXELS_CENTRES if centres else 0) | (abi.TEXELS_FLIP_NORMALS if flip_normals else 0)
    abi.check(abi.load_hip_lib().nrays_debug_surface_texels_passes(scene.device_handle(), int(node), width, height, flags, int(repeats), ms.ctypes.data_as(C.POINTER(C.c_float))))
    return ms


def bake_lightmap(scene, node, width, height, occlusion=None, centres=False, flip_normals=False, keys=None, device=None, dilate=0):
    """A light map of TriMesh node `node`: the direct lighting of its surface at the texels of a width x height map, (height, width, 4) float32 in
    NraysTexture row order (row 0 = the bottom row): shade_points() on surface_texels(), viewed against the normal (view_dirs = -normals), rgb = the lit
    colour, a = the material's alpha.  `occlusion=(sample_dirs, rotations, bias, max_toi)`: rgb is multiplied by the mean filter of occlusion_points() with
    these arguments at the same texels.  Uncovered texels are zeros.  `keys` (width * height,) RNG keys for area lights and the occlusion rotations
    (default: texel i has key i).  `device` as for surface_texels: with a torch device everything stays on the GPU, three calls on one stream; `keys` and
    the tables are then tensors (the tables may be anything numpy takes).  `dilate`: a radius in texels (1 .. 64): the gutters are filled from the nearest
    covered texel by dilate_texels(), one more call on the same stream; 0 = off, the calls and the result above exactly.  A map that is sampled with
    Bilinear (lightmap_texture()) needs dilate >= 2: the diagonal neighbour of a border texel lies at d2 = 2.
    A noisy map is denoised BETWEEN the bake and the dilation, by the calls themselves: tx = surface_texels(...); rgb = gather_points(...);
    rgb = denoise_texels(scene, tx, rgb, width=width, height=height); dilate_texels(..., values=rgb).
    Also `scene.bake_lightmap(node, ...)` on Scene and FileScene."""
    tx = surface_texels(scene, node, width, height, centres, flip_normals, want=("normals", "uv", "node"), device=device)
    rgba = shade_points(scene, tx.points, tx.normals, -tx.normals, tx.node, uvs=tx.uv, hit_flags=tx.flags, keys=keys)
    if occlusion is not None:
        sample_dirs, rotations, bias, max_toi = occlusion
        occ = occlusion_points(scene, tx.points, tx.normals, sample_dirs, rotations, bias, max_toi, hit_flags=tx.flags, keys=keys)
        rgba[:, :3] = rgba[:, :3] * occ.filter
    rgba = _bake_dilate(scene, tx.flags, rgba, width, height, _dilate_radius(dilate))
    return rgba.reshape(int(height), int(width), 4)


@_dilate_keyword
def bake_indirect(scene, node, width, height, sample_dirs, rotations=None, bias=1e-3, energy=1.0, max_depth=0, centres=False, flip_normals=False, keys=None,
                  device=None, unordered=False):
    """The indirect term of a light map of TriMesh node `node`: the mean incoming light at the texels of a width x height map, (height, width, 3) float32 in
    NraysTexture row order (row 0 = the bottom row): gather_points() with these arguments on surface_texels().  Uncovered texels are zeros.  `keys`
    (width * height,) RNG keys (default: texel i has key i).  `device` as for surface_texels: with a torch device everything stays on the GPU, two calls on one
    stream; `keys` is then a tensor (the tables may be anything numpy takes).  `unordered`: as for gather_points.  `dilate` (keyword only, see
    _dilate_keyword): as for bake_lightmap — a radius in texels, filled by dilate_texels() on the same stream; 0 = off, today's calls and result exactly;
    Bilinear sampling needs dilate >= 2 (the diagonal neighbour of a border texel lies at d2 = 2).  The mean of few rays is noisy; the recipe with the
    denoising step between the gather and the dilation: tx = surface_texels(...); rgb = gather_points(...); rgb = denoise_texels(scene, tx, rgb, width=width, height=height);
    dilate_texels(..., values=rgb).  Also `scene.bake_indirect(node, ...)` on Scene and FileScene."""
    tx = surface_texels(scene, node, width, height, centres, flip_normals, want=("normals",), device=device)
    rgb = gather_points(scene, tx.points, tx.normals, sample_dirs, rotations, bias, energy, max_depth, hit_flags=tx.flags, keys=keys, unordered=unordered)
    return rgb.reshape(int(height), int(width), 3)


def _dilate_args(flags, width, height, radius, values):
    """Checks shared by dilate_texels and dilate_texels_ref: (width, height, radius, channels); channels 0 without values."""
    width, height = _texel_lattice(width, height)
    radius = int(radius)
    if not 1 <= radius <= abi.DILATE_MAX_RADIUS:
        raise ValueError("radius must be in 1 .. %d, got %d" % (abi.DILATE_MAX_RADIUS, radius))
    n = width * height
    if int(np.prod(tuple(flags.shape))) != n:
        raise ValueError("flags must hold width * height = %d words, got shape %s" % (n, tuple(flags.shape)))
    channels = 0
    if values is not None:
        size = int(np.prod(tuple(values.shape)))
        channels = size // n
        if channels * n != size or not 1 <= channels <= 4:
            raise ValueError("values must hold 1 .. 4 floats per lattice point (%d points), got shape %s" % (n, tuple(values.shape)))
    return width, height, radius, channels


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


def dilate_texels(scene, flags, width, height, radius, values=None, want_source=False, device=None):
    """Gutter dilation of a width x height light map through nrays_dilate_texels_device / nrays_dilate_texels: every uncovered texel takes the values of
    the nearest covered texel within `radius` (1 .. 64; a Euclidean disc, no wrap-around, the smaller index y * width + x among equals).  `flags`:
    width * height words, texel (x, y) at y * width + x, covered iff bit 0 is set — the flags of surface_texels() as they are.  `values`: 1 .. 4
    float32 per texel ((n, c), (height, width, c) or (n,)), dilated IN PLACE when it is a C-contiguous float32 array or tensor (a converted copy
    otherwise): the words of the source are copied as bit patterns; covered texels and texels with nothing in reach are not written.
    Returns (values or None, source or None, flags): source (n,) int32 with want_source — the texel copied from, the texel itself where covered, -1 where
    nothing is in reach —; flags a new array, the input | abi.TEXEL_FILLED at the filled texels (bit 0 stays clear there).
    numpy arrays -> nrays_dilate_texels (blocking; flags out uint32).  torch tensors on the scene's GPU (flags int32, values float32) ->
    nrays_dilate_texels_device on torch.cuda.current_stream(), tensors there; `device` moves numpy arguments to that GPU first.
    Also `scene.dilate_texels(flags, ...)` on Scene and FileScene.  dilate_texels_ref() restates the result bit for bit."""
    w, h, r, channels = _dilate_args(flags, width, height, radius, values)
    n = w * h
    lib = abi.load_hip_lib()
    if device is not None and not _is_tensor(flags):
        import torch
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("device must be a GPU, got %s" % device)
        flags = torch.from_numpy(_np_ints("flags", flags, np.uint32).view(np.int32)).to(device)
        if values is not None:
            values = torch.from_numpy(_np_floats("values", values, np.float32)).to(device)
    if _is_tensor(flags):
        import torch
        dev = flags.device
        if dev.type != "cuda":
            raise ValueError("flags must be on a GPU, got %s" % dev)
        if device is not None and torch.device(device).index not in (None, dev.index):
            raise ValueError("flags is on %s, device is %s" % (dev, device))
        f_in, v = _torch_args((("flags", flags, (torch.int32, torch.uint32)), ("values", values, (torch.float32,))), dev)
        out_flags = torch.empty(n, dtype=torch.int32, device=dev)
        source = torch.empty(n, dtype=torch.int32, device=dev) if want_source else None
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        with torch.cuda.device(dev):
            abi.check(lib.nrays_dilate_texels_device(scene.device_handle(), w, h, ptr(f_in), r, channels, ptr(v), ptr(source), ptr(out_flags), 0,
                                                     torch.cuda.current_stream().cuda_stream))
        return v, source, out_flags
    if _is_tensor(values):
        raise ValueError("values: torch tensors and numpy arrays cannot be mixed in one call")
    f_in = _np_ints("flags", flags, np.uint32).reshape(n)
    v = None
    if values is not None:
        v = values if (isinstance(values, np.ndarray) and values.dtype == np.float32 and values.flags.c_contiguous and values.flags.writeable) else \
            np.array(_np_floats("values", values, np.float32), copy=True)
    out_flags = np.empty(n, dtype=np.uint32)
    source = np.empty(n, dtype=np.int32) if want_source else None
    ptr = lambda a, ct: None if a is None else a.ctypes.data_as(C.POINTER(ct))  # noqa: E731
    abi.check(lib.nrays_dilate_texels(scene.device_handle(), w, h, ptr(f_in, C.c_uint32), r, channels, ptr(v, C.c_float), ptr(source, C.c_int32),
                                      ptr(out_flags, C.c_uint32), 0))
    return v, source, out_flags


def lightmap_texture(rgba):
    """A baked (height, width, 4) light map — bake_lightmap()'s result, row 0 = the bottom row as NraysTexture wants it — as the Texture2d a material
    samples it through: float32 texels, Bilinear, ClampToEdges.  Bake with dilate >= 2, or the charts' borders blend with unlit texels."""
    if _is_tensor(rgba):
        rgba = rgba.detach().cpu().numpy()
    return Texture2d(ImageData(np.ascontiguousarray(rgba, dtype=np.float32)), Interpolation.Bilinear, Overflow.ClampToEdges)


def _dilate_radius(dilate):
    dilate = int(dilate)
    if dilate < 0 or dilate > abi.DILATE_MAX_RADIUS:
        raise ValueError("dilate must be 0 (off) or a radius in 1 .. %d, got %d" % (abi.DILATE_MAX_RADIUS, dilate))
    return dilate


def _bake_dilate(scene, flags, out, width, height, radius):
    """The bakers' last step: `out` (n, c) dilated in place by `radius` texels on the texels' `flags`; 0 = nothing is called."""
    if radius == 0:
        return out
    if not (out.is_contiguous() if _is_tensor(out) else out.flags.c_contiguous):
        out = out.contiguous() if _is_tensor(out) else np.ascontiguousarray(out)
    return dilate_texels(scene, flags, width, height, radius, values=out)[0]


# ---- light gathered from baked maps at the rays' closest hits: the bounces of a light map (include/nrays_abi.h: nrays_gather_maps_points_device) -----------------

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


def _gather_maps_args(scene, maps, node_map, max_toi, miss):
    """The checks of gather_maps_points that need no library: [(texels, interp, overflow)] with texels a (h, w, 4) float32 array or tensor, the node map as an
    int32 array of the scene's node count, max_toi and miss as floats."""
    if isinstance(maps, (Texture2d, np.ndarray)) or _is_tensor(maps) or maps is None:
        raise ValueError("maps must be a list of (height, width, 4) float32 arrays or tensors, or of Texture2d")
    maps = list(maps)
    if not 1 <= len(maps) <= abi.GATHER_MAX_MAPS:
        raise ValueError("maps must hold 1 .. %d maps, got %d" % (abi.GATHER_MAX_MAPS, len(maps)))
    out = []
    for i, m in enumerate(maps):
        interp, overflow = Interpolation.Bilinear, Overflow.ClampToEdges
        if isinstance(m, Texture2d):
            interp, overflow = m.interpol, m.overflow
            if m.data.format != abi.TEXEL_RGBA32F:
                raise ValueError("maps[%d]: a Texture2d of float32 texels is required" % i)
            m = m.data.pixels
        if interp not in (Interpolation.Bilinear, Interpolation.Nearest) or overflow not in (Overflow.Wrap, Overflow.ClampToEdges):
            raise ValueError("maps[%d]: unknown interpolation or overflow" % i)
        if _is_tensor(m):
            import torch
            ok = m.dtype == torch.float32
        else:
            if not isinstance(m, np.ndarray):
                raise ValueError("maps[%d] must be a numpy array, a torch tensor or a Texture2d, got %s" % (i, type(m).__name__))
            ok = m.dtype == np.float32
        if not ok or len(m.shape) != 3 or m.shape[2] != 4 or m.shape[0] < 1 or m.shape[1] < 1:
            raise ValueError("maps[%d] must be (height, width, 4) float32, got %s %s" % (i, tuple(m.shape), m.dtype))
        out.append((m, interp, overflow))
    num_nodes = int(scene.descriptor.desc.num_nodes)
    is_int = lambda x: isinstance(x, (int, np.integer)) and not isinstance(x, (bool, np.bool_))  # noqa: E731
    if isinstance(node_map, dict):
        nodes = np.full(num_nodes, -1, dtype=np.int32)
        for k, m in node_map.items():
            if not is_int(k) or not is_int(m):
                raise ValueError("node_map: nodes and maps must be integers, got %r: %r" % (k, m))
            if not 0 <= k < num_nodes:
                raise ValueError("node_map: node %d is not one of the scene's %d nodes" % (k, num_nodes))
            nodes[k] = min(max(int(m), -1), abi.GATHER_MAX_MAPS)
    else:
        if node_map is None or _is_tensor(node_map) or isinstance(node_map, (str, bytes)):
            raise ValueError("node_map must be a sequence of integers or a dict {node: map}")
        entries = list(node_map)
        if not all(is_int(m) for m in entries):
            raise ValueError("node_map: every entry must be an integer")
        if len(entries) != num_nodes:
            raise ValueError("node_map must have one entry per node of the scene (%d), got %d" % (num_nodes, len(entries)))
        nodes = np.array([min(max(int(m), -1), abi.GATHER_MAX_MAPS) for m in entries], dtype=np.int32).reshape(num_nodes)
    max_toi = float(max_toi)
    if not max_toi > 0.0:
        raise ValueError("max_toi must be > 0 (inf allowed)")
    miss = tuple(float(x) for x in np.asarray(miss, dtype=np.float64).reshape(-1))
    if len(miss) != 3 or not all(math.isfinite(x) and abs(x) <= float(np.finfo(np.float32).max) for x in miss):
        raise ValueError("miss must be 3 finite float32 values")
    return out, nodes, max_toi, miss


def _gather_maps_params(L, rot, bias, max_toi, recs, node_ptr, num_nodes, miss, ptr):
    """NraysGatherMapsParams over `recs` = [(texel address, width, height, interp, overflow)]; returns (params, the records' array, which must outlive the call)."""
    arr = (abi.NraysTexture * len(recs))()
    for t, (addr, w, h, interp, overflow) in zip(arr, recs):
        t.width, t.height, t.format, t.interp, t.overflow, t.texels = w, h, abi.TEXEL_RGBA32F, interp, overflow, addr
    params = abi.NraysGatherMapsParams(L.shape[0], 0 if rot is None else rot.shape[0], ptr(L), ptr(rot), bias, max_toi, len(recs), num_nodes,
                                       C.cast(arr, C.POINTER(abi.NraysTexture)), node_ptr, (C.c_float * 3)(*miss))
    return params, arr


def gather_maps_points(scene, points, normals, sample_dirs, maps, node_map, rotations=None, bias=1e-3, max_toi=math.inf, miss=(0.0, 0.0, 0.0), hit_flags=None,
                       keys=None, want_counts=False):
    """The light that baked maps hold at the closest hits of the hemisphere rays of n caller-supplied surface points — one diffuse bounce of a light-map baker —
    through nrays_gather_maps_points_device / nrays_gather_maps_points: per point the library builds the len(sample_dirs) rays of occlusion_points() ON THE DEVICE
    (the same rays bit for bit: occlusion_rays()), finds each ray's closest hit (the query of closest_hits(), with `max_toi`), samples the map of the node it hit
    at the hit's uv (lightmap_sample_ref() restates the sample bit for bit) and folds the colours in order: (n, 3) float32, the mean.  A ray that leaves the scene
    brings `miss`; a hit on a node without a map, or whose record carries no uv, brings black.  It equals closest_hits on occlusion_rays(), lightmap_sample_ref at
    the hits' uv, summed over j in float32 and divided by float32(k), bit for bit.  No ray or per-ray value is ever in memory.
    Also `scene.gather_maps_points(...)` on Scene and FileScene; gather_maps_hits() feeds it from closest_hits(), bake_bounces() loops it over a map.
    `maps`: 1 .. 16 maps, each a (height, width, 4) float32 array or CUDA tensor in NraysTexture row order (row 0 = the bottom row; what bake_lightmap returns),
    sampled Bilinear / ClampToEdges (bake with dilate >= 2), or a Texture2d of float32 texels for another mode.  `node_map`: one entry per node of the scene — the
    index of the map its surface reads, or -1 —, or a dict {node: map} (every other node -1).  `points`, `normals`, `sample_dirs`, `rotations`, `bias`,
    `hit_flags`, `keys`: as for occlusion_points (only the rotation pick reads the keys).  `want_counts`: returns (rgb, counts) with counts (n, 2) — the mapped
    and the missed rays of each point.
    numpy arrays -> nrays_gather_maps_points (blocking), numpy arrays (counts uint32).  torch tensors on the scene's GPU (points / normals float64; maps tensors
    there or numpy arrays, which are uploaded) -> nrays_gather_maps_points_device on torch.cuda.current_stream(), tensors (counts int32)."""
    n = _n_of(points, normals, ("points", "normals"))
    for name, a in (("hit_flags", hit_flags), ("keys", keys)):
        _check_vec(name, a, n)
    L, rot, bias, _ = _occlusion_tables(sample_dirs, rotations, bias, math.inf)
    ms, nodes, max_toi, miss = _gather_maps_args(scene, maps, node_map, max_toi, miss)
    if _is_tensor(points):
        import torch
        if points.device.type != "cuda":
            raise ValueError("torch tensors must be on the GPU, points is on %s" % points.device)
        f64 = (torch.float64,)
        keys_dt = tuple(d for d in (torch.int64, getattr(torch, "uint64", None)) if d is not None)
        flags_dt = tuple(d for d in (torch.int32, getattr(torch, "uint32", None)) if d is not None)
        L, rot = (t if t is None or _is_tensor(t) else torch.from_numpy(t).to(points.device) for t in (L, rot))
        p, nm, hf, k, L, rot = _torch_args((("points", points, f64), ("normals", normals, f64), ("hit_flags", hit_flags, flags_dt), ("keys", keys, keys_dt),
                                            ("sample_dirs", L, f64), ("rotations", rot, f64)), points.device)
        texels = [m if _is_tensor(m) else torch.from_numpy(np.ascontiguousarray(m)).to(points.device) for m, _, _ in ms]
        texels = list(_torch_args(tuple(("maps[%d]" % i, t, (torch.float32,)) for i, t in enumerate(texels)), points.device))
        node_t = torch.from_numpy(nodes).to(points.device)
        rgb = torch.empty((n, 3), dtype=torch.float32, device=points.device)
        counts = torch.empty((n, 2), dtype=torch.int32, device=points.device) if want_counts else None
        ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
        recs = [(t.data_ptr(), t.shape[1], t.shape[0], interp, overflow) for t, (_, interp, overflow) in zip(texels, ms)]
        params, keep = _gather_maps_params(L, rot, bias, max_toi, recs, node_t.data_ptr(), len(nodes), miss, ptr)
        lib = abi.load_hip_lib()
        with torch.cuda.device(points.device):
            abi.check(lib.nrays_gather_maps_points_device(scene.device_handle(), n, ptr(p), ptr(nm), ptr(hf), ptr(k), C.byref(params), ptr(rgb), ptr(counts), 0,
                                                          torch.cuda.current_stream().cuda_stream))
        del keep
        return (rgb, counts) if want_counts else rgb
    if any(_is_tensor(a) for a in (normals, hit_flags, keys, L, rot)) or any(_is_tensor(m) for m, _, _ in ms):
        raise ValueError("torch tensors and numpy arrays cannot be mixed in one call")
    p, nm = _np_floats("points", points, np.float64), _np_floats("normals", normals, np.float64)
    hf = None if hit_flags is None else _np_ints("hit_flags", hit_flags, np.uint32)
    k = None if keys is None else _np_keys(keys)
    texels = [np.ascontiguousarray(m) for m, _, _ in ms]
    rgb = np.empty((n, 3), dtype=np.float32)
    counts = np.empty((n, 2), dtype=np.uint32) if want_counts else None
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    recs = [(t.ctypes.data, t.shape[1], t.shape[0], interp, overflow) for t, (_, interp, overflow) in zip(texels, ms)]
    params, keep = _gather_maps_params(L, rot, bias, max_toi, recs, nodes.ctypes.data, len(nodes), miss, lambda a: None if a is None else a.ctypes.data)
    lib = abi.load_hip_lib()
    abi.check(lib.nrays_gather_maps_points(scene.device_handle(), n, ptr(p, C.c_double), ptr(nm, C.c_double), ptr(hf, C.c_uint32), ptr(k, C.c_uint64), C.byref(params),
                                           ptr(rgb, C.c_float), ptr(counts, C.c_uint32), 0))
    del keep
    return (rgb, counts) if want_counts else rgb


def gather_maps_hits(scene, origins, dirs, hits, sample_dirs, maps, node_map, rotations=None, bias=1e-3, max_toi=math.inf, miss=(0.0, 0.0, 0.0), keys=None,
                     want_counts=False):
    """The light of baked maps arriving at the closest hits of caller-supplied rays: gather_maps_points() at the hits of `hits = closest_hits(scene, origins, dirs)`
    (a CastHits with normal and flags), on the side the rays came from — the points and normals of occlusion_hits(), built the same way.  Misses come back as
    zeros.  numpy or torch as the inputs."""
    points, normals = _hit_points("gather_maps_hits", origins, dirs, hits)
    return gather_maps_points(scene, points, normals, sample_dirs, maps, node_map, rotations, bias, max_toi, miss, hit_flags=hits.flags, keys=keys,
                              want_counts=want_counts)


def bake_bounces(scene, node, width, height, sample_dirs, bounces, albedo, rotations=None, bias=1e-3, miss=(0.0, 0.0, 0.0), dilate=2, flip_normals=False, keys=None,
                 device=None):
    """The multi-bounce light map of TriMesh node `node`, (height, width, 4) float32 in NraysTexture row order (row 0 = the bottom row), on one stream, without a
    scene rebuild and — with `device` — without a host copy:
      tx  = surface_texels(node, width, height) on the default lattice, the one Texture2d::sample reads (there is no `centres` here);
      L_0 = shade_points at the texels viewed against the normal — what bake_lightmap() computes —, dilated;
      L_b = albedo * gather_maps_points(tx, maps=[L_{b-1}], node_map={node: 0}, miss = `miss` if b == 1 else 0), dilated, for b = 1 .. bounces: the sky reaches a
            texel once — later bounces carry it inside L_{b-1};
      the result is L_0 + L_1 + ... added in that order in float32, alpha from L_0.
    `albedo`: 3 floats or a (height, width, 3) array, the diffuse reflectance a bounce is multiplied by.  `sample_dirs` cosine-weighted (hemisphere_dirs()) make
    the mean the irradiance integral of a diffuse surface.  `dilate` (2 .. 64): every L_b is sampled Bilinear, which reads the diagonal neighbour of a border
    texel, so less than 2 raises ValueError.  `keys`, `rotations`, `bias`, `flip_normals`, `device`: as for bake_lightmap / bake_indirect.
    Denoising stays the caller's step, between the calls: this loop is tx = surface_texels(...); L = shade_points(...); dilate_texels(...);
    rgb = gather_maps_points(...); rgb = denoise_texels(scene, tx, rgb, width=width, height=height); dilate_texels(..., values=rgb); and so on.
    Also `scene.bake_bounces(node, ...)` on Scene and FileScene."""
    width, height = _texel_lattice(width, height)
    bounces = int(bounces)
    if bounces < 0:
        raise ValueError("bounces must be >= 0")
    radius = _dilate_radius(dilate)
    if radius < 2:
        raise ValueError("dilate must be >= 2: a Bilinear sample reads the diagonal neighbour of a border texel")
    _occlusion_tables(sample_dirs, rotations, bias, math.inf)
    _, _, _, miss = _gather_maps_args(scene, [np.zeros((1, 1, 4), np.float32)], {}, math.inf, miss)
    if _is_tensor(albedo):
        albedo = albedo.detach().cpu().numpy()
    a = np.asarray(albedo)
    if not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)) or a.shape not in ((3,), (height, width, 3)):
        raise ValueError("albedo must be 3 numbers or a (height, width, 3) array, got shape %s" % (a.shape,))
    a = np.array(a.astype(np.float32).reshape(-1, 3), copy=True, order="C")  # (n, 3) per texel, or (1, 3)
    tx = surface_texels(scene, node, width, height, False, flip_normals, want=("normals", "uv", "node"), device=device)
    level = shade_points(scene, tx.points, tx.normals, -tx.normals, tx.node, uvs=tx.uv, hit_flags=tx.flags, keys=keys)
    level = _bake_dilate(scene, tx.flags, level, width, height, radius)
    if _is_tensor(level):
        import torch
        a = torch.from_numpy(a).to(level.device)
    total = level.clone() if _is_tensor(level) else level.copy()
    for b in range(1, bounces + 1):
        rgb = gather_maps_points(scene, tx.points, tx.normals, sample_dirs, [level.reshape(height, width, 4)], {int(node): 0}, rotations, bias, math.inf,
                                 miss if b == 1 else (0.0, 0.0, 0.0), hit_flags=tx.flags, keys=keys)
        nxt = total.clone() if _is_tensor(total) else total.copy()  # (alpha from L_0; the rgb of every texel is written below or left to the dilation)
        nxt[:, :3] = a * rgb
        level = _bake_dilate(scene, tx.flags, nxt, width, height, radius)
        total[:, :3] = total[:, :3] + level[:, :3]
    return total.reshape(height, width, 4)


# ---- denoising a baked map: the a-trous joint-bilateral filter (include/nrays_abi.h: nrays_filter_texels_device) -----------------------------------------------

FILTER_TAPS = (1, 4, 6, 4, 1)  # the B3 spline; a tap's kernel weight is the product of two of them, 1 .. 36


def _filter_args(flags, width, height, points, normals, values, step, pos_radius, normal_cos):
    """Checks shared by filter_texels, filter_texels_ref and denoise_texels: (width, height, step, pos_radius, normal_cos, channels)."""
    width, height = _texel_lattice(width, height)
    step, pos_radius, normal_cos = int(step), float(pos_radius), float(normal_cos)
    if not 1 <= step <= abi.FILTER_MAX_STEP:
        raise ValueError("step must be in 1 .. %d, got %d" % (abi.FILTER_MAX_STEP, step))
    if not pos_radius > 0.0:
        raise ValueError("pos_radius must be > 0 (math.inf: no position weight), got %r" % pos_radius)
    if not -1.0 <= normal_cos < 1.0:
        raise ValueError("normal_cos must be in [-1, 1), got %r" % normal_cos)
    n = width * height
    for name, a, per in (("flags", flags, 1), ("points", points, 3), ("normals", normals, 3)):
        if a is None:
            raise ValueError("%s is required" % name)
        if int(np.prod(tuple(a.shape))) != n * per:
            raise ValueError("%s must hold %d x width * height = %d words, got shape %s" % (name, per, n * per, tuple(a.shape)))
    if values is None:
        raise ValueError("values is required")
    size = int(np.prod(tuple(values.shape)))
    channels = size // n
    if channels * n != size or not 1 <= channels <= 4:
        raise ValueError("values must hold 1 .. 4 floats per lattice point (%d points), got shape %s" % (n, tuple(values.shape)))
    return width, height, step, pos_radius, normal_cos, channels


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


def _filter_pass_device(lib, scene, w, h, f, p, nm, channels, v_in, v_out, step, pos_radius, normal_cos):
    """One nrays_filter_texels_device call on contiguous tensors of one GPU, on torch.cuda.current_stream()."""
    import torch
    with torch.cuda.device(f.device):
        abi.check(lib.nrays_filter_texels_device(scene.device_handle(), w, h, f.data_ptr(), p.data_ptr(), nm.data_ptr(), channels, v_in.data_ptr(), v_out.data_ptr(), step,
                                                 pos_radius, normal_cos, 0, torch.cuda.current_stream().cuda_stream))


def _filter_tensors(flags, points, normals, values, device):
    """The four arrays of a filter call as contiguous tensors on one GPU (flags int32 / uint32, points / normals float64, values float32): tensors are
    checked, numpy arrays are moved to `device`."""
    import torch
    if not _is_tensor(flags):
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("device must be a GPU, got %s" % device)
        flags = torch.from_numpy(_np_ints("flags", flags, np.uint32).view(np.int32)).to(device)
        points, normals = (torch.from_numpy(_np_floats(name, a, np.float64)).to(device) for name, a in (("points", points), ("normals", normals)))
        values = torch.from_numpy(_np_floats("values", values, np.float32)).to(device)
    dev = flags.device
    if dev.type != "cuda":
        raise ValueError("flags must be on a GPU, got %s" % dev)
    if device is not None and torch.device(device).index not in (None, dev.index):
        raise ValueError("flags is on %s, device is %s" % (dev, device))
    return _torch_args((("flags", flags, (torch.int32, torch.uint32)), ("points", points, (torch.float64,)), ("normals", normals, (torch.float64,)),
                        ("values", values, (torch.float32,))), dev)


def filter_texels(scene, flags, width, height, points, normals, values, step=1, pos_radius=math.inf, normal_cos=0.0, device=None):
    """One pass of the edge-aware filter that denoises a baked width x height light map, through nrays_filter_texels_device / nrays_filter_texels: a 5 x 5
    a-trous (B3-spline) joint-bilateral filter whose taps lie `step` (1 .. 64) texels apart.  A covered texel becomes the weighted mean of the covered
    texels among its 25 taps that lie on the same piece of surface: a tap's weight falls linearly with its squared world distance, reaching 0 at
    `pos_radius` (math.inf: no position weight), and with the cosine between the normals, reaching 0 at `normal_cos` (in [-1, 1); -1 with unit normals:
    no normal weight) — so nothing blends across a chart border, a gutter or a crease.  Uncovered texels keep their words.  `flags`, `points`,
    `normals`: flags / points / normals of surface_texels() as they are; `values`: 1 .. 4 float32 per texel ((n, c), (height, width, c) or (n,)).
    Returns a NEW array or tensor in the shape of `values`; the arguments stay as they are.
    numpy arrays -> nrays_filter_texels (blocking).  torch tensors on the scene's GPU (flags int32, points / normals float64, values float32) ->
    nrays_filter_texels_device on torch.cuda.current_stream(); `device` moves numpy arguments to that GPU first.  Also `scene.filter_texels(flags, ...)`
    on Scene and FileScene; denoise_texels() runs the passes with steps 1, 2, 4, ...; filter_texels_ref() restates the result bit for bit."""
    w, h, step, pos_radius, normal_cos, channels = _filter_args(flags, width, height, points, normals, values, step, pos_radius, normal_cos)
    lib = abi.load_hip_lib()
    if _is_tensor(flags) or device is not None:
        import torch
        f, p, nm, v = _filter_tensors(flags, points, normals, values, device)
        out = torch.empty_like(v)
        _filter_pass_device(lib, scene, w, h, f, p, nm, channels, v, out, step, pos_radius, normal_cos)
        return out.reshape(tuple(values.shape))
    for name, a in (("points", points), ("normals", normals), ("values", values)):
        if _is_tensor(a):
            raise ValueError("%s: torch tensors and numpy arrays cannot be mixed in one call" % name)
    f = _np_ints("flags", flags, np.uint32)
    p, nm, v = _np_floats("points", points, np.float64), _np_floats("normals", normals, np.float64), _np_floats("values", values, np.float32)
    out = np.empty_like(v)
    ptr = lambda a, ct: a.ctypes.data_as(C.POINTER(ct))  # noqa: E731
    abi.check(lib.nrays_filter_texels(scene.device_handle(), w, h, ptr(f, C.c_uint32), ptr(p, C.c_double), ptr(nm, C.c_double), channels, ptr(v, C.c_float), ptr(out, C.c_float),
                                      step, pos_radius, normal_cos, 0))
    return out.reshape(np.shape(values))


def denoise_texels(scene, tx, values, passes=3, pos_radius=math.inf, normal_cos=0.0, width=None, height=None):
    """A baked light map denoised: `passes` (1 .. 7) passes of filter_texels() with steps 1, 2, 4, ... on the texels `tx` — a SurfaceTexels with its normals,
    surface_texels()'s result as it is — between two buffers, all on torch.cuda.current_stream(), nothing read back in between.  Three passes reach 29 texels
    across at 75 taps.  `values`: (height, width, c) or, with `width` and `height` given, (n, c) / (n,); a tensor on the scene's GPU like tx's arrays, or
    numpy arrays all of them, which are moved to the current GPU once and the result back.  Returns a new array or tensor in the shape of `values`.
    The place of the call in a bake:
        tx = surface_texels(...); rgb = gather_points(...); rgb = denoise_texels(scene, tx, rgb, width=w, height=h); dilate_texels(..., values=rgb)
    Also `scene.denoise_texels(tx, values, ...)` on Scene and FileScene."""
    passes = int(passes)
    if not 1 <= passes <= 7:
        raise ValueError("passes must be in 1 .. 7 (steps 1 .. %d), got %d" % (abi.FILTER_MAX_STEP, passes))
    if width is None or height is None:
        if len(values.shape) != 3:
            raise ValueError("values must have shape (height, width, channels) unless width and height are given, got %s" % (tuple(values.shape),))
        height, width = int(values.shape[0]), int(values.shape[1])
    if getattr(tx, "normals", None) is None:
        raise ValueError("tx must hold normals (surface_texels(..., want=('normals', ...)))")
    w, h, _, pos_radius, normal_cos, channels = _filter_args(tx.flags, width, height, tx.points, tx.normals, values, 1, pos_radius, normal_cos)
    lib = abi.load_hip_lib()
    import torch
    as_numpy = not _is_tensor(tx.flags)
    f, p, nm, v = _filter_tensors(tx.flags, tx.points, tx.normals, values, torch.device("cuda", torch.cuda.current_device()) if as_numpy else None)
    bufs = [v, torch.empty_like(v), torch.empty_like(v) if passes > 1 else None]  # the input is never written
    src = 0
    for k in range(passes):
        dst = 1 if src != 1 else 2
        _filter_pass_device(lib, scene, w, h, f, p, nm, channels, bufs[src], bufs[dst], 1 << k, pos_radius, normal_cos)
        src = dst
    out = bufs[src].reshape(tuple(values.shape))
    return out.cpu().numpy() if as_numpy else out


def ray_order(scene, origins, dirs):
    """Test probe (nrays_debug_ray_order): the key and binning kernels of one unordered chunk on n <= 2^22 rays (numpy, (n, 3)).  Returns
    (keys uint64 (n,), order uint32 (n,) — order[j] = index of the ray traced j-th —, frame float64 (abi.RAY_FRAME_DOUBLES,),
    (K, B, reordered): significant bits of a key, leading bits the binning orders by, whether a hinted batch of n rays on this handle
    would be reordered)."""
    n = _n_of(origins, dirs)
    if n > 1 << 22:
        raise ValueError("at most one chunk (2^22 rays)")
    if _is_tensor(origins) or _is_tensor(dirs):
        raise ValueError("ray_order takes numpy arrays")
    o, d = _np_floats("origins", origins, np.float64), _np_floats("dirs", dirs, np.float64)
    keys, order = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    frame, info = np.zeros(abi.RAY_FRAME_DOUBLES, np.float64), (C.c_uint32 * 4)()
    dp = C.POINTER(C.c_double)
    abi.check(abi.load_hip_lib().nrays_debug_ray_order(scene.device_handle(), n, o.ctypes.data_as(dp), d.ctypes.data_as(dp), keys.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                       order.ctypes.data_as(C.POINTER(C.c_uint32)), frame.ctypes.data_as(dp), info))
    return keys, order, frame, (int(info[0]), int(info[1]), bool(info[2]))


def gather_order(scene, points, normals, sample_dirs, rotations=None, bias=1e-3, hit_flags=None, keys=None):
    """Test probe (nrays_debug_gather_order): the bounds, key and binning kernels of one reordered chunk of gather_points(unordered=True) on n points with
    n * len(sample_dirs) <= 2^22 (numpy).  Pair i * k + j is ray j of point i.  Returns (keys uint64 (n * k,) — zeros at a skipped point's pairs —,
    order uint32 (m,) — the m live pairs in trace order —, frame float64 (abi.RAY_FRAME_DOUBLES,), (K, B, reordered, m)) as ray_order() does for rays."""
    n = _n_of(points, normals, ("points", "normals"))
    for name, a in (("hit_flags", hit_flags), ("keys", keys)):
        _check_vec(name, a, n)
    L, rot, bias, _ = _occlusion_tables(sample_dirs, rotations, bias, math.inf)
    if any(_is_tensor(a) for a in (points, normals, hit_flags, keys, L, rot)):
        raise ValueError("gather_order takes numpy arrays")
    pairs = n * len(L)
    if pairs > 1 << 22:
        raise ValueError("at most one chunk (n * len(sample_dirs) <= 2^22)")
    p, nm = _np_floats("points", points, np.float64), _np_floats("normals", normals, np.float64)
    hf = None if hit_flags is None else _np_ints("hit_flags", hit_flags, np.uint32)
    k = None if keys is None else _np_keys(keys)
    out_keys, order = np.zeros(pairs, np.uint64), np.zeros(pairs, np.uint32)
    frame, info = np.zeros(abi.RAY_FRAME_DOUBLES, np.float64), (C.c_uint32 * 4)()
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    params = abi.NraysGatherParams(len(L), 0 if rot is None else len(rot), L.ctypes.data, None if rot is None else rot.ctypes.data, bias, 1.0, 0)
    abi.check(abi.load_hip_lib().nrays_debug_gather_order(scene.device_handle(), n, ptr(p, C.c_double), ptr(nm, C.c_double), ptr(hf, C.c_uint32), ptr(k, C.c_uint64),
                                                          C.byref(params), ptr(out_keys, C.c_uint64), ptr(order, C.c_uint32), ptr(frame, C.c_double), info))
    return out_keys, order[:int(info[3])].copy(), frame, (int(info[0]), int(info[1]), bool(info[2]), int(info[3]))


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
