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
from .marshal import (CURRENT, F32, F64, I32, MATERIAL_OUTPUTS, NEAREST_BEHIND, NEAREST_OUTPUTS, MaterialTerms, NearestHits, OCCLUSION_MAX_TABLE, SH_MAX_BANDS, TEXEL_OUTPUTS, TEXELS_MAX_POINTS, TEXELS_MAX_SIDE, U32, U64, Batch, Interpolation,  # noqa: F401
                      Overflow, PointLights, ProbeGrid, ProbeVisibility, SurfaceTexels, _check_rows, _check_vec, _depth_res, _dilate_args, _filter_args, _is_tensor, _material_args, _n_of, _np_floats,
                      _occlusion_tables, _point_lights, _probe_grid, _probe_lattice, _probe_visibility, _sh_bands, _texel_lattice, np_ptr, upload)
from .restated import (FILTER_TAPS, SALT_GATHER, SALT_OCCLUSION, SH_COSINE_LOBE, SH_K, _rng_hash, _rng_mix, _sh_terms, _texel_edge, camera_rays, dilate_texels_ref,  # noqa: F401
                       filter_texels_ref, gather_ray_keys, hemisphere_dirs, irradiance_points_ref, light_rays, lightmap_sample_ref, material_points_ref, nearest_box_bound_ref, nearest_points_ref, occlusion_rays, oct_texel, probe_depth_ref, probe_grid_positions, PROBE_NO_DIR, rotation_table, sh_basis, sh_fold_ref, sh_irradiance,
                       sphere_dirs, surface_texels_ref, texel_coords)


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
                m.vertices = np_ptr(geom.points)
                m.uvs = np_ptr(geom.uvs)
                m.indices = np_ptr(geom.indices)
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


class BatchCalls:
    """The batch calls as methods of a scene — anything with device_handle() (and, for gather_maps_points, .descriptor): Scene and scenefile.FileScene inherit them.
    Each forwards to the module-level function of the same name, resolved when it is called."""

    def cast_rays(self, origins, dirs, max_toi=None, unordered=False, want=("normal", "uv", "prim", "flags")):
        """The closest hits of caller-supplied rays on this scene: closest_hits(self, ...)."""
        return closest_hits(self, origins, dirs, max_toi, unordered, want)

    def shade_points(self, points, normals, view_dirs, nodes, uvs=None, hit_flags=None, keys=None):
        """The direct lighting of caller-supplied surface points of this scene: shade_points(self, ...)."""
        return shade_points(self, points, normals, view_dirs, nodes, uvs, hit_flags, keys)

    def material_points(self, nodes, normals=None, uvs=None, hit_flags=None, want=("ambient", "diffuse")):
        """The material terms at caller-supplied surface points of this scene, without the lights: material_points(self, ...)."""
        return material_points(self, nodes, normals, uvs, hit_flags, want)

    def nearest_points(self, points, max_dist=None, hit_flags=None, want=NEAREST_OUTPUTS):
        """The nearest surface of this scene to caller-supplied points: nearest_points(self, ...)."""
        return nearest_points(self, points, max_dist, hit_flags, want)

    def probe_clearance(self, positions, max_dist=None):
        """The distance from probe positions to this scene's nearest surface, and whether they lie behind it: probe_clearance(self, ...)."""
        return probe_clearance(self, positions, max_dist)

    def material_hits(self, hits, want=("ambient", "diffuse")):
        """The material terms at the closest hits of caller-supplied rays on this scene: material_hits(self, hits, ...)."""
        return material_hits(self, hits, want)

    def texel_albedo(self, node, width, height, flip_normals=False, device=None):
        """The diffuse reflectance of mesh node `node` at a light map's texels, the albedo bake_bounces takes: texel_albedo(self, node, ...)."""
        return texel_albedo(self, node, width, height, flip_normals, device)

    def indirect_points(self, points, normals, nodes, grid, uvs=None, hit_flags=None, facing=False, visibility=None):
        """The diffuse light a probe grid gives surface points of this scene: indirect_points(self, ...)."""
        return indirect_points(self, points, normals, nodes, grid, uvs, hit_flags, facing, visibility)

    def occlusion_points(self, points, normals, sample_dirs, rotations=None, bias=1e-3, max_toi=math.inf, hit_flags=None, keys=None):
        """Ambient occlusion at caller-supplied surface points of this scene: occlusion_points(self, ...)."""
        return occlusion_points(self, points, normals, sample_dirs, rotations, bias, max_toi, hit_flags, keys)

    def light_points(self, points, normals, lights, hit_flags=None, want_counts=True):
        """The direct light of a caller-supplied table of point lights at caller-supplied surface points of this scene: light_points(self, ...)."""
        return light_points(self, points, normals, lights, hit_flags, want_counts)

    def gather_points(self, points, normals, sample_dirs, rotations=None, bias=1e-3, energy=1.0, max_depth=0, hit_flags=None, keys=None, unordered=False):
        """The incoming light at caller-supplied surface points of this scene: gather_points(self, ...)."""
        return gather_points(self, points, normals, sample_dirs, rotations, bias, energy, max_depth, hit_flags, keys, unordered)

    def gather_sh_points(self, points, normals, sample_dirs, rotations=None, bias=1e-3, energy=1.0, max_depth=0, bands=3, hit_flags=None, keys=None, unordered=False):
        """The incoming light at caller-supplied points of this scene as spherical harmonics: gather_sh_points(self, ...)."""
        return gather_sh_points(self, points, normals, sample_dirs, rotations, bias, energy, max_depth, bands, hit_flags, keys, unordered)

    def gather_probes(self, positions, sample_dirs, bands=3, energy=1.0, max_depth=0, keys=None, unordered=True):
        """Irradiance probes at free points of this scene: gather_probes(self, ...)."""
        return gather_probes(self, positions, sample_dirs, bands, energy, max_depth, keys, unordered)

    def irradiance_points(self, points, normals, grid, facing=False, hit_flags=None, want_sh=False, want_weight=False, visibility=None):
        """The irradiance at caller-supplied points from a grid of SH probes, on this scene's GPU: irradiance_points(self, ...)."""
        return irradiance_points(self, points, normals, grid, facing, hit_flags, want_sh, want_weight, visibility)

    def probe_depth_points(self, points, normals, sample_dirs, res=8, max_dist=None, near_dist=0.0, rotations=None, bias=1e-3, hit_flags=None, keys=None,
                           want=("counts", "nearest", "nearest_dir")):
        """The depth moments, near / miss counts and nearest hit of the rays of caller-supplied points of this scene: probe_depth_points(self, ...)."""
        return probe_depth_points(self, points, normals, sample_dirs, res, max_dist, near_dist, rotations, bias, hit_flags, keys, want)

    def probe_depth(self, positions, sample_dirs, res=8, max_dist=None, near_dist=0.0, keys=None, want=("counts", "nearest", "nearest_dir")):
        """What probes at free points of this scene see of its geometry: probe_depth(self, ...)."""
        return probe_depth(self, positions, sample_dirs, res, max_dist, near_dist, keys, want)

    def bake_probe_visibility(self, grid, sample_dirs, res=8, max_dist=None, near_dist=None, max_near_fraction=0.25, floor=0.05, bias=0.0):
        """The depth moments and validity words of a grid of probes of this scene: bake_probe_visibility(self, grid, ...)."""
        return bake_probe_visibility(self, grid, sample_dirs, res, max_dist, near_dist, max_near_fraction, floor, bias)

    def bake_probe_grid(self, origin, cell, counts, sample_dirs, bands=3, energy=1.0, max_depth=0, keys=None, unordered=True, valid=None, measure=4.0 * math.pi, device=None):
        """A grid of irradiance probes of this scene: bake_probe_grid(self, ...)."""
        return bake_probe_grid(self, origin, cell, counts, sample_dirs, bands, energy, max_depth, keys, unordered, valid, measure, device)

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

    def gather_maps_sh_points(self, points, normals, sample_dirs, maps, node_map, bands=3, rotations=None, bias=1e-3, max_toi=math.inf, miss=(0.0, 0.0, 0.0), hit_flags=None,
                              keys=None, depth=None, want=("counts", "depth_counts", "nearest", "nearest_dir")):
        """The light of baked maps at caller-supplied points of this scene as spherical harmonics, with depth moments from the same rays: gather_maps_sh_points(self, ...)."""
        return gather_maps_sh_points(self, points, normals, sample_dirs, maps, node_map, bands, rotations, bias, max_toi, miss, hit_flags, keys, depth, want)

    def gather_maps_probes(self, positions, sample_dirs, maps, node_map, bands=3, max_toi=math.inf, miss=(0.0, 0.0, 0.0), keys=None, depth=None,
                           want=("counts", "depth_counts", "nearest", "nearest_dir")):
        """Irradiance probes at free points of this scene, filled from baked maps: gather_maps_probes(self, ...)."""
        return gather_maps_probes(self, positions, sample_dirs, maps, node_map, bands, max_toi, miss, keys, depth, want)

    def bake_probe_grid_maps(self, origin, cell, counts, sample_dirs, maps, node_map, bands=3, miss=(0.0, 0.0, 0.0), visibility=None, measure=4.0 * math.pi, device=None):
        """A grid of irradiance probes of this scene filled from baked maps, with its visibility from the same rays: bake_probe_grid_maps(self, ...)."""
        return bake_probe_grid_maps(self, origin, cell, counts, sample_dirs, maps, node_map, bands, miss, visibility, measure, device)

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


class Scene(BatchCalls):
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
    abi.check(lib.nrays_render(scene.device_handle(), C.byref(p), np_ptr(out)))
    return out


def cast_rays(scene, origins, dirs):
    """The closest-hit query of Scene::trace (src/scene.rs:164-166) on caller-supplied rays, by the HIP traversal and
    intersectors alone (nrays_debug_cast_batch).  Returns (hit mask, (n, 8) array of toi, nx, ny, nz, has_uv, u, v, node) —
    the layout of oracle.cast."""
    o = np.ascontiguousarray(origins, dtype=np.float64).reshape(-1, 3)
    d = np.ascontiguousarray(dirs, dtype=np.float64).reshape(-1, 3)
    n = len(o)
    res = (abi.NraysCastResult * max(n, 1))()
    abi.check(abi.load_hip_lib().nrays_debug_cast_batch(scene.device_handle(), 0, n, np_ptr(o),
                                                        np_ptr(d), None, res))
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
    abi.check(abi.load_hip_lib().nrays_debug_cast_batch(scene.device_handle(), 1, n, np_ptr(o),
                                                        np_ptr(d), np_ptr(t), res))
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

def trace_rays(scene, origins, dirs, refr=None, energy=None, keys=None, max_depth=0, unordered=False):
    """Scene::trace (src/scene.rs:163-193) on n caller-supplied rays: the colour of each, with the reflection / refraction recursion
    and the lights of a render.  `origins`, `dirs`: (n, 3); `refr` (n,) refraction index of the medium the ray is in (default 1.0),
    `energy` (n,) (default 1.0), `keys` (n,) RNG path keys for area-light sampling (default: ray i has key i); directions are used as
    given (unit length expected).  `max_depth` as in render().
    `unordered=True` (NRAYS_RAYS_UNORDERED) says that the rays come in no useful order — AO / baking rays, shuffled or gathered rays: the
    library may then bin them by a spatial key and trace them in that order.  The colours are bit-identical either way; only the time changes.
    numpy arrays -> nrays_trace_rays (blocking), (n, 3) float32 numpy array.  torch tensors on the scene's GPU (float64, energy float32,
    keys int64 / uint64) -> nrays_trace_rays_device on torch's current stream, (n, 3) float32 tensor."""
    n = _n_of(origins, dirs)
    for name, a in (("refr", refr), ("energy", energy), ("keys", keys)):
        _check_vec(name, a, n)
    if int(max_depth) < 0 or int(max_depth) >= 1 << 32:
        raise ValueError("max_depth must be in [0, 2^32)")
    b = Batch((("origins", origins, F64), ("dirs", dirs, F64), ("refr", refr, F64), ("energy", energy, F32), ("keys", keys, U64)), (("rgb", (n, 3), F32),))
    b.call(scene, "nrays_trace_rays", n, *b.pin, int(max_depth), *b.pout, *((abi.RAYS_UNORDERED,) if unordered else ()), ex=unordered)
    return b.outs[0]


def intersects_rays(scene, origins, dirs, max_toi, unordered=False):
    """Scene::intersects_ray (src/scene.rs:147-161) on n caller-supplied rays, through nrays_intersects_rays_device: returns
    (lit mask, (n, 3) float32 colour filters) — lit where the reference returns Some(filter); the filter is (0, 0, 0) elsewhere.
    numpy arrays in -> numpy out (blocking); torch tensors on the GPU (float64) -> tensors (bool, float32) on torch's current stream.
    `unordered=True`: as for trace_rays (nrays_intersects_rays_device_ex with NRAYS_RAYS_UNORDERED); the results are bit-identical."""
    n = _n_of(origins, dirs)
    _check_vec("max_toi", max_toi, n)
    if max_toi is None:
        raise ValueError("max_toi must be floating point, got object")
    host = not _is_tensor(origins)  # the ABI has no blocking form: numpy rays go to the current GPU and the answer comes back
    b = Batch((("origins", origins, F64), ("dirs", dirs, F64), ("max_toi", max_toi, F64)), (("filter", (n, 3), F32), ("lit", (n,), I32)), device=CURRENT)
    b.call(scene, "nrays_intersects_rays", n, *b.pin, *b.pout, *((abi.RAYS_UNORDERED,) if unordered else ()), ex=unordered)
    filt, lit = b.outs
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
    nrays_cast_rays_device on torch's current stream, tensors (flags int32)."""
    n = _n_of(origins, dirs)
    _check_vec("max_toi", max_toi, n)
    want = tuple(want)
    for name in want:
        if name not in CAST_OUTPUTS:
            raise ValueError("want: unknown output %r (one of %s)" % (name, ", ".join(CAST_OUTPUTS)))
    b = Batch((("origins", origins, F64), ("dirs", dirs, F64), ("max_toi", max_toi, F64)),
              (("toi", (n,), F64), ("node", (n,), I32), ("normal", (n, 3), F64, "normal" in want), ("uv", (n, 2), F64, "uv" in want), ("prim", (n,), I32, "prim" in want),
               ("flags", (n,), U32, "flags" in want)))
    b.call(scene, "nrays_cast_rays", n, *b.pin, *b.pout, abi.RAYS_UNORDERED if unordered else 0)
    return CastHits(*b.outs)


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
    uint32; keys int64 / uint64) -> nrays_shade_points_device on torch's current stream, tensor."""
    n = _n_of(points, normals, ("points", "normals"))
    for name, a in (("view_dirs", view_dirs), ("nodes", nodes)):
        if a is None:
            raise ValueError("%s is required" % name)
    _check_rows("view_dirs", view_dirs, n, 3)
    if uvs is not None:
        _check_rows("uvs", uvs, n, 2)
    for name, a in (("nodes", nodes), ("hit_flags", hit_flags), ("keys", keys)):
        _check_vec(name, a, n)
    b = Batch((("points", points, F64), ("normals", normals, F64), ("view_dirs", view_dirs, F64), ("uvs", uvs, F64), ("nodes", nodes, I32), ("hit_flags", hit_flags, U32),
               ("keys", keys, U64)), (("rgba", (n, 4), F32),))
    b.call(scene, "nrays_shade_points", n, *b.pin, *b.pout, 0)
    return b.outs[0]


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


# ---- the material terms at caller-supplied points, without the lights (include/nrays_abi.h: nrays_material_points_device) -----------------------------

def material_points(scene, nodes, normals=None, uvs=None, hit_flags=None, want=("ambient", "diffuse")):
    """The terms of the materials at n caller-supplied surface points WITHOUT the lights, through nrays_material_points_device / nrays_material_points: what
    shade_points folds into one colour, handed out.  Per point, with the material of scene node nodes[i]:
      ambient  (n, 4) float32: Material::ambiant (src/material.rs:7) — ka times the colour texture's sample, the opacity map's sample (or 1) in w; the Normal
               and UV materials' colour;
      diffuse  (n, 3) float32: kd times the colour texture's sample — the diffuse reflectance (albedo) of the point; zeros for the Normal and UV materials;
      specular (n, 4) float32: (ks, shininess); zeros for the Normal and UV materials;
      node     (n, 4) float64: the node's (alpha, refl_mix, refl_atenuation, refr_coeff), the constants Scene::trace reads at a hit.
    `want`: which of them to compute into memory (at least one); the colour texture is sampled once for ambient and diffuse together.  With closest_hits()
    this is all an integrator of the caller's own needs on top of the library's traversal.  Also `scene.material_points(...)` on Scene and FileScene;
    material_hits() feeds it from closest_hits(); material_points_ref() restates it bit for bit.
    `nodes` (n,) integers.  `normals` (n, 3), required for "ambient" (the Normal material reads it), else optional.  `uvs` (n, 2) or None (no point has a uv).
    `hit_flags` (n,) integers or None: the flag words of closest_hits — bit 0 clear: the point is skipped, bit 1: it carries a uv; None: every point is live
    and has a uv exactly when `uvs` is given.  A skipped point — flag bit 0 clear, node < 0 or >= the scene's node count — is zeros in every output.
    Returns MaterialTerms(ambient, diffuse, specular, node), None for what was not asked for.
    numpy arrays -> nrays_material_points (blocking), numpy arrays.  torch tensors on the scene's GPU (nodes int32; normals / uvs float64; hit_flags int32 /
    uint32) -> nrays_material_points_device on torch's current stream, tensors."""
    n, want = _material_args(nodes, normals, uvs, hit_flags, want)
    b = Batch((("nodes", nodes, I32), ("normals", normals, F64), ("uvs", uvs, F64), ("hit_flags", hit_flags, U32)),
              (("ambient", (n, 4), F32, "ambient" in want), ("diffuse", (n, 3), F32, "diffuse" in want), ("specular", (n, 4), F32, "specular" in want),
               ("node", (n, 4), F64, "node" in want)))
    b.call(scene, "nrays_material_points", n, b.pin[1], b.pin[2], b.pin[0], b.pin[3], *b.pout, 0)
    return MaterialTerms(*b.outs)


# ---- the nearest surface to caller-supplied points (include/nrays_abi.h: nrays_nearest_points_device) -----------------------------------------------

def nearest_points(scene, points, max_dist=None, hit_flags=None, want=NEAREST_OUTPUTS):
    """The nearest surface to n caller-supplied points, through nrays_nearest_points_device / nrays_nearest_points: how far it is, where, and on which node and
    triangle — the question the ray families cannot answer (probe clearance, transfer of baked light to points off the surface, distance fields).  A
    distance-pruned walk of both BVH levels, one lane a point; the result is the header's definition, restated bit for bit by nearest_points_ref().  Also
    `scene.nearest_points(...)` on Scene and FileScene.
    `points` (n, 3).  `max_dist` (n,) or None: the unbounded answer where its distance <= max_dist[i], a miss otherwise (NaN or negative: a miss).  `hit_flags` (n,)
    integers or None: bit 0 clear skips the point (the miss record; its coordinates may hold anything).  `want`: which of "point", "normal", "uv", "prim", "flags"
    to compute into memory.
    Returns NearestHits(dist (n,) f64, node (n,) i32, point (n, 3) f64, normal (n, 3) f64, uv (n, 2) f64, prim (n,) i32, flags (n,)), None for what was not wanted:
    closest_hits' record with `dist` for `toi`, plus `point`, so that point / normal / node / uv / flags pass unfiltered into shade_points, material_points,
    occlusion_points, the gather families and irradiance_points.  A miss has node -1, dist +inf, zeros, prim -1, flags 0; flags bit 0 = found, bit 1 = the record
    carries a uv, bit 2 (NEAREST_BEHIND) = the point lies behind the surface.  The normal faces the point.
    numpy arrays -> nrays_nearest_points (blocking), numpy arrays (flags uint32).  torch tensors on the scene's GPU (float64; hit_flags int32 / uint32) ->
    nrays_nearest_points_device on torch's current stream, tensors (flags int32)."""
    if points is None:
        raise ValueError("points is required")
    _check_rows("points", points, int(points.shape[0]) if len(points.shape) else 0, 3)
    n = int(points.shape[0])
    if n >= 1 << 32:
        raise ValueError("at most 2^32 - 1 points per call")
    _check_vec("max_dist", max_dist, n)
    _check_vec("hit_flags", hit_flags, n)
    want = tuple(want)
    for name in want:
        if name not in NEAREST_OUTPUTS:
            raise ValueError("want: unknown output %r (one of %s)" % (name, ", ".join(NEAREST_OUTPUTS)))
    b = Batch((("points", points, F64), ("max_dist", max_dist, F64), ("hit_flags", hit_flags, U32)),
              (("dist", (n,), F64), ("node", (n,), I32), ("point", (n, 3), F64, "point" in want), ("normal", (n, 3), F64, "normal" in want), ("uv", (n, 2), F64, "uv" in want),
               ("prim", (n,), I32, "prim" in want), ("flags", (n,), U32, "flags" in want)))
    b.call(scene, "nrays_nearest_points", n, *b.pin, *b.pout, 0)
    return NearestHits(*b.outs)


ProbeClearance = collections.namedtuple("ProbeClearance", ("dist", "behind"))


def probe_clearance(scene, positions, max_dist=None):
    """What a probe's validity and relocation should rest on: per probe position the distance to the scene's nearest surface (+inf beyond `max_dist`, a scalar or
    None) and whether the position lies behind it (flag bit 2 of nearest_points: inside a closed shape, under a plane, on the back of a triangle's winding).
    probe_depth() reports the nearest of its SAMPLED rays and misses what lies between them; this does not sample.  The rule stays the caller's
    (probe_valid_words is unchanged).  Returns ProbeClearance(dist (n,) float64, behind (n,) bool), numpy or torch as `positions`."""
    n = int(positions.shape[0])
    md = None
    if max_dist is not None:
        if _is_tensor(positions):
            import torch
            md = torch.full((n,), float(max_dist), dtype=torch.float64, device=positions.device)
        else:
            md = np.full(n, float(max_dist), np.float64)
    hits = nearest_points(scene, positions, md, want=("flags",))
    return ProbeClearance(hits.dist, (hits.flags & NEAREST_BEHIND) != 0)


def nearest_bound_probe(points, boxes):
    """nearest_box_bound of the device (nrays_debug_nearest_bound), points x boxes: (n, m) float64.  nearest_box_bound_ref() is its mirror."""
    P = np.ascontiguousarray(np.asarray(points, np.float64).reshape(-1, 3))
    B = np.ascontiguousarray(np.asarray(boxes, np.float64).reshape(-1, 6))
    out = np.zeros((len(P), len(B)), np.float64)
    abi.check(abi.load_hip_lib().nrays_debug_nearest_bound(len(P), len(B), np_ptr(P), np_ptr(B), np_ptr(out)))
    return out


def material_hits(scene, hits, want=("ambient", "diffuse")):
    """The material terms at the closest hits of caller-supplied rays: material_points() at `hits = closest_hits(scene, origins, dirs)` (a CastHits with uv and
    flags, and normal when "ambient" is wanted).  Misses come back as zeros.  MaterialTerms, numpy or torch as the hits."""
    for name in ("uv", "flags") + (("normal",) if not isinstance(want, str) and "ambient" in tuple(want) else ()):
        if getattr(hits, name) is None:
            raise ValueError("material_hits: hits.%s is None (closest_hits must be asked for it)" % name)
    return material_points(scene, hits.node, hits.normal, hits.uv, hits.flags, want)


def texel_albedo(scene, node, width, height, flip_normals=False, device=None):
    """The diffuse reflectance of TriMesh node `node` at the texels of a width x height light map — the `albedo` array bake_bounces() takes —, (height, width, 3)
    float32 in NraysTexture row order (row 0 = the bottom row): material_points(want=("diffuse",)) on surface_texels() on the default lattice, the one
    Texture2d::sample reads, two calls on one stream.  Texels no triangle covers are zeros.  `flip_normals`, `device`: as for surface_texels (with a torch device
    the array stays on the GPU as a tensor).  Also `scene.texel_albedo(node, ...)` on Scene and FileScene."""
    width, height = _texel_lattice(width, height)
    tx = surface_texels(scene, node, width, height, False, flip_normals, want=("uv", "node"), device=device)
    return material_points(scene, tx.node, None, tx.uv, tx.flags, want=("diffuse",)).diffuse.reshape(height, width, 3)


INV_PI_F32 = float(np.float32(0.3183098861837907))  # the float32 nearest 1 / pi


def indirect_points(scene, points, normals, nodes, grid, uvs=None, hit_flags=None, facing=False, visibility=None):
    """The diffuse light a probe grid gives n surface points, (n, 3) float32: the irradiance E = irradiance_points(points, normals, grid, facing, hit_flags,
    visibility=visibility) reflected by the surface's own diffuse reflectance d = material_points(nodes, uvs=uvs, hit_flags=hit_flags, want=("diffuse",)) —
    a Lambertian surface's radiance, in float32, each product rounded: (d * E) * float32(0.3183098861837907).  Two calls on one stream and two element-wise
    products; the numpy and the torch form are the same expression.  A skipped point (flag bit 0 clear, node outside the scene) gives zeros.  Arguments as for
    irradiance_points and material_points.  Also `scene.indirect_points(...)` on Scene and FileScene."""
    n = _n_of(points, normals, ("points", "normals"))
    if nodes is not None:
        _check_vec("nodes", nodes, n)
    _material_args(nodes, None, uvs, hit_flags, ("diffuse",))
    E =irradiance_points(scene, points, normals, grid, facing, hit_flags, visibility=visibility)
    d = material_points(scene, nodes, None, uvs, hit_flags, want=("diffuse",)).diffuse
    return (d * E) * INV_PI_F32


# ---- ambient occlusion at caller-supplied points: the hemisphere rays are built on the device (include/nrays_abi.h: NraysOcclusionParams) ----------

Occlusion = collections.namedtuple("Occlusion", ("filter", "open"))


def _point_batch(points, normals, hit_flags, keys, L, rot, outs, more=()):
    """The columns every call at surface points shares — its first four arguments — and the two tables of its params struct, which may be numpy next to tensors."""
    return Batch((("points", points, F64), ("normals", normals, F64), ("hit_flags", hit_flags, U32), ("keys", keys, U64), ("sample_dirs", L, F64, True),
                  ("rotations", rot, F64, True)) + more, outs)


def _tables(b):
    """The first four fields of the params structs: the tables' row counts and addresses."""
    L, rot = b.ins[4], b.ins[5]
    return len(L), 0 if rot is None else len(rot), b.addr(L), b.addr(rot)


def occlusion_ray_probe(scene, points, normals, sample_dirs, rotations=None, bias=1e-3, keys=None):
    """Test probe (nrays_debug_occlusion_rays): the rays as the library's own generator — the device function k_occlusion_points traces — builds them,
    in occlusion_rays()' layout.  numpy arrays, blocking."""
    n = _n_of(points, normals, ("points", "normals"))
    _check_vec("keys", keys, n)
    L, rot, bias, _ = _occlusion_tables(sample_dirs, rotations, bias, math.inf)
    b = _point_batch(points, normals, None, keys, L, rot, (("origins", (n, len(L), 3), F64), ("dirs", (n, len(L), 3), F64)))
    params = abi.NraysOcclusionParams(*_tables(b), bias, math.inf)
    b.call(scene, "nrays_debug_occlusion_rays", n, b.pin[0], b.pin[1], b.pin[3], C.byref(params), *b.pout)
    return tuple(b.outs)


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
    int64 / uint64; the tables tensors or anything numpy takes) -> nrays_occlusion_points_device on torch's current stream, tensors (open int32)."""
    n = _n_of(points, normals, ("points", "normals"))
    for name, a in (("hit_flags", hit_flags), ("keys", keys)):
        _check_vec(name, a, n)
    L, rot, bias, max_toi = _occlusion_tables(sample_dirs, rotations, bias, max_toi)
    b = _point_batch(points, normals, hit_flags, keys, L, rot, (("filter", (n, 3), F32), ("open", (n,), U32)))
    params = abi.NraysOcclusionParams(*_tables(b), bias, max_toi)
    b.call(scene, "nrays_occlusion_points", n, *b.pin[:4], C.byref(params), *b.pout, 0)
    return Occlusion(*b.outs)


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


# ---- direct light at caller-supplied points from a caller-supplied table of point lights (include/nrays_abi.h: NraysPointLights) ------------------------------

PointLighting = collections.namedtuple("PointLighting", ("rgb", "counts"))


def _light_batch(points, normals, hit_flags, lights, outs):
    """The columns of a call with a light table — points, normals, flags, then the three tables of the params struct, which may be numpy next to tensors — and the
    struct's settings."""
    pos, col, en, flags, bias, offset, min_dist = _point_lights(lights)
    b = Batch((("points", points, F64), ("normals", normals, F64), ("hit_flags", hit_flags, U32), ("lights.positions", pos, F64, True), ("lights.colors", col, F32, True),
               ("lights.normals", en, F64, True)), outs)
    return b, abi.NraysPointLights(len(pos), flags, b.addr(b.ins[3]), b.addr(b.ins[4]), b.addr(b.ins[5]), bias, offset, min_dist)


def light_ray_probe(scene, points, normals, lights):
    """Test probe (nrays_debug_light_rays): the shadow rays and weights as the library's own generator — the device function k_light_points traces — builds them, in
    light_rays()' layout.  numpy arrays, blocking."""
    n = _n_of(points, normals, ("points", "normals"))
    m = len(_point_lights(lights)[0])
    b, params = _light_batch(points, normals, None, lights, (("origins", (n, m, 3), F64), ("dirs", (n, m, 3), F64), ("t_max", (n, m), F64), ("w", (n, m), F32)))
    b.call(scene, "nrays_debug_light_rays", n, b.pin[0], b.pin[1], C.byref(params), *b.pout)
    return tuple(b.outs)


def light_points(scene, points, normals, lights, hit_flags=None, want_counts=True):
    """The direct light of a caller-supplied table of point lights at n caller-supplied surface points, through nrays_light_points_device / nrays_light_points: per
    point the library builds the shadow ray towards every light ON THE DEVICE (light_rays() restates them bit for bit), weights it with the cosine at the point — for
    lights with emitter normals also the emitter's cosine, with `inverse_square` the falloff —, runs Scene::intersects_ray — the query of intersects_rays() — on the
    rays whose weight is > 0 and sums colour * (filter * weight) over the open ones in the order of the table: PointLighting(rgb (n, 3) float32, counts (n, 2) — the
    lights that got a ray and the open ones among them; None without `want_counts`).  A light behind the surface costs nothing, the scene's own lights are not read
    (scene_point_lights() makes a table of them), and no ray or per-ray result is ever in memory.  Also `scene.light_points(...)` on Scene and FileScene; light_hits()
    feeds it from closest_hits(), vpls_from_hits() makes virtual point lights for it.
    `points`, `normals`: (n, 3), used as given (unit normals, pointing to the lit side).  `lights`: a PointLights.  `hit_flags` (n,) integers or None: the flag words of
    closest_hits / surface_texels — bit 0 clear: the point is skipped (zeros; its point and normal may hold anything).
    numpy arrays -> nrays_light_points (blocking), numpy arrays (counts uint32).  torch tensors on the scene's GPU (float64; hit_flags int32 / uint32; the tables
    tensors — colours float32 — or anything numpy takes) -> nrays_light_points_device on torch's current stream, tensors (counts int32)."""
    n = _n_of(points, normals, ("points", "normals"))
    _check_vec("hit_flags", hit_flags, n)
    b, params = _light_batch(points, normals, hit_flags, lights, (("rgb", (n, 3), F32), ("counts", (n, 2), U32, bool(want_counts))))
    b.call(scene, "nrays_light_points", n, *b.pin[:3], C.byref(params), *b.pout, 0)
    return PointLighting(*b.outs)


def light_points_ref(scene, points, normals, lights, hit_flags=None):
    """The definition of light_points from parts that existed before it, bit for bit: the mirror's rays (light_rays()) with a weight > 0 and a t_max > 0 through
    intersects_rays(), and the fold of the header in numpy float32 in the order of the lights.  numpy arrays; PointLighting(rgb, counts uint32)."""
    ro, rd, t_max, w = light_rays(points, normals, lights)
    col = _point_lights(lights)[1]
    n, m = w.shape
    live = np.ones(n, bool) if hit_flags is None else (np.asarray(hit_flags).astype(np.uint32) & 1) != 0
    ray = (w > 0) & live[:, None]
    traced = ray & (t_max > 0.0)
    open_, filt = ray.copy(), np.ones((n, m, 3), np.float32)
    if traced.any():
        lit, f = intersects_rays(scene, np.ascontiguousarray(ro[traced]), np.ascontiguousarray(rd[traced]), np.ascontiguousarray(t_max[traced]))
        open_[traced], filt[traced] = lit, f
    total = np.zeros((n, 3), np.float32)
    with np.errstate(all="ignore"):
        for k in range(m):
            c = col[k][None, :] * (filt[:, k] * w[:, k, None])
            total = np.where(open_[:, k, None], total + c, total)
    return PointLighting(total, np.stack([ray.sum(axis=1), open_.sum(axis=1)], axis=1).astype(np.uint32))


def light_hits(scene, origins, dirs, hits, lights, want_counts=True):
    """The direct light of a table of point lights at the closest hits of caller-supplied rays: light_points() at the hits of `hits = closest_hits(scene, origins,
    dirs)` (a CastHits with normal and flags), on the side the rays came from — the points and normals of occlusion_hits(), built the same way.  Misses come back as
    zeros.  numpy or torch as the inputs."""
    points, normals = _hit_points("light_hits", origins, dirs, hits)
    return light_points(scene, points, normals, lights, hit_flags=hits.flags, want_counts=want_counts)


def scene_point_lights(scene, **kw):
    """The scene's own lights of radius 0 as a PointLights (positions float64, colours float32, no emitter normals); `kw`: its other fields.  With bias=0 and
    offset=1e-3 light_points() then computes what shade_points() computes for a Phong node of ambient 0, diffuse (1, 1, 1), specular 0 and no texture, bit for bit."""
    d = scene.descriptor.desc
    rows = [d.lights[i] for i in range(d.num_lights) if d.lights[i].radius == 0.0]
    if not rows:
        raise ValueError("the scene has no light of radius 0")
    return PointLights(np.asarray([tuple(r.pos) for r in rows], np.float64), np.asarray([tuple(r.color) for r in rows], np.float32), None, **kw)


def vpls_from_hits(origins, dirs, hits, diffuse, power, **kw):
    """Virtual point lights (instant radiosity, Keller 1997) from the closest hits of caller-supplied rays: every hit (flags bit 0) becomes a light at the hit point
    — origins + dirs * toi, as occlusion_hits() builds it —, with the normal on the side the ray came from as its emitter normal and the colour
    float32(power) * diffuse[i]; misses make no light.  `diffuse` (n, 3) float32: the surface's diffuse reflectance, material_hits(want=("diffuse",)).diffuse.  `power`:
    what one VPL carries, e.g. the light's colour scale / (pi * paths).  `kw`: the other fields of the PointLights (inverse_square=True for a physical falloff).  The
    chain, every step on the device:
        hits = closest_hits(scene, origins, dirs)                                  # where the light's paths land
        diffuse = material_hits(scene, hits, want=("diffuse",)).diffuse             # what the surface there reflects
        vpls = vpls_from_hits(origins, dirs, hits, diffuse, power, inverse_square=True)
        indirect = light_points(scene, points, normals, vpls).rgb                  # one bounce at the points to be lit
    numpy or torch as the inputs; at most 4096 lights a table (split the hits otherwise)."""
    points, normals = _hit_points("vpls_from_hits", origins, dirs, hits)
    _check_rows("diffuse", diffuse, int(points.shape[0]), 3)
    if _is_tensor(points) != _is_tensor(diffuse):
        raise ValueError("torch tensors and numpy arrays cannot be mixed in one call")
    hit = (hits.flags & 1) != 0
    if _is_tensor(points):
        colors = diffuse.float() * float(np.float32(power))
    else:
        colors = np.float32(power) * np.asarray(diffuse, np.float32)
    return PointLights(points[hit], colors[hit], normals[hit], **kw)


# ---- incoming light at caller-supplied points (include/nrays_abi.h: nrays_gather_points_device) ------------------------------------------------------------


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
    the tables tensors or anything numpy takes) -> nrays_gather_points_device on torch's current stream, a tensor."""
    if not isinstance(unordered, (bool, np.bool_)):
        raise ValueError("unordered must be True or False, got %r" % (unordered,))
    n = _n_of(points, normals, ("points", "normals"))
    for name, a in (("hit_flags", hit_flags), ("keys", keys)):
        _check_vec(name, a, n)
    L, rot, bias, _ = _occlusion_tables(sample_dirs, rotations, bias, math.inf)
    energy, max_depth = _gather_settings(energy, max_depth)
    b = _point_batch(points, normals, hit_flags, keys, L, rot, (("rgb", (n, 3), F32),))
    params = abi.NraysGatherParams(*_tables(b), bias, energy, max_depth)
    b.call(scene, "nrays_gather_points", n, *b.pin[:4], C.byref(params), *b.pout, abi.RAYS_UNORDERED if unordered else 0, ex=unordered)
    return b.outs[0]


def gather_hits(scene, origins, dirs, hits, sample_dirs, rotations=None, bias=1e-3, energy=1.0, max_depth=0, keys=None, unordered=False):
    """The incoming light at the closest hits of caller-supplied rays: gather_points() at the hits of `hits = closest_hits(scene, origins, dirs)` (a CastHits
    with normal and flags), on the side the rays came from — the points and normals of occlusion_hits(), built the same way.  Misses come back as zeros.
    numpy or torch as the inputs.  `unordered`: as for gather_points."""
    points, normals = _hit_points("gather_hits", origins, dirs, hits)
    return gather_points(scene, points, normals, sample_dirs, rotations, bias, energy, max_depth, hit_flags=hits.flags, keys=keys, unordered=unordered)


# ---- gathered light kept by direction: spherical harmonics per point, irradiance probes (include/nrays_abi.h: nrays_gather_sh_points_device) ----------------


def _gather_sh_call(scene, points, normals, sample_dirs, rotations, bias, energy, max_depth, bands, hit_flags, keys, unordered):
    if not isinstance(unordered, (bool, np.bool_)):
        raise ValueError("unordered must be True or False, got %r" % (unordered,))
    bands = _sh_bands(bands)
    n = _n_of(points, normals, ("points", "normals"))
    for nm_, a in (("hit_flags", hit_flags), ("keys", keys)):
        _check_vec(nm_, a, n)
    L, rot, bias, _ = _occlusion_tables(sample_dirs, rotations, bias, math.inf)
    energy, max_depth = _gather_settings(energy, max_depth)
    b = _point_batch(points, normals, hit_flags, keys, L, rot, (("sh", (n, bands * bands, 3), F32),))
    params = abi.NraysGatherParams(*_tables(b), bias, energy, max_depth)
    b.call(scene, "nrays_gather_sh_points", n, *b.pin[:4], C.byref(params), bands, *b.pout, abi.RAYS_UNORDERED if unordered else 0)
    return b.outs[0]


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
    b = _point_batch(points, normals, hit_flags, keys, L, rot, (("sh", (n, bands * bands, 3), F32),), (("ray_colours", col, F32),))
    params, ms = abi.NraysGatherParams(*_tables(b), bias, 1.0, 0), C.c_float(0.0)
    b.call(scene, "nrays_debug_gather_sh_fold", n, *b.pin[:4], C.byref(params), bands, b.pin[6], *b.pout, C.byref(ms) if want_ms else None)
    return (b.outs[0], float(ms.value)) if want_ms else b.outs[0]


# ---- the consumer of the probes: irradiance at caller-supplied points from a grid of them (include/nrays_abi.h: nrays_irradiance_points_device) ---------------

Irradiance = collections.namedtuple("Irradiance", ("rgb", "sh", "weight"))


def irradiance_points(scene, points, normals, grid, facing=False, hit_flags=None, want_sh=False, want_weight=False, visibility=None):
    """The irradiance at n caller-supplied points with normals from a regular grid of SH probes — the indirect term of whatever moves through a baked scene —
    through nrays_irradiance_points_device / nrays_irradiance_points: per point the eight probes around it are blended with trilinear weights, the blend is folded
    with the cosine lobe at the normal and multiplied by grid.measure: (n, 3) float32.  irradiance_points_ref() restates it bit for bit; on a probe's position
    it is sh_irradiance() of that probe up to float32 rounding.  No ray is traced: the scene gives the GPU, the stream ordering and the staging memory.
    `grid`: a ProbeGrid — bake_probe_grid() makes one.  A point outside the grid takes the border's value.  `facing=True` (NRAYS_IRRADIANCE_FACING) multiplies a
    probe's weight by ((cos + 1) / 2)^2 + 0.2, cos between the normal and the direction to the probe: probes behind the surface count less.  grid.valid leaves
    probes out (bit 0 clear: never read, so its row may hold anything); deciding which probes are valid — inside a wall, say — is the caller's job, and
    bake_probe_visibility() / probe_valid_words() do it from what the probes see.  A point none of whose probes counts gets zeros and weight 0.
    `visibility`: None (nrays_irradiance_points*, exactly as without the keyword) or a ProbeVisibility — bake_probe_visibility() makes one — for
    nrays_irradiance_points_vis*: a valid probe whose mean depth towards the point is shorter than the point's distance is held down by Chebyshev's bound, cubed and
    kept above visibility.floor, so a point behind a wall is not lit by the probe on its other side.  Its moments follow the form of grid.sh.  `hit_flags` (n,) integers or None: bit 0 clear skips a point (zeros; its point and normal may hold anything).
    `want_sh` / `want_weight`: returns Irradiance(rgb, sh, weight) with the blended coefficients (n, bands^2, 3) and the weight sums (n,) that were asked for (None
    otherwise) instead of rgb alone.
    numpy arrays -> nrays_irradiance_points (blocking; the grid is staged once a call), numpy arrays.  torch tensors on the scene's GPU (points / normals float64;
    hit_flags int32 / uint32; grid.sh float32 and grid.valid int32 / uint32 tensors there, or numpy arrays, which are uploaded every call) ->
    nrays_irradiance_points_device on torch's current stream, tensors."""
    if not isinstance(facing, (bool, np.bool_)):
        raise ValueError("facing must be True or False, got %r" % (facing,))
    n = _n_of(points, normals, ("points", "normals"))
    _check_vec("hit_flags", hit_flags, n)
    origin, cell, counts, bands, sh, valid, measure = _probe_grid(grid)
    vis = None if visibility is None else _probe_visibility(visibility, counts[0] * counts[1] * counts[2])
    more = () if vis is None else (("visibility.moments", vis[0], F32, True),)
    b = Batch((("points", points, F64), ("normals", normals, F64), ("hit_flags", hit_flags, U32), ("grid.sh", sh, F32, True), ("grid.valid", valid, U32, True)) + more,
              (("rgb", (n, 3), F32), ("sh", (n, bands * bands, 3), F32, bool(want_sh)), ("weight", (n,), F32, bool(want_weight))))
    g = abi.NraysIrradianceGrid((C.c_double * 3)(*origin), (C.c_double * 3)(*cell), (C.c_uint32 * 3)(*counts), bands, b.addr(b.ins[3]), b.addr(b.ins[4]), measure, 0)
    if vis is None:
        b.call(scene, "nrays_irradiance_points", n, *b.pin[:3], C.byref(g), *b.pout, abi.IRRADIANCE_FACING if facing else 0)
    else:
        v = abi.NraysIrradianceVisibility(b.addr(b.ins[5]), vis[1], vis[2], vis[3])
        b.call(scene, "nrays_irradiance_points_vis", n, *b.pin[:3], C.byref(g), C.byref(v), *b.pout, abi.IRRADIANCE_FACING if facing else 0)
    return Irradiance(*b.outs) if want_sh or want_weight else b.outs[0]


def bake_probe_grid(scene, origin, cell, counts, sample_dirs, bands=3, energy=1.0, max_depth=0, keys=None, unordered=True, valid=None, measure=4.0 * math.pi, device=None):
    """A grid of irradiance probes: gather_probes() at probe_grid_positions(origin, cell, counts) with the sphere table `sample_dirs`, as a ProbeGrid for
    irradiance_points().  `valid` and `measure` are passed through (the solid angle of sphere_dirs is 4 pi); which probes are valid stays the caller's to decide —
    bake_probe_visibility() on the grid returns validity words from what the probes see.
    `device`: None bakes through the blocking form into numpy arrays; a GPU (or CURRENT) keeps the positions and the coefficients there as tensors."""
    origin, cell, counts = _probe_lattice(origin, cell, counts)
    positions = probe_grid_positions(origin, cell, counts)
    if device is not None:
        import torch
        positions = upload(positions, torch.device("cuda", torch.cuda.current_device()) if device is CURRENT else device)
    return ProbeGrid(origin, cell, counts, gather_probes(scene, positions, sample_dirs, bands, energy, max_depth, keys, unordered), valid, measure)


# ---- what a probe sees of the geometry: depth moments, near / miss counts, the nearest hit (include/nrays_abi.h: nrays_probe_depth_points_device) -------------

DEPTH_OUTPUTS = ("counts", "nearest", "nearest_dir")  # the optional outputs of probe_depth_points, in the order of nrays_probe_depth_points_device's arguments
ProbeDepth = collections.namedtuple("ProbeDepth", ("moments",) + DEPTH_OUTPUTS)


def _depth_settings(res, max_dist, near_dist):
    res = _depth_res(res)
    if max_dist is None:
        raise ValueError("max_dist is required")
    max_dist, near_dist = float(max_dist), float(near_dist)
    if not (math.isfinite(max_dist) and max_dist > 0.0):
        raise ValueError("max_dist must be finite and > 0, got %r" % max_dist)
    if not (math.isfinite(near_dist) and near_dist >= 0.0):
        raise ValueError("near_dist must be finite and >= 0, got %r" % near_dist)
    return res, max_dist, near_dist


def probe_depth_points(scene, points, normals, sample_dirs, res=8, max_dist=None, near_dist=0.0, rotations=None, bias=1e-3, hit_flags=None, keys=None, want=DEPTH_OUTPUTS):
    """What n caller-supplied points SEE of the geometry around them, through nrays_probe_depth_points_device / nrays_probe_depth_points: per point the library builds
    the len(sample_dirs) rays of occlusion_points() ON THE DEVICE (the same rays bit for bit: occlusion_rays()), runs the closest-hit query of closest_hits() on each
    and folds the distances into ProbeDepth(moments, counts, nearest, nearest_dir): moments (n, res^2, 2) float32 — per texel of the res x res octahedral map
    (oct_texel()) the mean and the mean square of the distances, clamped to `max_dist`, of the rays that fall into it, (max_dist, max_dist^2) where none does: the
    visibility term of DDGI (Majercik et al. 2019) that irradiance_points(visibility=) reads —, counts (n, 2): the rays that end closer than `near_dist` and the
    rays that hit nothing (probe_valid_words() decides a probe's validity from them), nearest (n,) float64 and nearest_dir (n,): the least distance and the index of
    its direction (inf and 0xFFFFFFFF when nothing was hit) — what moving a probe off a surface needs.  It equals probe_depth_ref(occlusion_rays()' directions,
    closest_hits' toi and flags) bit for bit.  No ray or per-ray distance is ever in the caller's memory; the handle's workspace keeps 4 bytes a ray of one chunk.
    `res`: 4, 8 or 16.  `max_dist` is required (finite, > 0).  `points`, `normals`, `sample_dirs`, `rotations`, `bias`, `hit_flags`, `keys`: as for occlusion_points;
    a skipped point holds the empty-texel pair everywhere, counts 0, inf and 0xFFFFFFFF.  `want`: which of "counts", "nearest", "nearest_dir" to compute (None otherwise).
    numpy arrays -> nrays_probe_depth_points (blocking), numpy arrays (words uint32).  torch tensors on the scene's GPU -> nrays_probe_depth_points_device on
    torch's current stream, tensors (words int32).  Also `scene.probe_depth_points(...)` on Scene and FileScene; probe_depth() is the form at free points."""
    res, max_dist, near_dist = _depth_settings(res, max_dist, near_dist)
    want = tuple(want)
    for w in want:
        if w not in DEPTH_OUTPUTS:
            raise ValueError("want must name outputs among %s, got %r" % (DEPTH_OUTPUTS, w))
    n = _n_of(points, normals, ("points", "normals"))
    for name, a in (("hit_flags", hit_flags), ("keys", keys)):
        _check_vec(name, a, n)
    L, rot, bias, _ = _occlusion_tables(sample_dirs, rotations, bias, math.inf)
    b = _point_batch(points, normals, hit_flags, keys, L, rot, (("moments", (n, res * res, 2), F32), ("counts", (n, 2), U32, "counts" in want),
                                                                ("nearest", (n,), F64, "nearest" in want), ("nearest_dir", (n,), U32, "nearest_dir" in want)))
    params = abi.NraysProbeDepthParams(*_tables(b), bias, max_dist, near_dist, res, 0)
    b.call(scene, "nrays_probe_depth_points", n, *b.pin[:4], C.byref(params), *b.pout, 0)
    return ProbeDepth(*b.outs)


def probe_depth(scene, positions, sample_dirs, res=8, max_dist=None, near_dist=0.0, keys=None, want=DEPTH_OUTPUTS):
    """probe_depth_points() at free points in space, as gather_probes() is gather_sh_points() there: normals (0, 0, 1), bias 0 and no rotations — that frame reproduces
    `sample_dirs` (sphere_dirs()) bit for bit as world directions and the origin is the position itself.  A ProbeDepth; numpy or torch as `positions`."""
    if len(positions.shape) != 2 or positions.shape[1] != 3:
        raise ValueError("positions must have shape (n, 3), got %s" % (tuple(positions.shape),))
    if _is_tensor(positions):
        import torch
        normals = torch.zeros_like(positions)
    else:
        normals = np.zeros((len(positions), 3), np.float64)
    normals[:, 2] = 1.0
    return probe_depth_points(scene, positions, normals, sample_dirs, res, max_dist, near_dist, None, 0.0, None, keys, want)


def probe_valid_words(counts, num_dirs, max_near_fraction=0.25):
    """Validity words for ProbeGrid.valid from the counts of probe_depth(): 1 where at most max_near_fraction of a probe's num_dirs rays ended closer than
    near_dist, 0 otherwise — a probe inside geometry sees a surface at once in most directions.  Compared in integers: counts[:, 0] <= floor(max_near_fraction *
    num_dirs).  (P, 2) integers, numpy or torch -> (P,) uint32 (numpy) or int32 (torch)."""
    num_dirs, frac = int(num_dirs), float(max_near_fraction)
    if not 1 <= num_dirs <= OCCLUSION_MAX_TABLE:
        raise ValueError("num_dirs must be in 1 .. %d" % OCCLUSION_MAX_TABLE)
    if not 0.0 <= frac <= 1.0:
        raise ValueError("max_near_fraction must be in [0, 1], got %r" % frac)
    if len(counts.shape) != 2 or counts.shape[1] != 2:
        raise ValueError("counts must have shape (P, 2), got %s" % (tuple(counts.shape),))
    limit = int(math.floor(frac * num_dirs))
    if _is_tensor(counts):
        import torch
        return (counts[:, 0].to(torch.int64) <= limit).to(torch.int32)
    counts = np.asarray(counts)
    if not np.issubdtype(counts.dtype, np.integer):
        raise ValueError("counts must be integers, got %s" % counts.dtype)
    return (counts[:, 0].astype(np.int64) <= limit).astype(np.uint32)


def _visibility_distances(cell, counts, max_dist, near_dist):
    """The defaults of bake_probe_visibility(): max_dist None -> 1.5 x the diagonal of a cell, near_dist None -> a fifth of the smallest spacing (axes with more than one probe)."""
    spans = [c for c, k in zip(cell, counts) if k > 1]
    if max_dist is None:
        if not spans:
            raise ValueError("max_dist is required for a grid of one probe")
        max_dist = 1.5 * math.sqrt(sum(c * c for c in spans))
    if near_dist is None:
        near_dist = 0.2 * min(spans) if spans else 0.0
    return max_dist, near_dist


def bake_probe_visibility(scene, grid, sample_dirs, res=8, max_dist=None, near_dist=None, max_near_fraction=0.25, floor=0.05, bias=0.0):
    """The visibility of a ProbeGrid: probe_depth() at the grid's probe_grid_positions() with the sphere table `sample_dirs` -> (ProbeVisibility(moments, res, floor,
    bias), valid_words): the first for irradiance_points(visibility=), the second — probe_valid_words() of the counts — for ProbeGrid.valid (grid._replace(valid=...)).
    `max_dist=None`: 1.5 x the diagonal of a cell (the axes with more than one probe), DDGI's convention; `near_dist=None`: a fifth of the smallest cell spacing (0 for
    a single probe).  Both defaults are conventions, not measured numbers.  The form follows grid.sh: numpy arrays bake through the blocking form, tensors on their GPU."""
    origin, cell, counts, _, sh, _, _ = _probe_grid(grid)
    max_dist, near_dist = _visibility_distances(cell, counts, max_dist, near_dist)
    L, _, _, _ = _occlusion_tables(sample_dirs, None, 0.0, math.inf)
    positions = probe_grid_positions(origin, cell, counts)
    if _is_tensor(sh):
        positions = upload(positions, sh.device)
    d = probe_depth(scene, positions, L, res, max_dist, near_dist, None, ("counts",))
    return ProbeVisibility(d.moments, _depth_res(res), float(floor), float(bias)), probe_valid_words(d.counts, len(L), max_near_fraction)


# ---- the surface of a mesh node at a light map's texels (include/nrays_abi.h: nrays_surface_texels_device) ---------------------------------------------


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
    on torch's current stream, tensors there (flags int32)."""
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
    b = Batch((), (("points", (n, 3), F64), ("normals", (n, 3), F64, "normals" in want), ("uv", (n, 2), F64, "uv" in want), ("node", (n,), I32, "node" in want),
                   ("prim", (n,), I32, "prim" in want), ("flags", (n,), U32)), device=device, texels=True)
    b.call(scene, "nrays_surface_texels", node, width, height, *b.pout, flags)
    return SurfaceTexels(*b.outs)


def surface_texels_passes(scene, node, width, height, centres=False, flip_normals=False, repeats=1):
    """Timing probe (nrays_debug_surface_texels_passes): the owner pass and the resolve pass of surface_texels, `repeats` times between events of their own.
    (repeats, 2) float32, milliseconds."""
    width, height = _texel_lattice(width, height)
    ms = np.zeros((int(repeats), 2), dtype=np.float32)
    flags = (abi.TEXELS_CENTRES if centres else 0) | (abi.TEXELS_FLIP_NORMALS if flip_normals else 0)
    abi.check(abi.load_hip_lib().nrays_debug_surface_texels_passes(scene.device_handle(), int(node), width, height, flags, int(repeats), np_ptr(ms)))
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


def dilate_texels(scene, flags, width, height, radius, values=None, want_source=False, device=None):
    """Gutter dilation of a width x height light map through nrays_dilate_texels_device / nrays_dilate_texels: every uncovered texel takes the values of
    the nearest covered texel within `radius` (1 .. 64; a Euclidean disc, no wrap-around, the smaller index y * width + x among equals).  `flags`:
    width * height words, texel (x, y) at y * width + x, covered iff bit 0 is set — the flags of surface_texels() as they are.  `values`: 1 .. 4
    float32 per texel ((n, c), (height, width, c) or (n,)), dilated IN PLACE when it is a C-contiguous float32 array or tensor (a converted copy
    otherwise): the words of the source are copied as bit patterns; covered texels and texels with nothing in reach are not written.
    Returns (values or None, source or None, flags): source (n,) int32 with want_source — the texel copied from, the texel itself where covered, -1 where
    nothing is in reach —; flags a new array, the input | abi.TEXEL_FILLED at the filled texels (bit 0 stays clear there).
    numpy arrays -> nrays_dilate_texels (blocking; flags out uint32).  torch tensors on the scene's GPU (flags int32, values float32) ->
    nrays_dilate_texels_device on torch's current stream, tensors there; `device` moves numpy arguments to that GPU first.
    Also `scene.dilate_texels(flags, ...)` on Scene and FileScene.  dilate_texels_ref() restates the result bit for bit."""
    w, h, r, channels = _dilate_args(flags, width, height, radius, values)
    n = w * h
    if values is not None and device is None and not _is_tensor(flags) and not _is_tensor(values) and not (
            isinstance(values, np.ndarray) and values.dtype == np.float32 and values.flags.c_contiguous and values.flags.writeable):
        values = np.array(_np_floats("values", values, np.float32), copy=True)  # the blocking form writes into the caller's array only when it can
    b = Batch((("flags", flags, U32), ("values", values, F32)), (("source", (n,), I32, want_source), ("flags", (n,), U32)), device=device, texels=True)
    b.call(scene, "nrays_dilate_texels", w, h, b.pin[0], r, channels, b.pin[1], *b.pout, 0)
    return b.ins[1], b.outs[0], b.outs[1]


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
    there or numpy arrays, which are uploaded) -> nrays_gather_maps_points_device on torch's current stream, tensors (counts int32)."""
    n = _n_of(points, normals, ("points", "normals"))
    for name, a in (("hit_flags", hit_flags), ("keys", keys)):
        _check_vec(name, a, n)
    L, rot, bias, _ = _occlusion_tables(sample_dirs, rotations, bias, math.inf)
    ms, nodes, max_toi, miss = _gather_maps_args(scene, maps, node_map, max_toi, miss)
    b = _point_batch(points, normals, hit_flags, keys, L, rot, (("rgb", (n, 3), F32), ("counts", (n, 2), U32, want_counts)),
                     tuple(("maps[%d]" % i, m, F32, True) for i, (m, _, _) in enumerate(ms)) + (("node_map", nodes, I32, True),))
    recs = (abi.NraysTexture * len(ms))()  # only the params struct refers to it: it lives until this function returns
    for t, m, (_, interp, overflow) in zip(recs, b.ins[6:-1], ms):
        t.width, t.height, t.format, t.interp, t.overflow, t.texels = m.shape[1], m.shape[0], abi.TEXEL_RGBA32F, interp, overflow, b.addr(m)
    params = abi.NraysGatherMapsParams(*_tables(b), bias, max_toi, len(ms), len(nodes), C.cast(recs, C.POINTER(abi.NraysTexture)), b.addr(b.ins[-1]), (C.c_float * 3)(*miss))
    b.call(scene, "nrays_gather_maps_points", n, *b.pin[:4], C.byref(params), *b.pout, 0)
    return tuple(b.outs) if want_counts else b.outs[0]


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
        a = upload(a, level.device)
    total = level.clone() if _is_tensor(level) else level.copy()
    for b in range(1, bounces + 1):
        rgb = gather_maps_points(scene, tx.points, tx.normals, sample_dirs, [level.reshape(height, width, 4)], {int(node): 0}, rotations, bias, math.inf,
                                 miss if b == 1 else (0.0, 0.0, 0.0), hit_flags=tx.flags, keys=keys)
        nxt = total.clone() if _is_tensor(total) else total.copy()  # (alpha from L_0; the rgb of every texel is written below or left to the dilation)
        nxt[:, :3] = a * rgb
        level = _bake_dilate(scene, tx.flags, nxt, width, height, radius)
        total[:, :3] = total[:, :3] + level[:, :3]
    return total.reshape(height, width, 4)


# ---- probes filled from baked maps, with their depth from the same rays (include/nrays_abi.h: nrays_gather_maps_sh_points_device) ------------------------------

GATHER_MAPS_SH_OUTPUTS = ("counts", "depth_counts", "nearest", "nearest_dir")  # the optional outputs of gather_maps_sh_points, in the order of the call's arguments
GatherMapsSh = collections.namedtuple("GatherMapsSh", ("sh", "counts", "depth"))
GatherMapsSh.__doc__ = """What gather_maps_sh_points returns: `sh` (n, bands^2, 3) float32; `counts` (n, 2) — the mapped and the missed rays — or None; `depth` a ProbeDepth
(moments, counts, nearest, nearest_dir), or None when no depth settings were given."""
_DEPTH_KEYS = ("res", "max_dist", "near_dist")


def _gather_depth(depth):
    """depth=None, or dict(res=, max_dist=, near_dist=) through _depth_settings (res 8 and near_dist 0 when left out, as probe_depth_points; max_dist is required)."""
    if depth is None:
        return None
    if not isinstance(depth, dict) or any(k not in _DEPTH_KEYS for k in depth):
        raise ValueError("depth must be None or a dict with keys among %s, got %r" % (_DEPTH_KEYS, depth))
    return _depth_settings(depth.get("res", 8), depth.get("max_dist"), depth.get("near_dist", 0.0))


def gather_maps_sh_points(scene, points, normals, sample_dirs, maps, node_map, bands=3, rotations=None, bias=1e-3, max_toi=math.inf, miss=(0.0, 0.0, 0.0), hit_flags=None,
                          keys=None, depth=None, want=GATHER_MAPS_SH_OUTPUTS):
    """gather_maps_points() that keeps WHERE the light came from, and probe_depth_points() from the same rays, through nrays_gather_maps_sh_points_device /
    nrays_gather_maps_sh_points: per point the len(sample_dirs) rays of occlusion_points() are built ON THE DEVICE and each runs the closest-hit query ONCE; the
    colours gather_maps_points() would average (a map's sample at the hit, `miss`, or black) are folded like gather_sh_points() folds its colours — the projection
    onto the real spherical harmonics of bands 0 .. bands - 1 of each ray's direction, (n, bands^2, 3) float32, no measure applied — and, with `depth`, the
    distances are folded into what probe_depth_points() returns.  A probe filled this way sees the bounced light the scene's baked maps hold.  It equals
    sh_fold_ref(occlusion_rays()' directions, the contributions of closest_hits + lightmap_sample_ref) and probe_depth_points() on the same inputs, bit for bit.
    `depth`: None, or dict(res=4 | 8 | 16, max_dist=finite > 0 (required), near_dist=0.0): the settings of probe_depth_points.  `max_toi` turns far hits into
    `miss` for the colours and counts only; the depth side sees the unbounded query.  `want`: which of "counts" (mapped, missed), "depth_counts", "nearest",
    "nearest_dir" to compute; the last three only with `depth`.  The other arguments, the numpy / torch forms and the maps: as for gather_maps_points.
    Returns GatherMapsSh(sh, counts, depth): depth a ProbeDepth, or None without `depth`.  The handle's workspace keeps 12 (16 with depth) bytes a ray of one
    chunk; no ray or per-ray value is ever in the caller's memory.  Also `scene.gather_maps_sh_points(...)` on Scene and FileScene; gather_maps_probes() is the form
    at free points."""
    bands = _sh_bands(bands)
    spec = _gather_depth(depth)
    want = tuple(want)
    for w in want:
        if w not in GATHER_MAPS_SH_OUTPUTS:
            raise ValueError("want must name outputs among %s, got %r" % (GATHER_MAPS_SH_OUTPUTS, w))
    n = _n_of(points, normals, ("points", "normals"))
    for name, a in (("hit_flags", hit_flags), ("keys", keys)):
        _check_vec(name, a, n)
    L, rot, bias, _ = _occlusion_tables(sample_dirs, rotations, bias, math.inf)
    ms, nodes, max_toi, miss = _gather_maps_args(scene, maps, node_map, max_toi, miss)
    deep, texels = spec is not None, (spec[0] * spec[0] if spec is not None else 0)
    b = _point_batch(points, normals, hit_flags, keys, L, rot,
                     (("sh", (n, bands * bands, 3), F32), ("counts", (n, 2), U32, "counts" in want), ("moments", (n, texels, 2), F32, deep),
                      ("depth_counts", (n, 2), U32, deep and "depth_counts" in want), ("nearest", (n,), F64, deep and "nearest" in want),
                      ("nearest_dir", (n,), U32, deep and "nearest_dir" in want)),
                     tuple(("maps[%d]" % i, m, F32, True) for i, (m, _, _) in enumerate(ms)) + (("node_map", nodes, I32, True),))
    recs = (abi.NraysTexture * len(ms))()  # only the params struct refers to it: it lives until this function returns
    for t, m, (_, interp, overflow) in zip(recs, b.ins[6:-1], ms):
        t.width, t.height, t.format, t.interp, t.overflow, t.texels = m.shape[1], m.shape[0], abi.TEXEL_RGBA32F, interp, overflow, b.addr(m)
    params = abi.NraysGatherMapsParams(*_tables(b), bias, max_toi, len(ms), len(nodes), C.cast(recs, C.POINTER(abi.NraysTexture)), b.addr(b.ins[-1]), (C.c_float * 3)(*miss))
    dspec = abi.NraysGatherDepthSpec(spec[1], spec[2], spec[0], 0) if deep else None
    b.call(scene, "nrays_gather_maps_sh_points", n, *b.pin[:4], C.byref(params), bands, b.pout[0], b.pout[1], C.byref(dspec) if deep else None, *b.pout[2:], 0)
    return GatherMapsSh(b.outs[0], b.outs[1], ProbeDepth(*b.outs[2:]) if deep else None)


def gather_maps_probes(scene, positions, sample_dirs, maps, node_map, bands=3, max_toi=math.inf, miss=(0.0, 0.0, 0.0), keys=None, depth=None, want=GATHER_MAPS_SH_OUTPUTS):
    """Irradiance probes at free points in space, filled from baked maps: gather_maps_sh_points() with normals (0, 0, 1), bias 0 and no rotations, as gather_probes()
    is gather_sh_points() and probe_depth() is probe_depth_points() there — that frame reproduces `sample_dirs` (sphere_dirs()) bit for bit as world directions and
    the origin is the position itself.  A GatherMapsSh; numpy or torch as `positions`."""
    if len(positions.shape) != 2 or positions.shape[1] != 3:
        raise ValueError("positions must have shape (n, 3), got %s" % (tuple(positions.shape),))
    if _is_tensor(positions):
        import torch
        normals = torch.zeros_like(positions)
    else:
        normals = np.zeros((len(positions), 3), np.float64)
    normals[:, 2] = 1.0
    return gather_maps_sh_points(scene, positions, normals, sample_dirs, maps, node_map, bands, None, 0.0, max_toi, miss, None, keys, depth, want)


_VISIBILITY_KEYS = {"res": 8, "max_dist": None, "near_dist": None, "max_near_fraction": 0.25, "floor": 0.05, "bias": 0.0}


def bake_probe_grid_maps(scene, origin, cell, counts, sample_dirs, maps, node_map, bands=3, miss=(0.0, 0.0, 0.0), visibility=None, measure=4.0 * math.pi, device=None):
    """A grid of irradiance probes filled from baked maps, and its visibility from the same rays, in ONE call into the library: gather_maps_probes() at
    probe_grid_positions(origin, cell, counts) with the sphere table `sample_dirs` -> (ProbeGrid, ProbeVisibility or None) for irradiance_points(grid, visibility=).
    The probes see what the maps hold — every bounce that was baked into them —, where bake_probe_grid() sees direct light only.
    `visibility`: None (no depth side; the grid's `valid` is None), or a dict with keys among res=8, max_dist=None, near_dist=None, max_near_fraction=0.25,
    floor=0.05, bias=0.0 — the parameters of bake_probe_visibility(), with its defaults for max_dist and near_dist: the moments are bit for bit what that call
    returns on the same grid, and the grid's `valid` is probe_valid_words() of the depth counts.  `maps`, `node_map`, `miss`: as for gather_maps_points.
    `device`: None bakes through the blocking form into numpy arrays; a GPU (or CURRENT) keeps positions and results there as tensors."""
    origin, cell, counts = _probe_lattice(origin, cell, counts)
    L, _, _, _ = _occlusion_tables(sample_dirs, None, 0.0, math.inf)
    depth = v = None
    if visibility is not None:
        if not isinstance(visibility, dict) or any(k not in _VISIBILITY_KEYS for k in visibility):
            raise ValueError("visibility must be None or a dict with keys among %s, got %r" % (tuple(_VISIBILITY_KEYS), visibility))
        v = dict(_VISIBILITY_KEYS, **visibility)
        max_dist, near_dist = _visibility_distances(cell, counts, v["max_dist"], v["near_dist"])
        depth = dict(res=v["res"], max_dist=max_dist, near_dist=near_dist)
        _gather_depth(depth)
        floor, vbias = float(v["floor"]), float(v["bias"])
        if not 0.0 <= floor <= 1.0 or not math.isfinite(vbias):
            raise ValueError("visibility: floor must be in [0, 1] and bias finite, got %r, %r" % (floor, vbias))
        probe_valid_words(np.zeros((1, 2), np.uint32), len(L), v["max_near_fraction"])  # (its checks, before any device work)
    positions = probe_grid_positions(origin, cell, counts)
    if device is not None:
        import torch
        positions = upload(positions, torch.device("cuda", torch.cuda.current_device()) if device is CURRENT else device)
    g = gather_maps_probes(scene, positions, L, maps, node_map, bands, math.inf, miss, None, depth, ("depth_counts",))
    if v is None:
        return ProbeGrid(origin, cell, counts, g.sh, None, measure), None
    valid = probe_valid_words(g.depth.counts, len(L), v["max_near_fraction"])
    return ProbeGrid(origin, cell, counts, g.sh, valid, measure), ProbeVisibility(g.depth.moments, _depth_res(v["res"]), floor, vbias)


# ---- denoising a baked map: the a-trous joint-bilateral filter (include/nrays_abi.h: nrays_filter_texels_device) -----------------------------------------------


def _filter_columns(flags, points, normals, values):
    return ("flags", flags, U32), ("points", points, F64), ("normals", normals, F64), ("values", values, F32)


def filter_texels(scene, flags, width, height, points, normals, values, step=1, pos_radius=math.inf, normal_cos=0.0, device=None):
    """One pass of the edge-aware filter that denoises a baked width x height light map, through nrays_filter_texels_device / nrays_filter_texels: a 5 x 5
    a-trous (B3-spline) joint-bilateral filter whose taps lie `step` (1 .. 64) texels apart.  A covered texel becomes the weighted mean of the covered
    texels among its 25 taps that lie on the same piece of surface: a tap's weight falls linearly with its squared world distance, reaching 0 at
    `pos_radius` (math.inf: no position weight), and with the cosine between the normals, reaching 0 at `normal_cos` (in [-1, 1); -1 with unit normals:
    no normal weight) — so nothing blends across a chart border, a gutter or a crease.  Uncovered texels keep their words.  `flags`, `points`,
    `normals`: flags / points / normals of surface_texels() as they are; `values`: 1 .. 4 float32 per texel ((n, c), (height, width, c) or (n,)).
    Returns a NEW array or tensor in the shape of `values`; the arguments stay as they are.
    numpy arrays -> nrays_filter_texels (blocking).  torch tensors on the scene's GPU (flags int32, points / normals float64, values float32) ->
    nrays_filter_texels_device on torch's current stream; `device` moves numpy arguments to that GPU first.  Also `scene.filter_texels(flags, ...)`
    on Scene and FileScene; denoise_texels() runs the passes with steps 1, 2, 4, ...; filter_texels_ref() restates the result bit for bit."""
    w, h, step, pos_radius, normal_cos, channels = _filter_args(flags, width, height, points, normals, values, step, pos_radius, normal_cos)
    b = Batch(_filter_columns(flags, points, normals, values), (("values", tuple(values.shape), F32),), device=device, texels=True)
    b.call(scene, "nrays_filter_texels", w, h, *b.pin[:3], channels, b.pin[3], *b.pout, step, pos_radius, normal_cos, 0)
    return b.outs[0]


def denoise_texels(scene, tx, values, passes=3, pos_radius=math.inf, normal_cos=0.0, width=None, height=None):
    """A baked light map denoised: `passes` (1 .. 7) passes of filter_texels() with steps 1, 2, 4, ... on the texels `tx` — a SurfaceTexels with its normals,
    surface_texels()'s result as it is — between two buffers, all on torch's current stream, nothing read back in between.  Three passes reach 29 texels
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
    shape = tuple(values.shape)
    b = Batch(_filter_columns(tx.flags, tx.points, tx.normals, values), (("ping", shape, F32), ("pong", shape, F32, passes > 1)), device=CURRENT, texels=True)
    bufs, src = [b.pin[3]] + b.pout, 0  # the input is never written
    for k in range(passes):
        dst = 1 if src != 1 else 2
        b.call(scene, "nrays_filter_texels", w, h, *b.pin[:3], channels, bufs[src], bufs[dst], 1 << k, pos_radius, normal_cos, 0)
        src = dst
    out = b.outs[src - 1]
    return out if _is_tensor(tx.flags) else out.cpu().numpy()


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
    b = Batch((("origins", origins, F64), ("dirs", dirs, F64)), ())
    keys, order = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    frame, info = np.zeros(abi.RAY_FRAME_DOUBLES, np.float64), (C.c_uint32 * 4)()
    b.call(scene, "nrays_debug_ray_order", n, *b.pin, np_ptr(keys), np_ptr(order), np_ptr(frame), info)
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
    b = _point_batch(points, normals, hit_flags, keys, L, rot, ())
    out_keys, order = np.zeros(pairs, np.uint64), np.zeros(pairs, np.uint32)
    frame, info = np.zeros(abi.RAY_FRAME_DOUBLES, np.float64), (C.c_uint32 * 4)()
    params = abi.NraysGatherParams(*_tables(b), bias, 1.0, 0)
    b.call(scene, "nrays_debug_gather_order", n, *b.pin[:4], C.byref(params), np_ptr(out_keys), np_ptr(order), np_ptr(frame), info)
    return out_keys, order[:int(info[3])].copy(), frame, (int(info[0]), int(info[1]), bool(info[2]), int(info[3]))
