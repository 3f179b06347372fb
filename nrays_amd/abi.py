"""ctypes mirror of include/nrays_abi.h (the C-ABI drop-in boundary for scene::render).

Every structure here is the `#[repr(C)]` twin of the C declaration of the same name; field order
and types must match include/nrays_abi.h exactly (tests/test_abi.py checks sizes and symbols).
"""
import ctypes as C
import os

ABI_VERSION = 7
COUNT_AS_TIMED = 1  # nrays_render_device_counted: count the work of the plain (timed) render, include/nrays_abi.h

# NraysStatus
OK = 0
ERR_BAD_ARG = -1
ERR_HIP = -2
ERR_OOM = -3
ERR_UNSUPPORTED = -4
ERR_NO_DEVICE = -5
ERR_QUEUE_OVERFLOW = -6
ERR_RCCL = -7
UNIQUE_ID_BYTES = 128

# NraysShapeKind (examples/loader3d.rs:593-695)
SHAPE_BALL, SHAPE_CUBOID, SHAPE_CYLINDER, SHAPE_CAPSULE, SHAPE_CONE, SHAPE_PLANE, SHAPE_TRIMESH = range(7)
# NraysMaterialKind
MAT_PHONG, MAT_NORMAL, MAT_UV = range(3)
TEXEL_RGBA8, TEXEL_RGBA32F = 0, 1
INTERP_BILINEAR, INTERP_NEAREST = 0, 1
OVERFLOW_WRAP, OVERFLOW_CLAMP = 0, 1


class NraysLight(C.Structure):
    _fields_ = [("pos", C.c_double * 3), ("radius", C.c_double), ("racsample", C.c_uint32), ("color", C.c_float * 3)]


class NraysTexture(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("format", C.c_uint32), ("interp", C.c_uint32),
                ("overflow", C.c_uint32), ("reserved", C.c_uint32), ("texels", C.c_void_p)]


class NraysMaterial(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("ambiant", C.c_float * 3), ("diffuse", C.c_float * 3),
                ("specular", C.c_float * 3), ("shininess", C.c_float), ("texture_id", C.c_int32),
                ("alpha_texture_id", C.c_int32)]


class NraysMesh(C.Structure):
    _fields_ = [("num_vertices", C.c_uint32), ("num_triangles", C.c_uint32), ("vertices", C.POINTER(C.c_double)),
                ("uvs", C.POINTER(C.c_double)), ("indices", C.POINTER(C.c_uint32))]


class NraysNode(C.Structure):
    _fields_ = [("shape_kind", C.c_uint32), ("solid", C.c_uint32), ("params", C.c_double * 3),
                ("translation", C.c_double * 3), ("axis_angle", C.c_double * 3), ("refl_mix", C.c_float),
                ("refl_atenuation", C.c_float), ("alpha", C.c_float), ("reserved0", C.c_float),
                ("refr_coeff", C.c_double), ("material_id", C.c_uint32), ("mesh_id", C.c_int32)]


class NraysSceneDesc(C.Structure):
    _fields_ = [("background", C.c_float * 3), ("num_lights", C.c_uint32), ("lights", C.POINTER(NraysLight)),
                ("num_materials", C.c_uint32), ("materials", C.POINTER(NraysMaterial)),
                ("num_textures", C.c_uint32), ("textures", C.POINTER(NraysTexture)),
                ("num_meshes", C.c_uint32), ("meshes", C.POINTER(NraysMesh)),
                ("num_nodes", C.c_uint32), ("nodes", C.POINTER(NraysNode))]


class NraysRenderParams(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("ray_per_pixel", C.c_uint32),
                ("max_depth", C.c_uint32), ("window_width", C.c_double), ("camera_eye", C.c_double * 3),
                ("inv_proj_view", C.c_double * 16), ("seed", C.c_uint64), ("band_rows", C.c_uint32),
                ("band_owner", C.c_uint32), ("band_owners", C.c_uint32), ("reserved", C.c_uint32)]


class NraysStats(C.Structure):
    _fields_ = [("rays_primary", C.c_uint64), ("rays_reflection", C.c_uint64), ("rays_refraction", C.c_uint64),
                ("rays_shadow", C.c_uint64), ("node_tests", C.c_uint64), ("tri_tests", C.c_uint64),
                ("prim_tests", C.c_uint64), ("hit_records", C.c_uint64), ("tex_samples", C.c_uint64),
                ("generations", C.c_uint32), ("instrumented", C.c_uint32), ("kernel_ms_primary", C.c_double),
                ("kernel_ms_total", C.c_double), ("frames_timed", C.c_uint32), ("reserved", C.c_uint32),
                ("rays_primary_traced", C.c_uint64), ("rays_shadow_elided", C.c_uint64), ("node_fetches", C.c_uint64)]

    def rays_traced(self):
        """Rays that went through a BVT query (total_rays() counts every primary ray the reference would trace)."""
        return self.rays_primary_traced + self.rays_reflection + self.rays_refraction + self.rays_shadow - self.rays_shadow_elided

    def total_rays(self):
        return self.rays_primary + self.rays_reflection + self.rays_refraction + self.rays_shadow

    def algorithmic_bytes(self, width=0, rows=0):
        """B = 32 N_node + 36 N_tri + 64 N_prim + 64 N_hit + 16 N_texsample + 64 per ray
        (+ 12 B per framebuffer pixel)."""
        return (32 * self.node_tests + 36 * self.tri_tests + 64 * self.prim_tests + 64 * self.hit_records
                + 16 * self.tex_samples + 64 * self.total_rays() + 12 * width * rows)

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class NraysMultiTimings(C.Structure):
    _fields_ = [("render_ms", C.c_double), ("exchange_ms", C.c_double), ("untile_ms", C.c_double), ("frames", C.c_uint32), ("owner", C.c_uint32)]


class NraysTileCosts(C.Structure):
    _fields_ = [("tiles", C.c_uint64), ("sum_cycles", C.c_uint64), ("max_cycles", C.c_uint64), ("resident_waves", C.c_uint64), ("shader_clock_hz", C.c_double), ("kernel_ms", C.c_double)]


class NraysCastResult(C.Structure):
    _fields_ = [("toi", C.c_double), ("normal", C.c_double * 3), ("uv", C.c_double * 2), ("node_id", C.c_int32), ("flags", C.c_uint32)]


class NraysOcclusionParams(C.Structure):
    """The tables of nrays_occlusion_points*: `dirs` / `rotations` are addresses (device memory for the _device form, host memory otherwise)."""
    _fields_ = [("num_dirs", C.c_uint32), ("num_rotations", C.c_uint32), ("dirs", C.c_void_p), ("rotations", C.c_void_p), ("bias", C.c_double), ("max_toi", C.c_double)]


LIGHTS_INVERSE_SQUARE = 1   # NRAYS_LIGHTS_INVERSE_SQUARE
LIGHTS_MAX = 4096           # the most rows of an NraysPointLights table


class NraysPointLights(C.Structure):
    """The light table of nrays_light_points*: `positions` / `colors` / `normals` are addresses (device memory for the _device form, host memory otherwise)."""
    _fields_ = [("num_lights", C.c_uint32), ("flags", C.c_uint32), ("positions", C.c_void_p), ("colors", C.c_void_p), ("normals", C.c_void_p), ("bias", C.c_double),
                ("offset", C.c_double), ("min_dist", C.c_double)]


class NraysGatherParams(C.Structure):
    """The tables and ray settings of nrays_gather_points*: `dirs` / `rotations` are addresses (device memory for the _device form, host memory otherwise)."""
    _fields_ = [("num_dirs", C.c_uint32), ("num_rotations", C.c_uint32), ("dirs", C.c_void_p), ("rotations", C.c_void_p), ("bias", C.c_double), ("energy", C.c_float),
                ("max_depth", C.c_uint32)]


GATHER_MAX_MAPS = 16        # NRAYS_GATHER_MAX_MAPS


class NraysGatherMapsParams(C.Structure):
    """The tables, maps and ray settings of nrays_gather_maps_points*: `maps` is always a host array of NraysTexture records; `dirs` / `rotations` / `node_map` and the
    records' texels are addresses (device memory for the _device form, host memory otherwise)."""
    _fields_ = [("num_dirs", C.c_uint32), ("num_rotations", C.c_uint32), ("dirs", C.c_void_p), ("rotations", C.c_void_p), ("bias", C.c_double), ("max_toi", C.c_double),
                ("num_maps", C.c_uint32), ("num_nodes", C.c_uint32), ("maps", C.POINTER(NraysTexture)), ("node_map", C.c_void_p), ("miss_rgb", C.c_float * 3)]


IRRADIANCE_FACING = 1       # NRAYS_IRRADIANCE_FACING
IRRADIANCE_MAX_COUNT, IRRADIANCE_MAX_PROBES = 1024, 1 << 22


class NraysIrradianceGrid(C.Structure):
    """The probe grid of nrays_irradiance_points*: `sh` / `valid` are addresses (device memory for the _device form, host memory otherwise)."""
    _fields_ = [("origin", C.c_double * 3), ("cell", C.c_double * 3), ("counts", C.c_uint32 * 3), ("bands", C.c_uint32), ("sh", C.c_void_p), ("valid", C.c_void_p),
                ("measure", C.c_float), ("reserved", C.c_uint32)]


class NraysProbeDepthParams(C.Structure):
    """The tables and settings of nrays_probe_depth_points*: `dirs` / `rotations` are addresses (device memory for the _device form, host memory otherwise)."""
    _fields_ = [("num_dirs", C.c_uint32), ("num_rotations", C.c_uint32), ("dirs", C.c_void_p), ("rotations", C.c_void_p), ("bias", C.c_double), ("max_dist", C.c_double),
                ("near_dist", C.c_double), ("res", C.c_uint32), ("reserved", C.c_uint32)]


PROBE_DEPTH_RES = (4, 8, 16)  # the resolutions of a probe's octahedral depth map


class NraysGatherDepthSpec(C.Structure):
    """The depth side of nrays_gather_maps_sh_points*: the settings of NraysProbeDepthParams that its NraysGatherMapsParams does not carry."""
    _fields_ = [("max_dist", C.c_double), ("near_dist", C.c_double), ("res", C.c_uint32), ("reserved", C.c_uint32)]


class NraysIrradianceVisibility(C.Structure):
    """The depth moments of nrays_irradiance_points_vis*: `moments` is an address (device memory for the _device form, host memory otherwise)."""
    _fields_ = [("moments", C.c_void_p), ("res", C.c_uint32), ("floor", C.c_float), ("bias", C.c_double)]


class NraysBlasDump(C.Structure):
    _fields_ = [("num_nodes", C.c_uint32), ("num_refs", C.c_uint32), ("root", C.c_int32), ("max_depth", C.c_int32), ("hairy", C.c_uint32),
                ("node_capacity", C.c_uint32), ("ref_capacity", C.c_uint32), ("pad", C.c_uint32), ("nodes", C.POINTER(C.c_float)), ("tri_ids", C.POINTER(C.c_uint32))]


class NraysSceneDump(C.Structure):
    """The buffers of nrays_debug_scene_dump: capacities in, sizes and scalars out (include/nrays_abi.h spells the record layouts)."""
    _fields_ = [("num_nodes", C.c_uint32), ("num_tris", C.c_uint32), ("num_instances", C.c_uint32), ("num_shadow_instances", C.c_uint32), ("num_planes", C.c_uint32),
                ("num_scene_nodes", C.c_uint32), ("node_capacity", C.c_uint32), ("tri_capacity", C.c_uint32), ("instance_capacity", C.c_uint32),
                ("shadow_instance_capacity", C.c_uint32), ("plane_capacity", C.c_uint32), ("scene_node_capacity", C.c_uint32), ("closest_root", C.c_int32),
                ("shadow_root", C.c_int32), ("max_bvh_depth", C.c_int32), ("bounded", C.c_uint32), ("dev_nodes", C.c_uint32), ("dev_tris", C.c_uint32),
                ("bounds_mn", C.c_float * 3), ("bounds_mx", C.c_float * 3), ("nodes", C.POINTER(C.c_float)), ("tris", C.POINTER(C.c_uint8)),
                ("instances", C.POINTER(C.c_uint8)), ("shadow_instances", C.POINTER(C.c_uint8)), ("links", C.POINTER(C.c_int32)), ("shadow_links", C.POINTER(C.c_int32)),
                ("planes", C.POINTER(C.c_int32)), ("shadow_planes", C.POINTER(C.c_int32)), ("node_aabbs", C.POINTER(C.c_double))]


# Every symbol include/nrays_abi.h declares, with its ctypes signature.
HIP_SYMBOLS = {
    "nrays_debug_blas_build": (C.c_int, [C.POINTER(NraysMesh), C.c_uint32, C.POINTER(NraysBlasDump)]),
    "nrays_debug_node_aabb": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_double)]),
    "nrays_debug_scene_dump": (C.c_int, [C.c_void_p, C.POINTER(NraysSceneDump)]),
    "nrays_debug_scene_flags": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "nrays_debug_last_permutation": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "nrays_debug_pipeline_counts": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "nrays_get_tile_costs": (C.c_int, [C.c_void_p, C.POINTER(NraysTileCosts)]),
    "nrays_debug_cast_batch": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                         C.POINTER(NraysCastResult)]),
    "nrays_debug_box_cull": (C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_float),
                                       C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_float)]),
    "nrays_trace_rays_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]),
    "nrays_trace_rays": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_float),
                                   C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_float)]),
    "nrays_intersects_rays_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "nrays_trace_rays_device_ex": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32,
                                             C.c_void_p]),
    "nrays_trace_rays_ex": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_float),
                                      C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_float), C.c_uint32]),
    "nrays_intersects_rays_device_ex": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "nrays_cast_rays_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_uint32, C.c_void_p]),
    "nrays_cast_rays": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                  C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.c_uint32]),
    "nrays_shade_points_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_uint32, C.c_void_p]),
    "nrays_shade_points": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                     C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_float), C.c_uint32]),
    "nrays_occlusion_points_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(NraysOcclusionParams), C.c_void_p, C.c_void_p,
                                                C.c_uint32, C.c_void_p]),
    "nrays_occlusion_points": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                         C.POINTER(NraysOcclusionParams), C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.c_uint32]),
    "nrays_debug_occlusion_rays": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(NraysOcclusionParams),
                                             C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "nrays_light_points_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(NraysPointLights), C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "nrays_light_points": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(NraysPointLights), C.POINTER(C.c_float),
                                     C.POINTER(C.c_uint32), C.c_uint32]),
    "nrays_debug_light_rays": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(NraysPointLights), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                         C.POINTER(C.c_double), C.POINTER(C.c_float)]),
    "nrays_gather_points_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(NraysGatherParams), C.c_void_p, C.c_uint32, C.c_void_p]),
    "nrays_gather_points": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                      C.POINTER(NraysGatherParams), C.POINTER(C.c_float), C.c_uint32]),
    "nrays_gather_points_device_ex": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(NraysGatherParams), C.c_void_p, C.c_uint32, C.c_void_p]),
    "nrays_gather_points_ex": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                         C.POINTER(NraysGatherParams), C.POINTER(C.c_float), C.c_uint32]),
    "nrays_debug_gather_order": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                           C.POINTER(NraysGatherParams), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(C.c_uint32)]),
    "nrays_gather_sh_points_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(NraysGatherParams), C.c_uint32, C.c_void_p, C.c_uint32,
                                                C.c_void_p]),
    "nrays_gather_sh_points": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                         C.POINTER(NraysGatherParams), C.c_uint32, C.POINTER(C.c_float), C.c_uint32]),
    "nrays_debug_gather_sh_fold": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                             C.POINTER(NraysGatherParams), C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "nrays_gather_maps_points_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(NraysGatherMapsParams), C.c_void_p, C.c_void_p,
                                                  C.c_uint32, C.c_void_p]),
    "nrays_gather_maps_points": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                           C.POINTER(NraysGatherMapsParams), C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.c_uint32]),
    "nrays_irradiance_points_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(NraysIrradianceGrid), C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_uint32, C.c_void_p]),
    "nrays_irradiance_points": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(NraysIrradianceGrid),
                                          C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint32]),
    "nrays_irradiance_points_vis_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(NraysIrradianceGrid), C.POINTER(NraysIrradianceVisibility),
                                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "nrays_irradiance_points_vis": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(NraysIrradianceGrid),
                                              C.POINTER(NraysIrradianceVisibility), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_uint32]),
    "nrays_probe_depth_points_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(NraysProbeDepthParams), C.c_void_p, C.c_void_p,
                                                  C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "nrays_probe_depth_points": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                           C.POINTER(NraysProbeDepthParams), C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.c_uint32]),
    "nrays_gather_maps_sh_points_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(NraysGatherMapsParams), C.c_uint32, C.c_void_p,
                                                     C.c_void_p, C.POINTER(NraysGatherDepthSpec), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "nrays_gather_maps_sh_points": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64),
                                              C.POINTER(NraysGatherMapsParams), C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(NraysGatherDepthSpec),
                                              C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.c_uint32]),
    "nrays_material_points_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32,
                                               C.c_void_p]),
    "nrays_material_points": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(C.c_float),
                                        C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_double), C.c_uint32]),
    "nrays_nearest_points_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_uint32, C.c_void_p]),
    "nrays_nearest_points": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(C.c_int32),
                                       C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.c_uint32]),
    "nrays_debug_nearest_bound": (C.c_int, [C.c_uint32, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "nrays_surface_texels_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_uint32, C.c_void_p]),
    "nrays_surface_texels": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                       C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.c_uint32]),
    "nrays_debug_surface_texels_passes": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]),
    "nrays_dilate_texels_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]),
    "nrays_dilate_texels": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint32, C.c_uint32, C.POINTER(C.c_float), C.POINTER(C.c_int32),
                                      C.POINTER(C.c_uint32), C.c_uint32]),
    "nrays_filter_texels_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_double, C.c_double,
                                             C.c_uint32, C.c_void_p]),
    "nrays_filter_texels": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_uint32, C.POINTER(C.c_float),
                                      C.POINTER(C.c_float), C.c_uint32, C.c_double, C.c_double, C.c_uint32]),
    "nrays_debug_ray_order": (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32),
                                        C.POINTER(C.c_double), C.POINTER(C.c_uint32)]),
    "nrays_scene_create": (C.c_int, [C.POINTER(NraysSceneDesc), C.POINTER(C.c_void_p)]),
    "nrays_render": (C.c_int, [C.c_void_p, C.POINTER(NraysRenderParams), C.POINTER(C.c_float)]),
    "nrays_render_rgb8": (C.c_int, [C.c_void_p, C.POINTER(NraysRenderParams), C.POINTER(C.c_uint8)]),
    "nrays_render_device": (C.c_int, [C.c_void_p, C.POINTER(NraysRenderParams), C.c_void_p, C.c_void_p]),
    "nrays_render_device_instrumented": (C.c_int, [C.c_void_p, C.POINTER(NraysRenderParams), C.c_void_p, C.c_void_p]),
    "nrays_render_device_counted": (C.c_int, [C.c_void_p, C.POINTER(NraysRenderParams), C.c_void_p, C.c_void_p, C.c_uint32]),
    "nrays_tile_rows": (C.c_uint32, [C.POINTER(NraysRenderParams)]),
    "nrays_untile_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
    "nrays_get_stats": (C.c_int, [C.c_void_p, C.POINTER(NraysStats)]),
    "nrays_get_primary_kernel_stats": (C.c_int, [C.c_void_p, C.POINTER(NraysStats)]),
    "nrays_scene_device_bytes": (C.c_uint64, [C.c_void_p]),
    "nrays_scene_destroy": (None, [C.c_void_p]),
    "nrays_comm_unique_id": (C.c_int, [C.POINTER(C.c_uint8)]),
    "nrays_comm_create": (C.c_int, [C.POINTER(C.c_uint8), C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p)]),
    "nrays_comm_create_local": (C.c_int, [C.c_uint32, C.POINTER(C.c_int32), C.POINTER(C.c_void_p)]),
    "nrays_comm_owners": (C.c_uint32, [C.c_void_p]),
    "nrays_comm_destroy": (None, [C.c_void_p]),
    "nrays_scene_set_create": (C.c_int, [C.POINTER(NraysSceneDesc), C.c_void_p, C.POINTER(C.c_void_p)]),
    "nrays_scene_set_destroy": (None, [C.c_void_p]),
    "nrays_scene_set_num_local": (C.c_uint32, [C.c_void_p]),
    "nrays_scene_set_local_scene": (C.c_void_p, [C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]),
    "nrays_render_multi": (C.c_int, [C.c_void_p, C.POINTER(NraysRenderParams), C.POINTER(C.c_float)]),
    "nrays_render_multi_device": (C.c_int, [C.c_void_p, C.POINTER(NraysRenderParams), C.c_void_p]),
    "nrays_multi_sync": (C.c_int, [C.c_void_p]),
    "nrays_multi_get_stats": (C.c_int, [C.c_void_p, C.POINTER(NraysStats)]),
    "nrays_multi_get_timings": (C.c_int, [C.c_void_p, C.POINTER(NraysMultiTimings)]),
    "nrays_last_error": (C.c_char_p, []),
    "nrays_abi_version": (C.c_uint32, []),
}

# Added after ABI version 7 without a bump: an older version-7 library (NRAYS_HIP_LIB: A/B runs against a parent build) may lack them.
POST_V7_SYMBOLS = ("nrays_trace_rays_device_ex", "nrays_trace_rays_ex", "nrays_intersects_rays_device_ex", "nrays_debug_ray_order",
                   "nrays_cast_rays_device", "nrays_cast_rays", "nrays_shade_points_device", "nrays_shade_points", "nrays_occlusion_points_device",
                   "nrays_occlusion_points", "nrays_debug_occlusion_rays", "nrays_surface_texels_device", "nrays_surface_texels",
                   "nrays_debug_surface_texels_passes", "nrays_debug_pipeline_counts", "nrays_gather_points_device", "nrays_gather_points",
                   "nrays_gather_points_device_ex", "nrays_gather_points_ex", "nrays_debug_gather_order", "nrays_dilate_texels_device", "nrays_dilate_texels",
                   "nrays_debug_box_cull", "nrays_filter_texels_device", "nrays_filter_texels", "nrays_gather_sh_points_device", "nrays_gather_sh_points",
                   "nrays_debug_gather_sh_fold", "nrays_gather_maps_points_device", "nrays_gather_maps_points", "nrays_irradiance_points_device",
                   "nrays_irradiance_points", "nrays_probe_depth_points_device", "nrays_probe_depth_points", "nrays_irradiance_points_vis_device",
                   "nrays_irradiance_points_vis", "nrays_gather_maps_sh_points_device", "nrays_gather_maps_sh_points", "nrays_material_points_device",
                   "nrays_material_points", "nrays_nearest_points_device", "nrays_nearest_points", "nrays_debug_nearest_bound", "nrays_debug_scene_dump",
                   "nrays_light_points_device", "nrays_light_points", "nrays_debug_light_rays")
RAYS_UNORDERED = 1          # NRAYS_RAYS_UNORDERED
TEXELS_CENTRES = 1          # NRAYS_TEXELS_CENTRES
TEXELS_FLIP_NORMALS = 2     # NRAYS_TEXELS_FLIP_NORMALS
DILATE_MAX_RADIUS = 64       # NRAYS_DILATE_MAX_RADIUS
TEXEL_FILLED = 4            # NRAYS_TEXEL_FILLED
FILTER_MAX_STEP = 64        # NRAYS_FILTER_MAX_STEP
RAY_FRAME_DOUBLES = 20      # NRAYS_RAY_FRAME_DOUBLES

_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# NRAYS_HIP_LIB overrides the library path (kernel A/B tuning with tools/kbench.py only).
HIP_LIB_PATH = os.environ.get("NRAYS_HIP_LIB") or os.path.join(_REPO, "nrays_amd", "lib", "libnrays_hip.so")
HOST_LIB_PATH = os.path.join(_REPO, "nrays_amd", "lib", "libnrays_host.so")

_hip_lib = None


class NraysError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("nrays status %d: %s" % (status, message))
        self.status = status


def load_hip_lib():
    """Loads the HIP product library.  Fails loudly: there is no CPU fallback in the product path."""
    global _hip_lib
    if _hip_lib is not None:
        return _hip_lib
    if not os.path.exists(HIP_LIB_PATH):
        raise ImportError("libnrays_hip.so is not built (%s missing); run `python -c 'import __graft_entry__ as g; "
                          "g.build()'` — the nrays_amd product path has no CPU fallback" % HIP_LIB_PATH)
    # torch bundles its own libamdhip64.so (SONAME libamdhip64.so.7).  It must be loaded FIRST so that
    # this library's NEEDED libamdhip64.so.7 binds to the same HIP runtime; two runtimes in one process
    # cannot both own the GPU ("no HIP device visible").  torch is plumbing here: device memory,
    # streams and torch.distributed.
    import torch  # noqa: F401
    lib = C.CDLL(HIP_LIB_PATH)
    for name, (res, args) in HIP_SYMBOLS.items():
        if name in POST_V7_SYMBOLS and os.environ.get("NRAYS_HIP_LIB") and not hasattr(lib, name):
            continue  # an older library named explicitly: calling the missing entry point is an AttributeError then
        fn = getattr(lib, name)  # AttributeError if the export is missing
        fn.restype = res
        fn.argtypes = args
    if lib.nrays_abi_version() != ABI_VERSION:
        raise ImportError("libnrays_hip.so ABI version %d != %d" % (lib.nrays_abi_version(), ABI_VERSION))
    _hip_lib = lib
    return lib


def check(status):
    if status != OK:
        msg = load_hip_lib().nrays_last_error()
        raise NraysError(status, msg.decode() if msg else "?")
