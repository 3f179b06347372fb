"""nrays_amd — MI355X-native replacement for nrays' per-pixel trace loop (scene::render).

The package holds only what that path needs: the HIP kernels + C ABI (csrc/), the C++ host
front-end (host/), and this thin ctypes mirror of the reference's scene-model surface.
"""
from . import abi  # noqa: F401
from .scene import (Ball, Capsule, Cone, Cuboid, Cylinder, ImageData, Interpolation, Isometry3, Light,  # noqa: F401
                    NormalMaterial, Overflow, PhongMaterial, Plane, Scene, SceneDescriptor, SceneNode, Texture2d,
                    TriMesh, UVMaterial, CastHits, Occlusion, camera_rays, cast_rays, closest_hits, get_stats, hemisphere_dirs, intersects_rays, last_permutation, make_params,
                    occlusion_hits, occlusion_points, occlusion_ray_probe, occlusion_rays, ray_order, render, rotation_table, shade_hits, shade_points, shadow_rays, trace_rays,
                    SurfaceTexels, bake_indirect, bake_lightmap, gather_hits, gather_order, gather_points, gather_ray_keys, surface_texels, surface_texels_passes, surface_texels_ref, texel_coords,
                    dilate_texels, dilate_texels_ref, lightmap_texture, denoise_texels, filter_texels, filter_texels_ref,
                    gather_probes, gather_sh_fold, gather_sh_points, sh_basis, sh_fold_ref, sh_irradiance, sphere_dirs,
                    bake_bounces, gather_maps_hits, gather_maps_points, lightmap_sample_ref,
                    Irradiance, ProbeGrid, bake_probe_grid, irradiance_points, irradiance_points_ref, probe_grid_positions,
                    ProbeDepth, ProbeVisibility, bake_probe_visibility, oct_texel, probe_depth, probe_depth_points, probe_depth_ref, probe_valid_words,
                    GatherMapsSh, bake_probe_grid_maps, gather_maps_probes, gather_maps_sh_points,
                    MaterialTerms, indirect_points, material_hits, material_points, material_points_ref, texel_albedo,
                    NEAREST_BEHIND, NearestHits, ProbeClearance, nearest_bound_probe, nearest_box_bound_ref, nearest_points, nearest_points_ref, probe_clearance,
                    PointLighting, PointLights, light_hits, light_points, light_points_ref, light_ray_probe, light_rays, scene_point_lights, vpls_from_hits)
