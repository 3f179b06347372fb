//! `gpu` — the MI355X trace loop behind the reference's own types: `GpuScene::new(&Scene)` replaces the BVT builds of
//! `Scene::new` (src/scene.rs:119-133), `gpu::render` has the signature and the meaning of `scene::render`
//! (src/scene.rs:29-36) and returns the same `Image`; `gpu::render_multi` tiles the frame over the GPUs of the node.
//!
//! `SceneNode` holds `Box<RayCast>` / `Arc<Box<Material>>` trait objects (src/scene_node.rs:14-16), which cannot be
//! inspected after the fact, so the plain-data descriptor of a node is captured where the concrete types are still
//! known: in the generic `SceneNode::new<G>` (src/scene_node.rs:22-47, bound `G: FlattenShape` added by the patch)
//! and through `Material::flatten` (a defaulted trait method added by the patch; user-defined materials return `None`
//! and such scenes stay on the CPU path).
//!
//! Dialect: Rust 2015 / nalgebra 0.15 / ncollide3d 0.16, like the rest of the crate.  This file cannot be compiled in
//! the repository that ships it (no Rust toolchain there); shape accessor names follow the ncollide3d 0.16 documentation.

use std::collections::HashMap;
use std::ffi::CStr;
use std::os::raw::c_void;
use std::ptr;
use std::sync::Arc;

use na::{Matrix4, Point2, Point3, Point4, Vector2, Vector3};
use ncollide3d::query::Ray;
use ncollide3d::shape::{Ball, Capsule, Cone, Cuboid, Cylinder, Plane, TriMesh};

use gpu_ffi::*;
use image::Image;
use light::Light;
use ray_with_energy::RayWithEnergy;
use math::{Isometry, Point, Scalar};
use scene::{Scene, Vless};
use scene_node::SceneNode;
use texture2d::{ImageData, Interpolation, Overflow, Texture2d};

// ------------------------------------------------------------------------------------------------ shapes
/// What `SceneNode::new<G>` can still see of its geometry: the arguments the loader passed to the shape constructor
/// (examples/loader3d.rs:601,612,623,634,645,656,695).
#[derive(Clone)]
pub enum ShapeDesc {
    Ball { radius: Scalar },
    Cuboid { half_extents: Vector3<Scalar> },
    Cylinder { half_height: Scalar, radius: Scalar },
    Capsule { half_height: Scalar, radius: Scalar },
    Cone { half_height: Scalar, radius: Scalar },
    Plane { normal: Vector3<Scalar> },
    TriMesh(MeshData),
}

/// The buffers of a `TriMesh` (shared `Arc`s, nothing is copied until the scene is flattened).
#[derive(Clone)]
pub struct MeshData {
    pub vertices: Arc<Vec<Point3<Scalar>>>,
    pub indices: Arc<Vec<Point3<usize>>>,
    pub uvs: Option<Arc<Vec<Point2<Scalar>>>>,
}

/// Implemented for every shape the loader constructs; the bound `G: FlattenShape` on `SceneNode::new` makes any other
/// geometry a compile-time error instead of a silent CPU fallback.
pub trait FlattenShape {
    fn shape_desc(&self) -> ShapeDesc;
}

impl FlattenShape for Ball<Scalar> {
    fn shape_desc(&self) -> ShapeDesc {
        ShapeDesc::Ball { radius: self.radius() }
    }
}
impl FlattenShape for Cuboid<Scalar> {
    fn shape_desc(&self) -> ShapeDesc {
        ShapeDesc::Cuboid { half_extents: *self.half_extents() }
    }
}
impl FlattenShape for Cylinder<Scalar> {
    fn shape_desc(&self) -> ShapeDesc {
        ShapeDesc::Cylinder { half_height: self.half_height(), radius: self.radius() }
    }
}
impl FlattenShape for Capsule<Scalar> {
    fn shape_desc(&self) -> ShapeDesc {
        ShapeDesc::Capsule { half_height: self.half_height(), radius: self.radius() }
    }
}
impl FlattenShape for Cone<Scalar> {
    fn shape_desc(&self) -> ShapeDesc {
        ShapeDesc::Cone { half_height: self.half_height(), radius: self.radius() }
    }
}
impl FlattenShape for Plane<Scalar> {
    fn shape_desc(&self) -> ShapeDesc {
        ShapeDesc::Plane { normal: self.normal().unwrap() }
    }
}
impl FlattenShape for TriMesh<Scalar> {
    fn shape_desc(&self) -> ShapeDesc {
        ShapeDesc::TriMesh(MeshData {
            vertices: self.vertices().clone(),
            indices: self.indices().clone(),
            uvs: self.uvs().clone(),
        })
    }
}

// --------------------------------------------------------------------------------------------- materials
/// Plain-data form of a material; the two textures are still `Texture2d`s, the `TextureTable` turns them into indices.
pub struct MaterialDesc {
    pub kind: u32, // NRAYS_MAT_*
    pub ambiant: [f32; 3],
    pub diffuse: [f32; 3],
    pub specular: [f32; 3],
    pub shininess: f32,
    pub texture: Option<Texture2d>,
    pub alpha: Option<Texture2d>,
}

impl MaterialDesc {
    /// NormalMaterial / UVMaterial: the colour fields are ignored by the library.
    pub fn special(kind: u32) -> MaterialDesc {
        MaterialDesc { kind: kind, ambiant: [0.0; 3], diffuse: [0.0; 3], specular: [0.0; 3], shininess: 0.0, texture: None, alpha: None }
    }
}

/// De-duplicates textures by the address of their shared `ImageData` (the loader's TextureManager hands out one `Arc`
/// per file, src/texture2d.rs:28-48) and keeps the `Arc`s alive until the library has copied the texels.
pub struct TextureTable {
    index: HashMap<(usize, u32, u32), i32>,
    keep: Vec<Arc<ImageData>>,
    pub records: Vec<NraysTexture>,
}

impl TextureTable {
    pub fn new() -> TextureTable {
        TextureTable { index: HashMap::new(), keep: Vec::new(), records: Vec::new() }
    }

    /// Index of `tex` in the texture array of the descriptor (-1 for `None`).
    pub fn id_of(&mut self, tex: &Option<Texture2d>) -> i32 {
        let tex = match *tex {
            Some(ref t) => t,
            None => return -1,
        };
        let data = tex.data(); // &Arc<ImageData>, accessor added by the patch
        let interp = match *tex.interpolation() {
            Interpolation::Bilinear => NRAYS_INTERP_BILINEAR,
            Interpolation::Nearest => NRAYS_INTERP_NEAREST,
        };
        let overflow = match *tex.overflow() {
            Overflow::Wrap => NRAYS_OVERFLOW_WRAP,
            Overflow::ClampToEdges => NRAYS_OVERFLOW_CLAMP,
        };
        let key = (&**data as *const ImageData as usize, interp, overflow);
        if let Some(id) = self.index.get(&key) {
            return *id;
        }
        let dims: Vector2<usize> = data.dims();
        let pixels: &[Point4<f32>] = data.pixels(); // row 0 = bottom row: from_png already flipped Y (texture2d.rs:99-107)
        self.records.push(NraysTexture {
            width: dims.x as u32,
            height: dims.y as u32,
            format: NRAYS_TEXEL_RGBA32F, // Point4<f32> is four packed f32: the reference's own in-memory form
            interp: interp,
            overflow: overflow,
            reserved: 0,
            texels: pixels.as_ptr() as *const c_void,
        });
        self.keep.push(data.clone());
        let id = self.records.len() as i32 - 1;
        self.index.insert(key, id);
        id
    }
}

// ------------------------------------------------------------------------------------------- flat scene
/// Owns every array the `NraysSceneDesc` points into; may be dropped as soon as `nrays_scene_create` has returned
/// (the library copies everything).
pub struct FlatScene {
    lights: Vec<NraysLight>,
    materials: Vec<NraysMaterial>,
    textures: TextureTable,
    mesh_keep: Vec<MeshData>,
    mesh_indices: Vec<Vec<u32>>,
    meshes: Vec<NraysMesh>,
    nodes: Vec<NraysNode>,
    background: [f32; 3],
}

impl FlatScene {
    pub fn desc(&self) -> NraysSceneDesc {
        NraysSceneDesc {
            background: self.background,
            num_lights: self.lights.len() as u32,
            lights: self.lights.as_ptr(),
            num_materials: self.materials.len() as u32,
            materials: self.materials.as_ptr(),
            num_textures: self.textures.records.len() as u32,
            textures: self.textures.records.as_ptr(),
            num_meshes: self.meshes.len() as u32,
            meshes: self.meshes.as_ptr(),
            num_nodes: self.nodes.len() as u32,
            nodes: self.nodes.as_ptr(),
        }
    }
}

fn flatten_light(l: &Light) -> NraysLight {
    NraysLight {
        pos: [l.pos.x, l.pos.y, l.pos.z],
        radius: l.radius,
        racsample: l.racsample as u32, // already floor(sqrt(nsample)), src/light.rs:20
        color: [l.color.x, l.color.y, l.color.z],
    }
}

impl Scene {
    /// The scene as plain data.  `Err` names the first node whose material cannot cross the FFI (a user-defined
    /// `Material` impl): such a scene keeps rendering through `scene::render`.
    pub fn flatten(&self) -> Result<FlatScene, String> {
        let mut flat = FlatScene {
            lights: self.lights().iter().map(flatten_light).collect(),
            materials: Vec::new(),
            textures: TextureTable::new(),
            mesh_keep: Vec::new(),
            mesh_indices: Vec::new(),
            meshes: Vec::new(),
            nodes: Vec::new(),
            background: { let b = self.background(); [b.x, b.y, b.z] }, // accessor added by the patch
        };
        // one NraysMaterial per distinct material object (nodes share them through Arc, loader3d.rs:556)
        let mut material_ids: HashMap<usize, u32> = HashMap::new();
        // one NraysMesh per distinct (vertices, indices) pair: the loader gives every OBJ group its own TriMesh over the
        // shared vertex array (loader3d.rs:690-695)
        let mut mesh_ids: HashMap<(usize, usize), i32> = HashMap::new();

        for (i, node) in self.nodes().iter().enumerate() { // Vec<Arc<SceneNode>> kept by Scene::new (patch)
            let mkey = &**node.material as *const _ as *const u8 as usize;
            let material_id = match material_ids.get(&mkey) {
                Some(id) => *id,
                None => {
                    let d = match node.material.flatten() {
                        Some(d) => d,
                        None => return Err(format!("node {}: this Material implementation has no GPU form", i)),
                    };
                    let rec = NraysMaterial {
                        kind: d.kind,
                        ambiant: d.ambiant,
                        diffuse: d.diffuse,
                        specular: d.specular,
                        shininess: d.shininess,
                        texture_id: flat.textures.id_of(&d.texture),
                        alpha_texture_id: flat.textures.id_of(&d.alpha),
                    };
                    flat.materials.push(rec);
                    let id = flat.materials.len() as u32 - 1;
                    material_ids.insert(mkey, id);
                    id
                }
            };
            let (shape_kind, params, mesh_id) = match node.shape {
                ShapeDesc::Ball { radius } => (NRAYS_SHAPE_BALL, [radius, 0.0, 0.0], -1),
                ShapeDesc::Cuboid { half_extents: h } => (NRAYS_SHAPE_CUBOID, [h.x, h.y, h.z], -1),
                ShapeDesc::Cylinder { half_height, radius } => (NRAYS_SHAPE_CYLINDER, [half_height, radius, 0.0], -1),
                ShapeDesc::Capsule { half_height, radius } => (NRAYS_SHAPE_CAPSULE, [half_height, radius, 0.0], -1),
                ShapeDesc::Cone { half_height, radius } => (NRAYS_SHAPE_CONE, [half_height, radius, 0.0], -1),
                ShapeDesc::Plane { normal: n } => (NRAYS_SHAPE_PLANE, [n.x, n.y, n.z], -1),
                ShapeDesc::TriMesh(ref m) => {
                    let key = (&**m.vertices as *const Vec<Point3<Scalar>> as usize, &**m.indices as *const Vec<Point3<usize>> as usize);
                    let id = match mesh_ids.get(&key) {
                        Some(id) => *id,
                        None => {
                            // Point3<usize> -> 3 x u32 (the ABI's index type); Point3<f64> / Point2<f64> are packed f64
                            let idx: Vec<u32> = m.indices.iter().flat_map(|t| vec![t.x as u32, t.y as u32, t.z as u32]).collect();
                            flat.mesh_indices.push(idx);
                            flat.mesh_keep.push(m.clone());
                            let kept = flat.mesh_keep.last().unwrap();
                            flat.meshes.push(NraysMesh {
                                num_vertices: kept.vertices.len() as u32,
                                num_triangles: kept.indices.len() as u32,
                                vertices: kept.vertices.as_ptr() as *const f64,
                                uvs: match kept.uvs { Some(ref uv) => uv.as_ptr() as *const f64, None => ptr::null() },
                                indices: flat.mesh_indices.last().unwrap().as_ptr(),
                            });
                            let id = flat.meshes.len() as i32 - 1;
                            mesh_ids.insert(key, id);
                            id
                        }
                    };
                    (NRAYS_SHAPE_TRIMESH, [0.0; 3], id)
                }
            };
            let t = node.transform.translation.vector;
            let w = node.transform.rotation.scaled_axis(); // Isometry3::new(t, axisangle) round trip (loader3d.rs:552)
            flat.nodes.push(NraysNode {
                shape_kind: shape_kind,
                solid: node.solid as u32,
                params: params,
                translation: [t.x, t.y, t.z],
                axis_angle: [w.x, w.y, w.z],
                refl_mix: node.refl_mix,
                refl_atenuation: node.refl_atenuation,
                alpha: node.alpha,
                reserved0: 0.0,
                refr_coeff: node.refr_coeff,
                material_id: material_id,
                mesh_id: mesh_id,
            });
        }
        Ok(flat)
    }
}

// ------------------------------------------------------------------------------------------- the drop-in
fn last_error() -> String {
    unsafe { CStr::from_ptr(nrays_last_error()).to_string_lossy().into_owned() }
}

fn params(resolution: &Vless, ray_per_pixel: usize, window_width: Scalar, camera_eye: &Point, projection: &Matrix4<Scalar>) -> NraysRenderParams {
    assert!(ray_per_pixel > 0); // src/scene.rs:37
    let mut m = [0.0f64; 16];
    m.copy_from_slice(projection.as_slice()); // nalgebra stores Matrix4 column-major, which is what the ABI expects
    NraysRenderParams {
        width: resolution.x as u32,
        height: resolution.y as u32,
        ray_per_pixel: ray_per_pixel as u32,
        max_depth: 0, // the energy rule alone, as in the reference (scene.rs:204)
        window_width: window_width,
        camera_eye: [camera_eye.x, camera_eye.y, camera_eye.z],
        inv_proj_view: m,
        seed: 0,
        band_rows: 0,
        band_owner: 0,
        band_owners: 1,
        reserved: 0,
    }
}

/// One closest hit of `GpuScene::cast_rays`: what `SceneNode::cast` returns (src/scene_node.rs:51-54) and which node returned it.
pub struct CastHit {
    pub node: usize,             // index into scene.nodes()
    pub toi: f64,
    pub normal: Vector3<f64>,    // world space
    pub uvs: Option<Point2<f64>>,
    pub triangle: Option<usize>, // index of the triangle in its TriMesh; None for an analytic shape
}

/// One covered lattice point of `GpuScene::surface_texels`.
pub struct SurfaceTexel {
    pub point: Point3<f64>,
    pub normal: Vector3<f64>,
    pub uvs: Point2<f64>,
    pub triangle: usize,
}

/// One surface point of `GpuScene::shade_points`: the arguments of `Material::compute` (src/material.rs:8-16) besides the scene.
pub struct SurfacePoint {
    pub node: usize,              // index into scene.nodes(): selects the material
    pub point: Point3<f64>,       // world space
    pub normal: Vector3<f64>,     // unit length, as the casts return it
    pub view_dir: Vector3<f64>,   // ray.ray.dir: the direction the viewer looks along, towards the surface
    pub uvs: Option<Point2<f64>>,
}

/// What `GpuScene::material_points` returns for one surface point: the terms of its node's material without the lights, and the node's own constants.
pub struct MaterialTerms {
    pub ambient: Point4<f32>,     // Material::ambiant(pt, normal, uvs), src/material.rs:7
    pub diffuse: Vector3<f32>,    // diffuse_color ⊙ texture.sample(uvs); zeros for the Normal and UV materials
    pub specular: Vector3<f32>,   // specular_color; zeros for the Normal and UV materials
    pub shininess: f32,
    pub alpha: f64,               // the SceneNode's: alpha, refl_mix, refl_atenuation, refr_coeff (src/scene_node.rs:8-19)
    pub refl_mix: f64,
    pub refl_atenuation: f64,
    pub refr_coeff: f64,
}

/// What `GpuScene::nearest_points` returns for one query point whose nearest surface lies within its bound: ncollide's PointQuery beside the RayCast.
pub struct NearestSurface {
    pub dist: f64,                // the distance from the query point to `point`
    pub node: usize,              // index into scene.nodes()
    pub point: Point3<f64>,       // the nearest surface point, in world space
    pub normal: Vector3<f64>,     // the normal there, facing the query point
    pub uvs: Option<Point2<f64>>,
    pub prim: Option<usize>,      // the triangle's index in its mesh; None for an analytic shape
    pub behind: bool,             // the query point lies behind the surface: the back of the triangle's winding, inside a closed shape, under a plane
}

/// A scene resident on ONE GPU (the calling thread's current HIP device).
pub struct GpuScene {
    raw: *mut NraysScene,
}
unsafe impl Send for GpuScene {} // one handle must not be used from two threads AT THE SAME TIME (include/nrays_abi.h)

impl GpuScene {
    pub fn new(scene: &Scene) -> Result<GpuScene, String> {
        let v = unsafe { nrays_abi_version() };
        if v != NRAYS_ABI_VERSION { return Err(format!("libnrays_hip.so ABI version {} != {}", v, NRAYS_ABI_VERSION)); }
        let flat = scene.flatten()?;
        let desc = flat.desc();
        let mut raw = ptr::null_mut();
        if unsafe { nrays_scene_create(&desc, &mut raw) } != NRAYS_OK {
            return Err(last_error());
        }
        Ok(GpuScene { raw: raw }) // the library copied everything: `flat` drops here
    }

    pub fn stats(&self) -> NraysStats {
        let mut st = NraysStats::default();
        unsafe { nrays_get_stats(self.raw, &mut st) };
        st
    }

    /// `scene.trace(ray)` (src/scene.rs:163-193) for every ray of the batch, in one call (nrays_trace_rays, blocking).  `keys[i]`
    /// is ray i's RNG path key for area-light sampling (None: key i); `max_depth` 0 = the energy rule alone, as `trace` does.
    pub fn trace_rays(&self, rays: &[RayWithEnergy], keys: Option<&[u64]>, max_depth: u32) -> Result<Vec<Vector3<f32>>, String> {
        self.trace_rays_flags(rays, keys, max_depth, 0)
    }

    /// `trace_rays` for a batch that comes in no useful order (AO / baking rays, shuffled or gathered rays; NRAYS_RAYS_UNORDERED): the library
    /// may bin the rays by a spatial key on the device and trace them in that order.  The colours are bit-identical to `trace_rays`'.
    pub fn trace_rays_unordered(&self, rays: &[RayWithEnergy], keys: Option<&[u64]>, max_depth: u32) -> Result<Vec<Vector3<f32>>, String> {
        self.trace_rays_flags(rays, keys, max_depth, NRAYS_RAYS_UNORDERED)
    }

    fn trace_rays_flags(&self, rays: &[RayWithEnergy], keys: Option<&[u64]>, max_depth: u32, flags: u32) -> Result<Vec<Vector3<f32>>, String> {
        if let Some(k) = keys { if k.len() != rays.len() { return Err(format!("{} keys for {} rays", k.len(), rays.len())); } }
        let n = rays.len();
        let mut o = Vec::with_capacity(3 * n);
        let mut d = Vec::with_capacity(3 * n);
        let mut refr = Vec::with_capacity(n);
        let mut energy = Vec::with_capacity(n);
        for r in rays {
            o.extend_from_slice(&[r.ray.origin.x, r.ray.origin.y, r.ray.origin.z]);
            d.extend_from_slice(&[r.ray.dir.x, r.ray.dir.y, r.ray.dir.z]);
            refr.push(r.refr);
            energy.push(r.energy);
        }
        let mut px: Vec<Vector3<f32>> = vec![Vector3::new(0.0f32, 0.0, 0.0); n];
        let kp = keys.map(|k| k.as_ptr()).unwrap_or(ptr::null());
        let rc = unsafe { nrays_trace_rays_ex(self.raw, n as u32, o.as_ptr(), d.as_ptr(), refr.as_ptr(), energy.as_ptr(), kp, max_depth, px.as_mut_ptr() as *mut f32, flags) };
        if rc != NRAYS_OK { return Err(last_error()); }
        Ok(px)
    }

    /// `scene.intersects_ray(ray, max_toi)` (src/scene.rs:147-161) for n rays in DEVICE memory (nrays_intersects_rays_device): origins / dirs
    /// n x 3 f64, max_toi n f64, out_filter n x 3 f32, out_lit n u32 (1 = Some(filter), 0 = None), enqueued on `hip_stream`.
    pub unsafe fn intersects_rays(&self, n: u32, origins: *const f64, dirs: *const f64, max_toi: *const f64, out_filter: *mut f32, out_lit: *mut u32,
                                  hip_stream: *mut c_void) -> Result<(), String> {
        if nrays_intersects_rays_device(self.raw, n, origins, dirs, max_toi, out_filter, out_lit, hip_stream) != NRAYS_OK { return Err(last_error()); }
        Ok(())
    }

    /// `intersects_rays` for rays that come in no useful order (NRAYS_RAYS_UNORDERED, as `trace_rays_unordered`): the same results, bit for bit.
    pub unsafe fn intersects_rays_unordered(&self, n: u32, origins: *const f64, dirs: *const f64, max_toi: *const f64, out_filter: *mut f32, out_lit: *mut u32,
                                            hip_stream: *mut c_void) -> Result<(), String> {
        if nrays_intersects_rays_device_ex(self.raw, n, origins, dirs, max_toi, out_filter, out_lit, NRAYS_RAYS_UNORDERED, hip_stream) != NRAYS_OK { return Err(last_error()); }
        Ok(())
    }

    /// The closest-hit query of `scene.trace` (src/scene.rs:164-166, 262-283) with the record `SceneNode::cast` returns (src/scene_node.rs:51-54)
    /// for every ray of the batch, in one call (nrays_cast_rays, blocking): `None` where ray i meets nothing within `max_toi[i]` (no bounds:
    /// unbounded), otherwise the node's index in `scene.nodes()`, toi, world normal, uvs where the shape carries them, and the triangle's index in
    /// its mesh (`None` for an analytic shape).  `unordered`: the rays come in no useful order (NRAYS_RAYS_UNORDERED); the results are the same.
    pub fn cast_rays(&self, rays: &[Ray<Scalar>], max_toi: Option<&[f64]>, unordered: bool) -> Result<Vec<Option<CastHit>>, String> {
        if let Some(t) = max_toi { if t.len() != rays.len() { return Err(format!("{} bounds for {} rays", t.len(), rays.len())); } }
        let n = rays.len();
        let mut o = Vec::with_capacity(3 * n);
        let mut d = Vec::with_capacity(3 * n);
        for r in rays {
            o.extend_from_slice(&[r.origin.x, r.origin.y, r.origin.z]);
            d.extend_from_slice(&[r.dir.x, r.dir.y, r.dir.z]);
        }
        let (mut toi, mut node, mut normal, mut uv) = (vec![0.0f64; n], vec![0i32; n], vec![0.0f64; 3 * n], vec![0.0f64; 2 * n]);
        let (mut prim, mut flags) = (vec![0i32; n], vec![0u32; n]);
        let tp = max_toi.map(|t| t.as_ptr()).unwrap_or(ptr::null());
        let rc = unsafe {
            nrays_cast_rays(self.raw, n as u32, o.as_ptr(), d.as_ptr(), tp, toi.as_mut_ptr(), node.as_mut_ptr(), normal.as_mut_ptr(), uv.as_mut_ptr(), prim.as_mut_ptr(),
                            flags.as_mut_ptr(), if unordered { NRAYS_RAYS_UNORDERED } else { 0 })
        };
        if rc != NRAYS_OK { return Err(last_error()); }
        Ok((0..n).map(|i| if flags[i] & 1 == 0 { None } else {
            Some(CastHit {
                node: node[i] as usize, toi: toi[i], normal: Vector3::new(normal[3 * i], normal[3 * i + 1], normal[3 * i + 2]),
                uvs: if flags[i] & 2 != 0 { Some(Point2::new(uv[2 * i], uv[2 * i + 1])) } else { None },
                triangle: if prim[i] >= 0 { Some(prim[i] as usize) } else { None },
            })
        }).collect())
    }

    /// The surface of TriMesh node `node` at the points of a `width` x `height` lattice in its uv space — a light map's texels (nrays_surface_texels,
    /// blocking): per lattice point, row 0 = the smallest v, `None` where no triangle covers it, otherwise the world point, the world normal, the lattice
    /// point's own (u, v) and the triangle's index in the node's mesh.  `centres`: the lattice (x + 0.5) / width instead of x / (width - 1), the points where
    /// `Texture2d::sample` reads texel x.  The records are what `shade_points` and `occlusion_points` take: no mesh copy, rasteriser or upload on the host.
    pub fn surface_texels(&self, node: usize, width: u32, height: u32, centres: bool, flip_normals: bool) -> Result<Vec<Option<SurfaceTexel>>, String> {
        let n = width as usize * height as usize;
        let (mut p, mut nm, mut uv) = (vec![0.0f64; 3 * n], vec![0.0f64; 3 * n], vec![0.0f64; 2 * n]);
        let (mut prim, mut flags) = (vec![0i32; n], vec![0u32; n]);
        let f = if centres { NRAYS_TEXELS_CENTRES } else { 0 } | if flip_normals { NRAYS_TEXELS_FLIP_NORMALS } else { 0 };
        let rc = unsafe { nrays_surface_texels(self.raw, node as u32, width, height, p.as_mut_ptr(), nm.as_mut_ptr(), uv.as_mut_ptr(), ptr::null_mut(), prim.as_mut_ptr(), flags.as_mut_ptr(), f) };
        if rc != NRAYS_OK { return Err(last_error()); }
        Ok((0..n).map(|i| if flags[i] & 1 == 0 { None } else {
            Some(SurfaceTexel {
                point: Point3::new(p[3 * i], p[3 * i + 1], p[3 * i + 2]), normal: Vector3::new(nm[3 * i], nm[3 * i + 1], nm[3 * i + 2]),
                uvs: Point2::new(uv[2 * i], uv[2 * i + 1]), triangle: prim[i] as usize,
            })
        }).collect())
    }

    /// `surface_texels` into DEVICE memory (nrays_surface_texels_device), enqueued on `hip_stream` without synchronisation: out_points (n x 3 f64) and
    /// out_flags (n u32) for n = width * height; out_normals (n x 3 f64), out_uv (n x 2 f64), out_node and out_prim (n i32) may each be null.  The arrays
    /// pass unfiltered into `shade_points_device` (nodes, hit_flags, uvs) and `occlusion_points_device` (hit_flags).  `flags`: NRAYS_TEXELS_* bits.
    pub unsafe fn surface_texels_device(&self, node: u32, width: u32, height: u32, out_points: *mut f64, out_normals: *mut f64, out_uv: *mut f64, out_node: *mut i32,
                                        out_prim: *mut i32, out_flags: *mut u32, flags: u32, hip_stream: *mut c_void) -> Result<(), String> {
        if nrays_surface_texels_device(self.raw, node, width, height, out_points, out_normals, out_uv, out_node, out_prim, out_flags, flags, hip_stream) != NRAYS_OK { return Err(last_error()); }
        Ok(())
    }

    /// Gutter dilation of a `width` x `height` light map (nrays_dilate_texels, blocking): every texel whose `flags` word has bit 0 clear takes the
    /// `channels` (1 ..= 4) floats of the nearest covered texel within `radius` (1 ..= NRAYS_DILATE_MAX_RADIUS; a Euclidean disc, no wrap-around, the
    /// smaller index y * width + x among equals), in place in `values`; covered texels and texels with nothing in reach stay as they are.  `flags` are
    /// the flags of `surface_texels_device` as they come.  Returns per texel the index it was filled from, its own index where covered, -1 where
    /// nothing is in reach.  Bilinear sampling of the map needs `radius >= 2`.
    pub fn dilate_texels(&self, width: u32, height: u32, flags: &[u32], radius: u32, channels: u32, values: &mut [f32]) -> Result<Vec<i32>, String> {
        let n = width as usize * height as usize;
        if flags.len() != n || values.len() != n * channels as usize { return Err("dilate_texels: flags / values do not match width * height".into()); }
        let mut source = vec![0i32; n];
        let rc = unsafe { nrays_dilate_texels(self.raw, width, height, flags.as_ptr(), radius, channels, values.as_mut_ptr(), source.as_mut_ptr(), ptr::null_mut(), 0) };
        if rc != NRAYS_OK { return Err(last_error()); }
        Ok(source)
    }

    /// `dilate_texels` on DEVICE memory (nrays_dilate_texels_device), two launches enqueued on `hip_stream` without synchronisation, behind the calls that
    /// baked `values`: flags_in n u32; values (n x channels f32, in place), out_source (n i32) and out_flags (n u32: flags_in, | NRAYS_TEXEL_FILLED at a
    /// filled texel; may be flags_in itself) may each be null, not all three.
    pub unsafe fn dilate_texels_device(&self, width: u32, height: u32, flags_in: *const u32, radius: u32, channels: u32, values: *mut f32, out_source: *mut i32,
                                       out_flags: *mut u32, hip_stream: *mut c_void) -> Result<(), String> {
        if nrays_dilate_texels_device(self.raw, width, height, flags_in, radius, channels, values, out_source, out_flags, 0, hip_stream) != NRAYS_OK { return Err(last_error()); }
        Ok(())
    }

    /// One pass of the edge-aware filter that denoises a baked `width` x `height` light map (nrays_filter_texels, blocking): a 5 x 5 a-trous joint-bilateral
    /// filter with taps `step` (1 ..= NRAYS_FILTER_MAX_STEP) texels apart.  A texel whose `flags` word has bit 0 set becomes the weighted mean of the covered
    /// texels among its taps, weighted by the B3 spline, by the squared world distance (0 at `pos_radius`; f64::INFINITY: off) and by the cosine between the
    /// normals (0 at `normal_cos`, in [-1, 1)); every other texel keeps its words.  `flags`, `points`, `normals` (n x 3 f64) are those of
    /// `surface_texels_device` as they come; `values` holds `channels` (1 ..= 4) floats per texel.  Returns the filtered copy; passes with step 1, 2, 4
    /// after one another are the usual denoiser, between the gather and `dilate_texels`.
    pub fn filter_texels(&self, width: u32, height: u32, flags: &[u32], points: &[f64], normals: &[f64], channels: u32, values: &[f32], step: u32, pos_radius: f64,
                         normal_cos: f64) -> Result<Vec<f32>, String> {
        let n = width as usize * height as usize;
        if flags.len() != n || points.len() != 3 * n || normals.len() != 3 * n || values.len() != n * channels as usize {
            return Err("filter_texels: flags / points / normals / values do not match width * height".into());
        }
        let mut out = vec![0f32; values.len()];
        let rc = unsafe { nrays_filter_texels(self.raw, width, height, flags.as_ptr(), points.as_ptr(), normals.as_ptr(), channels, values.as_ptr(), out.as_mut_ptr(), step, pos_radius, normal_cos, 0) };
        if rc != NRAYS_OK { return Err(last_error()); }
        Ok(out)
    }

    /// `filter_texels` on DEVICE memory (nrays_filter_texels_device), one launch enqueued on `hip_stream` without synchronisation, behind the calls that baked
    /// `values_in`: flags_in n u32, points / normals n x 3 f64, values_in / values_out n x channels f32.  values_out must not be values_in; any other
    /// overlap of the two is undefined.
    pub unsafe fn filter_texels_device(&self, width: u32, height: u32, flags_in: *const u32, points: *const f64, normals: *const f64, channels: u32, values_in: *const f32,
                                       values_out: *mut f32, step: u32, pos_radius: f64, normal_cos: f64, hip_stream: *mut c_void) -> Result<(), String> {
        if nrays_filter_texels_device(self.raw, width, height, flags_in, points, normals, channels, values_in, values_out, step, pos_radius, normal_cos, 0, hip_stream) != NRAYS_OK { return Err(last_error()); }
        Ok(())
    }

    /// `cast_rays` for n rays in DEVICE memory (nrays_cast_rays_device), enqueued on `hip_stream` without synchronisation: origins / dirs n x 3 f64,
    /// max_toi n f64 or null, out_toi n f64, out_node n i32; out_normal (n x 3 f64), out_uv (n x 2 f64), out_prim (n i32) and out_flags (n u32) may
    /// each be null.  A miss writes node -1 and toi +inf.  `flags`: 0 or NRAYS_RAYS_UNORDERED.
    pub unsafe fn cast_rays_device(&self, n: u32, origins: *const f64, dirs: *const f64, max_toi: *const f64, out_toi: *mut f64, out_node: *mut i32, out_normal: *mut f64,
                                   out_uv: *mut f64, out_prim: *mut i32, out_flags: *mut u32, flags: u32, hip_stream: *mut c_void) -> Result<(), String> {
        if nrays_cast_rays_device(self.raw, n, origins, dirs, max_toi, out_toi, out_node, out_normal, out_uv, out_prim, out_flags, flags, hip_stream) != NRAYS_OK { return Err(last_error()); }
        Ok(())
    }

    /// `scene.nodes()[p.node].material.compute(ray, &p.point, &p.normal, &p.uvs, scene)` (src/material.rs:8-16, src/phong_material.rs:72-151) for every
    /// point of the batch, in one call (nrays_shade_points, blocking): the lit colour and the material's alpha as the reference's `Point4<f32>`, without
    /// a closest-hit traversal and without reflection or refraction.  Of the ray only `dir` (p.view_dir) and the RNG path key matter: `keys[i]` is point
    /// i's key for area-light sampling (None: key i).  A node index outside `scene.nodes()` gives (0, 0, 0, 0).
    pub fn shade_points(&self, points: &[SurfacePoint], keys: Option<&[u64]>) -> Result<Vec<Point4<f32>>, String> {
        if let Some(k) = keys { if k.len() != points.len() { return Err(format!("{} keys for {} points", k.len(), points.len())); } }
        let n = points.len();
        let (mut p, mut nm, mut v, mut uv) = (Vec::with_capacity(3 * n), Vec::with_capacity(3 * n), Vec::with_capacity(3 * n), Vec::with_capacity(2 * n));
        let (mut node, mut hf) = (Vec::with_capacity(n), Vec::with_capacity(n));
        for s in points {
            p.extend_from_slice(&[s.point.x, s.point.y, s.point.z]);
            nm.extend_from_slice(&[s.normal.x, s.normal.y, s.normal.z]);
            v.extend_from_slice(&[s.view_dir.x, s.view_dir.y, s.view_dir.z]);
            match s.uvs { Some(t) => { uv.extend_from_slice(&[t.x, t.y]); hf.push(3u32); } None => { uv.extend_from_slice(&[0.0, 0.0]); hf.push(1u32); } }
            node.push(if s.node <= i32::max_value() as usize { s.node as i32 } else { -1 });
        }
        let mut out: Vec<Point4<f32>> = vec![Point4::new(0.0f32, 0.0, 0.0, 0.0); n];
        let kp = keys.map(|k| k.as_ptr()).unwrap_or(ptr::null());
        let rc = unsafe { nrays_shade_points(self.raw, n as u32, p.as_ptr(), nm.as_ptr(), v.as_ptr(), uv.as_ptr(), node.as_ptr(), hf.as_ptr(), kp, out.as_mut_ptr() as *mut f32, 0) };
        if rc != NRAYS_OK { return Err(last_error()); }
        Ok(out)
    }

    /// `shade_points` for n points in DEVICE memory (nrays_shade_points_device), enqueued on `hip_stream` without synchronisation: points / normals /
    /// view_dirs n x 3 f64, uvs n x 2 f64 or null, nodes n i32 (what cast_rays_device wrote to out_node), hit_flags n u32 or null (its out_flags: bit 0
    /// clear = skipped, bit 1 = the point carries a uv), keys n u64 or null, out_rgba n x 4 f32.  Skipped points write (0, 0, 0, 0).
    pub unsafe fn shade_points_device(&self, n: u32, points: *const f64, normals: *const f64, view_dirs: *const f64, uvs: *const f64, nodes: *const i32, hit_flags: *const u32,
                                      keys: *const u64, out_rgba: *mut f32, hip_stream: *mut c_void) -> Result<(), String> {
        if nrays_shade_points_device(self.raw, n, points, normals, view_dirs, uvs, nodes, hit_flags, keys, out_rgba, 0, hip_stream) != NRAYS_OK { return Err(last_error()); }
        Ok(())
    }

    /// The terms of the points' materials without the lights, in one call (nrays_material_points, blocking): per point
    /// `scene.nodes()[p.node].material.ambiant(&p.point, &p.normal, &p.uvs)` (src/material.rs:7) as the reference's `Point4<f32>`, the diffuse reflectance
    /// `diffuse_color.component_mul(tex_color)` (src/phong_material.rs:120-121), (specular_color, shininess), and the node's (alpha, refl_mix, refl_atenuation,
    /// refr_coeff) as f64 — everything `Scene::trace` reads from a hit besides the lights.  Of a SurfacePoint only normal, uvs and node matter.  A node index
    /// outside `scene.nodes()` gives zeros.
    pub fn material_points(&self, points: &[SurfacePoint]) -> Result<Vec<MaterialTerms>, String> {
        let n = points.len();
        let (mut nm, mut uv, mut node, mut hf) = (Vec::with_capacity(3 * n), Vec::with_capacity(2 * n), Vec::with_capacity(n), Vec::with_capacity(n));
        for s in points {
            nm.extend_from_slice(&[s.normal.x, s.normal.y, s.normal.z]);
            match s.uvs { Some(t) => { uv.extend_from_slice(&[t.x, t.y]); hf.push(3u32); } None => { uv.extend_from_slice(&[0.0, 0.0]); hf.push(1u32); } }
            node.push(if s.node <= i32::max_value() as usize { s.node as i32 } else { -1 });
        }
        let (mut amb, mut dif, mut spec, mut nd) = (vec![0.0f32; 4 * n], vec![0.0f32; 3 * n], vec![0.0f32; 4 * n], vec![0.0f64; 4 * n]);
        let rc = unsafe { nrays_material_points(self.raw, n as u32, nm.as_ptr(), uv.as_ptr(), node.as_ptr(), hf.as_ptr(), amb.as_mut_ptr(), dif.as_mut_ptr(), spec.as_mut_ptr(), nd.as_mut_ptr(), 0) };
        if rc != NRAYS_OK { return Err(last_error()); }
        Ok((0..n).map(|i| MaterialTerms { ambient: Point4::new(amb[4 * i], amb[4 * i + 1], amb[4 * i + 2], amb[4 * i + 3]),
                                          diffuse: Vector3::new(dif[3 * i], dif[3 * i + 1], dif[3 * i + 2]),
                                          specular: Vector3::new(spec[4 * i], spec[4 * i + 1], spec[4 * i + 2]), shininess: spec[4 * i + 3],
                                          alpha: nd[4 * i], refl_mix: nd[4 * i + 1], refl_atenuation: nd[4 * i + 2], refr_coeff: nd[4 * i + 3] }).collect())
    }

    /// `material_points` for n points in DEVICE memory (nrays_material_points_device), enqueued on `hip_stream` without synchronisation: normals n x 3 f64 (may
    /// be null when out_ambient is), uvs n x 2 f64 or null, nodes n i32 (what cast_rays_device wrote to out_node), hit_flags n u32 or null (its out_flags: bit 0
    /// clear = skipped, bit 1 = the point carries a uv); out_ambient n x 4 f32, out_diffuse n x 3 f32, out_specular n x 4 f32, out_node n x 4 f64, each may be
    /// null, not all.  Skipped points write zeros.
    pub unsafe fn material_points_device(&self, n: u32, normals: *const f64, uvs: *const f64, nodes: *const i32, hit_flags: *const u32, out_ambient: *mut f32,
                                         out_diffuse: *mut f32, out_specular: *mut f32, out_node: *mut f64, hip_stream: *mut c_void) -> Result<(), String> {
        if nrays_material_points_device(self.raw, n, normals, uvs, nodes, hit_flags, out_ambient, out_diffuse, out_specular, out_node, 0, hip_stream) != NRAYS_OK { return Err(last_error()); }
        Ok(())
    }

    /// The nearest surface to caller-supplied points (nrays_nearest_points, blocking): per point the closest point over every node of the scene — triangles by
    /// Ericson's closest point, the analytic shapes in closed form —, None where nothing lies within `max_dist` (None: unbounded).  Defined bit for bit in
    /// include/nrays_abi.h; ties go to the smaller node, then the smaller triangle.  A `SurfacePoint` for `shade_points` / `material_points` follows from a result
    /// field by field.
    pub fn nearest_points(&self, points: &[Point3<f64>], max_dist: Option<f64>) -> Result<Vec<Option<NearestSurface>>, String> {
        let n = points.len();
        let mut p = Vec::with_capacity(3 * n);
        for q in points { p.extend_from_slice(&[q.x, q.y, q.z]); }
        let md: Option<Vec<f64>> = max_dist.map(|m| vec![m; n]);
        let (mut dist, mut node, mut pt, mut nm, mut uv, mut prim, mut fl) = (vec![0.0f64; n], vec![0i32; n], vec![0.0f64; 3 * n], vec![0.0f64; 3 * n], vec![0.0f64; 2 * n], vec![0i32; n], vec![0u32; n]);
        let rc = unsafe { nrays_nearest_points(self.raw, n as u32, p.as_ptr(), md.as_ref().map_or(ptr::null(), |m| m.as_ptr()), ptr::null(), dist.as_mut_ptr(), node.as_mut_ptr(), pt.as_mut_ptr(),
                                               nm.as_mut_ptr(), uv.as_mut_ptr(), prim.as_mut_ptr(), fl.as_mut_ptr(), 0) };
        if rc != NRAYS_OK { return Err(last_error()); }
        Ok((0..n).map(|i| if fl[i] & 1 == 0 { None } else { Some(NearestSurface {
            dist: dist[i], node: node[i] as usize, point: Point3::new(pt[3 * i], pt[3 * i + 1], pt[3 * i + 2]), normal: Vector3::new(nm[3 * i], nm[3 * i + 1], nm[3 * i + 2]),
            uvs: if fl[i] & 2 != 0 { Some(Point2::new(uv[2 * i], uv[2 * i + 1])) } else { None }, prim: if prim[i] >= 0 { Some(prim[i] as usize) } else { None }, behind: fl[i] & 4 != 0 }) }).collect())
    }

    /// `nearest_points` for n points in DEVICE memory (nrays_nearest_points_device), enqueued on `hip_stream` without synchronisation: points n x 3 f64, max_dist n f64
    /// or null, hit_flags n u32 or null (bit 0 clear = skipped); out_dist n f64 and out_node n i32 required; out_point / out_normal n x 3 f64, out_uv n x 2 f64,
    /// out_prim n i32, out_flags n u32 may each be null.  The outputs carry cast_rays_device's layouts and pass unfiltered into the calls at surface points.
    pub unsafe fn nearest_points_device(&self, n: u32, points: *const f64, max_dist: *const f64, hit_flags: *const u32, out_dist: *mut f64, out_node: *mut i32, out_point: *mut f64,
                                        out_normal: *mut f64, out_uv: *mut f64, out_prim: *mut i32, out_flags: *mut u32, hip_stream: *mut c_void) -> Result<(), String> {
        if nrays_nearest_points_device(self.raw, n, points, max_dist, hit_flags, out_dist, out_node, out_point, out_normal, out_uv, out_prim, out_flags, 0, hip_stream) != NRAYS_OK { return Err(last_error()); }
        Ok(())
    }

    /// Ambient occlusion at caller-supplied surface points (nrays_occlusion_points, blocking): for every (point, unit normal) the library builds
    /// `sample_dirs.len()` hemisphere rays on the device — `sample_dirs` are directions of a local frame whose z axis is the normal, `rotations` an optional
    /// table of (cos, sin) pairs one of which is picked per point by hashing `keys[i]` (None: key i) —, runs `Scene::intersects_ray` with `max_toi` on each
    /// from `point + normal * bias` and folds them: the mean colour filter of the rays (blocked rays count as black) and the number that got through.
    /// The rays are defined bit for bit in include/nrays_abi.h (NraysOcclusionParams).
    pub fn occlusion_points(&self, points: &[(Point3<f64>, Vector3<f64>)], sample_dirs: &[Vector3<f64>], rotations: &[(f64, f64)], bias: f64, max_toi: f64,
                            keys: Option<&[u64]>) -> Result<Vec<(Vector3<f32>, u32)>, String> {
        if let Some(k) = keys { if k.len() != points.len() { return Err(format!("{} keys for {} points", k.len(), points.len())); } }
        let n = points.len();
        let (mut p, mut nm) = (Vec::with_capacity(3 * n), Vec::with_capacity(3 * n));
        for (pt, normal) in points { p.extend_from_slice(&[pt.x, pt.y, pt.z]); nm.extend_from_slice(&[normal.x, normal.y, normal.z]); }
        let dirs: Vec<f64> = sample_dirs.iter().flat_map(|d| vec![d.x, d.y, d.z]).collect();
        let rot: Vec<f64> = rotations.iter().flat_map(|r| vec![r.0, r.1]).collect();
        let params = NraysOcclusionParams { num_dirs: sample_dirs.len() as u32, num_rotations: rotations.len() as u32, dirs: dirs.as_ptr(),
                                            rotations: if rot.is_empty() { ptr::null() } else { rot.as_ptr() }, bias, max_toi };
        let (mut filter, mut open) = (vec![0.0f32; 3 * n], vec![0u32; n]);
        let kp = keys.map(|k| k.as_ptr()).unwrap_or(ptr::null());
        let rc = unsafe { nrays_occlusion_points(self.raw, n as u32, p.as_ptr(), nm.as_ptr(), ptr::null(), kp, &params, filter.as_mut_ptr(), open.as_mut_ptr(), 0) };
        if rc != NRAYS_OK { return Err(last_error()); }
        Ok((0..n).map(|i| (Vector3::new(filter[3 * i], filter[3 * i + 1], filter[3 * i + 2]), open[i])).collect())
    }

    /// `occlusion_points` for n points in DEVICE memory (nrays_occlusion_points_device), enqueued on `hip_stream` without synchronisation: points / normals
    /// n x 3 f64, hit_flags n u32 or null (out_flags of cast_rays_device: bit 0 clear = skipped, zeros), keys n u64 or null, out_filter n x 3 f32, out_open
    /// n u32 or null.  `params` is host memory; its two tables are device memory.
    pub unsafe fn occlusion_points_device(&self, n: u32, points: *const f64, normals: *const f64, hit_flags: *const u32, keys: *const u64, params: &NraysOcclusionParams,
                                          out_filter: *mut f32, out_open: *mut u32, hip_stream: *mut c_void) -> Result<(), String> {
        if nrays_occlusion_points_device(self.raw, n, points, normals, hit_flags, keys, params, out_filter, out_open, 0, hip_stream) != NRAYS_OK { return Err(last_error()); }
        Ok(())
    }

    /// Direct light at caller-supplied surface points from a caller-supplied table of point lights (nrays_light_points, blocking): for every (point, unit normal)
    /// and every light (position, colour, optional unit emitter normal) the library builds the shadow ray on the device, weights it with the cosine at the point
    /// (times the emitter's cosine for a light with a normal, times 1 / max(d^2, min_dist^2) when `min_dist` is Some), runs `Scene::intersects_ray` on the rays
    /// whose weight is > 0 and sums colour * (filter * weight) over the open ones in the table's order.  Per point: the sum, the lights that got a ray, the open ones.
    /// The scene's own lights are not read.  The arithmetic is defined bit for bit in include/nrays_abi.h (NraysPointLights).
    pub fn light_points(&self, points: &[(Point3<f64>, Vector3<f64>)], lights: &[(Point3<f64>, Vector3<f32>)], emitter_normals: Option<&[Vector3<f64>]>, min_dist: Option<f64>,
                        bias: f64, offset: f64) -> Result<Vec<(Vector3<f32>, u32, u32)>, String> {
        if let Some(e) = emitter_normals { if e.len() != lights.len() { return Err(format!("{} emitter normals for {} lights", e.len(), lights.len())); } }
        let n = points.len();
        let (mut p, mut nm) = (Vec::with_capacity(3 * n), Vec::with_capacity(3 * n));
        for (pt, normal) in points { p.extend_from_slice(&[pt.x, pt.y, pt.z]); nm.extend_from_slice(&[normal.x, normal.y, normal.z]); }
        let pos: Vec<f64> = lights.iter().flat_map(|l| vec![l.0.x, l.0.y, l.0.z]).collect();
        let col: Vec<f32> = lights.iter().flat_map(|l| vec![l.1.x, l.1.y, l.1.z]).collect();
        let en: Vec<f64> = emitter_normals.map(|e| e.iter().flat_map(|v| vec![v.x, v.y, v.z]).collect()).unwrap_or_default();
        let table = NraysPointLights { num_lights: lights.len() as u32, flags: if min_dist.is_some() { NRAYS_LIGHTS_INVERSE_SQUARE } else { 0 }, positions: pos.as_ptr(),
                                       colors: col.as_ptr(), normals: if emitter_normals.is_some() { en.as_ptr() } else { ptr::null() }, bias, offset,
                                       min_dist: min_dist.unwrap_or(1.0) };
        let (mut rgb, mut counts) = (vec![0.0f32; 3 * n], vec![0u32; 2 * n]);
        let rc = unsafe { nrays_light_points(self.raw, n as u32, p.as_ptr(), nm.as_ptr(), ptr::null(), &table, rgb.as_mut_ptr(), counts.as_mut_ptr(), 0) };
        if rc != NRAYS_OK { return Err(last_error()); }
        Ok((0..n).map(|i| (Vector3::new(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]), counts[2 * i], counts[2 * i + 1])).collect())
    }

    /// `light_points` for n points in DEVICE memory (nrays_light_points_device), enqueued on `hip_stream` without synchronisation: points / normals n x 3 f64,
    /// hit_flags n u32 or null (out_flags of cast_rays_device or surface_texels_device: bit 0 clear = skipped, zeros), out_rgb n x 3 f32, out_counts n x 2 u32 or
    /// null.  `lights` is host memory; its three tables are device memory.
    pub unsafe fn light_points_device(&self, n: u32, points: *const f64, normals: *const f64, hit_flags: *const u32, lights: &NraysPointLights, out_rgb: *mut f32,
                                      out_counts: *mut u32, hip_stream: *mut c_void) -> Result<(), String> {
        if nrays_light_points_device(self.raw, n, points, normals, hit_flags, lights, out_rgb, out_counts, 0, hip_stream) != NRAYS_OK { return Err(last_error()); }
        Ok(())
    }

    /// The light arriving at caller-supplied surface points from the rest of the scene (nrays_gather_points, blocking): the rays of `occlusion_points` with the
    /// same tables, `bias` and keys, each traced with `Scene::trace` as a `RayWithEnergy` of the given `energy` (`max_depth` as in `render`; its RNG key is
    /// hashed from the point's key and the ray's index), the colours summed in order and divided by their number: one mean colour per point, a light map's
    /// indirect term.  The value is defined in include/nrays_abi.h (NraysGatherParams).
    pub fn gather_points(&self, points: &[(Point3<f64>, Vector3<f64>)], sample_dirs: &[Vector3<f64>], rotations: &[(f64, f64)], bias: f64, energy: f32, max_depth: u32,
                         keys: Option<&[u64]>) -> Result<Vec<Vector3<f32>>, String> {
        self.gather_points_flags(points, sample_dirs, rotations, bias, energy, max_depth, keys, 0)
    }

    /// `gather_points` for points that come in no useful order (NRAYS_RAYS_UNORDERED through nrays_gather_points_ex, as `trace_rays_unordered`): the library may
    /// bin a chunk's (point, direction) pairs by a spatial key on the device and trace them in that order.  The colours are bit-identical to `gather_points`'.
    pub fn gather_points_unordered(&self, points: &[(Point3<f64>, Vector3<f64>)], sample_dirs: &[Vector3<f64>], rotations: &[(f64, f64)], bias: f64, energy: f32,
                                   max_depth: u32, keys: Option<&[u64]>) -> Result<Vec<Vector3<f32>>, String> {
        self.gather_points_flags(points, sample_dirs, rotations, bias, energy, max_depth, keys, NRAYS_RAYS_UNORDERED)
    }

    fn gather_points_flags(&self, points: &[(Point3<f64>, Vector3<f64>)], sample_dirs: &[Vector3<f64>], rotations: &[(f64, f64)], bias: f64, energy: f32, max_depth: u32,
                           keys: Option<&[u64]>, flags: u32) -> Result<Vec<Vector3<f32>>, String> {
        if let Some(k) = keys { if k.len() != points.len() { return Err(format!("{} keys for {} points", k.len(), points.len())); } }
        let n = points.len();
        let (mut p, mut nm) = (Vec::with_capacity(3 * n), Vec::with_capacity(3 * n));
        for (pt, normal) in points { p.extend_from_slice(&[pt.x, pt.y, pt.z]); nm.extend_from_slice(&[normal.x, normal.y, normal.z]); }
        let dirs: Vec<f64> = sample_dirs.iter().flat_map(|d| vec![d.x, d.y, d.z]).collect();
        let rot: Vec<f64> = rotations.iter().flat_map(|r| vec![r.0, r.1]).collect();
        let params = NraysGatherParams { num_dirs: sample_dirs.len() as u32, num_rotations: rotations.len() as u32, dirs: dirs.as_ptr(),
                                         rotations: if rot.is_empty() { ptr::null() } else { rot.as_ptr() }, bias, energy, max_depth };
        let mut rgb = vec![0.0f32; 3 * n];
        let kp = keys.map(|k| k.as_ptr()).unwrap_or(ptr::null());
        let rc = unsafe {
            if flags == 0 { nrays_gather_points(self.raw, n as u32, p.as_ptr(), nm.as_ptr(), ptr::null(), kp, &params, rgb.as_mut_ptr(), 0) }
            else { nrays_gather_points_ex(self.raw, n as u32, p.as_ptr(), nm.as_ptr(), ptr::null(), kp, &params, rgb.as_mut_ptr(), flags) }
        };
        if rc != NRAYS_OK { return Err(last_error()); }
        Ok((0..n).map(|i| Vector3::new(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2])).collect())
    }

    /// `gather_points` for n points in DEVICE memory (nrays_gather_points_device), enqueued on `hip_stream`: points / normals n x 3 f64, hit_flags n u32 or null
    /// (bit 0 clear = skipped, zeros), keys n u64 or null, out_rgb n x 3 f32.  `params` is host memory; its two tables are device memory.
    pub unsafe fn gather_points_device(&self, n: u32, points: *const f64, normals: *const f64, hit_flags: *const u32, keys: *const u64, params: &NraysGatherParams,
                                       out_rgb: *mut f32, hip_stream: *mut c_void) -> Result<(), String> {
        if nrays_gather_points_device(self.raw, n, points, normals, hit_flags, keys, params, out_rgb, 0, hip_stream) != NRAYS_OK { return Err(last_error()); }
        Ok(())
    }

    /// `gather_points_device` under NRAYS_RAYS_UNORDERED (nrays_gather_points_device_ex): the same values, bit for bit.
    pub unsafe fn gather_points_device_unordered(&self, n: u32, points: *const f64, normals: *const f64, hit_flags: *const u32, keys: *const u64,
                                                 params: &NraysGatherParams, out_rgb: *mut f32, hip_stream: *mut c_void) -> Result<(), String> {
        if nrays_gather_points_device_ex(self.raw, n, points, normals, hit_flags, keys, params, out_rgb, NRAYS_RAYS_UNORDERED, hip_stream) != NRAYS_OK { return Err(last_error()); }
        Ok(())
    }

    /// The light that baked maps hold at the closest hits of the hemisphere rays of caller-supplied surface points (nrays_gather_maps_points, blocking): the rays
    /// of `occlusion_points` with the same tables, `bias` and keys, each through the closest-hit query of `cast_rays` with `max_toi`; a hit on a node whose
    /// `node_map` entry names one of `maps` (1 .. 16 records of float32 texels in host memory, row 0 the bottom row) brings that map's sample at the hit's uv, a
    /// ray that leaves the scene brings `miss`, every other hit black; the colours are summed in order and divided by their number: one bounce of a light-map
    /// baker.  `node_map` has one entry per scene node (-1: no map).  Returns the mean colours and, per point, the numbers of mapped and of missed rays.  The
    /// value is defined in include/nrays_abi.h (NraysGatherMapsParams).
    pub fn gather_maps_points(&self, points: &[(Point3<f64>, Vector3<f64>)], sample_dirs: &[Vector3<f64>], rotations: &[(f64, f64)], bias: f64, max_toi: f64,
                              maps: &[NraysTexture], node_map: &[i32], miss: [f32; 3], keys: Option<&[u64]>) -> Result<(Vec<Vector3<f32>>, Vec<(u32, u32)>), String> {
        if let Some(k) = keys { if k.len() != points.len() { return Err(format!("{} keys for {} points", k.len(), points.len())); } }
        if maps.is_empty() || maps.len() > NRAYS_GATHER_MAX_MAPS as usize { return Err(format!("{} maps: 1 .. {} are allowed", maps.len(), NRAYS_GATHER_MAX_MAPS)); }
        let n = points.len();
        let (mut p, mut nm) = (Vec::with_capacity(3 * n), Vec::with_capacity(3 * n));
        for (pt, normal) in points { p.extend_from_slice(&[pt.x, pt.y, pt.z]); nm.extend_from_slice(&[normal.x, normal.y, normal.z]); }
        let dirs: Vec<f64> = sample_dirs.iter().flat_map(|d| vec![d.x, d.y, d.z]).collect();
        let rot: Vec<f64> = rotations.iter().flat_map(|r| vec![r.0, r.1]).collect();
        let params = NraysGatherMapsParams { num_dirs: sample_dirs.len() as u32, num_rotations: rotations.len() as u32, dirs: dirs.as_ptr(),
                                             rotations: if rot.is_empty() { ptr::null() } else { rot.as_ptr() }, bias, max_toi, num_maps: maps.len() as u32,
                                             num_nodes: node_map.len() as u32, maps: maps.as_ptr(), node_map: node_map.as_ptr(), miss_rgb: miss };
        let mut rgb = vec![0.0f32; 3 * n];
        let mut counts = vec![0u32; 2 * n];
        let kp = keys.map(|k| k.as_ptr()).unwrap_or(ptr::null());
        let rc = unsafe { nrays_gather_maps_points(self.raw, n as u32, p.as_ptr(), nm.as_ptr(), ptr::null(), kp, &params, rgb.as_mut_ptr(), counts.as_mut_ptr(), 0) };
        if rc != NRAYS_OK { return Err(last_error()); }
        Ok(((0..n).map(|i| Vector3::new(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2])).collect(), (0..n).map(|i| (counts[2 * i], counts[2 * i + 1])).collect()))
    }

    /// `gather_maps_points` for n points in DEVICE memory (nrays_gather_maps_points_device), enqueued on `hip_stream`: the arrays of `gather_points_device`,
    /// out_counts n x 2 u32 or null.  `params` and its `maps` records are host memory; its two tables, `node_map` and the maps' texels are device memory.
    pub unsafe fn gather_maps_points_device(&self, n: u32, points: *const f64, normals: *const f64, hit_flags: *const u32, keys: *const u64,
                                            params: &NraysGatherMapsParams, out_rgb: *mut f32, out_counts: *mut u32, hip_stream: *mut c_void) -> Result<(), String> {
        if nrays_gather_maps_points_device(self.raw, n, points, normals, hit_flags, keys, params, out_rgb, out_counts, 0, hip_stream) != NRAYS_OK { return Err(last_error()); }
        Ok(())
    }

    /// The gathered light of `gather_points` kept by direction (nrays_gather_sh_points, blocking): per point the projection of its rays' colours onto the real
    /// spherical harmonics of bands 0 .. `bands` - 1 (1 ..= 3; C = bands * bands coefficients), `out[i][c]` = coefficient c of point i as an RGB vector.  No measure
    /// is applied: multiply by 4 pi for uniform sphere directions.  An irradiance probe is a point with normal (0, 0, 1), bias 0 and no rotations under a table
    /// of sphere directions.  The value is defined in include/nrays_abi.h (nrays_gather_sh_points_device).
    pub fn gather_sh_points(&self, points: &[(Point3<f64>, Vector3<f64>)], sample_dirs: &[Vector3<f64>], rotations: &[(f64, f64)], bias: f64, energy: f32, max_depth: u32,
                            bands: u32, keys: Option<&[u64]>) -> Result<Vec<Vec<Vector3<f32>>>, String> {
        self.gather_sh_points_flags(points, sample_dirs, rotations, bias, energy, max_depth, bands, keys, 0)
    }

    /// `gather_sh_points` for points that come in no useful order (NRAYS_RAYS_UNORDERED, as `gather_points_unordered`): the same values, bit for bit.
    pub fn gather_sh_points_unordered(&self, points: &[(Point3<f64>, Vector3<f64>)], sample_dirs: &[Vector3<f64>], rotations: &[(f64, f64)], bias: f64, energy: f32,
                                      max_depth: u32, bands: u32, keys: Option<&[u64]>) -> Result<Vec<Vec<Vector3<f32>>>, String> {
        self.gather_sh_points_flags(points, sample_dirs, rotations, bias, energy, max_depth, bands, keys, NRAYS_RAYS_UNORDERED)
    }

    fn gather_sh_points_flags(&self, points: &[(Point3<f64>, Vector3<f64>)], sample_dirs: &[Vector3<f64>], rotations: &[(f64, f64)], bias: f64, energy: f32, max_depth: u32,
                              bands: u32, keys: Option<&[u64]>, flags: u32) -> Result<Vec<Vec<Vector3<f32>>>, String> {
        if let Some(k) = keys { if k.len() != points.len() { return Err(format!("{} keys for {} points", k.len(), points.len())); } }
        if bands < 1 || bands > 3 { return Err(format!("bands must be in 1 ..= 3, got {}", bands)); }
        let (n, c) = (points.len(), (bands * bands) as usize);
        let (mut p, mut nm) = (Vec::with_capacity(3 * n), Vec::with_capacity(3 * n));
        for (pt, normal) in points { p.extend_from_slice(&[pt.x, pt.y, pt.z]); nm.extend_from_slice(&[normal.x, normal.y, normal.z]); }
        let dirs: Vec<f64> = sample_dirs.iter().flat_map(|d| vec![d.x, d.y, d.z]).collect();
        let rot: Vec<f64> = rotations.iter().flat_map(|r| vec![r.0, r.1]).collect();
        let params = NraysGatherParams { num_dirs: sample_dirs.len() as u32, num_rotations: rotations.len() as u32, dirs: dirs.as_ptr(),
                                         rotations: if rot.is_empty() { ptr::null() } else { rot.as_ptr() }, bias, energy, max_depth };
        let mut sh = vec![0.0f32; 3 * c * n];
        let kp = keys.map(|k| k.as_ptr()).unwrap_or(ptr::null());
        let rc = unsafe { nrays_gather_sh_points(self.raw, n as u32, p.as_ptr(), nm.as_ptr(), ptr::null(), kp, &params, bands, sh.as_mut_ptr(), flags) };
        if rc != NRAYS_OK { return Err(last_error()); }
        Ok((0..n).map(|i| (0..c).map(|q| { let o = 3 * (i * c + q); Vector3::new(sh[o], sh[o + 1], sh[o + 2]) }).collect()).collect())
    }

    /// `gather_sh_points` for n points in DEVICE memory (nrays_gather_sh_points_device), enqueued on `hip_stream`: the arrays of `gather_points_device`, out_sh
    /// n x bands^2 x 3 f32.  `unordered` passes NRAYS_RAYS_UNORDERED.  `params` is host memory; its two tables are device memory.
    pub unsafe fn gather_sh_points_device(&self, n: u32, points: *const f64, normals: *const f64, hit_flags: *const u32, keys: *const u64, params: &NraysGatherParams,
                                          bands: u32, out_sh: *mut f32, unordered: bool, hip_stream: *mut c_void) -> Result<(), String> {
        let flags = if unordered { NRAYS_RAYS_UNORDERED } else { 0 };
        if nrays_gather_sh_points_device(self.raw, n, points, normals, hit_flags, keys, params, bands, out_sh, flags, hip_stream) != NRAYS_OK { return Err(last_error()); }
        Ok(())
    }

    /// The irradiance at caller-supplied points with normals from a regular grid of the probes `gather_sh_points` writes (nrays_irradiance_points, blocking): the
    /// eight probes around a point blended with trilinear weights, folded with the cosine lobe at the normal and multiplied by `measure` (4 pi for sphere
    /// directions).  Probe (ix, iy, iz) sits at origin + (ix, iy, iz) * cell and is row (iz * counts[1] + iy) * counts[0] + ix of `sh` (P x bands^2 x 3 f32);
    /// `valid` (P words, bit 0 clear: the probe is never read) leaves probes out — which ones is the caller's to decide, from the counts of `probe_depth_points`; `facing` holds down probes behind the
    /// surface.  Returns per point the colour and the sum of its weights (0: no probe counted).  The value is defined in include/nrays_abi.h (NraysIrradianceGrid).
    pub fn irradiance_points(&self, points: &[(Point3<f64>, Vector3<f64>)], origin: [f64; 3], cell: [f64; 3], counts: [u32; 3], bands: u32, sh: &[f32], valid: Option<&[u32]>,
                             measure: f32, facing: bool) -> Result<(Vec<Vector3<f32>>, Vec<f32>), String> {
        if bands < 1 || bands > 3 { return Err(format!("bands must be in 1 ..= 3, got {}", bands)); }
        let probes = counts.iter().map(|&c| c as usize).product::<usize>();
        if counts.iter().any(|&c| c < 1 || c > 1024) || probes > 1 << 22 { return Err(format!("counts must be in 1 ..= 1024 with a product <= 2^22, got {:?}", counts)); }
        if sh.len() != probes * (bands * bands) as usize * 3 { return Err(format!("{} coefficients for {} probes of {} bands", sh.len(), probes, bands)); }
        if let Some(v) = valid { if v.len() != probes { return Err(format!("{} validity words for {} probes", v.len(), probes)); } }
        let n = points.len();
        let (mut p, mut nm) = (Vec::with_capacity(3 * n), Vec::with_capacity(3 * n));
        for (pt, normal) in points { p.extend_from_slice(&[pt.x, pt.y, pt.z]); nm.extend_from_slice(&[normal.x, normal.y, normal.z]); }
        let grid = NraysIrradianceGrid { origin, cell, counts, bands, sh: sh.as_ptr(), valid: valid.map(|v| v.as_ptr()).unwrap_or(ptr::null()), measure, reserved: 0 };
        let mut rgb = vec![0.0f32; 3 * n];
        let mut weight = vec![0.0f32; n];
        let flags = if facing { NRAYS_IRRADIANCE_FACING } else { 0 };
        let rc = unsafe { nrays_irradiance_points(self.raw, n as u32, p.as_ptr(), nm.as_ptr(), ptr::null(), &grid, rgb.as_mut_ptr(), ptr::null_mut(), weight.as_mut_ptr(), flags) };
        if rc != NRAYS_OK { return Err(last_error()); }
        Ok(((0..n).map(|i| Vector3::new(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2])).collect(), weight))
    }

    /// `irradiance_points` for n points in DEVICE memory (nrays_irradiance_points_device), enqueued on `hip_stream`: points / normals n x 3 f64, hit_flags n u32 or
    /// null, out_rgb n x 3, out_sh n x bands^2 x 3 and out_weight n f32, each or null (out_rgb or out_sh is required).  `grid` is host memory; its `sh` and `valid`
    /// are device memory.
    pub unsafe fn irradiance_points_device(&self, n: u32, points: *const f64, normals: *const f64, hit_flags: *const u32, grid: &NraysIrradianceGrid, out_rgb: *mut f32,
                                           out_sh: *mut f32, out_weight: *mut f32, facing: bool, hip_stream: *mut c_void) -> Result<(), String> {
        let flags = if facing { NRAYS_IRRADIANCE_FACING } else { 0 };
        if nrays_irradiance_points_device(self.raw, n, points, normals, hit_flags, grid, out_rgb, out_sh, out_weight, flags, hip_stream) != NRAYS_OK { return Err(last_error()); }
        Ok(())
    }

    /// `irradiance_points` with visibility (nrays_irradiance_points_vis, blocking): `moments` (P x res^2 x 2 f32, what `probe_depth_points` writes at the grid's
    /// probes, rows as `sh`; res 4, 8 or 16) hold down a valid probe whose mean depth towards a point is shorter than the point's distance — Chebyshev's bound,
    /// cubed, never below `floor` (in [0, 1]); `vis_bias` moves a point along its normal before that distance is taken.  The value is defined in
    /// include/nrays_abi.h (NraysIrradianceVisibility).
    pub fn irradiance_points_vis(&self, points: &[(Point3<f64>, Vector3<f64>)], origin: [f64; 3], cell: [f64; 3], counts: [u32; 3], bands: u32, sh: &[f32], valid: Option<&[u32]>,
                                 measure: f32, facing: bool, moments: &[f32], res: u32, floor: f32, vis_bias: f64) -> Result<(Vec<Vector3<f32>>, Vec<f32>), String> {
        if bands < 1 || bands > 3 { return Err(format!("bands must be in 1 ..= 3, got {}", bands)); }
        if res != 4 && res != 8 && res != 16 { return Err(format!("res must be 4, 8 or 16, got {}", res)); }
        let probes = counts.iter().map(|&c| c as usize).product::<usize>();
        if counts.iter().any(|&c| c < 1 || c > 1024) || probes > 1 << 22 { return Err(format!("counts must be in 1 ..= 1024 with a product <= 2^22, got {:?}", counts)); }
        if sh.len() != probes * (bands * bands) as usize * 3 { return Err(format!("{} coefficients for {} probes of {} bands", sh.len(), probes, bands)); }
        if moments.len() != probes * (res * res) as usize * 2 { return Err(format!("{} moments for {} probes at res {}", moments.len(), probes, res)); }
        if let Some(v) = valid { if v.len() != probes { return Err(format!("{} validity words for {} probes", v.len(), probes)); } }
        let n = points.len();
        let (mut p, mut nm) = (Vec::with_capacity(3 * n), Vec::with_capacity(3 * n));
        for (pt, normal) in points { p.extend_from_slice(&[pt.x, pt.y, pt.z]); nm.extend_from_slice(&[normal.x, normal.y, normal.z]); }
        let grid = NraysIrradianceGrid { origin, cell, counts, bands, sh: sh.as_ptr(), valid: valid.map(|v| v.as_ptr()).unwrap_or(ptr::null()), measure, reserved: 0 };
        let vis = NraysIrradianceVisibility { moments: moments.as_ptr(), res, floor, bias: vis_bias };
        let mut rgb = vec![0.0f32; 3 * n];
        let mut weight = vec![0.0f32; n];
        let flags = if facing { NRAYS_IRRADIANCE_FACING } else { 0 };
        let rc = unsafe { nrays_irradiance_points_vis(self.raw, n as u32, p.as_ptr(), nm.as_ptr(), ptr::null(), &grid, &vis, rgb.as_mut_ptr(), ptr::null_mut(), weight.as_mut_ptr(), flags) };
        if rc != NRAYS_OK { return Err(last_error()); }
        Ok(((0..n).map(|i| Vector3::new(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2])).collect(), weight))
    }

    /// `irradiance_points_vis` for n points in DEVICE memory (nrays_irradiance_points_vis_device), enqueued on `hip_stream`: the arrays of
    /// `irradiance_points_device`.  `grid` and `vis` are host memory; `sh`, `valid` and `moments` are device memory.
    pub unsafe fn irradiance_points_vis_device(&self, n: u32, points: *const f64, normals: *const f64, hit_flags: *const u32, grid: &NraysIrradianceGrid,
                                               vis: &NraysIrradianceVisibility, out_rgb: *mut f32, out_sh: *mut f32, out_weight: *mut f32, facing: bool,
                                               hip_stream: *mut c_void) -> Result<(), String> {
        let flags = if facing { NRAYS_IRRADIANCE_FACING } else { 0 };
        if nrays_irradiance_points_vis_device(self.raw, n, points, normals, hit_flags, grid, vis, out_rgb, out_sh, out_weight, flags, hip_stream) != NRAYS_OK { return Err(last_error()); }
        Ok(())
    }

    /// What caller-supplied points see of the geometry around them (nrays_probe_depth_points, blocking): the rays of `occlusion_points` with the same tables, `bias`
    /// and keys, each through the closest-hit query of `cast_rays`; per point res x res (4, 8 or 16) octahedral texels of the mean and mean squared distance
    /// clamped to `max_dist` (the moments `irradiance_points_vis` reads), the numbers of rays that end closer than `near_dist` and of rays that hit nothing, the
    /// least distance (inf: none) and the index of its direction (u32::MAX: none).  A probe is a point with normal (0, 0, 1), bias 0 and no rotations.  The
    /// value is defined in include/nrays_abi.h (NraysProbeDepthParams).
    pub fn probe_depth_points(&self, points: &[(Point3<f64>, Vector3<f64>)], sample_dirs: &[Vector3<f64>], rotations: &[(f64, f64)], bias: f64, max_dist: f64, near_dist: f64,
                              res: u32, keys: Option<&[u64]>) -> Result<(Vec<f32>, Vec<(u32, u32)>, Vec<f64>, Vec<u32>), String> {
        if let Some(k) = keys { if k.len() != points.len() { return Err(format!("{} keys for {} points", k.len(), points.len())); } }
        if res != 4 && res != 8 && res != 16 { return Err(format!("res must be 4, 8 or 16, got {}", res)); }
        let n = points.len();
        let (mut p, mut nm) = (Vec::with_capacity(3 * n), Vec::with_capacity(3 * n));
        for (pt, normal) in points { p.extend_from_slice(&[pt.x, pt.y, pt.z]); nm.extend_from_slice(&[normal.x, normal.y, normal.z]); }
        let dirs: Vec<f64> = sample_dirs.iter().flat_map(|d| vec![d.x, d.y, d.z]).collect();
        let rot: Vec<f64> = rotations.iter().flat_map(|r| vec![r.0, r.1]).collect();
        let params = NraysProbeDepthParams { num_dirs: sample_dirs.len() as u32, num_rotations: rotations.len() as u32, dirs: dirs.as_ptr(),
                                             rotations: if rot.is_empty() { ptr::null() } else { rot.as_ptr() }, bias, max_dist, near_dist, res, reserved: 0 };
        let mut moments = vec![0.0f32; 2 * (res * res) as usize * n];
        let mut counts = vec![0u32; 2 * n];
        let mut nearest = vec![0.0f64; n];
        let mut nearest_dir = vec![0u32; n];
        let kp = keys.map(|k| k.as_ptr()).unwrap_or(ptr::null());
        let rc = unsafe { nrays_probe_depth_points(self.raw, n as u32, p.as_ptr(), nm.as_ptr(), ptr::null(), kp, &params, moments.as_mut_ptr(), counts.as_mut_ptr(),
                                                   nearest.as_mut_ptr(), nearest_dir.as_mut_ptr(), 0) };
        if rc != NRAYS_OK { return Err(last_error()); }
        Ok((moments, (0..n).map(|i| (counts[2 * i], counts[2 * i + 1])).collect(), nearest, nearest_dir))
    }

    /// `probe_depth_points` for n points in DEVICE memory (nrays_probe_depth_points_device), enqueued on `hip_stream`: the arrays of `gather_points_device`,
    /// out_moments n x res^2 x 2 f32; out_counts n x 2 u32, out_nearest n f64 and out_nearest_dir n u32, each or null.  `params` is host memory; its two tables
    /// are device memory.
    pub unsafe fn probe_depth_points_device(&self, n: u32, points: *const f64, normals: *const f64, hit_flags: *const u32, keys: *const u64, params: &NraysProbeDepthParams,
                                            out_moments: *mut f32, out_counts: *mut u32, out_nearest: *mut f64, out_nearest_dir: *mut u32,
                                            hip_stream: *mut c_void) -> Result<(), String> {
        if nrays_probe_depth_points_device(self.raw, n, points, normals, hit_flags, keys, params, out_moments, out_counts, out_nearest, out_nearest_dir, 0, hip_stream) != NRAYS_OK { return Err(last_error()); }
        Ok(())
    }

    /// Probes filled from baked maps, and what they see of the geometry, from one traversal of their rays (nrays_gather_maps_sh_points, blocking): the rays, the
    /// query, the maps and the colours of `gather_maps_points` (`max_toi` filters the colours and the counts only), folded as `gather_sh_points` folds its colours
    /// — `sh[i][c]` = coefficient c of point i as an RGB vector, C = bands * bands, no measure applied — with the numbers of mapped and of missed rays per point;
    /// with `depth` (max_dist, near_dist, res) also exactly what `probe_depth_points` returns for the same points, from the same query.  The value is defined in
    /// include/nrays_abi.h (nrays_gather_maps_sh_points_device).
    pub fn gather_maps_sh_points(&self, points: &[(Point3<f64>, Vector3<f64>)], sample_dirs: &[Vector3<f64>], rotations: &[(f64, f64)], bias: f64, max_toi: f64,
                                 maps: &[NraysTexture], node_map: &[i32], miss: [f32; 3], bands: u32, keys: Option<&[u64]>, depth: Option<(f64, f64, u32)>)
                                 -> Result<(Vec<Vec<Vector3<f32>>>, Vec<(u32, u32)>, Option<(Vec<f32>, Vec<(u32, u32)>, Vec<f64>, Vec<u32>)>), String> {
        if let Some(k) = keys { if k.len() != points.len() { return Err(format!("{} keys for {} points", k.len(), points.len())); } }
        if maps.is_empty() || maps.len() > NRAYS_GATHER_MAX_MAPS as usize { return Err(format!("{} maps: 1 .. {} are allowed", maps.len(), NRAYS_GATHER_MAX_MAPS)); }
        if bands < 1 || bands > 3 { return Err(format!("bands must be in 1 ..= 3, got {}", bands)); }
        if let Some((_, _, res)) = depth { if res != 4 && res != 8 && res != 16 { return Err(format!("res must be 4, 8 or 16, got {}", res)); } }
        let (n, c) = (points.len(), (bands * bands) as usize);
        let (mut p, mut nm) = (Vec::with_capacity(3 * n), Vec::with_capacity(3 * n));
        for (pt, normal) in points { p.extend_from_slice(&[pt.x, pt.y, pt.z]); nm.extend_from_slice(&[normal.x, normal.y, normal.z]); }
        let dirs: Vec<f64> = sample_dirs.iter().flat_map(|d| vec![d.x, d.y, d.z]).collect();
        let rot: Vec<f64> = rotations.iter().flat_map(|r| vec![r.0, r.1]).collect();
        let params = NraysGatherMapsParams { num_dirs: sample_dirs.len() as u32, num_rotations: rotations.len() as u32, dirs: dirs.as_ptr(),
                                             rotations: if rot.is_empty() { ptr::null() } else { rot.as_ptr() }, bias, max_toi, num_maps: maps.len() as u32,
                                             num_nodes: node_map.len() as u32, maps: maps.as_ptr(), node_map: node_map.as_ptr(), miss_rgb: miss };
        let spec = depth.map(|(max_dist, near_dist, res)| NraysGatherDepthSpec { max_dist, near_dist, res, reserved: 0 });
        let texels = spec.map(|s| (s.res * s.res) as usize).unwrap_or(0);
        let mut sh = vec![0.0f32; 3 * c * n];
        let mut counts = vec![0u32; 2 * n];
        let mut moments = vec![0.0f32; 2 * texels * n];
        let mut depth_counts = vec![0u32; 2 * n];
        let mut nearest = vec![0.0f64; n];
        let mut nearest_dir = vec![0u32; n];
        let kp = keys.map(|k| k.as_ptr()).unwrap_or(ptr::null());
        let rc = unsafe {
            match spec.as_ref() {
                Some(s) => nrays_gather_maps_sh_points(self.raw, n as u32, p.as_ptr(), nm.as_ptr(), ptr::null(), kp, &params, bands, sh.as_mut_ptr(), counts.as_mut_ptr(), s,
                                                       moments.as_mut_ptr(), depth_counts.as_mut_ptr(), nearest.as_mut_ptr(), nearest_dir.as_mut_ptr(), 0),
                None => nrays_gather_maps_sh_points(self.raw, n as u32, p.as_ptr(), nm.as_ptr(), ptr::null(), kp, &params, bands, sh.as_mut_ptr(), counts.as_mut_ptr(), ptr::null(),
                                                    ptr::null_mut(), ptr::null_mut(), ptr::null_mut(), ptr::null_mut(), 0),
            }
        };
        if rc != NRAYS_OK { return Err(last_error()); }
        let pairs = |w: &Vec<u32>| -> Vec<(u32, u32)> { (0..n).map(|i| (w[2 * i], w[2 * i + 1])).collect() };
        let sh_rows = (0..n).map(|i| (0..c).map(|k| { let at = 3 * (i * c + k); Vector3::new(sh[at], sh[at + 1], sh[at + 2]) }).collect()).collect();
        Ok((sh_rows, pairs(&counts), spec.map(|_| (moments, pairs(&depth_counts), nearest, nearest_dir))))
    }

    /// `gather_maps_sh_points` for n points in DEVICE memory (nrays_gather_maps_sh_points_device), enqueued on `hip_stream`: the arrays of
    /// `gather_maps_points_device`, out_sh n x bands^2 x 3 f32, out_counts n x 2 u32 or null.  `depth` None: the four depth outputs must be null; otherwise
    /// out_moments n x res^2 x 2 f32 is required and out_depth_counts, out_nearest, out_nearest_dir may each be null.  `params`, its `maps` records and `depth` are
    /// host memory; the two tables, `node_map` and the maps' texels are device memory.
    pub unsafe fn gather_maps_sh_points_device(&self, n: u32, points: *const f64, normals: *const f64, hit_flags: *const u32, keys: *const u64,
                                               params: &NraysGatherMapsParams, bands: u32, out_sh: *mut f32, out_counts: *mut u32, depth: Option<&NraysGatherDepthSpec>,
                                               out_moments: *mut f32, out_depth_counts: *mut u32, out_nearest: *mut f64, out_nearest_dir: *mut u32,
                                               hip_stream: *mut c_void) -> Result<(), String> {
        let spec = depth.map(|d| d as *const NraysGatherDepthSpec).unwrap_or(ptr::null());
        if nrays_gather_maps_sh_points_device(self.raw, n, points, normals, hit_flags, keys, params, bands, out_sh, out_counts, spec, out_moments, out_depth_counts, out_nearest, out_nearest_dir, 0, hip_stream) != NRAYS_OK { return Err(last_error()); }
        Ok(())
    }
}

impl Drop for GpuScene {
    fn drop(&mut self) {
        unsafe { nrays_scene_destroy(self.raw) }
    }
}

/// Same signature and meaning as `scene::render` (src/scene.rs:29-36), with the scene handle in place of `&Arc<Scene>`.
pub fn render(scene: &GpuScene, resolution: &Vless, ray_per_pixel: usize, window_width: Scalar, camera_eye: Point, projection: Matrix4<Scalar>) -> Image {
    let p = params(resolution, ray_per_pixel, window_width, &camera_eye, &projection);
    println!("Tracing {} rays.", (resolution.y * resolution.x * (ray_per_pixel as f64)) as i32);
    // Vector3<f32> is three packed f32: the frame is written straight into Image's pixel vector,
    // index i + j * resx (src/scene.rs:104)
    let mut px: Vec<Vector3<f32>> = vec![Vector3::new(0.0f32, 0.0, 0.0); (p.width as usize) * (p.height as usize)];
    if unsafe { nrays_render(scene.raw, &p, px.as_mut_ptr() as *mut f32) } != NRAYS_OK {
        panic!("nrays_render: {}", last_error());
    }
    Image::new(resolution.clone(), px)
}

/// The same frame already quantised as `Image::to_png` quantises it (src/image.rs:66-76: c * 255, clamped, truncated),
/// row-major RGB bytes — what loader3d hands to the PNG encoder, a quarter of the bytes over PCIe.
pub fn render_rgb8(scene: &GpuScene, resolution: &Vless, ray_per_pixel: usize, window_width: Scalar, camera_eye: Point, projection: Matrix4<Scalar>) -> Vec<u8> {
    let p = params(resolution, ray_per_pixel, window_width, &camera_eye, &projection);
    let mut px: Vec<u8> = vec![0u8; (p.width as usize) * (p.height as usize) * 3];
    if unsafe { nrays_render_rgb8(scene.raw, &p, px.as_mut_ptr()) } != NRAYS_OK {
        panic!("nrays_render_rgb8: {}", last_error());
    }
    px
}

/// A scene replicated on `num_gpus` GPUs of this node, driven by this one process (framebuffer bands + RCCL exchange
/// inside the library).
pub struct GpuSceneSet {
    comm: *mut NraysComm,
    set: *mut NraysSceneSet,
}
unsafe impl Send for GpuSceneSet {}

impl GpuSceneSet {
    pub fn new(scene: &Scene, num_gpus: u32) -> Result<GpuSceneSet, String> {
        let flat = scene.flatten()?;
        let desc = flat.desc();
        let mut comm = ptr::null_mut();
        if unsafe { nrays_comm_create_local(num_gpus, ptr::null(), &mut comm) } != NRAYS_OK {
            return Err(last_error());
        }
        let mut set = ptr::null_mut();
        if unsafe { nrays_scene_set_create(&desc, comm, &mut set) } != NRAYS_OK {
            let e = last_error();
            unsafe { nrays_comm_destroy(comm) };
            return Err(e);
        }
        Ok(GpuSceneSet { comm: comm, set: set })
    }
}

impl Drop for GpuSceneSet {
    fn drop(&mut self) {
        unsafe {
            nrays_scene_set_destroy(self.set);
            nrays_comm_destroy(self.comm);
        }
    }
}

/// `scene::render` on every GPU of the set; the frame is bit-identical to the single-GPU one.
pub fn render_multi(scene: &GpuSceneSet, resolution: &Vless, ray_per_pixel: usize, window_width: Scalar, camera_eye: Point, projection: Matrix4<Scalar>) -> Image {
    let p = params(resolution, ray_per_pixel, window_width, &camera_eye, &projection);
    let mut px: Vec<Vector3<f32>> = vec![Vector3::new(0.0f32, 0.0, 0.0); (p.width as usize) * (p.height as usize)];
    if unsafe { nrays_render_multi(scene.set, &p, px.as_mut_ptr() as *mut f32) } != NRAYS_OK {
        panic!("nrays_render_multi: {}", last_error());
    }
    Image::new(resolution.clone(), px)
}
