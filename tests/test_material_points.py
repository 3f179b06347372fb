"""The material terms at caller-supplied points (nrays_material_points_device / nrays_material_points; nrays_amd.material_points, material_hits, texel_albedo,
indirect_points, material_points_ref), the parts that need no GPU: the header, the ctypes table and the Rust declarations, the argument checks of the Python
wrappers, and the definition on its numpy mirror — against the CPU oracle's Material::compute bit for bit (tests/shade_oracle_shim.c), against the independent
restatement of Texture2d::sample (tests/texture_cases.py), the skip rule, and indirect_points in a furnace.  tests/test_material_points_gpu.py compares the device
with the mirror bit for bit and shares the scenes and point sets below."""
import ctypes as C
import math
import re
import subprocess

import numpy as np
import pytest

import nrays_amd as nr
import oracle
from nrays_amd import abi, math3d
from tests import texture_cases as tc
from tests.test_gather import FFI, GPU_RS, HEADER, HEADER_TEXT, _NoDevice, _c_params, no_library  # noqa: F401  (no_library is a fixture)
from tests.test_irradiance import furnace_bound, gamma, interior_points, unit_vectors
from tests.test_shade_points import build_shade_shim, rich_analytic_scene, scattered_rays, shim_shade
from tests.test_shade_points_gpu import quad_scene
from tests.test_texture_sample_gpu import SAMPLE
from tools import scenes_util as su

_IN = ["NraysScene*", "uint32_t", "const double*", "const double*", "const int32_t*", "const uint32_t*", "float*", "float*", "float*", "double*", "uint32_t"]
EXPECTED = {"nrays_material_points_device": _IN + ["void*"], "nrays_material_points": _IN}
RUST_TYPES = {"NraysScene*": "*mut NraysScene", "uint32_t": "u32", "const double*": "*const f64", "const int32_t*": "*const i32", "const uint32_t*": "*const u32",
              "float*": "*mut f32", "double*": "*mut f64", "void*": "*mut c_void"}
ALL = ("ambient", "diffuse", "specular", "node")
WANTS = [tuple(name for k, name in enumerate(ALL) if mask >> k & 1) for mask in range(1, 16)]  # every combination of outputs but none


def same(a, b):
    """Bit patterns equal (float32 or float64 alike), any NaN equal to any NaN."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    word = np.uint32 if a.dtype == np.float32 else np.uint64
    return bool(((a.view(word) == b.view(word)) | (np.isnan(a) & np.isnan(b))).all())


def same_terms(got, want):
    """Two MaterialTerms agree bit for bit, None where None."""
    return all((g is None and w is None) or (g is not None and w is not None and same(g, w)) for g, w in zip(got, want))


# ---- shared with the GPU tests: scenes and point sets ----------------------------------------------------------------------------------------------------------
def lightless(scene):
    """The scene without its lights: Material::compute is Material::ambiant there, for all three material kinds."""
    return nr.Scene(scene._nodes, [], scene._background)


def oracle_hits(scene, origins, dirs):
    """The closest hits of the CPU oracle as the arguments of material_points / shade_points: misses included (flags 0, node -1)."""
    hit, rec = oracle.cast(scene.descriptor, origins, dirs)
    flags = (hit.astype(np.uint32) | (np.where(rec[:, 4] != 0.0, 2, 0) * hit).astype(np.uint32))
    toi = np.where(hit, rec[:, 0], 0.0)
    return dict(points=origins + dirs * toi[:, None], normals=np.ascontiguousarray(rec[:, 1:4]), uvs=np.ascontiguousarray(rec[:, 5:7]),
                nodes=np.where(hit, rec[:, 7], -1).astype(np.int32), hit_flags=flags, view_dirs=dirs)


def quad_rays(w=64, h=64):
    sc, cam = quad_scene()
    proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], w, h)
    o, d, _ = nr.camera_rays((w, h), cam["eye"], proj, seed=9)
    return sc, o, d


def uv_variants(a, seed):
    """The point set as it is; without uvs; with flag bit 1 cleared on a third of the points; without flags (every point live, nodes still -1 at the misses)."""
    cleared = np.where(np.random.default_rng(seed).integers(0, 3, len(a["nodes"])) == 0, a["hit_flags"] & np.uint32(1), a["hit_flags"]).astype(np.uint32)
    return [a, dict(a, uvs=None), dict(a, hit_flags=cleared), dict(a, hit_flags=None)]


DIFFUSE_P = np.asarray([0.375, 0.0, -0.625])  # on the floor of diffuse_scene(), f32-exact


def diffuse_scene():
    """The construction under which Material::compute IS kd * tex: three PHONG nodes with ka = 0 and ks = 0 — quad_scene()'s two textured materials (RGBA8 Bilinear /
    Wrap colour texture; the second also the RGBA32F Nearest opacity map) and one without a texture — and one light of radius 0, one sample and colour (1, 1, 1) at
    DIFFUSE_P + 4 n, straight above the point DIFFUSE_P of a floor with n = (0, 1, 0).  Viewed along (1, 0, 0): dcoeff = 1, scoeff = -0, nothing in the way.  The node
    only selects the material, so every point of the set sits at DIFFUSE_P and differs in node, uv and flags; the other two quads lie far to the side."""
    src, _ = quad_scene()
    mats = [src._nodes[0].material, src._nodes[1].material]
    twins = [nr.PhongMaterial((0.0, 0.0, 0.0), m.diffuse_color, (0.0, 0.0, 0.0), m.texture, m.alpha, m.shininess) for m in mats]
    twins.append(nr.PhongMaterial((0.0, 0.0, 0.0), (0.7, 0.35, 0.125), (0.0, 0.0, 0.0), None, None, 10.0))
    idx = np.asarray([[0, 2, 1], [0, 3, 2]], dtype=np.uint32)
    uv = su.f32_exact([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])
    nodes = []
    for k, m in enumerate(twins):
        x = 100.0 * k
        quad = su.f32_exact([[x - 2.5, 0.0, -2.5], [x + 2.5, 0.0, -2.5], [x + 2.5, 0.0, 2.5], [x - 2.5, 0.0, 2.5]])
        nodes.append(nr.SceneNode(m, 0.0, 0.0, 1.0, 1.0, nr.Isometry3(), nr.TriMesh(quad, idx, uv)))
    return nr.Scene(nodes, [nr.Light(tuple(DIFFUSE_P + np.asarray([0.0, 4.0, 0.0])), 0.0, 1, (1.0, 1.0, 1.0))], (0.1, 0.2, 0.3))


def diffuse_points(n=600, seed=31):
    """The point set of diffuse_scene(): all at DIFFUSE_P, nodes 0 .. 2 in turn, uvs inside and outside [0, 1], flags 3 or 1."""
    rng = np.random.default_rng(seed)
    return dict(points=np.tile(DIFFUSE_P, (n, 1)), normals=np.tile([0.0, 1.0, 0.0], (n, 1)), view_dirs=np.tile([1.0, 0.0, 0.0], (n, 1)),
                nodes=(np.arange(n) % 3).astype(np.int32), uvs=rng.uniform(-1.0, 2.5, size=(n, 2)), hit_flags=np.where(rng.integers(0, 4, n) == 0, 1, 3).astype(np.uint32))


def material_args(a):
    return {k: a[k] for k in ("nodes", "normals", "uvs", "hit_flags")}


def mirror(scene, a, want):
    """material_points_ref over the scene's own SceneNode list at the point set `a`."""
    return nr.material_points_ref(scene._nodes, a["nodes"], a.get("normals"), a.get("uvs"), a.get("hit_flags"), want)


def shade_args(a):
    return {k: a[k] for k in ("points", "normals", "view_dirs", "nodes", "uvs", "hit_flags")}


MODES = [(f, i, o) for f in tc.FORMATS for i in (tc.BILINEAR, tc.NEAREST) for o in (tc.WRAP, tc.CLAMP)]
MODE_IDS = ["%s-%s-%s" % (f, "nearest" if i else "bilinear", "clamp" if o else "wrap") for f, i, o in MODES]


def sampler_nodes(fmt, interp, overflow):
    """One PHONG node with ka = (1, 1, 1) per texture of texture_cases.SIZES, the texture as colour texture AND opacity map: its ambient term is the sample's four
    channels, 1 * tc exactly."""
    nodes = []
    for size in tc.SIZES:
        tex = nr.Texture2d(nr.ImageData(tc.TEXTURES[size][fmt]), interp, overflow)
        mat = nr.PhongMaterial((1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), tex, tex, 1.0)
        nodes.append(nr.SceneNode(mat, 0.0, 0.0, 1.0, 1.0, nr.Isometry3((10.0 * len(nodes), 0.0, 0.0)), nr.Ball(1.0)))
    return nodes


_SAMPLER = {}


def sampler_case(fmt, interp, overflow):
    """Per mode, computed once and left unchanged: the uvs of every texture's pairs(w, h) and nonfinite_pairs() as float64, their nodes, and sample_ref's values."""
    key = (fmt, interp, overflow)
    if key not in _SAMPLER:
        uv, ids, ref = [], [], []
        for t, size in enumerate(tc.SIZES):
            c = np.concatenate([tc.pairs(*size), tc.nonfinite_pairs()])
            uv.append(c.astype(np.float64))
            ids.append(np.full(len(c), t, np.int32))
            with np.errstate(all="ignore"):
                ref.append(tc.sample_ref(tc.TEXTURES[size][fmt], interp, overflow, c[:, 0], c[:, 1]).value)
        _SAMPLER[key] = dict(uvs=np.concatenate(uv), nodes=np.concatenate(ids), ref=np.concatenate(ref))
        for a in _SAMPLER[key].values():
            a.setflags(write=False)
    return _SAMPLER[key]


def check_sampler(ambient, case, interp):
    """`ambient` (n, 4) float32 of sampler_nodes() at case's uvs against sample_ref: NaN exactly where the reference's arithmetic gives NaN; Nearest bit-equal,
    Bilinear within the bound of tests/test_texture_sample_gpu.py."""
    ref = case["ref"]
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(ambient), nan)
    worst = float(np.abs(ambient.astype(np.float64) - ref)[~nan].max())
    print("sampler: worst |got - reference| = %.4g (bound %.4g)" % (worst, 0.0 if interp == tc.NEAREST else SAMPLE))
    if interp == tc.NEAREST:
        assert same(ambient, ref.astype(np.float32))
    else:
        assert worst <= SAMPLE


# ---- the surface ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_header_ctypes_and_rust_declare_the_same_function(name):
    assert _c_params(name) == EXPECTED[name]
    assert name in abi.HIP_SYMBOLS and name in abi.POST_V7_SYMBOLS
    res, args = abi.HIP_SYMBOLS[name]
    assert res is C.c_int and len(args) == len(EXPECTED[name]) and args[1] is C.c_uint32 and args[10] is C.c_uint32
    m = re.search(r"pub fn %s\((.*?)\) -> c_int;" % name, FFI)
    assert m, "%s is not declared in gpu_ffi.rs" % name
    assert [p.split(": ", 1)[1] for p in m.group(1).split(", ")] == [RUST_TYPES[t] for t in EXPECTED[name]]
    assert "pub fn material_points(" in GPU_RS and "pub unsafe fn material_points_device(" in GPU_RS
    assert "nrays_material_points(" in GPU_RS and "nrays_material_points_device(" in GPU_RS


def test_the_symbols_are_exported_and_the_abi_version_is_still_7(built):
    assert re.search(r"#define NRAYS_ABI_VERSION 7\b", HEADER) and abi.ABI_VERSION == 7 and abi.load_hip_lib().nrays_abi_version() == 7
    note = re.search(r"Added after 7 WITHOUT a bump.*?\*/", HEADER_TEXT, re.S).group(0)
    exported = subprocess.check_output(["nm", "-D", "--defined-only", abi.HIP_LIB_PATH]).decode()
    for name in EXPECTED:
        assert re.search(r"%s\b" % name, note), name
        assert (" T " + name + "\n") in exported, name
        assert getattr(abi.load_hip_lib(), name).argtypes == abi.HIP_SYMBOLS[name][1]


def test_the_python_names_exist():
    for name in ("material_points", "material_hits", "material_points_ref", "texel_albedo", "indirect_points"):
        assert callable(getattr(nr, name)), name
    assert nr.MaterialTerms._fields == ALL
    from nrays_amd import scenefile
    for cls in (nr.Scene, scenefile.FileScene):
        for name in ("material_points", "material_hits", "texel_albedo", "indirect_points"):
            assert callable(getattr(cls, name)), name


def test_without_a_scene_every_call_is_a_bad_arg(built):
    """Without a scene nothing else is looked at; the other arguments one by one need a scene: tests/test_material_points_gpu.py."""
    lib = abi.load_hip_lib()
    nm, uv, node, hf = (C.c_double * 3)(0.0, 0.0, 1.0), (C.c_double * 2)(), (C.c_int32 * 1)(0), (C.c_uint32 * 1)(3)
    amb, dif, spec, nd = (C.c_float * 4)(7.0, 7.0, 7.0, 7.0), (C.c_float * 3)(7.0, 7.0, 7.0), (C.c_float * 4)(7.0, 7.0, 7.0, 7.0), (C.c_double * 4)(7.0, 7.0, 7.0, 7.0)
    adr = C.addressof
    for n in (0, 1):
        for flags in (0, 1):
            assert lib.nrays_material_points(None, n, nm, uv, node, hf, amb, dif, spec, nd, flags) == abi.ERR_BAD_ARG
            assert lib.nrays_material_points_device(None, n, adr(nm), adr(uv), adr(node), adr(hf), adr(amb), adr(dif), adr(spec), adr(nd), flags, None) == abi.ERR_BAD_ARG
    assert lib.nrays_last_error() and list(amb) == [7.0] * 4 and list(dif) == [7.0] * 3 and list(spec) == [7.0] * 4 and list(nd) == [7.0] * 4


# ---- the Python wrappers check before any library call ----------------------------------------------------------------------------------------------------------
def _good(n=4):
    return dict(nodes=np.zeros(n, np.int32), normals=np.tile([0.0, 1.0, 0.0], (n, 1)), uvs=np.zeros((n, 2)), hit_flags=np.full(n, 3, np.uint32))


def test_material_points_rejects_bad_arguments_before_any_library_call(no_library):
    import torch
    sc = _NoDevice()
    bad = [
        dict(nodes=None),                                                          # NULL nodes
        dict(want=()),                                                             # no output
        dict(normals=None), dict(normals=None, want=("ambient",)), dict(normals=None, want=ALL),  # NULL normals with out_ambient
        dict(want=("ambient", "albedo")), dict(want="ambient"),                    # unknown names
        dict(nodes=np.zeros(5, np.int32)), dict(nodes=np.zeros((4, 1), np.int32)), dict(nodes=np.zeros(4, np.float64)),
        dict(normals=np.zeros((5, 3))), dict(normals=np.zeros((4, 2))), dict(normals=np.zeros((4, 3), np.int32)),
        dict(uvs=np.zeros((4, 3))), dict(uvs=np.zeros(8)), dict(uvs=np.zeros((3, 2))), dict(uvs=np.zeros((4, 2), np.int32)),
        dict(hit_flags=np.ones(3, np.uint32)), dict(hit_flags=np.ones(4, np.float32)),
        dict(normals=torch.zeros((4, 3), dtype=torch.float64)),                    # numpy and torch mixed
        dict(nodes=torch.zeros(4, dtype=torch.int32)),
        dict(nodes=torch.zeros(4, dtype=torch.int32), normals=None, uvs=None, hit_flags=None, want=("diffuse",)),  # a torch tensor on the host
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            nr.material_points(sc, **dict(_good(), **kw))
    with pytest.raises(ValueError):
        nr.Scene([], []).material_points(np.zeros(4, np.int32), want=())
    # a well-formed call gets as far as the library: every legal combination of outputs, normals only where the ambient term needs them
    for want in WANTS:
        with pytest.raises(AssertionError, match="library was loaded"):
            nr.material_points(sc, **dict(_good(), want=want))
        if "ambient" not in want:
            with pytest.raises(AssertionError, match="library was loaded"):
                nr.material_points(sc, np.zeros(4, np.int32), want=want)
    # the mirror applies the same checks
    nodes = [nr.SceneNode(su.default_material(), 0.0, 0.0, 1.0, 1.0, nr.Isometry3(), nr.Ball(1.0))]
    for kw in (dict(want=()), dict(normals=None), dict(want=("rgb",)), dict(uvs=np.zeros((3, 2))), dict(hit_flags=np.ones(5, np.uint32)), dict(nodes=np.zeros(4))):
        g = dict(_good(), **kw)
        with pytest.raises(ValueError):
            nr.material_points_ref(nodes, g.pop("nodes"), **g)


def test_material_hits_refuses_incomplete_hits(no_library):
    sc = _NoDevice()
    full = nr.CastHits(toi=np.ones(4), node=np.zeros(4, np.int32), normal=np.tile([0.0, 0.0, -1.0], (4, 1)), uv=np.zeros((4, 2)), prim=None, flags=np.full(4, 3, np.uint32))
    for name in ("normal", "uv", "flags"):
        with pytest.raises(ValueError, match=name):
            nr.material_hits(sc, full._replace(**{name: None}))
    with pytest.raises(AssertionError, match="library was loaded"):  # the normal is not needed without the ambient term, prim never
        nr.material_hits(sc, full._replace(normal=None), want=("diffuse", "node"))
    with pytest.raises(AssertionError, match="library was loaded"):
        nr.material_hits(sc, full)


def test_texel_albedo_and_indirect_points_check_their_arguments_before_any_library_call(no_library):
    sc = _NoDevice()
    for kw in (dict(node=-1), dict(width=0), dict(height=0), dict(width=16385), dict(width=8192, height=4096), dict(device="cpu")):
        with pytest.raises(ValueError):
            nr.texel_albedo(sc, **dict(dict(node=0, width=8, height=8), **kw))
    with pytest.raises(AssertionError, match="library was loaded"):
        nr.texel_albedo(sc, 0, 8, 8)
    sh = np.zeros((8, 9, 3), np.float32)
    g = nr.ProbeGrid((0, 0, 0), (1, 1, 1), (2, 2, 2), sh)
    good = dict(points=np.zeros((4, 3)), normals=np.tile([0.0, 1.0, 0.0], (4, 1)), nodes=np.zeros(4, np.int32), grid=g)
    for kw in (dict(nodes=None), dict(nodes=np.zeros(5, np.int32)), dict(nodes=np.zeros(4)), dict(uvs=np.zeros((4, 3))), dict(hit_flags=np.ones(3, np.uint32)),
               dict(points=np.zeros((4, 2))), dict(normals=None), dict(grid=None), dict(facing=1), dict(grid=g._replace(sh=sh[:7]))):
        with pytest.raises(ValueError):
            nr.indirect_points(sc, **dict(good, **kw))
    with pytest.raises(AssertionError, match="library was loaded"):
        nr.indirect_points(sc, **good)


# ---- the mirror against the oracle, bit for bit -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shade_shim(tmp_path_factory.mktemp("material_shim"))


def _ambient_against_compute(shim, scene, a, seed):
    dark = lightless(scene)
    for v in uv_variants(a, seed):
        got = mirror(scene, v, ("ambient",)).ambient
        assert same(got, shim_shade(shim, dark, **shade_args(v)))
    return got


def test_ambient_is_compute_without_lights_on_the_analytic_scene(shim):
    """rich_analytic_scene(): PHONG without textures, NormalMaterial and UVMaterial nodes, at the oracle's hits of 800 scattered rays (misses included)."""
    sc, _ = rich_analytic_scene()
    o, d = scattered_rays(np.random.default_rng(1), 800)
    a = oracle_hits(sc, o, d)
    kinds = {sc._nodes[k].material.kind for k in set(a["nodes"][a["nodes"] >= 0].tolist())}
    assert kinds == {abi.MAT_PHONG, abi.MAT_NORMAL, abi.MAT_UV} and (a["nodes"] < 0).any()
    _ambient_against_compute(shim, sc, a, 5)


def test_ambient_is_compute_without_lights_on_the_textured_quads(shim):
    """quad_scene(): an RGBA8 Bilinear / Wrap colour texture on both quads, an RGBA32F Nearest opacity map on the upper one, at the hits of a 64 x 64 camera."""
    sc, o, d = quad_rays()
    a = oracle_hits(sc, o, d)
    assert set(a["nodes"].tolist()) == {-1, 0, 1}
    got = mirror(sc, a, ("ambient",)).ambient
    assert len(np.unique(got[a["nodes"] == 1, 3])) == 3 and np.unique(got[a["nodes"] == 0], axis=0).shape[0] > 100  # the opacity map's three texels; a textured floor
    _ambient_against_compute(shim, sc, a, 6)


def test_diffuse_is_compute_under_one_light_straight_above(shim):
    """diffuse_scene(): with ka = ks = 0 and the light straight above, compute is kd * tex — dcoeff = 1, scoeff = -0, unshadowed, axpy with 1 — as values."""
    sc = diffuse_scene()
    a = diffuse_points()
    for v in (a, dict(a, uvs=None), dict(a, hit_flags=None)):
        got = mirror(sc, v, ("diffuse",)).diffuse
        ref = shim_shade(shim, sc, **shade_args(v))[:, :3]
        assert not np.isnan(ref).any() and np.array_equal(got, ref)
    assert np.unique(got, axis=0).shape[0] > 300  # (textured: not the three kd)
    plain = mirror(sc, dict(a, uvs=None), ("diffuse",)).diffuse
    assert same(plain, np.asarray([n.material.diffuse_color for n in sc._nodes], np.float32)[a["nodes"]])


def test_specular_and_node_are_the_records_constants():
    sc, _ = rich_analytic_scene()
    ids = np.arange(-1, len(sc._nodes) + 1, dtype=np.int32)
    t = nr.material_points_ref(sc._nodes, ids, want=("specular", "node"))
    assert t.ambient is None and t.diffuse is None
    for i, k in enumerate(ids):
        if not 0 <= k < len(sc._nodes):
            assert not t.specular[i].any() and not t.node[i].any()
            continue
        n = sc._nodes[k]
        assert t.node[i].tolist() == [float(np.float32(n.alpha)), float(np.float32(n.refl_mix)), float(np.float32(n.refl_atenuation)), n.refr_coeff]
        phong = n.material.kind == abi.MAT_PHONG
        assert t.specular[i].tolist() == ([float(np.float32(x)) for x in n.material.specular_color + (n.material.shininess,)] if phong else [0.0] * 4)


# ---- the mirror's sampler against the independent restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,interp,overflow", MODES, ids=MODE_IDS)
def test_the_sampler_against_texture_cases(fmt, interp, overflow):
    assert (nr.Interpolation.Bilinear, nr.Interpolation.Nearest, nr.Overflow.Wrap, nr.Overflow.ClampToEdges) == (tc.BILINEAR, tc.NEAREST, tc.WRAP, tc.CLAMP)
    c = sampler_case(fmt, interp, overflow)
    n = len(c["nodes"])
    t = nr.material_points_ref(sampler_nodes(fmt, interp, overflow), c["nodes"], np.tile([0.0, 0.0, 1.0], (n, 1)), c["uvs"], want=("ambient", "diffuse"))
    check_sampler(t.ambient, c, interp)
    assert not t.diffuse.any() or np.isnan(t.diffuse).any()  # kd = 0


# ---- the skip rule ----------------------------------------------------------------------------------------------------------------------------------------------
def skip_case():
    """Points of quad_scene()'s two nodes, a third of them skipped one way each — flag bit 0 clear, node -1, node = the node count — with NaN in their inputs."""
    n = 300
    rng = np.random.default_rng(12)
    nodes = rng.integers(0, 2, n).astype(np.int32)
    flags = np.full(n, 3, np.uint32)
    normals, uvs = unit_vectors(13, n), rng.uniform(-1.0, 2.0, size=(n, 2))
    how = np.arange(n) % 6
    flags[how == 1] = 2
    nodes[how == 3] = -1
    nodes[how == 5] = 2
    skipped = (how == 1) | (how == 3) | (how == 5)
    normals[skipped] = np.nan
    uvs[skipped] = np.nan
    return dict(nodes=nodes, normals=normals, uvs=uvs, hit_flags=flags), skipped


def test_skipped_points_are_exact_zeros():
    sc, _ = quad_scene()
    a, skipped = skip_case()
    t = mirror(sc, a, ALL)
    for out in t:
        assert not out[skipped].view(np.uint32).any() and not np.isnan(out).any()
        assert (out[~skipped] != 0).any(axis=1).all()


# ---- indirect_points on the mirrors: a furnace ------------------------------------------------------------------------------------------------------------------
def test_indirect_points_in_a_furnace():
    """Probes that are sh_fold_ref of the constant radiance L: E = pi L within B = furnace_bound, so d E / pi = d L within d B / pi, and the two products of
    indirect_points and the rounding of 1 / pi to float32 are three more roundings of the value: gamma(3) d (L + B / pi).  d = kd * tex per channel."""
    dirs = nr.sphere_dirs(1024)
    L = np.asarray([0.5, 0.25, 0.125], np.float32)
    sh = nr.sh_fold_ref(dirs[None], np.broadcast_to(L, (1, 1024, 3)).copy())
    g = nr.ProbeGrid((0.25, 0.25, 0.25), (0.5, 0.5, 0.5), (2, 2, 2), np.ascontiguousarray(np.broadcast_to(sh, (8, 9, 3))))
    sc = diffuse_scene()
    n = 1200
    rng = np.random.default_rng(41)
    p, nm = interior_points(42, g, n), unit_vectors(43, n)
    nodes, uvs = (np.arange(n) % 3).astype(np.int32), rng.uniform(-1.0, 2.5, size=(n, 2))
    flags = np.where(np.arange(n) % 7 == 0, 0, np.where(np.arange(n) % 5 == 0, 1, 3)).astype(np.uint32)
    d = nr.material_points_ref(sc._nodes, nodes, uvs=uvs, hit_flags=flags, want=("diffuse",)).diffuse
    E = nr.irradiance_points_ref(p, nm, g, hit_flags=flags)[0]
    got = (d * E) * nr.scene.INV_PI_F32  # the expression of indirect_points on the two mirrors
    assert got.dtype == np.float32 and nr.scene.INV_PI_F32 == float(np.float32(0.3183098861837907))
    B, _ = furnace_bound(dirs, L)
    d64, L64 = d.astype(np.float64), L.astype(np.float64)
    bound = d64 * B / math.pi + gamma(3) * d64 * (L64 + B / math.pi)
    live = (flags & 1) != 0
    err = np.abs(got.astype(np.float64) - d64 * L64)
    print("furnace: worst error / bound = %.3g" % (err[live] / bound[live]).max())
    assert (err[live] <= bound[live]).all() and (d[live] > 0).all()
    assert not got[~live].view(np.uint32).any()
