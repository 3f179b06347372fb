"""Batched Scene::trace / Scene::intersects_ray on caller-supplied rays (nrays_trace_rays*, nrays_intersects_rays_device): the parts that
need no GPU — the ABI surface, argument checks, and camera_rays(), whose rays traced by the CPU oracle give the oracle's frame bit for bit
(tests/trace_oracle_shim.c: the oracle's scene_trace on caller rays)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import nrays_amd as nr
import oracle
from nrays_amd import abi, math3d

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("nrays_trace_rays_device", "nrays_trace_rays", "nrays_intersects_rays_device")


def build_shim(directory):
    """Compiles tests/trace_oracle_shim.c with the oracle Makefile's flags and loads it."""
    out = os.path.join(str(directory), "libtrace_oracle_shim.so")
    subprocess.check_call(["gcc", "-O3", "-std=c11", "-ffp-contract=off", "-fPIC", "-shared", "-o", out,
                           os.path.join(ROOT, "tests", "trace_oracle_shim.c"), "-lm", "-lpthread"])
    lib = C.CDLL(out)
    lib.trace_oracle_rays.restype = C.c_int
    lib.trace_oracle_rays.argtypes = [C.POINTER(abi.NraysSceneDesc), C.c_uint32, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double),
                                      C.POINTER(C.c_float), C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_float)]
    return lib


def shim_trace(lib, scene, origins, dirs, refr=None, energy=None, keys=None, max_depth=0):
    """The oracle's Scene::trace of every ray: (n, 3) float32."""
    o = np.ascontiguousarray(origins, dtype=np.float64)
    d = np.ascontiguousarray(dirs, dtype=np.float64)
    r = None if refr is None else np.ascontiguousarray(refr, dtype=np.float64)
    e = None if energy is None else np.ascontiguousarray(energy, dtype=np.float32)
    k = None if keys is None else np.ascontiguousarray(keys, dtype=np.uint64)
    out = np.empty((len(o), 3), dtype=np.float32)
    ptr = lambda a, t: None if a is None else a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    rc = lib.trace_oracle_rays(scene.descriptor.pointer(), len(o), ptr(o, C.c_double), ptr(d, C.c_double), ptr(r, C.c_double), ptr(e, C.c_float),
                               ptr(k, C.c_uint64), int(max_depth), ptr(out, C.c_float))
    assert rc == 0, rc
    return out


def average_samples(colours, w, h, spp):
    """scene.rs:91-94 on traced sample colours (pixel-major, samples innermost): f32 sum over the samples in order, then / spp."""
    c = colours.reshape(w * h, spp, 3)
    tot = np.zeros((w * h, 3), dtype=np.float32)
    for s in range(spp):
        tot = tot + c[:, s]
    return (tot / np.float32(spp)).reshape(h, w, 3)


def analytic_scene(background=(1.0, 1.0, 1.0)):
    """Balls, a box and a plane under an area light (two samples per axis); one node reflects AND refracts (both continuations at one hit)."""
    glass = nr.PhongMaterial((0.1, 0.1, 0.15), (0.6, 0.7, 0.9), (1, 1, 1), None, None, 80.0)
    white = nr.PhongMaterial((0.1, 0.1, 0.1), (0.8, 0.8, 0.8), (1, 1, 1), None, None, 60.0)
    iso = nr.Isometry3
    nodes = [nr.SceneNode(glass, 0.3, 0.4, 0.5, 1.3, iso((-1.2, 0, 0)), nr.Ball(1.0)),
             nr.SceneNode(white, 0.5, 0.25, 1.0, 1.0, iso((1.3, 0, 0.5)), nr.Ball(0.8)),
             nr.SceneNode(glass, 0.0, 0.0, 0.4, 1.5, iso((0.2, 0.9, 1.8)), nr.Cuboid((0.6, 0.6, 0.6))),
             nr.SceneNode(white, 0.25, 0.5, 1.0, 1.0, iso((0, -1.2, 0)), nr.Plane((0, 1, 0)))]
    lights = [nr.Light((2.0, 6.0, -4.0), 0.4, 2, (1, 1, 1))]
    cam = dict(eye=(0.0, 2.0, -7.0), at=(0.0, 0.0, 0.0), fovy=45.0)
    return nr.Scene(nodes, lights, background), cam


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(tmp_path_factory.mktemp("trace_shim"))


def test_abi_version_7(built):
    assert abi.ABI_VERSION == 7
    assert "#define NRAYS_ABI_VERSION 7" in open(os.path.join(ROOT, "include", "nrays_abi.h")).read()
    assert abi.load_hip_lib().nrays_abi_version() == 7


def test_new_symbols_are_exported_with_signatures(built):
    exported = subprocess.check_output(["nm", "-D", "--defined-only", abi.HIP_LIB_PATH]).decode()
    lib = abi.load_hip_lib()
    for name in NEW_SYMBOLS:
        assert (" T " + name) in exported, name
        res, args = abi.HIP_SYMBOLS[name]
        assert res is C.c_int
        assert getattr(lib, name).argtypes == args
    assert len(abi.HIP_SYMBOLS["nrays_trace_rays_device"][1]) == 10
    assert len(abi.HIP_SYMBOLS["nrays_trace_rays"][1]) == 9
    assert len(abi.HIP_SYMBOLS["nrays_intersects_rays_device"][1]) == 8


def test_null_arguments_are_bad_args(built):
    lib = abi.load_hip_lib()
    o = (C.c_double * 3)(0.0, 0.0, 0.0)
    out = (C.c_float * 3)()
    lit = (C.c_uint32 * 1)()
    for n in (0, 1):
        assert lib.nrays_trace_rays(None, n, o, o, None, None, None, 0, out) == abi.ERR_BAD_ARG
        assert lib.nrays_trace_rays_device(None, n, C.addressof(o), C.addressof(o), None, None, None, 0, C.addressof(out), None) == abi.ERR_BAD_ARG
        assert lib.nrays_intersects_rays_device(None, n, C.addressof(o), C.addressof(o), C.addressof(o), C.addressof(out), C.addressof(lit), None) == abi.ERR_BAD_ARG
    assert lib.nrays_last_error()


class _NoDevice:
    """A scene whose device handle must never be asked for: argument errors are raised first."""
    def device_handle(self):
        raise AssertionError("device touched before the arguments were checked")


@pytest.mark.parametrize("kw", [
    dict(origins=np.zeros((4, 2)), dirs=np.zeros((4, 3))),
    dict(origins=np.zeros((4, 3)), dirs=np.zeros((5, 3))),
    dict(origins=np.zeros(12), dirs=np.zeros((4, 3))),
    dict(origins=np.zeros((4, 3), np.int64), dirs=np.zeros((4, 3))),
    dict(origins=np.zeros((4, 3)), dirs=np.zeros((4, 3)), refr=np.ones(3)),
    dict(origins=np.zeros((4, 3)), dirs=np.zeros((4, 3)), energy=np.ones((4, 1))),
    dict(origins=np.zeros((4, 3)), dirs=np.zeros((4, 3)), keys=np.zeros(4, np.float64)),
    dict(origins=np.zeros((4, 3)), dirs=np.zeros((4, 3)), max_depth=-1),
])
def test_trace_rays_checks_arguments_before_the_device(built, kw):
    with pytest.raises(ValueError):
        nr.trace_rays(_NoDevice(), **kw)


@pytest.mark.parametrize("kw", [
    dict(origins=np.zeros((4, 3)), dirs=np.zeros((4, 3)), max_toi=np.ones(5)),
    dict(origins=np.zeros((4, 3)), dirs=np.zeros((3, 3)), max_toi=np.ones(4)),
    dict(origins=np.zeros((4, 3)), dirs=np.zeros((4, 3)), max_toi=np.ones(4, np.int32)),
])
def test_intersects_rays_checks_arguments_before_the_device(built, kw):
    with pytest.raises(ValueError):
        nr.intersects_rays(_NoDevice(), **kw)


def test_camera_rays_layout():
    cam = dict(eye=(0.0, 2.0, -7.0), at=(0.0, 0.0, 0.0), fovy=45.0)
    proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], 5, 3)
    o, d, k = nr.camera_rays((5, 3), cam["eye"], proj, ray_per_pixel=2)
    assert o.shape == d.shape == (30, 3) and k.shape == (30,) and o.dtype == d.dtype == np.float64 and k.dtype == np.uint64
    assert np.all(o == np.asarray(cam["eye"]))
    assert np.allclose(np.linalg.norm(d, axis=1), 1.0, atol=1e-15)
    assert np.array_equal(d[0], d[1]) and k[0] != k[1]  # window 0: the samples of a pixel share a direction, not a key
    with pytest.raises(ValueError):
        nr.camera_rays((0, 3), cam["eye"], proj)


@pytest.mark.parametrize("spp,window", [(1, 0.0), (4, 1.0)])
def test_camera_rays_through_the_oracle_trace_give_its_frame(shim, spp, window):
    """camera_rays() are scene::render's rays, bit for bit: traced one by one by the oracle and averaged as scene.rs:91-94 averages, they give
    oracle.render's frame exactly (area light: the keys matter; reflection + refraction at one hit)."""
    sc, cam = analytic_scene()
    w, h = 48, 32
    proj = math3d.inverse_projection(cam["eye"], cam["at"], cam["fovy"], w, h)
    p = nr.make_params((w, h), spp, window, cam["eye"], proj, seed=7)
    ref, _ = oracle.render(sc.descriptor, p, num_threads=4)
    o, d, k = nr.camera_rays((w, h), cam["eye"], proj, ray_per_pixel=spp, window_width=window, seed=7)
    img = average_samples(shim_trace(shim, sc, o, d, keys=k), w, h, spp)
    assert np.array_equal(img, ref)
