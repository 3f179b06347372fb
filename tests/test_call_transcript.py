"""The Python batch wrappers hand the library what they handed it before they shared one marshalling driver (nrays_amd/marshal.py).

tools/call_transcript.py runs every public wrapper and probe of nrays_amd.scene over a fixed list of small cases against a stand-in library that records its calls,
so no kernel runs: the entry point, every scalar, and for every pointer the NAME of the argument or result whose memory it is.  The goldens were recorded at the
commit before the driver (the numpy one on the CPU, the torch one on an MI355X with real CUDA tensors) and are never regenerated from a later tree."""
import json
import os

import numpy as np
import pytest

import nrays_amd as nr
from tools import call_transcript as ct

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "call_transcript_%s.json")


def _assert_same_as_golden(form):
    with open(GOLDEN % form) as f:
        want = json.load(f)
    got = json.loads(json.dumps(ct.transcript(nr, form)))  # (through JSON: tuples become lists, as in the golden)
    assert [r["case"] for r in got] == [r["case"] for r in want]
    for g, w in zip(got, want):
        assert g == w, "%s\n  recorded: %s\n  now:      %s" % (w["case"], json.dumps(w, sort_keys=True), json.dumps(g, sort_keys=True))


def test_numpy_forms_call_the_library_as_recorded():
    _assert_same_as_golden("numpy")


@pytest.mark.gpu
def test_torch_forms_call_the_library_as_recorded(gpu):
    _assert_same_as_golden("torch")


def _flags_and_values():
    return np.ones(16, np.uint32), np.arange(48, dtype=np.float32).reshape(16, 3)


def test_dilate_texels_writes_into_a_conforming_array_and_copies_any_other():
    flags, values = _flags_and_values()
    with ct.stand_in(nr.abi):
        assert nr.dilate_texels(ct.stub_scene(), flags, 4, 4, 2, values=values)[0] is values
        wide = np.arange(96, dtype=np.float32).reshape(16, 6)
        for other in (values.astype(np.float64), wide[:, ::2]):
            before = other.copy()
            out = nr.dilate_texels(ct.stub_scene(), flags, 4, 4, 2, values=other)[0]
            assert out is not other and not np.shares_memory(out, other)
            assert out.dtype == np.float32 and out.flags.c_contiguous and np.array_equal(out, before)
            assert np.array_equal(other, before) and other.dtype == before.dtype
        frozen = values.copy()
        frozen.flags.writeable = False
        assert not np.shares_memory(nr.dilate_texels(ct.stub_scene(), flags, 4, 4, 2, values=frozen)[0], frozen)


def test_conforming_points_are_passed_as_their_own_memory_by_every_family():
    """The transcript shows it for every column; here once, explicitly, on raw addresses."""
    import ctypes as C
    P, N = np.zeros((4, 3)), np.tile([0.0, 0.0, 1.0], (4, 1))
    L, m = nr.hemisphere_dirs(4), np.zeros((2, 2, 4), np.float32)
    calls = {"trace_rays": dict(origins=P, dirs=N), "closest_hits": dict(origins=P, dirs=N),
             "shade_points": dict(points=P, normals=N, view_dirs=N, nodes=np.zeros(4, np.int32)), "occlusion_points": dict(points=P, normals=N, sample_dirs=L),
             "gather_points": dict(points=P, normals=N, sample_dirs=L), "gather_sh_points": dict(points=P, normals=N, sample_dirs=L),
             "gather_probes": dict(positions=P, sample_dirs=L), "gather_maps_points": dict(points=P, normals=N, sample_dirs=L, maps=[m], node_map=[0, -1]),
             "filter_texels": dict(flags=np.ones(4, np.uint32), width=2, height=2, points=P, normals=N, values=np.zeros((4, 3), np.float32)),
             "occlusion_ray_probe": dict(points=P, normals=N, sample_dirs=L), "gather_order": dict(points=P, normals=N, sample_dirs=L),
             "ray_order": dict(origins=P, dirs=N), "gather_sh_fold": dict(points=P, normals=N, sample_dirs=L, ray_colours=np.zeros((4, 4, 3), np.float32))}
    for fn, kw in calls.items():
        with ct.stand_in(nr.abi) as rec:
            getattr(nr.scene, fn)(ct.stub_scene(), **kw)
        (_, args, _), = rec.calls
        passed = [C.cast(a, C.c_void_p).value for a in args if isinstance(a, C._Pointer)]
        assert P.ctypes.data in passed, fn
