"""Every k_primary permutation by name: each case of tests/permutation_cases.py is rendered on a fresh handle created under the case's
switches, and after every render the library is asked which permutation it launched (nrays_debug_last_permutation).

Per case:
  1. two frames through nrays_render_device (the second runs on the first one's cost order; the instrumented case renders through
     nrays_render_device_instrumented): after each the probe equals the case's (stats, feat, plain, occ) exactly — one launch, not mixed;
  2. each frame is within TOL = 1e-4 per channel of oracle.render of the same descriptor and parameters (BASELINE.json north_star, as
     tests/test_parity_gpu.py) and the four ray classes equal the oracle's exactly;
  3. each frame is BIT-identical to the same handle's nrays_render_device_instrumented frame (k_primary<true, 31>: "their results are
     identical, only slower", frame_path.hip) and the two frames to each other: one ulp of one pixel fails.
The last test of the module asserts that the tuples the probe reported are exactly the header's list: a skipped, deselected or
mis-parametrised case cannot hide a hole (run the module whole)."""
import ctypes as C

import numpy as np
import pytest

import nrays_amd as nr
from nrays_amd import abi
from tests import permutation_cases as pc

pytestmark = pytest.mark.gpu
TOL = 1e-4
RAY_CLASSES = ("rays_primary", "rays_reflection", "rays_refraction", "rays_shadow")
REPORTED = {}  # permutation -> the cases whose frames the probe named it for


def _render(scene, params, instrumented):
    import torch
    lib = abi.load_hip_lib()
    out = torch.empty((params.height, params.width, 3), dtype=torch.float32, device="cuda")
    fn = lib.nrays_render_device_instrumented if instrumented else lib.nrays_render_device
    abi.check(fn(scene.device_handle(), C.byref(params), C.c_void_p(out.data_ptr()), None))
    st = nr.get_stats(scene)  # (synchronises with the frame)
    return out.cpu().numpy(), {k: int(getattr(st, k)) for k in RAY_CLASSES}, nr.last_permutation(scene)


def test_probe_before_the_first_render(gpu):
    case = pc.CASES[0]
    sc, _ = case.build()
    assert nr.last_permutation(sc) == ((False, 0, False, 0), 0, False)
    sc._release()


@pytest.mark.parametrize("case", pc.CASES, ids=[c.name for c in pc.CASES])
def test_permutation(gpu, case):
    ref, ref_counts, _ = pc.oracle_frame(case)
    with case.environment():
        sc, cam = case.build()
        sc.device_handle()  # the switches are read here
        p = case.params(cam)
        try:
            frames = [_render(sc, p, case.kind == "instrumented") for _ in range(2)]
            full, full_counts, full_perm = _render(sc, p, True)
        finally:
            sc._release()
    for k, (img, counts, (perm, launches, mixed)) in enumerate(frames):
        REPORTED.setdefault(perm, []).append(case.name)
        assert (perm, launches, mixed) == (case.expect, 1, False), "frame %d ran %s (%d launches%s), the table expects %s" % (
            k, perm, launches, ", mixed" if mixed else "", case.expect)
    assert full_perm == ((True, 31, False, 0), 1, False)
    REPORTED.setdefault(full_perm[0], []).append(case.name + " (instrumented)")
    for k, (img, counts, _) in enumerate(frames):
        err = np.abs(img - ref)
        print("%s frame %d: max |hip - oracle| = %.3g, %d components differ from the instrumented frame" % (
            case.name, k, err.max(), int((img.view(np.uint32) != full.view(np.uint32)).sum())))
        assert err.max() <= TOL, "frame %d: max err %g at %s (mean %g)" % (k, err.max(), np.unravel_index(err.argmax(), err.shape), err.mean())
        assert counts == ref_counts, (k, counts, ref_counts)
    assert full_counts == ref_counts, (full_counts, ref_counts)
    for k, (img, _, _) in enumerate(frames):
        diff = img.view(np.uint32) != full.view(np.uint32)
        assert not diff.any(), "frame %d: %d components differ from the instrumented frame, first at %s: %r against %r" % (
            k, int(diff.sum()), tuple(np.argwhere(diff)[0]), img[diff][0], full[diff][0])
    assert np.array_equal(frames[0][0].view(np.uint32), frames[1][0].view(np.uint32)), "the second frame differs from the first"


def test_probe_flags_a_frame_whose_sample_batches_ran_different_permutations(gpu, monkeypatch):
    """Three samples per pixel without a window, one sample per launch (NRAYS_MAX_PRIMARY=1): the first batch is a plain frame's launch, the
    other two are general ones.  The probe names the last, counts three and says that they differ; the frame is still the oracle's."""
    import oracle
    from tools import scenes_util as su
    case = next(c for c in pc.CASES if c.expect == (False, 37, True, 0))
    monkeypatch.setenv("NRAYS_MAX_PRIMARY", "1")
    with case.environment():
        sc, cam = case.build()
        sc.device_handle()
    p, _ = su.camera_params(cam, 157, 99, spp=3, window=0.0, seed=7)
    ref, ost = oracle.render(sc.descriptor, p, 8)
    try:
        img, counts, probe = _render(sc, p, False)
        assert probe == ((False, 37, False, 0), 3, True)
        one, _, probe1 = _render(sc, case.params(cam), False)  # the next render starts the bookkeeping afresh
        assert probe1 == ((False, 37, True, 0), 1, False)
    finally:
        sc._release()
    err = np.abs(img - ref)
    print("batched frame: max |hip - oracle| = %.3g" % err.max())
    assert err.max() <= TOL
    assert counts == {k: int(getattr(ost, k)) for k in RAY_CLASSES}


def test_every_listed_permutation_was_reported(gpu):
    want = {t for _, t in pc.parse_permutations()}
    got = set(REPORTED)
    assert got == want, "never reported: %s; reported but not in NR_PRIMARY_PERMUTATIONS: %s" % (sorted(want - got), sorted(got - want))
