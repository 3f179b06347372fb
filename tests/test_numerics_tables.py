"""Exhaustive checks of the small exact shortcuts the device code takes instead of an IEEE division."""
import numpy as np


def test_byte_over_255_through_an_f64_product_is_the_correctly_rounded_f32_quotient():
    """trace_device.h: tex_at — `u8 as f32 / 255.0` (texture2d.rs:111-162) is evaluated as (float)((double)x * (1.0 / 255.0))."""
    x = np.arange(256, dtype=np.float32)
    ref = x / np.float32(255.0)
    got = (x.astype(np.float64) * (1.0 / 255.0)).astype(np.float32)
    assert np.array_equal(ref, got)
    # the tempting f32 shortcut is NOT exact: this is why the product is taken in f64
    assert int((x * (np.float32(1.0) / np.float32(255.0)) != ref).sum()) > 0


def test_pixel_over_resolution_by_reciprocal_and_one_fma_correction_is_the_ieee_quotient(tmp_path):
    """trace_device.h: generate_primary<PLAIN> — `ox / width` (scene.rs:81-82) is evaluated as q0 = a * RN(1 / b), q = fma(fma(-q0, b, a), RN(1 / b), q0).
    tools/probe/div_markstein.c compares it with a / b for EVERY pixel index of every resolution up to 16384 (the host launches no PLAIN kernel beyond)."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "div_markstein")
    subprocess.check_call(["gcc", "-O2", "-mfma", "-ffp-contract=off", "-o", exe, os.path.join(root, "tools", "probe", "div_markstein.c"), "-lm"])
    out = subprocess.run([exe], stdout=subprocess.PIPE, text=True)
    assert out.returncode == 0, out.stdout
    assert " 0 mismatches" in out.stdout


def test_wrap_by_copysign_of_x_minus_trunc_is_fmod_one_bit_for_bit():
    """trace_device.h: tex_sample — `ux % 1.0` (texture2d.rs:217-218) is evaluated as copysignf(x - truncf(x), x).  x - trunc(x) is exact in f32 (the
    fraction of x has no more bits than x), and copysign restores the -0.0 that fmod returns for a negative integer and for -0.0 itself.  Compared
    with np.fmod(x, 1) as bit patterns over every exponent of f32 (denormals included) x 8192 fixed-seed mantissas x both signs, +-0, the
    smallest and largest denormals, 2^23 +- 0.5 and every coordinate value of the texture tests (tests/texture_cases.py)."""
    from tests import texture_cases as tc
    rng = np.random.default_rng(0x2A5EED)
    mant = rng.integers(0, 1 << 23, size=(255, 8192), dtype=np.uint32)
    mant[:, 0], mant[:, 1] = 0, (1 << 23) - 1                                            # the ends of every binade
    bits = (np.arange(255, dtype=np.uint32)[:, None] << np.uint32(23)) | mant            # exponent fields 0 .. 254: every finite binade
    bits = np.concatenate([bits.ravel(), bits.ravel() | np.uint32(0x80000000)])
    extra = np.array([0.0, -0.0, 8388607.5, 8388608.0, 8388608.5, -8388607.5, -8388608.0], dtype=np.float32)
    tiny = np.array([1, 2, 0x007fffff, 0x80000001, 0x807fffff], dtype=np.uint32).view(np.float32)
    table = [tc.BASE_VALUES, tc.RANDOM_VALUES] + [tc.boundary_values(n)[0] for n in sorted({d for s in tc.SIZES for d in s}) if n > 1]
    x = np.concatenate([bits.view(np.float32), extra, tiny] + table).astype(np.float32)
    assert len(x) >= 4_000_000 and np.isfinite(x).all()
    got = np.copysign(x - np.trunc(x), x)
    ref = np.fmod(x, np.float32(1.0))
    assert got.dtype == np.float32 and ref.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert int(((ref == 0.0) & np.signbit(ref)).sum()) > 1000                            # the table really holds negative integers: -0.0 results
    nf = np.array([np.inf, -np.inf, np.nan], dtype=np.float32)                           # non-finite: NaN either way
    with np.errstate(invalid="ignore"):
        assert np.isnan(np.copysign(nf - np.trunc(nf), nf)).all() and np.isnan(np.fmod(nf, np.float32(1.0))).all()
