"""Irradiance at caller-supplied points from a grid of SH probes (nrays_irradiance_points_device / nrays_irradiance_points; nrays_amd.irradiance_points, ProbeGrid,
probe_grid_positions, bake_probe_grid, irradiance_points_ref), the parts that need no GPU: the header, the ctypes table and the Rust declarations, the struct's
layout against the C compiler's, the argument checks, and the properties of the definition on its numpy mirror — which tests/test_irradiance_gpu.py compares
the device with bit for bit.  The bounds below are derived from the roundings the definition names (u = 2^-24, one per f32 operation), never from a result."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import nrays_amd as nr
from nrays_amd import abi
from nrays_amd.restated import SH_COSINE_LOBE, SH_K
from tests.test_gather import FFI, GPU_RS, HEADER, HEADER_TEXT, _NoDevice, _c_params, no_library  # noqa: F401  (no_library is a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_IN = ["NraysScene*", "uint32_t", "const double*", "const double*", "const uint32_t*", "const NraysIrradianceGrid*", "float*", "float*", "float*", "uint32_t"]
EXPECTED = {"nrays_irradiance_points_device": _IN + ["void*"], "nrays_irradiance_points": _IN}
RUST_TYPES = {"NraysScene*": "*mut NraysScene", "uint32_t": "u32", "const double*": "*const f64", "const uint32_t*": "*const u32",
              "const NraysIrradianceGrid*": "*const NraysIrradianceGrid", "float*": "*mut f32", "void*": "*mut c_void"}
STRUCT_FIELDS = [("origin", "double", "[f64; 3]", C.c_double * 3), ("cell", "double", "[f64; 3]", C.c_double * 3), ("counts", "uint32_t", "[u32; 3]", C.c_uint32 * 3),
                 ("bands", "uint32_t", "u32", C.c_uint32), ("sh", "const float*", "*const f32", C.c_void_p), ("valid", "const uint32_t*", "*const u32", C.c_void_p),
                 ("measure", "float", "f32", C.c_float), ("reserved", "uint32_t", "u32", C.c_uint32)]
U = 2.0 ** -24  # the unit roundoff of f32
BAND = (0, 1, 1, 1, 2, 2, 2, 2, 2)
# max |Y_c| over unit vectors: K0; K1; K2 / 2 (|xy| <= 1/2); K3 * 2 (z = 1); K4 (x = 1)
Y_MAX = (SH_K[0], SH_K[1], SH_K[1], SH_K[1], SH_K[2] / 2, SH_K[2] / 2, SH_K[3] * 2, SH_K[2] / 2, SH_K[4])


def gamma(k):
    """The bound of k accumulated roundings (Higham): k u / (1 - k u)."""
    return k * U / (1.0 - k * U)


def same(a, b):
    """Bit patterns equal, any NaN equal to any NaN."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def unit_vectors(seed, n):
    v = np.random.default_rng(seed).normal(size=(n, 3))
    return v / np.sqrt((v * v).sum(axis=1))[:, None]


def random_grid(seed, counts, bands=3, origin=(-0.5, 0.25, 1.0), cell=(0.5, 0.75, 0.25), valid=None, measure=4.0 * math.pi):
    P = counts[0] * counts[1] * counts[2]
    sh = np.random.default_rng(seed).uniform(-1.0, 2.0, size=(P, bands * bands, 3)).astype(np.float32)
    return nr.ProbeGrid(origin, cell, counts, sh, valid, measure)


def interior_points(seed, grid, n):
    """n points inside the grid's box (on an axis with one probe: around it)."""
    r = np.random.default_rng(seed).uniform(0.0, 1.0, size=(n, 3))
    span = np.array([(c - 1) * s if c > 1 else 1.0 for c, s in zip(grid.counts, grid.cell)])
    return np.asarray(grid.origin) + r * span - np.array([0.0 if c > 1 else 0.5 for c in grid.counts])


def furnace_bound(dirs, colour, bands=3):
    """|E - pi L| <= this, per channel, for the irradiance nrays_irradiance_points* gives at ANY unit normal from probes that are sh_fold_ref of the constant radiance
    `colour` (3,) over the table `dirs` (k, 3) — a furnace —, blended from up to eight identical probes.  In exact arithmetic E = 4 pi sum_c A_c Y_c(n) mean_j Y_c(d_j) L;
    the c = 0 term is 4 pi * pi * K0^2 L = pi L, so the table's part is 4 pi sum_{c >= 1} A_c |mean Y_c| max|Y_c| L.  The f32 part: a term's basis value (1), its
    product (1), k sums and the division (k + 1) in the fold; the blend's weights (36, see test_an_affine_field...) and its 8 products and sums; a_c (1), its
    product (1), C sums, the measure (1) and the last product (1): k + C + 50 roundings on 4 pi A_c max|Y_c| mean_j |Y_c(d_j)| L."""
    C_ = bands * bands
    y = np.stack(nr.scene._sh_terms(dirs[:, 0], dirs[:, 1], dirs[:, 2], C_), axis=1)  # f64
    L = np.abs(np.asarray(colour, np.float64))
    table = 4.0 * math.pi * sum(SH_COSINE_LOBE[BAND[c]] * abs(y[:, c].mean()) * Y_MAX[c] for c in range(1, C_))
    f32 = gamma(len(dirs) + C_ + 50) * 4.0 * math.pi * sum(SH_COSINE_LOBE[BAND[c]] * np.abs(y[:, c]).mean() * Y_MAX[c] for c in range(C_))
    return (table + f32) * L, table / math.pi  # (the bound per channel; the table's part relative to pi L)


# ---- the surface --------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_header_ctypes_and_rust_declare_the_same_function(name):
    assert _c_params(name) == EXPECTED[name]
    assert name in abi.HIP_SYMBOLS and name in abi.POST_V7_SYMBOLS
    res, args = abi.HIP_SYMBOLS[name]
    assert res is C.c_int and len(args) == len(EXPECTED[name]) and args[1] is C.c_uint32
    assert args[EXPECTED[name].index("const NraysIrradianceGrid*")] is C.POINTER(abi.NraysIrradianceGrid)
    m = re.search(r"pub fn %s\((.*?)\) -> c_int;" % name, FFI)
    assert m, "%s is not declared in gpu_ffi.rs" % name
    assert [p.split(": ", 1)[1] for p in m.group(1).split(", ")] == [RUST_TYPES[t] for t in EXPECTED[name]]
    assert "pub fn irradiance_points(" in GPU_RS and "pub unsafe fn irradiance_points_device(" in GPU_RS
    assert "nrays_irradiance_points(" in GPU_RS and "nrays_irradiance_points_device(" in GPU_RS


def test_the_grid_struct_is_the_same_in_the_header_ctypes_rust_and_the_c_compiler(tmp_path):
    m = re.search(r"struct NraysIrradianceGrid \{(.*?)\};\s*typedef struct NraysIrradianceGrid NraysIrradianceGrid;", HEADER, re.S)
    assert m, "struct NraysIrradianceGrid is not declared in include/nrays_abi.h (struct plus separate typedef)"
    c_fields = [re.sub(r"\[.*\]", "", re.sub(r"\s*\*\s*", "* ", f.strip())).rsplit(" ", 1) for f in m.group(1).split(";") if f.strip()]
    assert [(n, t) for t, n in c_fields] == [(n, t) for n, t, _, _ in STRUCT_FIELDS]
    for name in ("double origin", "double cell", "uint32_t counts"):
        assert re.search(r"%s\[3\];" % name, m.group(1)), name
    r = re.search(r"#\[repr\(C\)\]\s*(?:#\[derive[^\]]*\]\s*)?pub struct NraysIrradianceGrid \{(.*?)\n\}", FFI, re.S)
    assert r and re.findall(r"pub (\w+): ([^,]+),", r.group(1)) == [(n, t) for n, _, t, _ in STRUCT_FIELDS]
    assert [(n, t) for n, t in abi.NraysIrradianceGrid._fields_] == [(n, t) for n, _, _, t in STRUCT_FIELDS]
    assert re.search(r"#define NRAYS_IRRADIANCE_FACING 1u\b", HEADER) and abi.IRRADIANCE_FACING == 1 and re.search(r"pub const NRAYS_IRRADIANCE_FACING: u32 = 1;", FFI)
    # the layout, from the C compiler itself
    src = tmp_path / "layout.c"
    names = [n for n, _, _, _ in STRUCT_FIELDS]
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "nrays_abi.h"\nint main(void) {\n    printf("%zu", sizeof(NraysIrradianceGrid));\n'
                   + "".join('    printf(" %%zu", offsetof(NraysIrradianceGrid, %s));\n' % n for n in names) + '    printf("\\n");\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).decode().split()]
    assert got == [C.sizeof(abi.NraysIrradianceGrid)] + [getattr(abi.NraysIrradianceGrid, n).offset for n in names]
    assert got == [88, 0, 24, 48, 60, 64, 72, 80, 84]


def test_the_symbols_are_exported_and_the_abi_version_is_still_7(built):
    assert re.search(r"#define NRAYS_ABI_VERSION 7\b", HEADER) and abi.ABI_VERSION == 7 and abi.load_hip_lib().nrays_abi_version() == 7
    note = re.search(r"Added after 7 WITHOUT a bump.*?\*/", HEADER_TEXT, re.S).group(0)
    exported = subprocess.check_output(["nm", "-D", "--defined-only", abi.HIP_LIB_PATH]).decode()
    for name in EXPECTED:
        assert re.search(r"%s\b" % name, note), name
        assert (" T " + name + "\n") in exported, name
        assert getattr(abi.load_hip_lib(), name).argtypes == abi.HIP_SYMBOLS[name][1]


def test_the_python_names_exist():
    for name in ("irradiance_points", "irradiance_points_ref", "probe_grid_positions", "bake_probe_grid"):
        assert callable(getattr(nr, name)), name
    assert nr.ProbeGrid._fields == ("origin", "cell", "counts", "sh", "valid", "measure")
    g = nr.ProbeGrid((0, 0, 0), (1, 1, 1), (1, 1, 1), None)
    assert g.valid is None and g.measure == 4.0 * math.pi
    from nrays_amd import scenefile
    for cls in (nr.Scene, scenefile.FileScene):
        assert callable(cls.irradiance_points) and callable(cls.bake_probe_grid)


def test_without_a_scene_every_call_is_a_bad_arg(built):
    lib = abi.load_hip_lib()
    a = (C.c_double * 3)(0.0, 0.0, 1.0)
    sh = (C.c_float * 3)(1.0, 1.0, 1.0)
    rgb, osh, wt = (C.c_float * 3)(7.0, 7.0, 7.0), (C.c_float * 3)(7.0, 7.0, 7.0), (C.c_float * 1)(7.0)
    grid = abi.NraysIrradianceGrid((C.c_double * 3)(0, 0, 0), (C.c_double * 3)(1, 1, 1), (C.c_uint32 * 3)(1, 1, 1), 1, C.addressof(sh), None, 1.0, 0)
    for n in (0, 1):
        assert lib.nrays_irradiance_points(None, n, a, a, None, C.byref(grid), rgb, osh, wt, 0) == abi.ERR_BAD_ARG
        assert lib.nrays_irradiance_points_device(None, n, C.addressof(a), C.addressof(a), None, C.byref(grid), C.addressof(rgb), C.addressof(osh), C.addressof(wt), 0, None) == abi.ERR_BAD_ARG
    assert lib.nrays_last_error() and list(rgb) == [7.0] * 3 and list(osh) == [7.0] * 3 and list(wt) == [7.0]


# ---- the Python wrapper checks before any library call ------------------------------------------------------------------------------------------------------
def _good(n=4):
    return dict(points=np.zeros((n, 3)), normals=np.tile([0.0, 1.0, 0.0], (n, 1)), grid=random_grid(1, (2, 3, 2)))


def test_irradiance_points_rejects_bad_arguments_before_any_library_call(no_library):
    import torch
    sc = _NoDevice()
    g = _good()["grid"]
    sh = g.sh
    bad = [
        dict(points=np.zeros((4, 2))), dict(points=None), dict(normals=None), dict(normals=np.zeros((5, 3))), dict(points=np.zeros((4, 3), np.int64)),
        dict(hit_flags=np.ones(3, np.uint32)), dict(hit_flags=np.ones(4, np.float32)), dict(facing=1), dict(facing=None),
        dict(grid=None), dict(grid=(g.origin, g.cell, g.counts, sh)), dict(grid=sh),
        dict(grid=g._replace(origin=(0.0, math.nan, 0.0))), dict(grid=g._replace(origin=(0.0, math.inf, 0.0))), dict(grid=g._replace(origin=(0.0, 0.0))),
        dict(grid=g._replace(cell=(0.5, 0.0, 0.5))), dict(grid=g._replace(cell=(0.5, -1.0, 0.5))), dict(grid=g._replace(cell=(math.inf, 1.0, 0.5))),
        dict(grid=g._replace(cell=(math.nan, 1.0, 0.5))), dict(grid=g._replace(cell=(1.0, 1.0))),
        dict(grid=g._replace(counts=(2, 3, 0))), dict(grid=g._replace(counts=(2, 3, 1025))), dict(grid=g._replace(counts=(2.0, 3.0, 2.0))), dict(grid=g._replace(counts=(2, 3))),
        dict(grid=g._replace(counts=(1024, 1024, 8), sh=np.zeros((1, 1, 3), np.float32))),  # more than 2^22 probes
        dict(grid=g._replace(counts=(2, 3, 3))),  # sh holds 12 probes
        dict(grid=g._replace(sh=sh.astype(np.float64))), dict(grid=g._replace(sh=sh[:, :8])), dict(grid=g._replace(sh=sh[:, :, :2])), dict(grid=g._replace(sh=None)),
        dict(grid=g._replace(sh=sh.tolist())), dict(grid=g._replace(sh=sh.reshape(-1))),
        dict(grid=g._replace(sh=torch.zeros((12, 9, 3), dtype=torch.float32))),  # numpy points, a host tensor as the table
        dict(grid=g._replace(valid=np.ones(11, np.uint32))), dict(grid=g._replace(valid=np.ones(12, np.float32))),
        dict(grid=g._replace(measure=math.inf)), dict(grid=g._replace(measure=math.nan)), dict(grid=g._replace(measure=1e39)),
        dict(normals=torch.zeros((4, 3), dtype=torch.float64)),  # numpy and torch mixed
    ]
    for kw in bad:
        args = dict(_good(), **kw)
        with pytest.raises(ValueError):
            nr.irradiance_points(sc, **args)
    with pytest.raises(ValueError):
        nr.irradiance_points(sc, torch.zeros((4, 3), dtype=torch.float64), torch.zeros((4, 3), dtype=torch.float64), g)  # host tensors
    # a cell on an axis with one probe is ignored, whatever it holds
    one = random_grid(2, (2, 1, 2), cell=(0.5, math.nan, 0.25))
    rgb, _, w = nr.irradiance_points_ref(interior_points(3, one, 9), unit_vectors(4, 9), one, facing=True)
    assert np.isfinite(rgb).all() and same(w, nr.irradiance_points_ref(interior_points(3, one, 9), unit_vectors(4, 9), one._replace(cell=(0.5, -7.0, 0.25)), facing=True)[2])
    for kw in (dict(origin=(0, 0)), dict(counts=(0, 1, 1)), dict(cell=(1.0, 0.0, 1.0))):
        with pytest.raises(ValueError):
            nr.probe_grid_positions(**dict(dict(origin=(0, 0, 0), cell=(1.0, 1.0, 1.0), counts=(2, 2, 2)), **kw))


def test_probe_grid_positions_are_in_row_order():
    pos = nr.probe_grid_positions((1.0, 2.0, 3.0), (0.5, 0.25, 2.0), (3, 2, 2))
    assert pos.shape == (12, 3) and pos.dtype == np.float64
    for iz in range(2):
        for iy in range(2):
            for ix in range(3):
                assert pos[(iz * 2 + iy) * 3 + ix].tolist() == [1.0 + ix * 0.5, 2.0 + iy * 0.25, 3.0 + iz * 2.0]
    assert nr.probe_grid_positions((1.0, 2.0, 3.0), (math.nan, 0.25, 2.0), (1, 2, 1)).tolist() == [[1.0, 2.0, 3.0], [1.0, 2.25, 3.0]]


# ---- the definition, on its mirror ---------------------------------------------------------------------------------------------------------------------------
def test_the_cosine_lobe_constants_are_the_ones_the_header_spells():
    assert SH_COSINE_LOBE == (3.141592653589793, 2.0943951023931953, 0.7853981633974483)
    for a in SH_COSINE_LOBE:
        assert repr(a) in HEADER_TEXT, a


@pytest.mark.parametrize("counts", [(2, 2, 2), (3, 1, 2), (1, 1, 1), (4, 3, 5)])
@pytest.mark.parametrize("bands", [1, 2, 3])
def test_on_a_probe_the_blend_is_the_probe_and_the_irradiance_is_sh_irradiance(counts, bands):
    """All probes valid, no facing, the point ON a probe: one weight is 1 and seven are 0, so s is the probe's row by bit pattern and wsum == 1.  Against
    sh_irradiance in f64 of the same row: a_c (1 rounding), its product (1), C sums, the measure as f32 (1), the last product (1) = C + 4 roundings on
    measure * sum_c |A_c Y_c s_c|."""
    g = random_grid(10 + bands, counts, bands)
    pos = nr.probe_grid_positions(g.origin, g.cell, g.counts)
    nm = unit_vectors(20, len(pos))
    rgb, s, w = nr.irradiance_points_ref(pos, nm, g)
    assert same(s, g.sh) and (w == np.float32(1.0)).all()
    want = nr.sh_irradiance(g.sh.astype(np.float64), nm, g.measure)
    C_ = bands * bands
    Y = np.stack(nr.scene._sh_terms(nm[:, 0], nm[:, 1], nm[:, 2], C_), axis=1)
    mag = g.measure * sum(SH_COSINE_LOBE[BAND[c]] * np.abs(Y[:, c])[:, None] * np.abs(g.sh[:, c].astype(np.float64)) for c in range(C_))
    err = np.abs(rgb.astype(np.float64) - want)
    print("relative error %.3g of the bound's %.3g" % ((err / mag).max(), gamma(C_ + 4)))
    assert (err <= gamma(C_ + 4) * mag).all()


def test_an_affine_field_of_coefficients_is_reproduced():
    """sh[probe] = alpha + beta . position, with values exact in f32, against its f64 evaluation at the point: trilinear weights reproduce an affine field exactly,
    so the error is the weights' and the fold's.  X, Y, Z carry an absolute error of 2 u each (f rounded, 1 - f rounded), which the other two factors of the eight
    corners spread to 3 axes * 2 u * 2 = 12 u over sum_k |w_k|; the two products add 2 u: sum_k |dw_k| <= 14 u.  wsum adds 7 u, so |wsum - 1| <= 21 u and, with
    the division's u, sum_k |wn_k - exact_k| <= 14 + 21 + 1 = 36 u.  The fold is a product and up to 7 sums a corner: 8 u.  44 roundings on max|sh|; the f64
    roundings of g (three, < 2^-50 each relative to the cell index, times the field's slope across a cell) are covered by 2^-45 max|sh|."""
    counts, origin, cell = (4, 3, 5), (-0.5, 0.25, 1.0), (0.5, 0.75, 0.25)
    pos = nr.probe_grid_positions(origin, cell, counts)
    rng = np.random.default_rng(30)
    alpha = rng.integers(-8, 9, size=(9, 3)) / 8.0
    beta = rng.integers(-8, 9, size=(9, 3, 3)) / 4.0
    field = lambda p: alpha[None] + np.einsum("cha,na->nch", beta, p)  # noqa: E731
    sh64 = field(pos)
    sh = sh64.astype(np.float32)
    assert (sh.astype(np.float64) == sh64).all()
    g = nr.ProbeGrid(origin, cell, counts, sh)
    p = interior_points(31, g, 4000)
    _, s, w = nr.irradiance_points_ref(p, unit_vectors(32, len(p)), g)
    bound = (44 * U + 2.0 ** -45) * float(np.abs(sh64).max())
    err = float(np.abs(s.astype(np.float64) - field(p)).max())
    print("error %.3g u max|sh| of the bound's 44" % (err / (U * float(np.abs(sh64).max()))))
    assert err <= bound
    assert (np.abs(w.astype(np.float64) - 1.0) <= 21 * U).all()


def test_points_outside_the_grid_and_non_finite_points_take_the_border():
    g = random_grid(40, (3, 2, 4))
    lo, hi = np.asarray(g.origin), np.asarray(g.origin) + (np.asarray(g.counts) - 1) * np.asarray(g.cell)
    mid = 0.5 * (lo + hi)
    pts, clamped = [], []
    for a in range(3):
        for side, edge in ((-1.0, lo), (1.0, hi)):
            for far in (0.125, 1e6, 1e300, math.inf):
                p = mid.copy(); p[a] = edge[a] + side * far
                q = mid.copy(); q[a] = edge[a]
                pts.append(p); clamped.append(q)
        p = mid.copy(); p[a] = math.nan
        q = mid.copy(); q[a] = lo[a]  # a NaN cell coordinate becomes 0
        pts.append(p); clamped.append(q)
    pts.append(np.full(3, math.nan)); clamped.append(lo)
    pts.append(np.array([math.inf, -math.inf, math.nan])); clamped.append(np.array([hi[0], lo[1], lo[2]]))
    pts, clamped = np.asarray(pts), np.asarray(clamped)
    nm = unit_vectors(41, len(pts))
    rgb, s, w = nr.irradiance_points_ref(pts, nm, g)
    want = nr.irradiance_points_ref(clamped, nm, g)
    assert np.isfinite(rgb).all() and np.isfinite(s).all() and (w == np.float32(1.0)).all()
    assert same(rgb, want[0]) and same(s, want[1])


def test_invalid_probes_never_reach_a_result():
    counts = (3, 3, 3)
    valid = np.random.default_rng(50).integers(0, 2, size=27).astype(np.uint32)
    valid[13] = 0
    valid[valid == 1] = np.random.default_rng(51).integers(0, 1 << 31, size=int(valid.sum())).astype(np.uint32) * 2 + 1  # only bit 0 counts
    valid[valid == 0] = 0x7ffffffe
    g = random_grid(52, counts, valid=valid)
    poisoned = g.sh.copy()
    poisoned[(valid & 1) == 0] = np.nan
    p, nm = interior_points(53, g, 600), unit_vectors(54, 600)
    for facing in (False, True):
        got = nr.irradiance_points_ref(p, nm, g._replace(sh=poisoned), facing=facing)
        want = nr.irradiance_points_ref(p, nm, g, facing=facing)
        assert all(np.isfinite(x).all() for x in got) and all(same(a, b) for a, b in zip(got, want))
        assert (got[2] < np.float32(1.0)).any() and (got[2] == 0).sum() < 600
    # every probe invalid: exact zeros and a weight of 0
    rgb, s, w = nr.irradiance_points_ref(p, nm, g._replace(sh=np.full_like(g.sh, np.nan), valid=np.zeros(27, np.uint32)), facing=True)
    for x in (rgb, s, w):
        assert (x.view(np.uint32) == 0).all()


def test_the_facing_factor_lies_in_its_range_and_changes_results():
    g = random_grid(60, (1, 1, 1), origin=(0.0, 0.0, 0.0))  # one probe: wsum is the factor itself
    nm = unit_vectors(61, 500)
    p = unit_vectors(62, 500) * np.random.default_rng(63).uniform(0.01, 3.0, size=(500, 1))
    rgb, s, w = nr.irradiance_points_ref(p, nm, g, facing=True)
    assert (w >= np.float32(0.2)).all() and (w <= np.float32(1.2 * (1 + 4 * U))).all() and w.min() < 0.3 and w.max() > 1.1
    assert same(s, np.broadcast_to(g.sh[0], s.shape))  # w / w == 1: the blend of one probe is the probe
    rgb0, s0, w0 = nr.irradiance_points_ref(p, nm, g)
    assert (w0 == 1).all() and same(rgb0, rgb)
    # the probe at the point itself: l2 == 0, t = 1, the factor is f32(1.2)
    assert nr.irradiance_points_ref(np.zeros((1, 3)), nm[:1], g, facing=True)[2][0] == np.float32(1.0 * 1.0 + 0.2)
    # more probes: the weights shift towards the probes the normal faces
    g8 = random_grid(64, (2, 2, 2))
    p8 = interior_points(65, g8, 200)
    a, b = nr.irradiance_points_ref(p8, nm[:200], g8, facing=True), nr.irradiance_points_ref(p8, nm[:200], g8)
    assert not same(a[0], b[0]) and not same(a[1], b[1])
    assert (a[2] >= np.float32(0.2 * (1 - 16 * U))).all() and (a[2] <= np.float32(1.2 * (1 + 16 * U))).all()


def test_skipped_points_are_zeros_and_read_nothing():
    g = random_grid(70, (2, 2, 2))
    p, nm = interior_points(71, g, 40), unit_vectors(72, 40)
    flags = np.random.default_rng(73).integers(0, 2, size=40).astype(np.uint32) | np.uint32(2)
    pp, nn = p.copy(), nm.copy()
    pp[(flags & 1) == 0] = np.nan; nn[(flags & 1) == 0] = np.nan
    got = nr.irradiance_points_ref(pp, nn, g, True, flags)
    want = nr.irradiance_points_ref(p, nm, g, True)
    live = (flags & 1) != 0
    for a, b in zip(got, want):
        assert same(a[live], b[live]) and (a[~live].view(np.uint32) == 0).all()


def test_the_furnace_gives_pi_times_the_radiance():
    """A constant radiance L folded by sh_fold_ref over sphere_dirs(1024), blended from eight identical probes, at any normal: pi L within furnace_bound."""
    dirs = nr.sphere_dirs(1024)
    L = np.asarray([0.5, 0.25, 0.125], np.float32)
    sh = nr.sh_fold_ref(dirs[None], np.broadcast_to(L, (1, 1024, 3)).copy())
    g = nr.ProbeGrid((0.25, 0.25, 0.25), (0.5, 0.5, 0.5), (2, 2, 2), np.ascontiguousarray(np.broadcast_to(sh, (8, 9, 3))))
    p, nm = interior_points(80, g, 2000), unit_vectors(81, 2000)
    bound, table_rel = furnace_bound(dirs, L)
    assert 7.8e-5 < table_rel < 8.0e-5  # the table's part, relative to pi L
    for facing in (False, True):
        rgb = nr.irradiance_points_ref(p, nm, g, facing=facing)[0].astype(np.float64)
        err = np.abs(rgb - math.pi * L.astype(np.float64))
        print("furnace: relative error %.3g, bound %.3g" % ((err / (math.pi * L)).max(), (bound / (math.pi * L)).max()))
        assert (err <= bound).all()
