"""The Rust side of the drop-in (integration/rust/) cannot be compiled here (no Rust toolchain), so
these tests keep it honest mechanically: the `#[repr(C)]` structs of gpu_ffi.rs list exactly the fields of
include/nrays_abi.h in the same order, every entry point of the header is declared, every type gpu.rs relies on is
defined, and the patch applies cleanly to the reference checkout (checked against digests of the checkout's text, see
tests/golden/make_reference_patch_digests.py)."""
import hashlib
import json
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUST = os.path.join(ROOT, "integration", "rust")
PATCH = os.path.join(RUST, "patches", "0001-gpu-trace-loop.patch")
PREIMAGE_DIGESTS = os.path.join(ROOT, "tests", "golden", "reference_patch_preimage.json")
HEADER = open(os.path.join(ROOT, "include", "nrays_abi.h")).read()
FFI = open(os.path.join(RUST, "src", "gpu_ffi.rs")).read()
GPU = open(os.path.join(RUST, "src", "gpu.rs")).read()


def _c_structs():
    out = {}
    for m in re.finditer(r"typedef struct (\w+) \{(.*?)\} \1;", HEADER, re.S):
        body = re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S)
        out[m.group(1)] = [re.sub(r"\[.*", "", f.strip().split()[-1]).lstrip("*") for f in body.split(";") if f.strip()]
    return out


def _rust_structs():
    out = {}
    for m in re.finditer(r"pub struct (\w+) \{(.*?)\n\}", FFI, re.S):
        out[m.group(1)] = re.findall(r"pub (\w+):", m.group(2))
    return out


def test_repr_c_structs_match_the_header_field_for_field():
    c, r = _c_structs(), _rust_structs()
    assert set(c) == {"NraysLight", "NraysTexture", "NraysMaterial", "NraysMesh", "NraysNode", "NraysSceneDesc", "NraysRenderParams", "NraysStats", "NraysCastResult", "NraysTileCosts", "NraysMultiTimings", "NraysBlasDump", "NraysSceneDump"}
    for name, fields in c.items():
        assert r.get(name) == fields, (name, fields, r.get(name))
        assert re.search(r"#\[repr\(C\)\]\s*(#\[derive[^\]]*\]\s*)?pub struct %s " % name, FFI), name


def test_every_entry_point_of_the_header_is_declared():
    c_fns = set(re.findall(r"\b(nrays_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)))
    rust_fns = set(re.findall(r"pub fn (nrays_\w+)\(", FFI))
    assert c_fns == rust_fns, (c_fns ^ rust_fns)
    for enum in re.findall(r"(NRAYS_(?:ERR|SHAPE|MAT|TEXEL|INTERP|OVERFLOW)_\w+|NRAYS_OK) = (-?\d+)", HEADER):
        assert re.search(r"pub const %s: \w+ = %s;" % enum, FFI), enum


def test_gpu_rs_defines_what_it_uses():
    for item in ("pub enum ShapeDesc", "pub struct MeshData", "pub trait FlattenShape", "pub struct MaterialDesc", "pub struct TextureTable",
                 "pub struct FlatScene", "pub fn flatten(&self) -> Result<FlatScene, String>", "pub struct GpuScene", "pub fn render(",
                 "pub struct GpuSceneSet", "pub fn render_multi("):
        assert item in GPU, item
    for shape in ("Ball", "Cuboid", "Cylinder", "Capsule", "Cone", "Plane", "TriMesh"):  # loader3d.rs:601-695
        assert "impl FlattenShape for %s<Scalar>" % shape in GPU, shape
    patch = open(os.path.join(RUST, "patches", "0001-gpu-trace-loop.patch")).read()
    for hook in ("+ FlattenShape,", "shape: geometry.shape_desc()", "fn flatten(&self) -> Option<MaterialDesc>", "pub fn nodes(&self)",
                 "pub fn background(&self)", "pub fn data(&self) -> &Arc<ImageData>", "NRAYS_GPUS", 'build   = "build.rs"'):
        assert hook in patch, hook
    # every ffi name gpu.rs calls exists in gpu_ffi.rs
    for name in set(re.findall(r"\b(nrays_\w+)\(", GPU)):
        assert "pub fn %s(" % name in FFI, name


def patch_hunks(text):
    """{path: [(first old line, old line count, pre-image lines)]} of a unified diff with a/ b/ prefixes; the hunk headers' counts are checked."""
    out, path, lines = {}, None, iter(text.split("\n"))
    for line in lines:
        if line.startswith("+++ "):
            path = line[4:].split("\t")[0].split("/", 1)[1]
            out[path] = []
        m = re.match(r"@@ -(\d+)(?:,(\d+))? \+(\d+)(?:,(\d+))? @@", line)
        if not m:
            continue
        n_old, n_new = int(m.group(2) or 1), int(m.group(4) or 1)
        pre, new = [], 0
        while len(pre) < n_old or new < n_new:
            body = next(lines)
            if body.startswith("\\"):  # "\ No newline at end of file"
                continue
            tag = body[:1] or " "
            assert tag in " -+", (path, body)
            if tag in " -":
                pre.append(body[1:])
            if tag in " +":
                new += 1
        assert len(pre) == n_old and new == n_new, (path, line)
        out[path].append((int(m.group(1)), n_old, pre))
    return out


def test_patch_applies_to_the_reference_checkout():
    """Every hunk's pre-image (context and '-' lines) is the reference checkout's text at the lines its header names — `patch -p1` applies it
    without offset or fuzz — checked against sha256 digests of those lines of the checkout (tests/golden/reference_patch_preimage.json)."""
    pinned = json.load(open(PREIMAGE_DIGESTS))
    assert pinned["patch"] == os.path.relpath(PATCH, ROOT)
    hunks = patch_hunks(open(PATCH, newline="").read())
    assert sorted(hunks) == sorted(pinned["files"])
    for path, hs in hunks.items():
        ref = pinned["files"][path]
        assert [(start, n) for start, n, _ in hs] == [(start, n) for start, n, _ in ref["hunks"]], path
        end = 0
        for (start, n, pre), (_, _, digest) in zip(hs, ref["hunks"]):
            assert end < start and start - 1 + n <= ref["lines"], (path, start)  # in order, inside the file
            assert hashlib.sha256("\n".join(pre).encode()).hexdigest() == digest, (path, start)
            end = start - 1 + n
