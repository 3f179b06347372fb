#!/usr/bin/env python
"""Is the device code of two builds of libnrays_hip.so the same?  Compares the gfx950 code objects of the two libraries kernel by kernel, as text.

  python tools/isa_same.py OLD.so NEW.so [--allow SUBSTRING ...]

The code objects (one per translation unit that holds a kernel, in link order) are cut out of the libraries' offload bundles and disassembled with llvm-objdump.
Per kernel symbol the instruction text is compared: addresses, encodings and comments are dropped, the padding behind a kernel is dropped, and the literal of the
two additions that follow an s_getpc_b64 (a pc-relative distance, which moves with a kernel's place in its code object) is masked.  Prints the number of kernels
compared, the kernels that differ, the kernels that moved to another unit and the kernels only one library has.  Exit status 0: same symbols, same units, nothing
differs or is missing except kernels whose name holds an --allow substring (a kernel whose argument list changed has another symbol: it is missing from both)."""
import os
import re
import struct
import subprocess
import sys
import tempfile

OBJDUMP = os.environ.get("LLVM_OBJDUMP", "/opt/rocm/lib/llvm/bin/llvm-objdump")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
PADDING = ("s_nop", "s_code_end", "...")


def code_objects(path):
    """The gfx950 code objects of the library's offload bundles, in file order."""
    data = open(path, "rb").read()
    out, at = [], data.find(MAGIC)
    while at >= 0:
        (count,) = struct.unpack_from("<Q", data, at + len(MAGIC))
        p = at + len(MAGIC) + 8
        for _ in range(count):
            off, size, idlen = struct.unpack_from("<QQQ", data, p)
            triple = data[p + 24:p + 24 + idlen].decode()
            p += 24 + idlen
            if "gfx950" in triple and size:
                out.append(data[at + off:at + off + size])
        at = data.find(MAGIC, at + len(MAGIC))
    return out


def kernels(co, directory, index):
    """{kernel symbol: [instruction text]} of one code object."""
    path = os.path.join(directory, "unit%d.co" % index)
    with open(path, "wb") as f:
        f.write(co)
    names = set()
    for line in subprocess.check_output([OBJDUMP, "--syms", path], text=True).splitlines():
        m = re.match(r"\S+\s+g\s+F\s+\.text\s+\S+\s+(?:\.protected\s+)?(\S+)$", line)
        if m:
            names.add(m.group(1))
    text = subprocess.check_output([OBJDUMP, "-d", "--no-show-raw-insn", "--no-leading-addr", path], text=True)
    found, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"(?:[0-9a-f]+ )?<(\S+)>:$", line.strip())
        if m:
            cur = found.setdefault(m.group(1), []) if m.group(1) in names else None
            continue
        if cur is None or not line.strip():
            continue
        cur.append(" ".join(line.split("//")[0].split()))
    for name, ins in found.items():
        while ins and ins[-1].split()[0] in PADDING:
            ins.pop()
        for k, text_ in enumerate(ins):
            if text_.startswith("s_getpc_b64"):
                for j in (k + 1, k + 2):
                    if j < len(ins) and ins[j].startswith(("s_add_u32", "s_addc_u32")):
                        ins[j] = re.sub(r",\s*(?:0x[0-9a-f]+|-?\d+)$", ", <pc-relative>", ins[j])
    return found


def library(path, directory):
    """{kernel symbol: (unit index, instructions)}."""
    out = {}
    for index, co in enumerate(code_objects(path)):
        for name, ins in kernels(co, directory, index).items():
            assert name not in out, "%s: %s in two units" % (path, name)
            out[name] = (index, ins)
    return out


def main():
    args, allow = sys.argv[1:], []
    while "--allow" in args:
        k = args.index("--allow")
        allow.append(args[k + 1])
        del args[k:k + 2]
    if len(args) != 2:
        raise SystemExit(__doc__)
    with tempfile.TemporaryDirectory() as d_old, tempfile.TemporaryDirectory() as d_new:
        old, new = library(args[0], d_old), library(args[1], d_new)
    both = sorted(set(old) & set(new))
    differing = [n for n in both if old[n][1] != new[n][1]]
    moved = [n for n in both if old[n][0] != new[n][0]]
    missing = sorted(set(old) ^ set(new))
    demangle = lambda names: subprocess.run(["c++filt"] + names, stdout=subprocess.PIPE, text=True).stdout.splitlines() if names else []  # noqa: E731
    print("code objects: %d and %d" % (1 + max((u for u, _ in old.values()), default=-1), 1 + max((u for u, _ in new.values()), default=-1)))
    print("kernels compared: %d" % len(both))
    print("differing: %d" % len(differing))
    for n, d in zip(differing, demangle(differing)):
        print("  %s   (%d and %d instructions)" % (re.sub(r"\(.*", "", d), len(old[n][1]), len(new[n][1])))
    print("in another unit: %d" % len(moved))
    for n, d in zip(moved, demangle(moved)):
        print("  %s   (unit %d and %d)" % (re.sub(r"\(.*", "", d), old[n][0], new[n][0]))
    print("missing from one library: %d" % len(missing))
    for n, d in zip(missing, demangle(missing)):
        print("  %s   (only in %s)" % (re.sub(r"\(.*", "", d), args[0] if n in old else args[1]))
    unexpected = [n for n in differing + missing if not any(a in n for a in allow)]
    return 1 if unexpected or moved else 0


if __name__ == "__main__":
    sys.exit(main())
