"""Writes tests/golden/reference_patch_preimage.json: for every hunk of integration/rust/patches/0001-gpu-trace-loop.patch, the sha256 of
the reference checkout's lines the hunk replaces (its context and '-' lines, at the line numbers of its header).  tests/test_integration_rust.py
checks the patch against these digests, so the test needs no checkout and no reference source is stored in this repository.

  python tests/golden/make_reference_patch_digests.py REFERENCE_CHECKOUT
Refuses to write when the patch's pre-image differs from the checkout's text at any hunk (the patch would not apply without offset or fuzz)."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests.test_integration_rust import PATCH, PREIMAGE_DIGESTS, patch_hunks  # noqa: E402


def main(ref):
    files = {}
    for path, hunks in patch_hunks(open(PATCH, newline="").read()).items():
        lines = open(os.path.join(ref, path), newline="").read().split("\n")
        rec = []
        for start, n, pre in hunks:
            window = lines[start - 1:start - 1 + n]
            if window != pre:
                raise SystemExit("%s: the hunk at line %d does not match the checkout" % (path, start))
            rec.append([start, n, hashlib.sha256("\n".join(window).encode()).hexdigest()])
        files[path] = {"lines": len(lines), "hunks": rec}
    with open(PREIMAGE_DIGESTS, "w") as f:
        json.dump({"patch": os.path.relpath(PATCH, ROOT), "files": files}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1])
