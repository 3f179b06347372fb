"""Which k_primary permutations does a test run reach?  A pytest plugin for one-off surveys, loaded by name only:

    NRAYS_PERMUTATION_LOG=perms.json python -m pytest -p tests.permutation_log -m gpu tests

Every render entry point of the ctypes library object (nrays_amd.abi.load_hip_lib) is wrapped on the Python side: after each call the
handle is asked what it launched (nrays_debug_last_permutation) and the tuple is counted under the running test's id.  The library reads
no such switch, the suite's own configuration does not load this module, and renders made from native code (the C++ front-end, the
multi-GPU entry points) are not seen."""
import ctypes as C
import json
import os

RENDER_CALLS = ("nrays_render", "nrays_render_rgb8", "nrays_render_device", "nrays_render_device_instrumented", "nrays_render_device_counted")
_seen = {}


def _install(path):
    from nrays_amd import abi
    load = abi.load_hip_lib

    def wrap(lib, name):
        fn = getattr(lib, name)

        def call(scene, *args):
            rc = fn(scene, *args)
            out = (C.c_uint32 * 6)()
            if rc == 0 and scene and lib.nrays_debug_last_permutation(scene, out) == 0 and out[4]:
                key = "%d,%d,%d,%d" % (out[0], out[1], out[2], out[3])
                test = os.environ.get("PYTEST_CURRENT_TEST", "?").split(" ")[0]
                e = _seen.setdefault(key, {"renders": 0, "tests": []})
                e["renders"] += 1
                if test not in e["tests"] and len(e["tests"]) < 8:
                    e["tests"].append(test)
            return rc
        return call

    def load_logged():
        lib = load()
        if not getattr(lib, "_permutation_log", False):
            for name in RENDER_CALLS:
                setattr(lib, name, wrap(lib, name))
            lib._permutation_log = True
        return lib
    abi.load_hip_lib = load_logged


def pytest_configure(config):
    if os.environ.get("NRAYS_PERMUTATION_LOG"):
        _install(os.environ["NRAYS_PERMUTATION_LOG"])


def pytest_sessionfinish(session, exitstatus):
    path = os.environ.get("NRAYS_PERMUTATION_LOG")
    if path:
        with open(path, "w") as f:
            json.dump(_seen, f, indent=1, sort_keys=True)
