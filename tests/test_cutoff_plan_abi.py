"""kmvp_cutoff_plan_read and the "cutoff_plan" option without a GPU: the entry is declared in include/kmvp.h, bound in
_lib.SYMBOLS with its seven arguments and exported by the built library, which holds the device build's kernels; the option
is documented where the options are, and the plugins translate cutoff_plan="host" | "device" before they touch the library."""
import ctypes
import os
import re

import numpy as np
import pytest

from kernel_matrix_benchmarks_amd import _lib
from kernel_matrix_benchmarks_amd.algorithms import mi355x

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "kmvp.h")).read()
    m = re.search(r"^int kmvp_cutoff_plan_read\(([^;]*)\);", header, flags=re.M)
    assert m, "include/kmvp.h does not declare kmvp_cutoff_plan_read"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert params == ["kmvp_ctx* ctx", "int64_t sizes[13]", "double grid[4]", "int64_t* tiles", "int64_t* runs", "int64_t* tmap",
                      "int64_t* smap"]
    entry = [s for s in _lib.SYMBOLS if s[0] == "kmvp_cutoff_plan_read"]
    assert len(entry) == 1 and entry[0][1] is ctypes.c_int and entry[0][2] == [ctypes.c_void_p] * 7
    lib = _lib.load()
    assert hasattr(lib, "kmvp_cutoff_plan_read")
    assert lib.kmvp_cutoff_plan_read(None, None, None, None, None, None, None) != 0      # a NULL context is an error, not a crash
    binary = open(_lib.LIB_PATH, "rb").read()
    for kernel in (b"cutoff_extent_partial_kernel", b"cutoff_keys_kernel", b"cutoff_first_kernel", b"cutoff_tile_write_kernel",
                   b"cutoff_tmap_kernel", b"cutoff_smap_kernel"):
        assert kernel in binary, kernel
    assert hasattr(_lib.Context, "cutoff_plan") and _lib.CUTOFF_PLAN_SIDES == ("host", "device")


def test_option_is_documented_and_the_lists_have_lost_the_item():
    header = open(os.path.join(ROOT, "include", "kmvp.h")).read()
    options = header[header.index("int kmvp_set_option(") - 12000:header.index("int kmvp_set_option(")]
    assert '"cutoff_plan"' in options and "0 (default) = on the host" in options and "1 = on the device" in options
    assert "sizes[13]" in header and "[12] the side" in header
    api = open(os.path.join(ROOT, "kernel_matrix_benchmarks_amd", "csrc", "kmvp_api.hip")).read()
    assert 'k == "cutoff_plan"' in api
    for name in ("include/kmvp.h", "README.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, name)).read()
        assert "a device-side plan build" not in text and "a device-side plan." not in text and "a device-side plan (" not in text, name
    assert "cutoff_plan" in open(os.path.join(ROOT, "README.md")).read()


def test_plugins_translate_the_option(monkeypatch):
    options = []

    class Quiet:
        comm_world = 0

        def __init__(self, device=0):
            pass

        def set_option(self, key, value):
            options.append((key, value))

        def set_points(self, y, x, dtype, j_offset=0, M_total=None):
            pass

        def close(self):
            pass

    monkeypatch.setattr(_lib, "Context", Quiet)
    y = np.random.RandomState(0).rand(50, 3)
    for side, want in (("host", []), ("device", [("cutoff_plan", 1)])):
        options.clear()
        algo = mi355x.MI355XProduct(kernel="gaussian", dimension=3, cutoff_plan=side)
        algo.prepare_data(source_points=y, target_points=y, same_points=True)
        assert [o for o in options if o[0] == "cutoff_plan"] == want
        options.clear()
        solver = mi355x.MI355XSolver(kernel="wendland-c2", dimension=3, support_radius=0.2, cutoff_plan=side)
        solver.prepare_data(source_points=y)
        assert [o for o in options if o[0] == "cutoff_plan"] == want
    for cls, extra in ((mi355x.MI355XProduct, {}), (mi355x.MI355XSolver, {"support_radius": 0.2})):
        with pytest.raises(ValueError, match="cutoff_plan"):
            cls(kernel="wendland-c2", dimension=3, cutoff_plan="gpu", **extra)
