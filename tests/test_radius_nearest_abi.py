"""kmvp_radius_nearest without a GPU: declared in include/kmvp.h, bound in _lib.SYMBOLS with its six arguments, exported by the
built library; MI355XProduct.query_radius_nearest refuses what it is not built for before it touches the library."""
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
    m = re.search(r"^int kmvp_radius_nearest\(([^;]*)\);", header, flags=re.M)
    assert m, "include/kmvp.h does not declare kmvp_radius_nearest"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    assert params == ["kmvp_ctx* ctx", "double radius", "int K", "int exclude_self", "int64_t* out_idx", "double* out_sqdist"]
    entry = [s for s in _lib.SYMBOLS if s[0] == "kmvp_radius_nearest"]
    assert len(entry) == 1 and entry[0][1] is ctypes.c_int and len(entry[0][2]) == 6
    assert entry[0][2][1] is ctypes.c_double and entry[0][2][2] is ctypes.c_int and entry[0][2][3] is ctypes.c_int
    lib = _lib.load()
    assert hasattr(lib, "kmvp_radius_nearest")
    assert lib.kmvp_radius_nearest(None, 0.5, 1, 0, None, None) != 0      # a NULL context is an error, not a crash
    assert b"lowd_cutoff_knn_kernel" in open(_lib.LIB_PATH, "rb").read()
    assert hasattr(_lib.Context, "radius_nearest") and hasattr(mi355x.MI355XProduct, "query_radius_nearest")
    # the "Not built" list of the cutoff entries has lost the item
    assert "Not built: K nearest within a radius" not in header


def test_plugin_refuses_before_it_touches_the_library(monkeypatch):
    calls = []

    class Quiet:
        comm_world = 0

        def __init__(self, device=0):
            pass

        def set_option(self, key, value):
            pass

        def set_points(self, y, x, dtype, j_offset=0, M_total=None):
            pass

        def radius_nearest(self, radius, K, exclude_self=False):
            calls.append((radius, K, exclude_self))
            return "rows"

        def cutoff_info(self):
            return {"cells": (1, 1, 1)}

        def close(self):
            pass

    monkeypatch.setattr(_lib, "Context", Quiet)
    y = np.random.RandomState(0).rand(50, 3)
    same = mi355x.MI355XProduct(kernel="gaussian", dimension=3)
    same.prepare_data(source_points=y, target_points=y, same_points=True)
    with pytest.raises(NotImplementedError, match="k = 17"):
        same.query_radius_nearest(17, 0.2)
    with pytest.raises(NotImplementedError, match="k = 16 > 15 with exclude_self"):
        same.query_radius_nearest(16, 0.2, exclude_self=True)
    other = mi355x.MI355XProduct(kernel="gaussian", dimension=3)
    other.prepare_data(source_points=y, target_points=y[:20], same_points=False)
    with pytest.raises(ValueError, match="exclude_self"):
        other.query_radius_nearest(3, 0.2, exclude_self=True)
    bf16 = mi355x.MI355XProduct(kernel="gaussian", dimension=16, precision="bfloat16")
    bf16.prepare_data(source_points=np.random.RandomState(1).rand(50, 16), target_points=None, same_points=True)
    with pytest.raises(NotImplementedError, match="bfloat16"):
        bf16.query_radius_nearest(3, 0.2)
    wide = mi355x.MI355XProduct(kernel="gaussian", dimension=4)
    wide.prepare_data(source_points=np.random.RandomState(1).rand(50, 4), target_points=None, same_points=True)
    with pytest.raises(NotImplementedError, match="D = 4"):
        wide.query_radius_nearest(3, 0.2)
    fresh = mi355x.MI355XProduct(kernel="gaussian", dimension=3)
    with pytest.raises(RuntimeError, match="prepare_data"):
        fresh.query_radius_nearest(3, 0.2)
    assert calls == []
    # ... and what is asked for properly reaches the library once, in get_nearest()'s slot, with the plan's info kept
    same.query_radius_nearest(15, 0.2, exclude_self=True)
    other.query_radius_nearest(16, 0.25)
    assert calls == [(0.2, 15, True), (0.25, 16, False)]
    assert same.get_nearest() == "rows" and same._cutoff_info == {"cells": (1, 1, 1)}
