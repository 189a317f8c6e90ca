"""kmvp_dbscan through the layers, without a GPU: declared in include/kmvp.h with its seven parameters, bound in
_lib.SYMBOLS, exported by the built library next to its pair loop, refusing a NULL context, and wrapped by MI355XDBSCAN."""
import ctypes
import os
import re

import numpy as np
import pytest

from kernel_matrix_benchmarks_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(HERE, "..", "include", "kmvp.h")


def test_header_declares_the_entry_with_seven_parameters():
    with open(HEADER) as f:
        text = f.read()
    m = re.search(r"^int kmvp_dbscan\(([^;]*)\);", text, flags=re.M)
    assert m, "include/kmvp.h does not declare kmvp_dbscan"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["kmvp_ctx* ctx", "double radius", "int64_t min_samples", "int64_t* labels", "int64_t* core_of_or_null",
                      "int64_t* counts_or_null", "int64_t info[6]"]


def test_symbols_bind_the_entry():
    entry = [s for s in _lib.SYMBOLS if s[0] == "kmvp_dbscan"]
    assert len(entry) == 1 and entry[0][1] is ctypes.c_int and len(entry[0][2]) == 7
    assert entry[0][2][1] is ctypes.c_double and entry[0][2][2] is ctypes.c_int64
    assert hasattr(_lib.Context, "dbscan")


def test_library_exports_the_entry_and_holds_the_kernel():
    lib = _lib.load()
    assert hasattr(lib, "kmvp_dbscan")
    with open(_lib.LIB_PATH, "rb") as f:
        blob = f.read()
    assert b"lowd_cutoff_label_kernel" in blob


def test_a_null_context_is_an_error_not_a_crash():
    lib = _lib.load()
    out, info = np.zeros(4, dtype=np.int64), np.zeros(6, dtype=np.int64)
    assert lib.kmvp_dbscan(None, 0.5, 3, out.ctypes.data, None, None, info.ctypes.data) == 1  # KMVP_E_INVALID
    assert lib.kmvp_dbscan(None, float("nan"), 0, None, None, None, None) == 1


def test_the_plugin_exists_and_checks_its_arguments():
    from kernel_matrix_benchmarks_amd.algorithms import mi355x

    algo = mi355x.MI355XDBSCAN(eps=0.1, min_samples=5, dimension=3, precision="float16", cutoff_plan="device", cutoff_cell_factor=1.5)
    assert algo.eps == 0.1 and algo.min_samples == 5 and "MI355XDBSCAN" in algo.name
    for method in ("prepare_data", "set_query_arguments", "query", "get_labels", "get_core_sample_indices", "get_core_of",
                   "get_counts", "get_memory_usage", "get_additional", "done"):
        assert callable(getattr(algo, method))
    assert algo.get_memory_usage() == 0 and algo.get_additional() == {}
    with pytest.raises(RuntimeError):
        algo.query()
    with pytest.raises(RuntimeError):
        algo.get_labels()
    for bad in (dict(eps=0.0), dict(eps=float("inf")), dict(min_samples=0), dict(min_samples=2.5)):
        with pytest.raises(ValueError):
            algo.set_query_arguments(**bad)
    with pytest.raises(ValueError):
        mi355x.MI355XDBSCAN(eps=0.1, min_samples=5, dimension=3, cutoff_plan="elsewhere")
    with pytest.raises(NotImplementedError):
        mi355x.MI355XDBSCAN(eps=0.1, min_samples=5, dimension=4)
    with pytest.raises(NotImplementedError):
        mi355x.MI355XDBSCAN(eps=0.1, min_samples=5, dimension=3, precision="bfloat16")
    with open(os.path.join(HERE, "..", "algos.yaml")) as f:
        assert "MI355XDBSCAN" not in f.read()  # an extension: the reference has no such role
