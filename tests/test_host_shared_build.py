"""One-cell workgroups of cellmm16_kernel's MAIN list (csrc/kmvp_plan.hpp: count_one_cell_blocks), without a GPU: the header
is plain C++, compiled here with the host compiler behind tests/host_shared_build_shim.cpp.

A workgroup whose four wavefronts own target tiles of one cell builds every source operand once and shares it (option
``cell_shared_build``); the others run the body they always ran.  Counted on the lists cell_tiles_split() really builds:

* the benchmark's config 2 (1e6 uniform points, 10 x 10 x 10 cells, eight tiles per wavefront): all 1000 workgroups of the
  MAIN list are one-cell, so the shared build is what the headline runs;
* the two clouds of tests/test_cellmm16_shared_build.py have one-cell AND mixed workgroups at four and at eight tiles per
  wavefront, and the second one a REST list at eight: the GPU test compares the two bodies where both run in one launch.
"""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "kernel_matrix_benchmarks_amd", "csrc")
i64, i32, vp = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p
P64 = ctypes.POINTER(i64)


@pytest.fixture(scope="module")
def plan():
    tmp = tempfile.mkdtemp(prefix="kmvp_host_shared_")
    so = os.path.join(tmp, "libhost_shared.so")
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC,
                           os.path.join(HERE, "host_shared_build_shim.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.hs_constants.argtypes = [P64]
    lib.hs_one_cell_blocks.argtypes = [vp, i64, i32, P64]
    lib.hs_shared_build.argtypes = [i32, i32]
    yield lib
    shutil.rmtree(tmp, ignore_errors=True)


def grid_keys(y):
    """Sorted cell keys of the float32 points `y` on the grid of cell_make_grid(): the bounding box in the fewest equal
    cells of side <= sqrt(2 CELL_T_MAX / D), 10 bits per axis."""
    y = np.asarray(y, np.float32)
    n, D = y.shape
    h_max = np.float32(np.sqrt(np.float32(2.0) * np.float32(0.016) / np.float32(D)))
    key = np.zeros(n, np.uint32)
    cells = []
    for a in range(D):
        lo, hi = y[:, a].min(), y[:, a].max()
        centre, half = np.float32(0.5) * (lo + hi), np.float32(0.5) * (hi - lo)
        g = int(max(1.0, np.ceil(2.0 * float(half) / float(h_max))))
        inv_h = np.float32(1.0) / np.float32(2.0 * float(half) / g)
        c = np.floor((y[:, a] - (centre - half)) * inv_h).astype(np.int64).clip(0, g - 1)
        key |= c.astype(np.uint32) << np.uint32(10 * a)
        cells.append(g)
    return np.sort(key), cells


def one_cell(plan, keys, tt):
    keys = np.ascontiguousarray(keys, np.uint32)
    out = (i64 * 4)()
    plan.hs_one_cell_blocks(keys.ctypes.data, len(keys), tt, out)
    return dict(zip(("n_main", "n_rest", "blocks", "one_cell"), out))


def cloud_a():
    return (np.random.RandomState(1).rand(40000, 3) * 0.3).astype(np.float32)


def cloud_b():
    return (np.random.RandomState(2).rand(35000, 3) * 0.2).astype(np.float32)


def test_headline_shape_is_all_one_cell(plan):
    n, D = 1_000_000, 3
    keys, cells = grid_keys(np.random.RandomState(n + D).rand(n, D))  # bench.py's config 2
    assert cells == [10, 10, 10]
    r = one_cell(plan, keys, 8)
    assert (r["n_main"], r["blocks"]) == (32000, 1000)
    assert r["one_cell"] == 1000


@pytest.mark.parametrize("tt", [4, 8])
@pytest.mark.parametrize("cloud", [cloud_a, cloud_b], ids=["A", "B"])
def test_clouds_have_one_cell_and_mixed_workgroups(plan, cloud, tt):
    keys, _ = grid_keys(cloud())
    r = one_cell(plan, keys, tt)
    print(cloud.__name__, tt, r)
    assert r["blocks"] * tt * 4 == r["n_main"]
    assert r["one_cell"] > 0 and r["blocks"] - r["one_cell"] > 0, r


def test_cloud_b_has_a_rest_list_at_eight_tiles(plan):
    keys, _ = grid_keys(cloud_b())
    assert one_cell(plan, keys, 8)["n_rest"] > 0


def test_count_on_hand_made_lists(plan):
    # eight tiles per wavefront, four wavefronts: 32 tiles per workgroup, compared by the first tile of each wavefront
    def count(tile_keys, tt):
        k = np.repeat(np.asarray(tile_keys, np.uint32), 32)  # one full tile of 32 points per key entry
        return one_cell(plan, k, tt)
    r = count([5] * 32 + [6] * 32, 8)          # two cells of exactly one workgroup each
    assert (r["blocks"], r["one_cell"], r["n_rest"]) == (2, 2, 0)
    r = count([5] * 16 + [6] * 16, 8)          # one workgroup, two wavefronts per cell
    assert (r["blocks"], r["one_cell"]) == (1, 0)
    r = count([5] * 24 + [6] * 8 + [7] * 32, 8)  # the last wavefront alone differs; then a one-cell workgroup
    assert (r["blocks"], r["one_cell"]) == (2, 1)
    r = count([5] * 8, 8)                      # one wavefront of tiles, the workgroup padded with empty tiles of the same key
    assert (r["blocks"], r["one_cell"]) == (1, 1)
    assert one_cell(plan, np.zeros(0, np.uint32), 8)["blocks"] == 0


def test_option_rule(plan):
    k = (i64 * 4)()
    plan.hs_constants(k)
    shared_tt = k[0]
    assert shared_tt == 8
    for tt in (1, 2, 4, 8):
        assert plan.hs_shared_build(tt, 0) == 0
        assert plan.hs_shared_build(tt, -1) == plan.hs_shared_build(tt, 1) == (1 if tt >= shared_tt else 0)
