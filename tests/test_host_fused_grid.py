"""The fused grid of cellmm16_kernel (csrc/kmvp_plan.hpp: fused_cell_grid, fused_cell_work), without a GPU: the header is
plain C++, compiled here with the host compiler behind tests/host_fused_grid_shim.cpp.

cellmm16_kernel runs both lists of target tiles in one launch, the REST list's workgroups behind the MAIN list's.  The
kernel decodes its workgroup index with fused_cell_work() itself, so what holds here holds on the device:

* every workgroup of the fused grid is exactly one (list, local index): the MAIN indices first, as they are, then the
  REST indices as bid - main_grid; the totals are grid(0) + grid(1);
* two launches remain where there is no REST list, at CELL_REST_TT tiles per wavefront or fewer, where the grids together
  exceed MAX_GRID, and when the option says so; an empty MAIN list with a REST list is a fused grid with main_grid = 0;
* the headline shape (the benchmark's config 2: 1e6 uniform points in 10 x 10 x 10 cells) is 8000 + 1664 workgroups.
"""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from host_plan_cases import key_sequences

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "kernel_matrix_benchmarks_amd", "csrc")
i64, i32, vp = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p
P64 = ctypes.POINTER(i64)

# run_product_cellmm's rule: stages of 12 source tiles and 8192 bytes, segments of >= 2 stages and <= 3 MiB, 7168 workgroups
CMM_RULE = dict(stage_tiles=12, stage_bytes=8192, min_seg=2, l2_seg_bytes=3 << 20, target_blocks=7168)
FIELDS = ("fused", "main_grid", "rest_grid", "total", "grid0", "grid1", "blocks0", "blocks1", "segments0", "segments1")


@pytest.fixture(scope="module")
def plan():
    tmp = tempfile.mkdtemp(prefix="kmvp_host_fused_")
    so = os.path.join(tmp, "libhost_fused.so")
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC,
                           os.path.join(HERE, "host_fused_grid_shim.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.hf_constants.argtypes = [P64]
    lib.hf_list_sizes.argtypes = [vp, i64, i32, P64, P64]
    lib.hf_fused_cell_grid.argtypes = [i64, i64, i64, i64, i32, i32, i32, i64, i64, i64, i64, i32, P64]
    lib.hf_fused_cell_grid_raw.argtypes = [i64, i32, i64, i32, i32, i32, P64]
    lib.hf_fused_cell_work.argtypes = [i64, i64, i64, vp, vp]
    yield lib
    shutil.rmtree(tmp, ignore_errors=True)


def constants(plan):
    out = (i64 * 4)()
    plan.hf_constants(out)
    return dict(zip(("rest_tt", "waves", "cell_tile", "max_grid"), out))


def list_sizes(plan, keys, tt):
    keys = np.ascontiguousarray(keys, np.uint32)
    nm, nr = i64(), i64()
    plan.hf_list_sizes(keys.ctypes.data, len(keys), tt, ctypes.byref(nm), ctypes.byref(nr))
    return nm.value, nr.value


def tiles_per_cell(keys, tile):
    sizes = np.diff(np.flatnonzero(np.r_[True, keys[1:] != keys[:-1], True])) if len(keys) else np.zeros(0, np.int64)
    return (sizes + tile - 1) // tile


def fused_grid(plan, n_points, m_tiles, n_main, n_rest, tt, opt_fused, opt_segments=0):
    out = (i64 * 10)()
    r = CMM_RULE
    plan.hf_fused_cell_grid(n_points, m_tiles, n_main, n_rest, tt, opt_segments, r["stage_tiles"], r["stage_bytes"],
                            r["min_seg"], r["l2_seg_bytes"], r["target_blocks"], opt_fused, out)
    return dict(zip(FIELDS, out))


def fused_grid_raw(plan, blocks0, segments0, blocks1, segments1, tt, opt_fused):
    out = (i64 * 10)()
    plan.hf_fused_cell_grid_raw(blocks0, segments0, blocks1, segments1, tt, opt_fused, out)
    return dict(zip(FIELDS, out))


def work(plan, bid0, n, main_grid):
    lst, loc = np.zeros(n, np.int64), np.zeros(n, np.int64)
    plan.hf_fused_cell_work(bid0, n, main_grid, lst.ctypes.data, loc.ctypes.data)
    return lst, loc


def check_map(plan, g):
    """every workgroup exactly one (list, local index); MAIN first and the identity, REST as bid - main_grid"""
    total, main = g["total"], g["main_grid"]
    assert total == g["grid0"] + g["grid1"] and main == g["grid0"] and g["rest_grid"] == g["grid1"]
    # whole grids up to a million workgroups, else the two ends and both sides of the seam
    spans = [(0, total)] if total <= 1 << 20 else [(0, 4096), (max(0, main - 4096), min(total, main + 4096)), (total - 4096, total)]
    for lo, hi in spans:
        lst, loc = work(plan, lo, hi - lo, main)
        bid = np.arange(lo, hi, dtype=np.int64)
        assert np.array_equal(lst, (bid >= main).astype(np.int64))
        assert np.array_equal(loc[lst == 0], bid[lst == 0])
        assert np.array_equal(loc[lst == 1], bid[lst == 1] - main)
        assert np.all(loc[lst == 0] < g["grid0"]) and np.all(loc[lst == 1] < g["grid1"]) and np.all(loc >= 0)
    if total <= 1 << 20:  # a bijection onto the two grids
        lst, loc = work(plan, 0, total, main)
        assert len(set(zip(lst.tolist(), loc.tolist()))) == total
        assert np.count_nonzero(lst == 0) == g["grid0"] and np.count_nonzero(lst == 1) == g["grid1"]


@pytest.mark.parametrize("tt", [1, 2, 4, 8])
def test_fused_grid_of_the_key_sequences(plan, tt):
    k = constants(plan)
    for name, keys in key_sequences():
        if len(keys) == 0:
            continue  # (a cloud has at least one point: cell_split() plans no launch over zero source stages)
        n_main, n_rest = list_sizes(plan, keys, tt)
        m_tiles = int(np.sum(tiles_per_cell(keys, k["cell_tile"])))
        for opt_segments in (0, 3, 8):
            auto = fused_grid(plan, len(keys), m_tiles, n_main, n_rest, tt, -1, opt_segments)
            on = fused_grid(plan, len(keys), m_tiles, n_main, n_rest, tt, 1, opt_segments)
            off = fused_grid(plan, len(keys), m_tiles, n_main, n_rest, tt, 0, opt_segments)
            assert auto == on, (name, tt)
            assert not off["fused"] and {f: off[f] for f in FIELDS[1:]} == {f: on[f] for f in FIELDS[1:]}, (name, tt)
            # fused exactly where there is a REST list, which takes more than CELL_REST_TT tiles per wavefront
            assert bool(on["fused"]) == (n_rest > 0), (name, tt)
            if tt <= k["rest_tt"]:
                assert n_rest == 0 and not on["fused"], (name, tt)
            assert on["blocks0"] == n_main // (tt * k["waves"]) and on["blocks1"] == n_rest // (k["rest_tt"] * k["waves"])
            assert on["grid0"] == on["blocks0"] * on["segments0"] and on["grid1"] == on["blocks1"] * on["segments1"]
            check_map(plan, on)


def test_fall_back_conditions(plan):
    k = constants(plan)
    big = k["max_grid"]
    for tt in (4, 8):
        assert fused_grid_raw(plan, 1000, 8, 52, 32, tt, -1)["fused"] == 1
        assert fused_grid_raw(plan, 1000, 8, 52, 32, tt, 1)["fused"] == 1
        assert fused_grid_raw(plan, 1000, 8, 52, 32, tt, 0)["fused"] == 0           # the option
        assert fused_grid_raw(plan, 1000, 8, 0, 0, tt, 1)["fused"] == 0             # no REST list
        g = fused_grid_raw(plan, 0, 8, 52, 32, tt, 1)                               # no MAIN list: fused, main_grid = 0
        assert g["fused"] == 1 and g["main_grid"] == 0 and g["total"] == 52 * 32
        check_map(plan, g)
        # the sum of the grids against MAX_GRID, each of them a legal launch on its own
        assert fused_grid_raw(plan, big - 1664, 1, 52, 32, tt, 1)["fused"] == 1
        assert fused_grid_raw(plan, big - 1663, 1, 52, 32, tt, 1)["fused"] == 0
        assert fused_grid_raw(plan, big // 8, 8, 52, 32, tt, 1)["fused"] == 0
        g = fused_grid_raw(plan, big - 1664, 1, 52, 32, tt, 1)
        assert g["total"] == big
        check_map(plan, g)
    for tt in range(1, k["rest_tt"] + 1):  # TT <= CELL_REST_TT: the kernel has no second body
        assert fused_grid_raw(plan, 1000, 8, 52, 32, tt, 1)["fused"] == 0
        assert fused_grid_raw(plan, 0, 8, 52, 32, tt, 1)["fused"] == 0


def headline_keys(n=1_000_000, D=3):
    """Sorted cell keys of the benchmark's config 2 (bench.py: RandomState(n + D).rand(n, D), float32) on the grid of
    cell_make_grid(): the bounding box in the fewest equal cells of side <= sqrt(2 CELL_T_MAX / D), 10 bits per axis."""
    y = np.random.RandomState(n + D).rand(n, D).astype(np.float32)
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


def test_headline_shape(plan):
    k = constants(plan)
    keys, cells = headline_keys()
    assert cells == [10, 10, 10]
    tiles = tiles_per_cell(keys, k["cell_tile"])
    assert len(tiles) == 1000
    assert [int(np.count_nonzero(tiles == t)) for t in range(29, 36)] == [6, 88, 294, 407, 174, 29, 2]
    assert tiles.min() == 29 and tiles.max() == 35
    n_main, n_rest = list_sizes(plan, keys, 8)
    assert (n_main, n_rest) == (32000, 416)
    g = fused_grid(plan, len(keys), int(tiles.sum()), n_main, n_rest, 8, -1)
    assert (g["blocks0"], g["segments0"], g["blocks1"], g["segments1"]) == (1000, 8, 52, 32)
    assert g["fused"] == 1 and (g["main_grid"], g["rest_grid"], g["total"]) == (8000, 1664, 9664)
    # main_grid is a multiple of 8: a REST workgroup keeps the index modulo 8 (the XCD) it had in a launch of its own
    assert g["main_grid"] % 8 == 0
    lst, loc = work(plan, 0, g["total"], g["main_grid"])
    bid = np.arange(g["total"])
    assert np.array_equal(loc[lst == 1] & 7, bid[lst == 1] & 7)
    check_map(plan, g)
    assert fused_grid(plan, len(keys), int(tiles.sum()), n_main, n_rest, 8, 0)["fused"] == 0
