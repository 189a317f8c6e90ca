"""Count-cut cells (csrc/kmvp_plan.hpp: count_cut_cells, count_cell_source_tiles, count_cell_target_tiles), without a GPU:
the header is plain C++, compiled here with the host compiler behind tests/host_cell_balance_shim.cpp.

Under the option ``cell_balance`` the lattice is kept in x and y and every (x, y) column is cut along z by point count.
The cell kernels index the tile lists without a bounds check and take a cell's centre on trust, so on every cloud:

* every point is in exactly one cell, no cell holds more than `full` points, every cell's bucket range is within the cap
  and holds its points' buckets, and every point is within half the range's width of the centre (to a float32 ulp);
* a cell is short only where the cap stopped it or its column ends, and a cell the cap stopped with at least `quantum`
  points holds a multiple of `quantum`;
* cells and lists are the same in two runs;
* the source tiles cover the sorted order exactly once, in cell order, without an empty tile; the target tiles of both
  lists cover it exactly once, a wavefront's tiles are of one cell, empty tiles repeat the preceding key, both lists are
  whole workgroups, and the cells whose MAIN tiles fill whole workgroups stand first in the MAIN list.

On the benchmark's points the lists are pinned, with the MFMA count of a launch, 2 m_tiles (n_main + n_rest), at most
0.965 of the lattice's 2 058 416 000 and at least 85 % of the MAIN workgroups one-cell.
"""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from cell_balance_cases import fine_keys, headline_points, small_clouds

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "kernel_matrix_benchmarks_amd", "csrc")
i64, i32, f32, vp = ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_void_p
P64 = ctypes.POINTER(i64)
TT = 8
LATTICE_MFMAS = 2_058_416_000  # 2 * 31750 * (32000 + 416): tests/test_host_fused_grid.py::test_headline_shape


@pytest.fixture(scope="module")
def plan():
    tmp = tempfile.mkdtemp(prefix="kmvp_host_balance_")
    so = os.path.join(tmp, "libhost_balance.so")
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC,
                           os.path.join(HERE, "host_cell_balance_shim.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.hb_constants.argtypes = [P64]
    lib.hb_cut.argtypes = [vp, i64, i32, i64, i64]
    lib.hb_cut.restype = i64
    lib.hb_cells.argtypes = [vp] * 5
    lib.hb_zcentre.argtypes = [ctypes.c_double, ctypes.c_double, i32, i32]
    lib.hb_zcentre.restype = f32
    lib.hb_source_tiles.restype = i64
    lib.hb_source_list.argtypes = [vp] * 3
    lib.hb_target_tiles.argtypes = [i32, P64, P64]
    lib.hb_target_list.argtypes = [vp] * 3
    lib.hb_one_cell_blocks.argtypes = [vp, i64, i32]
    lib.hb_one_cell_blocks.restype = i64
    lib.hb_applies.argtypes = [i32] * 4
    lib.hb_taken.argtypes = [i32, i32, i64, i64]
    yield lib
    shutil.rmtree(tmp, ignore_errors=True)


def constants(plan):
    out = (i64 * 7)()
    plan.hb_constants(out)
    return dict(zip(("zq_bits", "zq", "min_cap", "cell_tile", "waves", "rest_tt", "shared_tt"), out))


def cut(plan, fine, cap, quantum, full, tt=TT):
    """cells and lists of sorted fine keys, as arrays"""
    fine = np.ascontiguousarray(fine, np.uint32)
    n = plan.hb_cut(fine.ctypes.data, len(fine), cap, quantum, full)
    first, count = np.zeros(n, np.int64), np.zeros(n, np.int64)
    zlo, zhi, column = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint32)
    plan.hb_cells(first.ctypes.data, count.ctypes.data, zlo.ctypes.data, zhi.ctypes.data, column.ctypes.data)

    def tiles(size, fetch):
        s, c, k = np.zeros(size, np.int32), np.zeros(size, np.int32), np.zeros(size, np.uint32)
        fetch(s.ctypes.data, c.ctypes.data, k.ctypes.data)
        return s, c, k

    m_tiles = plan.hb_source_tiles()
    sources = tiles(m_tiles, plan.hb_source_list)
    nm, nr = i64(), i64()
    plan.hb_target_tiles(tt, ctypes.byref(nm), ctypes.byref(nr))
    targets = tiles(nm.value + nr.value, plan.hb_target_list)
    return dict(first=first, count=count, zlo=zlo, zhi=zhi, column=column, sources=sources, targets=targets,
                n_main=nm.value, n_rest=nr.value, m_tiles=m_tiles)


def same(a, b):
    return all(np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else
               (all(np.array_equal(u, v) for u, v in zip(a[k], b[k])) if isinstance(a[k], tuple) else a[k] == b[k]) for k in a)


def covered_once(start, count, n):
    """do the tiles [start, start + count) cover 0 .. n - 1 exactly once?"""
    live = count > 0
    hits = np.zeros(n + 1, np.int64)
    np.add.at(hits, start[live], 1)
    np.add.at(hits, start[live] + count[live], -1)
    return bool(np.all(np.cumsum(hits)[:n] == 1)) and int(count.sum()) == n


def check_cloud(plan, keyed, quantum, full, tt=TT):
    k = constants(plan)
    fine, z, cap = keyed["fine"], keyed["z"], keyed["cap"]
    n = len(fine)
    zq = (fine & np.uint32(k["zq"] - 1)).astype(np.int64)
    col = fine >> np.uint32(k["zq_bits"])
    r = cut(plan, fine, cap, quantum, full, tt)
    assert same(r, cut(plan, fine, cap, quantum, full, tt)), "two runs differ"
    first, count, zlo, zhi = r["first"], r["count"], r["zlo"].astype(np.int64), r["zhi"].astype(np.int64)
    cells = len(first)
    assert cells < 1 << 30
    # every point in exactly one cell, none above `full`, ranges within the cap
    assert first[0] == 0 and np.array_equal(first[1:], first[:-1] + count[:-1]) and first[-1] + count[-1] == n
    assert count.min() >= 1 and count.max() <= full
    assert np.all(zhi - zlo + 1 <= cap) and np.all(zlo <= zhi)
    cell_of = np.repeat(np.arange(cells), count)
    assert np.all(zq >= zlo[cell_of]) and np.all(zq <= zhi[cell_of]) and np.array_equal(col, r["column"][cell_of])
    # |z - centre| <= half the range's width, to an ulp of the coordinates
    centre = np.array([plan.hb_zcentre(float(keyed["lo_z"]), keyed["bucket"], int(a), int(b)) for a, b in zip(zlo, zhi)], np.float32)
    half = 0.5 * (zhi - zlo + 1) * keyed["bucket"]
    ulp = float(np.spacing(np.float32(np.abs(z).max())))
    excess = np.abs(z.astype(np.float64) - centre[cell_of].astype(np.float64)) - half[cell_of]
    print("max |z - centre| - half width, in ulps:", excess.max() / ulp)
    assert excess.max() <= ulp
    # short cells: the column ends, or the cap stopped them -- then cut back to a multiple of `quantum`
    end = first + count
    for c in np.flatnonzero(count < full):
        if end[c] == n or col[end[c]] != col[first[c]]:
            continue
        e = first[c] + 1
        while e < n and e - first[c] < full and col[e] == col[first[c]] and zq[e] - zlo[c] < cap:
            e += 1
        got = e - first[c]
        assert got < full and e < n and col[e] == col[first[c]], c  # it was the cap
        assert count[c] == (got if got < quantum else got // quantum * quantum), (c, got, count[c])
    # source tiles: cell order, no empty tile, none straddles a cell, the sorted order exactly once
    s_start, s_count, s_key = r["sources"]
    assert np.all(s_count >= 1) and np.all(s_count <= k["cell_tile"]) and np.all(np.diff(s_key.astype(np.int64)) >= 0)
    assert np.array_equal(s_start[1:], s_start[:-1] + s_count[:-1]) and s_start[0] == 0 and covered_once(s_start, s_count, n)
    assert np.all(s_start >= first[s_key]) and np.all(s_start + s_count <= end[s_key])
    assert r["m_tiles"] == int(((count + k["cell_tile"] - 1) // k["cell_tile"]).sum())
    # target tiles: both lists whole workgroups, a wavefront's tiles of one cell, empty tiles repeat the preceding key
    t_start, t_count, t_key = r["targets"]
    nm, nr = r["n_main"], r["n_rest"]
    assert nm % (tt * k["waves"]) == 0 and nr % (k["rest_tt"] * k["waves"]) == 0 and len(t_key) == nm + nr
    assert covered_once(t_start, t_count, n) and np.all(t_count <= k["cell_tile"]) and np.all(t_key < cells)
    live = t_count > 0
    assert np.all(t_start[live] >= first[t_key[live]]) and np.all(t_start[live] + t_count[live] <= end[t_key[live]])
    assert np.all(t_start >= 0) and np.all(t_start < n)  # (an empty tile's start is read, never its points)
    for lo, hi, group in ((0, nm, tt), (nm, nm + nr, k["rest_tt"])):
        if hi > lo:
            keys = t_key[lo:hi]
            assert np.all(keys.reshape(-1, group) == keys[::group, None]), "a wavefront with tiles of two cells"
            assert t_count[lo] > 0
            empty = np.flatnonzero(t_count[lo:hi] == 0)
            assert np.all(keys[empty] == keys[empty - 1])
    # the MAIN list: cells of whole workgroups first, the others behind them, each class in cell order
    tiles = (count + k["cell_tile"] - 1) // k["cell_tile"]
    rem = tiles % tt
    to_rest = (tt > k["rest_tt"]) & (rem > 0) & (rem <= tt // 2)  # split_cell_tiles
    m = np.where(to_rest, tiles - rem, (tiles + tt - 1) // tt * tt)
    whole = (m > 0) & (m % (tt * k["waves"]) == 0)
    want = np.r_[np.repeat(np.flatnonzero(whole), m[whole]), np.repeat(np.flatnonzero(~whole), m[~whole])]
    assert np.array_equal(t_key[:len(want)], want) and np.all(t_count[len(want):nm] == 0)
    r["one_cell"] = plan.hb_one_cell_blocks(np.ascontiguousarray(t_key[:nm]).ctypes.data, nm, tt)
    assert r["one_cell"] >= int(m[whole].sum()) // (tt * k["waves"])
    return r


@pytest.mark.parametrize("name", ["uniform", "sheet", "copies", "tall"])
def test_small_clouds(plan, name):
    keyed = fine_keys(small_clouds()[name])
    assert keyed["cap"] >= constants(plan)["min_cap"]
    r = check_cloud(plan, keyed, 32 * TT, 32 * TT * 4)
    full = int(np.count_nonzero(r["count"] == 1024))
    print(name, "cells", len(r["count"]), "full", full, "cap", keyed["cap"], "lists", r["m_tiles"], r["n_main"], r["n_rest"])
    if name == "uniform":  # four columns of ~10 cells, all full but each column's last
        assert keyed["g"][:2] == [2, 2] and len(r["count"]) == 40 and full == 36
    if name == "copies":  # one bucket holds more than a whole cell: two cells of one range and one centre
        twin = (r["zlo"][1:] == r["zlo"][:-1]) & (r["zhi"][1:] == r["zhi"][:-1]) & (r["column"][1:] == r["column"][:-1])
        assert twin.any() and np.all(r["zlo"][1:][twin] == r["zhi"][1:][twin])
    if name == "tall":  # the cap binds everywhere: no full cell, and most cells are cut back to one wavefront's targets
        assert full == 0
        end = r["first"] + r["count"]
        col = keyed["fine"] >> np.uint32(12)
        last = np.array([e == len(col) or col[e] != col[e - 1] for e in end])
        inner = r["count"][~last]
        assert np.all((inner < 32 * TT) | (inner % (32 * TT) == 0)) and np.count_nonzero(inner == 32 * TT) > 0.8 * len(inner)
    # a cloud that is only a source is cut to whole tiles, and at four tiles per wavefront the lists hold as well
    check_cloud(plan, keyed, 32, 32 * TT * 4)
    check_cloud(plan, keyed, 32 * 4, 32 * 4 * 4, tt=4)


def test_where_it_applies(plan):
    k = constants(plan)
    assert k["shared_tt"] == TT
    for D in (1, 2, 3):
        for f in (0, 1):
            for tt in (1, 2, 4, 8):
                for cap in (0, k["min_cap"] - 1, k["min_cap"], 4096):
                    assert plan.hb_applies(D, f, tt, cap) == int(D == 3 and f == 1 and tt == 8 and cap >= k["min_cap"])
    for applies in (0, 1):
        for N, M in ((40000, 40000), (500000, 99999), (499999, 100000), (500000, 100000), (1000000, 1000000)):
            assert plan.hb_taken(0, applies, N, M) == 0
            assert plan.hb_taken(1, applies, N, M) == applies
            assert plan.hb_taken(-1, applies, N, M) == int(applies and N >= 500000 and M >= 100000)


def test_headline_shape(plan):
    """the benchmark's config 2: 1e6 uniform points, lattice 10 x 10 in x and y"""
    keyed = fine_keys(headline_points())
    assert keyed["g"] == [10, 10, 10] and keyed["cap"] == 448  # floor(0.1095 / (1 / 4096))
    r = check_cloud(plan, keyed, 32 * TT, 32 * TT * 4)
    mfmas = 2 * r["m_tiles"] * (r["n_main"] + r["n_rest"])
    blocks = r["n_main"] // (TT * 4)
    full = int(np.count_nonzero(r["count"] == 1024))
    print("cells", len(r["count"]), "full", full, "m_tiles", r["m_tiles"], "n_main", r["n_main"], "n_rest", r["n_rest"],
          "mfmas", mfmas, mfmas / LATTICE_MFMAS, "one-cell", r["one_cell"], "of", blocks)
    assert mfmas <= 0.965 * LATTICE_MFMAS
    assert r["one_cell"] >= 0.85 * blocks
    assert (len(r["count"]), full, r["m_tiles"], r["n_main"], r["n_rest"], r["one_cell"], blocks) == PINNED


PINNED = (1006, 890, 31298, 31296, 136, 913, 978)  # cells, full cells, m_tiles, n_main, n_rest, one-cell workgroups, MAIN workgroups
