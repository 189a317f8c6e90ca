"""The cell list and launch plan of the cutoff-radius entries (csrc/kmvp_cutoff_plan.hpp; include/kmvp.h
kmvp_<kernel>_cutoff, kmvp_radius_count) without a GPU: the header is plain C++, compiled here with the host compiler
behind tests/host_cutoff_plan_shim.cpp and held to the numpy restatement (cutoff_reference.plan) entry by entry and,
property by property, to what the kernels rely on: lowd_cutoff_kernel indexes the tables without a bounds check, and its
result is right only if a tile's runs are disjoint and hold every source that can be inside."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import cutoff_reference as cr

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "kernel_matrix_benchmarks_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    tmp = tempfile.mkdtemp(prefix="kmvp_host_cutoff_plan_")
    so = os.path.join(tmp, "libhost_cutoff_plan.so")
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC,
                           os.path.join(HERE, "host_cutoff_plan_shim.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.hc_records.restype = ctypes.c_long
    lib.hc_max_axis.restype = ctypes.c_long
    lib.hc_build.restype = ctypes.c_void_p
    lib.hc_build.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_double,
                             ctypes.c_double]
    lib.hc_free.restype = None
    lib.hc_free.argtypes = [ctypes.c_void_p]
    for fn, n in ((lib.hc_sizes, 3), (lib.hc_tables, 3), (lib.hc_maps, 3)):
        fn.restype = None
        fn.argtypes = [ctypes.c_void_p] * n
    yield lib
    shutil.rmtree(tmp, ignore_errors=True)


def build(lib, y, x, R, factor=1.0):
    """The header's plan as cutoff_reference.plan's dict."""
    y = np.ascontiguousarray(y, dtype=np.float64)
    x = y if x is None else np.ascontiguousarray(x, dtype=np.float64)
    h = lib.hc_build(y.ctypes.data, len(y), x.ctypes.data, len(x), y.shape[1], float(R), float(factor))
    assert h
    try:
        sizes, grid = np.zeros(12, dtype=np.int64), np.zeros(4)
        lib.hc_sizes(h, sizes.ctypes.data, grid.ctypes.data)
        tiles, runs = np.zeros((int(sizes[8]), 3), dtype=np.int64), np.zeros((int(sizes[9]), 2), dtype=np.int64)
        tmap, smap = np.full(int(sizes[10]), -7, dtype=np.int64), np.full(int(sizes[11]), -7, dtype=np.int64)
        lib.hc_tables(h, tiles.ctypes.data, runs.ctypes.data)
        lib.hc_maps(h, tmap.ctypes.data, smap.ctypes.data)
    finally:
        lib.hc_free(h)
    return dict(g=sizes[:3].copy(), lo=grid[:3].copy(), h=float(grid[3]), n_pad=int(sizes[3]), m_pad=int(sizes[4]),
                m_alloc=int(sizes[5]), live_tiles=int(sizes[6]), walked=int(sizes[7]), tiles=tiles, runs=runs, tmap=tmap, smap=smap)


def check_properties(p, y, x, R, factor):
    """What the kernels rely on, from the plan alone (and the points it was built for)."""
    y = np.asarray(y, dtype=np.float64)
    x = y if x is None else np.asarray(x, dtype=np.float64)
    (M, D), N = y.shape, len(x)
    tiles, runs, tmap, smap = p["tiles"], p["runs"], p["tmap"], p["smap"]
    g = p["g"]
    # the grid: at least the asked side with its margin, within the caps
    assert p["h"] >= factor * R * (1 + 2.0 ** -16) and np.all(g >= 1) and np.all(g <= cr.MAX_AXIS) and np.all(g[D:] == 1)
    assert int(g[0]) * int(g[1]) * int(g[2]) <= max(1, 2 * (N + M))
    # tiles are whole workgroups, the maps cover them, the spare batch exists
    assert len(tiles) % cr.WAVES == 0 and p["n_pad"] == len(tiles) * cr.TILE == len(tmap)
    assert p["m_alloc"] == p["m_pad"] + cr.RECORDS == len(smap) and p["m_pad"] % cr.RECORDS == 0
    assert np.all(smap[p["m_pad"]:] == -1)
    # every source with finite coordinates is in exactly one record; the others are in none
    fy, fx = np.isfinite(y).all(axis=1), np.isfinite(x).all(axis=1)
    live_rec = smap[smap >= 0]
    assert np.array_equal(np.sort(live_rec), np.nonzero(fy)[0])
    pos = np.full(M, -1, dtype=np.int64)
    pos[live_rec] = np.nonzero(smap >= 0)[0]
    # every run: a positive multiple of 8 that starts on a multiple of 8, every read of the pair loop inside the array
    # (the first prefetch of 4 records and, per round of 8, the records up to 4 behind the run)
    rec0, length = runs[:, 0], runs[:, 1]
    assert np.all(rec0 % cr.RECORDS == 0) and np.all(length % cr.RECORDS == 0) and np.all(length > 0) and np.all(rec0 >= 0)
    assert np.all(rec0 + length + cr.RECORDS // 2 <= p["m_alloc"]) and np.all(rec0 + length <= p["m_pad"])
    cell = np.zeros(N, dtype=np.int64)      # the row of cells of every finite target, from the plan's own grid
    for d in range(D - 1, 0, -1):
        cell = cell * g[d] + cr._cells(np.where(fx, x[:, d], p["lo"][d]), p["lo"][d], p["h"], g[d])
    seen = np.zeros(N, dtype=np.int64)
    s = cr.sqdists(x, y)
    with np.errstate(invalid="ignore"):
        reach = s <= (R * (1 + 2.0 ** -17)) ** 2
    walked, used = 0, 0
    for t, (run0, nruns, live) in enumerate(tiles):
        slots = tmap[t * cr.TILE:(t + 1) * cr.TILE]
        assert 0 <= live <= cr.TILE and np.all(slots[live:] == -1) and np.all(slots[:live] >= 0)
        assert 0 <= nruns <= 3 ** (D - 1) and 0 <= run0 and run0 + nruns <= len(runs)
        if live == 0:
            assert nruns == 0
            continue
        i = slots[:live]
        seen[i] += 1
        if not fx[i].all():            # targets with a non-finite coordinate sit in tiles of their own that own no run
            assert not fx[i].any() and nruns == 0
            continue
        assert len(np.unique(cell[i])) == 1                   # no tile straddles a row of cells
        mine = runs[run0:run0 + nruns]
        order = np.argsort(mine[:, 0])
        assert np.all(mine[order][:-1, 0] + mine[order][:-1, 1] <= mine[order][1:, 0])      # pairwise disjoint
        walked += live * int(mine[:, 1].sum())
        used += nruns
        # covering: every source within R (1 + 2^-17) of any of the tile's targets lies in exactly one of its runs
        need = np.nonzero(reach[i].any(axis=0))[0]
        assert np.all(pos[need] >= 0)
        hits = ((pos[need, None] >= mine[None, :, 0]) & (pos[need, None] < mine[None, :, 0] + mine[None, :, 1])).sum(axis=1)
        assert np.all(hits == 1), (t, need[hits != 1][:5])
    assert np.all(seen == 1)                                  # every target in exactly one live lane
    assert walked == p["walked"] and used == len(runs)
    dead = np.nonzero(tiles[:, 2] == 0)[0]
    assert len(dead) < cr.WAVES and np.array_equal(dead, np.arange(len(tiles) - len(dead), len(tiles)))
    assert p["live_tiles"] == len(tiles) - len(dead)


def check(lib, y, x, R, factor=1.0):
    got = build(lib, y, x, R, factor)
    want = cr.plan(y, y if x is None else x, R, factor)
    for key in ("n_pad", "m_pad", "m_alloc", "live_tiles", "walked", "h"):
        assert got[key] == want[key], key
    for key in ("g", "lo", "tiles", "runs", "tmap", "smap"):
        assert np.array_equal(got[key], want[key]), key
    check_properties(got, y, x, R, factor)
    return got


def test_constants(lib):
    assert (lib.hc_tile(), lib.hc_waves(), lib.hc_records(), lib.hc_max_axis()) == (cr.TILE, cr.WAVES, cr.RECORDS, cr.MAX_AXIS)
    assert lib.hc_tile_bytes() == 16 and lib.hc_run_bytes() == 16


@pytest.mark.parametrize("factor", [1.0, 1.5, 2.0])
@pytest.mark.parametrize("D", [1, 2, 3])
def test_uniform_clouds(lib, D, factor):
    rs = np.random.RandomState(10 * D + int(2 * factor))
    R = {1: 0.01, 2: 0.07, 3: 0.15}[D]
    y, x = rs.rand(900, D), rs.rand(333, D) * 1.2 - 0.1
    p = check(lib, y, x, R, factor)
    assert p["g"][0] > 3 and p["walked"] < 0.7 * len(x) * len(y)
    check(lib, y, None, R, factor)                           # targets = sources


@pytest.mark.parametrize("D", [1, 2, 3])
def test_one_cell(lib, D):
    """R above the diameter: one cell, one run per tile, every source walked by every target."""
    rs = np.random.RandomState(D)
    y, x = rs.rand(100, D), rs.rand(70, D)
    p = check(lib, y, x, 2.0)
    assert np.all(p["g"] == 1) and np.all(p["tiles"][:p["live_tiles"], 1] == 1) and p["walked"] == 70 * 104


@pytest.mark.parametrize("D", [1, 2, 3])
def test_cell_cap(lib, D):
    """R so small that the caps engage: the cells are larger than asked for, never more than 2 (N + M) of them and never
    more than 2^20 along an axis."""
    rs = np.random.RandomState(20 + D)
    y, x = rs.rand(150, D), rs.rand(40, D)
    for R in (1e-5, 1e-9, 1e-300):
        p = check(lib, y, x, R)
        assert p["h"] > 2 * R and int(np.prod(p["g"])) <= 2 * 190
    y[0, 0] = 1e300                                          # an extent the asked side would cut into 1e300 cells
    p = check(lib, y, x, 0.1)
    assert int(np.prod(p["g"])) <= 2 * 190


def test_empty_sides(lib):
    rs = np.random.RandomState(5)
    pts = rs.rand(130, 3)
    p = check(lib, np.zeros((0, 3)), pts, 0.2)               # M = 0: no record but the spare batch, no run
    assert p["m_pad"] == 0 and p["m_alloc"] == cr.RECORDS and len(p["runs"]) == 0 and np.all(p["tiles"][:, 1] == 0)
    p = check(lib, pts, np.zeros((0, 3)), 0.2)               # N = 0: no tile at all
    assert p["n_pad"] == 0 and len(p["tiles"]) == 0
    p = check(lib, np.zeros((0, 2)), np.zeros((0, 2)), 0.2)
    assert p["n_pad"] == 0 and p["m_pad"] == 0


def test_duplicates(lib):
    """A cell that holds more than a tile of coincident targets, and sources on top of each other."""
    rs = np.random.RandomState(6)
    base = rs.rand(40, 2)
    y = np.concatenate([base, base, np.repeat(base[:1], 200, axis=0)])
    p = check(lib, y, None, 0.05)
    assert p["live_tiles"] >= 5
    check(lib, y, rs.rand(10, 2), 0.05, 1.5)


def test_non_finite_points(lib):
    rs = np.random.RandomState(7)
    y, x = rs.rand(300, 3), rs.rand(200, 3)
    y[[3, 77], [0, 2]] = [np.nan, np.inf]
    y[150] = -np.inf
    x[[5, 9, 150], [1, 0, 2]] = [np.nan, -np.inf, np.inf]
    x[[10]] = np.nan
    p = check(lib, y, x, 0.2)
    loose = p["tiles"][p["live_tiles"] - 1]
    assert loose[1] == 0 and loose[2] == 4                   # the four targets set aside, in a tile without runs
    assert set(p["tmap"][(p["live_tiles"] - 1) * cr.TILE:][:4]) == {5, 9, 10, 150}
    y[:] = np.nan                                            # nothing finite on the source side
    p = check(lib, y, x, 0.2)
    assert p["m_pad"] == 0 and len(p["runs"]) == 0


@pytest.mark.parametrize("precision", (np.float32, np.float64), ids=lambda p: np.dtype(p).name)
@pytest.mark.parametrize("name", cr.CLOUDS + ("lattice",))
def test_gpu_test_clouds(lib, name, precision):
    """The clouds tests/test_gpu_cutoff.py runs, at the factors it runs them; what the issue says about their shape."""
    y, x, R = cr.cloud(name, precision)
    if name != "lattice":
        assert cr.boundary_clear(y, x, R, precision)
    for factor in (1.0, 1.5, 2.0):
        p = check(lib, y, x, R, factor)
        if name == "C" and factor == 1.0:
            assert np.all(p["g"][1:] == 1) and list(p["tiles"][:p["live_tiles"], 2]) == [64, 64, 2]
    _, cnt = cr.dense("gaussian", y, y if x is None else x, None, R)
    if name == "A" and np.dtype(precision) == np.float32:
        assert (cnt.min(), cnt.max()) == (6, 54)
    if name == "B":
        assert int((cnt == 0).sum()) == 66
    if name == "K":
        p = check(lib, y, x, R)
        tcell = np.zeros(len(y), dtype=np.int64)
        for d in (2, 1, 0):
            tcell = tcell * p["g"][d] + cr._cells(y[:, d], p["lo"][d], p["h"], p["g"][d])
        assert np.bincount(tcell).max() > 64 and (cnt.min(), cnt.max()) == (1, 150)
