"""The layout and launch plan of the batched clouds (csrc/kmvp_batch_plan.hpp; include/kmvp.h kmvp_set_batches) without a
GPU: the header is plain C++, compiled here with the host compiler behind tests/host_batch_plan_shim.cpp and held to the
Python restatement (batch_reference.plan) and, property by property, to what the kernels rely on: the tile table is what
lowd_batch_kernel indexes without a bounds check."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import batch_reference as br

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "kernel_matrix_benchmarks_amd", "csrc")
P64 = ctypes.POINTER(ctypes.c_int64)


@pytest.fixture(scope="module")
def lib():
    tmp = tempfile.mkdtemp(prefix="kmvp_host_batch_plan_")
    so = os.path.join(tmp, "libhost_batch_plan.so")
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC,
                           os.path.join(HERE, "host_batch_plan_shim.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.hb_records.restype = ctypes.c_long
    lib.hb_max_range.restype = ctypes.c_long
    lib.hb_check.restype = ctypes.c_int
    lib.hb_check.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_long]
    lib.hb_build.restype = ctypes.c_void_p
    lib.hb_build.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.hb_free.restype = None
    lib.hb_free.argtypes = [ctypes.c_void_p]
    for fn, n in ((lib.hb_sizes, 2), (lib.hb_tiles, 2), (lib.hb_maps, 3)):
        fn.restype = None
        fn.argtypes = [ctypes.c_void_p] * n
    yield lib
    shutil.rmtree(tmp, ignore_errors=True)


def build(lib, y_off, x_off):
    """The header's plan as batch_reference.plan's dict, or None where it refuses."""
    y_off, x_off = np.ascontiguousarray(y_off, dtype=np.int64), np.ascontiguousarray(x_off, dtype=np.int64)
    assert len(y_off) == len(x_off)
    h = lib.hb_build(len(y_off) - 1, y_off.ctypes.data, x_off.ctypes.data)
    if not h:
        return None
    try:
        sizes = np.zeros(6, dtype=np.int64)
        lib.hb_sizes(h, sizes.ctypes.data)
        tiles = np.zeros((int(sizes[3]), 5), dtype=np.int64)
        tmap, smap = np.full(int(sizes[4]), -7, dtype=np.int64), np.full(int(sizes[5]), -7, dtype=np.int64)
        lib.hb_tiles(h, tiles.ctypes.data)
        lib.hb_maps(h, tmap.ctypes.data, smap.ctypes.data)
    finally:
        lib.hb_free(h)
    return dict(n_pad=int(sizes[0]), m_pad=int(sizes[1]), m_alloc=int(sizes[2]), tiles=tiles, tmap=tmap, smap=smap)


def check_properties(p, y_off, x_off):
    """What the kernels rely on, from the plan alone."""
    y_off, x_off = np.asarray(y_off, dtype=np.int64), np.asarray(x_off, dtype=np.int64)
    B, N, M = len(y_off) - 1, int(x_off[-1]), int(y_off[-1])
    tiles, tmap, smap = p["tiles"], p["tmap"], p["smap"]
    rec0, j0, i0, length, live = tiles.T
    # the totals are whole workgroups, the maps cover them, and the spare batch exists
    assert len(tiles) % br.WAVES == 0 and p["n_pad"] == len(tiles) * br.TILE == len(tmap)
    assert p["m_alloc"] == p["m_pad"] + br.RECORDS == len(smap) and p["m_pad"] % br.RECORDS == 0
    assert np.all(smap[p["m_pad"]:] == -1)
    # every batch's padded range: a multiple of 8 that starts where the previous batch's ended
    starts = np.concatenate([[0], np.cumsum(-(-np.diff(y_off) // br.RECORDS) * br.RECORDS)])
    assert starts[-1] == p["m_pad"]
    for b in range(B):
        m = int(y_off[b + 1] - y_off[b])
        seg = smap[starts[b]:starts[b + 1]]
        assert np.array_equal(seg[:m], np.arange(y_off[b], y_off[b + 1])) and np.all(seg[m:] == -1)   # pads map to -1
    # every caller index appears exactly once among the live lanes, and no tile mixes batches
    owner = np.searchsorted(x_off, np.arange(N), side="right") - 1     # batch of every target (empty batches skipped)
    seen = np.zeros(N, dtype=np.int64)
    for t in range(len(tiles)):
        slots = tmap[t * br.TILE:(t + 1) * br.TILE]
        assert 0 <= live[t] <= br.TILE and np.all(slots[live[t]:] == -1)
        assert length[t] % br.RECORDS == 0 and 0 <= length[t] <= 2 ** 31 - 8
        # every read of the pair loop stays inside the record array: the first prefetch of 4 records and, per round of
        # 8, the records up to 4 behind the range
        assert 0 <= rec0[t] and rec0[t] + max(length[t], 0) + br.RECORDS // 2 <= p["m_alloc"]
        if live[t] == 0:       # filler tiles have empty ranges and no live lane
            assert length[t] == 0
            continue
        assert np.array_equal(slots[:live[t]], i0[t] + np.arange(live[t]))
        seen[slots[:live[t]]] += 1
        b = owner[i0[t]]
        assert np.all(owner[slots[:live[t]]] == b)
        assert rec0[t] == starts[b] and length[t] == starts[b + 1] - starts[b] and j0[t] == y_off[b]
        # the tile's records are its batch's sources, in the caller's order
        m = int(y_off[b + 1] - y_off[b])
        assert np.array_equal(smap[rec0[t]:rec0[t] + m], j0[t] + np.arange(m))
    assert np.all(seen == 1)
    # filler tiles only at the end, fewer than a workgroup of them
    dead = np.nonzero(live == 0)[0]
    assert len(dead) < br.WAVES and np.array_equal(dead, np.arange(len(tiles) - len(dead), len(tiles)))


def check(lib, y_sizes, x_sizes):
    y_off, x_off = br.offsets(y_sizes), br.offsets(x_sizes)
    assert lib.hb_check(len(y_sizes), y_off.ctypes.data, int(y_off[-1])) == 0
    got, want = build(lib, y_off, x_off), br.plan(y_off, x_off)
    assert got is not None
    for key in ("n_pad", "m_pad", "m_alloc"):
        assert got[key] == want[key], key
    for key in ("tiles", "tmap", "smap"):
        assert np.array_equal(got[key], want[key]), key
    check_properties(got, y_off, x_off)
    return got


def test_constants(lib):
    assert (lib.hb_tile(), lib.hb_waves(), lib.hb_records()) == (br.TILE, br.WAVES, br.RECORDS)
    assert lib.hb_tile_bytes() == 32 and lib.hb_max_range() == 2 ** 31 - 8


HAND_MADE = [
    # (source sizes, target sizes)
    ([300], [130]),                                           # B = 1
    ([1], [1]),
    ([0, 5, 0, 0, 9, 0], [0, 64, 0, 3, 65, 0]),               # empty batches at the start, the middle and the end
    ([1, 7, 8, 9, 1], [1, 63, 64, 65, 129]),                  # the sizes around a tile and around a round of records
    ([0, 0, 0], [4, 64, 200]),                                # an all-empty source side
    ([4, 64, 200], [0, 0, 0]),                                # an all-empty target side: no tile at all
    ([0, 0], [0, 0]),                                         # both
    (list(br.SOURCE_SIZES), list(br.TARGET_SIZES)),           # the GPU tests' ragged batches
    ([8] * 40, [64] * 40),                                    # B = 40, nothing to pad, whole workgroups
    ([9] * 39, [65] * 39),                                    # everything to pad, filler tiles
]


@pytest.mark.parametrize("case", range(len(HAND_MADE)))
def test_hand_made_offsets(lib, case):
    y_sizes, x_sizes = HAND_MADE[case]
    p = check(lib, y_sizes, x_sizes)
    if sum(x_sizes) == 0:
        assert p["n_pad"] == 0 and len(p["tiles"]) == 0
    if sum(y_sizes) == 0:
        assert p["m_pad"] == 0 and p["m_alloc"] == br.RECORDS and np.all(p["tiles"][:, 3] == 0)


@pytest.mark.parametrize("B", [1, 2, 3, 5, 8, 13, 21, 40])
def test_random_offsets(lib, B):
    rs = np.random.RandomState(B)
    special_n, special_m = [0, 1, 63, 64, 65, 129], [0, 1, 7, 8, 9]
    for _ in range(6):
        x_sizes = [int(rs.choice(special_n)) if rs.rand() < 0.5 else int(rs.randint(0, 300)) for _ in range(B)]
        y_sizes = [int(rs.choice(special_m)) if rs.rand() < 0.5 else int(rs.randint(0, 300)) for _ in range(B)]
        check(lib, y_sizes, x_sizes)


def test_offsets_check(lib):
    def rc(off, total):
        off = np.ascontiguousarray(off, dtype=np.int64)
        return lib.hb_check(len(off) - 1, off.ctypes.data, total)

    assert rc([0, 3, 3, 10], 10) == 0
    assert rc([1, 3, 10], 10) == 1          # does not start at 0
    assert rc([0, 5, 3, 10], 10) == 2       # not monotone
    assert rc([0, 3, 9], 10) == 3 and rc([0, 3, 11], 10) == 3   # does not end at the number of points
    assert rc([0, 0], 0) == 0


def test_range_of_two_to_the_31_is_refused(lib):
    """The pair loop counts positions within a range in 32 bits: the longest padded range is 2^31 - 8.  (No target, so
    the plan of the accepted case stays small; the refusal comes before anything is allocated.)"""
    top = 2 ** 31 - 8
    assert build(lib, [0, top + 1], [0, 0]) is None
    assert build(lib, [0, 5, 5 + top + 1], [0, 0, 0]) is None
