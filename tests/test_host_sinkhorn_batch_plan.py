"""The plan of the batched Sinkhorn solve (csrc/kmvp_sinkhorn_batch_plan.hpp; include/kmvp.h kmvp_<kernel>_sinkhorn_batched)
without a GPU: the header is plain C++, compiled here with the host compiler behind tests/host_sinkhorn_batch_plan_shim.cpp
and held, property by property, to what the solver's kernels rely on without a bounds check: every tile of both directions
maps to its batch, the tiles of a batch are contiguous and ascending, a target's record in the other direction is the
record that holds the same point, and a retired tile (len = 0, nothing else) still points inside the record array."""
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


@pytest.fixture(scope="module")
def lib():
    tmp = tempfile.mkdtemp(prefix="kmvp_host_sinkhorn_batch_plan_")
    so = os.path.join(tmp, "libhost_sinkhorn_batch_plan.so")
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC,
                           os.path.join(HERE, "host_sinkhorn_batch_plan_shim.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.hs_one_sided.restype = ctypes.c_int
    lib.hs_one_sided.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.hs_build.restype = ctypes.c_void_p
    lib.hs_build.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.hs_free.restype = None
    lib.hs_free.argtypes = [ctypes.c_void_p]
    for fn, n in ((lib.hs_sizes, 1), (lib.hs_tiles, 1), (lib.hs_maps, 4)):
        fn.restype = None
        fn.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * n
    yield lib
    shutil.rmtree(tmp, ignore_errors=True)


def build(lib, y_off, x_off):
    """Both directions as dicts: 1 = targets x / records of y, 2 = targets y / records of x."""
    h = lib.hs_build(len(y_off) - 1, y_off.ctypes.data, x_off.ctypes.data)
    assert h
    out = {}
    try:
        for d in (1, 2):
            sizes = np.zeros(6, dtype=np.int64)
            lib.hs_sizes(h, d, sizes.ctypes.data)
            tiles = np.zeros((int(sizes[3]), 6), dtype=np.int64)
            begin, other = np.full(int(sizes[4]), -7, dtype=np.int64), np.full(int(sizes[5]), -7, dtype=np.int64)
            tmap, smap = np.full(int(sizes[0]), -7, dtype=np.int64), np.full(int(sizes[2]), -7, dtype=np.int64)
            lib.hs_tiles(h, d, tiles.ctypes.data)
            lib.hs_maps(h, d, begin.ctypes.data, other.ctypes.data, tmap.ctypes.data, smap.ctypes.data)
            out[d] = dict(n_pad=int(sizes[0]), m_pad=int(sizes[1]), m_alloc=int(sizes[2]), tiles=tiles, begin=begin, other=other,
                          tmap=tmap, smap=smap)
    finally:
        lib.hs_free(h)
    return out


def check(lib, y_sizes, x_sizes):
    y_off, x_off = br.offsets(y_sizes), br.offsets(x_sizes)
    B = len(y_sizes)
    p = build(lib, y_off, x_off)
    for d, s_off, t_off in ((1, y_off, x_off), (2, x_off, y_off)):
        me, other = p[d], p[3 - d]
        # the direction's plan is the batches' plan, with the offsets swapped for direction 2
        want = br.plan(s_off, t_off)
        for key in ("n_pad", "m_pad", "m_alloc"):
            assert me[key] == want[key], (d, key)
        assert np.array_equal(me["tiles"][:, :5], want["tiles"]) and np.array_equal(me["tmap"], want["tmap"])
        assert np.array_equal(me["smap"], want["smap"])
        rec0, _, i0, length, live, batch = me["tiles"].T
        nt = len(batch)
        assert len(me["other"]) == me["n_pad"] == nt * br.TILE
        # every tile maps to its batch: the batch that owns its lanes' targets; filler tiles to none
        for t in range(nt):
            if live[t] == 0:
                assert batch[t] == -1 and length[t] == 0
                continue
            b = batch[t]
            assert 0 <= b < B and t_off[b] <= i0[t] and i0[t] + live[t] <= t_off[b + 1]
        # the tiles of a batch are contiguous and ascending, and the ranges cover the real tiles exactly once
        begin = me["begin"]
        assert len(begin) == B + 1 and begin[0] == 0 and np.all(np.diff(begin) >= 0) and begin[-1] == int(np.sum(live > 0))
        for b in range(B):
            n = int(t_off[b + 1] - t_off[b])
            assert begin[b + 1] - begin[b] == -(-n // br.TILE)
            own = np.arange(begin[b], begin[b + 1])
            assert np.all(batch[own] == b)
            assert np.array_equal(i0[own], t_off[b] + br.TILE * np.arange(len(own)))   # ascending in the caller's order
        # a target's record in the other direction holds the same point; pads have none
        live_slot = me["tmap"] >= 0
        assert np.all(me["other"][~live_slot] == -1)
        recs = me["other"][live_slot]
        assert np.all((0 <= recs) & (recs < other["m_pad"]))
        assert np.array_equal(other["smap"][recs], me["tmap"][live_slot])
        # the signal slots the finish kernels write are distinct: no two targets share a record
        assert len(np.unique(recs)) == len(recs)
        # a retired tile keeps rec0 and takes len = 0: the first prefetch of 4 records stays inside the record array, as do
        # all reads of a running tile (the batches' own rule)
        assert np.all((0 <= rec0) & (rec0 + br.RECORDS // 2 <= me["m_alloc"]))
        assert np.all(rec0 + length + br.RECORDS // 2 <= me["m_alloc"])
    return p


HAND_MADE = [
    ([300], [130]),                                           # B = 1
    ([1], [1]),
    ([0, 5, 0, 0, 9, 0], [0, 64, 0, 3, 65, 0]),               # batches that are empty on both sides: start, middle, end
    ([9, 1, 8, 200, 7], [1, 63, 64, 65, 130]),                # the GPU tests' ragged batches
    ([1, 7, 8, 9, 1], [1, 63, 64, 65, 129]),                  # the sizes around a tile and around a round of records
    ([0, 0], [0, 0]),                                         # nothing at all
    ([8] * 40, [64] * 40),                                    # nothing to pad, whole workgroups
    ([65] * 39, [9] * 39),                                    # everything to pad, filler tiles in both directions
]


@pytest.mark.parametrize("case", range(len(HAND_MADE)))
def test_hand_made_offsets(lib, case):
    y_sizes, x_sizes = HAND_MADE[case]
    p = check(lib, y_sizes, x_sizes)
    if sum(x_sizes) == 0:
        assert p[1]["n_pad"] == 0 and p[2]["n_pad"] == 0


@pytest.mark.parametrize("B", [1, 2, 3, 5, 8, 13, 21])
def test_random_offsets(lib, B):
    rs = np.random.RandomState(100 + B)
    special = [0, 1, 7, 8, 9, 63, 64, 65, 129]
    for _ in range(5):
        x_sizes = [int(rs.choice(special)) if rs.rand() < 0.5 else int(rs.randint(0, 300)) for _ in range(B)]
        y_sizes = [int(rs.choice(special)) if rs.rand() < 0.5 else int(rs.randint(0, 300)) for _ in range(B)]
        check(lib, y_sizes, x_sizes)   # (one-sided batches included: the plan itself does not mind, the entry refuses them)


def test_one_sided_batches_are_found(lib):
    def first(y_sizes, x_sizes):
        y_off, x_off = br.offsets(y_sizes), br.offsets(x_sizes)
        return lib.hs_one_sided(len(y_sizes), y_off.ctypes.data, x_off.ctypes.data)

    assert first([3, 0, 5], [2, 0, 1]) == -1
    assert first([3, 0, 5], [2, 1, 1]) == 1
    assert first([3, 4, 5], [2, 1, 0]) == 2
    assert first([0], [0]) == -1 and first([0], [1]) == 0
