"""The merge step of the K-nearest-neighbour reduction (csrc/kmvp_knn_merge.hpp: S sorted candidate lists of one target
into the K smallest under (s, j), and the exclude-self drop) without a GPU: the header is plain C++ behind a macro for the
device attributes, compiled here with the host compiler behind tests/host_knn_merge_shim.cpp and held to the restatement
(knn_reference.py).  The lists are laid out as the pair-loop kernel leaves them: [list][2 KT][targets]."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import knn_reference as kn

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "kernel_matrix_benchmarks_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    tmp = tempfile.mkdtemp(prefix="kmvp_host_knn_merge_")
    so = os.path.join(tmp, "libhost_knn_merge.so")
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC,
                           os.path.join(HERE, "host_knn_merge_shim.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.hk_merge.restype = None
    lib.hk_merge.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_long, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                             ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long]
    lib.hk_drop_self.restype = None
    lib.hk_drop_self.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_long]
    yield lib
    shutil.rmtree(tmp, ignore_errors=True)


def capacity(need):
    return 1 if need <= 1 else 4 if need <= 4 else 16


def segment_lists(x, y, bounds, KT):
    """[S][2 KT][n] float64: per segment [lo, hi) of the sources, every target's KT sorted candidates with global indices,
    padded with (+inf, -1) -- what the pair loop leaves."""
    n = x.shape[0]
    lists = np.empty((len(bounds), 2 * KT, n))
    for l, (lo, hi) in enumerate(bounds):
        idx, sq = kn.nearest(x, y[lo:hi], KT, j_offset=lo)
        lists[l, :KT] = sq.T
        lists[l, KT:] = idx.T
    return lists


def merge(lib, lists, K):
    S, twoKT, n = lists.shape
    out = np.full((2 * K, n), 123.0)
    for i in range(n):
        lib.hk_merge(lists.ctypes.data + 8 * i, twoKT * n, n, S, twoKT // 2, K, out.ctypes.data + 8 * i,
                     out.ctypes.data + 8 * (K * n + i), n)
    return out[K:].T.astype(np.int64), np.ascontiguousarray(out[:K].T)


def split(M, S):
    """S contiguous segments of 0 .. M, uneven, some possibly empty."""
    cuts = np.sort(np.random.RandomState(M + S).randint(0, M + 1, size=S - 1)) if S > 1 else np.zeros(0, dtype=int)
    edges = [0] + [int(c) for c in cuts] + [M]
    return list(zip(edges[:-1], edges[1:]))


@pytest.mark.parametrize("K", [1, 4, 5, 16])
@pytest.mark.parametrize("S", [1, 3, 8])
def test_merge_equals_the_restatement(lib, S, K):
    """Lattice clouds (equal distances within and across the lists by the dozen), M = 40 sources in S uneven segments --
    with S = 8 and K = 16 most lists are padded -- and M = 3 (every list mostly pads, fewer than K candidates in all)."""
    assert K <= lib.hk_max_k()
    rs = np.random.RandomState(100 * S + K)
    for M in (40, 3):
        x, y = kn.lattice(rs, 11, 2), kn.lattice(rs, M, 2)
        lists = segment_lists(x, y, split(M, S), capacity(K))
        idx, sq = merge(lib, lists, K)
        want_idx, want_sq = kn.nearest(x, y, K)
        assert np.array_equal(idx, want_idx) and np.array_equal(sq, want_sq)


@pytest.mark.parametrize("S", [1, 3, 8])
def test_every_list_empty(lib, S):
    lists = np.empty((S, 8, 5))
    lists[:, :4] = np.inf
    lists[:, 4:] = -1.0
    idx, sq = merge(lib, lists, 3)
    assert np.all(idx == -1) and np.all(np.isposinf(sq))


def test_nan_target_row(lib):
    """A NaN target leaves (NaN, -1) lists in every segment: the merged row is (-1, NaN) in all K entries, its neighbours
    are untouched."""
    rs = np.random.RandomState(7)
    x, y = kn.lattice(rs, 6, 3), kn.lattice(rs, 20, 3)
    x[2, 0] = np.nan
    lists = segment_lists(x, y, split(20, 3), 4)
    idx, sq = merge(lib, lists, 4)
    want_idx, want_sq = kn.nearest(x, y, 4)
    assert np.array_equal(idx, want_idx) and np.array_equal(sq, want_sq, equal_nan=True)
    assert np.all(idx[2] == -1) and np.all(np.isnan(sq[2]))


def drop_self(lib, idx, sq):
    """knn_drop_self over every row of K + 1 sorted candidates, in the kernel's [2 (K + 1)][n] layout."""
    n, K1 = idx.shape
    s = np.ascontiguousarray(sq.T)
    j = np.ascontiguousarray(idx.T.astype(np.float64))
    for i in range(n):
        lib.hk_drop_self(s.ctypes.data + 8 * i, j.ctypes.data + 8 * i, n, K1, i)
    return j[: K1 - 1].T.astype(np.int64), np.ascontiguousarray(s[: K1 - 1].T)


@pytest.mark.parametrize("K", [1, 4, 15])
def test_exclude_self(lib, K):
    """Same points on a lattice with one point repeated 20 times: rows whose own index is among the K + 1 candidates (it is
    dropped), rows of the later duplicates, where K + 1 earlier duplicates precede it (the last candidate is dropped),
    and -- M = 3 -- fewer than K + 1 candidates altogether."""
    rs = np.random.RandomState(K)
    x = kn.lattice(rs, 40, 2)
    x[10:30] = x[10]
    for pts in (x, x[:3]):
        idx, sq = drop_self(lib, *kn.nearest(pts, pts, K + 1))
        want_idx, want_sq = kn.nearest(pts, pts, K, exclude_self=True)
        assert np.array_equal(idx, want_idx) and np.array_equal(sq, want_sq)
        assert not np.any(idx == np.arange(len(pts))[:, None])
    present = (kn.nearest(x, x, K + 1)[0] == np.arange(40)[:, None]).any(axis=1)
    assert present.any() and not present.all()  # both branches of the rule were taken
