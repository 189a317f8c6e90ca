"""The candidate list of the radius search (csrc/kmvp_radius_knn_list.hpp: lexicographic insertion on (s, caller's index), the
list that keeps K [+ 1] of KT entries, the end-of-row rule) without a GPU: the header is plain C++ behind a macro for the
device attributes, compiled here with the host compiler behind tests/host_radius_knn_list_shim.cpp and held to numpy's
lexsort((j, s))[:K] on candidates fed in shuffled order -- the order a cell list meets them in is not the index order."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import radius_nearest_reference as rn

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "kernel_matrix_benchmarks_amd", "csrc")
KS = (1, 2, 3, 4, 5, 8, 15, 16)


def capacity(need):
    """The smallest of the kernel's list capacities 1, 4, 16 that holds `need` entries."""
    return 1 if need <= 1 else 4 if need <= 4 else 16


@pytest.fixture(scope="module")
def lib():
    tmp = tempfile.mkdtemp(prefix="kmvp_host_radius_knn_list_")
    so = os.path.join(tmp, "libhost_radius_knn_list.so")
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC,
                           os.path.join(HERE, "host_radius_knn_list_shim.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    for name, real in (("hr_row_f32", ctypes.c_float), ("hr_row_f64", ctypes.c_double)):
        f = getattr(lib, name)
        f.restype = ctypes.c_int
        f.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, real, ctypes.c_int, ctypes.c_int, ctypes.c_long,
                      ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    yield lib
    shutil.rmtree(tmp, ignore_errors=True)


def header_row(lib, s, j, r2, K, exclude_self=False, self_index=-7, nan_row=False, precision=np.float32, KT=None):
    s, j = np.ascontiguousarray(s, dtype=precision), np.ascontiguousarray(j, dtype=np.int32)
    KT = capacity(K + bool(exclude_self)) if KT is None else KT
    idx, sq = np.full(K, -99, dtype=np.int64), np.full(K, -99.0)
    f = lib.hr_row_f64 if precision == np.float64 else lib.hr_row_f32
    assert f(KT, s.ctypes.data, j.ctypes.data, len(s), float(precision(r2)), K, int(exclude_self), self_index, int(nan_row),
             idx.ctypes.data, sq.ctypes.data) == 0
    return idx, sq


def numpy_row(s, j, r2, K, exclude_self=False, self_index=-7, precision=np.float32):
    s, j = np.asarray(s, dtype=precision), np.asarray(j)
    with np.errstate(invalid="ignore"):
        keep = np.nonzero(s <= precision(r2))[0]          # NaN and +inf candidates, and what is outside, never enter
    order = keep[np.lexsort((j[keep], s[keep]))][:K + bool(exclude_self)]
    return rn.finish(s[order].astype(np.float64), j[order], K, exclude_self, self_index)


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1], equal_nan=True)


@pytest.mark.parametrize("precision", (np.float32, np.float64), ids=("f32", "f64"))
@pytest.mark.parametrize("K", KS)
def test_shuffled_candidates_with_many_ties(lib, K, precision):
    """200 candidates on 6 distinct distances (more than 16 equal keys each), a third of them outside r2, some at +inf and
    NaN, fed in 8 shuffled orders: always lexsort's first K."""
    rs = np.random.RandomState(K)
    levels = np.array([0.0, 0.125, 0.25, 0.5, 0.75, 1.5])
    for trial in range(8):
        s = levels[rs.randint(0, 6, size=200)]
        s[rs.choice(200, 12, replace=False)] = [np.inf] * 6 + [np.nan] * 6
        j = rs.permutation(5000)[:200]
        for r2 in (0.5, 0.0, 2.0):
            assert same(header_row(lib, s, j, r2, K, precision=precision), numpy_row(s, j, r2, K, precision=precision)), (trial, r2)


@pytest.mark.parametrize("KT", (1, 4, 16))
def test_every_capacity_keeps_any_smaller_count(lib, KT):
    """A list of capacity KT asked to keep kc < KT entries returns the kc smallest -- and distinct random keys too."""
    rs = np.random.RandomState(KT)
    s, j = rs.rand(300).astype(np.float32), rs.permutation(300)
    for K in range(1, KT + 1):
        assert same(header_row(lib, s, j, 0.6, K, KT=KT), numpy_row(s, j, 0.6, K))


def test_fewer_candidates_than_k(lib):
    for K in (1, 4, 5, 16):
        for n in (0, 1, 3):
            got = header_row(lib, [0.25] * n, list(range(9, 9 - n, -1)), 1.0, K)
            want = numpy_row([0.25] * n, list(range(9, 9 - n, -1)), 1.0, K)
            assert same(got, want) and np.all(got[0][n:] == -1) and np.all(np.isposinf(got[1][n:]))
    # everything masked: a pair just outside, +inf, NaN
    got = header_row(lib, [np.nextafter(np.float32(1), np.float32(2)), np.inf, np.nan], [0, 1, 2], 1.0, 4)
    assert np.all(got[0] == -1) and np.all(np.isposinf(got[1]))
    # a pair exactly ON the boundary is inside
    assert header_row(lib, [1.0], [3], 1.0, 1)[0][0] == 3


@pytest.mark.parametrize("K", (1, 3, 4, 15))
def test_exclude_self(lib, K):
    """Own index present: dropped, the rest in order.  Absent: the last of the K + 1 dropped.  More than K + 1 candidates at
    distance 0 with indices below the own one: the K smallest indices.  Fewer than K + 1 inside: padded."""
    rs = np.random.RandomState(K)
    s, j = np.round(rs.rand(120) * 8) / 8, rs.permutation(400)[:120]
    for self_index in (int(j[5]), 399 if 399 not in j else 398, int(j[np.argmin(s)])):
        got = header_row(lib, s, j, 0.7, K, True, self_index)
        assert same(got, numpy_row(s, j, 0.7, K, True, self_index)) and self_index not in got[0]
    dup_j = rs.permutation(np.arange(40, 40 + K + 5))
    s2, j2 = np.concatenate([np.zeros(K + 5), [0.0], s]), np.concatenate([dup_j, [300], j + 1000])
    got = header_row(lib, s2, j2, 0.7, K, True, 300)
    assert np.array_equal(got[0], np.arange(40, 40 + K)) and np.all(got[1] == 0)
    got = header_row(lib, [0.0, 0.5], [7, 2], 1.0, K, True, 7)
    assert got[0][0] == 2 and np.all(got[0][1:] == -1) and got[1][0] == 0.5 and np.all(np.isposinf(got[1][1:]))


def test_nan_row(lib):
    for K, ex in ((1, False), (4, False), (5, True), (16, False)):
        idx, sq = header_row(lib, [0.1, 0.2], [3, 4], 1.0, K, ex, 3, nan_row=True)
        assert np.all(idx == -1) and np.all(np.isnan(sq))
