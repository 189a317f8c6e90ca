"""The per-cluster arithmetic and the verdict of one Lloyd iteration (csrc/kmvp_kmeans_step.hpp: new centroid, empty rule,
shift term, stop word) without a GPU: the header is plain C++ behind a macro for the device attributes, compiled here with
the host compiler behind tests/host_kmeans_step_shim.cpp and held to the restatement (kmeans_reference.py).  The sums are
laid out as the update kernels leave them: [D + 2][C], sum w x_d in rows 0 .. D - 1, sum w in row D, sum w s in row D + 1."""
import ctypes
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import kmeans_reference as kr
import knn_reference as kn

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "kernel_matrix_benchmarks_amd", "csrc")
HEADER = os.path.join(HERE, "..", "include", "kmvp.h")


@pytest.fixture(scope="module")
def lib():
    tmp = tempfile.mkdtemp(prefix="kmvp_host_kmeans_step_")
    so = os.path.join(tmp, "libhost_kmeans_step.so")
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC,
                           os.path.join(HERE, "host_kmeans_step_shim.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.hs_code.restype = ctypes.c_int
    lib.hs_code.argtypes = [ctypes.c_int]
    lib.hs_step_cluster.restype = ctypes.c_double
    lib.hs_step_cluster.argtypes = [ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    lib.hs_verdict.restype = ctypes.c_int
    lib.hs_verdict.argtypes = [ctypes.c_double] * 5 + [ctypes.c_int]
    yield lib
    shutil.rmtree(tmp, ignore_errors=True)


def sums_of(x, w, labels, s, C):
    """[D + 2][C] float64: what the update leaves for the points with a label."""
    D = x.shape[1]
    ok = labels >= 0
    tot = np.zeros((D + 2, C))
    for d in range(D):
        tot[d] = np.bincount(labels[ok], weights=w[ok] * x[ok, d], minlength=C)
    tot[D] = np.bincount(labels[ok], weights=w[ok], minlength=C)
    tot[D + 1] = np.bincount(labels[ok], weights=w[ok] * s[ok], minlength=C)
    return tot


def header_step(lib, tot, c):
    """Every cluster through km_step_cluster: (new centroids, weights, shift, inertia)."""
    D, C = tot.shape[0] - 2, tot.shape[1]
    cent = np.array(c, dtype=np.float64, order="C")
    weight = np.full(C, -7.0)
    shift = 0.0
    for j in range(C):
        shift += lib.hs_step_cluster(tot.ctypes.data + 8 * j, C, D, cent.ctypes.data + 8 * j * D, weight.ctypes.data + 8 * j)
    return cent, weight, shift, float(np.sum(tot[D + 1]))


def one_iteration(lib, x, w, c, tol=0.0, maxit=10, iters=1):
    labels, want_c, want_w, want_inertia, want_shift, unlabelled, _ = kr.step(x, w, c, np.float64)
    s = kn.nearest(x, c, 1)[1][:, 0]
    cent, weight, shift, inertia = header_step(lib, sums_of(x, w, labels, s, len(c)), c)
    assert np.array_equal(cent, want_c) and np.array_equal(weight, want_w)  # one division per coordinate: the same bits
    assert abs(shift - want_shift) <= 1e-15 * want_shift and abs(inertia - want_inertia) <= 1e-15 * want_inertia
    got = lib.hs_verdict(float(unlabelled), inertia, shift, float(iters), tol, maxit)
    assert got == kr.verdict(unlabelled, want_inertia, want_shift, iters, tol, maxit)
    return cent, weight, shift, got


def test_stop_codes_are_the_restatements(lib):
    assert [lib.hs_code(k) for k in range(4)] == [kr.RUNNING, kr.CONVERGED, kr.NONFINITE, kr.MAXIT]


@pytest.mark.parametrize("D", [1, 3, 8])
def test_one_iteration_equals_the_restatement(lib, D):
    rs = np.random.RandomState(D)
    x = rs.rand(200, D)
    for w in (np.ones(200), rs.randint(0, 3, size=200).astype(np.float64)):
        cent, weight, shift, got = one_iteration(lib, x, w, x[:9])
        assert shift > 0 and got == kr.RUNNING and np.all(weight > 0)


def test_an_empty_cluster_stays_in_place(lib):
    rs = np.random.RandomState(1)
    x = kn.lattice(rs, 100, 2)
    c = np.array([[4.0, 4.0], [4.0, 4.0], [11.0, 11.0], [100.0, -100.0]])
    cent, weight, shift, got = one_iteration(lib, x, np.ones(100), c)
    assert weight[1] == 0 and weight[3] == 0 and np.array_equal(cent[1], c[1]) and np.array_equal(cent[3], c[3])
    assert got == kr.RUNNING


def test_zero_total_weight_stays_in_place(lib):
    """Points carry the label, but none of positive weight: sum w = 0, sum w x = 0 -- no 0 / 0, the centroid stays."""
    rs = np.random.RandomState(2)
    x = kn.lattice(rs, 100, 2)
    w = np.where(x[:, 0] >= 8, 0.0, 1.0)
    c = np.array([[3.0, 8.0], [12.0, 8.0]])
    cent, weight, shift, got = one_iteration(lib, x, w, c)
    assert weight[1] == 0 and np.array_equal(cent[1], c[1]) and np.all(np.isfinite(cent))
    # the term of the shift of such a cluster is exactly 0
    tot = np.zeros((4, 1))
    keep = np.array([[1.5, -2.5]])
    assert lib.hs_step_cluster(tot.ctypes.data, 1, 2, keep.ctypes.data, np.empty(1).ctypes.data) == 0.0
    assert np.array_equal(keep, [[1.5, -2.5]])


def test_non_finite_verdict(lib):
    nan, inf = float("nan"), float("inf")
    for unlabelled, inertia, shift in ((1.0, 1.0, 0.0), (0.0, nan, 0.0), (0.0, inf, 0.0), (0.0, 1.0, nan), (0.0, 1.0, inf),
                                       (0.0, -inf, 0.0)):
        assert lib.hs_verdict(unlabelled, inertia, shift, 1.0, 1e300, 1) == kr.NONFINITE
        assert kr.verdict(unlabelled, inertia, shift, 1, 1e300, 1) == kr.NONFINITE
    # a NaN point through the whole step: label -1, one point unlabelled, the other clusters' means finite
    rs = np.random.RandomState(3)
    x = rs.rand(50, 2)
    x[7, 0] = nan
    cent, weight, shift, got = one_iteration(lib, x, np.ones(50), x[:3])
    assert got == kr.NONFINITE and weight.sum() == 49


def test_converged_and_maxit_verdicts(lib):
    assert lib.hs_verdict(0.0, 5.0, 0.0, 1.0, 0.0, 10) == kr.CONVERGED       # shift exactly 0 at tol = 0
    assert lib.hs_verdict(0.0, 5.0, 1e-300, 1.0, 0.0, 10) == kr.RUNNING
    assert lib.hs_verdict(0.0, 5.0, 1e-3, 4.0, 1e-3, 10) == kr.CONVERGED      # shift <= tol: equality counts
    assert lib.hs_verdict(0.0, 5.0, 2e-3, 9.0, 1e-3, 10) == kr.RUNNING
    assert lib.hs_verdict(0.0, 5.0, 2e-3, 10.0, 1e-3, 10) == kr.MAXIT
    assert lib.hs_verdict(0.0, 5.0, 1e-3, 10.0, 1e-3, 10) == kr.CONVERGED     # converged in the last iteration allowed
    # a fixed point through the whole step: the labels of the means are the labels, shift exactly 0
    rs = np.random.RandomState(4)
    x = rs.rand(120, 2)
    done = kr.kmeans(x, x[:4], tol=0.0, maxit=200)
    assert done["converged"]
    cent, weight, shift, got = one_iteration(lib, x, np.ones(120), done["centroids"])
    assert shift == 0.0 and got == kr.CONVERGED and np.array_equal(cent, done["centroids"])


def test_symbols_cover_the_header_entry():
    """include/kmvp.h declares kmvp_kmeans with eleven parameters, and _lib.SYMBOLS types every one of them."""
    from kernel_matrix_benchmarks_amd import _lib

    with open(HEADER) as f:
        text = f.read()
    m = re.search(r"^int kmvp_kmeans\(([^;]*)\);", text, flags=re.M)
    assert m, "include/kmvp.h does not declare kmvp_kmeans"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    entry = [s for s in _lib.SYMBOLS if s[0] == "kmvp_kmeans"]
    assert len(entry) == 1 and entry[0][1] is ctypes.c_int and len(entry[0][2]) == len(params) == 11
    assert entry[0][2][1] is ctypes.c_int and entry[0][2][3] is ctypes.c_double and entry[0][2][4] is ctypes.c_int
    assert hasattr(_lib.Context, "kmeans")
