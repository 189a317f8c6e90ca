"""The host side of the eigen-solver (csrc/kmvp_tridiag.hpp: implicit QL on a symmetric tridiagonal with the eigenvector
matrix accumulated) without a GPU: the header is plain C++, compiled here with the host compiler behind
tests/host_tridiag_shim.cpp, and held to numpy.linalg.eigvalsh and to the defining equations T Z = Z Lambda, Z'Z = I."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "kernel_matrix_benchmarks_amd", "csrc")


@pytest.fixture(scope="module")
def tri():
    tmp = tempfile.mkdtemp(prefix="kmvp_host_tridiag_")
    so = os.path.join(tmp, "libhost_tridiag.so")
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC,
                           os.path.join(HERE, "host_tridiag_shim.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    for fn in (lib.ht_eigen, lib.ht_eigen_last):
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    yield lib
    shutil.rmtree(tmp, ignore_errors=True)


def dense(alpha, beta):
    m = len(alpha)
    return np.diag(alpha) + np.diag(beta[: m - 1], 1) + np.diag(beta[: m - 1], -1)


def eigen(lib, alpha, beta):
    alpha, beta = np.ascontiguousarray(alpha, dtype=np.float64), np.ascontiguousarray(beta, dtype=np.float64)
    m = len(alpha)
    theta, Z = np.empty(m), np.empty((m, m))
    ok = lib.ht_eigen(alpha.ctypes.data, beta.ctypes.data, m, theta.ctypes.data, Z.ctypes.data)
    theta2, last = np.empty(m), np.empty(m)
    ok2 = lib.ht_eigen_last(alpha.ctypes.data, beta.ctypes.data, m, theta2.ctypes.data, last.ctypes.data)
    assert ok == ok2
    return bool(ok), theta, Z, theta2, last


def check(lib, alpha, beta):
    m = len(alpha)
    T = dense(alpha, beta)
    norm = np.linalg.norm(T, 2)
    ok, theta, Z, theta2, last = eigen(lib, alpha, beta)
    assert ok
    ref = np.linalg.eigvalsh(T)[::-1]
    assert np.all(np.diff(theta) <= 0) and np.all(np.diff(theta2) <= 0)
    assert np.max(np.abs(theta - ref)) <= 1e-13 * norm
    assert np.max(np.abs(theta2 - ref)) <= 1e-13 * norm
    assert np.linalg.norm(T @ Z - Z * theta, 2) <= m * 1e-14 * norm
    assert np.linalg.norm(Z.T @ Z - np.eye(m), 2) <= m * 1e-14 * norm
    # the last components: Z's last row up to the sign of each eigenvector.  An eigenvector moves by (backward error) /
    # (distance to the nearest other eigenvalue), so that is the scale of each comparison.
    sep = np.full(m, norm)
    if m > 1:
        d = -np.diff(ref)
        sep = np.minimum(np.r_[d, np.inf], np.r_[np.inf, d])
    assert np.all(np.abs(np.abs(last) - np.abs(Z[m - 1])) <= m * 1e-14 * norm / np.maximum(sep, 1e-300) + 1e-14)
    assert abs(np.sum(last ** 2) - 1.0) <= m * 1e-14
    return theta, Z


@pytest.mark.parametrize("m", (1, 2, 7, 64, 300))
def test_random_tridiagonals(tri, m):
    rs = np.random.RandomState(100 + m)
    check(tri, rs.standard_normal(m), rs.standard_normal(m))   # (the last off-diagonal entry is not part of the matrix)


def test_one_by_one_is_its_entry(tri):
    ok, theta, Z, theta2, last = eigen(tri, [2.5], [7.0])
    assert ok and theta[0] == 2.5 and Z[0, 0] == 1.0 and theta2[0] == 2.5 and last[0] == 1.0


def test_exact_split(tri):
    """A zero off-diagonal entry: two independent blocks, the eigenvectors of each are zero on the other."""
    rs = np.random.RandomState(7)
    alpha, beta = rs.standard_normal(12), rs.standard_normal(12)
    beta[4] = 0.0
    theta, Z = check(tri, alpha, beta)
    for i in range(12):
        top, bottom = np.linalg.norm(Z[:5, i]), np.linalg.norm(Z[5:, i])
        assert min(top, bottom) <= 1e-13


def test_lanczos_like_history(tri):
    """Rapidly decaying off-diagonals, as a converging Lanczos process leaves them."""
    m = 40
    alpha = np.linspace(3.0, 0.1, m)
    beta = 0.5 ** np.arange(m)
    check(tri, alpha, beta)


def test_nan_entry_fails(tri):
    rs = np.random.RandomState(9)
    for where in ("alpha", "beta"):
        alpha, beta = rs.standard_normal(7), rs.standard_normal(7)
        (alpha if where == "alpha" else beta)[3] = np.nan
        ok, theta, Z, theta2, last = eigen(tri, alpha, beta)
        assert not ok
        assert np.all(np.isnan(theta)) and np.all(np.isnan(Z)) and np.all(np.isnan(theta2)) and np.all(np.isnan(last))
    alpha, beta = rs.standard_normal(7), rs.standard_normal(7)
    beta[6] = np.nan   # beyond the matrix: not read
    assert eigen(tri, alpha, beta)[0]
