"""The small dense routines of the preconditioner (csrc/kmvp_precond.hpp: Cholesky of C = I + L D^-1 L', forward and back
substitution) without a GPU: the header is plain C++, compiled here with the host compiler behind
tests/host_precond_shim.cpp, and held to numpy on the C matrices of the restatement's systems (precond_reference.py)."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import precond_reference as pr

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "kernel_matrix_benchmarks_amd", "csrc")


@pytest.fixture(scope="module")
def dense():
    tmp = tempfile.mkdtemp(prefix="kmvp_host_precond_")
    so = os.path.join(tmp, "libhost_precond.so")
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC,
                           os.path.join(HERE, "host_precond_shim.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.hp_cholesky.restype = ctypes.c_int
    lib.hp_cholesky.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    for fn in (lib.hp_forward, lib.hp_backward):
        fn.restype = None
        fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    yield lib
    shutil.rmtree(tmp, ignore_errors=True)


def cholesky(lib, C, ld=None):
    """(ok, G): the factor in the lower triangle of a copy with leading dimension ld, the rest of the copy NaN so that
    a read outside the lower triangle shows."""
    n = C.shape[0]
    ld = n if ld is None else ld
    a = np.full((n, ld), np.nan)
    a[:, :n] = np.where(np.tri(n, dtype=bool), C, np.nan)
    ok = lib.hp_cholesky(a.ctypes.data, n, ld)
    return bool(ok), a


def solve(lib, a, n, ld, t):
    """C w = t per column of t (n, E) through both substitutions with the column stride the library uses."""
    w = np.array(t, dtype=np.float64, order="C", ndmin=2)
    E = w.shape[1]
    for e in range(E):
        col = w.ctypes.data + 8 * e
        lib.hp_forward(a.ctypes.data, n, ld, col, E)
        lib.hp_backward(a.ctypes.data, n, ld, col, E)
    return w


def relative(x, ref):
    return float(np.abs(x - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize("name", list(pr.SYSTEMS))
def test_against_numpy_on_the_table_systems(dense, name):
    """C = I + L D^-1 L' of the system's rank-32 factor (cond 1e2 .. 1e4): the factor against numpy.linalg.cholesky and
    the solve of three columns against numpy.linalg.solve, relative 1e-12; with a leading dimension of 128 as the library
    stores a factor that stopped early."""
    L, _, _ = pr.factor(name)
    C = pr.gram(L, pr.DIAG)
    t = L @ (pr.rhs(3) / pr.DIAG[:, None])
    for ld in (pr.RANK, 128):
        ok, a = cholesky(dense, C, ld)
        assert ok
        G = np.tril(a[:, :pr.RANK])
        w = solve(dense, a, pr.RANK, ld, t)
        ref = np.linalg.solve(C, t)
        print(f"{name} ld={ld}: cond {np.linalg.cond(C):.3g}, factor {relative(G, np.linalg.cholesky(C)):.3g}, solve "
              f"{relative(w[:, :2], ref[:, :2]):.3g}")
        assert relative(G, np.linalg.cholesky(C)) <= 1e-12
        assert relative(w[:, :2], ref[:, :2]) <= 1e-12
        assert not w[:, 2].any()  # the zero column
        assert np.isnan(a[np.triu_indices(pr.RANK, 1)]).all() and np.isnan(a[:, pr.RANK:]).all()  # nothing else was written


@pytest.mark.parametrize("n", [1, 2, 128])
def test_orders_one_two_and_the_largest(dense, n):
    assert dense.hp_max_rank() == pr.MAX_RANK == 128
    rs = np.random.RandomState(n)
    B = rs.randn(n, 3 * n)
    C = np.eye(n) + B @ B.T / n
    ok, a = cholesky(dense, C)
    assert ok and relative(np.tril(a), np.linalg.cholesky(C)) <= 1e-12
    t = rs.randn(n, 2)
    assert relative(solve(dense, a, n, n, t), np.linalg.solve(C, t)) <= 1e-12
    if n == 1:
        assert a[0, 0] == np.sqrt(C[0, 0])


def test_not_positive_definite_reports_failure(dense):
    """An indefinite matrix, a singular one, a zero and a NaN on the diagonal all return failure; order 0 succeeds."""
    assert not cholesky(dense, np.array([[1.0, 2.0], [2.0, 1.0]]))[0]
    assert not cholesky(dense, np.array([[1.0, 1.0], [1.0, 1.0]]))[0]
    assert not cholesky(dense, np.array([[0.0]]))[0]
    assert not cholesky(dense, np.array([[np.nan]]))[0]
    C = np.eye(5)
    C[3, 3] = -1e-3
    assert not cholesky(dense, C)[0]
    assert dense.hp_cholesky(None, 0, 0) == 1
