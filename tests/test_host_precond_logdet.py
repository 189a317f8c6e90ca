"""pc_logdet of csrc/kmvp_precond.hpp (log det C = 2 sum log G_tt off the Cholesky factor pc_cholesky left: the factor's
share of log det P in kmvp_<kernel>_lanczos_quadrature_precond) without a GPU: compiled with the host compiler behind
tests/host_precond_logdet_shim.cpp and held to numpy.linalg.slogdet."""
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
    tmp = tempfile.mkdtemp(prefix="kmvp_host_precond_logdet_")
    so = os.path.join(tmp, "libhost_precond_logdet.so")
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC,
                           os.path.join(HERE, "host_precond_logdet_shim.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.hl_cholesky.restype = ctypes.c_int
    lib.hl_cholesky.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    lib.hl_logdet.restype = ctypes.c_double
    lib.hl_logdet.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    yield lib
    shutil.rmtree(tmp, ignore_errors=True)


def logdet(lib, C, ld):
    """pc_logdet of pc_cholesky's factor, stored with leading dimension ld; everything outside the lower triangle is NaN,
    so a read there shows in the result."""
    n = C.shape[0]
    a = np.full((n, ld), np.nan)
    a[:, :n] = np.where(np.tri(n, dtype=bool), C, np.nan)
    assert lib.hl_cholesky(a.ctypes.data, n, ld)
    return lib.hl_logdet(a.ctypes.data, n, ld)


@pytest.mark.parametrize("n", [1, 16, 17, 128])
def test_against_numpy_on_random_spd_matrices(dense, n):
    """A sum of n logarithms of O(1) .. O(10) numbers, each from a pivot the factorisation leaves with a relative error of
    about n eps: absolute 1e-11 is 30 times n^2 eps at n = 128."""
    rs = np.random.RandomState(100 + n)
    B = rs.randn(n, 3 * n)
    C = np.eye(n) + B @ B.T * rs.uniform(0.1, 10.0)
    sign, ref = np.linalg.slogdet(C)
    for ld in (n, 128):
        got = logdet(dense, C, ld)
        print(f"n={n} ld={ld}: {got!r} numpy {ref!r} difference {abs(got - ref):.3g}")
        assert sign > 0 and abs(got - ref) <= 1e-11
    if n == 1:
        assert logdet(dense, C, 1) == 2.0 * np.log(np.sqrt(C[0, 0]))


@pytest.mark.parametrize("name", pr.CUBE)
def test_on_the_table_systems(dense, name):
    """C = I + L D^-1 L' of the rank-32 factors (cond up to 1e4, log det C about 150)."""
    C = pr.gram(pr.factor(name)[0], pr.DIAG)
    sign, ref = np.linalg.slogdet(C)
    got = logdet(dense, C, 128)
    print(f"{name}: {got!r} numpy {ref!r}")
    assert sign > 0 and abs(got - ref) <= 1e-11 * abs(ref)


def test_order_zero_is_zero(dense):
    assert dense.hl_logdet(None, 0, 0) == 0.0
