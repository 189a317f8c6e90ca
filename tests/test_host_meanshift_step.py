"""The rule of one mean-shift sweep for one point (csrc/kmvp_meanshift_step.hpp: update, squared step, freeze, the NaN
rule) without a GPU: the header is plain C++ behind a macro for the device attributes, compiled here with the host compiler
behind tests/host_meanshift_step_shim.cpp and held to the restatement (meanshift_reference.step) BIT FOR BIT.

-ffp-contract=off: the rule rounds every product and every sum on its own (on the device __dmul_rn / __dadd_rn); g++ has
no pragma for that, and would otherwise be free to fuse on a machine with fused multiply-add."""
import ctypes
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import meanshift_reference as mr

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "kernel_matrix_benchmarks_amd", "csrc")
HEADER = os.path.join(HERE, "..", "include", "kmvp.h")
ACTIVE, FROZEN, NONFINITE = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    tmp = tempfile.mkdtemp(prefix="kmvp_host_meanshift_step_")
    so = os.path.join(tmp, "libhost_meanshift_step.so")
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC,
                           os.path.join(HERE, "host_meanshift_step_shim.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.ms_code.restype = ctypes.c_int
    lib.ms_code.argtypes = [ctypes.c_int]
    lib.ms_step_rows.restype = None
    lib.ms_step_rows.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long, ctypes.c_int, ctypes.c_double,
                                 ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    yield lib
    shutil.rmtree(tmp, ignore_errors=True)


def header_step(lib, G, base, tol):
    G = np.ascontiguousarray(G, dtype=np.float64)
    base = np.ascontiguousarray(base, dtype=np.float64)
    n, D = G.shape
    z = np.full((n, D), -7.0)
    q = np.full(n, -7.0)
    verdict = np.full(n, -7, dtype=np.intc)
    lib.ms_step_rows(G.ctypes.data, base.ctypes.data, n, D, float(tol), z.ctypes.data, q.ctypes.data, verdict.ctypes.data)
    return z, q, verdict


def same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float64).view(np.uint64), np.asarray(b, dtype=np.float64).view(np.uint64))


def hold_to_restatement(lib, G, base, tol):
    z, q, verdict = header_step(lib, G, base, tol)
    want_z, want_q, frozen, nonfinite = mr.step(G, base, tol)
    want_verdict = np.where(nonfinite, NONFINITE, np.where(frozen, FROZEN, ACTIVE))
    # NaN rows: every NaN the rule writes is the one quiet NaN of __builtin_nan(""), numpy's np.nan
    assert same_bits(z, want_z) and same_bits(q, want_q) and np.array_equal(verdict, want_verdict)
    return z, q, verdict


def test_codes(lib):
    assert [lib.ms_code(k) for k in range(3)] == [ACTIVE, FROZEN, NONFINITE]


@pytest.mark.parametrize("D", [1, 2, 3, 5, 8])
def test_random_rows_equal_the_restatement(lib, D):
    rs = np.random.RandomState(D)
    n = 4000
    # steps over twenty orders of magnitude around the tolerance, positions of either sign
    G = rs.randn(n, D) * 10.0 ** rs.uniform(-12, 8, size=(n, 1))
    base = rs.randn(n, D) * 10.0 ** rs.uniform(-3, 3, size=(n, 1))
    for tol in (1e-4, 1e-10, 0.0, 3.0):
        z, q, verdict = hold_to_restatement(lib, G, base, tol)
        assert np.any(verdict == ACTIVE)
        assert np.any(verdict == FROZEN) or tol == 0.0


def test_equality_with_the_tolerance_freezes(lib):
    # q == tol^2 exactly: h = (3, 4) * 2^-20, q = 25 * 2^-40 = (5 * 2^-20)^2
    G = np.array([[6.0, 8.0]]) * 2.0 ** -20
    tol = 5.0 * 2.0 ** -20
    z, q, verdict = hold_to_restatement(lib, G, np.array([[1.0, -1.0]]), tol)
    assert q[0] == tol * tol and verdict[0] == FROZEN
    # one ulp less of tolerance: the point goes on
    z, q, verdict = hold_to_restatement(lib, G, np.array([[1.0, -1.0]]), np.nextafter(tol, 0.0))
    assert verdict[0] == ACTIVE


def test_tol_zero_freezes_only_a_step_of_exactly_zero(lib):
    G = np.array([[0.0, 0.0, 0.0], [0.0, -0.0, 0.0], [0.0, 5e-324, 0.0], [0.0, 1e-200, 0.0], [1e-150, 0.0, 0.0]])
    z, q, verdict = hold_to_restatement(lib, G, np.ones((5, 3)), 0.0)
    # 5e-324 / 2 and (1e-200 / 2)^2 round to 0: what counts is the q the rule computes, not the gradient
    assert list(verdict) == [FROZEN, FROZEN, FROZEN, FROZEN, ACTIVE]
    assert np.array_equal(z[:2], np.ones((2, 3)))


def test_non_finite_gradient_rows(lib):
    nan, inf = float("nan"), float("inf")
    G = np.array([[nan, 1.0], [1.0, nan], [inf, 0.0], [0.0, -inf], [inf, -inf], [1.0, 1.0], [1e200, 0.0]])
    base = np.arange(14, dtype=np.float64).reshape(7, 2)
    z, q, verdict = hold_to_restatement(lib, G, base, 1e-3)
    assert list(verdict) == [NONFINITE] * 5 + [ACTIVE, ACTIVE]
    assert np.all(np.isnan(z[:5])) and np.all(np.isnan(q[:5]))
    assert np.array_equal(z[5], [10.5, 11.5]) and q[5] == 0.5
    assert q[6] == np.inf  # a finite gradient whose square overflows: neither frozen nor non-finite, the point goes on
    # a NaN position under a finite gradient is no reason of its own: the rule looks at G (on the device a NaN coordinate
    # makes the whole row of G NaN)
    z, q, verdict = hold_to_restatement(lib, np.array([[0.0, 0.0]]), np.array([[nan, 1.0]]), 1e-3)
    assert verdict[0] == FROZEN and np.isnan(z[0, 0]) and z[0, 1] == 1.0


def test_in_place_update(lib):
    """ms_step_kernel passes separate arrays, but the rule documents that z may alias base."""
    rs = np.random.RandomState(11)
    G, base = rs.randn(50, 3), rs.randn(50, 3)
    want_z, want_q, _, _ = mr.step(G, base, 1e-4)
    buf = base.copy()
    q = np.empty(50)
    verdict = np.empty(50, dtype=np.intc)
    lib.ms_step_rows(G.ctypes.data, buf.ctypes.data, 50, 3, 1e-4, buf.ctypes.data, q.ctypes.data, verdict.ctypes.data)
    assert same_bits(buf, want_z) and same_bits(q, want_q)


def test_symbols_cover_the_header_entry():
    """include/kmvp.h declares kmvp_gaussian_meanshift with eight parameters, and _lib.SYMBOLS types every one of them."""
    from kernel_matrix_benchmarks_amd import _lib

    with open(HEADER) as f:
        text = f.read()
    m = re.search(r"^int kmvp_gaussian_meanshift\(([^;]*)\);", text, flags=re.M)
    assert m, "include/kmvp.h does not declare kmvp_gaussian_meanshift"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    entry = [s for s in _lib.SYMBOLS if s[0] == "kmvp_gaussian_meanshift"]
    assert len(entry) == 1 and entry[0][1] is ctypes.c_int and len(entry[0][2]) == len(params) == 8
    assert entry[0][2][1] is ctypes.c_double and entry[0][2][2] is ctypes.c_int
    assert hasattr(_lib.Context, "meanshift")
    assert "kmvp_absexp_meanshift" not in text  # Gaussian only: the header says why
