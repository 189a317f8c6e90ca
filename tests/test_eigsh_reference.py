"""CPU tests of the eigen-solver's restatement (eigsh_reference.py), made without the code under test: on the clouds the
GPU tests use it agrees with numpy.linalg.eigh, its basis is orthonormal, and the top eigenvalues are separated far enough
for an index-by-index comparison at both tolerances.  Also: the entry points are declared, exported and bound, and (where
sklearn imports) the centred Gaussian case is sklearn's KernelPCA."""
import os
import re

import numpy as np
import pytest

from kernel_matrix_benchmarks_amd import _lib
from kernel_matrix_benchmarks_amd.algorithms import mi355x

import eigsh_reference as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EIGSH_SYMBOLS = ("kmvp_gaussian_eigsh", "kmvp_absexp_eigsh", "kmvp_matern32_eigsh", "kmvp_matern52_eigsh")


def test_entry_points_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kmvp.h")).read(), flags=re.S)
    lib = _lib.load()
    bound = {s[0]: s for s in _lib.SYMBOLS}
    for name in EIGSH_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*kmvp_ctx\s*\*" % name, text), f"kmvp.h does not declare {name}"
        assert hasattr(lib, name), f"libkmvp.so lacks {name}"
        assert name in bound, f"_lib.SYMBOLS does not bind {name}"
        assert bound[name][2] == bound["kmvp_gaussian_eigsh"][2]
    assert not hasattr(lib, "kmvp_invdist_eigsh")
    assert re.search(r"KMVP_EIG_KERNEL\s*=\s*0\s*,\s*KMVP_EIG_CENTERED\s*=\s*1\s*,\s*KMVP_EIG_NORMALIZED\s*=\s*2", text)
    assert _lib.EIG_OPERATORS == {"kernel": 0, "centered": 1, "normalized": 2}
    assert lib.kmvp_abi_version() == 1  # entries were added, nothing changed
    assert callable(getattr(_lib.Context, "eigsh", None))
    for method in ("prepare_data", "set_query_arguments", "query", "get_eigenvalues", "get_eigenvectors", "get_residuals",
                   "get_degree", "get_embedding", "transform", "get_additional", "get_memory_usage", "done"):
        assert callable(getattr(mi355x.MI355XSpectral, method, None)), method


@pytest.mark.parametrize("op", er.OPERATORS)
@pytest.mark.parametrize("kernel", er.KERNELS)
def test_restatement_against_eigh(kernel, op):
    """At tol 1e-10 (24 - 40 steps): the eigenvalues are eigh's to N eps lambda_1 = 1.8e-13 lambda_1, the backward error of
    eigh itself on an N x N matrix (measured: <= 3e-15 lambda_1); the true residuals meet 1.5 tol; and the conditions of
    its own inputs that the GPU test's index-wise comparison and orthogonality bound rest on: X'X = I and V V' = I to
    1e-12 (measured: <= 3e-15), and the smallest gap among the top K + 1 eigenvalues is >= 100 tol lambda_1 for both
    tolerances of the GPU tests."""
    A, lam, _ = er.system(kernel, op)
    r = er.eigsh(A, er.K, er.start_vector(), 1e-10, er.MAXIT, centered=op == "centered")
    gap = float(np.min(-np.diff(lam[: er.K + 1]))) / lam[0]
    err = float(np.max(np.abs(r.eigenvalues - lam[: er.K]))) / lam[0]
    orth = float(np.max(np.abs(r.eigenvectors.T @ r.eigenvectors - np.eye(er.K))))
    basis = float(np.max(np.abs(r.V @ r.V.T - np.eye(r.steps))))
    print(f"{kernel} {op}: steps {r.steps}, eigenvalue error {err:.3g} lambda_1, X'X - I {orth:.3g}, V V' - I {basis:.3g}, "
          f"gap {gap:.3g} lambda_1, worst resid {r.resid.max():.3g}")
    assert r.converged and not r.breakdown and er.K <= r.steps < er.MAXIT and r.steps % er.LOOK == 0
    assert err <= er.N * np.finfo(np.float64).eps
    assert orth <= 1e-12 and basis <= 1e-12
    for tol in er.TOLS.values():
        assert gap >= 100.0 * tol, (gap, tol)
    assert np.all(r.resid <= 1.5e-10)
    if op == "normalized":
        assert abs(r.eigenvalues[0] - 1.0) <= er.N * np.finfo(np.float64).eps
    if op == "centered":
        assert np.max(np.abs(r.eigenvectors.sum(axis=0))) <= 1e-10 * np.sqrt(er.N)
    for c in range(er.K):
        assert r.eigenvectors[np.argmax(np.abs(r.eigenvectors[:, c])), c] > 0


def test_float32_cloud_keeps_the_gap():
    """The float32 cases run on the cloud rounded to float32: another matrix, the same separation."""
    for kernel in er.KERNELS:
        for op in er.OPERATORS:
            _, lam, _ = er.system(kernel, op, "float32")
            assert float(np.min(-np.diff(lam[: er.K + 1]))) / lam[0] >= 100.0 * er.TOLS["float32"]


def test_maxit_equal_k_and_breakdown():
    """maxit = k: k steps, one look, not converged, everything finite.  N = 8: the Krylov space is exhausted after at
    most 8 steps and the Ritz values are the eigenvalues."""
    A, lam, _ = er.system("absolute-exponential", "kernel")
    r = er.eigsh(A, er.K, er.start_vector(), 1e-10, er.K)
    assert r.steps == er.K and not r.converged and np.all(np.isfinite(r.eigenvectors)) and r.resid.max() > 1.5e-10
    y = er.cloud(8, seed=3)
    A8 = er.operator(er.kernel_matrix("gaussian", y), "kernel")
    r = er.eigsh(A8, 3, er.start_vector(8), 1e-12, 8)
    lam8 = np.linalg.eigvalsh(A8)[::-1]
    assert r.converged and r.steps <= 8
    assert np.max(np.abs(r.eigenvalues - lam8[:3])) <= 1e-12 * lam8[0]


def test_sign_rule_tie_goes_to_the_smallest_index():
    X = np.array([[-0.5, 0.5], [0.5, -0.5], [0.1, 0.7]])
    F = er.fix_signs(X)
    assert np.array_equal(F[:, 0], [0.5, -0.5, -0.1]) and np.array_equal(F[:, 1], X[:, 1])


def test_centred_gaussian_is_sklearns_kernel_pca():
    pytest.importorskip("sklearn")
    from sklearn.decomposition import KernelPCA
    A, lam, y = er.system("gaussian", "centered")
    r = er.eigsh(A, er.K, er.start_vector(), 1e-10, er.MAXIT, centered=True)
    pca = KernelPCA(n_components=er.K, kernel="rbf", gamma=1.0, eigen_solver="dense")
    Z = pca.fit_transform(y)
    assert np.max(np.abs(pca.eigenvalues_ - r.eigenvalues)) <= 1e-12 * lam[0]
    E = er.embedding("centered", r.eigenvalues, r.eigenvectors)
    signs = np.sign(np.sum(E * Z, axis=0))
    assert np.max(np.abs(E - Z * signs)) <= 1e-10 * np.sqrt(lam[0])
    x_new = er.cloud(50, seed=99)
    T = er.transform("gaussian", "centered", y, r.eigenvalues, r.eigenvectors, x_new)
    assert np.max(np.abs(T - pca.transform(x_new) * signs)) <= 1e-9 * np.sqrt(lam[0])
