"""CPU tests of the length-scale derivative and of the GP likelihood gradient built on it: the entry points are declared
and bound, the plugin refuses what is not built before a context exists, and the host-side assembly of the gradient
(mi355x.assemble_likelihood_gradient, a pure function) matches a dense numpy computation."""
import os
import re

import numpy as np
import pytest

import dscale_reference
from kernel_matrix_benchmarks_amd import _lib
from kernel_matrix_benchmarks_amd.algorithms import mi355x

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DSCALE_SYMBOLS = ("kmvp_gaussian_dscale", "kmvp_absexp_dscale", "kmvp_matern32_dscale", "kmvp_matern52_dscale")


def test_dscale_entry_points_are_declared_and_listed():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kmvp.h")).read(), flags=re.S)
    listed = {name: (restype, argtypes) for name, restype, argtypes in _lib.SYMBOLS}
    for name in DSCALE_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*kmvp_ctx\s*\*" % name, text), f"kmvp.h does not declare {name}"
        assert name in listed, f"_lib.SYMBOLS lacks {name}"
        assert listed[name][0] is _lib._c.c_int and listed[name][1] == [_lib._c.c_void_p]
    assert not re.search(r"kmvp_invdist_dscale|kmvp_expdot_dscale", text)  # no inverse-distance, no exp-dot entry
    assert callable(getattr(_lib.Context, "run_dscale", None))
    for method in ("query_scale_derivative", "get_scale_derivative"):
        assert callable(getattr(mi355x.MI355XProduct, method, None)), method
    assert callable(getattr(mi355x.MI355XSolver, "log_marginal_likelihood_gradient", None))
    assert mi355x.MarginalLikelihoodGradient._fields == (
        "value", "value_stderr", "d_log_lengthscale", "d_log_lengthscale_stderr", "d_ridge", "d_ridge_stderr", "converged")


def test_plugin_refuses_before_a_context_exists(monkeypatch):
    def no_context(*args, **kwargs):
        raise AssertionError("a refusal must not create a context")

    monkeypatch.setattr(_lib, "Context", no_context)
    refused = (
        (dict(kernel="inverse-distance"), "inverse-distance"),
        (dict(kernel="exp-dot"), "exp-dot"),
        (dict(kernel="gaussian", precision="bfloat16"), "bfloat16"),
        (dict(kernel="matern-3/2", normalize_rows=True), "normalize_rows"),
    )
    for kw, word in refused:
        p = mi355x.MI355XProduct(dimension=3, **kw)
        with pytest.raises(NotImplementedError, match=word):
            p.query_scale_derivative()
    # the solver's: the refusals of log_determinant(), also before a context exists
    for kw, word in ((dict(kernel="inverse-distance"), "inverse-distance"), (dict(kernel="exp-dot"), "exp-dot"),
                     (dict(kernel="gaussian", refine="float32"), "refine"),
                     (dict(kernel="matern-5/2", normalize_rows=True), "normalize_rows")):
        s = mi355x.MI355XSolver(dimension=3, **kw)
        with pytest.raises(NotImplementedError, match=word):
            s.log_marginal_likelihood_gradient()
    # what is built, but called out of order, is a call-order error and not a refusal
    with pytest.raises(RuntimeError, match="query"):
        mi355x.MI355XSolver(kernel="gaussian", dimension=3).log_marginal_likelihood_gradient()


def test_plugin_refuses_shapes_before_the_library_is_called(monkeypatch):
    calls = []

    class Quiet:
        comm_world = 0

        def __init__(self, device=0):
            pass

        def set_option(self, key, value):
            pass

        def set_points(self, y, x, dtype, j_offset=0, M_total=None):
            pass

        def set_signal(self, b):
            pass

        def run_dscale(self, kernel):
            calls.append(kernel)

        def close(self):
            pass

    monkeypatch.setattr(_lib, "Context", Quiet)
    rs = np.random.RandomState(0)

    def prepared(D=3, E=1, **kw):
        p = mi355x.MI355XProduct(dimension=D, **kw)
        y = rs.rand(50, D)
        p.prepare_data(source_points=y, target_points=y, same_points=True)
        p.prepare_query(source_signal=rs.randn(50, E))
        return p

    for kw, word in ((dict(kernel="gaussian", D=9), "D = 9"), (dict(kernel="absolute-exponential", E=5), "E = 5")):
        with pytest.raises(NotImplementedError, match=word):
            prepared(**kw).query_scale_derivative()
    assert calls == []
    # what IS built reaches the library: every kernel, float16 inputs (rounded, float32 arithmetic), the largest shape
    prepared(kernel="gaussian", precision=np.float16).query_scale_derivative()
    prepared(kernel="absolute-exponential", D=8, E=4, precision=np.float64).query_scale_derivative()
    prepared(kernel="matern-3/2").query_scale_derivative()
    prepared(kernel="matern-5/2", precision=np.float32).query_scale_derivative()
    assert calls == list(dscale_reference.KERNELS)


def kernel_matrix(kernel, y):
    """The covariance from its definition, float64."""
    s = np.sum((y[:, None, :] - y[None, :, :]) ** 2, axis=-1)
    r = np.sqrt(s)
    return {"gaussian": np.exp(-s), "absolute-exponential": np.exp(-r),
            "matern-3/2": (1 + np.sqrt(3) * r) * np.exp(-np.sqrt(3) * r),
            "matern-5/2": (1 + np.sqrt(5) * r + 5 * s / 3) * np.exp(-np.sqrt(5) * r)}[kernel]


def dense_pieces(kernel, M=40, D=2, E=2, ridge=0.3, seed=3):
    """A = K + ridge I and dA_d = dA / d log l_d as dense matrices, built column by column from the restatement."""
    rs = np.random.RandomState(seed)
    y, a = rs.rand(M, D) * 2.0, rs.randn(M, E)
    eye = np.eye(M)
    dA = dscale_reference.scale_derivative(kernel=kernel, source_points=y, source_signal=eye)      # (M, M, D): [i, j, d]
    return y, a, kernel_matrix(kernel, y) + ridge * eye, dA


@pytest.mark.parametrize("kernel", dscale_reference.KERNELS)
def test_assembly_matches_a_dense_computation(kernel):
    y, a, A, dA = dense_pieces(kernel)
    M, E = a.shape
    D = y.shape[1]
    lam, V = np.linalg.eigh(A)
    logA, invA = (V * np.log(lam)) @ V.T, (V / lam) @ V.T
    alpha = invA @ a
    h_alpha = np.einsum("ijd,je->ied", dA, alpha)

    def pieces(z):
        return invA @ z, np.einsum("ijd,jp->ipd", dA, z), np.einsum("ip,ij,jp->p", z, logA, z), np.einsum("ip,ij,jp->p", z, invA, z)

    # (1) the probes sqrt(M) e_p, p = 1 .. M, make every trace estimate the exact trace: the assembly IS the gradient
    x, h_z, logquad, invquad = pieces(np.sqrt(M) * np.eye(M))
    got = mi355x.assemble_likelihood_gradient(a, alpha, x, h_z, h_alpha, logquad, invquad)
    value = -0.5 * np.sum(a * alpha) - 0.5 * E * np.sum(np.log(lam)) - 0.5 * E * M * np.log(2 * np.pi)
    want = np.array([0.5 * sum(alpha[:, e] @ dA[:, :, d] @ alpha[:, e] for e in range(E)) - 0.5 * E * np.trace(invA @ dA[:, :, d])
                     for d in range(D)])
    want_ridge = 0.5 * np.sum(alpha * alpha) - 0.5 * E * np.trace(invA)
    assert isinstance(got, mi355x.MarginalLikelihoodGradient) and got.converged is True
    assert got.d_log_lengthscale.shape == (D,) and got.d_log_lengthscale_stderr.shape == (D,)
    assert abs(got.value - value) <= 1e-12 * abs(value)
    assert np.max(np.abs(got.d_log_lengthscale - want)) <= 1e-11 * np.max(np.abs(want))
    assert abs(got.d_ridge - want_ridge) <= 1e-11 * abs(want_ridge)

    # (2) Rademacher probes: means and standard errors from explicit per-probe loops
    P = 7
    z = np.where(np.random.RandomState(5).rand(M, P) < 0.5, -1.0, 1.0)
    x, h_z, logquad, invquad = pieces(z)
    got = mi355x.assemble_likelihood_gradient(a, alpha, x, h_z, h_alpha, logquad, invquad, converged=False)
    assert got.converged is False
    terms = np.array([[z[:, p] @ invA @ dA[:, :, d] @ z[:, p] for d in range(D)] for p in range(P)])
    quad = np.array([sum(alpha[:, e] @ dA[:, :, d] @ alpha[:, e] for e in range(E)) for d in range(D)])
    close = lambda u, v: np.max(np.abs(np.asarray(u) - np.asarray(v))) <= 1e-11 * max(np.max(np.abs(v)), 1e-300)
    assert close(got.d_log_lengthscale, 0.5 * quad - 0.5 * E * terms.mean(axis=0))
    assert close(got.d_log_lengthscale_stderr, 0.5 * E * terms.std(axis=0, ddof=1) / np.sqrt(P))
    assert close(got.d_ridge, 0.5 * np.sum(alpha * alpha) - 0.5 * E * invquad.mean())
    assert close(got.d_ridge_stderr, 0.5 * E * invquad.std(ddof=1) / np.sqrt(P))
    assert close(got.value, -0.5 * np.sum(a * alpha) - 0.5 * E * logquad.mean() - 0.5 * E * M * np.log(2 * np.pi))
    assert close(got.value_stderr, 0.5 * E * logquad.std(ddof=1) / np.sqrt(P))


@pytest.mark.parametrize("kernel", dscale_reference.KERNELS)
def test_sign_and_factor_conventions_against_central_differences_of_the_dense_likelihood(kernel):
    """Pure numpy: with the cloud scaled by exp(-theta_d) per axis, a central difference of the dense exact
    log-likelihood in theta_d = log l_d matches 1/2 alpha' dA_d alpha - E/2 tr(A^-1 dA_d); in the ridge likewise."""
    y, a, A, dA = dense_pieces(kernel)
    M, E = a.shape
    D = y.shape[1]
    ridge = 0.3

    def loglik(scale, ridge):
        A_s = kernel_matrix(kernel, y * scale) + ridge * np.eye(M)
        return (-0.5 * np.sum(a * np.linalg.solve(A_s, a)) - 0.5 * E * np.linalg.slogdet(A_s)[1]
                - 0.5 * E * M * np.log(2 * np.pi))

    invA = np.linalg.inv(A)
    alpha = invA @ a
    exact = np.array([0.5 * np.einsum("ie,ij,je->", alpha, dA[:, :, d], alpha) - 0.5 * E * np.trace(invA @ dA[:, :, d])
                      for d in range(D)])
    h = 1e-5
    for d in range(D):
        up, down = np.ones(D), np.ones(D)
        up[d], down[d] = np.exp(-h), np.exp(h)
        fd = (loglik(up, ridge) - loglik(down, ridge)) / (2 * h)
        assert abs(fd - exact[d]) <= 1e-6 * np.max(np.abs(exact)), (kernel, d, fd, exact[d])
    fd = (loglik(np.ones(D), ridge + h) - loglik(np.ones(D), ridge - h)) / (2 * h)
    want = 0.5 * np.sum(alpha * alpha) - 0.5 * E * np.trace(invA)
    assert abs(fd - want) <= 1e-6 * abs(want), (kernel, fd, want)
