"""CPU tests of the numpy restatement of the Sinkhorn iteration (sinkhorn_reference.py), which the GPU tests
(test_gpu_sinkhorn.py) hold kmvp_<kernel>_sinkhorn to, and of the library's new entry points being there at all."""
import os
import re

import numpy as np
import pytest

import lse_reference
import sinkhorn_reference as sr
from kernel_matrix_benchmarks_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = lse_reference.KERNELS


def small_case(kernel, eps, seed=3, N=37, M=53, D=2):
    rs = np.random.RandomState(seed)
    x, y = rs.rand(N, D), rs.rand(M, D) + 0.2
    a, b = rs.rand(N) + 0.1, rs.rand(M) + 0.1
    scale = 1.0 / np.sqrt(eps) if kernel == "gaussian" else 1.0 / eps
    return x * scale, y * scale, np.log(a / a.sum()), np.log(b / b.sum())


@pytest.mark.parametrize("kernel", KERNELS)
def test_restatement_is_the_textbook_scaling_iteration(kernel):
    """pi = diag(alpha) K diag(beta), K = exp(-C / eps) dense: beta = b / (K^T alpha), alpha = a / (K beta), from alpha = a.
    With alpha = a exp(u), beta = b exp(v) that is v = T2(u), u = T1(v).  eps = 0.1 on unit-size clouds: the smallest
    entry of K is ~exp(-30), nothing underflows."""
    x, y, la, lb = small_case(kernel, 0.1)
    a, b = np.exp(la), np.exp(lb)
    K = np.exp(lse_reference.logits(kernel, x, y))
    assert K.min() > 1e-40
    k = 25
    got = sr.sinkhorn(kernel=kernel, x=x, y=y, log_a=la, log_b=lb, tol=0.0, maxit=k)
    assert got.iters == k and not got.converged and len(got.errs) == k
    alpha = a.copy()
    for it in range(k):
        alpha_prev = alpha
        beta = b / (K.T @ alpha)
        alpha = a / (K @ beta)
    # the restatement returns (u_{k-1}, v_k)
    assert np.max(np.abs(got.u - np.log(alpha_prev / a))) < 1e-11
    assert np.max(np.abs(got.v - np.log(beta / b))) < 1e-11
    # and err_k is the row violation of diag(alpha_{k-1}) K diag(beta_k)
    pi = alpha_prev[:, None] * K * beta[None, :]
    assert abs(got.errs[-1] - np.sum(np.abs(pi.sum(axis=1) - a))) < 1e-13


@pytest.mark.parametrize("kernel,eps", sr.TABLE)
def test_documented_cases_converge_well_inside_maxit_and_err_never_rises(kernel, eps):
    """The four cases the GPU tests run, at tol = 1e-10: maxit = 1000 leaves room (a few hundred iterations at the
    smallest eps; the count is printed and depends on the draw of the clouds, sinkhorn_reference.table_case), and the L1
    marginal error is non-increasing."""
    x, y, la, lb = sr.table_case(kernel, eps)
    got = sr.sinkhorn(kernel=kernel, x=x, y=y, log_a=la, log_b=lb, tol=1e-10, maxit=1000)
    print(f"{kernel} eps={eps}: {got.iters} iterations, err {got.errs[-1]:.3e}, max |u| {np.abs(got.u).max():.3g}, P {got.P:.3g}")
    assert got.converged and got.iters <= 300 and got.errs[-1] <= 1e-10 < got.errs[-2]
    errs = np.array(got.errs)
    assert np.all(errs[1:] <= errs[:-1] * (1 + 1e-9) + 1e-15), "err_k rose"
    assert 1.0 < got.P < 30.0


@pytest.mark.parametrize("kernel", KERNELS)
def test_returned_plan_has_exact_columns_and_the_reported_row_violation(kernel):
    x, y, la, lb = small_case(kernel, 0.05, seed=5)
    for tol, maxit in ((1e-6, 1000), (0.0, 7)):  # stopped by the tolerance, stopped by maxit
        got = sr.sinkhorn(kernel=kernel, x=x, y=y, log_a=la, log_b=lb, tol=tol, maxit=maxit)
        assert got.converged == (tol > 0)
        pi = sr.plan(kernel, x, y, la, lb, got.u, got.v)
        assert np.max(np.abs(pi.sum(axis=0) - np.exp(lb))) < 1e-12
        assert abs(sr.row_violation(kernel, x, y, la, lb, got.u, got.v) - got.errs[-1]) < 1e-12
        assert abs(pi.sum() - 1.0) < 1e-12


@pytest.mark.parametrize("kernel", KERNELS)
def test_zero_mass_points_drop_out_and_keep_a_finite_potential(kernel):
    x, y, la, lb = small_case(kernel, 0.1, seed=9)
    dead_a, dead_b = [0, 11, 36], [5, 6, 52]
    a, b = np.exp(la), np.exp(lb)
    a[dead_a] = 0.0
    b[dead_b] = 0.0
    with np.errstate(divide="ignore"):
        la0, lb0 = np.log(a / a.sum()), np.log(b / b.sum())
    full = sr.sinkhorn(kernel=kernel, x=x, y=y, log_a=la0, log_b=lb0, tol=1e-9, maxit=1000)
    assert full.converged and np.isfinite(full.u).all() and np.isfinite(full.v).all() and np.isfinite(full.errs).all()
    pi = sr.plan(kernel, x, y, la0, lb0, full.u, full.v)
    assert np.all(pi[dead_a] == 0) and np.all(pi[:, dead_b] == 0)
    # the live points see the problem without the dead ones
    ka, kb = np.setdiff1d(np.arange(len(a)), dead_a), np.setdiff1d(np.arange(len(b)), dead_b)
    live = sr.sinkhorn(kernel=kernel, x=x[ka], y=y[kb], log_a=la0[ka], log_b=lb0[kb], tol=1e-9, maxit=1000)
    assert live.iters == full.iters
    assert np.max(np.abs(live.u - full.u[ka])) < 1e-12 and np.max(np.abs(live.v - full.v[kb])) < 1e-12
    assert np.allclose(live.errs, full.errs, rtol=1e-9, atol=1e-15)
    # a dead source's potential is the transform of u like any other's
    v_again, _ = sr.half_step(kernel, y, x, full.u, la0)
    assert np.array_equal(v_again, full.v)


def test_warm_start_from_a_converged_potential_stops_at_once():
    kernel = "gaussian"
    x, y, la, lb = small_case(kernel, 0.1)
    first = sr.sinkhorn(kernel=kernel, x=x, y=y, log_a=la, log_b=lb, tol=1e-8, maxit=1000)
    again = sr.sinkhorn(kernel=kernel, x=x, y=y, log_a=la, log_b=lb, tol=1e-8, maxit=1000, u0=first.u)
    assert first.iters > 5 and again.iters == 1
    assert np.array_equal(again.u, first.u) and np.array_equal(again.v, first.v) and again.errs[-1] == first.errs[-1]


def test_library_exports_and_header_declares_the_sinkhorn_entry_points():
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kmvp.h")).read(), flags=re.S)
    bound = {s[0] for s in _lib.SYMBOLS}
    for name in ("kmvp_gaussian_sinkhorn", "kmvp_absexp_sinkhorn"):
        assert hasattr(lib, name), f"libkmvp.so lacks {name}"
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"include/kmvp.h does not declare {name}"
        assert name in bound
    assert hasattr(_lib.Context, "sinkhorn")
    from kernel_matrix_benchmarks_amd.algorithms import mi355x

    assert hasattr(mi355x, "MI355XSinkhorn")


def test_python_wrapper_checks_weights_before_the_library_is_called():
    from kernel_matrix_benchmarks_amd.algorithms.mi355x import MI355XSinkhorn

    pts = np.random.RandomState(0).rand(5, 2)
    algo = MI355XSinkhorn(kernel="gaussian", dimension=2, eps=0.1)
    with pytest.raises(ValueError, match="non-negative"):
        algo.prepare_data(source_points=pts, target_points=pts, source_weights=[0.2, 0.2, 0.2, 0.2, 0.2],
                          target_weights=[0.5, 0.7, -0.2, 0.0, 0.0])
    with pytest.raises(ValueError, match="total masses differ"):
        algo.prepare_data(source_points=pts, target_points=pts, source_weights=np.full(5, 0.2), target_weights=np.full(5, 0.21))
    with pytest.raises(ValueError, match="entries"):
        algo.prepare_data(source_points=pts, target_points=pts, source_weights=np.full(4, 0.25))
    with pytest.raises(NotImplementedError):
        MI355XSinkhorn(kernel="inverse-distance", dimension=2, eps=0.1)
    with pytest.raises(ValueError):
        MI355XSinkhorn(kernel="gaussian", dimension=2, eps=0.0)
    with pytest.raises(ValueError, match="both needed"):
        algo.prepare_data(source_points=pts, target_points=None)
    for method in (algo.get_potentials, algo.dual_value, algo.barycentric_map):
        with pytest.raises(RuntimeError, match="no solution yet"):
            method()
    assert algo._ctx is None  # nothing reached the device
