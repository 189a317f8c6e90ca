"""Numpy restatement of the Sinkhorn iteration of include/kmvp.h kmvp_<kernel>_sinkhorn -- TEST INFRASTRUCTURE ONLY,
never imported by the package.

Built on ``lse_reference.logsumexp``.  Everything here is on the SCALED points and the dimensionless potentials u = f / eps,
v = g / eps, as the C layer (the temperature is the caller's scaling of the points).  With l the kernel's logit:

    T2(u)_j = -log sum_i exp( l(x_i, y_j) + u_i + log_a_i )        T1(v)_i = -log sum_j exp( l(x_i, y_j) + v_j + log_b_j )
    k = 1, 2, ...:   v_k = T2(u_{k-1});   ut = T1(v_k);   err_k = sum_i a_i | exp(u_{k-1,i} - ut_i) - 1 |
                     err_k <= tol: stop with (u_{k-1}, v_k);   otherwise u_k = ut

``test_sinkhorn_reference.py`` checks it against the textbook iteration in the scaling domain on a dense exp(-C / eps).
"""
import collections

import numpy as np

import lse_reference

Result = collections.namedtuple("Result", "u v iters errs converged P")


def log_weights(n, log_w):
    return np.full(n, -np.log(n)) if log_w is None else np.asarray(log_w, dtype=np.float64)


def half_step(kernel, targets, sources, pot, log_w, precision=np.float64):
    """-log sum_s exp(l(target, source_s) + pot_s + log_w_s) per target, and the log-sum-exp itself."""
    L = lse_reference.logsumexp(kernel=kernel, source_points=sources, target_points=targets,
                                source_signal=(pot + log_w).reshape(-1, 1), precision=precision)[:, 0]
    return -L, L


def marginal_error(log_a, u, ut):
    """sum_i a_i |exp(u_i - ut_i) - 1|; a point of mass 0 contributes exactly 0."""
    live = log_a > -np.inf
    return float(np.sum(np.exp(log_a[live]) * np.abs(np.expm1(u[live] - ut[live]))))


def sinkhorn(*, kernel, x, y, log_a=None, log_b=None, tol=0.0, maxit=1000, u0=None, precision=np.float64):
    """x (N, D) targets with weights a, y (M, D) sources with weights b.  Returns Result(u, v, iters, errs, converged, P):
    the pair (u_{k-1}, v_k) of the first k with err_k <= tol (or of k = maxit), the err_k sequence, and P = the largest
    |log-sum-exp| met on the way."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    log_a, log_b = log_weights(x.shape[0], log_a), log_weights(y.shape[0], log_b)
    u = np.zeros(x.shape[0]) if u0 is None else np.array(u0, dtype=np.float64)
    errs, P = [], 0.0
    for k in range(1, maxit + 1):
        v, Lv = half_step(kernel, y, x, u, log_a, precision)
        ut, Lu = half_step(kernel, x, y, v, log_b, precision)
        P = max(P, float(np.max(np.abs(Lv))), float(np.max(np.abs(Lu))))
        errs.append(marginal_error(log_a, u, ut))
        if errs[-1] <= tol:
            return Result(u, v, k, errs, True, P)
        if k < maxit:
            u = ut
    return Result(u, v, maxit, errs, False, P)


def plan(kernel, x, y, log_a, log_b, u, v):
    """pi_ij = a_i b_j exp(u_i + v_j + l_ij), float64 (N, M)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    log_a, log_b = log_weights(x.shape[0], log_a), log_weights(y.shape[0], log_b)
    with np.errstate(invalid="ignore"):
        return np.exp(lse_reference.logits(kernel, x, y) + (u + log_a)[:, None] + (v + log_b)[None, :])


def row_violation(kernel, x, y, log_a, log_b, u, v):
    """sum_i | sum_j pi_ij - a_i |"""
    pi = plan(kernel, x, y, log_a, log_b, u, v)
    return float(np.sum(np.abs(pi.sum(axis=1) - np.exp(log_weights(pi.shape[0], log_a)))))


def table_case(kernel, eps, seed=7):
    """The clouds of the four documented cases: x = rand(193, 3), y = rand(257, 3) + (0.25, 0, 0), random normalised weights;
    returns the SCALED points and the log-weights."""
    rs = np.random.RandomState(seed)
    x = rs.rand(193, 3)
    y = rs.rand(257, 3) + np.array([0.25, 0.0, 0.0])
    a, b = rs.rand(193), rs.rand(257)
    scale = 1.0 / np.sqrt(eps) if kernel == "gaussian" else 1.0 / eps
    return x * scale, y * scale, np.log(a / a.sum()), np.log(b / b.sum())


TABLE = (("gaussian", 0.1), ("gaussian", 0.02), ("absolute-exponential", 0.1), ("absolute-exponential", 0.03))
