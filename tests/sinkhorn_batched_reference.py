"""Numpy restatement of the batched Sinkhorn solve of include/kmvp.h kmvp_<kernel>_sinkhorn_batched -- TEST INFRASTRUCTURE
ONLY, never imported by the package.

Batch b is the transport problem between the targets x[x_off[b]:x_off[b + 1]] and the sources y[y_off[b]:y_off[b + 1]]; every
batch runs ``sinkhorn_reference.sinkhorn`` on its own clouds with its own clock: it stops at the first k with err_k <= tol
(status 1), on a potential or error of its own that is not finite (status 2) or at k == maxit (status 3), and a batch that is
empty on both sides has 0 iterations, error 0 and status 1.  Log-weights of None are uniform WITHIN each batch.

``test_sinkhorn_batched_reference.py`` checks it against the textbook iteration in the scaling domain on dense per-batch
matrices exp(-C).
"""
import collections

import numpy as np

import sinkhorn_reference as sr

CONVERGED, NONFINITE, MAXIT = 1, 2, 3
Result = collections.namedtuple("Result", "u v iters err status P")


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.int64)


def one_batch(kernel, x, y, log_a, log_b, tol, maxit, u0, precision=np.float64):
    """sinkhorn_reference.sinkhorn with the non-finite stop of the C layer: (u, v, iters, err, status, P)."""
    if x.shape[0] == 0 and y.shape[0] == 0:
        return np.zeros(0), np.zeros(0), 0, 0.0, CONVERGED, 0.0
    assert x.shape[0] > 0 and y.shape[0] > 0, "a batch with points on one side only has no transport problem"
    log_a, log_b = sr.log_weights(x.shape[0], log_a), sr.log_weights(y.shape[0], log_b)
    u = np.zeros(x.shape[0]) if u0 is None else np.array(u0, dtype=np.float64)
    v, P = np.zeros(y.shape[0]), 0.0
    with np.errstate(all="ignore"):
        for k in range(1, maxit + 1):
            v, Lv = sr.half_step(kernel, y, x, u, log_a, precision)
            ut, Lu = sr.half_step(kernel, x, y, v, log_b, precision)
            err = sr.marginal_error(log_a, u, ut)
            if not (np.isfinite(v).all() and np.isfinite(ut).all() and np.isfinite(err)):
                return u, v, k, err, NONFINITE, P
            P = max(P, float(np.max(np.abs(Lv))), float(np.max(np.abs(Lu))))
            if err <= tol:
                return u, v, k, err, CONVERGED, P
            if k < maxit:
                u = ut
    return u, v, maxit, err, MAXIT, P


def sinkhorn(*, kernel, x, y, x_off, y_off, log_a=None, log_b=None, tol=0.0, maxit=1000, u0=None, precision=np.float64):
    """Concatenated targets x (N, D) and sources y (M, D) with B + 1 offsets each; ``maxit`` an int or B ints (a batch's
    own iteration count, for the comparison at the device's k).  Returns Result(u (N), v (M), iters (B), err (B),
    status (B), P (B))."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    x_off, y_off = np.asarray(x_off, dtype=np.int64), np.asarray(y_off, dtype=np.int64)
    B = len(x_off) - 1
    maxits = np.broadcast_to(np.asarray(maxit, dtype=np.int64), (B,))
    u, v = np.zeros(x.shape[0]), np.zeros(y.shape[0])
    iters, err, status, P = np.zeros(B, dtype=np.int64), np.zeros(B), np.zeros(B, dtype=np.int64), np.zeros(B)
    for b in range(B):
        xs, ys = slice(x_off[b], x_off[b + 1]), slice(y_off[b], y_off[b + 1])
        u[xs], v[ys], iters[b], err[b], status[b], P[b] = one_batch(
            kernel, x[xs], y[ys], None if log_a is None else np.asarray(log_a, dtype=np.float64)[xs],
            None if log_b is None else np.asarray(log_b, dtype=np.float64)[ys], tol, int(maxits[b]),
            None if u0 is None else np.asarray(u0, dtype=np.float64)[xs], precision)
    return Result(u, v, iters, err, status, P)


# ---- the ragged case of the GPU tests ---------------------------------------------------------------------------------
TARGET_SIZES = (1, 63, 64, 65, 130)
SOURCE_SIZES = (9, 1, 8, 200, 7)
# the clouds of batch b are scaled by SPREAD[b] (1 / sqrt(eps_b), 1 / eps_b in effect): wider clouds need more iterations
SPREAD = (1.0, 1.5, 2.0, 2.5, 3.0)


def ragged_case(kernel, D=3, seed=11):
    """B = 5 ragged batches with targets of 1, 63, 64, 65, 130 points and sources of 9, 1, 8, 200, 7, random normalised
    weights per batch; returns the scaled points, the offsets and the log-weights."""
    rs = np.random.RandomState(seed)
    x_off, y_off = offsets(TARGET_SIZES), offsets(SOURCE_SIZES)
    xs, ys, las, lbs = [], [], [], []
    for n, m, spread in zip(TARGET_SIZES, SOURCE_SIZES, SPREAD):
        scale = spread if kernel == "gaussian" else spread * 1.5
        xs.append(rs.rand(n, D) * scale)
        ys.append((rs.rand(m, D) + np.array([0.25] + [0.0] * (D - 1))) * scale)
        a, b = rs.rand(n) + 0.1, rs.rand(m) + 0.1
        las.append(np.log(a / a.sum()))
        lbs.append(np.log(b / b.sum()))
    return np.concatenate(xs), np.concatenate(ys), x_off, y_off, np.concatenate(las), np.concatenate(lbs)
