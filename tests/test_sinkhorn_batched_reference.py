"""CPU tests of the numpy restatement of the batched Sinkhorn solve (sinkhorn_batched_reference.py), which the GPU tests
(test_gpu_sinkhorn_batched.py) hold kmvp_<kernel>_sinkhorn_batched to; of the ragged case those tests run; and of the
library's new entry points being there at all."""
import os
import re

import numpy as np
import pytest

import lse_reference
import sinkhorn_batched_reference as sbr
import sinkhorn_reference as sr
from kernel_matrix_benchmarks_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = lse_reference.KERNELS


def small_batches(kernel, sizes=((5, 9), (0, 0), (37, 53), (20, 3)), D=2, seed=3):
    rs = np.random.RandomState(seed)
    xs, ys, las, lbs = [], [], [], []
    for q, (n, m) in enumerate(sizes):
        scale = (1.0 + 0.7 * q) * (1.0 if kernel == "gaussian" else 2.0)
        xs.append(rs.rand(n, D) * scale)
        ys.append((rs.rand(m, D) + 0.2) * scale)
        a, b = rs.rand(n) + 0.1, rs.rand(m) + 0.1
        las.append(np.log(a / max(a.sum(), 1e-300)))
        lbs.append(np.log(b / max(b.sum(), 1e-300)))
    x_off, y_off = sbr.offsets([s[0] for s in sizes]), sbr.offsets([s[1] for s in sizes])
    return np.concatenate(xs), np.concatenate(ys), x_off, y_off, np.concatenate(las), np.concatenate(lbs)


@pytest.mark.parametrize("kernel", KERNELS)
def test_every_batch_is_the_textbook_scaling_iteration_on_its_own_dense_matrix(kernel):
    """Per batch, K_b = exp(-C_b) dense: beta = b / (K^T alpha), alpha = a / (K beta) from alpha = a; with alpha = a exp(u),
    beta = b exp(v) that is v = T2(u), u = T1(v).  The restatement returns (u_{k-1}, v_k) and the row violation of that plan."""
    x, y, x_off, y_off, la, lb = small_batches(kernel)
    k = 8  # (tol = 0 can be met: a small batch reaches err == 0 exactly after a dozen iterations)
    got = sbr.sinkhorn(kernel=kernel, x=x, y=y, x_off=x_off, y_off=y_off, log_a=la, log_b=lb, tol=0.0, maxit=k)
    for b in range(len(x_off) - 1):
        xs, ys = slice(x_off[b], x_off[b + 1]), slice(y_off[b], y_off[b + 1])
        if x_off[b + 1] == x_off[b]:
            assert (got.iters[b], got.err[b], got.status[b]) == (0, 0.0, sbr.CONVERGED)
            continue
        assert got.iters[b] == k and got.status[b] == sbr.MAXIT
        a, bw = np.exp(la[xs]), np.exp(lb[ys])
        K = np.exp(lse_reference.logits(kernel, x[xs], y[ys]))
        assert K.min() > 1e-40
        alpha = a.copy()
        for _ in range(k):
            alpha_prev = alpha
            beta = bw / (K.T @ alpha)
            alpha = a / (K @ beta)
        assert np.max(np.abs(got.u[xs] - np.log(alpha_prev / a))) < 1e-11
        assert np.max(np.abs(got.v[ys] - np.log(beta / bw))) < 1e-11
        pi = alpha_prev[:, None] * K * beta[None, :]
        assert abs(got.err[b] - np.sum(np.abs(pi.sum(axis=1) - a))) < 1e-13


@pytest.mark.parametrize("kernel", KERNELS)
def test_every_batch_has_its_own_clock_and_is_the_unbatched_restatement(kernel):
    """Stopped by the tolerance at different k: every batch is bit for bit sinkhorn_reference.sinkhorn on its clouds (the
    restatement shares its half-steps), also with uniform weights (None: -log n_b, -log m_b within the batch)."""
    x, y, x_off, y_off, la, lb = small_batches(kernel)
    for wa, wb in ((la, lb), (None, None)):
        got = sbr.sinkhorn(kernel=kernel, x=x, y=y, x_off=x_off, y_off=y_off, log_a=wa, log_b=wb, tol=1e-9, maxit=1000)
        assert len(set(got.iters[[0, 2, 3]])) >= 2, got.iters
        for b in (0, 2, 3):
            xs, ys = slice(x_off[b], x_off[b + 1]), slice(y_off[b], y_off[b + 1])
            one = sr.sinkhorn(kernel=kernel, x=x[xs], y=y[ys], log_a=None if wa is None else wa[xs],
                              log_b=None if wb is None else wb[ys], tol=1e-9, maxit=1000)
            assert one.converged and got.status[b] == sbr.CONVERGED and got.iters[b] == one.iters
            assert np.array_equal(got.u[xs], one.u) and np.array_equal(got.v[ys], one.v) and got.err[b] == one.errs[-1]
            assert got.P[b] == one.P


def test_a_non_finite_batch_stops_alone_with_status_2():
    kernel = "gaussian"
    x, y, x_off, y_off, la, lb = small_batches(kernel)
    clean = sbr.sinkhorn(kernel=kernel, x=x, y=y, x_off=x_off, y_off=y_off, log_a=la, log_b=lb, tol=1e-9, maxit=1000)
    x_nan = x.copy()
    x_nan[x_off[2] + 4, 1] = np.nan
    got = sbr.sinkhorn(kernel=kernel, x=x_nan, y=y, x_off=x_off, y_off=y_off, log_a=la, log_b=lb, tol=1e-9, maxit=1000)
    assert list(got.status) == [1, 1, 2, 1] and got.iters[2] == 1
    assert np.array_equal(got.u[x_off[2]:x_off[3]], np.zeros(x_off[3] - x_off[2]))  # u_0, uncommitted
    for b in (0, 3):
        xs, ys = slice(x_off[b], x_off[b + 1]), slice(y_off[b], y_off[b + 1])
        assert np.array_equal(got.u[xs], clean.u[xs]) and np.array_equal(got.v[ys], clean.v[ys]) and got.iters[b] == clean.iters[b]


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("tol", (1e-8, 1e-4))
def test_the_ragged_case_of_the_gpu_tests_stops_at_several_iteration_counts(kernel, tol):
    """What test_gpu_sinkhorn_batched.py asserts of the restatement, verified here: at both tolerances every batch converges
    well inside maxit = 1000 and the batches stop at two or more distinct k -- on the float64 points and on the
    float32-rounded ones."""
    x, y, x_off, y_off, la, lb = sbr.ragged_case(kernel)
    for npdt in (np.float64, np.float32):
        xr, yr = x.astype(npdt).astype(np.float64), y.astype(npdt).astype(np.float64)
        got = sbr.sinkhorn(kernel=kernel, x=xr, y=yr, x_off=x_off, y_off=y_off, log_a=la, log_b=lb, tol=tol, maxit=1000)
        print(f"{kernel} tol={tol:g} {np.dtype(npdt).name}: iterations {list(got.iters)}, P {np.round(got.P, 2)}")
        assert np.all(got.status == sbr.CONVERGED) and got.iters.max() <= 400
        assert len(set(got.iters)) >= 2, got.iters


def test_library_exports_and_header_declares_the_batched_entry_points():
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kmvp.h")).read(), flags=re.S)
    bound = {s[0] for s in _lib.SYMBOLS}
    for name in ("kmvp_gaussian_sinkhorn_batched", "kmvp_absexp_sinkhorn_batched"):
        assert hasattr(lib, name), f"libkmvp.so lacks {name}"
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), f"include/kmvp.h does not declare {name}"
        assert name in bound
    assert hasattr(_lib.Context, "sinkhorn_batched")


def test_plugin_checks_batches_and_weights_before_the_library_is_called():
    from kernel_matrix_benchmarks_amd.algorithms.mi355x import MI355XSinkhorn

    rs = np.random.RandomState(0)
    y, x = rs.rand(7, 2), rs.rand(5, 2)
    algo = MI355XSinkhorn(kernel="gaussian", dimension=2, eps=0.1)
    with pytest.raises(ValueError, match="needs source_batches"):
        algo.prepare_data(source_points=y, target_points=x, target_batches=[0, 2, 5])
    with pytest.raises(ValueError, match="same_points=True"):
        algo.prepare_data(source_points=y, target_points=x, source_batches=[0, 3, 7])
    with pytest.raises(ValueError, match="non-decreasing"):
        algo.prepare_data(source_points=y, target_points=x, source_batches=[0, 3, 6], target_batches=[0, 2, 5])
    with pytest.raises(ValueError, match="both hold"):
        algo.prepare_data(source_points=y, target_points=x, source_batches=[0, 3, 7], target_batches=[0, 2, 3, 5])
    with pytest.raises(ValueError, match="batch 1 has points on one side only"):
        algo.prepare_data(source_points=y, target_points=x, source_batches=[0, 3, 3, 7], target_batches=[0, 2, 3, 5])
    with pytest.raises(ValueError, match="total masses differ in batch 1"):
        algo.prepare_data(source_points=y, target_points=x, source_batches=[0, 3, 7], target_batches=[0, 2, 5],
                          source_weights=[1, 1, 1, 1, 1, 1, 1], target_weights=[1.5, 1.5, 1, 1, 1])
    assert algo._ctx is None  # nothing reached the device
