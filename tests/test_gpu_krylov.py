"""The Krylov drivers of csrc/kmvp_solvers.hip against their float64 restatement, iteration by iteration (-m gpu).

The other solver tests judge the end of a solve.  These hold conjugate gradients and MINRES, through Context.cg_solve
and set_solver_diagonal, to krylov_reference.py on the well-conditioned 257-point systems of its table, where the
trajectory of a solve is reproducible: the iteration count is the restatement's, the iterate is the restatement's
iterate OF THAT ITERATION (not the one at the end of the burst of eight: test_krylov_reference.py shows the two to be
at least 100 tolerances apart), a solve stopped by maxit returns x_maxit, a zero column stays 0, and nothing is left
behind on the context.

    error      max over the non-zero columns e of ||x_gpu[:, e] - x_ref[:, e]|| / ||x_ref[:, e]|| (the columns are
               scaled 1, 1e-6 and 1e3)
    tolerance  4 g TOL, TOL = 1e-11 (float64) / 1e-5 (float32) for the product's error and g the case's amplification
               of such an error, measured and recorded by the CPU tests (krylov_reference.SYSTEMS)
    resid      the library's verdict against numpy's max_e |a - A x_gpu| / |a| within kappa 1e-11
"""
import numpy as np
import pytest

import krylov_reference as kr
from kernel_matrix_benchmarks_amd import _lib

pytestmark = pytest.mark.gpu
ES = (4, 1)
CODES = {"float64": _lib.KMVP_F64, "float32": _lib.KMVP_F32}


def set_diagonal(ctx, name):
    s = kr.SYSTEMS[name]
    if s.d is not None:
        ctx.set_solver_diagonal(s.d, s.ridge)
    else:
        ctx.set_solver_diagonal(None, s.ridge)


def open_context(name, precision="float64"):
    ctx = _lib.Context(0)
    try:
        ctx.set_points(kr.points(name, precision), None, CODES[precision])
        set_diagonal(ctx, name)
    except Exception:
        ctx.close()
        raise
    return ctx


def gpu_solve(name, a, rtol, maxit, precision="float64"):
    ctx = open_context(name, precision)
    try:
        return ctx.cg_solve(kr.SYSTEMS[name].kernel, a, rtol, maxit)
    finally:
        ctx.close()


def check(label, name, E, rtol, maxit, result, precision="float64", resid_rule=True):
    """iters, x and resid of one solve against the restatement's trace of the same case; returns the trace."""
    x, iters, resid, ok = result
    t = kr.trace(name, E, rtol, maxit, precision)
    A, kappa = kr.matrix(name, precision)
    err, tol = kr.column_error(x, t.x), kr.tolerance(name, rtol, precision)
    numpy_resid = float(np.max(kr.true_residual(A, x, kr.rhs(E, precision))))
    print(f"[{label}] {name} {precision} E={E} rtol={rtol:g} maxit={maxit}: iters {iters} (reference {t.iters}) ok {ok} "
          f"resid {resid:.6g} (numpy {numpy_resid:.6g}, bound {kappa * 1e-11:.2g}) error {err:.3g} tolerance {tol:.3g}")
    assert iters == t.iters, (iters, t.iters)
    assert np.all(np.isfinite(x)) and np.isfinite(resid)
    if E == 4:
        assert not x[:, 3].any(), "the zero column is not exactly 0"
    assert err <= tol, (err, tol)
    if resid_rule:
        assert abs(resid - numpy_resid) <= kappa * 1e-11, (resid, numpy_resid)
    return t


@pytest.mark.parametrize("E", ES)
@pytest.mark.parametrize("name, rtol", [(s, rtol) for s in kr.STOPPING for rtol in kr.SYSTEMS[s].rtols])
def test_stops_at_the_first_iteration_that_meets_the_tolerance(name, rtol, E):
    """a. float64, maxit 1000: converged, the restatement's count, its iterate at that count, the true residual.
    (The MINRES cases are the regression test of the stop word's MS_MET state: with the x update of the stopping
    iteration skipped, Id+- at 1e-4 returned x_11 with the count 12 and a true residual of 3.6e-4.)"""
    result = gpu_solve(name, kr.rhs(E), rtol, 1000)
    check("a", name, E, rtol, 1000, result)
    assert result[3] and result[2] <= 1.5 * rtol, result[1:]


@pytest.mark.parametrize("E", ES)
@pytest.mark.parametrize("name, maxit", [(s, m) for s in ("G30", "Ed", "Id+-", "I0") for m in kr.MAXIT_CASES[s]])
def test_stops_on_maxit_with_that_iterate(name, maxit, E):
    """b. an unreachable tolerance: exactly maxit iterations (inside a burst, at its end, one past it, in the third),
    not converged, x_maxit."""
    result = gpu_solve(name, kr.rhs(E), kr.UNREACHABLE, maxit)
    check("b", name, E, kr.UNREACHABLE, maxit, result)
    assert result[1] == maxit and not result[3], result[1:]


@pytest.mark.parametrize("name", ("G30", "Id+-"))
def test_maxit_zero(name):
    x, iters, resid, ok = gpu_solve(name, kr.rhs(4), 1e-8, 0)
    print(f"[b] {name} maxit=0: iters {iters} resid {resid!r} ok {ok}")
    assert iters == 0 and not x.any() and resid == 1.0 and not ok


@pytest.mark.parametrize("name", ("G30", "Id+-"))
def test_degenerate_right_hand_sides(name):
    """c. an all-zero right-hand side is solved by x = 0 without an iteration; one NaN in one column of three is never
    a success."""
    x, iters, resid, ok = gpu_solve(name, np.zeros((kr.N, 2)), 1e-8, 1000)
    print(f"[c] {name} zero right-hand side: iters {iters} resid {resid!r} ok {ok}")
    assert ok and iters == 0 and resid == 0.0 and not x.any()
    a = kr.rhs(4)[:, :3].copy()
    a[5, 1] = np.nan
    x, iters, resid, ok = gpu_solve(name, a, 1e-8, 50)
    print(f"[c] {name} NaN in column 1: iters {iters} resid {resid!r} ok {ok}")
    assert not ok and not np.isfinite(resid)


@pytest.mark.parametrize("E", ES)
@pytest.mark.parametrize("name", kr.FLOAT32)
def test_float32_context(name, E):
    """d. points and right-hand side rounded to float32, the restatement on the matrix of the rounded points: the same
    count and the iterate within the float32 tolerance.  (The library's residual is of its float32 operator: it is
    printed, not compared.  At rtol = 1e-4 every later iterate lies within kappa 1e-4 of x_k, about one float32
    tolerance: here it is the count, not the iterate, that tells the first iteration from the end of the burst.)"""
    result = gpu_solve(name, kr.rhs(E, "float32"), 1e-4, 1000, "float32")
    check("d", name, E, 1e-4, 1000, result, "float32", resid_rule=False)


def test_one_context_three_solves_leave_nothing_behind():
    """e. to a tolerance, to maxit = 9, to the tolerance again on one context: the first and the third bitwise equal
    (no stop word, count or state survives a solve), each of the three as in a / b."""
    name, rtol = "G30", kr.SYSTEMS["G30"].rtols[1]
    ctx = open_context(name)
    try:
        first = ctx.cg_solve("gaussian", kr.rhs(4), rtol, 1000)
        second = ctx.cg_solve("gaussian", kr.rhs(4), kr.UNREACHABLE, 9)
        third = ctx.cg_solve("gaussian", kr.rhs(4), rtol, 1000)
    finally:
        ctx.close()
    check("e", name, 4, rtol, 1000, first)
    check("e", name, 4, kr.UNREACHABLE, 9, second)
    assert np.array_equal(first[0], third[0]) and first[1:] == third[1:], (first[1:], third[1:])


def test_diagonal_set_then_cleared_on_one_context():
    """e. Ed with its per-point diagonal, then the diagonal switched off and three iterations on the bare exp(-r)
    matrix of the same points (E0): nothing of the diagonal is left."""
    ctx = open_context("Ed")
    try:
        with_d = ctx.cg_solve("absolute-exponential", kr.rhs(4), 1e-4, 1000)
        ctx.set_solver_diagonal(None, 0.0)
        bare = ctx.cg_solve("absolute-exponential", kr.rhs(4), kr.UNREACHABLE, 3)
    finally:
        ctx.close()
    check("e", "Ed", 4, 1e-4, 1000, with_d)
    check("e", "E0", 4, kr.UNREACHABLE, 3, bare)
    assert with_d[3] and not bare[3]
