"""Regularised solves (K + ridge I + diag(d)) b = a on the GPU (-m gpu): kmvp_set_solver_diagonal and MI355XSolver(ridge=).

Ground truth everywhere is dense numpy in float64 on the inputs as the working precision sees them: K from the formulas
of oracle/kmvp_oracle.py, A = K + diag, numpy.linalg.solve.  With a ridge the systems are well posed, so a solve is held
to the dense SOLUTION VECTOR, not only to its residual:

    ||b - b_dense|| / ||b_dense||  <=  kappa 1.5 rtol + kappa 1e-11,      kappa = cond(A) from numpy.linalg.eigvalsh

(first term: the residual rule of include/kmvp.h, a relative residual of 1.5 rtol moves the solution by at most kappa
times that; second: the float64 operator tolerance of DESIGN.md section 4).  For these systems kappa ~ 1e4, so the bound
is ~2e-6 -- loose by design: a ridge applied twice, per rank, or not at all moves b by O(1).
"""
import json
import os

import numpy as np
import pytest

import kmvp_oracle
from kernel_matrix_benchmarks_amd import _lib
from kernel_matrix_benchmarks_amd.algorithms.mi355x import MI355XSolver
from test_gpu_multirank import _spawn

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
N, D = 2000, 3


def cube(n=N, seed=11):
    return np.random.RandomState(seed).rand(n, D)


def rhs(E, n=N, seed=13):
    return np.random.RandomState(seed).randn(n, E)


def dense_system(kernel, y, diag):
    """A = K + diag in float64 and its condition number max|lambda| / min|lambda| (A is symmetric)."""
    A = kmvp_oracle.kernel_matrix(kernel=kernel, source_points=np.asarray(y, dtype=np.float64))
    A = A + np.diag(np.broadcast_to(np.asarray(diag, dtype=np.float64), (A.shape[0],)))
    w = np.abs(np.linalg.eigvalsh(A))
    return A, float(w.max() / w.min())


def residual_of(A, b, a):
    a = np.asarray(a, dtype=np.float64)
    return float(np.max(np.linalg.norm(A @ b - a, axis=0) / np.linalg.norm(a, axis=0)))


def vector_error(A, b, a):
    dense = np.linalg.solve(A, np.asarray(a, dtype=np.float64))
    return float(np.max(np.linalg.norm(b - dense, axis=0) / np.linalg.norm(dense, axis=0)))


def vector_bound(kappa, rtol):
    return kappa * 1.5 * rtol + kappa * 1e-11


def plugin_solve(kernel, y, a, precision=np.float64, **kwargs):
    algo = MI355XSolver(kernel=kernel, dimension=y.shape[1], precision=precision, **kwargs)
    try:
        algo.prepare_data(source_points=y)
        algo.fit()
        algo.prepare_query(target_signal=a)
        algo.query()
        return algo.get_result(), algo.get_additional()
    finally:
        algo.done()


@pytest.mark.parametrize("E", [1, 3])
@pytest.mark.parametrize("kernel", ["gaussian", "absolute-exponential"])
def test_ridge_solution_vector_against_the_dense_solve(kernel, E):
    """Check 1: float64, ridge = 0.1, rtol = 1e-10.  The iteration cap catches a silently ignored ridge: dense CG needs
    69 (Gaussian) / 170 (exp(-r)) iterations on these systems, and the bare Gaussian system does not converge at all."""
    y, a, rtol = cube(), rhs(E), 1e-10
    A, kappa = dense_system(kernel, y, 0.1)
    b, info = plugin_solve(kernel, y, a, rtol=rtol, maxit=5000, ridge=0.1)
    err, bound = vector_error(A, b, a), vector_bound(kappa, rtol)
    print(f"{kernel} E={E}: kappa {kappa:.3g} iterations {info['cg_iterations']} residual {info['cg_relative_residual']:.3g} "
          f"(numpy: {residual_of(A, b, a):.3g}) vector error {err:.3g} bound {bound:.3g}")
    assert info["cg_converged"] and info["ridge"] == 0.1, info
    assert err <= bound, (err, bound, info)
    assert info["cg_iterations"] <= 400, info
    assert residual_of(A, b, a) <= 2 * rtol  # the residual keys describe the regularised system


@pytest.mark.parametrize("E", [1, 3])
@pytest.mark.parametrize("kernel", ["gaussian", "absolute-exponential"])
def test_ridge_float32_true_residual(kernel, E):
    """Check 2: float32 operator, rtol = 1e-4; the true residual of the regularised system, recomputed in numpy float64
    from the returned b on the inputs as float32 holds them."""
    y32, a32, rtol = cube().astype(np.float32), rhs(E).astype(np.float32), 1e-4
    A, kappa = dense_system(kernel, y32, 0.1)
    b, info = plugin_solve(kernel, y32, a32, precision="float32", rtol=rtol, maxit=5000, ridge=0.1)
    res = residual_of(A, b, a32)
    print(f"{kernel} float32 E={E}: kappa {kappa:.3g} iterations {info['cg_iterations']} residual {info['cg_relative_residual']:.3g} numpy {res:.3g}")
    assert info["cg_converged"], info
    assert res <= 2 * rtol, (res, info)


@pytest.mark.parametrize("E", [1, 3])
@pytest.mark.parametrize("ridge", [0.0, 0.05])
@pytest.mark.parametrize("kernel", ["gaussian", "absolute-exponential"])
def test_per_point_diagonal_with_and_without_a_ridge_on_top(kernel, ridge, E):
    """Check 3: d = uniform(0.05, 0.2) per point (heteroscedastic noise), through the C ABI so that ridge and d add up.
    Check 1's rule with A's own kappa, and its iteration cap (dense CG in numpy: 80 .. 193 iterations on these four)."""
    y, a, rtol = cube(), rhs(E), 1e-10
    d = np.random.RandomState(12).uniform(0.05, 0.2, N)
    A, kappa = dense_system(kernel, y, ridge + d)
    ctx = _lib.Context(0)
    try:
        ctx.set_points(y, None, _lib.KMVP_F64)
        ctx.set_solver_diagonal(d, ridge)
        b, iters, resid, ok = ctx.cg_solve(kernel, a, rtol, 5000)
    finally:
        ctx.close()
    err, bound = vector_error(A, b, a), vector_bound(kappa, rtol)
    print(f"{kernel} d + {ridge} E={E}: kappa {kappa:.3g} iterations {iters} residual {resid:.3g} vector error {err:.3g} bound {bound:.3g}")
    assert ok and iters <= 400, (iters, resid)
    assert err <= bound, (err, bound)
    if ridge == 0.0:  # the plugin's per-point form is the same call: bitwise the same solve
        b2, info = plugin_solve(kernel, y, a, rtol=rtol, maxit=5000, ridge=d)
        assert np.array_equal(b, b2) and info["cg_iterations"] == iters and info["ridge"] == d.max()


@pytest.mark.parametrize("E", [1, 3])
def test_minres_with_a_shift_of_either_sign(E):
    """Check 4: inverse-distance on the sphere (the cloud of the existing solver tests), ridge = +10 and -10, float64,
    rtol = 1e-8: the true residual rule for both, and the vector rule wherever its bound still says something
    (kappa 1.5 rtol <= 1e-2)."""
    y, a, rtol = kmvp_oracle.uniform_sphere_points(N), rhs(E), 1e-8
    compared = 0
    for ridge in (10.0, -10.0):
        A, kappa = dense_system("inverse-distance", y, ridge)
        b, info = plugin_solve("inverse-distance", y, a, rtol=rtol, maxit=20000, ridge=ridge)
        res, err, bound = residual_of(A, b, a), vector_error(A, b, a), vector_bound(kappa, rtol)
        print(f"inverse-distance ridge {ridge} E={E}: kappa {kappa:.3g} iterations {info['cg_iterations']} residual "
              f"{info['cg_relative_residual']:.3g} numpy {res:.3g} vector error {err:.3g} bound {bound:.3g}")
        assert info["cg_converged"] and info["ridge"] == ridge, info
        assert res <= 2 * rtol, (ridge, res, info)
        if kappa * 1.5 * rtol <= 1e-2:
            compared += 1
            assert err <= bound, (ridge, err, bound)
    assert compared >= 1


def test_refusals_through_the_c_abi():
    """Check 5: KMVP_E_INVALID with a message -- a negative effective diagonal on a CG entry, a wrong n, non-finite
    values; (NULL, 0, 0.0) switches the diagonal off again."""
    y, a = cube(500), rhs(1, 500)
    ctx = _lib.Context(0)
    try:
        ctx.set_points(y, None, _lib.KMVP_F64)
        fresh = ctx.cg_solve("absolute-exponential", a, 1e-8, 2000)

        def refused(call):
            with pytest.raises(_lib.KmvpError) as e:
                call()
            assert e.value.code == 1 and "diagonal" in str(e.value), str(e.value)

        for kernel in ("gaussian", "absolute-exponential"):
            ctx.set_solver_diagonal(None, -0.1)
            refused(lambda: ctx.cg_solve(kernel, a, 1e-8, 10))
            d = np.full(500, 0.2)
            d[123] = -0.3
            ctx.set_solver_diagonal(d, 0.2)  # 0.2 - 0.3 < 0 at one point
            refused(lambda: ctx.cg_solve(kernel, a, 1e-8, 10))
            d[123] = -0.2
            ctx.set_solver_diagonal(d, 0.2)  # exactly 0 there: semi-definite shift, allowed
            assert ctx.cg_solve("absolute-exponential", a, 1e-8, 2000)[3]
        for wrong in (499, 501):
            ctx.set_solver_diagonal(np.full(wrong, 0.1), 0.0)
            for kernel in ("gaussian", "inverse-distance"):
                refused(lambda: ctx.cg_solve(kernel, a, 1e-8, 10))
        ctx.set_solver_diagonal(None, 0.1)
        for bad_d, bad_ridge in ((None, float("nan")), (None, float("inf")), (np.full(500, np.nan), 0.0),
                                 (np.r_[np.zeros(499), np.inf], 0.0), (np.full(500, 1e308), 1e308)):
            refused(lambda: ctx.set_solver_diagonal(bad_d, bad_ridge))
        lib = _lib.load()
        assert lib.kmvp_set_solver_diagonal(ctx._ctx, None, 5, 0.1) == 1  # n values announced, none passed
        assert lib.kmvp_set_solver_diagonal(ctx._ctx, np.zeros(4).ctypes.data, -4, 0.1) == 1
        # a refused call leaves the diagonal that was set before: ridge = 0.1
        A, _ = dense_system("absolute-exponential", y, 0.1)
        b, iters, resid, ok = ctx.cg_solve("absolute-exponential", a, 1e-8, 2000)
        assert ok and residual_of(A, b, a) <= 2e-8
        ctx.set_solver_diagonal(None, 0.0)
        again = ctx.cg_solve("absolute-exponential", a, 1e-8, 2000)
        assert np.array_equal(again[0], fresh[0]) and again[1:] == fresh[1:]
    finally:
        ctx.close()


@pytest.mark.parametrize("kernel", ["gaussian", "inverse-distance"])
def test_nothing_changes_with_the_diagonal_off(kernel):
    """Check 6: the same solve on a fresh context, after setting and clearing a diagonal, and after set_points cleared it:
    b, iterations and resid bitwise equal; a product with a diagonal set equals the product without."""
    y = cube() if kernel == "gaussian" else kmvp_oracle.uniform_sphere_points(N)
    a, b_signal = rhs(3), rhs(2, seed=14)
    d = np.random.RandomState(12).uniform(0.05, 0.2, N)

    def solve(ctx):  # (the bare Gaussian system does not converge: 150 iterations of it are as deterministic as any)
        return ctx.cg_solve(kernel, a, 1e-8, 150 if kernel == "gaussian" else 5000)

    def product(ctx):
        ctx.set_signal(b_signal)
        ctx.run(kernel, False)
        return ctx.get_result(N, 2)

    runs, products = [], []
    for how in ("fresh", "set and cleared", "cleared by set_points"):
        ctx = _lib.Context(0)
        try:
            ctx.set_points(y, None, _lib.KMVP_F64)
            if how == "fresh":
                products.append(product(ctx))
            elif how == "set and cleared":
                ctx.set_solver_diagonal(d, 0.3)
                products.append(product(ctx))  # products are not affected
                with_diag = solve(ctx)
                ctx.set_solver_diagonal(None, 0.0)
            else:
                ctx.set_solver_diagonal(d, 0.3)
                ctx.set_points(y, None, _lib.KMVP_F64)
            runs.append(solve(ctx))
        finally:
            ctx.close()
    assert np.array_equal(products[0], products[1])
    for b, iters, resid, ok in runs[1:]:
        assert np.array_equal(b, runs[0][0]) and iters == runs[0][1] and resid == runs[0][2] and ok == runs[0][3]
    assert not np.array_equal(with_diag[0], runs[0][0])  # (and the diagonal did do something while it was set)


def test_long_cg_graph_replay_with_the_diagonal():
    """Check 7, as test_long_cg_graph_replay_equals_plain_launches does it (the burst is captured after 64 bursts of 8 =
    512 iterations): the diagonal's pointer and scalar are fixed for the solve, so the replayed burst gives the same
    iterates as launch by launch.  (MINRES does not go through the burst graph: nothing to replay there.)"""
    n = 1200
    y, _ = kmvp_oracle.uniform_cube(n, 3)
    y = y * 4.0
    a = rhs(1, n)
    d = np.random.RandomState(12).uniform(0.0, 1e-3, n)
    outs = []
    for no_graph in (False, True):
        if no_graph:
            os.environ["KMVP_NO_GRAPH"] = "1"
        else:
            os.environ.pop("KMVP_NO_GRAPH", None)
        ctx = _lib.Context(0)
        try:
            ctx.set_points(y, None, _lib.KMVP_F64)
            ctx.set_solver_diagonal(d, 1e-3)
            sol, iters, resid, ok = ctx.cg_solve("gaussian", a, 1e-15, 700)  # unreachable tolerance: runs to maxit
        finally:
            ctx.close()
            os.environ.pop("KMVP_NO_GRAPH", None)
        assert iters == 700
        outs.append(sol)
    assert np.array_equal(outs[0], outs[1])


@pytest.mark.parametrize("E", [1, 3])
def test_refinement_on_float32_with_a_ridge(E):
    """Check 8: refine="float32" -- the inner float32 context iterates on the same regularised operator, the outer
    float64 residual is a - (K x + ridge x); it must end on the tolerance and meet check 1's vector rule."""
    y, a, rtol = cube(), rhs(E), 1e-10
    A, kappa = dense_system("gaussian", y, 0.1)
    b, info = plugin_solve("gaussian", y, a, rtol=rtol, maxit=5000, ridge=0.1, refine="float32")
    err, bound = vector_error(A, b, a), vector_bound(kappa, rtol)
    print(f"refined E={E}: {info['refinement_steps']} steps, {info['cg_iterations']} inner iterations, residual "
          f"{info['cg_relative_residual']:.3g} vector error {err:.3g} bound {bound:.3g}")
    assert info["cg_converged"] and info["refinement_stop_reason"] == "tolerance", info
    assert err <= bound, (err, bound, info)
    assert residual_of(A, b, a) <= 2 * rtol


@pytest.mark.parametrize("E", [1, 3])
def test_exp_dot_with_a_ridge(E):
    """Check 9: (K + lambda I) b = a with K = exp(<x_i, x_j>), float64, through the Gaussian identity (the library gets
    lambda exp(-|x|^2) per point).  The unit cube: |x|^2/2 spans 1.5 (< 5), so the scaled system CG iterates on and the
    unscaled one the verdict is about differ by a modest diagonal scaling.  True residual in numpy."""
    x, a, rtol, lam = cube(), rhs(E), 1e-8, 0.1
    A = np.exp(x @ x.T) + lam * np.eye(N)
    b, info = plugin_solve("exp-dot", x, a, rtol=rtol, maxit=20000, ridge=lam)
    res = residual_of(A, b, a)
    print(f"exp-dot E={E}: iterations {info['cg_iterations']} residual {info['cg_relative_residual']:.3g} (scaled system "
          f"{info['cg_scaled_system_residual']:.3g}) numpy {res:.3g}")
    assert res <= 2 * rtol, (res, info)
    assert abs(info["cg_relative_residual"] - res) <= 0.5 * res + 1e-12, (res, info)  # the plugin's verdict includes the term


def test_two_ranks_on_one_gpu_solve_the_regularised_system():
    """Check 10: two ranks on GPU 0 through the host-staged exchange, uneven source shards: the diagonal is added once,
    after the all-reduce, so both ranks return bitwise the same b and it meets check 1 against the dense solve."""
    out = _spawn([os.path.join(HERE, "_ridge_rank_worker.py")], world=2, timeout=600)
    rep = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
    print(json.dumps(rep))
    assert rep["world"] == 2 and rep["shards"] == [[0, 1300], [1300, 2000]]
    assert len(rep["cases"]) == 2
    for case in rep["cases"]:
        assert case["ranks_bitwise_equal"] and case["converged"], case
        assert case["vector_error"] <= case["bound"] and case["iterations"] <= 400, case
