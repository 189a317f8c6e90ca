"""The pivoted-Cholesky preconditioner of the CG solvers on the GPU (-m gpu): kmvp_set_solver_preconditioner,
kmvp_get_solver_preconditioner and MI355XSolver(preconditioner_rank=), held to the float64 restatement of
precond_reference.py on its 384-point systems.

    factor     read back and compared with the restatement FOLLOWING THE DEVICE'S PIVOTS (no re-derived argmax: two nearly
               equal residual diagonals may be ordered either way), each column within 4 g_factor TOL of its norm, and each
               pivot within twice that of the maximum of the restatement's residual diagonal
    iterates   float64: after 1, 2, 3, 8, 9 iterations the restatement's iterate, the restatement fed the device's own L,
               within 4 g TOL (TOL = 1e-11 float64 / 1e-5 float32, g and g_factor measured by test_precond_reference.py;
               why not in float32: precond_reference.SYSTEMS)
    counts     at the table's tolerances the restatement's count and a true residual <= 1.5 rtol against the dense matrix
"""
import json
import os

import numpy as np
import pytest

import kmvp_oracle
import krylov_reference as kr
import precond_reference as pr
from kernel_matrix_benchmarks_amd import _lib
from kernel_matrix_benchmarks_amd.algorithms.mi355x import MI355XSolver
from test_gpu_multirank import _spawn

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CODES = {"float64": _lib.KMVP_F64, "float32": _lib.KMVP_F32}
PRECISIONS = [(s, p) for s in pr.SYSTEMS for p in (pr.F64, pr.F32) if p == pr.F64 or s in pr.FLOAT32]


def open_context(name, precision="float64", rank=pr.RANK):
    ctx = _lib.Context(0)
    try:
        ctx.set_points(pr.points(name, precision), None, CODES[precision])
        ctx.set_solver_diagonal(pr.DIAG, 0.0)
        ctx.set_solver_preconditioner(rank)
    except Exception:
        ctx.close()
        raise
    return ctx


def solve(name, E, rtol, maxit, precision="float64", rank=pr.RANK):
    """(x, iters, resid, ok), (rank_built, pivots, L), build ms of one solve on a context of its own."""
    ctx = open_context(name, precision, rank)
    try:
        result = ctx.cg_solve(pr.SYSTEMS[name].kernel, pr.rhs(E, precision), rtol, maxit)
        return result, ctx.get_solver_preconditioner(), ctx.last_preconditioner_ms
    finally:
        ctx.close()


@pytest.mark.parametrize("name, precision", PRECISIONS)
def test_factor_against_the_restatement_on_the_devices_pivots(name, precision):
    """4. (G12: D = 12, the column kernel's runtime loop over the coordinates.)"""
    _, (built, piv, L), ms = solve(name, 1, pr.UNREACHABLE, 1, precision)
    assert built == pr.RANK and L.shape == (pr.RANK, pr.N) and ms > 0
    assert len(set(piv.tolist())) == pr.RANK and piv.min() >= 0 and piv.max() < pr.N
    ref, _, before = pr.pivoted_cholesky(pr.kernel_matrix(name, precision), pr.RANK, pr.TAU[precision], pivots=piv)
    err, tol = pr.factor_error(L, ref), pr.factor_tolerance(name, precision)
    short = max(before[m].max() - before[m][piv[m]] for m in range(pr.RANK))
    own = pr.factor(name, precision)[1]
    print(f"{name} {precision}: factor error {err:.3g} tolerance {tol:.3g}; pivots short of the maximum by {short:.3g} "
          f"(allowed {2 * tol:.3g}); {int((piv == own).sum())} of {pr.RANK} pivots are the restatement's own; build {ms:.2f} ms")
    assert np.all(np.isfinite(L))
    assert err <= tol, (err, tol)
    assert short <= 2 * tol, (short, tol)
    assert piv[0] == 0  # d = 1 everywhere: the tie goes to the smallest index


@pytest.mark.parametrize("E", [1, 3])
@pytest.mark.parametrize("maxit", pr.MAXITS)
@pytest.mark.parametrize("name", list(pr.SYSTEMS))
def test_iterates_against_the_restatement_fed_the_devices_factor(name, maxit, E):
    """5. float64.  maxit = 1 is the apply on its own (x_1 = alpha P^-1 a); 8 ends the first burst, 9 is one past it."""
    (x, iters, resid, ok), (built, piv, L), _ = solve(name, E, pr.UNREACHABLE, maxit)
    t = pr.trace(name, E, pr.UNREACHABLE, maxit, L=L)
    err, tol = kr.column_error(x, t.x), pr.tolerance(name)
    print(f"{name} E={E} maxit={maxit}: iters {iters} error {err:.3g} tolerance {tol:.3g} resid {resid:.3g}")
    assert iters == maxit == t.iters and not ok and built == pr.RANK
    assert np.all(np.isfinite(x)) and np.isfinite(resid)
    if E == 3:
        assert not x[:, 2].any(), "the zero column is not exactly 0"
    assert err <= tol, (err, tol)


@pytest.mark.parametrize("E", [1, 3])
@pytest.mark.parametrize("name, rtol", [(s, rtol) for s in pr.SYSTEMS for rtol in pr.SYSTEMS[s].rtols])
def test_stops_at_the_restatements_count(name, rtol, E):
    """5. float64: the restatement's count (fed the device's L), converged, and the true residual against the dense matrix."""
    (x, iters, resid, ok), (built, piv, L), _ = solve(name, E, rtol, 1000)
    t = pr.trace(name, E, rtol, 1000, L=L)
    A, kappa = pr.matrix(name)
    numpy_resid = float(np.max(kr.true_residual(A, x, pr.rhs(E))))
    print(f"{name} E={E} rtol={rtol:g}: iters {iters} (restatement {t.iters}) resid {resid:.6g} (numpy {numpy_resid:.6g})")
    assert iters == t.iters, (iters, t.iters)
    assert ok and resid <= 1.5 * rtol and numpy_resid <= 1.5 * rtol
    assert abs(resid - numpy_resid) <= kappa * 1e-11
    if E == 3:
        assert not x[:, 2].any()


@pytest.mark.parametrize("name", pr.FLOAT32)
def test_float32_context_end_of_a_solve(name):
    """float32 operator, rtol = 1e-2: converged with the true residual of the float32 points' matrix, recomputed in
    float64, within 1.5 rtol, in fewer iterations than without the preconditioner.  (A float32 product errs by about
    eps |K| |x| <= 6e-8 x 150 x 100 |a| = 1e-3 |a| here -- |K| <= 150, |x| <= |a| / 0.01 --, so 1e-2 is within reach of
    the operator whatever the path.)"""
    rtol = 1e-2
    (_, plain, _, ok0), _, _ = solve(name, 3, rtol, 2000, pr.F32, rank=0)
    (x, iters, resid, ok), (built, _, _), _ = solve(name, 3, rtol, 2000, pr.F32)
    A, _ = pr.matrix(name, pr.F32)
    numpy_resid = float(np.max(kr.true_residual(A, x, pr.rhs(3, pr.F32))))
    print(f"{name} float32: {plain} iterations plain, {iters} with rank {built}; resid {resid:.3g} numpy {numpy_resid:.3g}")
    assert ok0 and ok and built == pr.RANK and iters < plain
    assert numpy_resid <= 1.5 * rtol and not x[:, 2].any()


@pytest.mark.parametrize("name", pr.CUBE)
def test_at_most_half_the_iterations(name):
    """6. The device's own counts to 1e-8, rank 32 against rank 0."""
    (_, plain, resid0, ok0), (built0, _, _), ms0 = solve(name, 1, pr.RATIO_RTOL, 5000, rank=0)
    (_, fewer, resid, ok), (built, _, _), _ = solve(name, 1, pr.RATIO_RTOL, 5000)
    print(f"{name}: {plain} iterations plain, {fewer} with rank {built} (ratio {plain / fewer:.2f})")
    assert ok0 and ok and built0 == 0 and ms0 == 0.0 and built == pr.RANK
    assert 2 * fewer <= plain, (fewer, plain)


def test_nothing_changes_when_off():
    """7. A fresh context, one that had the preconditioner on for a solve and off again, one where set_points cleared it:
    bitwise the same solve; products are not affected; and the preconditioner did do something while it was on."""
    name, kernel = "G", "gaussian"
    y, a, signal = pr.points(name), pr.rhs(3), np.random.RandomState(14).randn(pr.N, 2)

    def product(ctx):
        ctx.set_signal(signal)
        ctx.run(kernel, False)
        return ctx.get_result(pr.N, 2)

    runs, products = [], []
    for how in ("fresh", "set and cleared", "cleared by set_points"):
        ctx = _lib.Context(0)
        try:
            ctx.set_points(y, None, _lib.KMVP_F64)
            ctx.set_solver_diagonal(pr.DIAG, 0.0)
            if how == "fresh":
                products.append(product(ctx))
            elif how == "set and cleared":
                ctx.set_solver_preconditioner(32)
                products.append(product(ctx))
                with_p = ctx.cg_solve(kernel, a, 1e-8, 1000)
                assert ctx.get_solver_preconditioner()[0] == 32
                ctx.set_solver_preconditioner(0)
            else:
                ctx.set_solver_preconditioner(32)
                ctx.set_points(y, None, _lib.KMVP_F64)
                ctx.set_solver_diagonal(pr.DIAG, 0.0)
            runs.append(ctx.cg_solve(kernel, a, 1e-8, 1000))
            assert ctx.get_solver_preconditioner()[0] == 0 and ctx.last_preconditioner_ms == 0.0
        finally:
            ctx.close()
    assert np.array_equal(products[0], products[1])
    for b, iters, resid, ok in runs[1:]:
        assert np.array_equal(b, runs[0][0]) and (iters, resid, ok) == runs[0][1:]
    assert with_p[3] and runs[0][3] and with_p[1] < runs[0][1]
    assert not np.array_equal(with_p[0], runs[0][0])


def test_reuse_and_invalidation():
    """8. The factor is kept across solves and rebuilt when the diagonal, the kernel or the rank changes; every solve is
    bitwise reproducible, on one context and from context to context."""
    a = pr.rhs(3)
    ctx = open_context("G")
    try:
        first = ctx.cg_solve("gaussian", a, 1e-8, 1000)
        ms_first, factor_first = ctx.last_preconditioner_ms, ctx.get_solver_preconditioner()
        bytes_with = ctx.device_bytes
        second = ctx.cg_solve("gaussian", a, 1e-8, 1000)
        assert ms_first > 0 and ctx.last_preconditioner_ms == 0.0
        assert np.array_equal(first[0], second[0]) and first[1:] == second[1:]
        assert bytes_with >= 8 * pr.RANK * pr.N  # kmvp_device_bytes counts the factor
        rebuilt = []
        for change in (lambda: ctx.set_solver_diagonal(pr.DIAG, 0.05), lambda: None, lambda: ctx.set_solver_preconditioner(16)):
            change()
            kernel = "matern-5/2" if len(rebuilt) == 1 else "gaussian"
            out = ctx.cg_solve(kernel, a, 1e-8, 1000)
            rebuilt.append((ctx.last_preconditioner_ms, ctx.get_solver_preconditioner()[0], out))
            again = ctx.cg_solve(kernel, a, 1e-8, 1000)
            assert ctx.last_preconditioner_ms == 0.0 and np.array_equal(again[0], out[0]) and again[1:] == out[1:]
        print("rebuilds:", [(f"{ms:.2f} ms", built, out[1]) for ms, built, out in rebuilt])
        assert all(ms > 0 and out[3] for ms, _, out in rebuilt)
        assert [built for _, built, _ in rebuilt] == [32, 32, 16]
        assert rebuilt[0][2][1] < first[1]  # a larger diagonal: fewer iterations, so the factor's C was rebuilt with it
    finally:
        ctx.close()
    other, factor_other, _ = solve("G", 3, 1e-8, 1000)
    assert np.array_equal(other[0], first[0]) and other[1:] == first[1:]
    assert all(np.array_equal(u, v) for u, v in zip(factor_first, factor_other))


def test_long_pcg_graph_replay():
    """9. As test_long_cg_graph_replay_with_the_diagonal: the burst is captured after 64 bursts of 8; the factor, the
    uploaded Cholesky factor and the scratch are fixed for the solve, so the replayed burst gives the same iterates."""
    n = 1200
    y, _ = kmvp_oracle.uniform_cube(n, 3)
    y = y * 4.0
    a = np.random.RandomState(13).randn(n, 1)
    d = np.random.RandomState(12).uniform(1e-3, 2e-3, n)
    outs = []
    for no_graph in (False, True):
        if no_graph:
            os.environ["KMVP_NO_GRAPH"] = "1"
        else:
            os.environ.pop("KMVP_NO_GRAPH", None)
        ctx = _lib.Context(0)
        try:
            ctx.set_points(y, None, _lib.KMVP_F64)
            ctx.set_solver_diagonal(d, 0.0)
            ctx.set_solver_preconditioner(16)
            sol, iters, resid, ok = ctx.cg_solve("gaussian", a, 1e-15, 700)  # unreachable tolerance: runs to maxit
            assert ctx.get_solver_preconditioner()[0] == 16
        finally:
            ctx.close()
            os.environ.pop("KMVP_NO_GRAPH", None)
        assert iters == 700
        outs.append(sol)
    assert np.all(np.isfinite(outs[0])) and np.array_equal(outs[0], outs[1])


def test_refusals_through_the_c_abi():
    """10. A refused call leaves the previous setting in place."""
    y, a = pr.points("G"), pr.rhs(1)
    ctx = _lib.Context(0)
    try:
        ctx.set_points(y, None, _lib.KMVP_F64)
        ctx.set_solver_diagonal(pr.DIAG, 0.0)
        ctx.set_solver_preconditioner(8)
        good = ctx.cg_solve("gaussian", a, 1e-8, 1000)
        assert good[3] and ctx.get_solver_preconditioner()[0] == 8

        def refused(call, code):
            with pytest.raises(_lib.KmvpError) as e:
                call()
            assert e.value.code == code and "preconditioner" in str(e.value), str(e.value)

        refused(lambda: ctx.set_solver_preconditioner(-1), 1)
        refused(lambda: ctx.set_solver_preconditioner(129), 2)
        again = ctx.cg_solve("gaussian", a, 1e-8, 1000)  # still rank 8
        assert ctx.get_solver_preconditioner()[0] == 8 and np.array_equal(again[0], good[0]) and again[1:] == good[1:]
        ctx.set_solver_preconditioner(128)  # the largest rank is accepted
        ctx.set_solver_preconditioner(8)
        ctx.set_solver_diagonal(None, 0.0)  # no diagonal
        refused(lambda: ctx.cg_solve("gaussian", a, 1e-8, 10), 1)
        d = pr.DIAG.copy()
        d[123] = 0.0
        ctx.set_solver_diagonal(d, 0.0)  # 0 at one point: fine for plain CG, not for P
        refused(lambda: ctx.cg_solve("gaussian", a, 1e-8, 10), 1)
        d[123] = -0.5
        ctx.set_solver_diagonal(d, 0.5)  # ridge + d_i == 0 there
        refused(lambda: ctx.cg_solve("matern-3/2", a, 1e-8, 10), 1)
        assert ctx.get_solver_preconditioner()[0] == 0  # the refused solve used none
        ctx.set_solver_diagonal(pr.DIAG, 0.0)
        refused(lambda: ctx.cg_solve("inverse-distance", a, 1e-8, 10), 2)  # MINRES
        last = ctx.cg_solve("gaussian", a, 1e-8, 1000)  # the setting survived all of it
        assert np.array_equal(last[0], good[0]) and last[1:] == good[1:]
        ctx.set_solver_preconditioner(0)
        assert ctx.cg_solve("inverse-distance", a, 1e-6, 2000)[1] > 0  # MINRES runs again with the preconditioner off
    finally:
        ctx.close()


def test_plugin_refusals():
    """10. NotImplementedError for the kernels and modes without a preconditioner, ValueError without a ridge."""
    for kwargs in (dict(kernel="inverse-distance", ridge=0.1), dict(kernel="exp-dot", ridge=0.1),
                   dict(kernel="gaussian", ridge=0.1, refine="float32")):
        with pytest.raises(NotImplementedError):
            MI355XSolver(dimension=3, preconditioner_rank=8, **kwargs)
    with pytest.raises(ValueError):
        MI355XSolver(kernel="gaussian", dimension=3, preconditioner_rank=8)
    with pytest.raises(ValueError):
        MI355XSolver(kernel="gaussian", dimension=3, ridge=0.1, preconditioner_rank=-1)
    algo = MI355XSolver(kernel="gaussian", dimension=3, ridge=0.1)
    with pytest.raises(ValueError):
        algo.set_query_arguments(preconditioner_rank=8, ridge=0.0)
    # the name at rank 0 is what it was; a rank shows in it, as a ridge does
    assert algo.name == "MI355XSolver(float64, cg, rtol=1e-06, ridge=0.1)"
    assert MI355XSolver(kernel="gaussian", dimension=3, ridge=0.1, preconditioner_rank=8).name == \
        "MI355XSolver(float64, cg, rtol=1e-06, ridge=0.1, preconditioner_rank=8)"


def test_two_ranks_on_one_gpu():
    """11. Through the host transport, uneven shards."""
    out = _spawn([os.path.join(HERE, "_precond_rank_worker.py")], world=2, timeout=600)
    rep = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
    print(json.dumps(rep))
    assert rep["world"] == 2 and rep["shards"] == [[0, 250], [250, 384]]
    assert rep["ranks_bitwise_equal"] and rep["pivots_equal_single"] and rep["factor_equals_single"], rep
    assert rep["converged"] and rep["rank_built"] == pr.RANK, rep
    assert rep["resid"] <= 1.5 * rep["rtol"] and rep["numpy_resid"] <= 1.5 * rep["rtol"], rep
    assert abs(rep["iterations"] - rep["single_iterations"]) <= 1, rep  # (the sharded operator sums in another order)


def test_plugin_with_a_preconditioner():
    """12. MI355XSolver(preconditioner_rank=32) on the Matern 5/2 system with a scalar ridge."""
    y, a = pr.points("M52"), pr.rhs(3)
    out = {}
    for rank in (0, 32):
        algo = MI355XSolver(kernel="matern-5/2", dimension=3, precision=np.float64, rtol=1e-8, maxit=2000, ridge=0.015,
                            preconditioner_rank=rank)
        try:
            algo.prepare_data(source_points=y)
            algo.fit()
            algo.prepare_query(target_signal=a)
            algo.query()
            out[rank] = (algo.get_result(), algo.get_additional(), algo.log_marginal_likelihood(probes=8, seed=1), algo.name)
        finally:
            algo.done()
    (b0, info0, (l0, se0), name0), (b1, info1, (l1, se1), name1) = out[0], out[32]
    print(f"iterations {info0['cg_iterations']} -> {info1['cg_iterations']}; built {info1['preconditioner_rank']} in "
          f"{info1['preconditioner_ms']:.2f} ms; log likelihood {l0!r} +- {se0:.3g} / {l1!r} +- {se1:.3g}")
    assert info0["cg_converged"] and info1["cg_converged"]
    assert info1["cg_iterations"] < info0["cg_iterations"]
    assert "preconditioner_rank" not in info0 and "preconditioner_ms" not in info0 and "preconditioner" not in name0
    assert info1["preconditioner_rank"] == 32 and info1["preconditioner_ms"] > 0
    A = pr.kernel_matrix("M52") + 0.015 * np.eye(pr.N)
    assert np.max(kr.true_residual(A, b1, a)) <= 1.5e-8
    assert abs(l1 - l0) <= max(se0, se1), (l0, l1, se0, se1)  # same probes, solutions equal to 1e-8: far inside
