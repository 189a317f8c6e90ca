"""CPU tests of the Krylov restatement the GPU tests compare with (krylov_reference.py), made without the code under
test: it solves its systems, its recurrence residuals are the residuals of its iterates at every iteration, and every
case the GPU tests use can carry their assertions -- a product error of ten times the working precision's tolerance
moves neither the iteration count nor, by more than g times itself, the iterate, and where a solve stops inside a
burst of eight iterations the iterate of that iteration and the one at the end of the burst are far enough apart for a
driver that returned the wrong one to be noticed."""
import numpy as np
import pytest

import krylov_reference as kr

SEEDS = tuple(range(1, 9))
ES = (4, 1)


def uses():
    """Every (system, E, rtol, maxit, precision) test_gpu_krylov.py runs."""
    out = [(s, E, rtol, 1000, "float64") for s in kr.STOPPING for E in ES for rtol in kr.SYSTEMS[s].rtols]
    out += [(s, E, kr.UNREACHABLE, m, "float64") for s, ms in kr.MAXIT_CASES.items() for m in ms
            for E in (ES if s != "E0" else (4,))]
    out += [(s, E, 1e-4, 1000, "float32") for s in kr.FLOAT32 for E in ES]
    return out


def ident(u):
    return f"{u[0]}-E{u[1]}-rtol{u[2]:g}-maxit{u[3]}-{u[4]}"


@pytest.mark.parametrize("E", ES)
@pytest.mark.parametrize("name", list(kr.SYSTEMS))
def test_restatement_solves_and_its_residuals_are_true(name, E):
    """On every system: the recurrence's residual (CG's sqrt(rs) / |a|, MINRES' phibar / beta1) equals |a - A x_k| / |a|
    at every iteration within 1e-10 of the first residual (which is 1); run to a tolerance, the final iterate agrees
    with numpy.linalg.solve within kappa rtol per column; the zero column stays exactly 0.  (A MINRES column flagged
    done keeps its x while its scalars run on: its phibar is compared up to the flag, its x must not move after.)
    I0 and E0 are ill conditioned and used for their first iterations only: the residual equality alone."""
    A, kappa = kr.matrix(name)
    a = kr.rhs(E)
    lam = np.linalg.eigvalsh(A)
    runs = [(kr.UNREACHABLE, m) for m in kr.MAXIT_CASES.get(name, ())]
    if name in kr.STOPPING:
        runs += [(rtol, 1000) for rtol in kr.SYSTEMS[name].rtols]
        dense = np.linalg.solve(A, a)
    counts = []
    for rtol, maxit in runs:
        t = kr.trace(name, E, rtol, maxit)
        worst = 0.0
        for k in range(1, t.iters + 1):
            true = kr.true_residual(A, t.xs[k], a)
            for e in range(len(true)):
                flagged = t.done_at is not None and 0 <= t.done_at[e] < k
                if flagged:
                    assert np.array_equal(t.xs[k][:, e], t.xs[t.done_at[e]][:, e]), (name, rtol, k, e)
                else:
                    worst = max(worst, abs(t.rel[k - 1, e] - true[e]))
        assert worst <= 1e-10, (name, E, rtol, maxit, worst)
        assert np.all(np.isfinite(t.x))
        if E == 4:
            assert not t.xs[:, :, 3].any(), "the zero column moved"
        if maxit == 1000:
            counts.append(t.iters)
            assert t.iters < maxit and np.all(t.rel[-1, : min(E, 3)] <= rtol) and not np.all(t.rel[-2, : min(E, 3)] <= rtol)
            err = np.linalg.norm(t.x - dense, axis=0)[: min(E, 3)] / np.linalg.norm(dense, axis=0)[: min(E, 3)]
            assert np.all(err <= kappa * rtol), (name, E, rtol, err, kappa * rtol)
        else:
            assert t.iters == maxit
    print(f"{name} E={E}: cond {kappa:.3g}, {int((lam < 0).sum())} negative eigenvalues, |lambda| in "
          f"[{np.abs(lam).min():.4g}, {np.abs(lam).max():.4g}], counts at rtol {kr.SYSTEMS[name].rtols}: {counts}")


@pytest.mark.parametrize("use", uses(), ids=ident)
def test_case_tolerates_a_product_error(use):
    """The operator's output times 1 + p randn, p = ten times the working precision's product tolerance: the count
    does not move, and the iterate moves by at most g p with g as recorded in krylov_reference.SYSTEMS, g <= 8."""
    name, E, rtol, maxit, precision = use
    A, _ = kr.matrix(name, precision)
    a, p = kr.rhs(E, precision), kr.NOISE[precision]
    t = kr.trace(name, E, rtol, maxit, precision)
    g = 0.0
    for seed in SEEDS:
        n = kr.SOLVERS[kr.SYSTEMS[name].solver](A, a, rtol, maxit, noise=p, seed=seed)
        assert n.iters == t.iters, (use, seed, n.iters, t.iters)
        g = max(g, kr.column_error(n.x, t.x) / p)
    recorded = kr.SYSTEMS[name].g[(precision, rtol)]
    print(f"{ident(use)}: count {t.iters}, g {g:.2f} (recorded {recorded})")
    assert g <= recorded <= kr.G_MAX, (use, g, recorded)


@pytest.mark.parametrize("E", ES)
@pytest.mark.parametrize("name, rtol", [(s, rtol) for s in kr.STOPPING for rtol in kr.SYSTEMS[s].rtols])
def test_first_iteration_and_end_of_burst_are_apart(name, rtol, E):
    """A solve that stops at k, k no multiple of 8: x_k and the iterate at the end of its burst (unreachable tolerance,
    8 ceil(k / 8) iterations) differ by at least 100 times the GPU tolerance, or returning the wrong one would pass."""
    k = kr.trace(name, E, rtol, 1000).iters
    end = kr.BURST * -(-k // kr.BURST)
    if k == end:
        print(f"{name} E={E} rtol={rtol:g}: count {k} ends its burst")
        return
    x_k = kr.trace(name, E, rtol, 1000).x
    x_end = kr.trace(name, E, kr.UNREACHABLE, end).x
    assert kr.trace(name, E, kr.UNREACHABLE, end).iters == end
    dist, tol = kr.column_error(x_end, x_k), kr.tolerance(name, rtol)
    print(f"{name} E={E} rtol={rtol:g}: count {k}, burst end {end}, distance {dist:.3g} = {dist / tol:.0f} x tolerance {tol:.2g}")
    assert dist >= 100 * tol, (name, E, rtol, dist, tol)


def test_degenerate_right_hand_sides():
    """An all-zero right-hand side and maxit = 0 run no iteration and leave x = 0 (the GPU tests' expectation)."""
    for name in ("G30", "Id+-"):
        A, _ = kr.matrix(name)
        solver = kr.SOLVERS[kr.SYSTEMS[name].solver]
        t = solver(A, np.zeros((kr.N, 2)), 1e-8, 1000)
        assert t.iters == 0 and not t.x.any()
        t = solver(A, kr.rhs(4), 1e-8, 0)
        assert t.iters == 0 and not t.x.any()
