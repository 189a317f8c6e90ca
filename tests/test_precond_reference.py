"""CPU tests of the preconditioner's restatement (precond_reference.py), made without the code under test: its factor is a
partial Cholesky factor, its apply is the inverse of L' L + D, its preconditioned iteration solves its systems in at most
half the iterations of plain conjugate gradients, and every case the GPU tests use can carry their assertions."""
import numpy as np
import pytest

import krylov_reference as kr
import precond_reference as pr

SEEDS = tuple(range(1, 9))
ES = (3, 1)
PRECISIONS = (pr.F64, pr.F32)


@pytest.mark.parametrize("name", list(pr.SYSTEMS))
def test_factor_is_a_partial_cholesky_factor(name):
    """K - L' L is positive semi-definite up to rounding, vanishes on the pivot rows, and its diagonal is the residual
    diagonal the next step would look at; the pivots are distinct and each is the argmax of the diagonal before its
    step.  Following its own pivots as GIVEN pivots reproduces the factor bit for bit."""
    K = pr.kernel_matrix(name)
    L, piv, before = pr.factor(name)
    assert L.shape == (pr.RANK, pr.N) and len(set(piv.tolist())) == pr.RANK
    S = K - L.T @ L
    assert np.abs(S[piv]).max() <= 1e-13 and np.linalg.eigvalsh(S).min() >= -1e-12
    for m in range(1, pr.RANK):
        assert np.abs(before[m] - np.diag(K - L[:m].T @ L[:m])).max() <= 1e-13
    assert np.array_equal(before[0], np.ones(pr.N)) and piv[0] == 0  # ties go to the smaller index
    assert all(before[m][piv[m]] == before[m].max() for m in range(pr.RANK))
    again = pr.pivoted_cholesky(K, pr.RANK, pr.TAU[pr.F64], pivots=piv)
    assert np.array_equal(again[0], L) and np.array_equal(again[2], before)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(pr.SYSTEMS))
def test_tau_never_decides(name, precision):
    """Every pivot's residual diagonal is >= 100 tau of float32: no table system stops early, whatever the rounding."""
    _, piv, before = pr.factor(name, precision)
    smallest = min(before[m][piv[m]] for m in range(len(piv)))
    print(f"{name} {precision}: smallest pivot {smallest:.3g}, 100 tau(float32) = {100 * pr.TAU[pr.F32]:.3g}")
    assert len(piv) == pr.RANK and smallest >= 100 * pr.TAU[pr.F32]


def test_stops_on_tau():
    """A matrix of rank 3: the fourth residual diagonal is rounding alone, no fourth column is taken."""
    B = np.random.RandomState(3).rand(20, 3)
    K = B @ B.T
    K = K / np.sqrt(np.outer(np.diag(K), np.diag(K)))
    L, piv, _ = pr.pivoted_cholesky(K, 8, pr.TAU[pr.F64])
    assert L.shape[0] == 3 and np.abs(K - L.T @ L).max() <= 1e-14


@pytest.mark.parametrize("name", list(pr.SYSTEMS))
def test_apply_is_the_inverse_of_the_preconditioner(name):
    L, _, _ = pr.factor(name)
    P = L.T @ L + np.diag(pr.DIAG)
    for r in (pr.rhs(3), pr.rhs(1), pr.rhs(1)[:, 0]):
        ref = np.linalg.solve(P, r)
        assert np.abs(pr.apply(L, pr.DIAG, r) - ref).max() <= 1e-10 * np.abs(ref).max()
    assert np.array_equal(pr.apply(L[:0], pr.DIAG, pr.rhs(1)), pr.rhs(1) / pr.DIAG[:, None])  # rank 0: D^-1


@pytest.mark.parametrize("E", ES)
@pytest.mark.parametrize("name", list(pr.SYSTEMS))
def test_pcg_solves_in_at_most_half_the_iterations(name, E):
    """To RATIO_RTOL: the preconditioned iterate agrees with numpy.linalg.solve within kappa rtol, the zero column stays
    exactly 0, its recurrence residual is the true one, and it takes at most half of krylov_reference.cg's iterations."""
    A, kappa = pr.matrix(name)
    a, rtol = pr.rhs(E), pr.RATIO_RTOL
    t = pr.pcg(A, pr.factor(name)[0], pr.DIAG, a, rtol, 2000, history=True)
    plain = kr.cg(A, a, rtol, 5000)
    dense = np.linalg.solve(A, a)
    cols = slice(0, min(E, 2))
    err = np.linalg.norm(t.x - dense, axis=0)[cols] / np.linalg.norm(dense, axis=0)[cols]
    print(f"{name} E={E}: cond {kappa:.3g}, iterations {plain.iters} plain, {t.iters} preconditioned "
          f"(ratio {plain.iters / t.iters:.2f}), error {err.max():.3g}")
    assert np.all(err <= kappa * rtol)
    assert np.all(kr.true_residual(A, t.x, a) <= 1.5 * rtol)
    for k in range(1, t.iters + 1):
        assert np.abs(t.rel[k - 1, cols] - kr.true_residual(A, t.xs[k], a)).max() <= 1e-10
    if E == 3:
        assert not t.xs[:, :, 2].any(), "the zero column moved"
    assert 2 * t.iters <= plain.iters, (t.iters, plain.iters)


@pytest.mark.parametrize("E", ES)
@pytest.mark.parametrize("name, rtol", [(s, rtol) for s in pr.SYSTEMS for rtol in pr.SYSTEMS[s].rtols])
def test_tolerances_clear_the_stopping_test_and_survive_a_product_error(name, rtol, E):
    """The table's rtols: the last unmet residual is >= 1.05 rtol and the first met one <= 0.95 rtol, and the operator's
    output times 1 + 1e-10 randn (ten times the float64 product tolerance) does not move the count."""
    A, _ = pr.matrix(name)
    L, a = pr.factor(name)[0], pr.rhs(E)
    t = pr.pcg(A, L, pr.DIAG, a, rtol, 1000)
    worst = np.max(t.rel[:, : min(E, 2)], axis=1)
    print(f"{name} E={E} rtol={rtol:g}: count {t.iters}, residuals {worst[-2] / rtol:.2f} rtol -> {worst[-1] / rtol:.2f} rtol")
    assert 1 < t.iters < 1000 and worst[-2] >= 1.05 * rtol and worst[-1] <= 0.95 * rtol
    for seed in SEEDS:
        assert pr.pcg(A, L, pr.DIAG, a, rtol, 1000, noise=pr.NOISE[pr.F64], seed=seed).iters == t.iters, seed


@pytest.mark.parametrize("name", list(pr.SYSTEMS))
def test_first_iterates_tolerate_a_product_error(name):
    """After MAXITS iterations the iterate moves by at most g times a product error of ten times the float64 product
    tolerance, g as recorded and <= G_MAX; after 18 it moves by a thousand times more on the cube's systems, which is why
    the GPU tests compare iterates at MAXITS only."""
    precision = pr.F64
    A, _ = pr.matrix(name, precision)
    L, p = pr.factor(name, precision)[0], pr.NOISE[precision]
    g = late = 0.0
    for E in ES:
        a = pr.rhs(E, precision)
        for maxit in pr.MAXITS + (18,):
            t = pr.pcg(A, L, pr.DIAG, a, pr.UNREACHABLE, maxit)
            assert t.iters == maxit
            for seed in SEEDS:
                moved = kr.column_error(pr.pcg(A, L, pr.DIAG, a, pr.UNREACHABLE, maxit, noise=p, seed=seed).x, t.x) / p
                if maxit == 18:
                    late = max(late, moved)
                else:
                    g = max(g, moved)
    recorded = pr.SYSTEMS[name].g
    print(f"{name} {precision}: g {g:.2f} (recorded {recorded}), after 18 iterations {late:.3g}")
    assert g <= recorded <= pr.G_MAX, (g, recorded)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", list(pr.SYSTEMS))
def test_factor_tolerates_a_column_error(name, precision):
    """Kernel columns times 1 + p randn with the pivots held fixed: every column of L moves by at most g_factor p of its
    norm, and every pivot stays within 2 x that of the maximum of the residual diagonal (d = 1 - sum_t L_t^2 with
    sum_t L_t^2 <= 1, so d moves by at most twice the relative error of the columns)."""
    K, p = pr.kernel_matrix(name, precision), pr.NOISE[precision]
    L, piv, before = pr.factor(name, precision)
    g = 0.0
    for seed in SEEDS:
        Ln, _, bn = pr.pivoted_cholesky(K, pr.RANK, pr.TAU[precision], pivots=piv, noise=p, seed=seed)
        moved = pr.factor_error(Ln, L)
        g = max(g, moved / p)
        assert all(bn[m][piv[m]] >= bn[m].max() - 2 * moved for m in range(pr.RANK))
    recorded = pr.SYSTEMS[name].g_factor
    print(f"{name} {precision}: g_factor {g:.1f} (recorded {recorded})")
    assert g <= recorded, (g, recorded)
