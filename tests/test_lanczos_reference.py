"""CPU tests of the Lanczos-quadrature restatement the GPU tests compare with (lanczos_reference.py), made without the
code under test, on the six positive definite systems of krylov_reference: the quadrature on CG's coefficients is the
Gauss quadrature of z' log(A) z with an error of rtol^2, z' x is the quadrature of 1 / theta, the cases the GPU tests use
tolerate a product error, the stochastic estimates are within their own standard errors of the exact log-determinant and
trace of the inverse, and the per-column freeze behaves as stated."""
import numpy as np
import pytest

import krylov_reference as kr
import lanczos_reference as lz

SEEDS = tuple(range(1, 6))


def quadrature_bound(rtol):
    return 10.0 * rtol * rtol + 1e-13


@pytest.mark.parametrize("rtol", (1e-2, 1e-4, 1e-7))
@pytest.mark.parametrize("name", lz.SYSTEMS)
def test_quadrature_error_is_rtol_squared(name, rtol):
    """(a) |logquad - z' log(A) z| / S <= 10 rtol^2 + 1e-13 with the exact value from eigh(A);  (b) invquad equals the
    quadrature of 1 / theta and z' A^-1 z to the same bound, relative to itself."""
    z = lz.probes(kr.N, 8)
    A, _ = kr.matrix(name)
    t = lz.cg_lanczos(A, z, rtol, 1000)
    assert np.all(t.frozen == lz.TOLERANCE) and np.all(t.steps < 1000)
    err = np.abs(t.logquad - lz.exact_form(name, z, np.log)) / t.scale
    inv_quad = t.z2 * np.array([lz.quadrature(t.alpha[:m, e], t.beta[:m, e], lambda th: 1.0 / th) for e, m in enumerate(t.steps)])
    inv_exact = lz.exact_form(name, z, lambda lam: 1.0 / lam)
    err_q = np.abs(t.invquad - inv_quad) / np.abs(inv_exact)
    err_x = np.abs(t.invquad - inv_exact) / np.abs(inv_exact)
    print(f"{name} rtol={rtol:g}: steps {t.steps.min()}..{t.steps.max()}, log error / S {err.max():.3g}, z'x vs quadrature "
          f"{err_q.max():.3g}, vs z'A^-1 z {err_x.max():.3g}, bound {quadrature_bound(rtol):.3g}")
    assert err.max() <= quadrature_bound(rtol)
    assert err_q.max() <= 1e-13
    assert err_x.max() <= quadrature_bound(rtol)


def uses():
    """Every (system, P, rtol, maxit, precision) test_gpu_lanczos.py runs."""
    out = [(s, P, rtol, 1000, lz.F64) for s in lz.SYSTEMS for rtol in lz.RTOLS for P in (4, 1)]
    out += [(s, P, 1e-4, 1000, lz.F32) for s in lz.FLOAT32 for P in (4, 1)]
    out += [(s, 4, lz.UNREACHABLE, m, lz.F64) for s in lz.MAXIT_SYSTEMS for m in lz.MAXITS]
    out += [("G30", 9, 1e-7, 1000, lz.F64), ("G30", 64, 1e-7, 1000, lz.F64), ("Gr", 64, 1e-7, 1000, lz.F64)]
    return out


def ident(u):
    return f"{u[0]}-P{u[1]}-rtol{u[2]:g}-maxit{u[3]}-{u[4]}"


@pytest.mark.parametrize("use", uses(), ids=ident)
def test_case_tolerates_a_product_error(use):
    """(c) the operator's output times 1 + p randn, p = ten times the working precision's product tolerance, 5 seeds: no
    column's step count moves; logquad (relative to S), invquad (relative to itself) and every coefficient
    (lanczos_reference.coefficient_error, residual-weighted) move by at most G p, and every column of x (krylov_reference.column_error) by
    at most GX p, with G and GX as recorded in lanczos_reference."""
    name, P, rtol, maxit, precision = use
    A, _ = kr.matrix(name, precision)
    z, p = lz.block(P, precision), kr.NOISE[precision]
    t = lz.run(name, P, rtol, maxit, precision)
    live = t.z2 > 0
    g = gx = 0.0
    for seed in SEEDS:
        n = lz.cg_lanczos(A, z, rtol, maxit, noise=p, seed=seed)
        assert np.array_equal(n.steps, t.steps), (use, seed, n.steps, t.steps)
        g = max(g, float(np.max(np.abs(n.logquad - t.logquad)[live] / t.scale[live])) / p)
        g = max(g, float(np.max(np.abs(n.invquad - t.invquad)[live] / np.abs(t.invquad[live]))) / p)
        g = max(g, max(lz.coefficient_error(n.alpha, n.beta, t, e, weighted=True) for e in range(P)) / p)
        gx = max(gx, kr.column_error(n.x, t.x) / p)
    recorded, recorded_x = lz.G[(name, precision, rtol)], lz.GX[(name, precision, rtol)]
    print(f"{ident(use)}: steps {t.steps.min()}..{t.steps.max()}, G {g:.2f} (recorded {recorded}), GX {gx:.2f} (recorded {recorded_x})")
    assert g <= recorded <= lz.G_MAX, (use, g, recorded)
    assert gx <= recorded_x <= lz.G_MAX, (use, gx, recorded_x)


@pytest.mark.parametrize("name, precision, rtol", [(s, lz.F64, r) for s in lz.SYSTEMS for r in lz.RTOLS] + [(s, lz.F32, 1e-4) for s in lz.FLOAT32])
def test_unweighted_coefficients_at_the_rounding_level(name, precision, rtol):
    """The GPU tests hold the coefficients to 4 G TOL RELATIVE TO THEMSELVES, row by row.  At the noise of (c), 10 TOL,
    no run could meet that (the last rows move by up to 7e5 p); what lets the GPU meet it is that its product's error is
    far below TOL.  Shown here: with a product error at the rounding level of the working precision (2^-52 in float64,
    2^-23 in float32) the unweighted relative difference stays inside 4 G TOL on every case, 5 seeds."""
    A, _ = kr.matrix(name, precision)
    p = 2.0 ** -52 if precision == lz.F64 else 2.0 ** -23
    worst = 0.0
    for P in (4, 1):
        z, t = lz.block(P, precision), lz.run(name, P, rtol, 1000, precision)
        for seed in SEEDS:
            n = lz.cg_lanczos(A, z, rtol, 1000, noise=p, seed=seed)
            assert np.array_equal(n.steps, t.steps)
            worst = max(worst, max(lz.coefficient_error(n.alpha, n.beta, t, e) for e in range(P)))
    tol = lz.tolerance(name, rtol, precision)
    print(f"{name} {precision} rtol={rtol:g}: unweighted coefficient difference {worst:.3g} at noise {p:.2g}, tolerance {tol:.3g}")
    assert worst <= tol, (worst, tol)


def test_float32_at_1e_7_is_not_usable():
    """(c) at float32 and rtol 1e-7 the float32 product error does move the step counts: that case is not run on the GPU."""
    moved = False
    for name in lz.FLOAT32:
        A, _ = kr.matrix(name, lz.F32)
        z = lz.block(4, lz.F32)
        t = lz.cg_lanczos(A, z, 1e-7, 1000)
        moved |= any(not np.array_equal(lz.cg_lanczos(A, z, 1e-7, 1000, noise=kr.NOISE[lz.F32], seed=s).steps, t.steps)
                     for s in SEEDS)
    assert moved


@pytest.mark.parametrize("name", lz.SYSTEMS)
def test_estimates_are_within_their_standard_errors(name):
    """(d) 64 probes at seed 0: mean logquad and mean invquad within 4 standard errors of log det A and tr A^-1."""
    z = lz.probes(kr.N, 64)
    A, _ = kr.matrix(name)
    t = lz.cg_lanczos(A, z, 1e-7, 1000)
    lam, _ = lz.exact(name)
    for what, values, truth in (("log det", t.logquad, np.sum(np.log(lam))), ("tr inverse", t.invquad, np.sum(1.0 / lam))):
        stderr = values.std(ddof=1) / np.sqrt(len(values))
        dev = abs(values.mean() - truth) / stderr
        print(f"{name} {what}: estimate {values.mean():.6g} exact {truth:.6g} stderr {stderr:.3g} deviation {dev:.2f} stderr")
        assert dev <= 4.0, (name, what, dev)


def test_zero_column():
    """(e) a zero column is frozen from the start: steps 0, values 0, x = 0 -- alone and beside live columns."""
    A, _ = kr.matrix("G30")
    t = lz.cg_lanczos(A, np.zeros((kr.N, 1)), 1e-7, 1000)
    assert t.iters == 0 and t.steps[0] == 0 and t.logquad[0] == 0.0 and t.invquad[0] == 0.0 and not t.x.any()
    t = lz.run("G30", 4, 1e-7)
    assert t.frozen[3] == lz.ZERO and t.steps[3] == 0 and t.logquad[3] == 0.0 and t.invquad[3] == 0.0 and not t.x[:, 3].any()
    assert np.all(t.frozen[:3] == lz.TOLERANCE) and np.all(t.steps[:3] > 0)


def test_a_column_that_converges_early_keeps_its_x():
    """(f) nine probes on G30 freeze at different iterations; each column's x, steps and coefficients are those of that
    column run ALONE (where it stops at its own count) up to the rounding of numpy's product of one column against nine,
    so nothing moved after it froze."""
    A, _ = kr.matrix("G30")
    t = lz.run("G30", 9, 1e-7)
    assert len(set(t.steps.tolist())) > 1, t.steps
    z = lz.block(9)
    for e in range(9):
        alone = lz.cg_lanczos(A, z[:, e:e + 1], 1e-7, 1000)
        assert alone.steps[0] == t.steps[e] == alone.iters
        assert kr.column_error(alone.x, t.x[:, e:e + 1]) <= 1e-12
        assert np.allclose(alone.alpha[:alone.iters, 0], t.alpha[:alone.iters, e], rtol=1e-8, atol=0.0)
        assert not t.alpha[t.steps[e]:, e].any() and not t.beta[t.steps[e]:, e].any()


def test_breakdown_and_nan():
    """A column that hits pAp == 0 freezes with steps = k - 1 and a flag of its own; NaN never freezes a column."""
    A = np.diag([1.0, -1.0])
    t = lz.cg_lanczos(A, np.array([[1.0], [1.0]]), 1e-7, 10)   # p' A p = 0 in the first iteration
    assert t.frozen[0] == lz.BREAKDOWN and t.steps[0] == 0 and t.iters == 1 and not t.x.any()
    A, _ = kr.matrix("Gr")
    z = lz.block(4).copy()
    z[5, 1] = np.nan
    t = lz.cg_lanczos(A, z, 1e-4, 12)
    assert t.iters == 12 and t.frozen[1] == 0 and np.isnan(t.logquad[1])
    clean = lz.run("Gr", 4, 1e-4)
    for e in (0, 2, 3):   # the other columns are untouched by it
        assert t.steps[e] == clean.steps[e] and np.array_equal(t.x[:, e], clean.x[:, e]) and t.logquad[e] == clean.logquad[e]
