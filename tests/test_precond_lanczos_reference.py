"""CPU tests of the preconditioned quadrature's restatement (precond_lanczos_reference.py), made without the code under
test: log det P is slogdet's, every logquad is w' log(M) w from an eigendecomposition, the 16-probe estimates meet the
dense values, the preconditioner halves the steps and shrinks the deviation, and every figure the GPU tests rely on --
the amplification tables, the rounding yardsticks, the step counts that survive a product error -- is measured here."""
import math

import numpy as np
import pytest

import krylov_reference as kr
import lanczos_reference as lz
import precond_lanczos_reference as plr
import precond_reference as pr

SEEDS = tuple(range(8))
BLOCKS = (1, 4, 5)
NOISE = kr.NOISE[plr.F64]
PAIRS = [(s, rtol) for s in plr.SYSTEMS for rtol in plr.RTOLS[s]]


def up(v):
    return math.ceil(v * 2.0) / 2.0


@pytest.mark.parametrize("name", plr.SYSTEMS)
def test_logdet_p_is_slogdet_of_the_dense_preconditioner(name):
    L = pr.factor(name)[0]
    ref = np.linalg.slogdet(L.T @ L + np.diag(plr.DIAG))
    got = plr.logdet_p(L, plr.DIAG)
    print(f"{name}: {got!r} slogdet {ref[1]!r}")
    assert ref[0] > 0 and abs(got - ref[1]) <= 1e-11 * abs(ref[1])


@pytest.mark.parametrize("name", plr.SYSTEMS)
def test_probes_have_the_preconditioners_covariance(name):
    """z = D^1/2 g + L' h is linear in (g, h) with [D^1/2 | L'] [D^1/2 | L']' = P; rho_0 = |P^-1/2 z|^2; rows of h beyond
    the factor's are not read; the zero column of block(4) gives a zero column."""
    L = pr.factor(name)[0]
    B = np.concatenate([np.diag(np.sqrt(plr.DIAG)), L.T], axis=1)
    assert np.abs(B @ B.T - (L.T @ L + np.diag(plr.DIAG))).max() <= 1e-12
    g, h = plr.block(4)
    z = plr.form(L, plr.DIAG, g, h)
    assert np.abs(z - B @ np.concatenate([g, h])).max() <= 1e-12 and not z[:, 3].any()
    assert np.array_equal(plr.form(L[:7], plr.DIAG, g, h), plr.form(L[:7], plr.DIAG, g, h[:7]))
    t = plr.own(name, 4, plr.RTOLS[name][0])
    _, _, root = plr.preconditioned_spectrum(name)
    w2 = np.sum((root @ z) ** 2, axis=0)
    assert np.abs(t.rho0 - w2).max() <= 1e-9 * w2.max() and t.rho0[3] == 0.0
    assert t.steps[3] == 0 and t.frozen[3] == plr.ZERO and t.logquad[3] == 0.0 and t.invquad[3] == 0.0 and not t.x[:, 3].any()


@pytest.mark.parametrize("name, rtol", PAIRS)
def test_logquad_is_the_quadratic_form_of_log_m(name, rtol):
    """|logquad - w' log(M) w| <= QUADRATURE_RTOL2 rtol^2 S per column, and invquad = z' P^-1 A^-1 z to the solve's rtol."""
    A, _ = pr.matrix(name)
    worst = 0.0
    for P in BLOCKS:
        t = plr.own(name, P, rtol)
        nz = t.rho0 > 0
        assert np.all(t.frozen[nz] == plr.TOLERANCE)
        exact = plr.exact_logquad(name, t.z)
        worst = max(worst, float(np.max(np.abs(t.logquad - exact)[nz] / t.scale[nz])) / rtol ** 2)
        inv = np.sum(t.pz * np.linalg.solve(A, t.z), axis=0)
        assert np.all(np.abs(t.invquad - inv)[nz] <= 4 * rtol * np.abs(inv[nz]))
    print(f"{name} rtol={rtol:g}: quadrature error {worst:.3g} rtol^2 S (bound {plr.QUADRATURE_RTOL2})")
    assert worst <= plr.QUADRATURE_RTOL2


@pytest.mark.parametrize("name", plr.SYSTEMS)
def test_estimates_steps_and_deviation_against_the_plain_restatement(name):
    """The seed and the tolerance the GPU test uses: log det P + mean logquad and mean invquad within 3 standard errors of
    slogdet(A) and tr A^-1; at most half the plain restatement's steps; a smaller sample deviation of logquad."""
    A, _ = pr.matrix(name)
    g, h = plr.probes(plr.N, plr.RANK, plr.ESTIMATE_PROBES, plr.SEED)
    t = plr.run(A, pr.factor(name)[0], plr.DIAG, g, h, plr.RATIO_RTOL, 1000)
    plain = lz.cg_lanczos(A, lz.probes(plr.N, plr.ESTIMATE_PROBES, plr.SEED), plr.RATIO_RTOL, 5000)
    logdet, logdet_se, trinv, trinv_se = plr.estimates(t)
    dense_logdet, dense_trinv = plr.dense(name)
    sd, sd_plain = float(np.std(t.logquad, ddof=1)), float(np.std(plain.logquad, ddof=1))
    print(f"{name}: log det {logdet:.4f} +- {logdet_se:.4f} (dense {dense_logdet:.4f}), tr A^-1 {trinv:.2f} +- {trinv_se:.2f} "
          f"(dense {dense_trinv:.2f}); steps {t.steps.max()} against {plain.steps.max()}; deviation {sd:.3f} against {sd_plain:.3f}")
    assert np.all(t.frozen == plr.TOLERANCE) and np.all(plain.frozen == lz.TOLERANCE)
    assert abs(logdet - dense_logdet) <= 3 * logdet_se and abs(trinv - dense_trinv) <= 3 * trinv_se
    assert 2 * t.steps.max() <= plain.steps.max()
    assert sd < sd_plain
    assert abs(float(np.mean(plain.logquad)) - dense_logdet) <= 3 * sd_plain / 4.0  # the plain estimate is sound too


def _amplification(name, rtol, maxits):
    """(G, GX) as the reference module defines them, measured."""
    scal = itr = 0.0
    for maxit in maxits:
        for P in BLOCKS:
            ref = plr.own(name, P, rtol, maxit)
            nz = ref.rho0 > 0
            for seed in SEEDS:
                n = plr.case(name, P, rtol, maxit, noise=NOISE, seed=seed)
                assert np.array_equal(n.steps, ref.steps) and np.array_equal(n.pz, ref.pz) and np.array_equal(n.rho0, ref.rho0)
                scal = max(scal, float(np.max(np.abs(n.logquad - ref.logquad)[nz] / ref.rho0[nz])),
                           float(np.max(np.abs(n.invquad - ref.invquad)[nz] / np.abs(ref.invquad[nz]))),
                           max(lz.coefficient_error(n.alpha, n.beta, ref, e, weighted=True) for e in range(P)))
                itr = max(itr, kr.column_error(n.x, ref.x))
    return scal / NOISE, itr / NOISE


@pytest.mark.parametrize("name, rtol", list(plr.COMPARED) + [(s, plr.UNREACHABLE) for s in plr.SYSTEMS])
def test_amplification_tables(name, rtol):
    """The tables hold what is measured here, rounded up to the next half, and the tolerances they give are far below
    anything a wrong coefficient would produce."""
    g, gx = _amplification(name, rtol, plr.MAXITS if rtol == plr.UNREACHABLE else (1000,))
    print(f"{name} rtol={rtol:g}: G measured {g:.2f} table {plr.G[(name, rtol)]}; GX measured {gx:.2f} table {plr.GX[(name, rtol)]}")
    assert up(g) == plr.G[(name, rtol)] and up(gx) == plr.GX[(name, rtol)]
    assert plr.tolerance(name, rtol, plr.GX) <= 1e-9


@pytest.mark.parametrize("name, rtol", PAIRS)
def test_step_counts_survive_a_product_error(name, rtol):
    for P in BLOCKS:
        ref = plr.own(name, P, rtol)
        for seed in SEEDS:
            assert np.array_equal(plr.case(name, P, rtol, noise=NOISE, seed=seed).steps, ref.steps), (P, seed)


@pytest.mark.parametrize("name, precision", [(s, plr.F64) for s in plr.SYSTEMS] + [(s, plr.F32) for s in plr.FLOAT32])
def test_rounding_yardsticks(name, precision):
    """float64 against numpy.longdouble for the formulas that take no product, on the factor of either precision."""
    L = pr.factor(name, precision)[0]
    worst = {"logdet_p": 0.0, "pz": 0.0, "rho0": 0.0}
    for P in BLOCKS:
        g, h = plr.block(P)
        z = plr.form(L, plr.DIAG, g, h)
        pz = pr.apply(L, plr.DIAG, z)
        rho0 = np.sum(z * pz, axis=0)
        ld_logdet, ld_z, ld_pz, ld_rho0 = plr.longdouble_pieces(L, plr.DIAG, g, h)
        nz = rho0 > 0
        worst["logdet_p"] = max(worst["logdet_p"], float(abs(plr.logdet_p(L, plr.DIAG) - ld_logdet) / abs(ld_logdet)))
        worst["pz"] = max(worst["pz"], float(np.max(np.linalg.norm((pz - ld_pz)[:, nz].astype(np.float64), axis=0)
                                                    / np.linalg.norm(ld_pz[:, nz].astype(np.float64), axis=0))))
        worst["rho0"] = max(worst["rho0"], float(np.max(np.abs(rho0 - ld_rho0)[nz] / ld_rho0[nz])))
    print(f"{name} {precision}: " + ", ".join(f"{k} {v:.3g} (recorded {plr.ROUNDING[k]:.3g})" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= plr.ROUNDING[k]
        assert plr.rounding_tolerance(k) <= 1e-11


def test_graph_replay_systems_first_burst():
    """REPLAY_G, measured as the tables are, on the restatement's own rank-16 factor."""
    y, d, g, h = plr.replay_system()
    A = plr.replay_matrix(y, d)
    L = pr.pivoted_cholesky(A - np.diag(d), plr.REPLAY_RANK, pr.TAU[plr.F64])[0]
    ref = plr.run(A, L, d, g, h, plr.UNREACHABLE, kr.BURST)
    worst = 0.0
    for seed in SEEDS:
        n = plr.run(A, L, d, g, h, plr.UNREACHABLE, kr.BURST, noise=NOISE, seed=seed)
        worst = max(worst, max(lz.coefficient_error(n.alpha, n.beta, ref, e, weighted=True) for e in range(2)) / NOISE)
    print(f"replay system: G measured {worst:.2f} recorded {plr.REPLAY_G}")
    assert L.shape[0] == plr.REPLAY_RANK and ref.steps.tolist() == [kr.BURST] * 2 and up(worst) == plr.REPLAY_G


@pytest.mark.parametrize("seed", [plr.SEED])
def test_plugin_estimator_on_the_dense_matrix(seed):
    """What test_gpu_precond_lanczos.py::test_plugin asks of the device, with the restatement in its place: M52 with the
    scalar ridge 0.015, 16 probes; value, gradient and d_ridge within 3 standard errors of the dense ones."""
    import dscale_reference as dref
    from kernel_matrix_benchmarks_amd.algorithms.mi355x import assemble_likelihood_gradient
    y, a, ridge, E = pr.points("M52"), plr.plugin_rhs(), plr.PLUGIN_RIDGE, 2
    A = pr.kernel_matrix("M52") + ridge * np.eye(pr.N)
    dA = dref.scale_derivative(kernel="matern-5/2", source_points=y, source_signal=np.eye(pr.N))
    lam, V = np.linalg.eigh(A)
    invA = (V / lam) @ V.T
    alpha = invA @ a
    g, h = plr.probes(pr.N, pr.RANK, plr.ESTIMATE_PROBES, seed)
    t = plr.run(A, pr.factor("M52")[0], np.full(pr.N, ridge), g, h, 1e-8, 1000)
    got = assemble_likelihood_gradient(a, alpha, t.x, np.einsum("ijd,jp->ipd", dA, t.pz), np.einsum("ijd,je->ied", dA, alpha),
                                       t.logdet_p + t.logquad, t.invquad)
    exact = 0.5 * np.einsum("ie,ijd,je->d", alpha, dA, alpha) - 0.5 * E * np.einsum("ij,jid->d", invA, dA)
    exact_ridge = 0.5 * np.sum(alpha * alpha) - 0.5 * E * np.sum(1.0 / lam)
    value = -0.5 * np.sum(a * alpha) - 0.5 * E * np.sum(np.log(lam)) - 0.5 * E * pr.N * np.log(2 * np.pi)
    dev = np.abs(got.d_log_lengthscale - exact) / got.d_log_lengthscale_stderr
    print(f"gradient {dev} standard errors off, d_ridge {abs(got.d_ridge - exact_ridge) / got.d_ridge_stderr:.2f}, value "
          f"{abs(got.value - value) / got.value_stderr:.2f}")
    assert (dev <= 3).all() and abs(got.d_ridge - exact_ridge) <= 3 * got.d_ridge_stderr
    assert abs(got.value - value) <= 3 * got.value_stderr
