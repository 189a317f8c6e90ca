"""The preconditioned Lanczos quadrature on the GPU (-m gpu): kmvp_<kernel>_lanczos_quadrature_precond,
Context.lanczos_quadrature_precond and MI355XSolver's ``preconditioned=True``, held to the float64 restatement of
precond_lanczos_reference.py on the 384-point systems of precond_reference.py (rank 32, diagonals 0.01 .. 0.02).

    1  log det P, pz = P^-1 z and rho_0 (and through them the probes z) against the restatement fed the device's own L,
       within MARGIN times the restatement's own float64-against-longdouble discrepancy (ROUNDING): no product is involved
    2  coefficients, steps, logquad, invquad, x against the restatement fed the device's L within 4 G TOL / 4 GX TOL, where
       the recurrence is reproducible (COMPARED and the runs to maxit 7, 8, 9); P = 4 with a zero column, P = 1, P = 5
    2b the step counts at every tolerance of RTOLS
    3  the 16-probe estimates against the dense values, and the steps against the plain entry's
    4  nothing else moves;  5  graph replay;  6  refusals;  7  two ranks;  8  the plugin
"""
import json
import os

import numpy as np
import pytest

import dscale_reference as dref
import krylov_reference as kr
import lanczos_reference as lz
import precond_lanczos_reference as plr
import precond_reference as pr
from kernel_matrix_benchmarks_amd import _lib
from kernel_matrix_benchmarks_amd.algorithms.mi355x import MI355XSolver
from test_gpu_multirank import _spawn

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CODES = {"float64": _lib.KMVP_F64, "float32": _lib.KMVP_F32}
WANT = dict(want_x=True, want_pz=True, want_coefficients=True)
KEYS = ("logquad", "invquad", "wnorm2", "steps", "x", "pz", "alpha", "beta")


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


def quadrature(name, P, rtol, maxit, precision="float64"):
    """(outputs, L) of one call on a context of its own."""
    ctx = open_context(name, precision)
    try:
        g, h = plr.block(P)
        out = ctx.lanczos_quadrature_precond(pr.SYSTEMS[name].kernel, g, h, rtol, maxit, **WANT)
        built, _, L = ctx.get_solver_preconditioner()
        assert built == pr.RANK and ctx.last_preconditioner_ms > 0
        return out, L
    finally:
        ctx.close()


def same(a, b):
    m = int(max(a["steps"].max(), b["steps"].max()))
    return (a["logdet_p"] == b["logdet_p"] and a["converged"] == b["converged"]
            and all(np.array_equal(a[k], b[k]) for k in KEYS[:6])
            and all(np.array_equal(a[k][:m], b[k][:m]) for k in KEYS[6:]))


@pytest.mark.parametrize("name, precision", [(s, plr.F64) for s in plr.SYSTEMS] + [(s, plr.F32) for s in plr.FLOAT32])
def test_logdet_p_and_probes(name, precision):
    """1. One iteration on the block of five; L is float64 in every context, so the formulas are the same in float32."""
    out, L = quadrature(name, 5, plr.UNREACHABLE, 1, precision)
    g, h = plr.block(5)
    z = plr.form(L, plr.DIAG, g, h)
    pz = pr.apply(L, plr.DIAG, z)
    rho0 = np.sum(z * pz, axis=0)
    ref = plr.logdet_p(L, plr.DIAG)
    errs = {"logdet_p": abs(out["logdet_p"] - ref) / abs(ref), "pz": kr.column_error(out["pz"], pz),
            "rho0": float(np.max(np.abs(out["wnorm2"] - rho0) / rho0))}
    print(f"[1] {name} {precision}: log det P {out['logdet_p']!r} (restatement {ref!r}); " +
          ", ".join(f"{k} {v:.3g} (allowed {plr.rounding_tolerance(k):.3g})" for k, v in errs.items()))
    assert np.all(np.isfinite(out["pz"])) and out["steps"].tolist() == [1] * 5 and not out["converged"]
    for k, v in errs.items():
        assert v <= plr.rounding_tolerance(k), (k, v)


def check(label, name, P, rtol, maxit, out, L):
    """2. Everything the entry returns against the restatement fed the device's L."""
    t = plr.case(name, P, rtol, maxit, L=L)
    tol, tol_x = plr.tolerance(name, rtol), plr.tolerance(name, rtol, plr.GX)
    nz = t.rho0 > 0
    errs = {
        "logquad": float(np.max(np.abs(out["logquad"] - t.logquad)[nz] / t.rho0[nz])),
        "invquad": float(np.max(np.abs(out["invquad"] - t.invquad)[nz] / np.abs(t.invquad[nz]))),
        "coefficients": max(lz.coefficient_error(out["alpha"], out["beta"], t, e, weighted=True) for e in range(P)),
    }
    err_x = kr.column_error(out["x"], t.x)
    print(f"[{label}] {name} P={P} rtol={rtol:g} maxit={maxit}: steps {out['steps'].tolist()} " +
          ", ".join(f"{k} {v:.3g}" for k, v in errs.items()) + f" (allowed {tol:.3g}); x {err_x:.3g} (allowed {tol_x:.3g})")
    assert np.array_equal(out["steps"], t.steps), (out["steps"], t.steps)
    assert out["converged"] == bool(np.all(t.frozen[nz] == plr.TOLERANCE))
    assert all(np.all(np.isfinite(out[k])) for k in ("logquad", "invquad", "wnorm2", "x", "pz"))
    assert kr.column_error(out["pz"], t.pz) <= plr.rounding_tolerance("pz")
    assert np.max(np.abs(out["wnorm2"] - t.rho0)[nz] / t.rho0[nz]) <= plr.rounding_tolerance("rho0")
    for k, v in errs.items():
        assert v <= tol, (k, v, tol)
    assert err_x <= tol_x, (err_x, tol_x)
    if P == 4:  # the zero column never starts
        assert out["steps"][3] == 0 and out["wnorm2"][3] == 0.0 and out["logquad"][3] == 0.0 and out["invquad"][3] == 0.0
        assert not out["x"][:, 3].any() and not out["pz"][:, 3].any()


@pytest.mark.parametrize("P", [4, 1, 5])
@pytest.mark.parametrize("name, rtol", plr.COMPARED)
def test_iterations_to_a_tolerance_against_the_restatement(name, rtol, P):
    out, L = quadrature(name, P, rtol, 1000)
    check("2", name, P, rtol, 1000, out, L)
    assert out["converged"]


@pytest.mark.parametrize("P", [4, 1, 5])
@pytest.mark.parametrize("maxit", plr.MAXITS)
@pytest.mark.parametrize("name", plr.SYSTEMS)
def test_iterations_around_the_first_burst_against_the_restatement(name, maxit, P):
    """2. maxit 7, 8, 9: NOT_CONVERGED with everything written."""
    out, L = quadrature(name, P, plr.UNREACHABLE, maxit)
    check("2", name, P, plr.UNREACHABLE, maxit, out, L)
    assert not out["converged"] and out["steps"].max() == maxit


@pytest.mark.parametrize("name, rtol", [(s, rtol) for s in plr.SYSTEMS for rtol in plr.RTOLS[s]])
def test_step_counts_at_the_tables_tolerances(name, rtol):
    """2b. The tolerances at which the restatement's count survives a product error of 10 TOL."""
    out, L = quadrature(name, 5, rtol, 1000)
    t = plr.case(name, 5, rtol, 1000, L=L)
    print(f"[2b] {name} rtol={rtol:g}: steps {out['steps'].tolist()} restatement {t.steps.tolist()}")
    assert out["converged"] and np.array_equal(out["steps"], t.steps)


@pytest.mark.parametrize("name", plr.SYSTEMS)
def test_estimates_and_steps_against_the_plain_entry(name):
    """3. 16 probes, seed and tolerance as test_precond_lanczos_reference.py fixed them."""
    kernel = pr.SYSTEMS[name].kernel
    g, h = plr.probes(plr.N, plr.RANK, plr.ESTIMATE_PROBES, plr.SEED)
    ctx = open_context(name)
    try:
        out = ctx.lanczos_quadrature_precond(kernel, g, h, plr.RATIO_RTOL, 1000)
        plain = ctx.lanczos_quadrature(kernel, lz.probes(plr.N, plr.ESTIMATE_PROBES, plr.SEED), plr.RATIO_RTOL, 5000)
    finally:
        ctx.close()
    root = np.sqrt(plr.ESTIMATE_PROBES)
    logdet, logdet_se = out["logdet_p"] + np.mean(out["logquad"]), np.std(out["logquad"], ddof=1) / root
    trinv, trinv_se = np.mean(out["invquad"]), np.std(out["invquad"], ddof=1) / root
    dense_logdet, dense_trinv = plr.dense(name)
    print(f"[3] {name}: log det {logdet:.4f} +- {logdet_se:.4f} (dense {dense_logdet:.4f}), tr A^-1 {trinv:.2f} +- {trinv_se:.2f} "
          f"(dense {dense_trinv:.2f}); steps {out['steps'].max()} against {plain['steps'].max()} of the plain entry; sample "
          f"deviation of logquad {np.std(out['logquad'], ddof=1):.3f} against {np.std(plain['logquad'], ddof=1):.3f}")
    assert out["converged"] and plain["converged"]
    assert abs(logdet - dense_logdet) <= 4 * logdet_se and abs(trinv - dense_trinv) <= 4 * trinv_se
    assert 2 * out["steps"].max() <= plain["steps"].max()


def test_nothing_else_moves():
    """4. The plain entry ignores the setting; a solve, a product and a dscale product are the same before and after the
    new call; the new call is reproducible and reuses the factor; a new diagonal or rank rebuilds it."""
    name, kernel = "G", "gaussian"
    z, a, signal = lz.probes(plr.N, 3, seed=2), pr.rhs(3), np.random.RandomState(14).randn(pr.N, 2)
    g, h = plr.block(5)

    def others(ctx):
        ctx.set_signal(signal)
        ctx.run(kernel, False)
        product = ctx.get_result(pr.N, 2)
        ctx.set_signal(signal)
        ctx.run_dscale(kernel)
        return product, ctx.get_result(pr.N, 2 * 3), ctx.cg_solve(kernel, a, 1e-8, 1000)

    fresh = _lib.Context(0)
    try:
        fresh.set_points(pr.points(name), None, _lib.KMVP_F64)
        fresh.set_solver_diagonal(pr.DIAG, 0.0)
        plain_fresh = fresh.lanczos_quadrature(kernel, z, 1e-6, 1000, want_x=True, want_coefficients=True)
    finally:
        fresh.close()
    ctx = open_context(name)
    try:
        plain_set = ctx.lanczos_quadrature(kernel, z, 1e-6, 1000, want_x=True, want_coefficients=True)
        assert ctx.last_preconditioner_rank == 0   # the plain entry built and used nothing
        before = others(ctx)
        first = ctx.lanczos_quadrature_precond(kernel, g, h, 1e-4, 1000, **WANT)
        ms_first, built = ctx.last_preconditioner_ms, ctx.last_preconditioner_rank
        second = ctx.lanczos_quadrature_precond(kernel, g, h, 1e-4, 1000, **WANT)
        ms_second = ctx.last_preconditioner_ms
        after = others(ctx)
        plain_after = ctx.lanczos_quadrature(kernel, z, 1e-6, 1000, want_x=True, want_coefficients=True)
        ctx.set_solver_diagonal(pr.DIAG, 0.05)
        shifted = ctx.lanczos_quadrature_precond(kernel, g, h, 1e-4, 1000, **WANT)
        ms_shifted = ctx.last_preconditioner_ms
        ctx.set_solver_preconditioner(16)
        lower = ctx.lanczos_quadrature_precond(kernel, g[:, :5], h[:16], 1e-4, 1000, **WANT)
        ms_lower, built_lower = ctx.last_preconditioner_ms, ctx.last_preconditioner_rank
    finally:
        ctx.close()
    m = int(plain_fresh["steps"].max())
    for other in (plain_set, plain_after):
        assert all(np.array_equal(plain_fresh[k], other[k]) for k in ("logquad", "invquad", "steps", "x"))
        assert np.array_equal(plain_fresh["alpha"][:m], other["alpha"][:m]) and np.array_equal(plain_fresh["beta"][:m], other["beta"][:m])
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert np.array_equal(before[2][0], after[2][0]) and before[2][1:] == after[2][1:]
    assert same(first, second) and first["converged"]
    assert ms_first == 0.0 and built == pr.RANK   # the solve of `before` had built the factor: reused
    assert ms_second == 0.0
    assert ms_shifted > 0 and shifted["converged"] and shifted["logdet_p"] > first["logdet_p"] and not same(first, shifted)
    assert ms_lower > 0 and built_lower == 16 and lower["converged"] and lower["steps"].max() >= shifted["steps"].max()
    # a context whose FIRST call is the new one builds the factor in it, and gives the same bits
    own, _ = quadrature(name, 5, 1e-4, 1000)
    assert same(own, first)


def test_long_run_graph_replay():
    """5. In the manner of test_long_pcg_graph_replay (the burst is captured after 64 bursts of 8; an unreachable tolerance
    runs to maxit): the history row is the device's own count, so the replayed burst writes the rows that the same run cut
    into calls below the capture threshold writes, bit for bit; and the first rows are the restatement's."""
    maxit, short = 560, 40
    y, d, g, h = plr.replay_system()
    ctx = _lib.Context(0)
    try:
        ctx.set_points(y, None, _lib.KMVP_F64)
        ctx.set_solver_diagonal(d, 0.0)
        ctx.set_solver_preconditioner(16)
        long = ctx.lanczos_quadrature_precond("gaussian", g, h, 1e-15, maxit, want_coefficients=True)
        cut = ctx.lanczos_quadrature_precond("gaussian", g, h, 1e-15, short, want_coefficients=True)
        built, _, L = ctx.get_solver_preconditioner()
    finally:
        ctx.close()
    assert built == 16 and long["steps"].tolist() == [maxit, maxit] and not long["converged"]
    assert cut["steps"].tolist() == [short, short]
    assert long["alpha"][maxit - 1].all() and long["beta"][maxit - 1].all()   # the last row was written, by a replayed burst
    assert np.all(np.isfinite(long["alpha"])) and np.all(np.isfinite(long["beta"]))
    assert np.array_equal(long["alpha"][:short], cut["alpha"]) and np.array_equal(long["beta"][:short], cut["beta"])
    t = plr.run(plr.replay_matrix(y, d), L, d, g, h, 1e-15, kr.BURST)
    err = max(lz.coefficient_error(long["alpha"], long["beta"], t, e, weighted=True) for e in range(2))
    tol = 4.0 * plr.REPLAY_G * kr.TOL[plr.F64]
    print(f"[5] first burst against the restatement: {err:.3g} (allowed {tol:.3g})")
    assert err <= tol


def test_refusals_through_the_c_abi():
    """6. Every refusal of include/kmvp.h, each with a message; a refused call leaves the factor and the setting."""
    lib = _lib.load()
    assert not hasattr(lib, "kmvp_invdist_lanczos_quadrature_precond")
    g, h = plr.block(4)
    h128 = np.ascontiguousarray(np.concatenate([h, np.zeros((128 - pr.RANK, 4))]))
    logdet = np.zeros(1)
    logq, invq, w2, steps = np.zeros(4), np.zeros(4), np.zeros(4), np.zeros(4, dtype=np.intc)

    def raw(ctx, gg=g, hh=h128, P=4, rtol=1e-4, maxit=50, out=(logdet, logq, invq, w2, steps)):
        ptr = [None if a is None else a.ctypes.data for a in (gg, hh) + tuple(out)]
        rc = lib.kmvp_gaussian_lanczos_quadrature_precond(ctx._ctx, ptr[0], ptr[1], P, rtol, maxit, ptr[2], ptr[3], ptr[4],
                                                          ptr[5], ptr[6], None, None, None, None)
        return rc, lib.kmvp_last_error(ctx._ctx).decode()

    ctx = open_context("G")
    try:
        good = ctx.lanczos_quadrature_precond("gaussian", g, h, 1e-4, 1000, **WANT)
        assert good["converged"] and ctx.last_preconditioner_rank == pr.RANK
        with pytest.raises(NotImplementedError):
            ctx.lanczos_quadrature_precond("inverse-distance", g, h, 1e-4, 50)
        with pytest.raises(ValueError):
            ctx.lanczos_quadrature_precond("gaussian", g[:100], h, 1e-4, 50)
        with pytest.raises(ValueError):
            ctx.lanczos_quadrature_precond("gaussian", g, h[:, :3], 1e-4, 50)
        full = (logdet, logq, invq, w2, steps)
        for kwargs in [{"P": 0}, {"P": -1}, {"gg": None}, {"hh": None}, {"rtol": 0.0}, {"rtol": -1.0}, {"maxit": -1}] + \
                [{"out": full[:i] + (None,) + full[i + 1:]} for i in range(5)]:
            rc, msg = raw(ctx, **kwargs)
            assert rc == 1 and msg, (kwargs, rc, msg)
        ctx.set_solver_preconditioner(0)
        rc, msg = raw(ctx)
        assert rc == 1 and "preconditioner" in msg, (rc, msg)
        ctx.set_solver_preconditioner(pr.RANK)
        ctx.set_solver_diagonal(None, 0.0)   # no diagonal
        rc, msg = raw(ctx)
        assert rc == 1 and "preconditioner" in msg and "diagonal" in msg, (rc, msg)
        d = pr.DIAG.copy()
        d[123] = 0.0
        ctx.set_solver_diagonal(d, 0.0)      # ridge + d_i == 0 at one point
        rc, msg = raw(ctx)
        assert rc == 1 and "diagonal" in msg, (rc, msg)
        ctx.set_solver_diagonal(pr.DIAG[:-1], 0.0)
        rc, msg = raw(ctx)
        assert rc == 1 and "diagonal" in msg, (rc, msg)
        ctx.set_solver_diagonal(pr.DIAG, 0.0)
        again = ctx.lanczos_quadrature_precond("gaussian", g, h, 1e-4, 1000, **WANT)   # rank and points survived all of it
        assert same(good, again) and ctx.last_preconditioner_rank == pr.RANK
        ctx.set_points(pr.points("G"), pr.points("G")[:100], _lib.KMVP_F64)   # targets != sources (clears rank and diagonal)
        ctx.set_solver_diagonal(pr.DIAG, 0.0)
        ctx.set_solver_preconditioner(pr.RANK)
        rc, msg = raw(ctx)
        assert rc == 1 and msg, (rc, msg)
        ctx.set_points(pr.points("G", "float32"), None, _lib.KMVP_BF16)
        ctx.set_solver_diagonal(pr.DIAG, 0.0)
        ctx.set_solver_preconditioner(pr.RANK)
        rc, msg = raw(ctx)
        assert rc == 2 and "float32 or float64" in msg, (rc, msg)
    finally:
        ctx.close()


def test_two_ranks_on_one_gpu():
    """7. Through the host transport, uneven shards."""
    out = _spawn([os.path.join(HERE, "_precond_lanczos_rank_worker.py")], world=2, timeout=600)
    rep = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
    print(json.dumps(rep))
    assert rep["world"] == 2 and rep["shards"] == [[0, 250], [250, 384]]
    assert rep["ranks_bitwise_equal"] and rep["converged"] and rep["rank_built"] == pr.RANK, rep
    assert rep["steps_equal_single"] and rep["product_free_equal_single"], rep
    assert max(rep["logquad_error"], rep["invquad_error"], rep["coefficient_error"]) <= rep["tolerance"], rep
    assert rep["x_error"] <= rep["x_tolerance"], rep


def test_plugin():
    """8. MI355XSolver on M52 with a scalar ridge, rank 32, 16 probes: the three methods with preconditioned=True within 4
    standard errors of the dense float64 objective and gradient; preconditioned=False bit for bit what a solver without a
    rank returns; ValueError without a rank."""
    kernel, ridge, probes, seed = "matern-5/2", plr.PLUGIN_RIDGE, plr.ESTIMATE_PROBES, plr.SEED
    y, a = pr.points("M52"), plr.plugin_rhs()
    out = {}
    for rank in (0, pr.RANK):
        algo = MI355XSolver(kernel=kernel, dimension=3, precision=np.float64, rtol=1e-8, maxit=2000, ridge=ridge,
                            preconditioner_rank=rank)
        try:
            algo.prepare_data(source_points=y)
            algo.fit()
            if rank:
                ld_first = algo.log_determinant(probes=probes, seed=seed, preconditioned=True)   # before any solve: builds
                info_first = algo._ctx.last_preconditioner_rank, algo._ctx.last_preconditioner_ms
            algo.prepare_query(target_signal=a)
            algo.query()
            res = dict(plain=(algo.log_determinant(probes=probes, seed=seed),
                              algo.log_marginal_likelihood(probes=probes, seed=seed),
                              algo.log_marginal_likelihood_gradient(probes=probes, seed=seed)))
            if rank:
                res["off"] = (algo.log_determinant(probes=probes, seed=seed, preconditioned=False),
                              algo.log_marginal_likelihood(probes=probes, seed=seed, preconditioned=False),
                              algo.log_marginal_likelihood_gradient(probes=probes, seed=seed, preconditioned=False))
                res["on"] = (algo.log_determinant(probes=probes, seed=seed, preconditioned=True),
                             algo.log_marginal_likelihood(probes=probes, seed=seed, preconditioned=True),
                             algo.log_marginal_likelihood_gradient(probes=probes, seed=seed, preconditioned=True))
                res["info"] = algo.get_additional()
            else:
                for call in (algo.log_determinant, algo.log_marginal_likelihood, algo.log_marginal_likelihood_gradient):
                    with pytest.raises(ValueError):
                        call(probes=probes, seed=seed, preconditioned=True)
            out[rank] = res
        finally:
            algo.done()

    def equal(u, v):
        return all(np.array_equal(np.asarray(p), np.asarray(q)) for p, q in zip(u, v))

    # preconditioned=False: today's path.  The probes' quadrature never sees the preconditioner, so the log-determinant
    # is that of the solver without a rank bit for bit; the likelihood also holds the solve's a'b, equal to rtol only.
    assert equal(out[pr.RANK]["off"][0], out[0]["plain"][0]) and equal(out[pr.RANK]["off"][0], out[pr.RANK]["plain"][0])
    assert out[pr.RANK]["off"][1] == out[pr.RANK]["plain"][1] and equal(out[pr.RANK]["off"][2], out[pr.RANK]["plain"][2])
    ld, (lml, lml_se), grad = out[pr.RANK]["on"]
    ld_plain = out[0]["plain"][0]
    assert equal(ld, ld_first) and info_first[0] == pr.RANK and info_first[1] > 0
    assert out[pr.RANK]["info"]["preconditioner_rank"] == pr.RANK

    A = pr.kernel_matrix("M52") + ridge * np.eye(pr.N)
    dA = dref.scale_derivative(kernel=kernel, source_points=y, source_signal=np.eye(pr.N))   # [i, j, d]
    lam, V = np.linalg.eigh(A)
    invA = (V / lam) @ V.T
    alpha = invA @ a
    E = a.shape[1]
    logdet, trinv = float(np.sum(np.log(lam))), float(np.sum(1.0 / lam))
    value = -0.5 * np.sum(a * alpha) - 0.5 * E * logdet - 0.5 * E * pr.N * np.log(2 * np.pi)
    exact = 0.5 * np.einsum("ie,ijd,je->d", alpha, dA, alpha) - 0.5 * E * np.einsum("ij,jid->d", invA, dA)
    exact_ridge = 0.5 * np.sum(alpha * alpha) - 0.5 * E * trinv
    dev = np.abs(grad.d_log_lengthscale - exact) / grad.d_log_lengthscale_stderr
    print(f"[8] log det {ld.value:.4f} +- {ld.stderr:.4f} in {ld.steps.max()} steps (plain {ld_plain.value:.4f} +- "
          f"{ld_plain.stderr:.4f} in {ld_plain.steps.max()}; dense {logdet:.4f}); tr A^-1 {ld.trace_inverse:.2f} +- "
          f"{ld.trace_inverse_stderr:.2f} (dense {trinv:.2f}); likelihood {lml:.4f} +- {lml_se:.4f} (dense {value:.4f}); "
          f"dL/dlog l {grad.d_log_lengthscale} +- {grad.d_log_lengthscale_stderr} (dense {exact}: {dev} stderr); dL/dridge "
          f"{grad.d_ridge:.4g} +- {grad.d_ridge_stderr:.3g} (dense {exact_ridge:.4g})")
    assert ld.converged and grad.converged
    assert abs(ld.value - logdet) <= 4 * ld.stderr and abs(ld.trace_inverse - trinv) <= 4 * ld.trace_inverse_stderr
    assert abs(lml - value) <= 4 * lml_se and lml_se == 0.5 * E * ld.stderr
    assert abs(grad.value - value) <= 4 * grad.value_stderr and abs(grad.value - lml) <= 1e-9 * abs(lml)
    assert (dev <= 4).all() and abs(grad.d_ridge - exact_ridge) <= 4 * grad.d_ridge_stderr
    assert 2 * ld.steps.max() <= ld_plain.steps.max() and ld.stderr < ld_plain.stderr
