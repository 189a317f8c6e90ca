"""GPU tests of Wendland's compactly supported kernels (include/kmvp.h kmvp_wendland_<c>_cutoff, kmvp_wendland_<c>_cg_solve;
lowd_cutoff_kernel with wendland_value, csrc/kmvp_lowd_cutoff.hpp).

Products are held, element by element, to the model of tests/wendland_model.py -- the float64 product and a band derived
from the kernel's own sequence of operations; solves to a float64 residual of this file's own on the dense matrix of
tests/wendland_reference.py and to the iteration count of the float64 CG restatement (tests/krylov_reference.py).  No
tolerance of this file's own, with one addition stated at dense_residual()."""
import ctypes
import os

import numpy as np
import pytest

import krylov_reference as kr
import wendland_model as wm
import wendland_reference as wr
from kernel_matrix_benchmarks_amd import _lib
from kernel_matrix_benchmarks_amd.algorithms.mi355x import MI355XProduct, MI355XSolver

pytestmark = pytest.mark.gpu

PREC = {"f32": np.float32, "f64": np.float64}
INVALID, UNSUPPORTED, NOT_CONVERGED = 1, 2, 6
C2, C4 = wr.KERNELS
MODES = (("product", 1), ("product", 3), ("norm", 1), ("norm", 3), ("density", 1))


def codes(precision):
    return (_lib.KMVP_F64, np.float64) if np.dtype(precision) == np.float64 else (_lib.KMVP_F32, np.float32)


def rounded(a, precision):
    return np.asarray(a, dtype=precision).astype(np.float64)


def bits(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


class Ctx:
    """One context on sources y (M, D) and targets x (N, D) -- None: the targets are the sources."""

    def __init__(self, y, x, precision):
        self.dtype, self.npdt = codes(precision)
        self.ctx = _lib.Context(0)
        try:
            self.ctx.set_points(np.ascontiguousarray(y, dtype=self.npdt), None if x is None else np.ascontiguousarray(x, dtype=self.npdt),
                                self.dtype)
        except Exception:
            self.ctx.close()
            raise

    def product(self, kernel, R, normalise, b):
        """b: (M, E), or None for density estimation.  (N, E) float64."""
        self.ctx.set_signal(None if b is None else np.ascontiguousarray(b, dtype=self.npdt))
        self.ctx.run_cutoff(kernel, R, normalise)
        if self.ctx.N > 0:
            assert self.ctx.last_kernel_name == "lowd_cutoff_kernel"
        return self.ctx.get_result(self.ctx.N, 1 if b is None else b.shape[1])

    def solve(self, kernel, R, a, rtol, maxit=3000):
        out = self.ctx.cg_solve(kernel, np.ascontiguousarray(a, dtype=self.npdt), rtol, maxit, support_radius=R)
        assert self.ctx.last_kernel_name == "lowd_cutoff_kernel"
        return out

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.close()


# ---- 1. products inside the model's band -----------------------------------------------------------------------------------
def product_cloud(D, precision, same):
    """M = 3001 sources, N = 2999 targets (or the sources themselves), uniform in the unit cube, a mean of about 24 inside R;
    the last target of a separate cloud sits far outside: a row with nothing inside."""
    rs = np.random.RandomState(40 + D)
    y = rounded(rs.rand(3001, D), precision)
    x = None
    if not same:
        x = rounded(rs.rand(2999, D), precision)
        x[-1] = 5.0
    return y, x, wr.radius_for(3001, D, 24), rounded(rs.randn(3001, 3), precision)


@pytest.mark.parametrize("prec", list(PREC))
@pytest.mark.parametrize("D", (1, 2, 3))
def test_products_inside_the_model_band(D, prec):
    """C2 and C4 x product / normalised / density, E = 1 and 3, targets = sources and targets != sources, cell factors 1 and
    2: every element within wendland_model's band of its value; a row with nothing inside is 0, NaN when normalised."""
    precision = PREC[prec]
    chunk, worst, checked = 512, 0.0, 0
    for same in (True, False):
        y, x, R, b3 = product_cloud(D, precision, same)
        with Ctx(y, x, precision) as ct:
            for kernel in wr.KERNELS:
                prs = wm.pairs(kernel, y, x, R, precision)
                empty = np.bincount(prs.i, minlength=prs.N) == 0
                assert empty.sum() == (0 if same else 1)
                for factor in (1.0, 2.0):
                    ct.ctx.set_option("cutoff_cell_factor", factor)
                    models = {}
                    for sig, E in MODES:
                        b = None if sig == "density" else b3[:, :E]
                        got = ct.product(kernel, R, sig == "norm", b)
                        assert got.shape == (prs.N, E)
                        info = ct.ctx.cutoff_info()
                        folds = info["records"] // chunk + 3 ** (D - 1) + 1     # per row: one per chunk walked and one per run at most
                        if sig not in models:   # (the model's columns are independent: E = 3 serves E = 1)
                            models[sig] = wm.product(kernel, y, x, None if sig == "density" else b3, R, sig == "norm",
                                                     precision=precision, chunk=chunk, folds=folds, prs=prs)
                        value, band = models[sig].value[:, :E], models[sig].band[:, :E]
                        live = ~empty
                        err = np.abs(got[live] - value[live])
                        assert np.isfinite(got[live]).all()
                        with np.errstate(divide="ignore", invalid="ignore"):
                            ratio = float(np.max(np.where(err > 0, err / band[live], 0.0)))
                        worst, checked = max(worst, ratio), checked + err.size
                        assert (err <= band[live]).all(), (kernel, same, factor, sig, E, ratio)
                        if empty.any():
                            assert np.all(np.isnan(got[empty])) if sig == "norm" else np.all(got[empty] == 0)
    print(f"\nwendland model band D={D} {prec}: {checked} elements, worst err / band {worst:.3f}")
    assert checked > 0


# ---- 2. the support is exact ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", list(PREC))
def test_exact_support(prec):
    """32 probe targets; the sources farther than R (1 + 2^-16) from every probe carry a signal of 1e30, or 0 (removed from
    the sum): the probes' rows are the base signal's rows bit for bit, in the product and in the normalised product."""
    precision = PREC[prec]
    y, _, R, b3 = product_cloud(3, precision, True)
    rs = np.random.RandomState(5)
    probes = rs.choice(len(y), 32, replace=False)
    far = (wr.sqdists(y[probes], y) > (R * (1.0 + 2.0 ** -16)) ** 2).all(axis=0)
    assert 30 < far.sum() < len(y) - 50
    b = b3[:, :2]
    huge, gone = b.copy(), b.copy()
    huge[far], gone[far] = 1e30, 0.0
    with Ctx(y, None, precision) as ct:
        for kernel, normalise in ((C2, False), (C4, True)):
            base, got, cut = ct.product(kernel, R, normalise, b), ct.product(kernel, R, normalise, huge), ct.product(kernel, R, normalise, gone)
            assert bits(got[probes], base[probes]) and bits(cut[probes], base[probes]), kernel
            assert not bits(got, base)          # (the huge signal did reach the rows it is inside of)


# ---- 3. solves -------------------------------------------------------------------------------------------------------------------
def dense_residual(kernel, y, R, K, precision, diag, a, sol, rtol):
    """(residual, bound): this file's float64 residual max_e |a - (K + diag) b| / |a| on the dense matrix K, and 1.5 rtol plus
    the model's band on K b relative to |a|.  The one addition: the operator takes b rounded to the working precision
    (cutoff_signal_f64_kernel), |K (b' - b)| <= u K |b| = u mass elementwise in float32 -- charged with the band."""
    r = a - (K @ sol + np.reshape(diag, (-1, 1)) * sol)
    m = wm.product(kernel, y, None, sol, R, precision=precision, folds=8)
    slack = m.band + (wm.unit(precision) * m.mass if precision == np.float32 else 0.0)
    norm = np.linalg.norm(a, axis=0)
    return float(np.max(np.linalg.norm(r, axis=0) / norm)), 1.5 * rtol + float(np.max(np.linalg.norm(slack, axis=0) / norm))


@pytest.mark.parametrize("case", list(wr.SOLVE_CASES))
def test_solves(case):
    """KMVP_OK; the float64 residual on the dense matrix within dense_residual's bound; the iteration count of the float64 CG
    restatement on the dense matrix, as test_gpu_krylov.py asks of the other kernels (==), on draws where that count is
    reproducible (wendland_reference.SOLVE_CASES).  Reference counts: D = 3 bare 176, D = 3 with a ridge 106 .. 115, D = 1
    279, float32 at 1e-4 65 and 76."""
    prec, D, kernel, ridge, rtol, E, seed = wr.SOLVE_CASES[case]
    y, R, a, diag, K = wr.solve_system(case)
    with Ctx(y, None, PREC[prec]) as ct:
        if ridge == "d":
            ct.ctx.set_solver_diagonal(diag, 0.0)
        elif ridge:
            ct.ctx.set_solver_diagonal(None, ridge)
        sol, iters, resid, ok = ct.solve(kernel, R, a, rtol)
    ref = kr.cg(K + np.diag(diag), a, rtol, 3000)
    mine, bound = dense_residual(kernel, y, R, K, PREC[prec], diag, a, sol, rtol)
    print(f"\n[{case}] iters {iters} (reference {ref.iters}) ok {ok} resid {resid:.4g} dense float64 residual {mine:.4g} bound {bound:.4g}")
    assert ok and np.all(np.isfinite(sol)) and resid <= 1.5 * rtol
    assert mine <= bound, (mine, bound)
    assert iters == ref.iters, (iters, ref.iters)


def test_long_solve_graph_replay():
    """D = 2, C2, a mean of 32 inside, no ridge, float64: the solve runs past 512 iterations (the float64 CG restatement takes
    1367 on this draw), so its bursts are replayed as a hipGraph -- the same bits with KMVP_NO_GRAPH=1."""
    y, R, a3 = wr.solve_cloud(2, "f64", 62, 32)
    a = np.ascontiguousarray(a3[:, :1])
    outs = []
    for no_graph in (False, True):
        if no_graph:
            os.environ["KMVP_NO_GRAPH"] = "1"
        else:
            os.environ.pop("KMVP_NO_GRAPH", None)
        try:
            with Ctx(y, None, np.float64) as ct:
                sol, iters, resid, ok = ct.solve(C2, R, a, 1e-6, 5000)
        finally:
            os.environ.pop("KMVP_NO_GRAPH", None)
        print(f"\n[graph replay, KMVP_NO_GRAPH={int(no_graph)}] iters {iters} resid {resid:.4g} ok {ok}")
        assert ok and iters > 600
        outs.append((sol, iters, resid))
    assert np.array_equal(outs[0][0], outs[1][0]) and outs[0][1:] == outs[1][1:]


# ---- 4. bits -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", list(PREC))
def test_bitwise_and_the_other_entries_untouched(prec):
    """A repeated solve returns the same bits; a kmvp_gaussian_cutoff, a plain product and a kmvp_nearest return the same bits
    before and after a Wendland solve at a different radius (the Gaussian cutoff repacks its own signal: the records' signal
    slots held a Krylov vector); a Wendland product after the solve is the one before it."""
    precision = PREC[prec]
    y, R, a3 = wr.solve_cloud(3, prec, 71)
    y = y[:700]
    a = np.ascontiguousarray(a3[:700, :2])
    b = rounded(np.random.RandomState(13).randn(700, 2), precision)
    Rg, Rs = 0.21, 0.3

    def others(ct):
        out = [ct.product("gaussian", Rg, False, b), ct.product(C4, Rg, True, b)]
        ct.ctx.run("gaussian", False)
        out.append(ct.ctx.get_result(ct.ctx.N, 2))
        idx, sq = ct.ctx.run_nearest(4)
        return out + [idx.astype(np.float64), sq]

    with Ctx(y, None, precision) as ct:
        ct.ctx.set_solver_diagonal(None, 1e-2)
        before = others(ct)
        first = ct.solve(C2, Rs, a, 1e-5)
        between = others(ct)
        again = ct.solve(C2, Rs, a, 1e-5)
        # the Gaussian cutoff straight after a solve at ITS radius and record length: plan and coordinates are cached, the signal is not
        ct.ctx.set_signal(np.ascontiguousarray(b, dtype=ct.npdt))
        ct.ctx.run_cutoff("gaussian", Rs, False)
        at_rs = ct.ctx.get_result(700, 2)
        after = others(ct)
        assert first[3] and bits(first[0], again[0]) and first[1:] == again[1:]
        for u, v, w in zip(before, between, after):
            assert bits(u, v) and bits(u, w)
    with Ctx(y, None, precision) as fresh:
        assert bits(at_rs, fresh.product("gaussian", Rs, False, b))
        fresh.ctx.set_solver_diagonal(None, 1e-2)
        assert bits(first[0], fresh.solve(C2, Rs, a, 1e-5)[0])


# ---- 5. non-finite points ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", list(PREC))
def test_non_finite_points(prec):
    """A NaN point follows the cutoff's rules in the product: as a target a NaN row, as a source in no sum, every other row
    the bits of the cloud without it.  In the solve it is a NaN row of the operator: KMVP_E_NOT_CONVERGED, out_b written."""
    precision = PREC[prec]
    rs = np.random.RandomState(17)
    yf, R = rounded(rs.rand(300, 3), precision), 0.25
    bf = rounded(rs.randn(300, 2), precision)
    y = np.insert(yf, 100, [[0.5, np.nan, 0.5]], axis=0)
    b = np.insert(bf, 100, [[1.0, -1.0]], axis=0)
    keep = np.arange(301) != 100
    with Ctx(yf, None, precision) as base, Ctx(y, None, precision) as ct:
        for kernel, normalise in ((C2, False), (C4, True)):
            want, got = base.product(kernel, R, normalise, bf), ct.product(kernel, R, normalise, b)
            assert bits(got[keep], want) and np.all(np.isnan(got[100])), kernel
        a = np.ascontiguousarray(b, dtype=ct.npdt)
        out = np.full((301, 2), -7.0)
        iters, resid = ctypes.c_int(-1), ctypes.c_double(-1.0)
        ct.ctx.set_solver_diagonal(None, 1e-2)
        rc = ct.ctx._lib.kmvp_wendland_c2_cg_solve(ct.ctx._ctx, R, a.ctypes.data, 2, 1e-6, 100, out.ctypes.data, ctypes.byref(iters),
                                                   ctypes.byref(resid))
        assert rc == NOT_CONVERGED and not (out == -7.0).any() and not np.isfinite(resid.value)
        assert "finite" in ct.ctx._lib.kmvp_last_error(ct.ctx._ctx).decode()
        sol, _, _, ok = ct.solve(C2, R, a, 1e-6, 100)        # and through the wrapper: no exception, not converged
        assert not ok


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------
def small_context(rs, D=3, dtype=_lib.KMVP_F32, E=1, comm=False, M_total=None, batches=False, same=True, signal=True):
    ctx = _lib.Context(0)
    try:
        if comm:   # the rehearsal transport: a communicator of one rank without loading RCCL
            ctx.comm_init_host(lambda buf, op: None, 0, 1)
        y = np.ascontiguousarray(rs.rand(40, D), dtype=np.float32)
        ctx.set_points(y, None if same else np.ascontiguousarray(rs.rand(30, D), dtype=np.float32), dtype, 0, M_total)
        if signal:
            ctx.set_signal(np.ascontiguousarray(rs.randn(40, E), dtype=np.float32))
        if batches:
            ctx.set_batches([0, 10, 40])
    except Exception:
        ctx.close()
        raise
    return ctx


def refused(ctx, call, code, *words):
    with pytest.raises(_lib.KmvpError) as e:
        call()
    msg = ctx._lib.kmvp_last_error(ctx._ctx).decode()
    assert e.value.code == code, (e.value.code, msg)
    for w in words:
        assert w in msg, (w, msg)


def rhs(n, E=1):
    return np.ascontiguousarray(np.random.RandomState(3).randn(n, E), dtype=np.float32)


NOT_BUILT = {"D4": (dict(D=4), "D = 4"), "bfloat16": (dict(D=16, dtype=_lib.KMVP_BF16), "bfloat16"),
             "communicator": (dict(comm=True), "communicator"), "source_slice": (dict(M_total=50), "M < M_total"),
             "batches": (dict(batches=True), "kmvp_set_batches")}


@pytest.mark.parametrize("case", list(NOT_BUILT))
def test_unsupported(case):
    """Everything cutoff_unsupported refuses, for the product and for the solve: KMVP_E_UNSUPPORTED, the cutoff and the cause
    named."""
    kwargs, word = NOT_BUILT[case]
    ctx = small_context(np.random.RandomState(23), **kwargs)
    try:
        refused(ctx, lambda: ctx.run_cutoff(C2, 0.3, False), UNSUPPORTED, "cutoff", word)
        refused(ctx, lambda: ctx.run_cutoff(C4, 0.3, True), UNSUPPORTED, "cutoff", word)
        refused(ctx, lambda: ctx.cg_solve(C2, rhs(ctx.N), 1e-4, 10, support_radius=0.3), UNSUPPORTED, "cutoff", word)
        refused(ctx, lambda: ctx.cg_solve(C4, rhs(ctx.N), 1e-4, 10, support_radius=0.3), UNSUPPORTED, "cutoff", word)
    finally:
        ctx.close()


def test_refusals_of_the_library():
    """E > 4 (product and solve) and a preconditioner of rank > 0: KMVP_E_UNSUPPORTED.  A bad radius and targets that are not
    the sources: KMVP_E_INVALID.  kmvp_fit takes the codes 7 and 8 and builds nothing, refuses 5, 6 and 9.  No plain product."""
    rs = np.random.RandomState(29)
    ctx = small_context(rs, E=5)
    try:
        refused(ctx, lambda: ctx.run_cutoff(C2, 0.3, False), UNSUPPORTED, "cutoff", "E = 5")
        refused(ctx, lambda: ctx.cg_solve(C2, rhs(40, 5), 1e-4, 10, support_radius=0.3), UNSUPPORTED, "cutoff", "E = 5")
        ctx.set_solver_diagonal(None, 1e-2)
        ctx.set_solver_preconditioner(8)
        refused(ctx, lambda: ctx.cg_solve(C4, rhs(40), 1e-4, 10, support_radius=0.3), UNSUPPORTED, "preconditioner", "Wendland")
        ctx.set_solver_preconditioner(0)
        assert ctx.cg_solve(C4, rhs(40), 1e-4, 100, support_radius=0.3)[3]        # ... and without it the same call solves
        for radius in (0.0, -1.0, np.nan, np.inf):
            refused(ctx, lambda: ctx.cg_solve(C2, rhs(40), 1e-4, 10, support_radius=radius), INVALID, "radius")
            refused(ctx, lambda: ctx.run_cutoff(C2, radius, False), INVALID, "radius")
        refused(ctx, lambda: ctx.cg_solve(C2, rhs(40), -1.0, 10, support_radius=0.3), INVALID, "solver arguments")
        ctx.fit(C2)
        ctx.fit(C4)
        assert ctx._lib.kmvp_fit(ctx._ctx, 7) == 0 and ctx._lib.kmvp_fit(ctx._ctx, 8) == 0
        for code in (5, 6, 9):
            assert ctx._lib.kmvp_fit(ctx._ctx, code) == INVALID
        with pytest.raises(NotImplementedError, match="run_cutoff"):
            ctx.run(C2, False)
        with pytest.raises(ValueError, match="support_radius"):
            ctx.cg_solve(C2, rhs(40), 1e-4, 10)
        with pytest.raises(ValueError, match="support_radius"):
            ctx.cg_solve("gaussian", rhs(40), 1e-4, 10, support_radius=0.3)
    finally:
        ctx.close()
    ctx = small_context(rs, same=False)
    try:
        refused(ctx, lambda: ctx.cg_solve(C2, rhs(30), 1e-4, 10, support_radius=0.3), INVALID, "x == NULL")
    finally:
        ctx.close()
    ctx = _lib.Context(0)
    try:
        refused(ctx, lambda: ctx.cg_solve(C2, rhs(30), 1e-4, 10, support_radius=0.3), INVALID, "kmvp_set_points")
    finally:
        ctx.close()


def test_refusals_of_the_plugin():
    """MI355XProduct: query() and the other kernel-dependent queries name query_cutoff.  MI355XSolver: support_radius is
    required for the Wendland kernels and refused for the others; refine, preconditioner_rank > 0 and comm are refused."""
    rs = np.random.RandomState(31)
    y, b = rs.rand(200, 3), rs.randn(200, 2)
    algo = MI355XProduct(kernel=C2, dimension=3, precision=np.float32)
    try:
        algo.prepare_data(source_points=y, target_points=y, same_points=True)
        algo.fit()
        algo.prepare_query(source_signal=b)
        for method in ("query", "query_gradient", "query_scale_derivative", "query_logsumexp", "query_logsumexp_gradient"):
            with pytest.raises(NotImplementedError, match="query_cutoff"):
                getattr(algo, method)()
        algo.query_cutoff(0.3)
        assert algo.get_result().shape == (200, 2)
    finally:
        algo.done()
    with pytest.raises(NotImplementedError, match="bfloat16"):
        MI355XProduct(kernel=C4, dimension=3, precision="bfloat16")
    with pytest.raises(NotImplementedError, match="fast_sqdists"):
        MI355XProduct(kernel=C4, dimension=3, fast_sqdists=True)
    with pytest.raises(ValueError, match="support_radius"):
        MI355XSolver(kernel=C2, dimension=3)
    with pytest.raises(ValueError, match="support_radius"):
        MI355XSolver(kernel=C2, dimension=3, support_radius=-1.0)
    with pytest.raises(ValueError, match="support_radius"):
        MI355XSolver(kernel="gaussian", dimension=3, support_radius=0.3)
    with pytest.raises(NotImplementedError, match="refine"):
        MI355XSolver(kernel=C2, dimension=3, support_radius=0.3, refine="float32")
    with pytest.raises(NotImplementedError, match="preconditioner_rank"):
        MI355XSolver(kernel=C2, dimension=3, support_radius=0.3, ridge=1e-2, preconditioner_rank=4)
    with pytest.raises(NotImplementedError, match="comm"):
        MI355XSolver(kernel=C2, dimension=3, support_radius=0.3, comm=object())
    solver = MI355XSolver(kernel=C4, dimension=3, support_radius=0.3, ridge=1e-2)
    with pytest.raises(NotImplementedError):
        solver.set_query_arguments(preconditioner_rank=4)
    with pytest.raises(NotImplementedError, match="wendland-c4"):
        solver.log_determinant()


# ---- 7. the plugin ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", (np.float16, np.float32, np.float64), ids=lambda p: np.dtype(p).name)
def test_plugin(precision):
    """MI355XProduct.query_cutoff and MI355XSolver against the _lib calls on the same (rounded) inputs, bit for bit."""
    rs = np.random.RandomState(37)
    y, x, b, a, R = rs.rand(500, 3), rs.rand(200, 3), rs.randn(500, 2), rs.randn(500, 2), 0.2
    work = np.float64 if np.dtype(precision) == np.float64 else np.float32
    yr, xr, br, ar = rounded(y, precision), rounded(x, precision), rounded(b, precision), rounded(a, precision)
    for normalize in (False, True):
        algo = MI355XProduct(kernel=C4, dimension=3, precision=precision, normalize_rows=normalize)
        try:
            algo.prepare_data(source_points=y, target_points=x, same_points=False)
            algo.fit()
            algo.prepare_query(source_signal=b)
            algo.query_cutoff(R)
            got, extra = algo.get_result(), algo.get_additional()
            assert got.shape == (200, 2) and got.dtype == np.float64 and extra["device_kernel"] == "lowd_cutoff_kernel"
            assert extra["cutoff_walked"] > 0
        finally:
            algo.done()
        with Ctx(yr, xr, work) as ct:
            assert bits(got, ct.product(C4, R, normalize, br))
        m = wm.product(C4, yr, xr, br, R, normalize, precision=work, folds=8)
        assert (np.abs(got - m.value) <= m.band).all()
    solver = MI355XSolver(kernel=C2, dimension=3, precision=precision, support_radius=R, ridge=1e-2, rtol=1e-4)
    try:
        solver.prepare_data(source_points=y)
        solver.fit()
        solver.prepare_query(target_signal=a)
        solver.query()
        sol = solver.get_result()
        assert solver.converged and sol.shape == (500, 2) and sol.dtype == np.float64 and "ridge=0.01" in solver.name
        assert solver.get_additional()["device_kernel"] == "lowd_cutoff_kernel"
    finally:
        solver.done()
    with Ctx(yr, None, work) as ct:
        ct.ctx.set_solver_diagonal(None, 1e-2)
        ref, iters, resid, ok = ct.solve(C2, R, ar, 1e-4)
        assert ok and bits(sol, ref) and iters == solver.iterations
    mine, bound = dense_residual(C2, yr, R, wr.kernel_matrix(C2, yr, R), work, np.full(500, 1e-2), ar, sol, 1e-4)
    assert mine <= bound, (mine, bound)
