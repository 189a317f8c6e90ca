"""GPU tests of the device-resident Sinkhorn iteration (kmvp_sinkhorn.hip, include/kmvp.h kmvp_<kernel>_sinkhorn,
MI355XSinkhorn) against the float64 numpy restatement of the iteration (sinkhorn_reference.py, itself checked against the
textbook scaling-domain iteration in test_sinkhorn_reference.py).

The measure is, per entry, |u - u_ref| / max(1, |u_ref|), as in test_gpu_lse.py.  Every half-step is the log-sum-exp, held
there to TOL64 = 1e-11 / TOL32 = 1e-5 on that measure, and T1, T2 are non-expansive in the sup norm, so after k iterations
(2k half-steps) of potentials no larger than P

    max |u - u_ref|, max |v - v_ref|  <=  2 k TOL max(1, P)

with u_ref, v_ref and P from the restatement run for exactly the GPU's iteration count (tol = 0); for float32 the
restatement runs on the float32-rounded points.  The one-step check does not accumulate: the returned v against the
restatement's T2 of the returned u, at the log-sum-exp's own tolerance.
"""
import numpy as np
import pytest

import lse_grad_reference
import lse_reference
import sinkhorn_reference as sr
from conftest import rel_err
from kernel_matrix_benchmarks_amd import _lib
from kernel_matrix_benchmarks_amd.algorithms.mi355x import MI355XSinkhorn

import kmvp_oracle

pytestmark = pytest.mark.gpu

TOL64 = 1e-11
TOL32 = 1e-5
KERNELS = lse_reference.KERNELS
DTYPES = ((_lib.KMVP_F64, np.float64, TOL64), (_lib.KMVP_F32, np.float32, TOL32))
DTYPE_IDS = ("float64", "float32")


def rounded(a, npdt):
    return np.asarray(a, dtype=npdt).astype(np.float64)


def measure(got, want):
    assert got.shape == want.shape and np.isfinite(got).all() and np.isfinite(want).all(), (got.shape, want.shape)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


def sup(got, want):
    assert got.shape == want.shape and np.isfinite(got).all(), got.shape
    return float(np.max(np.abs(got - want)))


def bound(k, tol, P):
    return 2 * k * tol * max(1.0, P)


def solve(kernel, x, y, la, lb, dtype, tol, maxit, u0=None, options=(), ctx=None):
    """Through the C ABI's typed wrapper on the (already scaled) points; x is None: same points."""
    npdt = np.float64 if dtype == _lib.KMVP_F64 else np.float32
    own = ctx is None
    if own:
        ctx = _lib.Context(0)
    try:
        if own:
            for key, value in options:
                ctx.set_option(key, value)
            ctx.set_points(np.ascontiguousarray(y, dtype=npdt), None if x is None else np.ascontiguousarray(x, dtype=npdt), dtype)
        u, v, iters, err, converged = ctx.sinkhorn(kernel, la, lb, tol, maxit, u0)
        assert ctx.last_kernel_name == "lowd_lse_kernel" and ctx.last_dispatch_note == ""
        assert ctx.last_total_ms > 0 and ctx.last_kernel_ms == ctx.last_total_ms
        assert u.dtype == np.float64 and v.dtype == np.float64 and 1 <= iters <= maxit
        return u, v, iters, err, converged
    finally:
        if own:
            ctx.close()


_REF = {}


def reference(key, **kw):
    """One restatement run per distinct case, shared by the tests that need it and never modified."""
    if key not in _REF:
        _REF[key] = sr.sinkhorn(**kw)
    return _REF[key]


def one_step_tolerance(kernel, x, y, u, la, npdt, want):
    if npdt == np.float64:
        return TOL64
    own, _ = sr.half_step(kernel, y, x, u, la, precision=np.float32)
    return max(TOL32, 2 * measure(own, want))


def check_against_restatement(label, kernel, x, y, la, lb, got, npdt, TOL, key, one_step=True):
    """The accumulation bound at the GPU's own iteration count, and the one-step check; returns the exact-k restatement."""
    u, v, iters, err, _ = got
    ref = reference(key + (iters,), kernel=kernel, x=x, y=y, log_a=la, log_b=lb, tol=0.0, maxit=iters)
    assert ref.iters == iters
    lim = bound(iters, TOL, ref.P)
    du, dv = sup(u, ref.u), sup(v, ref.v)
    print(f"{label}: k = {iters}, P = {ref.P:.4g}, |u - u_ref| {du:.3e}, |v - v_ref| {dv:.3e} (bound {lim:.3e}); "
          f"err {err:.3e} (restatement {ref.errs[-1]:.3e})")
    assert du <= lim and dv <= lim, (label, du, dv, lim)
    if not one_step:
        return ref
    want_v, _ = sr.half_step(kernel, y, x, u, sr.log_weights(len(u), la))
    step_tol = one_step_tolerance(kernel, x, y, u, sr.log_weights(len(u), la), npdt, want_v)
    step = measure(v, want_v)
    print(f"{label}: one step, v against T2(u) of the restatement {step:.3e} (tolerance {step_tol:.1e})")
    assert step <= step_tol, (label, step, step_tol)
    return ref


# ---- the four documented cases -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,npdt,TOL", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("kernel,eps", sr.TABLE)
def test_documented_cases(kernel, eps, dtype, npdt, TOL):
    x, y, la, lb = sr.table_case(kernel, eps)
    x, y = rounded(x, npdt), rounded(y, npdt)
    tol = 1e-8 if dtype == _lib.KMVP_F64 else 1e-4
    got = solve(kernel, x, y, la, lb, dtype, tol, 1000)
    u, v, iters, err, converged = got
    label = f"{kernel} eps={eps} {np.dtype(npdt).name}"
    assert converged and err <= tol, (label, iters, err)
    ref_tol = reference((kernel, eps, npdt, "tol"), kernel=kernel, x=x, y=y, log_a=la, log_b=lb, tol=tol, maxit=1000)
    print(f"{label}: {iters} iterations (restatement {ref_tol.iters})")
    assert ref_tol.converged and abs(iters - ref_tol.iters) <= 1, (label, iters, ref_tol.iters)
    check_against_restatement(label, kernel, x, y, la, lb, got, npdt, TOL, (kernel, eps, npdt))
    if dtype == _lib.KMVP_F64:
        again = sr.row_violation(kernel, x, y, la, lb, u, v)
        print(f"{label}: row violation of the returned plan in numpy {again:.6e}, reported {err:.6e}")
        assert abs(again - err) <= 0.01 * err, (label, again, err)


# ---- shapes ------------------------------------------------------------------------------------------------------------
def random_case(seed, N, M, D, same=False):
    rs = np.random.RandomState(seed)
    y = rs.rand(M, D) * 3.0
    x = None if same else rs.rand(N, D) * 3.0 + 0.3
    a, b = rs.rand(M if same else N) + 0.1, rs.rand(M) + 0.1
    return x, y, np.log(a / a.sum()), np.log(b / b.sum())


@pytest.mark.parametrize("dtype,npdt,TOL", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_small_shapes(kernel, dtype, npdt, TOL):
    """same_points at N = M = 130, D = 2; D = 1 and D = 8 at N = 70, M = 33; one target; one source."""
    tol = 1e-8 if dtype == _lib.KMVP_F64 else 1e-4
    for seed, (N, M, D, same) in enumerate(((130, 130, 2, True), (70, 33, 1, False), (70, 33, 8, False), (1, 33, 3, False),
                                            (70, 1, 3, False))):
        x, y, la, lb = random_case(50 + seed, N, M, D, same)
        y = rounded(y, npdt)
        x = None if same else rounded(x, npdt)
        got = solve(kernel, x, y, la, lb, dtype, tol, 1000)
        label = f"{kernel} {np.dtype(npdt).name} N={N} M={M} D={D} same={same}"
        assert got[4] and got[0].shape == (N,) and got[1].shape == (M,), (label, got[2], got[3])
        check_against_restatement(label, kernel, y if same else x, y, la, lb, got, npdt, TOL, (kernel, seed, npdt))


@pytest.mark.parametrize("dtype,npdt,TOL", DTYPES, ids=DTYPE_IDS)
def test_several_segments_and_ragged_pads(dtype, npdt, TOL):
    """N = 3000, M = 5001, D = 3, chunk = 256 with 3 and with 24 segments (below and above SEG_SPLIT_FROM, ragged pad
    records, both directions on several segments), two iterations (tol = 0): each within the bound of the restatement, and
    the two segment counts within the SAME bound of each other (a cross-check of the segment merge that does not follow
    from the first) -- not bitwise: the segments change the order of the sums.  The points are
    float32 numbers for both precisions, so that one restatement run (seconds at this size) serves all four solves; the
    one-step check is left to the small cases."""
    kernel = "gaussian"
    x, y, la, lb = random_case(70, 3000, 5001, 3)
    x, y = rounded(x * 2.0, np.float32), rounded(y * 2.0, np.float32)
    k = 2
    runs = {}
    for seg in (3, 24):
        got = solve(kernel, x, y, la, lb, dtype, 0.0, k, options=(("segments", seg), ("chunk", 256)))
        assert not got[4] and got[2] == k
        ref = check_against_restatement(f"{kernel} {np.dtype(npdt).name} segments={seg}", kernel, x, y, la, lb, got, npdt, TOL,
                                        ("big",), one_step=False)
        runs[seg] = got
    lim = bound(k, TOL, ref.P)
    assert sup(runs[3][0], runs[24][0]) <= lim and sup(runs[3][1], runs[24][1]) <= lim


# ---- large logits, and the not-converged path -------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,npdt,TOL", DTYPES, ids=DTYPE_IDS)
def test_large_logits_and_maxit(dtype, npdt, TOL):
    """Sources translated by (3, 0, 0), Gaussian, eps = 1e-3: logits of order -1e4, exp() of none of them representable.
    maxit = 50 with tol = 0: KMVP_E_NOT_CONVERGED with everything written, finite, and within the bound at k = 50."""
    eps = 1e-3
    x, y, la, lb = sr.table_case("gaussian", eps)
    y = y + np.array([3.0, 0.0, 0.0]) / np.sqrt(eps)
    x, y = rounded(x, npdt), rounded(y, npdt)
    got = solve("gaussian", x, y, la, lb, dtype, 0.0, 50)
    u, v, iters, err, converged = got
    assert not converged and iters == 50  # (solve() raises on every status but OK and NOT_CONVERGED)
    assert np.isfinite(u).all() and np.isfinite(v).all() and np.isfinite(err) and err > 0
    ref = check_against_restatement(f"gaussian eps={eps} shifted {np.dtype(npdt).name}", "gaussian", x, y, la, lb, got, npdt, TOL,
                                    ("far", npdt))
    assert ref.P > 3000


# ---- zero-mass points --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,npdt,TOL", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_zero_mass_points(kernel, dtype, npdt, TOL):
    x, y, la, lb = random_case(80, 97, 140, 3)
    x, y = rounded(x, npdt), rounded(y, npdt)
    dead_a, dead_b = [0, 64, 96], [7, 8, 139]
    a, b = np.exp(la), np.exp(lb)
    a[dead_a] = 0.0
    b[dead_b] = 0.0
    with np.errstate(divide="ignore"):
        la, lb = np.log(a / a.sum()), np.log(b / b.sum())
    tol = 1e-8 if dtype == _lib.KMVP_F64 else 1e-4
    got = solve(kernel, x, y, la, lb, dtype, tol, 1000)
    assert got[4] and np.isfinite(got[0][dead_a]).all() and np.isfinite(got[1][dead_b]).all()
    check_against_restatement(f"{kernel} {np.dtype(npdt).name} three points of mass 0 on each side", kernel, x, y, la, lb, got,
                              npdt, TOL, (kernel, "dead", npdt))


# ---- non-finite potentials ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,npdt,TOL", DTYPES, ids=DTYPE_IDS)
def test_a_non_finite_potential_stops_the_solve(dtype, npdt, TOL):
    """A NaN coordinate, and a side without any mass (no row has a live term): KMVP_E_NOT_CONVERGED after the first
    iteration with the outputs written and a message; the context then solves the clean problem as if nothing had been."""
    kernel, eps = sr.TABLE[0]
    x, y, la, lb = sr.table_case(kernel, eps)
    clean = solve(kernel, x, y, la, lb, dtype, 1e-4, 1000)
    x_nan = x.copy()
    x_nan[5, 1] = np.nan
    ctx = _lib.Context(0)
    try:
        ctx.set_points(np.ascontiguousarray(y, dtype=npdt), np.ascontiguousarray(x_nan, dtype=npdt), dtype)
        u, v, iters, err, converged = ctx.sinkhorn(kernel, la, lb, 1e-4, 1000)
        # (x_5 is a target of T1: its potential is NaN in the first iteration, whatever its record did to v in T2)
        assert not converged and iters == 1 and v.shape == lb.shape and np.array_equal(u, np.zeros(len(la)))
        assert "not finite" in ctx._lib.kmvp_last_error(ctx._ctx).decode()
        ctx.set_points(np.ascontiguousarray(y, dtype=npdt), np.ascontiguousarray(x, dtype=npdt), dtype)
        u, v, iters, err, converged = ctx.sinkhorn(kernel, la, np.full(len(lb), -np.inf), 1e-4, 1000)
        assert not converged and iters == 1 and np.isfinite(v).all() and np.array_equal(u, np.zeros(len(la)))
        assert "not finite" in ctx._lib.kmvp_last_error(ctx._ctx).decode()
        again = ctx.sinkhorn(kernel, la, lb, 1e-4, 1000)
    finally:
        ctx.close()
    for p, q in zip(clean, again):
        assert np.array_equal(p, q)


# ---- warm start, reproducibility ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,npdt,TOL", DTYPES, ids=DTYPE_IDS)
def test_warm_start_and_bitwise_reproducibility(dtype, npdt, TOL):
    """Two solves return the same bits; a converged u passed back in stops at iters = 1 with the same plan (u is returned
    uncommitted, so v = T2(u) and err are recomputed from the same inputs in the same order)."""
    tol = 1e-8 if dtype == _lib.KMVP_F64 else 1e-4
    for kernel, eps in (sr.TABLE[0], sr.TABLE[3]):
        x, y, la, lb = sr.table_case(kernel, eps)
        first = solve(kernel, x, y, la, lb, dtype, tol, 1000)
        second = solve(kernel, x, y, la, lb, dtype, tol, 1000)
        assert first[4] and first[2] > 5
        for p, q in zip(first, second):
            assert np.array_equal(p, q), (kernel, "two contexts")
        ctx = _lib.Context(0)
        try:
            ctx.set_points(np.ascontiguousarray(y, dtype=npdt), np.ascontiguousarray(x, dtype=npdt), dtype)
            on_one = [solve(kernel, x, y, la, lb, dtype, tol, 1000, ctx=ctx) for _ in range(2)]
            warm = solve(kernel, x, y, la, lb, dtype, tol, 1000, u0=first[0], ctx=ctx)
        finally:
            ctx.close()
        for run in on_one:
            for p, q in zip(first, run):
                assert np.array_equal(p, q), (kernel, "one context")
        assert warm[4] and warm[2] == 1
        assert np.array_equal(warm[0], first[0]) and np.array_equal(warm[1], first[1]) and warm[3] == first[3], kernel


# ---- the context stays usable ------------------------------------------------------------------------------------------
def test_products_and_reductions_around_a_solve_are_untouched():
    """A product, a log-sum-exp and its gradient before and after a solve on ONE context: each matches its own reference at
    TOL64 and is bitwise what it was; the solve is bitwise what it is on a context of its own."""
    rs = np.random.RandomState(90)
    y, x, c = rs.rand(257, 3) * 2.0, rs.rand(193, 3) * 2.0, rs.randn(257, 1)
    a, b = rs.rand(193) + 0.1, rs.rand(257) + 0.1
    la, lb = np.log(a / a.sum()), np.log(b / b.sum())
    for kernel in KERNELS:
        want = {"product": kmvp_oracle.product(kernel=kernel, source_points=y, target_points=x, source_signal=c),
                "lse": lse_reference.logsumexp(kernel=kernel, source_points=y, target_points=x, source_signal=c),
                "lsegrad": lse_grad_reference.gradient(kernel=kernel, source_points=y, target_points=x, source_signal=c)}
        alone = solve(kernel, x, y, la, lb, _lib.KMVP_F64, 1e-8, 1000, options=(("fast_sqdists", 0),))
        ctx = _lib.Context(0)
        try:
            ctx.set_option("fast_sqdists", 0)
            ctx.set_points(y, x, _lib.KMVP_F64)
            ctx.set_signal(c)

            def three():
                got = {}
                ctx.run(kernel, False)
                got["product"] = ctx.get_result(193, 1)
                ctx.run_lse(kernel)
                got["lse"] = ctx.get_result(193, 1)
                ctx.run_lse_grad(kernel)
                got["lsegrad"] = ctx.get_result(193, 3).reshape(193, 1, 3)
                return got

            before = three()
            inside = solve(kernel, x, y, la, lb, _lib.KMVP_F64, 1e-8, 1000, ctx=ctx)
            after = three()
            again = solve(kernel, x, y, la, lb, _lib.KMVP_F64, 1e-8, 1000, ctx=ctx)
        finally:
            ctx.close()
        for got in (before, after):
            assert rel_err(got["product"], want["product"]) <= TOL64, kernel
            assert measure(got["lse"], want["lse"]) <= TOL64, kernel
            gerr = np.max(np.abs(got["lsegrad"] - want["lsegrad"]), axis=-1) / np.maximum(1.0, np.max(np.abs(want["lsegrad"]), axis=-1))
            assert float(np.max(gerr)) <= TOL64, kernel
        for what in before:
            assert np.array_equal(before[what], after[what]), (kernel, what)
        for p, q, r in zip(alone, inside, again):
            assert np.array_equal(p, q) and np.array_equal(p, r), kernel


# ---- the plugin --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,TOL", ((np.float64, TOL64), (np.float32, TOL32)), ids=DTYPE_IDS)
def test_plugin_potentials_dual_value_and_barycentric_map(precision, TOL):
    """MI355XSinkhorn on unscaled points: (f, g) = eps (u, v) of the C layer on the scaled points; dual_value() against the
    restatement (|difference| <= eps (sum a + sum b) x the potentials' bound); barycentric_map() against sum_j pi_ij y_j /
    sum_j pi_ij in numpy from the returned potentials, measured on G = -2 (x' - ybar') at the log-sum-exp gradient's tolerance;
    a warm start from the converged f stops at once."""
    kernel, eps = "gaussian", 0.05
    rs = np.random.RandomState(95)
    xp, yp = rs.rand(193, 3), rs.rand(257, 3) + np.array([0.25, 0.0, 0.0])
    a, b = rs.rand(193) + 0.1, rs.rand(257) + 0.1
    a, b = a / a.sum(), b / b.sum()
    tol = 1e-8 if precision == np.float64 else 1e-4
    algo = MI355XSinkhorn(kernel=kernel, dimension=3, eps=eps, precision=precision, tol=tol, maxit=1000)
    try:
        with pytest.raises(ValueError, match="total masses differ"):
            algo.prepare_data(source_points=yp, target_points=xp, source_weights=b, target_weights=a * 1.01)
        algo.prepare_data(source_points=yp, target_points=xp, source_weights=b, target_weights=a)
        algo.fit()
        algo.query()
        f, g = algo.get_potentials()
        extra = algo.get_additional()
        dual = algo.dual_value()
        T = algo.barycentric_map()
        iters = extra["iterations"]
        algo.query(warm_start=f)
        warm = algo.get_additional()
        f2, g2 = algo.get_potentials()
    finally:
        algo.done()
    assert extra["converged"] and extra["marginal_error"] <= tol and extra["device_kernel"] == "lowd_lse_kernel", extra
    assert extra["device_total_ms"] > 0 and f.shape == (193,) and g.shape == (257,) and T.shape == (193, 3)
    xs, ys = rounded(xp * algo.scale, precision), rounded(yp * algo.scale, precision)
    la, lb = np.log(a), np.log(b)
    ref = reference(("plugin", precision, iters), kernel=kernel, x=xs, y=ys, log_a=la, log_b=lb, tol=0.0, maxit=iters)
    lim = bound(iters, TOL, ref.P)
    du, dv = sup(f / eps, ref.u), sup(g / eps, ref.v)
    print(f"plugin {np.dtype(precision).name}: k = {iters}, |u - u_ref| {du:.3e}, |v - v_ref| {dv:.3e} (bound {lim:.3e})")
    assert du <= lim and dv <= lim
    dual_ref = eps * (np.dot(a, ref.u) + np.dot(b, ref.v))
    print(f"dual value {dual:.12g} (restatement {dual_ref:.12g}, allowed difference {2 * eps * lim:.3e})")
    assert abs(dual - dual_ref) <= eps * (a.sum() + b.sum()) * lim
    # the barycentric map of the RETURNED potentials
    c = (g / eps + lb).reshape(-1, 1)
    if precision == np.float32:
        c = rounded(c, np.float32)  # what the record's signal slot holds
    pi = sr.plan(kernel, xs, ys, la, np.zeros(257), f / eps, c[:, 0])
    T_np = (pi @ ys) / pi.sum(axis=1, keepdims=True) / algo.scale
    G, G_np = -2.0 * (xs - T * algo.scale), -2.0 * (xs - T_np * algo.scale)
    tol_g = TOL64
    if precision == np.float32:
        own = lse_grad_reference.gradient(kernel=kernel, source_points=ys, target_points=xs, source_signal=c, precision=np.float32)
        own_err = float(np.max(np.max(np.abs(own[:, 0, :] - G_np), axis=-1) / np.maximum(1.0, np.max(np.abs(G_np), axis=-1))))
        tol_g = max(TOL32, 2 * own_err)
    gerr = float(np.max(np.max(np.abs(G - G_np), axis=-1) / np.maximum(1.0, np.max(np.abs(G_np), axis=-1))))
    print(f"barycentric map: err {gerr:.3e} on G (tolerance {tol_g:.1e}), displacement up to {np.max(np.abs(T_np - xp)):.3f}")
    assert gerr <= tol_g
    assert warm["converged"] and warm["iterations"] == 1
    assert sup(f2, f) <= 1e-12 * max(1.0, np.abs(f).max()) and sup(g2, g) <= 1e-9 * max(1.0, np.abs(g).max())


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_c_abi_refusals():
    """bf16 context, D = 9, fast_sqdists = 1, a communicator of one rank, a source slice: KMVP_E_UNSUPPORTED with a message
    that names the cause; call-order and argument errors: KMVP_E_INVALID."""
    rs = np.random.RandomState(99)

    def refused(y, dtype, options=(), comm=False, M_total=None):
        ctx = _lib.Context(0)
        try:
            if comm:
                ctx.comm_init(_lib.comm_unique_id(), 0, 1)
            for key, value in options:
                ctx.set_option(key, value)
            npdt = np.float64 if dtype == _lib.KMVP_F64 else np.float32
            x = np.ascontiguousarray(rs.rand(40, y.shape[1]), dtype=npdt)
            ctx.set_points(np.ascontiguousarray(y, dtype=npdt), x, dtype, M_total=M_total)
            msg = ""
            for kernel in KERNELS:
                with pytest.raises(_lib.KmvpError) as e:
                    ctx.sinkhorn(kernel, None, None, 1e-6, 10)
                assert e.value.code == 2, (kernel, str(e.value))
                msg = ctx._lib.kmvp_last_error(ctx._ctx).decode()
                assert msg
        finally:
            ctx.close()
        return msg

    assert "bfloat16" in refused(rs.rand(64, 16), _lib.KMVP_BF16)
    assert "D = 9" in refused(rs.rand(64, 9), _lib.KMVP_F32)
    assert "fast_sqdists = 1" in refused(rs.rand(64, 3), _lib.KMVP_F32, options=(("fast_sqdists", 1),))
    assert "communicator" in refused(rs.rand(64, 3), _lib.KMVP_F64, comm=True)
    assert "slice" in refused(rs.rand(64, 3), _lib.KMVP_F64, M_total=100)
    ctx = _lib.Context(0)
    try:
        with pytest.raises(_lib.KmvpError) as e:  # no points
            ctx.sinkhorn("gaussian", None, None, 1e-6, 10)
        assert e.value.code == 1
        pts = np.ascontiguousarray(rs.rand(64, 3))
        ctx.set_points(pts, None, _lib.KMVP_F64)
        for tol, maxit in ((-1.0, 10), (float("nan"), 10), (1e-6, 0)):
            with pytest.raises(_lib.KmvpError) as e:
                ctx.sinkhorn("gaussian", None, None, tol, maxit)
            assert e.value.code == 1, (tol, maxit)
        u = np.zeros(64)
        rc = ctx._lib.kmvp_gaussian_sinkhorn(ctx._ctx, None, None, 1e-6, 10, u.ctypes.data, None, None, None)  # NULL outputs
        assert rc == 1 and ctx._lib.kmvp_last_error(ctx._ctx)
        with pytest.raises(NotImplementedError):  # the other kernels have no entry point
            ctx.sinkhorn("inverse-distance", None, None, 1e-6, 10)
        # uniform weights by default, and no signal was ever set
        got = ctx.sinkhorn("gaussian", None, None, 1e-8, 1000)
        assert got[4]
        ref = sr.sinkhorn(kernel="gaussian", x=pts, y=pts, tol=0.0, maxit=got[2])
        assert sup(got[0], ref.u) <= bound(got[2], TOL64, ref.P) and sup(got[1], ref.v) <= bound(got[2], TOL64, ref.P)
    finally:
        ctx.close()

