"""GPU tests of the batched Sinkhorn solve (kmvp_sinkhorn_batched.hip, lowd_batch_lse_kernel; include/kmvp.h
kmvp_<kernel>_sinkhorn_batched, MI355XSinkhorn with batches) against the float64 numpy restatement
(sinkhorn_batched_reference.py: sinkhorn_reference per batch with a per-batch stop, itself checked against the textbook
scaling-domain iteration in test_sinkhorn_batched_reference.py).

The measure and the bound are test_gpu_sinkhorn.py's, per batch: the pair arithmetic is lowd_lse_kernel's, held to
TOL64 = 1e-11 / TOL32 = 1e-5 on |L - L_ref| / max(1, |L_ref|), and T1, T2 are non-expansive in the sup norm, so after k
iterations of potentials no larger than P

    max |u - u_ref|, max |v - v_ref|  <=  2 k TOL max(1, P)

with u_ref, v_ref and P of that batch from the restatement run for exactly the device's iters[b] (tol = 0); for float32 the
restatement runs on the float32-rounded points.  The tolerances pair with the precisions as in test_gpu_sinkhorn.py:
1e-8 for float64, 1e-4 for float32 (float32 potentials cannot meet 1e-8).  Independence, retirement and isolation are
bitwise: no tolerance at all.
"""
import numpy as np
import pytest

import lse_reference
import sinkhorn_batched_reference as sbr
import sinkhorn_reference as sr
from kernel_matrix_benchmarks_amd import _lib
from kernel_matrix_benchmarks_amd.algorithms.mi355x import MI355XSinkhorn

pytestmark = pytest.mark.gpu

TOL64 = 1e-11
TOL32 = 1e-5
KERNELS = lse_reference.KERNELS
DTYPES = ((_lib.KMVP_F64, np.float64, TOL64, 1e-8), (_lib.KMVP_F32, np.float32, TOL32, 1e-4))
DTYPE_IDS = ("float64", "float32")
OK, INVALID, UNSUPPORTED, NOT_CONVERGED = 0, 1, 2, 6


def rounded(a, npdt):
    return np.asarray(a, dtype=npdt).astype(np.float64)


def measure(got, want):
    assert got.shape == want.shape and np.isfinite(got).all() and np.isfinite(want).all(), (got.shape, want.shape)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))


def sup(got, want):
    assert got.shape == want.shape and np.isfinite(got).all(), got.shape
    return float(np.max(np.abs(got - want))) if got.size else 0.0


def bound(k, tol, P):
    return 2 * k * tol * max(1.0, P)


def npdt_of(dtype):
    return np.float64 if dtype == _lib.KMVP_F64 else np.float32


def open_context(x, y, x_off, y_off, dtype, options=()):
    """A context on the (already scaled) concatenated clouds with the batches set; x is None: same points, and the
    sources' offsets serve both."""
    npdt = npdt_of(dtype)
    ctx = _lib.Context(0)
    try:
        for key, value in options:
            ctx.set_option(key, value)
        ctx.set_points(np.ascontiguousarray(y, dtype=npdt), None if x is None else np.ascontiguousarray(x, dtype=npdt), dtype)
        ctx.set_batches(y_off, None if x is None else x_off)
    except Exception:
        ctx.close()
        raise
    return ctx


def solve(kernel, x, y, x_off, y_off, la, lb, dtype, tol, maxit, u0=None, options=(), ctx=None):
    """Through the C ABI's typed wrapper: (u, v, iters, err, status)."""
    own = ctx is None
    if own:
        ctx = open_context(x, y, x_off, y_off, dtype, options)
    try:
        u, v, iters, err, status = ctx.sinkhorn_batched(kernel, la, lb, tol, maxit, u0)
        B = len(y_off) - 1
        assert ctx.last_kernel_name == "lowd_batch_lse_kernel" and ctx.last_dispatch_note == ""
        assert ctx.last_total_ms > 0 and ctx.last_kernel_ms == ctx.last_total_ms
        assert u.dtype == np.float64 and v.dtype == np.float64 and iters.shape == err.shape == status.shape == (B,)
        assert np.all((0 <= iters) & (iters <= maxit)) and np.all((1 <= status) & (status <= 3))
        return u, v, iters, err, status
    finally:
        if own:
            ctx.close()


def batch_of(got, x_off, y_off, b):
    """(u, v, iters, err, status) of batch b."""
    return (got[0][x_off[b]:x_off[b + 1]], got[1][y_off[b]:y_off[b + 1]], got[2][b], got[3][b], got[4][b])


def same_bits(p, q):
    return all(np.array_equal(np.asarray(s), np.asarray(t), equal_nan=True) for s, t in zip(p, q))


def pick(case, order):
    """The batches `order` of a case (x, y, x_off, y_off, la, lb), concatenated in that order."""
    x, y, x_off, y_off, la, lb = case
    xs = [slice(x_off[b], x_off[b + 1]) for b in order]
    ys = [slice(y_off[b], y_off[b + 1]) for b in order]
    return (np.concatenate([x[s] for s in xs]), np.concatenate([y[s] for s in ys]),
            sbr.offsets([s.stop - s.start for s in xs]), sbr.offsets([s.stop - s.start for s in ys]),
            np.concatenate([la[s] for s in xs]), np.concatenate([lb[s] for s in ys]))


def append(case, extra):
    """Two cases one behind the other."""
    return tuple(np.concatenate([p, q]) if k not in (2, 3) else np.concatenate([p, p[-1] + q[1:]])
                 for k, (p, q) in enumerate(zip(case, extra)))


_CACHE = {}


def cached(key, make):
    """One run per distinct case -- restatement or device --, shared by the tests that need it and never modified."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def ragged(kernel, npdt):
    x, y, x_off, y_off, la, lb = sbr.ragged_case(kernel)
    return rounded(x, npdt), rounded(y, npdt), x_off, y_off, la, lb


def ragged_solve(kernel, dtype, tol):
    """The ragged case at the precision's tolerance, maxit = 1000: the run the independence tests compare against."""
    case = ragged(kernel, npdt_of(dtype))
    return cached(("gpu", kernel, dtype, tol), lambda: solve(kernel, *case, dtype, tol, 1000))


def check_against_restatement(label, kernel, case, got, TOL, key):
    """Per batch, the accumulation bound at the device's own iteration count; returns the exact-k restatement."""
    x, y, x_off, y_off, la, lb = case
    iters = got[2]
    ref = cached(key + tuple(iters), lambda: sbr.sinkhorn(kernel=kernel, x=x, y=y, x_off=x_off, y_off=y_off, log_a=la, log_b=lb,
                                                           tol=0.0, maxit=np.maximum(iters, 1)))
    for b in range(len(iters)):
        if x_off[b + 1] == x_off[b]:
            continue
        assert ref.iters[b] == iters[b], (label, b, ref.iters[b], iters[b])
        lim = bound(int(iters[b]), TOL, ref.P[b])
        gu, gv = batch_of(got, x_off, y_off, b)[:2]
        ru, rv = batch_of(ref, x_off, y_off, b)[:2]
        du, dv = sup(gu, ru), sup(gv, rv)
        print(f"{label} batch {b}: k = {iters[b]}, P = {ref.P[b]:.4g}, |u - u_ref| {du:.3e}, |v - v_ref| {dv:.3e} "
              f"(bound {lim:.3e}); err {got[3][b]:.3e} (restatement {ref.err[b]:.3e})")
        assert du <= lim and dv <= lim, (label, b, du, dv, lim)
    return ref


# ---- agreement with the restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,npdt,TOL,tol", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_ragged_batches_agree_with_the_restatement(kernel, dtype, npdt, TOL, tol):
    """B = 5 ragged batches, targets of 1, 63, 64, 65, 130 points against sources of 9, 1, 8, 200, 7; the clouds' spreads
    grow with b, so the restatement alone stops the batches at two or more distinct k (asserted of the restatement here,
    verified without a GPU in test_sinkhorn_batched_reference.py)."""
    case = ragged(kernel, npdt)
    x, y, x_off, y_off, la, lb = case
    ref_tol = cached(("tol", kernel, npdt, tol), lambda: sbr.sinkhorn(kernel=kernel, x=x, y=y, x_off=x_off, y_off=y_off, log_a=la,
                                                                       log_b=lb, tol=tol, maxit=1000))
    assert np.all(ref_tol.status == sbr.CONVERGED) and len(set(ref_tol.iters)) >= 2, ref_tol.iters
    got = ragged_solve(kernel, dtype, tol)
    label = f"{kernel} {np.dtype(npdt).name} tol={tol:g}"
    print(f"{label}: iterations {list(got[2])} (restatement {list(ref_tol.iters)})")
    assert np.all(got[4] == sbr.CONVERGED) and np.all(got[3] <= tol), (label, got[2], got[3], got[4])
    assert np.all(np.abs(got[2] - ref_tol.iters) <= 1), (label, got[2], ref_tol.iters)
    check_against_restatement(label, kernel, case, got, TOL, ("exact", kernel, npdt))


# ---- one half-step: the kernel held directly ---------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,npdt,TOL,tol", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_one_half_step_at_the_log_sum_exp_tolerance(kernel, dtype, npdt, TOL, tol):
    """maxit = 1, tol = 0 from a random u_0: the returned v against sinkhorn_reference.half_step of u_0 per batch, at the
    log-sum-exp's own tolerance (float32: test_gpu_sinkhorn.one_step_tolerance's rule, twice the float32 restatement's own
    distance where that is larger) -- no accumulation.  With the default chunk and with chunk = 16, at which the 200-source
    batch folds its float32 sum 13 times."""
    case = ragged(kernel, npdt)
    x, y, x_off, y_off, la, lb = case
    u0 = np.random.RandomState(5).randn(len(la))
    for chunk in (512, 16):
        u, v, iters, err, status = solve(kernel, *case, dtype, 0.0, 1, u0=u0, options=(("chunk", chunk),))
        assert np.array_equal(u, u0) and np.all(iters == 1) and np.all(status == sbr.MAXIT) and np.all(err > 0)
        for b in range(len(iters)):
            xs, ys = slice(x_off[b], x_off[b + 1]), slice(y_off[b], y_off[b + 1])
            want, _ = sr.half_step(kernel, y[ys], x[xs], u0[xs], la[xs])
            step_tol = TOL
            if npdt == np.float32:
                own, _ = sr.half_step(kernel, y[ys], x[xs], u0[xs], la[xs], precision=np.float32)
                step_tol = max(TOL32, 2 * measure(own, want))
            step = measure(v[ys], want)
            print(f"{kernel} {np.dtype(npdt).name} chunk={chunk} batch {b}: v against T2(u_0) {step:.3e} (tolerance {step_tol:.1e})")
            assert step <= step_tol, (kernel, chunk, b, step, step_tol)


# ---- independence: bit for bit -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,npdt,TOL,tol", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_a_batch_is_its_own_solve_wherever_it_stands(kernel, dtype, npdt, TOL, tol):
    """Every batch of the ragged solve is bit for bit its B = 1 solve, the same with the clouds in permuted order, and the
    same in a second run."""
    case = ragged(kernel, npdt)
    x_off, y_off = case[2], case[3]
    base = ragged_solve(kernel, dtype, tol)
    again = solve(kernel, *case, dtype, tol, 1000)
    assert same_bits(base, again), "two runs"
    for b in range(5):
        one = pick(case, [b])
        alone = solve(kernel, *one, dtype, tol, 1000)
        assert same_bits(batch_of(alone, one[2], one[3], 0), batch_of(base, x_off, y_off, b)), (kernel, "B = 1", b)
    order = [3, 0, 4, 2, 1]
    perm = pick(case, order)
    moved = solve(kernel, *perm, dtype, tol, 1000)
    for q, b in enumerate(order):
        assert same_bits(batch_of(moved, perm[2], perm[3], q), batch_of(base, x_off, y_off, b)), (kernel, "permuted", b)


def companions(kernel, npdt):
    """Two more batches: one with a NaN target coordinate, and one whose clouds are so wide that it is still running when
    the ragged batches have long converged."""
    rs = np.random.RandomState(21)
    spread = 8.0 if kernel == "gaussian" else 40.0
    xn, yn = rs.rand(70, 3), rs.rand(9, 3)
    xn[3, 1] = np.nan
    xw, yw = rs.rand(70, 3) * spread, (rs.rand(50, 3) + 0.25) * spread
    x_off, y_off = sbr.offsets([70, 70]), sbr.offsets([9, 50])
    la = np.concatenate([np.full(70, -np.log(70.0))] * 2)
    lb = np.concatenate([np.full(9, -np.log(9.0)), np.full(50, -np.log(50.0))])
    return rounded(np.concatenate([xn, xw]), npdt), rounded(np.concatenate([yn, yw]), npdt), x_off, y_off, la, lb


@pytest.mark.parametrize("dtype,npdt,TOL,tol", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_a_batch_does_not_see_what_the_others_hold_or_when_they_stop(kernel, dtype, npdt, TOL, tol):
    """Next to a batch that turns non-finite in its first iteration and one that runs to maxit (three iterations beyond the
    slowest ragged batch), every ragged batch is bit for bit what it is without them -- with "sinkhorn_retire" 1 and 0, which
    also agree bit for bit on the two companions.  The call returns KMVP_E_NOT_CONVERGED with everything written."""
    case = ragged(kernel, npdt)
    x_off, y_off = case[2], case[3]
    base = ragged_solve(kernel, dtype, tol)
    both = append(case, companions(kernel, npdt))
    maxit = int(base[2].max()) + 3
    runs = {}
    for retire in (1, 0):
        ctx = open_context(*both[:4], dtype, options=(("sinkhorn_retire", retire),))
        try:
            runs[retire] = solve(kernel, *both, dtype, tol, maxit, ctx=ctx)
            rc = raw_return_code(ctx, kernel, both, tol, maxit)
        finally:
            ctx.close()
        assert rc == NOT_CONVERGED
        got = runs[retire]
        assert list(got[4]) == [1, 1, 1, 1, 1, sbr.NONFINITE, sbr.MAXIT], (retire, got[4])
        assert got[2][5] == 1 and got[2][6] == maxit and np.isfinite(got[3][6]) and got[3][6] > tol
        assert np.array_equal(got[0][both[2][5]:both[2][6]], np.zeros(70))   # the non-finite batch keeps u_0, uncommitted
        for b in range(5):
            assert same_bits(batch_of(got, both[2], both[3], b), batch_of(base, x_off, y_off, b)), (kernel, retire, b)
    assert same_bits(runs[0], runs[1]), "sinkhorn_retire 0 against 1"
    # and without an option set the default is retirement on: the same bits once more
    assert same_bits(solve(kernel, *both, dtype, tol, maxit), runs[1])


def raw_return_code(ctx, kernel, case, tol, maxit):
    """The C entry's own return value (the typed wrapper folds OK and NOT_CONVERGED into the status array)."""
    x, y, x_off, y_off, la, lb = case
    B = len(y_off) - 1
    entry = ctx._lib.kmvp_gaussian_sinkhorn_batched if kernel == "gaussian" else ctx._lib.kmvp_absexp_sinkhorn_batched
    la, lb = np.ascontiguousarray(la, dtype=np.float64), np.ascontiguousarray(lb, dtype=np.float64)
    u, v = np.zeros(len(la)), np.zeros(len(lb))
    iters, err, status = np.zeros(B, dtype=np.int32), np.zeros(B), np.zeros(B, dtype=np.int32)
    return entry(ctx._ctx, la.ctypes.data, lb.ctypes.data, float(tol), int(maxit), u.ctypes.data, v.ctypes.data, iters.ctypes.data,
                 err.ctypes.data, status.ctypes.data)


# ---- conventions -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,npdt,TOL,tol", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_zero_mass_points_maxit_and_warm_start(kernel, dtype, npdt, TOL, tol):
    """Points of mass 0 (log-weight -inf) on both sides of three batches: finite potentials, within the bound of the
    restatement.  maxit = 4 with tol = 0 on the three larger batches (the two smallest reach their fixed point, err == 0
    exactly, within a few iterations): status 3 in every batch with (u_3, v_4), within the bound at k = 4.  A warm start
    from a returned u stops at k = 1 in every batch with the same plan."""
    x, y, x_off, y_off, la, lb = ragged(kernel, npdt)
    a, b = np.exp(la), np.exp(lb)
    dead_a, dead_b = [x_off[2], x_off[3] + 64, x_off[4] + 129], [y_off[2] + 7, y_off[3], y_off[3] + 199]
    a[dead_a] = 0.0
    b[dead_b] = 0.0
    for k in range(5):   # renormalised per batch
        a[x_off[k]:x_off[k + 1]] /= a[x_off[k]:x_off[k + 1]].sum()
        b[y_off[k]:y_off[k + 1]] /= b[y_off[k]:y_off[k + 1]].sum()
    with np.errstate(divide="ignore"):
        la, lb = np.log(a), np.log(b)
    case = (x, y, x_off, y_off, la, lb)
    ctx = open_context(x, y, x_off, y_off, dtype)
    try:
        got = solve(kernel, *case, dtype, tol, 1000, ctx=ctx)
        warm = solve(kernel, *case, dtype, tol, 1000, u0=got[0], ctx=ctx)
    finally:
        ctx.close()
    larger = pick(case, [2, 3, 4])
    short = solve(kernel, *larger, dtype, 0.0, 4)
    label = f"{kernel} {np.dtype(npdt).name}"
    assert np.all(got[4] == sbr.CONVERGED) and np.isfinite(got[0][dead_a]).all() and np.isfinite(got[1][dead_b]).all()
    check_against_restatement(label + " points of mass 0", kernel, case, got, TOL, ("dead", kernel, npdt))
    assert np.all(short[4] == sbr.MAXIT) and np.all(short[2] == 4) and np.all(short[3] > 0)
    check_against_restatement(label + " maxit = 4", kernel, larger, short, TOL, ("dead, larger", kernel, npdt))
    assert np.all(warm[4] == sbr.CONVERGED) and np.all(warm[2] == 1)
    assert np.array_equal(warm[0], got[0]) and np.array_equal(warm[1], got[1]) and np.array_equal(warm[3], got[3])


@pytest.mark.parametrize("dtype,npdt,TOL,tol", DTYPES, ids=DTYPE_IDS)
def test_empty_batches_and_same_points(dtype, npdt, TOL, tol):
    """Batches that are empty on both sides at the start, in the middle and at the end: iters 0, err 0, status 1, and the
    others bit for bit what they are without them.  A batch with points on one side only: KMVP_E_INVALID, the message
    names it.  Same points with NULL target offsets: bit for bit the solve with the cloud passed twice."""
    kernel = "gaussian"
    case = ragged(kernel, npdt)
    x_off, y_off = case[2], case[3]
    base = ragged_solve(kernel, dtype, tol)
    x, y, _, _, la, lb = case
    holes = [None, 0, 1, None, None, 2, 3, 4, None]   # None: an empty batch
    xo = sbr.offsets([0 if b is None else x_off[b + 1] - x_off[b] for b in holes])
    yo = sbr.offsets([0 if b is None else y_off[b + 1] - y_off[b] for b in holes])
    got = solve(kernel, x, y, xo, yo, la, lb, dtype, tol, 1000)
    for q, b in enumerate(holes):
        if b is None:
            assert (got[2][q], got[3][q], got[4][q]) == (0, 0.0, 1), q
        else:
            assert same_bits(batch_of(got, xo, yo, q), batch_of(base, x_off, y_off, b)), (q, b)
    # all batches empty: nothing to launch
    nothing = solve(kernel, x[:0], y[:0], sbr.offsets([0, 0]), sbr.offsets([0, 0]), la[:0], lb[:0], dtype, tol, 10)
    assert list(nothing[2]) == [0, 0] and list(nothing[4]) == [1, 1]
    # one-sided
    yo_bad = yo.copy()
    yo_bad[3] = yo_bad[2]   # batch 2 (63 targets) loses its single source to batch 3, which has no target
    ctx = open_context(x, y, xo, yo_bad, dtype)
    try:
        with pytest.raises(_lib.KmvpError) as e:
            ctx.sinkhorn_batched(kernel, la, lb, tol, 10)
        assert e.value.code == INVALID and "batch 2 has points on one side only" in str(e.value), str(e.value)
    finally:
        ctx.close()
    # same points
    yy = np.concatenate([y, y[::-1] * 0.5])
    off = sbr.offsets([100, len(yy) - 100])
    twice = solve(kernel, yy, yy, off, off, None, None, dtype, tol, 1000)   # NULL weights: uniform within each batch
    shared = solve(kernel, None, yy, None, off, None, None, dtype, tol, 1000)
    assert np.all(twice[4] == 1) and same_bits(twice, shared)
    ref = sbr.sinkhorn(kernel=kernel, x=yy, y=yy, x_off=off, y_off=off, tol=0.0, maxit=twice[2])
    for b in range(2):
        lim = bound(int(twice[2][b]), TOL, ref.P[b])
        assert sup(shared[0][off[b]:off[b + 1]], ref.u[off[b]:off[b + 1]]) <= lim, b
        assert sup(shared[1][off[b]:off[b + 1]], ref.v[off[b]:off[b + 1]]) <= lim, b


# ---- isolation ---------------------------------------------------------------------------------------------------------
def test_the_context_is_untouched_around_a_batched_solve():
    """Batched Gaussian product and kmvp_nearest, and -- batches switched off -- plain product, log-sum-exp and plain Sinkhorn,
    recorded before and after a batched solve on ONE context: bitwise equal.  The plain Sinkhorn and log-sum-exp keep
    answering KMVP_E_UNSUPPORTED while batches are set."""
    kernel = "gaussian"
    case = ragged(kernel, np.float64)
    x, y, x_off, y_off, la, lb = case
    c = np.random.RandomState(31).randn(len(y), 1)
    N = len(x)
    alone = ragged_solve(kernel, _lib.KMVP_F64, 1e-8)
    ctx = _lib.Context(0)
    try:
        ctx.set_option("fast_sqdists", 0)
        ctx.set_points(np.ascontiguousarray(y), np.ascontiguousarray(x), _lib.KMVP_F64)
        ctx.set_signal(c)

        def everything():
            out = {}
            ctx.set_batches(y_off, x_off)
            ctx.run(kernel, False)
            out["batched product"] = ctx.get_result(N, 1)
            out["nearest idx"], out["nearest sq"] = ctx.run_nearest(3)
            for entry in (lambda: ctx.sinkhorn(kernel, la, lb, 1e-8, 50), lambda: ctx.run_lse(kernel)):
                with pytest.raises(_lib.KmvpError) as e:
                    entry()
                assert e.value.code == UNSUPPORTED and "kmvp_set_batches" in str(e.value)
            ctx.set_batches(None)
            ctx.run(kernel, False)
            out["product"] = ctx.get_result(N, 1)
            ctx.run_lse(kernel)
            out["lse"] = ctx.get_result(N, 1)
            plain = ctx.sinkhorn(kernel, None, None, 1e-6, 200)
            out["sinkhorn u"], out["sinkhorn v"], out["sinkhorn k"], out["sinkhorn err"] = plain[:4]
            ctx.set_batches(y_off, x_off)
            return out

        before = everything()
        inside = solve(kernel, *case, _lib.KMVP_F64, 1e-8, 1000, ctx=ctx)
        after = everything()
        again = solve(kernel, *case, _lib.KMVP_F64, 1e-8, 1000, ctx=ctx)
    finally:
        ctx.close()
    for what in before:
        assert np.array_equal(np.asarray(before[what]), np.asarray(after[what]), equal_nan=True), what
    assert same_bits(alone, inside) and same_bits(alone, again)


# ---- refusals, diagnostics -----------------------------------------------------------------------------------------------
def test_c_abi_refusals():
    """bf16 context, D = 9, fast_sqdists = 1, a communicator of one rank, a source slice: KMVP_E_UNSUPPORTED with a message
    that names the cause and the batches; batches not set, tol < 0 or NaN, maxit < 1, a NULL output: KMVP_E_INVALID."""
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
            ctx.set_batches([0, 30, 64], [0, 10, 40])
            msg = ""
            for kernel in KERNELS:
                with pytest.raises(_lib.KmvpError) as e:
                    ctx.sinkhorn_batched(kernel, None, None, 1e-6, 10)
                assert e.value.code == UNSUPPORTED, (kernel, str(e.value))
                msg = str(e.value)
                assert "kmvp_set_batches" in msg, msg
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
            ctx.sinkhorn_batched("gaussian", None, None, 1e-6, 10)
        assert e.value.code == INVALID
        pts = np.ascontiguousarray(rs.rand(64, 3))
        ctx.set_points(pts, None, _lib.KMVP_F64)
        with pytest.raises(_lib.KmvpError) as e:  # no batches
            ctx.sinkhorn_batched("gaussian", None, None, 1e-6, 10)
        assert e.value.code == INVALID and "batches are not set" in str(e.value) and "kmvp_set_batches" in str(e.value)
        ctx.set_batches([0, 20, 64])
        for tol, maxit in ((-1.0, 10), (float("nan"), 10), (1e-6, 0)):
            with pytest.raises(_lib.KmvpError) as e:
                ctx.sinkhorn_batched("gaussian", None, None, tol, maxit)
            assert e.value.code == INVALID, (tol, maxit)
        u, v = np.zeros(64), np.zeros(64)
        iters, err, status = np.zeros(2, dtype=np.int32), np.zeros(2), np.zeros(2, dtype=np.int32)
        ptrs = [u.ctypes.data, v.ctypes.data, iters.ctypes.data, err.ctypes.data, status.ctypes.data]
        for missing in range(5):   # a NULL u, v, iters, err or status
            args = [None if q == missing else p for q, p in enumerate(ptrs)]
            rc = ctx._lib.kmvp_gaussian_sinkhorn_batched(ctx._ctx, None, None, 1e-6, 10, *args)
            assert rc == INVALID and ctx._lib.kmvp_last_error(ctx._ctx), missing
        with pytest.raises(NotImplementedError):  # the other kernels have no entry point
            ctx.sinkhorn_batched("inverse-distance", None, None, 1e-6, 10)
        with pytest.raises(ValueError):           # a short array never reaches the library
            ctx.sinkhorn_batched("gaussian", np.zeros(63), None, 1e-6, 10)
        with pytest.raises(_lib.KmvpError):
            ctx.set_option("sinkhorn_retire", 2)
        # the accepted and ignored options, and uniform weights by default
        for key, value in (("segments", 7), ("feed", 1), ("targets_per_lane", 2)):
            ctx.set_option(key, value)
        got = ctx.sinkhorn_batched("gaussian", None, None, 1e-8, 1000)
        assert np.all(got[4] == 1) and ctx.last_kernel_name == "lowd_batch_lse_kernel" and ctx.last_dispatch_note == ""
        off = sbr.offsets([20, 44])
        ref = sbr.sinkhorn(kernel="gaussian", x=pts, y=pts, x_off=off, y_off=off, tol=0.0, maxit=got[2])
        for b in range(2):
            lim = bound(int(got[2][b]), TOL64, ref.P[b])
            assert sup(got[0][off[b]:off[b + 1]], ref.u[off[b]:off[b + 1]]) <= lim
            assert sup(got[1][off[b]:off[b + 1]], ref.v[off[b]:off[b + 1]]) <= lim
    finally:
        ctx.close()


# ---- the plugin --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,TOL", ((np.float64, TOL64), (np.float32, TOL32)), ids=DTYPE_IDS)
def test_plugin_with_batches_agrees_with_the_unbatched_plugin_per_cloud(precision, TOL):
    """MI355XSinkhorn with batches against an unbatched MI355XSinkhorn on every cloud, both for exactly k = 5 iterations
    (tol = 0, so that the two cannot stop one iteration apart): each is within 2 k TOL max(1, P) of the restatement, hence
    within twice that of the other -- potentials in units of eps, dual values times the batch's mass (<a> + <b> = 2).  Not
    bitwise: the plain entry folds and merges differently.  barycentric_map() raises with batches; without them the plugin
    returns what it always did (scalars, and the map)."""
    kernel, eps, k = "gaussian", 0.25, 5
    rs = np.random.RandomState(41)
    sizes_x, sizes_y = (65, 20, 130), (9, 63, 200)
    xs = [rs.rand(n, 3) for n in sizes_x]
    ys = [rs.rand(m, 3) + np.array([0.25, 0.0, 0.0]) for m in sizes_y]
    ws_a = [w / w.sum() for w in (rs.rand(n) + 0.1 for n in sizes_x)]
    ws_b = [w / w.sum() for w in (rs.rand(m) + 0.1 for m in sizes_y)]
    x_off, y_off = sbr.offsets(sizes_x), sbr.offsets(sizes_y)
    algo = MI355XSinkhorn(kernel=kernel, dimension=3, eps=eps, precision=precision, tol=0.0, maxit=k)
    try:
        algo.prepare_data(source_points=np.concatenate(ys), target_points=np.concatenate(xs), source_weights=np.concatenate(ws_b),
                          target_weights=np.concatenate(ws_a), source_batches=y_off, target_batches=x_off)
        algo.fit()
        algo.query()
        f, g = algo.get_potentials()
        dual = algo.dual_value()
        extra = algo.get_additional()
        with pytest.raises(NotImplementedError, match="batched"):
            algo.barycentric_map()
    finally:
        algo.done()
    assert f.shape == (sum(sizes_x),) and g.shape == (sum(sizes_y),) and dual.shape == (3,)
    assert extra["device_kernel"] == "lowd_batch_lse_kernel" and list(extra["iterations"]) == [k] * 3
    assert extra["marginal_error"].shape == (3,) and not extra["converged"].any()
    for b in range(3):
        one = MI355XSinkhorn(kernel=kernel, dimension=3, eps=eps, precision=precision, tol=0.0, maxit=k)
        try:
            one.prepare_data(source_points=ys[b], target_points=xs[b], source_weights=ws_b[b], target_weights=ws_a[b])
            one.fit()
            one.query()
            f1, g1 = one.get_potentials()
            dual1 = one.dual_value()
            extra1 = one.get_additional()
            T = one.barycentric_map()
        finally:
            one.done()
        assert extra1["iterations"] == k and extra1["converged"] is False and isinstance(dual1, float) and T.shape == (sizes_x[b], 3)
        assert extra1["device_kernel"] == "lowd_lse_kernel"
        xr, yr = rounded(xs[b] * one.scale, precision), rounded(ys[b] * one.scale, precision)
        ref = sbr.one_batch(kernel, xr, yr, np.log(ws_a[b]), np.log(ws_b[b]), 0.0, k, None)
        lim = 2 * bound(k, TOL, ref[5])
        du, dv = sup(f[x_off[b]:x_off[b + 1]] / eps, f1 / eps), sup(g[y_off[b]:y_off[b + 1]] / eps, g1 / eps)
        print(f"plugin {np.dtype(precision).name} batch {b}: |u - u_plain| {du:.3e}, |v - v_plain| {dv:.3e} (bound {lim:.3e}); "
              f"dual {dual[b]:.12g} against {dual1:.12g}")
        assert du <= lim and dv <= lim, (b, du, dv, lim)
        assert abs(dual[b] - dual1) <= eps * 2.0 * lim
