"""GPU tests of the device-resident Gaussian mean-shift (include/kmvp.h kmvp_gaussian_meanshift: lowd_lse_grad_kernel, the
step and the compaction of csrc/kmvp_meanshift.hip) against the numpy restatement of its definition
(meanshift_reference.py, itself tried on hand-made sequences in test_meanshift_reference.py).

Parity is BITWISE, no tolerance: the restatement is driven by a host loop on a second context that always holds all N
targets -- every sweep set_points(y, real(z)), the same signal, kmvp_gaussian_logsumexp_grad, get_result -- and the solver
must return its modes, iters, step2, sweeps and target_sweeps.  That holds because every target's arithmetic is its own
and the geometry of the source axis is pinned to the one the gradient takes for all N targets."""
import ctypes
import functools

import numpy as np
import pytest

import meanshift_reference as mr
from kernel_matrix_benchmarks_amd import _lib
from kernel_matrix_benchmarks_amd.algorithms.mi355x import MI355XMeanShift

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED, NOT_CONVERGED = 1, 2, 6
KEYS = ("modes", "iters", "step2", "sweeps", "target_sweeps", "converged")
MAXITS = (1, 2, 7, 40)
TOL = {"float32": 1e-4, "float64": 1e-10}
PRECISIONS = [np.float32, np.float64]
name_of = lambda p: np.dtype(p).name


def codes(precision):
    return (_lib.KMVP_F64, np.float64) if np.dtype(precision) == np.float64 else (_lib.KMVP_F32, np.float32)


def device_array(a, precision):
    return None if a is None else np.ascontiguousarray(a, dtype=codes(precision)[1])


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in KEYS)


def describe(a, b):
    return {k: (np.asarray(a[k]).ravel()[:6], np.asarray(b[k]).ravel()[:6]) for k in KEYS if not np.array_equal(a[k], b[k], equal_nan=True)}


class Ctx:
    """One context with sources y, seeds x (None: the cloud itself) and the log-weights c (None: all 0)."""

    def __init__(self, y, x, c, precision, options=()):
        self.ctx = _lib.Context(0)
        try:
            for key, value in options:
                self.ctx.set_option(key, value)
            self.ctx.set_points(device_array(y, precision), device_array(x, precision), codes(precision)[0])
            self.ctx.set_signal(device_array(c, precision))
        except Exception:
            self.ctx.close()
            raise

    def __enter__(self):
        return self.ctx

    def __exit__(self, *exc):
        self.ctx.close()


def solve(ctx, tol, maxit):
    out = ctx.meanshift(tol, maxit)
    assert out["modes"].shape == (ctx.N, ctx.D) and out["modes"].dtype == np.float64
    assert out["iters"].shape == (ctx.N,) and out["step2"].shape == (ctx.N,)
    assert ctx.last_kernel_name == "lowd_lse_grad_kernel" and ctx.last_dispatch_note == ""
    assert ctx.last_kernel_ms > 0 and ctx.last_total_ms == ctx.last_kernel_ms
    return out


def host_loop(y, x, c, precision, tol, maxits, options=()):
    """The restatement on the device's own gradient, for every maxit of `maxits` from ONE walk: a trajectory cut at a
    smaller maxit is a prefix of the longer one, so the k-th gradient is computed once and played back."""
    dtype = codes(precision)[0]
    yd, cd = device_array(y, precision), device_array(c, precision)
    N, D = (y if x is None else x).shape
    played = []
    ctx = _lib.Context(0)
    try:
        for key, value in options:
            ctx.set_option(key, value)
        out = {}
        for maxit in sorted(maxits):
            calls = [0]

            def grad(targets):
                k = calls[0]
                calls[0] += 1
                if k == len(played):
                    ctx.set_points(yd, np.ascontiguousarray(targets), dtype)  # all N targets, every sweep
                    ctx.set_signal(cd)
                    ctx.run_lse_grad("gaussian")
                    played.append((np.array(targets), ctx.get_result(N, D)))
                assert np.array_equal(played[k][0], targets, equal_nan=True)
                return played[k][1]

            seeds = y if x is None else x
            out[maxit] = mr.meanshift(grad, seeds, tol, maxit, precision=codes(precision)[1], all_rows=True)
        return out
    finally:
        ctx.close()


# ---- the inputs --------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (63, 5), (600, 2000), (300, 257)]


@functools.lru_cache(maxsize=None)
def inputs(D, N, M, weighted, seeds):
    """(y (M, D), x (N, D) or None, c (M, 1) or None).  seeds: "first" the first N points of the cloud (the data, as far
    as it reaches), "other" N points of another draw of the cloud, "same" the cloud itself through x == NULL (N == M)."""
    pts = mr.cloud(max(N, M), D, seed=D)
    y = pts[:M]
    x = {"first": pts[:N], "other": mr.cloud(max(N, 4), D, seed=50 + D)[:N] + 0.01, "same": None}[seeds]
    assert seeds != "same" or N == M
    c = None
    if weighted:
        rs = np.random.RandomState(7 * D + M)
        w = rs.rand(M) + 0.05
        w[rs.rand(M) < 0.1] = 0.0  # points of mass 0
        w[0] = 1.0                 # (M = 1: the one source keeps its mass)
        with np.errstate(divide="ignore"):
            c = np.log(w).reshape(M, 1)
    return y, x, c


@functools.lru_cache(maxsize=None)
def reference(D, precision_name, N, M, weighted, seeds, options=(), maxits=MAXITS):
    y, x, c = inputs(D, N, M, weighted, seeds)
    return host_loop(y, x, c, np.dtype(precision_name), TOL[precision_name], maxits, options)


def check_parity(D, precision, N, M, weighted, seeds, maxit, options=(), solver_options=None, maxits=MAXITS):
    y, x, c = inputs(D, N, M, weighted, seeds)
    want = reference(D, name_of(precision), N, M, weighted, seeds, options, maxits)[maxit]
    with Ctx(y, x, c, precision, options if solver_options is None else solver_options) as ctx:
        got = solve(ctx, TOL[name_of(precision)], maxit)
    print(f"D={D} {name_of(precision)} N={N} M={M} weighted={weighted} seeds={seeds} maxit={maxit}: sweeps {got['sweeps']} / "
          f"{want['sweeps']}, target_sweeps {got['target_sweeps']} / {want['target_sweeps']}, frozen "
          f"{int(np.sum(got['iters'] < got['sweeps']))}, converged {got['converged']} / {want['converged']}")
    assert same_bits(got, want), describe(got, want)
    return got, want


# ---- 1. trajectory parity ----------------------------------------------------------------------------------------------------
CASES = [(N, M, seeds) for (N, M) in SHAPES for seeds in ("first", "other")] + [(1, 1, "same"), (257, 257, "same")]


@pytest.mark.parametrize("maxit", MAXITS)
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("N,M,seeds", CASES)
@pytest.mark.parametrize("precision", PRECISIONS, ids=name_of)
@pytest.mark.parametrize("D", [1, 3, 8])
def test_trajectory_parity(D, precision, N, M, seeds, weighted, maxit):
    got, want = check_parity(D, precision, N, M, weighted, seeds, maxit)
    assert got["sweeps"] <= maxit and np.all(got["iters"] >= 1) and np.all(got["iters"] <= got["sweeps"])
    if (N, M) == (600, 2000) and maxit == 40:
        # the condition of the test: points freeze along the way, so the active set shrinks across the 256-target tiles
        assert got["target_sweeps"] < N * got["sweeps"]
        if seeds == "first":
            assert np.sum(want["iters"] < want["sweeps"]) >= 0.1 * N


# ---- 2. pinned geometry ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("options", [(("segments", 1),), (("segments", 3),), (), (("chunk", 64),), (("segments", 3), ("chunk", 256))],
                         ids=["segments1", "segments3", "auto", "chunk64", "segments3-chunk256"])
@pytest.mark.parametrize("N,M", [(600, 2000), (300, 257)])
@pytest.mark.parametrize("precision", PRECISIONS, ids=name_of)
def test_pinned_geometry(precision, N, M, options):
    for maxit in (7, 40):
        check_parity(3, precision, N, M, True, "first", maxit, options=options, maxits=(7, 40))


def test_pinned_geometry_when_the_active_count_leaves_the_large_regime():
    """33 000 seeds: the gradient's geometry for N >= 32768 targets (long segments) must stay while the active count
    falls below that threshold, where a launch sized afresh would take the short segments of a small problem."""
    N, M, D, maxit = 33000, 2000, 3, 12
    got, want = check_parity(D, np.float32, N, M, False, "other", maxit, maxits=(maxit,))
    frozen_before_last = int(np.sum(want["iters"] < want["sweeps"] - 1))
    assert N - frozen_before_last < 32768, "the condition of the test: the active count crosses the threshold"
    assert got["sweeps"] == maxit


# ---- 3. compaction -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("precision", PRECISIONS, ids=name_of)
@pytest.mark.parametrize("D", [1, 3, 8])
def test_compaction_does_not_enter_the_bits(D, precision, weighted):
    y, x, c = inputs(D, 600, 2000, weighted, "first")
    tol = TOL[name_of(precision)]
    with Ctx(y, x, c, precision) as ctx:
        default = solve(ctx, tol, 40)
        again = solve(ctx, tol, 40)  # run to run, on one context
        ctx.set_option("meanshift_compact", 0)
        riding = solve(ctx, tol, 40)
        ctx.set_option("meanshift_compact", 1)
        on = solve(ctx, tol, 40)
    with Ctx(y, x, c, precision, (("meanshift_compact", 0),)) as ctx:
        alone = solve(ctx, tol, 40)
    for other in (again, riding, on, alone):
        assert same_bits(default, other), describe(default, other)
    assert default["target_sweeps"] < 600 * default["sweeps"]
    with Ctx(y, x, c, precision) as ctx:
        with pytest.raises(_lib.KmvpError):
            ctx.set_option("meanshift_compact", 2)


# ---- 4. to convergence -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS, ids=name_of)
def test_to_convergence(precision):
    tol = TOL[name_of(precision)]
    got, want = check_parity(3, precision, 600, 2000, False, "first", 2000, maxits=(2000,))
    assert got["converged"] and want["converged"] and got["sweeps"] < 2000
    assert np.all(got["step2"] <= tol * tol) and np.all(np.isfinite(got["modes"]))
    assert np.array_equal(got["iters"] == got["sweeps"], want["iters"] == want["sweeps"])


# ---- 5. conventions ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS, ids=name_of)
def test_a_far_seed_is_finite_and_lands_on_the_data(precision):
    rs = np.random.RandomState(0)
    y = 0.25 * rs.randn(500, 3)
    x = np.array([[30.0, 0.0, 0.0], [0.0, -40.0, 0.0], [0.1, 0.1, 0.1]])
    tol = TOL[name_of(precision)]
    with Ctx(y, x, None, precision) as ctx:
        got = solve(ctx, tol, 500)
        ctx.run("gaussian", False)  # the plain density at the far seeds underflows to 0: the naive ratio is 0 / 0
        assert np.all(ctx.get_result(3, 1)[:2] == 0.0)
    assert got["converged"] and np.all(np.isfinite(got["modes"]))
    assert np.all(np.linalg.norm(got["modes"], axis=1) < 0.2)
    want = host_loop(y, x, None, precision, tol, (500,))[500]
    assert same_bits(got, want), describe(got, want)


@pytest.mark.parametrize("precision", PRECISIONS, ids=name_of)
def test_a_nan_seed_gives_a_nan_row_and_only_that_row(precision):
    y, x, c = inputs(3, 300, 257, True, "first")
    x = x.copy()
    x[17, 1] = np.nan
    tol = TOL[name_of(precision)]
    with Ctx(y, x, c, precision) as ctx:
        got = solve(ctx, tol, 40)
    with Ctx(y, np.delete(x, 17, axis=0), c, precision) as ctx:
        rest = solve(ctx, tol, 40)
    assert np.all(np.isnan(got["modes"][17])) and np.isnan(got["step2"][17]) and got["iters"][17] == 1 and not got["converged"]
    keep = np.arange(300) != 17
    assert np.all(np.isfinite(got["modes"][keep]))
    # the other rows are those of a solve without that seed (the seed count changes nothing either: M fixes the source axis
    # here, below the threshold between the geometries)
    assert np.array_equal(got["modes"][keep], rest["modes"]) and np.array_equal(got["iters"][keep], rest["iters"])
    assert np.array_equal(got["step2"][keep], rest["step2"])
    assert got["target_sweeps"] == rest["target_sweeps"] + 1
    want = host_loop(y, x, c, precision, tol, (40,))[40]
    assert same_bits(got, want), describe(got, want)


@pytest.mark.parametrize("precision", PRECISIONS, ids=name_of)
def test_no_mass_anywhere_is_nan_everywhere(precision):
    y, x, _ = inputs(3, 63, 5, False, "first")
    c = np.full((5, 1), -np.inf)
    with Ctx(y, x, c, precision) as ctx:
        got = solve(ctx, TOL[name_of(precision)], 40)
        rc = ctx._lib.kmvp_gaussian_meanshift(ctx._ctx, 1e-4, 40, got["modes"].ctypes.data, np.empty(63, dtype=np.intc).ctypes.data,
                                              got["step2"].ctypes.data, ctypes.byref(ctypes.c_int(0)), ctypes.byref(ctypes.c_int64(0)))
        assert rc == NOT_CONVERGED and "not finite" in ctx._lib.kmvp_last_error(ctx._ctx).decode()
    assert np.all(np.isnan(got["modes"])) and np.all(np.isnan(got["step2"])) and np.all(got["iters"] == 1)
    assert got["sweeps"] == 1 and got["target_sweeps"] == 63 and not got["converged"]


@pytest.mark.parametrize("precision", PRECISIONS, ids=name_of)
def test_maxit_reached_is_not_converged_with_everything_written(precision):
    y, x, c = inputs(3, 600, 2000, False, "first")
    tol = TOL[name_of(precision)]
    with Ctx(y, x, c, precision) as ctx:
        got = solve(ctx, tol, 7)
        modes = np.full((600, 3), -7.0)
        iters = np.full(600, -7, dtype=np.intc)
        step2 = np.full(600, -7.0)
        sweeps, ts = ctypes.c_int(-7), ctypes.c_int64(-7)
        rc = ctx._lib.kmvp_gaussian_meanshift(ctx._ctx, tol, 7, modes.ctypes.data, iters.ctypes.data, step2.ctypes.data,
                                              ctypes.byref(sweeps), ctypes.byref(ts))
        assert rc == NOT_CONVERGED and "maxit" in ctx._lib.kmvp_last_error(ctx._ctx).decode()
    assert not got["converged"] and got["sweeps"] == sweeps.value == 7 and ts.value == got["target_sweeps"]
    assert np.array_equal(modes, got["modes"]) and np.array_equal(iters, got["iters"]) and np.array_equal(step2, got["step2"])
    moving = got["step2"] > tol * tol
    assert np.any(moving) and np.all(got["iters"][moving] == 7) and np.all(got["step2"][~moving] <= tol * tol)
    assert np.all(np.isfinite(got["modes"])) and np.all(got["iters"] >= 1)


@pytest.mark.parametrize("precision", PRECISIONS, ids=name_of)
def test_no_side_effects_on_the_context(precision):
    """A product, its gradient, the log-sum-exp and its gradient, kmvp_nearest and kmvp_kmeans return the same bits before
    and after a mean-shift solve on the same context, and the same as on a context that never saw one."""
    y, x, c = inputs(3, 300, 257, True, "other")
    c = np.where(np.isfinite(c), c, -3.0)  # (a finite signal, so that the product is one too)
    tol = TOL[name_of(precision)]

    def others(ctx):
        ctx.run("gaussian", False)
        prod = ctx.get_result(300, 1)
        ctx.run_grad("gaussian")
        grad = ctx.get_result(300, 3)
        ctx.run_lse("gaussian")
        lse = ctx.get_result(300, 1)
        ctx.run_lse_grad("gaussian")
        lse_grad = ctx.get_result(300, 3)
        idx, sq = ctx.run_nearest(4, False)
        km = ctx.kmeans(5, x[:5], None, 0.0, 20)
        return (prod, grad, lse, lse_grad, idx, sq) + tuple(np.asarray(v) for v in km)

    with Ctx(y, x, c, precision) as ctx:
        first = solve(ctx, tol, 40)  # the solve itself packs the records: nothing before it
        before = others(ctx)
        out = solve(ctx, tol, 40)
        after = others(ctx)
        ctx.run_lse_grad("gaussian")
        out2 = solve(ctx, tol, 40)   # right behind the gradient whose scratch it shares
        again = others(ctx)
        # get_result still returns the result of the call before the solve
        ctx.run_lse("gaussian")
        lse = ctx.get_result(300, 1)
        solve(ctx, tol, 3)
        assert np.array_equal(ctx.get_result(300, 1), lse)
    with Ctx(y, x, c, precision) as ctx:
        alone = others(ctx)
    for got in (after, again, alone):
        assert all(np.array_equal(g, w, equal_nan=True) for g, w in zip(got, before))
    assert np.isfinite(before[0]).all() and same_bits(first, out) and same_bits(out, out2) and out["sweeps"] > 1


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------
def raw(ctx, tol=1e-4, maxit=10, null=()):
    """The entry point itself, every pointer spelled out; `null`: the outputs passed as NULL.  Returns (status, message)."""
    N, D = max(int(getattr(ctx, "N", 0)), 1), max(int(getattr(ctx, "D", 0)), 1)
    bufs = dict(modes=np.empty((N, D)), iters=np.empty(N, dtype=np.intc), step2=np.empty(N))
    sweeps, ts = ctypes.c_int(0), ctypes.c_int64(0)
    ptr = lambda name: None if name in null else bufs[name].ctypes.data
    ref = lambda name, v: None if name in null else ctypes.byref(v)
    rc = ctx._lib.kmvp_gaussian_meanshift(ctx._ctx, tol, maxit, ptr("modes"), ptr("iters"), ptr("step2"), ref("sweeps", sweeps),
                                          ref("target_sweeps", ts))
    return rc, ctx._lib.kmvp_last_error(ctx._ctx).decode()


def refused(prepare, **kwargs):
    ctx = _lib.Context(0)
    try:
        prepare(ctx)
        return raw(ctx, **kwargs)
    finally:
        ctx.close()


def test_invalid_arguments():
    x32 = np.ascontiguousarray(mr.cloud(200, 3), dtype=np.float32)
    rc, msg = refused(lambda ctx: None)
    assert rc == INVALID and "kmvp_set_points has not been called" in msg
    rc, msg = refused(lambda ctx: ctx.set_points(x32, None, _lib.KMVP_F32))
    assert rc == INVALID and "kmvp_set_signal has not been called" in msg
    ready = lambda ctx: (ctx.set_points(x32, None, _lib.KMVP_F32), ctx.set_signal(None))
    for kwargs in (dict(tol=-1e-9), dict(tol=float("nan")), dict(maxit=0), dict(maxit=-3), dict(null=("modes",)), dict(null=("iters",)),
                   dict(null=("step2",)), dict(null=("sweeps",)), dict(null=("target_sweeps",))):
        rc, msg = refused(ready, **kwargs)
        assert rc == INVALID and "bad mean-shift arguments" in msg, kwargs
    rc, msg = refused(ready, tol=0.0, maxit=1)
    assert rc in (0, NOT_CONVERGED)
    empty = np.empty((0, 3), dtype=np.float32)
    rc, msg = refused(lambda ctx: (ctx.set_points(x32, empty, _lib.KMVP_F32), ctx.set_signal(None)))  # N = 0
    assert rc == INVALID and "at least one seed and one source" in msg
    rc, msg = refused(lambda ctx: (ctx.set_points(empty, x32, _lib.KMVP_F32), ctx.set_signal(None)))  # M = 0
    assert rc == INVALID and "at least one seed and one source" in msg
    with pytest.raises(ValueError):
        MI355XMeanShift(dimension=3, tol=-1.0)
    with pytest.raises(ValueError):
        MI355XMeanShift(dimension=3).prepare_data(points=x32, weights=-np.ones(200))
    with pytest.raises(ValueError):
        MI355XMeanShift(dimension=3).prepare_data(points=x32, weights=np.full(200, np.inf))
    with pytest.raises(ValueError):
        MI355XMeanShift(dimension=3).prepare_data(points=x32, seeds=np.zeros((4, 2)))
    with pytest.raises(RuntimeError):
        MI355XMeanShift(dimension=3).query()


def test_unsupported_configurations():
    x32 = np.ascontiguousarray(mr.cloud(200, 3), dtype=np.float32)
    ready = lambda ctx, dtype=_lib.KMVP_F32: (ctx.set_points(x32, None, dtype), ctx.set_signal(None))
    rc, msg = refused(lambda ctx: ready(ctx, _lib.KMVP_BF16))
    assert rc == UNSUPPORTED and "not for bfloat16" in msg
    x9 = np.ascontiguousarray(np.random.RandomState(0).rand(50, 9), dtype=np.float32)
    rc, msg = refused(lambda ctx: (ctx.set_points(x9, None, _lib.KMVP_F32), ctx.set_signal(None)))
    assert rc == UNSUPPORTED and "D = 9 is beyond" in msg
    b2 = np.zeros((200, 2), dtype=np.float32)
    rc, msg = refused(lambda ctx: (ctx.set_points(x32, None, _lib.KMVP_F32), ctx.set_signal(b2)))
    assert rc == UNSUPPORTED and "2 columns" in msg
    for form in (1, 2, 3, 4):
        rc, msg = refused(lambda ctx: (ctx.set_option("fast_sqdists", form), ready(ctx)))
        assert rc == UNSUPPORTED and f"fast_sqdists = {form}" in msg
    for form in (-1, 0):
        rc, msg = refused(lambda ctx: (ctx.set_option("fast_sqdists", form), ready(ctx)))
        assert rc in (0, NOT_CONVERGED)
    rc, msg = refused(lambda ctx: (ctx.comm_init_host(lambda a, op: None, 0, 1), ready(ctx)))
    assert rc == UNSUPPORTED and "a communicator is attached" in msg
    rc, msg = refused(lambda ctx: (ctx.set_points(x32[:150], x32, _lib.KMVP_F32, j_offset=0, M_total=200), ctx.set_signal(None)))
    assert rc == UNSUPPORTED and "the sources are a slice" in msg
    with pytest.raises(NotImplementedError):
        MI355XMeanShift(dimension=3, precision="bfloat16")


# ---- 7. plugin ---------------------------------------------------------------------------------------------------------------
def plugin(points, weights, seeds, precision, tol, maxit, **options):
    algo = MI355XMeanShift(dimension=points.shape[1], precision=precision, **options)
    try:
        algo.prepare_data(points=points, weights=weights, seeds=seeds)
        algo.set_query_arguments(tol=tol, maxit=maxit)
        algo.fit()
        algo.query()
        extra = algo.get_additional()
        assert extra["device_kernel"] == "lowd_lse_grad_kernel" and extra["device_total_ms"] == extra["device_kernel_ms"] > 0
        assert algo.get_memory_usage() > 0
        out = dict(modes=algo.get_modes(), iters=algo.get_iterations(), step2=algo.step2, sweeps=extra["sweeps"],
                   target_sweeps=extra["target_sweeps"], converged=extra["converged"])
        return out, extra, algo.get_clusters
    finally:
        algo.done()


@pytest.mark.parametrize("precision", [np.float32, np.float64, np.float16], ids=name_of)
@pytest.mark.parametrize("seeds", ["same", "other"])
def test_plugin_gives_the_context_results(precision, seeds):
    M, N = 2000, (2000 if seeds == "same" else 600)
    y, x, c = inputs(3, N, M, True, seeds)
    with np.errstate(divide="ignore"):
        w = np.exp(c[:, 0])
    work = np.float64 if precision == np.float64 else np.float32
    tol = TOL[name_of(work)]
    r16 = (lambda a: None if a is None else a.astype(np.float16).astype(np.float64)) if precision == np.float16 else (lambda a: a)
    got, extra, _ = plugin(y, w, x, precision, tol, 25)
    # the plugin's log-weights are log(w) rounded to the working precision
    with np.errstate(divide="ignore"):
        cw = np.log(w).reshape(M, 1)
    with Ctx(r16(y), r16(x), cw, work) as ctx:
        want = solve(ctx, tol, 25)
    assert same_bits(got, want), describe(got, want)
    assert got["iters"].dtype == np.int64
    assert extra["unconverged"] == int(np.sum(~(got["step2"] <= tol * tol))) and extra["unconverged"] > 0
    if precision == np.float32:
        riding, _, _ = plugin(y, w, x, precision, tol, 25, compact=False, segments=3)
        with Ctx(y, x, cw, work, (("segments", 3),)) as ctx:
            assert same_bits(riding, solve(ctx, tol, 25))


@pytest.mark.parametrize("precision", PRECISIONS, ids=name_of)
def test_plugin_clusters_equal_the_restatements_rule(precision):
    y, _, _ = inputs(3, 600, 2000, False, "first")
    tol = TOL[name_of(precision)]
    # maxit = 60: most seeds have arrived, some are still moving (they get -1 and found nothing)
    got, extra, get_clusters = plugin(y, None, y[:600], precision, tol, 60)
    centres, labels = get_clusters(0.5)
    want_centres, want_labels = mr.clusters(got["modes"], got["step2"], tol, 0.5)
    print(f"{name_of(precision)}: {len(centres)} centres ({len(want_centres)} by the restatement), {extra['unconverged']} seeds unconverged")
    assert np.array_equal(centres, want_centres) and np.array_equal(labels, want_labels)
    assert labels.dtype == np.int64 and centres.dtype == np.float64 and centres.shape[1] == 3
    moving = ~(got["step2"] <= tol * tol)
    assert np.all(labels[moving] == -1) and np.all(labels[~moving] >= 0)
    # at least the two blobs, as distinct centres: one within 0.5 of the origin, one within 0.5 of 5 e_0
    near = lambda p: np.flatnonzero(np.linalg.norm(centres - np.asarray(p), axis=1) < 0.5)
    assert near([0, 0, 0]).size >= 1 and near([5, 0, 0]).size >= 1 and not set(near([0, 0, 0])) & set(near([5, 0, 0]))
    # another radius, and a radius of 0 (every distinct mode its own centre), against the rule as well
    for radius in (2.0, 0.0):
        c2, l2 = get_clusters(radius)
        w2, wl2 = mr.clusters(got["modes"], got["step2"], tol, radius)
        assert np.array_equal(c2, w2) and np.array_equal(l2, wl2)
