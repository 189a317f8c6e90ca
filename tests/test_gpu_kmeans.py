"""GPU tests of the device-resident Lloyd iteration (include/kmvp.h kmvp_kmeans: lowd_knn_kernel at K = 1, the centroid
update of csrc/kmvp_kmeans.hip) against the numpy restatement of its definition (kmeans_reference.py, itself checked
against a textbook loop in test_kmeans_reference.py).

The kernel's working-precision distance differs from the true one by at most gamma = (D + 3) u relative (as in
test_gpu_knn.py; u = 2^-24 for float32 / float16 inputs, 2^-53 for float64).  Exact parity of a whole trajectory is a fair
demand only where no point ever sits between two centroids within that: the trajectory tests first assert, on the
restatement alone, that the run's smallest relative gap (s2 - s1) / s2 is at least 8 gamma.  Sums are float64 on both
sides, in different orders: a centroid may differ by n_c 2^-52 max|x| + 2^-52 |c| per coordinate (n_c: points of the
cluster), the inertia by gamma relative."""
import ctypes
import functools

import numpy as np
import pytest

import kmeans_reference as kr
import knn_reference as kn
from kernel_matrix_benchmarks_amd import _lib
from kernel_matrix_benchmarks_amd.algorithms.mi355x import MI355XKMeans, MI355XProduct

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED, NOT_CONVERGED = 1, 2, 6
EPS64 = 2.0 ** -52


def unit(precision):
    return 2.0 ** -53 if np.dtype(precision) == np.float64 else 2.0 ** -24


def gamma_of(D, precision):
    return (D + 3) * unit(precision)


def rounded(a, precision):
    return np.asarray(a, dtype=precision).astype(np.float64)


def codes(precision):
    """(kmvp_dtype, host dtype) of a context that computes on inputs of `precision` (float16: rounded, then float32)."""
    return (_lib.KMVP_F64, np.float64) if np.dtype(precision) == np.float64 else (_lib.KMVP_F32, np.float32)


class Ctx:
    """One context whose targets are the points (the cloud itself), through the C ABI's typed wrapper."""

    def __init__(self, points, precision, *, options=()):
        dtype, npdt = codes(precision)
        self.ctx = _lib.Context(0)
        try:
            for key, value in options:
                self.ctx.set_option(key, value)
            self.ctx.set_points(np.ascontiguousarray(rounded(points, precision), dtype=npdt), None, dtype)
        except Exception:
            self.ctx.close()
            raise

    def __enter__(self):
        return self.ctx

    def __exit__(self, *exc):
        self.ctx.close()


KEYS = ("centroids", "labels", "cluster_weight", "iterations", "inertia", "shift", "converged")


def ctx_kmeans(ctx, C, c0, weights=None, tol=0.0, maxit=300):
    out = dict(zip(KEYS, ctx.kmeans(C, c0, weights, tol, maxit)))
    assert out["centroids"].shape == (C, ctx.D) and out["centroids"].dtype == np.float64
    assert out["labels"].shape == (ctx.N,) and out["labels"].dtype == np.int64
    assert out["cluster_weight"].shape == (C,) and out["cluster_weight"].dtype == np.float64
    assert ctx.last_kernel_name == "lowd_knn_kernel" and ctx.last_dispatch_note == ""
    assert ctx.last_kernel_ms > 0 and ctx.last_total_ms == ctx.last_kernel_ms
    return out


def plugin_kmeans(x, C, c0, precision, weights=None, tol=0.0, maxit=300, segments=0):
    algo = MI355XKMeans(n_clusters=C, dimension=x.shape[1], precision=precision, tol=tol, maxit=maxit, segments=segments)
    try:
        algo.prepare_data(points=x, weights=weights)
        algo.fit()
        algo.query(init=c0)
        extra = algo.get_additional()
        assert extra["device_kernel"] == "lowd_knn_kernel" and extra["device_total_ms"] == extra["device_kernel_ms"] > 0
        assert algo.get_memory_usage() > 0
        return dict(centroids=algo.get_centroids(), labels=algo.get_labels(), cluster_weight=algo.get_cluster_weights(),
                    iterations=extra["iterations"], inertia=extra["inertia"], shift=extra["shift"], converged=extra["converged"])
    finally:
        algo.done()


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in KEYS)


def centroid_tolerance(x, labels, centroids):
    """n_c 2^-52 max|x| + 2^-52 |c| per coordinate: float64 sums of n_c terms in another order, one division."""
    counts = np.bincount(labels[labels >= 0], minlength=len(centroids)).astype(np.float64)
    biggest = float(np.max(np.abs(x[np.isfinite(x).all(axis=1)])))  # (of the points that can carry a label)
    return counts[:, None] * EPS64 * biggest + EPS64 * np.abs(centroids)


# ---- 1. trajectory parity -------------------------------------------------------------------------------------------------
def cloud(D, seed, N, precision):
    return rounded(np.random.RandomState(100 * D + seed).rand(N, D), precision)


@functools.lru_cache(maxsize=None)
def restated(D, seed, N, C, precision_name, tol=0.0):
    x = cloud(D, seed, N, np.dtype(precision_name))
    return kr.kmeans(x, x[:C], tol=tol, maxit=300, precision=np.dtype(precision_name))


# the (shape, seed) cases whose smallest gap is far enough from the working precision's rounding; float64: all of them
F64_CASES = {D: [((1000, 7), s) for s in range(3)] + [((3000, 37), s) for s in range(3)] for D in (1, 3, 8)}
F32_CASES = {
    1: [((1000, 7), s) for s in range(3)] + [((3000, 37), s) for s in range(3)],
    3: [((1000, 7), 0), ((1000, 7), 2)] + [((3000, 37), s) for s in range(3)],
    8: [((1000, 7), 0), ((1000, 7), 1)] + [((3000, 37), s) for s in range(3)],
}


def check_against(want, got, x, gamma, label):
    print(f"{label}: iterations {got['iterations']} / {want['iterations']}, labels differing "
          f"{int(np.sum(got['labels'] != want['labels']))}, max centroid difference "
          f"{float(np.max(np.abs(got['centroids'] - want['centroids']))):.3e}, relative inertia difference "
          f"{abs(got['inertia'] - want['inertia']) / want['inertia']:.3e} (gamma {gamma:.3e}), shift {got['shift']!r}")
    assert got["iterations"] == want["iterations"], label
    assert np.array_equal(got["labels"], want["labels"]), label
    assert np.array_equal(got["cluster_weight"], want["cluster_weight"]), label
    assert np.all(np.abs(got["centroids"] - want["centroids"]) <= centroid_tolerance(x, want["labels"], want["centroids"])), label
    assert abs(got["inertia"] - want["inertia"]) <= gamma * want["inertia"], label
    assert bool(got["converged"]) == bool(want["converged"]), label


@pytest.mark.parametrize("precision", [np.float64, np.float32], ids=lambda p: np.dtype(p).name)
@pytest.mark.parametrize("D", [1, 3, 8])
def test_trajectory_parity(D, precision):
    """tol = 0 from the first C points: the iteration count, every label and every cluster weight equal the restatement's,
    the run ends converged with shift exactly 0, centroids and inertia agree to the rounding of their sums."""
    gamma = gamma_of(D, precision)
    cases = (F64_CASES if np.dtype(precision) == np.float64 else F32_CASES)[D]
    for i, ((N, C), seed) in enumerate(cases):
        want = restated(D, seed, N, C, np.dtype(precision).name)
        label = f"{np.dtype(precision).name} D={D} ({N}, {C}) seed {seed}"
        print(f"{label}: smallest relative gap of the restatement {want['min_gap'] / gamma:.3g} gamma")
        assert want["min_gap"] >= 8 * gamma, label  # the condition: on the restatement alone
        assert want["converged"] and want["shift"] == 0.0 and np.all(want["cluster_weight"] > 0), label
        x = cloud(D, seed, N, precision)
        with Ctx(x, precision) as ctx:
            got = ctx_kmeans(ctx, C, x[:C])
        check_against(want, got, x, gamma, label)
        assert got["converged"] and got["shift"] == 0.0, label
        if i % 3 == 0:  # the plugin is the same call: the same bits
            assert same_bits(plugin_kmeans(x, C, x[:C], precision), got), label


def test_trajectory_with_a_positive_tolerance():
    """tol between two consecutive shifts of the restatement's run: both stop at the same iteration."""
    D, seed, N, C = 3, 0, 1000, 7
    full = restated(D, seed, N, C, "float32")
    assert full["iterations"] > 6 and full["min_gap"] >= 8 * gamma_of(D, np.float32)
    tol = float(np.sqrt(full["shifts"][3] * full["shifts"][4]))
    # (no shift of the run within 0.1 % of tol: the two sides' shifts differ by the rounding of float64 sums only)
    assert full["shifts"][4] < tol < full["shifts"][3] and all(abs(s / tol - 1) > 1e-3 for s in full["shifts"])
    x = cloud(D, seed, N, np.float32)
    want = kr.kmeans(x, x[:C], tol=tol, maxit=300, precision=np.float32)
    assert want["converged"] and 1 < want["iterations"] < full["iterations"] and want["shift"] > 0
    with Ctx(x, np.float32) as ctx:
        got = ctx_kmeans(ctx, C, x[:C], tol=tol)
    check_against(want, got, x, gamma_of(D, np.float32), "tol > 0")
    assert got["converged"] and 0 < got["shift"] <= tol
    assert same_bits(plugin_kmeans(x, C, x[:C], np.float32, tol=tol), got)


@pytest.mark.parametrize("precision", [np.float64, np.float32], ids=lambda p: np.dtype(p).name)
def test_trajectory_with_weights(precision):
    """Non-uniform weights, a quarter of them 0: the same demands, the cluster weights now sums of small integers (exact)."""
    D, N, C = 3, 1000, 7
    gamma = gamma_of(D, precision)
    x = cloud(D, 0, N, precision)
    w = np.random.RandomState(77).randint(0, 4, size=N).astype(np.float64)
    want = kr.kmeans(x, x[:C], w, tol=0.0, maxit=300, precision=precision)
    print(f"weights {np.dtype(precision).name}: smallest relative gap {want['min_gap'] / gamma:.3g} gamma")
    assert want["min_gap"] >= 8 * gamma and want["converged"] and np.sum(w == 0) > 100
    with Ctx(x, precision) as ctx:
        got = ctx_kmeans(ctx, C, x[:C], w)
    check_against(want, got, x, gamma, "weights")
    assert got["converged"] and got["shift"] == 0.0
    assert same_bits(plugin_kmeans(x, C, x[:C], precision, weights=w), got)


# ---- 2. self-consistency ---------------------------------------------------------------------------------------------------
def check_one_iteration(out, x, w, prior, precision, label, rows=None):
    """`out`: one iteration (maxit = 1) from the centroids `prior`, held to the definition in extended precision on the
    rounded inputs.  rows: the points whose distances to ALL centroids are examined (None: every point)."""
    N, D = x.shape
    C = len(prior)
    gamma = gamma_of(D, precision)
    labels, cent, cw = out["labels"], out["centroids"], out["cluster_weight"]
    assert out["iterations"] == 1 and np.all(labels >= 0) and np.all(labels < C), label
    # cluster weights: the bincount of the labels (sums of small integers: exact)
    assert np.array_equal(cw, np.bincount(labels, weights=w, minlength=C)), label
    # centroids: the weighted mean of the points that carry the label; clusters without weight bitwise where they were
    xl, wl = x.astype(np.longdouble), w.astype(np.longdouble)
    empty = cw == 0
    assert np.array_equal(cent[empty], prior[empty]), label
    order = np.argsort(labels, kind="stable")
    starts = np.searchsorted(labels[order], np.arange(C + 1))
    worst = 0.0
    tol = centroid_tolerance(x, labels, cent)
    for c in np.nonzero(~empty)[0]:
        members = order[starts[c]:starts[c + 1]]
        m = np.sum(wl[members, None] * xl[members], axis=0) / np.sum(wl[members])
        err = np.abs(cent[c].astype(np.longdouble) - m)
        worst = max(worst, float(np.max(err / tol[c])))
    # the assignment: against the centroids as the kernel sees them, rounded to the working precision
    real = kr.working(precision)
    pr = prior.astype(real).astype(np.longdouble)
    own = np.sum((xl - pr[labels]) ** 2, axis=1)
    sel = np.arange(N) if rows is None else rows
    slack = np.inf
    for lo in range(0, len(sel), 256):
        r = sel[lo:lo + 256]
        s_all = np.sum((xl[r, None, :] - pr[None, :, :]) ** 2, axis=-1) if D > 1 else (xl[r, 0:1] - pr[None, :, 0]) ** 2
        slack = min(slack, float(np.min(s_all * (1 + gamma) - own[r, None] * (1 - gamma))))
    inertia = np.sum(wl * own)
    rel = float(abs(np.longdouble(out["inertia"]) - inertia) / inertia) if inertia > 0 else abs(out["inertia"])
    shift = float(np.sum((cent - prior) ** 2))
    print(f"{label}: worst centroid error {worst:.3f} of its tolerance; smallest slack of another centroid {slack:.3e}; "
          f"relative inertia error {rel:.3e} (gamma {gamma:.3e}); {int(empty.sum())} of {C} clusters empty")
    assert worst <= 1.0, label
    assert slack >= 0.0, label
    assert rel <= gamma, label
    assert abs(out["shift"] - shift) <= 1e-14 * shift, label


SMALL_SHAPES = ((1, 1), (63, 3), (65, 5), (300, 257))
# no single-pass LDS layout holds these: C > 160 KiB / (8 (D + 2))
BIG_SHAPES = {1: (20000, 8192), 8: (5000, 2100)}


@pytest.mark.parametrize("precision", [np.float64, np.float32, np.float16], ids=lambda p: np.dtype(p).name)
@pytest.mark.parametrize("D", [1, 3, 8])
def test_self_consistency(D, precision):
    """Random centroids (many clusters of (300, 257) empty or singletons), non-uniform weights: a few iterations, then ONE
    more from the centroids they returned, which is held to the definition; a run to the end whose last iteration, repeated,
    changes nothing."""
    rs = np.random.RandomState(10 * D + np.dtype(precision).itemsize)
    shapes = SMALL_SHAPES + ((BIG_SHAPES[D],) if D in BIG_SHAPES else ())
    for N, C in shapes:
        big = N >= 5000
        x = rounded(rs.rand(N, D), precision)
        c0 = rs.rand(C, D)
        w = rs.randint(1, 4, size=N).astype(np.float64)
        label = f"{np.dtype(precision).name} D={D} ({N}, {C})"
        with Ctx(x, precision) as ctx:
            first = ctx_kmeans(ctx, C, c0, w, maxit=1)
            check_one_iteration(first, x, w, c0, precision, label + " first", rows=np.arange(0, N, 16) if big else None)
            some = ctx_kmeans(ctx, C, c0, w, maxit=3)
            again = ctx_kmeans(ctx, C, some["centroids"], w, maxit=1)
            check_one_iteration(again, x, w, some["centroids"], precision, label + " fourth", rows=np.arange(0, N, 16) if big else None)
            if some["converged"]:
                assert some["shift"] == 0.0 and again["converged"] and again["shift"] == 0.0
            if not big:
                end = ctx_kmeans(ctx, C, c0, w, maxit=200)
                assert end["converged"] and end["shift"] == 0.0, label
                fixed = ctx_kmeans(ctx, C, end["centroids"], w, maxit=1)
                assert fixed["converged"] and fixed["shift"] == 0.0 and fixed["iterations"] == 1, label
                assert np.array_equal(fixed["centroids"], end["centroids"]) and np.array_equal(fixed["labels"], end["labels"]), label
                assert fixed["inertia"] == end["inertia"] and np.array_equal(fixed["cluster_weight"], end["cluster_weight"]), label
                check_one_iteration(fixed, x, w, end["centroids"], precision, label + " fixed point")
        if (N, C) == (300, 257):
            assert np.sum(first["cluster_weight"] == 0) > 50
            assert same_bits(plugin_kmeans(x, C, c0, precision, weights=w, maxit=3), some), label


# ---- 3. lattice ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [np.float64, np.float32, np.float16], ids=lambda p: np.dtype(p).name)
@pytest.mark.parametrize("D", [1, 3, 8])
def test_lattice_ties_and_empty_clusters(D, precision):
    """Small integers: every distance, every sum exact in every precision, so one iteration equals the restatement bit for
    bit.  Two identical initial centroids: every tie goes to the smaller index, the larger one stays empty and in place; a
    centroid at distance 100 stays empty and in place to the end of the run."""
    rs = np.random.RandomState(50 + D)
    x = kn.lattice(rs, 500, D)
    c0 = np.array([[2.0] * D, [6.0] * D, [10.0] * D, [14.0] * D, [6.0] * D, [100.0] * D])  # 4 == 1; 5 far away
    want = kr.kmeans(x, c0, tol=0.0, maxit=1, precision=precision)
    assert np.any(want["labels"] == 1) and not np.any(want["labels"] == 4) and not np.any(want["labels"] == 5)
    with Ctx(x, precision) as ctx:
        got = ctx_kmeans(ctx, 6, c0, maxit=1)
        end = ctx_kmeans(ctx, 6, c0, maxit=200)
    assert not got["converged"] and got["iterations"] == 1
    assert np.array_equal(got["labels"], want["labels"]) and np.array_equal(got["cluster_weight"], want["cluster_weight"])
    assert np.array_equal(got["centroids"], want["centroids"]) and got["inertia"] == want["inertia"]
    assert abs(got["shift"] - want["shift"]) <= 4 * EPS64 * want["shift"]
    assert np.array_equal(got["centroids"][4], c0[4]) and np.array_equal(got["centroids"][5], c0[5])
    assert got["cluster_weight"][4] == 0 and got["cluster_weight"][5] == 0
    assert end["converged"] and end["shift"] == 0.0 and not np.any(end["labels"] == 5)
    assert np.array_equal(end["centroids"][5], c0[5]) and end["cluster_weight"][5] == 0 and end["cluster_weight"].sum() == 500
    assert same_bits(plugin_kmeans(x, 6, c0, precision, maxit=1), got)


# ---- 4. chaining, reproducibility ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [np.float64, np.float32], ids=lambda p: np.dtype(p).name)
def test_chaining(precision):
    """k calls of maxit = 1, each fed the previous call's centroids, against one call of maxit = k: identical bits."""
    x = cloud(3, 0, 1000, precision)
    w = np.random.RandomState(3).rand(1000)
    for weights in (None, w):
        with Ctx(x, precision) as ctx:
            c = x[:7]
            for k in range(1, 5):
                one = ctx_kmeans(ctx, 7, c, weights, maxit=1)
                c = one["centroids"]
                whole = ctx_kmeans(ctx, 7, x[:7], weights, maxit=k)
                assert one["iterations"] == 1 and whole["iterations"] == k
                assert not one["converged"] and not whole["converged"] and one["shift"] > 0
                for key in ("centroids", "labels", "cluster_weight", "inertia", "shift"):
                    assert np.array_equal(one[key], whole[key]), (k, key)
    # a converged single call says so: the last step of a finished run
    with Ctx(x, precision) as ctx:
        end = ctx_kmeans(ctx, 7, x[:7], maxit=300)
        last = ctx_kmeans(ctx, 7, end["centroids"], maxit=1)
    assert end["converged"] and last["converged"] and last["iterations"] == 1 and last["shift"] == 0.0


@pytest.mark.parametrize("shape", [(3, 3000, 37), (3, 300, 257), (8, 5000, 2100)], ids=str)
def test_reproducible_and_independent_of_segments(shape):
    D, N, C = shape
    rs = np.random.RandomState(N)
    x, c0, w = rounded(rs.rand(N, D), np.float32), rs.rand(C, D), rs.rand(N)
    runs = []
    for options in ((), (), (("segments", 1),), (("segments", 3),), (("chunk", 64),)):
        with Ctx(x, np.float32, options=options) as ctx:
            runs.append(ctx_kmeans(ctx, C, c0, w, maxit=4))
            runs.append(ctx_kmeans(ctx, C, c0, w, maxit=4))  # and again on the same context
    assert all(same_bits(r, runs[0]) for r in runs[1:])
    assert same_bits(plugin_kmeans(x, C, c0, np.float32, weights=w, maxit=4, segments=3), runs[0])
    assert runs[0]["iterations"] == 4 and np.isfinite(runs[0]["inertia"])


# ---- 5. conventions and refusals -------------------------------------------------------------------------------------------
def test_a_nan_point_ends_the_solve():
    x = cloud(3, 0, 1000, np.float32)
    x[123, 1] = np.nan
    want = kr.kmeans(x, x[:7], tol=0.0, maxit=300, precision=np.float32)
    assert want["stop"] == kr.NONFINITE
    with Ctx(x, np.float32) as ctx:
        got = ctx_kmeans(ctx, 7, x[:7])
    assert not got["converged"] and got["iterations"] == 1 and got["labels"][123] == -1
    assert np.array_equal(got["labels"], want["labels"]) and np.all(np.delete(got["labels"], 123) >= 0)
    assert np.array_equal(got["cluster_weight"], want["cluster_weight"]) and got["cluster_weight"].sum() == 999
    assert np.all(np.isfinite(got["centroids"])) and np.isfinite(got["inertia"]) and np.isfinite(got["shift"])
    assert np.all(np.abs(got["centroids"] - want["centroids"]) <= centroid_tolerance(x, want["labels"], want["centroids"]))
    assert same_bits(plugin_kmeans(x, 7, x[:7], np.float32), got)
    # every distance overflows float32: the same end
    far = cloud(3, 1, 100, np.float32)
    far[5] = rounded(3e38, np.float32)
    want = kr.kmeans(far, far[:3], tol=0.0, maxit=300, precision=np.float32)
    with Ctx(far, np.float32) as ctx:
        got = ctx_kmeans(ctx, 3, far[:3])
    assert not got["converged"] and got["iterations"] == 1 and got["labels"][5] == -1
    assert np.array_equal(got["labels"], want["labels"]) and np.sum(got["labels"] < 0) == 1


def raw_kmeans(ctx, C, cent, weights=None, tol=0.0, maxit=10, null=()):
    """The entry point itself, every pointer spelled out; `null`: the outputs passed as NULL.  Returns (status, message)."""
    N = max(int(getattr(ctx, "N", 0)), 1)
    bufs = dict(centroids=cent, labels=np.empty(N, dtype=np.int64), cluster_weight=np.empty(max(C, 1)))
    iters, inertia, shift = ctypes.c_int(0), ctypes.c_double(0), ctypes.c_double(0)
    ptr = lambda name: None if name in null or bufs[name] is None else bufs[name].ctypes.data
    ref = lambda name, v: None if name in null else ctypes.byref(v)
    rc = ctx._lib.kmvp_kmeans(ctx._ctx, C, None if weights is None else weights.ctypes.data, tol, maxit, ptr("centroids"),
                              ptr("labels"), ptr("cluster_weight"), ref("iters", iters), ref("inertia", inertia),
                              ref("shift", shift))
    return rc, ctx._lib.kmvp_last_error(ctx._ctx).decode()


def test_invalid_arguments():
    x = cloud(3, 0, 200, np.float32)
    c0 = np.ascontiguousarray(x[:5])
    ctx = _lib.Context(0)
    try:
        rc, msg = raw_kmeans(ctx, 5, c0.copy())
        assert rc == INVALID and "kmvp_set_points has not been called" in msg
    finally:
        ctx.close()
    with Ctx(x, np.float32) as ctx:
        for kwargs in (dict(tol=-1e-9), dict(tol=float("nan")), dict(maxit=0), dict(null=("centroids",)), dict(null=("labels",)),
                       dict(null=("iters",)), dict(null=("inertia",)), dict(null=("shift",))):
            rc, msg = raw_kmeans(ctx, 5, c0.copy(), **kwargs)
            assert rc == INVALID and "bad k-means arguments" in msg, kwargs
        rc, msg = raw_kmeans(ctx, 0, c0.copy())
        assert rc == INVALID and "bad k-means arguments" in msg
        rc, msg = raw_kmeans(ctx, 5, c0.copy(), null=("cluster_weight",))  # optional
        assert rc in (0, NOT_CONVERGED)
        for bad in (np.nan, np.inf, -np.inf):
            c = c0.copy()
            c[3, 1] = bad
            rc, msg = raw_kmeans(ctx, 5, c)
            assert rc == INVALID and "initial centroid 3 is not finite" in msg
        for bad in (-1.0, np.nan, np.inf):
            w = np.ones(200)
            w[17] = bad
            rc, msg = raw_kmeans(ctx, 5, c0.copy(), weights=w)
            assert rc == INVALID and "weights[17] is negative or not finite" in msg
        with pytest.raises(ValueError):
            ctx.kmeans(5, c0[:4], None, 0.0, 10)
        with pytest.raises(ValueError):
            ctx.kmeans(5, c0, np.ones(199), 0.0, 10)
        with pytest.raises(_lib.KmvpError) as e:
            ctx.kmeans(5, c0, None, -1.0, 10)
        assert e.value.code == INVALID
    # no point at all: an empty target set next to a source cloud
    ctx = _lib.Context(0)
    try:
        ctx.set_points(np.ascontiguousarray(x, dtype=np.float32), np.empty((0, 3), dtype=np.float32), _lib.KMVP_F32)
        rc, msg = raw_kmeans(ctx, 5, c0.copy())
        assert rc == INVALID and "at least one point" in msg
    finally:
        ctx.close()
    with pytest.raises(ValueError):
        MI355XKMeans(n_clusters=0, dimension=3)
    with pytest.raises(ValueError):
        MI355XKMeans(n_clusters=3, dimension=3, init="farthest")
    with pytest.raises(ValueError):
        MI355XKMeans(n_clusters=3, dimension=3).prepare_data(points=x, weights=-np.ones(200))


def test_unsupported_configurations():
    x32 = np.ascontiguousarray(cloud(3, 0, 200, np.float32), dtype=np.float32)
    c0 = np.ascontiguousarray(x32[:5], dtype=np.float64)

    def refused(prepare, C=5, cent=None):
        ctx = _lib.Context(0)
        try:
            prepare(ctx)
            rc, msg = raw_kmeans(ctx, C, c0.copy() if cent is None else cent)
            return rc, msg
        finally:
            ctx.close()

    rc, msg = refused(lambda ctx: ctx.set_points(x32, None, _lib.KMVP_BF16))
    assert rc == UNSUPPORTED and "not for bfloat16" in msg
    x9 = np.ascontiguousarray(np.random.RandomState(0).rand(50, 9), dtype=np.float32)
    rc, msg = refused(lambda ctx: ctx.set_points(x9, None, _lib.KMVP_F32), C=2, cent=np.ascontiguousarray(x9[:2], dtype=np.float64))
    assert rc == UNSUPPORTED and "D = 9 is beyond" in msg
    for form in (1, 2, 3, 4):
        rc, msg = refused(lambda ctx: (ctx.set_option("fast_sqdists", form), ctx.set_points(x32, None, _lib.KMVP_F32)))
        assert rc == UNSUPPORTED and f"fast_sqdists = {form}" in msg
    for form in (-1, 0):
        rc, msg = refused(lambda ctx: (ctx.set_option("fast_sqdists", form), ctx.set_points(x32, None, _lib.KMVP_F32)))
        assert rc in (0, NOT_CONVERGED)
    rc, msg = refused(lambda ctx: (ctx.comm_init_host(lambda a, op: None, 0, 1), ctx.set_points(x32, None, _lib.KMVP_F32)))
    assert rc == UNSUPPORTED and "a communicator is attached" in msg
    rc, msg = refused(lambda ctx: ctx.set_points(x32[:150], x32, _lib.KMVP_F32, j_offset=0, M_total=200))
    assert rc == UNSUPPORTED and "the sources are a slice" in msg
    big = np.zeros((65537, 3))
    rc, msg = refused(lambda ctx: ctx.set_points(x32, None, _lib.KMVP_F32), C=65537, cent=big)
    assert rc == UNSUPPORTED and "C = 65537 is beyond" in msg


# ---- 6. no side effects, predict, initialisation ---------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [np.float64, np.float32], ids=lambda p: np.dtype(p).name)
def test_no_side_effects_on_the_context(precision):
    """A Gaussian product, its gradient and kmvp_nearest(K = 4) return the same bits before and after a k-means call on the
    same context, and the same as on a context that never saw one."""
    dtype, npdt = codes(precision)
    rs = np.random.RandomState(8)
    y, x, b = rounded(rs.rand(700, 3), precision), rounded(rs.rand(500, 3), precision), rounded(rs.randn(700, 2), precision)

    def others(ctx):
        ctx.run("gaussian", False)
        prod = ctx.get_result(500, 2)
        ctx.run_grad("gaussian")
        grad = ctx.get_result(500, 6)
        idx, sq = ctx.run_nearest(4, False)
        return prod, grad, idx, sq

    def fresh():
        ctx = _lib.Context(0)
        ctx.set_points(np.ascontiguousarray(y, dtype=npdt), np.ascontiguousarray(x, dtype=npdt), dtype)
        ctx.set_signal(np.ascontiguousarray(b, dtype=npdt))
        return ctx

    ctx = fresh()
    try:
        before = others(ctx)
        out = dict(zip(KEYS, ctx.kmeans(9, x[:9], None, 0.0, 50)))
        after = others(ctx)
        out2 = dict(zip(KEYS, ctx.kmeans(9, x[:9], None, 0.0, 50)))
        again = others(ctx)
    finally:
        ctx.close()
    ctx = fresh()
    try:
        alone = others(ctx)
    finally:
        ctx.close()
    for got in (after, again, alone):
        assert all(np.array_equal(g, w) for g, w in zip(got, before))
    assert np.isfinite(before[0]).all() and out["iterations"] > 1 and same_bits(out, out2)
    # the points of the solve were the TARGETS x, not the sources y
    assert out["labels"].shape == (500,) and out["cluster_weight"].sum() == 500
    with Ctx(x, precision) as ctx:
        assert same_bits(ctx_kmeans(ctx, 9, x[:9], maxit=50), out)


@pytest.mark.parametrize("precision", [np.float64, np.float32], ids=lambda p: np.dtype(p).name)
def test_predict_is_query_nearest_against_the_centroids(precision):
    rs = np.random.RandomState(21)
    x, fresh = rs.rand(2000, 3), rs.rand(777, 3)
    algo = MI355XKMeans(n_clusters=12, dimension=3, precision=precision, init="k-means++", seed=4)
    try:
        algo.prepare_data(points=x)
        algo.fit()
        algo.query()
        assert algo.get_additional()["converged"] and np.all(algo.get_cluster_weights() > 0)
        own, other = algo.predict(x), algo.predict(fresh)
        assert np.array_equal(own, algo.get_labels())  # shift == 0: every label is the nearest returned centroid
        cent = algo.get_centroids()
        warm = MI355XKMeans(n_clusters=12, dimension=3, precision=precision)
        try:
            warm.prepare_data(points=x)
            warm.query(init=cent)  # a warm start at the fixed point: one iteration, nothing moves
            assert warm.get_additional()["iterations"] == 1 and warm.get_additional()["converged"]
            assert np.array_equal(warm.get_centroids(), cent) and np.array_equal(warm.get_labels(), own)
        finally:
            warm.done()
    finally:
        algo.done()
    near = MI355XProduct(kernel="gaussian", dimension=3, precision=precision)
    try:
        near.prepare_data(source_points=cent.astype(kr.working(precision)), target_points=fresh, same_points=False)
        near.query_nearest(1)
        assert np.array_equal(other, near.get_nearest()[0][:, 0])
    finally:
        near.done()


def test_initialisations():
    """init="random": distinct points of the cloud, a function of the seed; init="k-means++": points of the cloud as well,
    spread out (a lower first inertia than the random draw's on clustered data, here by a wide margin)."""
    rs = np.random.RandomState(6)
    centres = rs.rand(8, 2) * 100
    x = np.repeat(centres, 250, axis=0) + rs.randn(2000, 2)
    first = {}
    for init in ("random", "k-means++"):
        algo = MI355XKMeans(n_clusters=8, dimension=2, precision=np.float64, init=init, seed=11, maxit=1)
        other = MI355XKMeans(n_clusters=8, dimension=2, precision=np.float64, init=init, seed=11, maxit=1)
        try:
            algo.prepare_data(points=x)
            other.prepare_data(points=x)
            c0 = algo._initial_centroids()
            assert np.array_equal(c0, other._initial_centroids())
            assert len({tuple(r) for r in c0}) == 8 and all((x == r).all(axis=1).any() for r in c0)
            algo.query()
            first[init] = algo.get_additional()["inertia"]
            algo.set_query_arguments(tol=0.0, maxit=100)
            algo.query()
            assert algo.get_additional()["converged"] and algo.get_additional()["inertia"] <= first[init]
        finally:
            algo.done()
            other.done()
    assert first["k-means++"] < first["random"]
