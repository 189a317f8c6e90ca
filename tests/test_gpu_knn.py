"""GPU tests of the K-nearest-neighbour reduction (lowd_knn_kernel, include/kmvp.h kmvp_nearest) against the numpy
restatement of its definition (knn_reference.py, itself checked against a Python double loop in test_knn_reference.py).

On a lattice of small integers every difference, square and sum is exact in float16, float32 and float64, so indices AND
distances must equal the restatement bit for bit, ties included.  On continuous clouds the kernel's working-precision
distance differs from the true one by at most gamma = (D + 3) u relative (one rounding in x - y, counted twice by the
square, one per square, one per fma; u = 2^-24 for float32 / float16 inputs, 2^-53 for float64), and the four rules of
check_continuous() say what that allows; the true distance is taken in extended precision there.
"""
import json
import os

import numpy as np
import pytest

import knn_reference as kn
from kernel_matrix_benchmarks_amd import _lib
from kernel_matrix_benchmarks_amd.algorithms.mi355x import MI355XProduct
from test_gpu_multirank import _spawn

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

PRECISIONS = (np.float64, np.float32, np.float16)
SHAPES = ((1, 1), (63, 3), (65, 5), (300, 257))  # (N, M): one pair, below / above a 64-target tile, a ragged batch of sources
KS = (1, 3, 4, 5, 16)


def rounded(a, precision):
    return None if a is None else np.asarray(a, dtype=precision).astype(np.float64)


def codes(precision):
    """(kmvp_dtype, host dtype) of a context that computes on inputs of `precision` (float16: rounded, then float32)."""
    return (_lib.KMVP_F64, np.float64) if np.dtype(precision) == np.float64 else (_lib.KMVP_F32, np.float32)


class Ctx:
    """One context on one pair of clouds, through the C ABI's typed wrapper."""

    def __init__(self, y, x, precision, *, options=(), j_offset=0, M_total=None, comm=False):
        dtype, npdt = codes(precision)
        self.ctx = _lib.Context(0)
        try:
            if comm:
                self.ctx.comm_init(_lib.comm_unique_id(), 0, 1)
            for key, value in options:
                self.ctx.set_option(key, value)
            self.ctx.set_points(np.ascontiguousarray(rounded(y, precision), dtype=npdt),
                                None if x is None else np.ascontiguousarray(rounded(x, precision), dtype=npdt), dtype,
                                j_offset=j_offset, M_total=M_total)
        except Exception:
            self.ctx.close()
            raise

    def __enter__(self):
        return self.ctx

    def __exit__(self, *exc):
        self.ctx.close()


def ctx_nearest(ctx, K, exclude_self=False):
    idx, sq = ctx.run_nearest(K, exclude_self)
    assert idx.shape == sq.shape == (ctx.N, K) and idx.dtype == np.int64 and sq.dtype == np.float64
    if ctx.N > 0 and ctx.M > 0:
        assert ctx.last_kernel_name == "lowd_knn_kernel" and ctx.last_dispatch_note == ""
        assert ctx.last_kernel_ms > 0 and ctx.last_total_ms >= ctx.last_kernel_ms
    return idx, sq


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1], equal_nan=True)


# ---- 1. exact parity on a lattice -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS, ids=lambda p: np.dtype(p).name)
@pytest.mark.parametrize("D", [1, 3, 8])
def test_exact_parity_on_a_lattice(D, precision):
    """Every shape, targets == sources and !=, every K (1 / 4 / 16 are the list capacities, 3 and 5 sit inside one), through
    the plugin and through Context: indices and distances equal the restatement exactly.  (63, 3) and (65, 5) with K > M
    exercise the (-1, +inf) tail."""
    rs = np.random.RandomState(1000 + D)
    runs = 0
    for N, M in SHAPES:
        y, x_other = kn.lattice(rs, M, D), kn.lattice(rs, N, D)
        for x in (None, x_other):
            targets = y if x is None else x
            want = {K: kn.nearest(targets, y, K) for K in KS}
            with Ctx(y, x, precision) as ctx:
                for K in KS:
                    assert same(ctx_nearest(ctx, K), want[K]), ("Context", N, M, x is None, K)
                    runs += 1
            algo = MI355XProduct(kernel="gaussian", dimension=D, precision=precision)
            try:
                algo.prepare_data(source_points=y, target_points=targets, same_points=x is None)
                for K in KS:
                    algo.query_nearest(K)
                    got = algo.get_nearest()
                    extra = algo.get_additional()
                    assert extra["device_kernel"] == "lowd_knn_kernel" and extra["dispatch_note"] == "", extra
                    assert got[0].flags["C_CONTIGUOUS"] and got[1].flags["C_CONTIGUOUS"]
                    assert same(got, want[K]), ("plugin", N, M, x is None, K)
                    runs += 1
            finally:
                algo.done()
            if M < 16:
                assert np.all(want[16][0][:, M:] == -1) and np.all(np.isposinf(want[16][1][:, M:]))
    assert runs == len(SHAPES) * 2 * len(KS) * 2


# ---- 2. continuous clouds --------------------------------------------------------------------------------------------------
def check_continuous(idx, sq, x, y, K, gamma, label):
    """(a) every returned distance within gamma of the true one of the returned source; (b) rows non-decreasing, equal
    values in ascending index; (c) no source left out is nearer than the last returned one beyond gamma; (d) a row whose
    restatement has no two of its first K + 1 distances within 2 gamma s of each other has exactly the restatement's indices."""
    diff = np.asarray(x, dtype=np.longdouble)[:, None, :] - np.asarray(y, dtype=np.longdouble)[None, :, :]
    s_true = np.sum(diff * diff, axis=-1)  # extended precision: its own error is far below gamma, also for float64
    N, M = s_true.shape
    assert np.all(idx >= 0) and np.all(idx < M), label
    s_ret = np.take_along_axis(s_true, idx, axis=1)
    a = float(np.max(np.abs(sq - s_ret) / np.where(s_ret > 0, s_ret, 1.0)))
    a_zero = bool(np.all(sq[s_ret == 0] == 0))
    b = bool(np.all(np.diff(sq, axis=1) >= 0) and np.all((np.diff(sq, axis=1) > 0) | (np.diff(idx, axis=1) > 0)))
    out = np.ones((N, M), dtype=bool)
    np.put_along_axis(out, idx, False, axis=1)
    slack = (s_true * (1 + gamma) - sq[:, K - 1:K])[out]
    c = float(slack.min()) if slack.size else 0.0
    want_idx, want_sq = kn.nearest(x, y, K + 1)
    gaps = np.diff(want_sq, axis=1)
    separated = np.all(gaps > 2 * gamma * want_sq[:, 1:], axis=1)
    d = bool(np.array_equal(idx[separated], want_idx[separated, :K]))
    print(f"{label}: (a) max relative distance error {a:.3e} (gamma {gamma:.3e}); (b) ordered {b}; (c) smallest slack of a "
          f"source left out {c:.3e}; (d) {int(separated.sum())} of {N} rows separated, indices identical there: {d}; "
          f"{int((idx != want_idx[:, :K]).any(axis=1).sum())} rows differ from the restatement in all")
    assert a <= gamma and a_zero, (label, "a", a, gamma)
    assert b, (label, "b")
    assert c >= 0.0, (label, "c", c)
    assert d, (label, "d")


@pytest.mark.parametrize("precision", PRECISIONS, ids=lambda p: np.dtype(p).name)
@pytest.mark.parametrize("D", [1, 3, 8])
def test_continuous_clouds(D, precision):
    """Normal coordinates, N = 200 targets and M = 1000 sources, both near the origin and both offset by 100 (the
    difference form far from the origin, as the gradient tests check it), inputs rounded to the precision; K = 16 and 5."""
    u = 2.0 ** -53 if np.dtype(precision) == np.float64 else 2.0 ** -24
    gamma = (D + 3) * u
    rs = np.random.RandomState(2000 + D)
    for offset in (0.0, 100.0):
        y, x = rounded(rs.randn(1000, D) + offset, precision), rounded(rs.randn(200, D) + offset, precision)
        with Ctx(y, x, precision) as ctx:
            for K in (16, 5):
                idx, sq = ctx_nearest(ctx, K)
                check_continuous(idx, sq, x, y, K, gamma, f"D = {D} {np.dtype(precision).name} offset {offset:g} K = {K}")


# ---- 3. segments -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def segments_cloud():
    """N = 1000 targets in the middle of the lattice, M = 5001 sources all over it, ordered by their distance from the
    middle; the restatement once for both orders."""
    rs = np.random.RandomState(31)
    x = rs.randint(6, 10, size=(1000, 3)).astype(np.float64)
    y = kn.lattice(rs, 5001, 3)
    order = np.argsort(np.sum((y - 7.5) ** 2, axis=1), kind="stable")
    clouds = {"nearest-first": y[order], "nearest-last": y[order[::-1]]}
    return x, clouds, {name: kn.nearest(x, ys, 16) for name, ys in clouds.items()}


@pytest.mark.parametrize("precision", (np.float32, np.float64), ids=lambda p: np.dtype(p).name)
@pytest.mark.parametrize("order", ["nearest-last", "nearest-first"])
def test_segments_give_identical_bits(segments_cloud, order, precision):
    """K = 16 with 1, 3 and 8 source segments and the automatic choice: identical bits, equal to the restatement.  Nearest-
    last: the lists change throughout the loop; nearest-first: they are settled after the first tile."""
    x, clouds, want = segments_cloud
    for segments in (1, 3, 8, 0):
        with Ctx(clouds[order], x, precision, options=(("segments", segments),)) as ctx:
            assert same(ctx_nearest(ctx, 16), want[order]), (order, segments)


# ---- 4. exclude-self -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 15])
def test_exclude_self(K):
    """Same points on the lattice with one point repeated 20 times (more than K + 1): equal to the restatement, no row
    holds its own index; targets != sources: KMVP_E_INVALID."""
    rs = np.random.RandomState(41)
    y = kn.lattice(rs, 300, 3)
    y[100:120] = y[100]
    want = kn.nearest(y, y, K, exclude_self=True)
    for precision in PRECISIONS:
        with Ctx(y, None, precision) as ctx:
            got = ctx_nearest(ctx, K, exclude_self=True)
        assert same(got, want), (K, precision)
        assert not np.any(got[0] == np.arange(300)[:, None])
    algo = MI355XProduct(kernel="gaussian", dimension=3, precision=np.float32)
    try:
        algo.prepare_data(source_points=y, target_points=y, same_points=True)
        algo.query_nearest(K, exclude_self=True)
        assert same(algo.get_nearest(), want)
    finally:
        algo.done()
    with Ctx(y, y[:50] + 1.0, np.float32) as ctx:
        with pytest.raises(_lib.KmvpError) as e:
            ctx.run_nearest(K, True)
        assert e.value.code == 1 and "exclude_self" in str(e.value)


# ---- 5. conventions --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", (np.float32, np.float64), ids=lambda p: np.dtype(p).name)
def test_conventions(precision):
    """A NaN target row is (-1, NaN) and its neighbours are intact; a NaN source and a source at 3e38 (float32: its squared
    distance overflows; float64: merely the farthest) are never returned although K exceeds the number of sources; two runs
    give identical bits; M == 0 and N == 0."""
    rs = np.random.RandomState(51)
    x, y = kn.lattice(rs, 70, 3), kn.lattice(rs, 12, 3)
    y[3, 1] = np.nan
    y[7] = 3.0e38
    x[5, 2] = np.nan
    f32 = np.dtype(precision) == np.float32
    want = kn.nearest(x, y, 16, precision=precision)
    with Ctx(y, x, precision) as ctx:
        got = ctx_nearest(ctx, 16)
        again = ctx_nearest(ctx, 16)
        one = ctx_nearest(ctx, 1)
    assert same(got, want) and same(got, again) and same(one, (want[0][:, :1], want[1][:, :1]))
    assert np.all(got[0][5] == -1) and np.all(np.isnan(got[1][5]))
    others = np.delete(np.arange(70), 5)
    live = 10 if f32 else 11
    assert np.all(got[0][others, :live] >= 0) and np.all(np.isfinite(got[1][others, :live]))
    assert np.all(got[0][others, live:] == -1) and np.all(np.isposinf(got[1][others, live:]))
    assert not np.any(got[0] == 3) and np.any(got[0] == 7) == (not f32)
    # M == 0: nothing but the tail; N == 0: nothing written
    with Ctx(np.zeros((0, 3)), x, precision) as ctx:
        idx, sq = ctx_nearest(ctx, 4)
        assert np.all(idx == -1) and np.all(np.isposinf(sq)) and idx.shape == (70, 4) and ctx.last_kernel_name == "none"
    with Ctx(y, np.zeros((0, 3)), precision) as ctx:
        idx, sq = ctx_nearest(ctx, 4)
        assert idx.shape == (0, 4) and sq.shape == (0, 4)


def test_c_abi_refusals():
    """K = 17, K = 16 with exclude_self, a bfloat16 context, D = 9 and fast_sqdists = 1: KMVP_E_UNSUPPORTED with a message;
    K = 0, a NULL output and no points: KMVP_E_INVALID."""
    rs = np.random.RandomState(52)

    def refused(y, dtype, K, exclude_self=False, options=(), code=2):
        ctx = _lib.Context(0)
        try:
            for key, value in options:
                ctx.set_option(key, value)
            ctx.set_points(np.ascontiguousarray(y, dtype=np.float32), None, dtype)
            with pytest.raises(_lib.KmvpError) as e:
                ctx.run_nearest(K, exclude_self)
            msg = ctx._lib.kmvp_last_error(ctx._ctx).decode()
            assert e.value.code == code and msg and ctx.last_dispatch_note == "", (e.value.code, msg)
        finally:
            ctx.close()
        return msg

    assert "K = 17" in refused(rs.rand(64, 3), _lib.KMVP_F32, 17)
    assert "exclude_self" in refused(rs.rand(64, 3), _lib.KMVP_F32, 16, exclude_self=True)
    assert "bfloat16" in refused(rs.rand(64, 16), _lib.KMVP_BF16, 4)
    assert "D = 9" in refused(rs.rand(64, 9), _lib.KMVP_F32, 4)
    assert "fast_sqdists = 1" in refused(rs.rand(64, 3), _lib.KMVP_F32, 4, options=(("fast_sqdists", 1),))
    assert "K" in refused(rs.rand(64, 3), _lib.KMVP_F32, 0, code=1)
    ctx = _lib.Context(0)
    try:
        out = np.empty((64, 2), dtype=np.int64)
        assert ctx._lib.kmvp_nearest(ctx._ctx, 2, 0, out.ctypes.data, out.ctypes.data) == 1  # no points
        ctx.set_points(np.ascontiguousarray(rs.rand(64, 3), dtype=np.float32), None, _lib.KMVP_F32)
        assert ctx._lib.kmvp_nearest(ctx._ctx, 2, 0, None, None) == 1 and ctx._lib.kmvp_last_error(ctx._ctx)
    finally:
        ctx.close()
    with pytest.raises(NotImplementedError):
        algo = MI355XProduct(kernel="gaussian", dimension=16, precision="bfloat16")
        try:
            algo.prepare_data(source_points=rs.rand(64, 16), target_points=rs.rand(64, 16), same_points=True)
            algo.query_nearest(3)
        finally:
            algo.done()


# ---- 6. no side effects ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", (np.float32, np.float64), ids=lambda p: np.dtype(p).name)
def test_no_side_effects_on_other_calls(precision):
    """ONE context with a signal set: product, nearest, product, log-sum-exp, nearest, log-sum-exp.  The repeated results are
    bit-identical to the first ones, both nearest results are identical (and right)."""
    rs = np.random.RandomState(61)
    y, x, b = rs.rand(2001, 3) * 3.0, rs.rand(500, 3) * 3.0, rs.randn(2001, 2)
    _, npdt = codes(precision)
    with Ctx(y, x, precision) as ctx:
        ctx.set_signal(np.ascontiguousarray(b, dtype=npdt))
        ctx.run("gaussian", False)
        prod0 = ctx.get_result(500, 2)
        near0 = ctx_nearest(ctx, 5)
        ctx.run("gaussian", False)
        prod1 = ctx.get_result(500, 2)
        ctx.run_lse("gaussian")
        lse0 = ctx.get_result(500, 2)
        near1 = ctx_nearest(ctx, 5)
        ctx.run_lse("gaussian")
        lse1 = ctx.get_result(500, 2)
    assert np.array_equal(prod0, prod1) and np.array_equal(lse0, lse1) and same(near0, near1)
    assert np.isfinite(prod0).all() and np.isfinite(lse0).all()
    with Ctx(y, x, precision) as ctx:  # the same on a context that never saw another call
        assert same(ctx_nearest(ctx, 5), near0)


# ---- 7. shards -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exclude_self", [False, True])
def test_partial_shards_merge_on_the_host(exclude_self):
    """Two slices with partial_shard = 1 and their j_offset, merged by (sqdist, idx): the unsharded result, global indices."""
    rs = np.random.RandomState(71)
    y = kn.lattice(rs, 301, 3)
    x = None if exclude_self else kn.lattice(rs, 130, 3)
    targets = y if x is None else x
    K = 7
    with Ctx(y, x, np.float32) as ctx:
        whole = ctx_nearest(ctx, K, exclude_self)
    assert same(whole, kn.nearest(targets, y, K, exclude_self=exclude_self))
    parts = []
    for lo, hi in ((0, 120), (120, 301)):
        options = (("partial_shard", 1),) + ((("same_points_global", 1),) if exclude_self else ())
        with Ctx(y[lo:hi], targets, np.float32, options=options, j_offset=lo, M_total=301) as ctx:
            parts.append(ctx_nearest(ctx, K, exclude_self))
        assert same(parts[-1], kn.nearest(targets, y[lo:hi], K, exclude_self=exclude_self, j_offset=lo))
    assert parts[1][0].max() >= 120
    assert same(kn.merge_shards(parts, K), whole)
    with Ctx(y[:120], targets, np.float32, j_offset=0, M_total=301) as ctx:  # a slice without the option: refused
        with pytest.raises(_lib.KmvpError) as e:
            ctx.run_nearest(K, False)
        assert e.value.code == 1


def test_through_a_communicator_of_one_rank():
    """world == 1 takes the real exchange path (RCCL all-reduce of the one slot): the same bits as without it."""
    rs = np.random.RandomState(72)
    y, x = kn.lattice(rs, 257, 3), kn.lattice(rs, 65, 3)
    with Ctx(y, x, np.float32) as ctx:
        plain = ctx_nearest(ctx, 5)
    with Ctx(y, x, np.float32, comm=True) as ctx:
        through = ctx_nearest(ctx, 5)
        assert ctx.last_allreduce_ms >= 0
    assert same(plain, through) and same(plain, kn.nearest(x, y, 5))


def test_two_ranks_on_one_gpu():
    """The plugin with the sources sharded over two ranks through the host-staged exchange (kmvp_comm_init_host): uneven
    splits, a rank with an EMPTY slice, exclude_self with same_points_global; the worker holds every case to the
    restatement of the whole cloud on every rank, and the ranks to bitwise equal results."""
    out = _spawn([os.path.join(HERE, "_knn_rank_worker.py")], world=2, timeout=240)
    rep = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
    print(json.dumps(rep))
    assert rep["world"] == 2 and len(rep["cases"]) == 6 and rep["ranks_bitwise_equal"], rep
    assert sum(1 for case in rep["cases"] if case["empty_slice"]) == 2, rep
    assert sum(1 for case in rep["cases"] if case["exclude_self"]) == 2, rep
