"""GPU tests of the radius search (include/kmvp.h kmvp_radius_nearest; lowd_cutoff_knn_kernel on the cell list of
csrc/kmvp_cutoff_plan.hpp with the lexicographic list of csrc/kmvp_radius_knn_list.hpp).

The contract is bitwise: a row equals the row of kmvp_nearest on the same context with every entry whose sqdist > r2
replaced by (-1, +inf), r2 formed in the working precision, whatever the cell factor.  No tolerance anywhere in this file.
The lattices have many exactly equal distances, and pairs exactly ON the boundary: there the walk order of the cell list
differs from the index order (tests/test_radius_nearest_reference.py asserts that it does), so the tie rule is exercised."""
import numpy as np
import pytest

import cutoff_reference as cr
import radius_nearest_reference as rn
from kernel_matrix_benchmarks_amd import _lib
from kernel_matrix_benchmarks_amd.algorithms.mi355x import MI355XProduct

pytestmark = pytest.mark.gpu

PREC = {"f32": np.float32, "f64": np.float64}
UNSUPPORTED, INVALID = 2, 1
KERNEL = "lowd_cutoff_knn_kernel"


def rounded(a, precision):
    return np.asarray(a, dtype=precision).astype(np.float64)


def bits(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def same(a, b):
    return bits(a[0], b[0]) and bits(a[1], b[1])


class Ctx:
    """One context on sources y (M, D) and targets x (N, D) -- None: the targets are the sources."""

    def __init__(self, y, x, precision):
        self.precision = np.float64 if np.dtype(precision) == np.float64 else np.float32
        self.dtype = _lib.KMVP_F64 if self.precision == np.float64 else _lib.KMVP_F32
        self.ctx = _lib.Context(0)
        try:
            self.ctx.set_points(np.ascontiguousarray(y, dtype=self.precision),
                                None if x is None else np.ascontiguousarray(x, dtype=self.precision), self.dtype)
        except Exception:
            self.ctx.close()
            raise

    def r2(self, R):
        """(real)(R R) as a float64."""
        return float(self.precision(R * R))

    def radius_nearest(self, R, K, exclude_self=False):
        idx, sq = self.ctx.radius_nearest(R, K, exclude_self)
        assert idx.shape == sq.shape == (self.ctx.N, K) and idx.dtype == np.int64 and sq.dtype == np.float64
        if self.ctx.N > 0:
            assert self.ctx.last_kernel_name == KERNEL and self.ctx.last_dispatch_note == ""
            assert self.ctx.last_kernel_ms > 0 and self.ctx.last_total_ms >= self.ctx.last_kernel_ms
        return idx, sq

    def masked_nearest(self, R, K, exclude_self=False):
        return rn.masked_nearest(*self.ctx.run_nearest(K, exclude_self), self.r2(R))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.close()


# ---- 1. equals the masked brute force, bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("prec", list(PREC))
@pytest.mark.parametrize("name", rn.CLOUDS)
def test_equals_the_masked_brute_force(name, prec):
    """K = 1, 3, 4, 5, 16, and with exclude_self (K = 15 in place of 16) where the targets are the sources, at the cell
    factors 1.0, 1.5, 2.0: kmvp_nearest's rows on the same context with the entries beyond r2 emptied, and hence the same
    arrays at the three factors.  B and K have rows with 0 - 1 and with fewer than 5 sources inside (the tails), every
    cloud rows with 17 or more (full lists): asserted."""
    precision = PREC[prec]
    y, x, R = rn.cloud(name, precision)
    cases = [(K, False) for K in (1, 3, 4, 5, 16)] + ([(K, True) for K in (1, 3, 4, 5, 15)] if x is None else [])
    with Ctx(y, x, precision) as ct:
        want = {c: ct.masked_nearest(R, *c) for c in cases}
        for factor in rn.FACTORS:
            ct.ctx.set_option("cutoff_cell_factor", factor)
            for c in cases:
                got = ct.radius_nearest(R, *c)
                assert same(got, want[c]), (factor, c, np.nonzero((got[0] != want[c][0]).any(axis=1))[0][:8])
        cnt = ct.ctx.radius_count(R)
    assert (cnt >= 17).any() and (want[(16, False)][0][:, -1] >= 0).any()
    if name in ("B", "K"):
        assert (cnt <= 1).sum() > 50 and (cnt < 5).sum() > 100 and (want[(5, False)][0][:, -1] < 0).any()


# ---- 2. integer brute force on the lattices ------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", list(PREC))
@pytest.mark.parametrize("name,bound", (("lattice", 25), ("lattice3", 9)))
def test_lattices_against_integer_arithmetic(name, bound, prec):
    """Independent of kmvp_nearest: s_int = the integer squared distance in units of 1 / 64, inside iff s_int <= bound, rows
    by lexsort on (index, s_int); sqdist == s_int / 64 exactly.  Many ties, and pairs exactly ON the boundary."""
    precision = PREC[prec]
    y, _, R = rn.cloud(name, precision)
    a = np.rint(y * 8).astype(np.int64)
    d = a[:, None, :] - a[None, :, :]
    s_int = (d * d).sum(axis=-1)
    assert (s_int == bound).any()
    with Ctx(y, None, precision) as ct:
        for factor in rn.FACTORS:
            ct.ctx.set_option("cutoff_cell_factor", factor)
            for K, ex in ((1, False), (4, False), (16, False), (15, True)):
                idx, sq = ct.radius_nearest(R, K, ex)
                for i in range(len(y)):
                    inside = np.nonzero(s_int[i] <= bound)[0]
                    if ex:
                        inside = inside[inside != i]    # one point per lattice site: the own pair is the only one at 0
                    order = inside[np.lexsort((inside, s_int[i, inside]))][:K]
                    n = len(order)
                    assert np.array_equal(idx[i, :n], order) and np.array_equal(sq[i, :n], s_int[i, order] / 64.0), (factor, K, ex, i)
                    assert np.all(idx[i, n:] == -1) and np.all(np.isposinf(sq[i, n:]))


# ---- 3. consistency with the count ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", list(PREC))
@pytest.mark.parametrize("name", ("A", "B", "K", "lattice3"))
def test_consistent_with_the_count(name, prec):
    """The number of entries with idx >= 0 in a row is min(K, kmvp_radius_count), with exclude_self on both sides."""
    precision = PREC[prec]
    y, x, R = rn.cloud(name, precision)
    with Ctx(y, x, precision) as ct:
        for ex in (False, True) if x is None else (False,):
            cnt = ct.ctx.radius_count(R, ex)
            for K in (1, 4, 7, 15):
                idx, sq = ct.radius_nearest(R, K, ex)
                assert np.array_equal((idx >= 0).sum(axis=1), np.minimum(K, cnt)), (K, ex)
                assert np.array_equal(idx >= 0, np.isfinite(sq)) and np.all(sq[:, 1:] >= sq[:, :-1])


# ---- 4. duplicates -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", list(PREC))
def test_duplicates_with_exclude_self(prec):
    """20 copies of one point among 300 others, exclude_self, K = 4 and 15: a copy's row holds the other copies in ascending
    index at distance 0, never its own index -- also for the copies whose index is above K + 1 others' (the own pair is then
    not among the K + 1 candidates and the last one is dropped)."""
    precision = PREC[prec]
    rs = np.random.RandomState(41)
    y = rounded(rs.rand(320, 3), precision)
    copies = np.sort(rs.choice(320, 20, replace=False))
    y[copies] = y[copies[0]]
    with Ctx(y, None, precision) as ct:
        for K in (4, 15):
            idx, sq = ct.radius_nearest(0.2, K, True)
            assert same((idx, sq), ct.masked_nearest(0.2, K, True))
            assert not (idx == np.arange(320)[:, None]).any()
            for i in copies:
                assert np.array_equal(idx[i], copies[copies != i][:K]) and np.all(sq[i] == 0), (K, i)


# ---- 5. non-finite coordinates ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", list(PREC))
def test_non_finite_coordinates(prec):
    """A NaN target: (-1, NaN) in all K entries.  An infinite target: (-1, +inf).  NaN and infinite sources never appear.
    None of them changes any other row by a bit.  M = 0 gives (-1, +inf) everywhere; N = 0 returns empty arrays."""
    precision = PREC[prec]
    rs = np.random.RandomState(17)
    yf, xf, R = rounded(rs.rand(300, 3), precision), rounded(rs.rand(150, 3), precision), 0.2
    bad_y = np.array([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [-np.inf, np.nan, 0.5]])
    at_y = [0, 100, 300]
    y = np.insert(yf, at_y, bad_y, axis=0)
    fy = np.isfinite(y).all(axis=1)
    bad_x = np.array([[0.5, np.nan, 0.5], [np.inf, 0.5, 0.5], [0.5, 0.5, -np.inf], [np.nan, np.inf, 0.5]])
    x = np.insert(xf, [0, 70, 70, 150], bad_x, axis=0)
    fx = np.isfinite(x).all(axis=1)
    nan_x = np.isnan(x).any(axis=1)
    orig = np.nonzero(fy)[0]                   # index in y of every finite source
    assert np.array_equal(y[fy], yf) and np.array_equal(x[fx], xf) and nan_x.sum() == 2 and (~fx).sum() == 4
    with Ctx(yf, xf, precision) as base, Ctx(y, x, precision) as ct:
        for K in (1, 4, 16):
            want_idx, want_sq = base.radius_nearest(R, K)
            idx, sq = ct.radius_nearest(R, K)
            assert same((idx, sq), ct.masked_nearest(R, K))
            assert bits(sq[fx], want_sq) and bits(idx[fx], np.where(want_idx >= 0, orig[np.maximum(want_idx, 0)], -1))
            assert np.all(idx[~fx] == -1) and np.all(np.isnan(sq[nan_x])) and np.all(np.isposinf(sq[~fx & ~nan_x]))
            assert not np.isin(idx, np.nonzero(~fy)[0]).any() and (idx[fx][:, 0] >= 0).any()
    with Ctx(y, None, precision) as ct:       # targets = sources with exclude_self
        idx, sq = ct.radius_nearest(R, 5, True)
        assert same((idx, sq), ct.masked_nearest(R, 5, True))
        assert np.all(idx[~fy] == -1) and not (idx == np.arange(len(y))[:, None]).any()
    with Ctx(np.zeros((0, 3)), x, precision) as ct:       # M = 0: no source at all, also for the NaN targets
        idx, sq = ct.radius_nearest(R, 3)
        assert np.all(idx == -1) and np.all(np.isposinf(sq)) and same((idx, sq), ct.masked_nearest(R, 3))
    with Ctx(yf, np.zeros((0, 3)), precision) as ct:      # N = 0
        idx, sq = ct.radius_nearest(R, 3)
        assert idx.shape == (0, 3) and sq.shape == (0, 3) and ct.ctx.cutoff_info()["records"] > 0


# ---- 6. shapes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", list(PREC))
@pytest.mark.parametrize("D", (1, 2, 3))
def test_shapes(D, prec):
    """N = 1, 63, 64, 65, 257 targets that are not the sources; a radius above the cloud's diameter (one cell, one run per
    tile: the plain kmvp_nearest, nothing masked); a radius with nothing inside."""
    precision = PREC[prec]
    rs = np.random.RandomState(50 + D)
    y = rounded(rs.rand(333, D), precision)
    R = (0.02, 0.12, 0.2)[D - 1]
    for N in (1, 63, 64, 65, 257):
        x = rounded(rs.rand(N, D), precision)
        with Ctx(y, x, precision) as ct:
            for K in (1, 4, 16):
                got = ct.radius_nearest(R, K)
                assert same(got, ct.masked_nearest(R, K)), (N, K)
            if N == 257:
                assert (got[0][:, 0] >= 0).any() and (got[0][:, -1] < 0).any()
                big = ct.radius_nearest(3.0, 16)
                assert same(big, ct.ctx.run_nearest(16)) and np.all(big[0] >= 0) and ct.ctx.cutoff_info()["cells"] == (1, 1, 1)
                assert ct.ctx.cutoff_info()["runs"] == ct.ctx.cutoff_info()["tiles"]
    with Ctx(y, 5.0 + rounded(rs.rand(70, D), precision), precision) as ct:      # nothing inside
        for K in (1, 5):
            idx, sq = ct.radius_nearest(0.5, K)
            assert np.all(idx == -1) and np.all(np.isposinf(sq))


# ---- 7. leaves no trace, shares the plan -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", list(PREC))
def test_leaves_no_trace_and_shares_the_plan(prec):
    precision = PREC[prec]
    y, x, R = rn.cloud("B", precision)
    b = rounded(np.random.RandomState(13).randn(len(y), 2), precision)

    def others(ct):
        ct.ctx.set_signal(np.ascontiguousarray(b, dtype=ct.precision))
        ct.ctx.run("gaussian", False)
        out = [ct.ctx.get_result(ct.ctx.N, 2)]
        ct.ctx.run_cutoff("matern-3/2", R, True)
        out.append(ct.ctx.get_result(ct.ctx.N, 2))
        out.append(ct.ctx.radius_count(R).astype(np.float64))
        idx, sq = ct.ctx.run_nearest(4)
        return out + [idx.astype(np.float64), sq]

    with Ctx(y, x, precision) as ct:
        before = others(ct)
        first = ct.radius_nearest(R, 5)
        ct.ctx.run("gaussian", False)            # the result of a product ...
        held = ct.ctx.get_result(ct.ctx.N, 2)
        again = ct.radius_nearest(R, 5)
        assert bits(ct.ctx.get_result(ct.ctx.N, 2), held)      # ... is still there: kmvp_get_result is not involved
        assert same(first, again)
        for a, c in zip(before, others(ct)):
            assert bits(a, c)
    with Ctx(y, x, precision) as ct:         # a count, then the search at the same R: one plan, the same tables
        ct.ctx.radius_count(R)
        info = ct.ctx.cutoff_info()
        got = ct.radius_nearest(R, 5)
        assert ct.ctx.cutoff_info() == info and same(got, first)
    with Ctx(y, x, precision) as ct:         # ... and the other way round, on a fresh context
        assert same(ct.radius_nearest(R, 5), first)
        info = ct.ctx.cutoff_info()
        ct.ctx.radius_count(R)
        assert ct.ctx.cutoff_info() == info


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------
def small_context(rs, D=3, dtype=_lib.KMVP_F32, comm=False, M_total=None, batches=False, same=True):
    ctx = _lib.Context(0)
    try:
        if comm:   # the rehearsal transport: a communicator of one rank without loading RCCL
            ctx.comm_init_host(lambda buf, op: None, 0, 1)
        y = np.ascontiguousarray(rs.rand(40, D), dtype=np.float32)
        ctx.set_points(y, None if same else np.ascontiguousarray(rs.rand(30, D), dtype=np.float32), dtype, 0, M_total)
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


NOT_BUILT = {"D4": (dict(D=4), "D = 4"), "bfloat16": (dict(D=16, dtype=_lib.KMVP_BF16), "bfloat16"),
             "communicator": (dict(comm=True), "communicator"), "source_slice": (dict(M_total=50), "M < M_total"),
             "batches": (dict(batches=True), "kmvp_set_batches")}


@pytest.mark.parametrize("case", list(NOT_BUILT))
def test_unsupported(case):
    kwargs, word = NOT_BUILT[case]
    ctx = small_context(np.random.RandomState(23), **kwargs)
    try:
        refused(ctx, lambda: ctx.radius_nearest(0.3, 3), UNSUPPORTED, "radius search", word)
    finally:
        ctx.close()


def test_invalid_and_k_beyond_the_lists():
    rs = np.random.RandomState(29)
    ctx = _lib.Context(0)
    try:
        refused(ctx, lambda: ctx.radius_nearest(0.3, 3), INVALID, "radius search", "kmvp_set_points")
    finally:
        ctx.close()
    ctx = small_context(rs)
    try:
        ctx.set_option("cutoff_cell_factor", 1.5)
        held = ctx.radius_nearest(0.3, 3, True)
        for radius in (0.0, -1.0, np.nan, np.inf, -np.inf):
            refused(ctx, lambda: ctx.radius_nearest(radius, 3), INVALID, "radius")
        for K in (0, -2):
            refused(ctx, lambda: ctx.radius_nearest(0.3, K), INVALID, "radius search", "K must be >= 1")
        refused(ctx, lambda: ctx.radius_nearest(0.3, 17), UNSUPPORTED, "radius search", "K = 17", "K <= 16")
        refused(ctx, lambda: ctx.radius_nearest(0.3, 16, True), UNSUPPORTED, "radius search", "K = 16 with exclude_self")
        out = np.empty((40, 3))
        code = ctx._lib.kmvp_radius_nearest(ctx._ctx, 0.3, 3, 0, None, out.ctypes.data)
        assert code == INVALID and "NULL" in ctx._lib.kmvp_last_error(ctx._ctx).decode()
        code = ctx._lib.kmvp_radius_nearest(ctx._ctx, 0.3, 3, 0, out.ctypes.data, None)
        assert code == INVALID and "NULL" in ctx._lib.kmvp_last_error(ctx._ctx).decode()
        # the settings and what ran before survive the refused calls
        assert ctx.cutoff_info()["cells"] != (1, 1, 1)
        assert same(ctx.radius_nearest(0.3, 3, True), held) and same(ctx.radius_nearest(0.3, 16), rn.masked_nearest(*ctx.run_nearest(16), float(np.float32(0.3 * 0.3))))
        assert same(ctx.radius_nearest(0.3, 15, True), rn.masked_nearest(*ctx.run_nearest(15, True), float(np.float32(0.3 * 0.3))))
    finally:
        ctx.close()
    ctx = small_context(rs, same=False)
    try:
        refused(ctx, lambda: ctx.radius_nearest(0.3, 3, True), INVALID, "radius search", "exclude_self")
        assert ctx.radius_nearest(0.3, 3)[0].shape == (30, 3)
    finally:
        ctx.close()


# ---- 9. the plugin ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", (np.float16, np.float32, np.float64), ids=lambda p: np.dtype(p).name)
def test_plugin(precision):
    """MI355XProduct.query_radius_nearest + get_nearest against the _lib call on the same (rounded) inputs, bit for bit;
    get_additional() carries the plan's info words; float16 is a float32 context of float16-rounded points."""
    rs = np.random.RandomState(31)
    y, x, R = rs.rand(500, 3), rs.rand(200, 3), 0.15
    work = np.float64 if np.dtype(precision) == np.float64 else np.float32
    yr, xr = rounded(y, precision), rounded(x, precision)
    algo = MI355XProduct(kernel="gaussian", dimension=3, precision=precision)
    try:
        algo.prepare_data(source_points=y, target_points=x, same_points=False)
        algo.query_radius_nearest(6, R)
        got, extra = algo.get_nearest(), algo.get_additional()
        assert extra["device_kernel"] == KERNEL and extra["cutoff_cells"][0] > 1 and extra["cutoff_walked"] > 0
        algo.query_nearest(6)
        assert same(got, rn.masked_nearest(*algo.get_nearest(), float(work(R * R))))
        with pytest.raises(ValueError):
            algo.query_radius_nearest(3, R, exclude_self=True)
        with pytest.raises(NotImplementedError):
            algo.query_radius_nearest(17, R)
    finally:
        algo.done()
    with Ctx(yr, xr, work) as ct:
        assert same(got, ct.radius_nearest(R, 6)) and (got[0][:, 0] >= 0).any() and (got[0][:, -1] < 0).any()
    algo = MI355XProduct(kernel="matern-3/2", dimension=3, precision=precision)
    try:
        algo.prepare_data(source_points=y, target_points=y, same_points=True)
        algo.query_radius_nearest(15, R, exclude_self=True)
        got = algo.get_nearest()
    finally:
        algo.done()
    with Ctx(yr, None, work) as ct:
        assert same(got, ct.radius_nearest(R, 15, True)) and not (got[0] == np.arange(500)[:, None]).any()
