"""GPU tests of the batched clouds (include/kmvp.h kmvp_set_batches; lowd_batch_kernel, lowd_batch_knn_kernel): B clouds
concatenated in one pair of arrays, every reduction restricted to a target's own batch.

The ragged batches combine the target sizes (0, 1, 63, 64, 65, 130) with the source sizes (300, 0, 1, 7, 8, 9), rotated
against each other (batch_reference.ragged_sizes).  The product is held, cloud by cloud, to the float64 model of the very
interact / kval code the kernel reuses (oracle/kmvp_lowd_model.py: path "lowd", the scalar-cache feed, the chunk of the
run), the nearest neighbours to the lattice restatement (knn_reference.py) and to the plain entry on a fresh context per
cloud -- no tolerance of this file's own."""
import numpy as np
import pytest

import batch_reference as br
import kmvp_lowd_model as lm
import knn_reference as kn
from kernel_matrix_benchmarks_amd import _lib
from kernel_matrix_benchmarks_amd.algorithms.mi355x import MI355XProduct
from test_gpu_knn import check_continuous

pytestmark = pytest.mark.gpu

KERNELS = ("gaussian", "absolute-exponential", "matern-3/2", "matern-5/2")
PREC = {"f32": np.float32, "f64": np.float64}
KS = (1, 3, 4, 5, 16)
UNSUPPORTED, INVALID = 2, 1


def codes(precision):
    """(kmvp_dtype, host dtype) of a context that computes on inputs of `precision` (float16: rounded, then float32)."""
    return (_lib.KMVP_F64, np.float64) if np.dtype(precision) == np.float64 else (_lib.KMVP_F32, np.float32)


def rounded(a, precision):
    return np.asarray(a, dtype=precision).astype(np.float64)


class Batched:
    """One context on the concatenation of per-cloud arrays ys[b] (m_b, D), xs[b] (n_b, D) -- xs None: the targets are the
    sources and the sources' offsets serve both -- with the batches set."""

    def __init__(self, ys, xs, precision, D, batches=True):
        self.dtype, self.npdt = codes(precision)
        self.precision = precision
        self.y_off = br.sizes_of(ys)
        self.x_off = self.y_off if xs is None else br.sizes_of(xs)
        self.ctx = _lib.Context(0)
        try:
            y = np.ascontiguousarray(rounded(br.concat(ys, D), precision), dtype=self.npdt)
            x = None if xs is None else np.ascontiguousarray(rounded(br.concat(xs, D), precision), dtype=self.npdt)
            self.ctx.set_points(y, x, self.dtype)
            if batches:
                self.on(explicit=xs is not None)
        except Exception:
            self.ctx.close()
            raise

    def on(self, explicit=True):
        self.ctx.set_batches(self.y_off, self.x_off if explicit else None)

    def off(self):
        self.ctx.set_batches(None)

    def product(self, kernel, normalise, bs, E, name="lowd_batch_kernel"):
        """bs: per-cloud signals (m_b, E), or None for density estimation.  (N, E) float64."""
        self.ctx.set_signal(None if bs is None else np.ascontiguousarray(rounded(br.concat(bs, E), self.precision), dtype=self.npdt))
        self.ctx.run(kernel, normalise)
        if name is not None and self.ctx.N > 0:
            assert self.ctx.last_kernel_name == name and self.ctx.last_dispatch_note == "", self.ctx.last_kernel_name
            assert self.ctx.last_kernel_ms > 0 and self.ctx.last_total_ms >= self.ctx.last_kernel_ms
        return self.ctx.get_result(self.ctx.N, 1 if bs is None else E)

    def nearest(self, K, name="lowd_batch_knn_kernel"):
        idx, sq = self.ctx.run_nearest(K)
        assert idx.shape == sq.shape == (self.ctx.N, K) and idx.dtype == np.int64 and sq.dtype == np.float64
        if name is not None and self.ctx.N > 0:
            assert self.ctx.last_kernel_name == name and self.ctx.last_dispatch_note == "", self.ctx.last_kernel_name
            assert self.ctx.last_kernel_ms > 0 and self.ctx.last_total_ms >= self.ctx.last_kernel_ms
        return idx, sq

    def rows(self, a, b):
        return a[self.x_off[b]:self.x_off[b + 1]]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.close()


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1], equal_nan=True)


def bits(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


# ---- 1. the model band ---------------------------------------------------------------------------------------------------
MODES = (("product", 1), ("product", 4), ("norm", 1), ("norm", 4), ("density", 1))
CHUNKS = (512, 8, 16)   # the default, and two at which the 300-source cloud folds 38 and 19 times
ORDER_OF_D = {1: 1, 3: 5, 8: 3}   # rotation of the source sizes against the target sizes: all three pair the 300 sources
                                  # with targets, two of them pair the empty source side with targets


def plain_empty_sources(x, kernel, sig, E, precision):
    """What the plain entry returns for these targets and M = 0 in this mode, from a plain call."""
    dtype, npdt = codes(precision)
    ctx = _lib.Context(0)
    try:
        ctx.set_points(np.zeros((0, x.shape[1]), dtype=npdt), np.ascontiguousarray(x, dtype=npdt), dtype)
        ctx.set_signal(None if sig == "density" else np.zeros((0, E), dtype=npdt))
        ctx.run(kernel, sig == "norm")
        return ctx.get_result(len(x), 1 if sig == "density" else E)
    finally:
        ctx.close()


@pytest.mark.parametrize("prec", list(PREC))
@pytest.mark.parametrize("kernel", KERNELS)
def test_model_band(kernel, prec):
    """Four kernels x product / normalised / density, E = 1 and 4, D = 1, 3, 8, the default chunk and chunk = 8, 16: every
    row of every cloud within the model's band of the model's value; the rows of a cloud without sources are the plain
    entry's M = 0 rows (read from run_product: zeros, NaN = 0 / 0 when normalised), bit for bit."""
    precision = PREC[prec]
    failures, checked, empty_checked = [], 0, 0
    for D, order in ORDER_OF_D.items():
        rs = np.random.RandomState(100 * D + len(kernel))
        xs, ys, bs4 = br.clouds(rs, D, 4, order, scale=1.5)
        with Batched(ys, xs, precision, D) as bt:
            for sig, E in MODES:
                bs = None if sig == "density" else [b[:, :E] for b in bs4]
                models = {}
                for chunk in CHUNKS:
                    bt.ctx.set_option("chunk", chunk)
                    got = bt.product(kernel, sig == "norm", bs, E)
                    assert got.shape == (bt.ctx.N, E)
                    for b in range(len(xs)):
                        rows = bt.rows(got, b)
                        if len(xs[b]) == 0:
                            continue
                        if len(ys[b]) == 0:
                            want = plain_empty_sources(rounded(xs[b], precision), kernel, sig, E, precision)
                            assert bits(rows, want), (D, sig, E, chunk, b)
                            assert np.all(np.isnan(want)) if sig == "norm" else np.all(want == 0)
                            empty_checked += 1
                            continue
                        key = (b, lm.chain_length("lowd", precision, len(ys[b]), chunk, 0))
                        if key not in models:
                            models[key] = lm.lowd_product(kernel, ys[b], xs[b], None if bs is None else bs[b], sig == "norm",
                                                          precision=precision, path="lowd", feed=0, chunk=chunk)
                        m = models[key]
                        assert not m.nonfinite.any() and not m.flagged.any()
                        err = np.abs(rows - m.value)
                        checked += rows.size
                        if not (np.isfinite(rows).all() and (err <= m.band).all()):
                            with np.errstate(divide="ignore", invalid="ignore"):
                                failures.append((D, sig, E, chunk, b, float(np.nanmax(err / m.band))))
    print(f"\nbatched model band {kernel} {prec}: {checked} elements inside the band, {empty_checked} empty-source clouds, "
          f"{len(failures)} failures")
    assert not failures, (len(failures), failures[:8])
    assert checked > 0 and empty_checked > 0


@pytest.mark.parametrize("prec", list(PREC))
def test_normalised_density(prec):
    """Normalised density estimation: ones, NaN (0 / 0) in a cloud without sources -- the plain entry's two answers."""
    rs = np.random.RandomState(3)
    xs, ys, _ = br.clouds(rs, 3, 1, 5)
    with Batched(ys, xs, PREC[prec], 3) as bt:
        got = bt.product("gaussian", True, None, 1, name=None)
        assert bt.ctx.last_kernel_name == "fill_kernel" and bt.ctx.last_kernel_ms == 0   # no pair loop, as the plain entry
        for b in range(len(xs)):
            rows = bt.rows(got, b)
            assert np.all(np.isnan(rows)) if len(ys[b]) == 0 else np.all(rows == 1.0)


# ---- 2. isolation --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", list(PREC))
def test_isolation(prec):
    """Every other cloud's signal at 1e30 and a NaN and an inf coordinate among the other clouds' sources: the rows of cloud
    b do not change by a bit, in the product, the normalised product and the nearest neighbours.  A NaN target coordinate
    makes its own row NaN and no other."""
    precision, D, E = PREC[prec], 3, 2
    rs = np.random.RandomState(11)
    xs, ys, bs = br.clouds(rs, D, E, 1)
    with Batched(ys, xs, precision, D) as bt:
        base = [bt.product("gaussian", False, bs, E), bt.product("absolute-exponential", True, bs, E)]
        base_near = bt.nearest(4)
    tested = 0
    for b in range(len(xs)):
        if len(xs[b]) == 0:
            continue
        ys2 = [y.copy() for y in ys]
        bs2 = [sb.copy() for sb in bs]
        for o in range(len(xs)):
            if o != b and len(ys[o]):
                bs2[o][:] = 1e30
                ys2[o][0, 0] = np.nan
                ys2[o][-1, D - 1] = np.inf
        with Batched(ys2, xs, precision, D) as bt:
            got = [bt.product("gaussian", False, bs2, E), bt.product("absolute-exponential", True, bs2, E)]
            near = bt.nearest(4)
            for g, w in zip(got, base):
                assert bits(bt.rows(g, b), bt.rows(w, b)), b
            assert same((bt.rows(near[0], b), bt.rows(near[1], b)), (bt.rows(base_near[0], b), bt.rows(base_near[1], b))), b
            tested += 1
    assert tested == 5
    # a NaN target coordinate: target 40 of the 130-target cloud (300 sources)
    xs2 = [x.copy() for x in xs]
    xs2[5][40, 1] = np.nan
    with Batched(ys, xs2, precision, D) as bt:
        got = [bt.product("gaussian", False, bs, E), bt.product("absolute-exponential", True, bs, E)]
        near = bt.nearest(4)
        r = int(bt.x_off[5]) + 40
        keep = np.arange(bt.ctx.N) != r
        for g, w in zip(got, base):
            assert np.all(np.isnan(g[r])) and bits(g[keep], w[keep])
        assert np.all(near[0][r] == -1) and np.all(np.isnan(near[1][r]))
        assert same((near[0][keep], near[1][keep]), (base_near[0][keep], base_near[1][keep]))


# ---- 3. independence of company and position ----------------------------------------------------------------------------
@pytest.mark.parametrize("prec", list(PREC))
def test_independent_of_company_and_position(prec):
    """Cloud b's rows from the ragged batch equal, bit for bit, the rows of a kmvp_set_batches call with B = 1 on cloud b
    alone, and the rows from the same clouds in reversed order; run to run they are bitwise equal."""
    precision, D, E = PREC[prec], 3, 3
    rs = np.random.RandomState(21)
    xs, ys, bs = br.clouds(rs, D, E, 5)
    B = len(xs)

    def run(bt):
        return [bt.product("gaussian", False, bs_of[bt], E), bt.product("matern-3/2", True, bs_of[bt], E),
                bt.product("absolute-exponential", False, None, 1)], bt.nearest(5)

    bs_of = {}
    with Batched(ys, xs, precision, D) as bt:
        bs_of[bt] = bs
        prods, near = run(bt)
        prods2, near2 = run(bt)
        assert all(bits(a, b) for a, b in zip(prods, prods2)) and same(near, near2)      # run to run
        x_off, y_off = bt.x_off, bt.y_off
    with Batched(ys[::-1], xs[::-1], precision, D) as rev:
        bs_of[rev] = bs[::-1]
        rprods, rnear = run(rev)
        for b in range(B):
            rb = B - 1 - b
            for a, r in zip(prods, rprods):
                assert bits(a[x_off[b]:x_off[b + 1]], rev.rows(r, rb)), ("reversed", b)
            idx, ridx = near[0][x_off[b]:x_off[b + 1]], rev.rows(rnear[0], rb)
            assert np.array_equal(np.where(idx >= 0, idx - y_off[b], -1), np.where(ridx >= 0, ridx - rev.y_off[rb], -1))
            assert np.array_equal(near[1][x_off[b]:x_off[b + 1]], rev.rows(rnear[1], rb), equal_nan=True)
    for b in range(B):
        if len(xs[b]) == 0:
            continue
        with Batched([ys[b]], [xs[b]], precision, D) as one:      # B = 1 on cloud b alone
            bs_of[one] = [bs[b]]
            oprods, onear = run(one)
            for a, o in zip(prods, oprods):
                assert bits(a[x_off[b]:x_off[b + 1]], o), ("alone", b)
            idx = near[0][x_off[b]:x_off[b + 1]]
            assert np.array_equal(np.where(idx >= 0, idx - y_off[b], -1), onear[0])
            assert np.array_equal(near[1][x_off[b]:x_off[b + 1]], onear[1], equal_nan=True)


# ---- 4. nearest neighbours, exact -----------------------------------------------------------------------------------------
def plain_nearest(y, x, K, precision):
    dtype, npdt = codes(precision)
    ctx = _lib.Context(0)
    try:
        ctx.set_points(np.ascontiguousarray(y, dtype=npdt), np.ascontiguousarray(x, dtype=npdt), dtype)
        return ctx.run_nearest(K)
    finally:
        ctx.close()


@pytest.mark.parametrize("precision", (np.float64, np.float32, np.float16), ids=lambda p: np.dtype(p).name)
@pytest.mark.parametrize("D", [1, 3, 8])
def test_nearest_exact_on_a_lattice(D, precision):
    """Lattice clouds (ties by the hundred), every K: indices and distances equal the restatement of every cloud with its
    offset, ties included; the tails are (-1, +inf) where m_b < K and in the cloud without sources; and all of it equals,
    bit for bit, the plain kmvp_nearest on a fresh context per cloud with the offset added."""
    rs = np.random.RandomState(4000 + D)
    xs, ys, _ = br.clouds(rs, D, 1, ORDER_OF_D[D], points=kn.lattice)
    work = np.float64 if np.dtype(precision) == np.float64 else np.float32
    tails = 0
    with Batched(ys, xs, precision, D) as bt:
        for K in KS:
            idx, sq = bt.nearest(K)
            for b in range(len(xs)):
                if len(xs[b]) == 0:
                    continue
                got = (bt.rows(idx, b), bt.rows(sq, b))
                want = kn.nearest(xs[b], ys[b], K, j_offset=int(bt.y_off[b]), precision=work)
                assert same(got, want), (K, b, "restatement")
                m = len(ys[b])
                if m < K:
                    assert np.all(got[0][:, m:] == -1) and np.all(np.isposinf(got[1][:, m:]))
                    tails += 1
                pidx, psq = plain_nearest(rounded(ys[b], precision), rounded(xs[b], precision), K, precision)
                assert same(got, (np.where(pidx >= 0, pidx + bt.y_off[b], -1), psq)), (K, b, "plain entry")
    assert tails > 0


@pytest.mark.parametrize("precision", (np.float64, np.float32), ids=lambda p: np.dtype(p).name)
def test_nearest_same_points_and_null_target_offsets(precision):
    """The targets are the sources and x_offsets is NULL: the sources' offsets serve both."""
    rs = np.random.RandomState(41)
    ys = [kn.lattice(rs, m, 3) for m in br.SOURCE_SIZES]
    with Batched(ys, None, precision, 3) as bt:
        for K in (1, 5):
            idx, sq = bt.nearest(K)
            for b in range(len(ys)):
                want = kn.nearest(ys[b], ys[b], K, j_offset=int(bt.y_off[b]))
                assert same((bt.rows(idx, b), bt.rows(sq, b)), want), (K, b)
        bsig = [rs.randn(len(y), 2) for y in ys]
        got = bt.product("gaussian", False, bsig, 2)
    with Batched(ys, ys, precision, 3) as bt:       # the same with explicit targets and offsets
        assert bits(got, bt.product("gaussian", False, bsig, 2))


@pytest.mark.parametrize("precision", (np.float64, np.float32), ids=lambda p: np.dtype(p).name)
def test_nearest_on_continuous_clouds(precision):
    """Normal coordinates offset by 100: the four rules of the plain entry's continuous test, cloud by cloud."""
    D = 3
    gamma = (D + 3) * (2.0 ** -53 if np.dtype(precision) == np.float64 else 2.0 ** -24)
    rs = np.random.RandomState(43)
    sizes = ((130, 300), (65, 40), (64, 1000))
    xs = [rounded(rs.randn(n, D) + 100.0, precision) for n, _ in sizes]
    ys = [rounded(rs.randn(m, D) + 100.0, precision) for _, m in sizes]
    with Batched(ys, xs, precision, D) as bt:
        for K in (16, 5, 1):
            idx, sq = bt.nearest(K)
            for b in range(len(xs)):
                check_continuous(bt.rows(idx, b) - bt.y_off[b], bt.rows(sq, b), xs[b], ys[b], K, gamma,
                                 f"batched {np.dtype(precision).name} cloud {b} K = {K}")


# ---- 5. the plain paths are untouched ------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", (np.float32, np.float64), ids=lambda p: np.dtype(p).name)
def test_plain_paths_untouched(precision):
    """Product, normalised product, kmvp_nearest, gradient and log-sum-exp on ONE context before kmvp_set_batches, between a
    batched product and a batched nearest (batches switched off), and after: bitwise equal.  kmvp_set_points clears the
    batches."""
    rs = np.random.RandomState(51)
    D, E = 3, 2
    xs, ys, bs = br.clouds(rs, D, E, 1, scale=2.0)
    _, npdt = codes(precision)

    def capture(bt):
        ctx = bt.ctx
        ctx.set_signal(np.ascontiguousarray(br.concat(bs, E), dtype=npdt))
        out = []
        for normalise in (False, True):
            ctx.run("gaussian", normalise)
            assert "batch" not in ctx.last_kernel_name
            out.append(ctx.get_result(ctx.N, E))
        idx, sq = ctx.run_nearest(5)
        assert ctx.last_kernel_name == "lowd_knn_kernel"
        out += [idx.astype(np.float64), sq]
        ctx.run_grad("gaussian")
        out.append(ctx.get_result(ctx.N, E * D))
        ctx.run_lse("gaussian")
        out.append(ctx.get_result(ctx.N, E))
        return out

    with Batched(ys, xs, precision, D, batches=False) as bt:
        before = capture(bt)
        bt.on()
        batched = bt.product("gaussian", False, bs, E)
        bt.off()
        between = capture(bt)
        bt.on()
        bt.nearest(5)
        assert bits(batched, bt.product("gaussian", False, bs, E))
        bt.off()
        after = capture(bt)
        assert not bits(batched, before[0])        # (the block-diagonal product is another thing than the full one)
        for a, b, c in zip(before, between, after):
            assert bits(a, b) and bits(a, c)
        # kmvp_set_points clears the batches
        bt.on()
        y = np.ascontiguousarray(br.concat(ys, D), dtype=npdt)
        x = np.ascontiguousarray(br.concat(xs, D), dtype=npdt)
        bt.ctx.set_points(y, x, bt.dtype)
        again = capture(bt)
        for a, b in zip(before, again):
            assert bits(a, b)
    with Batched(ys, xs, precision, D, batches=False) as fresh:    # a context that never saw a batch
        for a, b in zip(before, capture(fresh)):
            assert bits(a, b)


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------
def raw_set_batches(ctx, B, y_off, x_off):
    y = None if y_off is None else np.ascontiguousarray(y_off, dtype=np.int64)
    x = None if x_off is None else np.ascontiguousarray(x_off, dtype=np.int64)
    rc = ctx._lib.kmvp_set_batches(ctx._ctx, B, None if y is None else y.ctypes.data, None if x is None else x.ctypes.data)
    return rc, ctx._lib.kmvp_last_error(ctx._ctx).decode()


def test_set_batches_refusals():
    """Every KMVP_E_INVALID case of kmvp_set_batches, each with its message; a refused call leaves the previous setting,
    proved by running a product."""
    rs = np.random.RandomState(61)
    ctx = _lib.Context(0)
    try:
        rc, msg = raw_set_batches(ctx, 1, [0, 4], [0, 4])
        assert rc == INVALID and "kmvp_set_points" in msg                                   # no points set
        y, x = rs.rand(40, 3).astype(np.float32), rs.rand(30, 3).astype(np.float32)
        b = rs.randn(40, 1).astype(np.float32)
        ctx.set_points(y, x, _lib.KMVP_F32)
        ctx.set_signal(b)
        good = ([0, 10, 40], [0, 25, 30])
        rc, msg = raw_set_batches(ctx, 2, *good)
        assert rc == 0
        ctx.run("gaussian", False)
        want = ctx.get_result(30, 1)
        for B, yo, xo, word in ((-1, good[0], good[1], "B"), (2, None, good[1], "y_offsets"), (2, good[0], None, "x_offsets"),
                                (2, [1, 10, 40], good[1], "start at 0"), (2, [0, 30, 20], [0, 25, 30], "monotone"),
                                (2, [0, 10, 39], good[1], "M = 40"), (2, good[0], [0, 25, 31], "N = 30"),
                                (2, good[0], [0, 26, 25], "monotone"), (0, good[0], None, "B = 0")):
            rc, msg = raw_set_batches(ctx, B, yo, xo)
            assert rc == INVALID and word in msg and "batches" in msg, (B, yo, xo, rc, msg)
            ctx.run("gaussian", False)                                                       # the previous setting holds
            assert ctx.last_kernel_name == "lowd_batch_kernel" and bits(ctx.get_result(30, 1), want)
        rc, _ = raw_set_batches(ctx, 0, None, None)
        assert rc == 0
        ctx.run("gaussian", False)
        assert ctx.last_kernel_name != "lowd_batch_kernel"
        # a NULL x_offsets is fine when the targets are the sources
        ctx.set_points(y, None, _lib.KMVP_F32)
        rc, _ = raw_set_batches(ctx, 2, good[0], None)
        assert rc == 0
        with pytest.raises(ValueError):
            ctx.set_batches(np.array([[0, 40]]))
        with pytest.raises(ValueError):
            ctx.set_batches(np.array([0.0, 40.0]))
        with pytest.raises(ValueError):
            ctx.set_batches([0, 10, 40], [0, 40])
    finally:
        ctx.close()


def batched_context(rs, D=3, dtype=_lib.KMVP_F32, E=1, options=(), comm=False, M_total=None):
    """A float32 (bfloat16: float32 on the host) context on 40 points that are their own targets, two batches set."""
    ctx = _lib.Context(0)
    try:
        if comm:   # the rehearsal transport: a communicator of one rank without loading RCCL
            ctx.comm_init_host(lambda buf, op: None, 0, 1)
        for key, value in options:
            ctx.set_option(key, value)
        ctx.set_points(np.ascontiguousarray(rs.rand(40, D), dtype=np.float32), None, dtype, 0, M_total)
        ctx.set_signal(np.ascontiguousarray(rs.randn(40, E), dtype=np.float32))
        ctx.set_batches([0, 10, 40])
    except Exception:
        ctx.close()
        raise
    return ctx


def refused(ctx, call, *words):
    """KMVP_E_UNSUPPORTED with a message that names the batches and every one of `words`."""
    with pytest.raises(_lib.KmvpError) as e:
        call()
    msg = ctx._lib.kmvp_last_error(ctx._ctx).decode()
    assert e.value.code == UNSUPPORTED and "batch" in msg, (e.value.code, msg)
    for w in words:
        assert w in msg, (w, msg)


def test_unsupported_while_batches_are_set():
    """Every entry that is not built for the batches answers KMVP_E_UNSUPPORTED with a message that names them."""
    rs = np.random.RandomState(62)
    ctx = batched_context(rs)
    try:
        a = np.ascontiguousarray(rs.randn(40, 1), dtype=np.float32)
        refused(ctx, lambda: ctx.run("inverse-distance", False), "inverse-distance")
        refused(ctx, lambda: ctx.run("inverse-distance", True), "inverse-distance")
        refused(ctx, lambda: ctx.run("exp-dot", False), "exp(<x,y>)")
        refused(ctx, lambda: ctx.run("exp-dot", True), "exp(<x,y>)")
        for kernel in ("gaussian", "absolute-exponential", "inverse-distance", "matern-3/2", "matern-5/2"):
            refused(ctx, lambda: ctx.run_grad(kernel), "gradient")
        for kernel in ("gaussian", "absolute-exponential", "matern-3/2", "matern-5/2"):
            refused(ctx, lambda: ctx.run_dscale(kernel), "length-scale")
            refused(ctx, lambda: ctx.cg_solve(kernel, a, 1e-6, 10), "solver")
            refused(ctx, lambda: ctx.lanczos_quadrature(kernel, a, 1e-6, 10), "quadrature")
            refused(ctx, lambda: ctx.lanczos_quadrature_precond(kernel, a.astype(np.float64), np.zeros((1, 1)), 1e-6, 10), "quadrature")
        refused(ctx, lambda: ctx.cg_solve("inverse-distance", a, 1e-6, 10), "solver")
        for kernel in ("gaussian", "absolute-exponential"):
            refused(ctx, lambda: ctx.run_lse(kernel), "log-sum-exp")
            refused(ctx, lambda: ctx.run_lse_grad(kernel), "log-sum-exp")
            refused(ctx, lambda: ctx.sinkhorn(kernel, None, None, 1e-6, 10), "Sinkhorn")
        refused(ctx, lambda: ctx.kmeans(2, rs.rand(2, 3), None, 0.0, 5), "k-means")
        refused(ctx, lambda: ctx.meanshift(1e-4, 5), "mean-shift")
        refused(ctx, lambda: ctx.run_nearest(3, True), "exclude_self")
        ctx.run("gaussian", False)          # ... and what is built still runs
        ctx.run_nearest(3)
    finally:
        ctx.close()
    assert _lib.load().kmvp_abi_version() == 1


SHAPES_NOT_BUILT = {"D9": (dict(D=9), "D = 9"), "E5": (dict(E=5), "E = 5"), "fast_sqdists": (dict(options=(("fast_sqdists", 1),)), "fast_sqdists = 1"),
                    "bfloat16": (dict(D=16, dtype=_lib.KMVP_BF16), "bfloat16"), "communicator": (dict(comm=True), "communicator"),
                    "source_slice": (dict(M_total=50), "M < M_total")}


@pytest.mark.parametrize("case", list(SHAPES_NOT_BUILT))
def test_products_and_nearest_refuse_what_they_are_not_built_for(case):
    """D > 8, E > 4, an explicit fast_sqdists, a bfloat16 context, an attached communicator and a source slice: the batched
    products and kmvp_nearest answer KMVP_E_UNSUPPORTED with a message that names the batches and the reason."""
    kwargs, word = SHAPES_NOT_BUILT[case]
    ctx = batched_context(np.random.RandomState(63), **kwargs)
    try:
        refused(ctx, lambda: ctx.run("gaussian", False), word)
        refused(ctx, lambda: ctx.run("matern-5/2", True), word)
        if "E" not in kwargs:
            refused(ctx, lambda: ctx.run_nearest(3), word)
        assert ctx.last_dispatch_note == ""
    finally:
        ctx.close()


# ---- 7. the plugin ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", (np.float16, np.float32, np.float64), ids=lambda p: np.dtype(p).name)
def test_plugin(precision):
    """The ragged case through MI355XProduct: query() and query_nearest() on top of source_batches / target_batches, the
    result's contiguity and device_kernel, and the ValueErrors the host decides."""
    D, E = 3, 2
    rs = np.random.RandomState(71)
    xs, ys, bs = br.clouds(rs, D, E, 5, points=kn.lattice)
    ys = [y / 8.0 for y in ys]       # (exact in float16; distances small enough for the Gaussian to be well above 0)
    xs = [x / 8.0 for x in xs]
    y, x, b = br.concat(ys, D), br.concat(xs, D), br.concat(bs, E)
    y_off, x_off = br.sizes_of(ys), br.sizes_of(xs)
    work = np.float64 if np.dtype(precision) == np.float64 else np.float32
    algo = MI355XProduct(kernel="gaussian", dimension=D, precision=precision)
    try:
        algo.prepare_data(source_points=y, target_points=x, same_points=False, source_batches=y_off, target_batches=x_off)
        algo.fit()
        algo.prepare_query(source_signal=b)
        algo.query()
        got = algo.get_result()
        extra = algo.get_additional()
        assert extra["device_kernel"] == "lowd_batch_kernel" and extra["dispatch_note"] == "", extra
        assert got.shape == (len(x), E) and got.flags["C_CONTIGUOUS"] and got.dtype == np.float64
        for bi in range(len(xs)):
            rows = got[x_off[bi]:x_off[bi + 1]]
            if len(xs[bi]) == 0:
                continue
            if len(ys[bi]) == 0:
                assert np.all(rows == 0)
                continue
            m = lm.lowd_product("gaussian", rounded(ys[bi], precision), rounded(xs[bi], precision), rounded(bs[bi], precision),
                                False, precision=work, path="lowd", feed=0, chunk=512)
            assert (np.abs(rows - m.value) <= m.band).all(), bi
        algo.query_nearest(5)
        idx, sq = algo.get_nearest()
        assert algo.get_additional()["device_kernel"] == "lowd_batch_knn_kernel"
        assert idx.flags["C_CONTIGUOUS"] and sq.flags["C_CONTIGUOUS"]
        for bi in range(len(xs)):
            want = kn.nearest(xs[bi], ys[bi], 5, j_offset=int(y_off[bi]), precision=work)
            assert same((idx[x_off[bi]:x_off[bi + 1]], sq[x_off[bi]:x_off[bi + 1]]), want), bi
        for method in (algo.query_gradient, algo.query_scale_derivative, algo.query_logsumexp, algo.query_logsumexp_gradient):
            with pytest.raises(_lib.KmvpError) as e:
                method()
            assert e.value.code == UNSUPPORTED and "batch" in str(e.value)
        with pytest.raises(_lib.KmvpError):
            algo.prepare_data(source_points=y, target_points=y, same_points=True, source_batches=y_off)
            algo.query_nearest(3, exclude_self=True)
        # without batches prepare_data is what it was
        algo.prepare_data(source_points=y, target_points=x, same_points=False)
        algo.prepare_query(source_signal=b)
        algo.query()
        assert algo.get_additional()["device_kernel"] != "lowd_batch_kernel"
        # same points: the sources' offsets serve both
        algo.prepare_data(source_points=y, target_points=y, same_points=True, source_batches=y_off)
        algo.query_nearest(1)
        idx, sq = algo.get_nearest()
        for bi in range(len(ys)):
            assert same((idx[y_off[bi]:y_off[bi + 1]], sq[y_off[bi]:y_off[bi + 1]]), kn.nearest(ys[bi], ys[bi], 1, j_offset=int(y_off[bi])))
    finally:
        algo.done()
    # decided on the host, before any device call: shape, dtype, monotonicity, the ends, what the targets need
    algo = MI355XProduct(kernel="gaussian", dimension=D, precision=precision)
    try:
        for kw in (dict(source_batches=[[0, len(y)]], target_batches=x_off),
                   dict(source_batches=y_off.astype(np.float64), target_batches=x_off),
                   dict(source_batches=y_off[::-1].copy(), target_batches=x_off),
                   dict(source_batches=y_off + 1, target_batches=x_off),
                   dict(source_batches=y_off, target_batches=x_off[:-1]),
                   dict(source_batches=y_off[:-1], target_batches=x_off[:-1]),
                   dict(source_batches=y_off, target_batches=None),
                   dict(source_batches=None, target_batches=x_off),
                   dict(source_batches=[0], target_batches=[0])):
            with pytest.raises(ValueError):
                algo.prepare_data(source_points=y, target_points=x, same_points=False, **kw)
            assert algo._ctx is None
    finally:
        algo.done()
    with pytest.raises(NotImplementedError):
        MI355XProduct(kernel="inverse-distance", dimension=D, precision=precision).prepare_data(
            source_points=y, target_points=x, same_points=False, source_batches=y_off, target_batches=x_off)
