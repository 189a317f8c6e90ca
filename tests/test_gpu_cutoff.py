"""GPU tests of the cutoff-radius entries (include/kmvp.h kmvp_<kernel>_cutoff, kmvp_radius_count, kmvp_cutoff_info;
lowd_cutoff_kernel, lowd_cutoff_count_kernel on the cell list of csrc/kmvp_cutoff_plan.hpp).

The clouds (cutoff_reference.cloud) have no pair within 1e-5 R^2 (float32 inputs) / 1e-12 R^2 (float64) of the boundary, so
the inside set is the same in float64 and in the working precision, whose s chain is off by about (D + 2) 2^-24 relatively;
every test asserts that before it trusts its reference.  The lattice cloud has pairs exactly ON the boundary, where s and
r2 are exact in float32.  Counts are held to integer brute force; products, target by target, to the float64 model of the
very kval / accumulation code the kernel reuses (oracle/kmvp_lowd_model.py: path "lowd", the scalar-cache feed, the chunk of
the run) evaluated on that target's inside sources -- outside pairs add exact zeros, so the model on the inside subset
bounds the chain.  No tolerance of this file's own, with one addition stated at model_rows()."""
import numpy as np
import pytest

import cutoff_reference as cr
import kmvp_lowd_model as lm
from kernel_matrix_benchmarks_amd import _lib
from kernel_matrix_benchmarks_amd.algorithms.mi355x import MI355XProduct

pytestmark = pytest.mark.gpu

PREC = {"f32": np.float32, "f64": np.float64}
UNSUPPORTED, INVALID = 2, 1
MODES = (("product", 1), ("product", 4), ("norm", 1), ("norm", 4), ("density", 1))
FACTORS = (1.0, 1.5, 2.0)


def codes(precision):
    return (_lib.KMVP_F64, np.float64) if np.dtype(precision) == np.float64 else (_lib.KMVP_F32, np.float32)


def rounded(a, precision):
    return np.asarray(a, dtype=precision).astype(np.float64)


def bits(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


class Cut:
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

    def signal(self, b):
        self.ctx.set_signal(None if b is None else np.ascontiguousarray(b, dtype=self.npdt))

    def product(self, kernel, R, normalise, b):
        """b: (M, E), or None for density estimation.  (N, E) float64."""
        self.signal(b)
        self.ctx.run_cutoff(kernel, R, normalise)
        if self.ctx.N > 0:
            assert self.ctx.last_kernel_name == "lowd_cutoff_kernel" and self.ctx.last_dispatch_note == ""
            assert self.ctx.last_kernel_ms > 0 and self.ctx.last_total_ms >= self.ctx.last_kernel_ms
        return self.ctx.get_result(self.ctx.N, 1 if b is None else b.shape[1])

    def count(self, R, exclude_self=False):
        c = self.ctx.radius_count(R, exclude_self)
        assert c.shape == (self.ctx.N,) and c.dtype == np.int64
        if self.ctx.N > 0:
            assert self.ctx.last_kernel_name == "lowd_cutoff_count_kernel"
        return c

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.close()


def inside_sets(y, x, R, precision):
    """The float64 inside mask (N, M), after asserting that no pair is within the working precision's reach of the boundary."""
    assert cr.boundary_clear(y, x, R, precision), "a pair sits within the working precision's reach of the boundary"
    return cr.sqdists(y if x is None else x, y) <= R * R


# ---- 1. counts are exact ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", list(PREC))
@pytest.mark.parametrize("name", cr.CLOUDS + ("lattice",))
def test_counts_are_exact(name, prec):
    """Integer brute force, with and without exclude_self, identical at the three cell factors: the device-side proof that a
    tile's runs cover every inside source and are disjoint (a source in two runs would count twice)."""
    precision = PREC[prec]
    y, x, R = cr.cloud(name, precision)
    if name == "lattice":    # integer arithmetic: a pair is inside iff da^2 + db^2 <= 25; 12 pairs of an inner point sit ON the boundary
        a = np.rint(y * 8).astype(np.int64)
        d = a[:, None, :] - a[None, :, :]
        s_int = (d * d).sum(axis=-1)
        want = (s_int <= 25).sum(axis=1)
        assert (s_int == 25).sum(axis=1).max() == 12 and want.max() == 81
    else:
        want = inside_sets(y, x, R, precision).sum(axis=1)
    seen = []
    with Cut(y, x, precision) as ct:
        for factor in FACTORS:
            ct.ctx.set_option("cutoff_cell_factor", factor)
            got = ct.count(R)
            assert np.array_equal(got, want), (factor, np.nonzero(got != want)[0][:8])
            if x is None:
                assert np.array_equal(ct.count(R, exclude_self=True), want - 1), factor
            seen.append(ct.ctx.cutoff_info())
        assert seen[0]["walked"] <= seen[2]["walked"] and seen[0]["cells"] != seen[2]["cells"]
        if name == "C":
            assert seen[0]["cells"][1:] == (1, 1) and seen[0]["tiles"] == 3


# ---- 2. products inside the project's own band ----------------------------------------------------------------------------
def model_rows(kernel, y, xx, inside, b, normalise, precision, chunk):
    """(value, band, mass, empty) over all targets: the model of oracle/kmvp_lowd_model.py on every target's inside sources.
    The walk folds the float32 sum into float64 more often than the plain entry the model was written for -- at the end of
    every run and every `chunk` WALKED records, not every `chunk` live ones; what that adds is charged by the caller as
    folds * 2^-53 * mass on top of the model's band (float32 only: float64 keeps one chain)."""
    N = len(xx)
    E = 1 if b is None else b.shape[1]
    value, band, mass = np.zeros((N, E)), np.zeros((N, E)), np.zeros((N, E))
    empty = ~inside.any(axis=1)
    for i in np.nonzero(~empty)[0]:
        j = np.nonzero(inside[i])[0]
        m = lm.lowd_product(kernel, y[j], xx[i:i + 1], None if b is None else b[j], normalise, precision=precision, path="lowd",
                            feed=0, chunk=chunk)
        assert not m.flagged.any() and not m.nonfinite.any()
        value[i], band[i], mass[i] = m.value[0], m.band[0], m.mass[0]
    return value, band, mass, empty


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
@pytest.mark.parametrize("kernel", cr.KERNELS)
def test_model_band(kernel, prec):
    """Four kernels x product / normalised / density, E = 1 and 4, chunk 512 and 8, on A, B, C and K: every row within the
    model's band (plus the folds' term, see model_rows) of the model's value on its inside sources; a row with nothing
    inside is the plain entry's M = 0 row bit for bit; normalised density estimation is 1 where something is inside."""
    precision = PREC[prec]
    f32 = precision == np.float32
    failures, checked, empty_checked, plain_rows = [], 0, 0, {}
    for name in cr.CLOUDS:
        y, x, R = cr.cloud(name, precision)
        xx = y if x is None else x
        D = y.shape[1]
        inside = inside_sets(y, x, R, precision)
        b4 = rounded(np.random.RandomState(len(name) + len(kernel)).randn(len(y), 4), precision)
        with Cut(y, x, precision) as ct:
            for chunk in (512, 8):
                ct.ctx.set_option("chunk", chunk)
                models = {}
                for sig, E in MODES:
                    b = None if sig == "density" else b4[:, :E]
                    got = ct.product(kernel, R, sig == "norm", b)
                    assert got.shape == (len(xx), E)
                    info = ct.ctx.cutoff_info()
                    folds = info["records"] // chunk + 3 ** (D - 1) + 1    # per row: at most one per chunk walked and one per run
                    if sig not in models:    # (the model's columns are independent: E = 4 serves E = 1)
                        models[sig] = model_rows(kernel, y, xx, inside, None if sig == "density" else b4, sig == "norm", precision, chunk)
                    value, band, mass, empty = models[sig]
                    value, band, mass = value[:, :E], band[:, :E], mass[:, :E]
                    extra = folds * 2.0 ** -53 * (2 * (mass + np.abs(value)) if sig == "norm" else mass) if f32 else 0.0
                    live = ~empty
                    err = np.abs(got[live] - value[live])
                    checked += err.size
                    if not (np.isfinite(got[live]).all() and (err <= band[live] + (extra[live] if f32 else 0.0)).all()):
                        with np.errstate(divide="ignore", invalid="ignore"):
                            failures.append((name, sig, E, chunk, float(np.nanmax(err / band[live]))))
                    if empty.any():
                        if (name, sig, E) not in plain_rows:
                            plain_rows[name, sig, E] = plain_empty_sources(xx[empty], kernel, sig, E, precision)
                        want = plain_rows[name, sig, E]
                        assert bits(got[empty], want), (name, sig, E, chunk)
                        assert np.all(np.isnan(want)) if sig == "norm" else np.all(want == 0)
                        empty_checked += 1
                # normalised density estimation: v / v
                got = ct.product(kernel, R, True, None)
                assert bits(got, np.where(inside.any(axis=1), 1.0, np.nan).reshape(-1, 1)), (name, chunk)
    print(f"\ncutoff model band {kernel} {prec}: {checked} elements inside the band, {empty_checked} runs with empty rows, "
          f"{len(failures)} failures")
    assert not failures, (len(failures), failures[:8])
    assert checked > 0 and empty_checked > 0


# ---- 3. masking is exact ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", list(PREC))
def test_masking_is_exact(prec):
    """On A: the signal of every source outside all inside sets of 32 probe targets set to 1e30 -- the probes' rows do not
    change by a bit, in the product and in the normalised product: an outside pair adds k = 0 times b, exactly 0."""
    precision = PREC[prec]
    y, x, R = cr.cloud("A", precision)
    inside = inside_sets(y, x, R, precision)
    rs = np.random.RandomState(5)
    probes = rs.choice(len(y), 32, replace=False)
    far = ~inside[probes].any(axis=0)
    assert 30 < far.sum() < len(y) - 50
    b = rounded(rs.randn(len(y), 2), precision)
    b2 = b.copy()
    b2[far] = 1e30
    with Cut(y, x, precision) as ct:
        for kernel, normalise in (("gaussian", False), ("matern-3/2", True)):
            base, got = ct.product(kernel, R, normalise, b), ct.product(kernel, R, normalise, b2)
            assert bits(got[probes], base[probes]), kernel
            assert not bits(got, base)          # (the huge signal did reach the rows it is inside of)


# ---- 4. one cell ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", list(PREC))
def test_one_cell_is_the_full_product(prec):
    """R above the diameter: one cell, every pair inside, every row inside the model's band of the full product."""
    precision = PREC[prec]
    y, x, _ = cr.cloud("B", precision)
    b = rounded(np.random.RandomState(9).randn(len(y), 3), precision)
    with Cut(y, x, precision) as ct:
        assert np.array_equal(ct.count(3.0), np.full(len(x), len(y)))
        assert ct.ctx.cutoff_info()["cells"] == (1, 1, 1) and ct.ctx.cutoff_info()["runs"] == ct.ctx.cutoff_info()["tiles"]
        for kernel, normalise in (("gaussian", False), ("absolute-exponential", True), ("matern-5/2", False)):
            got = ct.product(kernel, 3.0, normalise, b)
            m = lm.lowd_product(kernel, y, x, b, normalise, precision=precision, path="lowd", feed=0, chunk=512)
            assert not m.flagged.any() and not m.nonfinite.any()
            assert (np.abs(got - m.value) <= m.band).all(), kernel


# ---- 5. bitwise -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", list(PREC))
def test_bitwise_and_the_other_entries_untouched(prec):
    """Results repeat run to run; the plain product, kmvp_nearest and a batched product return the same bits before and after
    cutoff calls on one context (the cutoff's layouts are its own)."""
    precision = PREC[prec]
    y, x, R = cr.cloud("B", precision)
    b = rounded(np.random.RandomState(13).randn(len(y), 2), precision)

    def others(ct):
        ct.signal(b)
        ct.ctx.run("gaussian", False)
        out = [ct.ctx.get_result(ct.ctx.N, 2)]
        idx, sq = ct.ctx.run_nearest(4)
        out += [idx.astype(np.float64), sq]
        ct.ctx.set_batches([0, 200, len(y)], [0, 100, len(x)])
        ct.ctx.run("gaussian", True)
        assert ct.ctx.last_kernel_name == "lowd_batch_kernel"
        out.append(ct.ctx.get_result(ct.ctx.N, 2))
        ct.ctx.set_batches(None)
        return out

    with Cut(y, x, precision) as ct:
        before = others(ct)
        first = [ct.product("gaussian", R, False, b), ct.product("matern-5/2", R, True, b), ct.product("absolute-exponential", R, False, None)]
        cnt = ct.count(R)
        between = others(ct)
        again = [ct.product("gaussian", R, False, b), ct.product("matern-5/2", R, True, b), ct.product("absolute-exponential", R, False, None)]
        assert all(bits(a, c) for a, c in zip(first, again)) and np.array_equal(cnt, ct.count(R))
        ct.ctx.set_option("cutoff_cell_factor", 2.0)
        ct.product("gaussian", R, False, b)
        after = others(ct)
        for a, c, d in zip(before, between, after):
            assert bits(a, c) and bits(a, d)
    with Cut(y, x, precision) as fresh:       # a fresh context returns the same cutoff bits
        assert bits(first[0], fresh.product("gaussian", R, False, b))


# ---- 6. non-finite coordinates ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", list(PREC))
def test_non_finite_coordinates(prec):
    """A NaN target: a NaN row and count -1.  An infinite target: 0 (NaN when normalised) and count 0.  NaN and infinite
    sources contribute to nothing.  None of them disturbs any other row by a bit: such points are in no cell, so the finite
    points' plan is the one without them.  N = 0 and M = 0 work."""
    precision = PREC[prec]
    rs = np.random.RandomState(17)
    yf, xf, R = rounded(rs.rand(300, 3), precision), rounded(rs.rand(150, 3), precision), 0.2
    bf = rounded(rs.randn(300, 2), precision)
    bad_y = np.array([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [-np.inf, np.nan, 0.5]])
    at_y = [0, 100, 300]
    y = np.insert(yf, at_y, bad_y, axis=0)
    b = np.insert(bf, at_y, [[1.0, -1.0]] * 3, axis=0)
    fy = np.isfinite(y).all(axis=1)
    bad_x = np.array([[0.5, np.nan, 0.5], [np.inf, 0.5, 0.5], [0.5, 0.5, -np.inf], [np.nan, np.inf, 0.5]])
    at_x = [0, 70, 70, 150]
    x = np.insert(xf, at_x, bad_x, axis=0)
    fx = np.isfinite(x).all(axis=1)
    nan_x = np.isnan(x).any(axis=1)
    assert np.array_equal(y[fy], yf) and np.array_equal(x[fx], xf) and nan_x.sum() == 2 and (~fx).sum() == 4
    with Cut(yf, xf, precision) as base, Cut(y, x, precision) as ct:
        for kernel, normalise, sig in (("gaussian", False, True), ("matern-3/2", True, True), ("absolute-exponential", False, False)):
            want = base.product(kernel, R, normalise, bf if sig else None)
            got = ct.product(kernel, R, normalise, b if sig else None)
            assert bits(got[fx], want), kernel
            assert np.all(np.isnan(got[nan_x]))
            inf_rows = got[~fx & ~nan_x]
            assert np.all(np.isnan(inf_rows)) if normalise else np.all(inf_rows == 0)
        cnt = ct.count(R)
        assert np.array_equal(cnt[fx], base.count(R)) and np.all(cnt[nan_x] == -1) and np.all(cnt[~fx & ~nan_x] == 0)
        assert cnt[fx].max() > 5
    with Cut(y, None, precision) as ct:       # targets = sources with exclude_self: only finite points subtract their own pair
        c0, c1 = ct.count(R), ct.count(R, exclude_self=True)
        assert np.array_equal(c1[fy], c0[fy] - 1) and np.array_equal(c1[~fy], c0[~fy]) and set(c0[~fy]) == {-1, 0}
    with Cut(np.zeros((0, 3)), xf, precision) as ct:      # M = 0
        assert np.all(ct.product("gaussian", R, False, np.zeros((0, 2))) == 0)
        assert np.all(np.isnan(ct.product("gaussian", R, True, np.zeros((0, 2))))) and np.all(ct.count(R) == 0)
    with Cut(yf, np.zeros((0, 3)), precision) as ct:      # N = 0
        assert ct.product("gaussian", R, False, bf).shape == (0, 2) and ct.count(R).shape == (0,)


# ---- 7. refusals --------------------------------------------------------------------------------------------------------------
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


NOT_BUILT = {"D4": (dict(D=4), "D = 4"), "E5": (dict(E=5), "E = 5"), "bfloat16": (dict(D=16, dtype=_lib.KMVP_BF16), "bfloat16"),
             "communicator": (dict(comm=True), "communicator"), "source_slice": (dict(M_total=50), "M < M_total"),
             "batches": (dict(batches=True), "kmvp_set_batches")}


@pytest.mark.parametrize("case", list(NOT_BUILT))
def test_unsupported(case):
    """D > 3, E > 4, a bfloat16 context, an attached communicator, a source slice and batches set: KMVP_E_UNSUPPORTED with a
    message that names the cutoff and the cause."""
    kwargs, word = NOT_BUILT[case]
    ctx = small_context(np.random.RandomState(23), **kwargs)
    try:
        refused(ctx, lambda: ctx.run_cutoff("gaussian", 0.3, False), UNSUPPORTED, "cutoff", word)
        refused(ctx, lambda: ctx.run_cutoff("matern-5/2", 0.3, True), UNSUPPORTED, "cutoff", word)
        if "E" not in kwargs:
            refused(ctx, lambda: ctx.radius_count(0.3), UNSUPPORTED, "cutoff", word)
    finally:
        ctx.close()


def test_invalid():
    """KMVP_E_INVALID: a radius that is not finite or not > 0, no points, no signal (the products), exclude_self when the
    targets are not the sources, kmvp_cutoff_info before any cutoff call, and a bad cell factor."""
    rs = np.random.RandomState(29)
    ctx = _lib.Context(0)
    try:
        refused(ctx, lambda: ctx.run_cutoff("gaussian", 0.3, False), INVALID, "kmvp_set_points")
        refused(ctx, lambda: ctx.radius_count(0.3), INVALID, "kmvp_set_points")
        refused(ctx, lambda: ctx.cutoff_info(), INVALID, "cutoff")
    finally:
        ctx.close()
    ctx = small_context(rs, signal=False)
    try:
        refused(ctx, lambda: ctx.run_cutoff("gaussian", 0.3, False), INVALID, "kmvp_set_signal")
        assert ctx.radius_count(0.3).shape == (40,)         # the count needs the points only
        ctx.set_signal(np.ascontiguousarray(rs.randn(40, 1), dtype=np.float32))
        for radius in (0.0, -1.0, np.nan, np.inf, -np.inf):
            refused(ctx, lambda: ctx.run_cutoff("gaussian", radius, False), INVALID, "radius")
            refused(ctx, lambda: ctx.radius_count(radius), INVALID, "radius")
        for factor in (0.5, np.nan, np.inf):
            refused(ctx, lambda: ctx.set_option("cutoff_cell_factor", factor), INVALID, "cutoff_cell_factor")
        ctx.run_cutoff("gaussian", 0.3, False)              # ... and what is asked for properly still runs
        with pytest.raises(NotImplementedError):
            ctx.run_cutoff("inverse-distance", 0.3, False)
    finally:
        ctx.close()
    ctx = small_context(rs, same=False)
    try:
        refused(ctx, lambda: ctx.radius_count(0.3, exclude_self=True), INVALID, "exclude_self")
        assert ctx.radius_count(0.3).shape == (30,)
    finally:
        ctx.close()


# ---- 8. the plugin --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", (np.float16, np.float32, np.float64), ids=lambda p: np.dtype(p).name)
def test_plugin(precision):
    """MI355XProduct.query_cutoff / query_radius_count against the _lib calls on the same (rounded) inputs, bit for bit;
    get_additional() carries the info words; query() after query_cutoff() is the plain product's bits."""
    rs = np.random.RandomState(31)
    y, x, b, R = rs.rand(500, 3), rs.rand(200, 3), rs.randn(500, 2), 0.15
    work = np.float64 if np.dtype(precision) == np.float64 else np.float32
    yr, xr, br = rounded(y, precision), rounded(x, precision), rounded(b, precision)
    for normalize in (False, True):
        algo = MI355XProduct(kernel="matern-3/2", dimension=3, precision=precision, normalize_rows=normalize)
        try:
            algo.prepare_data(source_points=y, target_points=x, same_points=False)
            algo.prepare_query(source_signal=b)
            algo.query()
            plain = algo.get_result()
            algo.query_cutoff(R)
            got, extra = algo.get_result(), algo.get_additional()
            assert got.shape == (200, 2) and got.flags["C_CONTIGUOUS"] and got.dtype == np.float64
            assert extra["device_kernel"] == "lowd_cutoff_kernel" and extra["cutoff_cells"][0] > 1 and extra["cutoff_walked"] > 0
            assert {"cutoff_tiles", "cutoff_runs", "cutoff_records", "cutoff_plan_ms"} <= set(extra)
            algo.query_radius_count(R)
            cnt = algo.get_radius_count()
            assert algo.get_additional()["device_kernel"] == "lowd_cutoff_count_kernel"
            algo.query()
            assert bits(algo.get_result(), plain) and "cutoff_cells" not in algo.get_additional()
            with pytest.raises(ValueError):
                algo.query_radius_count(R, exclude_self=True)
        finally:
            algo.done()
        with Cut(yr, xr, work) as ct:
            assert bits(got, ct.product("matern-3/2", R, normalize, br)) and np.array_equal(cnt, ct.count(R))
            assert not bits(got, plain)
    algo = MI355XProduct(kernel="gaussian", dimension=3, precision=precision)
    try:        # density estimation on targets = sources, and the count without a signal
        algo.prepare_data(source_points=y, target_points=y, same_points=True, density_estimation=True)
        algo.query_radius_count(R, exclude_self=True)
        cnt = algo.get_radius_count()
        algo.prepare_query(source_signal=None)
        algo.query_cutoff(R)
        got = algo.get_result()
    finally:
        algo.done()
    with Cut(yr, None, work) as ct:
        assert bits(got, ct.product("gaussian", R, False, None)) and np.array_equal(cnt, ct.count(R, exclude_self=True))
    with pytest.raises(NotImplementedError):
        algo = MI355XProduct(kernel="inverse-distance", dimension=3, precision=precision)
        try:
            algo.prepare_data(source_points=y, target_points=x, same_points=False)
            algo.prepare_query(source_signal=b)
            algo.query_cutoff(R)
        finally:
            algo.done()
