"""GPU tests of the cutoff-radius gradients (include/kmvp.h kmvp_<kernel>_cutoff_grad; lowd_cutoff_grad_kernel,
csrc/kmvp_lowd_cutoff_grad.hpp, on the cell list of csrc/kmvp_cutoff_plan.hpp).

The four truncated kernels are held, target by target, to the float64 model of the very grad_weight / accumulation code the
kernel reuses (oracle/kmvp_lowd_grad_model.py) evaluated on that target's inside sources -- outside pairs add exact zeros,
so the model on the inside subset bounds the chain; Wendland's two to tests/wendland_grad_model.py.  The clouds
(cutoff_reference.cloud) have no pair within the working precision's reach of the boundary, which every test asserts before
it trusts its inside sets.  No tolerance of this file's own, with the one addition test_gpu_cutoff.model_rows states: the
walk folds the float32 sums into float64 at the end of every run and every `chunk` WALKED records, charged as
folds * 2^-53 * mass on top of the model's band (float32 only)."""
import numpy as np
import pytest

import cutoff_grad_reference as gr
import cutoff_reference as cr
import kmvp_lowd_grad_model as gm
import wendland_grad_model as wgm
import wendland_reference as wr
from kernel_matrix_benchmarks_amd import _lib
from kernel_matrix_benchmarks_amd.algorithms.mi355x import MI355XProduct
from test_gpu_cutoff import INVALID, NOT_BUILT, PREC, UNSUPPORTED, Cut, bits, inside_sets, refused, rounded, small_context
from test_gpu_wendland import product_cloud

pytestmark = pytest.mark.gpu

MODES = (("product", 1), ("product", 4), ("density", 1))
FACTORS = (1.0, 2.0)
NAME = "lowd_cutoff_grad_kernel"


class GCut(Cut):
    def gradient(self, kernel, R, b):
        """b: (M, E), or None for density estimation.  (N, E, D) float64."""
        self.signal(b)
        self.ctx.run_cutoff_grad(kernel, R)
        if self.ctx.N > 0:
            assert self.ctx.last_kernel_name == NAME and self.ctx.last_dispatch_note == ""
            assert self.ctx.last_kernel_ms > 0 and self.ctx.last_total_ms >= self.ctx.last_kernel_ms
        E = 1 if b is None else b.shape[1]
        return self.ctx.get_result(self.ctx.N, E * self.ctx.D).reshape(self.ctx.N, E, self.ctx.D)

    def plain_gradient(self, kernel, b):
        self.signal(b)
        self.ctx.run_grad(kernel)
        assert self.ctx.last_kernel_name == "lowd_grad_kernel"
        E = 1 if b is None else b.shape[1]
        return self.ctx.get_result(self.ctx.N, E * self.ctx.D).reshape(self.ctx.N, E, self.ctx.D)


def fold_count(info, chunk, D):
    """Per row: at most one fold per chunk walked and one per run (test_gpu_cutoff.test_model_band)."""
    return info["records"] // chunk + 3 ** (D - 1) + 1


def model_rows(kernel, y, xx, inside, b, precision, chunk, rows=None):
    """(value, band, mass (N, E, D), empty (N,)): kmvp_lowd_grad_model.lowd_gradient on every target's inside sources."""
    N, D = xx.shape
    E = 1 if b is None else b.shape[1]
    value, band, mass = np.zeros((N, E, D)), np.zeros((N, E, D)), np.zeros((N, E, D))
    empty = ~inside.any(axis=1)
    for i in (np.nonzero(~empty)[0] if rows is None else rows):
        j = np.nonzero(inside[i])[0]
        m = gm.lowd_gradient(kernel, y[j], xx[i:i + 1], None if b is None else b[j], precision=precision, chunk=chunk)
        assert not m.nonfinite.any() and not m.poisoned.any()
        value[i], band[i], mass[i] = m.value[0], m.band[0], m.mass[0]
    return value, band, mass, empty


# ---- 1. the four truncated kernels inside the project's own band -------------------------------------------------------------
@pytest.mark.parametrize("prec", list(PREC))
@pytest.mark.parametrize("kernel", gr.TRUNCATED)
def test_model_band_truncated(kernel, prec):
    """A, B, C, K x product E = 1 and 4, density x chunk 512 and 8 x cell factors 1 and 2: every component of every live row
    within the model's band (plus the folds' term) of the model's value on its inside sources; empty rows are exactly 0."""
    precision = PREC[prec]
    f32 = precision == np.float32
    failures, checked, empty_checked, worst = [], 0, 0, 0.0
    for name in cr.CLOUDS:
        y, x, R = cr.cloud(name, precision)
        xx = y if x is None else x
        D = y.shape[1]
        inside = inside_sets(y, x, R, precision)
        b4 = rounded(np.random.RandomState(len(name) + len(kernel)).randn(len(y), 4), precision)
        with GCut(y, x, precision) as ct:
            for chunk in (512, 8):
                ct.ctx.set_option("chunk", chunk)
                models = {sig: model_rows(kernel, y, xx, inside, None if sig == "density" else b4, precision, chunk)
                          for sig in ("product", "density")}      # (the model's columns are independent: E = 4 serves E = 1)
                for factor in FACTORS:
                    ct.ctx.set_option("cutoff_cell_factor", factor)
                    for sig, E in MODES:
                        got = ct.gradient(kernel, R, None if sig == "density" else b4[:, :E])
                        assert got.shape == (len(xx), E, D)
                        folds = fold_count(ct.ctx.cutoff_info(), chunk, D)
                        value, band, mass, empty = models[sig]
                        value, band, mass = value[:, :E], band[:, :E], mass[:, :E]
                        live = ~empty
                        err = np.abs(got[live] - value[live])
                        bound = band[live] + (folds * 2.0 ** -53 * mass[live] if f32 else 0.0)
                        with np.errstate(divide="ignore", invalid="ignore"):
                            ratio = float(np.max(np.where(err > 0, err / bound, 0.0)))
                        worst, checked = max(worst, ratio), checked + err.size
                        if not (np.isfinite(got[live]).all() and (err <= bound).all()):
                            failures.append((name, sig, E, chunk, factor, ratio))
                        if empty.any():
                            assert np.all(got[empty] == 0) and not np.signbit(got[empty]).any(), (name, sig, E, chunk, factor)
                            empty_checked += 1
            ct.ctx.set_option("cutoff_cell_factor", 1.0)
    print(f"\ncutoff gradient model band {kernel} {prec}: {checked} components, worst err / band {worst:.3f}, "
          f"{empty_checked} runs with empty rows, {len(failures)} failures")
    assert not failures, (len(failures), failures[:8])
    assert checked > 0 and empty_checked > 0


# ---- 2. Wendland inside its model's band --------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", list(PREC))
@pytest.mark.parametrize("D", (1, 2, 3))
def test_model_band_wendland(D, prec):
    """test_gpu_wendland.product_cloud's shapes (M = 3001, N = 2999, about 24 inside, one far target), C2 and C4 x product
    E = 1 and 4, density x chunk 512 and 8 x cell factors 1 and 2: every component within wendland_grad_model's band."""
    precision = PREC[prec]
    worst, checked = 0.0, 0
    for same in (True, False):
        y, x, R, b3 = product_cloud(D, precision, same)
        b4 = np.concatenate([b3, rounded(np.random.RandomState(50 + D).randn(len(y), 1), precision)], axis=1)
        with GCut(y, x, precision) as ct:
            for kernel in gr.WENDLAND:
                prs = wgm.pairs(kernel, y, x, R, precision)
                empty = np.bincount(prs.i, minlength=prs.N) == 0
                assert empty.sum() == (0 if same else 1)
                for chunk in (512, 8):
                    ct.ctx.set_option("chunk", chunk)
                    for factor in FACTORS:
                        ct.ctx.set_option("cutoff_cell_factor", factor)
                        models = {}
                        for sig, E in MODES:
                            got = ct.gradient(kernel, R, None if sig == "density" else b4[:, :E])
                            assert got.shape == (prs.N, E, D)
                            folds = fold_count(ct.ctx.cutoff_info(), chunk, D)
                            if sig not in models:   # (the model's columns are independent: E = 4 serves E = 1)
                                models[sig] = wgm.gradient(kernel, y, x, None if sig == "density" else b4, R, precision=precision,
                                                           chunk=chunk, folds=folds, prs=prs)
                            value, band = models[sig].value[:, :E], models[sig].band[:, :E]
                            live = ~empty
                            err = np.abs(got[live] - value[live])
                            assert np.isfinite(got[live]).all()
                            with np.errstate(divide="ignore", invalid="ignore"):
                                ratio = float(np.max(np.where(err > 0, err / band[live], 0.0)))
                            worst, checked = max(worst, ratio), checked + err.size
                            assert (err <= band[live]).all(), (kernel, same, chunk, factor, sig, E, ratio)
                            if empty.any():
                                assert np.all(got[empty] == 0) and not np.signbit(got[empty]).any()
    print(f"\nwendland gradient model band D={D} {prec}: {checked} components, worst err / band {worst:.3f}")
    assert checked > 0


# ---- 3. the inside set and the masking ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", list(PREC))
def test_masking_is_exact(prec):
    """32 probe targets; the sources farther than R (1 + 2^-16) from every probe carry a signal of 1e30, or 0 (removed from
    the sum): the probes' rows are the base signal's rows bit for bit -- an outside pair adds exactly 0 to every component."""
    precision = PREC[prec]
    y, _, R, b3 = product_cloud(3, precision, True)
    rs = np.random.RandomState(5)
    probes = rs.choice(len(y), 32, replace=False)
    far = (wr.sqdists(y[probes], y) > (R * (1.0 + 2.0 ** -16)) ** 2).all(axis=0)
    assert 30 < far.sum() < len(y) - 50
    b = b3[:, :2]
    huge, gone = b.copy(), b.copy()
    huge[far], gone[far] = 1e30, 0.0
    with GCut(y, None, precision) as ct:
        for kernel in ("gaussian", "absolute-exponential", "matern-5/2", "wendland-c2", "wendland-c4"):
            base, got, cut = ct.gradient(kernel, R, b), ct.gradient(kernel, R, huge), ct.gradient(kernel, R, gone)
            assert bits(got[probes], base[probes]) and bits(cut[probes], base[probes]), kernel
            assert np.isfinite(base).all() and not bits(got, base)      # (the huge signal did reach the rows it is inside of)


@pytest.mark.parametrize("prec", list(PREC))
def test_lattice_boundary_pairs_are_inside(prec):
    """The 16 x 16 lattice of spacing 1/8 at R = 5/8: s and r2 are exact in float32, 12 pairs of an inner point sit exactly ON
    the boundary.  The density gradient against the integer-arithmetic inside set (da^2 + db^2 <= 25), within the model's
    band; the sum without the boundary pairs lies outside that band in some rows, so the test tells the two apart."""
    precision = PREC[prec]
    y, _, R = cr.cloud("lattice", precision)
    a = np.rint(y * 8).astype(np.int64)
    d = a[:, None, :] - a[None, :, :]
    s_int = (d * d).sum(axis=-1)
    inside = s_int <= 25
    assert (s_int == 25).sum(axis=1).max() == 12
    with GCut(y, None, precision) as ct:
        for kernel in ("gaussian", "absolute-exponential"):
            got = ct.gradient(kernel, R, None)
            folds = fold_count(ct.ctx.cutoff_info(), 512, 2)
            value, band, mass, empty = model_rows(kernel, y, y, inside, None, precision, 512)
            assert not empty.any()
            bound = band + (folds * 2.0 ** -53 * mass if precision == np.float32 else 0.0)
            assert (np.abs(got - value) <= bound).all(), kernel
            w = gm.weights(kernel, s_int / 64.0) * (s_int < 25)
            open_ball = gm.CONSTANT[kernel] * np.einsum("nm,nmd->nd", w, d / 8.0).reshape(-1, 1, 2)
            assert (np.abs(open_ball - value) > 4 * bound).any(), kernel


# ---- 4. one cell ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", list(PREC))
def test_one_cell_is_the_plain_gradient(prec):
    """R above the diameter: one cell, every pair inside; the result and kmvp_<kernel>_grad's agree within the sum of their two
    model bands (the same model on the whole cloud: the two kernels share the pair arithmetic and differ in the folds)."""
    precision = PREC[prec]
    y, x, _ = cr.cloud("A", precision)
    b = rounded(np.random.RandomState(9).randn(len(y), 2), precision)
    with GCut(y, x, precision) as ct:
        for kernel in gr.TRUNCATED:
            got = ct.gradient(kernel, 3.0, b)
            info = ct.ctx.cutoff_info()
            assert info["cells"] == (1, 1, 1) and info["runs"] == info["tiles"]
            plain = ct.plain_gradient(kernel, b)
            m = gm.lowd_gradient(kernel, y, None, b, precision=precision, chunk=512)
            assert not m.nonfinite.any() and not m.poisoned.any()
            extra = fold_count(info, 512, 3) * 2.0 ** -53 * m.mass if precision == np.float32 else 0.0
            assert (np.abs(got - m.value) <= m.band + extra).all(), kernel
            assert (np.abs(got - plain) <= 2 * m.band + extra).all(), kernel


# ---- 5. non-finite coordinates and coincidences --------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", list(PREC))
def test_non_finite_coordinates(prec):
    """A NaN target: a NaN row in every component.  An infinite target: zeros.  NaN and infinite sources are in no record:
    every other row is the row of the run without them, bit for bit (the plain gradient does not screen its sources)."""
    precision = PREC[prec]
    rs = np.random.RandomState(17)
    yf, xf, R = rounded(rs.rand(300, 3), precision), rounded(rs.rand(150, 3), precision), 0.2
    bf = rounded(rs.randn(300, 2), precision)
    bad_y = np.array([[np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [-np.inf, np.nan, 0.5]])
    at_y = [0, 100, 300]
    y = np.insert(yf, at_y, bad_y, axis=0)
    b = np.insert(bf, at_y, [[1.0, -1.0]] * 3, axis=0)
    bad_x = np.array([[0.5, np.nan, 0.5], [np.inf, 0.5, 0.5], [0.5, 0.5, -np.inf], [np.nan, np.inf, 0.5]])
    x = np.insert(xf, [0, 70, 70, 150], bad_x, axis=0)
    fx = np.isfinite(x).all(axis=1)
    nan_x = np.isnan(x).any(axis=1)
    assert np.array_equal(x[fx], xf) and nan_x.sum() == 2 and (~fx).sum() == 4
    with GCut(yf, xf, precision) as base, GCut(y, x, precision) as ct:
        for kernel, sig in (("gaussian", True), ("absolute-exponential", False), ("matern-3/2", True), ("wendland-c2", True),
                            ("wendland-c4", False)):
            want = base.gradient(kernel, R, bf if sig else None)
            got = ct.gradient(kernel, R, b if sig else None)
            assert bits(got[fx], want) and np.isfinite(want).all() and np.abs(want).max() > 0, kernel
            assert np.all(np.isnan(got[nan_x])), kernel
            inf_rows = got[~fx & ~nan_x]
            assert np.all(inf_rows == 0) and not np.signbit(inf_rows).any(), kernel
    with GCut(np.zeros((0, 3)), xf, precision) as ct:      # M = 0
        got = ct.gradient("gaussian", R, np.zeros((0, 2)))
        assert got.shape == (150, 2, 3) and np.all(got == 0) and not np.signbit(got).any()
    with GCut(yf, np.zeros((0, 3)), precision) as ct:      # N = 0
        assert ct.gradient("gaussian", R, bf).shape == (0, 2, 3)


@pytest.mark.parametrize("prec", list(PREC))
def test_absexp_coincident_points_contribute_nothing(prec):
    """exp(-r) on a cloud with duplicated points, targets = sources: finite everywhere, and every row within the model's band
    of the sum in which a pair at s = 0 -- the own pair and the duplicates -- contributes 0."""
    precision = PREC[prec]
    y, _, R = cr.cloud("K", precision)
    y = y.copy()
    dup = np.arange(0, 40, 2)
    y[dup + 1] = y[dup]
    inside = cr.sqdists(y, y) <= R * R
    b = rounded(np.random.RandomState(21).randn(len(y), 2), precision)
    with GCut(y, None, precision) as ct:
        got = ct.gradient("absolute-exponential", R, b)
        folds = fold_count(ct.ctx.cutoff_info(), 512, 3)
    assert np.isfinite(got).all()
    rows = np.arange(60)
    value, band, mass, _ = model_rows("absolute-exponential", y, y, inside, b, precision, 512, rows=rows)
    bound = band + (folds * 2.0 ** -53 * mass if precision == np.float32 else 0.0)
    assert (np.abs(got[rows] - value[rows]) <= bound[rows]).all()
    want = gr.dense("absolute-exponential", y, None, b, R)          # (the definition drops the pairs at s = 0)
    assert (np.abs(want[rows] - value[rows]) <= 2.0 ** -40 * mass[rows]).all()


# ---- 6. bits --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", list(PREC))
def test_bitwise_and_the_other_entries_untouched(prec):
    """Two runs are equal; product -> gradient -> product -> count -> plain product / plain gradient on one context return
    the bits each entry returns alone on a context of its own: the gradient reads the product's plan and packs and leaves
    them as the product left them."""
    precision = PREC[prec]
    y, x, R = cr.cloud("B", precision)
    b = rounded(np.random.RandomState(13).randn(len(y), 2), precision)

    def plain(ct):
        ct.signal(b)
        ct.ctx.run("gaussian", False)
        return ct.ctx.get_result(ct.ctx.N, 2)

    alone = []
    for call in (lambda ct: ct.product("gaussian", R, False, b), lambda ct: ct.gradient("gaussian", R, b),
                 lambda ct: ct.count(R).astype(np.float64), plain, lambda ct: ct.plain_gradient("gaussian", b),
                 lambda ct: ct.gradient("wendland-c4", R, None)):
        with GCut(y, x, precision) as ct:
            alone.append(call(ct))
    with GCut(y, x, precision) as ct:
        seq = [ct.product("gaussian", R, False, b), ct.gradient("gaussian", R, b), ct.product("gaussian", R, False, b),
               ct.count(R).astype(np.float64), plain(ct), ct.plain_gradient("gaussian", b), ct.gradient("wendland-c4", R, None),
               ct.gradient("gaussian", R, b)]
        assert ct.ctx.last_kernel_name == NAME
    assert bits(seq[0], alone[0]) and bits(seq[2], alone[0])
    assert bits(seq[1], alone[1]) and bits(seq[7], alone[1])
    assert bits(seq[3], alone[2]) and bits(seq[4], alone[3]) and bits(seq[5], alone[4]) and bits(seq[6], alone[5])


# ---- 7. refusals, invalid arguments, the plugin ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(NOT_BUILT))
def test_unsupported(case):
    """Everything kmvp_<kernel>_cutoff refuses -- D > 3, E > 4, bfloat16, a communicator, a source slice, batches:
    KMVP_E_UNSUPPORTED with a message that names the cutoff gradient and the cause."""
    kwargs, word = NOT_BUILT[case]
    ctx = small_context(np.random.RandomState(23), **kwargs)
    try:
        for kernel in ("gaussian", "wendland-c4"):
            refused(ctx, lambda: ctx.run_cutoff_grad(kernel, 0.3), UNSUPPORTED, "cutoff gradient", word)
    finally:
        ctx.close()


def test_invalid():
    """KMVP_E_INVALID: a radius that is not finite or not > 0, no points, no signal; no inverse-distance entry."""
    rs = np.random.RandomState(29)
    ctx = _lib.Context(0)
    try:
        refused(ctx, lambda: ctx.run_cutoff_grad("gaussian", 0.3), INVALID, "cutoff gradient", "kmvp_set_points")
    finally:
        ctx.close()
    ctx = small_context(rs, signal=False)
    try:
        refused(ctx, lambda: ctx.run_cutoff_grad("gaussian", 0.3), INVALID, "cutoff gradient", "kmvp_set_signal")
        ctx.set_signal(np.ascontiguousarray(rs.randn(40, 1), dtype=np.float32))
        for radius in (0.0, -1.0, np.nan, np.inf, -np.inf):
            refused(ctx, lambda: ctx.run_cutoff_grad("wendland-c2", radius), INVALID, "radius")
        ctx.run_cutoff_grad("gaussian", 0.3)                # ... and what is asked for properly still runs
        assert ctx.last_kernel_name == NAME and ctx.get_result(40, 3).shape == (40, 3)
        with pytest.raises(NotImplementedError):
            ctx.run_cutoff_grad("inverse-distance", 0.3)
    finally:
        ctx.close()


@pytest.mark.parametrize("precision", (np.float16, np.float32, np.float64), ids=lambda p: np.dtype(p).name)
def test_plugin(precision):
    """MI355XProduct.query_cutoff_gradient / get_gradient against the _lib call on the same (rounded) inputs, bit for bit, as
    (N, E, D); the NotImplementedError cases are raised before the library is called; query_gradient keeps refusing Wendland."""
    rs = np.random.RandomState(31)
    y, x, b, R = rs.rand(500, 3), rs.rand(200, 3), rs.randn(500, 2), 0.15
    work = np.float64 if np.dtype(precision) == np.float64 else np.float32
    yr, xr, br = rounded(y, precision), rounded(x, precision), rounded(b, precision)
    for kernel in ("matern-3/2", "wendland-c2"):
        algo = MI355XProduct(kernel=kernel, dimension=3, precision=precision)
        try:
            algo.prepare_data(source_points=y, target_points=x, same_points=False)
            algo.prepare_query(source_signal=b)
            algo.query_cutoff(R)
            product = algo.get_result()
            algo.query_cutoff_gradient(R)
            got, extra = algo.get_gradient(), algo.get_additional()
            assert got.shape == (200, 2, 3) and got.flags["C_CONTIGUOUS"] and got.dtype == np.float64
            assert extra["device_kernel"] == NAME and extra["cutoff_cells"][0] > 1 and extra["cutoff_walked"] > 0
            algo.query_cutoff(R)
            assert bits(algo.get_result(), product)
            if kernel == "wendland-c2":
                with pytest.raises(NotImplementedError, match="query_cutoff"):
                    algo.query_gradient()
        finally:
            algo.done()
        with GCut(yr, xr, work) as ct:
            assert bits(got, ct.gradient(kernel, R, br)) and np.abs(got).max() > 0
    algo = MI355XProduct(kernel="gaussian", dimension=3, precision=precision)
    try:        # density estimation on targets = sources
        algo.prepare_data(source_points=y, target_points=y, same_points=True, density_estimation=True)
        algo.prepare_query(source_signal=None)
        algo.query_cutoff_gradient(R)
        got = algo.get_gradient()
        assert got.shape == (500, 1, 3)
    finally:
        algo.done()
    with GCut(yr, None, work) as ct:
        assert bits(got, ct.gradient("gaussian", R, None))
    for kwargs, signal, word in ((dict(kernel="inverse-distance"), b, "inverse-distance"),
                                 (dict(kernel="gaussian", normalize_rows=True), b, "normalize_rows"),
                                 (dict(kernel="wendland-c4"), rs.randn(500, 5), "E = 5")):
        algo = MI355XProduct(dimension=3, precision=precision, **kwargs)
        try:
            algo.prepare_data(source_points=y, target_points=x, same_points=False)
            algo.prepare_query(source_signal=signal)
            with pytest.raises(NotImplementedError, match=word):
                algo.query_cutoff_gradient(R)
        finally:
            algo.done()
