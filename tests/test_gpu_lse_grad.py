"""GPU tests of the gradient of the log-sum-exp with respect to the target points (lowd_lse_grad_kernel, include/kmvp.h
kmvp_<kernel>_logsumexp_grad) against the numpy restatement of its definition (lse_grad_reference.py, itself checked
against central differences of lse_reference.logsumexp in test_lse_grad_reference.py).

The measure is, per row and column, max_d |G - G_ref| / max(1, max_d |G_ref|), with the project's tolerances (DESIGN.md
section 4, as test_gpu_lse.py):
  float64            <= 1e-11
  float32 / float16  <= max(1e-5, 2 x the restatement's own float32 error on the same (rounded) inputs)
Entries that are NaN in the restatement must be NaN on the GPU, and no others may be.
"""
import json
import os

import numpy as np
import pytest

import grad_reference
import kmvp_oracle
import lse_grad_reference
import lse_reference
from conftest import rel_err
from kernel_matrix_benchmarks_amd import _lib
from kernel_matrix_benchmarks_amd.algorithms.mi355x import MI355XProduct
from test_gpu_multirank import _spawn

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

TOL64 = 1e-11
TOL32 = 1e-5
KERNELS = lse_grad_reference.KERNELS
PRECISIONS = (np.float64, np.float32, np.float16)
NAME = "lowd_lse_grad_kernel"


def rounded(a, precision):
    return None if a is None else np.asarray(a, dtype=precision).astype(np.float64)


def grad_err(got, want):
    """max over the (row, column) pairs that are finite in the reference of max_d |G - G_ref| / max(1, max_d |G_ref|);
    NaN entries must coincide, and no entry of the result may be infinite where the reference is finite."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    same_class = (np.isnan(got) == np.isnan(want)) & (np.isfinite(got) == np.isfinite(want))
    bad = np.argwhere(~same_class)
    assert same_class.all(), ("NaN / non-finite entries differ", bad[:8].tolist(), got[~same_class][:8], want[~same_class][:8])
    fin = np.isfinite(want).all(axis=-1)
    if not fin.any():
        return 0.0
    diff = np.max(np.abs(got - want), axis=-1)[fin]
    return float(np.max(diff / np.maximum(1.0, np.max(np.abs(want), axis=-1)[fin])))


def tolerance(kernel, y, x, c, precision, want, rows=None):
    """The float32 rule: the restatement run in float32 on the same inputs sets the scale of what float32 can do."""
    if np.dtype(precision) == np.float64:
        return TOL64, 0.0
    own = lse_grad_reference.gradient(kernel=kernel, source_points=y, target_points=x, source_signal=c, precision=np.float32,
                                      rows=rows)
    fin = np.isfinite(want).all(axis=-1) & np.isfinite(own).all(axis=-1)
    own_err = 0.0
    if fin.any():
        own_err = float(np.max(np.max(np.abs(own - want), axis=-1)[fin] / np.maximum(1.0, np.max(np.abs(want), axis=-1)[fin])))
    return max(TOL32, 2 * own_err), own_err


def check(got, want, tol, label):
    err = grad_err(got, want)
    print(f"{label}: err {err:.3e} (tolerance {tol:.1e}, {int(np.isnan(want).sum())} NaN entries)")
    assert err <= tol, (label, err, tol)
    return err


def plugin_grad(kernel, y, x, c, precision, **options):
    """The runner's call order with query_logsumexp_gradient() / get_logsumexp_gradient() in the place of query() /
    get_result()."""
    algo = MI355XProduct(kernel=kernel, dimension=y.shape[1], precision=precision, **options)
    try:
        algo.prepare_data(source_points=y, target_points=y if x is None else x, same_points=x is None,
                          density_estimation=c is None)
        algo.fit()
        algo.prepare_query(source_signal=c)
        algo.query_logsumexp_gradient()
        G = algo.get_logsumexp_gradient()
        extra = algo.get_additional()
    finally:
        algo.done()
    N = y.shape[0] if x is None else x.shape[0]
    assert G.shape == (N, 1 if c is None else c.shape[1], y.shape[1])
    assert G.dtype == np.float64 and G.flags["C_CONTIGUOUS"]
    assert extra["device_kernel"] == NAME and extra["dispatch_note"] == "", extra
    return G


def ctx_grad(kernel, y, x, c, dtype, *, options=(), j_offset=0, M_total=None, comm=False):
    """Through the C ABI's typed wrapper."""
    npdt = np.float64 if dtype == _lib.KMVP_F64 else np.float32
    ctx = _lib.Context(0)
    try:
        if comm:
            ctx.comm_init(_lib.comm_unique_id(), 0, 1)
        for key, value in options:
            ctx.set_option(key, value)
        ctx.set_points(np.ascontiguousarray(y, dtype=npdt), None if x is None else np.ascontiguousarray(x, dtype=npdt), dtype,
                       j_offset=j_offset, M_total=M_total)
        ctx.set_signal(None if c is None else np.ascontiguousarray(c, dtype=npdt))
        N = y.shape[0] if x is None else x.shape[0]
        D = y.shape[1]
        NE = 1 if c is None else c.shape[1]
        ctx.run_lse_grad(kernel)
        if y.shape[0] > 0 and N > 0:
            assert ctx.last_kernel_name == NAME and ctx.last_dispatch_note == ""
            assert ctx.last_kernel_ms > 0 and ctx.last_total_ms >= ctx.last_kernel_ms
        return ctx.get_result(N, NE * D).reshape(N, NE, D)
    finally:
        ctx.close()


def ctx_lse(kernel, y, x, c, dtype, *, options=(), j_offset=0, M_total=None):
    npdt = np.float64 if dtype == _lib.KMVP_F64 else np.float32
    ctx = _lib.Context(0)
    try:
        for key, value in options:
            ctx.set_option(key, value)
        ctx.set_points(np.ascontiguousarray(y, dtype=npdt), None if x is None else np.ascontiguousarray(x, dtype=npdt), dtype,
                       j_offset=j_offset, M_total=M_total)
        ctx.set_signal(None if c is None else np.ascontiguousarray(c, dtype=npdt))
        ctx.run_lse(kernel)
        return ctx.get_result(y.shape[0] if x is None else x.shape[0], 1 if c is None else c.shape[1])
    finally:
        ctx.close()


# ---- parity ------------------------------------------------------------------------------------------------------------
SHAPES = ((1, 1), (63, 3), (65, 5), (300, 257))  # (N, M): one pair, below / above a 64-target tile, a ragged batch of sources


@pytest.mark.parametrize("precision", PRECISIONS, ids=[np.dtype(p).name for p in PRECISIONS])
@pytest.mark.parametrize("kernel", KERNELS)
def test_logsumexp_gradient_parity(kernel, precision):
    """D in {1, 3, 8} x E in {density, 1, 3, 4} x targets == sources and != x the four shapes (targets == sources: N = M, the
    shape's source count)."""
    worst = 0.0
    for D in (1, 3, 8):
        for E in (None, 1, 3, 4):
            for N, M in SHAPES:
                for same in (True, False):
                    rs = np.random.RandomState(1000 * D + 100 * (E or 0) + N + (7 if same else 0))
                    y = rounded(rs.randn(M, D), precision)
                    x = None if same else rounded(rs.randn(N, D) * 1.5, precision)
                    c = None if E is None else rounded(rs.randn(M, E) * 2.0, precision)
                    want = lse_grad_reference.gradient(kernel=kernel, source_points=y, target_points=x, source_signal=c)
                    got = plugin_grad(kernel, y, x, c, precision)
                    tol, own = tolerance(kernel, y, x, c, precision, want)
                    label = f"{kernel} {np.dtype(precision).name} D={D} E={E} N={M if same else N} M={M} same={same}"
                    err = grad_err(got, want)
                    assert err <= tol, (label, err, tol, own)
                    worst = max(worst, err / tol)
    print(f"{kernel} {np.dtype(precision).name}: worst err / tolerance over 96 cases {worst:.3f}")


# ---- several segments and chunks, the shift rising throughout or never -------------------------------------------------
_SEG = {}


def segment_case(kernel):
    """test_gpu_lse.py's cloud: N = 1000 targets in a small cluster, M = 5001 sources at distances 0 .. ~45 from it
    (Gaussian logits down to -2000), E = 2; the restatement once per kernel."""
    if kernel not in _SEG:
        rs = np.random.RandomState(77)
        x = rounded(rs.rand(1000, 3) * 0.5, np.float32)
        direction = rs.randn(5001, 3)
        direction /= np.linalg.norm(direction, axis=1, keepdims=True)
        y = rounded(0.25 + direction * (rs.rand(5001, 1) * 45.0), np.float32)
        c = rounded(rs.randn(5001, 2), np.float32)
        near_first = np.argsort(np.linalg.norm(y - 0.25, axis=1), kind="stable")
        want = lse_grad_reference.gradient(kernel=kernel, source_points=y, target_points=x, source_signal=c)
        tol32, own = tolerance(kernel, y, x, c, np.float32, want)
        _SEG[kernel] = (y, x, c, near_first, want, tol32)
    return _SEG[kernel]


@pytest.mark.parametrize("dtype", (_lib.KMVP_F32, _lib.KMVP_F64), ids=("float32", "float64"))
@pytest.mark.parametrize("kernel", KERNELS)
def test_logsumexp_gradient_on_several_segments_and_chunks(kernel, dtype):
    """segments = 3, chunk = 256: sources nearest-LAST (the shift rises throughout the loop, every rise rescales all D + 1
    sums) and nearest-FIRST (it never rises after the first batch) both meet the restatement; 1 and 8 segments agree with 3
    within the tolerance."""
    y, x, c, near_first, want, tol32 = segment_case(kernel)
    tol = TOL64 if dtype == _lib.KMVP_F64 else tol32
    runs = {}
    for name, order in (("nearest-last", near_first[::-1]), ("nearest-first", near_first)):
        got = ctx_grad(kernel, y[order], x, c[order], dtype, options=(("segments", 3), ("chunk", 256)))
        check(got, want, tol, f"{kernel} {name} segments=3 chunk=256")
        runs[name] = got
    for seg in (1, 8):
        other = ctx_grad(kernel, y[near_first[::-1]], x, c[near_first[::-1]], dtype, options=(("segments", seg), ("chunk", 256)))
        check(other, want, tol, f"{kernel} nearest-last segments={seg}")
        err = grad_err(other, runs["nearest-last"])
        print(f"{kernel}: segments={seg} against segments=3: {err:.3e}")
        assert err <= tol, (kernel, seg, err, tol)


# ---- the reason for the feature ----------------------------------------------------------------------------------------
def test_logsumexp_gradient_where_gradient_and_product_underflow():
    """Targets at distance ~100 from a unit cloud, float32: query_gradient() and query() with b = exp(c) are both exactly 0
    (the ratio is 0 / 0); the gradient of the log-sum-exp is finite, within tolerance, and -2 (x - ybar) has norm near 200.
    Near the cloud, where nothing underflows, it agrees with gradient / product at the float32 rule."""
    rs = np.random.RandomState(5)
    y = rounded(rs.rand(500, 3), np.float32)
    c = rounded(rs.randn(500, 2), np.float32)
    x_far = rounded(rs.rand(200, 3) + np.array([100.0, 0.0, 0.0]), np.float32)
    x_near = rounded(rs.rand(200, 3) + 0.5, np.float32)
    b32 = rounded(np.exp(c), np.float32)

    def product_and_gradient(x):
        algo = MI355XProduct(kernel="gaussian", dimension=3, precision=np.float32, fast_sqdists=False)
        try:
            algo.prepare_data(source_points=y, target_points=x, same_points=False)
            algo.fit()
            algo.prepare_query(source_signal=b32)
            algo.query()
            p = algo.get_result()
            algo.query_gradient()
            return p, algo.get_gradient()
        finally:
            algo.done()

    p_far, g_far = product_and_gradient(x_far)
    assert np.all(p_far == 0.0) and np.all(g_far == 0.0)
    want = lse_grad_reference.gradient(kernel="gaussian", source_points=y, target_points=x_far, source_signal=c)
    got = plugin_grad("gaussian", y, x_far, c, np.float32)
    assert np.isfinite(got).all()
    norm = np.linalg.norm(got, axis=-1)
    assert norm.min() > 195.0 and norm.max() < 205.0, (norm.min(), norm.max())
    tol, own = tolerance("gaussian", y, x_far, c, np.float32, want)
    check(got, want, tol, f"gaussian float32, targets at distance 100 (restatement's own float32 error {own:.1e})")

    # near the cloud: the float64 ratio of the two restatements with the weights the product was handed (exp(c) rounded)
    truth = (grad_reference.gradient(kernel="gaussian", source_points=y, target_points=x_near, source_signal=b32)
             / kmvp_oracle.product(kernel="gaussian", source_points=y, target_points=x_near, source_signal=b32)[:, :, None])
    own_ratio = (grad_reference.gradient(kernel="gaussian", source_points=y, target_points=x_near, source_signal=b32,
                                         precision=np.float32)
                 / kmvp_oracle.product(kernel="gaussian", source_points=y, target_points=x_near, source_signal=b32,
                                       precision=np.float32)[:, :, None])
    tol_new, own_new = tolerance("gaussian", y, x_near, c, np.float32, truth)
    tol_ratio = max(TOL32, 2 * grad_err(own_ratio, truth))
    p_near, g_near = product_and_gradient(x_near)
    e_ratio = grad_err(g_near / p_near[:, :, None], truth)
    e_new = grad_err(plugin_grad("gaussian", y, x_near, c, np.float32), truth)
    print(f"near the cloud: gradient / product err {e_ratio:.2e} (tolerance {tol_ratio:.1e}), log-sum-exp gradient err "
          f"{e_new:.2e} (tolerance {tol_new:.1e})")
    assert e_ratio <= tol_ratio and e_new <= tol_new, (e_ratio, tol_ratio, e_new, tol_new)


# ---- conventions -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (_lib.KMVP_F32, _lib.KMVP_F64), ids=("float32", "float64"))
@pytest.mark.parametrize("kernel", KERNELS)
def test_logsumexp_gradient_conventions(kernel, dtype):
    precision = np.float64 if dtype == _lib.KMVP_F64 else np.float32
    rs = np.random.RandomState(11)
    y, x = rounded(rs.rand(301, 3), precision), rounded(rs.rand(130, 3), precision)
    # some c = -inf, a column that is all -inf, a column spanning +-1e3
    c = rounded(rs.randn(301, 4), precision)
    c[::3, 0] = -np.inf
    c[:, 1] = -np.inf
    c[:, 2] = rounded(rs.uniform(-1e3, 1e3, 301), precision)
    want = lse_grad_reference.gradient(kernel=kernel, source_points=y, target_points=x, source_signal=c)
    assert np.isnan(want[:, 1]).all() and np.isfinite(want[:, [0, 2, 3]]).all()
    got = ctx_grad(kernel, y, x, c, dtype)
    tol, own = tolerance(kernel, y, x, c, precision, want)
    check(got, want, tol, f"{kernel} c = -inf entries, an all -inf column, c spanning +-1e3 (own {own:.1e})")
    assert np.isnan(got[:, 1]).all() and np.isfinite(got[:, [0, 2, 3]]).all()
    # every c = -inf and no source at all: NaN everywhere
    assert np.isnan(ctx_grad(kernel, y, x, np.full((301, 2), -np.inf), dtype)).all()
    empty = ctx_grad(kernel, y[:0], x, c[:0], dtype)
    assert empty.shape == (130, 4, 3) and np.isnan(empty).all()
    # a NaN target coordinate: that row NaN in every column, every other row bitwise unchanged
    xn = x.copy()
    xn[77, 2] = np.nan
    gn = ctx_grad(kernel, y, xn, c, dtype)
    assert np.isnan(gn[77]).all(), gn[77]
    assert np.array_equal(np.delete(gn, 77, axis=0), np.delete(got, 77, axis=0), equal_nan=True)
    # logits around -1e4 (float32) / -1e6 (float64): never exp(max logit)
    shift = {("gaussian", _lib.KMVP_F32): 1e2, ("gaussian", _lib.KMVP_F64): 1e3,
             ("absolute-exponential", _lib.KMVP_F32): 1e4, ("absolute-exponential", _lib.KMVP_F64): 1e6}[(kernel, dtype)]
    x_far = rounded(x + np.array([shift, 0.0, 0.0]), precision)
    want_far = lse_grad_reference.gradient(kernel=kernel, source_points=y, target_points=x_far, source_signal=c[:, [0, 3]])
    assert np.isfinite(want_far).all()
    tol, own = tolerance(kernel, y, x_far, c[:, [0, 3]], precision, want_far)
    check(ctx_grad(kernel, y, x_far, c[:, [0, 3]], dtype), want_far, tol, f"{kernel} targets shifted by {shift:g} (own {own:.1e})")


@pytest.mark.parametrize("dtype", (_lib.KMVP_F32, _lib.KMVP_F64), ids=("float32", "float64"))
@pytest.mark.parametrize("kernel", KERNELS)
def test_a_nan_or_infinite_log_weight_makes_its_column_non_finite(kernel, dtype):
    """One c = NaN (column 0) and one c = +inf (column 1) among live sources -- in the first batch, in the middle of a
    segment and in the last, guarded batch: no entry of that column is finite, for any target, also on several segments.
    Column 2 is clean: it meets the restatement and its bits do not depend on what the other columns hold."""
    precision = np.float64 if dtype == _lib.KMVP_F64 else np.float32
    rs = np.random.RandomState(14)
    y, x = rounded(rs.rand(301, 3), precision), rounded(rs.rand(130, 3), precision)
    clean = rounded(rs.randn(301, 3), precision)
    want = lse_grad_reference.gradient(kernel=kernel, source_points=y, target_points=x, source_signal=clean)
    tol, own = tolerance(kernel, y, x, clean, precision, want)
    for options in ((), (("segments", 3),)):
        base = ctx_grad(kernel, y, x, clean, dtype, options=options)
        check(base, want, tol, f"{kernel} clean log-weights {options}")
        for j in (1, 150, 300):
            c = clean.copy()
            c[j, 0] = np.nan
            c[j, 1] = np.inf
            ref = lse_grad_reference.gradient(kernel=kernel, source_points=y, target_points=x, source_signal=c)
            assert not np.isfinite(ref[:, :2]).any()  # the restatement keeps the convention too
            got = ctx_grad(kernel, y, x, c, dtype, options=options)
            assert not np.isfinite(got[:, 0]).any(), (kernel, j, "c = NaN", got[:, 0][np.isfinite(got[:, 0]).any(axis=-1)][:3])
            assert not np.isfinite(got[:, 1]).any(), (kernel, j, "c = +inf", got[:, 1][np.isfinite(got[:, 1]).any(axis=-1)][:3])
            assert np.array_equal(got[:, 2], base[:, 2]), (kernel, j)


@pytest.mark.parametrize("kernel", KERNELS)
def test_logsumexp_gradient_of_targets_at_1e20(kernel):
    """float32: every squared distance overflows to inf, no pair is live: NaN everywhere (where the log-sum-exp is -inf).
    The same cloud in float64 is finite and meets the restatement."""
    rs = np.random.RandomState(12)
    y = rounded(rs.rand(70, 3), np.float32)
    x = rounded(rounded(rs.rand(9, 3) + 1.0, np.float32) * 1e20, np.float32)
    c = rounded(rs.randn(70, 2), np.float32)
    got32 = ctx_grad(kernel, y, x, c, _lib.KMVP_F32)
    assert np.isnan(got32).all(), got32
    assert np.isneginf(ctx_lse(kernel, y, x, c, _lib.KMVP_F32)).all()
    want = lse_grad_reference.gradient(kernel=kernel, source_points=y, target_points=x, source_signal=c)
    assert np.isfinite(want).all()
    check(ctx_grad(kernel, y, x, c, _lib.KMVP_F64), want, TOL64, f"{kernel} float64, targets at 1e20")


@pytest.mark.parametrize("dtype", (_lib.KMVP_F32, _lib.KMVP_F64), ids=("float32", "float64"))
def test_own_and_duplicated_pairs_of_exp_minus_r(dtype):
    """same_points with exp(-r): the own pair (s == 0) drops out of the numerator and keeps its weight in the denominator,
    so every row is finite; duplicated source points count twice, and a target ON a duplicated source is finite too.
    M = 70 leaves pad records in the last batch, next to the coincident pairs."""
    precision = np.float64 if dtype == _lib.KMVP_F64 else np.float32
    rs = np.random.RandomState(13)
    y = rounded(rs.rand(70, 2), precision)
    y[[9, 40, 69]] = y[3]
    c = rounded(rs.randn(70, 2), precision)
    for kernel in KERNELS:
        want = lse_grad_reference.gradient(kernel=kernel, source_points=y, source_signal=c)
        assert np.isfinite(want).all()
        got = ctx_grad(kernel, y, None, c, dtype)
        assert np.isfinite(got).all()
        tol, own = tolerance(kernel, y, None, c, precision, want)
        check(got, want, tol, f"{kernel} same points with duplicates (own {own:.1e})")
        assert np.array_equal(got[9], got[3]) and np.array_equal(got[69], got[3])
    # one isolated point: only its own pair is live at float32 range -- the gradient is 0 / weight = 0, not NaN
    far = np.vstack([y, [[3.0e4, 3.0e4]]])
    got = ctx_grad("absolute-exponential", far, None, None, dtype)
    assert np.isfinite(got).all() and np.all(got[70] == 0.0), got[70]


# ---- reproducibility, layouts ------------------------------------------------------------------------------------------
def test_logsumexp_gradient_is_bitwise_reproducible():
    rs = np.random.RandomState(31)
    y, x, c = rs.rand(5001, 3) * 4.0, rs.rand(1000, 3) * 4.0, rs.randn(5001, 2)
    for kernel in KERNELS:
        for dtype in (_lib.KMVP_F32, _lib.KMVP_F64):
            for seg in (0, 5):
                first = ctx_grad(kernel, y, x, c, dtype, options=(("segments", seg),))
                again = ctx_grad(kernel, y, x, c, dtype, options=(("segments", seg),))
                assert np.array_equal(first, again), (kernel, dtype, seg)


ORDERS = (("product", "grad", "lse", "lsegrad"), ("lsegrad", "lse", "grad", "product"), ("lse", "lsegrad", "product", "grad"),
          ("grad", "lsegrad", "lse", "product"), ("lsegrad", "product", "lsegrad", "lse", "grad"))


def test_the_four_reductions_share_the_packed_layouts():
    """A product, a gradient, a log-sum-exp and its gradient on one context, in several orders: the same answers (one pack
    serves all), and the log-sum-exp's own bits do not depend on whether its gradient ran on the context."""
    rs = np.random.RandomState(34)
    y, x, c = rs.rand(257, 3), rs.rand(193, 3), rs.randn(257, 2)
    for kernel in KERNELS:
        want = {"lse": lse_reference.logsumexp(kernel=kernel, source_points=y, target_points=x, source_signal=c),
                "lsegrad": lse_grad_reference.gradient(kernel=kernel, source_points=y, target_points=x, source_signal=c),
                "grad": grad_reference.gradient(kernel=kernel, source_points=y, target_points=x, source_signal=c).reshape(193, -1),
                "product": kmvp_oracle.product(kernel=kernel, source_points=y, target_points=x, source_signal=c)}
        alone = ctx_lse(kernel, y, x, c, _lib.KMVP_F64, options=(("fast_sqdists", 0),))
        first = None
        for order in ORDERS:
            ctx = _lib.Context(0)
            try:
                ctx.set_option("fast_sqdists", 0)
                ctx.set_points(y, x, _lib.KMVP_F64)
                ctx.set_signal(c)
                got = {}
                for what in order:
                    if what == "product":
                        ctx.run(kernel, False)
                        got[what] = ctx.get_result(193, 2)
                    elif what == "grad":
                        ctx.run_grad(kernel)
                        got[what] = ctx.get_result(193, 6)
                    elif what == "lse":
                        ctx.run_lse(kernel)
                        got[what] = ctx.get_result(193, 2)
                        assert ctx.last_kernel_name == "lowd_lse_kernel"
                    else:
                        ctx.run_lse_grad(kernel)
                        got[what] = ctx.get_result(193, 6).reshape(193, 2, 3)
                        assert ctx.last_kernel_name == NAME
            finally:
                ctx.close()
            assert grad_err(got["lsegrad"], want["lsegrad"]) <= TOL64, (kernel, order)
            assert np.max(np.abs(got["lse"] - want["lse"]) / np.maximum(1.0, np.abs(want["lse"]))) <= TOL64, (kernel, order)
            assert rel_err(got["grad"], want["grad"]) <= TOL64 and rel_err(got["product"], want["product"]) <= TOL64, (kernel, order)
            assert np.array_equal(got["lse"], alone), (kernel, order)
            if first is None:
                first = got
            for what in got:
                assert np.array_equal(got[what], first[what]), (kernel, order, what)


# ---- shards ------------------------------------------------------------------------------------------------------------
def test_logsumexp_gradient_shards_merge_with_softmax_weights():
    """Three partial_shard source slices with chunk = 16, the second with every c = -inf in column 1 (its G_s is NaN
    there and its L_s -inf: weight 0), merged by the caller as G = sum_s exp(L_s - L) G_s with the shards' L_s from the
    log-sum-exp, equal the whole.  A slice without a communicator and without the option is refused, like a product."""
    rs = np.random.RandomState(32)
    y, x, c = rs.rand(200, 3) * 3.0, rs.rand(450, 3) * 3.0, rs.randn(200, 2)
    c[5::7, 1] = -np.inf
    c[67:131, 1] = -np.inf
    slices = ((0, 67), (67, 131), (131, 200))
    opts = (("partial_shard", 1), ("chunk", 16))
    for kernel in KERNELS:
        whole = ctx_grad(kernel, y, x, c, _lib.KMVP_F64)
        want = lse_grad_reference.gradient(kernel=kernel, source_points=y, target_points=x, source_signal=c)
        check(whole, want, TOL64, f"{kernel} whole")
        Gs = [ctx_grad(kernel, y[lo:hi], x, c[lo:hi], _lib.KMVP_F64, j_offset=lo, M_total=200, options=opts) for lo, hi in slices]
        Ls = [ctx_lse(kernel, y[lo:hi], x, c[lo:hi], _lib.KMVP_F64, j_offset=lo, M_total=200, options=opts) for lo, hi in slices]
        assert np.isnan(Gs[1][:, 1]).all() and np.isneginf(Ls[1][:, 1]).all() and np.isfinite(Gs[1][:, 0]).all()
        L = np.logaddexp(np.logaddexp(Ls[0], Ls[1]), Ls[2])
        merged = np.zeros_like(whole)
        for G_s, L_s in zip(Gs, Ls):
            weight = np.exp(L_s - L)[:, :, None]
            merged += weight * np.where(weight > 0, G_s, 0.0)  # a shard without a live term: weight 0, G_s NaN
        err = grad_err(merged, whole)
        print(f"{kernel}: softmax-weighted merge of 3 shards vs whole {err:.2e}")
        assert err <= 1e-12, (kernel, err)
    with pytest.raises(_lib.KmvpError) as e:
        ctx_grad("gaussian", y[:67], x, c[:67], _lib.KMVP_F64, j_offset=0, M_total=200)
    assert e.value.code == 1


def test_logsumexp_gradient_through_a_communicator_of_one_rank():
    """kmvp_comm_init with world == 1: the canonical unpadded layouts, all-reduce(min) of the exponents, rescale, one
    all-reduce(sum).  The merge of one rank with itself changes nothing: bitwise equal to the plain run."""
    rs = np.random.RandomState(33)
    y, x, c = rs.rand(301, 2), rs.rand(130, 2), rs.randn(301, 3)
    c[:, 2] = -np.inf
    for kernel in KERNELS:
        plain = ctx_grad(kernel, y, x, c, _lib.KMVP_F64)
        through = ctx_grad(kernel, y, x, c, _lib.KMVP_F64, comm=True)
        want = lse_grad_reference.gradient(kernel=kernel, source_points=y, target_points=x, source_signal=c)
        check(through, want, TOL64, f"{kernel} through a communicator of one rank")
        assert np.array_equal(plain, through, equal_nan=True), kernel


def test_two_ranks_on_one_gpu():
    """The plugin with the sources sharded over two ranks through the host-staged exchange (kmvp_comm_init_host): an uneven
    split, float32 cases, and a rank with an EMPTY slice; the worker checks every case against the restatement on every
    rank, and that the ranks hold bitwise equal results."""
    out = _spawn([os.path.join(HERE, "_lse_grad_rank_worker.py")], world=2, timeout=300)
    rep = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
    print(json.dumps(rep))
    assert rep["world"] == 2 and len(rep["cases"]) == 6 and rep["ranks_bitwise_equal"], rep
    assert sum(1 for case in rep["cases"] if case["empty_slice"]) == 2, rep
    assert any(case["precision"] == "float32" for case in rep["cases"]), rep


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_c_abi_refusals():
    """bf16 context, D = 9, E = 5, fast_sqdists = 2: KMVP_E_UNSUPPORTED with a message that names the cause and an empty
    dispatch note; call-order errors: KMVP_E_INVALID."""
    rs = np.random.RandomState(35)

    def refused(y, c, dtype, options=()):
        ctx = _lib.Context(0)
        try:
            for key, value in options:
                ctx.set_option(key, value)
            ctx.set_points(np.ascontiguousarray(y, dtype=np.float32), None, dtype)
            ctx.set_signal(np.ascontiguousarray(c, dtype=np.float32))
            for kernel, entry in (("gaussian", "kmvp_gaussian_logsumexp_grad"),
                                  ("absolute-exponential", "kmvp_absexp_logsumexp_grad")):
                rc = getattr(ctx._lib, entry)(ctx._ctx)
                msg = ctx._lib.kmvp_last_error(ctx._ctx).decode()
                assert rc == 2 and msg and ctx.last_dispatch_note == "", (entry, rc, msg)
                with pytest.raises(_lib.KmvpError) as e:
                    ctx.run_lse_grad(kernel)
                assert e.value.code == 2
        finally:
            ctx.close()
        return msg

    assert "bfloat16" in refused(rs.rand(64, 16), rs.randn(64, 1), _lib.KMVP_BF16)
    assert "D = 9" in refused(rs.rand(64, 9), rs.randn(64, 1), _lib.KMVP_F32)
    assert "E = 5" in refused(rs.rand(64, 3), rs.randn(64, 5), _lib.KMVP_F32)
    assert "fast_sqdists = 2" in refused(rs.rand(64, 3), rs.randn(64, 1), _lib.KMVP_F32, options=(("fast_sqdists", 2),))
    ctx = _lib.Context(0)
    try:
        assert ctx._lib.kmvp_gaussian_logsumexp_grad(ctx._ctx) == 1  # no points
        ctx.set_points(np.ascontiguousarray(rs.rand(64, 3), dtype=np.float32), None, _lib.KMVP_F32)
        assert ctx._lib.kmvp_absexp_logsumexp_grad(ctx._ctx) == 1  # no signal
        assert ctx._lib.kmvp_last_error(ctx._ctx)
        with pytest.raises(NotImplementedError):  # the other kernels have no entry point
            ctx.run_lse_grad("inverse-distance")
    finally:
        ctx.close()


# ---- end to end --------------------------------------------------------------------------------------------------------
def test_barycentric_map_after_sinkhorn_iterations_matches_numpy():
    """The setting of test_gpu_lse.py::test_sinkhorn_iterations_match_numpy (n = 300, D = 3, eps = 0.05, float64, ONE
    context, 20 symmetric iterations), then ONE query_logsumexp_gradient(): with the points scaled by 1 / sqrt(eps),
    G_i = -2 (x'_i - ybar'_i), so the barycentric map is T(x_i) = sqrt(eps) (x'_i + G_i / 2).  It equals numpy's
    sum_j pi_ij y_j / sum_j pi_ij of the same loop in numpy to 1e-9."""
    n, eps = 300, 0.05
    rs = np.random.RandomState(41)
    pts = rs.rand(n, 3)
    beta = rs.rand(n) + 0.5
    beta /= beta.sum()
    scaled = pts / np.sqrt(eps)
    cost = np.sum((pts[:, None, :] - pts[None, :, :]) ** 2, axis=-1)

    algo = MI355XProduct(kernel="gaussian", dimension=3, precision=np.float64)
    f_gpu, f_np = np.zeros(n), np.zeros(n)
    try:
        algo.prepare_data(source_points=scaled, target_points=scaled, same_points=True)
        algo.fit()
        for _ in range(20):
            algo.prepare_query(source_signal=(f_gpu / eps + np.log(beta)).reshape(-1, 1))
            algo.query_logsumexp()
            f_gpu = 0.5 * (f_gpu - eps * algo.get_logsumexp()[:, 0])
            f_np = 0.5 * (f_np - eps * np.logaddexp.reduce((f_np[None, :] - cost) / eps + np.log(beta)[None, :], axis=1))
        algo.prepare_query(source_signal=(f_gpu / eps + np.log(beta)).reshape(-1, 1))
        algo.query_logsumexp_gradient()
        G = algo.get_logsumexp_gradient()
        assert algo.get_additional()["device_kernel"] == NAME
    finally:
        algo.done()
    assert G.shape == (n, 1, 3)
    T_gpu = np.sqrt(eps) * (scaled + G[:, 0, :] / 2)
    log_pi = (f_np[:, None] + f_np[None, :] - cost) / eps + np.log(beta)[None, :]
    pi = np.exp(log_pi - log_pi.max(axis=1, keepdims=True))
    T_np = pi @ pts / pi.sum(axis=1, keepdims=True)
    err = float(np.max(np.abs(T_gpu - T_np)))
    print(f"barycentric map after 20 Sinkhorn iterations: differs from numpy's by {err:.2e} "
          f"(displacement up to {np.max(np.abs(T_np - pts)):.3f})")
    assert np.isfinite(T_gpu).all() and err <= 1e-9, err
