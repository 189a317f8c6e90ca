"""GPU tests of the log-sum-exp reduction (lowd_lse_kernel, include/kmvp.h kmvp_<kernel>_logsumexp) against the numpy
restatement of its definition (lse_reference.py, itself checked against numpy.logaddexp.reduce in test_lse_reference.py).

The measure is, per row and column, |L - L_ref| / max(1, |L_ref|), with the project's tolerances:
  float64            <= 1e-11
  float32 / float16  <= max(1e-5, 2 x the restatement's own float32 error on the same (rounded) inputs)
Rows that are -inf or NaN in the restatement must be exactly that on the GPU, and no other row may be.
"""
import json
import os

import numpy as np
import pytest

import kmvp_oracle
import lse_reference
from conftest import rel_err
from kernel_matrix_benchmarks_amd import _lib
from kernel_matrix_benchmarks_amd.algorithms.mi355x import MI355XProduct
from test_gpu_multirank import _spawn

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

TOL64 = 1e-11
TOL32 = 1e-5
KERNELS = lse_reference.KERNELS
PRECISIONS = (np.float64, np.float32, np.float16)


def rounded(a, precision):
    return None if a is None else np.asarray(a, dtype=precision).astype(np.float64)


def lse_err(got, want):
    """max over the finite entries of the reference of |L - L_ref| / max(1, |L_ref|); the others must be identical
    (-inf where -inf, NaN where NaN) and no finite entry of the reference may be non-finite in the result."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    fin = np.isfinite(want)
    same_class = (np.isnan(got) == np.isnan(want)) & (np.isneginf(got) == np.isneginf(want)) & (np.isfinite(got) == fin)
    bad = np.argwhere(~same_class)
    assert same_class.all(), ("-inf / NaN entries differ", bad[:8].tolist(), got[~same_class][:8], want[~same_class][:8])
    if not fin.any():
        return 0.0
    return float(np.max(np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin]))))


def tolerance(kernel, y, x, c, precision, want, rows=None):
    """The float32 rule: the restatement run in float32 on the same inputs sets the scale of what float32 can do."""
    if np.dtype(precision) == np.float64:
        return TOL64, 0.0
    own = lse_reference.logsumexp(kernel=kernel, source_points=y, target_points=x, source_signal=c, precision=np.float32,
                                  rows=rows)
    fin = np.isfinite(want) & np.isfinite(own)
    own_err = float(np.max(np.abs(own[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin])))) if fin.any() else 0.0
    return max(TOL32, 2 * own_err), own_err


def check(got, want, tol, label):
    err = lse_err(got, want)
    print(f"{label}: err {err:.3e} (tolerance {tol:.1e}, {int((~np.isfinite(want)).sum())} non-finite entries)")
    assert err <= tol, (label, err, tol)
    return err


def plugin_lse(kernel, y, x, c, precision, **options):
    """The runner's call order with query_logsumexp() / get_logsumexp() in the place of query() / get_result()."""
    algo = MI355XProduct(kernel=kernel, dimension=y.shape[1], precision=precision, **options)
    try:
        algo.prepare_data(source_points=y, target_points=y if x is None else x, same_points=x is None,
                          density_estimation=c is None)
        algo.fit()
        algo.prepare_query(source_signal=c)
        algo.query_logsumexp()
        L = algo.get_logsumexp()
        extra = algo.get_additional()
    finally:
        algo.done()
    N = y.shape[0] if x is None else x.shape[0]
    assert L.shape == (N, 1 if c is None else c.shape[1])
    assert L.dtype == np.float64 and L.flags["C_CONTIGUOUS"]
    assert extra["device_kernel"] == "lowd_lse_kernel" and extra["dispatch_note"] == "", extra
    return L


def ctx_lse(kernel, y, x, c, dtype, *, options=(), j_offset=0, M_total=None, comm=False):
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
        ctx.run_lse(kernel)
        if y.shape[0] > 0 and N > 0:
            assert ctx.last_kernel_name == "lowd_lse_kernel" and ctx.last_dispatch_note == ""
            assert ctx.last_kernel_ms > 0 and ctx.last_total_ms >= ctx.last_kernel_ms
        return ctx.get_result(N, 1 if c is None else c.shape[1])
    finally:
        ctx.close()


# ---- parity ------------------------------------------------------------------------------------------------------------
SHAPES = ((1, 1), (63, 3), (65, 5), (300, 257))  # (N, M): one pair, below / above a 64-target tile, a ragged batch of sources


@pytest.mark.parametrize("precision", PRECISIONS, ids=[np.dtype(p).name for p in PRECISIONS])
@pytest.mark.parametrize("kernel", KERNELS)
def test_logsumexp_parity(kernel, precision):
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
                    want = lse_reference.logsumexp(kernel=kernel, source_points=y, target_points=x, source_signal=c)
                    got = plugin_lse(kernel, y, x, c, precision)
                    tol, own = tolerance(kernel, y, x, c, precision, want)
                    label = f"{kernel} {np.dtype(precision).name} D={D} E={E} N={M if same else N} M={M} same={same}"
                    err = lse_err(got, want)
                    assert err <= tol, (label, err, tol, own)
                    worst = max(worst, err / tol)
    print(f"{kernel} {np.dtype(precision).name}: worst err / tolerance over 96 cases {worst:.3f}")


# ---- several segments and chunks, the shift rising throughout or never -------------------------------------------------
_SEG = {}


def segment_case(kernel):
    """N = 1000 targets in a small cluster, M = 5001 sources at distances 0 .. ~45 from it (Gaussian logits down to -2000),
    E = 2; the restatement once per kernel."""
    if kernel not in _SEG:
        rs = np.random.RandomState(77)
        x = rounded(rs.rand(1000, 3) * 0.5, np.float32)
        direction = rs.randn(5001, 3)
        direction /= np.linalg.norm(direction, axis=1, keepdims=True)
        y = rounded(0.25 + direction * (rs.rand(5001, 1) * 45.0), np.float32)
        c = rounded(rs.randn(5001, 2), np.float32)
        near_first = np.argsort(np.linalg.norm(y - 0.25, axis=1), kind="stable")
        want = lse_reference.logsumexp(kernel=kernel, source_points=y, target_points=x, source_signal=c)
        own = lse_reference.logsumexp(kernel=kernel, source_points=y, target_points=x, source_signal=c, precision=np.float32)
        _SEG[kernel] = (y, x, c, near_first, want, own)
    return _SEG[kernel]


@pytest.mark.parametrize("dtype", (_lib.KMVP_F32, _lib.KMVP_F64), ids=("float32", "float64"))
@pytest.mark.parametrize("kernel", KERNELS)
def test_logsumexp_on_several_segments_and_chunks(kernel, dtype):
    """segments = 3, chunk = 256: sources nearest-LAST (the shift rises throughout the loop) and nearest-FIRST (it never
    rises after the first batch) both meet the restatement; 1 and 8 segments agree with 3 within the tolerance."""
    y, x, c, near_first, want, own = segment_case(kernel)
    if dtype == _lib.KMVP_F64:
        tol = TOL64
    else:
        tol = max(TOL32, 2 * float(np.max(np.abs(own - want) / np.maximum(1.0, np.abs(want)))))
    runs = {}
    for name, order in (("nearest-last", near_first[::-1]), ("nearest-first", near_first)):
        got = ctx_lse(kernel, y[order], x, c[order], dtype, options=(("segments", 3), ("chunk", 256)))
        check(got, want, tol, f"{kernel} {name} segments=3 chunk=256")
        runs[name] = got
    for seg in (1, 8):
        other = ctx_lse(kernel, y[near_first[::-1]], x, c[near_first[::-1]], dtype, options=(("segments", seg), ("chunk", 256)))
        check(other, want, tol, f"{kernel} nearest-last segments={seg}")
        err = lse_err(other, runs["nearest-last"])
        print(f"{kernel}: segments={seg} against segments=3: {err:.3e}")
        assert err <= tol, (kernel, seg, err, tol)


# ---- the reason for the feature ----------------------------------------------------------------------------------------
def test_logsumexp_where_the_product_underflows():
    """Targets at distance ~100 from a unit cloud, float32: query() is exactly 0, the log-sum-exp is finite, near -1e4 and
    within tolerance.  Near the cloud, where nothing underflows, exp(L) is the plain product with b = exp(c): both meet the
    float32 rule against the float64 product."""
    rs = np.random.RandomState(5)
    y = rounded(rs.rand(500, 3), np.float32)
    c = rounded(rs.randn(500, 2), np.float32)
    x_far = rounded(rs.rand(200, 3) + np.array([100.0, 0.0, 0.0]), np.float32)
    x_near = rounded(rs.rand(200, 3) + 0.5, np.float32)
    b = np.exp(c)

    def product(x):
        algo = MI355XProduct(kernel="gaussian", dimension=3, precision=np.float32, fast_sqdists=False)
        try:
            algo.prepare_data(source_points=y, target_points=x, same_points=False)
            algo.fit()
            algo.prepare_query(source_signal=b)
            algo.query()
            return algo.get_result()
        finally:
            algo.done()

    assert np.all(product(x_far) == 0.0)
    want = lse_reference.logsumexp(kernel="gaussian", source_points=y, target_points=x_far, source_signal=c)
    got = plugin_lse("gaussian", y, x_far, c, np.float32)
    assert np.isfinite(got).all() and got.max() < -9.5e3 and got.min() > -1.05e4, (got.min(), got.max())
    tol, own = tolerance("gaussian", y, x_far, c, np.float32, want)
    check(got, want, tol, f"gaussian float32, targets at distance 100 (restatement's own float32 error {own:.1e})")

    b32 = rounded(b, np.float32)
    truth = kmvp_oracle.product(kernel="gaussian", source_points=y, target_points=x_near, source_signal=b32)
    own_p = rel_err(kmvp_oracle.product(kernel="gaussian", source_points=y, target_points=x_near, source_signal=b32,
                                        precision=np.float32), truth)
    tol_p = max(TOL32, 2 * own_p)
    e_prod = rel_err(product(x_near), truth)
    # exp(L) is about b = exp(c) exactly; the product was handed exp(c) rounded to float32 (2^-24 relative per weight)
    e_lse = rel_err(np.exp(plugin_lse("gaussian", y, x_near, c, np.float32)), truth)
    print(f"near the cloud: product rel_err {e_prod:.2e}, exp(L) rel_err {e_lse:.2e} (tolerance {tol_p:.1e})")
    assert e_prod <= tol_p and e_lse <= tol_p, (e_prod, e_lse, tol_p)


# ---- conventions -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", (_lib.KMVP_F32, _lib.KMVP_F64), ids=("float32", "float64"))
@pytest.mark.parametrize("kernel", KERNELS)
def test_logsumexp_conventions(kernel, dtype):
    precision = np.float64 if dtype == _lib.KMVP_F64 else np.float32
    rs = np.random.RandomState(11)
    y, x = rounded(rs.rand(301, 3), precision), rounded(rs.rand(130, 3), precision)
    # some c = -inf, a column that is all -inf, a column spanning +-1e3
    c = rounded(rs.randn(301, 4), precision)
    c[::3, 0] = -np.inf
    c[:, 1] = -np.inf
    c[:, 2] = rounded(rs.uniform(-1e3, 1e3, 301), precision)
    want = lse_reference.logsumexp(kernel=kernel, source_points=y, target_points=x, source_signal=c)
    assert np.isneginf(want[:, 1]).all() and np.isfinite(want[:, [0, 2, 3]]).all()
    got = ctx_lse(kernel, y, x, c, dtype)
    tol, own = tolerance(kernel, y, x, c, precision, want)
    check(got, want, tol, f"{kernel} c = -inf entries, an all -inf column, c spanning +-1e3 (own {own:.1e})")
    assert np.isneginf(got[:, 1]).all()
    # every c = -inf and no source at all: exactly -inf everywhere
    assert np.isneginf(ctx_lse(kernel, y, x, np.full((301, 2), -np.inf), dtype)).all()
    empty = ctx_lse(kernel, y[:0], x, c[:0], dtype)
    assert empty.shape == (130, 4) and np.isneginf(empty).all()
    # a NaN target coordinate: that row NaN in every column (the all -inf column included), no other row
    xn = x.copy()
    xn[77, 2] = np.nan
    gn = ctx_lse(kernel, y, xn, c, dtype)
    assert np.isnan(gn[77]).all(), gn[77]
    assert np.array_equal(np.delete(gn, 77, axis=0), np.delete(got, 77, axis=0))
    # logits around -1e4 (float32) / -1e6 (float64): never exp(max logit)
    shift = {("gaussian", _lib.KMVP_F32): 1e2, ("gaussian", _lib.KMVP_F64): 1e3,
             ("absolute-exponential", _lib.KMVP_F32): 1e4, ("absolute-exponential", _lib.KMVP_F64): 1e6}[(kernel, dtype)]
    x_far = rounded(x + np.array([shift, 0.0, 0.0]), precision)
    want_far = lse_reference.logsumexp(kernel=kernel, source_points=y, target_points=x_far, source_signal=c[:, [0, 3]])
    assert np.isfinite(want_far).all() and want_far.max() < -0.9 * (1e4 if dtype == _lib.KMVP_F32 else 1e6)
    tol, own = tolerance(kernel, y, x_far, c[:, [0, 3]], precision, want_far)
    check(ctx_lse(kernel, y, x_far, c[:, [0, 3]], dtype), want_far, tol, f"{kernel} logits near {want_far.mean():.3g} (own {own:.1e})")


@pytest.mark.parametrize("kernel", KERNELS)
def test_logsumexp_of_targets_at_1e20(kernel):
    """float32: every squared distance overflows to inf, every pair is at infinite distance: exactly -inf.  The same cloud
    in float64 is finite and meets the restatement."""
    rs = np.random.RandomState(12)
    y = rounded(rs.rand(70, 3), np.float32)
    x = rounded(rs.rand(9, 3) + 1.0, np.float32) * 1e20
    x = rounded(x, np.float32)
    c = rounded(rs.randn(70, 2), np.float32)
    got32 = ctx_lse(kernel, y, x, c, _lib.KMVP_F32)
    assert np.isneginf(got32).all(), got32
    want = lse_reference.logsumexp(kernel=kernel, source_points=y, target_points=x, source_signal=c)
    assert np.isfinite(want).all()
    check(ctx_lse(kernel, y, x, c, _lib.KMVP_F64), want, TOL64, f"{kernel} float64, targets at 1e20")


# ---- reproducibility, layouts ------------------------------------------------------------------------------------------
def test_logsumexp_is_bitwise_reproducible():
    rs = np.random.RandomState(31)
    y, x, c = rs.rand(5001, 3) * 4.0, rs.rand(1000, 3) * 4.0, rs.randn(5001, 2)
    for kernel in KERNELS:
        for dtype in (_lib.KMVP_F32, _lib.KMVP_F64):
            for seg in (0, 5):
                first = ctx_lse(kernel, y, x, c, dtype, options=(("segments", seg),))
                again = ctx_lse(kernel, y, x, c, dtype, options=(("segments", seg),))
                assert np.array_equal(first, again), (kernel, dtype, seg)


def test_product_gradient_and_logsumexp_share_the_packed_layouts():
    """A product, a gradient and a log-sum-exp on one context, in every order: the same answers (one pack serves all)."""
    import itertools

    import grad_reference

    rs = np.random.RandomState(34)
    y, x, c = rs.rand(257, 3), rs.rand(193, 3), rs.randn(257, 2)
    for kernel in KERNELS:
        want = {"lse": lse_reference.logsumexp(kernel=kernel, source_points=y, target_points=x, source_signal=c),
                "grad": grad_reference.gradient(kernel=kernel, source_points=y, target_points=x, source_signal=c).reshape(193, -1),
                "product": kmvp_oracle.product(kernel=kernel, source_points=y, target_points=x, source_signal=c)}
        first = None
        for order in itertools.permutations(("product", "grad", "lse")):
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
                    else:
                        ctx.run_lse(kernel)
                        got[what] = ctx.get_result(193, 2)
            finally:
                ctx.close()
            assert lse_err(got["lse"], want["lse"]) <= TOL64, (kernel, order)
            assert rel_err(got["grad"], want["grad"]) <= TOL64 and rel_err(got["product"], want["product"]) <= TOL64, (kernel, order)
            if first is None:
                first = got
            for what in got:
                assert np.array_equal(got[what], first[what]), (kernel, order, what)


# ---- shards ------------------------------------------------------------------------------------------------------------
def test_logsumexp_shards_merge_with_logaddexp():
    """Three partial_shard source slices, merged by the caller with logaddexp, equal the whole; a small chunk as well.  A
    slice without a communicator and without the option is refused, like a product."""
    rs = np.random.RandomState(32)
    y, x, c = rs.rand(200, 3) * 3.0, rs.rand(450, 3) * 3.0, rs.randn(200, 2)
    c[5::7, 1] = -np.inf
    for kernel in KERNELS:
        whole = ctx_lse(kernel, y, x, c, _lib.KMVP_F64)
        want = lse_reference.logsumexp(kernel=kernel, source_points=y, target_points=x, source_signal=c)
        check(whole, want, TOL64, f"{kernel} whole")
        parts = [ctx_lse(kernel, y[lo:hi], x, c[lo:hi], _lib.KMVP_F64, j_offset=lo, M_total=200,
                         options=(("partial_shard", 1), ("chunk", 16)))
                 for lo, hi in ((0, 67), (67, 131), (131, 200))]
        merged = np.logaddexp(np.logaddexp(parts[0], parts[1]), parts[2])
        err = lse_err(merged, whole)
        print(f"{kernel}: logaddexp of 3 shards vs whole {err:.2e}")
        assert err <= 1e-12, (kernel, err)
    with pytest.raises(_lib.KmvpError) as e:
        ctx_lse("gaussian", y[:67], x, c[:67], _lib.KMVP_F64, j_offset=0, M_total=200)
    assert e.value.code == 1


def test_logsumexp_through_a_communicator_of_one_rank():
    """kmvp_comm_init with world == 1: the canonical unpadded layout, all-reduce(min) of the exponents, rescale,
    all-reduce(sum).  The merge of one rank with itself changes nothing: bitwise equal to the plain run."""
    rs = np.random.RandomState(33)
    y, x, c = rs.rand(301, 2), rs.rand(130, 2), rs.randn(301, 3)
    for kernel in KERNELS:
        plain = ctx_lse(kernel, y, x, c, _lib.KMVP_F64)
        through = ctx_lse(kernel, y, x, c, _lib.KMVP_F64, comm=True)
        want = lse_reference.logsumexp(kernel=kernel, source_points=y, target_points=x, source_signal=c)
        check(through, want, TOL64, f"{kernel} through a communicator of one rank")
        assert np.array_equal(plain, through), kernel


def test_two_ranks_on_one_gpu():
    """The plugin with the sources sharded over two ranks through the host-staged exchange (kmvp_comm_init_host): an uneven
    split, the spatially ordered float32 Gaussian, and a rank with an EMPTY slice; the worker checks every case against
    the restatement on every rank, and that the ranks hold bitwise equal results."""
    out = _spawn([os.path.join(HERE, "_lse_rank_worker.py")], world=2, timeout=300)
    rep = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
    print(json.dumps(rep))
    assert rep["world"] == 2 and len(rep["cases"]) == 6 and rep["ranks_bitwise_equal"], rep
    assert sum(1 for case in rep["cases"] if case["empty_slice"]) == 2, rep


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_c_abi_refusals():
    """bf16 context, D = 9, E = 5, fast_sqdists = 2: KMVP_E_UNSUPPORTED with a message and an empty dispatch note;
    call-order errors: KMVP_E_INVALID."""
    rs = np.random.RandomState(35)

    def refused(y, c, dtype, options=()):
        ctx = _lib.Context(0)
        try:
            for key, value in options:
                ctx.set_option(key, value)
            ctx.set_points(np.ascontiguousarray(y, dtype=np.float32), None, dtype)
            ctx.set_signal(np.ascontiguousarray(c, dtype=np.float32))
            for kernel, entry in (("gaussian", "kmvp_gaussian_logsumexp"), ("absolute-exponential", "kmvp_absexp_logsumexp")):
                rc = getattr(ctx._lib, entry)(ctx._ctx)
                msg = ctx._lib.kmvp_last_error(ctx._ctx).decode()
                assert rc == 2 and msg and ctx.last_dispatch_note == "", (entry, rc, msg)
                with pytest.raises(_lib.KmvpError) as e:
                    ctx.run_lse(kernel)
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
        assert ctx._lib.kmvp_gaussian_logsumexp(ctx._ctx) == 1  # no points
        ctx.set_points(np.ascontiguousarray(rs.rand(64, 3), dtype=np.float32), None, _lib.KMVP_F32)
        assert ctx._lib.kmvp_absexp_logsumexp(ctx._ctx) == 1  # no signal
        assert ctx._lib.kmvp_last_error(ctx._ctx)
        with pytest.raises(NotImplementedError):  # the other kernels have no entry point
            ctx.run_lse("inverse-distance")
    finally:
        ctx.close()


# ---- end to end --------------------------------------------------------------------------------------------------------
def test_sinkhorn_iterations_match_numpy():
    """20 symmetric Sinkhorn iterations (entropic optimal transport of a cloud with itself, C = |x - y|^2), n = 300, D = 3,
    eps = 0.05, float64: the points scaled by 1 / sqrt(eps), c = g / eps + log beta, a new c every iteration on ONE context
    (prepare_query only).  The potentials agree with the same loop in numpy to 1e-9."""
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
    finally:
        algo.done()
    err = float(np.max(np.abs(f_gpu - f_np)))
    print(f"Sinkhorn, 20 symmetric iterations: potentials differ by {err:.2e} (|f| up to {np.max(np.abs(f_np)):.3f})")
    assert np.isfinite(f_gpu).all() and err <= 1e-9, err
