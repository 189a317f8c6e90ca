"""GPU tests of the derivative of the product in the logarithm of a per-axis length scale (lowd_dscale_kernel,
include/kmvp.h kmvp_<kernel>_dscale) against the float64 numpy restatement of its definition (dscale_reference.py, itself
checked against central differences of the pinned oracle in test_dscale_reference.py), and of the Gaussian-process
likelihood gradient MI355XSolver builds on it against dense float64 numpy.

Tolerances are the project's own, in conftest.rel_err over flattened (E D) rows:
  float64  <= 1e-11
  float32  <= max(1e-5, 2 x the restatement's own float32 error on the case), on the float32-rounded inputs
"""
import json
import os

import numpy as np
import pytest

import dscale_reference as dref
import golden_cases
import grad_reference
import kmvp_oracle
import matern_reference
from conftest import rel_err
from kernel_matrix_benchmarks_amd import _lib
from kernel_matrix_benchmarks_amd.algorithms.mi355x import MI355XProduct, MI355XSolver
from test_gpu_multirank import _spawn

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TOL64 = 1e-11
TOL32 = 1e-5
KERNELS = dref.KERNELS
# the shapes of the golden product cases (the Gaussian's list: it has every shape, the duplicate-point case included) the
# kernel is built for, each with the four kernels
SHAPES = [c for c in golden_cases.product_cases()
          if c["kernel"] == "gaussian" and not c["normalize_rows"] and c["D"] <= 8 and c["E"] <= 4]
CASES = [dict(c, kernel=k, name=c["name"].replace("gaussian", k)) for k in KERNELS for c in SHAPES]


def rounded(a, precision):
    return None if a is None else np.asarray(a, dtype=precision).astype(np.float64)


def plugin_dscale(kernel, y, x, b, precision, **options):
    """The runner's call order with query_scale_derivative() / get_scale_derivative() in the place of query() /
    get_result()."""
    algo = MI355XProduct(kernel=kernel, dimension=y.shape[1], precision=precision, **options)
    try:
        algo.prepare_data(source_points=y, target_points=y if x is None else x, same_points=x is None,
                          density_estimation=b is None)
        algo.fit()
        algo.prepare_query(source_signal=b)
        algo.query_scale_derivative()
        H = algo.get_scale_derivative()
        extra = algo.get_additional()
    finally:
        algo.done()
    N = y.shape[0] if x is None else x.shape[0]
    assert H.shape == (N, 1 if b is None else b.shape[1], y.shape[1])
    assert H.dtype == np.float64 and H.flags["C_CONTIGUOUS"]
    assert extra["device_kernel"] == "lowd_dscale_kernel" and extra["dispatch_note"] == ""
    return H


def tolerance(kernel, y, x, b, precision, want, rows=None):
    """The float32 rule: the restatement run in float32 on the same inputs sets the scale of what float32 can do."""
    if np.dtype(precision) == np.float64:
        return TOL64, 0.0
    own = dref.scale_derivative(kernel=kernel, source_points=y, target_points=x, source_signal=b, precision=np.float32, rows=rows)
    own_err = rel_err(own.reshape(len(own), -1), want.reshape(len(want), -1))
    return max(TOL32, 2 * own_err), own_err


def check(got, want, tol, label):
    n = want.shape[0]
    assert np.isfinite(got).all(), label
    err = rel_err(got.reshape(n, -1), want.reshape(n, -1))
    print(f"{label}: rel_err {err:.3e} (tolerance {tol:.1e})")
    assert err <= tol, (label, err, tol)
    return err


@pytest.mark.parametrize("precision", (np.float64, np.float32), ids=("float64", "float32"))
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_dscale_parity(case, precision):
    """Same / different points, density, ragged N and M, D = 1 .. 8, E = 1 .. 4, the coincident-pair case."""
    y, x, b = (rounded(a, precision) for a in golden_cases.make_inputs(case))
    want = dref.scale_derivative(kernel=case["kernel"], source_points=y, target_points=x, source_signal=b)
    got = plugin_dscale(case["kernel"], y, x, b, precision)
    tol, own = tolerance(case["kernel"], y, x, b, precision, want)
    check(got, want, tol, f"{case['name']} {np.dtype(precision).name} (restatement's own float32 error {own:.1e})")


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("E", (1, 4))
def test_dscale_on_a_cloud_of_several_segments_and_chunks(kernel, E):
    """N = 20 000 targets != M = 30 001 sources (M = 1 mod 4: pad records in the last batch), D = 3, float32, with the
    explicit options segments = 6 and chunk = 1024: tile, segment and chunk boundaries are all crossed; the restatement
    on 512 seeded rows."""
    rs = np.random.RandomState(4048 + E)
    y, x, b = (rounded(a, np.float32) for a in (rs.rand(30001, 3), rs.rand(20000, 3), rs.randn(30001, E)))
    rows = np.sort(rs.choice(20000, 512, replace=False))
    want = dref.scale_derivative(kernel=kernel, source_points=y, target_points=x, source_signal=b, rows=rows)
    got = plugin_dscale(kernel, y, x, b, np.float32, segments=6, chunk=1024)[rows]
    tol, own = tolerance(kernel, y, x, b, np.float32, want, rows=rows)
    check(got, want, tol, f"{kernel} N=20000 M=30001 E={E} float32 (restatement's own float32 error {own:.1e})")


@pytest.mark.parametrize("precision", (np.float64, np.float32), ids=("float64", "float32"))
@pytest.mark.parametrize("kernel", ("absolute-exponential", "matern-3/2", "matern-5/2"))
def test_coincident_pairs_contribute_zero(kernel, precision):
    """same_points with two duplicated points: rows finite and equal to the restatement; the own pair (and the
    duplicate) contributes 0 -- the row of point 5 is what the sources without 5 and 40 give."""
    rs = np.random.RandomState(41)
    y, b = rounded(rs.rand(193, 3), precision), rounded(rs.randn(193, 2), precision)
    y[40], y[100] = y[5], y[7]
    want = dref.scale_derivative(kernel=kernel, source_points=y, source_signal=b)
    got = plugin_dscale(kernel, y, None, b, precision)
    tol, own = tolerance(kernel, y, None, b, precision, want)
    check(got, want, tol, f"{kernel} duplicates {np.dtype(precision).name}")
    keep = ~np.isin(np.arange(193), (5, 40))
    others = plugin_dscale(kernel, y[keep], y[5:6], b[keep], precision)
    check(got[5:6], others, tol, f"{kernel} row 5 without its coincident sources {np.dtype(precision).name}")


@pytest.mark.parametrize("kernel", KERNELS)
def test_a_source_at_float32_overflow_distance_contributes_exactly_zero(kernel):
    """|x - y|^2 overflows float32 although x - y is finite: the far source alone gives exactly 0 (not NaN from
    0 * inf), in a guarded batch (M = 1) and in an unguarded one (first of 64 records, the rest with signal 0)."""
    rs = np.random.RandomState(42)
    x = rounded(rs.rand(130, 3), np.float32)
    far = np.array([[3e19, 0.5, 0.5]], dtype=np.float32).astype(np.float64)
    alone = plugin_dscale(kernel, far, x, np.array([[1e3, -1e3]]), np.float32)
    assert (alone == 0).all(), kernel
    y = np.concatenate((far, rounded(rs.rand(63, 3), np.float32)))
    b = np.zeros((64, 2))
    b[0] = (1e3, -1e3)
    first = plugin_dscale(kernel, y, x, b, np.float32)
    assert (first == 0).all(), kernel


@pytest.mark.parametrize("kernel", KERNELS)
def test_a_nan_target_coordinate_spoils_only_its_own_row(kernel):
    rs = np.random.RandomState(43)
    y, x, b = (rounded(a, np.float32) for a in (rs.rand(300, 3), rs.rand(130, 3), rs.randn(300, 2)))
    x_nan = x.copy()
    x_nan[77, 1] = np.nan
    others = np.arange(130) != 77
    for M in (300, 5):  # 5: every batch is guarded
        want = dref.scale_derivative(kernel=kernel, source_points=y[:M], target_points=x, source_signal=b[:M])
        tol, _ = tolerance(kernel, y[:M], x, b[:M], np.float32, want)
        H = plugin_dscale(kernel, y[:M], x_nan, b[:M], np.float32)
        assert np.isnan(H[77]).any(), (kernel, M)
        check(H[others], want[others], tol, f"{kernel} M={M}: the rows beside the NaN target")


def test_dscale_far_from_the_origin():
    """The cube cloud translated by +100 in every coordinate, float32: the difference form does not lose digits.  The
    [b y_d^2 | b y_d | b] expansion through existing gradient calls would subtract sums 1e4 times the result."""
    y, b = kmvp_oracle.uniform_cube(3000, 3)
    y, b = rounded(y + 100.0, np.float32), rounded(b, np.float32)
    for kernel in KERNELS:
        want = dref.scale_derivative(kernel=kernel, source_points=y, source_signal=b)
        got = plugin_dscale(kernel, y, None, b, np.float32)
        tol, own = tolerance(kernel, y, None, b, np.float32, want)
        check(got, want, tol, f"{kernel} +100 float32 (restatement's own float32 error {own:.1e})")


def ctx_dscale(kernel, y, x, b, dtype, *, options=(), j_offset=0, M_total=None):
    """Through the C ABI's typed wrapper."""
    npdt = np.float64 if dtype == _lib.KMVP_F64 else np.float32
    ctx = _lib.Context(0)
    try:
        for key, value in options:
            ctx.set_option(key, value)
        ctx.set_points(np.ascontiguousarray(y, dtype=npdt), None if x is None else np.ascontiguousarray(x, dtype=npdt), dtype,
                       j_offset=j_offset, M_total=M_total)
        ctx.set_signal(None if b is None else np.ascontiguousarray(b, dtype=npdt))
        N, D = (y.shape[0] if x is None else x.shape[0]), y.shape[1]
        E = 1 if b is None else b.shape[1]
        ctx.run_dscale(kernel)
        assert ctx.last_kernel_name == "lowd_dscale_kernel" and ctx.last_dispatch_note == ""
        assert ctx.last_kernel_ms > 0 and ctx.last_total_ms >= ctx.last_kernel_ms
        return ctx.get_result(N, E * D)
    finally:
        ctx.close()


def test_dscale_is_bitwise_reproducible():
    """No atomics, fixed summation order: bitwise equal results run to run, with 8 segments and with 24 (the segment
    reduction splits its sums over lanes from 16 on); between the two counts the results agree to rounding."""
    rs = np.random.RandomState(51)
    y, x, b = rs.rand(5001, 3), rs.rand(3000, 3), rs.randn(5001, 2)
    for kernel in KERNELS:
        for dtype in (_lib.KMVP_F32, _lib.KMVP_F64):
            runs = {}
            for seg in (8, 24):
                first = ctx_dscale(kernel, y, x, b, dtype, options=(("segments", seg),))
                again = ctx_dscale(kernel, y, x, b, dtype, options=(("segments", seg),))
                assert np.array_equal(first, again), (kernel, dtype, seg)
                runs[seg] = first
            assert rel_err(runs[8], runs[24]) <= (1e-12 if dtype == _lib.KMVP_F64 else 1e-6), (kernel, dtype)


def test_dscale_shards_sum_to_the_whole():
    """Three partial_shard source slices with j_offset / M_total add up to the whole in float64 (1e-11); a small chunk as
    well, so that the slices fold often.  A slice without a communicator and without the option is refused."""
    rs = np.random.RandomState(52)
    y, x, b = rs.rand(200, 3), rs.rand(450, 3), rs.randn(200, 2)
    for kernel in KERNELS:
        whole = ctx_dscale(kernel, y, x, b, _lib.KMVP_F64)
        want = dref.scale_derivative(kernel=kernel, source_points=y, target_points=x, source_signal=b)
        assert rel_err(whole, want.reshape(450, -1)) <= TOL64
        parts = sum(ctx_dscale(kernel, y[lo:hi], x, b[lo:hi], _lib.KMVP_F64, j_offset=lo, M_total=200,
                               options=(("partial_shard", 1), ("chunk", 16)))
                    for lo, hi in ((0, 67), (67, 131), (131, 200)))
        err = rel_err(parts, whole)
        print(f"{kernel}: sum of 3 shards vs whole {err:.2e}")
        assert err <= TOL64, (kernel, err)
    with pytest.raises(_lib.KmvpError) as e:
        ctx_dscale("gaussian", y[:67], x, b[:67], _lib.KMVP_F64, j_offset=0, M_total=200)
    assert e.value.code == 1


def test_dscale_through_a_communicator_of_one_rank():
    """kmvp_comm_init with world == 1: segment sums, the canonical unpadded exchange, the all-reduce."""
    rs = np.random.RandomState(53)
    y, x, b = rs.rand(301, 2), rs.rand(130, 2), rs.randn(301, 3)
    ctx = _lib.Context(0)  # one communicator for the four kernels: its start-up is most of this test's time
    try:
        ctx.comm_init(_lib.comm_unique_id(), 0, 1)
        ctx.set_points(y, x, _lib.KMVP_F64)
        ctx.set_signal(b)
        for kernel in KERNELS:
            ctx.run_dscale(kernel)
            assert ctx.last_kernel_name == "lowd_dscale_kernel"
            through = ctx.get_result(130, 6)
            want = dref.scale_derivative(kernel=kernel, source_points=y, target_points=x, source_signal=b)
            assert rel_err(through, want.reshape(130, -1)) <= TOL64
            assert np.array_equal(ctx_dscale(kernel, y, x, b, _lib.KMVP_F64), through), kernel  # the same additions in the same order
    finally:
        ctx.close()


def test_two_ranks_on_one_gpu():
    """The plugin's derivative with the sources sharded over two ranks, and the solver's likelihood gradient with the
    operator sharded, through the library's host-staged all-reduce; the worker checks the values on every rank and that
    both ranks hold the same bits."""
    out = _spawn([os.path.join(HERE, "_dscale_rank_worker.py")], world=2, timeout=300)
    rep = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
    print(json.dumps(rep))
    assert rep["world"] == 2 and rep["identical_bits"] is True, rep
    assert len(rep["cases"]) == 2 * len(KERNELS) + 1, rep
    assert all(c["device_kernel"] == "lowd_dscale_kernel" for c in rep["cases"]), rep


def reference_gradient(kernel, y, x, b):
    if kernel in matern_reference.KERNELS:
        return matern_reference.gradient(kernel=kernel, source_points=y, target_points=x, source_signal=b)
    return grad_reference.gradient(kernel=kernel, source_points=y, target_points=x, source_signal=b)


def reference_product(kernel, y, x, b):
    if kernel in matern_reference.KERNELS:
        return matern_reference.product(kernel=kernel, source_points=y, target_points=x, source_signal=b)
    return kmvp_oracle.product(kernel=kernel, source_points=y, target_points=x, source_signal=b)


def test_product_gradient_and_dscale_share_the_packed_layouts():
    """Product, gradient and length-scale derivative on one context in both orders: all three still match (one pack of
    the points and of the signal serves them), and a new signal (density) repacks the records for the derivative."""
    rs = np.random.RandomState(54)
    y, x, b = rs.rand(257, 3), rs.rand(193, 3), rs.randn(257, 2)
    for kernel in KERNELS:
        want_h = dref.scale_derivative(kernel=kernel, source_points=y, target_points=x, source_signal=b).reshape(193, -1)
        want_g = reference_gradient(kernel, y, x, b).reshape(193, -1)
        want_a = reference_product(kernel, y, x, b)
        for order in (("product", "grad", "dscale"), ("dscale", "grad", "product"), ("grad", "dscale", "product")):
            ctx = _lib.Context(0)
            got = {}
            try:
                ctx.set_option("fast_sqdists", 0)
                ctx.set_points(y, x, _lib.KMVP_F64)
                ctx.set_signal(b)
                for what in order:
                    if what == "product":
                        ctx.run(kernel, False)
                        assert ctx.last_kernel_name == "lowd_kernel"
                        got[what] = ctx.get_result(193, 2)
                    else:
                        (ctx.run_grad if what == "grad" else ctx.run_dscale)(kernel)
                        assert ctx.last_kernel_name == ("lowd_grad_kernel" if what == "grad" else "lowd_dscale_kernel")
                        got[what] = ctx.get_result(193, 6)
                ctx.set_signal(None)  # density: other records
                ctx.run_dscale(kernel)
                Hd = ctx.get_result(193, 3)
            finally:
                ctx.close()
            assert rel_err(got["dscale"], want_h) <= TOL64 and rel_err(got["grad"], want_g) <= TOL64, (kernel, order)
            assert rel_err(got["product"], want_a) <= TOL64, (kernel, order)
            want_d = dref.scale_derivative(kernel=kernel, source_points=y, target_points=x).reshape(193, -1)
            assert rel_err(Hd, want_d) <= TOL64, (kernel, order)


def test_c_abi_refusals():
    """bf16 context, D = 9, E = 5: KMVP_E_UNSUPPORTED with a message; no points, no signal, an unattached shard:
    KMVP_E_INVALID."""
    rs = np.random.RandomState(55)
    entries = (("gaussian", "kmvp_gaussian_dscale"), ("absolute-exponential", "kmvp_absexp_dscale"),
               ("matern-3/2", "kmvp_matern32_dscale"), ("matern-5/2", "kmvp_matern52_dscale"))

    def refused(y, b, dtype):
        ctx = _lib.Context(0)
        try:
            ctx.set_points(np.ascontiguousarray(y, dtype=np.float32), None, dtype)
            ctx.set_signal(np.ascontiguousarray(b, dtype=np.float32))
            for kernel, entry in entries:
                rc = getattr(ctx._lib, entry)(ctx._ctx)
                msg = ctx._lib.kmvp_last_error(ctx._ctx).decode()
                assert rc == 2 and msg, (entry, rc, msg)
                with pytest.raises(_lib.KmvpError) as e:
                    ctx.run_dscale(kernel)
                assert e.value.code == 2
        finally:
            ctx.close()
        return msg

    assert "bfloat16" in refused(rs.rand(64, 16), rs.randn(64, 1), _lib.KMVP_BF16)
    assert "D = 9" in refused(rs.rand(64, 9), rs.randn(64, 1), _lib.KMVP_F32)
    assert "E = 5" in refused(rs.rand(64, 3), rs.randn(64, 5), _lib.KMVP_F32)
    ctx = _lib.Context(0)
    try:
        for _, entry in entries:
            assert getattr(ctx._lib, entry)(ctx._ctx) == 1  # no points
        y32 = np.ascontiguousarray(rs.rand(64, 3), dtype=np.float32)
        ctx.set_points(y32, None, _lib.KMVP_F32)
        for _, entry in entries:
            assert getattr(ctx._lib, entry)(ctx._ctx) == 1  # no signal
            assert ctx._lib.kmvp_last_error(ctx._ctx)
        ctx.set_points(y32[:20], y32, _lib.KMVP_F32, j_offset=0, M_total=64)  # a shard nobody sums with
        ctx.set_signal(np.ascontiguousarray(rs.randn(20, 1), dtype=np.float32))
        for _, entry in entries:
            assert getattr(ctx._lib, entry)(ctx._ctx) == 1
            assert b"partial_shard" in ctx._lib.kmvp_last_error(ctx._ctx)
        with pytest.raises(NotImplementedError):  # no entry point for 1/r
            ctx.run_dscale("inverse-distance")
    finally:
        ctx.close()


# ---- the Gaussian-process likelihood gradient ----------------------------------------------------------------------------

GP_N, GP_D, GP_E, GP_RIDGE, GP_PROBES, GP_SEED = 600, 3, 2, 0.1, 32, 0
_dense_cache = {}


def gp_inputs():
    rs = np.random.RandomState(603)
    return 3.0 * rs.rand(GP_N, GP_D), rs.randn(GP_N, GP_E)


def kernel_matrix(kernel, y):
    if kernel in matern_reference.KERNELS:
        return matern_reference.kernel_matrix(kernel=kernel, source_points=y)
    return kmvp_oracle.kernel_matrix(kernel=kernel, source_points=y)


def dense(kernel, precision):
    """A, dA_d, the spectrum and alpha of the dense float64 problem on the inputs as ``precision`` holds them; computed
    once per (kernel, precision) and left unchanged."""
    key = (kernel, np.dtype(precision).name)
    if key not in _dense_cache:
        y, a = (rounded(v, precision) for v in gp_inputs())
        A = kernel_matrix(kernel, y) + GP_RIDGE * np.eye(GP_N)
        dA = dref.scale_derivative(kernel=kernel, source_points=y, source_signal=np.eye(GP_N))  # [i, j, d]
        lam, V = np.linalg.eigh(A)
        invA = (V / lam) @ V.T
        alpha = invA @ a
        z = np.where(np.random.RandomState(GP_SEED).rand(GP_N, GP_PROBES) < 0.5, -1.0, 1.0)
        _dense_cache[key] = dict(
            y=y, a=a, lam=lam, invA=invA, alpha=alpha, z=z, h_z=np.einsum("ijd,jp->ipd", dA, z),
            quad=np.einsum("ie,ijd,je->d", alpha, dA, alpha), trace=np.einsum("ij,jid->d", invA, dA),
            value=-0.5 * np.sum(a * alpha) - 0.5 * GP_E * np.sum(np.log(lam)) - 0.5 * GP_E * GP_N * np.log(2 * np.pi))
    return _dense_cache[key]


@pytest.mark.parametrize("precision,rtol", ((np.float64, 1e-8), (np.float32, 1e-4)), ids=("float64", "float32"))
@pytest.mark.parametrize("kernel", KERNELS)
def test_log_marginal_likelihood_gradient(kernel, precision, rtol):
    """N = 600, D = 3, E = 2, ridge 0.1, against dense float64 numpy with the same probes (seed 0: the dense estimator
    with its probes is within 1.2 of its standard errors of the exact gradient for every kernel and axis, checked on the
    CPU before the seed was fixed).  The sign and factor conventions are pinned without a device in
    test_dscale_host.py (central differences of the dense likelihood)."""
    ref = dense(kernel, precision)
    lam, invA, alpha, z = ref["lam"], ref["invA"], ref["alpha"], ref["z"]
    cond = lam[-1] / lam[0]
    assert lam[0] >= GP_RIDGE * (1 - 1e-9)
    algo = MI355XSolver(kernel=kernel, dimension=GP_D, precision=precision, rtol=rtol, maxit=5000, ridge=GP_RIDGE, device=0)
    try:
        algo.prepare_data(source_points=ref["y"])
        algo.fit()
        algo.prepare_query(target_signal=ref["a"])
        algo.query()
        assert algo.converged
        value, value_stderr = algo.log_marginal_likelihood(probes=GP_PROBES, seed=GP_SEED)
        got = algo.log_marginal_likelihood_gradient(probes=GP_PROBES, seed=GP_SEED)
        pieces = algo._likelihood_gradient_pieces(GP_PROBES, GP_SEED)
        sol = algo.get_result()
        assert algo.get_additional()["device_kernel"] == "lowd_dscale_kernel"
        again = algo.log_marginal_likelihood(probes=GP_PROBES, seed=GP_SEED)  # the operator still works afterwards
    finally:
        algo.done()
    assert got.converged is True and got.d_log_lengthscale.shape == (GP_D,) and got.d_log_lengthscale_stderr.shape == (GP_D,)
    # value: log_marginal_likelihood()'s, bit for bit
    assert got.value == value and got.value_stderr == value_stderr and again == (value, value_stderr)
    # the quadratic terms: the solve's rtol times the condition number (lambda_max / lambda_min <= lambda_max / 0.1), from
    # the dense matrix; and never looser than 1e-6 at rtol 1e-8 (1e-2 at 1e-4), the figure the bound was expected to have
    bound = min(rtol * cond, 100 * rtol)
    quad = np.einsum("me,med->d", sol, pieces["h_alpha"])
    quad_err = np.max(np.abs(quad - ref["quad"]) / np.abs(ref["quad"]))
    aa, aa_ref = np.sum(sol * sol), np.sum(alpha * alpha)
    print(f"{kernel} {np.dtype(precision).name}: cond {cond:.3g}, bound rtol * cond {bound:.2e}; quad_d rel err {quad_err:.2e}, "
          f"alpha'alpha rel err {abs(aa - aa_ref) / aa_ref:.2e}")
    assert quad_err <= bound and abs(aa - aa_ref) / aa_ref <= bound
    # per-probe terms: the recurrence's residual |r_p| <= rtol |z_p|, x_p - A^-1 z_p = A^-1 r_p, twice for the drift
    # between the recurrence and the true residual
    terms = np.einsum("mp,mpd->pd", pieces["x"], pieces["h_z"])
    terms_ref = np.einsum("mp,mpd->pd", invA @ z, ref["h_z"])
    slack = 2 * rtol * np.linalg.norm(z, axis=0)[:, None] * np.linalg.norm(ref["h_z"], axis=0) / lam[0]
    worst = np.max(np.abs(terms - terms_ref) / slack)
    print(f"{kernel} {np.dtype(precision).name}: per-probe terms use {worst:.2e} of their bound")
    assert worst <= 1.0
    # the estimate: within 4 of its reported standard errors of the exact gradient
    exact = 0.5 * ref["quad"] - 0.5 * GP_E * ref["trace"]
    exact_ridge = 0.5 * aa_ref - 0.5 * GP_E * np.sum(1.0 / lam)
    dev = np.abs(got.d_log_lengthscale - exact) / got.d_log_lengthscale_stderr
    dev_ridge = abs(got.d_ridge - exact_ridge) / got.d_ridge_stderr
    print(f"{kernel} {np.dtype(precision).name}: dL/dlog l = {got.d_log_lengthscale} +- {got.d_log_lengthscale_stderr} "
          f"(exact {exact}: {dev} stderr), dL/dridge = {got.d_ridge:.6g} +- {got.d_ridge_stderr:.3g} (exact {exact_ridge:.6g}), "
          f"value {got.value:.6f} +- {got.value_stderr:.3f} (exact {ref['value']:.6f})")
    assert (dev <= 4).all() and dev_ridge <= 4 and abs(got.value - ref["value"]) <= 4 * got.value_stderr
    assert (got.d_log_lengthscale_stderr <= 0.05 * np.abs(exact)).all()  # and the estimate says something
