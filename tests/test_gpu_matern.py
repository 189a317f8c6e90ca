"""GPU tests of the Matern 3/2 and 5/2 kernels (include/kmvp.h kmvp_matern32 / kmvp_matern52): product, row-normalised
product, density, gradient with respect to the targets, CG solves with and without a ridge, source shards -- against
the float64 numpy restatement of the definition (matern_reference.py, itself checked against the Bessel form and
central differences in test_matern_reference.py).

Tolerances are the project's own, in conftest.rel_err:
  float64  <= 1e-11
  float32  <= max(1e-5, 2 x the restatement's own float32 error on the case), on the float32-rounded inputs
Every test prints what it measured.
"""
import json
import os

import numpy as np
import pytest

import matern_reference as mref
from conftest import rel_err
from kernel_matrix_benchmarks_amd import _lib
from kernel_matrix_benchmarks_amd.algorithms.mi355x import MI355XProduct, MI355XSolver
from test_gpu_multirank import _spawn

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TOL64 = 1e-11
TOL32 = 1e-5
KERNELS = mref.KERNELS
PRECISIONS = (np.float64, np.float32)
PRECISION_IDS = ("float64", "float32")
SHAPES = ((1, 1), (3, 1), (3, 4), (8, 2))  # (D, E)
ENTRY = {"matern-3/2": "kmvp_matern32", "matern-5/2": "kmvp_matern52"}


def rounded(a, precision):
    return None if a is None else np.asarray(a, dtype=precision).astype(np.float64)


def tolerance(own, want, precision):
    """`own` is the restatement run in float32 on the same (float32-rounded) inputs."""
    if np.dtype(precision) == np.float64:
        return TOL64, 0.0
    own_err = rel_err(own.reshape(len(own), -1), want.reshape(len(want), -1))
    return max(TOL32, 2 * own_err), own_err


def check(got, want, own, precision, label):
    n = want.shape[0]
    tol, own_err = tolerance(own, want, precision)
    assert np.isfinite(got).all(), (label, "non-finite output")
    err = rel_err(got.reshape(n, -1), want.reshape(n, -1))
    print(f"{label}: rel_err {err:.3e} (tolerance {tol:.1e}, restatement's own float32 error {own_err:.1e})")
    assert err <= tol, (label, err, tol)
    return err


def plugin(kernel, y, x, b, precision, *, normalize=False, gradient=False, expect=None, **options):
    """The runner's call order; gradient: query_gradient() / get_gradient() in the place of query() / get_result()."""
    algo = MI355XProduct(kernel=kernel, dimension=y.shape[1], normalize_rows=normalize, precision=precision, **options)
    try:
        algo.prepare_data(source_points=y, target_points=y if x is None else x, same_points=x is None,
                          density_estimation=b is None)
        algo.fit()
        algo.prepare_query(source_signal=b)
        if gradient:
            algo.query_gradient()
            out = algo.get_gradient()
        else:
            algo.query()
            out = algo.get_result()
        extra = algo.get_additional()
    finally:
        algo.done()
    assert out.dtype == np.float64 and out.flags["C_CONTIGUOUS"]
    assert extra["dispatch_note"] == "", extra
    assert extra["device_kernel"] == (expect or ("lowd_grad_kernel" if gradient else "lowd_kernel")), extra
    assert extra["device_kernel_ms"] > 0 and extra["device_total_ms"] >= extra["device_kernel_ms"]
    return out


def product_triple(kernel, y, x, b, precision, label, rows=None, expect=None, **options):
    """Plain, row-normalised and density products of one case against the restatement."""
    for mode, signal, normalize in (("plain", b, False), ("normalised", b, True), ("density", None, False)):
        ref = dict(kernel=kernel, source_points=y, target_points=x, source_signal=signal, normalize_rows=normalize, rows=rows)
        want = mref.product(**ref)
        own = mref.product(precision=np.float32, **ref) if np.dtype(precision) == np.float32 else want
        got = plugin(kernel, y, x, signal, precision, normalize=normalize, expect=expect, **options)
        assert got.shape == ((y if x is None else x).shape[0], 1 if signal is None else signal.shape[1])
        check(got if rows is None else got[rows], want, own, precision, f"{label} {mode}")


def gradient_pair(kernel, y, x, b, precision, label):
    """Gradient of the product and of the density estimate against the restatement."""
    for mode, signal in (("gradient", b), ("density gradient", None)):
        ref = dict(kernel=kernel, source_points=y, target_points=x, source_signal=signal)
        want = mref.gradient(**ref)
        own = mref.gradient(precision=np.float32, **ref) if np.dtype(precision) == np.float32 else want
        got = plugin(kernel, y, x, signal, precision, gradient=True)
        assert got.shape == want.shape
        check(got, want, own, precision, f"{label} {mode}")


# ---- 1 (and the parity part of 5): lowd_kernel / lowd_grad_kernel ---------------------------------------------------------

@pytest.mark.parametrize("other", (False, True), ids=("same-M1003", "N777-M1003"))
@pytest.mark.parametrize("D, E", SHAPES, ids=[f"D{d}-E{e}" for d, e in SHAPES])
@pytest.mark.parametrize("precision", PRECISIONS, ids=PRECISION_IDS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_parity_of_products_and_gradients(kernel, precision, D, E, other):
    """Seeded cube clouds; M = 1003 is no multiple of the batch of 8, so pad records (y = +inf) are live in every case."""
    rs = np.random.RandomState(100 * D + 10 * E + int(other))
    y, b = rounded(rs.rand(1003, D), precision), rounded(rs.randn(1003, E), precision)
    x = rounded(rs.rand(777, D), precision) if other else None
    label = f"{kernel} {np.dtype(precision).name} D={D} E={E} {'N=777 M=1003' if other else 'same points M=1003'}"
    product_triple(kernel, y, x, b, precision, label)
    gradient_pair(kernel, y, x, b, precision, label)


@pytest.mark.parametrize("kernel", KERNELS)
def test_more_than_four_columns_and_float16_inputs(kernel):
    """E = 6 at D = 3: the difference form once per block of four columns (normalised: the denominator from the first
    block).  precision="float16": the inputs rounded to float16, float32 arithmetic."""
    rs = np.random.RandomState(17)
    y, x, b = (rounded(a, np.float32) for a in (rs.rand(1003, 3), rs.rand(300, 3), rs.randn(1003, 6)))
    for normalize in (False, True):
        ref = dict(kernel=kernel, source_points=y, target_points=x, source_signal=b, normalize_rows=normalize)
        want = mref.product(**ref)
        got = plugin(kernel, y, x, b, np.float32, normalize=normalize)
        check(got, want, mref.product(precision=np.float32, **ref), np.float32, f"{kernel} E=6 normalize={normalize}")
    y16, x16, b16 = (rounded(a, np.float16) for a in (y, x, b[:, :2]))
    ref = dict(kernel=kernel, source_points=y16, target_points=x16, source_signal=b16)
    got = plugin(kernel, y, x, b[:, :2], np.float16)
    check(got, mref.product(**ref), mref.product(precision=np.float32, **ref), np.float32, f"{kernel} float16 inputs")


# ---- 2: several segments and chunks ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("options", ({}, dict(segments=24, chunk=512)), ids=("auto", "segments24-chunk512"))
@pytest.mark.parametrize("E", (1, 3))
@pytest.mark.parametrize("kernel", KERNELS)
def test_products_on_a_cloud_of_several_segments_and_chunks(kernel, E, options):
    """N = 20 000 targets != M = 30 001 sources (ragged), D = 3, float32; the restatement on 512 seeded rows."""
    rs = np.random.RandomState(2025 + E)
    y, x, b = (rounded(a, np.float32) for a in (rs.rand(30001, 3), rs.rand(20000, 3), rs.randn(30001, E)))
    rows = np.sort(rs.choice(20000, 512, replace=False))
    ref = dict(kernel=kernel, source_points=y, target_points=x, source_signal=b, rows=rows)
    want = mref.product(**ref)
    got = plugin(kernel, y, x, b, np.float32, **options)[rows]
    check(got, want, mref.product(precision=np.float32, **ref), np.float32, f"{kernel} N=20000 M=30001 E={E} {options}")
    wantg = mref.gradient(**ref)
    gotg = plugin(kernel, y, x, b, np.float32, gradient=True, **options)[rows]
    check(gotg, wantg, mref.gradient(precision=np.float32, **ref), np.float32, f"{kernel} N=20000 M=30001 E={E} {options} gradient")


# ---- 3: the generic kernels -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D, E, name", ((20, 5, "lowd_mid_kernel"), (200, 3, "lowd_big_kernel")), ids=("D20-E5", "D200-E3"))
@pytest.mark.parametrize("precision", PRECISIONS, ids=PRECISION_IDS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_generic_kernels(kernel, precision, D, E, name):
    """N = 300, M = 501: coordinates in registers up to D = 128, the chunked walk beyond.  Cube / sqrt(D / 3): distances
    of order one, as at D = 3."""
    rs = np.random.RandomState(D + E)
    scale = np.sqrt(D / 3.0)
    y, x, b = (rounded(a, precision) for a in (rs.rand(501, D) / scale, rs.rand(300, D) / scale, rs.randn(501, E)))
    product_triple(kernel, y, x, b, precision, f"{kernel} {np.dtype(precision).name} D={D} E={E} {name}", expect=name)


# ---- 4: s = +inf ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("D, name", ((3, "lowd_kernel"), (20, "lowd_mid_kernel")), ids=("D3", "D20"))
@pytest.mark.parametrize("precision, far", ((np.float32, 1e20), (np.float64, 1e200)), ids=PRECISION_IDS[::-1])
@pytest.mark.parametrize("kernel", KERNELS)
def test_pairs_at_infinite_distance_contribute_exactly_zero(kernel, precision, far, D, name):
    """M = 1001 sources in the unit cube (pad records live); targets: 64 in the cube, one at (far, 0, ...) whose squared
    distance overflows the working precision, one at distance 200.  The polynomial times e^-t would be inf * 0 there.
    Every output is finite; the overflowing row is exactly 0.0 in the product, the density, the normalised numerator's
    plain product and every gradient component (D = 3: the gradient is built up to D = 8).  The row at distance 200 is
    exactly 0.0 in float32 (e^-t flushed from t = 104 on) and ~1e-150, held to the tolerance, in float64."""
    rs = np.random.RandomState(41)
    y, b = rounded(rs.rand(1001, D), precision), rounded(rs.randn(1001, 2), precision)
    x = rounded(rs.rand(66, D), precision)
    x[64] = 0.0
    x[64, 0] = far
    x[65] = 0.5
    x[65, 0] = 200.5
    zero_rows = [64, 65] if precision == np.float32 else [64]
    label = f"{kernel} {np.dtype(precision).name} D={D}"
    for mode, signal in (("plain", b), ("density", None)):
        ref = dict(kernel=kernel, source_points=y, target_points=x, source_signal=signal)
        want = mref.product(**ref)
        got = plugin(kernel, y, x, signal, precision, expect=name)
        assert (got[zero_rows] == 0.0).all(), (label, mode, got[64:])
        check(got, want, mref.product(precision=np.float32, **ref) if precision == np.float32 else want, precision, f"{label} {mode}")
        print(f"{label} {mode}: far rows {got[64:].tolist()}")
        if D <= 8:
            wantg = mref.gradient(**ref)
            gotg = plugin(kernel, y, x, signal, precision, gradient=True)
            assert (gotg[zero_rows] == 0.0).all(), (label, mode, gotg[64:])
            check(gotg, wantg, mref.gradient(precision=np.float32, **ref) if precision == np.float32 else wantg, precision,
                  f"{label} {mode} gradient")


# ---- 5: gradient ----------------------------------------------------------------------------------------------------------

def ctx_run(kernel, y, x, b, dtype, *, grad=False, normalize=False, options=(), j_offset=0, M_total=None):
    """Through the C ABI's typed wrapper."""
    npdt = np.float64 if dtype == _lib.KMVP_F64 else np.float32
    ctx = _lib.Context(0)
    try:
        for key, value in options:
            ctx.set_option(key, value)
        ctx.set_points(np.ascontiguousarray(y, dtype=npdt), None if x is None else np.ascontiguousarray(x, dtype=npdt), dtype,
                       j_offset=j_offset, M_total=M_total)
        ctx.fit(kernel)
        ctx.set_signal(None if b is None else np.ascontiguousarray(b, dtype=npdt))
        N, D = (y.shape[0] if x is None else x.shape[0]), y.shape[1]
        E = 1 if b is None else b.shape[1]
        if grad:
            ctx.run_grad(kernel)
        else:
            ctx.run(kernel, normalize)
        assert ctx.last_kernel_name == ("lowd_grad_kernel" if grad else "lowd_kernel") and ctx.last_dispatch_note == ""
        return ctx.get_result(N, E * D if grad else E)
    finally:
        ctx.close()


@pytest.mark.parametrize("precision", PRECISIONS, ids=PRECISION_IDS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_gradient_of_coincident_pairs(kernel, precision):
    """Five targets sit exactly on sources 0 .. 4.  Their rows are finite, and the coincident pair contributes 0: the row
    equals the restatement's row computed WITHOUT that source."""
    rs = np.random.RandomState(51)
    y, b = rounded(rs.rand(203, 3), precision), rounded(rs.randn(203, 2), precision)
    x = y[:5].copy()
    got = plugin(kernel, y, x, b, precision, gradient=True)
    assert np.isfinite(got).all()
    want = np.stack([mref.gradient(kernel=kernel, source_points=np.delete(y, i, axis=0), target_points=x[i : i + 1],
                                   source_signal=np.delete(b, i, axis=0))[0] for i in range(5)])
    own = mref.gradient(kernel=kernel, source_points=y, target_points=x, source_signal=b, precision=np.float32)
    check(got, want, own, precision, f"{kernel} {np.dtype(precision).name} coincident pairs")
    # one source, one target on it: the whole result is that pair's contribution
    lone = plugin(kernel, y[:1], y[:1].copy(), b[:1], precision, gradient=True)
    assert (lone == 0.0).all(), lone


@pytest.mark.parametrize("kernel", KERNELS)
def test_gradient_and_product_far_from_the_origin(kernel):
    """The cube translated by +100 in every coordinate, float32: the difference form keeps the float32 rule."""
    rs = np.random.RandomState(52)
    y, b = rounded(rs.rand(3000, 3) + 100.0, np.float32), rounded(rs.randn(3000, 1), np.float32)
    ref = dict(kernel=kernel, source_points=y, source_signal=b)
    check(plugin(kernel, y, None, b, np.float32, gradient=True), mref.gradient(**ref), mref.gradient(precision=np.float32, **ref),
          np.float32, f"{kernel} +100 float32 gradient")
    check(plugin(kernel, y, None, b, np.float32), mref.product(**ref), mref.product(precision=np.float32, **ref),
          np.float32, f"{kernel} +100 float32 product")


def test_results_are_bitwise_reproducible():
    """No atomics, fixed summation order: bitwise equal results run to run, below and above the segment count at which the
    segment reduction splits its sums over lanes (8 and 24 segments).  The two segment counts group the float32 chunk sums
    differently, so between THEM the results are not bitwise equal; each is held to the tolerance of DESIGN section 4
    against the restatement, which bounds their difference by twice that tolerance (printed)."""
    rs = np.random.RandomState(53)
    y, x, b = rs.rand(5001, 3), rs.rand(3000, 3), rs.randn(5001, 2)
    rows = np.sort(rs.choice(3000, 256, replace=False))  # the restatement on 256 seeded rows
    for kernel in KERNELS:
        for dtype, precision in ((_lib.KMVP_F32, np.float32), (_lib.KMVP_F64, np.float64)):
            yr, xr, br = (rounded(a, precision) for a in (y, x, b))
            for grad in (True, False):
                ref = dict(kernel=kernel, source_points=yr, target_points=xr, source_signal=br, rows=rows)
                fn = mref.gradient if grad else mref.product
                want = fn(**ref).reshape(256, -1)
                own = fn(precision=np.float32, **ref).reshape(256, -1) if precision == np.float32 else want
                runs = {}
                for seg in (8, 24):
                    first = ctx_run(kernel, yr, xr, br, dtype, grad=grad, options=(("segments", seg),))
                    again = ctx_run(kernel, yr, xr, br, dtype, grad=grad, options=(("segments", seg),))
                    assert np.array_equal(first, again), (kernel, dtype, grad, seg)
                    check(first[rows], want, own, precision,
                          f"{kernel} {np.dtype(precision).name} {'gradient' if grad else 'product'} segments={seg}")
                    runs[seg] = first
                print(f"{kernel} {np.dtype(precision).name} {'gradient' if grad else 'product'}: 8 against 24 segments "
                      f"{rel_err(runs[8], runs[24]):.3e}")


# ---- 6: solver ------------------------------------------------------------------------------------------------------------

SOLVE_N = 600


def solve_inputs():
    rs = np.random.RandomState(61)
    return rs.rand(SOLVE_N, 3), rs.randn(SOLVE_N, 2)


@pytest.mark.parametrize("ridge", ("scalar", "per-point"))
@pytest.mark.parametrize("kernel", KERNELS)
def test_ridge_solution_vector_against_the_dense_solve(kernel, ridge):
    """same_points, N = 600, D = 3, float64; ridge = 1e-2 or one value per point in [1e-3, 1e-1].  DESIGN section 4:
    ||b - b_dense|| / ||b_dense|| <= kappa (1.5 rtol + 1e-11), kappa from numpy.linalg.cond."""
    y, a = solve_inputs()
    rtol = 1e-10
    diag = 1e-2 if ridge == "scalar" else np.random.RandomState(62).uniform(1e-3, 1e-1, SOLVE_N)
    A = mref.kernel_matrix(kernel=kernel, source_points=y) + np.diag(np.broadcast_to(diag, (SOLVE_N,)))
    kappa = float(np.linalg.cond(A))
    dense = np.linalg.solve(A, a)
    algo = MI355XSolver(kernel=kernel, dimension=3, precision=np.float64, rtol=rtol, maxit=20000, ridge=diag)
    try:
        algo.prepare_data(source_points=y)
        algo.fit()
        algo.prepare_query(target_signal=a)
        algo.query()
        b, info = algo.get_result(), algo.get_additional()
    finally:
        algo.done()
    err = float(np.max(np.linalg.norm(b - dense, axis=0) / np.linalg.norm(dense, axis=0)))
    bound = kappa * (1.5 * rtol + 1e-11)
    res = float(np.max(np.linalg.norm(A @ b - a, axis=0) / np.linalg.norm(a, axis=0)))
    print(f"{kernel} ridge {ridge}: kappa {kappa:.3g} iterations {info['cg_iterations']} residual "
          f"{info['cg_relative_residual']:.3g} (numpy: {res:.3g}) vector error {err:.3g} bound {bound:.3g}")
    assert algo.method == "cg" and info["device_kernel"] == "lowd_kernel", info
    assert info["cg_converged"], info
    assert err <= bound, (err, bound, info)


@pytest.mark.parametrize("kernel", KERNELS)
def test_bare_solve_reports_its_true_residual(kernel):
    """Without a ridge, rtol = 1e-6: the matrix is positive definite but ill conditioned, so KMVP_OK and
    KMVP_E_NOT_CONVERGED are both legitimate ends; either way the reported residual is the true one -- it equals the
    residual recomputed in numpy from the returned b to 1e-9 absolute -- and the verdict follows from it."""
    y, a = solve_inputs()
    rtol = 1e-6
    K = mref.kernel_matrix(kernel=kernel, source_points=y)
    ctx = _lib.Context(0)
    try:
        ctx.set_points(y, None, _lib.KMVP_F64)
        ctx.fit(kernel)
        b, iters, resid, ok = ctx.cg_solve(kernel, a, rtol, 3000)
    finally:
        ctx.close()
    res = float(np.max(np.linalg.norm(K @ b - a, axis=0) / np.linalg.norm(a, axis=0)))
    print(f"{kernel} bare: {iters} iterations, reported residual {resid:.6e}, numpy {res:.6e}, converged {ok}, |b|max {np.max(np.abs(b)):.3g}")
    assert np.isfinite(b).all() and 0 < iters <= 3000
    assert abs(resid - res) <= 1e-9, (resid, res)
    assert ok == (resid <= 1.5 * rtol), (ok, resid)


@pytest.mark.parametrize("kernel", KERNELS)
def test_negative_ridge_is_refused(kernel):
    y, a = solve_inputs()
    ctx = _lib.Context(0)
    try:
        ctx.set_points(y, None, _lib.KMVP_F64)
        for d, ridge in ((None, -1e-2), (np.full(SOLVE_N, -1e-2), 0.0), (np.linspace(-1e-3, 1e-1, SOLVE_N), 0.0)):
            ctx.set_solver_diagonal(d, ridge)
            with pytest.raises(_lib.KmvpError) as e:
                ctx.cg_solve(kernel, a, 1e-6, 100)
            assert e.value.code == 1 and "ridge" in str(e.value), e.value
    finally:
        ctx.close()


# ---- 7: shards ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", KERNELS)
def test_source_shards_sum_to_the_whole(kernel):
    """partial_shard = 1: three source slices of M = 1003 with j_offset / M_total set add up to the unsharded product and
    gradient within 1e-12 in float64 (no index-based rule: the offsets do not enter the values)."""
    rs = np.random.RandomState(71)
    y, x, b = rs.rand(1003, 3), rs.rand(450, 3), rs.randn(1003, 2)
    for grad in (False, True):
        whole = ctx_run(kernel, y, x, b, _lib.KMVP_F64, grad=grad)
        want = (mref.gradient if grad else mref.product)(kernel=kernel, source_points=y, target_points=x, source_signal=b)
        assert rel_err(whole, want.reshape(450, -1)) <= TOL64
        parts = sum(ctx_run(kernel, y[lo:hi], x, b[lo:hi], _lib.KMVP_F64, grad=grad, j_offset=lo, M_total=1003,
                            options=(("partial_shard", 1),))
                    for lo, hi in ((0, 335), (335, 670), (670, 1003)))
        err = rel_err(parts, whole)
        print(f"{kernel} {'gradient' if grad else 'product'}: sum of 3 shards vs whole {err:.2e}")
        assert err <= 1e-12, (kernel, grad, err)
    with pytest.raises(_lib.KmvpError) as e:  # a slice with nobody to sum it with, and without the option
        ctx_run(kernel, y[:335], x, b[:335], _lib.KMVP_F64, j_offset=0, M_total=1003)
    assert e.value.code == 1


def test_two_ranks_on_one_gpu():
    """Products, a gradient and a ridge solve of the plugin with the sources sharded over two ranks, through the library's
    host-staged all-reduce (kmvp_comm_init_host); the worker checks them against the restatement on every rank."""
    out = _spawn([os.path.join(HERE, "_matern_rank_worker.py")], world=2, timeout=300)
    rep = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
    print(json.dumps(rep))
    assert rep["world"] == 2 and len(rep["cases"]) == 8, rep
    assert all(c["device_kernel"] in ("lowd_kernel", "lowd_grad_kernel") for c in rep["cases"]), rep


# ---- 8: refusals ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kernel", KERNELS)
def test_c_abi_refusals(kernel):
    """A bf16 context and an explicit fast_sqdists 1 / 2 / 3 (4 as well): KMVP_E_UNSUPPORTED with a message, for the plain
    and the normalised entry and inside a solve; fast_sqdists 0 and -1 run.  kmvp_fit takes the codes 3 and 4."""
    rs = np.random.RandomState(81)
    y32, b32 = rs.rand(64, 16).astype(np.float32), rs.randn(64, 1).astype(np.float32)

    def refused(ctx, word):
        for entry in (ENTRY[kernel], ENTRY[kernel] + "_norm"):
            rc = getattr(ctx._lib, entry)(ctx._ctx)
            msg = ctx._lib.kmvp_last_error(ctx._ctx).decode()
            assert rc == 2 and word in msg, (entry, rc, msg)
        with pytest.raises(_lib.KmvpError) as e:
            ctx.run(kernel, False)
        assert e.value.code == 2

    ctx = _lib.Context(0)
    try:
        ctx.set_points(y32, None, _lib.KMVP_BF16)
        ctx.set_signal(b32)
        refused(ctx, "bfloat16")
        with pytest.raises(_lib.KmvpError) as e:
            ctx.run_grad(kernel)
        assert e.value.code == 2
    finally:
        ctx.close()
    ctx = _lib.Context(0)
    try:
        ctx.set_points(y32[:, :3].copy(), None, _lib.KMVP_F32)
        ctx.set_signal(b32)
        for code in (1, 2, 3, 4):
            ctx.set_option("fast_sqdists", code)
            refused(ctx, "fast_sqdists")
        with pytest.raises(_lib.KmvpError) as e:
            ctx.cg_solve(kernel, b32, 1e-3, 10)
        assert e.value.code == 2
        for code in (0, -1):
            ctx.set_option("fast_sqdists", code)
            ctx.set_signal(b32)
            ctx.run(kernel, False)
            assert ctx.last_kernel_name == "lowd_kernel" and ctx.last_dispatch_note == ""
        assert ctx._lib.kmvp_fit(ctx._ctx, 3) == 0 and ctx._lib.kmvp_fit(ctx._ctx, 4) == 0
        assert ctx._lib.kmvp_fit(ctx._ctx, 5) == 1
    finally:
        ctx.close()
