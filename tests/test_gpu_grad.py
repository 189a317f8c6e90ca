"""GPU tests of the gradient of the product with respect to the targets (lowd_grad_kernel, include/kmvp.h
kmvp_<kernel>_grad) against the float64 numpy restatement of its definition (grad_reference.py, itself checked
against central differences of the pinned oracle in test_grad_reference.py).

Tolerances are the project's own, in conftest.rel_err over flattened (E D) rows:
  float64  <= 1e-11
  float32  <= max(1e-5, 2 x the restatement's own float32 error on the case), on the float32-rounded inputs
"""
import numpy as np
import pytest

import golden_cases
import grad_reference
import kmvp_oracle
from conftest import rel_err
from kernel_matrix_benchmarks_amd import _lib
from kernel_matrix_benchmarks_amd.algorithms.mi355x import MI355XProduct

pytestmark = pytest.mark.gpu

TOL64 = 1e-11
TOL32 = 1e-5
CASES = [c for c in golden_cases.product_cases() if not c["normalize_rows"] and c["D"] <= 8 and c["E"] <= 4]


def rounded(a, precision):
    return None if a is None else np.asarray(a, dtype=precision).astype(np.float64)


def plugin_gradient(kernel, y, x, b, precision, **options):
    """The runner's call order with query_gradient() / get_gradient() in the place of query() / get_result()."""
    algo = MI355XProduct(kernel=kernel, dimension=y.shape[1], precision=precision, **options)
    try:
        algo.prepare_data(source_points=y, target_points=y if x is None else x, same_points=x is None,
                          density_estimation=b is None)
        algo.fit()
        algo.prepare_query(source_signal=b)
        algo.query_gradient()
        G = algo.get_gradient()
        extra = algo.get_additional()
    finally:
        algo.done()
    N = y.shape[0] if x is None else x.shape[0]
    assert G.shape == (N, 1 if b is None else b.shape[1], y.shape[1])
    assert G.dtype == np.float64 and G.flags["C_CONTIGUOUS"]
    assert extra["device_kernel"] == "lowd_grad_kernel" and extra["dispatch_note"] == ""
    return G


def tolerance(kernel, y, x, b, precision, want, rows=None):
    """The float32 rule: the restatement run in float32 on the same inputs sets the scale of what float32 can do."""
    if np.dtype(precision) == np.float64:
        return TOL64, 0.0
    own = grad_reference.gradient(kernel=kernel, source_points=y, target_points=x, source_signal=b,
                                  precision=np.float32, rows=rows)
    own_err = rel_err(own.reshape(len(own), -1), want.reshape(len(want), -1))
    return max(TOL32, 2 * own_err), own_err


def check_rows(got, want, tol, label):
    """Non-finite rows of the restatement are non-finite in EVERY component on the GPU, no other row is; the rest is
    compared in rel_err (which leaves exactly those rows out)."""
    n = want.shape[0]
    got2, want2 = got.reshape(n, -1), want.reshape(n, -1)
    bad_want = ~np.isfinite(want2).all(axis=1)
    bad_got = ~np.isfinite(got2)
    assert (bad_got.any(axis=1) == bad_want).all(), (label, np.nonzero(bad_got.any(axis=1))[0], np.nonzero(bad_want)[0])
    assert bad_got[bad_want].all(), (label, "a non-finite row must be non-finite in every component")
    err = rel_err(got2, want2)
    print(f"{label}: rel_err {err:.3e} (tolerance {tol:.1e}, {int(bad_want.sum())} non-finite rows)")
    assert err <= tol, (label, err, tol)
    return err


@pytest.mark.parametrize("precision", (np.float64, np.float32), ids=("float64", "float32"))
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_gradient_parity(case, precision):
    """Every un-normalised golden case at D <= 8, E <= 4 (60 of them: test_grad_reference.py counts): same / different
    points, density, ragged N and M, the N > M wrap of the zero rule, D = 1 .. 8, E = 1 .. 4, the two coincident-pair
    cases."""
    y, x, b = (rounded(a, precision) for a in golden_cases.make_inputs(case))
    want = grad_reference.gradient(kernel=case["kernel"], source_points=y, target_points=x, source_signal=b)
    got = plugin_gradient(case["kernel"], y, x, b, precision)
    tol, own = tolerance(case["kernel"], y, x, b, precision, want)
    check_rows(got, want, tol, f"{case['name']} {np.dtype(precision).name} (restatement's own float32 error {own:.1e})")


@pytest.mark.parametrize("kernel", golden_cases.KERNELS)
@pytest.mark.parametrize("E", (1, 3))
def test_gradient_on_a_cloud_of_several_segments_and_chunks(kernel, E):
    """N = 20 000 targets != M = 30 001 sources (ragged: pad records in the last batch), D = 3, float32; the restatement on
    512 seeded rows."""
    rs = np.random.RandomState(2024 + E)
    y, x, b = (rounded(a, np.float32) for a in (rs.rand(30001, 3), rs.rand(20000, 3), rs.randn(30001, E)))
    rows = np.sort(rs.choice(20000, 512, replace=False))
    want = grad_reference.gradient(kernel=kernel, source_points=y, target_points=x, source_signal=b, rows=rows)
    got = plugin_gradient(kernel, y, x, b, np.float32)[rows]
    tol, own = tolerance(kernel, y, x, b, np.float32, want, rows=rows)
    check_rows(got, want, tol, f"{kernel} N=20000 M=30001 E={E} float32 (restatement's own float32 error {own:.1e})")


def test_gaussian_gradient_far_from_the_origin():
    """The case that motivates the difference form: the cube cloud translated by +100 in every coordinate, float32.  The
    gradient meets the float32 rule.  The [b | b y] identity  grad a_i = -2 (x_i sum_j k b_j - sum_j k y_j b_j)  run through
    the existing product on the same inputs subtracts two sums of size |x| sum |k b|: its error is recorded (printed), not
    asserted."""
    y, b = kmvp_oracle.uniform_cube(3000, 3)
    y, b = rounded(y + 100.0, np.float32), rounded(b, np.float32)
    want = grad_reference.gradient(kernel="gaussian", source_points=y, source_signal=b)
    got = plugin_gradient("gaussian", y, None, b, np.float32)
    tol, own = tolerance("gaussian", y, None, b, np.float32, want)
    check_rows(got, want, tol, f"gaussian +100 float32 (restatement's own float32 error {own:.1e})")
    algo = MI355XProduct(kernel="gaussian", dimension=3, precision=np.float32, fast_sqdists=False)
    try:
        algo.prepare_data(source_points=y, target_points=y, same_points=True)
        algo.fit()
        algo.prepare_query(source_signal=np.concatenate((b, b * y), axis=1))
        algo.query()
        a = algo.get_result()
    finally:
        algo.done()
    identity = -2.0 * (y * a[:, :1] - a[:, 1:])
    print(f"gaussian +100 float32: the [b | b y] identity through the product has rel_err "
          f"{rel_err(identity, want.reshape(3000, 3)):.3e}")


def ctx_gradient(kernel, y, x, b, dtype, *, options=(), j_offset=0, M_total=None, comm=False, before=None):
    """Through the C ABI's typed wrapper; `before`: a product (kernel name) run on the same context first."""
    npdt = np.float64 if dtype == _lib.KMVP_F64 else np.float32
    ctx = _lib.Context(0)
    try:
        if comm:
            ctx.comm_init(_lib.comm_unique_id(), 0, 1)
        for key, value in options:
            ctx.set_option(key, value)
        ctx.set_points(np.ascontiguousarray(y, dtype=npdt), None if x is None else np.ascontiguousarray(x, dtype=npdt), dtype,
                       j_offset=j_offset, M_total=M_total)
        ctx.set_signal(None if b is None else np.ascontiguousarray(b, dtype=npdt))
        N, D = (y.shape[0] if x is None else x.shape[0]), y.shape[1]
        E = 1 if b is None else b.shape[1]
        product = None
        if before:
            ctx.run(before, False)
            product = ctx.get_result(N, E)
        ctx.run_grad(kernel)
        assert ctx.last_kernel_name == "lowd_grad_kernel" and ctx.last_dispatch_note == ""
        assert ctx.last_kernel_ms > 0 and ctx.last_total_ms >= ctx.last_kernel_ms
        G = ctx.get_result(N, E * D)
        return (G, product) if before else G
    finally:
        ctx.close()


def test_gradient_is_bitwise_reproducible():
    """No atomics, fixed summation order: bitwise equal results run to run, with 8 segments (one thread per sum in the
    segment reduction) and with 24 (sums split over lanes: SEG_SPLIT_FROM = 16 lies between).  The two segment counts
    group the same terms differently, so between THEM the results agree to rounding (1e-12 in float64), not bitwise."""
    rs = np.random.RandomState(31)
    y, x, b = rs.rand(5001, 3), rs.rand(3000, 3), rs.randn(5001, 2)
    for kernel in golden_cases.KERNELS:
        for dtype in (_lib.KMVP_F32, _lib.KMVP_F64):
            runs = {}
            for seg in (8, 24):
                first = ctx_gradient(kernel, y, x, b, dtype, options=(("segments", seg),))
                again = ctx_gradient(kernel, y, x, b, dtype, options=(("segments", seg),))
                assert np.array_equal(first, again), (kernel, dtype, seg)
                runs[seg] = first
            assert rel_err(runs[8], runs[24]) <= (1e-12 if dtype == _lib.KMVP_F64 else 1e-6), (kernel, dtype)


def test_gradient_shards_sum_to_the_whole():
    """Three partial_shard source slices with j_offset / M_total (1/r included, N > M: the zero rule wraps) add up to the
    whole to 1e-12 in float64; a small chunk as well, so that the slices fold often."""
    rs = np.random.RandomState(32)
    y, x, b = rs.rand(200, 3), rs.rand(450, 3), rs.randn(200, 2)
    for kernel in golden_cases.KERNELS:
        whole = ctx_gradient(kernel, y, x, b, _lib.KMVP_F64)
        want = grad_reference.gradient(kernel=kernel, source_points=y, target_points=x, source_signal=b)
        assert rel_err(whole, want.reshape(450, -1)) <= TOL64
        parts = sum(ctx_gradient(kernel, y[lo:hi], x, b[lo:hi], _lib.KMVP_F64, j_offset=lo, M_total=200,
                                 options=(("partial_shard", 1), ("chunk", 16)))
                    for lo, hi in ((0, 67), (67, 131), (131, 200)))
        err = rel_err(parts, whole)
        print(f"{kernel}: sum of 3 shards vs whole {err:.2e}")
        assert err <= 1e-12, (kernel, err)
    # a slice without a communicator and without the option is refused, like a product
    with pytest.raises(_lib.KmvpError) as e:
        ctx_gradient("gaussian", y[:67], x, b[:67], _lib.KMVP_F64, j_offset=0, M_total=200)
    assert e.value.code == 1


def test_gradient_through_a_communicator_of_one_rank():
    """kmvp_comm_init with world == 1: segment sums, the canonical unpadded exchange, the all-reduce."""
    rs = np.random.RandomState(33)
    y, x, b = rs.rand(301, 2), rs.rand(130, 2), rs.randn(301, 3)
    for kernel in golden_cases.KERNELS:
        plain = ctx_gradient(kernel, y, x, b, _lib.KMVP_F64)
        through = ctx_gradient(kernel, y, x, b, _lib.KMVP_F64, comm=True)
        want = grad_reference.gradient(kernel=kernel, source_points=y, target_points=x, source_signal=b)
        assert rel_err(through, want.reshape(130, -1)) <= TOL64
        assert np.array_equal(plain, through), kernel  # the same additions in the same order


def test_product_and_gradient_share_the_packed_layouts():
    """A product followed by a gradient on one context and the reverse order: both still match (one pack serves both)."""
    rs = np.random.RandomState(34)
    y, x, b = rs.rand(257, 3), rs.rand(193, 3), rs.randn(257, 2)
    for kernel in golden_cases.KERNELS:
        want_g = grad_reference.gradient(kernel=kernel, source_points=y, target_points=x, source_signal=b).reshape(193, -1)
        want_a = kmvp_oracle.product(kernel=kernel, source_points=y, target_points=x, source_signal=b)
        G, a = ctx_gradient(kernel, y, x, b, _lib.KMVP_F64, options=(("fast_sqdists", 0),), before=kernel)
        assert rel_err(G, want_g) <= TOL64 and rel_err(a, want_a) <= TOL64, kernel
        ctx = _lib.Context(0)
        try:
            ctx.set_option("fast_sqdists", 0)
            ctx.set_points(y, x, _lib.KMVP_F64)
            ctx.set_signal(b)
            ctx.run_grad(kernel)
            G = ctx.get_result(193, 6)
            ctx.run(kernel, False)
            assert ctx.last_kernel_name == "lowd_kernel"
            a = ctx.get_result(193, 2)
            ctx.set_signal(None)  # density: other records, and the gradient of a density estimate
            ctx.run_grad(kernel)
            Gd = ctx.get_result(193, 3)
        finally:
            ctx.close()
        assert rel_err(G, want_g) <= TOL64 and rel_err(a, want_a) <= TOL64, kernel
        want_d = grad_reference.gradient(kernel=kernel, source_points=y, target_points=x).reshape(193, -1)
        assert rel_err(Gd, want_d) <= TOL64, kernel


def test_c_abi_refusals():
    """bf16 context, D = 9, E = 5: KMVP_E_UNSUPPORTED with a message; call-order errors: KMVP_E_INVALID."""
    rs = np.random.RandomState(35)

    def refused(y, b, dtype):
        ctx = _lib.Context(0)
        try:
            ctx.set_points(np.ascontiguousarray(y, dtype=np.float32), None, dtype)
            ctx.set_signal(np.ascontiguousarray(b, dtype=np.float32))
            for kernel, entry in (("gaussian", "kmvp_gaussian_grad"), ("absolute-exponential", "kmvp_absexp_grad"),
                                  ("inverse-distance", "kmvp_invdist_grad")):
                rc = getattr(ctx._lib, entry)(ctx._ctx)
                msg = ctx._lib.kmvp_last_error(ctx._ctx).decode()
                assert rc == 2 and msg, (entry, rc, msg)
                with pytest.raises(_lib.KmvpError) as e:
                    ctx.run_grad(kernel)
                assert e.value.code == 2
        finally:
            ctx.close()
        return msg

    assert "bfloat16" in refused(rs.rand(64, 16), rs.randn(64, 1), _lib.KMVP_BF16)
    assert "D = 9" in refused(rs.rand(64, 9), rs.randn(64, 1), _lib.KMVP_F32)
    assert "E = 5" in refused(rs.rand(64, 3), rs.randn(64, 5), _lib.KMVP_F32)
    ctx = _lib.Context(0)
    try:
        assert ctx._lib.kmvp_gaussian_grad(ctx._ctx) == 1  # no points
        ctx.set_points(np.ascontiguousarray(rs.rand(64, 3), dtype=np.float32), None, _lib.KMVP_F32)
        assert ctx._lib.kmvp_invdist_grad(ctx._ctx) == 1  # no signal
        assert ctx._lib.kmvp_last_error(ctx._ctx)
    finally:
        ctx.close()
