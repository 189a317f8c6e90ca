"""CPU tests of the gradient of the log-sum-exp with respect to the target points: the entry points exist, the plugin
refuses what the kernels are not built for before the library is called, and the numpy restatement the GPU tests compare
with (lse_grad_reference.py) is the derivative of lse_reference.logsumexp, with the conventions of include/kmvp.h."""
import os
import re

import numpy as np
import pytest

import grad_reference
import kmvp_oracle
import lse_grad_reference
import lse_reference
from conftest import rel_err
from kernel_matrix_benchmarks_amd import _lib
from kernel_matrix_benchmarks_amd.algorithms import mi355x

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("kmvp_gaussian_logsumexp_grad", "kmvp_absexp_logsumexp_grad")
KERNELS = lse_grad_reference.KERNELS


def test_entry_points_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kmvp.h")).read(), flags=re.S)
    lib = _lib.load()
    declared = {name for name, _, _ in _lib.SYMBOLS}
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*kmvp_ctx\s*\*" % name, text), f"kmvp.h does not declare {name}"
        assert name in declared, f"_lib.SYMBOLS lacks {name}"
        assert hasattr(lib, name), f"libkmvp.so lacks {name}"
    assert lib.kmvp_abi_version() == 1  # entries were added, nothing changed
    for method in ("query_logsumexp_gradient", "get_logsumexp_gradient"):
        assert callable(getattr(mi355x.MI355XProduct, method, None)), method
    # the other kernels have no entry point: refused by the wrapper before any library call
    ctx = _lib.Context.__new__(_lib.Context)
    ctx._lib = lib
    for kernel in ("inverse-distance", "matern-3/2", "exp-dot"):
        with pytest.raises(NotImplementedError):
            ctx.run_lse_grad(kernel)


def test_plugin_refuses_unsupported_gradients_before_the_library_is_called(monkeypatch):
    calls = []

    class Quiet:
        comm_world = 0

        def __init__(self, device=0):
            pass

        def set_option(self, key, value):
            pass

        def set_points(self, y, x, dtype, j_offset=0, M_total=None):
            pass

        def set_signal(self, b):
            pass

        def run_lse_grad(self, kernel):
            calls.append(kernel)

        def close(self):
            pass

    monkeypatch.setattr(_lib, "Context", Quiet)
    rs = np.random.RandomState(0)

    def prepared(D=3, E=1, density=False, **kw):
        p = mi355x.MI355XProduct(dimension=D, **kw)
        y = rs.rand(50, D)
        p.prepare_data(source_points=y, target_points=y, same_points=True, density_estimation=density)
        p.prepare_query(source_signal=None if density else rs.randn(50, E))
        return p

    refused = (
        (dict(kernel="inverse-distance"), "inverse-distance"),
        (dict(kernel="matern-5/2"), "matern-5/2"),
        (dict(kernel="exp-dot"), "exp-dot"),
        (dict(kernel="gaussian", normalize_rows=True), "normalize_rows"),
        (dict(kernel="gaussian", precision="bfloat16"), "bfloat16"),
        (dict(kernel="absolute-exponential", D=9), "D = 9"),
        (dict(kernel="gaussian", E=5), "E = 5"),
        (dict(kernel="gaussian", fast_sqdists=True), "fast_sqdists"),
        (dict(kernel="gaussian", fast_sqdists="cells"), "fast_sqdists"),
        (dict(kernel="absolute-exponential", fast_sqdists="centred"), "fast_sqdists"),
    )
    for kw, word in refused:
        p = prepared(**kw)
        with pytest.raises(NotImplementedError, match=word) as e:
            p.query_logsumexp_gradient()
        assert "query_logsumexp_gradient" in str(e.value)
    assert calls == []
    # what IS built reaches the library: both kernels, float16 inputs (rounded, float32 arithmetic), the largest shape,
    # density estimation, the difference form asked for by name
    prepared(kernel="gaussian", precision=np.float16).query_logsumexp_gradient()
    prepared(kernel="absolute-exponential", D=8, E=4, precision=np.float64).query_logsumexp_gradient()
    prepared(kernel="gaussian", density=True, fast_sqdists=False).query_logsumexp_gradient()
    assert calls == ["gaussian", "absolute-exponential", "gaussian"]


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("D", (1, 2, 3, 5, 8))
@pytest.mark.parametrize("E", (None, 1, 3))
def test_restatement_is_the_derivative_of_the_logsumexp(kernel, D, E):
    """Central differences (h = 1e-4) of lse_reference.logsumexp in float64 at generic points (separated clouds, r >= 0.5:
    exp(-r) is not differentiable at r = 0).  Truncation is h^2 |L'''| / 6 with L''' of order 1/r^2 <= 4 and of the
    third cumulant of the softmax (cloud diameter^3 times 8 at most, a few units): some 1e-7 at most; rounding is
    2e-16 |L| / h ~ 1e-11.  The bound is test_grad_reference.py's 1e-6."""
    rs = np.random.RandomState(2000 + 10 * D + (E or 0))
    y = rs.rand(97, D)
    x = rs.rand(130, D)
    x[:, 0] += 1.5
    c = None if E is None else rs.randn(97, E)
    h = 1e-4
    NE = 1 if E is None else E
    fd = np.empty((130, NE, D))
    for d in range(D):
        step = np.zeros(D)
        step[d] = h
        hi = lse_reference.logsumexp(kernel=kernel, source_points=y, target_points=x + step, source_signal=c)
        lo = lse_reference.logsumexp(kernel=kernel, source_points=y, target_points=x - step, source_signal=c)
        fd[:, :, d] = (hi - lo) / (2 * h)
    G = lse_grad_reference.gradient(kernel=kernel, source_points=y, target_points=x, source_signal=c)
    assert G.shape == (130, NE, D) and G.dtype == np.float64 and G.flags["C_CONTIGUOUS"]
    err = rel_err(G.reshape(130, -1), fd.reshape(130, -1))
    print(f"{kernel} D={D} E={E}: restatement vs central differences {err:.2e}")
    assert err <= 1e-6, (kernel, D, E, err)
    # a rows= subset, and same points
    rows = np.array([0, 5, 96])
    own = lse_grad_reference.gradient(kernel=kernel, source_points=y, source_signal=c, rows=rows)
    whole = lse_grad_reference.gradient(kernel=kernel, source_points=y, target_points=y, source_signal=c)
    assert np.array_equal(own, whole[rows])


@pytest.mark.parametrize("D", (1, 3, 8))
def test_gaussian_gradient_points_at_the_softmax_barycentre(D):
    """G = -2 (x - ybar) with ybar from an explicit softmax of the logits."""
    rs = np.random.RandomState(50 + D)
    y, x, c = rs.randn(61, D), rs.randn(33, D) * 1.5, rs.randn(61, 2) * 2.0
    G = lse_grad_reference.gradient(kernel="gaussian", source_points=y, target_points=x, source_signal=c)
    t = -np.sum((x[:, None, :] - y[None, :, :]) ** 2, axis=-1)[:, :, None] + c[None, :, :]
    p = np.exp(t - np.logaddexp.reduce(t, axis=1, keepdims=True))                 # (n, M, E), rows sum to 1
    ybar = np.einsum("nme,md->ned", p, y)
    want = -2.0 * (x[:, None, :] - ybar)
    assert np.max(np.abs(G - want)) <= 1e-13 * max(1.0, np.max(np.abs(want)))


@pytest.mark.parametrize("kernel", KERNELS)
def test_gradient_is_the_ratio_of_gradient_and_product_where_nothing_underflows(kernel):
    """Near the cloud G = grad(K b) / (K b) with b = exp(c): the route the log-sum-exp's gradient replaces."""
    rs = np.random.RandomState(60)
    y, x, c = rs.rand(83, 3), rs.rand(47, 3) + 0.25, rs.randn(83, 2)
    x[:5] = y[:5]  # coincident pairs: both restatements take the symmetric subgradient
    b = np.exp(c)
    G = lse_grad_reference.gradient(kernel=kernel, source_points=y, target_points=x, source_signal=c)
    ratio = (grad_reference.gradient(kernel=kernel, source_points=y, target_points=x, source_signal=b)
             / kmvp_oracle.product(kernel=kernel, source_points=y, target_points=x, source_signal=b)[:, :, None])
    assert np.isfinite(G).all()
    assert np.max(np.abs(G - ratio)) <= 1e-12 * max(1.0, np.max(np.abs(ratio)))


@pytest.mark.parametrize("kernel", KERNELS)
def test_restatement_conventions(kernel):
    """c = -inf is weight 0 (equal to leaving the source out); a (row, column) without a live term is NaN in all D
    components -- exactly where the log-sum-exp is -inf -- and leaves the other columns alone; a NaN target: a NaN row
    and no other; logits near -1e6 and c spanning +-1e3 stay finite; float32 arithmetic is available and close."""
    rs = np.random.RandomState(7)
    y, x = rs.rand(41, 3), rs.rand(19, 3)
    c = rs.randn(41, 3)
    c[::3, 0] = -np.inf
    c[:, 1] = -np.inf
    got = lse_grad_reference.gradient(kernel=kernel, source_points=y, target_points=x, source_signal=c)
    L = lse_reference.logsumexp(kernel=kernel, source_points=y, target_points=x, source_signal=c)
    assert got.shape == (19, 3, 3)
    assert np.array_equal(np.isnan(got), np.broadcast_to(np.isneginf(L)[:, :, None], got.shape))
    assert np.isnan(got[:, 1]).all() and np.isfinite(got[:, [0, 2]]).all()
    keep = np.isfinite(c[:, 0])
    left_out = lse_grad_reference.gradient(kernel=kernel, source_points=y[keep], target_points=x, source_signal=c[keep][:, [0, 2]])
    assert np.allclose(got[:, 0], left_out[:, 0], rtol=0, atol=1e-13)
    # every c = -inf, and no source at all: NaN everywhere, in the result's full shape
    assert np.isnan(lse_grad_reference.gradient(kernel=kernel, source_points=y, target_points=x,
                                                source_signal=np.full((41, 2), -np.inf))).all()
    empty = lse_grad_reference.gradient(kernel=kernel, source_points=y[:0], target_points=x, source_signal=c[:0])
    assert empty.shape == (19, 3, 3) and np.isnan(empty).all()
    xn = x.copy()
    xn[4, 1] = np.nan
    gn = lse_grad_reference.gradient(kernel=kernel, source_points=y, target_points=xn, source_signal=c[:, [0, 2]])
    assert np.isnan(gn[4]).all() and np.isfinite(np.delete(gn, 4, axis=0)).all()
    assert np.array_equal(np.delete(gn, 4, axis=0), np.delete(got[:, [0, 2]], 4, axis=0))
    shift = 1e3 if kernel == "gaussian" else 1e6
    far = lse_grad_reference.gradient(kernel=kernel, source_points=y, target_points=x + shift,
                                      source_signal=rs.uniform(-1e3, 1e3, (41, 2)))
    assert np.isfinite(far).all()
    norm = np.linalg.norm(far, axis=-1)
    if kernel == "gaussian":
        assert np.all(np.abs(norm / (2 * shift * np.sqrt(3)) - 1) < 2e-3)  # -2 (x - ybar), |x - ybar| ~ sqrt(3) shift
    else:
        assert np.all(np.abs(norm - 1) < 1e-6)                             # unit vectors all but parallel
    y32, x32, c32 = (a.astype(np.float32).astype(np.float64) for a in (y, x, c[:, [0, 2]]))
    f64 = lse_grad_reference.gradient(kernel=kernel, source_points=y32, target_points=x32, source_signal=c32)
    f32 = lse_grad_reference.gradient(kernel=kernel, source_points=y32, target_points=x32, source_signal=c32, precision=np.float32)
    assert f32.dtype == np.float64 and np.max(np.abs(f32 - f64)) / max(1.0, np.max(np.abs(f64))) < 1e-5


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("precision", (np.float64, np.float32))
def test_a_nan_or_infinite_log_weight_makes_its_column_non_finite(kernel, precision):
    """c = NaN or c = +inf in one entry: no entry of that column is finite; the other columns are bitwise unchanged."""
    rs = np.random.RandomState(9)
    y, x, clean = rs.rand(41, 3), rs.rand(19, 3), rs.randn(41, 3)
    base = lse_grad_reference.gradient(kernel=kernel, source_points=y, target_points=x, source_signal=clean, precision=precision)
    assert np.isfinite(base).all()
    for j in (0, 20, 40):
        c = clean.copy()
        c[j, 0] = np.nan
        c[j, 1] = np.inf
        got = lse_grad_reference.gradient(kernel=kernel, source_points=y, target_points=x, source_signal=c, precision=precision)
        assert not np.isfinite(got[:, :2]).any()
        assert np.array_equal(got[:, 2], base[:, 2])


def test_coincident_pairs_of_exp_minus_r_drop_out_of_the_numerator_only():
    """same_points: the own pair (s == 0) contributes 0 to the numerator and keeps its weight in the denominator, so every
    row is finite and equals the sum over the OTHER sources divided by the full denominator.  A duplicated source counts
    twice.  The Gaussian needs no rule: g = -2 (x - y) is 0 there by itself."""
    rs = np.random.RandomState(8)
    y, c = rs.rand(30, 2), rs.randn(30, 1)
    y[7] = y[3]
    G = lse_grad_reference.gradient(kernel="absolute-exponential", source_points=y, source_signal=c)
    assert np.isfinite(G).all()
    diffs = y[:, None, :] - y[None, :, :]
    r = np.sqrt(np.sum(diffs ** 2, axis=-1))
    w = np.exp(-r + c[:, 0][None, :])
    with np.errstate(invalid="ignore", divide="ignore"):
        unit = np.where(r[:, :, None] > 0, diffs / r[:, :, None], 0.0)
    want = -np.einsum("nm,nmd->nd", w, unit) / np.sum(w, axis=1, keepdims=True)
    assert np.max(np.abs(G[:, 0] - want)) <= 1e-14
    # one target ON a source, far from all others: the denominator is dominated by the own pair, the gradient is ~ 0
    far = lse_grad_reference.gradient(kernel="absolute-exponential", source_points=np.vstack([y, [[50.0, 50.0]]]),
                                      target_points=np.array([[50.0, 50.0]]))
    assert np.all(np.abs(far) < 1e-25) and np.isfinite(far).all()
    Gg = lse_grad_reference.gradient(kernel="gaussian", source_points=y, source_signal=c)
    assert np.isfinite(Gg).all()
