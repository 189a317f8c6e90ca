"""CPU tests of the log-sum-exp reduction: the entry points exist, the plugin refuses what the kernels are not built
for before the library is called, and the numpy restatement the GPU tests compare with (lse_reference.py) is
``numpy.logaddexp.reduce`` of the logits."""
import os
import re

import numpy as np
import pytest

import lse_reference
from kernel_matrix_benchmarks_amd import _lib
from kernel_matrix_benchmarks_amd.algorithms import mi355x

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LSE_SYMBOLS = ("kmvp_gaussian_logsumexp", "kmvp_absexp_logsumexp")


def test_logsumexp_entry_points_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kmvp.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in LSE_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*kmvp_ctx\s*\*" % name, text), f"kmvp.h does not declare {name}"
        assert hasattr(lib, name), f"libkmvp.so lacks {name}"
    assert lib.kmvp_abi_version() == 1  # entries were added, nothing changed
    assert callable(getattr(_lib.Context, "run_lse", None))
    for method in ("query_logsumexp", "get_logsumexp", "_check_logsumexp_supported"):
        assert callable(getattr(mi355x.MI355XProduct, method, None)), method


def test_plugin_refuses_unsupported_logsumexps_before_the_library_is_called(monkeypatch):
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

        def run_lse(self, kernel):
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
        (dict(kernel="matern-3/2"), "matern-3/2"),
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
        with pytest.raises(NotImplementedError, match=word):
            p.query_logsumexp()
    assert calls == []
    # what IS built reaches the library: both kernels, float16 inputs (rounded, float32 arithmetic), the largest shape,
    # density estimation, the difference form asked for by name
    prepared(kernel="gaussian", precision=np.float16).query_logsumexp()
    prepared(kernel="absolute-exponential", D=8, E=4, precision=np.float64).query_logsumexp()
    prepared(kernel="gaussian", density=True, fast_sqdists=False).query_logsumexp()
    assert calls == ["gaussian", "absolute-exponential", "gaussian"]


@pytest.mark.parametrize("kernel", lse_reference.KERNELS)
@pytest.mark.parametrize("D", (1, 3, 8))
@pytest.mark.parametrize("E", (None, 1, 3))
def test_restatement_is_logaddexp_reduce_of_the_logits(kernel, D, E):
    """Small clouds, targets != sources, log-weights of a few units; density estimation (E = None) is c = 0."""
    rs = np.random.RandomState(100 + 10 * D + (E or 0))
    y, x = rs.randn(37, D), rs.randn(23, D) * 2.0
    c = None if E is None else rs.randn(37, E) * 3.0
    got = lse_reference.logsumexp(kernel=kernel, source_points=y, target_points=x, source_signal=c)
    s = np.sum((x[:, None, :] - y[None, :, :]) ** 2, axis=-1)
    ell = -s if kernel == "gaussian" else -np.sqrt(s)
    cc = np.zeros((37, 1)) if c is None else c
    want = np.logaddexp.reduce(ell[:, :, None] + cc[None, :, :], axis=1)
    assert got.shape == (23, 1 if E is None else E) and got.dtype == np.float64
    err = float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))
    print(f"{kernel} D={D} E={E}: restatement vs logaddexp.reduce {err:.2e}")
    assert err <= 1e-13, (kernel, D, E, err)
    # same points and a rows= subset
    rows = np.array([0, 5, 36])
    own = lse_reference.logsumexp(kernel=kernel, source_points=y, source_signal=c, rows=rows)
    whole = lse_reference.logsumexp(kernel=kernel, source_points=y, target_points=y, source_signal=c)
    assert np.array_equal(own, whole[rows])


@pytest.mark.parametrize("kernel", lse_reference.KERNELS)
def test_restatement_conventions(kernel):
    """c = -inf is weight 0 (equal to leaving the source out); an all -inf column is exactly -inf and leaves the other
    columns alone; no source: -inf; a NaN target: a NaN row and no other; logits near -1e6 and c spanning +-1e3 stay
    finite; float32 arithmetic is available and close."""
    rs = np.random.RandomState(7)
    y, x = rs.rand(41, 3), rs.rand(19, 3)
    c = rs.randn(41, 3)
    c[::3, 0] = -np.inf
    c[:, 1] = -np.inf
    with np.errstate(invalid="ignore"):
        got = lse_reference.logsumexp(kernel=kernel, source_points=y, target_points=x, source_signal=c)
    keep = np.isfinite(c[:, 0])
    left_out = lse_reference.logsumexp(kernel=kernel, source_points=y[keep], target_points=x, source_signal=c[keep][:, [0, 2]])
    s = np.sum((x[:, None, :] - y[None, :, :]) ** 2, axis=-1)
    ell = -s if kernel == "gaussian" else -np.sqrt(s)
    with np.errstate(invalid="ignore"):
        want = np.logaddexp.reduce(ell[:, :, None] + c[None, :, :], axis=1)
    assert np.allclose(got[:, 0], left_out[:, 0], rtol=0, atol=1e-13)
    assert np.all(np.isneginf(got[:, 1]))
    assert np.allclose(got[:, [0, 2]], want[:, [0, 2]], rtol=0, atol=1e-13) and np.isfinite(got[:, [0, 2]]).all()
    # an all -inf row of c in every column: that source simply vanishes; every c = -inf: every row -inf
    assert np.all(np.isneginf(lse_reference.logsumexp(kernel=kernel, source_points=y, target_points=x,
                                                      source_signal=np.full((41, 2), -np.inf))))
    assert np.all(np.isneginf(lse_reference.logsumexp(kernel=kernel, source_points=y[:0], target_points=x)))
    xn = x.copy()
    xn[4, 1] = np.nan
    gn = lse_reference.logsumexp(kernel=kernel, source_points=y, target_points=xn, source_signal=c[:, [0, 2]])
    assert np.isnan(gn[4]).all() and np.isfinite(np.delete(gn, 4, axis=0)).all()
    far = lse_reference.logsumexp(kernel=kernel, source_points=y, target_points=x + (1e3 if kernel == "gaussian" else 1e6),
                                  source_signal=rs.uniform(-1e3, 1e3, (41, 2)))
    assert np.isfinite(far).all() and far.min() < -5e5
    y32, x32, c32 = (a.astype(np.float32).astype(np.float64) for a in (y, x, c[:, [0, 2]]))
    f64 = lse_reference.logsumexp(kernel=kernel, source_points=y32, target_points=x32, source_signal=c32)
    f32 = lse_reference.logsumexp(kernel=kernel, source_points=y32, target_points=x32, source_signal=c32, precision=np.float32)
    assert f32.dtype == np.float64 and np.max(np.abs(f32 - f64) / np.maximum(1, np.abs(f64))) < 1e-5
