"""CPU tests of the Matern 3/2 and 5/2 kernels: the numpy restatement the GPU tests compare with (matern_reference.py)
is the Matern covariance of the textbooks and its gradient is the derivative of its product; the eight entry points
exist in the header, the binding and the built library; the plugin accepts the two names and refuses what is not
built before the library is called."""
import os
import re

import numpy as np
import pytest

import matern_reference
from conftest import rel_err
from kernel_matrix_benchmarks_amd import _lib
from kernel_matrix_benchmarks_amd.algorithms import mi355x

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRODUCT_SYMBOLS = ("kmvp_matern32", "kmvp_matern32_norm", "kmvp_matern52", "kmvp_matern52_norm")
GRAD_SYMBOLS = ("kmvp_matern32_grad", "kmvp_matern52_grad")
SOLVE_SYMBOLS = ("kmvp_matern32_cg_solve", "kmvp_matern52_cg_solve")


@pytest.mark.parametrize("kernel, nu", (("matern-3/2", 1.5), ("matern-5/2", 2.5)))
def test_restatement_is_the_bessel_form(kernel, nu):
    """k(r) = 2^(1 - nu) / Gamma(nu) (sqrt(2 nu) r)^nu K_nu(sqrt(2 nu) r) at length scale 1."""
    special = pytest.importorskip("scipy.special")
    r = np.logspace(-3, 1.5, 200)
    z = np.sqrt(2 * nu) * r
    want = 2.0 ** (1 - nu) / special.gamma(nu) * z ** nu * special.kv(nu, z)
    got = matern_reference.kernel_values(kernel, r * r)
    err = float(np.max(np.abs(got - want) / want))
    print(f"{kernel}: restatement vs the Bessel form, largest relative difference {err:.2e}")
    assert err <= 1e-12, (kernel, err)


@pytest.mark.parametrize("kernel", matern_reference.KERNELS)
def test_restatement_at_zero_and_at_infinite_distance(kernel):
    for dt in (np.float64, np.float32):
        k = matern_reference.kernel_values(kernel, np.array([0.0, np.inf], dtype=dt))
        w = matern_reference.gradient_weights(kernel, np.array([0.0, np.inf], dtype=dt))
        assert k.dtype == dt and k[0] == 1.0 and k[1] == 0.0, (kernel, dt, k)
        assert w[0] == dt({"matern-3/2": -3.0, "matern-5/2": -5.0 / 3.0}[kernel]) and w[1] == 0.0, (kernel, dt, w)


@pytest.mark.parametrize("kernel", matern_reference.KERNELS)
@pytest.mark.parametrize("D", (1, 3, 8))
@pytest.mark.parametrize("E", (1, 3))
def test_restatement_gradient_is_the_derivative_of_its_product(kernel, D, E):
    """Central differences (h = 1e-5, float64) of the restatement's own product on separated clouds (r >= 0.5).
    Truncation h^2 |k'''| / (6 |k'|) is below 1e-9 here and the rounding of the differences about 1e-16 / h = 1e-11 of
    the product, so 1e-6 holds with room."""
    rs = np.random.RandomState(500 + 10 * D + E)
    y, x, b = rs.rand(97, D), rs.rand(130, D), rs.randn(97, E)
    x[:, 0] += 1.5
    h = 1e-5
    fd = np.empty((130, E, D))
    for d in range(D):
        step = np.zeros(D)
        step[d] = h
        hi = matern_reference.product(kernel=kernel, source_points=y, target_points=x + step, source_signal=b)
        lo = matern_reference.product(kernel=kernel, source_points=y, target_points=x - step, source_signal=b)
        fd[:, :, d] = (hi - lo) / (2 * h)
    G = matern_reference.gradient(kernel=kernel, source_points=y, target_points=x, source_signal=b)
    assert G.shape == (130, E, D) and G.dtype == np.float64 and G.flags["C_CONTIGUOUS"]
    err = rel_err(G.reshape(130, -1), fd.reshape(130, -1))
    print(f"{kernel} D={D} E={E}: restatement vs central differences {err:.2e}")
    assert err <= 1e-6, (kernel, D, E, err)


@pytest.mark.parametrize("kernel", matern_reference.KERNELS)
def test_restatement_gradient_of_a_coincident_pair_is_exactly_zero(kernel):
    p = np.array([[0.25, 0.5, 0.75]])
    for precision in (np.float64, np.float32):
        G = matern_reference.gradient(kernel=kernel, source_points=p, target_points=p.copy(), source_signal=np.array([[2.0]]),
                                      precision=precision)
        assert G.shape == (1, 1, 3) and (G == 0.0).all(), (kernel, G)


def test_restatement_products():
    """Density is b = 1, the normalised product is the ratio of the two, `rows` selects targets, float32 runs in float32."""
    rs = np.random.RandomState(7)
    y, x, b = rs.rand(61, 3), rs.rand(40, 3), rs.randn(61, 2)
    for kernel in matern_reference.KERNELS:
        K = matern_reference.kernel_matrix(kernel=kernel, source_points=y, target_points=x)
        assert np.allclose(K, K.clip(0, 1)) and K.shape == (40, 61)
        a = matern_reference.product(kernel=kernel, source_points=y, target_points=x, source_signal=b)
        den = matern_reference.product(kernel=kernel, source_points=y, target_points=x)
        nrm = matern_reference.product(kernel=kernel, source_points=y, target_points=x, source_signal=b, normalize_rows=True)
        assert np.allclose(a, K @ b, rtol=1e-14) and np.allclose(den, K.sum(axis=1, keepdims=True), rtol=1e-14)
        assert np.allclose(nrm, a / den, rtol=1e-13)
        rows = np.array([3, 17, 39])
        assert np.allclose(matern_reference.product(kernel=kernel, source_points=y, target_points=x, source_signal=b, rows=rows),
                           a[rows], rtol=1e-14)
        a32 = matern_reference.product(kernel=kernel, source_points=y, target_points=x, source_signal=b, precision=np.float32)
        assert 0 < rel_err(a32, a) < 1e-5
        Ks = matern_reference.kernel_matrix(kernel=kernel, source_points=y)
        assert np.array_equal(Ks, Ks.T) and (np.diag(Ks) == 1.0).all() and np.linalg.eigvalsh(Ks).min() > 0


def test_entry_points_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kmvp.h")).read(), flags=re.S)
    lib = _lib.load()
    bound = {s[0]: s for s in _lib.SYMBOLS}
    for name in PRODUCT_SYMBOLS + GRAD_SYMBOLS + SOLVE_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*kmvp_ctx\s*\*" % name, text), f"kmvp.h does not declare {name}"
        assert hasattr(lib, name), f"libkmvp.so lacks {name}"
        assert name in bound, f"_lib.SYMBOLS does not bind {name}"
    for name in SOLVE_SYMBOLS:
        assert bound[name][2] == bound["kmvp_gaussian_cg_solve"][2]
    assert lib.kmvp_abi_version() == 1  # entries were added, nothing changed
    assert _lib.FIT_CODES["matern-3/2"] == 3 and _lib.FIT_CODES["matern-5/2"] == 4


def test_plugin_accepts_the_kernels_and_refuses_what_is_not_built(monkeypatch):
    calls = []

    class Quiet:
        comm_world = 0

        def __init__(self, device=0):
            calls.append("create")

    monkeypatch.setattr(_lib, "Context", Quiet)
    for kernel in matern_reference.KERNELS:
        assert kernel in mi355x.SUPPORTED_KERNELS
        for precision in (np.float16, np.float32, np.float64, "float32"):
            for fast in (None, False):
                p = mi355x.MI355XProduct(kernel=kernel, dimension=3, precision=precision, fast_sqdists=fast)
                assert p.kernel == kernel and p._device_kernel_fn == kernel
                assert callable(p.query_gradient)
        assert mi355x.MI355XSolver(kernel=kernel, dimension=3).method == "cg"
        assert mi355x.MI355XSolver(kernel=kernel, dimension=3, ridge=0.01, precision=np.float32).method == "cg"
        with pytest.raises(ValueError, match="non-negative"):
            mi355x.MI355XSolver(kernel=kernel, dimension=3, ridge=-0.01)
        with pytest.raises(NotImplementedError, match="bfloat16"):
            mi355x.MI355XProduct(kernel=kernel, dimension=3, precision="bfloat16")
        with pytest.raises(NotImplementedError):
            mi355x.MI355XSolver(kernel=kernel, dimension=3, precision="bfloat16")
        for fast in (True, "centred", "cells", "cells-valu"):
            with pytest.raises(NotImplementedError, match="fast_sqdists"):
                mi355x.MI355XProduct(kernel=kernel, dimension=3, fast_sqdists=fast)
    assert calls == []  # refused (and accepted) at construction: the library was never asked


def test_plugin_call_order_reaches_the_right_entries(monkeypatch):
    """prepare_data / fit / prepare_query / query / query_gradient hand the kernel's own name to the binding; a sharded
    prepare_data keeps the caller's source order (no spatial order for these kernels)."""
    seen = []

    class Recording:
        comm_world = 0

        def __init__(self, device=0):
            pass

        def set_option(self, key, value):
            seen.append(("option", key, value))

        def set_points(self, y, x, dtype, j_offset=0, M_total=None):
            seen.append(("points", y.copy(), j_offset, M_total))

        def fit(self, kernel):
            seen.append(("fit", kernel))

        def set_signal(self, b):
            seen.append(("signal", None if b is None else b.copy()))

        def run(self, kernel, normalize_rows):
            seen.append(("run", kernel, normalize_rows))

        def run_grad(self, kernel):
            seen.append(("grad", kernel))

        def close(self):
            pass

    class TwoRanks:
        rank, world = 1, 2

        def attach(self, ctx):
            pass

    monkeypatch.setattr(_lib, "Context", Recording)
    rs = np.random.RandomState(3)
    y, b = rs.rand(51, 3).astype(np.float32), rs.randn(51, 2).astype(np.float32)
    for kernel in matern_reference.KERNELS:
        del seen[:]
        p = mi355x.MI355XProduct(kernel=kernel, dimension=3, normalize_rows=True, comm=TwoRanks())
        p.prepare_data(source_points=y, target_points=y, same_points=True)
        p.fit()
        p.prepare_query(source_signal=b)
        p.query()
        lo, hi = p.shard
        points = [s for s in seen if s[0] == "points"][0]
        assert (lo, hi) == (26, 51) and np.array_equal(points[1], y[lo:hi]) and points[2:] == (lo, 51)
        assert np.array_equal([s for s in seen if s[0] == "signal"][0][1], b[lo:hi])
        assert ("fit", kernel) in seen and ("run", kernel, True) in seen
        q = mi355x.MI355XProduct(kernel=kernel, dimension=3)
        q.prepare_data(source_points=y, target_points=y, same_points=True)
        q.prepare_query(source_signal=b)
        q.query_gradient()
        assert seen[-1] == ("grad", kernel)
