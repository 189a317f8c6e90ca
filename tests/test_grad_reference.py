"""CPU tests of the gradient of the product with respect to the targets: the entry points exist, the plugin refuses
what the kernels are not built for before the library is called, and the numpy restatement the GPU tests compare
with (grad_reference.py) is the derivative of the pinned oracle's product."""
import os
import re

import numpy as np
import pytest

import golden_cases
import grad_reference
import kmvp_oracle
from conftest import rel_err
from kernel_matrix_benchmarks_amd import _lib
from kernel_matrix_benchmarks_amd.algorithms import mi355x

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRAD_SYMBOLS = ("kmvp_gaussian_grad", "kmvp_absexp_grad", "kmvp_invdist_grad")


def gradient_cases():
    """The product cases the gradient is defined and built for: 60 of them."""
    return [c for c in golden_cases.product_cases() if not c["normalize_rows"] and c["D"] <= 8 and c["E"] <= 4]


def test_gradient_entry_points_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kmvp.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in GRAD_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*kmvp_ctx\s*\*" % name, text), f"kmvp.h does not declare {name}"
        assert hasattr(lib, name), f"libkmvp.so lacks {name}"
    assert lib.kmvp_abi_version() == 1  # entries were added, nothing changed
    assert callable(getattr(_lib.Context, "run_grad", None))
    assert callable(getattr(mi355x.MI355XProduct, "query_gradient", None))
    assert callable(getattr(mi355x.MI355XProduct, "get_gradient", None))


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

        def run_grad(self, kernel):
            calls.append(kernel)

        def close(self):
            pass

    monkeypatch.setattr(_lib, "Context", Quiet)
    rs = np.random.RandomState(0)

    def prepared(D=3, E=1, **kw):
        p = mi355x.MI355XProduct(dimension=D, **kw)
        y = rs.rand(50, D)
        p.prepare_data(source_points=y, target_points=y, same_points=True)
        p.prepare_query(source_signal=rs.randn(50, E))
        return p

    refused = (
        (dict(kernel="gaussian", normalize_rows=True), "normalize_rows"),
        (dict(kernel="exp-dot"), "exp-dot"),
        (dict(kernel="gaussian", precision="bfloat16"), "bfloat16"),
        (dict(kernel="inverse-distance", D=9), "D = 9"),
        (dict(kernel="absolute-exponential", E=5), "E = 5"),
    )
    for kw, word in refused:
        p = prepared(**kw)
        with pytest.raises(NotImplementedError, match=word):
            p.query_gradient()
    assert calls == []
    # what IS built reaches the library: every kernel, float16 inputs (rounded, float32 arithmetic), the largest shape
    prepared(kernel="gaussian", precision=np.float16).query_gradient()
    prepared(kernel="absolute-exponential", D=8, E=4, precision=np.float64).query_gradient()
    prepared(kernel="inverse-distance").query_gradient()
    assert calls == ["gaussian", "absolute-exponential", "inverse-distance"]


@pytest.mark.parametrize("kernel", golden_cases.KERNELS)
@pytest.mark.parametrize("D", (1, 2, 3, 5, 8))
@pytest.mark.parametrize("E", (1, 3))
def test_restatement_is_the_derivative_of_the_oracle_product(kernel, D, E):
    """Central differences (h = 1e-4) of kmvp_oracle.product on separated clouds (r >= 0.5): truncation
    h^2 |k'''| / (6 |k'|) is at most 8e-8 (1/r at r = 0.5), so 1e-6 holds with room.  Overlapping clouds are unsuitable:
    near pairs of 1/r at D <= 2 put finite differences themselves off by up to 0.5."""
    rs = np.random.RandomState(1000 + 10 * D + E)
    y = rs.rand(97, D)
    x = rs.rand(130, D)
    x[:, 0] += 1.5
    b = rs.randn(97, E)
    h = 1e-4
    fd = np.empty((130, E, D))
    for d in range(D):
        step = np.zeros(D)
        step[d] = h
        hi = kmvp_oracle.product(kernel=kernel, source_points=y, target_points=x + step, source_signal=b)
        lo = kmvp_oracle.product(kernel=kernel, source_points=y, target_points=x - step, source_signal=b)
        fd[:, :, d] = (hi - lo) / (2 * h)
    G = grad_reference.gradient(kernel=kernel, source_points=y, target_points=x, source_signal=b)
    assert G.shape == (130, E, D) and G.dtype == np.float64 and G.flags["C_CONTIGUOUS"]
    err = rel_err(G.reshape(130, -1), fd.reshape(130, -1))
    print(f"{kernel} D={D} E={E}: restatement vs central differences {err:.2e}")
    assert err <= 1e-6, (kernel, D, E, err)


def test_restatement_conventions_on_the_golden_cases():
    """Non-finite rows: exactly the rows of a coincident pair the inverse-distance zero rule does not drop -- {5, 40} of the
    same-points duplicate case, {7} of the other -- and complete there (every component); nowhere else, in particular not at
    the own pairs of same_points (exp(-r): s == 0 contributes 0) nor in the Gaussian's duplicate case."""
    cases = gradient_cases()
    assert len(cases) == 60
    seen = {}
    for case in cases:
        y, x, b = golden_cases.make_inputs(case)
        G = grad_reference.gradient(kernel=case["kernel"], source_points=y, target_points=x, source_signal=b)
        assert G.shape == (case["N"], case["E"], case["D"])
        bad = ~np.isfinite(G).reshape(case["N"], -1)
        assert (bad.any(axis=1) == bad.all(axis=1)).all(), case["name"]
        rows = set(np.nonzero(bad.any(axis=1))[0].tolist())
        if rows:
            seen[case["name"]] = rows
    assert seen == {"inverse-distance-N64-M64-D3-E1-sp-dup": {5, 40}, "inverse-distance-N70-M64-D3-E1-dup": {7}}, seen


def test_restatement_shards_add_up_with_the_global_zero_rule():
    """j_offset / M_total as kmvp_oracle.kernel_block: source slices of 1/r (N > M: the rule wraps) sum to the whole."""
    rs = np.random.RandomState(5)
    y, x, b = rs.rand(64, 3), rs.rand(150, 3), rs.randn(64, 2)
    whole = grad_reference.gradient(kernel="inverse-distance", source_points=y, target_points=x, source_signal=b)
    parts = sum(grad_reference.gradient(kernel="inverse-distance", source_points=y[lo:hi], target_points=x,
                                        source_signal=b[lo:hi], j_offset=lo, M_total=64)
                for lo, hi in ((0, 20), (20, 45), (45, 64)))
    assert rel_err(parts.reshape(150, -1), whole.reshape(150, -1)) <= 1e-13
