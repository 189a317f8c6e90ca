"""CPU tests of the regularised solves (K + ridge I + diag(d)) b = a: the plugin's ``ridge`` contract, the declaration of
``kmvp_set_solver_diagonal`` against its binding, and the scaling the exp-dot route hands to the library.
No compute call is made here -- there is no GPU (the solves themselves: test_gpu_solver_ridge.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

from kernel_matrix_benchmarks_amd import _lib
from kernel_matrix_benchmarks_amd.algorithms import mi355x

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CG_KERNELS = ("gaussian", "absolute-exponential", "exp-dot")


def test_ridge_constructor_contract():
    for kernel in CG_KERNELS + ("inverse-distance",):
        plain = mi355x.MI355XSolver(kernel=kernel, dimension=3)
        method = "minres" if kernel == "inverse-distance" else "cg"
        # without a ridge nothing moves: name (result files of existing runs), method, the default itself
        assert plain.name == f"MI355XSolver(float64, {method}, rtol=1e-06)" and plain.method == method
        assert plain.ridge == 0.0 and "ridge" not in plain.get_additional()  # (the fresh instance's record is pinned too)
        assert mi355x.MI355XSolver(kernel=kernel, dimension=3, ridge=0.0).name == plain.name
        with_ridge = mi355x.MI355XSolver(kernel=kernel, dimension=3, ridge=0.1)
        assert with_ridge.name == f"MI355XSolver(float64, {method}, rtol=1e-06, ridge=0.1)" and with_ridge.method == method
        assert with_ridge.ridge == 0.1 and with_ridge.get_additional()["ridge"] == 0.1
        per_point = mi355x.MI355XSolver(kernel=kernel, dimension=3, ridge=np.array([0.05, 0.2, 0.1]))
        assert per_point.name.startswith(plain.name[:-1] + ", ridge=") and per_point.name != with_ridge.name
        assert per_point.get_additional()["ridge"] == 0.2  # the vector's largest value
        assert np.array_equal(per_point.ridge, [0.05, 0.2, 0.1])
        assert isinstance(mi355x.MI355XSolver(kernel=kernel, dimension=3, ridge=1).ridge, float)  # an int is a number too
    refined = mi355x.MI355XSolver(kernel="gaussian", dimension=3, refine="float32", ridge=0.5)
    assert refined.name == "MI355XSolver(float64, cg + refinement on float32, rtol=1e-06, ridge=0.5)"
    assert mi355x.MI355XSolver(kernel="gaussian", dimension=3, refine="float32").name == (
        "MI355XSolver(float64, cg + refinement on float32, rtol=1e-06)")


def test_ridge_value_errors():
    for kernel in CG_KERNELS:  # positive definite only with a non-negative shift
        with pytest.raises(ValueError):
            mi355x.MI355XSolver(kernel=kernel, dimension=3, ridge=-1e-3)
        with pytest.raises(ValueError):
            mi355x.MI355XSolver(kernel=kernel, dimension=3, ridge=[0.1, -0.1])
    # MINRES: a shifted indefinite system is still symmetric
    assert mi355x.MI355XSolver(kernel="inverse-distance", dimension=3, ridge=-10.0).ridge == -10.0
    assert mi355x.MI355XSolver(kernel="inverse-distance", dimension=3, ridge=[1.0, -1.0]).get_additional()["ridge"] == 1.0
    for kernel in ("gaussian", "inverse-distance"):
        for bad in (float("nan"), float("inf"), [0.1, float("nan")], "much", np.ones((2, 2)), []):
            with pytest.raises(ValueError):
                mi355x.MI355XSolver(kernel=kernel, dimension=3, ridge=bad)


class Recorder:
    """Stands in for _lib.Context: records what the plugin hands to the library."""

    comm_world = 0
    last_kernel_name = ""
    rccl_ranks = 1

    def __init__(self, device=0):
        self.diagonals = []
        self.solves = 0

    def set_option(self, key, value):
        pass

    def set_points(self, y, x, dtype, j_offset=0, M_total=None):
        self.M = y.shape[0] if M_total is None else M_total
        self.diagonals.append("set_points")  # (the library clears its diagonal here)

    def set_solver_diagonal(self, d, ridge=0.0):
        self.diagonals.append((None if d is None else np.array(d, dtype=np.float64, copy=True), float(ridge)))

    def cg_solve(self, kernel, a, rtol, maxit):
        self.solves += 1
        return np.zeros(a.shape), 0, 0.0, True

    def set_signal(self, b):
        self.E = b.shape[1]

    def run(self, kernel, normalize):
        pass

    def get_result(self, N, E):
        return np.zeros((N, E))

    def close(self):
        pass


def test_set_query_arguments_and_when_the_library_is_told(monkeypatch):
    monkeypatch.setattr(_lib, "Context", Recorder)
    y = np.random.RandomState(0).rand(40, 3)
    a = np.ones((40, 1))
    s = mi355x.MI355XSolver(kernel="gaussian", dimension=3)
    s.prepare_data(source_points=y)
    s.prepare_query(target_signal=a)
    s.query()
    assert s._ctx.diagonals == ["set_points"], "without a ridge the library's diagonal is never touched"
    s.set_query_arguments(ridge=0.25)
    assert s.ridge == 0.25 and s.name.endswith(", ridge=0.25)") and s._ctx.diagonals == ["set_points"]  # ... at the next query()
    s.query()
    s.query()  # unchanged: not handed down again
    assert len(s._ctx.diagonals) == 2 and s._ctx.diagonals[1][0] is None and s._ctx.diagonals[1][1] == 0.25
    d = np.linspace(0.05, 0.2, 40)
    s.set_query_arguments(ridge=d, rtol=1e-3)
    assert s.rtol == 1e-3
    s.query()
    assert np.array_equal(s._ctx.diagonals[2][0], d) and s._ctx.diagonals[2][1] == 0.0
    s.set_query_arguments(maxit=7)  # other arguments leave the ridge alone
    assert s.maxit == 7 and np.array_equal(s.ridge, d)
    s.set_query_arguments(ridge=0.0)
    assert s.name == "MI355XSolver(float64, cg, rtol=1e-06)"
    s.query()
    assert s._ctx.diagonals[3][0] is None and s._ctx.diagonals[3][1] == 0.0  # switched off in the library too
    # new points clear the library's diagonal: a ridge that is still set goes down again
    s.set_query_arguments(ridge=0.5)
    s.query()
    s.prepare_data(source_points=y)
    s.prepare_query(target_signal=a)
    s.query()
    assert s._ctx.diagonals[-2] == "set_points" and s._ctx.diagonals[-1][1] == 0.5
    # the errors of the constructor, and the length once M is known
    for bad in (-0.1, float("nan"), np.ones(39), np.ones(41)):
        with pytest.raises(ValueError):
            s.set_query_arguments(ridge=bad)
    assert s.ridge == 0.5, "a refused value leaves the old one"
    late = mi355x.MI355XSolver(kernel="gaussian", dimension=3, ridge=np.ones(39))
    with pytest.raises(ValueError):
        late.prepare_data(source_points=y)
    # refine="float32": the inner float32 context gets the same diagonal
    r = mi355x.MI355XSolver(kernel="gaussian", dimension=3, refine="float32", ridge=d)
    r.prepare_data(source_points=y)
    r.prepare_query(target_signal=a)
    r.query()
    for ctx in (r._ctx, r._ctx32):
        assert np.array_equal(ctx.diagonals[-1][0], d) and ctx.diagonals[-1][1] == 0.0


def declaration(name):
    text = open(os.path.join(ROOT, "include", "kmvp.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, f"include/kmvp.h does not declare {name}"
    return m.group(1), [" ".join(p.split()) for p in m.group(2).split(",")]


def test_set_solver_diagonal_is_declared_bound_and_exported():
    restype, params = declaration("kmvp_set_solver_diagonal")
    assert restype == "int"
    assert params == ["kmvp_ctx* ctx", "const double* d_or_null", "int64_t n", "double ridge"]
    bound = {s[0]: s for s in _lib.SYMBOLS}
    assert "kmvp_set_solver_diagonal" in bound, "the binding table lacks kmvp_set_solver_diagonal"
    _, res, args = bound["kmvp_set_solver_diagonal"]
    assert res is ctypes.c_int
    assert args == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_double]  # pointers as void*, like every entry
    assert hasattr(_lib.load(), "kmvp_set_solver_diagonal")
    assert _lib.load().kmvp_abi_version() == 1  # purely additive
    # the typed wrapper refuses what the library would misread, before any call (no GPU: never bound to a kmvp_ctx)
    c = _lib.Context.__new__(_lib.Context)
    c._ctx = None
    with pytest.raises(ValueError):
        _lib.Context.set_solver_diagonal(c, np.ones((5, 2)), 0.0)
    # a NULL ctx is refused by the library itself (no device needed)
    assert _lib.load().kmvp_set_solver_diagonal(None, None, 0, 0.0) == 1  # KMVP_E_INVALID


@pytest.mark.parametrize("lam", [0.3, "per-point"])
def test_exp_dot_hands_the_library_the_scaled_diagonal(monkeypatch, lam):
    """K = D G D with D = diag(exp(|x|^2/2)): (K + L) b = a is (G + D^-1 L D^-1) z = D^-1 a, so the library must get
    l_i exp(-|x_i|^2) per point, in float64."""
    monkeypatch.setattr(_lib, "Context", Recorder)
    rs = np.random.RandomState(3)
    x = rs.rand(25, 3) * 1.5
    lam_i = np.full(25, lam) if lam != "per-point" else rs.uniform(0.05, 0.2, 25)
    s = mi355x.MI355XSolver(kernel="exp-dot", dimension=3, precision=np.float64, ridge=lam if lam != "per-point" else lam_i)
    s.prepare_data(source_points=x)
    s.prepare_query(target_signal=rs.randn(25, 2))
    s.query()
    (d, ridge), = [e for e in s._ctx.diagonals if e != "set_points"]
    want = lam_i * np.exp(-np.sum(x * x, axis=1))
    assert ridge == 0.0 and d.dtype == np.float64 and d.shape == (25,)
    assert np.max(np.abs(d - want) / want) <= 1e-14
    assert s.get_additional()["ridge"] == np.max(lam_i)  # reported on the caller's scale
