"""GPU tests of the device-side build of the cutoff plan ("cutoff_plan" = 1, kmvp_cutoff_plan_read of include/kmvp.h;
csrc/kmvp_cutoff_plan_device.hip).

The contract is equality, not accuracy: for the points as the context holds them the device-built plan is the numpy
restatement's (cutoff_reference.plan, which tests/test_host_cutoff_plan.py holds to the host build) entry for entry, and so
every cutoff entry returns the same bits under either value of the option.  No tolerance anywhere in this file."""
import numpy as np
import pytest

import cutoff_plan_cases as cases
import cutoff_reference as cr
from kernel_matrix_benchmarks_amd import _lib
from kernel_matrix_benchmarks_amd.algorithms.mi355x import MI355XProduct, MI355XSolver

pytestmark = pytest.mark.gpu

PREC = {"f32": np.float32, "f64": np.float64}
INVALID = 1


def codes(precision):
    return (_lib.KMVP_F64, np.float64) if np.dtype(precision) == np.float64 else (_lib.KMVP_F32, np.float32)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)


class Ctx:
    """One context on sources y and targets x (None: the sources), its plan built on `side`."""

    def __init__(self, y, x, precision, side):
        self.dtype, self.npdt = codes(precision)
        self.ctx = _lib.Context(0)
        try:
            self.ctx.set_option("cutoff_plan", _lib.CUTOFF_PLAN_SIDES.index(side))
            self.points(y, x)
        except Exception:
            self.ctx.close()
            raise

    def points(self, y, x):
        self.ctx.set_points(np.ascontiguousarray(y, dtype=self.npdt), None if x is None else np.ascontiguousarray(x, dtype=self.npdt),
                            self.dtype)

    def plan(self, R, factor=1.0):
        """The plan a neighbour count at R builds (or finds cached), read back."""
        self.ctx.set_option("cutoff_cell_factor", factor)
        self.ctx.radius_count(R)
        return self.ctx.cutoff_plan()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.close()


def reference(y, x, R, factor):
    return cr.plan(y, y if x is None else x, R, factor)


# ---- (a), (b): the plan, entry for entry, from either side ------------------------------------------------------------------
@pytest.mark.parametrize("side", ["device", "host"])
@pytest.mark.parametrize("prec", list(PREC))
def test_plan_equals_the_reference(prec, side):
    """Every case of cutoff_plan_cases.cases(): the test clouds at two cell factors, D = 1, 2, 3 with the targets the sources
    and not, and the shapes at which a stage can go wrong (rows of 64 and 65 targets, ties across a tile boundary, loose
    tiles, non-finite and empty sides, one cell, the cell cap's loop, empty rows, float neighbours of the cell boundaries).
    The read-back copies from the buffers the kernels read, so the host side checks the upload as well."""
    seen = {}
    for name, y, x, R, factor in cases.cases(PREC[prec]):
        with Ctx(y, x, PREC[prec], side) as ct:
            got = ct.plan(R, factor)
            assert got.pop("built_on") == side, name
            try:
                cases.equal_plans(got, reference(y, x, R, factor))
            except AssertionError as e:
                raise AssertionError(f"{name} ({prec}, {side}): {e}") from None
            info = ct.ctx.cutoff_info()
            assert info["built_on"] == side and info["cells"] == tuple(got["g"]) and info["walked"] == got["walked"], name
            seen[name] = got
    assert any(p["live_tiles"] % cr.WAVES for p in seen.values())                 # a tile count that is no multiple of 4
    assert seen["130 loose targets"]["tiles"][seen["130 loose targets"]["live_tiles"] - 3, 1] == 0
    assert seen["cell cap"]["h"] > 2e-9 and np.all(seen["one cell"]["g"] == 1) and seen["N = 0"]["n_pad"] == 0


def test_read_before_any_plan_is_refused():
    ctx = _lib.Context(0)
    try:
        with pytest.raises(_lib.KmvpError) as e:
            ctx.cutoff_plan()
        assert e.value.code == INVALID
        ctx.set_points(np.random.RandomState(0).rand(40, 3).astype(np.float32), None, _lib.KMVP_F32)
        with pytest.raises(_lib.KmvpError) as e:
            ctx.cutoff_plan()
        assert e.value.code == INVALID
    finally:
        ctx.close()


# ---- (c): the same bits from every entry ----------------------------------------------------------------------------------------
def every_entry(ct, R, E_signals, solve):
    """Every cutoff entry's result on one context, as a list of (name, array); the Wendland solve where `solve`."""
    ctx, out = ct.ctx, []
    N = ctx.N
    for E, b in E_signals.items():
        ctx.set_signal(np.ascontiguousarray(b, dtype=ct.npdt))
        for kernel in ("gaussian", "matern-5/2"):
            ctx.run_cutoff(kernel, R, False)
            out.append((f"{kernel} E={E}", ctx.get_result(N, E)))
        ctx.run_cutoff("gaussian", R, True)
        out.append((f"gaussian normalised E={E}", ctx.get_result(N, E)))
        ctx.run_cutoff_grad("gaussian", R)
        out.append((f"gaussian gradient E={E}", ctx.get_result(N, E * ctx.D)))
        ctx.run_cutoff("wendland-c2", R, False)
        out.append((f"wendland-c2 E={E}", ctx.get_result(N, E)))
    ctx.set_signal(None)
    ctx.run_cutoff("gaussian", R, False)
    out.append(("density", ctx.get_result(N, 1)))
    out.append(("count", ctx.radius_count(R)))
    out.append(("count exclude_self", ctx.radius_count(R, True)))
    for K in (1, 4, 16):
        idx, sq = ctx.radius_nearest(R, K)
        out += [(f"nearest {K} idx", idx), (f"nearest {K} sqdist", sq)]
    if not solve:
        return out
    a = np.ascontiguousarray(E_signals[1], dtype=ct.npdt)
    ctx.set_solver_diagonal(None, 0.05)
    sol, its, res, ok = ctx.cg_solve("wendland-c2", a, 1e-4, 200, support_radius=R)
    out += [("cg solution", sol), ("cg iterations", np.array([its, int(ok)])), ("cg residual", np.array([res]))]
    return out


@pytest.mark.parametrize("prec", list(PREC))
def test_every_entry_returns_the_same_bits(prec):
    rs = np.random.RandomState(11)
    clean = rs.rand(1500, 3)
    marked = clean.copy()
    marked[[7, 300], [0, 2]] = [np.nan, np.inf]           # NaN rows compare as NaN; the solve runs on the clean cloud
    R = 0.13
    signals = {1: rs.randn(1500, 1), 4: rs.randn(1500, 4)}
    for y, solve in ((marked, False), (clean, True)):
        with Ctx(y, None, PREC[prec], "host") as h, Ctx(y, None, PREC[prec], "device") as d:
            want, got = every_entry(h, R, signals, solve), every_entry(d, R, signals, solve)
            assert h.ctx.cutoff_info()["built_on"] == "host" and d.ctx.cutoff_info()["built_on"] == "device"
        assert [n for n, _ in got] == [n for n, _ in want] and len(want) == (22 if solve else 19)
        for (name, a), (_, b) in zip(got, want):
            assert same(a, b), (name, prec, solve)
        if solve:
            assert dict(want)["cg iterations"][0] > 1 and np.isfinite(dict(want)["cg solution"]).all()
        else:
            assert np.isnan(dict(want)["gaussian E=1"][7]).all() and dict(want)["count"][7] == -1


def test_plugins_carry_the_option():
    rs = np.random.RandomState(5)
    y, b = rs.rand(900, 3), rs.randn(900, 1)
    results = {}
    for side in ("host", "device"):
        algo = MI355XProduct(kernel="gaussian", dimension=3, precision="float32", cutoff_plan=side)
        try:
            algo.prepare_data(source_points=y, target_points=y[:200] + 0.01, same_points=False)
            algo.prepare_query(source_signal=b)
            algo.query_cutoff(0.2)
            results[side] = algo.get_result()
            assert algo.get_additional()["cutoff_built_on"] == side
        finally:
            algo.done()
        solver = MI355XSolver(kernel="wendland-c2", dimension=3, precision="float32", support_radius=0.2, ridge=0.01, rtol=1e-4,
                              cutoff_plan=side)
        try:
            solver.prepare_data(source_points=y)
            solver.prepare_query(target_signal=b)
            solver.query()
            results["solve " + side] = solver.get_result()
            assert solver.get_additional()["cutoff_built_on"] == side
        finally:
            solver.done()
    assert same(results["host"], results["device"]) and same(results["solve host"], results["solve device"])


# ---- (d): cache and isolation ----------------------------------------------------------------------------------------------------
def test_cache_and_isolation():
    rs = np.random.RandomState(21)
    y, x, b = rs.rand(1200, 3), rs.rand(500, 3), rs.randn(1200, 2)
    R = 0.15
    with Ctx(y, x, np.float32, "host") as ct:
        ctx = ct.ctx
        ctx.set_signal(b.astype(np.float32))

        def others():
            ctx.run("gaussian", False)
            plain = ctx.get_result(500, 2)
            return [plain, *ctx.run_nearest(3)]

        before = others()
        ctx.run_cutoff("gaussian", R, False)
        first, count = ctx.get_result(500, 2), ctx.radius_count(R)
        assert ctx.cutoff_info()["built_on"] == "host"
        # flipping the option between two calls rebuilds the plan; the results stay
        ctx.set_option("cutoff_plan", 1)
        ctx.run_cutoff("gaussian", R, False)
        assert ctx.cutoff_info()["built_on"] == "device" and same(ctx.get_result(500, 2), first)
        plan = ctx.cutoff_plan()
        assert same(ctx.radius_count(R), count) and ctx.cutoff_info()["built_on"] == "device"
        for a, b_ in zip(others(), before):              # every other entry: the same bits before and after device-plan calls
            assert same(a, b_)
        # run to run
        ctx.set_option("cutoff_cell_factor", 1.5)
        ctx.radius_count(R)
        ctx.set_option("cutoff_cell_factor", 1.0)
        ctx.run_cutoff("gaussian", R, False)
        again = ctx.cutoff_plan()
        assert same(ctx.get_result(500, 2), first) and all(same(np.asarray(again[k]), np.asarray(plan[k])) for k in plan if k != "built_on")
        ctx.set_option("cutoff_plan", 0)
        ctx.radius_count(R)
        assert ctx.cutoff_info()["built_on"] == "host"
        ctx.set_option("cutoff_plan", 1)
        # new points: the new reference plan
        y2, x2 = rs.rand(700, 3) * 2.0, rs.rand(333, 3) * 2.0
        ct.points(y2, x2)
        got = ct.plan(R)
        assert got.pop("built_on") == "device"
        cases.equal_plans(got, reference(np.asarray(y2, dtype=np.float32).astype(np.float64), np.asarray(x2, dtype=np.float32).astype(np.float64), R, 1.0))


def test_batched_product_is_untouched():
    rs = np.random.RandomState(22)
    y, b = rs.rand(900, 3).astype(np.float32), rs.randn(900, 1).astype(np.float32)
    offsets = np.array([0, 300, 900])
    ctx = _lib.Context(0)
    try:
        ctx.set_option("cutoff_plan", 1)
        ctx.set_points(y, None, _lib.KMVP_F32)
        ctx.set_signal(b)
        ctx.set_batches(offsets)
        ctx.run("gaussian", False)
        before = ctx.get_result(900, 1)
        ctx.set_batches(None)
        ctx.run_cutoff("gaussian", 0.2, False)
        assert ctx.cutoff_info()["built_on"] == "device"
        ctx.set_batches(offsets)
        ctx.run("gaussian", False)
        assert same(ctx.get_result(900, 1), before)
    finally:
        ctx.close()


# ---- (e): option values ----------------------------------------------------------------------------------------------------------
def test_option_values():
    ctx = _lib.Context(0)
    try:
        for bad in (2, -1):
            with pytest.raises(_lib.KmvpError) as e:
                ctx.set_option("cutoff_plan", bad)
            assert e.value.code == INVALID
        ctx.set_option("cutoff_plan", 1)
        ctx.set_option("cutoff_plan", 0)
    finally:
        ctx.close()
