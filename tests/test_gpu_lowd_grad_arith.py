"""lowd_grad_kernel (kmvp_<kernel>_grad) and lowd_dscale_kernel (kmvp_<kernel>_dscale) held element by element to the
float64 model of their arithmetic (oracle/kmvp_lowd_grad_model.py): |got - value| <= band on EVERY element -- not
relative to the heaviest row --, the band derived term by term in the model's docstring, nothing fitted to kernel
output; the rows the model calls non-finite (a NaN target, a coincident 1/r pair that is not zeroed) are non-finite here
in every component, and no others; every run asserts the device kernel's name and an empty dispatch note.  MAXIMA collects
err / band, err / mass and band / mass per (device kernel, kernel function, precision, near / far) for the record
(pytest -s).

The clouds and configurations come from tests/lowd_grad_model_cases.py, where tests/test_lowd_grad_model.py keeps clean
emulations of the kernels' steps inside the band on the same clouds and shows that an emulation with one defect leaves
it."""
import os
import re

import numpy as np
import pytest

import kmvp_lowd_model as lm
import lowd_grad_model_cases as gc
from kernel_matrix_benchmarks_amd import _lib

pytestmark = pytest.mark.gpu

# (device kernel, kernel function, precision, far) -> [max err / band, max err / mass, max band / mass, elements]
MAXIMA = {}
PREC = {"f32": np.float32, "f64": np.float64}
DTYPE = {np.dtype(np.float32): _lib.KMVP_F32, np.dtype(np.float64): _lib.KMVP_F64}
EACH = [(kernel, p) for kernel in gc.KERNELS for p in PREC]
IDS = [f"{k}-{p}" for k, p in EACH]
CSRC = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lowd_grad_parent.npz")


def check(c, cfg, got, model, what, failures):
    """The elements the model calls poisoned (the non-finite rows in every component; the axis of a non-finite source
    coordinate, the column of a NaN signal entry in every row) are non-finite; every other element is finite and within
    the band -- but on a `loose` case (a non-finite source coordinate), where an element that is not poisoned may be
    non-finite too, and is within the band of the other sources' sum if it is finite."""
    msg = None
    bad = model.poisoned
    loose = bool(c["kw"].get("loose"))
    if got.shape != model.value.shape:
        msg = f"shape {got.shape}"
    elif np.isfinite(got[bad]).any():
        rows = np.nonzero((bad & np.isfinite(got)).any(axis=(1, 2)))[0]
        msg = f"finite where the model is not: rows {rows[:8]}, e.g. {got[rows[0]].ravel()[:6]}"
    elif not loose and not np.isfinite(got[~bad]).all():
        msg = f"non-finite rows {np.nonzero((~np.isfinite(got) & ~bad).any(axis=(1, 2)))[0][:8]}"
    else:
        must = ~bad & np.isfinite(got)
        if must.any():
            err, band, mass = np.abs(got - model.value)[must], model.band[must], model.mass[must]
            with np.errstate(divide="ignore", invalid="ignore"):
                ratio = np.where(band > 0, err / band, np.where(err > 0, np.inf, 0.0))
                r = MAXIMA.setdefault((gc.NAME[cfg[0]], c["kernel"], c["precision"].name, c["name"][0] == "far"), [0.0, 0.0, 0.0, 0])
                r[0] = max(r[0], float(ratio.max()))
                r[1] = max(r[1], float(np.where(mass > 0, err / mass, 0.0).max()))
                r[2] = max(r[2], float(np.where(mass > 0, band / mass, 0.0).max()))
                r[3] += ratio.size
            if (err > band).any():
                k = int(np.argmax(ratio))
                i, e, d = (a[k] for a in np.nonzero(must))
                msg = (f"err/band {ratio.max():.3g} at row {i} column {e} axis {d}: err {err[k]:.3g} band {band[k]:.3g} "
                       f"mass {mass[k]:.3g}; {int((err > band).sum())} elements")
    if msg is not None:
        failures.append((what, msg))


class Grad:
    """One context on a case's clouds (or a slice of its sources) in the case's precision."""

    def __init__(self, c, lo=None, hi=None, M_total=None):
        self.ctx = _lib.Context(0)
        self.ctx.set_option("fast_sqdists", 0)                  # (for the products of the state test: the difference form)
        self.lo, self.hi = lo, hi
        self.set_points(c, M_total)

    def set_points(self, c, M_total=None):
        self.c = c
        dt = c["precision"]
        self.y = np.ascontiguousarray(c["y"][self.lo:self.hi], dtype=dt)
        x = c["x"]
        self.N = len(self.y) if x is None else len(x)
        self.ctx.set_points(self.y, None if x is None else np.ascontiguousarray(x, dtype=dt), DTYPE[dt], self.lo or 0, M_total)

    def run(self, cfg, options=()):
        which, sig, E, chunk, segments = cfg
        c = self.c
        for k, v in (("chunk", chunk), ("segments", segments)) + tuple(options):
            self.ctx.set_option(k, v)
        b = gc.signal_of(c, sig, E)
        self.ctx.set_signal(None if b is None else np.ascontiguousarray(b[self.lo:self.hi]))
        (self.ctx.run_dscale if which == "dscale" else self.ctx.run_grad)(c["kernel"])
        name, note = self.ctx.last_kernel_name, self.ctx.last_dispatch_note
        assert name == gc.NAME[which] and note == "", (c["name"], cfg, name, note)
        EC, D = (1 if b is None else b.shape[1]), self.y.shape[1]
        return self.ctx.get_result(self.N, EC * D).reshape(self.N, EC, D)       # column e D + d

    def product(self, T):
        self.ctx.set_option("targets_per_lane", T)
        self.ctx.run(self.c["kernel"], False)
        assert self.ctx.last_kernel_name == "lowd_kernel"

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.close()


def model_of(c, cfg, cache):
    """The model of one configuration; configurations whose longest chain is the same share it."""
    key = cfg[:3] + (lm.chain_length("lowd", c["precision"], len(c["y"]), cfg[3], 1),)
    if key not in cache:
        cache[key] = gc.model(c, cfg)
    return cache[key]


def run_cases(case_list, failures, reached=None):
    for c in case_list:
        cache = {}
        with Grad(c) as g:
            for cfg in gc.configs(c):
                model = model_of(c, cfg, cache)
                assert list(np.nonzero(model.nonfinite)[0]) == c["kw"].get("bad_rows", []), (c["name"], cfg)
                check(c, cfg, g.run(cfg), model, (c["name"], cfg), failures)
                if reached is not None:
                    reached.add((cfg[0], c["y"].shape[1], cfg[1], cfg[2]))


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for (kname, fn, prec, far), (eb, em, bm, n) in sorted(MAXIMA.items()):
        print(f"\nlowd grad model {kname:18s} {fn:22s} {prec} {'far ' if far else 'near'}: max |err|/band {eb:.3g}  max |err|/mass {em:.3g}  "
              f"max band/mass {bm:.3g}  ({n} elements)")


def inst_grid(which):
    """(which, D, sig, E) of every instantiation of one kernel function and precision, read from the unit that makes them:
    one `case D:` per launch_e<D>, one `case E:` per launch_one<D, E, SIG_PRODUCT>, and the density variant."""
    text = open(os.path.join(CSRC, f"kmvp_lowd_{which}_inst.hip")).read()
    assert f"lowd_{which}_kernel<KERNEL, D, E, SIG, real>" in text
    dims = sorted(int(d) for d, d2 in re.findall(r"case (\d+): return launch_e<(\d+)>", text) if d == d2)
    cols = sorted(int(e) for e, e2 in re.findall(r"case (\d+): return launch_one<D, (\d+), SIG_PRODUCT>", text) if e == e2)
    assert "launch_one<D, 1, SIG_DENSITY>" in text and dims and cols
    return {(which, D, sig, E) for D in dims for sig, E in [("product", e) for e in cols] + [("density", 1)]}


def test_the_grids_are_eight_dimensions_by_four_columns_and_density():
    for which in ("grad", "dscale"):
        assert inst_grid(which) == {(which, D, s, e) for D in range(1, 9) for s, e in gc.MODES}


@pytest.mark.parametrize("kernel,prec", EACH, ids=IDS)
def test_every_instantiation(kernel, prec):
    """D = 1 ... 8 x (E = 1 ... 4 and density), N = 67 targets != M = 101 sources and the same points at D = 3, chunk = 8
    and 512, signal columns distinct in scale and sign; the reached set equals the grid of the two _inst.hip units."""
    reached, failures = set(), []
    run_cases(gc.grid_cases(kernel, PREC[prec]), failures, reached)
    assert not failures, (len(failures), failures[:8])
    grid = set().union(*(inst_grid(w) for w in gc.whiches(kernel)))
    assert reached == grid, sorted(grid ^ reached)[:20]


@pytest.mark.parametrize("kernel,prec", EACH, ids=IDS)
def test_edges_of_every_loop(kernel, prec):
    """N of 1 ... 257 and M of 1 ... 1030 around every batch, guard zone (M <= 8: every batch guarded), LDS tile and fold,
    chunk = 8, 256, 512; N = 65 x M = 1030 under 1, 2, 3 and 17 segments."""
    failures = []
    run_cases(gc.groups(kernel, PREC[prec])["edges"], failures)
    assert not failures, (len(failures), failures[:8])


@pytest.mark.parametrize("kernel,prec", EACH, ids=IDS)
def test_range_and_exact_rules(kernel, prec):
    """Clouds at +100; targets whose exponent runs through the flush and the Matern clamp (float32) and through the
    denormal range, exact zeros and the clamp at 800 (float64); the overflowing squared distance (float32); duplicated
    points (exp(-r) at s = 0; 1/r: coincident pairs, non-finite rows); 1/r: the zero column wrapping inside a tile and
    across tiles."""
    failures = []
    run_cases(gc.groups(kernel, PREC[prec])["range"], failures)
    assert not failures, (len(failures), failures[:8])


@pytest.mark.parametrize("kernel,prec", EACH, ids=IDS)
def test_non_finite_inputs(kernel, prec):
    """A NaN target at M = 5, 8 (every batch guarded) and 101, for 1/r also inside a wrapping tile: its row is non-finite
    in every component, every other row in band.  A NaN, +inf or -inf source coordinate at j = 0, in the middle and in
    the guard zone: include/kmvp.h's rule, the same at all three positions -- the components of that axis are non-finite
    in every row, every other element is non-finite too or the other sources' sum.  A NaN signal entry: its column is
    non-finite in every row, the other column in band."""
    failures = []
    run_cases(gc.groups(kernel, PREC[prec])["nonfinite"], failures)
    assert not failures, (len(failures), failures[:8])


@pytest.mark.parametrize("prec", list(PREC))
def test_zero_rule_on_three_source_slices(prec):
    """1/r, N = 450 > M_total + 1, on the slices (0, 67), (67, 131), (131, 200) with j_offset / M_total under
    partial_shard: each slice inside its own model, and the partial results add up to the whole's model."""
    failures = []
    c = list(gc.zero_rule_cases(PREC[prec]))[0]
    M = len(c["y"])
    cfgs = list(gc.configs(c))
    total = {cfg: 0.0 for cfg in cfgs}
    for lo, hi in gc.SHARDS:
        part = dict(c, y=c["y"][lo:hi], b=c["b"][lo:hi], kw=dict(j_offset=lo, M_total=M))
        cache = {}
        with Grad(c, lo, hi, M_total=M) as g:
            for cfg in cfgs:
                got = g.run(cfg, [("partial_shard", 1)])
                check(part, cfg, got, model_of(part, cfg, cache), (c["name"], cfg, (lo, hi)), failures)
                total[cfg] = total[cfg] + got
    cache = {}
    for cfg in cfgs:
        check(c, cfg, total[cfg], model_of(c, cfg, cache), (c["name"], cfg, "three slices"), failures)
    assert not failures, (len(failures), failures[:8])


@pytest.mark.parametrize("prec", list(PREC))
def test_state_on_one_context(prec):
    """On one context: a product (one target per lane), the gradient, the derivative, a new signal, the gradient, density,
    another kernel function, a product with two targets per lane and then the gradient, new points.  Every result is in
    band and bit-equal to the same call on a fresh context: the packed records are rebuilt exactly when they must be,
    and the segments are summed in index order."""
    failures = []
    dt = PREC[prec]
    c = [c for c in gc.grid_cases("gaussian", dt) if c["name"][:1] == ("grid",) and c["name"][2] == 3][0]
    rs = np.random.RandomState(3)
    c2 = dict(c, b=gc.signal(rs, *c["b"].shape, dt))
    c3 = dict(c2, kernel="matern-5/2")
    c4 = dict(c3, y=gc.cases.points(rs, *c["y"].shape, dt), x=gc.cases.points(rs, *c["x"].shape, dt))
    g2, d2, gd = ("grad", "product", 2, 512, 0), ("dscale", "product", 2, 512, 0), ("grad", "density", 1, 512, 0)
    steps = ((c, 1, g2), (c, 0, d2), (c2, 0, g2), (c2, 0, gd), (c3, 0, ("grad", "product", 3, 8, 2)), (c3, 2, g2), (c4, 0, g2), (c4, 0, d2))
    with Grad(c) as g:
        for cc, T, cfg in steps:                                   # T: a product with T targets per lane first
            if cc is c4 and g.c is not c4:
                g.set_points(c4)
            g.c = cc
            if T:
                g.ctx.set_signal(np.ascontiguousarray(cc["b"][:, :2]))
                g.product(T)
            got = g.run(cfg)
            check(cc, cfg, got, model_of(cc, cfg, {}), (cc["kernel"], cfg, "reuse"), failures)
            with Grad(cc) as fresh:
                assert np.array_equal(got, fresh.run(cfg), equal_nan=True), (cc["kernel"], cfg, "fresh context")
    assert not failures, (len(failures), failures[:8])


def test_finite_inputs_give_the_bits_recorded_before_the_guard_changed():
    """tests/golden/lowd_grad_parent.npz holds both kernels' results on gc.golden_cases(), recorded from the library of the
    commit before the guard's select went from the squared distance to the record's index and the NaN row was restored:
    M = 37 has three pad records and a guard zone that holds real sources too.  Bit for bit."""
    want = np.load(GOLDEN)
    seen = 0
    for c in gc.golden_cases():
        with Grad(c) as g:
            for which in gc.whiches(c["kernel"]):
                got = g.run((which, "product", 2, 512, 0))
                assert np.array_equal(got, want[gc.golden_key(c, which)]), (c["kernel"], c["precision"].name, which)
                seen += 1
    assert seen == len(want.files) == 18
