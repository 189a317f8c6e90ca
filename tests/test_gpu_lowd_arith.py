"""The pair-loop kernels of the difference form (lowd_kernel, lowd_mid_kernel, lowd_big_kernel) held element by element to
the float64 model of their arithmetic (oracle/kmvp_lowd_model.py): |got - value| <= band on every element, the band
derived term by term in the model's docstring, nothing fitted to kernel output; no row is ever flagged; the rows the model
calls non-finite (a NaN target, a planted coincident 1/r pair, 0 / 0) are non-finite here and no others.  Every run forces
the difference form (fast_sqdists = 0), asserts the device kernel's name and -- where a (T, feed) pair is requested -- the
pair the dispatch note says ran.  MAXIMA collects err / band, err / mass and band / mass per (device kernel, kernel
function, precision) for the record (pytest -s).

The clouds and configurations come from tests/lowd_model_cases.py, where tests/test_lowd_model.py keeps clean emulations
of the kernels' steps inside the band on the same clouds and shows that an emulation with one defect leaves it."""
import numpy as np
import pytest

import kmvp_lowd_model as lm
import lowd_model_cases as cases
from kernel_matrix_benchmarks_amd import _lib

pytestmark = pytest.mark.gpu

# (device kernel, kernel function, precision, far) -> [max err / band, max err / mass, max band / mass, elements]; far: the
# clouds with targets far from the sources, whose bands are the absolute terms (denormal results, the flush), kept apart
MAXIMA = {}
PREC = {"f32": np.float32, "f64": np.float64}
DTYPE = {np.dtype(np.float32): _lib.KMVP_F32, np.dtype(np.float64): _lib.KMVP_F64}
EACH = [(kernel, p) for kernel in cases.KERNELS for p in PREC]
IDS = [f"{k}-{p}" for k, p in EACH]


def check(c, got, model, what, failures):
    """Rows the model calls non-finite are non-finite here and no others; every other element within the band."""
    bad = model.nonfinite
    assert not model.flagged.any()
    msg = None
    if got.shape != model.value.shape:
        msg = f"shape {got.shape}"
    elif np.isfinite(got[bad]).any():
        msg = f"finite where the model's row is not: rows {np.nonzero(bad & np.isfinite(got).any(axis=1))[0][:8]}"
    elif not np.isfinite(got[~bad]).all():
        msg = f"non-finite rows {np.nonzero(~np.isfinite(got).all(axis=1) & ~bad)[0][:8]}"
    elif (~bad).any():
        err, band, mass = np.abs(got[~bad] - model.value[~bad]), model.band[~bad], model.mass[~bad]
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(band > 0, err / band, np.where(err > 0, np.inf, 0.0))
            far = str(c["name"][0]).startswith("far")
            r = MAXIMA.setdefault((cases.NAME[c["path"]], c["kernel"], c["precision"].name, far), [0.0, 0.0, 0.0, 0])
            r[0] = max(r[0], float(ratio.max()))
            r[1] = max(r[1], float(np.where(mass > 0, err / mass, 0.0).max()))
            r[2] = max(r[2], float(np.where(mass > 0, band / mass, 0.0).max()))
            r[3] += ratio.size
        if (err > band).any():
            i, e = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
            msg = (f"err/band {ratio.max():.3g} at row {np.nonzero(~bad)[0][i]} column {e}: err {err[i, e]:.3g} band {band[i, e]:.3g} "
                   f"mass {mass[i, e]:.3g}; {int((err > band).sum())} elements")
    if msg is not None:
        failures.append((what, msg))


class Product:
    """One context on a case's clouds (or a slice of its sources) in the case's precision, the difference form forced."""

    def __init__(self, c, lo=None, hi=None, M_total=None):
        self.c, self.ctx = c, _lib.Context(0)
        self.ctx.set_option("fast_sqdists", 0)
        self.lo, self.hi = lo, hi
        self.set_points(c, M_total)

    def set_points(self, c, M_total=None):
        self.c = c
        dt = c["precision"]
        self.y = np.ascontiguousarray(c["y"][self.lo:self.hi], dtype=dt)
        x = c["x"]
        if x is None and self.lo is not None:
            x = c["y"]
        self.N = len(self.y) if x is None else len(x)
        self.ctx.set_points(self.y, None if x is None else np.ascontiguousarray(x, dtype=dt), DTYPE[dt], self.lo or 0, M_total)

    def run(self, cfg, options=()):
        sig, E, T, feed, chunk, segments = cfg
        c = self.c
        for k, v in (("targets_per_lane", T), ("feed", feed if T else -1), ("chunk", chunk), ("segments", segments)) + tuple(options):
            self.ctx.set_option(k, v)
        b = cases.signal_of(c, sig, E)
        self.ctx.set_signal(None if b is None else np.ascontiguousarray(b[self.lo:self.hi]))
        self.ctx.run(c["kernel"], sig == "norm")
        name, note = self.ctx.last_kernel_name, self.ctx.last_dispatch_note
        assert name == cases.NAME[c["path"]], (c["name"], cfg, name, note)
        if T:   # run_product_t replaces a pair that is not instantiated without an error: the note names the pair that ran
            assert f"targets_per_lane = {T}, feed = {feed}" in note, (c["name"], cfg, note)
        return self.ctx.get_result(self.N, 1 if b is None else b.shape[1])

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.close()


def model_of(c, cfg, cache):
    """The model of one configuration; configurations whose longest chain is the same share it."""
    sig, E, T, feed, chunk, _ = cfg
    feed = feed if T else 1                                     # (run_product_blocked takes the default pair (1, 1))
    key = (sig, E, lm.chain_length(c["path"], c["precision"], len(c["y"]), chunk, feed))
    if key not in cache:
        cache[key] = cases.model(c, sig, E, feed=feed, chunk=chunk)
    return cache[key]


def run_cases(case_list, failures, reached=None):
    for c in case_list:
        cache = {}
        with Product(c) as p:
            for cfg in cases.configs(c):
                model = model_of(c, cfg, cache)
                if "bad_rows" in c["kw"]:
                    assert list(np.nonzero(model.nonfinite)[0]) == c["kw"]["bad_rows"], (c["name"], cfg)
                check(c, p.run(cfg), model, (c["name"], cfg), failures)
                if reached is not None:
                    reached.add((c["y"].shape[1],) + cfg[:4])


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for (kname, fn, prec, far), (eb, em, bm, n) in sorted(MAXIMA.items()):
        print(f"\nlowd model {kname:16s} {fn:22s} {prec} {'far ' if far else 'near'}: max |err|/band {eb:.3g}  max |err|/mass {em:.3g}  "
              f"max band/mass {bm:.3g}  ({n} elements, 0 rows flagged)")


def lowd_grid():
    """(D, sig, E, T, feed) of every lowd_kernel instantiation of one kernel function and precision in kmvp_lowd_inst.hip:
    D = 1 ... 8; the product and normalised rows at E = 1 ... 4, density; (T, feed) = (1, 1) and (2, 0), and at D = 3,
    E = 1 all eight pairs."""
    modes = [(s, e) for s in ("product", "norm") for e in (1, 2, 3, 4)] + [("density", 1)]
    return {(D, s, e, T, f) for D in range(1, 9) for s, e in modes
            for T, f in (cases.HEADLINE_TUNINGS if D == 3 and e == 1 else cases.TUNINGS)}


@pytest.mark.parametrize("kernel,prec", EACH, ids=IDS)
def test_every_lowd_kernel_instantiation(kernel, prec):
    """N = 67 x M = 101 at chunk = 8 and the default; the reached set equals the grid."""
    reached, failures = set(), []
    run_cases(cases.grid_cases(kernel, PREC[prec]), failures, reached)
    assert not failures, (len(failures), failures[:8])
    assert reached == lowd_grid(), sorted(lowd_grid() ^ reached)[:20]


def mid_grid(precision):
    """(DCH, sig, EBW) of every lowd_mid_kernel instantiation of one kernel function and precision: DCH = 2 ... 16 (D <= 8
    never reaches the kernel: DCH = 1 is not built), three signal modes, column blocks of 8, and of 32 for float32 rows of
    up to 64 coordinates with a signal."""
    f32 = np.dtype(precision) == np.float32
    return {(dch, sig, ebw) for dch in range(2, 17) for sig in cases.SIGS
            for ebw in ((8, 32) if f32 and dch <= 8 and sig != "density" else (8,))}


@pytest.mark.parametrize("kernel,prec", EACH, ids=IDS)
def test_every_lowd_mid_kernel_instantiation(kernel, prec):
    """Every DCH at D = 8 DCH and at one ragged D; one and two passes of each column block."""
    reached, failures, passes = set(), [], set()
    run_cases(cases.mid_cases(kernel, PREC[prec]), failures, reached)
    assert not failures, (len(failures), failures[:8])
    got = set()
    for D, sig, E, _, _ in reached:
        ebw = cases.mid_colblock(PREC[prec], D, E)
        got.add(((D + 7) // 8, sig, ebw))
        passes.add((ebw, -(-E // ebw)))
    assert got == mid_grid(PREC[prec]), sorted(mid_grid(PREC[prec]) ^ got)[:20]
    assert passes >= ({(8, 1), (8, 2), (32, 1), (32, 2)} if prec == "f32" else {(8, 1), (8, 2)}), passes


@pytest.mark.parametrize("kernel,prec", EACH, ids=IDS)
def test_every_lowd_big_kernel_instantiation(kernel, prec):
    """Three signal modes at D = 129, 160 and 161, one and two column blocks."""
    reached, failures = set(), []
    run_cases(cases.big_cases(kernel, PREC[prec]), failures, reached)
    assert not failures, (len(failures), failures[:8])
    assert {(D, sig) for D, sig, _, _, _ in reached} == {(D, sig) for D in cases.BIG_DIMS for sig in cases.SIGS}


@pytest.mark.parametrize("kernel,prec", EACH, ids=IDS)
def test_column_blocks_of_four(kernel, prec):
    """run_product_blocked: E = 5, 6 and 9 at D = 3, normalised (the denominator from the first block) and not."""
    failures = []
    run_cases(cases.block_cases(kernel, PREC[prec]), failures)
    assert not failures, (len(failures), failures[:8])


@pytest.mark.parametrize("kernel,prec", EACH, ids=IDS)
def test_edges(kernel, prec):
    """Sizes around every batch, tile and fold; 1 / 2 / 3 / 17 segments; targets far from the cloud (denormal sums, exact
    zeros, the flush, the clamps); clouds at +100; a NaN target, sources at +-inf, a coincident 1/r pair; 1/r with the
    zero column wrapping inside a tile and across tiles -- on all three kernels."""
    failures = []
    run_cases(cases.groups(kernel, PREC[prec])["edges"], failures)
    assert not failures, (len(failures), failures[:8])


@pytest.mark.parametrize("prec", list(PREC))
def test_zero_rule_on_three_source_slices(prec):
    """1/r, N = 450 > M_total + 1, on the slices (0, 67), (67, 131), (131, 200) with j_offset / M_total: each slice inside
    its own model, and the partial results add up to the whole's model, on all three kernels."""
    failures = []
    for path in ("lowd", "mid", "big"):
        c = list(cases.zero_rule_cases(PREC[prec], path))[0]
        M = len(c["y"])
        cfgs = [cfg for cfg in cases.configs(c) if cfg[0] != "norm"]   # (a slice normalises by its own denominator: not a sum)
        total = {cfg: 0.0 for cfg in cfgs}
        for lo, hi in cases.SHARDS:
            part = dict(c, y=c["y"][lo:hi], b=c["b"][lo:hi], kw=dict(j_offset=lo, M_total=M))
            cache = {}
            with Product(c, lo, hi, M_total=M) as p:
                for cfg in cfgs:
                    got = p.run(cfg, [("partial_shard", 1)])
                    check(part, got, model_of(part, cfg, cache), (c["name"], cfg, (lo, hi)), failures)
                    total[cfg] = total[cfg] + got
        cache = {}
        for cfg in cfgs:
            check(c, total[cfg], model_of(c, cfg, cache), (c["name"], cfg, "three slices"), failures)
    assert not failures, (len(failures), failures[:8])


@pytest.mark.parametrize("prec", list(PREC))
def test_second_product_on_one_context(prec):
    """On one context: a product, then another signal with normalised rows at another chunk, density, another kernel
    function, the first again, then new points -- the packed records (points_stale, signal_stale) and the padded rows of
    lowd_mid_kernel / lowd_big_kernel (gen_points_ver, gen_kernel) are rebuilt exactly when they must be."""
    failures = []
    dt = PREC[prec]
    for gen in (cases.grid_cases, cases.mid_cases, cases.big_cases):
        c = list(gen("gaussian", dt))[2]
        rs = np.random.RandomState(3)
        c2 = dict(c, b=cases.signal(rs, *c["b"].shape, dt))
        c3 = dict(c, kernel="matern-5/2")
        c4 = dict(c, y=cases.points(rs, *c["y"].shape, dt), x=None if c["x"] is None else cases.points(rs, *c["x"].shape, dt))
        T, feed = (2, 0) if c["path"] == "lowd" else (0, 0)
        with Product(c) as p:
            for cc, cfg in ((c, ("product", 2, T, feed, 512, 0)), (c2, ("norm", 1, T, feed, 8, 0)), (c, ("density", 1, T, feed, 8, 0)),
                            (c3, ("product", 2, T, feed, 8, 0)), (c, ("product", 2, T, feed, 512, 0)), (c2, ("product", 1, T, feed, 512, 2)),
                            (c4, ("product", 2, T, feed, 512, 0)), (c4, ("norm", 1, T, feed, 512, 0))):
                if cc is c4 and p.c is not c4:
                    p.set_points(c4)
                p.c = cc
                check(cc, p.run(cfg), model_of(cc, cfg, {}), (c["name"], cc["kernel"], cfg, "reuse"), failures)
    assert not failures, (len(failures), failures[:8])
