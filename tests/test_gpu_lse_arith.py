"""lowd_lse_kernel (kmvp_<kernel>_logsumexp), lowd_lse_grad_kernel (kmvp_<kernel>_logsumexp_grad) and
lowd_batch_lse_kernel (through kmvp_<kernel>_sinkhorn_batched) held element by element to the float64 model of their
arithmetic (oracle/kmvp_lse_model.py): |got - value| <= band on EVERY element -- absolute in L, per component in G, not
relative to max(1, |L|) or to the row's largest component --, the band derived term by term in the model's docstring,
nothing fitted to kernel output; non-finite exactly where the model says (-inf / NaN without a live term, a NaN target's
row, the column of a NaN or +inf log-weight), and nowhere else; every run asserts the device kernel's name and an empty
dispatch note.  MAXIMA collects err / band and band / max(1, |value|) per (device kernel, kernel function, precision) for
the record (pytest -s).

The clouds and configurations come from tests/lse_model_cases.py, where tests/test_lse_model.py keeps clean emulations of
the kernels' steps inside the band on the same clouds and shows that an emulation with one defect leaves it."""
import os
import re

import numpy as np
import pytest

import kmvp_lowd_model as lm
import kmvp_lse_model as sm
import lse_model_cases as lc
from kernel_matrix_benchmarks_amd import _lib

pytestmark = pytest.mark.gpu

# (device kernel, kernel function, precision) -> [max err / band, max band / max(1, |value|), elements]
MAXIMA = {}
PREC = {"f32": np.float32, "f64": np.float64}
DTYPE = {np.dtype(np.float32): _lib.KMVP_F32, np.dtype(np.float64): _lib.KMVP_F64}
EACH = [(kernel, p) for kernel in lc.KERNELS for p in PREC]
IDS = [f"{k}-{p}" for k, p in EACH]
CSRC = os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "csrc")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lse_parent.npz")
UNIT = {"lse": "lse", "grad": "lse_grad"}


def record(name, c, got, model):
    must = ~model.poisoned & np.isfinite(model.value) & np.isfinite(got)
    if must.any():
        with np.errstate(divide="ignore", invalid="ignore"):
            err, band = np.abs(got - model.value)[must], model.band[must]
            far = " at 1e20" if c["name"][2] == "targets-at-1e20" else ""      # (its own line: bands of another scale)
            r = MAXIMA.setdefault((name + far, c["kernel"], c["precision"].name), [0.0, 0.0, 0])
            r[0] = max(r[0], float(np.where(band > 0, err / band, np.where(err > 0, np.inf, 0.0)).max()))
            r[1] = max(r[1], float((band / np.maximum(1.0, np.abs(model.value[must]))).max()))
            r[2] += int(must.sum())


def check(c, cfg, got, model, what, failures):
    record(lc.NAME[cfg[0]], c, got, model)
    _, msg = lc.compare(got, model, lc.loose(c, cfg[0]))
    if msg is not None:
        failures.append((what, msg))


class Lse:
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
        b = lc.signal_of(c, sig, E)
        self.ctx.set_signal(None if b is None else np.ascontiguousarray(b[self.lo:self.hi]))
        (self.ctx.run_lse_grad if which == "grad" else self.ctx.run_lse)(c["kernel"])
        if len(self.y) > 0 and self.N > 0:                       # (no source: nothing is launched)
            name, note = self.ctx.last_kernel_name, self.ctx.last_dispatch_note
            assert name == lc.NAME[which] and note == "", (c["name"], cfg, name, note)
        NC, D = (1 if b is None else b.shape[1]), self.y.shape[1]
        if which == "grad":
            return self.ctx.get_result(self.N, NC * D).reshape(self.N, NC, D)      # column e D + d
        return self.ctx.get_result(self.N, NC)

    def product(self):
        self.ctx.run(self.c["kernel"], False)
        assert self.ctx.last_kernel_name == "lowd_kernel"

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.close()


def model_of(c, cfg, cache):
    """The model of one configuration; configurations whose longest chain is the same share it."""
    key = cfg[:3] + (lm.chain_length("lowd", c["precision"], max(len(c["y"]), 1), cfg[3], 1),)
    if key not in cache:
        cache[key] = lc.model(c, cfg)
    return cache[key]


def run_cases(case_list, failures, reached=None):
    for c in case_list:
        cache = {}
        with Lse(c) as g:
            for cfg in lc.configs(c):
                model = model_of(c, cfg, cache)
                assert list(np.nonzero(model.nonfinite)[0]) == c["kw"].get("bad_rows", []), (c["name"], cfg)
                check(c, cfg, g.run(cfg), model, (c["name"], cfg), failures)
                if reached is not None:
                    reached.add((cfg[0], c["y"].shape[1], cfg[1], cfg[2]))


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for (kname, fn, prec), (eb, bv, n) in sorted(MAXIMA.items()):
        print(f"\nlse model {kname:30s} {fn:22s} {prec}: max |err|/band {eb:.3g}  max band/max(1,|value|) {bv:.3g}  ({n} elements)")


def inst_grid(which):
    """(which, D, sig, E) of every instantiation of one kernel function and precision, read from the unit that makes them:
    one `case D:` per launch_e<D>, one `case E:` per launch_one<D, E, SIG_PRODUCT>, and the density variant."""
    text = open(os.path.join(CSRC, f"kmvp_lowd_{UNIT[which]}_inst.hip")).read()
    assert f"lowd_{UNIT[which]}_kernel<KERNEL, D, E, SIG, real>" in text
    dims = sorted(int(d) for d, d2 in re.findall(r"case (\d+): return launch_e<(\d+)>", text) if d == d2)
    cols = sorted(int(e) for e, e2 in re.findall(r"case (\d+): return launch_one<D, (\d+), SIG_PRODUCT>", text) if e == e2)
    assert "launch_one<D, 1, SIG_DENSITY>" in text and dims and cols
    return {(which, D, sig, E) for D in dims for sig, E in [("product", e) for e in cols] + [("density", 1)]}


def test_the_grids_are_eight_dimensions_by_four_columns_and_density():
    for which in lc.WHICH:
        assert inst_grid(which) == {(which, D, s, e) for D in range(1, 9) for s, e in lc.MODES}


@pytest.mark.parametrize("kernel,prec", EACH, ids=IDS)
def test_every_instantiation(kernel, prec):
    """D = 1 ... 8 x (E = 1 ... 4 and density), N = 67 targets != M = 101 sources and the same points at D = 3, chunk = 8
    and 512, log-weight columns distinct in scale and sign; the reached set equals the grid of the two _inst.hip units."""
    reached, failures = set(), []
    run_cases(lc.grid_cases(kernel, PREC[prec]), failures, reached)
    assert not failures, (len(failures), failures[:8])
    grid = set().union(*(inst_grid(w) for w in lc.WHICH))
    assert reached == grid, sorted(grid ^ reached)[:20]


@pytest.mark.parametrize("kernel,prec", EACH, ids=IDS)
def test_edges_of_every_loop(kernel, prec):
    """N of 1, 63, 64, 65, 257 and M of 1 ... 1030 around every batch of 4, pad of 8, LDS tile and fold, chunk = 8, 256, 512;
    N = 65 x M = 1030 under 1, 2, 3 and 17 segments."""
    failures = []
    run_cases(lc.groups(kernel, PREC[prec])["edges"], failures)
    assert not failures, (len(failures), failures[:8])


@pytest.mark.parametrize("kernel,prec", EACH, ids=IDS)
def test_the_shift_on_its_edges(kernel, prec):
    """D = 3, chunk = 256, 1 and 3 segments: sources nearest-last and nearest-first; a rise in the first batch after a
    fold; the same beyond the clamp of the rescale (300 / 4000 binades, by c); a rise on one lane of a wave; on one column
    of four; inside the gradient's guarded last 8 records; a first segment without a live term."""
    failures = []
    run_cases(lc.groups(kernel, PREC[prec])["shift"], failures)
    assert not failures, (len(failures), failures[:8])


@pytest.mark.parametrize("kernel,prec", EACH, ids=IDS)
def test_range_and_exact_rules(kernel, prec):
    """Logits near -1e4 (float32) / -1e6 (float64) with c spanning +-1e3; some c = -inf, an all -inf column, all -inf; M = 0;
    targets at 1e20 (float32: exactly -inf, NaN for the gradient; float64: in a band of 2e-15 |L| for L -- the weights are
    positive, so L moves by at most the largest logit error -- and, for G, of the sources' spread on an axis plus the
    rounding of x - y, since V / Z is a convex combination of the directions); duplicated points (exp(-r): the own
    pair and an off-diagonal coincident pair add 0 to V)."""
    failures = []
    cs = lc.groups(kernel, PREC[prec])["range"]
    run_cases(cs, failures)
    assert not failures, (len(failures), failures[:8])
    far = [c for c in cs if c["name"][2] == "targets-at-1e20"][0]
    for cfg in (("lse", "density", 1, 512, 0), ("grad", "density", 1, 512, 0)):
        v = lc.model(far, cfg).value
        assert (np.isneginf(v) | np.isnan(v)).all() if prec == "f32" else np.isfinite(v).all()


@pytest.mark.parametrize("kernel,prec", EACH, ids=IDS)
def test_non_finite_inputs(kernel, prec):
    """A NaN target at M = 5, 8 and 101: its row is NaN in every column, every other row in band.  A NaN and a +inf
    log-weight in one column of two: include/kmvp.h's rule -- no entry of that column is finite, for any target, the other
    column in band.  A NaN, +inf or -inf source coordinate at j = 0, in the middle and in the guard zone: L with an
    infinite coordinate is the other sources' sum (include/kmvp.h: pairs at infinite distance contribute exactly 0); G
    (include/kmvp.h: 0 * inf) is NaN in the components of that axis in every row, at all three positions alike; what no
    rule covers (a NaN coordinate in L, the other axes of G) is `loose`: non-finite too, or the other sources' sum in
    band.  What the kernels do there, for the record: a NaN source coordinate leaves nothing finite in L and G in either
    precision; with an infinite one the other axes of G hold the other sources' sum."""
    failures = []
    run_cases(lc.groups(kernel, PREC[prec])["nonfinite"], failures)
    assert not failures, (len(failures), failures[:8])


def merge_gradients(Ls, Gs):
    """include/kmvp.h: G = sum_s exp(L_s - L) G_s with L the logaddexp of the shards' L_s."""
    L = np.logaddexp.reduce(Ls, axis=0)
    return sum(np.exp(Ls_ - L)[:, :, None] * G for Ls_, G in zip(Ls, Gs))


@pytest.mark.parametrize("kernel,prec", EACH, ids=IDS)
def test_three_source_slices(kernel, prec):
    """The slices (0, 67), (67, 131), (131, 200) under partial_shard: each partial result inside its own model, their
    logaddexp (L) and the caller-side merge of include/kmvp.h (G) inside the whole's."""
    failures = []
    c = list(lc.shard_cases(kernel, PREC[prec]))[0]
    M = len(c["y"])
    cfgL, cfgG = ("lse", "product", 2, 512, 0), ("grad", "product", 2, 512, 0)
    Ls, Gs = [], []
    for lo, hi in lc.SHARDS:
        part = dict(c, y=c["y"][lo:hi], b=c["b"][lo:hi], kw=dict(j_offset=lo, M_total=M))
        with Lse(c, lo, hi, M_total=M) as g:
            for cfg, out in ((cfgL, Ls), (cfgG, Gs)):
                got = g.run(cfg, [("partial_shard", 1)])
                check(part, cfg, got, lc.model(part, cfg), (c["name"], cfg, (lo, hi)), failures)
                out.append(got)
    check(c, cfgL, np.logaddexp.reduce(Ls, axis=0), lc.model(c, cfgL), (c["name"], cfgL, "three slices"), failures)
    check(c, cfgG, merge_gradients(Ls, Gs), lc.model(c, cfgG), (c["name"], cfgG, "three slices"), failures)
    assert not failures, (len(failures), failures[:8])


@pytest.mark.parametrize("prec", list(PREC))
def test_state_on_one_context(prec):
    """On one context: a product, L, G, a new signal, L, density, the other kernel function, new points.  Every result is
    in band and bit-equal to the same call on a fresh context: the packed records are rebuilt exactly when they must be,
    and the segments are merged in index order."""
    failures = []
    dt = PREC[prec]
    c = [c for c in lc.grid_cases("gaussian", dt) if c["name"][:1] == ("grid",) and c["name"][2] == 3][0]
    rs = np.random.RandomState(3)
    c2 = dict(c, b=lc.logweights(rs, *c["b"].shape, dt))
    c3 = dict(c2, kernel="absolute-exponential")
    c4 = dict(c3, y=lc.cases.points(rs, *c["y"].shape, dt), x=lc.cases.points(rs, *c["x"].shape, dt))
    L2, G2 = ("lse", "product", 2, 512, 0), ("grad", "product", 2, 512, 0)
    steps = ((c, True, L2), (c, False, G2), (c2, False, L2), (c2, False, G2), (c2, False, ("grad", "density", 1, 512, 0)),
             (c2, False, ("lse", "density", 1, 512, 0)), (c3, False, ("lse", "product", 3, 8, 2)), (c3, True, G2), (c4, False, G2),
             (c4, False, L2))
    with Lse(c) as g:
        for cc, product, cfg in steps:
            if cc is c4 and g.c is not c4:
                g.set_points(c4)
            g.c = cc
            if product:
                g.ctx.set_signal(np.ascontiguousarray(cc["b"][:, :2]))
                g.product()
            got = g.run(cfg)
            check(cc, cfg, got, model_of(cc, cfg, {}), (cc["kernel"], cfg, "reuse"), failures)
            with Lse(cc) as fresh:
                assert np.array_equal(got, fresh.run(cfg), equal_nan=True), (cc["kernel"], cfg, "fresh context")
    assert not failures, (len(failures), failures[:8])


# ---- lowd_batch_lse_kernel through the batched Sinkhorn solve -----------------------------------------------------------
# kmvp_sinkhorn_batched.hip: the first launch is v_1 = T2(u_0), the log-sum-exp over the batch's x of the slot
# (real)(u_0 + log a) at the batch's y as targets, and v = -L; a batch stopped by maxit commits no new u.  So maxit = 1
# returns one application of the kernel.  maxit = 2 returns (u_1, v_2) with u_1 = T1(v_1) and v_2 = T2(u_1): with the
# device's own v_1 (maxit = 1) and u_1 as the models' inputs -- the runs are bitwise reproducible -- both directions are
# isolated.  The entry refuses a batch with points on one side only, so the ragged sizes of tests/test_gpu_batched.py are
# paired without their one-sided combinations; the empty batch is empty on both sides.
BATCH_X = (300, 1, 7, 8, 9, 0, 40)       # the kernel's sources in direction 2 (the solve's x)
BATCH_Y = (1, 63, 64, 65, 130, 0, 5)     # its targets (the solve's y)
NAN_BATCH = 6                            # a NaN coordinate in y point 2 of the last batch


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def batch_model_check(kernel, dt, src, tgt, src_off, tgt_off, slot, got, chunk, what, failures):
    """got = -L per batch, L the log-sum-exp of `slot` over the batch's src at the batch's tgt (feed = 0)."""
    for b in range(len(src_off) - 1):
        s, t = slice(src_off[b], src_off[b + 1]), slice(tgt_off[b], tgt_off[b + 1])
        if t.stop == t.start:
            continue
        c = lc.case(("batched", kernel, b), kernel, dt, src[s], tgt[t], slot[s].reshape(-1, 1), feed=0)
        m = sm.lse(kernel, src[s], tgt[t], slot[s].reshape(-1, 1), precision=dt, chunk=chunk, feed=0)
        record("lowd_batch_lse_kernel", c, -got[t].reshape(-1, 1), m)
        _, msg = lc.compare(-got[t].reshape(-1, 1), m, False)
        if msg is not None:
            failures.append((what, b, msg))


@pytest.mark.parametrize("kernel,prec", EACH, ids=IDS)
def test_one_application_of_the_batched_kernel_in_each_direction(kernel, prec):
    dt = np.dtype(PREC[prec])
    failures = []
    for D in (1, 3, 8):
        rs = np.random.RandomState(lc.cases.seed("lse-batched", kernel, D))
        x = lc.cases.points(rs, sum(BATCH_X), D, dt)
        y = lc.cases.points(rs, sum(BATCH_Y), D, dt) + dt.type(0.25)
        x_off, y_off = offsets(BATCH_X), offsets(BATCH_Y)
        y[y_off[NAN_BATCH] + 2, D - 1] = np.nan
        la, lb = np.log(rs.rand(len(x)) + 0.1), np.log(rs.rand(len(y)) + 0.1)
        u0 = rs.randn(len(x)) * 2.0
        for chunk in (512, 8):
            ctx = _lib.Context(0)
            try:
                ctx.set_option("chunk", chunk)
                ctx.set_points(y, x, DTYPE[dt])
                ctx.set_batches(y_off, x_off)
                runs = []
                for maxit in (1, 2):
                    u, v, iters, err, status = ctx.sinkhorn_batched(kernel, la, lb, 0.0, maxit, u0)
                    assert ctx.last_kernel_name == "lowd_batch_lse_kernel" and ctx.last_dispatch_note == ""
                    runs.append((u, v, iters, status))
            finally:
                ctx.close()
            (u_a, v1, it1, st1), (u1, v2, it2, st2) = runs
            live = [b for b in range(len(BATCH_X)) if BATCH_X[b] > 0]
            assert it1[5] == 0 and st1[5] == 1 and st1[NAN_BATCH] == 2 and np.isnan(v1[y_off[NAN_BATCH] + 2])
            assert all(st1[b] == 3 and it1[b] == 1 for b in live if b != NAN_BATCH), (st1, it1)
            assert all(st2[b] == 3 and it2[b] == 2 for b in live if b != NAN_BATCH), (st2, it2)
            assert np.array_equal(u_a, u0)                            # a batch stopped by maxit commits no new u
            slot = (u0 + la).astype(dt)
            batch_model_check(kernel, dt, x, y, x_off, y_off, slot, v1, chunk, (kernel, prec, D, chunk, "v_1"), failures)
            ok = np.ones(len(BATCH_X), bool)
            ok[NAN_BATCH] = False                                     # stopped at k = 1: no second iteration
            keep = lambda off: np.concatenate([np.arange(off[b], off[b + 1]) for b in range(len(ok)) if ok[b]])
            sub = lambda a, off: a[keep(off)]
            sizes_x, sizes_y = [n for n, o in zip(BATCH_X, ok) if o], [n for n, o in zip(BATCH_Y, ok) if o]
            xo, yo = offsets(sizes_x), offsets(sizes_y)
            # u_1 = T1(v_1): sources y with the slot (real)(v_1 + log b), targets x
            batch_model_check(kernel, dt, sub(y, y_off), sub(x, x_off), yo, xo, sub((v1 + lb).astype(dt), y_off), sub(u1, x_off), chunk,
                              (kernel, prec, D, chunk, "u_1"), failures)
            # v_2 = T2(u_1)
            batch_model_check(kernel, dt, sub(x, x_off), sub(y, y_off), xo, yo, sub((u1 + la).astype(dt), x_off), sub(v2, y_off), chunk,
                              (kernel, prec, D, chunk, "v_2"), failures)
    assert not failures, (len(failures), failures[:8])


def test_finite_inputs_give_the_bits_recorded_before_the_nan_select_and_the_guard_changed():
    """tests/golden/lse_parent.npz holds both kernels' results on lc.golden_cases(), recorded from the library of the commit
    before lse_exp2_neg passed a NaN on in float64 and the gradient's guard went from the squared distance to the
    record's index: M = 37 has three pad records and a guard zone that holds real sources too.  Bit for bit."""
    want = np.load(GOLDEN)
    seen = 0
    for c in lc.golden_cases():
        with Lse(c) as g:
            for which in lc.WHICH:
                for segments in (1, 2):
                    got = g.run((which, "product", 2, 512, segments))
                    assert np.array_equal(got, want[lc.golden_key(c, which) + f"|{segments}"]), (c["kernel"], c["precision"].name, which)
                    seen += 1
    assert seen == len(want.files) == 16
