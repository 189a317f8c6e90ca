"""The float32 single-column matrix-core products (fast_kernel, cfast_kernel) held element by element to a float64 model
of their arithmetic (oracle/kmvp_f32_model.py): |got - model| <= band on every unflagged element, the band derived term
by term in the model's docstring, nothing fitted to kernel output; rows the model calls non-finite are non-finite here and
no others.  MAXIMA collects err / band, err / mass and the flagged share per (device kernel, kernel function) for the
record.

The clouds come from tests/f32_model_cases.py, where tests/test_f32_model.py holds the model on them to the flag cap (at
most 5 % of a cloud's rows flagged) and shows that an emulation of fast_kernel with one defect leaves the band on them."""
import numpy as np
import pytest

import f32_model_cases as cases
from kernel_matrix_benchmarks_amd import _lib

pytestmark = pytest.mark.gpu

MAXIMA = {}  # (device kernel, kernel function) -> [max err / band, max err / mass, flagged rows, rows]
FORCE = {"fast": ("fast_sqdists", 1), "cfast": ("fast_sqdists", 2)}
NAME = {"fast": "fast_kernel", "cfast": "cfast_kernel"}


def fast_grid():
    """(function, D, SIG, TT) of every instantiation in kmvp_fast_inst.hip: three kernel functions, D = 1 ... FAST_MAX_D,
    three signal modes, four target tiles per wave up to FAST_MAX_D_FOUR_TILES, two up to FAST_MAX_D_TWO_TILES, one
    beyond."""
    return {(kernel, D, sig, tt) for kernel in cases.KERNELS for D in range(1, cases.FAST_MAX_D + 1) for sig in cases.SIGS
            for tt in ((1, 2, 4) if D <= cases.FAST_MAX_D_FOUR_TILES else ((1, 2) if D <= cases.FAST_MAX_D_TWO_TILES else (1,)))}


def cfast_grid():
    """kmvp_cfast_inst.hip: three kernel functions x three signal modes x TT 1, 2, 4 (the kernel is the same for every
    D <= 4; D = 1 and 4 are both run)."""
    return {(kernel, D, sig, tt) for kernel in cases.KERNELS for D in (1, 4) for sig in cases.SIGS for tt in (1, 2, 4)}


def check(c, got, model, what, failures=None):
    """Rows the model calls non-finite are non-finite here too; every other unflagged element within the band; at most
    5 % of the rows flagged."""
    msg = None
    bad = model.nonfinite
    ok = ~model.flagged & ~bad
    r = MAXIMA.setdefault((NAME[c["path"]], c["kernel"]), [0.0, 0.0, 0, 0])
    r[2] += int((model.flagged & ~bad).sum())
    r[3] += len(bad)
    if (model.flagged & ~bad).sum() > 0.05 * len(bad):
        msg = (what, f"{int((model.flagged & ~bad).sum())} of {len(bad)} rows flagged")
    elif got.shape != model.value.shape:
        msg = (what, f"shape {got.shape}")
    elif np.isfinite(got[bad]).any():
        msg = (what, "finite where the model's row is not")
    elif not np.isfinite(got[~bad]).all():
        msg = (what, f"non-finite rows {np.nonzero(~np.isfinite(got).all(axis=1) & ~bad)[0][:8]}")
    elif ok.any():
        err = np.abs(got[ok] - model.value[ok])
        band = model.band[ok]
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(band > 0, err / band, np.where(err > 0, np.inf, 0.0))
            r[0] = max(r[0], float(ratio.max()))
            r[1] = max(r[1], float(np.where(model.mass[ok] > 0, err / model.mass[ok], 0.0).max()))
        if (err > band).any():
            i = int(np.argmax(ratio[:, 0]))
            msg = (what, f"err/band {ratio.max():.3g} at row {np.nonzero(ok)[0][i]}: err {err[i, 0]:.3g} band {band[i, 0]:.3g} "
                         f"mass {model.mass[ok][i, 0]:.3g}; {int((err > band).sum())} elements")
    if msg is not None:
        if failures is None:
            raise AssertionError(msg)
        failures.append(msg)


class Product:
    """One float32 context on a case's clouds (or a slice of its sources): products in any signal mode, any options."""

    def __init__(self, c, lo=None, hi=None, x=None, M_total=None):
        self.c, self.ctx = c, _lib.Context(0)
        self.y = np.ascontiguousarray(c["y"][lo:hi], dtype=np.float32)
        self.b = np.ascontiguousarray(c["b"][lo:hi], dtype=np.float32)
        x = c["x"] if x is None else x
        self.N = len(self.y) if x is None else len(x)
        self.ctx.set_option(*FORCE[c["path"]])
        self.ctx.set_points(self.y, None if x is None else np.ascontiguousarray(x, dtype=np.float32), _lib.KMVP_F32,
                            lo or 0, M_total)

    def run(self, sig, options=(), b=None):
        for k, v in options:
            self.ctx.set_option(k, v)
        self.ctx.set_signal(None if sig == "density" else (self.b if b is None else b))
        self.ctx.run(self.c["kernel"], sig == "norm")
        assert self.ctx.last_kernel_name == NAME[self.c["path"]], (self.c["name"], sig, options, self.ctx.last_kernel_name,
                                                                   self.ctx.last_dispatch_note)
        return self.ctx.get_result(self.N, 1)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.close()


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for (kname, fn), (eb, em, nf, n) in sorted(MAXIMA.items()):
        print(f"\nf32 model {kname:12s} {fn:22s} max |err|/band {eb:.3g}  max |err|/mass {em:.3g}  flagged rows {nf} of {n}")


def test_every_fast_kernel_instantiation_against_the_model():
    """Every (function, D, SIG, TT) of kmvp_fast_inst.hip on N = 67 x M = 101; the reached set equals the grid."""
    reached, failures = set(), []
    for c in cases.fast_grid_cases():
        D = c["y"].shape[1]
        with Product(c) as p:
            for sig in cases.SIGS:
                model = cases.model(c, sig)
                for tt in cases.fast_tile_counts(D):
                    check(c, p.run(sig, [("fast_tiles", tt)]), model, (c["name"], sig, tt), failures)
                    reached.add((c["kernel"], D, sig, tt))
    assert not failures, (len(failures), failures[:8])
    assert reached == fast_grid(), sorted(fast_grid() ^ reached)[:20]


def test_every_cfast_kernel_instantiation_against_the_model():
    """Every (function, SIG, TT) of kmvp_cfast_inst.hip at D = 1 and 4 on N = 130 x M = 301 (three groups, the last
    padded); 1/r on the sources themselves, which the dispatch requires."""
    reached, failures = set(), []
    for c in cases.cfast_grid_cases():
        with Product(c) as p:
            for sig in cases.SIGS:
                model = cases.model(c, sig)
                for tt in (1, 2, 4):
                    check(c, p.run(sig, [("fast_tiles", tt)]), model, (c["name"], sig, tt), failures)
                    reached.add((c["kernel"], c["y"].shape[1], sig, tt))
    assert not failures, (len(failures), failures[:8])
    assert reached == cfast_grid(), sorted(cfast_grid() ^ reached)


def test_fast_kernel_stages_segments_and_folds():
    """cases.stress_cases: 24 stages of four tiles (D = 3) and six of two with a ragged last one (D = 24), forced segment
    counts 1 / 2 / 3 / 17 and chunk = 32 (a fold at every stage), the largest terms last, rows of e^-2 ... e^-80: a band
    per row, where rel_err sees only the heaviest row."""
    failures = []
    for c in cases.stress_cases():
        with Product(c) as p:
            for sig in cases.SIGS:
                model = cases.model(c, sig)
                for segs in cases.STRESS_SEGMENTS:
                    got = p.run(sig, [("segments", segs), ("chunk", cases.STRESS_CHUNK)])
                    check(c, got, model, (c["name"], sig, segs), failures)
    assert not failures, (len(failures), failures[:8])


def test_cfast_kernel_rare_branch():
    """cases.rare_cases: recomputed pairs, groups skipped by the reach gate, a cluster at +100; 1/r with an off-diagonal
    coincident pair: exactly those two rows are non-finite."""
    failures = []
    for c in cases.rare_cases():
        with Product(c) as p:
            for sig in cases.SIGS:
                model = cases.model(c, sig)
                if c["name"][-1]:
                    assert list(np.nonzero(model.nonfinite)[0]) == [17, 200]
                for tt in (1, 2):
                    check(c, p.run(sig, [("fast_tiles", tt)]), model, (c["name"], sig, tt), failures)
    assert not failures, (len(failures), failures[:8])


def test_zero_rule_and_own_pair_rule_whole_and_sliced():
    """cases.zero_rule_cases, each whole and as the sum of three partial_shard source slices with j_offset / M_total
    (same_points_global where the targets are the sources): the sum is inside the band of the whole."""
    failures = []
    for c in cases.zero_rule_cases():
        M = len(c["y"])
        with Product(c) as p:
            for sig in cases.SIGS:
                check(c, p.run(sig), cases.model(c, sig), (c["name"], sig, "whole"), failures)
        same = c["x"] is None
        total = {sig: 0.0 for sig in ("product", "density")}   # (a slice normalises by its own denominator: not a sum)
        for lo, hi in cases.SHARDS:
            with Product(c, lo, hi, x=c["y"] if same else c["x"], M_total=M) as p:
                for sig in total:
                    total[sig] = total[sig] + p.run(sig, [("partial_shard", 1), ("same_points_global", int(same))])
        for sig in total:
            check(c, total[sig], cases.model(c, sig), (c["name"], sig, "three slices"), failures)
    assert not failures, (len(failures), failures[:8])


def test_edges_ragged_and_non_finite():
    """(M, N) of 1 and not multiples of 32; a NaN target coordinate: that row is NaN and every other row inside the band;
    sources at +-inf contribute 0 on cfast_kernel."""
    failures = []
    for c in cases.edge_cases():
        with Product(c) as p:
            for sig in cases.SIGS:
                check(c, p.run(sig), cases.model(c, sig), (c["name"], sig), failures)
    for c in cases.nonfinite_cases():
        with Product(c) as p:
            for sig in cases.SIGS:
                model = cases.model(c, sig)
                assert list(np.nonzero(model.nonfinite)[0]) == [5]
                got = p.run(sig)
                assert np.isnan(got[5]).all(), (c["name"], sig, got[5])
                check(c, got, model, (c["name"], sig), failures)
    assert not failures, (len(failures), failures[:8])


def test_second_product_on_one_context_reuses_the_pack():
    """On one context: a product, then a new signal with normalised rows, then density, then the first signal again --
    the points stay packed (points_stale), the source image is rebuilt when the signal or its mode changes
    (signal_stale)."""
    failures = []
    for c in list(cases.fast_grid_cases())[2::39] + list(cases.cfast_grid_cases())[1::2]:
        rs = np.random.RandomState(3)
        b2 = cases.signal(rs, rs.randint(4, size=len(c["y"])))
        c2 = dict(c, b=b2)
        with Product(c) as p:
            for sig, cc in (("product", c), ("norm", c2), ("density", c), ("product", c), ("product", c2), ("norm", c)):
                check(cc, p.run(sig, b=cc["b"]), cases.model(cc, sig), (c["name"], sig, "reuse"), failures)
    assert not failures, (len(failures), failures[:8])
