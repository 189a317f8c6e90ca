"""The cell-form Gaussian kernels (cell_kernel, cellmm_kernel, cellmm16_kernel, cell64_kernel) held element by element to
the float64 model of their arithmetic (oracle/kmvp_cell_model.py): |got - value| <= band on every element of every run, the
band derived term by term in the model's docstring, nothing fitted to kernel output; the rows the model calls non-finite
are non-finite here and no others.  The model takes the cells as data from kmvp_cell_layout and re-checks its preconditions
on the library's real layout: a violated one fails the test with the cell named.  Every run forces its kernel by option
and asserts the device kernel's name and the dispatch note.  MAXIMA collects err / band, err / mass and band / mass per
(device kernel, cloud class) for the record (pytest -s).

The clouds and runs come from tests/cell_model_cases.py, where tests/test_cell_model.py keeps numpy emulations of the
kernels' steps inside the band on the same clouds and shows that an emulation with one defect leaves it."""
import hashlib

import numpy as np
import pytest

import cell_model_cases as cases
import kmvp_cell_model as cm
from kernel_matrix_benchmarks_amd import _lib

pytestmark = pytest.mark.gpu

MAXIMA = {}   # (device kernel, cloud class) -> [max err / band, max err / mass, max band / mass, elements]
DTYPE = {np.dtype(np.float32): _lib.KMVP_F32, np.dtype(np.float64): _lib.KMVP_F64}
COUNT_CUT_NOTE = "count-cut cells"


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for (kname, cls), (eb, em, bm, n) in sorted(MAXIMA.items()):
        print(f"\ncell model {kname:16s} {cls:8s}: max |err|/band {eb:.3g}  max |err|/mass {em:.3g}  max band/mass {bm:.3g}  ({n} elements)")


def check(c, path, got, model, what, failures):
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
            r = MAXIMA.setdefault((cases.NAME[path], str(c["name"][0])), [0.0, 0.0, 0.0, 0])
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
    """One context on a case's clouds in the case's precision."""

    def __init__(self, c):
        self.ctx = _lib.Context(0)
        self.models = {}
        self.set_points(c)

    def set_points(self, c):
        self.c = c
        self.N = len(c["y"]) if c["x"] is None else len(c["x"])
        self.ctx.set_points(c["y"], c["x"], DTYPE[c["precision"]])
        self.models.clear()

    def run(self, run, note_starts=None):
        """One product: the result, the layout it ran on and the model of the same (shared by the runs of one layout)."""
        path, sig, E, options = run
        c = self.c
        for k, v in cases.DEFAULTS + cases.OPTIONS[path] + tuple(options):
            self.ctx.set_option(k, v)
        b = cases.signal_of(c, sig, E)
        self.ctx.set_signal(None if b is None else np.ascontiguousarray(b))
        self.ctx.run("gaussian", sig == "norm")
        name, note = self.ctx.last_kernel_name, self.ctx.last_dispatch_note
        assert name == cases.NAME[path], (c["name"], run, name, note)
        balanced = dict(options).get("cell_balance", -1) == 1
        if note_starts is not None:
            assert note.startswith(note_starts), (c["name"], run, note)
        else:
            assert note == "" or (balanced and note.startswith(COUNT_CUT_NOTE)), (c["name"], run, note)
        got = self.ctx.get_result(self.N, 1 if b is None else b.shape[1])
        lay = self.ctx.cell_layout()
        tt = dict(options).get("fast_tiles", 0)
        assert lay["image"] == {"cell": 0, "cellmm": 1, "cellmm16": 1, "cell64": 2}[path], (c["name"], run, lay["image"])
        assert lay["tile_points"] == (cm.CELL64_TILE if path == "cell64" else cm.CELL_TILE)
        assert tt == 0 or path == "cell64" or lay["tiles_per_wavefront"] == tt, (c["name"], run, lay["tiles_per_wavefront"])
        assert lay["count_cut"] == note.startswith(COUNT_CUT_NOTE), (c["name"], run, note)
        h = hashlib.sha1()
        for k in ("source_cell", "target_cell", "source_centres", "target_centres"):
            h.update(np.ascontiguousarray(lay[k]).tobytes())
        chunk = dict(options).get("chunk", 512)
        key = (h.hexdigest(), lay["sigma_b"], cm.C_W[path], path == "cell", sig, E, chunk if path == "cell" else 0)
        if key not in self.models:
            self.models[key] = cases.model(c, path, sig, E, lay, chunk=chunk)    # raises on a violated precondition, the cell named
        return got, lay, self.models[key]

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.close()


def run_cases(case_list, failures, seen=None):
    for c in case_list:
        with Product(c) as p:
            for run in c["runs"]:
                got, lay, model = p.run(run)
                check(c, run[0], got, model, (c["name"], run), failures)
                if seen is not None:
                    seen.append((c, run, lay))


@pytest.mark.parametrize("D", (1, 2, 3))
def test_every_instantiation_on_the_smallest_cells(D):
    """2^D cells of 1, 31, 32, 33, 8 x 32, 8 x 32 + 1, 12 x 32 + 5 and no points; TT = 1, 2, 4, 8; plain, density and
    normalised; E = 1, 2, 5 on the cellmm kernels; targets = sources and another cloud."""
    failures, seen = [], []
    run_cases([c for c in cases.grid_cases() if c["name"][1] == D], failures, seen)
    assert not failures, (len(failures), failures[:8])
    reached = {(run[0], run[1], lay["tiles_per_wavefront"]) for _, run, lay in seen}
    assert reached >= {(p, s, tt) for p in ("cell", "cellmm", "cellmm16") for s in cases.SIGS for tt in (1, 2, 4, 8)}
    assert all(len(lay["source_centres"]) == (2 ** D if D < 3 else 7) for _, _, lay in seen)      # D = 3: one cell is empty


PLANS = [c["name"] for c in cases.plan_cases()]
RANGES = [c["name"] for c in cases.range_cases()]
SIGNALS = [c["name"] for c in cases.signal_cases()]
ids = lambda names: ["-".join(map(str, n[1:])) for n in names]


@pytest.mark.parametrize("name", PLANS, ids=ids(PLANS))
def test_plans(name):
    """1 / 2 / 3 / 17 segments; the REST list present and absent; fused against two launches and the shared build against
    every wavefront's own, bit for bit; count-cut cells on two column clouds."""
    failures, seen, results = [], [], {}
    c = cases.by_name(name)
    with Product(c) as p:
        for run in c["runs"]:
            got, lay, model = p.run(run)
            check(c, run[0], got, model, (c["name"], run), failures)
            results[run] = got
            seen.append(lay)
    assert not failures, (len(failures), failures[:8])
    for lay in seen:
        if name[1] == "rest":
            assert lay["rest_tiles"] > 0 and lay["main_tiles"] > 0
        if name[1] == "no-rest":
            assert lay["rest_tiles"] == 0
        if name[1] == "count-cut":
            assert lay["count_cut"] and lay["tiles_per_wavefront"] == 8
            columns, cells = np.unique(lay["source_centres"][:, :2], axis=0, return_counts=True)
            assert len(columns) == 4 and cells.min() >= 3, cells                  # every column cut at least twice
    same = [r for r in c["runs"] if r[0] == "cellmm16" and r[1] == "product" and name[1] in ("rest", "no-rest")]
    assert all(np.array_equal(results[same[0]], results[r]) for r in same[1:])     # one plan, four ways to run it: the same bits


@pytest.mark.parametrize("name", RANGES, ids=ids(RANGES))
def test_range(name):
    """The longest line the radius rule admits, rows that are far as a whole, cell_kernel outside the radius rule down to
    e^-100 (the flush of U), the worst corners and one corner with one-signed b, clouds at +100 and +1000."""
    failures = []
    c = cases.by_name(name)
    with Product(c) as p:
        for run in c["runs"]:
            outside = name[1] == "flush"
            got, lay, model = p.run(run, "cell_kernel instead of cellmm_kernel" if outside else None)
            check(c, run[0], got, model, (c["name"], run), failures)
            if outside:       # the last rows are past the flush: the model's band covers them whole, and they are exact zeros
                lost = model.value[:, 0] < 2.0 ** -140
                assert lost.any() and (model.band[lost] >= model.value[lost]).all() and (got[lost] == 0).all()
            if name[1] == "far-rows":
                assert model.mass.max() < np.exp(-9.0)        # every pair below e^-16
    assert not failures, (len(failures), failures[:8])


@pytest.mark.parametrize("name", SIGNALS, ids=ids(SIGNALS))
def test_signals(name):
    """|b| over 2^+-20 with the small sources next to their own targets; one entry of 1e6; an all-zero column among three;
    3000 copies of one point with b of alternating sign."""
    failures = []
    run_cases([cases.by_name(name)], failures)
    assert not failures, (len(failures), failures[:8])


def test_non_finite_inputs():
    """A NaN target: its row is NaN, every other row in band.  A NaN entry of b: every row is NaN.  An infinite source
    coordinate: the cell form refuses and the note says why."""
    failures = []
    base = [c for c in cases.grid_cases() if c["name"] == ("grid", 3, "other")][0]
    runs = [(p, "product", 1, (("fast_tiles", 2),)) for p in ("cell", "cellmm", "cellmm16")]
    x = base["x"].copy()
    x[5, 1] = np.nan
    c = dict(base, name=("nan", "target"), x=x, runs=runs)
    with Product(c) as p:
        for run in runs:
            got, lay, model = p.run(run)
            assert list(np.nonzero(model.nonfinite)[0]) == [5]
            check(c, run[0], got, model, (c["name"], run), failures)
    b = base["b"].copy()
    b[7, 0] = np.nan
    c = dict(base, name=("nan", "signal"), b=b, runs=runs)
    with Product(c) as p:
        for run in runs:
            got, lay, model = p.run(run)
            assert model.nonfinite.all()
            check(c, run[0], got, model, (c["name"], run), failures)
    y = base["y"].copy()
    y[3, 0] = np.inf
    with Product(dict(base, y=y)) as p:
        for k, v in cases.DEFAULTS + cases.OPTIONS["cellmm16"]:
            p.ctx.set_option(k, v)
        p.ctx.set_signal(np.ascontiguousarray(base["b"][:, :1]))
        p.ctx.run("gaussian", False)
        assert "cell" not in p.ctx.last_kernel_name, p.ctx.last_kernel_name
        assert p.ctx.last_dispatch_note.startswith("cell form not taken"), p.ctx.last_dispatch_note
        with pytest.raises(_lib.KmvpError):
            p.ctx.cell_layout()
    assert not failures, (len(failures), failures[:8])


def test_second_product_on_one_context():
    """On one context: a product, then another signal, other tiles per wavefront, the other MFMA shape, count-cut cells, new
    points and cell_kernel -- images, tile lists and sigma_b are rebuilt exactly when they must be."""
    failures = []
    c1, c2 = cases.state_cases()                            # the column cloud, then the 2^3-cell cloud
    rs = np.random.RandomState(5)
    c1b = dict(c1, b=np.ascontiguousarray(cases.signal(rs, len(c1["y"]), 1) * 1.0e3, dtype=np.float32))
    steps = ((c1, ("cellmm16", "product", 1, (("fast_tiles", 8),))), (c1b, ("cellmm16", "product", 1, (("fast_tiles", 8),))),
             (c1b, ("cellmm", "norm", 1, (("fast_tiles", 4),))), (c1, ("cellmm16", "product", 1, (("fast_tiles", 8), ("cell_balance", 1)))),
             (c1b, ("cell", "product", 1, (("fast_tiles", 8), ("cell_balance", 1)))), (c1, ("cellmm16", "density", 1, (("fast_tiles", 8),))),
             (c2, ("cellmm16", "product", 1, (("fast_tiles", 8),))), (c2, ("cell", "norm", 1, (("fast_tiles", 2),))),
             (c2, ("cellmm", "product", 1, (("fast_tiles", 2),))))
    with Product(c1) as p:
        for cc, run in steps:
            if cc["y"] is not p.c["y"]:
                p.set_points(cc)
            p.c = cc
            got, lay, model = p.run(run)
            check(cc, run[0], got, model, (cc["name"], run, "reuse"), failures)
    assert not failures, (len(failures), failures[:8])


def test_cell64_kernel():
    """2^3 cells at cell64_kernel's own side with 1, 127, 128, 129 points among them; plain, density and normalised; one
    and three segments; another target cloud; rows that are far as a whole; a second product on one context."""
    failures = []
    cs = list(cases.cell64_cases())
    run_cases(cs, failures)
    with Product(cs[0]) as p:
        for cc, run in ((cs[0], cs[0]["runs"][0]), (cs[0], cs[0]["runs"][4]), (cs[2], cs[2]["runs"][0]), (cs[2], cs[2]["runs"][1])):
            if cc["y"] is not p.c["y"]:
                p.set_points(cc)
            got, lay, model = p.run(run)
            check(cc, run[0], got, model, (cc["name"], run, "reuse"), failures)
    assert not failures, (len(failures), failures[:8])
