"""oracle/kmvp_cell_model.py on the CPU: the model with rounding disabled against the float64 oracle; its preconditions
raised with the cell named; on every cloud and run of tests/test_gpu_cell_arith.py (tests/cell_model_cases.py), with the
layout of a Python lattice, no precondition raised, no row flagged and a numpy emulation of the kernel's own steps inside
the band on every element it computes; the same emulation with ONE defect outside it.  Prints band / mass per cloud, the
emulations' err / band and the defects' margins (pytest -s), for the record.

Emulated rows: every target of clouds up to 1200 points, every ROW_STEP-th target of the larger ones (the emulation holds
an (N, 32) array per step); the model's preconditions and bands are formed for every row of every cloud."""
import numpy as np
import pytest

import cell_model_cases as cases
import kmvp_cell_model as cm
import kmvp_oracle

ROW_LIMIT, ROW_STEP = 1200, 23
SHARPNESS = {}
MARGINS = []
OLD_RULE = 1.0e-5     # the rule this model replaces: 1e-5 of the heaviest row
# Defects that cannot clear the band, and why.  no-kahan: a plain fp32 sum of the n_S <= 94 weights of a cell errs by about
# sqrt(n_S) u (at most n_S u / 2 = 47 u), and the band's floor -- K_BAND times v_exp_f32 at TRANS = 4 u on U and on W -- is
# 16 u of the row already: the compensation buys accuracy the band cannot certify while the exponentials are granted 2 ulp.
EXCEPTIONS = ("no-kahan",)


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for name, (lo, hi, top, worst) in sorted(SHARPNESS.items(), key=str):
        print(f"\ncell model {str(name):44s} band / mass {lo:.3g} ... {hi:.3g}   max band / heaviest row {top:.3g}   emulation err / band <= {worst:.3g}")
    for line in MARGINS:
        print("\n" + line)


@pytest.mark.parametrize("sig", cases.SIGS)
@pytest.mark.parametrize("same", (False, True))
def test_model_without_rounding_is_the_float64_product(sig, same):
    rs = np.random.RandomState(3)
    y = rs.rand(70, 3)
    x = None if same else rs.rand(90, 3)
    b = None if sig == "density" else rs.randn(70, 3) + 0.5
    for path in ("cellmm", "cell64"):
        b = b if b is None or path == "cellmm" else b[:, :1]
        got = cm.cell_product(y, x, b, sig == "norm", path=path, rounding=False)
        dt = np.float64 if path == "cell64" else np.float32
        r = lambda a: None if a is None else a.astype(dt).astype(np.float64)
        want = kmvp_oracle.product(kernel="gaussian", source_points=r(y), target_points=r(x), source_signal=r(b), normalize_rows=sig == "norm")
        assert got.value.shape == want.shape and not got.band.any() and not got.flagged.any() and not got.nonfinite.any()
        assert np.abs(got.value - want).max() <= 1e-12 * np.abs(want).max()


def test_preconditions_raise_and_name_the_cell():
    c = cases.groups()["grid"][4]                       # D = 3, targets = sources
    lay = cases.lattice(c, "cellmm")
    lay["sigma_b"] = cases.sigma_of(c, "product", 1, 0, lay)
    assert cases.model(c, "cellmm", "product", 1, lay).band.min() > 0
    for bad, what in ((-1, "source 5 is in no cell"), (-2, "source 5 is in more than one cell")):
        broken = dict(lay, source_cell=lay["source_cell"].copy())
        broken["source_cell"][5] = bad
        with pytest.raises(ValueError, match=what):
            cases.model(c, "cellmm", "product", 1, broken)
    one = dict(lay, source_cell=np.zeros_like(lay["source_cell"]), source_centres=lay["source_centres"][:1])
    with pytest.raises(ValueError, match=r"\|2 d\.e\| reaches .* source cell 0"):
        cases.model(c, "cellmm", "product", 1, one)
    with pytest.raises(ValueError, match="sigma_b is missing"):
        cases.model(c, "cellmm16", "product", 1, dict(lay, sigma_b=0.0))
    wide = cases.case(("wide",), np.array([[0.05, 0, 0], [60.05, 0, 0]]), None, np.ones((2, 1)), [])
    ids, cen = np.array([0, 1], np.int32), np.array([[0.0, 0, 0], [60.0, 0, 0]])     # e = 0.05 against Delta = 60: W = e^6 > 2^8
    lw = dict(source_cell=ids, target_cell=ids, source_centres=cen, target_centres=cen)
    with pytest.raises(ValueError, match=r"W = .* > 2\^8"):
        cases.model(wide, "cellmm", "product", 1, dict(lw, sigma_b=1.0))
    assert cases.model(wide, "cell", "product", 1, lw).band.min() >= 0       # cell_kernel takes any W
    far = cases.case(("far",), np.zeros((4, 3)), np.full((3, 3), 5.9), np.ones((4, 1)), [])
    with pytest.raises(ValueError, match="denominator"):
        cases.model(far, "cell", "norm", 1, cases.lattice(far, "cell"))


def _rows(c):
    n = len(c["y"]) if c["x"] is None else len(c["x"])
    return None if n <= ROW_LIMIT else np.arange(0, n, ROW_STEP)


def _inside(c, run, models=None, defect=None, rows="auto"):
    """max err / band of the emulation of one run against the model of the same, and the model."""
    path, sig, E, opts = run
    opts = dict(opts)
    lay = cases.lattice(c, path)
    sigma = lambda col: cases.sigma_of(c, sig, E, col, lay)
    lay["sigma_b"] = sigma(E if sig == "norm" else E - 1)
    key = (cm.C_W[path], path == "cell", sig, E, opts.get("chunk", 512) if path == "cell" else 0)
    models = {} if models is None else models
    if key not in models:
        models[key] = cases.model(c, path, sig, E, lay, chunk=opts.get("chunk", 512))
    m = models[key]
    rows = _rows(c) if isinstance(rows, str) else rows
    got = cases.emulate(c, path, sig, E, lay, sigma, max(1, opts.get("segments", 1)), opts.get("chunk", 512), defect, rows)
    sel = slice(None) if rows is None else rows
    value, band, bad = m.value[sel], m.band[sel], m.nonfinite[sel]
    assert got.shape == value.shape and not m.flagged.any()
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.abs(got - value)
        ratio = np.where(band > 0, err / band, np.where(err > 0, np.inf, 0.0))[~bad]
    assert np.array_equal(np.isfinite(got).all(axis=1), ~bad), (c["name"], run)
    return (float(ratio.max()) if ratio.size else 0.0), m


@pytest.mark.parametrize("group", ("grid", "plan", "range", "signal", "cell64"))
def test_clean_emulations_stay_inside_the_band_on_the_gpu_tests_clouds(group):
    """Every cloud, every run whose arithmetic differs: no precondition raised, no row flagged, the emulation within the
    band; on the near clouds the band is no looser than the old rule, 1e-5 of the heaviest row."""
    for c in cases.groups()[group]:
        seen, models = set(), {}
        for run in c["runs"]:
            path, sig, E, opts = run
            o = dict(opts)
            key = (path, sig, E, o.get("segments", 1) if path != "cell" else 0, o.get("chunk", 512) if path == "cell" else 0)
            if key in seen:
                continue
            seen.add(key)
            worst, m = _inside(c, run, models)
            assert worst <= 1.0, (c["name"], run, worst)
            ok = ~m.nonfinite[:, None] & (m.mass > 0)              # (an all-zero column has no mass and a band of zero)
            rel = m.band[ok] / m.mass[ok]
            heaviest = np.where(ok, m.mass, 0.0).max(axis=0)
            top = float((np.where(ok, m.band, 0.0).max(axis=0)[heaviest > 0] / heaviest[heaviest > 0]).max())
            r = SHARPNESS.setdefault((c["name"], path, sig, E), [np.inf, 0.0, 0.0, 0.0])
            r[0], r[1], r[2], r[3] = min(r[0], float(rel.min())), max(r[1], float(rel.max())), max(r[2], top), max(r[3], worst)
            if c["near"] and path != "cell64":
                assert top <= OLD_RULE, (c["name"], run, top)


def _pick(group, name):
    return [c for c in cases.groups()[group] if c["name"] == name][0]


def _defect_runs(defect):
    grid = _pick("grid", ("grid", 3, "same"))
    corners = _pick("range", ("range", "corners"))
    copies = _pick("signal", ("signal", "copies"))
    one = _pick("range", ("range", "one-corner"))
    mm16 = ("cellmm16", "product", 1, (("fast_tiles", 8),))
    if defect in ("no-mid", "xz-for-yz"):
        return [(one, mm16), (one, ("cellmm", "product", 1, ()))]
    if defect == "no-kahan":                               # a cell of 94 tiles, b of one sign (alternating signs sum exactly)
        return [(dict(copies, b=np.abs(copies["b"])), mm16)]
    if defect == "vprev-stale":
        return [(grid, mm16), (corners, mm16)]
    if defect == "segment-end-unfolded":
        return [(grid, ("cellmm16", "product", 1, (("segments", 2),))), (grid, ("cellmm", "density", 1, ()))]
    if defect == "sigma-times-2":
        return [(grid, mm16)]
    if defect == "pad-b-one":
        return [(grid, mm16)]
    if defect == "dm-of-v":
        return [(corners, ("cell", "product", 1, ())), (grid, ("cell", "norm", 1, ()))]
    if defect == "cell64-degree-5":
        return [(_pick("cell64", ("cell64", "grid")), ("cell64", "product", 1, ()))]
    if defect == "u-own-centre":
        return [(grid, mm16), (grid, ("cell", "product", 1, ())), (_pick("cell64", ("cell64", "grid")), ("cell64", "density", 1, ()))]
    raise KeyError(defect)


@pytest.mark.parametrize("defect", cases.DEFECTS)
def test_a_defective_kernel_leaves_the_band(defect):
    """The emulation with one defect is outside the band on every cloud listed for it, where the clean emulation is inside
    on every element; records by how much."""
    for c, run in _defect_runs(defect):
        clean, _ = _inside(c, run, rows=None if len(c["y"]) <= 1300 else np.arange(0, len(c["y"]), 7))
        worst, _ = _inside(c, run, defect=defect, rows=None if len(c["y"]) <= 1300 else np.arange(0, len(c["y"]), 7))
        MARGINS.append(f"cell defect {defect:22s} {cases.NAME[run[0]]:16s} {str(c['name']):28s} {run[1]:8s}: err / band {worst:.3g} (clean {clean:.3g})")
        assert clean <= 1.0, (defect, c["name"], clean)
        if defect in EXCEPTIONS:
            assert worst <= 1.0, (defect, c["name"], run, worst, "no longer an exception: take it off the list")
        else:
            assert worst > 1.0, (defect, c["name"], run, worst)


def test_a_pad_source_of_cell_kernel_is_guarded_twice():
    """The issue's seventh defect on cell_kernel -- a pad source with b != 0 -- cannot leave the band: a pad row's constant slot
    is 0 and its offsets are 0, so all sixteen slots of its operand row are zero and its b is multiplied by 0 whatever it is:
    the result is the same bit for bit.  (cellmm's pads have no such guard: pad-b-one above.)"""
    c = _pick("grid", ("grid", 3, "same"))
    lay = cases.lattice(c, "cell")
    assert np.array_equal(cases.emulate(c, "cell", "norm", 1, lay), cases.emulate(c, "cell", "norm", 1, lay, defect="pad-b-one"))
