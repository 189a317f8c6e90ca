"""oracle/kmvp_lowd_grad_model.py on the CPU: the model with rounding disabled against the restatements
(tests/grad_reference.py, tests/dscale_reference.py, tests/matern_reference.py) on every cloud of finite inputs; numpy
emulations of lowd_grad_kernel's and lowd_dscale_kernel's own steps inside the band on every cloud and configuration
tests/test_gpu_lowd_grad_arith.py runs; the same emulations with one defect at a time outside it.  Prints band / mass per
(kernel, function, precision, chunk) and the defects' margins (pytest -s), for the record."""
import numpy as np
import pytest

import dscale_reference
import grad_reference
import kmvp_lowd_grad_model as gm
import lowd_grad_model_cases as gc
import matern_reference

PREC = {"f32": np.float32, "f64": np.float64}
EACH = [(kernel, p) for kernel in gc.KERNELS for p in PREC]
IDS = [f"{k}-{p}" for k, p in EACH]


def restatement(c, cfg):
    """The committed restatement in float64 arithmetic on the inputs as rounded to the case's precision."""
    which, sig, E, _, _ = cfg
    dt = c["precision"]
    r64 = lambda a: None if a is None else np.asarray(a, dtype=dt).astype(np.float64)
    kw = dict(kernel=c["kernel"], source_points=r64(c["y"]), target_points=r64(c["x"]), source_signal=r64(gc.signal_of(c, sig, E)))
    if which == "dscale":
        return dscale_reference.scale_derivative(**kw)
    if c["kernel"] in matern_reference.KERNELS:
        return matern_reference.gradient(**kw)
    return grad_reference.gradient(j_offset=c["kw"].get("j_offset", 0), M_total=c["kw"].get("M_total"), **kw)


@pytest.mark.parametrize("kernel,prec", EACH, ids=IDS)
def test_model_without_rounding_is_the_restatement(kernel, prec):
    """Every cloud of finite inputs, one product and the density per kernel.  The restatements run in float64, whose own
    exp(-s) is off by about s D u: 1e-10 of the element's mass covers s <= 830, D = 8 (7e-13) with room; where the terms
    are denormal each of the restatement's products is off by one denormal step, which the factors that follow it
    multiply: at most |c| P (1 + max |b|) (1 + max |x - y|)^2 steps per source, |c| <= 3 the constant and
    P <= 1 + sqrt(5) max |x - y| the weight's polynomial."""
    seen = 0
    for group in ("grid", "edges", "range"):
        for c in gc.groups(kernel, PREC[prec])[group]:
            for cfg in {(w, s, e, 512, 0) for w, s, e, _, _ in gc.configs(c)}:
                m = gc.model(c, cfg, rounding=False)
                want = restatement(c, cfg)
                assert m.value.shape == want.shape and not m.band.any()
                assert np.array_equal(np.isfinite(want).all(axis=(1, 2)), ~m.nonfinite), (c["name"], cfg)
                assert list(np.nonzero(m.nonfinite)[0]) == c["kw"].get("bad_rows", []), (c["name"], cfg)
                ok = ~m.nonfinite
                far = 1.0 + np.abs(np.asarray(c["y"] if c["x"] is None else c["x"], np.float64)).max() + np.abs(np.asarray(c["y"], np.float64)).max()
                tol = 1e-10 * m.mass[ok] + len(c["y"]) * 2.0 ** -1074 * (1.0 + np.abs(c["b"]).max()) * far ** 2 * 3.0 * (1.0 + 2.2360679775 * far)
                assert (np.abs(m.value[ok] - want[ok]) <= tol).all(), (c["name"], cfg)
                seen += 1
    assert seen > 40


def test_model_of_three_source_slices_adds_up_to_the_whole():
    c = list(gc.zero_rule_cases(np.float64))[0]
    cfg = ("grad", "product", 1, 512, 0)
    whole = gc.model(c, cfg, rounding=False)
    parts = sum(gc.model(dict(c, y=c["y"][lo:hi], b=c["b"][lo:hi], kw=dict(j_offset=lo, M_total=200)), cfg, rounding=False).value
                for lo, hi in gc.SHARDS)
    assert (np.abs(parts - whole.value) <= 1e-12 * whole.mass).all()


def test_preconditions_raise():
    y = np.zeros((4, 2), np.float32)
    tiny = np.full((3, 2), 1e-30, np.float32)                  # s = 2e-60: below the smallest normal float32
    for kernel in ("gaussian", "absolute-exponential"):
        with pytest.raises(ValueError, match="smallest normal"):
            gm.lowd_gradient(kernel, y, tiny, None, precision=np.float32)
    with pytest.raises(ValueError, match="1/r\\^3"):           # r = 1e15: r^-3 = 1e-45 is denormal in float32
        gm.lowd_gradient("inverse-distance", y, np.full((3, 2), 1e15, np.float32), None, precision=np.float32)
    with pytest.raises(ValueError, match="infinite target"):
        gm.lowd_gradient("gaussian", y, np.full((3, 2), np.inf, np.float32), None, precision=np.float32)
    with pytest.raises(ValueError):
        gm.lowd_gradient("inverse-distance", y, tiny, None, precision=np.float32, dscale=True)
    # a squared distance that overflows is no error: the pair contributes exactly 0, with no band of its own
    m = gm.lowd_gradient("gaussian", y, np.full((3, 2), 1e30, np.float32), None, precision=np.float32, dscale=True)
    assert not m.value.any() and (m.band <= 4 * 4 * 2.0 ** -150).all() and not m.nonfinite.any()


def test_non_finite_inputs_follow_the_stated_rules():
    rs = np.random.RandomState(1)
    y, x, b = rs.randn(9, 3), rs.randn(6, 3), rs.randn(9, 2)
    clean = gm.lowd_gradient("gaussian", np.delete(y, 4, axis=0), x, np.delete(b, 4, axis=0), precision=np.float64)
    for v in (np.nan, np.inf, -np.inf):
        yb = y.copy()
        yb[4, 1] = v
        m = gm.lowd_gradient("gaussian", yb, x, b, precision=np.float64)
        assert not m.nonfinite.any() and m.poisoned[:, :, 1].all() and not m.poisoned[:, :, [0, 2]].any()
        assert np.isnan(m.value[:, :, 1]).all()
        assert np.allclose(m.value[:, :, [0, 2]], clean.value[:, :, [0, 2]], rtol=1e-14, atol=0)
    bb = b.copy()
    bb[4, 0] = np.nan
    m = gm.lowd_gradient("gaussian", y, x, bb, precision=np.float64)
    assert m.poisoned[:, 0, :].all() and not m.poisoned[:, 1, :].any() and not m.nonfinite.any()
    xb = x.copy()
    xb[2, 0] = np.nan
    m = gm.lowd_gradient("gaussian", y, xb, b, precision=np.float64, dscale=True)
    assert list(np.nonzero(m.nonfinite)[0]) == [2] and m.poisoned[2].all() and not np.delete(m.poisoned, 2, axis=0).any()


def test_the_product_branches_count_their_own_roundings():
    assert [gm.roundings(False, E, d) for E, d in ((1, False), (4, False), (1, True))] == [2, 2, 1]
    assert [gm.roundings(True, E, d) for E, d in ((1, False), (4, False), (1, True))] == [4, 4, 3]


SHARPNESS = {}   # (device kernel, function, precision, chunk) -> [min, max of band / mass, max emulation err / band]


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for (name, fn, prec, chunk), (lo, hi, worst) in sorted(SHARPNESS.items()):
        print(f"\nlowd grad model {name:18s} {fn:22s} {prec} chunk {chunk:3d}: band / mass {lo:.3g} ... {hi:.3g}, emulation err / band <= {worst:.3g}")


def inside(c, cfg, cache=None, **more):
    """(model, max err / band over the elements that must be finite, whether the non-finite elements are the model's)."""
    cache = {} if cache is None else cache
    key = cfg[:4] if c["precision"] == np.float32 else cfg[:3]
    if key not in cache:
        cache[key] = gc.model(c, cfg)
    m = cache[key]
    got = gc.emulate(c, cfg, **more)
    assert got.shape == m.value.shape
    must = ~m.poisoned
    rows_ok = bool((~np.isfinite(got[m.poisoned])).all())
    if c["kw"].get("loose"):                                   # what is not poisoned is non-finite too, or the other sources' sum
        must = must & np.isfinite(got)
    else:
        rows_ok = rows_ok and bool(np.isfinite(got[must]).all())
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.abs(got - m.value)
        ratio = np.where(m.band > 0, err / m.band, np.where(err > 0, np.inf, 0.0))[must]
    ratio = ratio[~np.isnan(ratio)]
    return m, (float(ratio.max()) if ratio.size else 0.0), rows_ok


def _emulation_key(c, cfg):
    """What of a configuration the emulation's arithmetic depends on: float64 has no fold; in float32 the folds fall at
    whole tiles of 256, so chunks that round up to the same number of tiles are one emulation."""
    which, sig, E, chunk, segments = cfg
    return which, sig, E, (-(-chunk // 256) if c["precision"] == np.float32 else 0), segments


GROUPS = [(kernel, p, g) for kernel in gc.KERNELS for p in PREC for g in ("grid", "edges", "range", "nonfinite")]


@pytest.mark.parametrize("kernel,prec,group", GROUPS, ids=["-".join(g) for g in GROUPS])
def test_clean_emulations_stay_inside_the_band_on_the_gpu_tests_clouds(kernel, prec, group):
    for c in gc.groups(kernel, PREC[prec])[group]:
        seen, cache = set(), {}
        for cfg in gc.configs(c):
            key = _emulation_key(c, cfg)
            if key in seen:
                continue
            seen.add(key)
            m, worst, rows_ok = inside(c, cfg, cache)
            assert rows_ok, (c["name"], cfg)
            assert worst <= 1.0, (c["name"], cfg, worst)
            assert list(np.nonzero(m.nonfinite)[0]) == c["kw"].get("bad_rows", []), (c["name"], cfg)
            ok = ~m.poisoned & (m.mass > 0)
            if ok.any() and group == "grid":
                rel = m.band[ok] / m.mass[ok]
                r = SHARPNESS.setdefault((gc.NAME[cfg[0]], kernel, prec, cfg[3]), [np.inf, 0.0, 0.0])
                r[0], r[1], r[2] = min(r[0], float(rel.min())), max(r[1], float(rel.max())), max(r[2], worst)


def test_far_rows_reach_the_flush_the_denormal_range_and_exact_zeros():
    for kernel in gc.DSCALE:
        far = lambda p: [c for c in gc.shared_cases(kernel, p) if c["name"][1] == "far"][0]
        m = gc.model(far(np.float64), ("dscale", "density", 1, 512, 0))
        v = np.abs(m.value[:, 0, 0])
        assert (v > 0).any() and (v[v > 0] < 2.0 ** -1022).any() and (v == 0).any(), kernel
        m = gc.model(far(np.float32), ("grad", "density", 1, 512, 0))
        lost = np.abs(m.value[:, 0, 0]) < 2.0 ** -130
        assert lost.any() and (m.band[lost, 0, 0] >= np.abs(m.value[lost, 0, 0])).all(), kernel


def _grid(kernel, prec, D=3, same=False):
    return [c for c in gc.grid_cases(kernel, prec) if c["name"][2] == D and (c["name"][0] == "grid-same") == same][0]


def _first(gen, *a, pick=lambda c: True):
    return [c for c in gen(*a) if pick(c)][0]


def _defect_runs(defect):
    """(case, configuration) on which a defect is tried: clouds and configurations of the GPU test."""
    F32, F64 = np.float32, np.float64
    g1, d1 = ("grad", "product", 1, 8, 0), ("dscale", "product", 1, 8, 0)
    g2, d2 = ("grad", "product", 2, 512, 0), ("dscale", "product", 2, 512, 0)
    if defect == "guard-s-lt-inf":     # the parent's select drops a non-finite source of the guard zone instead of letting it spoil every row
        return [(_first(gc.bad_source_cases, k, p, pick=lambda c: c["name"][2:] == (tag, 98)), g2)
                for k in ("gaussian", "inverse-distance", "matern-5/2") for p in (F32, F64) for tag in ("nan", "+inf")]
    if defect == "no-nan-row":         # float64 and the Matern kernels: the clamps turn the NaN s into w = 0
        return [(_first(gc.nan_target_cases, k, p, pick=lambda c: c["name"][2] == M), cfg)
                for k, p in (("gaussian", F64), ("matern-3/2", F32), ("absolute-exponential", F64)) for M in (5, 101) for cfg in (g2, d2)]
    if defect in ("no-wrap", "no-j-offset"):
        c = list(gc.zero_rule_cases(F32))[0]
        if defect == "no-wrap":
            return [(c, g1), (list(gc.zero_rule_cases(F64))[0], g1)]
        lo, hi = gc.SHARDS[1]
        return [(dict(c, y=c["y"][lo:hi], b=c["b"][lo:hi], kw=dict(j_offset=lo, M_total=200)), g1)]
    if defect in ("pad-df-kept", "drop-ragged", "fold-assigns"):
        big = lambda k, p: _first(gc.size_cases, k, p, pick=lambda c: c["name"][3] == 1030)
        pick = big if defect == "fold-assigns" else _grid       # M = 101: 3 pad records, M mod 4 = 1
        return [(pick("gaussian", F32), g1), (pick("matern-5/2", F32), d2)] + ([] if defect == "fold-assigns" else [(pick("gaussian", F64), d1)])
    if defect == "columns-transposed":                          # D = 3 != E = 2, 4: the signal columns differ in scale and sign
        return [(_grid("gaussian", p), cfg) for p in (F32, F64) for cfg in (g2, d2, ("grad", "product", 4, 512, 0))]
    if defect == "matern-value-degree":
        return [(_grid(k, p), cfg) for k in ("matern-3/2", "matern-5/2") for p in (F32, F64) for cfg in (g1, d2)]
    if defect == "five-thirds-is-one":
        return [(_grid("matern-5/2", p), cfg) for p in (F32, F64) for cfg in (g1, d2)]
    if defect == "no-s0-select":
        return [(list(gc.duplicate_cases("absolute-exponential", p))[0], cfg) for p in (F32, F64) for cfg in (g2, d2)]
    if defect == "kept-square":
        return [(list(gc.overflow_cases(k, F32))[0], d1) for k in gc.DSCALE]
    if defect == "b0-for-every-e":
        return [(_grid("gaussian", p), d2) for p in (F32, F64)]
    if defect == "constant-sign":
        return [(_grid(k, F32), cfg) for k in gc.KERNELS for cfg in (g1, d1) if cfg[0] in gc.whiches(k)]
    raise KeyError(defect)


@pytest.mark.parametrize("defect", gc.DEFECTS)
def test_a_defective_kernel_leaves_the_band(defect):
    """The emulation with one defect is outside the band, or non-finite where the model is finite, or finite where it
    is not, on every cloud listed for it, where the clean emulation is inside on every element; prints by how much."""
    runs = _defect_runs(defect)
    assert runs
    for c, cfg in runs:
        _, clean, rows_ok = inside(c, cfg)
        assert rows_ok and clean <= 1.0, (defect, c["name"], clean)
        _, worst, rows_ok = inside(c, cfg, defect=defect)
        margin = np.inf if not rows_ok else worst
        print(f"\nlowd grad defect {defect:20s} {gc.NAME[cfg[0]]:18s} {c['kernel']:22s} {c['precision'].name} {c['name'][0]}: err / band {margin:.3g} (clean {clean:.3g})")
        assert margin > 1.0, (defect, c["name"], cfg, margin)


def test_the_parents_select_and_a_nan_target():
    """The issue's first defect as worded -- the guard's select written as s < inf, with a NaN target at M <= 8 and on a
    wrapping 1/r tile -- shows only together with the missing NaN row: the parent's two defects gave a row of exact zeros
    (M <= 8, every batch guarded) or a row that is NaN on one axis only.  With the row restored when it is written, the
    select alone gives the same bits at a NaN target: a stated exception.  What it still changes is a non-finite SOURCE
    of the guard zone (test_a_defective_kernel_leaves_the_band)."""
    for kernel, p, tag in (("gaussian", np.float32, 5), ("gaussian", np.float64, 8), ("matern-5/2", np.float32, 5),
                           ("inverse-distance", np.float64, "wrap"), ("inverse-distance", np.float32, 5)):
        c = _first(gc.nan_target_cases, kernel, p, pick=lambda c: c["name"][2] == tag)
        row = c["kw"]["bad_rows"][0]
        for cfg in [("grad", "product", c["b"].shape[1], 512, 0)] + ([] if kernel == "inverse-distance" else [("dscale", "product", 2, 512, 0)]):
            clean = gc.emulate(c, cfg)
            alone = gc.emulate(c, cfg, defect="guard-s-lt-inf")
            assert np.array_equal(clean, alone, equal_nan=True), (c["name"], cfg)
            parent = gc.emulate(c, cfg, defect=("guard-s-lt-inf", "no-nan-row"))
            print(f"\nlowd grad parent's NaN row {kernel:22s} {np.dtype(p).name} {tag}: {parent[row].ravel()[:6]}")
            assert np.isfinite(parent[row]).any() and np.isnan(clean[row]).all(), (c["name"], cfg)
            assert not parent[row][np.isfinite(parent[row])].any(), "what the parent leaves finite are exact zeros"
