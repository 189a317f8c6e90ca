"""oracle/kmvp_lse_model.py on the CPU: the model with rounding disabled against the restatements (tests/lse_reference.py,
tests/lse_grad_reference.py) on every cloud of the GPU test but those with a NaN or +inf log-weight, a NaN source
coordinate (no restatement of a rule that is not stated) and the targets at 1e20 (see the test); numpy emulations of
lowd_lse_kernel's and lowd_lse_grad_kernel's own steps (tests/lse_model_cases.py: the batch of 4, ceil, the rescales with
their clamps, the folds, the merge, the finish) inside the band on every cloud and configuration
tests/test_gpu_lse_arith.py runs, and of lowd_batch_lse_kernel's feed; the same emulations with one defect at a time
outside it.  Prints the band per (kernel, function, precision, chunk) and the defects' margins (pytest -s).

The case each defective emulation leaves the band on (test_a_defective_kernel_leaves_the_band):
  rise-skips-fp64        a rise after a fold rescales the fp32 sum and not the fp64 one: ("shift", *, "after-fold"), float32,
                         one segment (L and G); float64 has no fp64 partner
  rise-skips-V           a rise rescales Z and not V: ("shift", *, "nearest-last"), G, both precisions
  merge-first-exponent   the merge takes the first segment's exponent: ("shift", *, "dead-first-segment"), three segments,
                         column 0 -- the first segment has no live term there, its exponent is +inf.  Where every segment
                         is live the defect is NOT a defect of the result: the factors 2^(K - k_s) are exact powers of two
                         for any common K, also above 1, so ("segments", *) stays inside the band with it (asserted)
  drop-ragged            the last batch of a ragged tile dropped: ("grid", *, 3), M = 101
  no-newton              float64 exp(-r) logit from the bare rsq estimate: ("grid", "absolute-exponential", 3), float64
  no-guard               the guard removed from the pad batches: ("grid", *, 3), G: NaN where the model is finite
  no-s0-select           exp(-r) gradient with the coincident pair's direction not zeroed: ("range", *, "duplicates"), G
and the two defects the GPU test found in the kernels themselves:
  nan-weight-dropped     float64 L: the exponential's clamp turns the NaN of m - u into a weight of 0:
                         ("bad-logweight", *, "nan") and, under 3 segments, ("bad-logweight", *, "+inf"): a finite column
  guard-s-lt-inf         the gradient's guard written as s < inf: ("bad-source", *, "+inf" / "-inf", 98), the source in the
                         guard zone: its axis finite where include/kmvp.h says NaN"""
import numpy as np
import pytest

import kmvp_lse_model as sm
import lse_grad_reference
import lse_model_cases as lc
import lse_reference

PREC = {"f32": np.float32, "f64": np.float64}
EACH = [(kernel, p) for kernel in lc.KERNELS for p in PREC]
IDS = [f"{k}-{p}" for k, p in EACH]
CLEAN_GROUPS = ("grid", "edges", "shift", "range")


def restatement(c, cfg):
    """The committed restatement in float64 arithmetic on the inputs as rounded to the case's precision."""
    which, sig, E, _, _ = cfg
    dt = c["precision"]
    r64 = lambda a: None if a is None else np.asarray(a, dtype=dt).astype(np.float64)
    kw = dict(kernel=c["kernel"], source_points=r64(c["y"]), target_points=r64(c["x"]), source_signal=r64(lc.signal_of(c, sig, E)))
    return lse_grad_reference.gradient(**kw) if which == "grad" else lse_reference.logsumexp(**kw)


@pytest.mark.parametrize("kernel,prec", EACH, ids=IDS)
def test_model_without_rounding_is_the_restatement(kernel, prec):
    """The restatements run in float64: a logit is off by about (|c| + nl) D u, which L takes absolutely and the softmax
    weights relatively.  1e-12 (1 + |L| + max |c|) for L and 1e-9 of the component's mass for G cover logits down to -1e6
    with room.  From the non-finite group: a NaN target (its row NaN in both, every other row compared) and, for L, a
    +-inf source coordinate (its pairs weigh 0 in both).  Left out: the targets at 1e20 -- in float32 the restatement's
    own float64 squares do not overflow where the kernels' do, in float64 the restatement's float64 logits of -1e40
    cannot be told apart (the model's value is formed in extended precision and its band there is 2e-15 |L|)."""
    seen = 0
    extra = [c for c in lc.groups(kernel, PREC[prec])["nonfinite"]
             if c["name"][0] == "nan-target" or (c["name"][0] == "bad-source" and c["name"][2] != "nan")]
    for group in CLEAN_GROUPS + ("nonfinite",):
        for c in (extra if group == "nonfinite" else lc.groups(kernel, PREC[prec])[group]):
            if c["name"][2] == "targets-at-1e20":
                continue
            for cfg in {(w, s, e, 512, 0) for w, s, e, _, _ in lc.configs(c) if w == "lse" or c["name"][0] != "bad-source"}:
                m = lc.model(c, cfg, rounding=False)
                want = restatement(c, cfg)
                assert m.value.shape == want.shape and not m.band.any()
                assert np.array_equal(np.nonzero(m.poisoned.reshape(len(want), -1).any(axis=1))[0], c["kw"].get("bad_rows", []))
                assert np.array_equal(np.isnan(want), np.isnan(m.value)) and np.array_equal(np.isneginf(want), np.isneginf(m.value)), (c["name"], cfg)
                fin = np.isfinite(want)
                cmax = float(np.abs(c["b"][np.isfinite(c["b"])]).max()) if np.isfinite(c["b"]).any() else 0.0
                tol = 1e-12 * (1.0 + np.abs(want[fin]) + cmax) if cfg[0] == "lse" else 1e-9 * m.mass[fin] + 1e-300
                assert (np.abs(m.value[fin] - want[fin]) <= tol).all(), (c["name"], cfg, float(np.abs(m.value[fin] - want[fin]).max()))
                seen += 1
    assert seen > 80


def test_preconditions_raise():
    y = np.zeros((4, 2), np.float32)
    for fn in (sm.lse, sm.lse_gradient):
        with pytest.raises(ValueError, match="smallest normal"):
            fn("gaussian", y, np.full((3, 2), 1e-30, np.float32), None, precision=np.float32)
        with pytest.raises(ValueError, match="infinite target"):
            fn("gaussian", y, np.full((3, 2), np.inf, np.float32), None, precision=np.float32)
        with pytest.raises(ValueError, match="may or may not overflow"):
            fn("gaussian", y, np.array([[1.8446744e19, 0.0]], np.float32), None, precision=np.float32)
        with pytest.raises(ValueError):
            fn("inverse-distance", y, None, None, precision=np.float32)
    # a squared distance that overflows is no error: the pair contributes exactly 0; a row of such pairs has no live term
    m = sm.lse("gaussian", y, np.full((3, 2), 1e30, np.float32), None, precision=np.float32)
    assert np.isneginf(m.value).all() and not m.band.any() and not m.poisoned.any()
    m = sm.lse_gradient("gaussian", y, np.full((3, 2), 1e30, np.float32), None, precision=np.float32)
    assert np.isnan(m.value).all() and not m.poisoned.any()


def test_exact_rules_are_properties_of_the_value():
    rs = np.random.RandomState(1)
    y, x, b = rs.randn(9, 3), rs.randn(6, 3), rs.randn(9, 2)
    for fn in (sm.lse, sm.lse_gradient):
        clean = fn("absolute-exponential", np.delete(y, 4, axis=0), x, np.delete(b, 4, axis=0), precision=np.float64)
        bb = b.copy()
        bb[4] = -np.inf                                            # weight 0: the same value as without the source
        m = fn("absolute-exponential", y, x, bb, precision=np.float64)
        assert np.allclose(m.value, clean.value, rtol=1e-14, atol=0) and not m.poisoned.any()
        for v in (np.nan, np.inf):                                 # the column is poisoned for every target, the other untouched
            bb = b.copy()
            bb[4, 1] = v
            m = fn("absolute-exponential", y, x, bb, precision=np.float64)
            assert m.poisoned[:, 1].all() and not m.poisoned[:, 0].any() and np.isnan(m.value[:, 1]).all()
        xb = x.copy()
        xb[2, 0] = np.nan
        m = fn("absolute-exponential", y, xb, b, precision=np.float64)
        assert list(np.nonzero(m.nonfinite)[0]) == [2] and m.poisoned[2].all() and not np.delete(m.poisoned, 2, axis=0).any()
        for v in (np.nan, np.inf, -np.inf):                        # a non-finite source coordinate leaves the modelled sums
            yb = y.copy()
            yb[4, 1] = v
            m = fn("absolute-exponential", yb, x, b, precision=np.float64)
            if fn is sm.lse:
                assert not m.poisoned.any() and np.allclose(m.value, clean.value, rtol=1e-14, atol=0)
            else:
                assert m.poisoned[:, :, 1].all() and not m.poisoned[:, :, [0, 2]].any()
                assert np.allclose(m.value[:, :, [0, 2]], clean.value[:, :, [0, 2]], rtol=1e-14, atol=0)
    empty = sm.lse("gaussian", y[:0], x, None, precision=np.float32)
    assert empty.value.shape == (6, 1) and np.isneginf(empty.value).all()
    assert np.isnan(sm.lse_gradient("gaussian", y[:0], x, b[:0], precision=np.float32).value).all()
    # exp(-r): a coincident pair adds nothing to V and keeps its weight in Z
    yd = y.copy()
    yd[7] = x[3]
    g = sm.lse_gradient("absolute-exponential", yd, x, None, precision=np.float64)
    want = lse_grad_reference.gradient(kernel="absolute-exponential", source_points=yd, target_points=x)
    assert np.allclose(g.value, want, rtol=1e-12, atol=1e-15)


def test_the_band_is_absolute_in_the_logit_and_below_the_old_rule_where_it_was_loose():
    """float64: two orders below 1e-11 max(1, |L|) on ordinary clouds (M = 101: a chain of 80 u and K_BAND).  float32 at logits near -1e4: the old rule allowed about
    0.1 in L; the chain of s (D + 2 = 5 roundings), c - nl and the two of LOG2E give a few 1e-3 for the Gaussian.  float32
    rows with |L| below 1: the 256-long fp32 chain alone allows min(256, 8 sqrt 256) u = 7.6e-6, twice that with K_BAND:
    looser than the old 1e-5, as stated in LAB_NOTES.md."""
    cfg = ("lse", "product", 2, 512, 0)
    for kernel in lc.KERNELS:
        grid = [c for c in lc.grid_cases(kernel, np.float64) if c["name"][2] == 3][0]
        assert lc.model(grid, cfg).band.max() < 1e-13
        large = [c for c in lc.range_cases(kernel, np.float32) if c["name"][2] == "large-logits"][0]
        m = lc.model(large, cfg)
        assert np.abs(m.value).min() > 5e3 and m.band.max() < (2e-2 if kernel == "gaussian" else 5e-2), (kernel, m.band.max())
        m64 = lc.model([c for c in lc.range_cases(kernel, np.float64) if c["name"][2] == "large-logits"][0], cfg)
        assert np.abs(m64.value).min() > 5e5 and m64.band.max() < 1e-8, (kernel, m64.band.max())
        grid32 = [c for c in lc.grid_cases(kernel, np.float32) if c["name"][2] == 3][0]
        b = lc.model(grid32, cfg).band
        assert 5e-6 < b.min() and b.max() < 5e-5, (kernel, b.min(), b.max())


SHARPNESS = {}   # (device kernel, function, precision, chunk) -> [min, max of band / mass, max emulation err / band]


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for (name, fn, prec, chunk), (lo, hi, worst) in sorted(SHARPNESS.items()):
        print(f"\nlse model {name:20s} {fn:22s} {prec} chunk {chunk:3d}: band / mass {lo:.3g} ... {hi:.3g}, emulation err / band <= {worst:.3g}")


def inside(c, cfg, cache=None, **more):
    """(model, max err / band, what is wrong or None) of the emulation of one configuration."""
    cache = {} if cache is None else cache
    key = cfg[:4] if c["precision"] == np.float32 else cfg[:3]
    if key not in cache:
        cache[key] = lc.model(c, cfg)
    m = cache[key]
    worst, msg = lc.compare(lc.emulate(c, cfg, **more), m, lc.loose(c, cfg[0]))
    return m, worst, msg


def _emulation_key(c, cfg):
    """float64 has no fold; in float32 the folds fall at whole tiles of 256."""
    which, sig, E, chunk, segments = cfg
    return which, sig, E, (-(-chunk // 256) if c["precision"] == np.float32 else 0), segments


GROUPS = [(kernel, p, g) for kernel in lc.KERNELS for p in PREC for g in CLEAN_GROUPS + ("nonfinite",)]


@pytest.mark.parametrize("kernel,prec,group", GROUPS, ids=["-".join(g) for g in GROUPS])
def test_clean_emulations_stay_inside_the_band_on_the_gpu_tests_clouds(kernel, prec, group):
    for c in lc.groups(kernel, PREC[prec])[group]:
        seen, cache = set(), {}
        for cfg in lc.configs(c):
            key = _emulation_key(c, cfg)
            if key in seen:
                continue
            seen.add(key)
            m, worst, msg = inside(c, cfg, cache)
            assert msg is None, (c["name"], cfg, msg)
            assert list(np.nonzero(m.nonfinite)[0]) == c["kw"].get("bad_rows", []), (c["name"], cfg)
            ok = ~m.poisoned & np.isfinite(m.value) & (m.mass > 0)
            if ok.any() and group == "grid":
                rel = m.band[ok] / m.mass[ok]
                r = SHARPNESS.setdefault((lc.NAME[cfg[0]], kernel, prec, cfg[3]), [np.inf, 0.0, 0.0])
                r[0], r[1], r[2] = min(r[0], float(rel.min())), max(r[1], float(rel.max())), max(r[2], worst)


@pytest.mark.parametrize("kernel,prec", EACH, ids=IDS)
def test_the_scalar_cache_feed_of_the_batched_kernel_stays_inside_its_band(kernel, prec):
    """feed = 0: no segments, a fold every `chunk` rounded up to 8 -- M = 300 under chunk = 8, 64 and 512."""
    rs = np.random.RandomState(lc.cases.seed("lse-feed0", kernel))
    c = lc.case(("feed0", kernel), kernel, PREC[prec], lc.cases.points(rs, 300, 3, PREC[prec]), lc.cases.points(rs, 65, 3, PREC[prec]),
                lc.logweights(rs, 300, 1, PREC[prec]), feed=0)
    for chunk in (8, 64, 512):
        m, worst, msg = inside(c, ("lse", "product", 1, chunk, 0))
        assert msg is None, (chunk, msg)
    if prec == "f32":
        assert lc.model(c, ("lse", "product", 1, 8, 0)).band.max() < lc.model(c, ("lse", "product", 1, 512, 0)).band.max()


def _pick(gen, kernel, p, tag):
    return [c for c in gen(kernel, p) if c["name"][2] == tag][0]


def _defect_runs(defect):
    """(case, configuration) on which a defect is tried: clouds and configurations of the GPU test."""
    F32, F64 = np.float32, np.float64
    both = [(k, p) for k in lc.KERNELS for p in (F32, F64)]
    L1, G1 = ("lse", "product", 2, 256, 1), ("grad", "product", 2, 256, 1)
    L3, G3 = ("lse", "product", 2, 256, 3), ("grad", "product", 2, 256, 3)
    if defect == "rise-skips-fp64":
        return [(_pick(lc.shift_cases, k, F32, "after-fold"), cfg) for k in lc.KERNELS for cfg in (L1, G1)]
    if defect == "rise-skips-V":
        return [(_pick(lc.shift_cases, k, p, "nearest-last"), G1) for k, p in both]
    if defect == "merge-first-exponent":
        return [(_pick(lc.shift_cases, k, p, "dead-first-segment"), cfg) for k, p in both for cfg in (L3, G3)]
    if defect == "drop-ragged":
        return [(_pick(lc.grid_cases, k, p, 3), (w, "product", 1, 8, 0)) for k, p in both for w in lc.WHICH]
    if defect == "no-newton":
        return [(_pick(lc.grid_cases, "absolute-exponential", F64, 3), (w, "product", 2, 512, 0)) for w in lc.WHICH]
    if defect == "no-guard":
        return [(_pick(lc.grid_cases, k, p, 3), ("grad", "product", 2, 512, 0)) for k, p in both]
    if defect == "no-s0-select":
        return [(_pick(lc.range_cases, "absolute-exponential", p, "duplicates"), ("grad", s, e, 512, 0))
                for p in (F32, F64) for s, e in (("product", 2), ("density", 1))]
    if defect == "nan-weight-dropped":
        bad = lambda k, tag: [c for c in lc.nonfinite_cases(k, F64) if c["name"][0] == "bad-logweight" and c["name"][2] == tag][0]
        return [(bad(k, "nan"), ("lse", "product", 2, 512, 0)) for k in lc.KERNELS] + [(bad(k, "+inf"), ("lse", "product", 2, 512, 3)) for k in lc.KERNELS]
    if defect == "guard-s-lt-inf":
        return [([c for c in lc.nonfinite_cases(k, p) if c["name"][0] == "bad-source" and c["name"][2:] == (tag, 98)][0], ("grad", "product", 2, 512, 0))
                for k, p in both for tag in ("+inf", "-inf")]
    raise KeyError(defect)


@pytest.mark.parametrize("defect", lc.DEFECTS)
def test_a_defective_kernel_leaves_the_band(defect):
    """The emulation with one defect is outside the band, or non-finite where the model is finite, on every cloud listed
    for it, where the clean emulation is inside on every element; prints by how much."""
    runs = _defect_runs(defect)
    assert runs
    for c, cfg in runs:
        _, clean, msg = inside(c, cfg)
        assert msg is None and clean <= 1.0, (defect, c["name"], msg)
        _, worst, msg = inside(c, cfg, defect=defect)
        print(f"\nlse defect {defect:22s} {lc.NAME[cfg[0]]:20s} {c['kernel']:22s} {c['precision'].name} {c['name'][2]}: {msg} (clean {clean:.3g})")
        assert msg is not None, (defect, c["name"], cfg, worst)


def test_the_first_segments_exponent_is_harmless_where_every_segment_is_live():
    """The stated exception of merge-first-exponent: any common exponent gives the same sum up to the order of exact
    rescales, so with every segment live the emulation stays inside the band."""
    for kernel in lc.KERNELS:
        c = list(lc.segment_cases(kernel, np.float32))[0]
        for cfg in (("lse", "product", 2, 512, 3), ("grad", "product", 2, 512, 17)):
            _, worst, msg = inside(c, cfg, defect="merge-first-exponent")
            assert msg is None, (kernel, cfg, msg)
