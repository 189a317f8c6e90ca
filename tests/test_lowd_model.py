"""oracle/kmvp_lowd_model.py on the CPU: the model with rounding disabled against the float64 oracle and the Matern
definition; numpy emulations of lowd_kernel's, lowd_mid_kernel's and lowd_big_kernel's own steps inside the band on every
cloud and configuration tests/test_gpu_lowd_arith.py runs; the same emulations with one defect at a time outside it.
Prints band / mass per (kernel, function, precision) and the defects' margins (pytest -s), for the record."""
import numpy as np
import pytest

import kmvp_lowd_model as lm
import kmvp_oracle
import lowd_model_cases as cases
import matern_reference

PLAIN = [(kernel, sig, same) for kernel in cases.KERNELS for sig in cases.SIGS for same in (False, True)]
PREC = {"f32": np.float32, "f64": np.float64}


@pytest.mark.parametrize("kernel,sig,same", PLAIN, ids=["-".join(map(str, p)) for p in PLAIN])
def test_model_without_rounding_is_the_float64_product(kernel, sig, same):
    rs = np.random.RandomState(len(kernel) + len(sig))
    D, M, N = 5, 70, 70 if same else 90                       # N > M + 1: the zero rule wraps
    y = rs.rand(M, D) / np.sqrt(D)
    x = None if same else rs.rand(N, D) / np.sqrt(D)
    b = None if sig == "density" else rs.randn(M, 3) + 0.5
    got = lm.lowd_product(kernel, y, x, b, sig == "norm", precision=np.float64, rounding=False)
    ref = matern_reference.product if kernel in matern_reference.KERNELS else kmvp_oracle.product
    want = ref(kernel=kernel, source_points=y, target_points=x, source_signal=b, normalize_rows=sig == "norm")
    assert got.value.shape == want.shape == (N, 1 if b is None else 3)
    assert not got.band.any() and not got.flagged.any() and not got.nonfinite.any()
    assert np.abs(got.value - want).max() <= 1e-12 * np.abs(want).max()


def test_model_rounds_the_inputs_to_the_working_precision_first():
    rs = np.random.RandomState(4)
    y, x, b = rs.rand(40, 3), rs.rand(30, 3), rs.randn(40, 2)
    got = lm.lowd_product("gaussian", y, x, b, precision=np.float32, rounding=False).value
    want = kmvp_oracle.product(kernel="gaussian", source_points=y.astype(np.float32).astype(np.float64),
                               target_points=x.astype(np.float32).astype(np.float64), source_signal=b.astype(np.float32).astype(np.float64))
    assert np.abs(got - want).max() <= 1e-14 * np.abs(want).max()


def test_model_of_a_source_slice_follows_the_global_zero_rule():
    """Three slices with j_offset / M_total, N > M_total + 1: their values add up to the whole's."""
    rs = np.random.RandomState(2)
    y, x, b = rs.rand(200, 3), rs.rand(450, 3), rs.randn(200, 1)
    whole = lm.lowd_product("inverse-distance", y, x, b, precision=np.float64, rounding=False).value
    parts = sum(lm.lowd_product("inverse-distance", y[lo:hi], x, b[lo:hi], precision=np.float64, j_offset=lo, M_total=200,
                                rounding=False).value for lo, hi in cases.SHARDS)
    assert np.abs(parts - whole).max() <= 1e-12 * np.abs(whole).max()


def test_preconditions_raise():
    y = np.zeros((4, 2), np.float32)
    x = np.full((3, 2), 1e-30, np.float32)                    # s = 2e-60: below the smallest normal float32
    with pytest.raises(ValueError, match="smallest normal"):
        lm.lowd_product("gaussian", y, x, None, precision=np.float32)
    with pytest.raises(ValueError, match="overflows"):
        lm.lowd_product("gaussian", y, np.full((3, 2), 1e30, np.float32), None, precision=np.float32)
    far = np.full((3, 2), 7.1, np.float32)                    # e^-101: every pair of a float32 row may be flushed
    with pytest.raises(ValueError, match="denominator"):
        lm.lowd_product("gaussian", y, far, np.ones((4, 1), np.float32), True, precision=np.float32)
    assert not lm.lowd_product("gaussian", y, far, None, precision=np.float32).flagged.any()


def test_chain_lengths_follow_the_code():
    assert lm.chain_length("lowd", np.float32, 1000, chunk=8, feed=0) == 8
    assert lm.chain_length("lowd", np.float32, 1000, chunk=12, feed=0) == 16      # rounded up to the ping-pong of 8
    assert lm.chain_length("lowd", np.float32, 1000, chunk=8, feed=1) == 256      # whole LDS tiles
    assert lm.chain_length("lowd", np.float32, 1000, chunk=512, feed=1) == 512
    assert lm.chain_length("lowd", np.float32, 101, chunk=512, feed=1) == 101     # at most the sources
    assert lm.chain_length("mid", np.float32, 1000) == lm.chain_length("big", np.float32, 1000) == 64
    assert lm.chain_length("mid", np.float64, 1000) == 1000                       # float64: one chain


def _emulation_key(c, cfg):
    """What of a configuration the emulation's arithmetic depends on (T never; float64 lowd_kernel has no folds)."""
    sig, E, T, feed, chunk, segments = cfg
    if c["path"] != "lowd" or c["precision"] == np.float64:
        feed, chunk = 1, 512
    return sig, E, feed, chunk, segments


SHARPNESS = {}   # (device kernel, function, precision, chunk) -> [min, max] of band / mass over the clean runs
GROUPS = [(kernel, p, g) for kernel in cases.KERNELS for p in PREC for g in ("grid", "mid", "big", "blocks", "edges")]


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for (name, fn, prec, chunk), (lo, hi, worst) in sorted(SHARPNESS.items()):
        print(f"\nlowd model {name:16s} {fn:22s} {prec} chunk {chunk:3d}: band / mass {lo:.3g} ... {hi:.3g}, emulation err / band <= {worst:.3g}")


def _inside(c, cfg, cache=None, **more):
    """The emulation of one configuration against the model of the same: max err / band over the finite rows; rows the
    model calls non-finite are non-finite in the emulation, and no others."""
    sig, E, T, feed, chunk, segments = cfg
    if c["path"] == "lowd" and T == 0:
        feed = 1
    key = (sig, E, lm.chain_length(c["path"], c["precision"], len(c["y"]), chunk, feed))
    cache = {} if cache is None else cache                   # configurations whose longest chain is the same share a model
    if key not in cache:
        cache[key] = cases.model(c, sig, E, feed=feed, chunk=chunk)
    m = cache[key]
    got = cases.emulate(c, sig, E, feed=feed, chunk=chunk, segments=max(segments, 1), **more)
    assert got.shape == m.value.shape and not m.flagged.any()
    bad = m.nonfinite
    finite = np.isfinite(got).all(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        err = np.abs(got - m.value)
        ratio = np.where(m.band > 0, err / m.band, np.where(err > 0, np.inf, 0.0))[~bad]
    return m, (ratio.max() if ratio.size else 0.0), np.array_equal(finite, ~bad)


@pytest.mark.parametrize("kernel,prec,group", GROUPS, ids=["-".join(g) for g in GROUPS])
def test_clean_emulations_stay_inside_the_band_on_the_gpu_tests_clouds(kernel, prec, group):
    """Every case of cases.groups() under every configuration of cases.configs() whose arithmetic differs: the emulation
    within the band on every element, non-finite exactly where the model is, no row flagged."""
    for c in cases.groups(kernel, PREC[prec])[group]:
        seen, cache = set(), {}
        for cfg in cases.configs(c):
            key = _emulation_key(c, cfg)
            if key in seen:
                continue
            seen.add(key)
            m, worst, same_rows = _inside(c, cfg, cache)
            assert same_rows, (c["name"], cfg)
            assert worst <= 1.0, (c["name"], cfg, worst)
            if "bad_rows" in c["kw"]:
                assert list(np.nonzero(m.nonfinite)[0]) == c["kw"]["bad_rows"], (c["name"], cfg)
            else:
                # (beyond e^-745 a normalised float64 row is 0 / 0, as is 1/r's only pair under the zero rule)
                assert not m.nonfinite.any() or c["name"][0] == "far" or c["name"][2:] == ("inverse-distance", 1, 1), (c["name"], cfg)
            ok = ~m.nonfinite & (m.mass > 0).all(axis=1)
            if ok.any() and c["name"][0] in ("grid", "mid", "big"):
                rel = (m.band[ok] / m.mass[ok])
                r = SHARPNESS.setdefault((cases.NAME[c["path"]], kernel, prec, cfg[4]), [np.inf, 0.0, 0.0])
                r[0], r[1], r[2] = min(r[0], float(rel.min())), max(r[1], float(rel.max())), max(r[2], float(worst))


def test_far_rows_reach_the_denormal_range_the_flush_and_the_clamps():
    """The far clouds do what their docstring says: float64 rows with denormal sums and with exact zeros past e^-745,
    float32 rows past the flush; no row of them is non-finite unless it is normalised."""
    for kernel in cases.KERNELS[:2] + cases.KERNELS[3:]:
        c = [c for c in cases.far_cases(kernel, np.float64) if c["name"][0] == "far"][0]
        v = cases.model(c, "density").value[:, 0]
        assert (v > 0).any() and (v[v > 0] < 2.0 ** -1022).any() and (v == 0).any(), kernel
        c = [c for c in cases.far_cases(kernel, np.float32) if c["name"][0] == "far"][0]
        m = cases.model(c, "density")
        assert (m.value[:, 0] < 2.0 ** -126).any() and (m.band >= m.value)[m.value[:, 0] < 2.0 ** -130].all(), kernel


def _case(group, kernel, prec, pick=lambda c: True):
    return [c for c in cases.groups(kernel, prec)[group] if pick(c)][0]


def _defect_runs(defect):
    """(case, configuration, emulation arguments) on which a defect is tried: clouds of the GPU test, chunk = 8."""
    F32, F64 = np.float32, np.float64
    lowd = ("product", 1, 2, 0, 8, 0)
    if defect == "no-wrap":
        return [(c, lowd if c["path"] == "lowd" else ("product", 1, 0, 0, 512, 0)) for p in ("lowd", "mid", "big") for c in cases.zero_rule_cases(F32, p)]
    if defect == "no-j-offset":
        out = []
        for p in ("lowd", "mid", "big"):
            c = list(cases.zero_rule_cases(F32, p))[0]
            lo, hi = cases.SHARDS[1]
            out.append((dict(c, y=c["y"][lo:hi], b=c["b"][lo:hi], kw=dict(j_offset=lo, M_total=200)), lowd if p == "lowd" else ("product", 1, 0, 0, 512, 0)))
        return out
    if defect == "drop-ragged":
        return [(list(cases.grid_cases("gaussian", F32))[2], lowd), (list(cases.big_cases("gaussian", F32))[0], ("product", 1, 0, 0, 512, 0)),
                (list(cases.grid_cases("gaussian", F64))[2], lowd)]
    if defect == "fold-assigns":
        return [(list(cases.grid_cases("gaussian", F32))[2], lowd), (list(cases.mid_cases("gaussian", F32))[0], ("product", 1, 0, 0, 512, 0)),
                (list(cases.big_cases("gaussian", F64))[0], ("product", 1, 0, 0, 512, 0))]
    if defect == "scaled-coords":
        return [(list(cases.moved_cases(k, F32, "lowd"))[0], lowd) for k in ("gaussian", "absolute-exponential")]
    if defect in ("no-newton",):
        return [(list(cases.grid_cases(k, F64))[2], lowd) for k in ("absolute-exponential", "inverse-distance", "matern-3/2", "matern-5/2")]
    if defect in ("no-cw-lo", "poly-deg4"):
        # (the polynomial's last term is at most 3.9e-14 of a pair and of either sign: few sources, so that it does not average out)
        pick = (lambda c: c["name"][3:] == (65, 5)) if defect == "poly-deg4" else (lambda c: c["name"][3:] == (257, 9))
        return [(_case("edges", k, F64, lambda c: c["name"][0] == "size" and c["path"] == "lowd" and pick(c)), lowd)
                for k in ("gaussian", "absolute-exponential", "matern-3/2", "matern-5/2")]
    if defect == "matern52-no-t2":
        return [(list(cases.grid_cases("matern-5/2", p))[2], lowd) for p in (F32, F64)]
    if defect == "clamp-after-poly":
        return [(list(cases.grid_cases(k, p))[2], lowd) for k in ("matern-3/2", "matern-5/2") for p in (F32, F64)]
    if defect == "den-wrong-block":
        return [(list(cases.block_cases("gaussian", p))[0], ("norm", 6, 0, 0, 8, 0)) for p in (F32, F64)]
    raise KeyError(defect)


MARGINS = {}


@pytest.mark.parametrize("defect", cases.DEFECTS)
def test_a_defective_kernel_leaves_the_band(defect):
    """The emulation with one defect is outside the band (or non-finite where the model is finite) on every cloud listed
    for it, where the emulation without the defect is inside on every element; prints by how much."""
    for c, cfg in _defect_runs(defect):
        _, clean, rows_ok = _inside(c, cfg)
        assert rows_ok and clean <= 1.0, (defect, c["name"], clean)
        _, worst, rows_ok = _inside(c, cfg, defect=defect)
        margin = np.inf if not rows_ok else worst
        print(f"\nlowd defect {defect:16s} {cases.NAME[c['path']]:16s} {c['kernel']:22s} {c['precision'].name}: err / band {margin:.3g} (clean {clean:.3g})")
        assert margin > 1.0, (defect, c["name"], margin)


def test_the_denominator_is_the_same_sum_in_every_column_block():
    """The issue's eleventh defect as worded -- the normalised denominator taken from the second column block -- cannot
    leave the band: K 1 is the same chain of the same kernel values in whichever launch it is summed, so the result is
    bit for bit the same.  (What can go wrong is WHICH column is read: den-wrong-block above.)"""
    c = list(cases.block_cases("gaussian", np.float32))[0]
    first = cases.emulate(c, "norm", 6, chunk=8)
    c2 = dict(c, b=np.ascontiguousarray(np.concatenate((c["b"][:, 4:6], c["b"][:, :4]), axis=1)))
    second = cases.emulate(c2, "norm", 6, chunk=8)
    assert np.array_equal(first[:, :4], second[:, 2:6]) and np.array_equal(first[:, 4:6], second[:, :2])
