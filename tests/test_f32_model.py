"""oracle/kmvp_f32_model.py on the CPU: the model with rounding disabled against the float64 oracle; numpy emulations of
fast_kernel's and cfast_kernel's own steps inside the band; the same emulation with one defect at a time outside it, on
the clouds tests/test_gpu_f32_arith.py runs; the share of flagged rows on those clouds."""
import itertools

import numpy as np
import pytest

import f32_model_cases as cases
import kmvp_f32_model as f1
import kmvp_oracle

PLAIN = [(path, kernel, sig, same) for path in ("fast", "cfast") for kernel in cases.KERNELS for sig in cases.SIGS
         for same in (False, True)]


@pytest.mark.parametrize("path,kernel,sig,same", PLAIN, ids=["-".join(map(str, p)) for p in PLAIN])
def test_model_without_rounding_is_the_float64_product(path, kernel, sig, same):
    rs = np.random.RandomState(len(kernel) + len(sig))
    D, M, N = (3, 53, 53 if same else 37) if path == "cfast" else (7, 70, 70 if same else 90)   # N > M: the rule wraps
    y = rs.rand(M, D) / np.sqrt(D)
    x = None if same else rs.rand(N, D) / np.sqrt(D)
    b = None if sig == "density" else rs.randn(M, 1) + 0.5
    got = f1.f32_product(kernel, y, x, b, sig == "norm", path=path, rounding=False)
    want = kmvp_oracle.product(kernel=kernel, source_points=y, target_points=x, source_signal=b, normalize_rows=sig == "norm")
    assert got.value.shape == want.shape == (N, 1)
    assert not got.band.any() and not got.flagged.any()
    assert np.abs(got.value - want).max() <= 1e-12 * np.abs(want).max()


def test_model_of_a_source_slice_follows_the_global_zero_rule():
    """Three slices with j_offset / M_total, N > M_total: their values add up to the whole's."""
    rs = np.random.RandomState(2)
    y, x, b = rs.rand(200, 3), rs.rand(450, 3), rs.randn(200, 1)
    for kernel in cases.KERNELS:
        whole = f1.f32_product(kernel, y, x, b, rounding=False).value
        parts = sum(f1.f32_product(kernel, y[lo:hi], x, b[lo:hi], j_offset=lo, M_total=200, rounding=False).value
                    for lo, hi in cases.SHARDS)
        assert np.abs(parts - whole).max() <= 1e-12 * np.abs(whole).max()


EMU_FAST = [(kernel, D, same) for kernel in cases.KERNELS for D, same in ((1, False), (3, True), (8, False), (24, True))]


@pytest.mark.parametrize("kernel,D,same", EMU_FAST, ids=[f"{k}-D{d}" for k, d, _ in EMU_FAST])
def test_emulated_fast_kernel_stays_inside_the_band(kernel, D, same):
    """Ragged M and N, several stages and folds (chunk = 32: one per stage), two segments."""
    rs = np.random.RandomState(11 + D)
    y, x, lab = cases.cloud(rs, kernel, D, 300, 45, same)
    c = cases.case("emu", kernel, "fast", y, x, cases.signal(rs, lab), chunk=32)
    worst = 0.0
    for sig in cases.SIGS:
        m = cases.model(c, sig, seg_len=160)
        got = cases.emulate_fast(kernel, y, x, c["b"], sig, chunk=32, segments=2)
        ok = ~m.flagged
        assert ok.mean() >= 0.95
        ratio = (np.abs(got - m.value) / m.band)[ok]
        assert (ratio <= 1).all(), (sig, float(ratio.max()))
        worst = max(worst, float(ratio.max()))
    assert worst > 1e-4  # the emulation's errors are not negligible against the band: the band is not vacuous


EMU_CFAST = [(kernel, D) for kernel in cases.KERNELS for D in (1, 4)]


@pytest.mark.parametrize("kernel,D", EMU_CFAST, ids=[f"{k}-D{d}" for k, d in EMU_CFAST])
def test_emulated_cfast_group_stays_inside_the_band(kernel, D):
    """One group of 101 sources (the fourth row tile ragged) on themselves: the diagonal and the closest pairs take the
    exact branch."""
    rs = np.random.RandomState(21 + D)
    y, _, lab = cases.cloud(rs, kernel, D, 101, 0, True)
    c = cases.case("emu", kernel, "cfast", y, None, cases.signal(rs, lab))
    for sig in cases.SIGS:
        m = cases.model(c, sig)
        got = cases.emulate_cfast_group(kernel, y, None, c["b"], sig)
        ok = ~m.flagged
        assert ok.mean() >= 0.95
        ratio = (np.abs(got - m.value) / m.band)[ok]
        assert (ratio <= 1).all(), (sig, float(ratio.max()))


def _clouds_for(defect):
    """The GPU test's clouds on which a defect can show."""
    if defect == "no-wrap":
        return [c for c in cases.zero_rule_cases() if c["name"][0] == "wrap"]
    if defect == "no-own-pair":
        return [c for c in itertools.chain(cases.zero_rule_cases(), cases.fast_grid_cases())
                if c["path"] == "fast" and c["kernel"] == "absolute-exponential" and c["x"] is None]
    return cases.fast_grid_cases()


@pytest.mark.parametrize("defect", cases.DEFECTS)
def test_a_defective_kernel_leaves_the_band(defect):
    """fast_kernel's emulation with one defect -- the x_l y_h and x_h y_l columns dropped, the m m column dropped, the lo
    piece of |y'|^2 dropped, one chain of eight sources of a tile left out, exp(-r)'s own-pair rule skipped, the zero rule
    without its wrap -- is outside the band on an unflagged element of a cloud the GPU test runs, where the emulation
    without the defect is inside on every one."""
    for c in _clouds_for(defect):
        m = cases.model(c, "product")
        ok = ~m.flagged & ~m.nonfinite
        good = cases.emulate_fast(c["kernel"], c["y"], c["x"], c["b"], "product")
        bad = cases.emulate_fast(c["kernel"], c["y"], c["x"], c["b"], "product", defect=defect)
        assert (np.abs(good - m.value) <= m.band)[ok].all(), c["name"]
        if (np.abs(bad - m.value) > m.band)[ok].any():
            return
    raise AssertionError(f"defect {defect} stays inside the band on every cloud")


def test_forced_absexp_clouds_beyond_four_dimensions_are_outside_the_radius_rule():
    """run_product sends exp(-r) with a signal at 4 < D <= 64 to fastmm_kernel when the scaled squared half-diagonal of
    the clouds' box is at most FAST_AUTO_RADIUS2 = 8: fast_kernel's instantiations there are reached on wider clouds."""
    n = 0
    for c in itertools.chain(cases.fast_grid_cases(), cases.stress_cases()):
        if c["kernel"] == "absolute-exponential" and c["y"].shape[1] > 4:
            pts = c["y"] if c["x"] is None else np.concatenate((c["y"], c["x"]))
            half = (pts.max(0).astype(np.float64) - pts.min(0)) / 2
            assert (half ** 2).sum() * f1.kernel_constant("absolute-exponential") ** 2 > 1.25 * 8.0, c["name"]
            n += 1
    assert n == 36


def test_flagged_rows_are_few_on_every_cloud_of_the_gpu_test():
    """At most 5 % of the rows of any cloud are flagged, in every signal mode, so no (kernel function, D) is left without
    unflagged rows; rows the model calls non-finite are the NaN target's and the coincident pair's only."""
    seen = set()
    for c in cases.all_cases():
        for sig in cases.SIGS:
            m = cases.model(c, sig)
            n = len(m.flagged)
            flagged = m.flagged & ~m.nonfinite
            assert flagged.sum() <= 0.05 * n, (c["name"], sig, int(flagged.sum()), n)
            with np.errstate(all="ignore"):
                want = kmvp_oracle.product(kernel=c["kernel"], source_points=c["y"], target_points=c["x"], normalize_rows=sig == "norm",
                                           source_signal=None if sig == "density" else c["b"])
            assert np.array_equal(m.nonfinite, ~np.isfinite(want).all(axis=1)), (c["name"], sig, np.nonzero(m.nonfinite)[0])
            if c["name"][0] in ("nonfinite", "rare"):
                want_bad = [5] if c["name"][0] == "nonfinite" else ([17, 200] if c["name"][-1] else [])
                assert list(np.nonzero(m.nonfinite)[0]) == want_bad, (c["name"], sig, np.nonzero(m.nonfinite)[0])
            assert np.isfinite(m.band[~m.flagged & ~m.nonfinite]).all(), (c["name"], sig)
        seen.add((c["path"], c["kernel"], c["y"].shape[1]))
    assert {("fast", k, D) for k in cases.KERNELS for D in range(1, 40)} <= seen
    assert {("cfast", k, D) for k in cases.KERNELS for D in (1, 4)} <= seen
