"""The float32 matrix-core products with several signal columns (fastmm_kernel, cfastmm_kernel) held element by element
to a float64 model of their arithmetic (oracle/kmvp_f32mm_model.py): |got - model| <= band, the band derived term by
term in the model's docstring, nothing fitted to kernel output.  MAXIMA collects err / band and err / mass per kernel
function for the record.

Clouds discriminate: clusters whose kernel values within a row span about e^0 ... e^-6, signals of mixed sign with a
nonzero mean and per-cluster offsets, column scales spanning decades (the per-column sigma_e of the signal split)."""
import numpy as np
import pytest

import kmvp_f32mm_model as fm
from kernel_matrix_benchmarks_amd import _lib

pytestmark = pytest.mark.gpu

FMM_MAX_KS, FMM_MAX_KS_TWO_TILES = 25, 4
MAXIMA = {}  # kernel function -> [max err / band, max err / mass]


def fastmm_grid():
    """(function, device kernel, KS, MODE, TT) of every instantiation in kmvp_fastmm_inst.hip that the dispatch reaches:
    the Gaussian with and without the online shift, exp(-r) beyond the centred forms' D = 4 (KS >= 3), and exp(<x,y>) on
    the Gaussian build (online only)."""
    grid = set()
    for fn, ks0 in (("gaussian", 1), ("gaussian-online", 1), ("absexp", 3), ("absexp-online", 3), ("exp-dot", 1)):
        for ks in range(ks0, FMM_MAX_KS + 1):
            for mode in (0, 1):
                for tt in ((1, 2) if ks <= FMM_MAX_KS_TWO_TILES else (1,)):
                    grid.add((fn, "fastmm_kernel", ks, mode, tt))
    return grid


def cfastmm_grid():
    """kmvp_cfastmm_inst.hip: Gaussian and exp(-r) with and without the online shift, 1/r online only; MODE x TT."""
    return {(fn, "cfastmm_kernel", 0, mode, tt) for fn in ("gaussian", "gaussian-online", "absexp", "absexp-online",
                                                             "inverse-distance-online")
            for mode in (0, 1) for tt in (1, 2)}


def clustered(rs, n, D, spread, centres=None, k=6):
    if centres is None:
        centres = rs.randn(k, D) * np.sqrt(spread / D)
    lab = rs.randint(len(centres), size=n)
    pts = centres[lab] + rs.randn(n, D) * (0.35 * np.sqrt(spread / D))
    return pts.astype(np.float32), lab, centres


def signal(rs, lab, E):
    """Mixed signs, nonzero mean, per-cluster offsets, column scales spanning decades -- and every entry 0.45 f16 units
    above an 11-bit value, so that the low f16 half b_l of b sigma_e is never negligible and always of one sign: a kernel
    that lost b_l would be off by ~2^-12 of the row's mass, not by a random walk of it."""
    off = rs.randn(lab.max() + 1, E) * 2.0
    colscale = 10.0 ** rs.uniform(-3, 3, size=E)  # column scales spanning decades
    b = (rs.randn(len(lab), E) + 1.0 + off[lab]) * colscale
    m, e = np.frexp(b)
    return np.ldexp(np.round(m * 2048.0) / 2048.0 + 0.45 / 2048.0, e).astype(np.float32)


def check(fn, got, model, what, failures=None):
    """Rows the model calls non-finite are non-finite here too; every other unflagged element within the band."""
    msg = None
    bad = model.nonfinite
    if not (~np.isfinite(got[bad]).all(axis=1) if bad.any() else np.ones(0, bool)).all():
        msg = (what, "finite where the model's row is not")
    ok = ~model.flagged & ~bad
    if msg is None and not np.isfinite(got[ok]).all():
        msg = (what, f"non-finite rows {np.nonzero(~np.isfinite(got[ok]).all(axis=1))[0][:8]}")
    if msg is None and ok.any():
        err = np.abs(got[ok] - model.value[ok])
        band = model.band[ok]
        r = MAXIMA.setdefault(fn, [0.0, 0.0])
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(band > 0, err / band, np.where(err > 0, np.inf, 0.0))
            r[0] = max(r[0], float(ratio.max()))
            r[1] = max(r[1], float(np.where(model.mass[ok] > 0, err / model.mass[ok], 0.0).max()))
        if (err > band).any():
            i = np.unravel_index(np.argmax(ratio), ratio.shape)
            msg = (what, f"err/band {ratio.max():.3g} at {i}: err {err[i]:.3g} band {band[i]:.3g} mass {model.mass[ok][i]:.3g}; "
                         f"{int((err > band).sum())} elements")
    if msg is not None:
        if failures is None:
            raise AssertionError(msg)
        failures.append(msg)


def product(kernel, y, x, b, norm, options=()):
    """One product in a fresh float32 context: (result, device kernel, dispatch note)."""
    ctx = _lib.Context(0)
    try:
        for k, v in options:
            ctx.set_option(k, v)
        ctx.set_points(np.ascontiguousarray(y, dtype=np.float32), None if x is None else np.ascontiguousarray(x, dtype=np.float32),
                       _lib.KMVP_F32)
        ctx.set_signal(np.ascontiguousarray(b, dtype=np.float32))
        ctx.run(kernel, norm)
        return ctx.get_result(len(y) if x is None else len(x), b.shape[1]), ctx.last_kernel_name, ctx.last_dispatch_note
    finally:
        ctx.close()


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for fn, (eb, em) in sorted(MAXIMA.items()):
        print(f"\nf32mm model {fn:24s} max |err|/band {eb:.3g}  max |err|/mass {em:.3g}")


SPREAD = {"gaussian": 2.0, "absolute-exponential": 0.5, "exp-dot": 1.5}


def test_every_fastmm_instantiation_against_the_model():
    """Both ends of D for every KS, E across the column blocks (1 / 16 / 17 / 33: MODE 0, MODE 1, two blocks with the
    denominator column), one and two target tiles per wave; the reached set equals the grid."""
    reached, failures = set(), []
    N, M = 67, 101
    for fn, kernel, same in (("gaussian", "gaussian", True), ("gaussian-online", "gaussian", False),
                             ("absexp", "absolute-exponential", True), ("absexp-online", "absolute-exponential", False),
                             ("exp-dot", "exp-dot", False)):
        for ks in range(1, FMM_MAX_KS + 1):
            lo = 5 if kernel == "absolute-exponential" else 1
            ds = [d for d in range(lo, 65) if fm.fmm_ksteps(d) == ks]
            if not ds:
                continue
            for D in sorted({ds[0], ds[-1]}):
                rs = np.random.RandomState(100 * ks + D + len(fn))
                y, lab, cen = clustered(rs, M, D, SPREAD[kernel])
                x = None if same else clustered(rs, N, D, SPREAD[kernel], cen)[0]
                for E in (1, 16, 17, 33) if kernel != "gaussian" else (2, 16, 17, 33):
                    b = signal(rs, lab, E)
                    norm = (D + E) % 2 == 0 if E not in (16, 17) else E == 16  # NE 17: MODE 1 from the denominator
                    NE = E + (1 if norm else 0)
                    mode = 1 if NE > 16 else 0
                    model = fm.f32mm_product(kernel, y, x, b, norm, online=not same or kernel == "exp-dot")
                    for tt in ((1, 2) if ks <= FMM_MAX_KS_TWO_TILES else (1,)):
                        opts = [("fast_tiles", tt)] + ([] if kernel == "exp-dot" else [("fast_sqdists", 1)])
                        got, kname, note = product(kernel, y, x, b, norm, opts)
                        if fn != "gaussian" and fn != "absexp":
                            assert "online shift" in note, (fn, D, E, kname, note)
                        check(fn, got, model, (fn, D, E, norm, tt, kname), failures)
                        reached.add((fn, kname, fm.fmm_ksteps(D), mode, tt))
    assert not failures, (len(failures), failures[:8])
    assert reached == fastmm_grid(), sorted(fastmm_grid() ^ reached)[:20]


def test_every_cfastmm_instantiation_against_the_model():
    reached, failures = set(), []
    N, M = 130, 301
    for fn, kernel, same in (("gaussian", "gaussian", True), ("gaussian-online", "gaussian", False),
                             ("absexp", "absolute-exponential", True), ("absexp-online", "absolute-exponential", False),
                             ("inverse-distance-online", "inverse-distance", True)):
        for D in (1, 4):
            rs = np.random.RandomState(7 * D + len(fn))
            if kernel == "inverse-distance":
                y = (rs.rand(M, D) * 2.0).astype(np.float32)
                lab = rs.randint(6, size=M)
                x = None
            else:
                y, lab, cen = clustered(rs, M, D, SPREAD[kernel])
                x = None if same else clustered(rs, N, D, SPREAD[kernel], cen)[0]
            for E in (2, 16, 17, 33):
                b = signal(rs, lab, E)
                norm = E == 16 or (E == 33 and D == 4)
                mode = 1 if E + (1 if norm else 0) > 16 else 0
                model = fm.f32mm_product(kernel, y, x, b, norm, path="cfastmm", online=not same or kernel == "inverse-distance")
                for tt in (1, 2):
                    got, kname, note = product(kernel, y, x, b, norm, [("fast_tiles", tt), ("fast_sqdists", 2)])
                    if fn.endswith("online"):
                        assert "online shift" in note, (fn, D, E, kname, note)
                    check(fn + "-cf", got, model, (fn, D, E, norm, tt, kname), failures)
                    reached.add((fn, kname, 0, mode, tt))
    assert not failures, (len(failures), failures[:8])
    assert reached == cfastmm_grid(), sorted(cfastmm_grid() ^ reached)


def test_online_shift_under_stress():
    """Sources ordered so that each target's largest values arrive last (the shift moves with sums under way), forced
    segment counts 1 / 2 / 3 / 17 with chunk = 8 (many folds), targets far from every source (Gaussian on fastmm_kernel:
    e^-2 ... e^-80; exp(-r) on cfastmm_kernel: e^-1 ... e^-55), exp(<x,y>) logits of several hundred either sign.  (The
    hysteresis itself: test_hysteresis_both_sides.)"""
    rs = np.random.RandomState(31)
    failures = []
    D, M, N, E = 3, 3000, 200, 8
    y = (rs.rand(M, D) * 0.6).astype(np.float32)
    for kernel in ("gaussian", "absolute-exponential", "exp-dot"):
        if kernel == "exp-dot":
            yy = (rs.randn(M, 6) * 4.0).astype(np.float32)
            x = (rs.randn(N, 6) * 4.0).astype(np.float32)   # logits of several hundred, either sign
        else:
            # Gaussian: targets e^-2 ... e^-80 from the cloud (fastmm_kernel, forced); exp(-r): e^-1 ... e^-55 (cfastmm_kernel)
            offs = np.repeat([1.6, 4.2, 6.5, 9.0], N // 4) if kernel == "gaussian" else np.repeat([0.5, 12.0, 35.0, 55.0], N // 4)
            x = (rs.rand(N, D) * 0.6).astype(np.float32)
            x[:, 0] += offs.astype(np.float32)
            yy = y
        # far sources first, the closest last: every target's row maximum arrives late in each segment
        key = yy @ x.mean(0) if kernel == "exp-dot" else -np.linalg.norm(yy - x.mean(0), axis=1)
        ys = np.ascontiguousarray(yy[np.argsort(key)])
        b = signal(rs, rs.randint(6, size=M), E)
        for segs in (1, 2, 3, 17):
            for norm in (False, True):
                force = {"gaussian": [("fast_sqdists", 1)], "absolute-exponential": [("fast_sqdists", 2)], "exp-dot": []}
                opts = [("segments", segs), ("chunk", 8)] + force[kernel]
                got, kname, note = product(kernel, ys, x, b, norm, opts)
                # (exp(-r) at D = 3 and targets 12 ... 55 away: cfastmm_kernel, the form outside the radius rule)
                assert kname in ("fastmm_kernel", "cfastmm_kernel") and "online shift" in note, (kernel, kname, note)
                path = "fastmm" if kname == "fastmm_kernel" else "cfastmm"
                model = fm.f32mm_product(kernel, ys, x, b, norm, path=path, chunk=8, seg_len=-(-M // segs))
                check(kernel, got, model, ("stress", kernel, segs, norm), failures)
    assert not failures, (len(failures), failures[:8])


def test_hysteresis_both_sides():
    """Per target a seed source in the first tile sets the shift to kop = a + 1 (exponent a + 1.01); a closer source in the
    second tile has exponent a + 1 - f, f in {0.3, 0.45, 0.55, 0.7, 1.2, 1.45}: with the half binade of hysteresis the
    first two keep kop (T = 2^(15 + f) < 2^15.5), the others move it; f = 1.2 / 1.45 would overflow f16 (T >= 2^16)
    under a hysteresis of 1.5."""
    rs = np.random.RandomState(3)
    N, a = 32, 3.0
    f = np.array([0.3, 0.45, 0.55, 0.7, 1.2, 1.45] * 6)[:N]
    x = np.zeros((N, 2))
    x[:, 0] = np.arange(N) * 6.0
    seed = x + np.c_[np.sqrt((a + 1.01) / fm.LOG2E) * np.ones(N), np.zeros(N)]
    close = x + np.c_[np.zeros(N), np.sqrt((a + 1 - f) / fm.LOG2E)]
    y = np.concatenate((seed, close)).astype(np.float32)  # sources 0..31: the first tile; 32..63: the second
    x = x.astype(np.float32)
    b = signal(rs, rs.randint(3, size=len(y)), 3)
    failures = []
    for norm in (False, True):
        got, kname, note = product("gaussian", y, x, b, norm, [("fast_sqdists", 1), ("segments", 1)])
        assert kname == "fastmm_kernel" and "online shift" in note, (kname, note)
        check("gaussian", got, fm.f32mm_product("gaussian", y, x, b, norm), ("hysteresis", norm), failures)
    assert not failures, failures


def test_exp_dot_range_of_the_shift():
    """The per-target exponent is clamped at 32000 binades: logits of 2.5e4 (beyond 32000 ln 2 ~ 2.2e4) fail with an error
    on both native paths (float32 fastmm_kernel, bfloat16 mfma kernels), plain and row-normalised, instead of returning
    inf / NaN rows; 2.0e4 still runs, with the row-normalised result inside the model's band."""
    rs = np.random.RandomState(8)
    D, M, N = 4, 200, 40
    y = (rs.randn(M, D) * 0.1).astype(np.float32)
    x = (rs.randn(N, D) * 0.1).astype(np.float32)
    b = signal(rs, rs.randint(4, size=M), 3)
    for logit in (2.5e4, 2.0e4):
        yy, xx = y.copy(), x.copy()
        yy[17, 0], xx[5, 0] = 160.0, logit / 160.0
        for dt in (_lib.KMVP_F32, _lib.KMVP_BF16):
            for norm in (False, True):
                if logit < 2.2e4 and (dt == _lib.KMVP_BF16 or not norm):
                    continue  # (inside the range: the plain row overflows float64, as numpy's would; bf16 has its own model)
                ctx = _lib.Context(0)
                try:
                    ctx.set_points(yy, xx, dt)
                    ctx.set_signal(b)
                    if logit > 2.2e4:
                        with pytest.raises(_lib.KmvpError, match="2.2e4"):
                            ctx.run("exp-dot", norm)
                    else:
                        ctx.run("exp-dot", norm)
                        got = ctx.get_result(N, 3)
                        check("exp-dot", got, fm.f32mm_product("exp-dot", yy, xx, b, norm), ("range 2e4", norm))
                finally:
                    ctx.close()


def test_edges_ragged_same_points_and_non_finite():
    """N and M of 1 and not multiples of 32; targets == sources (ONLINE = 0); a NaN target coordinate: that row is NaN --
    float32 exp(<x,y>) included, plain and normalised -- and every other row inside the band; a source at +-inf
    contributes 0 (cfastmm_kernel)."""
    rs = np.random.RandomState(5)
    failures = []
    for kernel, path, D in (("gaussian", "fastmm", 3), ("absolute-exponential", "fastmm", 6), ("exp-dot", "fastmm", 5),
                            ("gaussian", "cfastmm", 3), ("absolute-exponential", "cfastmm", 2)):
        opts = [("fast_sqdists", 1 if path == "fastmm" else 2)] if kernel != "exp-dot" else []
        sp = SPREAD[kernel]
        for M, N in ((1, 1), (1, 33), (33, 1), (31, 65), (97, 129)):
            y, lab, cen = clustered(rs, M, D, sp)
            x = clustered(rs, N, D, sp, cen)[0]
            b = signal(rs, lab, 5)
            for norm in (False, True):
                got, kname, _ = product(kernel, y, x, b, norm, opts)
                check(kernel, got, fm.f32mm_product(kernel, y, x, b, norm, path=path), ("ragged", kernel, path, M, N, norm, kname),
                      failures)
        # targets == sources (ONLINE = 0 except exp-dot)
        y, lab, _ = clustered(rs, 200, D, sp)
        b = signal(rs, lab, 17)
        for norm in (False, True):
            got, kname, _ = product(kernel, y, None, b, norm, opts)
            check(kernel, got, fm.f32mm_product(kernel, y, None, b, norm, path=path), ("same", kernel, path, norm, kname), failures)
        # a NaN target coordinate, a source at +-inf
        y, lab, cen = clustered(rs, 300, D, sp)
        x = clustered(rs, 64, D, sp, cen)[0]
        x[5, D - 1] = np.nan
        if path == "cfastmm":  # (sources at +-inf: the centred forms; exp(<x, inf>) is not 0)
            y[7, 0], y[11, 0] = np.inf, -np.inf
        b = signal(rs, lab, 3)
        for norm in (False, True):
            got, kname, _ = product(kernel, y, x, b, norm, opts)
            assert np.isnan(got[5]).all(), (kernel, path, norm, kname, got[5])
            ok = np.arange(64) != 5
            model = fm.f32mm_product(kernel, y, x[ok], b, norm, path=path)
            check(kernel, got[ok], model, ("non-finite", kernel, path, norm, kname), failures)
    assert not failures, (len(failures), failures[:8])


def test_inverse_distance_zero_rule():
    """1/r on cfastmm_kernel: targets == sources, the pair with the target's own index dropped."""
    rs = np.random.RandomState(9)
    y = (rs.rand(500, 3) * 2.0).astype(np.float32)
    b = signal(rs, rs.randint(4, size=500), 20)
    for norm in (False, True):
        got, kname, note = product("inverse-distance", y, None, b, norm, [("fast_sqdists", 2)])
        assert kname == "cfastmm_kernel", kname
        model = fm.f32mm_product("inverse-distance", y, None, b, norm, path="cfastmm")
        assert not model.flagged.any()
        check("inverse-distance", got, model, ("zero rule", norm))


def test_large_cloud_row_subset():
    """N = M = 1e5, D = 3, E = 16 (low-D attention), targets != sources: 512 rows against the model."""
    rs = np.random.RandomState(12)
    n = 100000
    y = (rs.rand(n, 3) * 1.5).astype(np.float32)
    x = (rs.rand(n, 3) * 1.5).astype(np.float32)
    b = signal(rs, rs.randint(8, size=n), 16)
    rows = np.sort(rs.choice(n, 512, replace=False))
    for norm in (False, True):
        got, kname, note = product("gaussian", y, x, b, norm, [("fast_sqdists", 1)])
        assert kname == "fastmm_kernel" and "online shift" in note
        check("gaussian", got[rows], fm.f32mm_product("gaussian", y, x, b, norm, rows=rows), ("1e5", norm))
