"""The bf16 matrix-core products (run_product_mfma: mfma_pipe_kernel / mfma_kernel) held to a float64 model of their own
arithmetic (oracle/kmvp_bf16_model.py) instead of the float64 product of the unrounded inputs.

Every element is checked as |got - model| <= band, band = K (amb + acc + floor) with K = 2 (the model's docstring
derives each term): amb sums |Delta P~| |b~| over the pairs whose kernel value may round to either bf16 neighbour, acc
bounds the fp32 accumulation (8 sqrt(n) 2^-24 mass, n = M sources: no segment is longer), floor the values under the
fp32 range.  Normalised rows carry the propagated numerator and denominator bands.  No band is fitted to what the
kernels produce; MAXIMA collects err / band and err / mass per kernel function for the record.

Clouds discriminate: clusters whose kernel values in a row span e^0 ... e^-6, signals of mixed sign with a nonzero mean
and per-cluster offsets (rows are not near the column mean).  1/r clouds keep a minimum pair separation far above the
cancellation range of the kernel's expanded S, so no row is flagged; exact duplicates are checked for the finite /
non-finite pattern only."""
import numpy as np
import pytest

import kmvp_bf16_model as bm
from kernel_matrix_benchmarks_amd import _lib

pytestmark = pytest.mark.gpu

DIST = ("gaussian", "absolute-exponential", "inverse-distance")
FUNCS = DIST + ("gaussian-shifted", "exp-dot")
PIPE_MAX_KS, PIPE_MAX_NT, MAX_KS, MAX_NT = 6, 2, 9, 4
VARIANTS = (0, 1, 4, 5)
MAXIMA = {}  # kernel function -> [max err / band, max err / mass]


def instantiated_grid():
    """(kernel function, device kernel, KS, NT, variant or TW) of every instantiation in kmvp_mfma_inst.hip."""
    grid = set()
    for fn in FUNCS:
        for ks in range(1, MAX_KS + 1):
            for nt in range(1, MAX_NT + 1):
                for tw in (1, 2):
                    grid.add((fn, "mfma_kernel", ks, nt, tw))
                if ks <= PIPE_MAX_KS and nt <= PIPE_MAX_NT:
                    for v in (VARIANTS if fn in DIST else (0,)):
                        grid.add((fn, "mfma_pipe_kernel", ks, nt, v))
    return grid


def d_range(fn, ks):
    """Both ends of the dimensions that take KS k-steps."""
    aug = {"exp-dot": 3, "gaussian-shifted": 9}.get(fn, 6)
    return sorted({max(1, 16 * (ks - 1) - aug + 1), 16 * ks - aug})


E_ENDS = (1, 32, 33, 64, 65, 96, 97, 128)


def clustered(rs, n, D, kernel, centres=None, k=6):
    """Clusters whose pair values within a row span about e^0 ... e^-6 under `kernel` (coordinates in caller's units)."""
    spread = {"gaussian": 3.0, "gaussian-shifted": 3.0, "absolute-exponential": 12.0, "inverse-distance": 3.0,
              "exp-dot": 1.5}[kernel]
    if centres is None:
        centres = rs.randn(k, D) * np.sqrt(spread / D)
    lab = rs.randint(len(centres), size=n)
    pts = centres[lab] + rs.randn(n, D) * (0.35 * np.sqrt(spread / D))
    return pts.astype(np.float32), lab, centres


def signal(rs, lab, E):
    off = rs.randn(lab.max() + 1, E) * 2.0
    return (rs.randn(len(lab), E) + 1.0 + off[lab]).astype(np.float32)


def check(fn, got, model, what, failures=None):
    """Every element within the model's band; rows the model calls non-finite (1/r duplicates, a normalised row whose
    only pair is the zero rule's: 0/0) non-finite here too; flagged finite rows are not held to a band.  With a list
    `failures`, a miss is appended to it instead of failing at once."""
    model_fin = np.isfinite(model.value).all(axis=1)
    msg = None
    if not np.array_equal(np.isfinite(got).all(axis=1)[~model_fin], np.zeros((~model_fin).sum(), bool)):
        msg = (what, "finite where the model's row is not")
    ok = ~model.flagged & model_fin
    if msg is None and not np.isfinite(got[ok]).all():
        msg = (what, "non-finite rows")
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
            msg = (what, f"err/band {ratio.max():.3g} at {i}: err {err[i]:.3g} band {band[i]:.3g} mass {model.mass[ok][i]:.3g} "
                         f"amb {model.amb[ok][i]:.3g} acc {model.acc[ok][i]:.3g}; {int((err > band).sum())} elements")
    if msg is not None:
        if failures is None:
            raise AssertionError(msg)
        failures.append(msg)


def run(ctx, kernel, norm, N, E):
    ctx.run("gaussian" if kernel == "gaussian-shifted" else kernel, norm)
    return ctx.get_result(N, E), ctx.last_kernel_name


def set_run_options(ctx, fn, option):
    """option: ("pipe", variant) or ("plain", TW)."""
    kind, v = option
    ctx.set_option("targets_per_lane", 0 if kind == "pipe" else v)
    if fn in DIST:
        ctx.set_option("mfma_variant", v if kind == "pipe" else 0)  # an explicit variant: the plain Gaussian for x != y
    else:
        ctx.set_option("mfma_variant", -1)


@pytest.fixture(scope="module", autouse=True)
def report():
    yield
    for fn, (eb, em) in sorted(MAXIMA.items()):
        print(f"\nbf16 model {fn:22s} max |err|/band {eb:.3g}  max |err|/mass {em:.3g}")


def test_every_instantiation_against_the_model():
    """Both ends of every k-step (D) and column-tile count (E), every mfma_variant of the pipelined kernel where it is
    instantiated, the plain kernel with one and two target tiles per wave; the set reached must equal the grid.  (The
    shifted Gaussian's targets 12 kernel lengths out found mfma_kernel reading its distances before the MFMA had written
    them: the wait states kmvp_mfma.hpp now forces ahead of mfma_tile_max.)"""
    reached, failures = set(), []
    N, M = 67, 101
    for fi, fn in enumerate(FUNCS):
        for ks in range(1, MAX_KS + 1):
            for D in d_range(fn, ks):
                assert bm.ksteps(fn, D) == ks
                rs = np.random.RandomState(1000 * fi + D)
                y, lab, cen = clustered(rs, M, D, fn)
                x, _, _ = clustered(rs, N, D, fn, cen)
                if fn == "gaussian-shifted":  # half the targets 12 kernel lengths out: 9+ from every source of the cloud
                    u = rs.randn(N, D)
                    far = (rs.rand(N) < 0.5)[:, None]
                    x = (x + far * 12.0 * u / np.linalg.norm(u, axis=1, keepdims=True)).astype(np.float32)
                ctx = _lib.Context(0)
                try:
                    ctx.set_points(y, x, _lib.KMVP_BF16)
                    for E in E_ENDS:
                        nt = (E + 31) // 32
                        b = signal(rs, lab, E)
                        ctx.set_signal(b)
                        opts = [("plain", 1), ("plain", 2)]
                        if ks <= PIPE_MAX_KS and nt <= PIPE_MAX_NT:
                            opts += [("pipe", v) for v in (VARIANTS if fn in DIST else (0,))]
                        models = {}
                        for oi, opt in enumerate(opts):
                            den_mfma = opt[0] == "pipe" and opt[1] & 1 == 1
                            norm = den_mfma or (D + E + oi) % 2 == 0
                            set_run_options(ctx, fn, opt)
                            got, kname = run(ctx, fn, norm, N, E)
                            if fn == "gaussian-shifted":
                                assert "online shift" in ctx.last_dispatch_note, ctx.last_dispatch_note
                            key = (norm, den_mfma)
                            if key not in models:
                                models[key] = bm.mfma_product(fn, y, x, b, norm, variant_den_mfma=den_mfma)
                            check(fn, got, models[key], (fn, D, E, opt, norm, kname), failures)
                            reached.add((fn, kname, bm.ksteps(fn, D), nt, opt[1]))
                finally:
                    ctx.close()
    assert not failures, (len(failures), failures[:8])
    assert reached == instantiated_grid(), sorted(instantiated_grid() ^ reached)


def _product(fn, y, x, b, norm, options=(), j_offset=0, M_total=None):
    ctx = _lib.Context(0)
    try:
        for k, v in options:
            ctx.set_option(k, v)
        ctx.set_points(y, x, _lib.KMVP_BF16, j_offset=j_offset, M_total=M_total)
        ctx.set_signal(b)
        got, kname = run(ctx, fn, norm, len(y) if x is None else len(x), 1 if b is None else b.shape[1])
    finally:
        ctx.close()
    return got, kname


@pytest.mark.parametrize("fn", DIST + ("gaussian-shifted",))
def test_ragged_shapes_segments_density_and_same_points(fn):
    """M in {1, 31, 33, 4097}, N in {1, 127, 129, 300}; forced segment counts 1, 3, 8 and one that leaves a one-tile last
    segment (M = 4321: 136 tiles, 16 segments of 9 tiles, the last one holding a single live source); same points, density
    estimation, normalised and plain rows."""
    rs = np.random.RandomState(17 + len(fn))
    D, E = 40, 3
    failures = []
    cases = [(M, N, False) for M in (1, 31, 33, 4097) for N in (1, 127, 129, 300)]
    if fn != "gaussian-shifted":
        cases += [(M, M, True) for M in (1, 31, 33, 4097)]
    for M, N, same in cases:
        y, lab, cen = clustered(rs, M, D, fn)
        x = None if same else clustered(rs, N, D, fn, cen)[0]
        rows = np.sort(rs.choice(N, 256, replace=False)) if N > 512 else np.arange(N)
        for segs in ((0, 1, 3, 8) if M == 4097 else (0,)):
            for density, norm in ((False, False), (False, True), (True, False)):  # density + norm: ones, no kernel
                b = None if density else signal(rs, lab, E)
                opts = [("segments", segs)] + ([("mfma_variant", 0)] if fn in DIST and not same else [])
                got, kname = _product(fn, y, x, b, norm, opts)
                model = bm.mfma_product(fn, y, x, b, norm, density=density, rows=rows)
                check(fn, got[rows], model, (fn, M, N, same, segs, density, norm, kname), failures)
    y, lab, cen = clustered(rs, 4321, D, fn)
    x = None if fn != "gaussian-shifted" else clustered(rs, 300, D, fn, cen)[0]
    for norm in (False, True):
        b = signal(rs, lab, E)
        got, kname = _product(fn, y, x, b, norm, [("segments", 16)])
        check(fn, got, bm.mfma_product(fn, y, x, b, norm), (fn, 4321, "one-tile last segment", norm, kname), failures)
    assert not failures, (len(failures), failures[:8])


def separated_cloud(rs, n, D, min_sep2=0.05):
    """Uniform points with every pair at squared distance >= min_sep2 (1/r stays far from its cancellation range)."""
    pts = (rs.rand(n, D) * 2.0).astype(np.float32)
    d2 = ((pts[:, None, :].astype(np.float64) - pts[None, :, :]) ** 2).sum(-1) if n <= 2000 else None
    if d2 is not None:
        np.fill_diagonal(d2, np.inf)
        assert d2.min() >= min_sep2
    return pts


def test_inverse_distance_zero_rule():
    """1/r: the diagonal of same points, the wrapped zero rule of N > M + 1, and a source shard (j_offset / M_total with
    partial_shard) -- each at every kernel of the path; exact duplicates keep the reference's non-finite rows."""
    rs = np.random.RandomState(5)
    D, E = 24, 2
    y = separated_cloud(rs, 150, D)
    x = separated_cloud(rs, 400, D)  # N = 400 > M + 1 = 151: rows 151.. wrap
    b = (rs.randn(150, E) + 1.0).astype(np.float32)
    for opts in ([], [("mfma_variant", 1)], [("mfma_variant", 5)], [("targets_per_lane", 1)], [("targets_per_lane", 2)]):
        for tgt in (None, x):
            for norm in (False, True):
                got, kname = _product("inverse-distance", y, tgt, b, norm, opts)
                model = bm.mfma_product("inverse-distance", y, tgt, b, norm,
                                        variant_den_mfma=dict(opts).get("mfma_variant", 0) & 1 == 1)
                assert not model.flagged.any()
                check("inverse-distance", got, model, ("zero rule", tgt is None, opts, norm, kname))
    # a shard of the sources [40, 110) of M_total = 150, raw partial sums
    lo, hi = 40, 110
    for tgt in (None, x):
        got, kname = _product("inverse-distance", y[lo:hi], y if tgt is None else tgt, b[lo:hi], False,
                              [("partial_shard", 1)], j_offset=lo, M_total=150)
        model = bm.mfma_product("inverse-distance", y[lo:hi], y if tgt is None else tgt, b[lo:hi], j_offset=lo, M_total=150)
        check("inverse-distance", got, model, ("shard", tgt is None, kname))
    # exact duplicates off the zero rule: non-finite rows where the model's are
    yd = y.copy()
    yd[7] = yd[3]
    got, _ = _product("inverse-distance", yd, None, b, False)
    model = bm.mfma_product("inverse-distance", yd, None, b)
    assert np.array_equal(~np.isfinite(got).all(axis=1), model.nonfinite), np.nonzero(model.nonfinite)


def test_dimension_limits():
    """D = 138 (9 k-steps) runs on the distance kernels; D = 139 is refused with the path's own UNSUPPORTED message."""
    rs = np.random.RandomState(9)
    for fn in DIST:
        y, lab, _ = clustered(rs, 64, 138, fn)
        b = signal(rs, lab, 2)
        got, kname = _product(fn, y, None, b, True)
        check(fn, got, bm.mfma_product(fn, y, None, b, True), (fn, 138, kname))
        y139 = np.ascontiguousarray(np.concatenate((y, y[:, :1]), axis=1))
        with pytest.raises(_lib.KmvpError) as exc:
            _product(fn, y139, None, b, True)
        assert "bf16 MFMA path is instantiated for D <= 138" in str(exc.value), str(exc.value)


def test_config3_attention_65536_rows_under_the_model():
    """The config-3 shape (N = M = 65536, D = 64, E = 64, row-normalised, same points) on a clustered cloud; 128 rows
    against the model, exp(-r) with its default variant (rotated pipeline) and the Gaussian."""
    n, D, E = 65536, 64, 64
    rs = np.random.RandomState(n + D + 2)
    centres = rs.randn(64, D) * (2.0 / np.sqrt(D))
    lab = np.repeat(np.arange(64), n // 64)
    y = (centres[lab] + rs.randn(n, D) * (0.25 / np.sqrt(D))).astype(np.float32)
    b = (rs.randn(n, E) + 1.0 + rs.randn(64, E)[lab] * 3.0).astype(np.float32)
    rows = np.random.RandomState(1).choice(n, size=128, replace=False)
    for fn in ("absolute-exponential", "gaussian"):
        got, kname = _product(fn, y, None, b, True)
        assert kname == "mfma_pipe_kernel"
        model = bm.mfma_product(fn, y, None, b, True, rows=rows)
        check(fn, got[rows], model, (fn, "config 3", kname))


def test_stateful_sweep_bf16_products_under_the_model():
    """tools/fuzz_stateful.py at a fixed seed: contexts living through random sequences of set_points / set_signal / fit /
    option changes / products of different kernel functions (the packed-layout cache: points_stale / signal_stale /
    record_packed).  Eight bfloat16 contexts, every product within the model's band, and four of random precision."""
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("fuzz_stateful", os.path.join(root, "tools", "fuzz_stateful.py"))
    fuzz = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fuzz)
    done, failures = fuzz.sweep(8, 30, 2024, precision="bfloat16", verbose=False)
    assert not failures, failures
    assert done >= 20, done
    done, failures = fuzz.sweep(4, 30, 2025, verbose=False)
    assert not failures, failures
