"""Clouds, configurations and numpy emulations shared by tests/test_lse_model.py (CPU) and tests/test_gpu_lse_arith.py
(GPU): the GPU test runs lowd_lse_kernel and lowd_lse_grad_kernel on exactly the clouds on which the CPU test keeps the
clean emulations of their steps inside the model's band (oracle/kmvp_lse_model.py) and shows that an emulation with one
defect leaves it.

What the cases vary is what these kernels add to the pair loops: log-weight columns that differ in scale and sign, every
batch of 4, pad of 8, LDS tile and fold boundary, and the online shift placed on its edges -- a rise in most batches and
in none, right after a fold, beyond the clamp of the rescale, on one lane of a wave, on one column of four, inside the
gradient's guarded records --, large logits, dead terms, duplicated points, non-finite inputs.

A configuration is (which, sig, E, chunk, segments): which = "lse" / "grad", sig = "product" (the signal read as
log-weights) / "density" (c = 0), segments = 0 for the library's own choice."""
import itertools

import numpy as np

import kmvp_lse_model as sm
import kmvp_lowd_model as lm
import lowd_model_cases as cases
from lowd_model_cases import _fma, f32, f64

KERNELS = sm.KERNELS
PRECISIONS = (np.float32, np.float64)
NAME = {"lse": "lowd_lse_kernel", "grad": "lowd_lse_grad_kernel"}
WHICH = ("lse", "grad")
COLUMN_SCALES = np.array([1.0, -3.0, 0.25, 7.0])             # log-weight columns distinct in scale and sign
MODES = [("product", e) for e in (1, 2, 3, 4)] + [("density", 1)]
N_EDGES = (1, 63, 64, 65, 257)
M_EDGES = (1, 3, 4, 5, 8, 9, 255, 256, 257, 513, 1030)
SEGMENTS = cases.SEGMENTS
SHARDS = cases.SHARDS
U, GUARD_RECORDS = 4, 8                                       # sources per batch; the gradient's guard zone: the last 2 U records
SHIFT_SEGMENTS = (1, 3)
CLAMP_DROP = {np.dtype(np.float32): 250.0, np.dtype(np.float64): 3000.0}   # in c: 360 > 300 and 4328 > 4000 binades


def logweights(rs, M, E, precision):
    return (cases.signal(rs, M, E, np.float64) * COLUMN_SCALES[:E]).astype(precision)


def case(name, kernel, precision, y, x, b, **kw):
    return dict(name=name, kernel=kernel, precision=np.dtype(precision), y=y, x=x, b=b, kw=kw)


def signal_of(c, sig, E=None):
    return None if sig == "density" else np.ascontiguousarray(c["b"][:, :E])


def model(c, cfg, **more):
    which, sig, E, chunk, _ = cfg
    fn = sm.lse_gradient if which == "grad" else sm.lse
    kw = {k: v for k, v in c["kw"].items() if k in ("j_offset", "M_total", "feed")}
    return fn(c["kernel"], c["y"], c["x"], signal_of(c, sig, E), precision=c["precision"], chunk=chunk, **dict(kw, **more))


def loose(c, which):
    """Whether an element the model does not call poisoned may be non-finite too: a non-finite source coordinate -- but
    for L an infinite one, whose pairs contribute exactly 0 by include/kmvp.h."""
    tag = c["kw"].get("bad_source")
    return tag is not None and not (which == "lse" and tag != "nan")


def grid_cases(kernel, precision):
    """D = 1 ... 8 on N = 67 targets x M = 101 sources (ragged in both), four log-weight columns; the same points at D = 3."""
    for D in range(1, cases.LOWD_MAX_D + 1):
        rs = np.random.RandomState(cases.seed("lse-grid", kernel, D))
        y = cases.points(rs, 101, D, precision)
        yield case(("grid", kernel, D), kernel, precision, y, cases.points(rs, 67, D, precision), logweights(rs, 101, 4, precision))
        if D == 3:
            yield case(("grid-same", kernel, D), kernel, precision, y, None, logweights(rs, 101, 4, precision))


def size_cases(kernel, precision):
    """Every M of M_EDGES (batches of 4, the pad of 8, LDS tiles of 256, folds) with the N of N_EDGES in turn; D = 3."""
    for M, N in zip(M_EDGES, itertools.cycle(N_EDGES)):
        rs = np.random.RandomState(cases.seed("lse-size", kernel, N, M))
        yield case(("size", kernel, N, M), kernel, precision, cases.points(rs, M, 3, precision), cases.points(rs, N, 3, precision),
                   logweights(rs, M, 2, precision))


def segment_cases(kernel, precision):
    rs = np.random.RandomState(cases.seed("lse-seg", kernel))
    yield case(("segments", kernel, 1030), kernel, precision, cases.points(rs, 1030, 3, precision), cases.points(rs, 65, 3, precision),
               logweights(rs, 1030, 2, precision))


def _far_ring(rs, M, radius):
    """M points at `radius` from the origin (D = 3), in float64."""
    v = rs.randn(M, 3)
    return v / np.linalg.norm(v, axis=1, keepdims=True) * radius * (1.0 + 0.05 * rs.rand(M, 1))


def shift_cases(kernel, precision):
    """The online shift on its edges: D = 3, chunk = 256, 1 and 3 segments.  M = 1100: m_pad = 1104, three segments of 368
    begin at 0, 368, 736; the fp32 sums fold 256 sources into a segment: at 256, 512, 768, 1024 (one segment) and at 256,
    624, 992 (three)."""
    tag = lambda t: ("shift", kernel, t)
    far = 3.0 if kernel == "gaussian" else 9.0                 # logits of about -9 against about -0.1 of a near source
    # a rise in most batches: the sources come nearer and nearer to the (tight) targets; and none after the first batch
    rs = np.random.RandomState(cases.seed("lse-shift-order", kernel))
    x = (rs.randn(67, 3) * 0.05)
    y = _far_ring(rs, 700, 1.0) * np.linspace(far, 0.2, 700)[:, None]
    b = logweights(rs, 700, 2, precision)
    yield case(tag("nearest-last"), kernel, precision, y.astype(precision), x.astype(precision), b)
    yield case(tag("nearest-first"), kernel, precision, y[::-1].astype(precision), x.astype(precision), b[::-1].copy())
    # one near source in the first batch after a fold, the fp64 sum non-zero when the rise comes; nearer ones at the
    # three-segment launch's folds
    rs = np.random.RandomState(cases.seed("lse-shift-fold", kernel))
    y = _far_ring(rs, 1100, far)
    for j, r in ((256, 1.0), (624, 0.5), (992, 0.1)):
        y[j] = y[j] / np.linalg.norm(y[j]) * r
    b = logweights(rs, 1100, 2, precision)
    yield case(tag("after-fold"), kernel, precision, y.astype(precision), x.astype(precision), b)
    # the same with the rise beyond the clamp of the rescale: every other source's log-weight CLAMP_DROP lower, in column 0
    drop = CLAMP_DROP[np.dtype(precision)]
    bc = b.copy()
    bc[:, 0] -= drop
    bc[[256, 624, 992], 0] += drop
    yield case(tag("beyond-clamp"), kernel, precision, y.astype(precision), x.astype(precision), bc.astype(precision), no_density=True)
    # a rise on one lane of a wave only: 64 targets, the late source (j = 256) sits on target 17 and far from the others
    rs = np.random.RandomState(cases.seed("lse-shift-lane", kernel))
    x1 = rs.randn(64, 3) * 0.05
    y1 = rs.randn(600, 3) * 0.3
    x1[17] = (far, 0.0, 0.0)
    y1[256] = (far, 0.01, 0.0)
    yield case(tag("one-lane"), kernel, precision, y1.astype(precision), x1.astype(precision), logweights(rs, 600, 2, precision))
    # a rise on one column of four only: a late source (j = 256) with a log-weight of +30 in column 2
    b4 = logweights(rs, 600, 4, precision)
    b4[256, 2] = 30.0
    yield case(tag("one-column"), kernel, precision, (rs.randn(600, 3) * 0.5).astype(precision), x.astype(precision), b4, no_density=True)
    # a rise inside the guarded last 8 records: M = 301, m_pad = 304, the nearest source at j = 299, pads from 301 on
    rs = np.random.RandomState(cases.seed("lse-shift-guard", kernel))
    y2 = _far_ring(rs, 301, far)
    y2[299] = (0.1, 0.0, 0.0)
    yield case(tag("in-guard"), kernel, precision, y2.astype(precision), x.astype(precision), logweights(rs, 301, 2, precision))
    # three segments, the first without a live term in column 0
    b5 = logweights(rs, 1100, 2, precision)
    b5[:400, 0] = -np.inf
    yield case(tag("dead-first-segment"), kernel, precision, _far_ring(rs, 1100, 1.0).astype(precision), x.astype(precision), b5,
               no_density=True)


LARGE_LOGIT = {np.dtype(np.float32): 1.0e4, np.dtype(np.float64): 1.0e6}


def range_cases(kernel, precision):
    """Logits near -1e4 (float32) / -1e6 (float64) with c spanning +-1e3; dead terms; no source; targets at 1e20; duplicated
    points."""
    tag = lambda t: ("range", kernel, t)
    dt = np.dtype(precision)
    rs = np.random.RandomState(cases.seed("lse-range", kernel))
    y, x = cases.points(rs, 101, 3, np.float64), cases.points(rs, 67, 3, np.float64)
    b = logweights(rs, 101, 2, np.float64)
    b[:, 1] = np.linspace(-1.0e3, 1.0e3, 101)[rs.permutation(101)]
    xl = x.copy()
    xl[:, 0] += cases.exponent_to_distance(kernel, LARGE_LOGIT[dt])
    yield case(tag("large-logits"), kernel, precision, y.astype(precision), xl.astype(precision), b.astype(precision))
    b3 = logweights(rs, 101, 3, np.float64)
    b3[::3, 0] = -np.inf
    b3[:, 1] = -np.inf
    b3[:, 2] = np.linspace(-1.0e3, 1.0e3, 101)[rs.permutation(101)]
    yield case(tag("dead-terms"), kernel, precision, y.astype(precision), x.astype(precision), b3.astype(precision), no_density=True)
    yield case(tag("all-dead"), kernel, precision, y.astype(precision), x.astype(precision), np.full((101, 2), -np.inf, precision),
               no_density=True)
    yield case(tag("no-source"), kernel, precision, y[:0].astype(precision), x.astype(precision), b[:0].astype(precision))
    x20 = x.copy()
    x20[:, 1] += 1.0e20
    yield case(tag("targets-at-1e20"), kernel, precision, y.astype(precision), x20.astype(precision), b.astype(precision))
    yd = y.astype(precision)
    yd[90], yd[33] = yd[17], yd[2]
    yield case(tag("duplicates"), kernel, precision, yd, None, b.astype(precision))


SOURCE_POSITIONS = (0, 50, 98)                                # M = 101: the first, the middle, the guard zone (96 ... 103)


def nonfinite_cases(kernel, precision):
    """A NaN target (row 5) at M = 5, 8, 101; a NaN and a +inf log-weight in column 1 of two; a NaN, +inf and -inf source
    coordinate (axis 1 of 3) at each of SOURCE_POSITIONS."""
    for M in (5, 8, 101):
        rs = np.random.RandomState(cases.seed("lse-nan-target", kernel, M))
        y, x = cases.points(rs, M, 3, precision), cases.points(rs, 67, 3, precision)
        x[5, 2] = np.nan
        yield case(("nan-target", kernel, M), kernel, precision, y, x, logweights(rs, M, 2, precision), bad_rows=[5])
    rs = np.random.RandomState(cases.seed("lse-bad-source", kernel))
    y, x, b = cases.points(rs, 101, 3, precision), cases.points(rs, 67, 3, precision), logweights(rs, 101, 2, precision)
    for tag, v in (("nan", np.nan), ("+inf", np.inf)):
        bb = b.copy()
        bb[40, 1] = v
        yield case(("bad-logweight", kernel, tag), kernel, precision, y, x, bb, no_density=True)
    for tag, v in (("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf)):
        for j in SOURCE_POSITIONS:
            yb = y.copy()
            yb[j, 1] = v
            yield case(("bad-source", kernel, tag, j), kernel, precision, yb, x, b, bad_source=tag)


def shard_cases(kernel, precision):
    rs = np.random.RandomState(cases.seed("lse-shards", kernel))
    yield case(("shards", kernel, 200), kernel, precision, cases.points(rs, 200, 3, precision), cases.points(rs, 67, 3, precision),
               logweights(rs, 200, 2, precision))


def configs(c):
    """What the GPU test runs on a case."""
    group = c["name"][0]
    E_all = c["b"].shape[1]
    modes = [("product", E_all)] + ([] if c["kw"].get("no_density") else [("density", 1)])
    for which in WHICH:
        if group in ("grid", "grid-same"):
            for sig, E in MODES:
                for chunk in (8, 512):
                    yield which, sig, E, chunk, 0
        elif group == "size":
            for sig, E in modes:
                for chunk in (8, 256, 512):
                    yield which, sig, E, chunk, 0
        elif group == "segments":
            for segments in SEGMENTS:
                for chunk in (8, 512):
                    yield which, "product", 2, chunk, segments
        elif group == "shift":
            for sig, E in modes:
                for segments in SHIFT_SEGMENTS:
                    yield which, sig, E, 256, segments
        else:
            for sig, E in modes:
                yield which, sig, E, 512, 0


def groups(kernel, precision):
    return {"grid": list(grid_cases(kernel, precision)),
            "edges": [c for gen in (size_cases, segment_cases) for c in gen(kernel, precision)],
            "shift": list(shift_cases(kernel, precision)),
            "range": list(range_cases(kernel, precision)),
            "nonfinite": list(nonfinite_cases(kernel, precision))}


def golden_cases():
    """One small cloud per kernel function and precision (N = 24 x M = 37, D = 3, E = 2) whose results, recorded from the
    library BEFORE lse_exp2_neg and the gradient's guard were changed, are in tests/golden/lse_parent.npz."""
    for kernel in KERNELS:
        for precision in PRECISIONS:
            rs = np.random.RandomState(cases.seed("lse-golden", kernel))
            yield case(("golden", kernel, 37), kernel, precision, cases.points(rs, 37, 3, precision), cases.points(rs, 24, 3, precision),
                       logweights(rs, 37, 2, precision))


def golden_key(c, which):
    return f"{which}|{c['kernel']}|{c['precision'].name}"


# ---- numpy emulation of the kernels' own steps -------------------------------------------------------------------------

DEFECTS = ("rise-skips-fp64", "rise-skips-V", "merge-first-exponent", "drop-ragged", "no-newton", "no-guard", "no-s0-select",
           "nan-weight-dropped", "guard-s-lt-inf")           # the last two: what the kernels did before this model was written
LN2 = 0.6931471805599453


def _defects(defect):
    return () if defect is None else (defect,) if isinstance(defect, str) else tuple(defect)


def _exp2_neg(a, keep_nan=True):
    """lse_exp2_neg: v_exp_f32 of -a; kexp_neg_f64(a ln 2), a NaN passed on by the select (without it: the clamp's 0)."""
    if a.dtype == f32:
        return cases._exp2f(-a)
    w = cases._kexp_neg_f64(a * LN2)
    return np.where(np.isnan(a), a, w) if keep_nan else w


def emulate(c, cfg, *, defect=None):
    """lowd_lse_kernel's / lowd_lse_grad_kernel's steps (feed = 0 in the case's kw: lowd_batch_lse_kernel's) in numpy in
    the working precision: the kept differences, the chain of s, lse_neg_logit, the logits in log2 units, batches of 4 with
    the largest logit, ceil, the rescales of the working-precision and fp64 sums with their clamps, the weights, the D + 1
    sums, the guard zone, the folds (every `chunk` rounded up to tiles of 256; feed = 0: to 8), the segments, the merge,
    the finish, the NaN row -- (N, NC) or (N, NC, D) float64."""
    which, sig, E, chunk, segments = cfg
    defect = _defects(defect)
    grad, density = which == "grad", sig == "density"
    dt = c["precision"].type
    kernel, feed = c["kernel"], c["kw"].get("feed", 1)
    y = np.asarray(c["y"], dt)
    x = y if c["x"] is None else np.asarray(c["x"], dt)
    M, D = y.shape
    N = x.shape[0]
    cc = np.zeros((M, 1), dt) if density else np.ascontiguousarray(c["b"][:, :E]).astype(dt)
    NC, K = cc.shape[1], (D + 1 if grad else 1)
    out_shape = (N, NC, D) if grad else (N, NC)
    if M == 0 or N == 0:
        return np.full(out_shape, np.nan if grad else -np.inf)
    segments = 1 if feed == 0 else max(segments, 1)
    m_pad = cases._round_up(M, lm.LOWD_BATCH)
    y = np.concatenate((y, np.full((m_pad - M, D), np.inf, dt)))
    cc = np.concatenate((cc, np.zeros((m_pad - M, NC), dt)))
    seg_len = cases._round_up(-(-m_pad // segments), lm.LOWD_BATCH)
    clamp = -300.0 if dt == f32 else -4000.0
    with np.errstate(all="ignore"):
        df = (x[:, None, :] - y[None, :, :]).astype(dt)
        s = (df[:, :, 0] * df[:, :, 0]).astype(dt)
        for d in range(1, D):
            s = _fma(df[:, :, d], df[:, :, d], s)
        if kernel == "gaussian":
            nl = s
        elif dt == f32:
            nl = np.sqrt(s)
        else:
            _, yy = cases._rsq_step(s, "no-newton" if "no-newton" in defect else None)
            nl = np.where((s == 0) | (s == np.inf), s, s * yy)
        if density:
            u = (nl * dt(-sm.LOG2E)).astype(dt)[:, :, None]
        else:
            u = ((cc[None, :, :] - nl[:, :, None]).astype(dt) * dt(sm.LOG2E)).astype(dt)
        q = None
        if grad and kernel != "gaussian":
            q = cases.emulate_kval("inverse-distance", s)
            if "no-s0-select" not in defect:
                q = np.where((s >= np.finfo(dt).tiny) & (s < np.inf), q, dt(0))
        x_nan = np.isnan(x).any(axis=1)
        stop_all = M // U * U if "drop-ragged" in defect else m_pad
        parts = []
        for j0 in range(0, m_pad, seg_len):
            j1 = min(j0 + seg_len, m_pad)
            acc, accd = np.zeros((N, NC, K), dt), np.zeros((N, NC, K))
            m = np.full((N, NC), sm.SENTINEL[np.dtype(dt)], dt)
            folds = set(cases._fold_points("lowd", dt, j0, j1, feed, chunk))
            for jb in range(j0, j1, U):
                if jb < stop_all:
                    ub, dfb = u[:, jb:jb + U, :], df[:, jb:jb + U, :]
                    if grad and jb + U > m_pad - GUARD_RECORDS and "no-guard" not in defect:
                        live = np.broadcast_to((np.arange(jb, jb + U) < M)[None, :], (N, U))   # the record's index, not s
                        if "guard-s-lt-inf" in defect:
                            live = s[:, jb:jb + U] < np.inf
                        dfb = np.where(live[:, :, None], dfb, dt(0))
                    bmax = np.fmax.reduce(ub, axis=1)
                    rise = bmax > m
                    m_new = np.where(rise, np.ceil(bmax), m).astype(dt)
                    e = np.where(rise, np.fmax(m - m_new, dt(clamp)), 0).astype(np.int32)[:, :, None]
                    if "rise-skips-V" in defect:
                        acc[:, :, :1], accd[:, :, :1] = np.ldexp(acc[:, :, :1], e), np.ldexp(accd[:, :, :1], e)
                    else:
                        acc = np.ldexp(acc, e)
                        if "rise-skips-fp64" not in defect:
                            accd = np.ldexp(accd, e)
                    m = m_new
                    for k in range(U):
                        w = _exp2_neg((m - ub[:, k, :]).astype(dt), grad or "nan-weight-dropped" not in defect)
                        acc[:, :, 0] = (acc[:, :, 0] + w).astype(dt)
                        if grad:
                            wq = w if q is None else (w * q[:, jb + k, None]).astype(dt)
                            acc[:, :, 1:] = _fma(np.broadcast_to(wq[:, :, None], (N, NC, D)),
                                                 np.broadcast_to(dfb[:, k, None, :], (N, NC, D)), acc[:, :, 1:])
                if jb + U in folds:
                    accd = accd + acc.astype(f64)
                    acc = np.zeros((N, NC, K), dt)
            v = accd
            v[x_nan] = np.nan
            parts.append((v, np.where(v[:, :, 0] == 0, np.inf, -m.astype(f64))))
        # lse_reduce_kernel / lse_grad_reduce_kernel
        kmin = parts[0][1] if "merge-first-exponent" in defect else np.fmin.reduce([k for _, k in parts])
        sums = np.zeros((N, NC, K))
        for v, ks in parts:
            e = np.clip(np.where(np.isnan(kmin - ks), -100000.0, kmin - ks), -100000.0, 100000.0).astype(np.int64)
            sums = sums + np.where((ks < np.inf)[:, :, None], np.ldexp(v, e[:, :, None]), 0.0)
        alive = kmin < 1.0e300
        if not grad:
            return np.where(alive, (np.log2(sums[:, :, 0]) - kmin) * LN2, -np.inf)
        return np.where(alive[:, :, None], sm.CONSTANT[kernel] * sums[:, :, 1:] / sums[:, :, :1], np.nan)


def compare(got, m, is_loose):
    """(max err / band over the elements that must be in band, what is wrong or None).  The elements the model calls
    poisoned are non-finite; where its value is -inf (L) or NaN (G) without being poisoned -- no live term -- the result
    is exactly that; every other element is finite and within the band, which must itself be finite on every such
    element: there is no list of exceptions.  On a loose case an element that is not
    poisoned may be non-finite instead."""
    if got.shape != m.value.shape:
        return 0.0, f"shape {got.shape} for {m.value.shape}"
    bad = m.poisoned
    if np.isfinite(got[bad]).any():
        where = np.argwhere(bad & np.isfinite(got))
        return 0.0, f"finite where the model is not: {len(where)} elements, first {where[0].tolist()} = {got[tuple(where[0])]!r}"
    exact = ~bad & ~np.isfinite(m.value)
    must = ~bad & np.isfinite(m.value)
    if is_loose:
        exact, must = exact & np.isfinite(got), must & np.isfinite(got)
    elif not np.isfinite(got[must]).all():
        where = np.argwhere(must & ~np.isfinite(got))
        return 0.0, f"non-finite where the model is finite: {len(where)} elements, first {where[0].tolist()} = {got[tuple(where[0])]!r}"
    if not np.array_equal(got[exact], m.value[exact], equal_nan=True):
        where = np.argwhere(exact & ~((got == m.value) | (np.isnan(got) & np.isnan(m.value))))
        return 0.0, f"not exactly {m.value[tuple(where[0])]!r}: {len(where)} elements, first {where[0].tolist()} = {got[tuple(where[0])]!r}"
    if not must.any():
        return 0.0, None
    if not np.isfinite(m.band[must]).all():                     # a band of inf would hold the kernel to finiteness only
        where = np.argwhere(must & ~np.isfinite(m.band))
        return 0.0, f"the model's band is not finite: {len(where)} elements, first {where[0].tolist()}"
    with np.errstate(divide="ignore", invalid="ignore"):
        err, band = np.abs(got - m.value)[must], m.band[must]
        ratio = np.where(band > 0, err / band, np.where(err > 0, np.inf, 0.0))
    k = int(np.argmax(ratio))
    if ratio[k] > 1.0:
        at = [int(a[k]) for a in np.nonzero(must)]
        return float(ratio[k]), f"err/band {ratio[k]:.3g} at {at}: err {err[k]:.3g} band {band[k]:.3g}; {int((ratio > 1).sum())} elements"
    return float(ratio[k]), None
