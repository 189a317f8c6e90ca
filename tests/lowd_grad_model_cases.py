"""Clouds, configurations and numpy emulations shared by tests/test_lowd_grad_model.py (CPU) and
tests/test_gpu_lowd_grad_arith.py (GPU): the GPU test runs lowd_grad_kernel and lowd_dscale_kernel on exactly the clouds
on which the CPU test keeps the clean emulations of their steps inside the model's band
(oracle/kmvp_lowd_grad_model.py) and shows that an emulation with one defect leaves it.

The far targets, the clouds at +100 and the zero-rule clouds are tests/lowd_model_cases.py's own; what is added here is
what the two kernels add: signal columns that differ in scale and sign (the column order e D + d), every batch, guard
zone, tile and fold boundary, the overflowing difference, duplicated points, non-finite inputs.

A configuration is (which, sig, E, chunk, segments): which = "grad" / "dscale", sig = "product" / "density", segments = 0
for the library's own choice."""
import itertools

import numpy as np

import kmvp_lowd_grad_model as gm
import kmvp_lowd_model as lm
import lowd_model_cases as cases
from lowd_model_cases import _fma, f32, f64

KERNELS = gm.KERNELS
DSCALE = gm.DSCALE_KERNELS                                   # no length-scale derivative for 1/r
PRECISIONS = (np.float32, np.float64)
NAME = {"grad": "lowd_grad_kernel", "dscale": "lowd_dscale_kernel"}
COLUMN_SCALES = np.array([1.0, -3.0, 0.25, 7.0])             # signal columns distinct in scale and sign
MODES = [("product", e) for e in (1, 2, 3, 4)] + [("density", 1)]
N_EDGES = (1, 63, 64, 65, 255, 256, 257)
M_EDGES = (1, 3, 4, 5, 7, 8, 9, 12, 15, 16, 17, 255, 256, 257, 260, 513, 1030)
SEGMENTS = cases.SEGMENTS
SHARDS = cases.SHARDS
U, GUARD_RECORDS = 4, 8                                       # sources per batch; the guard zone: the array's last 2 U records


def whiches(kernel):
    return ("grad",) if kernel == "inverse-distance" else ("grad", "dscale")


def signal(rs, M, E, precision):
    return (cases.signal(rs, M, E, np.float64) * COLUMN_SCALES[:E]).astype(precision)


def case(name, kernel, precision, y, x, b, **kw):
    return dict(name=name, kernel=kernel, precision=np.dtype(precision), y=y, x=x, b=b, kw=kw)


def signal_of(c, sig, E=None):
    return None if sig == "density" else np.ascontiguousarray(c["b"][:, :E])


def model(c, cfg, **more):
    which, sig, E, chunk, _ = cfg
    kw = {k: v for k, v in c["kw"].items() if k in ("j_offset", "M_total")}
    return gm.lowd_gradient(c["kernel"], c["y"], c["x"], signal_of(c, sig, E), precision=c["precision"], dscale=which == "dscale",
                            chunk=chunk, **dict(kw, **more))


def grid_cases(kernel, precision):
    """D = 1 ... 8 on N = 67 targets x M = 101 sources (ragged in both: pad records, a guard zone that starts inside a
    batch of real sources), four signal columns; and the same points at D = 3."""
    for D in range(1, cases.LOWD_MAX_D + 1):
        rs = np.random.RandomState(cases.seed("grad-grid", kernel, D))
        y = cases.points(rs, 101, D, precision)
        yield case(("grid", kernel, D), kernel, precision, y, cases.points(rs, 67, D, precision), signal(rs, 101, 4, precision))
        if D == 3:
            yield case(("grid-same", kernel, D), kernel, precision, y, None, signal(rs, 101, 4, precision))


def size_cases(kernel, precision):
    """Every M of M_EDGES (batches of 4, the guard zone of 8 -- all of the array for M <= 8 --, LDS tiles of 256, folds)
    with the N of N_EDGES in turn (one lane, a wave less one, whole waves, a block and one more); D = 3."""
    for M, N in zip(M_EDGES, itertools.cycle(N_EDGES)):
        rs = np.random.RandomState(cases.seed("grad-size", kernel, N, M))
        yield case(("size", kernel, N, M), kernel, precision, cases.points(rs, M, 3, precision), cases.points(rs, N, 3, precision),
                   signal(rs, M, 2, precision))


def segment_cases(kernel, precision):
    rs = np.random.RandomState(cases.seed("grad-seg", kernel))
    yield case(("segments", kernel), kernel, precision, cases.points(rs, 1030, 3, precision), cases.points(rs, 65, 3, precision),
               signal(rs, 1030, 2, precision))


def shared_cases(kernel, precision):
    """tests/lowd_model_cases.py's far targets (float32: e^-2 ... e^-150, the flush, the Matern clamp; float64: e^-400 ...
    e^-830, denormal terms, exact zeros, the clamp at 800) and its clouds at +100, as they are."""
    for c in list(cases.far_cases(kernel, precision, "lowd")) + list(cases.moved_cases(kernel, precision, "lowd")):
        yield case(("far" if str(c["name"][0]).startswith("far") else "moved",) + tuple(c["name"]), kernel, precision, c["y"], c["x"], c["b"])


def overflow_cases(kernel, precision):
    """float32: two sources at 3e19 in one coordinate, one in an unguarded batch and one in the guard zone (M = 70:
    records 64 ... 71): every |x_0 - y_0|^2 with them overflows although x - y is finite."""
    if np.dtype(precision) != np.float32 or kernel == "inverse-distance":
        return
    rs = np.random.RandomState(cases.seed("grad-overflow", kernel))
    y = cases.points(rs, 70, 3, precision)
    y[0, 0], y[66, 0] = 3e19, -3e19
    yield case(("overflow", kernel), kernel, precision, y, cases.points(rs, 67, 3, precision), signal(rs, 70, 2, precision))


def duplicate_cases(kernel, precision):
    """The same points with two duplicated points: exp(-r) at s = 0 off the diagonal (0 by the select); 1/r: the planted
    pairs are coincident and not zeroed: rows 2, 17, 33, 90 are non-finite."""
    rs = np.random.RandomState(cases.seed("grad-duplicate", kernel))
    y = cases.points(rs, 101, 3, precision)
    y[90], y[33] = y[17], y[2]
    bad = [2, 17, 33, 90] if kernel == "inverse-distance" else []
    yield case(("duplicates", kernel), kernel, precision, y, None, signal(rs, 101, 2, precision), bad_rows=bad)


def zero_rule_cases(precision):
    """tests/lowd_model_cases.py's 1/r cloud: N = 450 > M_total + 1 = 201, the zero column wraps inside the tile of rows
    192 ... 255 and across tiles."""
    for c in cases.zero_rule_cases(precision, "lowd"):
        yield case(("wrap",), "inverse-distance", precision, c["y"], c["x"], c["b"])


def nan_target_cases(kernel, precision):
    """A NaN coordinate in target 5 at M = 5 and M = 8 (every batch guarded) and M = 101; 1/r also in row 200 of the
    wrapping cloud, inside the tile in which every batch is guarded."""
    for M in (5, 8, 101):
        rs = np.random.RandomState(cases.seed("grad-nan-target", kernel, M))
        y, x = cases.points(rs, M, 3, precision), cases.points(rs, 67, 3, precision)
        x[5, 2] = np.nan
        yield case(("nan-target", kernel, M), kernel, precision, y, x, signal(rs, M, 2, precision), bad_rows=[5])
    if kernel == "inverse-distance":
        c = list(zero_rule_cases(precision))[0]
        x = c["x"].copy()
        x[200, 0] = np.nan
        yield case(("nan-target", kernel, "wrap"), kernel, precision, c["y"], x, c["b"], bad_rows=[200])


SOURCE_POSITIONS = (0, 50, 98)                                # M = 101: the first, the middle, the guard zone (96 ... 103)


def bad_source_cases(kernel, precision):
    """A NaN, a +inf and a -inf source coordinate (axis 1 of 3) at each of SOURCE_POSITIONS; a NaN signal entry."""
    rs = np.random.RandomState(cases.seed("grad-bad-source", kernel))
    y, x, b = cases.points(rs, 101, 3, precision), cases.points(rs, 67, 3, precision), signal(rs, 101, 2, precision)
    for tag, v in (("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf)):
        for j in SOURCE_POSITIONS:
            yb = y.copy()
            yb[j, 1] = v
            yield case(("bad-source", kernel, tag, j), kernel, precision, yb, x, b, loose=True)
    bb = b.copy()
    bb[40, 1] = np.nan
    yield case(("nan-signal", kernel), kernel, precision, y, x, bb)


def configs(c):
    """What the GPU test runs on a case."""
    group, kernel = c["name"][0], c["kernel"]
    E_all = c["b"].shape[1]
    for which in whiches(kernel):
        if group in ("grid", "grid-same"):
            for sig, E in MODES:
                for chunk in (8, 512):
                    yield which, sig, E, chunk, 0
        elif group == "size":
            for sig, E in (("product", 2), ("density", 1)):
                for chunk in (8, 256, 512):
                    yield which, sig, E, chunk, 0
        elif group == "segments":
            for segments in SEGMENTS:
                for chunk in (8, 512):
                    yield which, "product", 2, chunk, segments
        else:
            for sig, E in (("product", E_all), ("density", 1)):
                if sig == "density" and group == "nan-signal":
                    continue
                yield which, sig, E, 512, 0


def groups(kernel, precision):
    out = {"grid": list(grid_cases(kernel, precision)),
           "edges": [c for gen in (size_cases, segment_cases) for c in gen(kernel, precision)],
           "range": [c for gen in (shared_cases, overflow_cases, duplicate_cases) for c in gen(kernel, precision)],
           "nonfinite": [c for gen in (nan_target_cases, bad_source_cases) for c in gen(kernel, precision)]}
    if kernel == "inverse-distance":
        out["range"] += list(zero_rule_cases(precision))
    return out


def golden_cases():
    """One small cloud per kernel function and precision (N = 24 x M = 37, D = 3, E = 2) whose results, recorded from the
    library BEFORE the guard's select and the NaN row were changed, are in tests/golden/lowd_grad_parent.npz."""
    for kernel in KERNELS:
        for precision in PRECISIONS:
            rs = np.random.RandomState(cases.seed("grad-golden", kernel))
            yield case(("golden", kernel), kernel, precision, cases.points(rs, 37, 3, precision), cases.points(rs, 24, 3, precision),
                       signal(rs, 37, 2, precision))


def golden_key(c, which):
    return f"{which}|{c['kernel']}|{c['precision'].name}"


# ---- numpy emulation of the two kernels' own steps -------------------------------------------------------------------

DEFECTS = ("guard-s-lt-inf", "no-nan-row", "no-wrap", "no-j-offset", "pad-df-kept", "drop-ragged", "fold-assigns", "columns-transposed",
           "matern-value-degree", "five-thirds-is-one", "no-s0-select", "kept-square", "b0-for-every-e", "constant-sign")


def _defects(defect):
    """None, one name or several: a tuple of names."""
    return () if defect is None else (defect,) if isinstance(defect, str) else tuple(defect)


def emulate_weight(kernel, s, defect=None):
    """grad_weight<KERNEL>(s) and exp(-r)'s positive_normal select, in the dtype of s."""
    defect = _defects(defect)
    dt = s.dtype.type
    with np.errstate(all="ignore"):
        if kernel == "gaussian":
            return cases.emulate_kval("gaussian", s)
        if kernel in gm.DEG_W:
            if "matern-value-degree" in defect:
                return cases.emulate_kval(kernel, s)
            deg = gm.DEG_W[kernel]
            if dt == f32:
                a = np.fmin((np.sqrt(s) * f32(lm.SQRT_2NU[kernel] * cases.LOG2E)).astype(f32), f32(192.0))
                e = cases._exp2f(-a)
                return e if deg == 0 else (_fma(a, f32(0.6931471805599453), np.ones_like(a)) * e).astype(f32)
            y0, y = cases._rsq_step(s)
            r = np.where((s == 0) | (s == np.inf), s, s * y)
            t = np.fmin(r * lm.SQRT_2NU[kernel], 800.0)
            ex = cases._kexp_neg_f64(t)
            return ex if deg == 0 else (1.0 + t) * ex
        q = cases.emulate_kval("inverse-distance", s)
        if kernel == "inverse-distance":
            return ((q * q).astype(dt) * q).astype(dt)
        w = (cases.emulate_kval("gaussian", (s * q).astype(dt)) * q).astype(dt)
        if "no-s0-select" in defect:
            return w
        return np.where((s >= np.finfo(dt).tiny) & (s < np.inf), w, dt(0))


def guarded(N, M, m_pad, kernel, j_offset, M_total, defect=None):
    """(N, m_pad) mask of the pairs that run grad_interact<GUARD = true>, and each target's zero column (-1: none)."""
    defect = _defects(defect)
    j = np.arange(m_pad)
    first = j // U * U                                        # the pair's batch
    guard = np.broadcast_to((first + U > m_pad - GUARD_RECORDS)[None, :], (N, m_pad)).copy()
    jz = np.full(N, -1, dtype=np.int64)
    if kernel == "inverse-distance":
        i = np.arange(N)
        i0 = i // 64 * 64
        wrap = "no-wrap" not in defect
        off = 0 if "no-j-offset" in defect else j_offset
        g = i % (M_total + 1) if wrap else i
        jz = np.where(g < M_total, g - off, -1)
        g_lo = i0 % (M_total + 1) if wrap else i0
        g_hi = g_lo + 63
        whole = g_hi > M_total
        lo, hi = (g_lo - off)[:, None], (g_hi - off)[:, None]
        guard |= whole[:, None] | ((first[None, :] + U - 1 >= lo) & (first[None, :] <= hi))
    return guard, jz


def emulate(c, cfg, *, defect=None):
    """lowd_grad_kernel's / lowd_dscale_kernel's steps in numpy in the working precision: the kept differences, the chain
    of s, grad_weight, batches of 4 with the guard zone and its selects, the 1/r zero rule, both branches of the
    derivative's product, the chains between folds (every `chunk` rounded up to tiles of 256), the segments, the
    constant, the NaN row -- (N, E, D) float64."""
    which, sig, E, chunk, segments = cfg
    segments = max(segments, 1)
    defect = _defects(defect)
    dt = c["precision"].type
    kernel, dscale, density = c["kernel"], which == "dscale", sig == "density"
    y = np.asarray(c["y"], dt)
    x = y if c["x"] is None else np.asarray(c["x"], dt)
    M, D = y.shape
    N = x.shape[0]
    b = np.ones((M, 1), dt) if density else np.ascontiguousarray(c["b"][:, :E]).astype(dt)
    EC = b.shape[1]
    j_offset, M_total = c["kw"].get("j_offset", 0), c["kw"].get("M_total", M)
    m_pad = cases._round_up(max(M, 1), lm.LOWD_BATCH)
    y = np.concatenate((y, np.full((m_pad - M, D), np.inf, dt)))
    b = np.concatenate((b, np.zeros((m_pad - M, EC), dt)))
    seg_len = cases._round_up(-(-m_pad // segments), lm.LOWD_BATCH)
    with np.errstate(all="ignore"):
        df = (x[:, None, :] - y[None, :, :]).astype(dt)
        s = (df[:, :, 0] * df[:, :, 0]).astype(dt)
        for d in range(1, D):
            s = _fma(df[:, :, d], df[:, :, d], s)
        w = emulate_weight(kernel, s, defect)
        guard, jz = guarded(N, M, m_pad, kernel, j_offset, M_total, defect)
        pad = ~(s < np.inf) if "guard-s-lt-inf" in defect else np.broadcast_to((np.arange(m_pad) >= M)[None, :], s.shape)
        pad = guard & pad
        w = np.where(pad, dt(0), w)
        if "pad-df-kept" not in defect:
            df = np.where(pad[:, :, None], dt(0), df)
        if kernel == "inverse-distance":
            w = np.where(guard & (np.arange(m_pad)[None, :] == jz[:, None]), dt(0), w)
        stop_all = M // U * U if "drop-ragged" in defect else m_pad
        total = np.zeros((N, EC, D))
        const = gm.CONSTANT[kernel]
        if "five-thirds-is-one" in defect and kernel == "matern-5/2":
            const = -1.0
        if dscale:
            const = -const
        if "constant-sign" in defect:
            const = -const
        for j0 in range(0, m_pad, seg_len):
            j1 = min(j0 + seg_len, m_pad)
            acc, accd = np.zeros((N, EC, D), dt), np.zeros((N, EC, D))
            folds = set(cases._fold_points("lowd", dt, j0, j1, 1, chunk))
            for j in range(j0, j1):
                if j < stop_all:
                    wj, dj = w[:, j], df[:, j, :]
                    if not dscale:
                        wb = wj[:, None] if density else (wj[:, None] * b[j][None, :]).astype(dt)
                        acc = _fma(np.broadcast_to(wb[:, :, None], acc.shape), np.broadcast_to(dj[:, None, :], acc.shape), acc)
                    elif density or E == 1:
                        wb = wj if density else (wj * b[j, 0]).astype(dt)
                        if "kept-square" in defect:
                            acc = _fma(np.broadcast_to(wb[:, None, None], acc.shape), np.broadcast_to((dj * dj).astype(dt)[:, None, :], acc.shape), acc)
                        else:
                            t = (wb[:, None] * dj).astype(dt)
                            acc = _fma(t[:, None, :], dj[:, None, :], acc)
                    else:
                        ud = ((wj[:, None] * dj).astype(dt) * dj).astype(dt)
                        be = np.broadcast_to(b[j, 0], (EC,)) if "b0-for-every-e" in defect else b[j]
                        acc = _fma(np.broadcast_to(ud[:, None, :], acc.shape), np.broadcast_to(be[None, :, None], acc.shape), acc)
                if j + 1 in folds:
                    accd = acc.astype(f64) if "fold-assigns" in defect else accd + acc.astype(f64)
                    acc = np.zeros((N, EC, D), dt)
            total = total + const * accd
        if "columns-transposed" in defect:                    # written at d E + e, read at e D + d
            total = np.ascontiguousarray(total.transpose(0, 2, 1)).reshape(N, EC, D)
        if "no-nan-row" not in defect:
            total[np.isnan(x).any(axis=1)] = np.nan           # nan_target
    return total
