"""Clouds, signals and numpy emulations shared by tests/test_lowd_model.py (CPU) and tests/test_gpu_lowd_arith.py (GPU): the
GPU test runs lowd_kernel, lowd_mid_kernel and lowd_big_kernel on exactly the clouds on which the CPU test keeps the clean
emulations of their steps inside the model's band (oracle/kmvp_lowd_model.py) and shows that an emulation with one defect
leaves it.

The difference form has relative accuracy in s, so the clouds are plain Gaussian ones (no lattice is needed to keep pairs
apart); what the cases vary is the shape, the feed, the fold length, the distance of the targets and the exact rules."""
import numpy as np

import kmvp_lowd_model as lm

KERNELS = lm.KERNELS
PRECISIONS = (np.float32, np.float64)
SIGS = ("product", "norm", "density")
LOWD_MAX_D, LOWD_MAX_E, LOWD_MID_MAX_D = 8, 4, 128          # kmvp_internal.hpp
TUNINGS = ((1, 1), (2, 0))                                  # (T, feed) every lowd_kernel shape is instantiated for
HEADLINE_TUNINGS = tuple((T, feed) for feed in (1, 0) for T in (1, 2, 4, 8))   # D = 3, E = 1: the whole grid
CHUNKS = (8, 512)                                           # the "chunk" option: a fold at every ping-pong, the default
NAME = {"lowd": "lowd_kernel", "mid": "lowd_mid_kernel", "big": "lowd_big_kernel"}


def path_of(D, E):
    return "lowd" if D <= LOWD_MAX_D else ("mid" if D <= LOWD_MID_MAX_D else "big")


def points(rs, n, D, precision, spread=1.5):
    """A Gaussian cloud whose squared distances are about 2 spread."""
    return (rs.randn(n, D) * np.sqrt(spread / D)).astype(precision)


def signal(rs, M, E, precision):
    """E columns of mixed sign with a nonzero mean."""
    return (rs.randn(M, E) + 0.5).astype(precision)


def case(name, kernel, precision, y, x, b, **kw):
    D = y.shape[1]
    return dict(name=name, kernel=kernel, precision=np.dtype(precision), path=path_of(D, b.shape[1]), y=y, x=x, b=b, kw=kw)


def signal_of(c, sig, E=None):
    return None if sig == "density" else np.ascontiguousarray(c["b"][:, :E])


def model(c, sig, E=None, **more):
    """The model of a case for one signal mode and the first E signal columns."""
    kw = dict(model_kw(c), **more)
    return lm.lowd_product(c["kernel"], c["y"], c["x"], signal_of(c, sig, E), sig == "norm", precision=c["precision"],
                           path=c["path"], **kw)


def seed(*key):
    """A seed from a case's key that does not depend on the interpreter's hash randomisation."""
    return sum((i + 1) * ord(ch) for i, ch in enumerate(repr(key))) % (2 ** 31)


def grid_cases(kernel, precision):
    """lowd_kernel: D = 1 ... 8 on N = 67 x M = 101 (ragged in both: pad records, two ping-pongs short of a tile), the
    same points and different points alternating over D, four signal columns."""
    for D in range(1, LOWD_MAX_D + 1):
        rs = np.random.RandomState(seed("grid", kernel, D))
        y = points(rs, 101, D, precision)
        x = None if D % 2 == 0 else points(rs, 67, D, precision)
        yield case(("grid", kernel, D), kernel, precision, y, x, signal(rs, 101, 4, precision))


MID_RAGGED_D = {np.dtype(np.float32): 61, np.dtype(np.float64): 45}


def mid_dims(precision):
    return [8 * dch for dch in range(2, 17)] + [MID_RAGGED_D[np.dtype(precision)]]


def mid_columns(precision, D):
    """Signal column counts of lowd_mid_kernel's column blocks: EBW = 8 with one and two passes; float32 rows of up to 64
    coordinates take EBW = 32 from nine columns on: one and two passes of that."""
    return (1, 9, 33) if np.dtype(precision) == np.float32 and D <= 64 else (1, 9)


def mid_colblock(precision, D, E):
    return 32 if np.dtype(precision) == np.float32 and D <= 64 and E > 8 else 8


def mid_cases(kernel, precision):
    """lowd_mid_kernel: every DCH = 2 ... 16 at D = 8 DCH and one ragged D, N = 67 x M = 101 (two fp32 chunks of 64)."""
    for D in mid_dims(precision):
        rs = np.random.RandomState(seed("mid", kernel, D))
        y = points(rs, 101, D, precision)
        x = None if (D // 8) % 2 == 0 else points(rs, 67, D, precision)
        yield case(("mid", kernel, D), kernel, precision, y, x, signal(rs, 101, max(mid_columns(precision, D)), precision))


BIG_DIMS = (129, 160, 161)


def big_cases(kernel, precision):
    """lowd_big_kernel at D = 129, 160 (five whole chunks of 32) and 161; M = 101 = 12 batches of 8 and a ragged one."""
    for D in BIG_DIMS:
        rs = np.random.RandomState(seed("big", kernel, D))
        y = points(rs, 101, D, precision)
        x = None if D == 160 else points(rs, 67, D, precision)
        yield case(("big", kernel, D), kernel, precision, y, x, signal(rs, 101, 9, precision))


SIZES = ((1, 1), (63, 3), (65, 5), (255, 7), (257, 9), (2049, 255), (1, 257), (63, 513), (65, 1030))   # (N, M)
SIZE_DIMS = {"lowd": 3, "mid": 20, "big": 129}


def size_cases(kernel, precision, path):
    """N and M around the batch of 4, the ping-pong of 8, LDS_TILE = 256, BIG_BATCH = 8 and the fold at 64; more than one
    target block (N = 2049) on lowd_kernel only."""
    for N, M in SIZES:
        if path != "lowd" and N > 300:
            continue
        rs = np.random.RandomState(seed("size", kernel, N, M))
        D = SIZE_DIMS[path]
        yield case(("size", path, kernel, N, M), kernel, precision, points(rs, M, D, precision), points(rs, N, D, precision),
                   signal(rs, M, 2, precision))


SEGMENTS = (1, 2, 3, 17)


def segment_cases(kernel, precision, path):
    """N = 65 x M = 1030 under forced segment counts: 17 is past SEG_SPLIT_FROM = 16 (the split reduction); 1030 / 17 and
    1030 / 3 end a segment inside a batch."""
    rs = np.random.RandomState(seed("seg", kernel, path))
    D = SIZE_DIMS[path]
    yield case(("segments", path, kernel), kernel, precision, points(rs, 1030, D, precision), points(rs, 65, D, precision),
               signal(rs, 1030, 2, precision))


BLOCK_COLUMNS = (5, 6, 9)


def block_cases(kernel, precision):
    """run_product_blocked: E = 5, 6 and 9 columns at D = 3 in blocks of four, the denominator from the first block."""
    rs = np.random.RandomState(seed("block", kernel))
    y = points(rs, 101, 3, precision)
    yield case(("blocks", kernel), kernel, precision, y, points(rs, 67, 3, precision), signal(rs, 101, 9, precision))


def exponent_to_distance(kernel, expo):
    """The distance at which the kernel's exponential has exponent -expo (1/r: the Gaussian's)."""
    if kernel in ("gaussian", "inverse-distance"):
        return np.sqrt(expo)
    return expo / (lm.SQRT_2NU[kernel] if kernel in lm.SQRT_2NU else 1.0)


FAR_RANGE = {np.dtype(np.float32): ((2.0, 80.0), (2.0, 150.0)), np.dtype(np.float64): ((400.0, 690.0), (400.0, 830.0))}


def far_cases(kernel, precision, path="lowd"):
    """Targets along a ray away from a tight cloud, so that the exponent of the kernel's exponential runs through
    float64: 400 ... 745 (denormal results, then exact zeros) and past the clamp at 800; float32: e^-2 ... e^-80, past the
    flush at e^-87.3 and past the Matern clamp at 192 binades.  The first range (no row may lose every pair) also runs
    normalised; the second runs the product and the density only."""
    D = SIZE_DIMS[path]
    for tag, (lo, hi) in zip(("far-norm", "far"), FAR_RANGE[np.dtype(precision)]):
        rs = np.random.RandomState(seed("far", kernel, tag, path))
        y = (points(rs, 101, D, np.float64) * 0.1).astype(precision)
        x = (points(rs, 67, D, np.float64) * 0.1)
        x[:, 0] += exponent_to_distance(kernel, np.linspace(lo, hi, 67))
        yield case((tag, path, kernel), kernel, precision, y, x.astype(precision), signal(rs, 101, 2, precision),
                   sigs=SIGS if tag == "far-norm" else ("product", "density"))


def moved_cases(kernel, precision, path):
    """Both clouds translated by +100 in every coordinate: nothing may be scaled or rounded before the subtraction."""
    rs = np.random.RandomState(seed("moved", kernel, path))
    D = SIZE_DIMS[path]
    y = (points(rs, 101, D, np.float64) + 100.0).astype(precision)
    x = (points(rs, 67, D, np.float64) + 100.0).astype(precision)
    yield case(("moved", path, kernel), kernel, precision, y, x, signal(rs, 101, 2, precision))


SHARDS = ((0, 67), (67, 131), (131, 200))


def zero_rule_cases(precision, path):
    """1/r with N = 450 > M_total + 1 = 201: the zero column wraps, inside a target tile (rows 192 ... 255 at T = 1, the
    one tile at T = 8) and across tiles; whole, and as three source slices (SHARDS) with j_offset / M_total."""
    rs = np.random.RandomState(seed("zero", path))
    D = SIZE_DIMS[path]
    yield case(("wrap", path), "inverse-distance", precision, points(rs, 200, D, precision), points(rs, 450, D, precision),
               signal(rs, 200, 1, precision))


def nonfinite_cases(kernel, precision, path):
    """A NaN target coordinate (row 5) and sources at +inf and -inf, which contribute 0; 1/r also on the sources
    themselves with one planted coincident off-diagonal pair (17, 90): exactly those two rows are non-finite."""
    rs = np.random.RandomState(seed("nonfinite", kernel, path))
    D = SIZE_DIMS[path]
    y, x = points(rs, 101, D, precision), points(rs, 67, D, precision)
    x[5, D - 1] = np.nan
    y[7, 0], y[11, D - 1] = np.inf, -np.inf
    yield case(("nan-inf", path, kernel), kernel, precision, y, x, signal(rs, 101, 2, precision), bad_rows=[5])
    if kernel == "inverse-distance":
        y = points(rs, 101, D, precision)
        y[90] = y[17]
        yield case(("coincident", path), kernel, precision, y, None, signal(rs, 101, 2, precision), bad_rows=[17, 90])


def configs(c):
    """What the GPU test runs on a case: (sig, E, T, feed, chunk, segments); T = feed = 0 where the kernel has no tuning
    (lowd_mid_kernel, lowd_big_kernel, and run_product_blocked, which takes the default pair (1, 1)); segments = 0: the
    library's own choice."""
    group, path, D = c["name"][0], c["path"], c["y"].shape[1]
    lowd = path == "lowd"
    chunks = CHUNKS if lowd else (512,)
    if group == "grid":
        for sig, E in [(s, e) for s in ("product", "norm") for e in (1, 2, 3, 4)] + [("density", 1)]:
            for T, feed in (HEADLINE_TUNINGS if D == 3 and E == 1 else TUNINGS):
                for chunk in chunks:
                    yield sig, E, T, feed, chunk, 0
    elif group in ("mid", "big"):
        for E in (mid_columns(c["precision"], D) if group == "mid" else (1, 9)):
            for sig in ("product", "norm"):
                yield sig, E, 0, 0, 512, 0
        yield "density", 1, 0, 0, 512, 0
    elif group == "blocks":
        for E in BLOCK_COLUMNS:
            for sig in ("product", "norm"):
                for chunk in chunks:
                    yield sig, E, 0, 0, chunk, 0
    else:
        tunings = TUNINGS if lowd else ((0, 0),)
        if group == "wrap" and lowd:
            tunings = ((1, 1), (8, 1), (2, 0))
        for sig, E in (("product", 1), ("norm", 2), ("density", 1)) if c["b"].shape[1] > 1 else (("product", 1), ("norm", 1), ("density", 1)):
            if sig not in c["kw"].get("sigs", SIGS):
                continue
            for T, feed in tunings:
                for chunk in chunks:
                    for segments in (SEGMENTS if group == "segments" else (0,)):
                        yield sig, E, T, feed, chunk, segments


def groups(kernel, precision):
    """Every case of one kernel function and precision, by the GPU test that runs it."""
    paths = ("lowd", "mid", "big")
    out = {"grid": list(grid_cases(kernel, precision)), "mid": list(mid_cases(kernel, precision)),
           "big": list(big_cases(kernel, precision)), "blocks": list(block_cases(kernel, precision)),
           "edges": [c for p in paths for gen in (size_cases, segment_cases, moved_cases, nonfinite_cases)
                     for c in gen(kernel, precision, p)] + [c for p in paths for c in far_cases(kernel, precision, p)]}
    if kernel == "inverse-distance":
        out["edges"] += [c for p in paths for c in zero_rule_cases(precision, p)]
    return out


MODEL_KEYS = ("feed", "chunk", "j_offset", "M_total")


def model_kw(c):
    return {k: v for k, v in c["kw"].items() if k in MODEL_KEYS}


# ---- numpy emulations of the kernels' own steps ----------------------------------------------------------------------

f32, f64 = np.float32, np.float64
DEFECTS = ("no-wrap", "no-j-offset", "drop-ragged", "fold-assigns", "scaled-coords", "no-newton", "no-cw-lo", "poly-deg4",
           "matern52-no-t2", "clamp-after-poly", "den-wrong-block")
LOG2E = 1.4426950408889634
HAVE_LONGDOUBLE = np.finfo(np.longdouble).nmant > 52


def _fma(a, b, c):
    """fma in the dtype of a: float32 with the product and sum in float64, rounded once; float64 in longdouble where
    the machine has one."""
    a, b, c = np.asarray(a), np.asarray(b), np.asarray(c)
    if a.dtype == f32:
        return (a.astype(f64) * b.astype(f64) + c.astype(f64)).astype(f32)
    L = np.longdouble
    return (a.astype(L) * b.astype(L) + c.astype(L)).astype(f64)


def _exp2f(v):
    """v_exp_f32: no denormal results."""
    k = np.exp2(v.astype(f64)).astype(f32)
    return np.where(k < f32(2.0 ** -126), f32(0), k)


EXP_TAB = np.exp2(np.arange(64) / 64.0)


def _kexp_neg_f64(v, defect=None):
    """kexp_neg_f64 step by step (fmin returns its other argument for a NaN)."""
    v = np.fmin(v, 800.0)
    n = np.rint(v * -92.332482616893657)
    r = _fma(n, -0.010830424696905538, -v)
    if defect != "no-cw-lo":
        r = _fma(n, 6.563929801064195e-13, r)
    ni = n.astype(np.int64)
    t = EXP_TAB[ni & 63]
    p = np.full_like(r, 1.0 / 24.0) if defect == "poly-deg4" else _fma(r, 1.0 / 120.0, np.full_like(r, 1.0 / 24.0))
    for coeff in (1.0 / 6.0, 0.5, 1.0, 1.0):
        p = _fma(p, r, np.full_like(r, coeff))
    return np.ldexp(t * p, (ni >> 6).astype(np.int32))


def _rsq_estimate(s):
    """v_rsq_f64 taken as 1 / sqrt(s) rounded to 27 bits (|e| <= 2^-26, inside the code's stated 2^-25)."""
    y = 1.0 / np.sqrt(s)
    m, e = np.frexp(y)
    return np.ldexp(np.round(m * 2.0 ** 27) / 2.0 ** 27, e)


def _rsq_step(s, defect=None):
    """(y0, y): the estimate and the third-order step."""
    y0 = _rsq_estimate(s)
    if defect == "no-newton":
        return y0, y0
    e = _fma(-(s * y0), y0, np.ones_like(s))
    return y0, _fma(y0 * e, _fma(e, 0.375, np.full_like(s, 0.5)), y0)


def emulate_kval(kernel, s, defect=None):
    """kval<KERNEL>(s) of kmvp_lowd.hpp in the dtype of s."""
    with np.errstate(all="ignore"):
        if s.dtype == f32:
            if kernel == "gaussian":
                return _exp2f((s * f32(-LOG2E)).astype(f32))
            if kernel == "absolute-exponential":
                return _exp2f((np.sqrt(s) * f32(-LOG2E)).astype(f32))
            if kernel == "inverse-distance":
                return (1.0 / np.sqrt(s.astype(f64))).astype(f32)
            c, ln2 = f32(lm.SQRT_2NU[kernel] * LOG2E), f32(0.6931471805599453)
            raw = (np.sqrt(s) * c).astype(f32)
            a = np.fmin(raw, f32(192.0))
            e = _exp2f(-a)
            if defect == "clamp-after-poly":
                a = raw
            if kernel == "matern-3/2":
                return (_fma(a, ln2, np.ones_like(a)) * e).astype(f32)
            inner = np.full_like(a, ln2) if defect == "matern52-no-t2" else _fma(a, f32(0.6931471805599453 ** 2 / 3.0), np.full_like(a, ln2))
            return (_fma(a, inner, np.ones_like(a)) * e).astype(f32)
        edge = (s == 0) | (s == np.inf)
        if kernel == "gaussian":
            return _kexp_neg_f64(s, defect)
        y0, y = _rsq_step(s, defect)
        if kernel == "inverse-distance":
            return np.where(edge, y0, y)
        r = np.where(edge, s, s * y)
        if kernel == "absolute-exponential":
            return _kexp_neg_f64(r, defect)
        raw = r * lm.SQRT_2NU[kernel]
        t = np.fmin(raw, 800.0)
        ex = _kexp_neg_f64(t, defect)
        if defect == "clamp-after-poly":
            t = raw
        if kernel == "matern-3/2":
            return (1.0 + t) * ex
        inner = np.ones_like(t) if defect == "matern52-no-t2" else _fma(t, 1.0 / 3.0, np.ones_like(t))
        return _fma(t, inner, np.ones_like(t)) * ex


def emulate_sqdist(x, y, path, scale=None):
    """The chain of interact (lowd_kernel: a rounded product, then D - 1 FMAs) or of lowd_mid_kernel / lowd_big_kernel
    (D FMAs from 0; the pad dimensions add exact zeros and are left out)."""
    dt = y.dtype.type
    if scale is not None:                                        # the defect the header warns of: scaled before the subtraction
        x, y = (x * dt(scale)).astype(dt), (y * dt(scale)).astype(dt)
    s = None
    with np.errstate(all="ignore"):
        for d in range(y.shape[1]):
            df = (x[:, d, None] - y[None, :, d]).astype(dt)
            if s is None:
                s = (df * df).astype(dt) if path == "lowd" else _fma(df, df, np.zeros_like(df))
            else:
                s = _fma(df, df, s)
    return s


def _round_up(v, q):
    return -(-v // q) * q


def _fold_points(path, precision, j0, j1, feed, chunk):
    """Source indices (exclusive ends) after which the working-precision sums of a segment [j0, j1) are folded."""
    if precision == f64 and path == "lowd":
        return [j1]
    if path != "lowd":
        step = lm.MID_CHUNK
    else:
        c = _round_up(max(chunk, lm.LOWD_BATCH), lm.LOWD_BATCH)
        step = c if feed == 0 else _round_up(c, lm.LDS_TILE)
    return [min(j, j1) for j in range(j0 + step, j1 + step, step)]


_LAST_VALUES = [None, None, None, None]


def emulate(c, sig, E=None, *, feed=1, chunk=512, segments=1, defect=None):
    """The three kernels' steps in numpy in the working precision: the squared-distance chain, the kernel function, the
    exact rules, the pad records (lowd_kernel), the chains between folds, the folds, the segments -- (N, E) float64."""
    dt = c["precision"].type
    kernel, path = c["kernel"], c["path"]
    y = np.asarray(c["y"], dt)
    x = y if c["x"] is None else np.asarray(c["x"], dt)
    b = signal_of(c, sig, E)
    M, D = y.shape
    N = x.shape[0]
    j_offset, M_total = c["kw"].get("j_offset", 0), c["kw"].get("M_total", M)
    if path == "lowd":                                           # pad records: y = +inf, b = 0
        m_pad = _round_up(max(M, 1), lm.LOWD_BATCH)
        y = np.concatenate((y, np.full((m_pad - M, D), np.inf, dt)))
        b = None if b is None else np.concatenate((b, np.zeros((m_pad - M, b.shape[1]), dt)))
        seg_len = _round_up(-(-m_pad // segments), lm.LOWD_BATCH)
    else:
        m_pad = M
        seg_len = -(-M // segments)
    scale = None
    if defect == "scaled-coords":
        scale = np.sqrt(LOG2E) if kernel == "gaussian" else LOG2E
    key = (id(c["y"]), id(c["x"]), kernel, path, defect)         # (the configurations of one case share its kernel values)
    if _LAST_VALUES[0] != key:
        s = emulate_sqdist(x, y, path, scale)
        if scale is not None:
            s = (s / dt(scale * scale)).astype(dt)               # (so that the kernel function below stays the same)
        _LAST_VALUES[:] = [key, emulate_kval(kernel, s, defect), c["y"], c["x"]]
    k = _LAST_VALUES[1].copy()
    if kernel == "inverse-distance":
        i = np.arange(N)
        g = i if defect == "no-wrap" else i % (M_total + 1)
        jz = np.where(g < M_total, g if defect == "no-j-offset" else g - j_offset, -1)
        hit = (jz >= 0) & (jz < M)
        k[i[hit], jz[hit]] = 0
    last = m_pad
    if defect == "drop-ragged":
        last = M // 4 * 4 if path == "lowd" else None
    cols = 1 if b is None else b.shape[1]
    num, den = np.zeros((N, cols)), np.zeros((N, 1))
    with np.errstate(all="ignore"):
        for j0 in range(0, m_pad, seg_len):
            j1 = min(j0 + seg_len, m_pad)
            stop = j1
            if defect == "drop-ragged":
                stop = min(j1, last) if path == "lowd" else j0 + (j1 - j0) // 8 * 8
            acc, dn = np.zeros((N, cols), dt), np.zeros((N, 1), dt)
            accd, dnd = np.zeros((N, cols)), np.zeros((N, 1))
            folds = set(_fold_points(path, c["precision"].type, j0, j1, feed, chunk))
            for j in range(j0, j1):
                if j < stop:
                    kj = k[:, j, None]
                    if b is None:
                        acc = (acc + kj).astype(dt)
                    else:
                        acc = _fma(np.broadcast_to(kj, acc.shape), np.broadcast_to(b[j][None, :], acc.shape), acc)
                        if sig == "norm":
                            dn = (dn + kj).astype(dt)
                if j + 1 in folds:
                    if defect == "fold-assigns":
                        accd, dnd = acc.astype(f64), dn.astype(f64)
                    else:
                        accd, dnd = accd + acc, dnd + dn
                    acc, dn = np.zeros((N, cols), dt), np.zeros((N, 1), dt)
            num, den = num + accd, den + dnd
        # the clamps of kexp_neg_f64 and of the Matern exponents are fmin, which returns its other argument for a NaN: the
        # kernels restore a NaN target's row when they write it (nan_target in kmvp_lowd.hpp)
        bad = np.isnan(x).any(axis=1)
        num[bad], den[bad] = np.nan, np.nan
        if sig == "norm":
            if defect == "den-wrong-block":                      # the second column block's first column read as the denominator
                den = num[:, LOWD_MAX_E:LOWD_MAX_E + 1]
            return num / den
    return num
