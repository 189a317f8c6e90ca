"""Float64 model of the pair-loop products in the difference form -- TEST INFRASTRUCTURE ONLY.

lowd_kernel, lowd_mid_kernel and lowd_big_kernel (kmvp_lowd.hpp; run_product_t, run_product_blocked) form every squared
distance from the caller's own coordinates, s = sum_d (x_d - y_d)^2, and so have RELATIVE accuracy in s everywhere: there
is no split, no expansion, no centre and no grouping to bound, and no row is ever flagged on finite inputs.  The contract
is that of kmvp_f32mm_model.py and kmvp_f32_model.py: `value` is the float64 product of the caller's inputs as rounded to
the working precision, `band` a per-element upper bound derived from the code, term by term, below; nothing is fitted to
kernel output.  (u = 2^-24 in float32, 2^-53 in float64: one rounding to nearest.)

* s.  interact (lowd_kernel): df = x_d - y_d (one rounding each), s = df_0 df_0 (one rounding), then D - 1 FMAs
  s = fma(df, df, s) (one rounding each).  Every term is non-negative, so the D roundings of the chain and the two
  roundings inside a term compound to |s' - s| <= ((1 + u)^(D + 2) - 1) s =: gamma_s s.  lowd_mid_kernel starts from
  s = 0 and runs 8 DCH FMAs: the first is a rounded product, the pad dimensions add fma(0, 0, s) = s exactly: the same
  D roundings.  lowd_big_kernel carries s across its chunks of 32 in a register: the same chain again.  An FMA whose
  result is denormal adds eta = 2^-150 (2^-1075) absolutely: D eta / s more, at most D u where s is a normal number.
* kernel value, float32 (kval(float), matern_value(float)); every v_exp_f32 / v_sqrt_f32 / v_rsq_f32 taken at TRANS = 2 ulp:
    Gaussian   kexp2(s * f32(-log2 e)): the constant and the product, 2 u                 L = s (gamma_s + 2 u) + TRANS
    exp(-r)    kexp2(v_sqrt(s) * f32(-log2 e)): rho = gamma_s / 2 + TRANS + 2 u           L = r rho + TRANS
    1/r        v_rsq(s)                                                                   L = -ln(1 - gamma_s) / 2 + TRANS
    Matern     a = min(v_sqrt(s) * f32(sqrt(2 nu) log2 e), 192) is the exponent in binades, relative error rho as above;
               e = kexp2(-a); the polynomial P_1 = fma(a, ln2, 1), P_2 = fma(a, fma(a, ln2^2 / 3, ln2), 1) is taken in a
               (positive terms: DEG rho from a, one u per constant and per FMA), then one multiply:
                                                                                          L = t rho + TRANS + DEG rho + 5 u
               (t = sqrt(2 nu) r.)  The clamp at 192 binades changes no result: v_exp_f32 returns 0 from 2^-126 down.
  Relative error of k: expm1(L).  kexp2 is the bare v_exp_f32, which returns 0 for a result below FLUSH = 2^-126: a pair
  whose exponential (1 - its bound) may be below FLUSH may be lost whole and is charged with k itself, as in
  kmvp_f32_model (for the Matern kernels the exponential is e^-t, not k = P e^-t).
* kernel value, float64.  kexp_neg_f64(v) for v >= 0:
    the clamp at 800: e^-800 = 2^-1154 is 0 in float64, as is the exact value from v ~ 745.2 on: covered by the
      denormal term below;
    n = rint(-64 v / ln 2); r = fma(n, -hi, -v) is exact (hi = ln2/64 to 30 bits: n hi is exact and the difference of
      two neighbours fits), r = fma(n, lo, r): one rounding of |r| <= ln2/128 and the rounding of lo itself, together
      below 2^-7 u (the header's "exact to ~1e-19");
    the table 2^(j/64) from the device's exp2 at 2 ulp: 4 u;
    the degree-5 Taylor polynomial: truncation (ln2/128)^6 / 720 = 3.5e-17 (0.32 u) and its Horner roundings
      u (1 + |r| + ...) <= 1.01 u;
    t * p: u;  ldexp: exact, except into the denormal range (v > 708): 2^-1075 absolutely per pair.
  EXP64 = 4 u + 3.6e-17 + 1.01 u + u + 2^-7 u (6.3 u; a numpy restatement without true FMAs measures 2.9 ulp = 5.8 u
  on [0, 700] -- an anchor, not the tolerance).
  1/sqrt(s): y0 = v_rsq_f64(s), e = fma(-s y0, y0, 1), y = fma(y0 e, fma(e, 3/8, 1/2), y0) = y0 (1 + e/2 + 3 e^2/8).
  ASSUMPTION (the code's own statement): |e| <= 2^-25.  Then the dropped term is 5 e^3 / 16 <= 2^-76; the rounding of
  s y0 enters e absolutely with u, hence y with u / 2; the last FMA: u; the two roundings inside, each times |e|:
  RSQ64 = 1.5 u + 2^-23 u + 2^-76.  s = 0 and s = inf pass through (1/r: inf and 0 from the estimate itself;
  exp(-r) and Matern: kexp_neg_f64(0) = 1, kexp_neg_f64(inf) = 0).
    Gaussian   L = s gamma_s + EXP64
    exp(-r)    r = s y: rho = gamma_s / 2 + RSQ64 + u                                     L = r rho + EXP64
    1/r        L = -ln(1 - gamma_s) / 2 + RSQ64
    Matern     t = min(r sqrt(2 nu), 800): rho_t = rho + 2 u; (1 + t) resp. fma(t, fma(t, 1/3, 1), 1), one multiply:
                                                                                          L = t rho_t + EXP64 + DEG rho_t + 4 u
  and P(t) 2^-1075 absolutely for every pair with an exponent beyond 700.
* exact rules.  1/r: the pair whose local source index is the target's flat index mod (M_total + 1), less j_offset, has
  k = 0 (kmvp_oracle.zero_column; it wraps when N > M_total + 1).  Pad records (y = +inf, b = 0) and pad rows give k = 0
  exactly.  A coincident off-diagonal 1/r pair has k = inf in the kernels (v_rsq of 0) as in the reference: the row is
  non-finite.  An infinite coordinate gives s = inf and k = 0; a NaN coordinate gives a NaN row.  All of these are
  properties of `value`.
* accumulation.  float32: acc = fma(k, b, acc) (density: acc += k) in fp32 between folds into fp64 -- a chain of
  n = `chunk` sources (lowd_kernel, the scalar-cache feed; rounded up to the ping-pong of 8), `chunk` rounded up to whole
  tiles of LDS_TILE = 256 (lowd_kernel, the LDS feed), MID_CHUNK = 64 (lowd_mid_kernel, lowd_big_kernel), at most M.
  Every partial sum is at most the row's mass sum_j k |b_j|: |error| <= min(n, lam sqrt n) u mass -- the
  deterministic bound, or the probabilistic rule of kmvp_f32mm_model (Higham and Mary 2019, Thm 2.4, lam = 8) where that
  is smaller.  float64: one fp64 chain per segment, n = M.  The folds, segments, column blocks and shards are added in
  fp64: 2^-50 mass.  The library is built with denormals on: a denormal FMA result is off by at most eta, M eta a row.
* value.  float32: the float64 product.  float64: numpy's float64 evaluation of exp(-s) is itself off by about s D u, as
  much as the kernels, so the product is formed in the machine's extended precision (x87: u = 2^-64) and rounded to
  float64 once; where there is no such type the band is doubled for the value's own error.
* normalised rows: the denominator is the same chain with b = 1; kmvp_f32_model's formula
  band = (band_num + |value| band_den) / (den - band_den).

band = K_BAND (pair + acc), K_BAND = 2 over the upper bounds for the second-order terms they drop.

Preconditions, checked and RAISED (not flagged: the kernels are not wrong there, the model just does not cover them):
  every non-zero squared distance of finite points is a normal number of the working precision and does not overflow;
  a normalised row's denominator stays above its own band (float32 rows all of whose pairs may be flushed are 0 / 0 in
  the kernels).
Known limit, not modelled and not tested: float32 v_rsq_f32 / v_sqrt_f32 do not take denormal inputs; the reference does.

Parity status: no reference counterpart; checked against kmvp_oracle.product and tests/matern_reference.py with rounding
disabled by tests/test_lowd_model.py.
"""
import numpy as np

import kmvp_oracle
from kmvp_f32_model import FLUSH
from kmvp_f32mm_model import K_BAND, LAM, TRANS, U_RNE, Model

KERNELS = ("gaussian", "absolute-exponential", "inverse-distance", "matern-3/2", "matern-5/2")
SQRT_2NU = {"matern-3/2": 1.7320508075688772, "matern-5/2": 2.23606797749979}
DEG = {"matern-3/2": 1, "matern-5/2": 2}
U64 = 2.0 ** -53
ETA64 = 2.0 ** -1074         # the denormal step: the rounding 2^-1075 is not a float64, so a whole step is charged
LDS_TILE, MID_CHUNK, LOWD_BATCH = 256, 64, 8
EXP64 = 4 * U64 + 1.01 * (np.log(2.0) / 128) ** 6 / 720 + 1.01 * U64 + U64 + 2.0 ** -7 * U64
RSQ64 = 1.5 * U64 + 2.0 ** -23 * U64 + 2.0 ** -76
HAVE_LONGDOUBLE = np.finfo(np.longdouble).nmant > 52
DENORMAL_FROM = 700.0      # exponents from here on may land in the float64 denormal range (708, less every bound on them)


def unit(precision):
    return U_RNE if np.dtype(precision) == np.float32 else U64


def chain_length(path, precision, M, chunk=512, feed=1):
    """Roundings of the longest chain a row's sum passes through in the working precision."""
    if np.dtype(precision) == np.float64:
        return max(M, 1)
    if path == "lowd":
        c = -(-max(chunk, LOWD_BATCH) // LOWD_BATCH) * LOWD_BATCH
        n = c if feed == 0 else -(-c // LDS_TILE) * LDS_TILE
    else:
        n = MID_CHUNK
    return max(1, min(n, M))


def kernel_values(kernel, s):
    """k(s) in the dtype of s: exp(-inf) = 1/inf = 0, the Matern kernels exactly 0 at s = inf, NaN stays NaN."""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        if kernel == "gaussian":
            return np.exp(-s)
        if kernel == "absolute-exponential":
            return np.exp(-np.sqrt(s))
        if kernel == "inverse-distance":
            return 1 / np.sqrt(s)
        t = np.sqrt(s.dtype.type(3 if kernel == "matern-3/2" else 5)) * np.sqrt(s)
        p = 1 + t if kernel == "matern-3/2" else 1 + t + t * t / 3
        return np.where(np.isinf(s), s.dtype.type(0), p * np.exp(-t))


def pair_bound(kernel, precision, s, k, D):
    """Upper bound on |k' - k| of one pair from the squared distance s and the exact value k (both float64, (n, M))."""
    f32 = np.dtype(precision) == np.float32
    u = unit(precision)
    eta = 2.0 ** -150 if f32 else ETA64
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        live = np.isfinite(s) & (s > 0)
        ss = np.where(live, s, 1.0)
        gs = np.where(live, np.expm1((D + 2) * np.log1p(u)) + D * eta / ss, 0.0)
        r = np.sqrt(ss)
        absolute = 0.0
        if f32:
            rho = gs / 2 + TRANS + 2 * u
            if kernel == "gaussian":
                L, ex = ss * (gs + 2 * u) + TRANS, np.exp(-ss)
            elif kernel == "absolute-exponential":
                L, ex = r * rho + TRANS, np.exp(-r)
            elif kernel == "inverse-distance":
                L, ex = -0.5 * np.log1p(-gs) + TRANS, None
            else:
                t = SQRT_2NU[kernel] * r
                L, ex = t * rho + TRANS + DEG[kernel] * rho + 5 * u, np.exp(-t)
        else:
            rho = gs / 2 + RSQ64 + u
            if kernel == "gaussian":
                L, arg, poly = ss * gs + EXP64, ss, 1.0
            elif kernel == "absolute-exponential":
                L, arg, poly = r * rho + EXP64, r, 1.0
            elif kernel == "inverse-distance":
                L, arg, poly = -0.5 * np.log1p(-gs) + RSQ64, None, 1.0
            else:
                t = SQRT_2NU[kernel] * r
                rho = rho + 2 * u
                L, arg = t * rho + EXP64 + DEG[kernel] * rho + 4 * u, t
                poly = 1.0 + t if kernel == "matern-3/2" else 1.0 + t + t * t / 3.0
            if arg is not None:
                absolute = np.where(live & (arg > DENORMAL_FROM), poly * ETA64, 0.0)
        if not f32 and kernel != "inverse-distance":   # s = 0 passes through: the table's entry 0 and the polynomial at r = 0
            L = np.where(s == 0, EXP64, L)
        rel = np.expm1(np.where(live | (s == 0), L, 0.0))
        kf = np.where(np.isfinite(k), k, 0.0)
        each = kf * rel + absolute
        if f32 and ex is not None:                      # v_exp_f32 returns 0 below the smallest normal number
            each = np.where(live & (ex * (1.0 - rel) < FLUSH), np.maximum(each, kf), each)
    return each


def check_preconditions(precision, s):
    info = np.finfo(np.dtype(precision))
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(s) & (s > 0)
        if (fin & (s < info.tiny)).any():
            raise ValueError("a non-zero squared distance is below the smallest normal number of the working precision")
        if (fin & (s > info.max)).any():
            raise ValueError("a squared distance of finite points overflows the working precision")


def lowd_product(kernel, y, x=None, b=None, normalize_rows=False, *, precision=np.float32, path="lowd", feed=1, chunk=512,
                 rows=None, j_offset=0, M_total=None, rounding=True):
    """Modelled result of run_product_t / run_product_blocked in the difference form and its per-element band.

    kernel: one of KERNELS.  y (M, D) sources, x (N, D) targets (None: the same points), b (M, E) signal (None: density
    estimation), all rounded to `precision` first.  path: "lowd" (lowd_kernel), "mid" or "big"; feed: lowd_kernel's
    source feed (0 the scalar-cache feed, 1 LDS tiles); chunk: the "chunk" option.  j_offset / M_total: y is a slice of
    the sources.  rows: target indices to model.  rounding=False: the float64 product, no band.
    Returns Model(value, band, mass, pair, tsplit, bsplit, acc (n, E) each, flagged (n,), nonfinite (n,)); tsplit, bsplit
    and flagged are zero / False: these kernels split nothing and no row is ever flagged."""
    if kernel not in KERNELS or path not in ("lowd", "mid", "big"):
        raise ValueError((kernel, path))
    precision = np.dtype(precision)
    y = np.asarray(y, dtype=precision).astype(np.float64)
    xa = y if x is None else np.asarray(x, dtype=precision).astype(np.float64)
    rows = np.arange(xa.shape[0], dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    M, D = y.shape
    if b is None and normalize_rows:
        raise ValueError("normalised density rows are ones by definition: no kernel runs")
    b = np.ones((M, 1)) if b is None else np.asarray(b, dtype=precision).astype(np.float64)
    block = max(1, 2 ** 22 // max(1, M * D))
    n_chain = chain_length(path, precision, M, chunk, feed)
    parts = [_block(kernel, y, xa[rows[r0:r0 + block]], rows[r0:r0 + block], b, normalize_rows, precision, n_chain, j_offset,
                    M if M_total is None else M_total, rounding) for r0 in range(0, max(len(rows), 1), block)]
    return Model(*(np.concatenate(f) for f in zip(*parts)))


def _block(kernel, y, x, rows, b, normalize_rows, precision, n_chain, j_offset, M_total, rounding):
    M, D = y.shape
    n = len(rows)
    # float64 kernels: numpy's own float64 evaluation of exp(-s) is off by about s D u, as much as the kernels are, so
    # the value is formed in extended precision where the machine has one (and the band doubled where it has none)
    wide = precision == np.float64 and HAVE_LONGDOUBLE
    W = np.longdouble if wide else np.float64
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        sw = kmvp_oracle.sqdists_block(x.astype(W), y.astype(W), False)
        kw = kernel_values(kernel, sw)
        if kernel == "inverse-distance":
            jz = kmvp_oracle.zero_column(rows, M_total) - j_offset
            hit = (jz >= 0) & (jz < M)
            kw[np.nonzero(hit)[0], jz[hit]] = 0
            sw[np.nonzero(hit)[0], jz[hit]] = np.inf               # the dropped pair: nothing to bound
        num = (kw @ b.astype(W))
        den = kw.sum(axis=1, keepdims=True)
        value = (num / den if normalize_rows else num).astype(np.float64)
        num, den, s, k = num.astype(np.float64), den.astype(np.float64), sw.astype(np.float64), kw.astype(np.float64)
    kf = np.where(np.isfinite(k), k, 0.0)
    babs = np.abs(b)
    mass = kf @ babs
    nonfinite = ~np.isfinite(value).all(axis=1)
    flagged = np.zeros(n, dtype=bool)
    z = np.zeros_like(num)
    if not rounding:
        return Model(value, z, mass / den if normalize_rows else mass, z, z, z, z, flagged, nonfinite)
    check_preconditions(precision, s[~nonfinite])
    u = unit(precision)
    eta = 2.0 ** -150 if precision == np.float32 else ETA64
    each = pair_bound(kernel, precision, s, k, D)
    acc_rel = min(n_chain, LAM * np.sqrt(n_chain)) * u + 2.0 ** -50
    pair = each @ babs
    acc = acc_rel * mass + M * eta
    own = 1.0 if wide or precision == np.float32 else 2.0          # float64 without an extended type: the value's own error
    band_num = own * K_BAND * (pair + acc)
    if not normalize_rows:
        return Model(num, band_num, mass, pair, z, z, acc, flagged, nonfinite)
    ksum = kf.sum(axis=1, keepdims=True)
    bden = own * K_BAND * (each.sum(axis=1, keepdims=True) + acc_rel * ksum + M * eta)
    room = den - bden
    if not (room[~nonfinite] > 0).all():
        raise ValueError("a normalised row's denominator does not stay above its own band (every pair may be flushed)")
    with np.errstate(divide="ignore", invalid="ignore"):
        band = (band_num + np.abs(value) * bden) / room
        return Model(value, band, mass / den, pair / den, z, z, acc / den, flagged, nonfinite)
