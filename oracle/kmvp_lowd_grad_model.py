"""Float64 model of lowd_grad_kernel and lowd_dscale_kernel -- TEST INFRASTRUCTURE ONLY.

    gradient    G[i, e, d] = c sum_j W(s_ij) b_je  (x_id - y_jd)         (kmvp_lowd_grad.hpp,   kmvp_<kernel>_grad)
    derivative  H[i, e, d] = -c sum_j W(s_ij) b_je (x_id - y_jd)^2       (kmvp_lowd_dscale.hpp, kmvp_<kernel>_dscale)

with W = |w| without its constant (grad_weight) and c = grad_constant: -2 (Gaussian), -1 (exp(-r), 1/r), -3 (Matern 3/2),
-5/3 (Matern 5/2).  The contract is kmvp_lowd_model.py's: `value` is the float64 result on the caller's inputs as rounded
to the working precision (float64 kernels: formed in the machine's extended precision and rounded once; the band is
doubled where np.longdouble has no extra bits), `band` a per-element upper bound derived from the code, term by term,
below; nothing is fitted to kernel output.  Both kernels form s from the caller's own differences and so have relative
accuracy in s: no row is ever flagged.  u = 2^-24 (2^-53); gamma_s, TRANS, EXP64, RSQ64, FLUSH, LAM, K_BAND are
kmvp_lowd_model's, whose docstring derives them.

* df_d = x_d - y_d: one rounding, (1 + u).  It is KEPT: the same df_d enters s and the product, so its rounding is
  counted once in s (inside gamma_s) and once per factor df_d of the product.  A difference below the smallest normal
  number is exact.
* s: interact's chain, |s' - s| <= gamma_s s, gamma_s = (1 + u)^(D + 2) - 1 (+ D eta / s for denormal FMA results).
* W (grad_weight), relative error expm1(L); h = -ln(1 - gamma_s) / 2 >= gamma_s / 2 is what the error of s' does to a
  square root or its reciprocal; Lq = h + TRANS (float32: v_rsq_f32), h + RSQ64 (float64: estimate and one step):
    Gaussian   W = k:  kmvp_lowd_model's L:  s (gamma_s + 2 u) + TRANS   |   s gamma_s + EXP64
    1/r        W = q q q: three factors q and two roundings:                        L = 3 Lq + 2 u
    exp(-r)    W = kval<gaussian>(s q) q.  r' = s' q' = sqrt(s') (1 + rsq's error), one rounding: rho_r = Lq + u;
               float32: the constant f32(-log2 e) and its product, rho = rho_r + 2 u, k: r rho + TRANS;
               float64: k: r rho_r + EXP64; then the factor q and one rounding:
                                                 L = r (Lq + 3 u) + TRANS + Lq + u  |  r (Lq + u) + EXP64 + Lq + u
    Matern     matern_value<.., DEG - 1>: the value's own steps (v_sqrt_f32, resp. r = s y) with the polynomial of ONE
               DEGREE LESS, P_0 = 1 (nu = 3/2), P_1 = 1 + t (nu = 5/2); kmvp_lowd_model's formula at DEG - 1:
                  L = t rho + TRANS + (DEG - 1) rho + 5 u,  rho = gamma_s / 2 + TRANS + 2 u            (float32)
                  L = t rho_t + EXP64 + (DEG - 1) rho_t + 4 u,  rho_t = Lq + 3 u                       (float64)
  float32: v_exp_f32 returns 0 below FLUSH = 2^-126: a pair whose exponential (1 - its bound) may be below FLUSH may be
  lost whole and is charged with its whole term.  float64: an exponent beyond 700 may land in the denormal range:
  P eta absolutely (eta = 2^-1074); exp(-r)'s last product k q may be denormal in either precision: eta more.
* the pair product, each rounding (1 + u), NR roundings on top of W's error, counting the kept df_d once per factor:
    gradient                  wb = w b (none for density), fma(wb, df_d, acc):                NR = 2, density 1
    derivative, E = 1         wb = w b, t = wb df_d, fma(t, df_d, acc): wb, t, df_d twice:    NR = 4, density 3
    derivative, E > 1         u_d = (w df_d) df_d, fma(u_d, b_e, acc): two products, df_d twice:         NR = 4
  (the rounding of the FMA itself belongs to the chain).  An intermediate product that is denormal is off by eta
  absolutely, and reaches the sum multiplied by the factors that follow it: at most eta (1 + |df_d|)^p (1 + |b_e|) per
  pair, p = 1 (gradient), 2 (derivative).
  |term' - term| <= [dW (1 + r_NR) + W r_NR] |b_e| |df_d|^p + that,   r_NR = (1 + u)^NR - 1, dW the bound on |W' - W|.
* the chain.  since_fold += LDS_TILE: the float32 sums are folded into fp64 every `chunk` rounded up to whole tiles of
  256 sources, at the segment's end at the latest: n = kmvp_lowd_model.chain_length("lowd", feed = 1), at most M;
  float64: one chain per segment, n <= M.  Every partial sum is at most the element's mass:
  min(n, LAM sqrt n) u mass.  Folds, segments, reduce_and_finish and the constant are fp64: -2, -3 and -1 are exact,
  -5/3 is a rounded constant and its product one more fp64 rounding: all inside 2^-50 mass.  A denormal FMA result is
  off by eta: M eta per element.
* exact rules, all properties of `value`:
    pad records and pad rows give 0;
    1/r: the pair whose local index is (i mod (M_total + 1)) - j_offset is dropped (kmvp_oracle.zero_column; it wraps);
      a coincident pair that is not dropped is inf * 0: the row is non-finite in every component;
    exp(-r): a pair with s = 0 contributes 0, the own pair of same_points included;
    a pair whose squared distance overflows the working precision although x - y is finite has W = 0 and contributes
      exactly 0 -- in the derivative too, whose squares enter as two factors;
    a NaN target coordinate makes exactly its own row non-finite, in every component (nan_target);
    a source coordinate that is NaN or +-inf is not screened by the kernels: in EVERY row the components of that axis
      (every e) are non-finite; a NaN entry of b makes its column non-finite in every row and component.  Such
      elements are `poisoned`.  The source's W is 0 (s = inf, or the clamps' answer to a NaN) or NaN, so an element that
      is not poisoned is either non-finite too (float32 Gaussian, exp(-r), 1/r on a NaN: v_exp_f32 / v_rsq_f32 pass the
      NaN on) or holds the sum over the other sources: `value` and `band` are those of the other sources.
* mass[i, e, d] = |c| sum_j W |b_je| |x_d - y_d|^p.
band = K_BAND (|c| pair + acc), K_BAND = 2 over the second-order terms the bounds drop.

Preconditions, RAISED (the kernels are not wrong there, the model does not cover them): every non-zero squared distance
of finite points is a normal number of the working precision (exp(-r): positive_normal treats a denormal s as
coincident -- a hard precondition); 1/r: r^-3 is a normal, finite number of the working precision; no target coordinate
is +-inf.  A squared distance that overflows is NOT an error here: it is the exact rule above.

Parity status: no reference counterpart; with rounding disabled `value` equals tests/grad_reference.py,
tests/dscale_reference.py and tests/matern_reference.py (tests/test_lowd_grad_model.py).
"""
from collections import namedtuple

import numpy as np

import kmvp_lowd_model as lm
import kmvp_oracle
from kmvp_f32_model import FLUSH
from kmvp_lowd_model import DENORMAL_FROM, ETA64, EXP64, HAVE_LONGDOUBLE, K_BAND, LAM, RSQ64, SQRT_2NU, TRANS, unit

KERNELS = lm.KERNELS
DSCALE_KERNELS = tuple(k for k in KERNELS if k != "inverse-distance")
CONSTANT = {"gaussian": -2.0, "absolute-exponential": -1.0, "inverse-distance": -1.0, "matern-3/2": -3.0,
            "matern-5/2": -5.0 / 3.0}
DEG_W = {"matern-3/2": 0, "matern-5/2": 1}       # the weight's polynomial: one degree less than the value's

GradModel = namedtuple("GradModel", "value band mass pair acc nonfinite poisoned")


def weights(kernel, s):
    """W(s) = |w| without its constant, in the dtype of s: 0 at s = inf; exp(-r): 0 at s = 0; 1/r: inf at s = 0."""
    one = s.dtype.type(1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        r = np.sqrt(s)
        if kernel == "gaussian":
            return np.exp(-s)
        if kernel == "absolute-exponential":
            return np.where((s > 0) & np.isfinite(s), np.exp(-r) / np.where(s > 0, r, one), 0)
        if kernel == "inverse-distance":
            return one / (s * r)
        t = np.sqrt(s.dtype.type(3 if kernel == "matern-3/2" else 5)) * r
        p = one if kernel == "matern-3/2" else one + t
        return np.where(np.isinf(s), 0, p * np.exp(-t))


def roundings(dscale, E, density):
    """NR of the docstring."""
    if not dscale:
        return 1 if density else 2
    return 3 if density else 4


def weight_bound(kernel, precision, s, W, D):
    """Upper bound on |W' - W| of one pair from the squared distance s and the exact weight W (float64, (n, M))."""
    f32 = np.dtype(precision) == np.float32
    u = unit(precision)
    eta = 2.0 ** -150 if f32 else ETA64
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        live = np.isfinite(s) & (s > 0)
        ss = np.where(live, s, 1.0)
        gs = np.where(live, np.expm1((D + 2) * np.log1p(u)) + D * eta / ss, 0.0)
        h = -0.5 * np.log1p(-gs)
        r = np.sqrt(ss)
        ex, absolute = None, 0.0
        if f32:
            Lq = h + TRANS
            if kernel == "gaussian":
                L, ex = ss * (gs + 2 * u) + TRANS, np.exp(-ss)
            elif kernel == "inverse-distance":
                L = 3 * Lq + 2 * u
            elif kernel == "absolute-exponential":
                L, ex, absolute = r * (Lq + 3 * u) + TRANS + Lq + u, np.exp(-r), eta
            else:
                t = SQRT_2NU[kernel] * r
                rho = gs / 2 + TRANS + 2 * u
                L, ex = t * rho + TRANS + DEG_W[kernel] * rho + 5 * u, np.exp(-t)
            at_zero = TRANS + 5 * u
        else:
            Lq = h + RSQ64
            arg, poly = None, 1.0
            if kernel == "gaussian":
                L, arg = ss * gs + EXP64, ss
            elif kernel == "inverse-distance":
                L = 3 * Lq + 2 * u
            elif kernel == "absolute-exponential":
                L, arg, poly = r * (Lq + u) + EXP64 + Lq + u, r, 1.0 / r
            else:
                t = SQRT_2NU[kernel] * r
                rho_t = Lq + 3 * u
                L, arg = t * rho_t + EXP64 + DEG_W[kernel] * rho_t + 4 * u, t
                poly = 1.0 if kernel == "matern-3/2" else 1.0 + t
            if arg is not None:
                absolute = np.where(live & (arg > DENORMAL_FROM), poly * ETA64, 0.0)
            if kernel == "absolute-exponential":
                absolute = absolute + ETA64
            at_zero = EXP64 + 4 * u
        L = np.where(live, np.minimum(L, 700.0), at_zero if kernel != "inverse-distance" else 0.0)
        rel = np.expm1(L)
        Wf = np.where(np.isfinite(W), W, 0.0)
        each = np.where(Wf > 0, Wf * rel, 0.0) + np.where(live, absolute, 0.0)
        if ex is not None:                                    # v_exp_f32 returns 0 below the smallest normal number
            each = np.where(live & (ex * (1.0 - rel) < FLUSH), np.maximum(each, Wf), each)
    return each


def check_preconditions(kernel, precision, s, W):
    info = np.finfo(np.dtype(precision))
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(s) & (s > 0)
        if (fin & (s < info.tiny)).any():
            raise ValueError("a non-zero squared distance is below the smallest normal number of the working precision")
        if kernel == "inverse-distance" and (fin & ((W < info.tiny) | (W > info.max))).any():
            raise ValueError("1/r^3 of a pair is not a normal, finite number of the working precision")


def lowd_gradient(kernel, y, x=None, b=None, *, precision=np.float32, dscale=False, chunk=512, rows=None, j_offset=0,
                  M_total=None, rounding=True):
    """Modelled result of kmvp_<kernel>_grad (dscale=False) or kmvp_<kernel>_dscale (dscale=True) and its band.

    y (M, D) sources, x (N, D) targets (None: the same points), b (M, E) signal (None: density estimation), all rounded
    to `precision` first.  chunk: the "chunk" option.  j_offset / M_total: y is a slice of the sources (1/r's zero rule).
    rows: target indices to model.  rounding=False: the float64 value, no band.
    Returns GradModel(value, band, mass, pair, acc (n, E, D) each, nonfinite (n,), poisoned (n, E, D))."""
    if kernel not in (DSCALE_KERNELS if dscale else KERNELS):
        raise ValueError(kernel)
    precision = np.dtype(precision)
    y = np.asarray(y, dtype=precision).astype(np.float64)
    xa = y if x is None else np.asarray(x, dtype=precision).astype(np.float64)
    if np.isinf(xa).any():
        raise ValueError("an infinite target coordinate is not covered by the model")
    rows = np.arange(xa.shape[0], dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    M, D = y.shape
    density = b is None
    b = np.ones((M, 1)) if density else np.asarray(b, dtype=precision).astype(np.float64)
    block = max(1, 2 ** 21 // max(1, M * D))
    n_chain = lm.chain_length("lowd", precision, M, chunk, 1)
    parts = [_block(kernel, y, xa[rows[r0:r0 + block]], rows[r0:r0 + block], b, density, dscale, precision, n_chain, j_offset,
                    M if M_total is None else M_total, rounding) for r0 in range(0, max(len(rows), 1), block)]
    return GradModel(*(np.concatenate(f) for f in zip(*parts)))


def _block(kernel, y, x, rows, b, density, dscale, precision, n_chain, j_offset, M_total, rounding):
    M, D = y.shape
    E = b.shape[1]
    n = len(rows)
    p = 2 if dscale else 1
    c = CONSTANT[kernel]
    wide = precision == np.float64 and HAVE_LONGDOUBLE
    Wt = np.longdouble if wide else np.float64
    # non-finite inputs: the exact rules.  The sums run over the clean sources and signal entries only.
    bad_src = ~np.isfinite(y)                                   # (M, D)
    bad_b = ~np.isfinite(b)                                     # (M, E)
    nan_row = np.isnan(x).any(axis=1)
    yc = np.where(bad_src.any(axis=1, keepdims=True), 0.0, y)
    bc = np.where(bad_b, 0.0, b) * (~bad_src.any(axis=1))[:, None]
    xc = np.where(nan_row[:, None], 0.0, x)
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        df = xc.astype(Wt)[:, None, :] - yc.astype(Wt)[None, :, :]          # (n, M, D)
        sw = (df * df).sum(axis=2)
        ww = weights(kernel, sw)
        dropped = np.broadcast_to(bad_src.any(axis=1)[None, :], sw.shape).copy()   # pairs that enter no sum
        if kernel == "inverse-distance":
            jz = kmvp_oracle.zero_column(rows, M_total) - j_offset
            hit = (jz >= 0) & (jz < M)
            dropped[np.nonzero(hit)[0], jz[hit]] = True
        ww = np.where(dropped, 0, ww)
        coincident = np.isinf(ww).any(axis=1)                   # 1/r: a pair at s = 0 that is not dropped
        ww = np.where(np.isinf(ww), 0, ww)
        fac = df * df if dscale else df
        value = ((-c if dscale else c) * np.einsum("nm,me,nmd->ned", ww, bc.astype(Wt), fac)).astype(np.float64)
        s, W = sw.astype(np.float64), ww.astype(np.float64)
        adf = np.abs(df.astype(np.float64))
    nonfinite = nan_row | coincident
    poisoned = np.zeros((n, E, D), dtype=bool)
    poisoned[nonfinite] = True
    poisoned[:, :, bad_src.any(axis=0)] = True
    poisoned[:, bad_b.any(axis=0), :] = True
    value[poisoned] = np.nan
    babs = np.abs(bc)
    apow = adf * adf if dscale else adf
    mass = abs(c) * np.einsum("nm,me,nmd->ned", W, babs, apow)
    z = np.zeros_like(mass)
    if not rounding:
        return GradModel(value, z, mass, z, z, nonfinite, poisoned)
    ok = ~nonfinite
    check_preconditions(kernel, precision, np.where(dropped, np.inf, s)[ok], W[ok])
    u = unit(precision)
    eta = 2.0 ** -150 if precision == np.float32 else ETA64
    # a squared distance that overflows whatever its roundings: s' = inf, W' = 0 and every product an exact 0
    over = s * (1.0 - np.expm1((D + 2) * np.log1p(u))) > float(np.finfo(precision).max)
    dropped = dropped | over
    each = np.where(dropped, 0.0, weight_bound(kernel, precision, s, W, D))
    r_nr = np.expm1(roundings(dscale, E, density) * np.log1p(u))
    live = (~dropped).astype(np.float64)
    pair = np.einsum("nm,me,nmd->ned", each * (1 + r_nr) + W * r_nr, babs, apow)
    pair = pair + eta * np.einsum("nm,me,nmd->ned", live, 1.0 + babs, (1.0 + adf) ** p)
    acc_rel = min(n_chain, LAM * np.sqrt(n_chain)) * u + 2.0 ** -50
    acc = acc_rel * mass + M * eta
    own = 1.0 if wide or precision == np.float32 else 2.0          # float64 without an extended type: the value's own error
    band = own * K_BAND * (abs(c) * pair + acc)
    return GradModel(value, band, mass, abs(c) * pair, acc, nonfinite, poisoned)
