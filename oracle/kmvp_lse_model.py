"""Float64 model of the log-sum-exp kernels and of their gradient -- TEST INFRASTRUCTURE ONLY.

    L[i, e]    = log sum_j exp(l_ij + c_je)                       lowd_lse_kernel (kmvp_lowd_lse.hpp), lse_reduce_kernel,
                                                                  finish_lse_kernel; lowd_batch_lse_kernel (feed = 0)
    G[i, e, :] = sum_j p_ij^e g_ij,  p = softmax_j(l_ij + c_je)   lowd_lse_grad_kernel (kmvp_lowd_lse_grad.hpp),
                                                                  lse_grad_reduce_kernel, lse_grad_value
    gaussian l = -s, g = -2 (x - y);   exp(-r) l = -r, g = -(x - y) / r;   s = |x - y|^2, r = sqrt(s)

The contract is kmvp_lowd_model.py's and kmvp_lowd_grad_model.py's: `value` is the result on the caller's inputs as rounded
to the working precision, formed in the machine's extended precision and rounded to float64 once (the band is doubled
where np.longdouble has no extra bits); `band` is a per-element upper bound derived from the code, term by term, below;
nothing is fitted to kernel output.  u = 2^-24 (float32), 2^-53 (float64); u64 = 2^-53; gamma_s, TRANS, EXP64, RSQ64, FLUSH,
LAM, K_BAND, LDS_TILE, LOWD_BATCH and chain_length are kmvp_lowd_model's, whose docstring derives them.

Every sum of these kernels is a sum of POSITIVE weights w_j = 2^(u_j - m) at one scale 2^m per (target, column); the
rescales between scales are exact powers of two.  So the errors below are RELATIVE errors eps_j of the single weights,
and they turn into an ABSOLUTE error of L: that is why the band has no factor max(1, |L|).

* the logit in log2 units, u_j = log2(e) (c_j - nl_j) (lse_logits; the gradient's batch step restates it):
    s: interact's chain, |s' - s| <= gamma_s s, gamma_s = (1 + u)^(D + 2) - 1 (+ D eta / s for denormal FMA results);
    nl = lse_neg_logit(s): Gaussian s itself, rho_nl = gamma_s.  exp(-r): h = -ln(1 - gamma_s) / 2 is what the error of s
      does to a square root; float32 v_sqrt_f32 at TRANS: rho_nl = h + TRANS; float64 r = s y with y the rsq estimate and
      its one correction step (RSQ64) and one multiply: rho_nl = h + RSQ64 + u.  s = 0 and s = inf pass through exactly.
    t = c - nl: one rounding, u |c - nl| (density: no subtraction, no rounding);
    t * LOG2E: the constant rounded to the working precision and the product: 2 u |c - nl|.
  In natural-log units (the factor ln 2 log2(e) = 1):  d_j = nl rho_nl + 3 u |c - nl|   (density: nl rho_nl + 2 u nl).
  These grow with |c| + nl: absolute errors of the logit that no exponent shift can undo.
* the weight 2^-(a), a = m - u' >= 0 with the shift m in force when the pair is added (a is at most its value at the final
  shift, a_j = m_final - u_j, and the kernel's final shift is at most one above ceil(max_j u_j): a_j + 1 is used):
    a = m - u': one rounding, u a binades = ln2 u a;
    float32 v_exp_f32 at TRANS;  float64 kexp_neg_f64(a * ln2) at EXP64, the constant ln 2 and the product: 2 u a ln2.
  eps_j = d_j + ln2 (a_j + 1) u [3 u in float64] + TRANS [EXP64];  |w' - w| <= w expm1(eps_j).
  float32: v_exp_f32 returns 0 below FLUSH = 2^-126: a weight that may be below it is lost whole and charged with itself.
  float64: a result in the denormal range (a ln2 > 700) is charged with itself too (it is below 2^-1009 of Z).
* the shift.  m = ceil(bmax) per batch of four is an integer held exactly in the working precision (every float32 from 2^24
  on is an integer) and ldexp by m - m' is exact -- except
    a float32 (float64) sum rescaled into the denormal range: ldexp rounds it to a multiple of 2^-149 (2^-1074) or the
      hardware flushes it: at most FLUSH (2^-1022) per rescale, at most one rescale per batch: ceil(M / 4) of them;
    the clamp of the exponent: float32 `acc` times 2^-300 is exactly 0 where the true factor is smaller still -- the sum
      was at most 256 ceil(chunk / 256), so less than 2^-280 is lost; its fp64 partner keeps accd 2^-300 where less is
      due: accd <= M, at most M 2^-300 stays.  float64 at -4000: ldexp gives exactly 0, the true value is below
      M 2^-4000, which is not a float64.
  All of these are absolute at a scale at which the finished sum is Z >= 1/2 (the largest weight is in (1/2, 1] at the
  final shift), i.e. relative to Z they are at most twice themselves:
      SHIFT = 2 (ceil(M / 4) FLUSH + (M + 1) 2^-280)   (float32),   2 ceil(M / 4) 2^-1022   (float64).
* accumulation.  Z is a sum of positive terms: min(n, LAM sqrt n) u Z with n = chain_length("lowd", feed) roundings
  in the working precision -- the LDS feed (feed = 1) advances since_fold by whole tiles, so the chain is `chunk` rounded
  up to tiles of 256; the scalar-cache feed of lowd_batch_lse_kernel (feed = 0) folds every `chunk` rounded up to 8;
  float64 keeps one chain of M.  The folds and the segment merge are fp64 additions of positive terms, the merge's
  ldexp factors exact: (folds + segments) u64 Z, with at most ceil(M / 8) + 1 folds and at most ceil(M / 8) segments:
  ADD64 = (M / 4 + 2) u64.
* the finish, lse_value = (log2(sum) - k) ln 2.  No documentation shipped with the math library states a bound for the device's
  fp64 log2.  ASSUMPTION: 2 ulp = 4 u64 relative, the figure the other models charge the device's exp2 in the table term.
  1/2 <= sum <= M + 1, so |log2(sum)| <= log2(M + 1) + 1: 4 u64 ln2 (log2(M + 1) + 1) in L; the subtraction u64 |L|, the
  rounded constant and the product 2 u64 |L|:   FINISH = 4 u64 ln2 (log2(M + 1) + 1) + 3 u64 |L|.
  rho_Z = K_BAND (sum_j w_j expm1(eps_j) / Z + ACC + ADD64 + SHIFT);   band(L) = -ln(1 - rho_Z) + FINISH   (inf if rho_Z >= 1).
  That form is the one the gradient's quotient needs, but it is useless once eps_j is not small (logits of -1e20:
  eps_j ~ 1e4): rho_Z >= 1.  The weights are POSITIVE and each is off by a factor e^(+-eps_j), a lost one by a factor in
  [0, e^eps_j], so the sum of the perturbed weights lies between sum_j w_j e^-eps_j (lost ones left out) and
  sum_j w_j e^eps_j whatever the size of eps_j, and the rounded sum of positive terms is that times 1 +- (ACC + ADD64 +
  SHIFT):
      PAIR = max( ln(sum_j w_j e^eps_j / Z),  -ln(sum_{j not lost} w_j e^-eps_j / Z) )   <= max_j eps_j
      band(L) = min( the form above,  K_BAND (PAIR - ln(1 - ACC - ADD64 - SHIFT)) ) + FINISH,
  evaluated in the log domain (eps_j is not capped).  To first order in eps the two agree.  It is finite unless every
  term of the row may be lost: about 1e4 at |L| = 1e20 for exp(-r), 1e25 at |L| = 1e40 for the Gaussian, a few 1e-15 of |L|.
* the gradient.  Per column D + 1 sums on one shift, Z as above and V[d] = sum_j w_j q_j df_jd:
    df_d = x_d - y_d: one rounding, KEPT: the same df_d enters s (inside gamma_s) and the product (one factor);
    exp(-r): q = lse_grad_rinv(s) = kval<1/r>(s): Lq = h + TRANS (float32 v_rsq_f32), h + RSQ64 (float64), and the product
      w q: one rounding; q = 0 exactly where s is not a positive normal number;
    fma(wq, df, V): its rounding belongs to the chain.   NR = 1 (Gaussian), 2 (exp(-r));  r_NR = (1 + u)^NR - 1
    |term' - term| <= w g [expm1(eps_j + Lq) (1 + r_NR) + r_NR],  g = |df_d| (Gaussian), |df_d| / r (exp(-r));
    a product that is denormal is off by eta: (1 + |df_d|) eta per pair.
  mass[d] = sum_j w_j g_jd / Z >= |V[d]| / Z.  Chain, folds, merge and shift as for Z, on the mass; the shift's leftovers
  times (1 + max |df|).  The quotient is kmvp_f32_model's: (band_V + |V / Z| band_Z) / (Z - band_Z); lse_grad_value's
  multiply and divide in fp64: 2 u64 |G|; the constants -2 and -1 are exact.
  Where eps_j is not small the quotient form has no room (Z - band_Z <= 0).  What holds whatever eps_j is: the perturbed
  weights are still positive, fl(sum t_j) = sum t_j (1 + theta_j) with |theta_j| <= ACC + ADD64, so V'[d] / Z' is a CONVEX
  combination of the directions g_jd of the column's live pairs, each off by a factor 1 + xi_j, |xi_j| <= r_NR + Lq + 2
  (ACC + ADD64).  The exact V[d] / Z is a convex combination of the same g_jd, so with hi, lo, gmax the largest, smallest
  and largest absolute g_jd over the live pairs
      |G' - G| <= |constant| K_BAND [ (hi - lo) + gmax (r_NR + Lq + 2 ACC + 2 ADD64) + SHIFT (1 + max |df| + gmax) + 2 eta sum_j (1 + |df_jd|) ]
                  + 2 u64 |G|
  and band(G) is the smaller of the two forms.  At targets 1e20 away the Gaussian's hi - lo is the spread of the sources
  on that axis (a few units against |G| = 2e20) and the term that counts is gmax u = 1e4, the rounding of x - y.
* exact rules, all properties of `value`:
    c = -inf, pad records (y = +inf) and pairs whose squared distance overflows the working precision contribute exactly
      0; a +-inf SOURCE coordinate is such a pair for L (include/kmvp.h: pairs at infinite distance contribute 0);
    a (row, column) without a live term is exactly -inf (L) or NaN in all D components (G); M = 0 is that everywhere;
    a NaN target coordinate makes its row NaN in every column, and no other row;
    exp(-r): a pair at s = 0 adds 0 to V and keeps its weight in Z;
    c = NaN or +inf in one entry: G has no finite entry in that column, for any target, and the other columns are
      untouched (the kernel: the weight is NaN, by v_exp_f32 itself or by a select on m - u in float64).  L: include/kmvp.h
      says "unspecified but not finite".  The kernels: float32 v_exp_f32 passes the NaN of m - u on (c = +inf: m = +inf,
      inf - inf), so the column is NaN.  float64's exponential clamps its argument with a min that drops a NaN, which
      made the pair's weight exactly 0 -- a finite column for c = NaN, and for c = +inf in a launch of several
      segments (the segment that holds it is taken for one without a live term): against the header.  lse_exp2_neg now
      passes the NaN on in float64 as well.  The model: every entry of the column is `poisoned`, value NaN.
    a source coordinate that is NaN or +-inf is not screened by the kernels.  G: x - y is non-finite on that axis and
      0 * inf is NaN (the header's rule for an infinite coordinate): in EVERY row and column the components of that axis
      are `poisoned`.  Everything else -- the other axes of G, all of L for a NaN coordinate, for which the header
      states no rule -- is either non-finite too (the source's weight is NaN: every u of a NaN source is NaN, max() drops
      it from the shift, and the exponential passes it on) or holds the sum over the other sources: `value` and `band`
      are those of the other sources, and the tests take such a case as `loose`.
* mass.  L: max(1, |L|) (for the record only: the band does not scale with it).  G: |constant| sum_j p_j g_jd.

Preconditions, RAISED (the kernels are not wrong there, the model does not cover them): every non-zero squared distance
of finite points is a normal number of the working precision; a squared distance is either representable or overflows
whatever its roundings; no target coordinate is +-inf; every live logit is above lse_sentinel (-3e38 / -1e299 binades).
Known limit, not modelled: a float32 row all of whose sources lie so far away that s * LOG2E overflows although s does
not (s > 2.3e38) comes out -inf / NaN while the true value is finite; float32 v_sqrt_f32 / v_rsq_f32 do not take denormal
inputs.

Parity status: no reference counterpart; with rounding disabled `value` equals tests/lse_reference.py and
tests/lse_grad_reference.py (tests/test_lse_model.py).
"""
from collections import namedtuple

import numpy as np

from kmvp_f32_model import FLUSH
from kmvp_lowd_model import (ETA64, EXP64, HAVE_LONGDOUBLE, K_BAND, LAM, LDS_TILE, LOWD_BATCH, RSQ64, TRANS, U64, chain_length,
                             unit)

KERNELS = ("gaussian", "absolute-exponential")
CONSTANT = {"gaussian": -2.0, "absolute-exponential": -1.0}
SENTINEL = {np.dtype(np.float32): -3.0e38, np.dtype(np.float64): -1.0e299}
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
LOG2_ULPS = 4 * U64                      # ASSUMPTION: the device's fp64 log2 at 2 ulp
BATCH = 4                                # sources per batch of the shift
assert LDS_TILE == 256 and LOWD_BATCH == 8

# Model's fields with `poisoned` (kmvp_lowd_grad_model's) beside `nonfinite`; flagged is always False: no row is flagged
LseModel = namedtuple("LseModel", "value band mass flagged nonfinite poisoned")


def _prepare(kernel, y, x, c, precision, rows):
    if kernel not in KERNELS:
        raise ValueError(kernel)
    precision = np.dtype(precision)
    y = np.asarray(y, dtype=precision).astype(np.float64)
    xa = y if x is None else np.asarray(x, dtype=precision).astype(np.float64)
    if np.isinf(xa).any():
        raise ValueError("an infinite target coordinate is not covered by the model")
    rows = np.arange(xa.shape[0], dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    density = c is None
    c = np.zeros((y.shape[0], 1)) if density else np.asarray(c, dtype=precision).astype(np.float64)
    if c.ndim == 1:
        c = c.reshape(-1, 1)
    return precision, y, xa, c, density, rows


def lse(kernel, y, x=None, c=None, *, precision=np.float32, chunk=512, feed=1, rows=None, j_offset=0, M_total=None,
        rounding=True):
    """Modelled L (n, NC) of kmvp_<kernel>_logsumexp (feed = 1) or of one application of lowd_batch_lse_kernel (feed = 0).

    y (M, D) sources, x (N, D) targets (None: the same points), c (M, E) log-weights (None: density, c = 0, one column),
    all rounded to `precision` first.  chunk: the "chunk" option.  j_offset / M_total: accepted for a slice of the sources
    (no rule of these kernels depends on them).  rows: target indices to model.  rounding=False: the value, no band."""
    return _run(False, kernel, y, x, c, precision, chunk, feed, rows, rounding)


def lse_gradient(kernel, y, x=None, c=None, *, precision=np.float32, chunk=512, feed=1, rows=None, j_offset=0, M_total=None,
                 rounding=True):
    """Modelled G (n, NC, D) of kmvp_<kernel>_logsumexp_grad; the arguments are lse's."""
    return _run(True, kernel, y, x, c, precision, chunk, feed, rows, rounding)


def _run(grad, kernel, y, x, c, precision, chunk, feed, rows, rounding):
    precision, y, xa, c, density, rows = _prepare(kernel, y, x, c, precision, rows)
    M, D = y.shape
    NC = c.shape[1]
    if len(rows) == 0 or M == 0:
        shape = (len(rows), NC, D) if grad else (len(rows), NC)
        z = np.zeros(shape)
        return LseModel(np.full(shape, np.nan if grad else -np.inf), z, z, np.zeros(len(rows), bool),
                        np.isnan(xa[rows]).any(axis=1), np.zeros(shape, bool))
    block = max(1, 2 ** 20 // max(1, M * max(D, NC)))
    n_chain = chain_length("lowd", precision, M, chunk, feed)
    parts = [_block(grad, kernel, y, xa[rows[r0:r0 + block]], c, density, precision, n_chain, rounding)
             for r0 in range(0, len(rows), block)]
    return LseModel(*(np.concatenate(f) for f in zip(*parts)))


def _logsum(a):
    """ln sum_j exp(a_j) over axis 1; -inf where no term is finite."""
    top = a.max(axis=1, keepdims=True)
    top = np.where(np.isfinite(top), top, 0.0)
    return top[:, 0] + np.log(np.exp(a - top).sum(axis=1))


def _block(grad, kernel, y, x, c, density, precision, n_chain, rounding):
    M, D = y.shape
    NC = c.shape[1]
    n = x.shape[0]
    f32 = precision == np.float32
    u = unit(precision)
    info = np.finfo(precision)
    wide = HAVE_LONGDOUBLE
    W = np.longdouble if wide else np.float64
    gs0 = np.expm1((D + 2) * np.log1p(u))
    # ---- the exact rules: which pairs enter a sum, which elements are non-finite whatever the arithmetic
    bad_src = ~np.isfinite(y)                                     # (M, D): not screened by the kernels, see the rules
    out_src = bad_src.any(axis=1)                                 # such a source leaves the modelled sums
    bad_c = np.isnan(c) | (c == np.inf)                           # (M, NC)
    nan_row = np.isnan(x).any(axis=1)
    yc = np.where(out_src[:, None], 0.0, y)
    xc = np.where(nan_row[:, None], 0.0, x)
    with np.errstate(all="ignore"):
        df = xc.astype(W)[:, None, :] - yc.astype(W)[None, :, :]             # (n, M, D)
        sw = (df * df).sum(axis=2)
        s = sw.astype(np.float64)
        dropped = np.broadcast_to(out_src[None, :], s.shape).copy()
        over = s * (1.0 - gs0) > float(info.max)                   # overflows whatever its roundings: nl = inf, u = -inf
        maybe = (s * (1.0 + gs0) > float(info.max)) & ~over
        dropped |= over
        nlw = sw if kernel == "gaussian" else np.sqrt(sw)
        cw = np.where(bad_c, -np.inf, c).astype(W)                # (a poisoned column: the other entries' sum, for the record)
        U = (cw[None, :, :] - nlw[:, :, None]) * W(LOG2E)         # (n, M, NC) log2 units
        U = np.where(dropped[:, :, None], -np.inf, U)
        top = U.max(axis=1)                                       # (n, NC)
        live = np.isfinite(top)
        m = np.where(live, np.ceil(top), 0.0)
        w = np.exp2(U - m[:, None, :])                            # (n, M, NC), the largest in (1/2, 1]
        Z = w.sum(axis=1)                                         # (n, NC)
        L = (np.log(Z) + m * W(LN2)).astype(np.float64)
        L = np.where(live, L, -np.inf)
        if grad:
            if kernel == "gaussian":
                g = df
            else:
                normal = (sw >= W(info.tiny)) & np.isfinite(sw)
                g = np.where(normal[:, :, None], df / np.where(normal, nlw, 1)[:, :, None], 0)
            g = np.where(dropped[:, :, None], 0, g)
            V = np.einsum("nme,nmd->ned", w, g)
            G = (W(CONSTANT[kernel]) * V / Z[:, :, None]).astype(np.float64)
            G = np.where(live[:, :, None], G, np.nan)
    shape = (n, NC, D) if grad else (n, NC)
    poisoned = np.zeros(shape, dtype=bool)
    poisoned[nan_row] = True
    poisoned[:, bad_c.any(axis=0)] = True
    if grad:
        poisoned[:, :, bad_src.any(axis=0)] = True
    value = G if grad else L
    value = np.where(poisoned, np.nan, value)
    nonfinite = nan_row.copy()
    flagged = np.zeros(n, dtype=bool)
    w64, Z64 = w.astype(np.float64), Z.astype(np.float64)
    with np.errstate(all="ignore"):
        if grad:
            ag = np.abs(g.astype(np.float64))
            massV = np.einsum("nme,nmd->ned", w64, ag)
            mass = abs(CONSTANT[kernel]) * massV / Z64[:, :, None]
        else:
            mass = np.maximum(1.0, np.abs(np.where(np.isfinite(L), L, 0.0)))
    zero = np.zeros(shape)
    if not rounding:
        return LseModel(value, zero, mass, flagged, nonfinite, poisoned)
    # ---- preconditions
    ok = ~nan_row
    with np.errstate(invalid="ignore"):
        pos = np.isfinite(s) & (s > 0) & ~dropped
        if (pos & (s < float(info.tiny)))[ok].any():
            raise ValueError("a non-zero squared distance is below the smallest normal number of the working precision")
        if maybe[ok].any():
            raise ValueError("a squared distance may or may not overflow the working precision")
        Uf = U.astype(np.float64)
        if (np.isfinite(Uf) & (Uf <= SENTINEL[precision]))[ok].any():
            raise ValueError("a live logit is not above lse_sentinel")
    # ---- the weights' relative errors
    eta = 2.0 ** -150 if f32 else ETA64
    with np.errstate(all="ignore"):
        ss = np.where(pos, s, 1.0)
        gs = np.where(pos, gs0 + D * eta / ss, 0.0)
        h = -0.5 * np.log1p(-gs)
        nl = np.where(pos, nlw.astype(np.float64), 0.0)
        if kernel == "gaussian":
            rho_nl = gs
        else:
            rho_nl = h + (TRANS if f32 else RSQ64 + u)
        cf = np.where(np.isfinite(c) & ~bad_c, c, 0.0)
        t_abs = nl[:, :, None] if density else np.abs(cf[None, :, :] - nl[:, :, None])
        d = (nl * rho_nl)[:, :, None] + (2 if density else 3) * u * t_abs
        a = np.where(np.isfinite(Uf), m.astype(np.float64)[:, None, :] - Uf, 0.0) + 1.0
        eps = d + LN2 * a * u * (1 if f32 else 3) + (TRANS if f32 else EXP64)
        rel = np.expm1(np.minimum(eps, 700.0))
        lost = (a * (1.0 + u) + eps * LOG2E > 126.0) if f32 else (a * LN2 > 700.0)
        each = np.where(lost, np.maximum(rel, 1.0), rel) * w64     # (n, M, NC), absolute at the final scale
        nb = -(-M // BATCH)
        shift = 2.0 * (nb * FLUSH + (M + 1) * 2.0 ** -280) if f32 else 2.0 * nb * 2.0 ** -1022
        acc_rel = min(n_chain, LAM * np.sqrt(n_chain)) * u + (M / 4.0 + 2.0) * U64
        own = 1.0 if wide else 2.0
        pairZ = each.sum(axis=1)                                   # (n, NC)
        bandZ = own * K_BAND * (pairZ + (acc_rel + shift) * Z64)   # absolute, at the scale of Z
        if not grad:
            rho = bandZ / Z64
            finish = LOG2_ULPS * LN2 * (np.log2(M + 1.0) + 1.0) + 3 * U64 * np.abs(L)
            band = np.where(rho < 0.999, -np.log1p(-np.minimum(rho, 0.999)), np.inf)
            lw = np.where(np.isfinite(Uf), (Uf - m.astype(np.float64)[:, None, :]) * LN2, -np.inf)     # ln w_j
            pair = np.maximum(_logsum(lw + eps) - _logsum(lw), _logsum(lw) - _logsum(np.where(lost, -np.inf, lw - eps)))
            band = np.minimum(band, own * K_BAND * (pair - np.log1p(-(acc_rel + shift)))) + finish
            band = np.where(live, band, 0.0)
            return LseModel(value, band, mass, flagged, nonfinite, poisoned)
        Lq = 0.0 if kernel == "gaussian" else (h + (TRANS if f32 else RSQ64))[:, :, None]
        nr = 1 if kernel == "gaussian" else 2
        r_nr = np.expm1(nr * np.log1p(u))
        relV = np.expm1(np.minimum(eps + Lq, 700.0))
        eachV = np.where(lost, np.maximum(relV, 1.0), relV) * (1 + r_nr) + r_nr       # (n, M, NC)
        pairV = np.einsum("nme,nmd->ned", eachV * w64, ag)
        adf = np.abs(np.where(dropped[:, :, None], 0.0, df.astype(np.float64)))
        far = 1.0 + adf.max(axis=1)                                # (n, D)
        pairV = pairV + eta * (1.0 + adf).sum(axis=1)[:, None, :]
        accV = acc_rel * massV + (shift * Z64)[:, :, None] * far[:, None, :]
        bandV = own * K_BAND * (pairV + accV)
        room = (Z64 - bandZ)[:, :, None]
        c0 = abs(CONSTANT[kernel])
        q = np.abs(np.where(np.isfinite(G), G, 0.0))
        band = np.where(room > 0, (c0 * bandV + q * bandZ[:, :, None]) / np.where(room > 0, room, 1.0), np.inf)
        # the convex-combination form, for weights whose errors are not small
        alive = np.isfinite(Uf)[:, :, :, None]                                         # (n, M, NC, 1)
        g64 = g.astype(np.float64)[:, :, None, :]                                      # (n, M, 1, D)
        hi, lo = np.where(alive, g64, -np.inf).max(axis=1), np.where(alive, g64, np.inf).min(axis=1)   # (n, NC, D)
        gmax = np.maximum(np.abs(hi), np.abs(lo))
        xi = r_nr + float(np.max(Lq)) + 2 * acc_rel
        convex = (hi - lo) + gmax * xi + shift * (far[:, None, :] + gmax) + 2 * eta * (1.0 + adf).sum(axis=1)[:, None, :]
        band = np.minimum(band, c0 * own * K_BAND * convex) + 2 * U64 * q
        band = np.where(live[:, :, None], band, 0.0)
        return LseModel(value, band, mass, flagged, nonfinite, poisoned)
