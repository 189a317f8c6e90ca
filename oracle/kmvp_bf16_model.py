"""Float64 model of the bf16 matrix-core product (kmvp_mfma.hpp) -- TEST INFRASTRUCTURE ONLY.

The bf16 path (run_product_mfma) is not held to the float64 product of the caller's inputs: most of its difference
from that comes from rounding the inputs to bf16, which the kernel is built to do.  This module restates the
kernel's own arithmetic in float64 instead, and bounds per row what it cannot restate.

Arithmetic of the kernels (kmvp_mfma.hpp, kmvp_mfma_pack.hpp, kmvp_lowd.hpp):

* operands: x~ = bf16(f32(x) * f32(c)), c = sqrt(log2 e) (Gaussian, exp(<x,y>)), log2 e (exp(-r)), 1 (1/r);
* S = |x~ - y~|^2 (exp(<x,y>): <x~, y~>) as the fp32 MFMA sum of KD = 16 KS exact bf16 products, the norms
  entering as fmaf chains over D split three ways into bf16 (split3);
* p = exp2(-S), exp2(-sqrt|S|), rsq|S| or exp2(S) on the VALU (v_exp_f32, v_sqrt_f32, v_rsq_f32); v_exp_f32
  flushes results below 2^-126 to zero; 1/r has the flat-index zero rule (kmvp_oracle.zero_column);
* P = bf16(p) round-to-nearest-even, signal b~ = bf16(b); numerators are fp32 MFMA sums of P b~ per source
  segment, reduced over segments in fp64;
* denominators: the fp32 VALU sum of the unrounded p, or the MFMA sum of P (DEN_MFMA, mfma_variant bit 0).

The model evaluates S~ from the rounded points in float64 (exact: the products of bf16 numbers and their sums fit in
53 bits for the clouds the tests use), p from S~, P~ = bf16(p) and the sums in float64.  What it cannot restate:

* pairs whose kernel value lies, within the error bound of the kernel's S and transcendental, on both sides of a
  bf16 rounding midpoint (AMBIGUOUS pairs): the kernel may round to either neighbour.  Bound per pair, as a
  bound on |log p_kernel - log p~|:
    e_S  = gamma(KD) T + (gamma(D) + 2^-27) (|x~|^2 + |y~|^2),   gamma(n) = n u / (1 - n u),  u = 2^-23
      T  = |x~|^2 + |y~|^2 + 2 sum_d |x~_d y~_d| (+ |m| for the shifted kernels): the absolute sum of the MFMA's
           terms; gamma(KD) T is the worst case of KD roundings whatever the MFMA's internal order and rounding
           mode (u = one fp32 ulp, not half of one); gamma(D) |x~|^2 the fmaf chain of the norm; 2^-27 |x~|^2 the
           split3 residual (three bf16 pieces: 24 bits, the last one rounded at 2^-9 of 2^-18)
    v_exp_f32 / v_sqrt_f32 / v_rsq_f32: 1 ulp each by the ISA, taken as 2 ulp (2^-22 relative) per instruction
    Gaussian    L = ln2 e_S + 2^-22
    exp(-r)     L = ln2 (min(sqrt e_S, e_S / sqrt S~) + 2^-22 (sqrt S~ + sqrt e_S)) + 2^-22
    1/r         L = -ln(1 - e_S / S~) / 2 + 2^-22 (pairs with e_S / S~ > 2^-8 are FLAGGED: see below)
    exp(<x,y>)  L = ln2 e_S + 2^-22
  amb_i = sum over ambiguous pairs of |bf16(p e^L) - bf16(p e^-L)| |b~_j|;
* fp32 accumulation of the sums.  Each numerator is a chain of fp32 roundings of at most n = (sources per
  segment) terms whose absolute sum is mass_i = sum_j P~_ij |b~_j|.  With rounding errors independent and of mean
  zero (round to nearest), |error| <= lam sqrt(n) 2^-24 mass_i with probability >= 1 - 2 n exp(-lam^2 / 2)
  (Higham and Mary, "A new approach to probabilistic rounding error analysis", SIAM J. Sci. Comput. 2019, Thm 2.4
  applied to recursive summation).  lam = 8: below 1e-9 per row for n <= 2^17.  The VALU denominators: the same
  with n = sources per segment.
* values below the fp32 normal range, which the kernel flushes (v_exp_f32) or keeps: at most
  M 2^-125 max|b~| per row (exp(<x,y>) / the shifted Gaussian: relative to the row's shift, whose placement puts
  the flush at least 60 binades under the row maximum: M 2^-60 max|b~| 2^(row max)).

band_i = K (amb_i + acc_i + floor_i) with K = 2: amb, acc and floor are each upper bounds; the factor covers the
second-order terms the bounds drop (products of two relative errors, the linearised quotient of normalised rows).

Rows the model cannot hold to a band are FLAGGED: 1/r pairs within the cancellation range of S (rounded points that
coincide off the zero rule, or nearly so: the kernel's expanded S is a small number of either sign where S~ = 0),
rows whose whole mass lies under the fp32 range (unshifted exp kernels), normalised rows whose denominator band
reaches the denominator.

Parity status: no reference counterpart (the reference has no bf16 path); checked against kmvp_oracle.product with
rounding disabled by tests/test_bf16_model.py.
"""
from collections import namedtuple

import numpy as np

import kmvp_oracle

C_GAUSSIAN = 1.2011224087864498   # sqrt(log2 e): the Gaussian's and exp(<x,y>)'s coordinate scale (coord_scale)
C_ABSEXP = 1.4426950408889634     # log2 e
SCALE = {"gaussian": C_GAUSSIAN, "gaussian-shifted": C_GAUSSIAN, "absolute-exponential": C_ABSEXP,
         "inverse-distance": 1.0, "exp-dot": C_GAUSSIAN}
MFMA_AUG, MFMA_DOT_AUG = 6, 3
U_ACC = 2.0 ** -23        # one fp32 ulp (relative): any rounding mode
U_RNE = 2.0 ** -24        # fp32 unit roundoff, round to nearest
TRANS = 2.0 ** -22        # v_exp_f32 / v_sqrt_f32 / v_rsq_f32 relative error, 2 ulp
FLUSH = 2.0 ** -126
LAM = 8.0
K_BAND = 2.0
FLAG_1R = 2.0 ** -8

Model = namedtuple("Model", "value band mass amb acc floor flagged nonfinite")


def bf16_round(a, c=None):
    """What the bf16 packing kernels make of the plugin's float32 inputs, as float64: (float32 a) x (float32 c) -- ONE float32
    product, as the kernel forms it -- rounded to the nearest bfloat16 (ties to even), then divided by c again.  (Multiplying in
    float64 instead lands on the other side of a bf16 rounding boundary for about one operand in a million, and a logit of
    ~1000 then moves by half a unit: a one-row artefact of the emulation that looked like a kernel defect.)  NaN stays NaN
    (whatever its payload: adding the rounding increment to it would carry into the exponent)."""
    v = np.ascontiguousarray(a, dtype=np.float32)
    if c is not None:
        v = v * np.float32(c)
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    with np.errstate(invalid="ignore"):
        r = np.where(np.isnan(v), np.nan, u.view(np.float32).astype(np.float64))
    return r if c is None else r / c


def bf16_of_f64(p):
    """float64 -> nearest bfloat16 (ties to even), in one rounding: 8 significant bits, normal range only (the
    values given here are kernel values, flushed below 2^-126 by the caller)."""
    p = np.asarray(p, dtype=np.float64)
    m, e = np.frexp(p)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.where(np.isfinite(p), np.ldexp(np.rint(m * 256.0), e - 8), p)


def ksteps(kernel, D):
    aug = {"exp-dot": MFMA_DOT_AUG, "gaussian-shifted": MFMA_AUG + MFMA_DOT_AUG}.get(kernel, MFMA_AUG)
    return (D + aug + 15) // 16


def _gamma(n, u=U_ACC):
    return n * u / (1.0 - n * u)


def mfma_product(kernel, y, x=None, b=None, normalize_rows=False, density=False, variant_den_mfma=False, j_offset=0,
                 M_total=None, *, rows=None, seg_len=None, rounding=True, eta=1.0):
    """Modelled result of run_product_mfma and its per-element band.

    kernel: "gaussian", "absolute-exponential", "inverse-distance", "gaussian-shifted" (the bf16 Gaussian with targets !=
    sources and the default variant) or "exp-dot".  y (M,D) sources, x (N,D) targets (None: the same points), b (M,E)
    signal (None or density: a column of ones).  j_offset / M_total: the source shard (1/r zero rule).  rows: global
    target indices to model (default all).  seg_len: sources per segment (the longest fp32 chain; default M).
    rounding=False: no bf16 rounding and no bands -- the float64 product, for checking the model against the oracle.
    eta scales every per-pair error bound (eta = 0: no pair is ambiguous).

    Returns Model(value (n,E), band (n,E), mass (n,E), amb (n,E), acc (n,E), floor (n,E), flagged (n,), nonfinite (n,))."""
    y = np.asarray(y, dtype=np.float64)
    rows = np.arange((y if x is None else x).shape[0], dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    block = max(1, 2 ** 21 // max(1, y.shape[0]))  # rows per block: a few (block, M) float64 arrays at a time
    parts = [_mfma_block(kernel, y, x, b, normalize_rows, density, variant_den_mfma, j_offset, M_total, rows[r0:r0 + block],
                         seg_len, rounding, eta) for r0 in range(0, max(len(rows), 1), block)]
    return Model(*(np.concatenate(f) for f in zip(*parts)))


def _mfma_block(kernel, y, x, b, normalize_rows, density, variant_den_mfma, j_offset, M_total, rows, seg_len, rounding, eta):
    shifted = kernel in ("gaussian-shifted", "exp-dot")
    y = np.asarray(y, dtype=np.float64)
    same = x is None
    x = y if same else np.asarray(x, dtype=np.float64)
    M, D = y.shape
    x = x[rows]
    n = len(rows)
    if density or b is None:
        b = np.ones((M, 1))
    b = np.asarray(b, dtype=np.float64)
    E = b.shape[1]
    if normalize_rows and density:
        z = np.zeros((n, 1))
        return Model(np.ones((n, 1)), z, z, z, z, z, np.zeros(n, bool), np.zeros(n, bool))

    c = SCALE[kernel]
    if rounding:
        ys, xs, bs = bf16_round(y, c) * c, bf16_round(x, c) * c, bf16_round(b)
    else:
        ys, xs, bs = y * c, x * c, b
    # S~ of the scaled, rounded points (exact in float64 here), and the absolute sum T of the MFMA's terms
    dot = xs @ ys.T
    nx, ny = (xs * xs).sum(1)[:, None], (ys * ys).sum(1)[None, :]
    if kernel == "exp-dot":
        s = dot                                                     # log2 p = s - m_i
    else:
        s = nx + ny - 2.0 * dot
        if not rounding:
            s = kmvp_oracle.sqdists_block(x, y, False) * c * c      # the difference form: no cancellation
        s = np.maximum(s, 0.0)
    KD = 16 * ksteps(kernel, D)
    absdot = np.abs(xs) @ np.abs(ys).T
    if kernel == "exp-dot":
        smax = s.max(axis=1, keepdims=True) if M else np.zeros((n, 1))
        shift = np.ceil(smax)                                       # an integer: bf16 rounding commutes with 2^shift
        # the kernel's running shift m_i lies between the ceilings of its first tile's and the row's maxima
        T = absdot + np.abs(s).max(axis=1, keepdims=True) + 1.0 if M else absdot
        e_s = _gamma(KD) * T
        logp = (s - shift) * np.log(2.0)
    else:
        T = nx + ny + 2.0 * absdot
        e_s = _gamma(KD) * T + (_gamma(D) + 2.0 ** -27) * (nx + ny)
        if kernel == "gaussian-shifted":
            smin = s.min(axis=1, keepdims=True) if M else np.zeros((n, 1))
            shift = -np.floor(smin)
            e_s = e_s + _gamma(KD) * (s.max(axis=1, keepdims=True) + 1.0)  # |m_i| <= the row's largest S + 1
        else:
            shift = np.zeros((n, 1))
    # kernel values (relative to 2^shift for the shifted kernels) and the log-bound L of each pair
    flagged = np.zeros(n, dtype=bool)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if kernel in ("gaussian", "gaussian-shifted"):
            p = np.exp2(-(s + shift))
            L = np.log(2.0) * e_s + TRANS
        elif kernel == "exp-dot":
            p = np.exp(logp)
            L = np.log(2.0) * e_s + TRANS
        elif kernel == "absolute-exponential":
            r = np.sqrt(s)
            p = np.exp2(-r)
            dr = np.minimum(np.sqrt(e_s), e_s / r) + TRANS * (r + np.sqrt(e_s))
            L = np.log(2.0) * dr + TRANS
        else:
            p = 1.0 / np.sqrt(s)
            ratio = e_s / s
            L = -0.5 * np.log1p(-np.minimum(ratio, 0.5)) + TRANS
            jz = kmvp_oracle.zero_column(rows, M if M_total is None else M_total) - j_offset
            hit = (jz >= 0) & (jz < M)
            p[np.nonzero(hit)[0], jz[hit]] = 0.0
            L[np.nonzero(hit)[0], jz[hit]] = 0.0
            live = p != 0.0
            flagged |= ((ratio > FLAG_1R) & live).any(axis=1)
    if not rounding:
        P = p * np.exp2(shift) if shifted else p
        num = P @ b
        den = P.sum(axis=1, keepdims=True)
        with np.errstate(divide="ignore", invalid="ignore"):
            value = num / den if normalize_rows else num
        z = np.zeros_like(value)
        return Model(value, z, np.abs(P) @ np.abs(b), z, z, z, flagged, ~np.isfinite(value).all(axis=1))

    L = eta * L
    flush = lambda v: np.where(v < FLUSH, 0.0, v)  # noqa: E731
    with np.errstate(invalid="ignore", over="ignore"):
        p = flush(p)
        p_lo, p_hi = flush(p * np.exp(-L)), flush(p * np.exp(L))
        P, P_lo, P_hi = bf16_of_f64(p), bf16_of_f64(p_lo), bf16_of_f64(p_hi)
        dP = np.where(P_hi != P_lo, np.abs(P_hi - P_lo), 0.0)
        dP = np.where(np.isfinite(dP), dP, 0.0)
    babs = np.abs(bs)
    Pf = np.where(np.isfinite(P), P, 0.0)
    nonfinite = ~np.isfinite(P).all(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        num = P @ bs
        mass = Pf @ babs
        amb = dP @ babs
    n_chain = float(seg_len if seg_len else max(M, 1))
    acc = LAM * np.sqrt(n_chain) * U_RNE * mass
    bmax = babs.max(axis=0, keepdims=True) if M else np.zeros((1, E))
    floor = (M * 2.0 ** -60 if shifted else M * 2.0 ** -125) * bmax * np.ones((n, 1))
    band_num = K_BAND * (amb + acc + floor)
    if not shifted and kernel != "inverse-distance":
        flagged |= (mass < 2.0 ** -100 * np.maximum(bmax, 1e-300)).all(axis=1) & (M > 0)
    scale = np.exp2(shift)  # shifted kernels: back to the caller's units (exact powers of two)
    if not normalize_rows:
        return Model(num * scale, band_num * scale, mass * scale, amb * scale, acc * scale, floor * scale, flagged,
                     nonfinite)
    if variant_den_mfma:
        den = Pf.sum(axis=1, keepdims=True)
        bden = K_BAND * (dP.sum(axis=1, keepdims=True) + LAM * np.sqrt(n_chain) * U_RNE * den + M * 2.0 ** -125)
    else:
        den = p.sum(axis=1, keepdims=True)
        bden = K_BAND * ((p * np.expm1(L)).sum(axis=1, keepdims=True) + LAM * np.sqrt(n_chain) * U_RNE * den
                         + (M * 2.0 ** -60 if shifted else M * 2.0 ** -125))
    with np.errstate(divide="ignore", invalid="ignore"):
        value = num / den
        room = den - bden
        band = (band_num + np.abs(value) * bden) / room
        flagged |= ~(room > 0).all(axis=1)
        return Model(value, band, mass / den, amb / den, acc / den, floor / den, flagged, nonfinite)
