"""Float64 model of the float32 single-column matrix-core products -- TEST INFRASTRUCTURE ONLY.

fast_kernel (kmvp_fast.hpp, kmvp_fast_pack.hpp, run_product_fast) and cfast_kernel (kmvp_cfast.hpp, kmvp_cfast_pack.hpp,
run_product_cfast) serve one signal column (E = 1), density estimation (no signal) and normalised rows.  They take the
squared distance from the same split-bf16 expansion as fastmm_kernel / cfastmm_kernel and then sum k b_j on the VALU in
fp32: no f16 split of T or b, no second matrix product.  This model is therefore the subset of kmvp_f32mm_model.py that
bounds S and k -- imported from there, not restated -- plus an fp32 accumulation term.  The contract is the same: `value`
is the float64 product of the caller's float32 inputs, `band` a per-element upper bound derived from the code, nothing
fitted to kernel output.  (u = 2^-24, U = 2^-23.)

fast_kernel, step by step:

* operands (pack_fast_targets_kernel, pack_fast_sources_kernel): x' = f32(f32(x - c) scale), c the box midpoint from
  fast_center_kernel, scale = scale_for(kernel); |x'|^2 summed in double and rounded once (row[D], fast_row_norm); both
  split three ways into bf16 (targets in the kernel by fast_split3f, sources at pack time by fast_split3 /
  fast_row_coord).  The same code as fastmm's operands: the bound is kmvp_f32mm_model.expansion_error's operand part
  (4u sqrt(s) (|x'| + |y'|), the three dropped cross products U sum_d |x'_d y'_d|, the norms (u + 2^-27)(|x'|^2 + |y'|^2)).
* S (fast_kernel: the `ks` loop of v_mfma_f32_32x32x16_bf16): K = 6 D + 6 columns in k order in KS = ceil(K / 16) chained
  MFMAs -- the 6 D coordinate products (fast_target_elem roles against fast_row_coord's (h, h, m, h, m, l)), then three
  norm pieces of the source against ones and three ones against the target's norm pieces; the pad columns are zero and add
  exactly.  The matrix cores are taken to sum an MFMA's products as a k-ordered chain with one round-to-nearest rounding
  per product, the assumption kmvp_f32mm_model states (for the fp32 MFMA in the CDNA4 notes, taken for the bf16 one):
  e_S = u (6 D A + 6 T_abs) + the operands' part, A = 2 sum_d |x'_d y'_d|, T_abs = |x'|^2 + |y'|^2 + A.  That is
  expansion_error with tail = 6 and without FMM_SHIFT and the online columns.
* kernel value (fast_kval), each transcendental (v_exp_f32, v_sqrt_f32, v_rsq_f32: 1 ulp by the ISA) taken at 2 ulp:
    Gaussian  kexp2(-S)           relative error of k: expm1(ln2 e_S + 2^-22)
    exp(-r)   kexp2(-sqrt|S|)     |sqrt|S| - sqrt s| <= min(sqrt e_S, e_S / sqrt s) (also where S < 0 by rounding);
                                  expm1(ln2 (that + 2^-22 (sqrt s + sqrt e_S)) + 2^-22)   (absexp_log_error, no fp32 add
                                  in the argument here)
    1/r       rsq|S|              1 / sqrt(1 - e_S / s) - 1 (invdist_log_error); a pair with e_S / s >= 1/4 FLAGS its row
  exp(-r) and 1/r have only the ABSOLUTE accuracy e_S in s on this path, so neither bound is linearised.  exp(-r)'s bound
  holds for every e_S / s and flags nothing.
  kexp2 is __builtin_amdgcn_exp2f, the bare v_exp_f32, which has no denormal handling: a result below 2^-126 (k < e^-87.3)
  comes back as 0.  A pair whose k (1 - relative bound) is below 2^-126 may therefore be lost whole: its bound is k itself.
  Nothing rescales these kernels' sums (fastmm_kernel's online shift does), so a row whose mass is near 2^-126 -- a target
  nine units from a Gaussian cloud -- carries this term; found by the GPU test on exactly such rows.
* exact rules (fast_kernel: jz, `check`): the pair whose source index is the target's flat index mod (M_total + 1), less
  j_offset, gets k = 0 for 1/r (the reference's flat-index zero rule; it wraps when N > M_total) and k = 1 for exp(-r)
  when the targets are the sources (same points, or the same_points_global option): no error on that pair.  Pad sources
  carry |y'|^2 = +inf and b = 0: k = 0, nothing to bound.
* accumulation (fast_kernel: p0 / p1, acc, accd): per source tile and lane half two fp32 chains of 8 FMAs (adds for
  density), p0 + p1, acc += ; acc is folded into fp64 every chunk_stages = max(1, chunk / (32 ST)) stages
  (run_product_fast), ST = fast_stage_tiles(KS); lane halves (__shfl_xor), segments and shards are added in fp64.  A lane
  half's fp32 sum between two folds therefore holds n = 18 x (tiles per chunk, at most a segment's and the cloud's)
  roundings: |error| <= lam sqrt(n) u mass with lam = 8, the probabilistic rule of kmvp_f32mm_model (Higham and Mary 2019,
  Thm 2.4); the fp64 part 2^-50 mass.  The library is built with fp32 denormals on (no flush flag in the Makefile): an
  FMA or add whose result is denormal is off by at most 2^-150, over all CHAIN_TILE x tiles operations of a row.
* normalised rows: the denominator is the same chain with b = 1 (q0 / q1); band = (band_num + |value| band_den) /
  (den - band_den), rows whose denominator band reaches the denominator FLAGGED.

cfast_kernel: S is expanded around the Morton group's centre with two MFMAs (K = 32) and a pair with S <= tau_g is
recomputed from the raw coordinates: kmvp_f32mm_model.centred_error as it stands (neither the grouping nor tau_g restated;
a recomputed pair takes gamma(D + 1) s; either bound).  The exact branch also carries the 1/r zero rule (s = +inf where the
stored global original index lidx equals the target's flat index mod (M_total + 1)), the exact s = 0 of the diagonal and
the reference's behaviour for non-finite coordinates (inf - x: s = inf, k = 0; NaN stays NaN): all three are properties of
`value`, which is the difference form in float64.  1/r: pairs with e_S / s > 2^-8 flag their row, as for cfastmm.
Accumulation as above with chunk_stages = max(1, chunk / 128) and four tiles per stage.

band = K (pair + acc) with kmvp_f32mm_model.K_BAND.  rounding=False gives the plain float64 product with no band.

What the band can and cannot see (tests/test_f32_model.py builds each defect into an emulation of the kernel's steps):
the pieces x_l y_h, x_h y_l, x_m y_m and the lo piece of |y'|^2 are each ~2^-16 of their term, 2^8 above u, and leave the
band wherever A or |y'|^2 is not small against 1 / (6 D + 6); a lost chain of eight sources, a skipped own-pair rule
(sqrt turns S ~ 1e-7 into 3e-4) and an unwrapped zero rule are errors of the size of single terms.

Parity status: no reference counterpart; checked against kmvp_oracle.product with rounding disabled by
tests/test_f32_model.py.
"""
import numpy as np

import kmvp_oracle
from kmvp_f32mm_model import (CF_GROUP, FLAG_1R, K_BAND, LAM, TRANS, U_RNE, Model, absexp_log_error, centred_error,
                              cloud_geometry, expansion_error, invdist_log_error, kernel_constant)

FLAG_FAST_1R = 0.25        # fast_kernel, 1/r: a pair with e_S / s at or above it flags its row
FLUSH = 2.0 ** -126        # the smallest normal fp32 number: v_exp_f32 returns 0 below it
CHAIN_TILE = 18            # fp32 roundings per source tile in a lane half: 16 FMAs, p0 + p1, acc +=


def fast_ksteps(D):
    return (6 * D + 6 + 15) // 16


def fast_stage_tiles(ks):
    return 4 if ks <= 9 else 2


def stage_sources(path, D):
    """Sources per LDS stage: 32 fast_stage_tiles(KS) (fast_kernel), one group of 128 (cfast_kernel)."""
    return 32 * fast_stage_tiles(fast_ksteps(D)) if path == "fast" else CF_GROUP


def acc_roundings(path, D, M, chunk=512, seg_len=None):
    """fp32 roundings of a lane half's sum between two folds into fp64: CHAIN_TILE per source tile, over the tiles of
    chunk_stages stages, of a segment (seg_len sources, whole stages) or of the whole cloud, whichever is fewest."""
    per = stage_sources(path, D)
    stages = min(max(1, chunk // per), -(-max(M, 1) // per))
    if seg_len:
        stages = min(stages, -(-seg_len // per))
    return CHAIN_TILE * stages * (per // 32)


def f32_product(kernel, y, x=None, b=None, normalize_rows=False, *, path="fast", same_global=False, rows=None, chunk=512,
                seg_len=None, j_offset=0, M_total=None, rounding=True):
    """Modelled result of run_product_fast / run_product_cfast and its per-element band.

    kernel: "gaussian", "absolute-exponential" or "inverse-distance".  y (M,D) sources, x (N,D) targets (None: the same
    points), b (M,1) signal (None: density estimation, a sum of kernel values).  same_global: the targets are the
    unsharded sources although x was passed (the same_points_global option).  j_offset / M_total: y is a slice of the
    sources.  rows: target indices to model.  chunk: the "chunk" option; seg_len: sources per segment.
    rounding=False: the float64 product, no band.
    Returns Model(value, band, mass, pair, tsplit, bsplit, acc (n, 1) each, flagged (n,), nonfinite (n,)); tsplit and
    bsplit are zero (these kernels split neither T nor b)."""
    if path not in ("fast", "cfast"):
        raise ValueError(path)
    y = np.asarray(y, dtype=np.float64)
    same = x is None
    xa = y if same else np.asarray(x, dtype=np.float64)
    rows = np.arange(xa.shape[0], dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    M = y.shape[0]
    if b is None and normalize_rows:
        raise ValueError("normalised density rows are ones by definition: no kernel runs")
    b = np.ones((M, 1)) if b is None else np.asarray(b, dtype=np.float64)
    if b.shape[1] != 1:
        raise ValueError("one signal column: several are fastmm_kernel's and cfastmm_kernel's (kmvp_f32mm_model)")
    geo = cloud_geometry(y, xa, same)
    block = max(1, 2 ** 21 // max(1, M))
    parts = [_block(kernel, y, xa, b, normalize_rows, path, same or same_global, rows[r0:r0 + block], chunk, seg_len,
                    j_offset, M if M_total is None else M_total, rounding, geo)
             for r0 in range(0, max(len(rows), 1), block)]
    return Model(*(np.concatenate(f) for f in zip(*parts)))


def _block(kernel, y, xa, b, normalize_rows, path, own, rows, chunk, seg_len, j_offset, M_total, rounding, geo):
    M, D = y.shape
    x = xa[rows]
    n = len(rows)
    with np.errstate(invalid="ignore", over="ignore"):
        s = kmvp_oracle.sqdists_block(x, y, False)                  # the difference form: s in the caller's units
    # the pair of the target's flat index: 1/r drops it, exp(-r) on the sources themselves has k = 1 exactly
    jz = kmvp_oracle.zero_column(rows, M_total) - j_offset
    hit = (jz >= 0) & (jz < M)
    own_i, own_j = np.nonzero(hit)[0], jz[hit]
    flagged = np.zeros(n, dtype=bool)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        if kernel == "gaussian":
            k = np.exp(-s)
        elif kernel == "absolute-exponential":
            k = np.exp(-np.sqrt(s))
        else:
            k = 1.0 / np.sqrt(s)
            k[own_i, own_j] = 0.0
        kf = np.where(np.isfinite(k), k, 0.0)                       # inf sources contribute 0; NaN stays NaN in num
        babs = np.abs(b)
        num = k @ b
        mass = kf @ babs
        den = k.sum(axis=1, keepdims=True)
    nonfinite = ~np.isfinite(num).all(axis=1) | (normalize_rows & ~(den[:, 0] > 0))
    z = np.zeros((n, 1))
    if not rounding:
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            value = num / den if normalize_rows else num
        return Model(value, z, mass, z, z, z, z, flagged, ~np.isfinite(value).all(axis=1))

    c = kernel_constant(kernel)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        ss = s * c * c                                              # scaled squared distance
        r = np.sqrt(ss)
        if path == "fast":
            e_s = expansion_error(x, y, geo["mid"], c, r, 6)        # six norm columns after the 6 D products
        else:
            e_s = centred_error(r, ss, geo["ydiam"], c, D)
        if kernel == "gaussian":
            L = np.log(2.0) * e_s + TRANS
        elif kernel == "absolute-exponential":
            L = absexp_log_error(e_s, r)
        else:
            ratio = e_s / ss
            L = invdist_log_error(ratio)
            live = kf != 0.0
            flagged |= ((ratio >= FLAG_FAST_1R if path == "fast" else ratio > FLAG_1R) & live).any(axis=1)
        L = np.where(np.isfinite(L), L, 0.0)
        pair_rel = np.expm1(L)
        if kernel == "absolute-exponential" and own:
            pair_rel[own_i, own_j] = 0.0                            # k = 1 exactly (fast_kernel: the own-pair rule;
            #                                                         cfast_kernel: s = 0 exactly in the exact branch)
        pair_each = kf * pair_rel
        if kernel != "inverse-distance":                            # v_exp_f32 returns 0 below the smallest normal number
            pair_each = np.where(kf * (1.0 - pair_rel) < FLUSH, np.maximum(pair_each, kf), pair_each)
        lam_n = LAM * np.sqrt(acc_roundings(path, D, M, chunk, seg_len)) * U_RNE
        under = CHAIN_TILE * -(-M // 32) * 2.0 ** -150               # denormal results of the row's fp32 operations
        pair = pair_each @ babs
        acc = lam_n * mass + 2.0 ** -50 * mass + under
        band_num = K_BAND * (pair + acc)
    if not normalize_rows:
        return Model(num, band_num, mass, pair, z, z, acc, flagged, nonfinite)
    ksum = kf.sum(axis=1, keepdims=True)
    bden = K_BAND * (pair_each.sum(axis=1, keepdims=True) + lam_n * ksum + 2.0 ** -50 * ksum + under)
    with np.errstate(divide="ignore", invalid="ignore"):
        value = num / den
        room = den - bden
        band = (band_num + np.abs(value) * bden) / room
        flagged |= ~(room > 0).all(axis=1)
        return Model(value, band, mass / den, pair / den, z, z, acc / den, flagged, nonfinite)
