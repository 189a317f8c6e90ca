"""Float64 model of the cell-form Gaussian products -- TEST INFRASTRUCTURE ONLY.

cell_kernel (kmvp_cell.hpp), cellmm_kernel and cellmm16_kernel (kmvp_cellmm.hpp, both bodies of cellmm16_body) and
cell64_kernel (kmvp_cell64.hpp) with their packers (kmvp_cell_pack.hpp, kmvp_cellmm_pack.hpp, kmvp_cell64_pack.hpp) and the
host side (run_product_cell, run_product_cellmm, run_product_cell64).  The contract is that of kmvp_f32_model.py and
kmvp_lowd_model.py: `value` is the float64 product of the caller's inputs as rounded to the working precision (float64
kernels: formed in extended precision, kmvp_lowd_model), `band` a per-element upper bound derived from the code, term by
term, below; nothing is fitted to kernel output.  u = 2^-24 (float32 kernels) or 2^-53 (cell64_kernel).

The cells are DATA here: the model takes the layout that kmvp_cell_layout reads back from the library (the cell of every
source and target, the stored centres, sigma_b) and restates neither the grid rule nor the count cut.  The factorisation

    exp(-|x - y|^2) = U_i(S) W_j(T) exp(t_ij),   x = c_T + d,  y = c_S + e,  Delta = c_T - c_S,
    U_i(S) = exp(-|d + Delta|^2),  W_j(T) = exp(e.(2 Delta - e)),  t_ij = 2 d.e

is exact for ANY centres, so all the model needs from the layout are the preconditions it checks itself and RAISES:
  every point is in exactly one cell (ids -1 and -2 of kmvp_cell_layout name the point);
  |2 d.e| <= CELL_T_MAX (CELL64_T_MAX) for every pair of a target cell and a source cell, from their max |d_c| and max
    |e_c| per axis -- with the room the stored float32 centres themselves take: 4 u (|c_T| + |c_S|) (max|d| + max|e|) per
    axis, and 2^-18 of the bound for the float32 cell side;
  W_j(T) <= 2^CMM_MAX_WLOG2 and every first-order entry of A inside f16 where cellmm_kernel / cellmm16_kernel run;
  U and W are computed from finite arguments (no overflow of W);
  a normalised row's denominator stays above its own band.

Terms (float32 kernels; a = sum_c |e_c| (2 |Delta_c| + |e_c|), T1 = sum_c |d_c 2 e_c| >= |t|, T2 = T1^2 / 2):

* offsets and centres.  d = fl(x - c_T), e = fl(y - c_S) (the packers: one subtraction each), Delta = fl(c_T - c_S) -- the
  SAME rounded difference in U (new_cell: dl + (cT - cs)) and in W (D1 = (cT - cs) log2 e; cell_kernel: 2 (cT - hc)), so
  the kernels factorise exp(-|Delta + d - e|^2) exactly and what is lost against |x - y|^2 is
  L_off = 2 u sum_c |x_c - y_c| (|Delta_c| + |d_c| + |e_c|).
* U_i(S).  df = fl(d + Delta): u |df|; s2 = fma(df, df, s2) three times: non-negative terms, 3 u s2; s2 * -log2 e: the
  constant and the product, 2 u; v_exp_f32 at TRANS:  L_U = 7 u s2 + TRANS.  v_exp_f32 returns 0 below FLUSH = 2^-126: a
  pair whose U (1 - its bound) may be below FLUSH is lost whole, with every pair of its fold, and is charged with k
  itself, as kmvp_f32_model does -- here at kernel values up to W = 2^8 times larger than on the difference form.
* W_j(T).  cellmm / cellmm16: arg = fma(f_x, D1_x, fma(f_y, D1_y, fma(f_z, D1_z, g))), f = 2 e exact, g = fl(fl(|e|^2)
  -log2 e) (pack_cellmm_points_kernel: three roundings of non-negative terms, the constant, the product: 5 u |e|^2),
  D1 = fl(Delta log2 e) (2 u), three FMA roundings of partial sums below sum_c |f_c D1_c| + |g|:  L_W = 8 u a + TRANS.
  cell_kernel: arg = fma(e_c, fl(2 Delta_c - e_c), arg) three times, then * log2 e:  L_W = 6 u a + TRANS.  At W = 2^8
  (a = 5.5) this is 2.7e-6: |arg| u matters.  W b: one rounding, u (b sigma_b is exact: a power of two).
* remainder, truncation: |exp(t) - 1 - t - t^2 / 2| <= |t|^3 / 6 e^|t| from the pair's own t.
* remainder, cell_kernel (16 bf16 slots, one v_mfma_f32_32x32x16_bf16 from zero): d_h = bf16(d), d_m = bf16(d - d_h) and
  the same for 2 e: 2^-18 each side and the dropped d_m e_m, 3 2^-18 T1; the quadratic monomials one bf16 term a side
  (2^-9 each, after two fp32 roundings each): (2^-8 + 2^-17 + 4 u) T2; the MFMA's sixteen products are exact in fp32 and
  summed as a k-ordered chain with one rounding each (the ASSUMPTION of kmvp_f32mm_model): 16 u (1 + T1 + T2).
* remainder, cellmm / cellmm16 (15 f16 slots, accumulating MFMAs).  Targets (cellmm_target_operand): s = 64 d exact,
  s_h = f16(s) and s_m = f16(s - s_h) to nearest: 2^-22 |s|, and 2^-25 absolutely where s_m is a denormal f16.  Sources
  (cellmm16_operand): u1 = fl(f_c W b); v_cvt_pkrtz rounds toward zero: the hi part c1 is exact by construction (its
  remainder is formed exactly: u1 - c1, cellmm16: fma(f_c, W b, -c1)), the mid part loses <= 2^-10 of itself = 2^-20 |u1|,
  and < 2^-24 absolutely where it is a denormal f16 -- the ABSOLUTE quantum; the dropped s_m x mid: 2^-21.  Linear part:
  (2^-22 + 2^-21 + 2^-20 + u) T1.  Quadratic slots: one RTZ product a side on the sources (2^-10, two fp32 roundings), one
  round-to-nearest on the targets (2^-11, two roundings): (2^-10 + 2^-11 + 4 u) T2.  The f16 x f16 products are exact in fp32.
  The absolute quantum in the result's units: a source entry is off by < 2^-24 / sigma_b whatever its size, against target
  entries |d_c|, d_c^2 / 2, |d_a d_b| (the 2^6 cancels):  Q_ij = [b_j != 0] 2^-24 / sigma_b (|d|_1 + |d|_1^2 / 2), times
  U_i(S), summed over the sources -- the term that makes rows fed by small |b| honest: their entries sink into f16
  denormals because sigma_b is sized from max |b| alone.  The targets' denormals: 2^-31 W |b| (|f|_1 + |f|_1^2).
  sigma_b is the layout's, of the LAST column the library ran (for normalised rows the denominator's); another column's is
  taken from the ratio of the columns' max |b| and one power of two lower (the rule's own mantissa is not restated).
* accumulation, cell_kernel.  Per source tile and lane half two chains of eight FMAs from zero, p0 + p1: 9 u of the
  tile's own sum; acc = fma(U, p0 + p1, acc): one rounding of the running sum per tile, over the T_c tiles of chunk_stages =
  max(1, chunk / 128) stages of four between two folds into fp64: min(T_c, lam sqrt T_c) u mass (lam = 8: the probabilistic
  rule of kmvp_f32mm_model).  fp32 denormals are on: 2^-149 per operation.
* accumulation, cellmm / cellmm16.  The accumulators are never reset; a cell's share is (v - vprev) + s0.  Running |v| is
  bounded by V_i = sum_j W_j(T) |b_j| (|t_ij| + t_ij^2 / 2) over the WHOLE source list (no segment plan restated; the
  pair's own t, which is what the accumulators hold, not T_MAX).  Per fold of a cell S of n_S tiles:
    the MFMAs' k-ordered chains, 16 roundings per tile of accumulators below V_i: min(16 n_S, lam sqrt(16 n_S)) u V_i;
    the row sums of v and of vprev (four levels of adds and the cross-half add, cellmm16: fold4's butterfly -- the same
      count in another order): 2 x 5 u V_i.  A row sum's rounding does NOT cancel between the fold that reads it as v and
      the next that reads it as vprev: the two are multiplied by different U;
    s0: the Kahan sum over the cell's tiles, 2 u + 2 n_S u^2 (cellmm16: fmaf(bq, wexp, -S0c), one rounding less), the five
      DPP adds and the add of the two readlanes: 6 u; x 64 exact;  (v - vprev) + s0, x U: 3 u;  together 11 u + 2 n_S u^2
      of P_iS = sum_{j in S} W_j |b_j| (1 + |t| + t^2 / 2);
    times U_i(S); the product U x (...) is a denormal fp32 below 2^-126: 2^-149 / (64 sigma_b) per fold.
  Segments, the REST list and the gather are fp64: 2^-50 mass.
* cell64_kernel (u = 2^-53; exp: kmvp_lowd_model.EXP64, ASSUMED to hold for kexp_neg_f64 at negative arguments, where W >
  1).  L_off as above; L_U = 7 u s2 + EXP64; L_W = 6 u a + EXP64 (fma(m, fma(m, -1/4, D), ...), m = 2 e); t: three
  roundings, 3 u T1; cell64_exp: the degree-7 Horner form, t^8 / 8! e^|t| truncation and 8 u e^|t| for its seven FMAs;
  acc_c = fma(p, w, acc_c) over the cell's n sources: min(n, lam sqrt n) u P_iS; acc = fma(U, acc_c, acc) over the cells:
  min(n_S, lam sqrt n_S) u mass; segments: 2^-48 mass.  The value is formed in extended precision; without such a type
  the band is doubled.
* normalised rows: band = (band_num + |value| band_den) / (den - band_den), the denominator the same sum with b = 1.

band = K_BAND (pair + acc).  rounding=False: the plain float64 product, no band, no layout needed.

Parity status: no reference counterpart; checked against kmvp_oracle.product with rounding disabled, and against numpy
emulations of the kernels' steps with and without defects, by tests/test_cell_model.py.
"""
import numpy as np

import kmvp_oracle
from kmvp_f32_model import FLUSH
from kmvp_f32mm_model import K_BAND, LAM, TRANS, U_RNE, Model
from kmvp_lowd_model import EXP64, HAVE_LONGDOUBLE, U64

PATHS = ("cell", "cellmm", "cellmm16", "cell64")
CELL_T_MAX = float(np.float32(0.016))     # kmvp_cell.hpp
CELL64_T_MAX = 0.05                       # kmvp_cell64.hpp
CMM_MAX_WLOG2 = 8                         # kmvp_cellmm.hpp
CELL_TILE, CELL64_TILE = 32, 128
F16_MAX = 65504.0
C_W = {"cell": 6.0, "cellmm": 8.0, "cellmm16": 8.0, "cell64": 6.0}


def _rule(n):
    """min(n, lam sqrt n): the deterministic count of roundings or the probabilistic rule, whichever is smaller."""
    n = np.asarray(n, dtype=np.float64)
    return np.minimum(n, LAM * np.sqrt(n))


def check_layout(layout, M, N):
    """Every point in exactly one cell; raises with the point named."""
    for side, n in (("source", M), ("target", N)):
        ids = np.asarray(layout[side + "_cell"])
        cen = np.asarray(layout[side + "_centres"])
        if ids.shape != (n,):
            raise ValueError(f"layout: {side}_cell has shape {ids.shape}, expected ({n},)")
        bad = np.nonzero((ids < 0) | (ids >= len(cen)))[0]
        if bad.size:
            what = {-1: "is in no cell", -2: "is in more than one cell"}.get(int(ids[bad[0]]), "names a cell that does not exist")
            raise ValueError(f"layout: {side} {bad[0]} {what} ({bad.size} such points)")


def offsets(points, ids, centres, precision):
    """d = fl(x - c) in the working precision, as the packers form it (one subtraction), as float64."""
    p = np.asarray(points, dtype=precision)
    c = np.asarray(centres, dtype=np.float64)[ids][:, :p.shape[1]].astype(precision)
    with np.errstate(invalid="ignore", over="ignore"):
        return (p - c).astype(np.float64)


def check_cells(path, d, e, tcell, scell, tcen, scen, finite_t):
    """|2 d.e| <= T_MAX for every pair of cells from their max |d_c| and max |e_c|; raises with the cells named."""
    D = d.shape[1]
    t_max = CELL64_T_MAX if path == "cell64" else CELL_T_MAX
    u = U64 if path == "cell64" else U_RNE
    dmax = np.zeros((len(tcen), D))
    np.maximum.at(dmax, tcell[finite_t], np.abs(d[finite_t]))
    emax = np.zeros((len(scen), D))
    np.maximum.at(emax, scell, np.abs(e))
    t = 2.0 * dmax @ emax.T
    room = 4 * U_RNE * ((np.abs(tcen[:, :D]) @ emax.T) + dmax @ np.abs(scen[:, :D]).T + (np.abs(tcen[:, :D]) * dmax).sum(1)[:, None]
                        + (np.abs(scen[:, :D]) * emax).sum(1)[None, :])
    over = t > t_max * (1 + 2.0 ** -18) + room + 8 * u
    if over.any():
        T, S = np.unravel_index(int(np.argmax(t - room)), t.shape)
        raise ValueError(f"layout: |2 d.e| reaches {t[T, S]:.6g} > {t_max} between target cell {T} (centre {tcen[T]}, max |d| {dmax[T]}) "
                         f"and source cell {S} (centre {scen[S]}, max |e| {emax[S]})")


def column_scales(layout, b, density):
    """sigma_b of every column (and of the denominator's b = 1 launch, last) from the layout's -- that of the LAST launch --
    by the ratio of the columns' max |b|, one power of two lower for every column but the last."""
    sig = float(layout.get("sigma_b", 0.0))
    if not sig > 0:
        raise ValueError("layout: sigma_b is missing (no cellmm_kernel / cellmm16_kernel product has run)")
    with np.errstate(invalid="ignore"):
        bmax = np.ones(1) if density else np.abs(b).max(axis=0)
    tops = np.concatenate((bmax, [1.0]))            # (E,) then the denominator's launch

    def fe(v):
        return np.frexp(v)[1] if np.isfinite(v) and v > 0 else None

    def scales(last):
        out = np.ones(len(tops))                      # (launches behind the last one did not run)
        for c, v in enumerate(tops[:last + 1]):
            if c == last:
                out[c] = sig
            elif fe(v) is None:
                out[c] = 1.0                                    # (cellmm_scale_kernel: ex = 0 for max |b| = 0, inf or NaN)
            elif fe(tops[last]) is None:
                raise ValueError("sigma_b of the last column says nothing about the others: its max |b| is 0 or not finite")
            else:
                out[c] = sig * 2.0 ** (fe(tops[last]) - fe(v) - 1)
        return out
    return scales


def cell_product(y, x=None, b=None, normalize_rows=False, *, path="cellmm16", layout=None, chunk=512, rows=None, rounding=True):
    """Modelled result of run_product_cell / run_product_cellmm / run_product_cell64 and its per-element band.

    y (M, D) sources, x (N, D) targets (None: the same points), b (M, E) signal (None: density estimation), rounded to the
    working precision first (float64 for path "cell64", else float32).  path: "cell" (cell_kernel), "cellmm" (cellmm_kernel),
    "cellmm16" (cellmm16_kernel) or "cell64".  layout: the dict of kmvp_cell_layout (_lib.Context.cell_layout): source_cell,
    target_cell, source_centres, target_centres and, for the cellmm paths, sigma_b.  chunk: the "chunk" option (cell_kernel).
    rows: target indices to model.  rounding=False: the float64 product, no band.
    Returns Model(value, band, mass, pair, tsplit, bsplit, acc (n, E) each, flagged (n,), nonfinite (n,)); tsplit holds the
    absolute f16 quantum's share of `pair` (cellmm paths), bsplit is zero, no row is ever flagged."""
    if path not in PATHS:
        raise ValueError(path)
    precision = np.dtype(np.float64 if path == "cell64" else np.float32)
    y = np.asarray(y, dtype=precision).astype(np.float64)
    xa = y if x is None else np.asarray(x, dtype=precision).astype(np.float64)
    M, D = y.shape
    N = xa.shape[0]
    rows = np.arange(N, dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    if b is None and normalize_rows:
        raise ValueError("normalised density rows are ones by definition: no kernel runs")
    density = b is None
    b = np.ones((M, 1)) if density else np.asarray(b, dtype=precision).astype(np.float64)
    if b.shape[1] != 1 and path in ("cell", "cell64"):
        raise ValueError("one signal column: several are cellmm_kernel's and cellmm16_kernel's")
    geo = None
    if rounding:
        if layout is None:
            raise ValueError("the band needs the cell layout (kmvp_cell_layout)")
        check_layout(layout, M, N)
        scell, tcell = np.asarray(layout["source_cell"], np.int64), np.asarray(layout["target_cell"], np.int64)
        scen = np.asarray(layout["source_centres"], np.float64).reshape(-1, 3)
        tcen = np.asarray(layout["target_centres"], np.float64).reshape(-1, 3)
        if not np.isfinite(y).all():
            raise ValueError("a source coordinate is not finite: the cell form refuses such clouds")
        e = offsets(y, scell, scen, precision)
        d = offsets(xa, tcell, tcen, precision)
        finite_t = np.isfinite(d).all(axis=1)
        check_cells(path, d, e, tcell, scell, tcen, scen, finite_t)
        order = np.argsort(scell, kind="stable")               # sources cell by cell: the folds' sums are reduceat's
        cells, first, count = np.unique(scell[order], return_index=True, return_counts=True)
        scales = column_scales(layout, b, density) if path in ("cellmm", "cellmm16") else None
        geo = dict(e=e[order], d=d, scell=np.searchsorted(cells, scell[order]), tcell=tcell, scen=scen[cells][:, :D], tcen=tcen[:, :D],
                   first=first, count=count, order=order, scales=scales, E=b.shape[1])
    block = max(1, 2 ** 19 // max(1, M))
    parts = [_block(path, precision, y, xa[rows[r0:r0 + block]], rows[r0:r0 + block], b, normalize_rows, chunk, rounding, geo)
             for r0 in range(0, max(len(rows), 1), block)]
    return Model(*(np.concatenate(f) for f in zip(*parts)))


def _value(precision, x, y, b):
    """Numerator, denominator and kernel values of a block: float64, or extended precision rounded once for float64 inputs."""
    wide = precision == np.float64 and HAVE_LONGDOUBLE
    W = np.longdouble if wide else np.float64
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        s = kmvp_oracle.sqdists_block(x.astype(W), y.astype(W), False)
        k = np.exp(-s)
        num = (k @ b.astype(W)).astype(np.float64)
        den = k.sum(axis=1, keepdims=True).astype(np.float64)
    return num, den, k.astype(np.float64), wide


def _block(path, precision, y, x, rows, b, normalize_rows, chunk, rounding, geo):
    n, E = len(rows), b.shape[1]
    num, den, k, wide = _value(precision, x, y, b)
    with np.errstate(invalid="ignore", divide="ignore"):
        value = num / den if normalize_rows else num
    babs = np.abs(b)
    kf = np.where(np.isfinite(k), k, 0.0)
    with np.errstate(invalid="ignore"):
        mass = kf @ babs
    nonfinite = ~np.isfinite(value).all(axis=1)
    flagged = np.zeros(n, dtype=bool)
    z = np.zeros_like(num)
    if not rounding:
        return Model(value, z, mass / den if normalize_rows else mass, z, z, z, z, flagged, nonfinite)

    f64 = path == "cell64"
    mm = path in ("cellmm", "cellmm16")
    u = U64 if f64 else U_RNE
    trans = EXP64 if f64 else TRANS
    o = geo["order"]
    ys, bs = y[o], babs[o]
    e, scell, first, count = geo["e"], geo["scell"], geo["first"], geo["count"]
    d = np.where(np.isfinite(geo["d"][rows]), geo["d"][rows], 0.0)           # (a NaN target's row is non-finite: no band)
    xs = np.where(np.isfinite(x), x, 0.0)
    cT = geo["tcen"][geo["tcell"][rows]]
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        # per (target, source cell): Delta as the kernels round it, U
        delta = (cT[:, None, :].astype(precision) - geo["scen"][None, :, :].astype(precision)).astype(np.float64)   # (n, nS, D)
        df = d[:, None, :] + delta
        s2 = (df * df).sum(axis=2)
        U = np.exp(-s2)
        relU = np.expm1(7 * u * s2 + trans)
        flush = np.zeros_like(U, dtype=bool) if f64 else U * (1.0 - relU) < FLUSH
        # per pair
        dl = delta[:, scell, :]                                              # (n, M, D)
        ea = np.abs(e)[None, :, :]
        a = (ea * (2 * np.abs(dl) + ea)).sum(axis=2)
        argw = (e[None, :, :] * (2 * dl - e[None, :, :])).sum(axis=2)
        if not np.isfinite(argw).all() or argw.max(initial=0.0) > 80.0:
            raise ValueError("W_j(T) overflows or is not finite on this layout")
        Wj = np.exp(argw)
        if mm and Wj.max(initial=0.0) > 2.0 ** CMM_MAX_WLOG2 * (1 + 2.0 ** -10):
            i, j = np.unravel_index(int(np.argmax(Wj)), Wj.shape)
            raise ValueError(f"layout: W = {Wj[i, j]:.6g} > 2^{CMM_MAX_WLOG2} between target cell {geo['tcell'][rows[i]]} and "
                             f"source cell {scell[j]} where cellmm runs")
        t = 2.0 * d @ e.T
        T1 = 2.0 * np.abs(d) @ np.abs(e).T
        T2 = 0.5 * T1 * T1
        et = np.exp(np.abs(t))
        r_abs = np.abs(xs[:, None, :] - ys[None, :, :])
        L_off = 2 * u * (r_abs * (np.abs(dl) + np.abs(d)[:, None, :] + ea)).sum(axis=2)
        Up = U[:, scell]
        rel = np.expm1(L_off) + relU[:, scell] + np.expm1(C_W[path] * u * a + trans) + u
        if f64:
            R = np.abs(t) ** 8 / 40320.0 * et + (3 * T1 + 8) * u * et
        elif mm:
            R = np.abs(t) ** 3 / 6.0 * et + (2.0 ** -22 + 2.0 ** -21 + 2.0 ** -20 + u) * T1 + (2.0 ** -10 + 2.0 ** -11 + 4 * u) * T2
        else:
            R = np.abs(t) ** 3 / 6.0 * et + 3 * 2.0 ** -18 * T1 + (2.0 ** -8 + 2.0 ** -17 + 4 * u) * T2 + 16 * u * (1 + T1 + T2)
        each = Up * Wj * (np.exp(t) * rel + R)                              # per unit |b_j|
        each = np.where(flush[:, scell], np.maximum(each, kf[:, o]), each)
        UW = Up * Wj
        d1 = np.abs(d).sum(axis=1)
        f1 = 2.0 * np.abs(e).sum(axis=1)
        tiles = -(-count // CELL_TILE)
        n_cells = len(count)

        def column(bcol, sigma):
            """pair, quantum share, acc of one launch: bcol (M,) = |b| in cell order, sigma its sigma_b."""
            pair = each @ bcol
            quantum = np.zeros(n)
            if mm:
                live = (bcol != 0).astype(np.float64)
                quantum = 2.0 ** -24 / sigma * (d1 + 0.5 * d1 * d1) * (Up @ live) + 2.0 ** -31 * (UW @ (bcol * (f1 + f1 * f1)))
                top = float(np.nanmax(Wj * (bcol * 2.0 * np.abs(e).max(axis=1))[None, :], initial=0.0)) * sigma
                if top > F16_MAX:
                    raise ValueError(f"a first-order entry of A reaches {top:.6g}: outside f16 at sigma_b = {sigma}")
                V = (Wj * (np.abs(t) + 0.5 * t * t)) @ bcol                 # running |v|, whole source list
                P = np.add.reduceat(Wj * (1 + np.abs(t) + 0.5 * t * t) * bcol[None, :], first, axis=1)      # (n, nS)
                fold = (_rule(16 * tiles) + 10) * u * V[:, None] + (11 * u + 2 * tiles * u * u) * P
                acc = (U * fold).sum(axis=1) + 2.0 ** -50 * (kf[:, o] @ bcol) + n_cells * 2.0 ** -149 / (64 * sigma)
            elif f64:
                P = np.add.reduceat(Wj * et * bcol[None, :], first, axis=1)
                acc = (U * (_rule(count) * u * P)).sum(axis=1) + (_rule(n_cells) * u + 2.0 ** -48) * (kf[:, o] @ bcol)
            else:
                tc = min(max(1, chunk // 128) * 4, int(tiles.sum()))
                acc = (9 + _rule(tc)) * u * (kf[:, o] @ bcol) + 2.0 ** -50 * (kf[:, o] @ bcol) + 20 * int(tiles.sum()) * 2.0 ** -149
            return pair + quantum, quantum, acc

        own = 1.0 if wide or not f64 else 2.0
        scales = geo["scales"](E if normalize_rows else E - 1) if mm else np.ones(E + 1)
        cols = [column(bs[:, c], scales[c]) for c in range(E)]
        pair, quantum, acc = (np.stack([c[q] for c in cols], axis=1) for q in range(3))
        band_num = own * K_BAND * (pair + acc)
        if not normalize_rows:
            return Model(num, band_num, mass, pair, quantum, z, acc, flagged, nonfinite)
        pd, _, ad = column(np.ones(len(bs)), scales[E])
        bden = (own * K_BAND * (pd + ad))[:, None]
        room = den - bden
        if not (room[~nonfinite] > 0).all():
            raise ValueError("a normalised row's denominator does not stay above its own band (every pair may be flushed)")
        band = (band_num + np.abs(value) * bden) / room
        return Model(value, band, mass / den, pair / den, quantum / den, z, acc / den, flagged, nonfinite)
