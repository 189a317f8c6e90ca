"""Per-element model of lowd_cutoff_kernel with Wendland's kernels (csrc/kmvp_lowd_cutoff.hpp wendland_value) -- TEST
INFRASTRUCTURE ONLY.  Built the way oracle/kmvp_lowd_model.py builds its own: `value` is the float64 (extended, where the
machine has it, for float64 contexts) product of the inputs as rounded to the working precision, `band` an upper bound
derived from the code, term by term; nothing is fitted to kernel output.  u = unit(precision): one rounding to nearest.

The sequence (include/kmvp.h), in the working precision:
    s  = knn_sqdist                  |s' - s| <= gamma_s s, gamma_s = (1 + u)^(D + 2) - 1 (+ D eta / s), as in kmvp_lowd_model
    q  = s * iR2                     iR2 = (real)(1 / R^2): its rounding and the product's, 2 u
    t  = sqrt(q)                     float32: v_sqrt_f32 at TRANS; float64: q * rsq(q) in the one-step form, RSQ64 + u
                                     rho_t = (gamma_s + 2 u) / 2 + TRANS          (float32)
                                     rho_t = (gamma_s + 2 u) / 2 + RSQ64 + u      (float64)
    w  = max(1 - t, 0)               one rounding delta (exact for t >= 1/2, Sterbenz): w' = (1 - t') (1 + delta)
    k  = phi(t') (1 + delta)^p (1 + roundings of the products and fmas)
so  |k' - k| <= sup |phi'| * t rho_t + n_ops u k',  the supremum over the interval t' can lie in.  With w_hi = min(1, w + dt),
t_hi = t + dt, dt = t rho_t, and |phi'| increasing in t and in w separately:
    C2  phi' = -20 t w^3                  |phi'| <= 20 t_hi w_hi^3
    C4  phi' = -(56/3) t w^5 (5 t + 1)    |phi'| <= (56/3) t_hi w_hi^5 (5 t_hi + 1)
(the bound at w_hi also covers t > 1, where k = 0 and k' may be as large as phi(1 - dt)).  n_ops, each rounding counted with
the power it enters k:
    C2  delta 4 (0 for t >= 1/2); u2 = w w enters squared: 2; u2 u2: 1; fma(4, t, 1): 1; the last product: 1       -> 9 (5)
    C4  delta 6 (0 for t >= 1/2); u2 enters cubed: 3; two products: 2; 35/3 rounded, two fmas of positive terms: 3;
        the last product: 1                                                                                          -> 15 (9)
The select k = s <= r2 ? k : 0 with r2 = (real)(R R): a pair with |s - R^2| <= (gamma_s + 2 u) s may be classified either
way and is charged its whole k (there k = O(u^4): the analogue of kmvp_lowd_model's flush rule).  Pad records, pairs beyond
the support and NaN distances give exactly 0.
Accumulation, folds and normalised rows: kmvp_lowd_model's formulas, on the chain of a row's pairs inside the support
(outside pairs add exact zeros) -- float32: `chunk` walked records at most between two folds, the folds' own float64
additions charged as folds * 2^-53 * mass (test_gpu_cutoff.model_rows); float64: one chain.
band = K_BAND (pair + acc), K_BAND = 2 over the second-order terms the bounds drop.
"""
from collections import namedtuple

import numpy as np

import kmvp_lowd_model as lm
import wendland_reference as wr
from kmvp_lowd_model import K_BAND, RSQ64, TRANS, chain_length, unit

Model = namedtuple("Model", "value band mass")
N_OPS = {"wendland-c2": (4, 5), "wendland-c4": (6, 9)}      # (the subtraction's power, every other rounding)


def gamma_s(precision, s, D):
    u = unit(precision)
    eta = 2.0 ** -150 if np.dtype(precision) == np.float32 else lm.ETA64
    with np.errstate(divide="ignore", invalid="ignore"):
        live = np.isfinite(s) & (s > 0)
        return np.where(live, np.expm1((D + 2) * np.log1p(u)) + D * eta / np.where(live, s, 1.0), 0.0)


def pair_bound(kernel, precision, s, R, D):
    """(k, each): the float64 value of every pair from its float64 squared distance s, and the bound on |k' - k|."""
    f32 = np.dtype(precision) == np.float32
    u = unit(precision)
    with np.errstate(invalid="ignore", over="ignore"):
        fin = np.isfinite(s)
        ss = np.where(fin, s, 4.0 * R * R)                  # (non-finite distances: far outside, k = k' = 0)
        t = np.sqrt(ss) / R
        k = wr.values(kernel, t)
        gs = gamma_s(precision, ss, D)
        rho_t = (gs + 2 * u) / 2 + (TRANS if f32 else RSQ64 + u)
        dt = t * rho_t
        w_hi = np.clip(1.0 - t + dt, 0.0, 1.0)
        t_hi = t + dt
        if kernel == "wendland-c2":
            slope = 20.0 * t_hi * w_hi ** 3
        else:
            slope = (56.0 / 3.0) * t_hi * w_hi ** 5 * (5.0 * t_hi + 1.0)
        dphi = slope * dt
        sub, rest = N_OPS[kernel]
        n_ops = np.where(t < 0.5, sub + rest, rest)
        each = dphi + n_ops * u * (k + dphi)
        edge = np.abs(ss - R * R) <= (gs + 2 * u) * ss
        each = np.where(edge, np.maximum(each, k + dphi), each)
        each = np.where(fin, each, 0.0)
    return np.where(fin, k, 0.0), each


def restate(kernel, y, x, R, precision):
    """wendland_value after knn_sqdist, operation by operation in numpy's `precision` -- k' (N, M) as the kernel forms it,
    the select included.  An fma is the float64 result rounded once more (double rounding: below 2^-29 u)."""
    real = np.dtype(precision).type
    y = np.asarray(y, dtype=real)
    xa = y if x is None else np.asarray(x, dtype=real)

    def fma(a, b, c):
        return (a.astype(np.longdouble) * b.astype(np.longdouble) + c.astype(np.longdouble)).astype(real)

    with np.errstate(invalid="ignore", over="ignore"):
        df = xa[:, 0:1] - y[None, :, 0]
        s = df * df
        for d in range(1, y.shape[1]):
            df = xa[:, d:d + 1] - y[None, :, d]
            s = fma(df, df, s)
        r2, iR2 = real(R * R), real(1.0 / (R * R))
        t = np.sqrt(s * iR2)
        u = np.maximum(real(1) - t, real(0))
        u2 = u * u
        one = np.ones_like(t)
        if kernel == "wendland-c2":
            k = (u2 * u2) * fma(np.full_like(t, 4), t, one)
        else:
            k = ((u2 * u2) * u2) * fma(t, fma(t, np.full_like(t, real(35.0 / 3.0)), np.full_like(t, 6)), one)
        return np.where(s <= r2, k, real(0))


Pairs = namedtuple("Pairs", "i j kw k each N M D")
MARGIN = 1e-5      # pairs with s > R^2 (1 + MARGIN) are beyond every rounding's reach (t rho_t < 1e-6 t): k = k' = 0 exactly


def pairs(kernel, y, x, R, precision):
    """The pairs that can contribute, as index lists: (i, j), the value kw in the widest float type, its float64 rounding k
    and the bound `each`.  y, x as product() takes them.  Computed once per (cloud, kernel, R, precision) and shared."""
    precision = np.dtype(precision)
    y = np.asarray(y, dtype=precision).astype(np.float64)
    xa = y if x is None else np.asarray(x, dtype=precision).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        i, j = np.nonzero(wr.sqdists(xa, y) <= R * R * (1.0 + MARGIN))          # (NaN and infinite distances: never)
        wide = precision == np.float64 and lm.HAVE_LONGDOUBLE
        W = np.longdouble if wide else np.float64
        df = xa[i].astype(W) - y[j].astype(W)
        sw = (df * df).sum(axis=1)
        kw = wr.values(kernel, np.sqrt(sw) / W(R))
    k, each = pair_bound(kernel, precision, sw.astype(np.float64), R, y.shape[1])
    return Pairs(i, j, kw, k, each, xa.shape[0], y.shape[0], y.shape[1])


def _rows(i, v, N):
    """Row sums of the per-pair values v (P, E) in v's own dtype."""
    out = np.zeros((N, v.shape[1]), dtype=v.dtype)
    np.add.at(out, i, v)
    return out


def product(kernel, y, x, b, R, normalize_rows=False, *, precision=np.float32, chunk=512, folds=0, prs=None):
    """Modelled result of kmvp_wendland_<c>_cutoff and its per-element band.  y (M, D) sources, x (N, D) targets (None: the
    same points), b (M, E) signal (None: density estimation), all rounded to `precision` first; chunk: the "chunk" option;
    folds: an upper bound on a row's folds into float64 (float32 only); prs: pairs() of the same arguments, to share.
    Model(value, band, mass), (N, E) each; a normalised row with nothing inside is NaN with band 0."""
    precision = np.dtype(precision)
    f32 = precision == np.float32
    p = pairs(kernel, y, x, R, precision) if prs is None else prs
    b = np.ones((p.M, 1)) if b is None else np.asarray(b, dtype=precision).astype(np.float64)
    wide = not f32 and lm.HAVE_LONGDOUBLE
    bj = b[p.j]
    num = _rows(p.i, p.kw[:, None] * bj.astype(p.kw.dtype), p.N)
    den = _rows(p.i, p.kw[:, None], p.N)
    with np.errstate(divide="ignore", invalid="ignore"):
        value = (num / den if normalize_rows else num).astype(np.float64)
    num, den = num.astype(np.float64), den.astype(np.float64)
    u = unit(precision)
    eta = 2.0 ** -150 if f32 else lm.ETA64
    mass = _rows(p.i, p.k[:, None] * np.abs(bj), p.N)
    # the longest chain of a row in the working precision: its pairs that may be inside, cut by the folds in float32
    live = _rows(p.i, (p.each > 0).astype(np.float64)[:, None], p.N)
    n_chain = np.maximum(1.0, np.minimum(live, chain_length("lowd", precision, p.M, chunk, feed=0)) if f32 else live)
    acc_rel = np.minimum(n_chain, lm.LAM * np.sqrt(n_chain)) * u + 2.0 ** -50 + (folds * 2.0 ** -53 if f32 else 0.0)
    own = 1.0 if wide or f32 else 2.0
    band_num = own * K_BAND * (_rows(p.i, p.each[:, None] * np.abs(bj), p.N) + acc_rel * mass + live * eta)
    if not normalize_rows:
        return Model(num, band_num, mass)
    ksum = _rows(p.i, p.k[:, None], p.N)
    bden = own * K_BAND * (_rows(p.i, p.each[:, None], p.N) + acc_rel * ksum + live * eta)
    empty = den == 0                     # nothing inside: 0 / 0 = NaN in the kernel and in `value`, nothing to bound
    room = den - bden
    if not (room[~empty] > 0).all():
        raise ValueError("a normalised row's denominator does not stay above its own band")
    with np.errstate(divide="ignore", invalid="ignore"):
        band = np.where(empty, 0.0, (band_num + np.abs(value) * bden) / room)
        return Model(value, band, mass / den)
