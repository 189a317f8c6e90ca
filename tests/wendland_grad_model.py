"""Per-element model of lowd_cutoff_grad_kernel with Wendland's kernels (csrc/kmvp_lowd_cutoff_grad.hpp
wendland_grad_weight) -- TEST INFRASTRUCTURE ONLY.  Built the way tests/wendland_model.py builds its own: `value` is the
float64 (extended, where the machine has it, for float64 contexts) gradient on the inputs as rounded to the working
precision, `band` an upper bound derived from the code, term by term; nothing is fitted to kernel output.
u = unit(precision): one rounding to nearest.

    G[i, e, d] = c sum_j W(s_ij) b_je (x_id - y_jd),   C2: W = w^3, c = -20 / R^2;   C4: W = w^5 (5 t + 1), c = -56 / (3 R^2)

The sequence (include/kmvp.h), in the working precision; s, q, t and w = max(1 - t, 0) are wendland_value's, and so are
rho_t and dt = t rho_t (wendland_model's docstring):
    df_d = x_d - y_d, KEPT           one rounding, counted once inside gamma_s and once per factor of the pair product
    W  = Phi(t') (1 + delta)^p (1 + roundings of the products and the fma),   delta the subtraction's (0 for t >= 1/2)
so  |W' - W| <= sup |dW/dt| dt + n_ops u W',  the supremum over the interval t' can lie in.  With w_hi = min(1, w + dt),
t_hi = t + dt:
    C2  W = w^3             dW/dt = -3 w^2                                       |dW/dt| <= 3 w_hi^2
    C4  W = w^5 (5 t + 1)   dW/dt = -5 w^4 (5 t + 1) + 5 w^5 = -30 t w^4         |dW/dt| <= 30 t_hi w_hi^4
(the bound at w_hi also covers t > 1, where W = 0 and W' may be as large as Phi(1 - dt)).  n_ops, each rounding counted with
the power it enters W:
    C2  delta 3 (0 for t >= 1/2); u2 = w w: 1; u2 w: 1                                                            -> 5 (2)
    C4  delta 5 (0 for t >= 1/2); u2 enters squared: 2; u2 u2: 1; (u2 u2) w: 1; fma(5, t, 1): 1; the last product: 1
                                                                                                                  -> 11 (6)
The pair product, as oracle/kmvp_lowd_grad_model.py counts it: wb = W b (none for density) and the kept df_d once per
factor, NR = 2, density 1 (the fma's own rounding belongs to the chain); a denormal intermediate product is off by eta and
reaches the sum times the factors that follow: eta (1 + |df_d|) (1 + |b_e|) per pair.
    |term' - term| <= [dW (1 + r_NR) + W r_NR] |b_e| |df_d| + that,   r_NR = (1 + u)^NR - 1.
The select on s <= r2, r2 = (real)(R R), zeroes W and the differences together: a pair with |s - R^2| <= (gamma_s + 2 u) s may
be classified either way and is charged its whole term (there W = O(u^3)).  Pad records, pairs beyond the support and NaN
distances add exactly 0.
The constant c is formed in double and applied once per row in float64: its roundings and the product's are inside the
2^-50 mass of the chain term.  Accumulation and folds: wendland_model.product's formulas on the chain of a row's pairs that
may be inside -- float32: `chunk` walked records at most between two folds, the folds' own float64 additions charged as
folds * 2^-53 * mass; float64: one chain.  mass[i, e, d] = |c| sum_j W |b_je| |x_d - y_d|.
band = K_BAND (|c| pair + acc), K_BAND = 2 over the second-order terms the bounds drop.
"""
from collections import namedtuple

import numpy as np

import cutoff_grad_reference as gr
import kmvp_lowd_model as lm
import wendland_model as wm
import wendland_reference as wr
from kmvp_lowd_model import K_BAND, RSQ64, TRANS, chain_length, unit

Model = namedtuple("Model", "value band mass")
N_OPS = {"wendland-c2": (3, 2), "wendland-c4": (5, 6)}      # (the subtraction's power, every other rounding)
MARGIN = wm.MARGIN


def weight_bound(kernel, precision, s, R, D):
    """(W, each, edge): the float64 weight of every pair from its float64 squared distance s, the bound on |W' - W| before the
    select, and whether the select may go either way."""
    f32 = np.dtype(precision) == np.float32
    u = unit(precision)
    with np.errstate(invalid="ignore", over="ignore"):
        fin = np.isfinite(s)
        ss = np.where(fin, s, 4.0 * R * R)                  # (non-finite distances: far outside, W = W' = 0)
        t = np.sqrt(ss) / R
        W = gr.weights(kernel, ss, R)
        gs = wm.gamma_s(precision, ss, D)
        rho_t = (gs + 2 * u) / 2 + (TRANS if f32 else RSQ64 + u)
        dt = t * rho_t
        w_hi = np.clip(1.0 - t + dt, 0.0, 1.0)
        t_hi = t + dt
        slope = 3.0 * w_hi ** 2 if kernel == "wendland-c2" else 30.0 * t_hi * w_hi ** 4
        dphi = slope * dt
        sub, rest = N_OPS[kernel]
        n_ops = np.where(t < 0.5, sub + rest, rest)
        each = dphi + n_ops * u * (W + dphi)
        edge = fin & (np.abs(ss - R * R) <= (gs + 2 * u) * ss)
        each = np.where(fin, each, 0.0)
    return np.where(fin, W, 0.0), each, edge, np.where(fin, dphi, 0.0)


def restate(kernel, y, x, R, precision):
    """cutoff_grad_interact's per-pair sequence up to the accumulation, operation by operation in numpy's `precision`:
    (W' (N, M), df' (N, M, D)) as the kernel forms them, the select included.  An fma is the float64 (extended) result rounded
    once more (double rounding: below 2^-29 u)."""
    real = np.dtype(precision).type
    y = np.asarray(y, dtype=real)
    xa = y if x is None else np.asarray(x, dtype=real)

    def fma(a, b, c):
        return (a.astype(np.longdouble) * b.astype(np.longdouble) + c.astype(np.longdouble)).astype(real)

    with np.errstate(invalid="ignore", over="ignore"):
        df = xa[:, None, :] - y[None, :, :]
        s = df[:, :, 0] * df[:, :, 0]
        for d in range(1, y.shape[1]):
            s = fma(df[:, :, d], df[:, :, d], s)
        r2, iR2 = real(R * R), real(1.0 / (R * R))
        t = np.sqrt(s * iR2)
        u = np.maximum(real(1) - t, real(0))
        u2 = u * u
        if kernel == "wendland-c2":
            W = u2 * u
        else:
            W = ((u2 * u2) * u) * fma(np.full_like(t, 5), t, np.ones_like(t))
        inside = s <= r2
        return np.where(inside, W, real(0)), np.where(inside[:, :, None], df, real(0))


Pairs = namedtuple("Pairs", "i j Ww W each dfw df N M D")


def pairs(kernel, y, x, R, precision):
    """The pairs that can contribute, as index lists: (i, j), the weight Ww and the differences dfw in the widest float type,
    their float64 roundings W, df and the bound `each` on |W' - W| (a pair the select may classify either way: its whole
    weight).  Computed once per (cloud, kernel, R, precision) and shared."""
    precision = np.dtype(precision)
    y = np.asarray(y, dtype=precision).astype(np.float64)
    xa = y if x is None else np.asarray(x, dtype=precision).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        i, j = np.nonzero(wr.sqdists(xa, y) <= R * R * (1.0 + MARGIN))          # (NaN and infinite distances: never)
        wide = precision == np.float64 and lm.HAVE_LONGDOUBLE
        Wt = np.longdouble if wide else np.float64
        dfw = xa[i].astype(Wt) - y[j].astype(Wt)
        sw = (dfw * dfw).sum(axis=1)
        Ww = gr.weights(kernel, sw, R)
    W, each, edge, dphi = weight_bound(kernel, precision, sw.astype(np.float64), R, y.shape[1])
    each = np.where(edge, np.maximum(each, W + dphi), each)
    return Pairs(i, j, Ww, W, each, dfw, dfw.astype(np.float64), xa.shape[0], y.shape[0], y.shape[1])


def _rows(i, v, N):
    """Row sums of the per-pair values v (P, E, D) in v's own dtype."""
    out = np.zeros((N,) + v.shape[1:], dtype=v.dtype)
    np.add.at(out, i, v)
    return out


def gradient(kernel, y, x, b, R, *, precision=np.float32, chunk=512, folds=0, prs=None, rounding=True):
    """Modelled result of kmvp_wendland_<c>_cutoff_grad and its per-element band.  y (M, D) sources, x (N, D) targets (None:
    the same points), b (M, E) signal (None: density estimation), all rounded to `precision` first; chunk: the "chunk"
    option; folds: an upper bound on a row's folds into float64 (float32 only); prs: pairs() of the same arguments, to share;
    rounding=False: the float64 value alone.  Model(value, band, mass), (N, E, D) each."""
    precision = np.dtype(precision)
    f32 = precision == np.float32
    p = pairs(kernel, y, x, R, precision) if prs is None else prs
    density = b is None
    b = np.ones((p.M, 1)) if density else np.asarray(b, dtype=precision).astype(np.float64)
    c = gr.constant(kernel, R)
    wide = not f32 and lm.HAVE_LONGDOUBLE
    bj = b[p.j]
    Wt = p.Ww.dtype.type
    value = (Wt(c) * _rows(p.i, (p.Ww[:, None] * bj.astype(Wt))[:, :, None] * p.dfw[:, None, :], p.N)).astype(np.float64)
    babs, adf = np.abs(bj)[:, :, None], np.abs(p.df)[:, None, :]
    mass = abs(c) * _rows(p.i, p.W[:, None, None] * babs * adf, p.N)
    if not rounding:
        return Model(value, np.zeros_like(mass), mass)
    u = unit(precision)
    eta = 2.0 ** -150 if f32 else lm.ETA64
    r_nr = np.expm1((1 if density else 2) * np.log1p(u))
    pair = _rows(p.i, (p.each * (1 + r_nr) + p.W * r_nr)[:, None, None] * babs * adf + eta * (1.0 + babs) * (1.0 + adf), p.N)
    # the longest chain of a row in the working precision: its pairs that may be inside, cut by the folds in float32
    live = _rows(p.i, (p.each > 0).astype(np.float64)[:, None, None], p.N)
    n_chain = np.maximum(1.0, np.minimum(live, chain_length("lowd", precision, p.M, chunk, feed=0)) if f32 else live)
    acc_rel = np.minimum(n_chain, lm.LAM * np.sqrt(n_chain)) * u + 2.0 ** -50 + (folds * 2.0 ** -53 if f32 else 0.0)
    own = 1.0 if wide or f32 else 2.0
    band = own * K_BAND * (abs(c) * pair + acc_rel * mass + live * eta)
    return Model(value, band, mass)
