"""Numpy restatement of the gradient of the log-sum-exp reduction with respect to the target points -- TEST
INFRASTRUCTURE ONLY, never imported by the package.

No reference method stands behind it (include/kmvp.h kmvp_<kernel>_logsumexp_grad), so this is the definition written
down, and ``test_lse_grad_reference.py`` checks it against central differences of ``lse_reference.logsumexp``:

    G[i, e, :] = sum_j p_ij^e g(x_i, y_j),   p_ij^e = exp(l_ij + c[j, e]) / sum_j' exp(l_ij' + c[j', e])
    gaussian              l = -|x - y|^2   g = -2 (x - y)
    absolute-exponential  l = -|x - y|     g = -(x - y) / r, and exactly 0 where s = |x - y|^2 is not a positive normal
                                           number of ``precision`` (the symmetric subgradient of a coincident pair: it
                                           keeps its weight in the denominator)

stabilised by the row's largest logit.  ``c = -inf`` is a source of weight 0; a (row, column) without a live term is NaN
in all D components (exactly where ``lse_reference.logsumexp`` is -inf); a NaN target coordinate gives a NaN row.
The arithmetic runs in ``precision``, the result is float64 (n, E, D); ``rows=`` restricts it to some targets.
"""
import numpy as np

import lse_reference

KERNELS = lse_reference.KERNELS
CONSTANT = {"gaussian": -2.0, "absolute-exponential": -1.0}


def gradient(*, kernel, source_points, target_points=None, source_signal=None, precision=np.float64, rows=None,
             block_rows=None):
    if kernel not in KERNELS:
        raise NotImplementedError(f"no log-sum-exp gradient for kernel {kernel}")
    precision = np.dtype(precision)
    y = np.ascontiguousarray(source_points, dtype=precision)
    x = y if target_points is None else np.ascontiguousarray(target_points, dtype=precision)
    M, D = y.shape
    c = np.zeros((M, 1), dtype=precision) if source_signal is None else np.ascontiguousarray(source_signal, dtype=precision)
    if c.ndim == 1:
        c = c.reshape(-1, 1)
    E = c.shape[1]
    rows = np.arange(x.shape[0], dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    n = rows.shape[0]
    out = np.full((n, E, D), np.nan, dtype=np.float64)
    if M == 0 or n == 0:
        return out
    if block_rows is None:
        block_rows = max(1, min(n, int(2 ** 23 // max(1, M * max(D, E)))))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for r0 in range(0, n, block_rows):
            rr = rows[r0 : r0 + block_rows]
            diffs = x[rr].reshape(-1, 1, D) - y.reshape(1, M, D)                # (n, M, D), in `precision`
            s = np.sum(diffs ** 2, axis=-1)
            if kernel == "gaussian":
                ell, g = -s, diffs
            else:
                r = np.sqrt(s)
                ell = -r
                coincident = ~(s >= np.finfo(precision).tiny)                   # 0, denormal (and NaN: the row is NaN anyway)
                g = np.where(coincident[:, :, None], 0, diffs / np.where(coincident, 1, r)[:, :, None]).astype(precision)
            t = ell[:, :, None] + c[None, :, :]                                 # (n, M, E)
            top = np.max(np.where(np.isnan(t), -np.inf, t), axis=1)             # the largest logit of the row / column
            live = np.isfinite(top) | (top == np.inf)
            shift = np.where(np.isfinite(top), top, 0).astype(precision)
            w = np.exp(t - shift[:, None, :])                                   # weight 0 for c = -inf and s = inf
            z = np.sum(w, axis=1, dtype=precision)                              # (n, E)
            v = np.einsum("nme,nmd->ned", w, g).astype(precision)               # (n, E, D)
            val = (precision.type(CONSTANT[kernel]) * v / z[:, :, None]).astype(np.float64)
            out[r0 : r0 + block_rows] = np.where(live[:, :, None], val, np.nan)
    return out
