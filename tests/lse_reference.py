"""Numpy restatement of the log-sum-exp reduction of the Gaussian and exp(-r) kernels -- TEST INFRASTRUCTURE ONLY,
never imported by the package.

No reference method stands behind it (include/kmvp.h kmvp_<kernel>_logsumexp), so this is the definition written down,
and ``test_lse_reference.py`` checks it against ``numpy.logaddexp.reduce``:

    L[i, e] = log sum_j exp( l(x_i, y_j) + c[j, e] )
    gaussian              l = -|x - y|^2
    absolute-exponential  l = -|x - y|

stabilised by the row's largest logit (which is subtracted before exp and added back after log).  ``c = -inf`` is a
source of weight 0; a row / column without a live term is exactly ``-inf``; a NaN target coordinate gives a NaN row.
The arithmetic runs in ``precision``, the result is float64 (n, E); ``rows=`` restricts it to some targets.
"""
import numpy as np

KERNELS = ("gaussian", "absolute-exponential")


def logits(kernel, x, y):
    """l(x_i, y_j) in the arrays' own precision, squared distances in the difference form."""
    s = np.sum((x[:, None, :] - y[None, :, :]) ** 2, axis=-1)
    if kernel == "gaussian":
        return -s
    if kernel == "absolute-exponential":
        return -np.sqrt(s)
    raise NotImplementedError(f"no log-sum-exp for kernel {kernel}")


def logsumexp(*, kernel, source_points, target_points=None, source_signal=None, precision=np.float64, rows=None,
              block_rows=None):
    precision = np.dtype(precision)
    y = np.ascontiguousarray(source_points, dtype=precision)
    x = y if target_points is None else np.ascontiguousarray(target_points, dtype=precision)
    M = y.shape[0]
    c = np.zeros((M, 1), dtype=precision) if source_signal is None else np.ascontiguousarray(source_signal, dtype=precision)
    if c.ndim == 1:
        c = c.reshape(-1, 1)
    E = c.shape[1]
    rows = np.arange(x.shape[0], dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    n = rows.shape[0]
    out = np.full((n, E), -np.inf, dtype=np.float64)
    if M == 0 or n == 0:
        return out
    if block_rows is None:
        block_rows = max(1, min(n, int(2 ** 23 // max(1, M * max(y.shape[1], E)))))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for r0 in range(0, n, block_rows):
            rr = rows[r0 : r0 + block_rows]
            t = logits(kernel, x[rr], y)[:, :, None] + c[None, :, :]            # (n, M, E), in `precision`
            top = np.max(np.where(np.isnan(t), -np.inf, t), axis=1)             # the largest logit of the row / column
            live = np.isfinite(top)
            shift = np.where(live, top, 0).astype(precision)
            total = np.sum(np.exp(t - shift[:, None, :]), axis=1, dtype=precision)
            val = np.log(total).astype(np.float64) + shift.astype(np.float64)   # a NaN logit: NaN through the sum
            val = np.where(live | np.isnan(total), val, -np.inf)
            out[r0 : r0 + block_rows] = np.where(top == np.inf, np.inf, val)
    return out
