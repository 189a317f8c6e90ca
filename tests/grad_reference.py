"""Numpy restatement of the gradient of the kernel product with respect to the target points -- TEST
INFRASTRUCTURE ONLY, never imported by the package.

No reference method stands behind the gradient (include/kmvp.h kmvp_<kernel>_grad), so this is the definition
written down, and ``test_grad_reference.py`` checks it against central differences of the pinned oracle's
``product``:

    G[i, e, :] = sum_j w(s_ij) (x_i - y_j) b[j, e],   s = |x_i - y_j|^2, r = sqrt(s), k the kernel value
    gaussian              w = -2 k
    absolute-exponential  w = -k / r, and exactly 0 where s == 0 (symmetric subgradient)
    inverse-distance      w = -1 / r^3 = -k^3 with k from ``kmvp_oracle.kernel_block``: the pairs its flat-index rule
                          zeroes contribute 0; a coincident pair that is not zeroed gives inf * 0 = NaN in every
                          component of the row

The arithmetic runs in ``precision``, the result is float64 (N, E, D); ``j_offset`` / ``M_total`` as in
``kmvp_oracle.kernel_block``.
"""
import numpy as np

import kmvp_oracle


def gradient(*, kernel, source_points, target_points=None, source_signal=None, precision=np.float64, rows=None,
             j_offset=0, M_total=None, block_rows=None):
    precision = np.dtype(precision)
    y = np.ascontiguousarray(source_points, dtype=precision)
    x = y if target_points is None else np.ascontiguousarray(target_points, dtype=precision)
    M, D = y.shape
    b = np.ones((M, 1), dtype=precision) if source_signal is None else np.ascontiguousarray(source_signal, dtype=precision)
    E = b.shape[1]
    rows = np.arange(x.shape[0], dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    n = rows.shape[0]
    if block_rows is None:
        block_rows = max(1, min(max(n, 1), int(2 ** 24 // max(1, M * max(D, E)))))
    out = np.empty((n, E, D), dtype=precision)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for r0 in range(0, n, block_rows):
            rr = rows[r0 : r0 + block_rows]
            diffs = x[rr].reshape(-1, 1, D) - y.reshape(1, M, D)
            s = np.sum(diffs ** 2, axis=-1)
            k = kmvp_oracle.kernel_block(kernel, s, rr, M, j_offset=j_offset, M_total=M_total)
            if kernel == "gaussian":
                w = -2 * k
            elif kernel == "absolute-exponential":
                w = np.where(s > 0, -k / np.sqrt(np.maximum(s, 0)), 0).astype(precision)
            elif kernel == "inverse-distance":
                w = -(k * k * k)
            else:
                raise NotImplementedError(f"no gradient for kernel {kernel}")
            wb = w[:, :, None] * b[None, :, :]                                   # (n, M, E)
            out[r0 : r0 + block_rows] = np.einsum("nme,nmd->ned", wb, diffs)    # inf * 0 -> NaN for every (e, d)
    return np.ascontiguousarray(out, dtype=np.float64)
