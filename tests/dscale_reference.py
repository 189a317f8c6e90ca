"""Numpy restatement of the derivative of the kernel product in the logarithm of a per-axis length scale -- TEST
INFRASTRUCTURE ONLY, never imported by the package.

No reference method stands behind it (include/kmvp.h kmvp_<kernel>_dscale), so this is the definition written down,
and ``test_dscale_reference.py`` checks it against central differences of the pinned oracle's ``product`` under a
per-axis scaling of both clouds:

    H[i, e, d] = sum_j h_d(x_i, y_j) b[j, e],   h_d = -w(s_ij) (x_{i,d} - y_{j,d})^2,   s = |x_i - y_j|^2, r = sqrt(s)
    gaussian              w = -2 k                            (k from ``kmvp_oracle.kernel_block``)
    absolute-exponential  w = -k / r, and exactly 0 where s == 0 (the limit of h_d is 0 there)
    matern-3/2, -5/2      w from ``matern_reference.gradient_weights``

h_d is formed as (w D_d) D_d: where s overflows ``precision`` although D = x - y is finite, w is exactly 0 and the pair
contributes exactly 0 (0 * D_d^2 would be 0 * inf).  ``isotropic`` is the closed form of sum_d h_d = -s w, for the
check that the axes add up to the derivative in one length scale.  The arithmetic runs in ``precision``, the result is
float64 (n, E, D); ``rows`` restricts the targets.
"""
import numpy as np

import kmvp_oracle
import matern_reference

KERNELS = ("gaussian", "absolute-exponential", "matern-3/2", "matern-5/2")


def weights(kernel, s, rows, M):
    """w(s) = k'(r) / r in the dtype of s."""
    if kernel in matern_reference.KERNELS:
        return matern_reference.gradient_weights(kernel, s)
    k = kmvp_oracle.kernel_block(kernel, s, rows, M)
    if kernel == "gaussian":
        return -2 * k
    if kernel == "absolute-exponential":
        return np.where(s > 0, -k / np.sqrt(np.maximum(s, 0)), 0).astype(s.dtype)
    raise NotImplementedError(f"no length-scale derivative for kernel {kernel}")


def scale_derivative(*, kernel, source_points, target_points=None, source_signal=None, precision=np.float64, rows=None,
                     block_rows=None):
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
            w = weights(kernel, np.sum(diffs ** 2, axis=-1), rr, M)
            h = -(w[:, :, None] * diffs) * diffs                          # (n, M, D)
            out[r0 : r0 + block_rows] = np.einsum("nmd,me->ned", h, b)
    return np.ascontiguousarray(out, dtype=np.float64)


def isotropic(*, kernel, source_points, target_points=None, source_signal=None):
    """sum_j -s w(s) b[j, e] in float64 from the closed forms: 2 s k, r k, 3 r^2 e^-t, (5/3) r^2 (1 + t) e^-t: (N, E)."""
    y = np.asarray(source_points, dtype=np.float64)
    x = y if target_points is None else np.asarray(target_points, dtype=np.float64)
    b = np.ones((y.shape[0], 1)) if source_signal is None else np.asarray(source_signal, dtype=np.float64)
    s = np.sum((x[:, None, :] - y[None, :, :]) ** 2, axis=-1)
    r = np.sqrt(s)
    if kernel == "gaussian":
        m = 2.0 * s * np.exp(-s)
    elif kernel == "absolute-exponential":
        m = r * np.exp(-r)
    elif kernel == "matern-3/2":
        m = 3.0 * s * np.exp(-np.sqrt(3.0) * r)
    elif kernel == "matern-5/2":
        m = (5.0 / 3.0) * s * (1.0 + np.sqrt(5.0) * r) * np.exp(-np.sqrt(5.0) * r)
    else:
        raise NotImplementedError(kernel)
    return m @ b
