"""Numpy restatement of the Matern 3/2 and 5/2 kernels, their products and the gradient of the product with respect to
the target points -- TEST INFRASTRUCTURE ONLY, never imported by the package.

No reference method stands behind these kernels (include/kmvp.h kmvp_matern32 / kmvp_matern52), so this is the
definition written down at length scale 1, and ``test_matern_reference.py`` checks it against the general Matern form
with the modified Bessel function K_nu and against central differences of its own product:

    s = |x - y|^2, r = sqrt(s)
    matern-3/2   t = sqrt(3) r   k = (1 + t) e^-t             w = -3 e^-t
    matern-5/2   t = sqrt(5) r   k = (1 + t + t^2 / 3) e^-t   w = -(5/3) (1 + t) e^-t
    G[i, e, :] = sum_j w(s_ij) (x_i - y_j) b[j, e]

A pair at infinite distance (s = inf, also where a float32 s overflows) contributes exactly 0 to the product and to
the gradient.  The arithmetic runs in ``precision``, results are float64; ``rows`` restricts the targets.
"""
import numpy as np

KERNELS = ("matern-3/2", "matern-5/2")
SQRT_2NU = {"matern-3/2": 1.7320508075688772, "matern-5/2": 2.23606797749979}


def kernel_values(kernel, s):
    """k(s) in the dtype of s; exactly 0 at s = inf."""
    s = np.asarray(s)
    one, c = s.dtype.type(1), s.dtype.type(SQRT_2NU[kernel])
    with np.errstate(invalid="ignore", over="ignore"):
        t = c * np.sqrt(s)
        e = np.exp(-t)
        poly = one + t if kernel == "matern-3/2" else one + t + t * t / s.dtype.type(3)
        return np.where(np.isfinite(t), poly * e, 0).astype(s.dtype)


def gradient_weights(kernel, s):
    """w(s) in the dtype of s; exactly 0 at s = inf."""
    s = np.asarray(s)
    one, c = s.dtype.type(1), s.dtype.type(SQRT_2NU[kernel])
    with np.errstate(invalid="ignore", over="ignore"):
        t = c * np.sqrt(s)
        e = np.exp(-t)
        w = -s.dtype.type(3) * e if kernel == "matern-3/2" else -(s.dtype.type(5) / s.dtype.type(3)) * (one + t) * e
        return np.where(np.isfinite(t), w, 0).astype(s.dtype)


def _inputs(source_points, target_points, source_signal, precision, rows):
    precision = np.dtype(precision)
    y = np.ascontiguousarray(source_points, dtype=precision)
    x = y if target_points is None else np.ascontiguousarray(target_points, dtype=precision)
    b = np.ones((y.shape[0], 1), dtype=precision) if source_signal is None else np.ascontiguousarray(source_signal, dtype=precision)
    rows = np.arange(x.shape[0], dtype=np.int64) if rows is None else np.asarray(rows, dtype=np.int64)
    return precision, y, x, b, rows


def _blocks(n, M, width):
    step = max(1, min(max(n, 1), int(2 ** 24 // max(1, M * width))))
    return [(r0, min(n, r0 + step)) for r0 in range(0, n, step)]


def kernel_matrix(*, kernel, source_points, target_points=None, precision=np.float64, rows=None):
    """(len(rows), M) kernel values, difference form."""
    precision, y, x, _, rows = _inputs(source_points, target_points, None, precision, rows)
    with np.errstate(over="ignore", invalid="ignore"):
        diffs = x[rows].reshape(-1, 1, y.shape[1]) - y.reshape(1, -1, y.shape[1])
        return kernel_values(kernel, np.sum(diffs ** 2, axis=-1))


def product(*, kernel, source_points, target_points=None, source_signal=None, normalize_rows=False, precision=np.float64,
            rows=None):
    """a = K b, or (K b) / (K 1) row-normalised; ``source_signal=None`` is density estimation (b = 1): (n, E) float64."""
    precision, y, x, b, rows = _inputs(source_points, target_points, source_signal, precision, rows)
    n, (M, D) = rows.shape[0], y.shape
    out = np.empty((n, b.shape[1]), dtype=precision)
    for r0, r1 in _blocks(n, M, D):
        K = kernel_matrix(kernel=kernel, source_points=y, target_points=x, precision=precision, rows=rows[r0:r1])
        a = K @ b
        if normalize_rows:
            a = a / np.sum(K, axis=1, keepdims=True)
        out[r0:r1] = a
    return np.ascontiguousarray(out, dtype=np.float64)


def gradient(*, kernel, source_points, target_points=None, source_signal=None, precision=np.float64, rows=None):
    """(n, E, D) float64, the targets being independent variables (also with target_points=None)."""
    precision, y, x, b, rows = _inputs(source_points, target_points, source_signal, precision, rows)
    n, (M, D), E = rows.shape[0], y.shape, b.shape[1]
    out = np.empty((n, E, D), dtype=precision)
    with np.errstate(over="ignore", invalid="ignore"):
        for r0, r1 in _blocks(n, M, max(D, E)):
            diffs = x[rows[r0:r1]].reshape(-1, 1, D) - y.reshape(1, M, D)
            w = gradient_weights(kernel, np.sum(diffs ** 2, axis=-1))
            wb = w[:, :, None] * b[None, :, :]
            out[r0:r1] = np.einsum("nme,nmd->ned", wb, diffs)
    return np.ascontiguousarray(out, dtype=np.float64)
