"""Float64 dense reference of the cutoff-radius gradients (include/kmvp.h kmvp_<kernel>_cutoff_grad) -- TEST INFRASTRUCTURE
ONLY, never imported by the package.  The reference project has no such entry: this is the definition.

    G[i, e, :] = sum_{j : s_ij <= R R} w(s_ij) (x_i - y_j) b[j, e],      s = |x_i - y_j|^2, r = sqrt(s), t = r / R, u = max(1 - t, 0)
    gaussian               w = -2 exp(-s)
    absolute-exponential   w = -exp(-r) / r, and 0 at s = 0
    matern-3/2             w = -3 exp(-sqrt(3) r)
    matern-5/2             w = -(5/3) (1 + sqrt(5) r) exp(-sqrt(5) r)
    wendland-c2            w = -(20 / R^2) u^3                      (phi' = -20 t u^3)
    wendland-c4            w = -(56 / (3 R^2)) u^5 (5 t + 1)        (phi' = -(56/3) t u^5 (5 t + 1))

A source with a non-finite coordinate is in no sum, a target with an infinite coordinate has nothing inside (a row of 0), a
target with a NaN coordinate gets a NaN row."""
import numpy as np

TRUNCATED = ("gaussian", "absolute-exponential", "matern-3/2", "matern-5/2")
WENDLAND = ("wendland-c2", "wendland-c4")
KERNELS = TRUNCATED + WENDLAND


def constant(kernel, R):
    """c, the factor the entries apply once per row."""
    return {"gaussian": -2.0, "absolute-exponential": -1.0, "matern-3/2": -3.0, "matern-5/2": -5.0 / 3.0,
            "wendland-c2": -20.0 / (R * R), "wendland-c4": -56.0 / (3.0 * (R * R))}[kernel]


def weights(kernel, s, R):
    """W(s) >= 0 without its constant, in the dtype of s (float64 or wider), for finite s >= 0."""
    one = s.dtype.type(1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        r = np.sqrt(s)
        if kernel == "gaussian":
            return np.exp(-s)
        if kernel == "absolute-exponential":
            return np.where(s > 0, np.exp(-r) / np.where(s > 0, r, one), 0)
        if kernel == "matern-3/2":
            return np.exp(-np.sqrt(s.dtype.type(3)) * r)
        if kernel == "matern-5/2":
            t = np.sqrt(s.dtype.type(5)) * r
            return (one + t) * np.exp(-t)
        t = r / s.dtype.type(R)
        u = np.maximum(one - t, 0)
        if kernel == "wendland-c2":
            return u * u * u
        if kernel == "wendland-c4":
            return u * u * u * u * u * (5 * t + one)
    raise ValueError(kernel)


def dense(kernel, y, x, b, R):
    """(N, E, D) float64 by the dense masked evaluation over all N x M pairs; x = None: the targets are the sources, b = None:
    density estimation (E = 1)."""
    y = np.asarray(y, dtype=np.float64)
    xa = y if x is None else np.asarray(x, dtype=np.float64)
    bb = np.ones((len(y), 1)) if b is None else np.asarray(b, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        df = xa[:, None, :] - y[None, :, :]
        s = np.sum(df * df, axis=-1)
        inside = s <= R * R                       # NaN and infinite distances: outside
    w = np.where(inside, weights(kernel, np.where(inside, s, 0.0), R), 0.0)
    out = constant(kernel, R) * np.einsum("nm,me,nmd->ned", w, bb, np.where(inside[:, :, None], df, 0.0))
    out[np.isnan(xa).any(axis=1)] = np.nan
    return out
