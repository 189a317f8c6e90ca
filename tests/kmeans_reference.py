"""float64 numpy restatement of Lloyd's k-means as include/kmvp.h kmvp_kmeans states it, iteration by iteration:

    k = 1, 2, ...:  l_k(i)    = the nearest of c_{k-1} to x_i -- knn_reference.nearest with K = 1 against the centroids ROUNDED
                                to the working precision; ties go to the smaller centroid index
                    c_k[c]    = sum_{l_k(i) = c} w_i x_i / sum_{l_k(i) = c} w_i ; a cluster of total weight 0 keeps its position
                    inertia_k = sum_i w_i s_i, s_i the squared distance to c_{k-1}
                    shift_k   = sum_c |c_k[c] - c_{k-1}[c]|^2
    a point without a qualifying centroid (label -1) or a non-finite inertia / shift ends the solve (not converged);
    the first k with shift_k <= tol converges; k == maxit stops (not converged).  The outputs are those of iteration k.

The points are taken as given (the caller rounds them to the precision under test).  Over the whole run the restatement also
reports the smallest relative gap (s2 - s1) / s2 between a point's two nearest centroids: where that is far above the
rounding of a working-precision distance, an implementation in that precision must take the very same labels."""
import numpy as np

import knn_reference as kn

RUNNING, CONVERGED, NONFINITE, MAXIT = 0, 1, 2, 3


def working(precision):
    """float16 data is computed on in float32 (the points rounded to float16, the centroids to float32)."""
    return np.float64 if np.dtype(precision) == np.float64 else np.float32


def step(x, w, c, precision):
    """One iteration from the centroids c: (labels, new centroids, cluster weights, inertia, shift, unlabelled, min gap)."""
    C = c.shape[0]
    real = working(precision)
    with np.errstate(over="ignore"):
        cr = c.astype(real).astype(np.float64)
    idx, sq = kn.nearest(x, cr, min(2, C), precision=real)
    labels, s = idx[:, 0], sq[:, 0]
    ok = labels >= 0
    gap = np.inf
    if C >= 2:
        s2 = sq[:, 1]
        two = ok & np.isfinite(s2) & (s2 > 0)
        if two.any():
            gap = float(np.min((s2[two] - s[two]) / s2[two]))
    W = np.bincount(labels[ok], weights=w[ok], minlength=C)
    new = c.copy()
    live = W > 0
    for d in range(x.shape[1]):
        sums = np.bincount(labels[ok], weights=w[ok] * x[ok, d], minlength=C)
        new[live, d] = sums[live] / W[live]
    inertia = float(np.sum(w[ok] * s[ok]))
    shift = float(np.sum((new - c) ** 2))
    return labels, new, W, inertia, shift, int(np.sum(~ok)), gap


def verdict(unlabelled, inertia, shift, iters, tol, maxit):
    if unlabelled or not (np.isfinite(inertia) and np.isfinite(shift)):
        return NONFINITE
    if shift <= tol:
        return CONVERGED
    if iters >= maxit:
        return MAXIT
    return RUNNING


def kmeans(x, c0, weights=None, tol=0.0, maxit=300, precision=np.float64):
    """Returns a dict: centroids, labels, cluster_weight, iterations, inertia, shift, converged, stop, min_gap, and the
    per-iteration histories inertias / shifts."""
    x = np.asarray(x, dtype=np.float64)
    c = np.array(c0, dtype=np.float64, ndmin=2)
    w = np.ones(x.shape[0]) if weights is None else np.asarray(weights, dtype=np.float64)
    k, stop, min_gap = 0, RUNNING, np.inf
    inertias, shifts = [], []
    while stop == RUNNING:
        labels, c, W, inertia, shift, unlabelled, gap = step(x, w, c, precision)
        k += 1
        min_gap = min(min_gap, gap)
        inertias.append(inertia)
        shifts.append(shift)
        stop = verdict(unlabelled, inertia, shift, k, tol, maxit)
    return dict(centroids=c, labels=labels, cluster_weight=W, iterations=k, inertia=inertia, shift=shift,
                converged=stop == CONVERGED, stop=stop, min_gap=min_gap, inertias=inertias, shifts=shifts)
