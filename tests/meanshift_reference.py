"""Float64 / numpy restatement of the Gaussian mean-shift of include/kmvp.h (kmvp_gaussian_meanshift), of the cluster rule
of MI355XMeanShift.get_clusters, and the test cloud both are tried on.

The iteration takes the gradient as a callable ``grad(targets) -> G``: targets (n, D) in the working precision, G (n, D)
float64, the rows of the log-sum-exp gradient at those targets.  On the CPU that is lse_grad_reference.gradient; the GPU
tests feed it the device's own kmvp_gaussian_logsumexp_grad, so that the restatement walks through the device's bits.

Every product and every sum below is a separate numpy operation on float64 arrays: one rounding each, no fused
multiply-add -- the arithmetic csrc/kmvp_meanshift_step.hpp spells with __dmul_rn / __dadd_rn."""
import numpy as np


def step(G, base, tol):
    """One sweep for the rows given: (z (n, D), q (n,), frozen (n,) bool, nonfinite (n,) bool).
    z = base + 0.5 G, q = sum_d (0.5 G_d)^2 with d ascending; a row with a non-finite component of G: z and q NaN."""
    G = np.asarray(G, dtype=np.float64)
    base = np.asarray(base, dtype=np.float64)
    n, D = G.shape
    q = np.zeros(n, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        h = 0.5 * G
        z = base + h
        for d in range(D):
            q = q + h[:, d] * h[:, d]
    nonfinite = ~np.all(np.isfinite(G), axis=1)
    z[nonfinite] = np.nan
    q[nonfinite] = np.nan
    with np.errstate(invalid="ignore"):
        frozen = (q <= tol * tol) | nonfinite
    return z, q, frozen, nonfinite


def meanshift(grad, seeds, tol, maxit, precision=np.float64, all_rows=False):
    """The iteration of kmvp_gaussian_meanshift.  ``grad`` sees the ACTIVE rows only (all_rows=False) or all N rows every
    sweep, frozen ones at their last position (all_rows=True: a host loop on a context that always holds all N targets);
    the rows of the active points are used either way.  Returns a dict: modes (N, D), iters (N,) int64, step2 (N,),
    sweeps, target_sweeps, converged."""
    precision = np.dtype(precision)
    z = np.array(seeds, dtype=precision).astype(np.float64)  # the seeds as the device holds them, widened exactly
    N, D = z.shape
    iters = np.zeros(N, dtype=np.int64)
    step2 = np.zeros(N, dtype=np.float64)
    active = np.arange(N)
    sweeps, target_sweeps = 0, 0
    while active.size and sweeps < maxit:
        sweeps += 1
        target_sweeps += int(active.size)
        with np.errstate(over="ignore"):
            rounded = z.astype(precision)  # real(z_{k-1})
        if all_rows:
            G = np.asarray(grad(rounded), dtype=np.float64).reshape(N, D)[active]
        else:
            G = np.asarray(grad(rounded[active]), dtype=np.float64).reshape(active.size, D)
        znew, q, frozen, _ = step(G, rounded[active].astype(np.float64), tol)
        z[active] = znew
        step2[active] = q
        iters[active[frozen]] = sweeps
        active = active[~frozen]
    iters[active] = sweeps  # still moving at the end: maxit
    with np.errstate(invalid="ignore"):
        converged = bool(active.size == 0 and np.all(step2 <= tol * tol))
    return {"modes": z, "iters": iters, "step2": step2, "sweeps": sweeps, "target_sweeps": target_sweeps,
            "converged": converged}


def clusters(modes, step2, tol, merge_radius):
    """The cluster rule: (centres (C, D), labels (N,) int64).  Walk the converged modes (finite, step2 <= tol^2) in
    ascending index; a mode founds a centre if no earlier centre lies within merge_radius (Euclidean, float64, <=).
    Afterwards every converged point gets the label of its nearest centre, ties to the smaller label; the others -1."""
    modes = np.asarray(modes, dtype=np.float64)
    N, D = modes.shape
    with np.errstate(invalid="ignore"):
        ok = np.all(np.isfinite(modes), axis=1) & (np.asarray(step2, dtype=np.float64) <= tol * tol)

    def distance(a, b):  # Euclidean, float64, the squares added with d ascending
        s = 0.0
        for d in range(D):
            s = s + (a[d] - b[d]) ** 2
        return np.sqrt(s)

    centres = []
    for i in range(N):  # the plain double loop: the definition, not the implementation
        if not ok[i]:
            continue
        if all(distance(modes[i], c) > merge_radius for c in centres):
            centres.append(modes[i].copy())
    labels = np.full(N, -1, dtype=np.int64)
    for i in range(N):
        if ok[i]:
            labels[i] = int(np.argmin([distance(modes[i], c) for c in centres]))  # argmin: the first smallest
    return np.array(centres, dtype=np.float64).reshape(len(centres), D), labels


def cloud(N, D, seed=0):
    """The test cloud, (N, D) float64: a quarter a tight blob (sd 0.25) at the origin, a quarter a wide blob (sd 0.7) at
    5 e_0, a quarter a ridge (sd 0.15) around a segment of length 6 along axis 0, offset 6 along the last axis (D = 1:
    offset 14 on the axis), the rest uniform on [-2, 8]^D; all shuffled."""
    rs = np.random.RandomState(seed)
    q = N // 4
    tight = 0.25 * rs.randn(q, D)
    wide = 0.7 * rs.randn(q, D)
    wide[:, 0] += 5.0
    ridge = 0.15 * rs.randn(q, D)
    ridge[:, 0] += 6.0 * rs.rand(q)
    ridge[:, D - 1] += 6.0 if D > 1 else 14.0
    rest = rs.uniform(-2.0, 8.0, size=(N - 3 * q, D))
    pts = np.concatenate([tight, wide, ridge, rest], axis=0)
    return np.ascontiguousarray(pts[rs.permutation(N)])
