"""Dense float64 restatement of cg_lanczos (csrc/kmvp_solvers.hip) and of the Gauss quadrature on its coefficients
(csrc/kmvp_quadrature.hpp) -- TEST INFRASTRUCTURE ONLY, never imported by the package.  Systems, matrices and points
are krylov_reference's.

    cg_lanczos  x = 0, r = p = z, every column on its own clock.  Iteration k, for each column e that is not frozen:
                alpha = rs_old / pAp (0 when pAp == 0 or not rs_old > 0);  a column with pAp == 0 or rs_old <= 0 FREEZES
                here with steps[e] = k - 1 ("breakdown");  otherwise x += alpha p, r -= alpha Ap,
                beta = rs_new / rs_old (0 when not rs_old > 0), the row k - 1 of the coefficient history is written,
                steps[e] = k, and the column freezes on sqrt(rs_new / |z_e|^2) <= rtol ("tolerance"), else
                p = r + beta p.  A frozen column takes no further update (a select, not a product with 0); a zero
                column is frozen from the start with steps 0; NaN never freezes a column.  The loop ends after the first
                iteration that leaves every column frozen, or at maxit.  No residual replacement.
    quadrature  the Jacobi matrix of alpha[0..m), beta[0..m):  d_1 = 1 / alpha_1, d_k = 1 / alpha_k + beta_{k-1} / alpha_{k-1},
                e_k = sqrt(beta_k) / alpha_k (k < m);  theta, tau = its eigenvalues and the first components of its
                eigenvectors (numpy.linalg.eigh here, implicit QL in the library);  sum tau^2 f(theta).  m = 0 gives 0, a
                theta <= 0 or a non-finite coefficient NaN.

    logquad[e] = |z_e|^2 sum tau^2 log(theta) ~ z_e' log(A) z_e,   invquad[e] = z_e' x_e ~ z_e' A^-1 z_e,
    S[e] = |z_e|^2 sum tau^2 |log theta|: the scale quadrature errors are measured in (log theta changes sign).
"""
import functools
from collections import namedtuple

import numpy as np

import krylov_reference as kr

Run = namedtuple("Run", "x steps frozen alpha beta rel z2 logquad invquad scale iters")
TOLERANCE, BREAKDOWN, ZERO = 1, 2, 3   # why a column froze (0: it did not)
SYSTEMS = ("G30", "E30", "M32", "M52", "Gr", "Ed")   # the positive definite ones
RTOLS = (1e-4, 1e-7)
FLOAT32 = ("G30", "Ed")
MAXITS = (7, 8, 9)
MAXIT_SYSTEMS = ("G30", "Ed")
F64, F32, UNREACHABLE = kr.F64, kr.F32, kr.UNREACHABLE

# How many times a relative product error comes back in logquad (relative to S), in invquad (relative to itself) and in a
# coefficient alpha_k / beta_k (residual-weighted: see coefficient_error), keyed by (system, working precision, rtol) with UNREACHABLE for
# the runs to a fixed iteration count: the largest value test_lanczos_reference.py measures with noise = 10 TOL over the
# probe blocks the GPU tests use, rounded up to the next half.  (logquad alone: 2.6 on G30 with four columns and 3.7
# with 64, 1.3 on E30, 1.1 on the Matern systems, 0.05 on Gr and Ed, where invquad and the coefficients set the 0.5.)
# The GPU tolerance is 4 G TOL (krylov_reference.tolerance's rule).
G = {
    ("G30", F64, 1e-4): 3.0, ("G30", F64, 1e-7): 4.0, ("G30", F64, UNREACHABLE): 3.0, ("G30", F32, 1e-4): 3.0,
    ("E30", F64, 1e-4): 1.5, ("E30", F64, 1e-7): 1.5,
    ("M32", F64, 1e-4): 1.5, ("M32", F64, 1e-7): 1.5,
    ("M52", F64, 1e-4): 1.5, ("M52", F64, 1e-7): 1.5,
    ("Gr", F64, 1e-4): 0.5, ("Gr", F64, 1e-7): 0.5,
    ("Ed", F64, 1e-4): 0.5, ("Ed", F64, 1e-7): 0.5, ("Ed", F64, UNREACHABLE): 0.5, ("Ed", F32, 1e-4): 0.5,
}
# The same for the iterate x (krylov_reference.column_error), kept apart so that the scalar outputs are not held to the
# iterate's larger figure.
GX = {
    ("G30", F64, 1e-4): 2.0, ("G30", F64, 1e-7): 2.5, ("G30", F64, UNREACHABLE): 1.5, ("G30", F32, 1e-4): 2.0,
    ("E30", F64, 1e-4): 1.5, ("E30", F64, 1e-7): 1.5,
    ("M32", F64, 1e-4): 2.0, ("M32", F64, 1e-7): 2.0,
    ("M52", F64, 1e-4): 2.0, ("M52", F64, 1e-7): 2.0,
    ("Gr", F64, 1e-4): 1.5, ("Gr", F64, 1e-7): 1.5,
    ("Ed", F64, 1e-4): 1.5, ("Ed", F64, 1e-7): 2.0, ("Ed", F64, UNREACHABLE): 2.0, ("Ed", F32, 1e-4): 1.5,
}
G_MAX = 8.0


def probes(n, count, seed=0):
    """Rademacher columns exactly as MI355XSolver.log_determinant draws them."""
    return np.where(np.random.RandomState(seed).rand(n, count) < 0.5, -1.0, 1.0)


def block(P, precision="float64"):
    """The probe blocks of the tests.  P = 4: three Rademacher columns and a zero column; otherwise P Rademacher columns."""
    z = np.concatenate([probes(kr.N, 3), np.zeros((kr.N, 1))], axis=1) if P == 4 else probes(kr.N, P)
    return np.ascontiguousarray(z, dtype=precision)


def jacobi(alpha, beta):
    """The dense Jacobi matrix of one column's coefficients alpha[0..m), beta[0..m)."""
    alpha, beta = np.asarray(alpha, dtype=np.float64), np.asarray(beta, dtype=np.float64)
    m = len(alpha)
    T = np.zeros((m, m))
    for k in range(m):
        T[k, k] = 1.0 / alpha[k] + (beta[k - 1] / alpha[k - 1] if k else 0.0)
        if k + 1 < m:
            T[k, k + 1] = T[k + 1, k] = np.sqrt(beta[k]) / alpha[k]
    return T


def nodes(alpha, beta):
    """(theta, tau^2) of one column, or None where the library returns NaN."""
    alpha, beta = np.asarray(alpha, dtype=np.float64), np.asarray(beta, dtype=np.float64)
    with np.errstate(all="ignore"):
        T = jacobi(alpha, beta)
    if not np.all(np.isfinite(T)):
        return None
    theta, V = np.linalg.eigh(T)
    return theta, V[0] ** 2


def quadrature(alpha, beta, f=np.log, positive=True):
    """sum tau^2 f(theta); 0 for m = 0; NaN for a non-finite coefficient or (positive) a theta <= 0."""
    if len(alpha) == 0:
        return 0.0
    n = nodes(alpha, beta)
    if n is None or (positive and not np.all(n[0] > 0)):
        return float("nan")
    return float(np.sum(n[1] * f(n[0])))


def cg_lanczos(A, z, rtol, maxit, noise=0.0, seed=0):
    apply = kr._operator(A, noise, seed)
    z = np.array(z, dtype=np.float64, ndmin=2)
    P = z.shape[1]
    x, r, p = np.zeros_like(z), z.copy(), z.copy()
    z2 = np.sum(z * z, axis=0)
    rs_old = z2.copy()
    frozen = np.where(z2 == 0.0, ZERO, 0)
    steps = np.zeros(P, dtype=np.int64)
    alphas, betas, rels = np.zeros((maxit, P)), np.zeros((maxit, P)), np.zeros((maxit, P))
    k = 0
    while k < maxit and not np.all(frozen):
        k += 1
        Ap = apply(p)
        pAp = np.sum(p * Ap, axis=0)
        with np.errstate(invalid="ignore"):
            alpha = kr._guarded(rs_old, pAp, (pAp != 0.0) & (rs_old > 0.0))
            frozen = np.where((frozen == 0) & ((pAp == 0.0) | (rs_old <= 0.0)), BREAKDOWN, frozen)
        live = frozen == 0
        x = np.where(live, x + alpha * p, x)
        r = np.where(live, r + (-alpha) * Ap, r)
        rs_new = np.sum(r * r, axis=0)
        with np.errstate(invalid="ignore"):
            beta = kr._guarded(rs_new, rs_old, rs_old > 0.0)
            rel = np.sqrt(rs_new / np.where(z2 == 0.0, 1.0, z2))
            met = rel <= rtol   # NaN: not met
        alphas[k - 1] = np.where(live, alpha, 0.0)
        betas[k - 1] = np.where(live, beta, 0.0)
        rels[k - 1] = np.where(live, rel, 0.0)
        rs_old = np.where(live, rs_new, rs_old)
        steps = np.where(live, k, steps)
        frozen = np.where(live & met, TOLERANCE, frozen)
        p = np.where(frozen == 0, r + beta * p, p)
    logq = np.array([quadrature(alphas[:m, e], betas[:m, e]) for e, m in enumerate(steps)])
    scale = np.array([quadrature(alphas[:m, e], betas[:m, e], lambda t: np.abs(np.log(t))) for e, m in enumerate(steps)])
    return Run(x, steps, frozen, alphas, betas, rels, z2, z2 * logq, np.sum(z * x, axis=0), z2 * scale, k)


@functools.lru_cache(maxsize=None)
def run(name, P, rtol, maxit=1000, precision="float64"):
    """The restatement's run of one case of the tests; computed once and shared, never modified."""
    A, _ = kr.matrix(name, precision)
    t = cg_lanczos(A, block(P, precision), rtol, maxit)
    for arr in t[:-1]:
        arr.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def exact(name, precision="float64"):
    """(eigenvalues, eigenvectors) of A: z' f(A) z = sum (V' z)^2 f(lambda), log det A = sum log lambda."""
    A, _ = kr.matrix(name, precision)
    lam, V = np.linalg.eigh(A)
    lam.setflags(write=False)
    V.setflags(write=False)
    return lam, V


def exact_form(name, z, f, precision="float64"):
    lam, V = exact(name, precision)
    return np.sum((V.T @ np.asarray(z, dtype=np.float64)) ** 2 * f(lam)[:, None], axis=0)


def coefficient_error(got_a, got_b, ref, e, weighted=False):
    """max over the rows k < steps[e] of column e of |c_k - ref_k| / |ref_k| for c = alpha and beta (0 without rows): the
    relative difference the GPU tests hold to 4 G TOL.
    weighted: each row times rel_k, the restatement's relative residual after iteration k + 1 -- the figure G is measured
    in.  A product error of relative size p enters r at the size of the iterate's terms, |z|, whatever the residual has
    shrunk to, so it shows in rs_k = |r_k|^2 -- and in the two coefficients formed from it -- as p / rel_k: with
    p = 10 TOL the last rows of a run to 1e-7 move by 1e4 .. 7e5 p unweighted and by at most 0.6 p weighted
    (test_lanczos_reference.py).  The unweighted bound therefore asks of the product an error of TOL rel_k, not TOL."""
    m = int(ref.steps[e])
    if m == 0:
        return 0.0
    w = ref.rel[:m, e] if weighted else 1.0
    da = np.abs(got_a[:m, e] - ref.alpha[:m, e]) / np.abs(ref.alpha[:m, e]) * w
    nz = ref.beta[:m, e] != 0.0
    db = (np.abs(got_b[:m, e] - ref.beta[:m, e]) * w / np.abs(np.where(nz, ref.beta[:m, e], 1.0)))[nz]
    return float(max(da.max(), db.max() if db.size else 0.0))


def tolerance(name, rtol, precision="float64", table=G):
    """4 G TOL: G was measured with random noise and a kernel's error need not be random.  table=GX: for the iterate."""
    return 4.0 * table[(name, precision, rtol)] * kr.TOL[precision]
