"""Dense float64 restatement of the pivoted-Cholesky preconditioner (csrc/kmvp_precond.hip) and of preconditioned conjugate
gradients (csrc/kmvp_solvers.hip pcg_solve), and the table of systems the GPU tests run -- TEST INFRASTRUCTURE ONLY, never
imported by the package.

    pivoted_cholesky   d = 1 exactly; step m: the argmax of d (ties to the smaller index) or the pivot it is GIVEN, so that a
                       comparison with the device follows the device's own pivots; no step once d_max <= tau;
                       L[m] = (K[:, p] - L[:m]' L[:m, p]) / sqrt(d_max);  d = max(d - L[m]^2, 0), d[p] = 0 exactly.
                       Returns L (rank_built, N) -- row t = column t of the factor, as the library hands it back --, the
                       pivots, and the residual diagonal BEFORE every step (rank_built, N).
    apply              z = D^-1 r - D^-1 L' (I + L D^-1 L')^-1 L D^-1 r, the Woodbury form of (L' L + D)^-1 r.
    pcg                x = 0, r = a, z = P^-1 r, p = z, rho = r . z;  alpha = rho / pAp (0 when pAp == 0 or rho <= 0);
                       x += alpha p;  r -= alpha Ap;  rs = r . r;  stops after the first iteration with
                       sqrt(rs / |a|^2) <= rtol in every column with |a| > 0 -- krylov_reference.cg's test, on the
                       UNPRECONDITIONED residual --;  z = P^-1 r;  beta = rho' / rho (0 when rho <= 0);  p = z + beta p.
                       The same Trace and the same ``noise`` hook as krylov_reference.cg.
"""
import functools
from collections import namedtuple

import numpy as np

import kmvp_oracle
import krylov_reference as kr
import matern_reference
from krylov_reference import Trace, _guarded, _operator, _worst

EPS = {"float64": 2.0 ** -53, "float32": 2.0 ** -24}      # unit roundoff of the working precision
TAU = {p: 256.0 * e for p, e in EPS.items()}               # PC_TAU_* of csrc/kmvp_precond.hip
MAX_RANK = 128


def pivoted_cholesky(K, rank, tau, pivots=None, noise=0.0, seed=0):
    """``noise`` multiplies every kernel column by 1 + noise * randn (how far a column error of that size moves L)."""
    K = np.asarray(K, dtype=np.float64)
    n = K.shape[0]
    rs = np.random.RandomState(seed)
    d = np.ones(n)
    L, piv, before = np.zeros((rank, n)), [], []
    for m in range(rank):
        p = int(np.argmax(d)) if pivots is None else int(pivots[m])  # numpy's argmax: the first of equal maxima
        if pivots is None and not d[p] > tau:
            break
        before.append(d.copy())
        col = K[:, p] * (1.0 + noise * rs.standard_normal(n)) if noise else K[:, p]
        L[m] = (col - L[:m].T @ L[:m, p]) / np.sqrt(d[p])
        d = np.maximum(d - L[m] * L[m], 0.0)
        d[p] = 0.0
        piv.append(p)
    built = len(piv)
    return L[:built], np.array(piv, dtype=np.int64), np.array(before).reshape(built, n)


def gram(L, D):
    """C = I + L D^-1 L' (L as (R, N))."""
    return np.eye(L.shape[0]) + (L / D) @ L.T


def apply(L, D, r):
    r = np.asarray(r, dtype=np.float64)
    D = np.asarray(D, dtype=np.float64).reshape((-1,) + (1,) * (r.ndim - 1))
    w = np.linalg.solve(gram(L, D.reshape(-1)), L @ (r / D))
    return (r - L.T @ w) / D


def pcg(A, L, D, a, rtol, maxit, history=False, noise=0.0, seed=0):
    op = _operator(A, noise, seed)
    a = np.array(a, dtype=np.float64, ndmin=2)
    x, r = np.zeros_like(a), a.copy()
    a2 = np.sum(a * a, axis=0)
    nonzero = a2 > 0
    z = apply(L, D, r)
    p = z.copy()
    rho = np.sum(r * z, axis=0)
    rel = np.where(nonzero, 1.0, 0.0)
    rels, xs, it = [], [x.copy()], 0
    while it < maxit and _worst(rel, nonzero) > rtol:
        Ap = op(p)
        pAp = np.sum(p * Ap, axis=0)
        alpha = _guarded(rho, pAp, (pAp != 0.0) & (rho > 0.0))
        x = x + alpha * p
        r = r + (-alpha) * Ap
        rs = np.sum(r * r, axis=0)
        it += 1
        with np.errstate(invalid="ignore"):
            rel = np.where(nonzero, np.sqrt(rs / np.where(nonzero, a2, 1.0)), 0.0)
        rels.append(rel)
        if history:
            xs.append(x.copy())
        if np.all(rel[nonzero] <= rtol):
            break
        z = apply(L, D, r)
        rho_new = np.sum(r * z, axis=0)
        beta = _guarded(rho_new, rho, rho > 0.0)
        rho = rho_new
        p = z + beta * p
    return Trace(x, it, np.array(rels).reshape(it, a.shape[1]), np.array(xs) if history else None, None)


# ----------------------------------------------------------------------------------------------------------------
# the systems: a uniform cube, one value of the diagonal per point in [0.01, 0.02], rank 32

N = 384  # one and a half workgroups of 256
RANK = 32
UNREACHABLE = kr.UNREACHABLE
TOL, NOISE = kr.TOL, kr.NOISE  # a product's error in the working precision; ten times that: the level g is measured at
G_MAX = 8.0
F64, F32 = "float64", "float32"
MAXITS = (1, 2, 3, 8, 9)  # the apply alone, inside the first burst of 8, its end, one past it

System = namedtuple("System", "kernel dim side rtols g g_factor")
# These matrices are ill conditioned on purpose (cond 4e3 .. 2e4: the diagonal is 0.01 .. 0.02), and the trajectory of
# conjugate gradients on such a matrix is reproducible only in its first iterations: test_precond_reference.py shows a
# product error of 1e-10 to come back 2 .. 4 times in the iterates 1 .. 9 and 1e3 .. 1e6 times in the iterates 18 .. 30,
# before the solve converges to the same solution.  Hence
# rtols: the tolerances the system is run to in float64 -- those at which the iteration COUNT survives that product error
#   (every looser one of a 1-2-5 grid does, none tighter than the last does), and which the stopping test clears on both
#   sides: the last residual that does not meet it is >= 1.05 rtol, the first that does <= 0.95 rtol.  At a tolerance the
#   GPU tests compare the count and the true residual, not the iterate.
# g: how many times a relative product error comes back in the iterate after MAXITS iterations in float64; the largest
#   value test_precond_reference.py measures over E = 1, 3 and eight seeds, rounded up to the next half.  GPU tolerance
#   4 g TOL.  There is no float32 entry: a float32 product errs by eps |K| |p|, and on these matrices K p is up to cond(A)
#   times smaller than |K| |p| -- an error RELATIVE TO THE OUTPUT, which is what ``noise`` models and TOL bounds on the
#   parity suite's clouds, does not describe it.  In float32 the GPU tests compare the factor, which is built from kernel
#   values alone, and the end of a solve.
# g_factor: how many times a relative error of the kernel columns comes back in a column of L, relative to that column's
#   norm, with the pivots held fixed; measured the same way, rounded up to the next ten.  GPU tolerance for L: 4 g_factor TOL.
SYSTEMS = {
    "G": System("gaussian", 3, 1.5, (5e-3, 1e-4), 3.0, 190.0),
    "M52": System("matern-5/2", 3, 1.5, (2e-2, 1e-4), 3.5, 160.0),
    "M32": System("matern-3/2", 3, 1.5, (1e-2, 5e-3), 4.5, 70.0),
    "E": System("absolute-exponential", 3, 1.5, (5e-2, 1e-2), 3.5, 20.0),
    "G12": System("gaussian", 12, 0.5, (1e-3,), 4.0, 40.0),  # D > 8: the column kernel's runtime loop
}
CUBE = ("G", "M52", "M32", "E")  # the four kernels on the cube of side 1.5
FLOAT32 = ("G", "E", "G12")
RATIO_RTOL = 1e-8  # where the iteration counts with and without the preconditioner are compared

_rs = np.random.RandomState(23)
_CUBE = _rs.rand(N, 12)
DIAG = _rs.uniform(0.01, 0.02, N)
RHS = np.concatenate([_rs.randn(N, 2) * np.array([1.0, 1e3]), np.zeros((N, 1))], axis=1)  # E = 3, last column 0
del _rs


def points(name, precision="float64"):
    """The cloud as the working precision holds it."""
    s = SYSTEMS[name]
    return np.ascontiguousarray(s.side * _CUBE[:, :s.dim], dtype=precision)


def rhs(E, precision="float64"):
    """E = 3: two scaled columns and the zero column; E = 1: the first column alone."""
    return np.ascontiguousarray(RHS[:, :E], dtype=precision)


@functools.lru_cache(maxsize=None)
def kernel_matrix(name, precision="float64"):
    """K in float64 on the points as ``precision`` holds them."""
    s, y = SYSTEMS[name], points(name, precision).astype(np.float64)
    module = matern_reference if s.kernel in matern_reference.KERNELS else kmvp_oracle
    K = np.asarray(module.kernel_matrix(kernel=s.kernel, source_points=y), dtype=np.float64)
    K.setflags(write=False)
    return K


@functools.lru_cache(maxsize=None)
def matrix(name, precision="float64"):
    """A = K + diag(DIAG) and cond(A)."""
    A = kernel_matrix(name, precision) + np.diag(DIAG)
    lam = np.linalg.eigvalsh(A)
    A.setflags(write=False)
    return A, float(lam.max() / lam.min())


@functools.lru_cache(maxsize=None)
def factor(name, precision="float64", rank=RANK):
    """The restatement's own factor (its own argmax): (L, pivots, residual diagonals)."""
    out = pivoted_cholesky(kernel_matrix(name, precision), rank, TAU[precision])
    for arr in out:
        arr.setflags(write=False)
    return out


def trace(name, E, rtol, maxit, precision="float64", L=None):
    """pcg on one case with every iterate, preconditioned by ``L`` (default: the restatement's own factor)."""
    A, _ = matrix(name, precision)
    return pcg(A, factor(name, precision)[0] if L is None else L, DIAG, rhs(E, precision), rtol, maxit, history=True)


def tolerance(name):
    """4 g TOL (float64): g was measured with random noise and a kernel's error need not be random."""
    return 4.0 * SYSTEMS[name].g * TOL[F64]


def factor_tolerance(name, precision="float64"):
    return 4.0 * SYSTEMS[name].g_factor * TOL[precision]


def factor_error(L, ref):
    """max over the columns t of |L[t] - ref[t]| / |ref[t]|."""
    return float(np.max(np.linalg.norm(np.asarray(L) - ref, axis=1) / np.linalg.norm(ref, axis=1)))
