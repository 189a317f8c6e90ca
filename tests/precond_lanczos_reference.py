"""Dense float64 restatement of cg_lanczos_precond (csrc/kmvp_solvers.hip; include/kmvp.h
kmvp_<kernel>_lanczos_quadrature_precond) -- TEST INFRASTRUCTURE ONLY, never imported by the package.  Systems, matrices,
points and the factor are precond_reference's (N = 384, rank 32, diagonal 0.01 .. 0.02); the quadrature is
lanczos_reference's.

    form        z = D^1/2 g + L' h (L as (rank', N): row t = column t of the factor; rows t >= rank' of h are not read)
    logdet_p    sum log D_i + log det (I + L D^-1 L'), the latter by slogdet of precond_reference.gram
    run         x = 0, r = z, pz = P^-1 z, p = pz, rho_0 = z . pz, every column on its own clock.  Iteration k, for each
                column that is not frozen: alpha = rho / pAp (0 when pAp == 0 or not rho > 0); a column with pAp == 0 or
                rho <= 0 FREEZES here with steps = k - 1; otherwise x += alpha p, r -= alpha Ap, zr = P^-1 r,
                rho' = r . zr, beta = rho' / rho, row k - 1 of the history, steps = k, and the column freezes on
                sqrt(rho' / rho_0) <= rtol, else p = zr + beta p.  A column with rho_0 == 0 is frozen from the start; NaN
                never freezes a column.  No residual replacement.
    logquad[e] = rho_0 sum tau^2 log(theta) ~ w' log(M) w,  w = P^-1/2 z,  M = P^-1/2 A P^-1/2;   invquad[e] = pz_e . x_e;
    S[e] = rho_0 sum tau^2 |log theta|: the scale quadrature errors are measured in.
"""
import functools
from collections import namedtuple

import numpy as np

import krylov_reference as kr
import lanczos_reference as lz
import precond_reference as pr

Run = namedtuple("Run", "x pz steps frozen alpha beta rel rho0 logquad invquad scale logdet_p z iters")
TOLERANCE, BREAKDOWN, ZERO = lz.TOLERANCE, lz.BREAKDOWN, lz.ZERO
F64, F32, UNREACHABLE = pr.F64, pr.F32, pr.UNREACHABLE
N, RANK, DIAG = pr.N, pr.RANK, pr.DIAG
SYSTEMS = pr.CUBE            # G, M52, M32, E: the four kernels on the cube of side 1.5
FLOAT32 = ("G", "E")
MAXITS = (7, 8, 9)           # around the end of the first burst of 8
SEED = 0                     # of the 16-probe estimates, on the CPU and on the GPU
ESTIMATE_PROBES = 16

# (system, rtol) with a step-count assertion on the GPU: tolerances of a 1-2-5 grid at which the restatement's steps do not
# move under a relative product error of kr.NOISE over eight seeds on the probe blocks P = 1, 4, 5
# (test_precond_lanczos_reference.py; on M32 and E none tighter than the second does).  These matrices are ill conditioned
# on purpose (precond_reference.SYSTEMS), and the preconditioned recurrence is reproducible in its first ten iterations
# only: at the first tolerance of G and M52 (8 and 11 steps) and in the runs to MAXITS a product error comes back less than
# ten times; at the others (14 .. 22 steps) 60 .. 4e7 times, and there the GPU tests compare the count, not the values.
RTOLS = {"G": (1e-2, 1e-4), "M52": (1e-2, 2e-4), "M32": (2e-2, 5e-3), "E": (5e-2, 1e-2)}
COMPARED = (("G", 1e-2), ("M52", 1e-2))   # with the runs to MAXITS: where values are compared iteration by iteration
RATIO_RTOL = 1e-8   # where the step counts with and without the preconditioner are compared (precond_reference's)
# The quadrature's own error |logquad - w' log(M) w| / S, in units of rtol^2: the largest value
# test_precond_lanczos_reference.py measures over RTOLS and the probe blocks is 0.92 (G at 1e-4; 0.54 at its 1e-2, below
# 0.25 on the Matern systems, 0.02 on E).  The plain entry quotes 1.5 for its systems.
QUADRATURE_RTOL2 = 1.0

# How many times a relative product error comes back in logquad (relative to rho_0), in invquad (relative to itself) and
# in a coefficient alpha_k / beta_k (residual-weighted: lanczos_reference.coefficient_error), keyed by (system, rtol) with
# UNREACHABLE for the runs to MAXITS: the largest value test_precond_lanczos_reference.py measures with noise = kr.NOISE
# over eight seeds and the probe blocks P = 1, 4, 5, rounded up to the next half.  GPU tolerance 4 G TOL.
# logquad is measured against rho_0 and not against S as in lanczos_reference: M's spectrum surrounds 1, so S = rho_0 sum
# tau^2 |log theta| is as small as the preconditioner is good (0.02 rho_0 on G), while a product error moves theta, and
# with it log theta, by an absolute amount.  (Measured: logquad 1.9 on G, 1.5 on M52, below 1 on M32 and E; the
# coefficients set the figure everywhere.)
G = {
    ("G", 1e-2): 4.5, ("M52", 1e-2): 3.5,
    ("G", UNREACHABLE): 4.5, ("M52", UNREACHABLE): 3.5, ("M32", UNREACHABLE): 4.0, ("E", UNREACHABLE): 2.0,
}
# The same for the iterate x (krylov_reference.column_error).  pz and wnorm2 take no product: see ROUNDING.
GX = {
    ("G", 1e-2): 10.0, ("M52", 1e-2): 9.5,
    ("G", UNREACHABLE): 10.5, ("M52", UNREACHABLE): 9.0, ("M32", UNREACHABLE): 7.0, ("E", UNREACHABLE): 6.0,
}

# logdet_p, the probes z, pz = P^-1 z and rho_0 involve no kernel product: given L they are float64 arithmetic on both
# sides, in different orders.  The yardstick is how far this module's float64 formulas are from the same formulas in
# numpy.longdouble (test_precond_lanczos_reference.py measures it on the four systems and on the float32 contexts'
# factors): relative to |logdet_p|, to the column norm of pz and to rho_0 the largest values are 1.2e-16, 5.5e-14 and
# 3.9e-14 -- P^-1 amplifies a rounding error of z by up to cond(P) = 1e4.  MARGIN times the figures below is the GPU
# tolerance: the device adds in other orders (partial sums per workgroup, fma chains, a blocked substitution), each as good
# as numpy's, so its distance from the restatement is a small multiple of the restatement's distance from the exact value.
ROUNDING = {"logdet_p": 1.5e-16, "pz": 6e-14, "rho0": 4e-14}
MARGIN = 16.0


# The long run of the graph-replay test (the cloud and diagonal of test_gpu_precond.py::test_long_pcg_graph_replay, rank 16,
# two probe columns): its first burst of 8 iterations is compared with the restatement.  On this matrix (diagonal
# 1e-3 .. 2e-3) rho rises before it falls -- sqrt(rho_k / rho_0) is 4.7 .. 8.4 over those iterations -- and a product
# error comes back 17.2 times in the residual-weighted coefficients (test_precond_lanczos_reference.py).
REPLAY_N, REPLAY_RANK, REPLAY_G = 1200, 16, 17.5


def replay_system():
    """(points, diagonal, g, h) of the graph-replay test."""
    import kmvp_oracle
    y, _ = kmvp_oracle.uniform_cube(REPLAY_N, 3)
    d = np.random.RandomState(12).uniform(1e-3, 2e-3, REPLAY_N)
    signs = np.where(np.random.RandomState(13).rand(REPLAY_N + REPLAY_RANK, 2) < 0.5, -1.0, 1.0)
    return y * 4.0, d, np.ascontiguousarray(signs[:REPLAY_N]), np.ascontiguousarray(signs[REPLAY_N:])


def replay_matrix(y, d):
    import kmvp_oracle
    return np.asarray(kmvp_oracle.kernel_matrix(kernel="gaussian", source_points=y), dtype=np.float64) + np.diag(d)


PLUGIN_RIDGE = 0.015   # the scalar ridge of the plugin test on M52 (test_gpu_precond.py's)


def plugin_rhs():
    """E = 2, both columns O(1): precond_reference's first column and a Rademacher column."""
    return np.ascontiguousarray(np.concatenate([pr.rhs(1), lz.probes(N, 1, seed=5)], axis=1))


def probes(n, rank, count, seed=0):
    """Rademacher (g (n, count), h (rank, count)) exactly as MI355XSolver draws them for preconditioned=True."""
    signs = np.where(np.random.RandomState(seed).rand(n + rank, count) < 0.5, -1.0, 1.0)
    return np.ascontiguousarray(signs[:n]), np.ascontiguousarray(signs[n:])


def block(P):
    """The probe blocks of the tests.  P = 4: three Rademacher columns and a zero column (in g and in h); otherwise P."""
    if P != 4:
        return probes(N, RANK, P)
    g, h = probes(N, RANK, 3)
    return (np.ascontiguousarray(np.concatenate([g, np.zeros((N, 1))], axis=1)),
            np.ascontiguousarray(np.concatenate([h, np.zeros((RANK, 1))], axis=1)))


def form(L, D, g, h):
    L = np.asarray(L)
    return np.sqrt(np.asarray(D, dtype=L.dtype))[:, None] * g + L.T @ np.asarray(h, dtype=L.dtype)[:L.shape[0]]


def logdet_p(L, D):
    sign, logdet_c = np.linalg.slogdet(pr.gram(L, D))
    assert sign > 0
    return float(np.sum(np.log(D)) + logdet_c)


def run(A, L, D, g, h, rtol, maxit, noise=0.0, seed=0):
    op = kr._operator(A, noise, seed)
    z = form(L, D, np.array(g, dtype=np.float64, ndmin=2), np.array(h, dtype=np.float64, ndmin=2))
    P = z.shape[1]
    x, r = np.zeros_like(z), z.copy()
    pz = pr.apply(L, D, r)
    p = pz.copy()
    rho0 = np.sum(r * pz, axis=0)
    rho = rho0.copy()
    frozen = np.where(rho0 == 0.0, ZERO, 0)
    steps = np.zeros(P, dtype=np.int64)
    alphas, betas, rels = np.zeros((maxit, P)), np.zeros((maxit, P)), np.zeros((maxit, P))
    k = 0
    while k < maxit and not np.all(frozen):
        k += 1
        Ap = op(p)
        pAp = np.sum(p * Ap, axis=0)
        with np.errstate(invalid="ignore"):
            alpha = kr._guarded(rho, pAp, (pAp != 0.0) & (rho > 0.0))
            frozen = np.where((frozen == 0) & ((pAp == 0.0) | (rho <= 0.0)), BREAKDOWN, frozen)
        live = frozen == 0
        x = np.where(live, x + alpha * p, x)
        r = np.where(live, r + (-alpha) * Ap, r)
        zr = pr.apply(L, D, r)
        rho_new = np.sum(r * zr, axis=0)
        with np.errstate(invalid="ignore"):
            beta = kr._guarded(rho_new, rho, rho > 0.0)
            rel = np.sqrt(rho_new / np.where(rho0 == 0.0, 1.0, rho0))
            met = rel <= rtol   # NaN: not met
        alphas[k - 1] = np.where(live, alpha, 0.0)
        betas[k - 1] = np.where(live, beta, 0.0)
        rels[k - 1] = np.where(live, rel, 0.0)
        rho = np.where(live, rho_new, rho)
        steps = np.where(live, k, steps)
        frozen = np.where(live & met, TOLERANCE, frozen)
        p = np.where(frozen == 0, zr + beta * p, p)
    logq = np.array([lz.quadrature(alphas[:m, e], betas[:m, e]) for e, m in enumerate(steps)])
    scale = np.array([lz.quadrature(alphas[:m, e], betas[:m, e], lambda t: np.abs(np.log(t))) for e, m in enumerate(steps)])
    return Run(x, pz, steps, frozen, alphas, betas, rels, rho0, rho0 * logq, np.sum(pz * x, axis=0), rho0 * scale,
               logdet_p(L, D), z, k)


def case(name, P, rtol, maxit=1000, L=None, precision="float64", noise=0.0, seed=0):
    """One case of the tests on ``L`` (default: the restatement's own factor)."""
    A, _ = pr.matrix(name, precision)
    g, h = block(P)
    return run(A, pr.factor(name, precision)[0] if L is None else L, DIAG, g, h, rtol, maxit, noise, seed)


@functools.lru_cache(maxsize=None)
def own(name, P, rtol, maxit=1000):
    """case() on the restatement's own factor, computed once and shared, never modified."""
    t = case(name, P, rtol, maxit)
    for arr in t[:-3] + (t.z,):
        arr.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def preconditioned_spectrum(name):
    """(eigenvalues, eigenvectors, P^-1/2) of M = P^-1/2 A P^-1/2 with the restatement's own factor."""
    A, _ = pr.matrix(name)
    L = pr.factor(name)[0]
    lam_p, V_p = np.linalg.eigh(L.T @ L + np.diag(DIAG))
    root = (V_p / np.sqrt(lam_p)) @ V_p.T
    M = root @ A @ root
    lam, V = np.linalg.eigh(0.5 * (M + M.T))
    for arr in (lam, V, root):
        arr.setflags(write=False)
    return lam, V, root


def exact_logquad(name, z):
    """w' log(M) w per column of z, w = P^-1/2 z."""
    lam, V, root = preconditioned_spectrum(name)
    return np.sum((V.T @ (root @ np.asarray(z, dtype=np.float64))) ** 2 * np.log(lam)[:, None], axis=0)


@functools.lru_cache(maxsize=None)
def dense(name):
    """(log det A, tr A^-1) of the dense matrix."""
    A, _ = pr.matrix(name)
    lam = np.linalg.eigvalsh(A)
    return float(np.sum(np.log(lam))), float(np.sum(1.0 / lam))


def estimates(t):
    """(log det estimate, its standard error, tr A^-1 estimate, its standard error) of a run on Rademacher probes."""
    root = np.sqrt(len(t.logquad))
    return (t.logdet_p + float(np.mean(t.logquad)), float(np.std(t.logquad, ddof=1) / root),
            float(np.mean(t.invquad)), float(np.std(t.invquad, ddof=1) / root))


def tolerance(name, rtol, table=G):
    """4 G TOL (float64): G was measured with random noise and a kernel's error need not be random.  table=GX: the iterate."""
    return 4.0 * table[(name, rtol)] * kr.TOL[F64]


def rounding_tolerance(what):
    return MARGIN * ROUNDING[what]


# ---- the same formulas in numpy.longdouble, for ROUNDING

def _ld_cholesky(C):
    C = np.array(C, dtype=np.longdouble)
    n = C.shape[0]
    G = np.zeros_like(C)
    for j in range(n):
        G[j, j] = np.sqrt(C[j, j] - np.dot(G[j, :j], G[j, :j]))
        G[j + 1:, j] = (C[j + 1:, j] - G[j + 1:, :j] @ G[j, :j]) / G[j, j]
    return G


def longdouble_pieces(L, D, g, h):
    """(logdet_p, z, pz, rho_0) in numpy.longdouble from the float64 L, D, g, h."""
    L, D = np.asarray(L, dtype=np.longdouble), np.asarray(D, dtype=np.longdouble)
    z = form(L, D, np.asarray(g, dtype=np.longdouble), h)
    G = _ld_cholesky(np.eye(L.shape[0], dtype=np.longdouble) + (L / D) @ L.T)
    w = L @ (z / D[:, None])
    for i in range(len(w)):                      # G y = w
        w[i] = (w[i] - G[i, :i] @ w[:i]) / G[i, i]
    for i in range(len(w) - 1, -1, -1):          # G' v = y
        w[i] = (w[i] - G[i + 1:, i] @ w[i + 1:]) / G[i, i]
    pz = (z - L.T @ w) / D[:, None]
    return np.sum(np.log(D)) + 2 * np.sum(np.log(np.diag(G))), z, pz, np.sum(z * pz, axis=0)
