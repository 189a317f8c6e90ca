"""Dense float64 restatement of the two Krylov drivers of csrc/kmvp_solvers.hip, iteration by iteration, and the table of
well-conditioned systems on which a step-by-step comparison with the GPU means something -- TEST INFRASTRUCTURE ONLY,
never imported by the package.

The restatement follows the RULES of the device code, not a library routine: the guards on the step lengths, the
columns of one right-hand side iterating together, the stop in the first iteration in which every non-zero column meets
the tolerance, MINRES' per-column ``done`` flags.  ``A`` is the dense matrix with the solver's diagonal already added;
the reductions are numpy's, so the scalars differ from the device's by rounding only (1e-16), far below what the tests
ask.  ``noise`` multiplies every operator output by ``1 + noise * randn``: test_krylov_reference.py measures with it how
far a product error of that size moves the iterate (the amplification ``g`` recorded in SYSTEMS below).

    cg      x = 0, r = p = a;  alpha = rs_old / pAp (0 when pAp == 0 or rs_old <= 0);  x += alpha p;  r -= alpha Ap;
            beta = rs_new / rs_old (0 when rs_old <= 0);  p = r + beta p.  Stops after the first iteration with
            sqrt(rs_new / |a|^2) <= rtol in every column with |a| > 0; columns that met it earlier go on iterating.
            No residual replacement: the systems below never enter the restart.
    minres  Paige & Saunders as minres_scalars_kernel writes it, from cs = -1, sn = 0, phibar = beta = beta1.  A column
            is flagged done by phibar <= rtol beta1, by beta == 0 or by a zero right-hand side, and from the NEXT
            iteration on takes 1 / gamma := 0, phi := 0 (and v := 0 at once): its x stays, its scalars run on.  Stops
            after the first iteration with phibar / beta1 <= rtol in every non-zero column.

Both return a Trace: the iterate, the number of iterations that ran, rel[k - 1, e] = the recurrence's relative residual
of column e after iteration k as the device state holds it, and with ``history=True`` every iterate (xs[k] after
iteration k, xs[0] = 0).  For MINRES done_at[e] is the iteration in which column e was flagged (0: from the start, -1:
never); rel is the residual of x only up to there.
"""
import functools
from collections import namedtuple

import numpy as np

import kmvp_oracle
import matern_reference

Trace = namedtuple("Trace", "x iters rel xs done_at")


def _operator(A, noise, seed):
    A = np.asarray(A, dtype=np.float64)
    if not noise:
        return lambda v: A @ v
    rs = np.random.RandomState(seed)
    return lambda v: (A @ v) * (1.0 + noise * rs.standard_normal(v.shape))


def _worst(rel, nonzero):
    """The host's `rel`: the largest relative residual over the non-zero columns, NaN if any is (0 without columns)."""
    w = 0.0
    for v in rel[nonzero]:
        if not np.isnan(w) and not v <= w:
            w = v
    return w


def _guarded(num, den, ok):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(ok, num / np.where(ok, den, 1.0), 0.0)


def cg(A, a, rtol, maxit, history=False, noise=0.0, seed=0):
    apply = _operator(A, noise, seed)
    a = np.array(a, dtype=np.float64, ndmin=2)
    x, r, p = np.zeros_like(a), a.copy(), a.copy()
    a2 = np.sum(a * a, axis=0)
    nonzero = a2 > 0
    rs_old = a2.copy()
    rel = np.where(nonzero, 1.0, 0.0)
    rels, xs, it = [], [x.copy()], 0
    while it < maxit and _worst(rel, nonzero) > rtol:
        Ap = apply(p)
        pAp = np.sum(p * Ap, axis=0)
        alpha = _guarded(rs_old, pAp, (pAp != 0.0) & (rs_old > 0.0))
        x = x + alpha * p
        r = r + (-alpha) * Ap
        rs_new = np.sum(r * r, axis=0)
        beta = _guarded(rs_new, rs_old, rs_old > 0.0)
        rs_old = rs_new
        it += 1
        with np.errstate(invalid="ignore"):
            rel = np.where(nonzero, np.sqrt(rs_new / np.where(nonzero, a2, 1.0)), 0.0)
        rels.append(rel)
        if history:
            xs.append(x.copy())
        if np.all(rel[nonzero] <= rtol):  # the device's stop word: NaN is "not met"
            break
        p = r + beta * p
    return Trace(x, it, np.array(rels).reshape(it, a.shape[1]), np.array(xs) if history else None, None)


def minres(A, a, rtol, maxit, history=False, noise=0.0, seed=0):
    apply = _operator(A, noise, seed)
    a = np.array(a, dtype=np.float64, ndmin=2)
    E = a.shape[1]
    x, w, w2 = np.zeros_like(a), np.zeros_like(a), np.zeros_like(a)
    y, r1, r2 = a.copy(), a.copy(), a.copy()
    beta1 = np.sqrt(np.sum(y * y, axis=0))
    nonzero = beta1 > 0
    beta, oldb = beta1.copy(), np.zeros(E)
    dbar, epsln = np.zeros(E), np.zeros(E)
    cs, sn = -np.ones(E), np.zeros(E)
    phibar = beta1.copy()
    done = ~nonzero
    done_at = np.where(done, 0, -1)
    t0 = _guarded(1.0, beta1, nonzero)  # v = y / beta
    t1 = np.zeros(E)                    # y = A v - (beta / oldb) r1: no r1 term in iteration 1
    rel = _guarded(phibar, beta1, nonzero)
    v = t0 * y
    rels, xs, it = [], [x.copy()], 0
    while it < maxit and _worst(rel, nonzero) > rtol:
        y = apply(v) + t1 * r1
        alfa = np.sum(v * y, axis=0)
        y = y + _guarded(-alfa, beta, beta > 0.0) * r2
        r1, r2 = r2, y
        dot = np.sum(r2 * r2, axis=0)
        # the Givens step, each product rounded on its own as the device does
        oldb, oldeps = beta, epsln
        beta = np.sqrt(np.maximum(dot, 0.0))
        delta = cs * dbar + sn * alfa
        gbar = sn * dbar - cs * alfa
        epsln = sn * beta
        dbar = -cs * beta
        gamma = np.maximum(np.sqrt(gbar * gbar + beta * beta), 1e-300)
        cs, sn = gbar / gamma, beta / gamma
        phi = cs * phibar
        phibar = sn * phibar
        dn = np.where(done, 0.0, 1.0 / gamma)
        step = np.where(done, 0.0, phi)
        with np.errstate(invalid="ignore"):
            done1 = done | (phibar <= rtol * beta1) | (beta == 0.0)
        it += 1
        done_at = np.where(done1 & ~done, it, done_at)
        done = done1
        w1, w2 = w2, w
        w = dn * v
        w = w + (-oldeps * dn) * w1
        w = w + (-delta * dn) * w2
        x = x + step * w
        t0 = _guarded(1.0, beta, ~done & (beta > 0.0))
        t1 = _guarded(-beta, oldb, oldb > 0.0)
        v = t0 * y
        rel = _guarded(phibar, beta1, nonzero)
        rels.append(rel)
        if history:
            xs.append(x.copy())
        if np.all(rel[nonzero] <= rtol):
            break
    return Trace(x, it, np.array(rels).reshape(it, E), np.array(xs) if history else None, done_at)


# ----------------------------------------------------------------------------------------------------------------
# the systems

N, D = 257, 3  # no multiple of 64 or 256
UNREACHABLE = 1e-30
BURST = 8  # CG_CHECK of kmvp_solvers.hip: iterations between two looks of the host
TOL = {"float64": 1e-11, "float32": 1e-5}      # a product's error in the working precision (the parity suite's)
NOISE = {"float64": 1e-10, "float32": 1e-4}    # ten times that: the level g is measured at
G_MAX = 8.0

_rs = np.random.RandomState(7)
Y = _rs.rand(N, D)
RHS = np.concatenate([_rs.randn(N, 3) * np.array([1.0, 1e-6, 1e3]), np.zeros((N, 1))], axis=1)  # E = 4, last column 0
D_ED = _rs.uniform(40.0, 60.0, N)
D_ID = 600.0 * (1.0 + 0.3 * _rs.rand(N)) * np.where(np.arange(N) % 2 == 0, 1.0, -1.0)
del _rs

System = namedtuple("System", "solver kernel scale d ridge rtols g")
# rtols: the two tolerances the system is run to in float64.  The second is 1e-8 where the solve then ends its burst
# of 8 (E30 after 16 iterations, Gr after 8) or leaves x_k at least 100 GPU tolerances from the iterate at the end of
# the burst (Ir-).  On the other six that distance is 18 to 95 tolerances at 1e-8 -- a driver returning the end of the
# burst could pass -- so they run to 1e-7 instead, where it is 200 to 1800.
# g: how many times a relative product error comes back in the iterate, keyed by (working precision, rtol) with
# UNREACHABLE for the runs to a fixed iteration count: the largest value test_krylov_reference.py measures over the
# E and maxit the GPU tests use, rounded up to the next half.  The GPU tolerance is 4 g TOL.
# "E0" is the bare exp(-r) matrix of Y, run for three iterations only, "I0" the bare inverse-distance matrix, for
# up to four: both are ill conditioned (cond 1e4), only their first steps are comparable.
F64, F32 = "float64", "float32"
SYSTEMS = {
    "G30": System("cg", "gaussian", 30.0, None, 0.0, (1e-4, 1e-7),
                  {(F64, 1e-4): 2.5, (F64, 1e-7): 2.5, (F64, UNREACHABLE): 2.5, (F32, 1e-4): 2.5}),
    "E30": System("cg", "absolute-exponential", 30.0, None, 0.0, (1e-4, 1e-8), {(F64, 1e-4): 1.5, (F64, 1e-8): 1.5}),
    "M32": System("cg", "matern-3/2", 30.0, None, 0.0, (1e-4, 1e-7), {(F64, 1e-4): 2.5, (F64, 1e-7): 2.5}),
    "M52": System("cg", "matern-5/2", 30.0, None, 0.0, (1e-4, 1e-7), {(F64, 1e-4): 3.0, (F64, 1e-7): 3.0}),
    "Gr": System("cg", "gaussian", 1.0, None, 50.0, (1e-4, 1e-8), {(F64, 1e-4): 1.5, (F64, 1e-8): 1.5}),
    "Ed": System("cg", "absolute-exponential", 1.0, D_ED, 0.0, (1e-4, 1e-7),
                 {(F64, 1e-4): 1.5, (F64, 1e-7): 2.5, (F64, UNREACHABLE): 2.5, (F32, 1e-4): 1.5}),
    "Id+-": System("minres", "inverse-distance", 1.0, D_ID, 0.0, (1e-4, 1e-7),
                   {(F64, 1e-4): 1.5, (F64, 1e-7): 1.5, (F64, UNREACHABLE): 5.5, (F32, 1e-4): 1.5}),
    "Ir-": System("minres", "inverse-distance", 1.0, None, -1000.0, (1e-4, 1e-8), {(F64, 1e-4): 1.5, (F64, 1e-8): 1.5}),
    "Ir+": System("minres", "inverse-distance", 1.0, None, 200.0, (1e-4, 1e-7), {(F64, 1e-4): 1.5, (F64, 1e-7): 1.5}),
    "I0": System("minres", "inverse-distance", 1.0, None, 0.0, (), {(F64, UNREACHABLE): 4.5}),
    "E0": System("cg", "absolute-exponential", 1.0, None, 0.0, (), {(F64, UNREACHABLE): 4.0}),
}
STOPPING = tuple(s for s in SYSTEMS if s not in ("I0", "E0"))   # run to a tolerance
MAXIT_CASES = {"G30": (1, 7, 8, 9, 17), "Ed": (1, 7, 8, 9, 17), "Id+-": (1, 7, 8, 9, 17), "I0": (1, 2, 3, 4), "E0": (3,)}
FLOAT32 = ("G30", "Ed", "Id+-")
SOLVERS = {"cg": cg, "minres": minres}


def points(name, precision="float64"):
    """The cloud as the working precision holds it."""
    return np.ascontiguousarray(SYSTEMS[name].scale * Y, dtype=precision)


def rhs(E, precision="float64"):
    """E = 4: the three scaled columns and the zero column; E = 1: the first column alone."""
    return np.ascontiguousarray(RHS[:, :E], dtype=precision)


def diagonal(name):
    """ridge + d_i per point in float64 (the solver keeps it in float64 whatever the working precision)."""
    s = SYSTEMS[name]
    return np.full(N, s.ridge) + (0.0 if s.d is None else s.d)


@functools.lru_cache(maxsize=None)
def matrix(name, precision="float64"):
    """A = K + diag in float64 on the points as ``precision`` holds them, and cond(A) = max|lambda| / min|lambda|."""
    s, y = SYSTEMS[name], points(name, precision).astype(np.float64)
    module = matern_reference if s.kernel in matern_reference.KERNELS else kmvp_oracle
    A = np.asarray(module.kernel_matrix(kernel=s.kernel, source_points=y), dtype=np.float64) + np.diag(diagonal(name))
    lam = np.abs(np.linalg.eigvalsh(A))
    A.setflags(write=False)
    return A, float(lam.max() / lam.min())


@functools.lru_cache(maxsize=None)
def trace(name, E, rtol, maxit, precision="float64"):
    """The restatement's run of one case with every iterate; computed once and shared, never modified."""
    A, _ = matrix(name, precision)
    t = SOLVERS[SYSTEMS[name].solver](A, rhs(E, precision), rtol, maxit, history=True)
    for arr in (t.x, t.rel, t.xs):
        arr.setflags(write=False)
    return t


def column_error(x, ref):
    """max over the non-zero columns of ref of ||x[:, e] - ref[:, e]|| / ||ref[:, e]||: the columns differ by nine
    orders of magnitude, a norm over whole rows would hide two of them."""
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    scale = np.linalg.norm(ref, axis=0)
    keep = scale > 0
    if not keep.any():
        return 0.0
    return float(np.max(np.linalg.norm(x - ref, axis=0)[keep] / scale[keep]))


def true_residual(A, x, a):
    """|a - A x| / |a| in float64 for each non-zero column of a."""
    a = np.asarray(a, dtype=np.float64)
    norm = np.linalg.norm(a, axis=0)
    keep = norm > 0
    return np.linalg.norm(a - A @ x, axis=0)[keep] / norm[keep]


def tolerance(name, rtol, precision="float64"):
    """4 g TOL: g was measured with random noise and a kernel's error need not be random."""
    return 4.0 * SYSTEMS[name].g[(precision, rtol)] * TOL[precision]
