"""Dense float64 numpy restatement of kmvp_<kernel>_eigsh (include/kmvp.h): the three operators, the Lanczos process with
classical Gram-Schmidt twice, the look schedule, the breakdown rule and the sign rule, written without the code under
test.  test_eigsh_reference.py checks it against numpy.linalg.eigh; the GPU tests compare with both."""
import collections

import numpy as np

KERNELS = ("gaussian", "absolute-exponential", "matern-3/2", "matern-5/2")
OPERATORS = ("kernel", "centered", "normalized")
N, D, K, SIDE = 800, 3, 6, 4.0
MAXIT = 256
LOOK = 8
BREAKDOWN = 1e-13
TOLS = {"float64": 1e-10, "float32": 1e-4}


def cloud(n=N, seed=49, dtype=np.float64):
    """n uniform points in a cube of side SIDE, rounded to ``dtype`` (what the device holds), as float64.  The symmetry of
    a cube brings near-multiple eigenvalues; seed 49 is one of those (about one in five) whose cloud keeps the seven
    largest eigenvalues of all twelve operators apart by more than 1e-2 lambda_1 (test_eigsh_reference.py asserts it)."""
    y = np.random.RandomState(seed).uniform(0.0, SIDE, size=(n, D))
    return np.asarray(y.astype(dtype), dtype=np.float64)


def start_vector(n=N, seed=5):
    return np.random.RandomState(seed).standard_normal(n)


def cross_kernel(kernel, x, y):
    d2 = np.maximum(np.sum(x * x, axis=1)[:, None] + np.sum(y * y, axis=1)[None, :] - 2.0 * x @ y.T, 0.0)
    if kernel == "gaussian":
        return np.exp(-d2)
    r = np.sqrt(d2)
    if kernel == "absolute-exponential":
        return np.exp(-r)
    if kernel == "matern-3/2":
        t = np.sqrt(3.0) * r
        return (1.0 + t) * np.exp(-t)
    if kernel == "matern-5/2":
        t = np.sqrt(5.0) * r
        return (1.0 + t + t * t / 3.0) * np.exp(-t)
    raise ValueError(kernel)


def kernel_matrix(kernel, y):
    """Exact differences on the square problem (the diagonal is exactly 1)."""
    diff = y[:, None, :] - y[None, :, :]
    d2 = np.sum(diff * diff, axis=2)
    if kernel == "gaussian":
        return np.exp(-d2)
    r = np.sqrt(d2)
    if kernel == "absolute-exponential":
        return np.exp(-r)
    t = np.sqrt(3.0 if kernel == "matern-3/2" else 5.0) * r
    return (1.0 + t) * np.exp(-t) if kernel == "matern-3/2" else (1.0 + t + t * t / 3.0) * np.exp(-t)


def operator(Kmat, op, ridge=0.0, d=None):
    """The dense A of include/kmvp.h, symmetric by construction."""
    n = Kmat.shape[0]
    if op == "kernel":
        A = Kmat + ridge * np.eye(n)
        return A if d is None else A + np.diag(d)
    if op == "centered":
        H = np.eye(n) - np.full((n, n), 1.0 / n)
        A = H @ Kmat @ H
    elif op == "normalized":
        s = 1.0 / np.sqrt(Kmat.sum(axis=1))
        A = s[:, None] * Kmat * s[None, :]
    else:
        raise ValueError(op)
    return 0.5 * (A + A.T)


def fix_signs(X):
    """Each column's component of largest magnitude made positive (np.argmax: the smallest index on a tie)."""
    X = np.array(X, dtype=np.float64)
    for c in range(X.shape[1]):
        if X[np.argmax(np.abs(X[:, c])), c] < 0:
            X[:, c] = -X[:, c]
    return X


def looks_at(j, k, maxit):
    return (j >= k and j % LOOK == 0) or j == maxit


Result = collections.namedtuple("Result", "eigenvalues eigenvectors resid steps converged alpha beta breakdown V")


def eigsh(A, k, v0, tol, maxit, centered=False):
    """The process of include/kmvp.h on the dense symmetric A.  alpha, beta: (maxit,), rows >= steps zero."""
    n = A.shape[0]
    v = np.array(v0, dtype=np.float64)
    if centered:
        v = v - v.mean()
    V = np.zeros((maxit + 1, n))
    V[0] = v / np.linalg.norm(v)
    alpha, beta = np.zeros(maxit), np.zeros(maxit)
    j, breakdown, theta, S = 0, False, None, None
    while j < maxit:
        Vj = V[: j + 1]
        w = A @ V[j]
        h = Vj @ w
        w = w - Vj.T @ h
        h2 = Vj @ w
        w = w - Vj.T @ h2
        alpha[j] = h[j] + h2[j]
        beta[j] = np.linalg.norm(w)
        j += 1
        breakdown = beta[j - 1] <= BREAKDOWN * np.max(np.abs(alpha[:j]))
        if not breakdown:
            V[j] = w / beta[j - 1]
        if not (breakdown or looks_at(j, k, maxit)):
            continue
        if j < k:
            break  # breakdown before k steps
        T = np.diag(alpha[:j]) + np.diag(beta[: j - 1], 1) + np.diag(beta[: j - 1], -1)
        lam, Z = np.linalg.eigh(T)
        theta, S = lam[::-1][:k], Z[:, ::-1][:, :k]
        if breakdown or np.all(beta[j - 1] * np.abs(S[-1]) <= tol * abs(theta[0])):
            break
    if theta is None:
        nan = np.full(k, np.nan)
        return Result(nan, np.full((n, k), np.nan), nan, j, False, alpha, beta, breakdown, V[:j])
    X = V[:j].T @ S
    X = fix_signs(X / np.linalg.norm(X, axis=0))
    resid = np.linalg.norm(A @ X - X * theta, axis=0) / (abs(theta[0]) * np.linalg.norm(X, axis=0))
    ok = bool(np.all(np.isfinite(resid)) and np.all(resid <= 1.5 * tol))
    return Result(theta, X, resid, j, ok, alpha, beta, breakdown, V[:j])


def embedding(op, theta, X):
    """get_embedding() of the plugin: X sqrt(max(theta, 0)), or unit rows for the normalised operator."""
    if op != "normalized":
        return X * np.sqrt(np.maximum(theta, 0.0))
    norms = np.linalg.norm(X, axis=1, keepdims=True)
    return X / np.where(norms > 0, norms, 1.0)


def transform(kernel, op, y, theta, X, x_new):
    """Out-of-sample embedding, dense: K(x, Y) (centred as sklearn's KernelCenterer does for "centered") times X theta^-1/2."""
    Kxy = cross_kernel(kernel, x_new, y)
    if op == "centered":
        Kyy = kernel_matrix(kernel, y)
        Kxy = Kxy - Kxy.mean(axis=1, keepdims=True) - Kyy.mean(axis=0)[None, :] + Kyy.mean()
    return Kxy @ (X / np.sqrt(theta))


_cache = {}


def system(kernel, op, dtype="float64"):
    """(A, lam descending, y) of the N-point cloud as the device holds it in ``dtype``; computed once."""
    key = (kernel, op, dtype)
    if key not in _cache:
        y = cloud(dtype=np.dtype(dtype))
        kk = ("K", kernel, dtype)
        if kk not in _cache:
            _cache[kk] = kernel_matrix(kernel, y)
        A = operator(_cache[kk], op)
        _cache[key] = (A, np.linalg.eigvalsh(A)[::-1], y)
    return _cache[key]


def kmatrix(kernel, dtype="float64"):
    system(kernel, "kernel", dtype)
    return _cache[("K", kernel, dtype)]
