"""GPU tests of kmvp_<kernel>_eigsh (include/kmvp.h) and the MI355XSpectral plugin: the returned pairs are eigenpairs of
the dense float64 operator built in numpy (residual, the residual bound on the eigenvalues index by index, orthonormal
vectors), the process is the one the header states (first coefficients and the history's own Ritz values against the
restatement, eigsh_reference.py), and the contract around it (diagonal, maxit, breakdown, bits, refusals, NaN, two ranks)."""
import json
import os

import numpy as np
import pytest

import eigsh_reference as er
import krylov_reference as kr
from kernel_matrix_benchmarks_amd import _lib
from kernel_matrix_benchmarks_amd.algorithms.mi355x import MI355XSpectral
from test_gpu_multirank import _spawn

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CODES = {"float64": _lib.KMVP_F64, "float32": _lib.KMVP_F32}
K, N, MAXIT = er.K, er.N, er.MAXIT


def device_points(precision, n=N, seed=49):
    return np.ascontiguousarray(er.cloud(n, seed, np.dtype(precision)), dtype=np.dtype(precision))


def open_context(precision="float64"):
    ctx = _lib.Context(0)
    try:
        ctx.set_points(device_points(precision), None, CODES[precision])
    except Exception:
        ctx.close()
        raise
    return ctx


def gpu_eigsh(kernel, op, precision="float64", tol=None, maxit=MAXIT, k=K, **kwargs):
    ctx = open_context(precision)
    try:
        return ctx.eigsh(kernel, k, op, er.start_vector(), er.TOLS[precision] if tol is None else tol, maxit, **kwargs)
    finally:
        ctx.close()


def obeys_sign_rule(X):
    return all(X[np.argmax(np.abs(X[:, c])), c] > 0 for c in range(X.shape[1]))


@pytest.mark.parametrize("precision", ("float64", "float32"))
@pytest.mark.parametrize("op", er.OPERATORS)
@pytest.mark.parametrize("kernel", er.KERNELS)
def test_eigenpairs_of_the_dense_operator(kernel, op, precision):
    """1. against the dense float64 A of the points as the device holds them."""
    tol = er.TOLS[precision]
    A, lam, _ = er.system(kernel, op, precision)
    r = gpu_eigsh(kernel, op, precision)
    theta, X = r["eigenvalues"], r["eigenvectors"]
    rho = np.linalg.norm(A @ X - X * theta, axis=0) / np.linalg.norm(X, axis=0)
    err = np.abs(theta - lam[:K])
    orth = float(np.max(np.abs(X.T @ X - np.eye(K))))
    print(f"[1] {kernel} {op} {precision}: steps {r['steps']}, rho / theta_1 {rho.max() / theta[0]:.3g} (bound {2 * tol:.3g}), "
          f"eigenvalue error / lambda_1 {err.max() / lam[0]:.3g}, X'X - I {orth:.3g}, resid {r['resid'].max():.3g}")
    assert r["converged"] and K <= r["steps"] < MAXIT and r["steps"] % er.LOOK == 0
    assert np.all(np.diff(theta) < 0)
    assert np.all(rho <= 2.0 * tol * theta[0])
    assert np.all(err <= rho * (1.0 + 1e-9) + 1e-14 * lam[0])
    assert orth <= 1e-10
    assert np.all(r["resid"] <= 1.5 * tol)
    assert obeys_sign_rule(X)
    if op == "normalized":
        assert abs(theta[0] - 1.0) <= 2.0 * tol
        q = er.kmatrix(kernel, precision).sum(axis=1)
        assert np.max(np.abs(r["degree"] - q)) <= kr.TOL[precision] * np.max(q)
    else:
        assert "degree" not in r
    if op == "centered":
        assert np.max(np.abs(X.sum(axis=0))) <= 1e-10 * np.sqrt(N)


@pytest.mark.parametrize("op", er.OPERATORS)
@pytest.mark.parametrize("kernel", er.KERNELS)
def test_the_process_is_the_one_stated(kernel, op):
    """2. float64: alpha_1 and beta_1 are the restatement's for the same v0, and the k largest eigenvalues of the tridiagonal of the returned history are the returned eigenvalues."""
    A, lam, _ = er.system(kernel, op)
    ref = er.eigsh(A, K, er.start_vector(), er.TOLS["float64"], MAXIT, centered=op == "centered")
    r = gpu_eigsh(kernel, op, want_coefficients=True)
    j = r["steps"]
    a, b = r["alpha"], r["beta"]
    print(f"[2] {kernel} {op}: steps {j} (restatement {ref.steps}), alpha_1 {a[0]!r} vs {ref.alpha[0]!r}, beta_1 {b[0]!r} vs {ref.beta[0]!r}")
    assert a.shape == b.shape == (MAXIT,)
    assert abs(a[0] - ref.alpha[0]) <= 1e-12 * lam[0] and abs(b[0] - ref.beta[0]) <= 1e-12 * lam[0]
    T =np.diag(a[:j]) + np.diag(b[: j - 1], 1) + np.diag(b[: j - 1], -1)
    assert np.max(np.abs(np.linalg.eigvalsh(T)[::-1][:K] - r["eigenvalues"])) <= 1e-12 * lam[0]


def test_solver_diagonal_in_kernel_mode():
    """3. ridge = 0.1 and a per-point d: the eigenvalues of K + 0.1 I + diag(d); refused with the other operators."""
    tol = er.TOLS["float64"]
    d = np.random.RandomState(21).uniform(0.0, 0.05, N)
    A = er.operator(er.kmatrix("matern-5/2"), "kernel", ridge=0.1, d=d)
    lam = np.linalg.eigvalsh(A)[::-1]
    ctx = open_context()
    try:
        ctx.set_solver_diagonal(d, 0.1)
        r = ctx.eigsh("matern-5/2", K, "kernel", er.start_vector(), tol, MAXIT)
        for op in ("centered", "normalized"):
            with pytest.raises(_lib.KmvpError) as e:
                ctx.eigsh("matern-5/2", K, op, er.start_vector(), tol, MAXIT)
            assert e.value.code == 1 and "diagonal" in str(e.value)
        ctx.set_solver_diagonal(None, 0.0)
        bare = ctx.eigsh("matern-5/2", K, "kernel", er.start_vector(), tol, MAXIT)
    finally:
        ctx.close()
    X, theta = r["eigenvectors"], r["eigenvalues"]
    rho = np.linalg.norm(A @ X - X * theta, axis=0)
    assert r["converged"] and np.all(rho <= 2.0 * tol * theta[0])
    assert np.all(np.abs(theta - lam[:K]) <= rho * (1.0 + 1e-9) + 1e-14 * lam[0])
    assert np.all(theta - bare["eigenvalues"] >= 0.1 - 1e-9)   # the shift is there: A >= K + 0.1 I


def test_maxit_equal_k_is_not_converged_with_everything_written():
    """4. exp(-r), maxit = k: one look after k steps."""
    tol = er.TOLS["float64"]
    A, lam, _ = er.system("absolute-exponential", "kernel")
    ref = er.eigsh(A, K, er.start_vector(), tol, K)
    r = gpu_eigsh("absolute-exponential", "kernel", maxit=K, want_coefficients=True)
    assert not r["converged"] and r["steps"] == K
    for key in ("eigenvalues", "eigenvectors", "resid"):
        assert np.all(np.isfinite(r[key])), key
    assert np.all(np.isfinite(r["alpha"])) and np.all(np.isfinite(r["beta"]))
    assert r["resid"].max() > 1.5 * tol
    assert np.max(np.abs(r["eigenvalues"] - ref.eigenvalues)) <= 1e-10 * lam[0]


def test_breakdown_on_eight_points():
    """5. N = 8, k = 3, maxit = 8, tol 1e-12: the Krylov space is the whole space after at most 8 steps."""
    y = device_points("float64", 8, seed=3)
    A = er.operator(er.kernel_matrix("gaussian", np.asarray(y, dtype=np.float64)), "kernel")
    lam = np.linalg.eigvalsh(A)[::-1]
    ctx = _lib.Context(0)
    try:
        ctx.set_points(y, None, _lib.KMVP_F64)
        r = ctx.eigsh("gaussian", 3, "kernel", er.start_vector(8), 1e-12, 8)
    finally:
        ctx.close()
    print(f"[5] steps {r['steps']}, resid {r['resid']}")
    assert r["converged"] and r["steps"] <= 8
    assert np.max(np.abs(r["eigenvalues"] - lam[:3])) <= 1e-12 * lam[0]


def same(a, b):
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in a if k != "converged") and a["converged"] == b["converged"]


def test_bitwise_and_nothing_left_behind():
    """6. two calls return the same bits, the vectors obey the sign rule, no signal is left behind, and a product on the
    same context returns the same bits before and after."""
    b_signal = np.random.RandomState(4).standard_normal((N, 2))

    def product(ctx):
        ctx.set_signal(b_signal)
        ctx.run("gaussian", False)
        return ctx.get_result(N, 2)

    ctx = open_context()
    try:
        before = product(ctx)
        outs = [ctx.eigsh("gaussian", K, op, er.start_vector(), 1e-10, MAXIT, want_coefficients=True)
                for op in ("normalized", "normalized", "centered", "centered")]
        assert ctx.last_total_ms > 0.0 and ctx.last_kernel_ms == ctx.last_total_ms
        with pytest.raises(_lib.KmvpError):   # no signal is left behind
            ctx.run("gaussian", False)
        after = product(ctx)
    finally:
        ctx.close()
    assert same(outs[0], outs[1]) and same(outs[2], outs[3])
    assert all(obeys_sign_rule(o["eigenvectors"]) for o in outs)
    assert np.array_equal(before, after)


def test_refusals_through_the_c_abi():
    """7. every KMVP_E_INVALID and KMVP_E_UNSUPPORTED case of the header, each with its message; the context works after."""
    lib = _lib.load()
    assert not hasattr(lib, "kmvp_invdist_eigsh")
    v0 = er.start_vector()
    ev, X, resid, steps = np.zeros(N), np.zeros((N, N)), np.zeros(N), np.zeros(1, dtype=np.intc)

    def raw(ctx, k=K, op=0, v=v0, tol=1e-8, maxit=64, out=(ev, X, resid, steps)):
        ptr = [None if a is None else a.ctypes.data for a in out]
        rc = lib.kmvp_gaussian_eigsh(ctx._ctx, k, op, None if v is None else v.ctypes.data, tol, maxit, ptr[0], ptr[1], ptr[2],
                                     ptr[3], None, None, None)
        return rc, lib.kmvp_last_error(ctx._ctx).decode()

    ctx = _lib.Context(0)
    try:
        rc, msg = raw(ctx)
        assert rc == 1 and "kmvp_set_points" in msg, (rc, msg)   # no points set
        ctx.set_points(device_points("float64"), None, _lib.KMVP_F64)
        with pytest.raises(NotImplementedError):
            ctx.eigsh("inverse-distance", K, "kernel", v0, 1e-8, 64)
        with pytest.raises(ValueError):
            ctx.eigsh("gaussian", K, "kernel", v0[:100], 1e-8, 64)
        with pytest.raises(ValueError):
            ctx.eigsh("gaussian", K, "diffusion", v0, 1e-8, 64)
        nan_v, const_v = v0.copy(), np.full(N, 0.25)
        nan_v[17] = np.nan
        inf_v = v0.copy()
        inf_v[3] = np.inf
        cases = [({"k": 0}, "k ="), ({"k": -2}, "k ="), ({"k": N + 1, "maxit": N}, "k ="),
                 ({"maxit": K - 1}, "maxit"), ({"maxit": 513}, "maxit"), ({"op": 3}, "operator"), ({"op": -1}, "operator"),
                 ({"tol": 0.0}, "tol"), ({"tol": -1.0}, "tol"), ({"tol": float("nan")}, "tol"),
                 ({"v": None}, "NULL"), ({"out": (None, X, resid, steps)}, "NULL"), ({"out": (ev, None, resid, steps)}, "NULL"),
                 ({"out": (ev, X, None, steps)}, "NULL"), ({"out": (ev, X, resid, None)}, "NULL"),
                 ({"v": nan_v}, "finite"), ({"v": inf_v}, "finite"), ({"v": np.zeros(N)}, "zero"),
                 ({"v": const_v, "op": 1}, "zero after centring")]
        for kwargs, word in cases:
            rc, msg = raw(ctx, **kwargs)
            assert rc == 1 and word in msg, (kwargs, rc, msg)
        rc, msg = raw(ctx, v=const_v)   # a constant start is fine for the plain operator
        assert rc in (0, 6), (rc, msg)
        # maxit > N on a small cloud
        ctx.set_points(device_points("float64", 40), None, _lib.KMVP_F64)
        rc, msg = raw(ctx, v=er.start_vector(40), maxit=41)
        assert rc == 1 and "maxit" in msg, (rc, msg)
        # targets != sources
        y = device_points("float64")
        ctx.set_points(y, y[:100], _lib.KMVP_F64)
        rc, msg = raw(ctx)
        assert rc == 1 and msg, (rc, msg)
        # batches set
        ctx.set_points(y, None, _lib.KMVP_F64)
        ctx.set_batches(np.array([0, 300, N]))
        rc, msg = raw(ctx)
        assert rc == 2 and "eigen-solver" in msg and "batch" in msg, (rc, msg)
        ctx.set_batches(None)
        # a bfloat16 context
        ctx.set_points(device_points("float32"), None, _lib.KMVP_BF16)
        rc, msg = raw(ctx)
        assert rc == 2 and "float32 or float64" in msg, (rc, msg)
        # and the context still works
        ctx.set_points(y, None, _lib.KMVP_F64)
        ctx.set_solver_preconditioner(16)   # ignored
        r = ctx.eigsh("gaussian", K, "kernel", v0, 1e-10, MAXIT)
    finally:
        ctx.close()
    assert r["converged"] and same(r, gpu_eigsh("gaussian", "kernel"))


@pytest.mark.parametrize("op", er.OPERATORS)
def test_a_nan_coordinate_returns_not_converged(op):
    """8. the call returns, KMVP_E_NOT_CONVERGED, outputs non-finite."""
    y = device_points("float64")
    y[123, 1] = np.nan
    ctx = _lib.Context(0)
    try:
        ctx.set_points(y, None, _lib.KMVP_F64)
        r = ctx.eigsh("gaussian", K, op, er.start_vector(), 1e-10, 64)
    finally:
        ctx.close()
    assert not r["converged"]
    assert not np.any(np.isfinite(r["eigenvalues"])) and not np.any(np.isfinite(r["resid"]))
    assert not np.all(np.isfinite(r["eigenvectors"]))


@pytest.mark.parametrize("precision", ("float64", "float32"))
@pytest.mark.parametrize("op", er.OPERATORS)
def test_plugin(op, precision):
    """9. MI355XSpectral: eigenpairs, get_embedding() and transform() of 50 fresh points against the dense formulas."""
    kernel, tol = "gaussian", er.TOLS[precision]
    A, lam, y = er.system(kernel, op, precision)
    algo = MI355XSpectral(kernel=kernel, dimension=er.D, precision=np.dtype(precision), n_components=K, operator=op, seed=3)
    try:
        with pytest.raises(RuntimeError):
            algo.query()
        algo.prepare_data(points=device_points(precision))
        with pytest.raises(RuntimeError):
            algo.get_embedding()
        algo.fit()
        algo.query()
        theta, X = algo.get_eigenvalues(), algo.get_eigenvectors()
        extra = algo.get_additional()
        assert extra["converged"] and extra["steps"] >= K and algo.get_memory_usage() > 0
        assert np.all(algo.get_residuals() <= 1.5 * tol)
        rho = np.linalg.norm(A @ X - X * theta, axis=0)
        assert np.all(rho <= 2.0 * tol * theta[0])
        assert np.all(np.abs(theta - lam[:K]) <= rho * (1.0 + 1e-9) + 1e-14 * lam[0])
        assert np.array_equal(algo.get_embedding(), er.embedding(op, theta, X))
        if op == "normalized":
            assert np.max(np.abs(np.linalg.norm(algo.get_embedding(), axis=1) - 1.0)) <= 1e-14
            assert np.max(np.abs(algo.get_degree() - er.kmatrix(kernel, precision).sum(axis=1))) <= kr.TOL[precision] * N
        x_new = device_points(precision, 50, seed=99)
        if op == "normalized":
            with pytest.raises(NotImplementedError):
                algo.transform(x_new)
        else:
            got = algo.transform(x_new)
            ref = er.transform(kernel, op, y, theta, X, np.asarray(x_new, dtype=np.float64))
            print(f"[9] {op} {precision}: transform error {np.max(np.abs(got - ref)):.3g}, bound {2 * tol * np.sqrt(lam[0]):.3g}")
            assert got.shape == (50, K) and np.max(np.abs(got - ref)) <= 2.0 * tol * np.sqrt(lam[0])
    finally:
        algo.done()


def test_plugin_arguments():
    with pytest.raises(NotImplementedError):
        MI355XSpectral(kernel="inverse-distance", dimension=3, n_components=2)
    with pytest.raises(NotImplementedError):
        MI355XSpectral(kernel="gaussian", dimension=3, n_components=2, precision="bfloat16")
    with pytest.raises(ValueError):
        MI355XSpectral(kernel="gaussian", dimension=3, n_components=2, operator="diffusion")
    with pytest.raises(ValueError):
        MI355XSpectral(kernel="gaussian", dimension=3, n_components=2, operator="centered", ridge=0.1)
    with pytest.raises(ValueError):
        MI355XSpectral(kernel="gaussian", dimension=3, n_components=0)
    algo = MI355XSpectral(kernel="gaussian", dimension=3, n_components=K, ridge=0.1, precision=np.float16)
    try:
        algo.prepare_data(points=er.cloud())
        algo.set_query_arguments(tol=1e-4, maxit=128)
        algo.query(v0=er.start_vector())
        assert algo.get_additional()["converged"] and algo.get_degree() is None
        y16 = er.cloud(dtype=np.float16)   # float16: rounded points, float32 arithmetic
        lam = np.linalg.eigvalsh(er.operator(er.kernel_matrix("gaussian", y16), "kernel", ridge=0.1))[::-1]
        assert np.max(np.abs(algo.get_eigenvalues() - lam[:K])) <= 2e-4 * lam[0]
    finally:
        algo.done()


def test_two_ranks_on_one_gpu():
    """10. two ranks on GPU 0 through the host-staged exchange, uneven source shards: both ranks return the same bits,
    and the eigenvalues are those of the single-GPU run to 1e-12 lambda_1."""
    out = _spawn([os.path.join(HERE, "_eigsh_rank_worker.py")], world=2, timeout=600)
    rep = json.loads([l for l in out.splitlines() if l.startswith("{")][-1])
    assert rep["world"] == 2 and rep["shards"] == [[0, 300], [300, N]] and rep["ranks_bitwise_equal"], rep
    for op in er.OPERATORS:
        one = gpu_eigsh("gaussian", op)
        two = rep["outputs"][op]
        _, lam, _ = er.system("gaussian", op)
        assert two["converged"] and two["steps"] == one["steps"]
        assert np.max(np.abs(np.array(two["eigenvalues"]) - one["eigenvalues"])) <= 1e-12 * lam[0]
        assert np.max(np.array(two["resid"])) <= 1.5e-10
