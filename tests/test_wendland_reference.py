"""CPU tests of the Wendland reference and model (tests/wendland_reference.py, tests/wendland_model.py): the closed forms,
positive definiteness for D <= 3, and the model's per-pair band against a numpy float32 restatement of the kernel's own
sequence of operations."""
import numpy as np
import pytest

import krylov_reference as kr
import wendland_model as wm
import wendland_reference as wr


def test_closed_forms():
    """t = 0: 1;  t = 1/2: C2 = 3 / 16, C4 = (35/4 + 9 + 3) / (3 * 64) = 83 / 768;  t = 1 and beyond: exactly 0;  NaN stays."""
    t = np.array([0.0, 0.5, 1.0, 1.0 + 2.0 ** -52, 1.5, 1e300, np.inf])
    c2, c4 = wr.values("wendland-c2", t), wr.values("wendland-c4", t)
    assert c2[0] == 1.0 and c4[0] == 1.0
    assert c2[1] == 3.0 / 16.0 and abs(c4[1] - 83.0 / 768.0) <= 2.0 ** -53
    assert not c2[2:].any() and not c4[2:].any()
    assert np.isnan(wr.values("wendland-c2", np.array([np.nan]))[0])
    with pytest.raises(ValueError):
        wr.values("gaussian", t)
    # the polynomials: u^4 (4 t + 1) and u^6 (35 t^2 + 18 t + 3) / 3 on a grid, and both decrease on [0, 1]
    g = np.linspace(0.0, 1.0, 1001)
    assert np.allclose(wr.values("wendland-c2", g), (1 - g) ** 4 * (4 * g + 1), rtol=0, atol=1e-15)
    assert np.allclose(wr.values("wendland-c4", g), (1 - g) ** 6 * (35 * g * g + 18 * g + 3) / 3, rtol=0, atol=1e-15)
    assert (np.diff(wr.values("wendland-c2", g)) <= 0).all() and (np.diff(wr.values("wendland-c4", g)) <= 0).all()


def test_products_and_radius():
    rs = np.random.RandomState(3)
    y, x, b = rs.rand(300, 3), rs.rand(100, 3), rs.randn(300, 2)
    R = wr.radius_for(300, 3, 20)
    K = wr.kernel_matrix("wendland-c2", y, R, x)
    assert K.shape == (100, 300) and (K >= 0).all() and (K <= 1).all()
    inside = wr.sqdists(x, y) < R * R
    assert np.array_equal(K > 0, inside) and 10 < inside.sum(axis=1).mean() < 20      # (the boundary takes its share)
    assert np.allclose(wr.product("wendland-c2", y, R, b, x), K @ b)
    assert np.allclose(wr.product("wendland-c2", y, R, None, x, normalize_rows=True)[inside.any(axis=1)], 1.0)
    S = wr.kernel_matrix("wendland-c4", y, R)
    assert np.array_equal(S, S.T) and np.all(np.diag(S) == 1.0)


@pytest.mark.parametrize("D", (1, 2, 3))
def test_positive_definite(D):
    """2000 uniform points, R for a mean of 16 and of 32 points inside: the smallest eigenvalue of both matrices is positive.
    On these draws it runs from 1.3e-10 (C2, D = 1) to 1.4e-2 (D = 3), condition numbers 2.7e2 .. 1.3e11.  The one
    exception is C4 at D = 1, condition 1e13 and 8e14: there the computed lambda_min (7.3e-13, 1.9e-14) is below what
    eigvalsh itself resolves, n 2^-52 lambda_max = 7e-12 (its backward error bound), so the assertion there is
    lambda_min > -n 2^-52 lambda_max -- positive as far as float64 can tell."""
    y = np.random.RandomState(100 + D).rand(2000, D)
    for inside in (16, 32):
        R = wr.radius_for_mean(y, inside)
        for kernel in wr.KERNELS:
            lam = np.linalg.eigvalsh(wr.kernel_matrix(kernel, y, R))
            resolved = len(y) * 2.0 ** -52 * lam[-1]
            print(f"D={D} inside={inside} {kernel}: lambda_min {lam[0]:.3g} cond {lam[-1] / lam[0]:.3g} (eigvalsh resolves {resolved:.1g})")
            floor = -resolved if (D == 1 and kernel == "wendland-c4") else 0.0
            assert lam[0] > floor, (D, inside, kernel, lam[0])


@pytest.mark.parametrize("kernel", wr.KERNELS)
@pytest.mark.parametrize("D", (1, 2, 3))
def test_float32_restatement_inside_the_band(kernel, D):
    """Every pair of a 2000-point cloud: the float32 restatement of the kernel's sequence (numpy's correctly rounded sqrt in
    place of v_sqrt_f32: inside TRANS) is within K_BAND x the derived per-pair bound of the float64 value.  Prints the worst
    error in units of 2^-24 and the worst err / band."""
    y = np.random.RandomState(200 + D).rand(2000, D).astype(np.float32)
    R = wr.radius_for(2000, D, 32)
    got = wm.restate(kernel, y, None, R, np.float32).astype(np.float64)
    k, each = wm.pair_bound(kernel, np.float32, wr.sqdists(y.astype(np.float64), y.astype(np.float64)), R, D)
    err = np.abs(got - k)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err > 0, err / (wm.K_BAND * each), 0.0)
    print(f"\n{kernel} D={D}: worst error {err.max() / 2.0 ** -24:.2f} x 2^-24, worst err / band {ratio.max():.3f}, "
          f"{int((k > 0).sum())} pairs inside")
    assert (err <= wm.K_BAND * each).all(), float(ratio.max())
    assert (got[k == 0] == 0).all() or (each[(k == 0) & (got != 0)] > 0).all()
    assert 0.05 < ratio.max(), "the band is not vacuous"


def test_model_value_and_modes():
    """Rounding aside the model's value is the reference's product; normalised rows; an empty row is 0 resp. NaN with band 0."""
    rs = np.random.RandomState(5)
    y, b = rs.rand(400, 2).astype(np.float32), rs.randn(400, 3).astype(np.float32)
    x = np.concatenate([rs.rand(50, 2), [[5.0, 5.0]]]).astype(np.float32)
    R = wr.radius_for(400, 2, 12)
    for precision in (np.float32, np.float64):
        m = wm.product("wendland-c4", y, x, b, R, precision=precision, folds=4)
        want = wr.product("wendland-c4", y, R, b, x)
        assert np.allclose(m.value, want, rtol=1e-13, atol=1e-15) and (m.band[:-1] > 0).all() and not m.band[-1].any()
        assert (m.band[:-1] < 1e-4 * (m.mass[:-1] + 1e-30)).all()
        n = wm.product("wendland-c4", y, x, b, R, True, precision=precision, folds=4)
        assert np.allclose(n.value[:-1], wr.product("wendland-c4", y, R, b, x, True)[:-1], rtol=1e-12, atol=1e-15)
        assert np.isnan(n.value[-1]).all() and not n.band[-1].any()
        d = wm.product("wendland-c2", y, None, None, R, precision=precision)
        assert d.value.shape == (400, 1) and (d.value >= 1.0).all()


@pytest.mark.parametrize("case", list(wr.SOLVE_CASES))
def test_solve_draws_are_reproducible(case):
    """The float64 CG restatement takes the same number of iterations on the system of every solve case when each operator
    output carries rounding-level noise (wendland_reference.SOLVE_NOISE), three seeds: what makes the GPU test's "the same
    count" meaningful on a 2000-point system."""
    prec, D, kernel, ridge, rtol, E, seed = wr.SOLVE_CASES[case]
    y, R, a, diag, K = wr.solve_system(case)
    A = K + np.diag(diag)
    ref = kr.cg(A, a, rtol, 3000)
    noisy = [kr.cg(A, a, rtol, 3000, noise=wr.SOLVE_NOISE[prec], seed=s).iters for s in range(3)]
    print(f"{case}: {ref.iters} iterations, with noise {noisy}, mean inside {(K > 0).sum(axis=1).mean():.1f}")
    assert ref.rel[-1].max() <= rtol and noisy == [ref.iters] * 3
