"""CPU tests of the numpy restatement the GPU tests of the length-scale derivative compare with (dscale_reference.py): it
is the derivative of the pinned oracle's product (Matern: of matern_reference's, itself pinned to the Bessel form) under
a per-axis scaling of both clouds, its axes add up to the closed-form isotropic derivative, and its conventions hold."""
import numpy as np
import pytest

import dscale_reference
import kmvp_oracle
import matern_reference
from conftest import rel_err


def product(kernel, y, x, b):
    if kernel in matern_reference.KERNELS:
        return matern_reference.product(kernel=kernel, source_points=y, target_points=x, source_signal=b)
    return kmvp_oracle.product(kernel=kernel, source_points=y, target_points=x, source_signal=b)


@pytest.mark.parametrize("kernel", dscale_reference.KERNELS)
@pytest.mark.parametrize("D", (1, 2, 3, 5, 8))
@pytest.mark.parametrize("E", (1, 3))
def test_restatement_is_the_derivative_of_the_product_in_log_length_scales(kernel, D, E):
    """Length scales l_d = exp(theta_d) are the caller's scaling of the points: both clouds times exp(-theta_d) on axis d.
    Central differences in theta_d (h = 1e-4) on separated clouds (r >= 0.5, as the gradient's check): the truncation
    h^2 |f'''| / (6 |f'|) of f(theta) = k(r(theta)) is below 1e-7 for these kernels there, so 1e-6 holds with room."""
    rs = np.random.RandomState(2000 + 10 * D + E)
    y = rs.rand(97, D)
    x = rs.rand(130, D)
    x[:, 0] += 1.5
    b = rs.randn(97, E)
    h = 1e-4
    fd = np.empty((130, E, D))
    for d in range(D):
        up, down = np.ones(D), np.ones(D)
        up[d], down[d] = np.exp(-h), np.exp(h)
        fd[:, :, d] = (product(kernel, y * up, x * up, b) - product(kernel, y * down, x * down, b)) / (2 * h)
    H = dscale_reference.scale_derivative(kernel=kernel, source_points=y, target_points=x, source_signal=b)
    assert H.shape == (130, E, D) and H.dtype == np.float64 and H.flags["C_CONTIGUOUS"]
    err = rel_err(H.reshape(130, -1), fd.reshape(130, -1))
    print(f"{kernel} D={D} E={E}: restatement vs central differences {err:.2e}")
    assert err <= 1e-6, (kernel, D, E, err)


@pytest.mark.parametrize("kernel", dscale_reference.KERNELS)
def test_axes_add_up_to_the_isotropic_closed_form(kernel):
    """sum_d H_d = sum_j -s w(s) b_j: 2 s k, r k, 3 r^2 e^-t, (5/3) r^2 (1 + t) e^-t -- overlapping clouds, same points
    (own pairs: 0) and density mode."""
    rs = np.random.RandomState(7)
    y, x, b = rs.rand(120, 3), rs.rand(77, 3), rs.randn(120, 2)
    for xx, bb in ((x, b), (None, b), (x, None)):
        H = dscale_reference.scale_derivative(kernel=kernel, source_points=y, target_points=xx, source_signal=bb)
        want = dscale_reference.isotropic(kernel=kernel, source_points=y, target_points=xx, source_signal=bb)
        assert H.shape[1:] == (want.shape[1], 3)
        assert rel_err(H.sum(axis=2), want) <= 1e-13, kernel


@pytest.mark.parametrize("kernel", dscale_reference.KERNELS)
def test_restatement_conventions(kernel):
    """Coincident pairs contribute 0 (rows finite; dropping the duplicate source changes nothing), a source whose squared
    distance overflows float32 contributes exactly 0, a NaN target coordinate spoils its own row only."""
    rs = np.random.RandomState(11)
    y, b = rs.rand(64, 3), rs.randn(64, 2)
    y[40] = y[5]
    H = dscale_reference.scale_derivative(kernel=kernel, source_points=y, source_signal=b)
    assert np.isfinite(H).all()
    keep = np.arange(64) != 40
    without = dscale_reference.scale_derivative(kernel=kernel, source_points=y[keep], target_points=y[5:6], source_signal=b[keep])
    assert rel_err(H[5:6].reshape(1, -1), without.reshape(1, -1)) <= 1e-14
    for precision in (np.float32, np.float64):
        far = np.array([[3e19, 0.5, 0.5]]) if precision == np.float32 else np.array([[2e154, 0.5, 0.5]])
        alone = dscale_reference.scale_derivative(kernel=kernel, source_points=far, target_points=y,
                                                  source_signal=np.array([[1e3, -1e3]]), precision=precision)
        assert (alone == 0).all(), (kernel, precision)
    x = rs.rand(10, 3)
    x[3, 1] = np.nan
    H = dscale_reference.scale_derivative(kernel=kernel, source_points=y, target_points=x, source_signal=b)
    bad = ~np.isfinite(H).reshape(10, -1)
    assert bad[3].any() and not bad[np.arange(10) != 3].any()
