"""CPU tests of the cutoff-radius gradients' test infrastructure (tests/cutoff_grad_reference.py, tests/wendland_grad_model.py)
and of the entry points' declarations (include/kmvp.h kmvp_<kernel>_cutoff_grad).  No GPU."""
import os
import re

import numpy as np
import pytest

import cutoff_grad_reference as gr
import cutoff_reference as cr
import wendland_grad_model as wgm
import wendland_reference as wr
from kernel_matrix_benchmarks_amd import _lib
from kernel_matrix_benchmarks_amd.algorithms import mi355x

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("kmvp_gaussian_cutoff_grad", "kmvp_absexp_cutoff_grad", "kmvp_matern32_cutoff_grad", "kmvp_matern52_cutoff_grad",
           "kmvp_wendland_c2_cutoff_grad", "kmvp_wendland_c4_cutoff_grad")
H = 2.0 ** -27      # the finite-difference step: below the clouds' clearance of the boundary (see test_reference_is_...)


def test_entry_points_are_declared_exported_and_bound():
    """The CPU test that fails without the feature: the six symbols in the header, in the built library and in _lib."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kmvp.h")).read(), flags=re.S)
    lib = _lib.load()
    listed = {name: (restype, argtypes) for name, restype, argtypes in _lib.SYMBOLS}
    for name in SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(\s*kmvp_ctx\s*\*\s*\w+\s*,\s*double\s+\w+\s*\)" % name, text), f"kmvp.h does not declare {name}"
        assert hasattr(lib, name), f"libkmvp.so lacks {name}"
        assert name in listed, f"_lib.SYMBOLS lacks {name}"
        assert listed[name][0] is _lib._c.c_int and listed[name][1] == [_lib._c.c_void_p, _lib._c.c_double]
    assert not re.search(r"kmvp_invdist_cutoff_grad|kmvp_expdot_cutoff_grad", text)   # no inverse-distance entry
    assert lib.kmvp_abi_version() == 1  # entries were added, nothing changed
    assert callable(getattr(_lib.Context, "run_cutoff_grad", None))
    assert callable(getattr(mi355x.MI355XProduct, "query_cutoff_gradient", None))


def _product(kernel, y, x, b, R):
    if kernel in gr.WENDLAND:
        return wr.product(kernel, y, R, b, x)
    return cr.dense(kernel, y, x, b, R)[0]


@pytest.mark.parametrize("kernel", gr.KERNELS)
@pytest.mark.parametrize("name", ("A", "B", "C"))
def test_reference_is_the_finite_difference_of_the_product(name, kernel):
    """Central differences of wendland_reference.product, resp. cutoff_reference.dense, in every target coordinate at step
    h = 2^-27.  The float32 clouds have no pair within 1e-5 R^2 of the boundary in s, i.e. within 5e-6 R >= 2.5e-7 in r: the
    step moves no pair across it, so the truncated sums are differentiated where they are smooth.  Tolerance, per element:
    64 * 2^-53 * sum_j k |b_j| / h for the float64 roundings of the two products (a few units in exp and sqrt per pair) plus
    h^2 * 1e6 * sum_j |b_j| for the truncation (h^2 / 6 times a third derivative below 6e6 at these radii)."""
    y, x, R = cr.cloud(name, np.float32)
    assert cr.boundary_clear(y, x, R, np.float32)
    xx = y.copy() if x is None else x
    b = np.random.RandomState(3).randn(len(y), 2)
    want = gr.dense(kernel, y, xx, b, R)
    kmass = _product(kernel, y, xx, np.abs(b), R)
    tol = 64 * 2.0 ** -53 * kmass / H + H * H * 1e6 * np.abs(b).sum(axis=0)
    for d in range(y.shape[1]):
        step = np.zeros(y.shape[1])
        step[d] = H
        fd = (_product(kernel, y, xx + step, b, R) - _product(kernel, y, xx - step, b, R)) / (2 * H)
        err = np.abs(fd - want[:, :, d])
        assert (err <= tol).all(), (d, float(np.max(err / tol)))
    assert np.abs(want).max() > 1e3 * tol.max()      # (the tolerance is far below the gradients it checks)


@pytest.mark.parametrize("kernel", gr.KERNELS)
def test_weighted_gradients_cancel(kernel):
    """sum_i b_i G_i = sum_ij b_i b_j w_ij (x_i - x_j) = 0 when the targets are the sources: w is symmetric, the difference
    antisymmetric.  To float64 rounding: M terms per row and N rows, 2 (N + M) 2^-53 of the sum of the absolute terms."""
    for name in ("A", "K"):
        y, _, R = cr.cloud(name, np.float64)
        b = np.random.RandomState(4).randn(len(y), 1)
        G = gr.dense(kernel, y, None, b, R)[:, 0, :]
        Gabs = np.abs(gr.constant(kernel, R)) * np.einsum("nm,nmd->nd", _absw(kernel, y, R) * np.abs(b[:, 0])[None, :],
                                                          np.abs(y[:, None, :] - y[None, :, :]))
        total = (b * G).sum(axis=0)
        assert (np.abs(total) <= 4 * len(y) * 2.0 ** -53 * (np.abs(b) * Gabs).sum(axis=0)).all(), (name, total)
        assert np.abs(G).max() > 0.1


def _absw(kernel, y, R):
    s = cr.sqdists(y, y)
    inside = s <= R * R
    return np.where(inside, gr.weights(kernel, np.where(inside, s, 0.0), R), 0.0)


@pytest.mark.parametrize("kernel", gr.WENDLAND)
def test_wendland_model_without_rounding_is_the_reference(kernel):
    for name in ("A", "B", "C"):
        for precision in (np.float32, np.float64):
            y, x, R = cr.cloud(name, precision)
            b = np.asarray(np.random.RandomState(6).randn(len(y), 3), dtype=precision).astype(np.float64)
            for sig in (b, None):
                m = wgm.gradient(kernel, y, x, sig, R, precision=precision, rounding=False)
                want = gr.dense(kernel, y, x, sig, R)
                assert m.value.shape == want.shape == (len(y if x is None else x), 1 if sig is None else 3, y.shape[1])
                assert (np.abs(m.value - want) <= 2.0 ** -44 * m.mass + 1e-300).all(), (name, precision)


@pytest.mark.parametrize("prec", ("f32", "f64"))
@pytest.mark.parametrize("kernel", gr.WENDLAND)
def test_restated_pair_sequence_is_inside_the_pair_bound(kernel, prec):
    """cutoff_grad_interact's sequence in numpy's float32 / float64 on every pair of cloud A: a pair the model lists (it may
    be inside) has its weight within `each` and its density term W' df'_d within the pair bound at NR = 1; every other pair is
    an exact 0 in the weight and in every difference."""
    precision = np.dtype({"f32": np.float32, "f64": np.float64}[prec])
    y, x, R = cr.cloud("A", precision)
    W1, df1 = wgm.restate(kernel, y, x, R, precision)
    p = wgm.pairs(kernel, y, x, R, precision)
    listed = np.zeros(W1.shape, dtype=bool)
    listed[p.i, p.j] = True
    assert (W1[~listed] == 0).all() and (df1[~listed] == 0).all() and not np.signbit(W1[~listed]).any()
    u = wgm.unit(precision)
    eta = 2.0 ** -150 if precision == np.float32 else wgm.lm.ETA64
    Wp = W1[p.i, p.j].astype(np.float64)
    assert (np.abs(Wp - p.W) <= p.each).all(), float(np.max(np.abs(Wp - p.W) / np.maximum(p.each, 1e-300)))
    term = Wp[:, None] * df1[p.i, p.j].astype(np.float64)
    bound = (p.each * (1 + u) + p.W * u)[:, None] * np.abs(p.df) + eta * 2.0 * (1.0 + np.abs(p.df))
    assert (np.abs(term - p.W[:, None] * p.df) <= bound).all()
    assert (p.W > 0.1).sum() > 1000          # (the cloud does exercise the weights)
