"""The numpy restatement of the cutoff-radius entries (tests/cutoff_reference.py) against itself: the truncated product
and the neighbour count formed the way the kernels form them -- tile by tile over the runs of the cell-list plan -- are
held to the dense masked evaluation over all N x M pairs in float64.  The counts must be equal; the products differ by
the order of a float64 sum at most."""
import numpy as np
import pytest

import cutoff_reference as cr


def agree(got, want, mass, den, M):
    """Equal counts, NaN in the same places, and the products within the rounding of two float64 sums of M terms taken in
    different orders: 2 M 2^-53 times the row's mass sum_j k |b_j| (normalised: the quotient's share, over the denominator)."""
    (a, ca), (b, cb) = got, want
    assert np.array_equal(ca, cb)
    assert np.array_equal(np.isnan(a), np.isnan(b))
    u = 2.0 * M * 2.0 ** -53
    with np.errstate(all="ignore"):
        tol = u * mass if den is None else 2 * u * (mass / den + np.abs(b))
    ok = ~np.isnan(b)
    assert np.all(np.abs(a - b)[ok] <= np.broadcast_to(tol, b.shape)[ok])


@pytest.mark.parametrize("kernel", cr.KERNELS)
@pytest.mark.parametrize("name", cr.CLOUDS + ("lattice",))
def test_walk_is_the_dense_masked_product(name, kernel):
    y, x, R = cr.cloud(name, np.float64)
    xx = y if x is None else x
    rs = np.random.RandomState(len(name) + len(kernel))
    b = rs.randn(len(y), 3)
    for factor in (1.0, 1.5, 2.0):
        p = cr.plan(y, xx, R, factor)
        for sig, normalize in ((b, False), (b, True), (None, False), (None, True)):
            mass = cr.dense(kernel, y, xx, None if sig is None else np.abs(sig), R)[0].max(axis=1, keepdims=True)
            den = cr.dense(kernel, y, xx, None, R)[0] if normalize else None
            agree(cr.walk(kernel, y, xx, sig, R, normalize, x is None, p=p),
                  cr.dense(kernel, y, xx, sig, R, normalize, x is None), mass, den, len(y))


def test_lattice_boundary_pairs_count():
    """16 x 16 points (a / 8, b / 8), R = 5 / 8: s and R R are exact, and the pairs at offset (+-3, +-4), (+-4, +-3),
    (+-5, 0), (0, +-5) sit exactly on the boundary and count."""
    y, _, R = cr.cloud("lattice", np.float32)
    _, cnt = cr.walk("gaussian", y, y, None, R)
    a, b = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    want = np.zeros(256, dtype=np.int64)
    for i, (pa, pb) in enumerate(zip(a.ravel(), b.ravel())):
        want[i] = int((((a - pa) ** 2 + (b - pb) ** 2) <= 25).sum())
    assert np.array_equal(cnt, want) and cnt.max() == 81 and cnt[0] == 26


def test_non_finite_rules():
    rs = np.random.RandomState(3)
    y, x = rs.rand(200, 2), rs.rand(90, 2)
    b = rs.randn(200, 2)
    base = cr.walk("gaussian", y, x, b, 0.2)
    y2, x2 = y.copy(), x.copy()
    y2 = np.concatenate([y2, [[np.nan, 0.5], [0.5, np.inf]]])
    b2 = np.concatenate([b, [[1.0, 1.0], [1.0, 1.0]]])
    x2[7, 0], x2[8, 1] = np.nan, np.inf
    for fn in (cr.walk, cr.dense):
        out, cnt = fn("gaussian", y2, x2, b2, 0.2)
        keep = np.ones(90, dtype=bool)
        keep[[7, 8]] = False
        assert np.all(np.isnan(out[7])) and cnt[7] == -1 and np.all(out[8] == 0) and cnt[8] == 0
        assert np.array_equal(cnt[keep], base[1][keep]) and np.allclose(out[keep], base[0][keep], rtol=1e-13, atol=0)
        out, _ = fn("gaussian", y2, x2, b2, 0.2, True)
        assert np.all(np.isnan(out[8]))
    out, cnt = cr.walk("gaussian", y, y, None, 0.2, exclude_self=True)
    assert np.array_equal(cnt + 1, cr.dense("gaussian", y, y, None, 0.2)[1])
