"""The radius search's restatement against brute force, without a GPU (tests/radius_nearest_reference.py): walk() inserts
every inside record of the cell-list plan in walk order under the lexicographic rule on (s, caller's index) and must give
dense()'s rows -- numpy's lexsort over all pairs -- on every cloud of the GPU tests, at the three cell factors.  The
lattices are what gives the tie rule teeth: there the brute-force kernels' strict s < s_t, applied in walk order, returns
other rows, and the last test asserts that it does."""
import numpy as np
import pytest

import cutoff_reference as cr
import radius_nearest_reference as rn


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1], equal_nan=True)


@pytest.mark.parametrize("name", rn.CLOUDS)
def test_walk_equals_dense(name):
    """K = 1, 4, 16 (and 15 with exclude_self where the targets are the sources), factors 1.0 / 1.5 / 2.0."""
    y, x, R = rn.cloud(name, np.float32)
    cases = [(1, False), (4, False), (16, False)] + ([(3, True), (15, True)] if x is None else [])
    want = {c: rn.dense(y, x, R, *c) for c in cases}
    full = tail = 0
    for factor in rn.FACTORS:
        p = cr.plan(y, y if x is None else x, R, factor)
        for c in cases:
            got = rn.walk(y, x, R, *c, factor=factor, p=p)
            assert same(got, want[c]), (name, factor, c)
    idx = want[(16, False)][0]
    full, tail = int((idx[:, -1] >= 0).sum()), int((idx[:, 4] < 0).sum())
    assert full > 0                                     # every cloud has rows with a full list of 16 ...
    if name in ("B", "K"):
        assert tail > 0                                 # ... and B and K rows with fewer than 5 sources inside


def test_dense_on_the_lattices_is_integer_arithmetic():
    """On the lattices s is an integer / 64 and R R = 25 / 64, resp. 9 / 64: dense() is the integer brute force, with
    pairs exactly ON the boundary inside."""
    for name, bound, on_boundary in (("lattice", 25, 12), ("lattice3", 9, 30)):
        y, _, R = rn.cloud(name, np.float32)
        a = np.rint(y * 8).astype(np.int64)
        d = a[:, None, :] - a[None, :, :]
        s_int = (d * d).sum(axis=-1)
        assert (s_int == bound).sum(axis=1).max() == on_boundary and R * R == bound / 64.0
        idx, sq = rn.dense(y, None, R, 16)
        for i in range(len(y)):
            inside = np.nonzero(s_int[i] <= bound)[0]
            order = inside[np.lexsort((inside, s_int[i, inside]))][:16]
            assert np.array_equal(idx[i, :len(order)], order) and np.array_equal(sq[i, :len(order)], s_int[i, order] / 64.0)
            assert np.all(idx[i, len(order):] == -1)


def test_finish_rule():
    """The end-of-row rule: self dropped where it is, else the last; short lists padded."""
    assert same(rn.finish([0.0, 1.0, 2.0], [5, 7, 9], 2, True, 7), (np.array([5, 9]), np.array([0.0, 2.0])))
    assert same(rn.finish([0.0, 0.0, 0.0], [1, 2, 3], 2, True, 7), (np.array([1, 2]), np.array([0.0, 0.0])))
    assert same(rn.finish([0.0], [7], 2, True, 7), (np.array([-1, -1]), np.array([np.inf, np.inf])))
    assert same(rn.finish([0.5], [4], 3, False, 0), (np.array([4, -1, -1]), np.array([0.5, np.inf, np.inf])))


def test_non_finite_rows():
    y = np.array([[0.0, 0.0], [0.1, 0.0], [np.nan, 0.0], [np.inf, 0.0]])
    x = np.array([[0.0, 0.0], [np.nan, 0.0], [-np.inf, 0.0]])
    for f in (rn.dense, rn.walk):
        idx, sq = f(y, x, 0.5, 3)
        assert np.array_equal(idx, [[0, 1, -1], [-1, -1, -1], [-1, -1, -1]])
        assert np.array_equal(sq[0], [0.0, 0.1 * 0.1, np.inf]) and np.all(np.isnan(sq[1])) and np.all(np.isposinf(sq[2]))
        idx, sq = f(np.zeros((0, 2)), x, 0.5, 2)
        assert np.all(idx == -1) and np.all(np.isposinf(sq))


def test_a_walk_order_tie_rule_disagrees_on_both_lattices():
    """The brute-force kernels' insertion (strict s < s_t, ties left to the order of arrival) applied in walk order is NOT
    the answer: on both lattices, at every factor, rows differ from dense() for K = 4 and K = 16 -- the cell list meets a
    source with a larger index in an earlier row of cells first.  If a lattice is ever changed so that this stops being
    true, the tie tests of the radius search have lost their teeth."""
    for name in ("lattice", "lattice3"):
        y, x, R = rn.cloud(name, np.float32)
        for K in (4, 16):
            want = rn.dense(y, x, R, K)
            for factor in rn.FACTORS:
                got = rn.walk(y, x, R, K, factor=factor, tie="walk")
                rows = int((got[0] != want[0]).any(axis=1).sum())
                assert np.array_equal(got[1], want[1])      # the same distances: only the choice among ties differs
                assert rows > 0, (name, K, factor)
