"""The numpy restatement of Lloyd's k-means (kmeans_reference.py) against a textbook loop written from the definition, and
against the properties the definition implies: inertia that never increases, duplicated points that count as integer
weights, the empty-cluster rule and the tie rule."""
import numpy as np
import pytest

import kmeans_reference as kr
import knn_reference as kn


def textbook(x, c0, w, maxit):
    """Lloyd's iteration with Python loops: every distance from the definition, the first smallest wins, means point by
    point in index order; stops at the first iteration that moves no centroid."""
    c = np.array(c0, dtype=np.float64)
    N, C = len(x), len(c)
    for k in range(1, maxit + 1):
        labels = np.empty(N, dtype=np.int64)
        inertia = 0.0
        for i in range(N):
            best, arg = np.inf, -1
            for j in range(C):
                s = float(np.sum((x[i] - c[j]) ** 2))
                if s < best:
                    best, arg = s, j
            labels[i] = arg
            inertia += w[i] * best
        new = c.copy()
        weight = np.zeros(C)
        for j in range(C):
            acc = np.zeros(x.shape[1])
            for i in range(N):
                if labels[i] == j:
                    acc += w[i] * x[i]
                    weight[j] += w[i]
            if weight[j] > 0:
                new[j] = acc / weight[j]
        moved = float(np.sum((new - c) ** 2))
        c = new
        if moved == 0.0:
            return c, labels, weight, k, inertia, True
    return c, labels, weight, maxit, inertia, False


@pytest.mark.parametrize("D", [1, 2, 5])
@pytest.mark.parametrize("weighted", [False, True])
def test_equals_a_textbook_loop(D, weighted):
    rs = np.random.RandomState(10 * D + weighted)
    x = rs.rand(120, D)
    w = rs.randint(0, 4, size=120).astype(np.float64) if weighted else np.ones(120)
    got = kr.kmeans(x, x[:6], w, tol=0.0, maxit=200)
    c, labels, weight, k, inertia, done = textbook(x, x[:6], w, 200)
    assert done and got["converged"] and got["shift"] == 0.0 and got["iterations"] == k
    assert np.array_equal(got["labels"], labels) and np.array_equal(got["cluster_weight"], weight)
    assert np.allclose(got["centroids"], c, rtol=0, atol=1e-13) and abs(got["inertia"] - inertia) <= 1e-12 * inertia
    assert got["min_gap"] > 1e-9  # (the comparison of labels above was a fair one)


@pytest.mark.parametrize("seed", range(4))
def test_inertia_never_increases(seed):
    rs = np.random.RandomState(seed)
    x = rs.randn(400, 3)
    out = kr.kmeans(x, x[:9], tol=0.0, maxit=300)
    inertias = np.array(out["inertias"])
    assert out["converged"] and out["iterations"] > 3
    assert np.all(np.diff(inertias) <= 1e-12 * inertias[:-1])
    assert out["shifts"][-1] == 0.0 and all(s > 0 for s in out["shifts"][:-1])


def test_duplicates_are_integer_weights():
    rs = np.random.RandomState(5)
    x = rs.rand(150, 2)
    reps = rs.randint(1, 4, size=150)
    dup = np.repeat(x, reps, axis=0)
    a = kr.kmeans(x, x[:5], reps.astype(np.float64), tol=0.0, maxit=200)
    b = kr.kmeans(dup, x[:5], None, tol=0.0, maxit=200)
    assert a["converged"] and b["converged"] and a["iterations"] == b["iterations"]
    assert np.array_equal(np.repeat(a["labels"], reps), b["labels"])
    assert np.array_equal(a["cluster_weight"], b["cluster_weight"])
    assert np.allclose(a["centroids"], b["centroids"], rtol=0, atol=1e-13)
    assert abs(a["inertia"] - b["inertia"]) <= 1e-12 * a["inertia"]


def test_empty_cluster_and_ties():
    """Two identical initial centroids: in the iteration that sees them every tie goes to the smaller index, the larger
    one stays empty and in place (afterwards the smaller one has moved and they are two centroids like any other); a
    centroid far away stays empty and in place to the end; a cluster whose points all weigh 0 keeps its position, too."""
    rs = np.random.RandomState(2)
    x = kn.lattice(rs, 200, 2)
    c0 = np.array([[3.0, 3.0], [3.0, 3.0], [12.0, 12.0], [100.0, 100.0]])
    one = kr.kmeans(x, c0, tol=0.0, maxit=1)
    assert np.any(one["labels"] == 0) and not np.any(one["labels"] == 1) and not np.any(one["labels"] == 3)
    assert np.array_equal(one["centroids"][1], c0[1]) and one["cluster_weight"][1] == 0
    out = kr.kmeans(x, c0, tol=0.0, maxit=100)
    assert out["converged"] and not np.any(out["labels"] == 3)
    assert np.array_equal(out["centroids"][3], c0[3])
    assert out["cluster_weight"][3] == 0 and out["cluster_weight"].sum() == 200
    # equidistant on the lattice: point (5, 5) between centroids (3, 5) and (7, 5)
    tie = kr.kmeans(np.array([[5.0, 5.0]]), np.array([[7.0, 5.0], [3.0, 5.0]]), tol=0.0, maxit=1)
    assert tie["labels"][0] == 0
    w = np.ones(200)
    far = x[:, 0] >= 8
    w[far] = 0.0
    c1 = np.array([[3.0, 8.0], [12.0, 8.0]])
    zero = kr.kmeans(x, c1, w, tol=0.0, maxit=1)
    assert np.any(zero["labels"] == 1) and zero["cluster_weight"][1] == 0 and np.array_equal(zero["centroids"][1], c1[1])


def test_stopping_rules():
    rs = np.random.RandomState(9)
    x = rs.rand(300, 2)
    full = kr.kmeans(x, x[:7], tol=0.0, maxit=300)
    assert full["converged"] and full["iterations"] > 4
    cut = kr.kmeans(x, x[:7], tol=0.0, maxit=3)
    assert not cut["converged"] and cut["stop"] == kr.MAXIT and cut["iterations"] == 3 and cut["shift"] == full["shifts"][2]
    tol = float(np.sqrt(full["shifts"][1] * full["shifts"][2]))  # between the second and the third shift
    loose = kr.kmeans(x, x[:7], tol=tol, maxit=300)
    first = next(k for k, s in enumerate(full["shifts"], 1) if s <= tol)
    assert loose["converged"] and loose["iterations"] == first
    # chaining: maxit = 1 three times walks through the same states
    c = x[:7]
    for k in range(3):
        one = kr.kmeans(x, c, tol=0.0, maxit=1)
        c = one["centroids"]
    assert np.array_equal(c, cut["centroids"]) and np.array_equal(one["labels"], cut["labels"])
    # a NaN point: label -1, the solve ends, the other rows keep valid labels
    bad = x.copy()
    bad[17, 1] = np.nan
    out = kr.kmeans(bad, x[:7], tol=0.0, maxit=300)
    assert out["stop"] == kr.NONFINITE and out["iterations"] == 1 and out["labels"][17] == -1
    assert np.all(np.delete(out["labels"], 17) >= 0) and np.all(np.isfinite(out["centroids"]))
