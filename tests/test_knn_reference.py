"""The restatement of the K-nearest-neighbour reduction (knn_reference.py) against an independent Python double loop on
tiny clouds: ties, duplicates, K beyond the number of sources, NaN and out-of-range sources, a NaN target, exclude_self
and j_offset."""
import math

import numpy as np
import pytest

import knn_reference as kn


def loop_nearest(x, y, K, exclude_self=False, j_offset=0, s_max=float("inf")):
    idx, sq = [], []
    for i, xi in enumerate(x):
        if any(math.isnan(v) for v in xi):
            idx.append([-1] * K)
            sq.append([float("nan")] * K)
            continue
        cand = []
        for j, yj in enumerate(y):
            s = 0.0
            for a, b in zip(xi, yj):
                s += (a - b) * (a - b)
            if math.isnan(s) or math.isinf(s) or s > s_max:
                continue
            if exclude_self and j + j_offset == i:
                continue
            cand.append((s, j + j_offset))
        cand.sort()  # lexicographic on (s, j)
        cand = cand[:K] + [(float("inf"), -1)] * (K - len(cand[:K]))
        idx.append([c[1] for c in cand])
        sq.append([c[0] for c in cand])
    return np.array(idx, dtype=np.int64).reshape(len(x), K), np.array(sq, dtype=np.float64).reshape(len(x), K)


def same(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1], equal_nan=True)


@pytest.mark.parametrize("K", [1, 3, 5, 16])
@pytest.mark.parametrize("D", [1, 3])
def test_lattice_with_ties(D, K):
    rs = np.random.RandomState(10 * D + K)
    x, y = kn.lattice(rs, 9, D), kn.lattice(rs, 13, D)
    y[5] = y[2]  # duplicates
    y[7] = y[2]
    assert same(kn.nearest(x, y, K), loop_nearest(x.tolist(), y.tolist(), K))


@pytest.mark.parametrize("K", [1, 4])
def test_continuous(K):
    rs = np.random.RandomState(K)
    x, y = rs.randn(7, 3), rs.randn(11, 3)
    assert same(kn.nearest(x, y, K), loop_nearest(x.tolist(), y.tolist(), K))


def test_tail_when_fewer_sources_than_K_and_no_source():
    rs = np.random.RandomState(3)
    x, y = kn.lattice(rs, 4, 2), kn.lattice(rs, 3, 2)
    idx, sq = kn.nearest(x, y, 5)
    assert same((idx, sq), loop_nearest(x.tolist(), y.tolist(), 5))
    assert np.all(idx[:, 3:] == -1) and np.all(np.isinf(sq[:, 3:])) and np.all(idx[:, :3] >= 0)
    idx, sq = kn.nearest(x, np.zeros((0, 2)), 2)
    assert np.all(idx == -1) and np.all(np.isposinf(sq)) and idx.shape == (4, 2)
    idx, sq = kn.nearest(np.zeros((0, 2)), y, 2)
    assert idx.shape == (0, 2) and sq.shape == (0, 2)


def test_disqualified_sources_and_nan_target():
    rs = np.random.RandomState(4)
    x, y = kn.lattice(rs, 5, 3), kn.lattice(rs, 8, 3)
    y[1, 0] = np.nan
    y[6] = 3.0e38  # s ~ 2.7e77: finite in float64, overflowed in float32
    x[2, 1] = np.nan
    got64 = kn.nearest(x, y, 8)
    assert same(got64, loop_nearest(x.tolist(), y.tolist(), 8))
    got32 = kn.nearest(x, y, 8, precision=np.float32)
    assert same(got32, loop_nearest(x.tolist(), y.tolist(), 8, s_max=float(np.finfo(np.float32).max)))
    assert not np.any(got64[0] == 1) and np.any(got64[0] == 6) and not np.any(got32[0] == 6) and not np.any(got32[0] == 1)
    assert np.all(got32[0][2] == -1) and np.all(np.isnan(got32[1][2])) and not np.isnan(got32[1][[0, 1, 3, 4]]).any()


@pytest.mark.parametrize("K", [1, 3, 15])
def test_exclude_self_with_duplicates(K):
    rs = np.random.RandomState(5)
    x = kn.lattice(rs, 24, 2)
    x[3:21] = x[3]  # 18 copies of one point: more than K + 1 for every K here
    got = kn.nearest(x, x, K, exclude_self=True)
    assert same(got, loop_nearest(x.tolist(), x.tolist(), K, exclude_self=True))
    assert not np.any(got[0] == np.arange(24)[:, None])
    # the duplicates see each other at distance 0, smallest indices first
    assert np.array_equal(got[0][20, : min(K, 17)], np.arange(3, 3 + min(K, 17))) and got[1][20, 0] == 0.0


def test_j_offset_and_shard_merge():
    rs = np.random.RandomState(6)
    x = kn.lattice(rs, 10, 3)
    whole = kn.nearest(x, x, 4, exclude_self=True)
    parts = [kn.nearest(x, x[lo:hi], 4, exclude_self=True, j_offset=lo) for lo, hi in ((0, 3), (3, 3), (3, 10))]
    assert same(parts[0], loop_nearest(x.tolist(), x[:3].tolist(), 4, exclude_self=True))
    assert same(parts[2], loop_nearest(x.tolist(), x[3:].tolist(), 4, exclude_self=True, j_offset=3))
    assert same(kn.merge_shards(parts, 4), whole)
