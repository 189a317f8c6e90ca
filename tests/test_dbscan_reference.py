"""The test infrastructure of DBSCAN (tests/dbscan_reference.py) held to scikit-learn, and what tests/test_gpu_dbscan.py
takes for granted about the named clouds, asserted without a GPU.

sklearn.cluster.DBSCAN agrees with the canonical definition on everything that does not depend on its traversal order: the
core points, the labels of the core points (it numbers clusters in the order it meets their first core point, which is the
ascending order of the clusters' smallest core indices) and the noise set.  A border point with core neighbours in two
clusters goes to whichever cluster sklearn reaches first; the reference sends it to its nearest core point."""
import numpy as np
import pytest

import dbscan_reference as dr

NAMES = list(dr.CLOUDS)
_cache = {}


def solved(name):
    if name not in _cache:
        x, R, min_samples = dr.cloud(name)
        inside, s = dr.inside_dense(x, R)
        _cache[name] = (x, R, min_samples, inside, s, dr.dbscan(inside, s, min_samples))
    return _cache[name]


@pytest.mark.parametrize("name", NAMES)
def test_equals_sklearn_on_cores_core_labels_and_noise(name):
    cluster = pytest.importorskip("sklearn.cluster")
    x, R, min_samples, inside, s, (labels, core_of, counts) = solved(name)
    sk = cluster.DBSCAN(eps=R, min_samples=min_samples, algorithm="brute").fit(x)
    core = core_of == np.arange(len(x))
    assert np.array_equal(sk.core_sample_indices_, np.flatnonzero(core))
    assert np.array_equal(sk.labels_[core], labels[core])
    assert np.array_equal(sk.labels_ == -1, labels == -1)
    torn = dr.torn_borders(inside, labels, core_of)
    differ = np.flatnonzero(sk.labels_ != labels)
    assert set(differ.tolist()) <= set(torn.tolist())  # sklearn may differ only where a border point had a choice
    print(f"{name}: {len(torn)} border points with core neighbours in two clusters, sklearn differs on {len(differ)}")


@pytest.mark.parametrize("name", NAMES)
def test_border_points_join_the_cluster_of_an_inside_core_point(name):
    x, R, min_samples, inside, s, (labels, core_of, counts) = solved(name)
    core = core_of == np.arange(len(x))
    assert np.array_equal(core, counts >= min_samples) and np.array_equal(counts, inside.sum(axis=1))
    border = np.flatnonzero((core_of >= 0) & ~core)
    for i in border:
        j = core_of[i]
        assert core[j] and inside[i, j] and labels[i] == labels[j]
        cand = np.flatnonzero(inside[i] & core)
        assert s[i, j] == s[i, cand].min()
    noise = np.flatnonzero(core_of < 0)
    assert np.all(labels[noise] == -1) and not np.any(inside[noise][:, core])
    # the numbering: cluster c's smallest core index grows with c
    firsts = [np.flatnonzero(core & (labels == c))[0] for c in range(labels.max() + 1)]
    assert firsts == sorted(firsts) and all(core_of[f] == f for f in firsts)


@pytest.mark.parametrize("name", NAMES)
def test_named_clouds_are_unambiguous_and_first_seed(name):
    """No pair within 4 gamma of the boundary and no border point with its two nearest core points within 4 gamma, in
    float32 (and so in float64): the float64 inside set and border choice are the working precision's.  The seed is the
    first from 0 upward with that property, three clusters or more, noise and border points."""
    D, N, R, min_samples, seed = dr.CLOUDS[name]
    for earlier in range(seed + 1):
        x = dr.make_cloud(D, N, earlier, name == "uniform3")
        clear = len(dr.ambiguous(x, R, np.float32)) == 0 and len(dr.ambiguous_borders(x, R, min_samples, np.float32)) == 0
        inside, s = dr.inside_dense(x, R)
        info = dr.summary(*dr.dbscan(inside, s, min_samples)[:2])
        good = clear and info["n_clusters"] >= 3 and info["n_noise"] > 0 and info["n_border"] > 0
        assert good == (earlier == seed), (name, earlier, clear, info)
    assert len(dr.ambiguous(x, R, np.float64)) == 0 and N % 64 != 0
    assert np.array_equal(x, x.astype(np.float32).astype(np.float64))


def test_ambiguous_finds_a_planted_pair():
    x = np.array([[0.0, 0.0], [0.5, 0.0], [0.0, 0.5 * (1 + 1e-7)], [3.0, 3.0]])
    assert dr.ambiguous(x, 0.5, np.float32).tolist() == [[0, 1], [0, 2]]
    assert dr.ambiguous(x, 0.5, np.float64).tolist() == [[0, 1]]


def test_some_cloud_has_border_points_with_a_choice():
    x, R, min_samples, inside, s, (labels, core_of, counts) = solved("uniform3")
    assert len(dr.torn_borders(inside, labels, core_of)) > 0 and counts.max() <= 16


@pytest.mark.parametrize("name", dr.LATTICES)
def test_lattices_have_boundary_pairs_clusters_borders_and_noise(name):
    k, x, R, r2, min_samples = dr.lattice(name)
    inside, s = dr.inside_lattice(k, r2)
    labels, core_of, counts = dr.dbscan(inside, s, min_samples)
    info = dr.summary(labels, core_of)
    assert info["n_clusters"] >= 2 and info["n_border"] > 0 and info["n_noise"] > 0, info
    assert np.any(s == r2) and np.any(counts == min_samples)  # pairs on the boundary decide who is a core point
    # the float64 builder agrees: k / 8 and R R = r2 / 64 are exact
    inside64, _ = dr.inside_dense(x, R)
    assert np.array_equal(inside64, inside) and float(R * R) == r2 / 64.0


def test_the_three_builders_agree():
    x, R, min_samples, inside, s, want = solved("uniform3")
    K = int(inside.sum(axis=1).max())
    order = np.argsort(np.where(inside, s, np.inf), axis=1, kind="stable")[:, :K]
    found = np.take_along_axis(inside, order, axis=1)
    idx, sq = np.where(found, order, -1), np.where(found, np.take_along_axis(s, order, axis=1), np.inf)
    inside_l, s_l = dr.inside_lists(idx, sq)
    assert np.array_equal(inside_l, inside)
    got = dr.dbscan(inside_l, s_l, min_samples)
    assert all(np.array_equal(g, w) for g, w in zip(got, want))


def test_chains():
    for order in ("ascending", "descending", "random"):
        x, R = dr.chain(order, n=256)
        inside, s = dr.inside_dense(x, R)
        labels, core_of, counts = dr.dbscan(inside, s, 3)
        assert np.all(labels == 0) and sorted(counts.tolist())[:3] == [2, 2, 3] and len(dr.ambiguous(x, R, np.float32)) == 0
