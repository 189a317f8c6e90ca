"""The canonical DBSCAN of include/kmvp.h kmvp_dbscan from a given inside set -- TEST INFRASTRUCTURE ONLY.

dbscan(inside, s, min_samples)   union-find over the inside pairs of core points; a cluster's root is its smallest core
                                 index, clusters are numbered in ascending order of their roots; a point that is no core
                                 point joins the cluster of its nearest inside core point, the minimum of (s, index);
                                 everything else is noise, -1.
The inside set (N x N bool) and the values s that order a border point's candidates come from one of three builders:
  inside_dense(x, R)        s <= R R on the float64 squared distances of the given coordinates (a NaN s is outside)
  inside_lattice(k, r2)     integer arithmetic: k (N, D) integer coordinates, r2 the squared radius in the same units
  inside_lists(idx, sq)     neighbour lists, (N, K) indices with -1 for an empty entry and their squared distances
The named clouds of the GPU tests and ambiguous(), the pairs a working precision might decide differently from float64,
are here too, so that tests/test_dbscan_reference.py can assert without a GPU what tests/test_gpu_dbscan.py relies on."""
import numpy as np

import cutoff_reference as cr


# ---- the inside sets ----------------------------------------------------------------------------------------------------
def inside_dense(x, R):
    x = np.asarray(x, dtype=np.float64)
    s = cr.sqdists(x, x)
    with np.errstate(invalid="ignore"):
        return s <= R * R, s


def inside_lattice(k, r2):
    k = np.asarray(k)
    assert np.issubdtype(k.dtype, np.integer)
    d = k[:, None, :].astype(np.int64) - k[None, :, :].astype(np.int64)
    s = np.sum(d * d, axis=-1)
    return s <= int(r2), s


def inside_lists(idx, sq):
    N = idx.shape[0]
    inside, s = np.zeros((N, N), dtype=bool), np.full((N, N), np.inf)
    rows = np.repeat(np.arange(N), idx.shape[1])[idx.ravel() >= 0]
    cols = idx.ravel()[idx.ravel() >= 0]
    inside[rows, cols] = True
    s[rows, cols] = sq.ravel()[idx.ravel() >= 0]
    return inside, s


# ---- the definition -----------------------------------------------------------------------------------------------------
def dbscan(inside, s, min_samples, nan_points=None):
    """(labels, core_of, counts), three (N,) int64 arrays.  nan_points: a bool mask of the points whose count is -1 (a NaN
    coordinate: no pair of such a point is inside, itself included)."""
    N = inside.shape[0]
    assert inside.shape == (N, N) and np.array_equal(inside, inside.T), "the graph is undirected"
    counts = inside.sum(axis=1).astype(np.int64)
    if nan_points is not None:
        assert not inside[nan_points].any()
        counts[nan_points] = -1
    core = counts >= min_samples
    parent = np.arange(N)

    def find(a):
        r = a
        while parent[r] != r:
            r = parent[r]
        while parent[a] != r:
            parent[a], a = r, parent[a]
        return r

    ii, jj = np.nonzero(np.triu(inside & core[:, None] & core[None, :], 1))
    for a, b in zip(ii.tolist(), jj.tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)  # the root is the smallest index of the component
    root = np.array([find(i) for i in range(N)])
    core_of = np.where(core, np.arange(N), -1).astype(np.int64)
    for i in np.flatnonzero(~core):
        cand = np.flatnonzero(inside[i] & core)
        if cand.size:
            core_of[i] = cand[np.lexsort((cand, s[i, cand]))[0]]
    roots = np.unique(root[core])  # ascending
    labels = np.full(N, -1, dtype=np.int64)
    has = core_of >= 0
    labels[has] = np.searchsorted(roots, root[core_of[has]])
    return labels, core_of, counts


def summary(labels, core_of):
    """The info words a result implies: n_clusters, n_core, n_border, n_noise."""
    N = len(labels)
    core = core_of == np.arange(N)
    return dict(n_clusters=int(labels.max() + 1) if N else 0, n_core=int(core.sum()),
                n_border=int(((core_of >= 0) & ~core).sum()), n_noise=int((core_of < 0).sum()))


def torn_borders(inside, labels, core_of):
    """The border points with inside core points in more than one cluster: where a rule has to choose."""
    N = len(labels)
    core = core_of == np.arange(N)
    out = []
    for i in np.flatnonzero((core_of >= 0) & ~core):
        if len(np.unique(labels[np.flatnonzero(inside[i] & core)])) > 1:
            out.append(i)
    return np.array(out, dtype=np.int64)


# ---- the pairs a working precision may decide differently ---------------------------------------------------------------
def unit_roundoff(precision):
    return 2.0 ** -53 if np.dtype(precision) == np.float64 else 2.0 ** -24


def ambiguous(x, R, precision):
    """The pairs (i, j), i < j, with |s64 / R^2 - 1| <= 4 gamma, gamma = (D + 3) u the bound of tests/test_gpu_knn.py on the
    working precision's s.  s and r2 = (real)(R R) each carry at most gamma: 4 gamma is a factor 2 over their sum."""
    x = np.asarray(x, dtype=np.float64)
    gamma = (x.shape[1] + 3) * unit_roundoff(precision)
    s = cr.sqdists(x, x)
    with np.errstate(invalid="ignore"):
        near = np.abs(s / (R * R) - 1.0) <= 4 * gamma
    return np.argwhere(np.triu(near, 1))


def ambiguous_borders(x, R, min_samples, precision):
    """The points that are no core points whose two nearest inside core points are within 4 gamma of each other in s
    (relative): where the working precision's order of the candidates may differ from float64's."""
    x = np.asarray(x, dtype=np.float64)
    gamma = (x.shape[1] + 3) * unit_roundoff(precision)
    inside, s = inside_dense(x, R)
    core = inside.sum(axis=1) >= min_samples
    out = []
    for i in np.flatnonzero(~core):
        c = np.sort(s[i, inside[i] & core])
        if len(c) >= 2 and c[1] - c[0] <= 4 * gamma * c[1]:
            out.append(i)
    return np.array(out, dtype=np.int64)


# ---- the named clouds ---------------------------------------------------------------------------------------------------
# name: (D, N, R, min_samples, seed).  Coordinates are rounded to float32, so one cloud serves both precisions; the seed is
# the first from 0 upward at which no pair is ambiguous in float32 (hence none in float64) and the cloud has three clusters
# or more, noise and border points: tests/test_dbscan_reference.py asserts all of it.
CLOUDS = {
    "blobs1": (1, 2501, 0.004, 8, 0),
    "blobs2": (2, 2503, 0.03, 8, 0),
    "blobs3": (3, 2497, 0.06, 8, 0),
    "uniform3": (3, 3000, 0.07, 4, 0),
}
BLOBS = ("blobs1", "blobs2", "blobs3")


def make_cloud(D, N, seed, uniform):
    rs = np.random.RandomState(seed)
    if uniform:
        x = rs.rand(N, D)
    else:  # five blobs of different widths on 70 % of the points, uniform noise on the rest
        nb = int(0.7 * N)
        centres = rs.rand(5, D)
        width = 0.01 + 0.03 * rs.rand(5)
        which = rs.randint(0, 5, size=nb)
        x = np.concatenate([centres[which] + width[which, None] * rs.randn(nb, D), rs.rand(N - nb, D)])
        x = x[rs.permutation(N)]
    return x.astype(np.float32).astype(np.float64)


def cloud(name):
    """(x (N, D) float64 of float32-representable coordinates, R, min_samples)."""
    D, N, R, min_samples, seed = CLOUDS[name]
    return make_cloud(D, N, seed, name == "uniform3"), R, min_samples


def lattice(name):
    """(k integer coordinates, x = k / 8, R, r2 in lattice units, min_samples): lattices at spacing 1 / 8 like
    radius_nearest_reference's, with pairs exactly ON the boundary (25 = 3^2 + 4^2 = 5^2 in the plane, 9 = 3^2 = 1 + 4 + 4 in
    space), thinned to 95 % near a few centres and to 12 % elsewhere: several clusters, border points and noise."""
    rs = np.random.RandomState(7)
    if name == "lattice":  # 32 x 32, R = 5 / 8
        a, b = np.meshgrid(np.arange(32), np.arange(32), indexing="ij")
        k, r2, min_samples = np.stack([a.ravel(), b.ravel()], axis=1), 25, 50
        centres, reach = np.array([[6, 6], [6, 25], [24, 8], [23, 24], [15, 16]]), 5.0
    elif name == "lattice3":  # 12 x 12 x 12, R = 3 / 8
        a, b, c = np.meshgrid(np.arange(12), np.arange(12), np.arange(12), indexing="ij")
        k, r2, min_samples = np.stack([a.ravel(), b.ravel(), c.ravel()], axis=1), 9, 60
        centres, reach = np.array([[3, 3, 3], [8, 8, 3], [3, 8, 8], [9, 3, 9]]), 3.0
    else:
        raise ValueError(name)
    near = np.min(np.sum((k[:, None, :] - centres[None, :, :]) ** 2, axis=-1), axis=1) <= reach * reach
    k = k[rs.rand(len(k)) < np.where(near, 0.95, 0.12)]
    k = k[rs.permutation(len(k))]
    return k, k / 8.0, np.sqrt(r2) / 8.0, r2, min_samples


LATTICES = ("lattice", "lattice3")


def chain(order, n=4096, seed=0):
    """(x (n, 1), R): n points on a line at spacing 1 / 128 = 0.75 R, R = 1 / 96, in ascending, descending or random index
    order.  Only the two neighbours on the line are inside (s = 0.5625 R^2, the next 2.25 R^2: far from the boundary)."""
    h = 1.0 / 128.0
    pos = np.arange(n) * h
    if order == "descending":
        pos = pos[::-1]
    elif order == "random":
        pos = pos[np.random.RandomState(seed).permutation(n)]
    elif order != "ascending":
        raise ValueError(order)
    return np.ascontiguousarray(pos.reshape(n, 1)), h / 0.75
