"""float64 numpy restatement of the K-nearest-neighbour reduction (include/kmvp.h kmvp_nearest), from the definition:

    s[i, j] = sum_d (x[i, d] - y[j, d])^2

A source qualifies for a target when s is finite in the working precision (a NaN coordinate and an overflowed squared
distance never do).  Of the qualifying sources the K smallest under the order (s, j) are returned, nearest first -- a
STABLE sort, so equal distances come in ascending index.  Indices are global (j_offset + position in y).  Where fewer than
K sources qualify the tail is (-1, +inf); a target with a NaN coordinate has (-1, NaN) in all K entries.  exclude_self
leaves the source whose global index equals the target's index out of that row."""
import numpy as np


def sqdists(x, y):
    """(N, M) float64 squared distances from the definition (no expansion: exact on small-integer lattices)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        diff = x[:, None, :] - y[None, :, :]
        return np.sum(diff * diff, axis=-1)


def nearest(x, y, K, exclude_self=False, j_offset=0, precision=np.float64):
    """(idx (N, K) int64, sqdist (N, K) float64).  precision: the working precision whose range decides whether a squared
    distance is finite (float32: s beyond 3.4e38 has overflowed there)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    N, M = x.shape[0], y.shape[0]
    s = sqdists(x, y) if M else np.zeros((N, 0))
    with np.errstate(invalid="ignore"):
        live = np.isfinite(s) & (s <= float(np.finfo(precision).max))
    key = np.where(live, s, np.inf)
    if exclude_self:
        rows = np.arange(N) - j_offset
        ok = (rows >= 0) & (rows < M)
        key[np.nonzero(ok)[0], rows[ok]] = np.inf
        live[np.nonzero(ok)[0], rows[ok]] = False
    order = np.argsort(key, axis=1, kind="stable")[:, :K]   # ties: the smaller index first
    idx = np.full((N, K), -1, dtype=np.int64)
    sq = np.full((N, K), np.inf)
    if M:
        took = np.take_along_axis(live, order, axis=1)
        k = order.shape[1]
        idx[:, :k] = np.where(took, order + j_offset, -1)
        sq[:, :k] = np.where(took, np.take_along_axis(s, order, axis=1), np.inf)
    nan_rows = np.isnan(x).any(axis=1)
    idx[nan_rows] = -1
    sq[nan_rows] = np.nan
    return idx, sq


def merge_shards(results, K):
    """What a caller does with partial shards: the K smallest of the shards' (sqdist, idx) pairs per row."""
    idx = np.concatenate([r[0] for r in results], axis=1)
    sq = np.concatenate([r[1] for r in results], axis=1)
    order = np.lexsort((np.where(idx < 0, np.iinfo(np.int64).max, idx), sq), axis=1)[:, :K]
    return np.take_along_axis(idx, order, axis=1), np.take_along_axis(sq, order, axis=1)


def lattice(rs, n, D):
    """n points with integer coordinates in 0 .. 15: exact in float16, float32 and float64, every difference, square and
    sum exact (s <= 8 * 225), ties by the thousand."""
    return rs.randint(0, 16, size=(n, D)).astype(np.float64)
