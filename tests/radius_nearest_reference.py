"""float64 restatement of the radius search (include/kmvp.h kmvp_radius_nearest) -- TEST INFRASTRUCTURE ONLY.

finish()     the end-of-row rule on a sorted candidate list: K entries, or K + 1 with the row's own index dropped if it is
             there and the last one otherwise; (-1, +inf) where the list is short
dense()      brute force: all N x M squared distances, the inside ones sorted by (s, index) with numpy's lexsort
walk()       the way the kernel forms a row: tile by tile over the runs of cutoff_reference.plan(), every inside record
             inserted IN WALK ORDER into a list of K (+ 1) entries -- under the lexicographic rule (tie="index": an entry
             moves down when s < s_t or s == s_t and j < j_t), or under the brute-force kernels' strict s < s_t
             (tie="walk"), which is only right when the sources are met in ascending index
Everything is float64: the inside test is s <= R R on the float64 squared distance of the given coordinates."""
import bisect

import numpy as np

import cutoff_reference as cr

CLOUDS = cr.CLOUDS + ("lattice", "lattice3")
FACTORS = (1.0, 1.5, 2.0)


def cloud(name, precision):
    """cutoff_reference's clouds and lattice3: 8 x 8 x 8 points at spacing 1/8 with R = 3/8, targets = sources.  Every
    squared distance is an integer / 64, and 30 pairs of an inner point sit exactly ON the boundary (s = 9 / 64)."""
    if name != "lattice3":
        return cr.cloud(name, precision)
    a, b, c = np.meshgrid(np.arange(8) / 8.0, np.arange(8) / 8.0, np.arange(8) / 8.0, indexing="ij")
    y = np.stack([a.ravel(), b.ravel(), c.ravel()], axis=1)
    return np.asarray(y, dtype=precision).astype(np.float64), None, 3.0 / 8.0


def finish(s, j, K, exclude_self, self_index):
    """s, j: the row's sorted candidates, at most K + bool(exclude_self) of them.  (idx (K,), sqdist (K,))."""
    s, j = list(s), list(j)
    kc = K + bool(exclude_self)
    assert len(s) <= kc
    s += [np.inf] * (kc - len(s))
    j += [-1] * (kc - len(j))
    if exclude_self:
        at = j.index(self_index) if self_index in j else kc - 1
        del s[at], j[at]
    return np.array(j, dtype=np.int64), np.array(s, dtype=np.float64)


def _rows(N, K):
    return np.full((N, K), -1, dtype=np.int64), np.full((N, K), np.inf)


def dense(y, x, R, K, exclude_self=False):
    """(idx (N, K) int64, sqdist (N, K) float64) by brute force.  A NaN target row is (-1, NaN) where there is a source."""
    y = np.asarray(y, dtype=np.float64)
    xx = y if x is None else np.asarray(x, dtype=np.float64)
    s = cr.sqdists(xx, y)
    idx, sq = _rows(len(xx), K)
    kc = K + bool(exclude_self)
    for i in range(len(xx)):
        with np.errstate(invalid="ignore"):
            inside = np.nonzero(s[i] <= R * R)[0]
        order = inside[np.lexsort((inside, s[i, inside]))][:kc]
        idx[i], sq[i] = finish(s[i, order], order, K, exclude_self, i)
    if len(y):
        sq[np.isnan(xx).any(axis=1)] = np.nan
    return idx, sq


def walk(y, x, R, K, exclude_self=False, factor=1.0, p=None, tie="index"):
    """The same rows the way the kernel forms them (see the module's head)."""
    y = np.asarray(y, dtype=np.float64)
    xx = y if x is None else np.asarray(x, dtype=np.float64)
    p = cr.plan(y, xx, R, factor) if p is None else p
    idx, sq = _rows(len(xx), K)
    kc = K + bool(exclude_self)
    for t, (run0, nruns, live) in enumerate(p["tiles"]):
        if live == 0:
            continue
        rows = p["tmap"][t * cr.TILE:t * cr.TILE + live]
        rec = np.concatenate([np.arange(r0, r0 + n) for r0, n in p["runs"][run0:run0 + nruns]] + [np.zeros(0, dtype=np.int64)])
        js = p["smap"][rec.astype(np.int64)]
        js = js[js >= 0]                                   # pad records sit at +inf: never inside
        s = cr.sqdists(xx[rows], y[js])
        for lane, i in enumerate(rows):
            keys, lst = [], []                             # the list: (s, j) pairs, and their s alone
            with np.errstate(invalid="ignore"):
                inside = np.nonzero(s[lane] <= R * R)[0]
            for c in inside:                               # in walk order
                cand = (float(s[lane, c]), int(js[c]))
                at = bisect.bisect_left(lst, cand) if tie == "index" else bisect.bisect_right(keys, cand[0])
                lst.insert(at, cand)
                keys.insert(at, cand[0])
                del lst[kc:], keys[kc:]
            idx[i], sq[i] = finish(keys, [c[1] for c in lst], K, exclude_self, int(i))
    if len(y):
        sq[np.isnan(xx).any(axis=1)] = np.nan
    return idx, sq


def masked_nearest(idx, sq, r2):
    """kmvp_nearest's rows with every entry whose sqdist > r2 replaced by (-1, +inf): the contract's right-hand side."""
    with np.errstate(invalid="ignore"):
        out = sq > r2
    return np.where(out, -1, idx), np.where(out, np.inf, sq)
