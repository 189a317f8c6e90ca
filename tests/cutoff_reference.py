"""numpy restatement of the cutoff-radius entries (include/kmvp.h kmvp_<kernel>_cutoff, kmvp_radius_count) -- TEST
INFRASTRUCTURE ONLY.

plan()       the cell list and launch plan of csrc/kmvp_cutoff_plan.hpp, operation by operation in float64, so that the
             header's tables and maps can be compared entry by entry (tests/test_host_cutoff_plan.py)
walk()       the truncated product and the neighbour count as the kernels form them: tile by tile over the plan's runs,
             the inside test on every record walked
dense()      the same two by a dense masked evaluation over all N x M pairs
Everything is float64: the inside test is s <= R R on the float64 squared distance of the given coordinates."""
import numpy as np

TILE, WAVES, RECORDS, MAX_AXIS = 64, 4, 8, 1 << 20
KERNELS = ("gaussian", "absolute-exponential", "matern-3/2", "matern-5/2")


def round_up(v, q):
    return (v + q - 1) // q * q


def kernel_values(kernel, s):
    with np.errstate(all="ignore"):
        if kernel == "gaussian":
            return np.exp(-s)
        if kernel == "absolute-exponential":
            return np.exp(-np.sqrt(s))
        t = np.sqrt(3.0 if kernel == "matern-3/2" else 5.0) * np.sqrt(s)
        p = 1 + t if kernel == "matern-3/2" else 1 + t + t * t / 3
        return np.where(np.isinf(s), 0.0, p * np.exp(-t))


def sqdists(x, y):
    """(n, m) float64 squared distances; NaN where a difference is NaN (inf - inf included)."""
    with np.errstate(all="ignore"):
        d = x[:, None, :] - y[None, :, :]
        return np.sum(d * d, axis=-1)


def _axis_cells(ext, h):
    with np.errstate(all="ignore"):
        q = np.floor(np.float64(ext) / np.float64(h))
    return MAX_AXIS if not (q < MAX_AXIS) else int(q) + 1


def _cells(v, lo, h, g):
    with np.errstate(all="ignore"):
        q = np.floor((v - lo) / h)
    return np.where(~(q > 0), 0, np.where(~(q < g), g - 1, q)).astype(np.int64)


def plan(y, x, R, factor=1.0):
    """The plan of cutoff_plan_build(y, M, x, N, D, R, factor) as a dict: g (3,), lo (3,), h, n_pad, m_pad, m_alloc,
    live_tiles, walked, tiles (T, 3) [run0, nruns, live], runs (Q, 2) [rec0, len], tmap (n_pad,), smap (m_alloc,)."""
    y, x = np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64)
    (M, D), N = y.shape, len(x)
    fy, fx = np.isfinite(y).all(axis=1), np.isfinite(x).all(axis=1)
    pts = np.concatenate([y[fy], x[fx]])
    lo, ext = np.zeros(3), np.zeros(3)
    if len(pts):
        lo[:D] = pts.min(axis=0)
        with np.errstate(all="ignore"):
            ext[:D] = pts.max(axis=0) - lo[:D]
    with np.errstate(all="ignore"):
        h = np.float64(factor) * np.float64(R) * (1.0 + 1.0 / 65536.0)
        for d in range(D):
            if not (ext[d] / h < MAX_AXIS - 1):
                need = ext[d] / np.float64(MAX_AXIS - 1)
                if need > h:
                    h = need
        if not np.isfinite(h):
            h = np.float64(np.inf)
        cap = max(1, 2 * (N + M))
        while True:
            g = [(_axis_cells(ext[d], h) if d < D else 1) for d in range(3)]
            if g[0] * g[1] * g[2] <= cap or not np.isfinite(h):
                break
            h = h * 1.25
        if not np.isfinite(h):
            g = [1, 1, 1]
    g0, g1, g2 = g
    ncells, nrows = g0 * g1 * g2, g1 * g2

    def cell_of(p):
        c = np.zeros(len(p), dtype=np.int64)
        for d in range(D - 1, -1, -1):
            c = c * g[d] + _cells(p[:, d], lo[d], h, g[d])
        return c

    # sources
    sj = np.nonzero(fy)[0]
    sc = cell_of(y[sj])
    count = np.bincount(sc, minlength=ncells).astype(np.int64).reshape(nrows, g0)
    rowlen = round_up(count.sum(axis=1), RECORDS)
    rowstart = np.concatenate([[0], np.cumsum(rowlen)]).astype(np.int64)
    cstart = (rowstart[:-1, None] + np.cumsum(count, axis=1) - count).reshape(-1)
    cend = cstart + count.reshape(-1)
    m_pad = int(rowstart[-1])
    m_alloc = m_pad + RECORDS
    smap = np.full(m_alloc, -1, dtype=np.int64)
    o = np.argsort(sc, kind="stable")
    first = np.cumsum(count.reshape(-1)) - count.reshape(-1)
    smap[cstart[sc[o]] + np.arange(len(o)) - first[sc[o]]] = sj[o]

    # targets
    ti = np.nonzero(fx)[0]
    tc = cell_of(x[ti])
    o = np.argsort(tc, kind="stable")
    ti, tc = ti[o], tc[o]
    tiles, runs, tmap, walked = [], [], [], 0

    def push(idx, run0, nruns):
        tiles.append((run0, nruns, len(idx)))
        tmap.extend(list(idx) + [-1] * (TILE - len(idx)))

    trow = tc // g0
    for r in np.unique(trow):
        sel = np.nonzero(trow == r)[0]
        r1, r2 = int(r) % g1, int(r) // g1
        for s0 in range(0, len(sel), TILE):
            lanes = sel[s0:s0 + TILE]
            cf, cl = int(tc[lanes[0]]) - int(r) * g0, int(tc[lanes[-1]]) - int(r) * g0
            a, b = max(cf - 1, 0), min(cl + 1, g0 - 1)
            run0, total = len(runs), 0
            for d2 in (-1, 0, 1):
                for d1 in (-1, 0, 1):
                    n1, n2 = r1 + d1, r2 + d2
                    if n1 < 0 or n1 >= g1 or n2 < 0 or n2 >= g2:
                        continue
                    row = n1 + g1 * n2
                    s, e = int(cstart[row * g0 + a]), int(cend[row * g0 + b])
                    if e <= s:
                        continue
                    rec0 = s // RECORDS * RECORDS
                    runs.append((rec0, round_up(e, RECORDS) - rec0))
                    total += runs[-1][1]
            push(ti[lanes], run0, len(runs) - run0)
            walked += len(lanes) * total
    loose = np.nonzero(~fx)[0]
    for s0 in range(0, len(loose), TILE):
        push(loose[s0:s0 + TILE], len(runs), 0)
    live_tiles = len(tiles)
    while len(tiles) % WAVES:
        push([], len(runs), 0)
    return dict(g=np.array(g, dtype=np.int64), lo=lo, h=float(h), n_pad=len(tiles) * TILE, m_pad=m_pad, m_alloc=m_alloc,
                live_tiles=live_tiles, walked=walked, tiles=np.array(tiles, dtype=np.int64).reshape(-1, 3),
                runs=np.array(runs, dtype=np.int64).reshape(-1, 2), tmap=np.array(tmap, dtype=np.int64), smap=smap)


def _finish(num, den, cnt, x, b, normalize, exclude_self):
    nan = np.isnan(x).any(axis=1)
    fin = np.isfinite(x).all(axis=1)
    with np.errstate(all="ignore"):
        if b is None:
            out = den / den if normalize else den
        else:
            out = num / den if normalize else num
    out = np.where(nan[:, None], np.nan, out)
    cnt = np.where(nan, -1, cnt - (fin & bool(exclude_self)))
    return out, cnt.astype(np.int64)


def dense(kernel, y, x, b, R, normalize=False, exclude_self=False):
    """(product (N, E) float64, counts (N,) int64) by the dense masked evaluation: all N x M pairs, s <= R R."""
    y, x = np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64)
    s = sqdists(x, y)
    with np.errstate(all="ignore"):
        inside = s <= R * R
    k = np.where(inside, kernel_values(kernel, np.where(inside, s, 0.0)), 0.0)
    bb = np.ones((len(y), 1)) if b is None else np.asarray(b, dtype=np.float64)
    return _finish(k @ bb, k.sum(axis=1, keepdims=True), inside.sum(axis=1), x, b, normalize, exclude_self)


def walk(kernel, y, x, b, R, normalize=False, exclude_self=False, factor=1.0, p=None):
    """The same two the way the kernels form them: every tile of the plan walks the records of its runs."""
    y, x = np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64)
    p = plan(y, x, R, factor) if p is None else p
    bb = np.ones((len(y), 1)) if b is None else np.asarray(b, dtype=np.float64)
    N = len(x)
    num, den, cnt = np.zeros((N, bb.shape[1])), np.zeros((N, 1)), np.zeros(N, dtype=np.int64)
    for t, (run0, nruns, live) in enumerate(p["tiles"]):
        if live == 0:
            continue
        i = p["tmap"][t * TILE:t * TILE + live]
        rec = np.concatenate([np.arange(r0, r0 + n) for r0, n in p["runs"][run0:run0 + nruns]] + [np.zeros(0, dtype=np.int64)])
        j = p["smap"][rec.astype(np.int64)]
        j = j[j >= 0]                                   # pad records sit at +inf: never inside
        s = sqdists(x[i], y[j])
        with np.errstate(all="ignore"):
            inside = s <= R * R
        k = np.where(inside, kernel_values(kernel, np.where(inside, s, 0.0)), 0.0)
        num[i], den[i], cnt[i] = k @ bb[j], k.sum(axis=1, keepdims=True), inside.sum(axis=1)
    return _finish(num, den, cnt, x, b, normalize, exclude_self)


# ---- the clouds of the GPU tests (tests/test_gpu_cutoff.py), also planned on the host -------------------------------------
CLOUDS = ("A", "B", "C", "K")


def cloud(name, precision):
    """(y, x or None for targets = sources, R) of the named cloud, the coordinates rounded to `precision`."""
    f32 = np.dtype(precision) != np.float64
    if name == "A":
        rs = np.random.RandomState(1 if f32 else 0)
        y, x, R = rs.rand(700, 3), None, 0.23
    elif name == "B":
        rs = np.random.RandomState(0)
        x = rs.rand(300, 2)
        y, R = 0.2 + 1.2 * rs.rand(500, 2), 0.11
    elif name == "C":
        rs = np.random.RandomState(0)
        y = rs.rand(400, 1)
        x, R = rs.rand(130, 1), 0.05
    elif name == "K":
        rs = np.random.RandomState(0)
        c = rs.rand(3, 3)
        blobs = [c[i] + 0.02 * rs.randn(150, 3) for i in range(3)]
        y, x, R = np.concatenate(blobs + [rs.rand(200, 3)]), None, 0.08
    elif name == "lattice":
        a, b = np.meshgrid(np.arange(16) / 8.0, np.arange(16) / 8.0, indexing="ij")
        y, x, R = np.stack([a.ravel(), b.ravel()], axis=1), None, 5.0 / 8.0
    else:
        raise ValueError(name)
    rnd = lambda a: None if a is None else np.asarray(a, dtype=precision).astype(np.float64)
    return rnd(y), rnd(x), R


def boundary_clear(y, x, R, precision):
    """No pair within the working precision's reach of the boundary: |s - R R| > tol R R for every pair, tol = 1e-5 for
    float32 inputs and 1e-12 for float64 -- the inside set is then the same in float64 and in the working precision."""
    tol = 1e-12 if np.dtype(precision) == np.float64 else 1e-5
    s = sqdists(y if x is None else x, y)
    return not np.any(np.abs(s - R * R) <= tol * R * R)
