"""Clouds for the count-cut cells (option ``cell_balance``; csrc/kmvp_plan.hpp: count_cut_cells), shared by
tests/test_host_cell_balance.py and tests/test_cellmm16_balance.py, and a numpy restatement of how cell_prepare() makes
fine keys from points: cell_make_grid(), cell_balance_cap() and cell_fine_keys_kernel, in their arithmetic (the lattice in
float32, the buckets along z in float64)."""
import numpy as np

CELL_T_MAX = np.float32(0.016)
CELL_Z_WIDTH_MAX = 0.125
ZQ_BITS, ZQ = 12, 4096


def small_clouds():
    """name -> (40000, 3) float64 points in the box 0.2 x 0.2 x 1 (four lattice columns) or 0.2 x 0.2 x 4"""
    box = np.array([0.2, 0.2, 1.0])
    uniform = np.random.RandomState(11).rand(40000, 3) * box
    sheet = uniform.copy()  # half the points in the sheet 0.5 <= z <= 0.52
    sheet[::2, 2] = 0.5 + 0.02 * np.random.RandomState(12).rand(20000)
    copies = uniform.copy()  # 3000 copies of one point: one bucket holds more than a whole cell
    copies[:3000] = np.array([0.13, 0.07, 0.41])
    tall = np.random.RandomState(11).rand(40000, 3) * np.array([0.2, 0.2, 4.0])  # the cap binds everywhere
    return {"uniform": uniform, "sheet": sheet, "copies": copies, "tall": tall}


def other_targets():
    """30011 targets of their own in the box of the 'uniform' cloud"""
    return np.random.RandomState(13).rand(30011, 3) * np.array([0.2, 0.2, 1.0])


def headline_points(n=1_000_000, D=3):
    """the benchmark's config 2 (bench.py)"""
    return np.random.RandomState(n + D).rand(n, D)


def fine_keys(points, box_of=None):
    """Sorted fine keys of `points` (float32) on the grid of the bounding box of `box_of` (default: the points themselves).
    Returns dict(fine, z (sorted alike), cap, bucket, lo_z, g (cells per axis), h (cell sides))."""
    y = np.asarray(points, np.float32)
    ref = y if box_of is None else np.asarray(box_of, np.float32)
    D = y.shape[1]
    assert D == 3
    h_max = np.float32(np.sqrt(np.float32(2.0) * CELL_T_MAX / np.float32(D)))
    idx, g, h, glo = [], [], [], []
    for a in range(D):
        lo, hi = ref[:, a].min(), ref[:, a].max()
        centre, half = np.float32(0.5) * (lo + hi), np.float32(0.5) * (hi - lo)
        cells = int(max(1.0, np.ceil(2.0 * float(half) / float(h_max))))
        side = np.float32(2.0 * float(half) / cells)
        inv_h = np.float32(1.0) / side
        origin = np.float32(centre - half)
        idx.append(np.floor((y[:, a] - origin) * inv_h).astype(np.int64).clip(0, cells - 1))
        g.append(cells)
        h.append(side)
        glo.append(origin)
    column = (idx[0] | (idx[1] << 10)).astype(np.uint32)
    extent = float(g[2]) * float(h[2])
    bucket = extent / ZQ
    zq_per_unit = ZQ / extent
    zq = np.floor((y[:, 2].astype(np.float64) - float(glo[2])) * zq_per_unit).astype(np.int64).clip(0, ZQ - 1)
    room = 2.0 * float(CELL_T_MAX) - float(h[0]) * float(h[0]) - float(h[1]) * float(h[1])
    width = min(np.sqrt(room), CELL_Z_WIDTH_MAX)
    cap = int(min(ZQ, np.floor(width / bucket)))
    fine = (column << np.uint32(ZQ_BITS)) | zq.astype(np.uint32)
    order = np.argsort(fine, kind="stable")
    return dict(fine=fine[order], z=y[order, 2], cap=cap, bucket=bucket, lo_z=glo[2], g=g, h=h, order=order)
