"""Inputs of tests/test_host_plan.py: the grid the launch plans are recorded over (tests/golden/host_plan.json) and the
seeded sequences of sorted cell keys the tile lists are built from."""
import numpy as np

GRID_N = [1, 31, 32, 2000, 32767, 32768, 100000, 1000000, 10000000]
GRID_M = GRID_N
GRID_OPT = [0, 1, 3, 8, 17, 70000]  # the "segments" option; 0: the rule decides
SETTLE_UNITS = [1, 7, 8, 9, 63, 64, 100, 1000, 7813, 78125]
SETTLE_SEG = [1, 3, 8, 16, 17, 24, 40, 65535]
CELL_TT = [1, 2, 4, 8]  # target tiles per wavefront
CELL_TILE = 32


def key_sequences():
    """(name, sorted uint32 keys): no point at all, one point, one cell, and random cells of 1 .. 40 tiles of 32 points
    (every remainder modulo 8 occurs), the last tile of a cell filled to 1 .. 32 points."""
    seqs = [("empty", np.zeros(0, np.uint32)), ("one_point", np.array([5], np.uint32)),
            ("one_cell", np.full(1000, 7, np.uint32)), ("one_tile_cells", np.arange(37, dtype=np.uint32).repeat(3))]
    for seed in range(6):
        rs = np.random.RandomState(1000 + seed)
        ncells = int(rs.randint(1, 60))
        tiles = rs.randint(1, 41, size=ncells)
        counts = (tiles - 1) * CELL_TILE + rs.randint(1, CELL_TILE + 1, size=ncells)
        keys = np.cumsum(rs.randint(1, 1 << 20, size=ncells)).astype(np.uint32)  # increasing, distinct
        seqs.append(("seed%d" % seed, np.repeat(keys, counts)))
    return seqs
