"""Clouds, options and the stage pattern of tests/test_cellmm16_runs.py and tests/make_cellmm16_runs_golden.py.

cellmm16_kernel walks a stage of 12 source tiles in CELL RUNS: one ballot finds where the current cell's tiles end, and the
tile loop between holds a tile's work alone.  What can go wrong is where runs meet stages, so the clouds here are MADE to
put the runs there: 27 lattice cells (a box of side 0.3 in cells of side 0.1) filled with a prescribed number of source
TILES each, in the order the kernel walks them (x fastest).  With ``TILES`` below, the sources' tiles are

    cell   0: tiles   0 ..  63   stages 0-4 whole: four stages without a change, the cell carried from stage to stage
    cell   1: tiles  64 ..  71   ends with stage 5, so stage 6 starts with a change at position 0
    cell   2: tiles  72 ..  82
    cell   3: tile   83          a change at position 11 of stage 6, and a run of ONE tile
    cell   4: tile   84          a run of one tile at position 0
    ...
    cell  26: 7, 6 or 11 tiles   529, 528 or 533 tiles in all: the last stage holds 1, 12 or 5 source tiles

``stage_pattern`` recomputes all of this from the layout the library reads back (kmvp_cell_layout, kmvp_cell_lists), and the
test asserts the edges from that, not from this table.

No list of the plan ever has a segment without a stage (settle_segments and cell_split round the segments to
ceil(m_stages / ceil(m_stages / segments))), so that edge cannot be reached through the library; ``stage_pattern`` reports
the empty segments of every list and the test asserts that there are none.
"""
import numpy as np

STAGE_TILES = 12
TILE = 32
#        cell 0   1   2  3  4   5   6  7   8   9 10  11  12 13  14  15 16  17  18 19  20  21  22  23 24  25
TILES = [64, 8, 11, 1, 1, 23, 40, 9, 30, 17, 5, 44, 12, 3, 26, 35, 2, 19, 28, 7, 33, 14, 21, 38, 6, 25]
LAST = {"live1": 7, "live12": 6, "live5": 11}  # tiles of cell 26 -> source tiles of the last stage: 1, 12, 5
CLOUDS = tuple(LAST)

BASE = dict(fast_sqdists=3, cellmm_shape=1, cell_balance=0, segments=4)
# the TAIL list on cloud live1 at eight tiles per wavefront: found on the host (csrc/kmvp_plan.hpp behind the shims of
# tests/test_host_cell_tail.py and tests/test_host_shared_build.py), asserted from kmvp_cell_lists in the test
TAIL = dict(cell_tail=1, cell_tail_resident=48)


def make_cloud(name):
    """(sources = targets (M, 3) float32, signal (M, 1) float32) of cloud `name`"""
    tiles = TILES + [LAST[name]]
    rs = np.random.RandomState(20 + CLOUDS.index(name))
    pts = []
    for c, t in enumerate(tiles):
        n = TILE * (t - 1) + int(rs.randint(1, TILE + 1))  # t tiles, the last one partly filled
        origin = 0.1 * np.array([c % 3, (c // 3) % 3, c // 9])
        p = origin + 0.1 * (0.05 + 0.9 * rs.rand(n, 3))
        if c == 0:
            p[0] = 0.0  # the box's corners: the lattice is 3 x 3 x 3 cells of side 0.1
        if c == 26:
            p[0] = 0.3
        pts.append(p)
    y = np.concatenate(pts)
    y = y[rs.permutation(len(y))].astype(np.float32)
    b = rs.randn(len(y), 1).astype(np.float32)
    return y, b


def cases():
    """(id, cloud, options, normalised): every tile count, shared build on and off, plain and normalised rows on live1; the
    other last stages at eight and two tiles per wavefront; the TAIL list; one launch with the rule's own segments"""
    out = []
    for tiles in (1, 2, 4, 8):
        for norm in (False, True):
            out.append((f"live1-t{tiles}-{'norm' if norm else 'plain'}", "live1", dict(fast_tiles=tiles), norm))
    for norm in (False, True):
        out.append((f"live1-t8-own-{'norm' if norm else 'plain'}", "live1", dict(fast_tiles=8, cell_shared_build=0), norm))
        out.append((f"live1-t8-tail-{'norm' if norm else 'plain'}", "live1", dict(fast_tiles=8, **TAIL), norm))
    out.append(("live1-t8-tail-own-plain", "live1", dict(fast_tiles=8, cell_shared_build=0, **TAIL), False))
    for name in ("live12", "live5"):
        for tiles in (2, 8):
            out.append((f"{name}-t{tiles}-plain", name, dict(fast_tiles=tiles), False))
    out.append(("live5-t8-rule-segments-plain", "live5", dict(fast_tiles=8, segments=0), False))
    return out


def sample_rows(n):
    """the rows the golden file holds in full (beside a digest of the whole output)"""
    return np.sort(np.random.RandomState(7).choice(n, 1024, replace=False))


def stage_pattern(layout, lists):
    """The source tiles as cellmm16_kernel walks them, from the layout and the lists read back from the library.
    Returns a dict: tiles (cell of every source tile), m_stages, n_live (source tiles of the last stage), runs (length of
    every cell run within a stage of a MAIN segment), and the stages s of the MAIN list that are not the first of their
    segment and
      change_at_0[s]   start with another cell than stage s - 1 ended with (the run before ended with its stage),
      change_at_11[s]  change cell at their last position,
      carried[s]       hold 12 tiles of the cell stage s - 1 ended with (no change, the cell carried),
    and empty_segments, the segments without a stage over all lists."""
    cell = layout["source_cell"]
    assert cell.min() >= 0
    counts = np.bincount(cell, minlength=len(layout["source_centres"]))
    tiles = np.repeat(np.arange(len(counts)), -(-counts // TILE))
    m_stages = -(-len(tiles) // STAGE_TILES)
    empty = 0
    for segments in lists["segments"]:
        if segments:
            empty += segments - -(-m_stages // -(-m_stages // segments))
    seg_stages = -(-m_stages // lists["segments"][0])
    p = dict(tiles=tiles, m_stages=m_stages, n_live=len(tiles) - STAGE_TILES * (m_stages - 1), empty_segments=empty,
             seg_stages=seg_stages, runs=[], change_at_0=[], change_at_11=[], carried=[])
    for s in range(m_stages):
        st = tiles[STAGE_TILES * s:STAGE_TILES * (s + 1)]
        cuts = np.flatnonzero(np.diff(st)) + 1
        p["runs"] += list(np.diff(np.concatenate(([0], cuts, [len(st)]))))
        if s % seg_stages == 0:
            continue
        before = tiles[STAGE_TILES * s - 1]
        if st[0] != before:
            p["change_at_0"].append(s)
        if len(st) == STAGE_TILES and st[11] != st[10]:
            p["change_at_11"].append(s)
        if len(st) == STAGE_TILES and len(cuts) == 0 and st[0] == before:
            p["carried"].append(s)
    return p
