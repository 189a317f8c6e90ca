"""Python restatement of the batched clouds (include/kmvp.h kmvp_set_batches) -- TEST INFRASTRUCTURE ONLY.

plan(): the layout and launch plan of csrc/kmvp_batch_plan.hpp from its description, batch by batch:
  * targets: every batch padded to whole tiles of TILE = 64 slots, the total rounded up to whole workgroups of WAVES = 4
    tiles with filler tiles (empty range, no live lane);
  * sources: every batch padded to a multiple of RECORDS = 8, a batch's range starting where the previous one ended, one
    spare batch of 8 records behind the last range;
  * one entry per tile: (first record, the caller's index of that record's source, the caller's index of lane 0, padded
    length of the range, live lanes); the padded -> caller maps with -1 for pads.
clouds(): the ragged batches the GPU tests share, as per-cloud arrays."""
import numpy as np

TILE, WAVES, RECORDS = 64, 4, 8

# the sizes of the GPU tests' ragged batches: targets x sources, permuted against each other below
TARGET_SIZES = (0, 1, 63, 64, 65, 130)
SOURCE_SIZES = (300, 0, 1, 7, 8, 9)


def offsets(sizes):
    return np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.int64)


def plan(y_off, x_off):
    """dict(n_pad, m_pad, m_alloc, tiles (T, 5) int64 [rec0, j0, i0, len, live], tmap (n_pad,), smap (m_alloc,))."""
    y_off, x_off = np.asarray(y_off, dtype=np.int64), np.asarray(x_off, dtype=np.int64)
    tiles, tmap, smap = [], [], []
    rec = 0
    for b in range(len(y_off) - 1):
        m, n = int(y_off[b + 1] - y_off[b]), int(x_off[b + 1] - x_off[b])
        length = -(-m // RECORDS) * RECORDS
        for t0 in range(0, n, TILE):
            live = min(TILE, n - t0)
            tiles.append((rec, int(y_off[b]), int(x_off[b]) + t0, length, live))
            tmap += [int(x_off[b]) + t0 + l if l < live else -1 for l in range(TILE)]
        smap += [int(y_off[b]) + j if j < m else -1 for j in range(length)]
        rec += length
    smap += [-1] * RECORDS
    while len(tiles) % WAVES:
        tiles.append((0, 0, 0, 0, 0))
        tmap += [-1] * TILE
    return dict(n_pad=len(tiles) * TILE, m_pad=rec, m_alloc=rec + RECORDS,
                tiles=np.array(tiles, dtype=np.int64).reshape(-1, 5), tmap=np.array(tmap, dtype=np.int64),
                smap=np.array(smap, dtype=np.int64))


def ragged_sizes(order=0):
    """(target sizes, source sizes) of the six ragged batches: every target size meets one source size; `order` rotates
    the source sizes against the target sizes, so that over the rotations every target size meets every source size."""
    k = order % len(SOURCE_SIZES)
    return list(TARGET_SIZES), list(SOURCE_SIZES[k:] + SOURCE_SIZES[:k])


def clouds(rs, D, E, order=0, points=None, scale=1.0):
    """The ragged batches as lists of per-cloud float64 arrays: xs[b] (n_b, D), ys[b] (m_b, D), bs[b] (m_b, E).  points:
    a generator (rs, n, D) -> (n, D), default uniform in [0, scale)^D."""
    ns, ms = ragged_sizes(order)
    gen = points or (lambda rs, n, D: rs.rand(n, D) * scale)
    xs = [gen(rs, n, D) for n in ns]
    ys = [gen(rs, m, D) for m in ms]
    bs = [rs.randn(m, E) for m in ms]
    return xs, ys, bs


def concat(parts, width):
    return np.ascontiguousarray(np.concatenate([p.reshape(-1, width) for p in parts], axis=0))


def sizes_of(parts):
    return offsets([len(p) for p in parts])
