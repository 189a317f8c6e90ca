"""cellmm16_kernel (16x16x32 f16 MFMA cell form) forced at sizes where its source-cell fold runs often.

The fold sums each half tile's accumulator over its 64 lanes when the source cell changes, and leaves lane row k with
the column sums of half tile 4 g + k (one target per lane; at one tile per wave the group is padded with zeros).  These
tests force ``cellmm_shape = 1`` and check every tile count against the float64 oracle on sampled rows, on clouds whose
cells hold one or two tiles (a fold at almost every tile and at stage boundaries) and about ten tiles (one whole group
of eight per cell in the main launch, the rest in the leftover launch), with N not a multiple of 32, targets != sources
and normalised rows; bitwise equal run to run, and the same sums across tile counts to float32 rounding.
"""
import numpy as np
import pytest

import c_oracle
from conftest import rel_err
from kernel_matrix_benchmarks_amd import _lib

pytestmark = pytest.mark.gpu

TOL32 = 1e-5          # the float32 tolerance of the parity suite
TILE_RULE = 5e-6      # test_matrix_core_kernels_reproducible_and_tile_count_independent: max |diff| <= 5e-6 max |a|


def cellmm16(y, x, b, tiles, norm, runs=2):
    """Cell form on the 16x16x32 shape with `tiles` target tiles per wave; asserts bitwise equality over `runs` runs."""
    ctx = _lib.Context(0)
    try:
        ctx.set_option("fast_sqdists", 3)
        ctx.set_option("cellmm_shape", 1)
        ctx.set_option("fast_tiles", tiles)
        ctx.set_points(y, x, _lib.KMVP_F32)
        ctx.fit("gaussian")
        ctx.set_signal(b)
        n = len(y) if x is None else len(x)
        outs = []
        for _ in range(runs):
            ctx.run("gaussian", norm)
            outs.append(ctx.get_result(n, 1))
        assert ctx.last_kernel_name == "cellmm16_kernel"
    finally:
        ctx.close()
    for o in outs[1:]:
        assert np.array_equal(o, outs[0]), (tiles, norm)
    return outs[0]


def cloud(m, n_targets, seed):
    rs = np.random.RandomState(seed)
    y = rs.rand(m, 3).astype(np.float32)
    b = rs.randn(m, 1).astype(np.float32)
    x = None if n_targets is None else rs.rand(n_targets, 3).astype(np.float32)
    return y, x, b


# (sources, targets or None for targets == sources): the unit cube holds 10^3 cells, so 40 007 points are one or two
# tiles of 32 per cell, 330 017 about ten
CLOUDS = [(40_007, None), (40_007, 30_011), (330_017, None), (330_017, 50_021)]


@pytest.mark.parametrize("m,n_targets", CLOUDS, ids=[f"m{m}_n{n}" for m, n in CLOUDS])
@pytest.mark.parametrize("norm", [False, True], ids=["plain", "normalised"])
def test_cellmm16_every_tile_count_against_the_oracle(m, n_targets, norm):
    y, x, b = cloud(m, n_targets, seed=m + (n_targets or 0))
    n = m if n_targets is None else n_targets
    rows = np.arange(0, n, max(1, n // 400))
    want = c_oracle.product(kernel="gaussian", source_points=y.astype(np.float64),
                            target_points=None if x is None else x.astype(np.float64),
                            source_signal=b.astype(np.float64), normalize_rows=norm, rows=rows)
    base = None
    for tiles in (1, 2, 4, 8):
        got = cellmm16(y, x, b, tiles, norm)
        assert np.all(np.isfinite(got)), tiles
        assert rel_err(got[rows], want) <= TOL32, (tiles, rel_err(got[rows], want))
        if base is None:
            base = got
        else:
            scale = np.max(np.abs(base))
            assert np.max(np.abs(got - base)) <= TILE_RULE * scale, (tiles, np.max(np.abs(got - base)) / scale)
