"""cellmm16_kernel with both lists of target tiles in ONE launch (option ``cell_fused``) against two launches.

The cells' whole groups of ``fast_tiles`` target tiles (the MAIN list) and their leftover tiles (the REST list, two per
wavefront) used to be two launches, the second one starting when the first had drained.  Now the REST list's workgroups
are the last workgroups of one grid.  Only the schedule differs: every workgroup computes what it computed in a launch
of its own, so the sums must be the same BIT FOR BIT, on every row, with ``cell_fused = 1`` and ``cell_fused = 0``.

Clouds in the unit cube (10^3 cells), ``cellmm_shape = 1`` and ``fast_sqdists = 3`` forced:
  a  330 017 points, targets = sources, 8 and 4 tiles per wave: about ten tiles per cell, one main group (or two) per cell
     plus leftover tiles -- both lists non-empty, N no multiple of 32; also held to the float64 oracle on sampled rows
  b  330 017 sources, 50 021 other targets, 8 tiles per wave: about two tiles per cell, every tile in the REST list -- the
     fused kernel with a MAIN grid of 0
  c  cloud a, 2 tiles per wave: no split, the option changes nothing
each with plain and with normalised rows (two columns, so two fused launches per product).
"""
import numpy as np
import pytest

import c_oracle
from conftest import rel_err
from kernel_matrix_benchmarks_amd import _lib

pytestmark = pytest.mark.gpu

TOL32 = 1e-5  # the float32 tolerance of the parity suite


def cloud(m, n_targets):
    rs = np.random.RandomState(m + (n_targets or 0))
    y = rs.rand(m, 3).astype(np.float32)
    b = rs.randn(m, 1).astype(np.float32)
    x = None if n_targets is None else rs.rand(n_targets, 3).astype(np.float32)
    return y, x, b


@pytest.fixture(scope="module")
def cloud_a():
    return cloud(330_017, None)


@pytest.fixture(scope="module")
def cloud_b():
    return cloud(330_017, 50_021)


@pytest.fixture(scope="module")
def oracle_a(cloud_a):
    """float64 truth of cloud a on ~400 sampled rows, plain and normalised: computed once"""
    y, _, b = cloud_a
    rows = np.arange(0, len(y), len(y) // 400)
    want = {norm: c_oracle.product(kernel="gaussian", source_points=y.astype(np.float64), target_points=None,
                                   source_signal=b.astype(np.float64), normalize_rows=norm, rows=rows)
            for norm in (False, True)}
    return rows, want


def run(y, x, b, tiles, norm, fused, runs=2):
    """the product with `tiles` target tiles per wave on either schedule; bitwise equal over `runs` runs"""
    ctx = _lib.Context(0)
    try:
        ctx.set_option("fast_sqdists", 3)
        ctx.set_option("cellmm_shape", 1)
        ctx.set_option("fast_tiles", tiles)
        ctx.set_option("cell_fused", fused)
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
        assert np.array_equal(o, outs[0]), (tiles, norm, fused)
    assert np.all(np.isfinite(outs[0])), (tiles, norm, fused)
    return outs[0]


def both_schedules(y, x, b, tiles, norm):
    two = run(y, x, b, tiles, norm, fused=0)
    one = run(y, x, b, tiles, norm, fused=1)
    assert np.array_equal(one, two), (tiles, norm, int(np.count_nonzero(one != two)))
    return one


@pytest.mark.parametrize("norm", [False, True], ids=["plain", "normalised"])
@pytest.mark.parametrize("tiles", [8, 4])
def test_both_lists_in_one_launch(cloud_a, oracle_a, tiles, norm):
    y, x, b = cloud_a
    got = both_schedules(y, x, b, tiles, norm)
    rows, want = oracle_a
    err = rel_err(got[rows], want[norm])
    print(f"tiles {tiles} normalised {norm}: error against the oracle on {len(rows)} rows {err:.3e}")
    assert err <= TOL32, (tiles, norm, err)
    # the automatic setting is the fused schedule, and the same numbers
    auto = run(y, x, b, tiles, norm, fused=-1, runs=1)
    assert np.array_equal(auto, got)


@pytest.mark.parametrize("norm", [False, True], ids=["plain", "normalised"])
def test_rest_list_alone_through_the_fused_kernel(cloud_b, norm):
    y, x, b = cloud_b
    both_schedules(y, x, b, 8, norm)


@pytest.mark.parametrize("norm", [False, True], ids=["plain", "normalised"])
def test_no_split_at_two_tiles_per_wave(cloud_a, norm):
    y, x, b = cloud_a
    both_schedules(y, x, b, 2, norm)


def test_option_range():
    ctx = _lib.Context(0)
    try:
        for v in (-1, 0, 1):
            ctx.set_option("cell_fused", v)
        for v in (-2, 2):
            with pytest.raises(_lib.KmvpError):
                ctx.set_option("cell_fused", v)
    finally:
        ctx.close()
