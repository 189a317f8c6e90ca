"""cellmm16_kernel's shared operand build (option ``cell_shared_build``) against every wavefront building its own.

A workgroup whose four wavefronts own target tiles of ONE cell builds each source tile's A operand once -- wavefront w the
tiles 3 w .. 3 w + 2 of a stage -- and all four read it from LDS; every other workgroup runs the body it always ran.  Each
lane sums the same weights in the same order and feeds the same operand bits to the same MFMAs, so the sums must be the
same BIT FOR BIT, on every row, with ``cell_shared_build = 1`` and ``= 0``.  A race between builders and readers, a slip
in the image's layout or a barrier one wavefront misses shows as a mismatch here, not as a tolerance question.

``fast_sqdists = 3`` and ``cellmm_shape = 1`` forced, as in tests/test_cellmm16_fold.py.  Clouds whose cells hold many tiles, so
that one launch has one-cell AND mixed workgroups (counted without a GPU in tests/test_host_shared_build.py):

* A = RandomState(1).rand(40000, 3) * 0.3: 27 cells of 45-48 tiles;
* B = RandomState(2).rand(35000, 3) * 0.2: 8 cells of 134-140 tiles, with a REST list and the fused launch at eight tiles
  per wavefront (also run as two launches, ``cell_fused = 0``);
* A's sources with 30 011 other targets in the same box.

Every tile count (1, 2, 4, 8; the shared body exists at 8, below it the option must change nothing), plain and normalised:
``= 1`` equals ``= 0`` on all rows, two runs with ``= 1`` are equal, and ``= 1`` meets the float32 tolerance of the parity suite
against the float64 oracle on about 400 sampled rows.
"""
import numpy as np
import pytest

import c_oracle
from conftest import rel_err
from kernel_matrix_benchmarks_amd import _lib

pytestmark = pytest.mark.gpu

TOL32 = 1e-5  # the float32 tolerance of the parity suite


def make_cloud(name):
    if name == "A":
        rs, m, side, n_targets = np.random.RandomState(1), 40000, 0.3, None
    elif name == "B":
        rs, m, side, n_targets = np.random.RandomState(2), 35000, 0.2, None
    else:  # "A_other_targets"
        rs, m, side, n_targets = np.random.RandomState(1), 40000, 0.3, 30011
    y = (rs.rand(m, 3) * side).astype(np.float32)
    b = rs.randn(m, 1).astype(np.float32)
    x = None if n_targets is None else (np.random.RandomState(3).rand(n_targets, 3) * side).astype(np.float32)
    return y, x, b


_clouds, _oracle = {}, {}


def cloud(name):
    if name not in _clouds:
        _clouds[name] = make_cloud(name)
    return _clouds[name]


def oracle(name, norm):
    """float64 oracle on ~400 sampled rows, computed once per (cloud, normalisation)"""
    if (name, norm) not in _oracle:
        y, x, b = cloud(name)
        n = len(y) if x is None else len(x)
        rows = np.arange(0, n, max(1, n // 400))
        want = c_oracle.product(kernel="gaussian", source_points=y.astype(np.float64),
                                target_points=None if x is None else x.astype(np.float64),
                                source_signal=b.astype(np.float64), normalize_rows=norm, rows=rows)
        _oracle[name, norm] = (rows, want)
    return _oracle[name, norm]


def products(name, tiles, norm, fused=-1):
    """(shared build, shared build again, every wavefront its own) of one context"""
    y, x, b = cloud(name)
    n = len(y) if x is None else len(x)
    ctx = _lib.Context(0)
    try:
        ctx.set_option("fast_sqdists", 3)
        ctx.set_option("cellmm_shape", 1)
        ctx.set_option("fast_tiles", tiles)
        ctx.set_option("cell_fused", fused)
        ctx.set_points(y, x, _lib.KMVP_F32)
        ctx.fit("gaussian")
        ctx.set_signal(b)
        outs = []
        for shared in (1, 1, 0):
            ctx.set_option("cell_shared_build", shared)
            ctx.run("gaussian", norm)
            outs.append(ctx.get_result(n, 1))
            assert ctx.last_kernel_name == "cellmm16_kernel"
    finally:
        ctx.close()
    return outs


def check(name, tiles, norm, fused=-1):
    on, again, off = products(name, tiles, norm, fused)
    rows, want = oracle(name, norm)
    err = rel_err(on[rows], want)
    print(f"cloud {name} tiles {tiles} normalised {norm} fused {fused}: equal to own builds {np.array_equal(on, off)}, "
          f"run to run {np.array_equal(on, again)}, rel_err {err:.2e}")
    assert np.all(np.isfinite(on)), (name, tiles)
    assert np.array_equal(on, off), (name, tiles, norm, float(np.max(np.abs(on - off))))
    assert np.array_equal(on, again), (name, tiles, norm)
    assert err <= TOL32, (name, tiles, norm, err)


@pytest.mark.parametrize("tiles", [1, 2, 4, 8])
@pytest.mark.parametrize("norm", [False, True], ids=["plain", "normalised"])
@pytest.mark.parametrize("name", ["A", "B", "A_other_targets"])
def test_shared_build_is_bitwise_the_own_build(name, norm, tiles):
    check(name, tiles, norm)


@pytest.mark.parametrize("norm", [False, True], ids=["plain", "normalised"])
def test_shared_build_in_two_launches(norm):
    check("B", 8, norm, fused=0)


def test_option_values():
    ctx = _lib.Context(0)
    try:
        for v in (-1, 0, 1):
            ctx.set_option("cell_shared_build", v)
        for v in (-2, 2):
            with pytest.raises(_lib.KmvpError):
                ctx.set_option("cell_shared_build", v)
    finally:
        ctx.close()
