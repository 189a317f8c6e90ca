"""The float32 cell kernels on count-cut cells (option ``cell_balance``): lattice columns cut along z by point count.

With ``cell_balance = 1`` cell_prepare() sorts by fine keys, cuts every (x, y) column into cells of up to 1024 points
(csrc/kmvp_plan.hpp: count_cut_cells; the lists are held to their invariants without a GPU in
tests/test_host_cell_balance.py) and hands the packers a table of centres.  The kernels are the ones they were; what is
checked here is that they are right on these cells.

``fast_sqdists = 3``, ``cellmm_shape = 1``, ``fast_tiles = 8`` and ``cell_balance = 1`` forced, as
tests/test_cellmm16_shared_build.py forces its options.  Clouds of tests/cell_balance_cases.py: 40 000 points in a box of
0.2 x 0.2 x 1 (four columns of ~10 cells) -- uniform; half of them in the sheet 0.5 <= z <= 0.52; with 3000 copies of one
point (cells of one range and one centre); the box 0.2 x 0.2 x 4, where the cap on a cell's width binds everywhere -- and the
uniform cloud as sources of 30 011 other targets (each cloud its own cut and table).  Plain and normalised:

* results are finite and within the parity suite's rule, max(TOL32, 2 x the float32 reference's own error), of the float64
  oracle on about 400 sampled rows; the float32 reference is the brute-force product (differences, exp, matrix product)
  carried out in numpy float32 on those rows;
* two runs are equal bit for bit; ``cell_shared_build`` 1 against 0 and ``cell_fused`` 1 against 0 are equal bit for bit
  on these cells too;
* ``cellmm_shape = 0`` (cellmm_kernel) and ``fast_sqdists = 4`` (cell_kernel) on the same cells meet the same tolerance;
* at ``fast_tiles = 4`` the option changes nothing: the result equals ``cell_balance = 0`` bit for bit;
* option values -1, 0, 1 are accepted, -2 and 2 refused.

Measured on an MI355X: errors of 1.4e-7 ... 1.4e-6 on every cloud but the sheet, whose dense, sign-cancelling sums give
4.7e-6 (cellmm16_kernel, cellmm_kernel) and 9.7e-6 (cell_kernel) -- the cloud, not the cells: the lattice's cells give
4.4e-6 and 1.2e-5 there.  Every figure is within TOL32 itself.
"""
import numpy as np
import pytest

import c_oracle
from cell_balance_cases import other_targets, small_clouds
from conftest import rel_err
from kernel_matrix_benchmarks_amd import _lib

pytestmark = pytest.mark.gpu

TOL32 = 1e-5  # the float32 tolerance of the parity suite
NAMES = ["uniform", "sheet", "copies", "tall", "uniform_other_targets"]

_clouds, _oracle = {}, {}


def cloud(name):
    if name not in _clouds:
        base = small_clouds()[name.replace("_other_targets", "")].astype(np.float32)
        x = other_targets().astype(np.float32) if name.endswith("_other_targets") else None
        b = np.random.RandomState(5).randn(len(base), 1).astype(np.float32)
        _clouds[name] = (base, x, b)
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
        targets = (y if x is None else x)[rows]
        ref32 = np.empty((len(rows), 1), np.float32)
        for lo in range(0, len(rows), 64):  # the brute-force product in float32
            d = targets[lo:lo + 64, None, :] - y[None, :, :]
            k = np.exp(-np.sum(d * d, axis=-1))
            ref32[lo:lo + 64] = (k @ b) / k.sum(axis=1, keepdims=True) if norm else k @ b
        assert ref32.dtype == np.float32
        _oracle[name, norm] = (rows, want, max(TOL32, 2 * rel_err(ref32.astype(np.float64), want)))
    return _oracle[name, norm]


def context(name, tiles, balance):
    y, x, b = cloud(name)
    ctx = _lib.Context(0)
    try:
        ctx.set_option("fast_sqdists", 3)
        ctx.set_option("cellmm_shape", 1)
        ctx.set_option("fast_tiles", tiles)
        ctx.set_option("cell_balance", balance)
        ctx.set_points(y, x, _lib.KMVP_F32)
        ctx.fit("gaussian")
        ctx.set_signal(b)
    except Exception:
        ctx.close()
        raise
    return ctx, (len(y) if x is None else len(x))


@pytest.mark.parametrize("norm", [False, True], ids=["plain", "normalised"])
@pytest.mark.parametrize("name", NAMES)
def test_count_cut_cells(name, norm):
    rows, want, tol = oracle(name, norm)
    ctx, n = context(name, 8, 1)
    try:
        def run(kernel_name, **options):
            for k, v in options.items():
                ctx.set_option(k, v)
            ctx.run("gaussian", norm)
            out = ctx.get_result(n, 1)
            assert ctx.last_kernel_name == kernel_name and "count-cut cells" in ctx.last_dispatch_note, \
                (ctx.last_kernel_name, ctx.last_dispatch_note)
            return out

        first = run("cellmm16_kernel")
        again = run("cellmm16_kernel")
        own = run("cellmm16_kernel", cell_shared_build=0)
        two = run("cellmm16_kernel", cell_shared_build=1, cell_fused=0)
        mm32 = run("cellmm_kernel", cell_fused=-1, cellmm_shape=0)
        valu = run("cell_kernel", fast_sqdists=4)
    finally:
        ctx.close()
    errs = {k: rel_err(v[rows], want) for k, v in (("cellmm16", first), ("cellmm", mm32), ("cell", valu))}
    print(f"cloud {name} normalised {norm}: run to run {np.array_equal(first, again)}, own builds {np.array_equal(first, own)}, "
          f"two launches {np.array_equal(first, two)}, rel_err {errs}, tolerance {tol:.2e}")
    for out in (first, mm32, valu):
        assert np.all(np.isfinite(out)), name
    assert np.array_equal(first, again), (name, norm)
    assert np.array_equal(first, own), (name, norm, float(np.max(np.abs(first - own))))
    assert np.array_equal(first, two), (name, norm, float(np.max(np.abs(first - two))))
    for k, e in errs.items():
        assert e <= tol, (name, norm, k, e, tol)


@pytest.mark.parametrize("name", ["uniform", "uniform_other_targets"])
def test_four_tiles_per_wavefront_keep_the_lattice(name):
    outs = []
    for balance in (1, 0):
        ctx, n = context(name, 4, balance)
        try:
            ctx.run("gaussian", False)
            outs.append(ctx.get_result(n, 1))
            assert ctx.last_kernel_name == "cellmm16_kernel" and ctx.last_dispatch_note == "", ctx.last_dispatch_note
        finally:
            ctx.close()
    assert np.array_equal(outs[0], outs[1])
    rows, want, tol = oracle(name, False)
    assert rel_err(outs[0][rows], want) <= tol


def test_option_values():
    ctx = _lib.Context(0)
    try:
        for v in (-1, 0, 1):
            ctx.set_option("cell_balance", v)
        for v in (-2, 2):
            with pytest.raises(_lib.KmvpError):
                ctx.set_option("cell_balance", v)
    finally:
        ctx.close()
