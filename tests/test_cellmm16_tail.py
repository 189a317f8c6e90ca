"""cellmm16_kernel's TAIL list (option ``cell_tail``): the target blocks of the fused grid's last, partial round of MAIN
workgroups in more, shorter source segments (csrc/kmvp_plan.hpp: cell_tail_plan; the plan is held to its properties
without a GPU in tests/test_host_cell_tail.py).  What is checked here is that the kernel is right on the three lists.

``fast_sqdists = 3``, ``cellmm_shape = 1`` and ``fast_tiles = 8`` forced, as tests/test_cellmm16_balance.py forces them,
on the 40 000-point clouds of tests/cell_balance_cases.py, uniform and sheet, E = 1: 40 target blocks on the lattice's cells
and on count-cut cells alike.  A round of 16 or 32 resident workgroups cannot give these clouds a TAIL of two blocks or more
in twice the segments: the TAIL's segments are a multiple of 8, so two blocks of it are 16 workgroups, which leaves room
for no REST list in a round of 16 and, in a round of 32, asks for 37 or 38 blocks in whole rounds -- and whole rounds are
multiples of a power of two.  So ``segments = 4`` and ``cell_tail_resident = 48``: rounds of 12 blocks, 36 blocks stay, 4
take 8 segments (k = 2) beside a REST list that weighs 1 to 5 workgroups.  Asserted from kmvp_cell_lists.

* ``cell_tail = 0`` equals the default options bit for bit;
* with ``cell_tail = 1`` the rows outside the TAIL blocks equal those of ``cell_tail = 0`` bit for bit;
* the TAIL rows -- and the same rows with the option off -- lie within the band of oracle/kmvp_cell_model.py on the layout
  read back from the library (every 32nd of them: ~125 rows);
* the same with ``cell_shared_build = 0`` and with ``cell_balance = 1``;
* with rounds of 32 workgroups and 8 segments the 40 blocks are whole rounds: no TAIL, the two lists as ever, and the note
  does not speak of one;
* option values -1, 0, 1 are accepted, -2 and 2 refused; ``cell_tail_resident`` takes 0 and positive counts.
"""
import numpy as np
import pytest

import cell_model_cases as cases
from cell_balance_cases import small_clouds
from kernel_matrix_benchmarks_amd import _lib

pytestmark = pytest.mark.gpu

cm = cases.cm
TAIL_NOTE = "tail list"
VARIANTS = {"default": {}, "own_builds": {"cell_shared_build": 0}, "count_cut": {"cell_balance": 1}}

_clouds, _models = {}, {}


def cloud(name):
    if name not in _clouds:
        y = small_clouds()[name].astype(np.float32)
        _clouds[name] = (y, np.random.RandomState(5).randn(len(y), 1).astype(np.float32))
    return _clouds[name]


def context(name, **options):
    y, b = cloud(name)
    ctx = _lib.Context(0)
    try:
        for k, v in {**dict(fast_sqdists=3, cellmm_shape=1, fast_tiles=8, cell_balance=0), **options}.items():
            ctx.set_option(k, v)
        ctx.set_points(y, None, _lib.KMVP_F32)
        ctx.fit("gaussian")
        ctx.set_signal(b)
    except Exception:
        ctx.close()
        raise
    return ctx


def run(ctx, n, **options):
    for k, v in options.items():
        ctx.set_option(k, v)
    ctx.run("gaussian", False)
    assert ctx.last_kernel_name == "cellmm16_kernel", ctx.last_kernel_name
    return ctx.get_result(n, 1), ctx.last_dispatch_note


def model(name, variant, layout, rows):
    """the cell model on `rows`, once per cloud and kind of cells (the layout does not depend on the other options)"""
    key = (name, bool(layout["count_cut"]))
    if key not in _models:
        y, b = cloud(name)
        _models[key] = (rows, cm.cell_product(y, None, b, False, path="cellmm16", layout=layout, rows=rows))
    assert np.array_equal(_models[key][0], rows), (name, variant)
    return _models[key][1]


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", ["uniform", "sheet"])
def test_tail_list(name, variant):
    n = len(cloud(name)[0])
    ctx = context(name, segments=4, cell_tail_resident=48, **VARIANTS[variant])
    try:
        default, note_default = run(ctx, n)
        off, note_off = run(ctx, n, cell_tail=0)
        lists_off = ctx.cell_lists()
        on, note_on = run(ctx, n, cell_tail=1)
        lists = ctx.cell_lists()
        layout = ctx.cell_layout()
    finally:
        ctx.close()
    assert TAIL_NOTE not in note_default and TAIL_NOTE not in note_off and TAIL_NOTE in note_on, (note_default, note_off, note_on)
    assert layout["count_cut"] == (variant == "count_cut") and layout["tiles_per_wavefront"] == 8
    # the lists: 40 blocks x 4 segments -> 36 blocks stay (three rounds of 48), 4 take 8 segments
    assert lists_off["fused"] and lists_off["blocks"][0] == 40 and lists_off["blocks"][1] == 0 and lists_off["segments"][0] == 4
    b_full, b_tail, b_rest = lists["blocks"]
    s_main, s_tail, _ = lists["segments"]
    assert lists["fused"] and lists["resident"] == 48 and (b_full, b_tail, s_main, s_tail) == (36, 4, 4, 8), lists
    assert b_tail >= 2 and s_tail >= 2 * s_main and (b_full * s_main) % 48 == 0 and b_rest == lists_off["blocks"][2] > 0
    tail = lists["target_list"] == 2
    assert np.array_equal(lists_off["target_list"] == 1, lists["target_list"] == 1) and not (lists_off["target_list"] == 2).any()
    assert (b_tail - 1) * 1024 < np.count_nonzero(tail) <= b_tail * 1024  # (a block's slots; some are padding)
    # (a) the option off is the default, (b) rows outside the TAIL blocks are untouched
    assert np.array_equal(default, off)
    assert np.array_equal(on[~tail], off[~tail]), float(np.max(np.abs(on[~tail] - off[~tail])))
    # (c) the TAIL rows within the model's band, with the option on and off
    rows = np.flatnonzero(tail)[::32]
    m = model(name, variant, layout, rows)
    assert not m.flagged.any() and not m.nonfinite.any()
    for what, got in (("on", on), ("off", off)):
        err = np.abs(got[rows] - m.value)
        print(f"cloud {name} {variant} cell_tail {what}: {len(rows)} TAIL rows, max |err|/band {float(np.max(err / m.band)):.3g}, "
              f"max |on - off| / mass {float(np.max(np.abs(on[rows] - off[rows]) / m.mass)):.3g}")
        assert np.all(np.isfinite(got)) and np.all(err <= m.band), (name, variant, what, float(np.max(err / m.band)))


@pytest.mark.parametrize("name", ["uniform", "sheet"])
def test_whole_rounds_have_no_tail(name):
    """rounds of 32 workgroups, 8 segments: 40 blocks are ten whole rounds, and the two lists run as they ever did"""
    n = len(cloud(name)[0])
    ctx = context(name, segments=8, cell_tail_resident=32)
    try:
        off, note_off = run(ctx, n, cell_tail=0)
        on, note_on = run(ctx, n, cell_tail=1)
        lists = ctx.cell_lists()
    finally:
        ctx.close()
    assert note_on == note_off == "" and lists["fused"], (note_on, note_off)
    assert lists["blocks"][0] == 40 and lists["blocks"][1] == 0 and lists["segments"][:2] == (8, 0) and lists["resident"] == 32
    assert not (lists["target_list"] == 2).any()
    assert np.array_equal(on, off)


def test_option_values():
    ctx = _lib.Context(0)
    try:
        for v in (-1, 0, 1):
            ctx.set_option("cell_tail", v)
        for v in (0, 16, 32, 512):
            ctx.set_option("cell_tail_resident", v)
        for k, v in (("cell_tail", -2), ("cell_tail", 2), ("cell_tail_resident", -1)):
            with pytest.raises(_lib.KmvpError):
                ctx.set_option(k, v)
    finally:
        ctx.close()
