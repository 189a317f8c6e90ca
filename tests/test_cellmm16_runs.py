"""cellmm16_kernel's tile loop in cell runs, against the loop that asked every tile for its key.

The kernel walks a stage's 12 source tiles run by run: the stage's live tiles are counted once, a run's end comes from one
ballot over the keys, a change of cell folds between two runs, and the tile loop between holds reads, weight sum and MFMAs
alone.  No arithmetic moved, so every sum must be what it was BIT FOR BIT.  ``tests/golden/cellmm16_runs_parent.npz`` holds
the sums of the library before the change on the cases of ``cellmm16_runs_cases.py`` (tests/make_cellmm16_runs_golden.py):
the SHA-256 of every whole output and 1024 rows in full.

The clouds are built to put the runs where the walk can go wrong, and every case asserts from what the library reads back
(kmvp_cell_layout, kmvp_cell_lists; a stage is 12 consecutive source tiles) that it still does -- in stages that are not
the first of their MAIN segment, where the cell in hand is the previous stage's:

1. a run that ends with its stage, the next stage changing cell at position 0;
2. a change at position 11;
3. a run of a single tile (cells of at most 32 points are taken when the cell form is forced);
4. a cell over more than two whole stages: stages without a change, the cell carried across them;
5. a last stage of 1, of 12 and of 5 source tiles (clouds live1, live12, live5);
6. a segment without a stage: NOT reachable -- every list's segments are rounded to ceil(stages / ceil(stages /
   segments)) by the plan (csrc/kmvp_plan.hpp), so none is empty; asserted, so that a plan that starts to leave one shows;
7. 1, 2, 4 and 8 tiles per wavefront, at 4 and 8 a fused launch with a REST list, at 8 one with a TAIL list, the shared
   build on and off, plain and normalised rows.

Each case also meets the parity suite's float32 tolerance against the float64 oracle on about 400 rows.
``fast_sqdists = 3``, ``cellmm_shape = 1`` and ``fast_tiles`` forced, as in tests/test_cellmm16_shared_build.py.
"""
import hashlib
import os

import numpy as np
import pytest

import c_oracle
import cellmm16_runs_cases as rc
from conftest import rel_err
from kernel_matrix_benchmarks_amd import _lib

TOL32 = 1e-5  # the float32 tolerance of the parity suite
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cellmm16_runs_parent.npz")
N_LIVE = {"live1": 1, "live12": 12, "live5": 5}
CASES = rc.cases()

_clouds, _oracle, _golden = {}, {}, {}


def cloud(name):
    if name not in _clouds:
        _clouds[name] = rc.make_cloud(name)
    return _clouds[name]


def oracle(name, norm):
    """float64 oracle on ~400 rows, once per (cloud, normalisation)"""
    if (name, norm) not in _oracle:
        y, b = cloud(name)
        rows = np.arange(0, len(y), max(1, len(y) // 400))
        want = c_oracle.product(kernel="gaussian", source_points=y.astype(np.float64), target_points=None,
                                source_signal=b.astype(np.float64), normalize_rows=norm, rows=rows)
        _oracle[name, norm] = (rows, want)
    return _oracle[name, norm]


def golden():
    if not _golden:
        with np.load(GOLDEN, allow_pickle=False) as z:
            _golden.update({k: z[k] for k in z.files})
    return _golden


def product(name, options, norm):
    y, b = cloud(name)
    ctx = _lib.Context(0)
    try:
        for k, v in {**rc.BASE, **options}.items():
            ctx.set_option(k, v)
        ctx.set_points(y, None, _lib.KMVP_F32)
        ctx.fit("gaussian")
        ctx.set_signal(b)
        ctx.run("gaussian", norm)
        assert ctx.last_kernel_name == "cellmm16_kernel", ctx.last_kernel_name
        return ctx.get_result(len(y), 1), ctx.cell_layout(), ctx.cell_lists()
    finally:
        ctx.close()


def check_pattern(name, options, layout, lists):
    """the edges of the module's docstring, from the layout and the lists the library read back"""
    tiles = options["fast_tiles"]
    p = rc.stage_pattern(layout, lists)
    print(f"  {p['m_stages']} stages of {len(p['tiles'])} source tiles, {p['seg_stages']} per MAIN segment, last stage {p['n_live']} tiles; "
          f"change at 0 in stages {p['change_at_0']}, at 11 in {p['change_at_11']}, carried {p['carried']}, shortest run {min(p['runs'])}; "
          f"blocks {lists['blocks']} segments {lists['segments']} fused {lists['fused']}")
    assert not layout["count_cut"] and layout["tiles_per_wavefront"] == tiles and layout["image"] == 1
    assert len(p["change_at_0"]) > 0, "no run ends with its stage"                                     # 1
    assert len(p["change_at_11"]) > 0, "no change at position 11"                                      # 2
    assert min(p["runs"]) == 1, "no run of a single tile"                                              # 3
    assert any(s + 1 in p["carried"] for s in p["carried"]), "no cell over two stages without a change"  # 4
    assert p["n_live"] == N_LIVE[name]                                                                 # 5
    assert p["empty_segments"] == 0                                                                    # 6
    b_main, b_tail, b_rest = lists["blocks"]                                                           # 7
    assert b_main > 0 and (lists["segments"][0] == 4 or options.get("segments") == 0)
    assert (b_rest > 0 and lists["fused"]) == (tiles >= 4), lists
    assert (b_tail >= 2 and lists["segments"][1] == 2 * lists["segments"][0] and lists["resident"] == 48) == ("cell_tail" in options), lists


@pytest.mark.gpu
@pytest.mark.parametrize("cid,name,options,norm", CASES, ids=[c[0] for c in CASES])
def test_sums_are_bitwise_the_parents(cid, name, options, norm):
    got, layout, lists = product(name, options, norm)
    check_pattern(name, options, layout, lists)
    assert np.all(np.isfinite(got)), cid
    rows, want = oracle(name, norm)
    err = rel_err(got[rows], want)
    sample = rc.sample_rows(len(got))
    g = golden()
    same_rows = np.array_equal(got[sample, 0], g[cid + "/rows"])
    same_all = hashlib.sha256(got.tobytes()).digest() == g[cid + "/sha256"].tobytes()
    print(f"  {cid}: sampled rows equal {same_rows}, whole output equal {same_all}, rel_err {err:.2e}")
    assert same_rows, (cid, float(np.max(np.abs(got[sample, 0] - g[cid + "/rows"]))))
    assert same_all, cid
    assert err <= TOL32, (cid, err)


def test_golden_holds_every_case():
    assert sorted(golden()) == sorted(f"{c[0]}/{what}" for c in CASES for what in ("rows", "sha256"))
    # the shared build never changed a sum (tests/test_cellmm16_shared_build.py): the parent's own two bodies agree
    for norm in ("plain", "norm"):
        assert np.array_equal(golden()[f"live1-t8-{norm}/sha256"], golden()[f"live1-t8-own-{norm}/sha256"])
