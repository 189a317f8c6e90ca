"""The TAIL list of cellmm16_kernel's fused grid (csrc/kmvp_plan.hpp: cell_tail_plan, cell_tail_split, fused_cell_work),
without a GPU: the header is plain C++, compiled here with the host compiler behind tests/host_cell_tail_shim.cpp.

The MAIN list's workgroups come in rounds of R resident workgroups; the target blocks of the last, partial round are cut
off as a third list whose segments are k times as many and k times shorter, so that they run at once beside the REST
list.  The kernel decodes its workgroup index with fused_cell_work() itself, and kmvp_product.hip plans with
cell_tail_split(), so what holds here holds on the device:

* the headline shape (the benchmark's config 2 on count-cut cells: 978 MAIN blocks x 8 segments, R = 512; 1598 short REST
  workgroups that weigh 35 of the MAIN list's) is pinned: 960 blocks stay, 18 take 24 segments of 109 stages, the grid is
  7680 + 432 + 1598;
* over a sweep of B, S, R, rest_grid and m_stages: every (target block, stage) pair is taken exactly once, b_full S is a
  multiple of R, TAIL + REST fit R, the TAIL's segments are a multiple of 8 within the cap, more than S, none empty and
  none shorter than the rule's minimum, every part of the grid starts at a multiple of 8, and every workgroup index is
  exactly one (list, block, segment);
* no TAIL without whole rounds, without blocks left over, when k < 2, when the launch is not fused, at two tiles per
  wavefront or fewer, or when the option says so; the slots and the regions of the partial sums of the three lists
  tile their buffers in the order MAIN, TAIL, REST.
"""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from cell_balance_cases import fine_keys, headline_points

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "kernel_matrix_benchmarks_amd", "csrc")
i64, i32, vp = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p
P64 = ctypes.POINTER(i64)

# run_product_cellmm's rule: stages of 12 source tiles and 8192 bytes, segments of >= 2 stages and <= 3 MiB, 7168 workgroups
CMM_RULE = dict(stage_tiles=12, stage_bytes=8192, min_seg=2, l2_seg_bytes=3 << 20, target_blocks=7168)
LIST_FIELDS = ("blocks", "segments", "seg_stages", "slots", "slot_base", "region_offset")
MAIN, REST, TAIL = 0, 1, 2


@pytest.fixture(scope="module")
def plan():
    tmp = tempfile.mkdtemp(prefix="kmvp_host_tail_")
    so = os.path.join(tmp, "libhost_tail.so")
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC,
                           os.path.join(HERE, "host_cell_tail_shim.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.ht_constants.argtypes = [P64]
    lib.ht_count_cut_lists.argtypes = [vp, i64, i32, i32, P64, P64, P64]
    lib.ht_tail_plan.argtypes = [i64, i32, i64, i64, i64, i64, P64]
    lib.ht_tail_taken.argtypes = [i32, i32, i32, i64, i64]
    lib.ht_lists.argtypes = [i64, i64, i64, i64, i32, i32, i32, i64, i64, i64, i64, i32, i32, i64, P64]
    lib.ht_fused_cell_work.argtypes = [i64, i64, i64, i64, vp, vp]
    yield lib
    shutil.rmtree(tmp, ignore_errors=True)


def constants(plan):
    out = (i64 * 5)()
    plan.ht_constants(out)
    return dict(zip(("max_segments", "rest_tt", "waves", "cell_tile", "auto"), out))


def tail_plan(plan, B, S, R, m_stages, rest_grid, min_seg):
    out = (i64 * 4)()
    plan.ht_tail_plan(B, S, R, m_stages, rest_grid, min_seg, out)
    return dict(zip(("b_full", "b_tail", "segments", "seg_stages"), out))


def lists(plan, n_points, m_tiles, n_main, n_rest, tt, take_tail, resident, opt_fused=-1, opt_segments=0):
    out = (i64 * 27)()
    r = CMM_RULE
    plan.ht_lists(n_points, m_tiles, n_main, n_rest, tt, opt_segments, r["stage_tiles"], r["stage_bytes"], r["min_seg"],
                  r["l2_seg_bytes"], r["target_blocks"], opt_fused, take_tail, resident, out)
    g = dict(zip(("tail", "fused", "main_grid", "tail_grid", "rest_grid", "total", "m_stages", "n_slots"), out[:8]))
    for l in range(3):
        g[l] = dict(zip(LIST_FIELDS, out[8 + 6 * l:14 + 6 * l]))
    g["part_doubles"] = out[26]
    return g


def work(plan, total, main_grid, tail_grid):
    lst, loc = np.zeros(total, np.int64), np.zeros(total, np.int64)
    plan.ht_fused_cell_work(0, total, main_grid, tail_grid, lst.ctypes.data, loc.ctypes.data)
    return lst, loc


def block_to_work(bid, segments, tile_blocks):
    """csrc/kmvp_lowd.hpp block_to_work(): workgroup of a list's own grid -> (target block, segment)"""
    if segments % 8 == 0:
        q = bid >> 3
        return q % tile_blocks, (bid & 7) + 8 * (q // tile_blocks)
    return bid // segments, bid % segments  # (bid: an array of indices)


def check_grid(plan, B, S, m_stages, rest_grid, t):
    """the fused grid MAIN (b_full blocks, S segments), TAIL (t), REST (rest_grid workgroups): one (list, block, segment) per
    workgroup index, and every (target block, stage) pair of the B blocks exactly once"""
    main_grid, tail_grid = t["b_full"] * S, t["b_tail"] * t["segments"]
    total = main_grid + tail_grid + rest_grid
    lst, loc = work(plan, total, main_grid, tail_grid)
    bid = np.arange(total)
    assert np.array_equal(lst, np.where(bid < main_grid, MAIN, np.where(bid < main_grid + tail_grid, TAIL, REST)))
    assert np.array_equal(loc, bid - np.where(lst == MAIN, 0, np.where(lst == TAIL, main_grid, main_grid + tail_grid)))
    assert len(set(zip(lst.tolist(), loc.tolist()))) == total
    # a list's workgroups are every (block, segment) of it once, and its segments [seg seg_stages, (seg + 1) seg_stages) cut
    # [0, m_stages) into non-empty pieces: together, every (target block, stage) pair of the B blocks exactly once
    assert t["b_full"] + t["b_tail"] == B
    for which, blocks, segs, seg_stages in ((MAIN, t["b_full"], S, -(-m_stages // S)),
                                           (TAIL, t["b_tail"], t["segments"], t["seg_stages"])):
        local = loc[lst == which]
        assert len(local) == blocks * segs
        if blocks == 0:
            continue
        tb, seg = block_to_work(local, segs, blocks)
        assert tb.min() >= 0 and tb.max() < blocks and seg.min() >= 0 and seg.max() < segs
        assert np.array_equal(np.sort(tb * segs + seg), np.arange(blocks * segs)), (B, S, m_stages, rest_grid, t)
        assert (segs - 1) * seg_stages < m_stages <= segs * seg_stages, (B, S, m_stages, rest_grid, t)
    if t["b_tail"]:  # the XCD of a workgroup (index modulo 8) is the one it has in its own list's grid
        assert main_grid % 8 == 0 and tail_grid % 8 == 0
        assert np.array_equal(loc[lst != MAIN] & 7, bid[lst != MAIN] & 7)


def settled(m_stages, S):
    """S as cell_split leaves it: segments of whole stages, none empty"""
    seg_stages = -(-m_stages // S)
    return -(-m_stages // seg_stages)


def test_sweep(plan):
    k = constants(plan)
    cap = k["max_segments"]
    seen = dict(tail=0, none=0, no_full=0, no_left=0, k1=0, short=0)
    for R in (16, 32, 96, 512):
        for S0 in (1, 2, 3, 4, 8, 16, 24, 32, 64):
            for m_stages in (5, 16, 33, 109, 327):
                S = settled(m_stages, min(S0, m_stages))
                for B in sorted({1, 2, 3, 5, 8, 13, 16, 18, 31, 32, 33, 64, 67, 100, R // S, R // S + 1, 2 * R + 3} - {0}):
                    for rest_grid in (0, 1, 7, 34, R - 8, R):
                        for min_seg in (1, 2):
                            t = tail_plan(plan, B, S, R, m_stages, rest_grid, min_seg)
                            assert t["b_full"] + t["b_tail"] == B
                            check_grid(plan, B, S, m_stages, rest_grid, t)
                            q = R // np.gcd(R, S)
                            if t["b_tail"] == 0:
                                assert t["b_full"] == B and t["segments"] == 0
                                seen["none"] += 1
                                seen["no_full"] += B < q
                                seen["no_left"] += B % q == 0
                                seen["k1"] += B >= q and B % q != 0 and (B % q) * S * 2 + rest_grid > R
                                continue
                            seen["tail"] += 1
                            seen["short"] += m_stages < S * ((R - rest_grid) // (t["b_tail"] * S))
                            assert t["b_full"] > 0 and (t["b_full"] * S) % R == 0 and t["b_full"] == B // q * q
                            assert t["b_tail"] * t["segments"] + rest_grid <= R
                            assert t["segments"] % 8 == 0 and S < t["segments"] <= cap
                            assert t["segments"] <= S * ((R - rest_grid) // (t["b_tail"] * S))  # at most S k
                            assert (R - rest_grid) // (t["b_tail"] * S) >= 2
                            assert t["seg_stages"] == -(-m_stages // t["segments"]) and t["seg_stages"] >= min_seg
                            assert -(-m_stages // t["seg_stages"]) == t["segments"]  # no empty segment
    print(seen)
    assert all(v > 0 for v in seen.values()), seen


def test_no_tail_conditions(plan):
    k = constants(plan)
    assert tail_plan(plan, 978, 8, 512, 2616, 34, 2)["b_tail"] == 18
    assert tail_plan(plan, 63, 8, 512, 2616, 34, 2)["b_tail"] == 0    # B < R / S: no whole round
    assert tail_plan(plan, 960, 8, 512, 2616, 34, 2)["b_tail"] == 0   # whole rounds alone
    assert tail_plan(plan, 992, 8, 512, 2616, 34, 2)["b_tail"] == 0   # 32 blocks left: 2 x 256 + 34 > 512, k = 1
    assert tail_plan(plan, 991, 8, 512, 2616, 34, 2)["b_tail"] == 0   # 31 left: 496 + 34 > 512
    assert tail_plan(plan, 989, 8, 512, 2616, 34, 2) == dict(b_full=960, b_tail=29, segments=16, seg_stages=164)
    assert tail_plan(plan, 961, 8, 512, 2616, 34, 2)["segments"] == k["max_segments"] == 64  # k = 59: the cap
    assert tail_plan(plan, 978, 8, 512, 20, 34, 2)["b_tail"] == 0     # 20 stages of >= 2: 10 segments at most, settled 8 = S
    assert tail_plan(plan, 978, 8, 512, 2616, 512, 2)["b_tail"] == 0  # the REST list fills the round
    # the option, the launch, the tile count
    big, small = (500000, 100000), (499999, 100000)
    for tt in (1, 2, 4, 8):
        for N, M in (big, small, (40000, 40000)):
            assert plan.ht_tail_taken(0, tt, 1, N, M) == 0 and plan.ht_tail_taken(1, tt, 0, N, M) == 0 and plan.ht_tail_taken(-1, tt, 0, N, M) == 0
            assert plan.ht_tail_taken(1, tt, 1, N, M) == int(tt > k["rest_tt"])
        # automatic: eight tiles per wavefront, from the sizes from which cellmm16_kernel is taken by itself
        assert plan.ht_tail_taken(-1, tt, 1, *big) == int(k["auto"] and tt == 8)
        assert plan.ht_tail_taken(-1, tt, 1, *small) == 0 and plan.ht_tail_taken(-1, tt, 1, 500000, 99999) == 0
    assert k["auto"] == 1


def check_buffers(g):
    """slots and regions of the lists tile their buffers in the order MAIN, TAIL, REST"""
    at_slot = at_region = 0
    for l in (MAIN, TAIL, REST):
        assert g[l]["slot_base"] == at_slot and g[l]["region_offset"] == at_region, (l, g)
        at_slot += g[l]["slots"]
        at_region += g[l]["segments"] * g[l]["slots"]
    assert at_slot == g["n_slots"] and at_region == g["part_doubles"]


def test_headline_shape(plan):
    """the benchmark's config 2 (1e6 uniform points) on count-cut cells, 256 CUs x 2 resident workgroups"""
    keyed = fine_keys(headline_points())
    fine = np.ascontiguousarray(keyed["fine"], np.uint32)
    m_tiles, n_main, n_rest = i64(), i64(), i64()
    plan.ht_count_cut_lists(fine.ctypes.data, len(fine), keyed["cap"], 8, ctypes.byref(m_tiles), ctypes.byref(n_main), ctypes.byref(n_rest))
    m_tiles, n_main, n_rest = m_tiles.value, n_main.value, n_rest.value
    assert (m_tiles, n_main, n_rest) == (31298, 31296, 136)  # tests/test_host_cell_balance.py::test_headline_shape
    off = lists(plan, len(fine), m_tiles, n_main, n_rest, 8, 0, 512)
    assert (off["tail"], off["fused"], off["main_grid"], off["tail_grid"], off["rest_grid"], off["total"]) == (0, 1, 7824, 0, 1598, 9422)
    assert (off[MAIN]["blocks"], off[MAIN]["segments"], off[MAIN]["seg_stages"], off["m_stages"]) == (978, 8, 327, 2609)
    assert off[TAIL] == dict(blocks=0, segments=0, seg_stages=1, slots=0, slot_base=off[MAIN]["slots"], region_offset=8 * off[MAIN]["slots"])
    check_buffers(off)
    on = lists(plan, len(fine), m_tiles, n_main, n_rest, 8, 1, 512)
    assert on["tail"] == 1 and on["fused"] == 1
    assert (on[MAIN]["blocks"], on[TAIL]["blocks"], on[TAIL]["segments"], on[TAIL]["seg_stages"]) == (960, 18, 24, 109)
    assert (on["main_grid"], on["tail_grid"], on["rest_grid"], on["total"]) == (7680, 432, 1598, 9710)
    assert (0, on["main_grid"], on["main_grid"] + on["tail_grid"]) == (0, 7680, 8112)  # where MAIN, TAIL and REST start
    # the REST list is 17 blocks x 94 segments of 28 stages x 2 tiles per wavefront: by number more than a round, by work
    # ceil(1598 x 28 x 2 / (327 x 8)) = 35 workgroups of the MAIN list's length (cell_rest_weight), and that is what the plan
    # keeps free beside the TAIL
    assert (off[REST]["blocks"], off[REST]["segments"], off[REST]["seg_stages"]) == (17, 94, 28)
    rest_weight = -(-1598 * 28 * 2 // (327 * 8))
    assert rest_weight == 35 and on["main_grid"] % 512 == 0 and on["tail_grid"] + rest_weight <= 512
    assert on[REST] == dict(off[REST], region_offset=on[REST]["region_offset"]) and on[MAIN]["segments"] == 8
    assert on[MAIN]["slots"] + on[TAIL]["slots"] == off[MAIN]["slots"] and on[TAIL]["slot_base"] == 960 * 1024
    assert on[REST]["slot_base"] == off[REST]["slot_base"] == n_main * 32 and on["n_slots"] == off["n_slots"]
    check_buffers(on)
    t = dict(b_full=960, b_tail=18, segments=24, seg_stages=109)
    assert tail_plan(plan, 978, 8, 512, on["m_stages"], rest_weight, 2) == t
    check_grid(plan, 978, 8, on["m_stages"], on["rest_grid"], t)
    # not fused, or not asked for: the two lists as they were
    assert lists(plan, len(fine), m_tiles, n_main, n_rest, 8, 1, 512, opt_fused=0) == dict(off, fused=0)
    # other devices: 304 CUs -> rounds of 608 = 76 blocks: 912 stay, 66 x 8 = 528 workgroups are left, k = 1: no TAIL
    assert lists(plan, len(fine), m_tiles, n_main, n_rest, 8, 1, 608)["tail"] == 0
