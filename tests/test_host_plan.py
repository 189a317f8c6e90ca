"""The launch plans of csrc/kmvp_plan.hpp, without a GPU: the header is plain C++, compiled here with the host compiler
behind tests/host_plan_shim.cpp.

* The staged paths' geometry (padded sizes, segments, grid) reproduces tests/golden/host_plan.json entry by entry: the
  numbers the commit before the plans were factored out computed in its four runners (the file says how they were
  recorded).  The segment count fixes the order of the fp64 partial sums, so this is part of bitwise reproducibility.
* The tile lists of the cell kernels are what the kernels assume, and cell_split_count() -- which prices lists that
  cell_tiles_split() builds -- agrees with the lists actually built.
"""
import ctypes
import hashlib
import json
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

from host_plan_cases import CELL_TILE, CELL_TT, GRID_M, GRID_N, GRID_OPT, key_sequences

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "kernel_matrix_benchmarks_amd", "csrc")
i64, i32, vp = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p
P64 = ctypes.POINTER(i64)


@pytest.fixture(scope="module")
def plan():
    tmp = tempfile.mkdtemp(prefix="kmvp_host_plan_")
    so = os.path.join(tmp, "libhost_plan.so")
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC,
                           os.path.join(HERE, "host_plan_shim.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    lib.hp_constants.argtypes = [P64]
    lib.hp_settle_segments.argtypes = [i64, i32]
    lib.hp_plan_stages.argtypes = [i64, i64, i32, i32, i32, i32, i64, i64, i64, i64, i32, P64]
    lib.hp_cell_split.argtypes = [i64, i64, i64, i64, i32, i32, i32, i32, i64, i64, i64, i64, P64]
    lib.hp_cell_split_count.argtypes = [vp, i64, i32, P64, P64]
    lib.hp_cell_tiles_split.argtypes = [vp, i64, i32, vp, i64, P64, P64]
    lib.hp_cell_tiles_split.restype = i64
    lib.hp_cell_tiles.argtypes = [vp, i64, i32, vp, i64]
    lib.hp_cell_tiles.restype = i64
    lib.hp_key_runs.argtypes = [vp, i64, vp, i64]
    lib.hp_key_runs.restype = i64
    yield lib
    shutil.rmtree(tmp, ignore_errors=True)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "host_plan.json")) as f:
        return json.load(f)


def constants(plan):
    out = (i64 * 6)()
    plan.hp_constants(out)
    return dict(zip(("waves", "cell_tile", "rest_tt", "small_targets", "seg_split_from", "max_grid"), out))


def test_grid_is_the_recorded_one(golden):
    assert golden["N"] == GRID_N and golden["M"] == GRID_M and golden["opt_segments"] == GRID_OPT
    assert {v["path"] for v in golden["stage_variants"]} == {"fast", "fastmm", "cfast", "cfastmm"}
    assert {(c["sequence"], c["TT"]) for c in golden["cell_lists"]} == {(n, t) for n, _ in key_sequences() for t in CELL_TT}


def test_settle_segments_as_recorded(plan, golden):
    s = golden["settle"]
    got = [[plan.hp_settle_segments(u, seg) for seg in s["seg"]] for u in s["units"]]
    assert got == s["values"]


def test_staged_plans_as_recorded(plan, golden):
    """Every (variant, N, M, segments option): n_pad, tile_blocks, m_stages, segments, seg_stages, grid as recorded; the
    refusal exactly where the grid exceeds what a launch takes."""
    k = constants(plan)
    out = (i64 * 8)()
    for v in golden["stage_variants"]:
        rows = []
        for N in golden["N"]:
            for M in golden["M"]:
                m_stages = (M + v["stage_sources"] - 1) // v["stage_sources"]
                for opt in golden["opt_segments"]:
                    # TT tiles per wave requested (the recorded runs fix TT); the rule for few targets is the plan's own
                    plan.hp_plan_stages(N, m_stages, v["TT"], v["TT"], v["TT"], opt, v["stage_bytes"], v["min_seg"],
                                        v["l2_seg_bytes"], v["target_blocks"], v["cols"], out)
                    row = list(out)[:6]
                    assert out[7] == v["TT"]
                    assert bool(out[6]) == (row[5] <= k["max_grid"]), (v["path"], N, M, opt)
                    assert row[3] >= 1 and row[4] * row[3] >= row[2] and row[4] * (row[3] - 1) < row[2], (v, N, M, opt, row)
                    rows.append(row)
        if "rows" in v:  # the variants recorded in full tell WHERE a plan differs
            for got, want in zip(rows, v["rows"]):
                assert got == want, (v["path"], v["example"], got, want)
        digest = hashlib.sha256("".join(",".join(str(x) for x in r) + "\n" for r in rows).encode()).hexdigest()
        assert digest == v["sha256"], (v["path"], v["example"], v["TT"])


def test_tiles_per_wave(plan):
    """as requested up to what is instantiated; else one tile for few targets, else the path's default"""
    k = constants(plan)
    out = (i64 * 8)()
    for N in (1, k["small_targets"] - 1, k["small_targets"], 10**6):
        for opt, tt_max, tt_default in ((0, 4, 4), (0, 2, 4), (0, 4, 2), (1, 4, 4), (4, 2, 2), (8, 4, 2), (2, 4, 4)):
            plan.hp_plan_stages(N, 100, opt, tt_max, tt_default, 0, 4096, 4, 2 << 20, 16384, 1, out)
            want = min(opt, tt_max) if opt > 0 else (1 if N < k["small_targets"] else min(tt_default, tt_max))
            assert out[7] == want and out[0] == -(-N // (128 * want)) * 128 * want, (N, opt, tt_max, tt_default)


def test_cell_split_as_recorded(plan, golden):
    """the two launches of the float32 cell kernels: blocks, slots and each launch's own segments"""
    out = (i64 * 10)()
    for args, want in golden["cell_split"]["rows"]:
        plan.hp_cell_split(*args, out)
        assert list(out) == want, args


def build_split(plan, keys, TT):
    cap = 3 * (len(keys) + 64 * (len(keys) // 16 + 64))
    out = np.zeros(cap, np.int32)
    nm, nr = i64(), i64()
    G = plan.hp_cell_tiles_split(keys.ctypes.data, len(keys), TT, out.ctypes.data, cap, ctypes.byref(nm), ctypes.byref(nr))
    assert G >= 0 and G == nm.value + nr.value
    return out[: 3 * G].copy(), nm.value, nr.value


def check_cover(keys, start, count, tkey, tile):
    """every position in exactly one tile, no tile across a key change, every tile inside the array"""
    n = len(keys)
    hits = np.zeros(n, np.int64)
    for s, c, k in zip(start, count, tkey):
        assert 0 <= c <= tile and 0 <= s and s + c <= n
        if n:
            assert s < n and keys[s] == k  # (an empty tile still names a point of its cell)
        hits[s:s + c] += 1
        assert np.all(keys[s:s + c] == k)
    assert np.all(hits == 1)


@pytest.mark.parametrize("TT", CELL_TT)
def test_split_lists_are_what_the_kernels_assume(plan, golden, TT):
    k = constants(plan)
    assert k["cell_tile"] == CELL_TILE
    recorded = {(c["sequence"], c["TT"]): c for c in golden["cell_lists"]}
    for name, keys in key_sequences():
        keys = np.ascontiguousarray(keys, np.uint32)
        flat, n_main, n_rest = build_split(plan, keys, TT)
        G = n_main + n_rest
        start, count, tkey = flat[:G], flat[G:2 * G], flat[2 * G:].view(np.uint32)
        check_cover(keys, start, count, tkey, CELL_TILE)
        # whole workgroups of 4 wavefronts x TT (main) or 2 (rest) tiles; a wavefront's tiles share their cell
        assert n_main % (TT * k["waves"]) == 0 and n_rest % (k["rest_tt"] * k["waves"]) == 0
        for lo, hi, group in ((0, n_main, TT), (n_main, G, k["rest_tt"])):
            g = tkey[lo:hi].reshape(-1, group)
            assert np.all(g == g[:, :1])
        # the live tiles are the cells' tiles, everything else is padding without a point
        sizes = np.diff(np.flatnonzero(np.r_[True, keys[1:] != keys[:-1], True])) if len(keys) else np.zeros(0, np.int64)
        assert int(np.count_nonzero(count)) == int(np.sum((sizes + CELL_TILE - 1) // CELL_TILE))
        if len(keys) == 0:
            assert G == 0
        # what cell_prepare's auto choice prices is what gets built
        cm, cr = i64(), i64()
        plan.hp_cell_split_count(keys.ctypes.data, len(keys), TT, ctypes.byref(cm), ctypes.byref(cr))
        up = lambda v, q: (v + q - 1) // q * q
        assert up(cm.value, TT * k["waves"]) == n_main and up(cr.value, k["rest_tt"] * k["waves"]) == n_rest, (name, TT)
        if TT <= k["rest_tt"]:
            assert n_rest == 0
        # byte for byte the lists of the commit before the refactor
        want = recorded[(name, TT)]
        assert (n_main, n_rest) == (want["n_main"], want["n_rest"]), (name, TT)
        assert hashlib.sha256(flat.tobytes()).hexdigest() == want["sha256"], (name, TT)


@pytest.mark.parametrize("tile", [32, 64])
def test_plain_list_and_key_runs(plan, tile):
    for name, keys in key_sequences():
        keys = np.ascontiguousarray(keys, np.uint32)
        cap = 3 * (len(keys) + 64)
        out = np.zeros(cap, np.int32)
        G = plan.hp_cell_tiles(keys.ctypes.data, len(keys), tile, out.ctypes.data, cap)
        assert G >= 0
        start, count, tkey = out[:G], out[G:2 * G], out[2 * G:3 * G].view(np.uint32)
        check_cover(keys, start, count, tkey, tile)
        assert np.all(count > 0)
        runs = np.zeros(cap, np.int64)
        R = plan.hp_key_runs(keys.ctypes.data, len(keys), runs.ctypes.data, cap)
        r = runs[: 3 * R].reshape(-1, 3)
        edges = np.flatnonzero(np.r_[True, keys[1:] != keys[:-1], True]) if len(keys) else np.zeros(1, np.int64)
        assert np.array_equal(r[:, 0], edges[:-1]) and np.array_equal(r[:, 1], np.diff(edges))
        assert np.array_equal(r[:, 2], keys[edges[:-1]].astype(np.int64))
        assert G == int(np.sum((r[:, 1] + tile - 1) // tile))
