"""The integer rules of DBSCAN's rounds and of its renumbering (csrc/kmvp_dbscan_step.hpp: initial label, hook, chase, root
flag, core_of, label) without a GPU: the header is plain C++ behind a macro for the device attributes, compiled here with
the host compiler behind tests/host_dbscan_step_shim.cpp.  The sweep -- nxt[i] = the smallest label among i's inside core
points -- is restated in numpy on a given inside set; the rounds built from the header's rules are held to the union-find of
tests/dbscan_reference.py on small forests, long descending chains included."""
import ctypes
import os
import shutil
import subprocess
import tempfile

import numpy as np
import pytest

import dbscan_reference as dr

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "kernel_matrix_benchmarks_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    tmp = tempfile.mkdtemp(prefix="kmvp_host_dbscan_step_")
    so = os.path.join(tmp, "libhost_dbscan_step.so")
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler is needed"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-shared", "-fPIC", "-I", CSRC,
                           os.path.join(HERE, "host_dbscan_step_shim.cpp"), "-o", so])
    lib = ctypes.CDLL(so)
    p, n = ctypes.c_void_p, ctypes.c_int64
    lib.hs_none.restype = ctypes.c_int
    lib.hs_init.restype = None
    lib.hs_init.argtypes = [p, n, p, n]
    lib.hs_hook.restype = n
    lib.hs_hook.argtypes = [p, p, p, p, n]
    lib.hs_chase.restype = None
    lib.hs_chase.argtypes = [p, p, n]
    lib.hs_renumber.restype = n
    lib.hs_renumber.argtypes = [p, p, p, p, p, p, n]
    yield lib
    shutil.rmtree(tmp, ignore_errors=True)


NONE = 2 ** 31 - 1


def sweep(inside, lab):
    """nxt[i] for a core point: the smallest label among its inside core points (itself included)."""
    masked = np.where(inside & (lab != NONE)[None, :], lab[None, :], NONE)
    return np.where(lab != NONE, masked.min(axis=1), NONE).astype(np.int32)


def run(lib, inside, s, min_samples, rs=None):
    """kmvp_dbscan.hip's steps on the header's rules: (labels, core_of, counts, rounds)."""
    N = len(inside)
    counts = inside.sum(axis=1).astype(np.int64)
    lab, par = np.empty(N, dtype=np.int32), np.empty(N, dtype=np.int32)
    lib.hs_init(counts.ctypes.data, min_samples, lab.ctypes.data, N)
    assert np.array_equal(lab != NONE, counts >= min_samples)
    rounds = 0
    while np.any(lab != NONE):
        rounds += 1
        assert rounds <= N
        core = lab != NONE
        assert np.all(lab[core] <= np.flatnonzero(core)) and np.all(lab[lab[core]] == lab[core])  # labels are roots
        nxt = sweep(inside, lab)
        assert np.all(nxt[core] <= lab[core])
        order = np.arange(N, dtype=np.int64) if rs is None else rs.permutation(N).astype(np.int64)
        asked = lib.hs_hook(lab.ctypes.data, nxt.ctypes.data, par.ctypes.data, order.ctypes.data, N)
        if rs is not None:  # the hook's result is a pure minimum: another order of the requests, the same par
            other, par2 = np.ascontiguousarray(order[::-1]), np.empty_like(par)
            assert lib.hs_hook(lab.ctypes.data, nxt.ctypes.data, par2.ctypes.data, other.ctypes.data, N) == asked
            assert np.array_equal(par, par2)
        assert np.all(par[core] <= lab[core]) and np.all(par[~core] == NONE)
        before = lab.copy()
        lib.hs_chase(par.ctypes.data, lab.ctypes.data, N)
        assert np.all(lab <= before)
        if asked == 0:
            assert np.array_equal(lab, before)
            break
        assert np.unique(lab[core]).size < np.unique(before[core]).size  # every other round removes a root
    # the border rule on the given s, as the BORDER walk leaves it
    core = lab != NONE
    attach = np.full(N, -1, dtype=np.int32)
    for i in np.flatnonzero(~core):
        cand = np.flatnonzero(inside[i] & core)
        if cand.size:
            attach[i] = cand[np.lexsort((cand, s[i, cand]))[0]]
    flag, cid = np.empty(N, dtype=np.int32), np.empty(N, dtype=np.int32)
    labels, core_of = np.empty(N, dtype=np.int64), np.empty(N, dtype=np.int64)
    C = lib.hs_renumber(lab.ctypes.data, attach.ctypes.data, flag.ctypes.data, cid.ctypes.data, labels.ctypes.data,
                        core_of.ctypes.data, N)
    assert C == (labels.max() + 1 if N else 0)
    return labels, core_of, counts, rounds


def same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got[:3], want[:3]))


def test_the_sentinel_is_int32_max(lib):
    assert lib.hs_none() == NONE


@pytest.mark.parametrize("seed", range(6))
def test_random_graphs_equal_the_union_find(lib, seed):
    rs = np.random.RandomState(seed)
    N = 150
    x = rs.randint(0, 24, size=(N, 2))
    inside, s = dr.inside_lattice(x, 5)
    for min_samples in (1, 3, 5, 50):
        got = run(lib, inside, s, min_samples, rs)
        assert same(got, dr.dbscan(inside, s, min_samples)), (seed, min_samples)
        assert (got[3] == 0) == (not np.any(got[2] >= min_samples))


@pytest.mark.parametrize("order", ["ascending", "descending", "random"])
def test_long_chains(lib, order):
    """A path of 600 points in which only neighbours on the line are inside, indexed along the line, against it, and at
    random: one cluster rooted at the smallest core index, in few rounds although the labels have far to travel."""
    x, R = dr.chain(order, n=600, seed=3)
    inside, s = dr.inside_dense(x, R)
    labels, core_of, counts, rounds = run(lib, inside, s, 3, np.random.RandomState(0))
    assert same((labels, core_of, counts), dr.dbscan(inside, s, 3))
    assert np.all(labels == 0) and (core_of != np.arange(600)).sum() == 2
    print(f"chain of 600, {order}: {rounds} rounds")
    assert rounds <= 600
    if order == "ascending":
        assert rounds == 2  # every root hooks to its left neighbour in the first round: one chain in par, chased at once


def test_forest_of_descending_hooks(lib):
    """par as one round's hook may leave it: a descending chain of roots 9 -> 7 -> 4 -> 0 with leaves on every root."""
    par = np.array([0, 0, 0, NONE, 0, 4, 4, 4, 7, 7, 9, 9], dtype=np.int32)
    lab = np.full(12, -5, dtype=np.int32)
    lib.hs_chase(par.ctypes.data, lab.ctypes.data, 12)
    assert lab.tolist() == [0, 0, 0, -5, 0, 0, 0, 0, 0, 0, 0, 0]  # a point that is no core point is not touched


def test_renumbering_in_ascending_order_of_the_roots(lib):
    #                 0  1     2  3  4     5   6
    lab = np.array([NONE, 1, NONE, 1, 4, NONE, 4], dtype=np.int32)
    attach = np.array([6, -7, -1, -7, -7, 3, -7], dtype=np.int32)  # (a core point's entry is never read)
    flag, cid = np.empty(7, dtype=np.int32), np.empty(7, dtype=np.int32)
    labels, core_of = np.empty(7, dtype=np.int64), np.empty(7, dtype=np.int64)
    C = lib.hs_renumber(lab.ctypes.data, attach.ctypes.data, flag.ctypes.data, cid.ctypes.data, labels.ctypes.data,
                        core_of.ctypes.data, 7)
    assert C == 2 and flag.tolist() == [0, 1, 0, 0, 1, 0, 0]
    assert core_of.tolist() == [6, 1, -1, 3, 4, 3, 6] and labels.tolist() == [1, 0, -1, 0, 1, 0, 1]
