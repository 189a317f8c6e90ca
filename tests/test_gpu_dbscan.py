"""GPU tests of DBSCAN on the cell list (include/kmvp.h kmvp_dbscan; lowd_cutoff_label_kernel between the integer rules of
csrc/kmvp_dbscan_step.hpp, driver csrc/kmvp_dbscan.hip).

The definition is canonical -- core counts, components of the core points rooted at their smallest index, border points to
their nearest inside core point -- so there is no tolerance anywhere in this file: labels, core_of and counts are held to
tests/dbscan_reference.py with array_equal.  What decides whether a pair is inside is, per test: integer arithmetic (the
lattices, with pairs exactly on the boundary), float64 on clouds without an ambiguous pair (asserted on the CPU in
tests/test_dbscan_reference.py), or the library's own radius search."""
import numpy as np
import pytest

import dbscan_reference as dr
from kernel_matrix_benchmarks_amd import _lib
from kernel_matrix_benchmarks_amd.algorithms.mi355x import MI355XDBSCAN

pytestmark = pytest.mark.gpu

PREC = {"f32": np.float32, "f64": np.float64}
UNSUPPORTED, INVALID = 2, 1
KERNEL = "lowd_cutoff_label_kernel"


class Ctx:
    """One context whose targets are its sources."""

    def __init__(self, x, precision, **options):
        self.precision = np.float64 if np.dtype(precision) == np.float64 else np.float32
        self.dtype = _lib.KMVP_F64 if self.precision == np.float64 else _lib.KMVP_F32
        self.ctx = _lib.Context(0)
        try:
            for key, value in options.items():
                self.ctx.set_option(key, value)
            self.ctx.set_points(np.ascontiguousarray(x, dtype=self.precision), None, self.dtype)
        except Exception:
            self.ctx.close()
            raise

    def dbscan(self, R, min_samples):
        labels, core_of, counts, info = self.ctx.dbscan(R, min_samples)
        N = self.ctx.N
        assert labels.shape == core_of.shape == counts.shape == (N,) and labels.dtype == core_of.dtype == counts.dtype == np.int64
        assert self.ctx.last_kernel_name == KERNEL and self.ctx.last_dispatch_note == ""
        assert self.ctx.last_kernel_ms > 0 and self.ctx.last_total_ms >= self.ctx.last_kernel_ms
        # the info words are what the arrays imply, and the walks are the count, the rounds and the border walk
        want = dr.summary(labels, core_of)
        assert {k: info[k] for k in want} == want, (info, want)
        assert info["n_core"] + info["n_border"] + info["n_noise"] == N
        border_walk = 0 < info["n_core"] < N
        assert info["walks"] == 1 + info["rounds"] + border_walk and (info["rounds"] >= 1) == (info["n_core"] > 0), info
        return labels, core_of, counts, info

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.ctx.close()


def same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got[:3], want[:3]))


def partition(labels):
    """The clustering as a set of frozensets, noise apart: what a renumbering leaves alone."""
    return {frozenset(np.flatnonzero(labels == c).tolist()) for c in np.unique(labels[labels >= 0])}, \
        frozenset(np.flatnonzero(labels < 0).tolist())


_reference = {}


def reference(name):
    """The float64 reference of a named cloud, computed once per session and only read."""
    if name not in _reference:
        x, R, min_samples = dr.cloud(name)
        inside, s = dr.inside_dense(x, R)
        _reference[name] = (x, R, min_samples, dr.dbscan(inside, s, min_samples))
    return _reference[name]


# ---- 1. lattices: integer arithmetic is the judge ---------------------------------------------------------------------------
@pytest.mark.parametrize("prec", list(PREC))
@pytest.mark.parametrize("name", dr.LATTICES)
def test_lattices_equal_integer_arithmetic_at_every_cell_factor(name, prec):
    k, x, R, r2, min_samples = dr.lattice(name)
    inside, s = dr.inside_lattice(k, r2)
    want = dr.dbscan(inside, s, min_samples)
    assert np.any(s == r2) and dr.summary(want[0], want[1])["n_clusters"] >= 2 and len(dr.torn_borders(inside, *want[:2])) > 0
    for factor in (1.0, 1.5, 2.0):
        with Ctx(x, PREC[prec], cutoff_cell_factor=factor) as c:
            got = c.dbscan(R, min_samples)
        assert same(got, want), (name, prec, factor)


# ---- 2. blobs plus uniform noise: float64 is the judge ------------------------------------------------------------------------
@pytest.mark.parametrize("prec", list(PREC))
@pytest.mark.parametrize("name", dr.BLOBS)
def test_blobs_equal_the_float64_reference(name, prec):
    x, R, min_samples, want = reference(name)
    assert len(x) % 64 != 0
    with Ctx(x, PREC[prec]) as c:
        labels, core_of, counts, info = c.dbscan(R, min_samples)
        assert np.array_equal(counts, c.ctx.radius_count(R))  # the count's own bits
    assert same((labels, core_of, counts), want), (name, prec, info)
    assert np.array_equal(core_of == np.arange(len(x)), counts >= min_samples)
    assert info["n_clusters"] >= 3 and info["n_border"] > 0 and info["n_noise"] > 0, info


# ---- 3. the library's own neighbour lists are the judge -----------------------------------------------------------------------
@pytest.mark.parametrize("prec", list(PREC))
def test_equals_the_reference_on_the_librarys_own_lists(prec):
    x, R, min_samples = dr.cloud("uniform3")
    with Ctx(x, PREC[prec]) as c:
        assert c.ctx.radius_count(R).max() <= 16
        idx, sq = c.ctx.radius_nearest(R, 16)
        got = c.dbscan(R, min_samples)
    inside, s = dr.inside_lists(idx, sq)
    want = dr.dbscan(inside, s, min_samples)
    assert same(got, want), (prec, got[3])
    assert len(dr.torn_borders(inside, *want[:2])) > 0  # the border rule had to choose


# ---- 4. chains ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", list(PREC))
@pytest.mark.parametrize("order", ["ascending", "descending", "random"])
def test_a_chain_is_one_cluster(order, prec):
    x, R = dr.chain(order)
    N = len(x)
    lo, hi = int(np.argmin(x[:, 0])), int(np.argmax(x[:, 0]))
    with Ctx(x, PREC[prec]) as c:
        labels, core_of, counts, info = c.dbscan(R, 3)
        again = c.dbscan(R, 3)
    assert np.all(labels == 0) and info["n_clusters"] == 1 and info["n_border"] == 2 and info["n_noise"] == 0, info
    core = core_of == np.arange(N)
    assert set(np.flatnonzero(~core).tolist()) == {lo, hi} and counts[lo] == counts[hi] == 2 and np.all(counts[core] == 3)
    # the ends hang on their only neighbour on the line; the root is the smallest core index
    order_on_line = np.argsort(x[:, 0])
    assert core_of[lo] == order_on_line[1] and core_of[hi] == order_on_line[-2]
    assert min(np.flatnonzero(core)) == (0 if 0 not in (lo, hi) else 1)
    assert same(again, (labels, core_of, counts)) and again[3] == info  # the rounds are the same run to run
    if order == "random":
        assert info["rounds"] >= 2, info


@pytest.mark.parametrize("prec", list(PREC))
def test_two_interleaved_chains_are_two_clusters(prec):
    a, R = dr.chain("random", n=2048, seed=1)
    b, _ = dr.chain("random", n=2048, seed=2)
    x = np.empty((4096, 1))
    x[0::2], x[1::2] = a, b + 100.0  # interleaved in index, more than R apart (the coordinates stay float32-exact)
    with Ctx(x, PREC[prec]) as c:
        labels, core_of, counts, info = c.dbscan(R, 3)
    assert info["n_clusters"] == 2 and info["n_border"] == 4 and info["n_noise"] == 0, info
    assert len(set(labels[0::2])) == 1 and len(set(labels[1::2])) == 1 and labels[0] != labels[1]
    inside, s = dr.inside_dense(x, R)
    assert same((labels, core_of, counts), dr.dbscan(inside, s, 3))


# ---- 5. permuting the points ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", list(PREC))
def test_permuting_the_points_permutes_the_result(prec):
    x, R, min_samples, want = reference("blobs2")
    assert len(dr.ambiguous_borders(x, R, min_samples, np.float32)) == 0  # no distance tie for the border rule to break
    perm = np.random.RandomState(5).permutation(len(x))
    with Ctx(x[perm], PREC[prec]) as c:
        labels, core_of, counts, info = c.dbscan(R, min_samples)
    inv = np.argsort(perm)  # point perm[a] of the cloud is point a of the permuted one
    assert np.array_equal(counts, want[2][perm])
    assert np.array_equal(core_of, np.where(want[1][perm] >= 0, inv[np.maximum(want[1][perm], 0)], -1))
    back = np.empty_like(labels)
    back[perm] = labels
    assert partition(back) == partition(want[0])


# ---- 6. edge cases --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", list(PREC))
def test_min_samples_one_and_beyond_the_largest_count(prec):
    x, R, _, want = reference("blobs3")
    inside, s = dr.inside_dense(x, R)
    with Ctx(x, PREC[prec]) as c:
        got = c.dbscan(R, 1)
        assert got[3]["n_noise"] == 0 and got[3]["n_border"] == 0 and np.all(got[0] >= 0)
        assert same(got, dr.dbscan(inside, s, 1))
        top = int(want[2].max())
        none = c.dbscan(R, top + 1)
        assert np.all(none[0] == -1) and np.all(none[1] == -1) and np.array_equal(none[2], want[2])
        assert none[3] == dict(n_clusters=0, n_core=0, n_border=0, n_noise=len(x), rounds=0, walks=1)
        edge = c.dbscan(R, top)  # exactly at the largest count: those points alone are core points
        assert same(edge, dr.dbscan(inside, s, top)) and edge[3]["n_core"] == int((want[2] == top).sum())


@pytest.mark.parametrize("prec", list(PREC))
@pytest.mark.parametrize("N", [1, 64, 65])
def test_small_clouds_and_duplicates(N, prec):
    rs = np.random.RandomState(N)
    x = rs.randint(0, 4, size=(N, 2)) / 8.0  # many duplicate points
    k = np.rint(x * 8).astype(np.int64)
    inside, s = dr.inside_lattice(k, 1)  # R = 1 / 8: the four lattice neighbours are exactly on the boundary
    for min_samples in (1, 3, 9):
        with Ctx(x, PREC[prec]) as c:
            got = c.dbscan(1.0 / 8.0, min_samples)
        assert same(got, dr.dbscan(inside, s, min_samples)), (N, prec, min_samples)


@pytest.mark.parametrize("prec", list(PREC))
def test_non_finite_points_join_nothing(prec):
    x, R, min_samples, _ = reference("blobs2")
    x = x.copy()
    x[10, 0], x[500, 1], x[77, 0] = np.nan, np.inf, -np.inf
    bad = np.array([10, 500, 77])
    inside, s = dr.inside_dense(x, R)
    assert not inside[bad].any() and not inside[:, bad].any()
    want = dr.dbscan(inside, s, min_samples, nan_points=np.isnan(x).any(axis=1))
    with Ctx(x, PREC[prec]) as c:
        got = c.dbscan(R, min_samples)
    assert same(got, want)
    assert np.all(got[0][bad] == -1) and np.all(got[1][bad] == -1) and got[2][10] == -1 and got[2][500] == got[2][77] == 0
    keep = np.setdiff1d(np.arange(len(x)), bad)
    alone = dr.dbscan(inside[np.ix_(keep, keep)], s[np.ix_(keep, keep)], min_samples)
    assert partition(got[0][keep]) == partition(alone[0])  # the rest clusters as if they were not there


# ---- 7. argument checks ---------------------------------------------------------------------------------------------------------
def raises(code, word, fn):
    with pytest.raises(_lib.KmvpError) as e:
        fn()
    assert e.value.code == code and word in str(e.value) and len(str(e.value)) > 20, str(e.value)


def test_invalid_arguments():
    x = np.random.RandomState(0).rand(100, 2)
    with Ctx(x, np.float32) as c:
        for R in (0.0, -1.0, np.inf, np.nan):
            raises(INVALID, "radius", lambda: c.ctx.dbscan(R, 3))
        for m in (0, -4):
            raises(INVALID, "min_samples", lambda: c.ctx.dbscan(0.1, m))
        lib, ctx = c.ctx._lib, c.ctx._ctx
        out, info = np.zeros(100, dtype=np.int64), np.zeros(6, dtype=np.int64)
        assert lib.kmvp_dbscan(ctx, 0.1, 3, None, None, None, info.ctypes.data) == INVALID and b"NULL" in lib.kmvp_last_error(ctx)
        assert lib.kmvp_dbscan(ctx, 0.1, 3, out.ctypes.data, None, None, None) == INVALID and b"NULL" in lib.kmvp_last_error(ctx)
        assert lib.kmvp_dbscan(ctx, 0.1, 3, out.ctypes.data, None, None, info.ctypes.data) == 0  # the optional outputs
        c.ctx.set_points(np.ascontiguousarray(x, dtype=np.float32), np.ascontiguousarray(x[:50], dtype=np.float32), _lib.KMVP_F32)
        raises(INVALID, "targets", lambda: c.ctx.dbscan(0.1, 3))
    fresh = _lib.Context(0)
    try:
        fresh.N = 0
        raises(INVALID, "kmvp_set_points", lambda: fresh.dbscan(0.1, 3))
    finally:
        fresh.close()


def test_unsupported_contexts_name_dbscan():
    rs = np.random.RandomState(0)
    x = rs.rand(128, 2).astype(np.float32)
    ctx = _lib.Context(0)
    try:
        ctx.set_points(x, None, _lib.KMVP_BF16)
        raises(UNSUPPORTED, "DBSCAN", lambda: ctx.dbscan(0.1, 3))
        ctx.set_points(rs.rand(128, 4).astype(np.float32), None, _lib.KMVP_F32)
        raises(UNSUPPORTED, "DBSCAN", lambda: ctx.dbscan(0.1, 3))
        ctx.set_points(x, None, _lib.KMVP_F32, j_offset=0, M_total=256)  # a source slice
        raises(UNSUPPORTED, "DBSCAN", lambda: ctx.dbscan(0.1, 3))
        ctx.set_points(x, None, _lib.KMVP_F32)
        ctx.set_batches(np.array([0, 64, 128]), None)
        raises(UNSUPPORTED, "DBSCAN", lambda: ctx.dbscan(0.1, 3))
    finally:
        ctx.close()
    # an attached communicator: the host-side rehearsal transport of one rank
    ctx = _lib.Context(0)
    try:
        ctx.set_points(x, None, _lib.KMVP_F32)
        ctx.comm_init_host(lambda buf, op: None, 0, 1)
        raises(UNSUPPORTED, "DBSCAN", lambda: ctx.dbscan(0.1, 3))
    finally:
        ctx.close()


# ---- 8. the other entries, and the side that plans ------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", list(PREC))
def test_other_entries_return_the_same_bits_around_dbscan(prec):
    x, R, min_samples, want = reference("blobs3")
    b = np.random.RandomState(1).randn(len(x), 1)
    with Ctx(x, PREC[prec]) as c:
        ctx = c.ctx
        ctx.set_signal(np.ascontiguousarray(b, dtype=c.precision))

        def others():
            ctx.run_cutoff("gaussian", R, False)
            product = ctx.get_result(len(x), 1)
            return ctx.radius_count(R), ctx.radius_nearest(R, 4), product

        before = others()
        got = c.dbscan(R, min_samples)
        after = others()
        again = c.dbscan(R, min_samples)
    assert same(got, want) and same(again, want) and again[3] == got[3]
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[2], after[2])
    assert np.array_equal(before[1][0], after[1][0]) and np.array_equal(before[1][1], after[1][1])


@pytest.mark.parametrize("prec", list(PREC))
def test_plan_built_on_either_side_gives_the_same_arrays(prec):
    x, R, min_samples, want = reference("blobs2")
    out = []
    for side in (0, 1):
        with Ctx(x, PREC[prec], cutoff_plan=side) as c:
            out.append(c.dbscan(R, min_samples))
            assert c.ctx.cutoff_info()["built_on"] == _lib.CUTOFF_PLAN_SIDES[side]
    assert same(out[0], want) and same(out[1], want) and out[0][3] == out[1][3]


# ---- 9. the plugin ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["float32", "float64"])
def test_plugin_end_to_end(precision):
    x, R, min_samples, want = reference("blobs2")
    algo = MI355XDBSCAN(eps=2 * R, min_samples=min_samples + 1, dimension=2, precision=precision, cutoff_plan="device",
                        cutoff_cell_factor=1.5)
    try:
        with pytest.raises(RuntimeError):
            algo.query()
        algo.prepare_data(points=x)
        with pytest.raises(RuntimeError):
            algo.get_labels()
        algo.set_query_arguments(eps=R, min_samples=min_samples)
        algo.fit()
        algo.query()
        labels, core_of, counts, extra = algo.get_labels(), algo.get_core_of(), algo.get_counts(), algo.get_additional()
        cores = algo.get_core_sample_indices()
        assert algo.get_memory_usage() > 0 and extra["device_kernel"] == KERNEL and extra["device_kernel_ms"] > 0
    finally:
        algo.done()
    assert same((labels, core_of, counts), want)
    assert np.array_equal(cores, np.flatnonzero(want[1] == np.arange(len(x))))
    assert extra["n_clusters"] == labels.max() + 1 and extra["rounds"] >= 1
    with pytest.raises(ValueError):
        algo.set_query_arguments(min_samples=0)
    with pytest.raises(NotImplementedError):
        MI355XDBSCAN(eps=R, min_samples=3, dimension=4)
