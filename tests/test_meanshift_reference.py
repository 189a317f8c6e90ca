"""The restatement of the Gaussian mean-shift (meanshift_reference.py) on its own, without a GPU: freeze and iters
semantics on hand-made gradient sequences, target_sweeps, the NaN rule, a far seed on lse_grad_reference.gradient, the
cluster rule, the test cloud."""
import numpy as np
import pytest

import lse_grad_reference
import meanshift_reference as mr


def scripted(rows_per_call):
    """grad() that plays back hand-made rows: call k returns rows_per_call[k], which must match the rows it is asked for."""
    calls = []

    def grad(targets):
        G = np.asarray(rows_per_call[len(calls)], dtype=np.float64)
        assert G.shape == targets.shape, (len(calls), G.shape, targets.shape)
        calls.append(np.array(targets))
        return G

    grad.calls = calls
    return grad


def test_freeze_and_iters_on_a_hand_made_sequence():
    # three points in 1-D, tol = 0.1 (q <= 0.01 freezes: |G| <= 0.2)
    #   point 0: steps 1, 0.5, 0.05 -> freezes in sweep 3 and KEEPS that sweep's update
    #   point 1: step 0.1 exactly at the tolerance -> freezes in sweep 1
    #   point 2: never arrives
    grad = scripted([[[2.0], [0.2], [4.0]], [[1.0], [4.0]], [[0.1], [4.0]], [[4.0]], [[4.0]]])
    r = mr.meanshift(grad, np.array([[0.0], [10.0], [20.0]]), tol=0.1, maxit=5)
    assert list(r["iters"]) == [3, 1, 5] and r["sweeps"] == 5 and not r["converged"]
    assert r["target_sweeps"] == 3 + 2 + 2 + 1 + 1
    assert np.array_equal(r["modes"], [[1.0 + 0.5 + 0.05], [10.1], [30.0]])
    assert np.array_equal(r["step2"], [0.05 * 0.05, 0.1 * 0.1, 4.0])
    # the frozen points are no longer asked about: the calls shrink, and each sees the positions of the sweep before
    assert [c.shape[0] for c in grad.calls] == [3, 2, 2, 1, 1]
    assert np.array_equal(grad.calls[2], [[1.5], [24.0]])


def test_everything_frozen_ends_the_solve_before_maxit():
    grad = scripted([[[1.0, 0.0], [0.0, 0.0]], [[0.0, 0.0]]])
    r = mr.meanshift(grad, np.zeros((2, 2)), tol=1e-3, maxit=100)
    assert r["converged"] and r["sweeps"] == 2 and r["target_sweeps"] == 3 and list(r["iters"]) == [2, 1]
    assert np.array_equal(r["modes"], [[0.5, 0.0], [0.0, 0.0]]) and np.array_equal(r["step2"], [0.0, 0.0])


def test_maxit_is_honoured_and_the_last_sweep_can_still_converge():
    grad = scripted([[[2.0]], [[0.0]]])
    r = mr.meanshift(grad, np.zeros((1, 1)), tol=0.0, maxit=1)
    assert not r["converged"] and r["sweeps"] == 1 and list(r["iters"]) == [1] and r["step2"][0] == 1.0 and r["modes"][0, 0] == 1.0
    grad = scripted([[[2.0]], [[0.0]]])
    r = mr.meanshift(grad, np.zeros((1, 1)), tol=0.0, maxit=2)
    assert r["converged"] and r["sweeps"] == 2 and list(r["iters"]) == [2] and r["step2"][0] == 0.0


def test_all_rows_mode_feeds_every_row_and_uses_the_active_ones():
    """The host loop of the GPU tests keeps all N targets on its context: the frozen rows are still asked about, at their
    last position, and whatever comes back for them is ignored."""
    seen = []

    def grad(targets):
        seen.append(np.array(targets))
        G = np.full(targets.shape, 4.0)
        G[1] = 0.0 if len(seen) == 1 else 1e9  # point 1 freezes at once; later answers for it must not matter
        return G

    r = mr.meanshift(grad, np.array([[0.0], [7.0], [1.0]]), tol=1e-3, maxit=3, all_rows=True)
    assert all(s.shape == (3, 1) for s in seen) and len(seen) == 3
    assert list(r["iters"]) == [3, 1, 3] and r["target_sweeps"] == 3 + 2 + 2
    assert np.array_equal(r["modes"], [[6.0], [7.0], [7.0]]) and seen[2][1, 0] == 7.0


def test_the_nan_rule():
    nan, inf = float("nan"), float("inf")
    grad = scripted([[[1.0, 1.0], [nan, 0.0], [0.0, 0.0]], [[0.0, inf]]])
    r = mr.meanshift(grad, np.zeros((3, 2)), tol=1e-6, maxit=10)
    assert list(r["iters"]) == [2, 1, 1] and r["sweeps"] == 2 and r["target_sweeps"] == 4
    assert np.all(np.isnan(r["modes"][:2])) and np.all(np.isnan(r["step2"][:2]))  # all D components, also the finite one
    assert np.array_equal(r["modes"][2], [0.0, 0.0]) and r["step2"][2] == 0.0
    assert not r["converged"]  # every point froze, but not every one with a finite q


def test_the_working_precision_rounds_the_position_the_gradient_is_taken_at():
    # z_1 = 1 + 2^-30 does not fit float32: the second gradient is asked at 1, and base is 1, so the 2^-30 is dropped
    grad = scripted([[[2.0 + 2.0 ** -29]], [[2.0]], [[0.0]]])
    r = mr.meanshift(grad, np.zeros((1, 1)), tol=0.0, maxit=3, precision=np.float32)
    assert grad.calls[1].dtype == np.float32 and grad.calls[1][0, 0] == 1.0
    assert r["modes"][0, 0] == 2.0 and r["converged"]
    grad = scripted([[[2.0 + 2.0 ** -29]], [[2.0]], [[0.0]]])
    r = mr.meanshift(grad, np.zeros((1, 1)), tol=0.0, maxit=3, precision=np.float64)
    assert r["modes"][0, 0] == 2.0 + 2.0 ** -30


@pytest.mark.parametrize("precision", [np.float32, np.float64])
def test_a_far_seed_moves_onto_the_blob(precision):
    rs = np.random.RandomState(0)
    y = (0.25 * rs.randn(200, 3)).astype(precision).astype(np.float64)
    seed = np.array([[30.0, 0.0, 0.0]])
    # the naive ratio sum(k y) / sum(k) is 0 / 0 there: every kernel value underflows
    k = np.exp(-np.sum((seed.astype(precision) - y.astype(precision)) ** 2, axis=1))
    assert np.all(k == 0)
    with np.errstate(invalid="ignore"):
        assert np.all(np.isnan((k @ y) / np.sum(k)))

    def grad(t):
        return lse_grad_reference.gradient(kernel="gaussian", source_points=y, target_points=t, precision=precision)[:, 0, :]

    tol = 1e-4 if precision == np.float32 else 1e-10
    r = mr.meanshift(grad, seed, tol=tol, maxit=200, precision=precision)
    assert r["converged"] and np.all(np.isfinite(r["modes"]))
    assert np.linalg.norm(r["modes"][0]) < 0.2  # on the blob, near its mean
    assert np.min(np.linalg.norm(y - r["modes"][0], axis=1)) < 0.25
    # the first step alone covers almost all of the distance: the softmax sits on the nearest points of the blob
    one = mr.meanshift(grad, seed, tol=tol, maxit=1, precision=precision)
    assert one["modes"][0, 0] < 1.0 and one["step2"][0] > 29.0 ** 2


def test_the_cluster_rule_with_a_tie_and_an_unconverged_point():
    tol = 1e-3
    modes = np.array([[0.0, 0.0],    # 0 founds centre 0
                      [0.3, 0.0],    # 1 within 0.5 of centre 0
                      [2.0, 0.0],    # 2 founds centre 1
                      [1.0, 0.0],    # 3 founds centre 2 (1.0 from both), and ties between centres 0 and 1 ... as a centre it is its own
                      [0.5, 0.0],    # 4 exactly at the radius of centre 0 (<=: no new centre); equally far from centres 0 and 2
                      [9.0, 9.0],    # 5 still moving: -1, and it founds nothing
                      [np.nan, 0.0],  # 6 NaN: -1
                      [1.5, 0.0]])   # 7 equally far from centres 1 and 2: the smaller label
    step2 = np.array([0.0, 0.0, 0.0, 0.0, 1e-6, 1.0, np.nan, 0.0])
    centres, labels = mr.clusters(modes, step2, tol, merge_radius=0.5)
    assert np.array_equal(centres, [[0.0, 0.0], [2.0, 0.0], [1.0, 0.0]])
    assert list(labels) == [0, 0, 1, 2, 0, -1, -1, 1]
    # a radius of 0 merges only coincident modes; nothing converged: no centre at all
    centres, labels = mr.clusters(modes[[0, 0, 1]], np.zeros(3), tol, merge_radius=0.0)
    assert centres.shape == (2, 2) and list(labels) == [0, 0, 1]
    centres, labels = mr.clusters(modes[:3], np.ones(3), tol, merge_radius=0.5)
    assert centres.shape == (0, 2) and list(labels) == [-1, -1, -1]


@pytest.mark.parametrize("D", [1, 3, 8])
def test_the_cloud(D):
    pts = mr.cloud(2000, D)
    assert pts.shape == (2000, D) and pts.flags.c_contiguous and np.all(np.isfinite(pts))
    assert np.array_equal(pts, mr.cloud(2000, D))  # deterministic
    tight = np.sum(np.linalg.norm(pts, axis=1) < 4 * 0.25 * np.sqrt(D))
    assert tight >= 500 * 0.95  # the tight blob is there (plus whatever of the rest falls into it)
    far = pts[:, D - 1] > (5.0 if D > 1 else 13.0)
    assert np.sum(far) >= 500 * 0.95  # and the ridge, away from both blobs
    assert pts.min() >= -4.5 and pts.max() <= (8.0 if D > 1 else 21.0)  # D = 1: the ridge is the stretch [14, 20]
