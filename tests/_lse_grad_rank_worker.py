"""One rank of tests/test_gpu_lse_grad.py::test_two_ranks_on_one_gpu (started with RANK / WORLD_SIZE / MASTER_* in the
environment), after the pattern of _multirank_worker.py.

Every rank drives the plugin's gradient of the log-sum-exp on GPU 0 with the sources sharded over the ranks, through the
real libkmvp.so; the exchange -- all-reduce(min) of the exponents, then ONE all-reduce(sum) of the D + 1 sums per column
and target -- is staged through host memory and reduced by gloo (include/kmvp.h kmvp_comm_init_host): test
infrastructure, selected explicitly.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(HERE, "..", "oracle"), os.path.join(HERE, "..")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402


def main():
    from kernel_matrix_benchmarks_amd import _lib, sharding

    _lib.load()  # the system ROCm stack first (bench.py does the same)
    import torch
    import torch.distributed as dist

    import lse_grad_reference
    from kernel_matrix_benchmarks_amd.algorithms.mi355x import MI355XProduct

    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    comm = sharding.torch_gloo_communicator(exchange="host")
    report = []
    ranks_equal = True

    def rounded(a, precision):
        return None if a is None else np.asarray(a, dtype=precision).astype(np.float64)

    # (kernel, precision, M, N or None for targets == sources, E or None for density estimation)
    cases = (("gaussian", np.float64, 1001, 300, 2),            # uneven split: 501 + 500
             ("gaussian", np.float32, 2001, None, 1),           # the float32 Gaussian shards in spatial order
             ("absolute-exponential", np.float64, 777, 130, 3),
             ("absolute-exponential", np.float32, 1500, 257, None),
             ("gaussian", np.float64, 1, 50, 2),                # one source: the second rank's slice is empty
             ("absolute-exponential", np.float32, 1, 50, 1))
    for kernel, precision, M, N, E in cases:
        rs = np.random.RandomState(M + (N or 0))
        y = rounded(rs.rand(M, 3) * 3.0, precision)
        x = None if N is None else rounded(rs.rand(N, 3) * 3.0, precision)
        c = None if E is None else rounded(rs.randn(M, E), precision)
        if c is not None and M > 10:
            c[3::5, 0] = -np.inf
        algo = MI355XProduct(kernel=kernel, dimension=3, precision=precision, device=0, comm=comm)
        try:
            algo.prepare_data(source_points=y, target_points=y if x is None else x, same_points=x is None,
                              density_estimation=c is None)
            algo.fit()
            algo.prepare_query(source_signal=c)
            algo.query_logsumexp_gradient()
            got = algo.get_logsumexp_gradient()
            meta = algo.get_additional()
            lo, hi = algo.shard
        finally:
            algo.done()
        want = lse_grad_reference.gradient(kernel=kernel, source_points=y, target_points=x, source_signal=c)

        def err(a):  # per (row, column): max_d |a - want| / max(1, max_d |want|)
            return float(np.max(np.max(np.abs(a - want), axis=-1) / np.maximum(1.0, np.max(np.abs(want), axis=-1))))

        tol = 1e-11
        if precision == np.float32:
            own = lse_grad_reference.gradient(kernel=kernel, source_points=y, target_points=x, source_signal=c,
                                              precision=np.float32)
            tol = max(1e-5, 2 * err(own))
        assert got.shape == want.shape and np.isfinite(want).all()
        e = err(got)
        assert meta["rccl_ranks"] == world and meta["n_gpus"] == world and meta["dispatch_note"] == "", meta
        assert (lo, hi) == tuple(sharding.shard_range(M, rank, world))
        assert meta["device_kernel"] == ("none" if lo == hi else "lowd_lse_grad_kernel"), meta
        assert np.isfinite(got).all() and e <= tol, (kernel, M, e, tol, meta)
        # every rank must hold the same bits
        t = torch.from_numpy(got.copy())
        lo_t, hi_t = t.clone(), t.clone()
        dist.all_reduce(lo_t, op=dist.ReduceOp.MIN)
        dist.all_reduce(hi_t, op=dist.ReduceOp.MAX)
        ranks_equal = ranks_equal and bool(torch.equal(lo_t, hi_t))
        empty = [list(sharding.shard_range(M, r, world)) for r in range(world)]
        report.append({"kernel": kernel, "precision": np.dtype(precision).name, "M": M, "err": e, "tolerance": tol,
                       "empty_slice": any(a == b for a, b in empty)})

    assert ranks_equal, "ranks disagree on the results"
    if rank == 0:
        print(json.dumps({"world": world, "ranks_bitwise_equal": ranks_equal, "cases": report}), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
