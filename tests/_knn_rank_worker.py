"""One rank of tests/test_gpu_knn.py::test_two_ranks_on_one_gpu (started with RANK / WORLD_SIZE / MASTER_* in the
environment), after the pattern of _lse_rank_worker.py.

Every rank drives the plugin's nearest-neighbour query on GPU 0 with the sources sharded over the ranks, through the real
libkmvp.so; the exchange -- ONE all-reduce(sum) of the zero-filled [world][2 K][N] candidate slots -- is staged through
host memory and reduced by gloo (include/kmvp.h kmvp_comm_init_host): test infrastructure, selected explicitly.  Every
collective of the group runs under the group's own time limit, so a rank that died ends the others instead of leaving
them waiting.
"""
import datetime
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

    import knn_reference as kn
    from kernel_matrix_benchmarks_amd.algorithms.mi355x import MI355XProduct

    dist.init_process_group("gloo", timeout=datetime.timedelta(seconds=60))
    rank, world = dist.get_rank(), dist.get_world_size()
    comm = sharding.torch_gloo_communicator(exchange="host")
    report = []
    ranks_equal = True

    # lattice clouds (exact in every precision: the sharded result must equal the restatement of the WHOLE cloud bit for bit)
    # (precision, M, N or None for targets == sources, K, exclude_self)
    cases = ((np.float64, 1001, 300, 16, False),   # uneven split: 501 + 500
             (np.float32, 257, 65, 5, False),
             (np.float16, 301, None, 4, False),
             (np.float32, 1, 50, 3, False),        # M_total = 1: the second rank's slice is empty
             (np.float64, 401, None, 15, True),    # exclude_self on a source shard: same_points_global
             (np.float32, 1, None, 1, True))       # ... with an empty slice: nothing but the own point, so no neighbour at all
    for precision, M, N, K, exclude_self in cases:
        rs = np.random.RandomState(M + (N or 0) + K)
        y = kn.lattice(rs, M, 3)
        if M > 30:
            y[5:27] = y[5]  # 22 coincident points: more than K + 1
        x = None if N is None else kn.lattice(rs, N, 3)
        # (absolute-exponential: the float32 Gaussian plugin deals its sources to the ranks in cell order and refuses this query)
        algo = MI355XProduct(kernel="absolute-exponential", dimension=3, precision=precision, device=0, comm=comm)
        try:
            algo.prepare_data(source_points=y, target_points=y if x is None else x, same_points=x is None)
            algo.query_nearest(K, exclude_self=exclude_self)
            idx, sq = algo.get_nearest()
            meta = algo.get_additional()
            lo, hi = algo.shard
        finally:
            algo.done()
        want_idx, want_sq = kn.nearest(y if x is None else x, y, K, exclude_self=exclude_self)
        assert meta["rccl_ranks"] == world and meta["n_gpus"] == world and meta["dispatch_note"] == "", meta
        assert (lo, hi) == tuple(sharding.shard_range(M, rank, world))
        assert meta["device_kernel"] == ("none" if lo == hi else "lowd_knn_kernel"), meta
        assert idx.dtype == np.int64 and sq.dtype == np.float64 and idx.shape == want_idx.shape == sq.shape
        assert np.array_equal(idx, want_idx) and np.array_equal(sq, want_sq), (precision, M, N, K, exclude_self)
        if exclude_self:
            assert not np.any(idx == np.arange(M)[:, None])
        # every rank must hold the same bits
        for got in (idx.astype(np.float64), sq):
            t = torch.from_numpy(np.where(np.isinf(got), -2.0, got))
            lo_t, hi_t = t.clone(), t.clone()
            dist.all_reduce(lo_t, op=dist.ReduceOp.MIN)
            dist.all_reduce(hi_t, op=dist.ReduceOp.MAX)
            ranks_equal = ranks_equal and bool(torch.equal(lo_t, hi_t))
        empty = [list(sharding.shard_range(M, r, world)) for r in range(world)]
        report.append({"precision": np.dtype(precision).name, "M": M, "K": K, "exclude_self": exclude_self,
                       "empty_slice": any(a == b for a, b in empty)})

    assert ranks_equal, "ranks disagree on the results"
    if rank == 0:
        print(json.dumps({"world": world, "ranks_bitwise_equal": ranks_equal, "cases": report}), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
