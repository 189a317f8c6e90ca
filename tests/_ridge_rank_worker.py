"""One rank of test_gpu_solver_ridge.py::test_two_ranks_on_one_gpu_solve_the_regularised_system (started with RANK /
WORLD_SIZE / MASTER_* in the environment).

Both ranks sit on GPU 0 and drive the C ABI directly, so that the source shards can be UNEVEN (1300 + 700 of 2000): the
Gaussian operator is sharded over the sources, the Krylov vectors are replicated, the exchange is staged through host
memory and summed by gloo (include/kmvp.h kmvp_comm_init_host), and every rank passes the FULL diagonal.  The ranks must
end with bitwise the same b -- the diagonal term is added once, after the all-reduce -- and b is held to the dense solve.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(HERE, "..", "oracle"), os.path.join(HERE, "..")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

N, SPLIT, RTOL = 2000, 1300, 1e-10


def main():
    from kernel_matrix_benchmarks_amd import _lib, sharding

    _lib.load()  # the system ROCm stack first (bench.py does the same)
    import torch.distributed as dist

    import kmvp_oracle

    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert world == 2
    comm = sharding.torch_gloo_communicator(exchange="host")
    lo, hi = (0, SPLIT) if rank == 0 else (SPLIT, N)
    y = np.random.RandomState(11).rand(N, 3)
    a = np.random.RandomState(13).randn(N, 3)
    d = np.random.RandomState(12).uniform(0.05, 0.2, N)
    K = kmvp_oracle.kernel_matrix(kernel="gaussian", source_points=y)
    cases = []
    for diag, ridge in ((None, 0.1), (d, 0.05)):
        ctx = _lib.Context(0)
        try:
            comm.attach(ctx)
            ctx.set_option("same_points_global", 1)
            ctx.set_points(np.ascontiguousarray(y[lo:hi]), y, _lib.KMVP_F64, j_offset=lo, M_total=N)
            ctx.set_solver_diagonal(diag, ridge)
            b, iters, resid, ok = ctx.cg_solve("gaussian", a, RTOL, 5000)
            assert ctx.rccl_ranks == world
        finally:
            ctx.close()
        A = K + np.diag(ridge + (np.zeros(N) if diag is None else diag))
        w = np.abs(np.linalg.eigvalsh(A))
        kappa = float(w.max() / w.min())
        dense = np.linalg.solve(A, a)
        err = float(np.max(np.linalg.norm(b - dense, axis=0) / np.linalg.norm(dense, axis=0)))
        digests = [None] * world
        dist.all_gather_object(digests, hashlib.sha256(np.ascontiguousarray(b).tobytes()).hexdigest())
        cases.append({"ridge": ridge, "per_point": diag is not None, "converged": bool(ok), "iterations": int(iters),
                      "resid": float(resid), "kappa": kappa, "vector_error": err, "bound": kappa * 1.5 * RTOL + kappa * 1e-11,
                      "ranks_bitwise_equal": len(set(digests)) == 1})
    shards = [None] * world
    dist.all_gather_object(shards, [lo, hi])
    if rank == 0:
        print(json.dumps({"world": world, "shards": shards, "cases": cases}), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
