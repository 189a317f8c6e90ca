"""One rank of test_gpu_precond.py::test_two_ranks_on_one_gpu (started with RANK / WORLD_SIZE / MASTER_* in the
environment).

Both ranks sit on GPU 0 and drive the C ABI directly with UNEVEN source shards (250 + 134 of 384): the Matern 5/2 operator
of precond_reference's system M52 is sharded over the sources, the Krylov vectors are replicated, the exchange is staged
through host memory and summed by gloo.  The preconditioner is built from the targets, the full cloud on every rank, so both
ranks must hold the same pivots -- those of a single unsharded context -- and end with bitwise the same b.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(HERE, "..", "oracle"), os.path.join(HERE, "..")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

SPLIT, NAME, RTOL = 250, "M52", 1e-8


def main():
    from kernel_matrix_benchmarks_amd import _lib, sharding

    _lib.load()  # the system ROCm stack first (bench.py does the same)
    import torch.distributed as dist

    import precond_reference as pr

    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert world == 2
    comm = sharding.torch_gloo_communicator(exchange="host")
    lo, hi = (0, SPLIT) if rank == 0 else (SPLIT, pr.N)
    y, a, kernel = pr.points(NAME), pr.rhs(3), pr.SYSTEMS[NAME].kernel
    ctx = _lib.Context(0)
    try:
        comm.attach(ctx)
        ctx.set_option("same_points_global", 1)
        ctx.set_points(np.ascontiguousarray(y[lo:hi]), y, _lib.KMVP_F64, j_offset=lo, M_total=pr.N)
        ctx.set_solver_diagonal(pr.DIAG, 0.0)
        ctx.set_solver_preconditioner(pr.RANK)
        b, iters, resid, ok = ctx.cg_solve(kernel, a, RTOL, 1000)
        built, pivots, factor = ctx.get_solver_preconditioner()
    finally:
        ctx.close()
    single = _lib.Context(0)  # the same system unsharded, on this rank alone
    try:
        single.set_points(y, None, _lib.KMVP_F64)
        single.set_solver_diagonal(pr.DIAG, 0.0)
        single.set_solver_preconditioner(pr.RANK)
        _, single_iters, _, _ = single.cg_solve(kernel, a, RTOL, 1000)
        _, single_pivots, single_factor = single.get_solver_preconditioner()
    finally:
        single.close()
    A, _ = pr.matrix(NAME)
    from krylov_reference import true_residual
    digest = hashlib.sha256(np.ascontiguousarray(b).tobytes() + pivots.tobytes() + factor.tobytes()).hexdigest()
    digests = [None] * world
    dist.all_gather_object(digests, digest)
    shards = [None] * world
    dist.all_gather_object(shards, [lo, hi])
    if rank == 0:
        print(json.dumps({"world": world, "shards": shards, "converged": bool(ok), "iterations": int(iters),
                          "single_iterations": int(single_iters), "resid": float(resid), "rank_built": int(built),
                          "numpy_resid": float(np.max(true_residual(A, b, a))), "rtol": RTOL,
                          "pivots_equal_single": bool(np.array_equal(pivots, single_pivots)),
                          "factor_equals_single": bool(np.array_equal(factor, single_factor)),
                          "ranks_bitwise_equal": len(set(digests)) == 1}), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
