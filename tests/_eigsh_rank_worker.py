"""One rank of test_gpu_eigsh.py::test_two_ranks_on_one_gpu (started with RANK / WORLD_SIZE / MASTER_* in the
environment).

Both ranks sit on GPU 0 and drive the C ABI directly, so that the source shards can be UNEVEN (300 + 500 of 800): the
Gaussian operator on eigsh_reference's cloud is sharded over the sources, the Lanczos basis is replicated, the exchange is
staged through host memory and summed by gloo (include/kmvp.h kmvp_comm_init_host).  The ranks must end with bitwise the
same outputs for each of the three operators; rank 0 prints them for the test to hold against the single-GPU run.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(HERE, "..", "oracle"), os.path.join(HERE, "..")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

SPLIT, TOL = 300, 1e-10
KEYS = ("eigenvalues", "eigenvectors", "resid", "alpha", "beta")


def main():
    from kernel_matrix_benchmarks_amd import _lib, sharding

    _lib.load()  # the system ROCm stack first (bench.py does the same)
    import torch.distributed as dist

    import eigsh_reference as er

    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert world == 2
    comm = sharding.torch_gloo_communicator(exchange="host")
    lo, hi = (0, SPLIT) if rank == 0 else (SPLIT, er.N)
    y = er.cloud()
    outs = {}
    ctx = _lib.Context(0)
    try:
        comm.attach(ctx)
        ctx.set_option("same_points_global", 1)
        ctx.set_points(np.ascontiguousarray(y[lo:hi]), y, _lib.KMVP_F64, j_offset=lo, M_total=er.N)
        for op in er.OPERATORS:
            outs[op] = ctx.eigsh("gaussian", er.K, op, er.start_vector(), TOL, er.MAXIT, want_coefficients=True)
        assert ctx.rccl_ranks == world
    finally:
        ctx.close()
    h = hashlib.sha256()
    for op in er.OPERATORS:
        for k in KEYS + (("degree",) if op == "normalized" else ()):
            h.update(np.ascontiguousarray(outs[op][k]).tobytes())
        h.update(str((outs[op]["steps"], outs[op]["converged"])).encode())
    digests, shards = [None] * world, [None] * world
    dist.all_gather_object(digests, h.hexdigest())
    dist.all_gather_object(shards, [lo, hi])
    if rank == 0:
        outputs = {op: {"eigenvalues": outs[op]["eigenvalues"].tolist(), "resid": outs[op]["resid"].tolist(),
                        "steps": int(outs[op]["steps"]), "converged": bool(outs[op]["converged"])} for op in er.OPERATORS}
        print(json.dumps({"world": world, "shards": shards, "ranks_bitwise_equal": len(set(digests)) == 1,
                          "outputs": outputs}), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
