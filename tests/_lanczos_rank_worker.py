"""One rank of test_gpu_lanczos.py::test_two_ranks_on_one_gpu (started with RANK / WORLD_SIZE / MASTER_* in the
environment).

Both ranks sit on GPU 0 and drive the C ABI directly, so that the source shards can be UNEVEN (150 + 107 of 257): the
Gaussian operator of krylov_reference's Gr is sharded over the sources, the Krylov vectors are replicated, the exchange is
staged through host memory and summed by gloo (include/kmvp.h kmvp_comm_init_host).  The ranks must end with bitwise the
same outputs; rank 0 prints them for the test to hold against the restatement.  Then the same through the plugin:
MI355XSolver(comm=...).log_determinant, which shards the sources itself.
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(HERE, "..", "oracle"), os.path.join(HERE, "..")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

SPLIT, RTOL = 150, 1e-7
KEYS = ("logquad", "invquad", "steps", "x", "alpha", "beta")


def main():
    from kernel_matrix_benchmarks_amd import _lib, sharding

    _lib.load()  # the system ROCm stack first (bench.py does the same)
    import torch.distributed as dist

    import krylov_reference as kr
    import lanczos_reference as lz

    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert world == 2
    comm = sharding.torch_gloo_communicator(exchange="host")
    lo, hi = (0, SPLIT) if rank == 0 else (SPLIT, kr.N)
    y = kr.points("Gr")
    ctx = _lib.Context(0)
    try:
        comm.attach(ctx)
        ctx.set_option("same_points_global", 1)
        ctx.set_points(np.ascontiguousarray(y[lo:hi]), y, _lib.KMVP_F64, j_offset=lo, M_total=kr.N)
        ctx.set_solver_diagonal(None, kr.SYSTEMS["Gr"].ridge)
        out = ctx.lanczos_quadrature("gaussian", lz.block(4), RTOL, 1000, want_x=True, want_coefficients=True)
        assert ctx.rccl_ranks == world
    finally:
        ctx.close()
    # the plugin with the communicator: MI355XSolver shards the sources itself (even shards)
    from kernel_matrix_benchmarks_amd.algorithms.mi355x import MI355XSolver

    algo = MI355XSolver(kernel="gaussian", dimension=kr.D, precision=np.float64, rtol=RTOL, maxit=1000,
                        ridge=kr.SYSTEMS["Gr"].ridge, comm=comm)
    try:
        algo.prepare_data(source_points=y)
        algo.fit()
        ld = algo.log_determinant(probes=64, seed=0)
        plug = {"value": ld.value, "stderr": ld.stderr, "trace_inverse": ld.trace_inverse, "steps": ld.steps.tolist(),
                "converged": bool(ld.converged), "n_gpus": algo.get_additional()["n_gpus"]}
        plug_shard = list(algo._shard)
    finally:
        algo.done()
    plug_digests, plug_shards = [None] * world, [None] * world
    dist.all_gather_object(plug_digests, json.dumps(plug))
    dist.all_gather_object(plug_shards, plug_shard)
    plug.update(ranks_bitwise_equal=len(set(plug_digests)) == 1, shards=plug_shards)
    digest = hashlib.sha256(b"".join(np.ascontiguousarray(out[k]).tobytes() for k in KEYS)).hexdigest()
    digests, shards = [None] * world, [None] * world
    dist.all_gather_object(digests, digest)
    dist.all_gather_object(shards, [lo, hi])
    if rank == 0:
        m = int(out["steps"].max())  # (rows beyond the last step are zero: not printed)
        outputs = {k: out[k].tolist() for k in ("logquad", "invquad", "steps", "x")}
        outputs["alpha"], outputs["beta"] = out["alpha"][:m].tolist(), out["beta"][:m].tolist()
        print(json.dumps({"world": world, "shards": shards, "converged": bool(out["converged"]),
                          "ranks_bitwise_equal": len(set(digests)) == 1, "outputs": outputs, "plugin": plug}), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
