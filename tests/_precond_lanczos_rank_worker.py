"""One rank of test_gpu_precond_lanczos.py::test_two_ranks_on_one_gpu (started with RANK / WORLD_SIZE / MASTER_* in the
environment).

Both ranks sit on GPU 0 and drive the C ABI directly with UNEVEN source shards (250 + 134 of 384): the Matern 5/2 operator
of precond_reference's system M52 is sharded over the sources, the Krylov vectors are replicated, the exchange is staged
through host memory and summed by gloo.  The factor is built from the targets, the full cloud on every rank, so log det P,
the probes, pz and rho_0 are bitwise those of a single unsharded context, and both ranks end with bitwise the same
everything; against one rank the operator's sums differ in their order, so the iterated values agree within the
product's tolerance (precond_lanczos_reference.tolerance).
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.join(HERE, "..", "oracle"), os.path.join(HERE, "..")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

SPLIT, NAME, P = 250, "M52", 5


def main():
    from kernel_matrix_benchmarks_amd import _lib, sharding

    _lib.load()  # the system ROCm stack first (bench.py does the same)
    import torch.distributed as dist

    import krylov_reference as kr
    import lanczos_reference as lz
    import precond_lanczos_reference as plr
    import precond_reference as pr

    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    assert world == 2
    comm = sharding.torch_gloo_communicator(exchange="host")
    lo, hi = (0, SPLIT) if rank == 0 else (SPLIT, pr.N)
    y, kernel, rtol = pr.points(NAME), pr.SYSTEMS[NAME].kernel, plr.COMPARED[1][1]
    assert plr.COMPARED[1][0] == NAME
    g, h = plr.block(P)
    want = dict(want_x=True, want_pz=True, want_coefficients=True)
    ctx = _lib.Context(0)
    try:
        comm.attach(ctx)
        ctx.set_option("same_points_global", 1)
        ctx.set_points(np.ascontiguousarray(y[lo:hi]), y, _lib.KMVP_F64, j_offset=lo, M_total=pr.N)
        ctx.set_solver_diagonal(pr.DIAG, 0.0)
        ctx.set_solver_preconditioner(pr.RANK)
        out = ctx.lanczos_quadrature_precond(kernel, g, h, rtol, 1000, **want)
        built = ctx.last_preconditioner_rank
    finally:
        ctx.close()
    single = _lib.Context(0)  # the same system unsharded, on this rank alone
    try:
        single.set_points(y, None, _lib.KMVP_F64)
        single.set_solver_diagonal(pr.DIAG, 0.0)
        single.set_solver_preconditioner(pr.RANK)
        one = single.lanczos_quadrature_precond(kernel, g, h, rtol, 1000, **want)
    finally:
        single.close()
    m = int(out["steps"].max())
    keys = ("logquad", "invquad", "wnorm2", "steps", "x", "pz")
    blob = b"".join(np.ascontiguousarray(out[k]).tobytes() for k in keys) + out["alpha"][:m].tobytes() + \
        out["beta"][:m].tobytes() + np.float64(out["logdet_p"]).tobytes()
    digests = [None] * world
    dist.all_gather_object(digests, hashlib.sha256(blob).hexdigest())
    shards = [None] * world
    dist.all_gather_object(shards, [lo, hi])
    if rank == 0:
        ref = plr.Run(one["x"], one["pz"], one["steps"], None, one["alpha"], one["beta"], plr.own(NAME, P, rtol).rel,
                      one["wnorm2"], one["logquad"], one["invquad"], None, one["logdet_p"], None, m)
        nz = one["wnorm2"] > 0
        print(json.dumps({
            "world": world, "shards": shards, "converged": bool(out["converged"]), "rank_built": int(built),
            "ranks_bitwise_equal": len(set(digests)) == 1,
            "steps_equal_single": bool(np.array_equal(out["steps"], one["steps"])),
            "product_free_equal_single": bool(out["logdet_p"] == one["logdet_p"] and np.array_equal(out["pz"], one["pz"])
                                              and np.array_equal(out["wnorm2"], one["wnorm2"])),
            "logquad_error": float(np.max(np.abs(out["logquad"] - one["logquad"])[nz] / one["wnorm2"][nz])),
            "invquad_error": float(np.max(np.abs(out["invquad"] - one["invquad"])[nz] / np.abs(one["invquad"][nz]))),
            "coefficient_error": float(max(lz.coefficient_error(out["alpha"], out["beta"], ref, e, weighted=True)
                                           for e in range(P))),
            "x_error": float(kr.column_error(out["x"], one["x"])),
            "tolerance": plr.tolerance(NAME, rtol), "x_tolerance": plr.tolerance(NAME, rtol, plr.GX)}), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
