"""One rank of tests/test_gpu_matern.py::test_two_ranks_on_one_gpu (started with RANK / WORLD_SIZE / MASTER_* in the
environment), after the pattern of _multirank_worker.py.

Every rank drives the plugin on GPU 0 with the Matern kernels' sources sharded over the ranks (the caller's order: no
spatial order for these kernels), through the real libkmvp.so; the exchange is staged through host memory and summed by
gloo (include/kmvp.h kmvp_comm_init_host) -- test infrastructure, selected explicitly.
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

    import matern_reference as mref
    from conftest import rel_err
    from kernel_matrix_benchmarks_amd.algorithms.mi355x import MI355XProduct, MI355XSolver

    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    comm = sharding.torch_gloo_communicator(exchange="host")
    report = []

    def rounded(a, precision):
        return np.asarray(a, dtype=precision).astype(np.float64)

    for kernel in mref.KERNELS:
        # (what, normalize, precision, n, E, x != y)
        for what, normalize, precision, n, E, other in (("product", True, np.float64, 3001, 2, True),
                                                        ("product", False, np.float32, 5000, 1, False),
                                                        ("gradient", False, np.float64, 1003, 2, True)):
            rs = np.random.RandomState(n + E)
            y, b = rounded(rs.rand(n, 3), precision), rounded(rs.randn(n, E), precision)
            x = rounded(rs.rand(n // 2 + 3, 3), precision) if other else None
            algo = MI355XProduct(kernel=kernel, dimension=3, normalize_rows=normalize, precision=precision, device=0, comm=comm)
            try:
                algo.prepare_data(source_points=y, target_points=y if x is None else x, same_points=x is None)
                algo.fit()
                algo.prepare_query(source_signal=b)
                if what == "gradient":
                    algo.query_gradient()
                    got = algo.get_gradient()
                else:
                    algo.query()
                    got = algo.get_result()
                meta = algo.get_additional()
                lo, hi = algo.shard
            finally:
                algo.done()
            ref = dict(kernel=kernel, source_points=y, target_points=x, source_signal=b)
            if what == "gradient":
                want, own = mref.gradient(**ref), None
            else:
                want = mref.product(normalize_rows=normalize, **ref)
                own = mref.product(normalize_rows=normalize, precision=np.float32, **ref) if precision == np.float32 else None
            tol = 1e-11 if own is None else max(1e-5, 2 * rel_err(own, want))
            e = rel_err(got.reshape(len(got), -1), want.reshape(len(want), -1))
            assert meta["rccl_ranks"] == world and meta["n_gpus"] == world and meta["dispatch_note"] == "", meta
            assert (lo, hi) == tuple(sharding.shard_range(n, rank, world))
            assert np.isfinite(got).all() and e <= tol, (kernel, what, e, tol, meta)
            report.append({"kernel": kernel, "what": what, "precision": np.dtype(precision).name, "shard": [lo, hi],
                           "rel_err": e, "device_kernel": meta["device_kernel"]})

        # sharded ridge solve: replicated Krylov vectors, operator summed over the ranks, the diagonal added once
        rs = np.random.RandomState(61)
        y, a = rs.rand(600, 3), rs.randn(600, 2)
        rtol = 1e-10
        A = mref.kernel_matrix(kernel=kernel, source_points=y) + 1e-2 * np.eye(600)
        dense = np.linalg.solve(A, a)
        algo = MI355XSolver(kernel=kernel, dimension=3, precision=np.float64, device=0, rtol=rtol, maxit=20000, comm=comm, ridge=1e-2)
        try:
            algo.prepare_data(source_points=y)
            algo.fit()
            algo.prepare_query(target_signal=a)
            algo.query()
            sol = algo.get_result()
            meta = algo.get_additional()
        finally:
            algo.done()
        e = float(np.max(np.linalg.norm(sol - dense, axis=0) / np.linalg.norm(dense, axis=0)))
        bound = float(np.linalg.cond(A)) * (1.5 * rtol + 1e-11)
        assert meta["cg_converged"] and meta["rccl_ranks"] == world and e <= bound, (kernel, e, bound, meta)
        report.append({"kernel": kernel, "what": "ridge solve", "iterations": meta["cg_iterations"], "rel_err": e, "bound": bound,
                       "device_kernel": meta["device_kernel"]})

    # every rank must hold the same answers: compare a digest
    digest = torch.tensor([sum(r["rel_err"] for r in report)], dtype=torch.float64)
    lo_t, hi_t = digest.clone(), digest.clone()
    dist.all_reduce(lo_t, op=dist.ReduceOp.MIN)
    dist.all_reduce(hi_t, op=dist.ReduceOp.MAX)
    assert float(lo_t[0]) == float(hi_t[0]), "ranks disagree on the results"
    if rank == 0:
        print(json.dumps({"world": world, "cases": report}), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
