"""One rank of tests/test_gpu_dscale.py::test_two_ranks_on_one_gpu (started with RANK / WORLD_SIZE / MASTER_* in the
environment), after the pattern of _matern_rank_worker.py.

Every rank drives the plugins on GPU 0 with the sources sharded over the ranks, through the real libkmvp.so; the
exchange is staged through host memory and summed by gloo (include/kmvp.h kmvp_comm_init_host) -- test infrastructure,
selected explicitly.  The length-scale derivative of the product (every kernel, float64 and float32) and one
Gaussian-process likelihood gradient of the solver; every rank must hold the same bits.
"""
import hashlib
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

    import dscale_reference as dref
    import matern_reference
    from conftest import rel_err
    from kernel_matrix_benchmarks_amd.algorithms.mi355x import MI355XProduct, MI355XSolver

    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    comm = sharding.torch_gloo_communicator(exchange="host")
    report, bits = [], hashlib.sha256()

    def rounded(a, precision):
        return np.asarray(a, dtype=precision).astype(np.float64)

    for kernel in dref.KERNELS:
        # (precision, n, E, x != y)
        for precision, n, E, other in ((np.float64, 1003, 2, True), (np.float32, 2001, 1, False)):
            rs = np.random.RandomState(n + E)
            y, b = rounded(rs.rand(n, 3), precision), rounded(rs.randn(n, E), precision)
            x = rounded(rs.rand(n // 2 + 3, 3), precision) if other else None
            algo = MI355XProduct(kernel=kernel, dimension=3, precision=precision, device=0, comm=comm)
            try:
                algo.prepare_data(source_points=y, target_points=y if x is None else x, same_points=x is None)
                algo.fit()
                algo.prepare_query(source_signal=b)
                algo.query_scale_derivative()
                got = algo.get_scale_derivative()
                meta = algo.get_additional()
                lo, hi = algo.shard
            finally:
                algo.done()
            ref = dict(kernel=kernel, source_points=y, target_points=x, source_signal=b)
            want = dref.scale_derivative(**ref)
            tol = 1e-11
            if precision == np.float32:
                own = dref.scale_derivative(precision=np.float32, **ref)
                tol = max(1e-5, 2 * rel_err(own.reshape(len(own), -1), want.reshape(len(want), -1)))
            e = rel_err(got.reshape(len(got), -1), want.reshape(len(want), -1))
            assert meta["rccl_ranks"] == world and meta["n_gpus"] == world and meta["dispatch_note"] == "", meta
            assert (lo, hi) == tuple(sharding.shard_range(n, rank, world))
            assert np.isfinite(got).all() and e <= tol, (kernel, e, tol, meta)
            bits.update(got.tobytes())
            report.append({"kernel": kernel, "what": "dscale", "precision": np.dtype(precision).name, "shard": [lo, hi],
                           "rel_err": e, "device_kernel": meta["device_kernel"]})

    # the likelihood gradient with the operator sharded: replicated vectors, H [z | alpha] summed over the ranks
    kernel, n, E, ridge, rtol = "matern-5/2", 600, 2, 0.1, 1e-8
    rs = np.random.RandomState(603)
    y, a = 3.0 * rs.rand(n, 3), rs.randn(n, E)
    algo = MI355XSolver(kernel=kernel, dimension=3, precision=np.float64, device=0, rtol=rtol, maxit=5000, comm=comm, ridge=ridge)
    try:
        algo.prepare_data(source_points=y)
        algo.fit()
        algo.prepare_query(target_signal=a)
        algo.query()
        value = algo.log_marginal_likelihood(probes=32, seed=0)
        got = algo.log_marginal_likelihood_gradient(probes=32, seed=0)
        meta = algo.get_additional()
    finally:
        algo.done()
    A = matern_reference.kernel_matrix(kernel=kernel, source_points=y) + ridge * np.eye(n)
    dA = dref.scale_derivative(kernel=kernel, source_points=y, source_signal=np.eye(n))
    invA = np.linalg.inv(A)
    alpha = invA @ a
    exact = 0.5 * np.einsum("ie,ijd,je->d", alpha, dA, alpha) - 0.5 * E * np.einsum("ij,jid->d", invA, dA)
    dev = np.abs(got.d_log_lengthscale - exact) / got.d_log_lengthscale_stderr
    assert meta["cg_converged"] and meta["rccl_ranks"] == world and got.converged, meta
    assert (got.value, got.value_stderr) == value and (dev <= 4).all(), (got, value, exact)
    for v in got[:6]:
        bits.update(np.asarray(v, dtype=np.float64).tobytes())
    report.append({"kernel": kernel, "what": "likelihood gradient", "d_log_lengthscale": got.d_log_lengthscale.tolist(),
                   "exact": exact.tolist(), "stderrs_off": dev.tolist(), "device_kernel": meta["device_kernel"]})

    # every rank must hold the same bits
    digest = torch.tensor(np.frombuffer(bits.digest(), dtype=np.int64).copy())
    lo_t, hi_t = digest.clone(), digest.clone()
    dist.all_reduce(lo_t, op=dist.ReduceOp.MIN)
    dist.all_reduce(hi_t, op=dist.ReduceOp.MAX)
    identical = bool(torch.equal(lo_t, hi_t))
    assert identical, "ranks disagree on the results"
    if rank == 0:
        print(json.dumps({"world": world, "identical_bits": identical, "cases": report}), flush=True)
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
