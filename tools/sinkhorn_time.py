#!/usr/bin/env python3
"""Time per Sinkhorn iteration of the device-resident solver (kmvp_<kernel>_sinkhorn) against the two things it replaces,
on one shape, in one process.  LAB_NOTES.md section 18 and the README row take their numbers from this.

    python tools/sinkhorn_time.py [--n 200000] [--iters 100] [--host-iters 20] [--reps 3] [--eps 0.05] [--json out.json]

Needs the GPU.  N = M = n, D = 3, float32, Gaussian cost, uniform weights, x = rand, y = rand + (0.25, 0, 0), points scaled by
1 / sqrt(eps); `iters` iterations with tol = 0 (so the solver returns KMVP_E_NOT_CONVERGED at maxit, by design).  Arms:

  solver        MI355XSinkhorn.query(): kmvp_last_total_ms / iters (events around the whole solve) and wall clock / iters
  host loop     what a caller writes on the log-sum-exp alone: two MI355XProduct instances (targets x over sources y, and
                the roles swapped); per half-step the N potentials come to the host, log-weights are added,
                prepare_query() uploads and repacks, query_logsumexp() runs.  Wall clock / iteration over `host_iters`
  2 x bare lse  twice kmvp_last_total_ms of one kmvp_gaussian_logsumexp at the shape (median of 5 after a warm-up): the
                floor of any iteration built on that kernel

Each arm runs `reps` times after one warm-up run; the median is reported.  Stated, not asserted: the solver is no slower
than the host loop and within launch overhead of two bare log-sum-exps.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from kernel_matrix_benchmarks_amd.algorithms.mi355x import MI355XProduct, MI355XSinkhorn  # noqa: E402


def host_loop(px, py, log_a, log_b, iters):
    """v = T2(u), u = T1(v) through query_logsumexp(); px: targets x over sources y, py: targets y over sources x."""
    u = np.zeros(log_a.shape[0])
    for _ in range(iters):
        py.prepare_query(source_signal=(u + log_a).reshape(-1, 1))
        py.query_logsumexp()
        v = -py.get_logsumexp()[:, 0]
        px.prepare_query(source_signal=(v + log_b).reshape(-1, 1))
        px.query_logsumexp()
        u = -px.get_logsumexp()[:, 0]
    return u, v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--host-iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--eps", type=float, default=0.05)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    rs = np.random.RandomState(0)
    n = args.n
    x = rs.rand(n, 3)
    y = rs.rand(n, 3) + np.array([0.25, 0.0, 0.0])
    scale = 1.0 / np.sqrt(args.eps)
    log_w = np.full(n, -np.log(n))

    solver = MI355XSinkhorn(kernel="gaussian", dimension=3, eps=args.eps, precision=np.float32, tol=0.0, maxit=args.iters)
    px = MI355XProduct(kernel="gaussian", dimension=3, precision=np.float32, fast_sqdists=False)
    py = MI355XProduct(kernel="gaussian", dimension=3, precision=np.float32, fast_sqdists=False)
    try:
        solver.prepare_data(source_points=y, target_points=x)
        solver.fit()
        px.prepare_data(source_points=y * scale, target_points=x * scale)
        py.prepare_data(source_points=x * scale, target_points=y * scale)
        px.fit()
        py.fit()

        solver_dev, solver_wall = [], []
        for rep in range(args.reps + 1):
            t0 = time.perf_counter()
            solver.query()
            wall = (time.perf_counter() - t0) * 1e3
            extra = solver.get_additional()
            assert extra["iterations"] == args.iters and extra["device_kernel"] == "lowd_lse_kernel", extra
            if rep:  # the first run packs and warms up
                solver_dev.append(extra["device_total_ms"] / args.iters)
                solver_wall.append(wall / args.iters)
            print(f"solver     run {rep}: {extra['device_total_ms'] / args.iters:8.3f} ms / iteration on the device, "
                  f"{wall / args.iters:8.3f} wall ({args.iters} iterations, marginal error {extra['marginal_error']:.3e})")
        u_solver = solver.get_potentials()[0] / args.eps

        host_wall = []
        for rep in range(args.reps + 1):
            t0 = time.perf_counter()
            u_host, _ = host_loop(px, py, log_w, log_w, args.host_iters)
            wall = (time.perf_counter() - t0) * 1e3
            if rep:
                host_wall.append(wall / args.host_iters)
            print(f"host loop  run {rep}: {wall / args.host_iters:8.3f} ms / iteration wall ({args.host_iters} iterations)")

        bare = []
        px.prepare_query(source_signal=(u_host + log_w).reshape(-1, 1))
        for rep in range(6):
            px.query_logsumexp()
            if rep:
                bare.append(px.get_additional()["device_total_ms"])
        print(f"bare lse   kmvp_last_total_ms: median {np.median(bare):8.3f} ms (min {min(bare):.3f}, max {max(bare):.3f})")
    finally:
        solver.done()
        px.done()
        py.done()

    report = {"n": n, "D": 3, "precision": "float32", "kernel": "gaussian", "eps": args.eps, "iters": args.iters,
              "host_iters": args.host_iters, "reps": args.reps,
              "solver_ms_per_iteration_device": float(np.median(solver_dev)),
              "solver_ms_per_iteration_wall": float(np.median(solver_wall)),
              "host_loop_ms_per_iteration_wall": float(np.median(host_wall)),
              "two_bare_logsumexp_ms": 2.0 * float(np.median(bare)),
              # the same iterates either way, up to float32: the host loop's u after host_iters is not the solver's after iters
              "max_abs_u_solver": float(np.max(np.abs(u_solver)))}
    line = json.dumps(report)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
