#!/usr/bin/env python3
"""Conjugate gradients with and without the pivoted-Cholesky preconditioner (kmvp_set_solver_preconditioner) on one shape, and
the same unpreconditioned solve on a build of the parent commit.  LAB_NOTES.md section 23 and the README row take their
numbers from this.

    python tools/precond_time.py [--n 100000] [--ranks 0 16 64 128] [--rtol 1e-6] [--reps 2] [--parent-tree DIR] [--trace]
                                 [--json out.json]

Needs the GPU.  Config 5's cloud (uniform cube, D = 3, seed n + 3: the Lanczos row's system), float64, one right-hand side
(randn, seed 0), two systems: Gaussian with ridge 0.1 and Matern 5/2 with ridge 0.01.  Per system and rank, on one context:
a first solve, which builds the factor (rank > 0), then `reps` more, which reuse it.  Reported:
  iterations, converged, rank_built
  build_ms            kmvp_last_preconditioner_ms of the first solve
  wall_ms             median wall clock of the solves that reuse the factor (upload, iteration, true residual, download)
  ms_per_iteration    wall_ms / operator applications: the solve launches whole bursts of 8 iterations and ends with one
                      more product for the true residual
  apply_ms            ms_per_iteration minus rank 0's: what the three launches of the apply and the second dot product add
                      per iteration, as far as the wall clock resolves it (--trace measures it directly)
--parent-tree DIR: a checkout of the parent commit with its library built.  The rank-0 solve is repeated in a child process
that imports the package from DIR, and reported as "parent" beside this tree's rank 0.
--trace: one more Gaussian solve at the largest rank, 16 iterations, in a child process under `rocprofv3 --kernel-trace`:
the kernels' own times per operator application and per apply.
Stated, not asserted.
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

SYSTEMS = (("gaussian", 0.1), ("matern-5/2", 0.01))
APPLY_KERNELS = ("pc_project_kernel", "pc_solve_kernel", "pc_finish_kernel")
VECTOR_KERNELS = ("cg_", "pcg_", "residual_")  # the iteration's own kernels; everything else is the operator's


def load(package_root):
    sys.path.insert(0, package_root)
    from kernel_matrix_benchmarks_amd import _lib
    return _lib


def inputs(n):
    return np.random.RandomState(n + 3).rand(n, 3), np.random.RandomState(0).randn(n, 1)


def applications(iters):
    return 8 * -(-iters // 8) + 1


def run_rank(_lib, y, a, kernel, ridge, rank, rtol, maxit, reps):
    ctx = _lib.Context(0)
    try:
        ctx.set_points(y, None, _lib.KMVP_F64)
        ctx.fit(kernel)
        ctx.set_solver_diagonal(None, ridge)
        if rank:
            ctx.set_solver_preconditioner(rank)
        t0 = time.perf_counter()
        _, iters, resid, ok = ctx.cg_solve(kernel, a, rtol, maxit)
        first = (time.perf_counter() - t0) * 1e3
        row = {"iterations": int(iters), "converged": bool(ok), "residual": float(resid), "first_wall_ms": first}
        if rank:
            row["build_ms"] = ctx.last_preconditioner_ms
            row["rank_built"] = ctx.last_preconditioner_rank
        wall = []
        for _ in range(reps):
            t0 = time.perf_counter()
            _, again, _, _ = ctx.cg_solve(kernel, a, rtol, maxit)
            wall.append((time.perf_counter() - t0) * 1e3)
            assert again == iters and (not rank or ctx.last_preconditioner_ms == 0.0)
        row["wall_ms"] = float(np.median(wall))
        row["wall_ms_all"] = wall
        row["ms_per_iteration"] = row["wall_ms"] / applications(iters)
        row["device_kernel"] = ctx.last_kernel_name
        row["device_bytes"] = ctx.device_bytes
        return row
    finally:
        ctx.close()


def child_trace(_lib, n, rank):
    y, a = inputs(n)
    kernel, ridge = SYSTEMS[0]
    ctx = _lib.Context(0)
    try:
        ctx.set_points(y, None, _lib.KMVP_F64)
        ctx.fit(kernel)
        ctx.set_solver_diagonal(None, ridge)
        ctx.set_solver_preconditioner(rank)
        ctx.cg_solve(kernel, a, 1e-30, 16)
    finally:
        ctx.close()


def traced(n, rank):
    """Kernel times of child_trace() in microseconds: per operator application, per apply, and the build's total."""
    prof = shutil.which("rocprofv3")
    if prof is None:
        return None
    tmp = tempfile.mkdtemp(prefix="precond_time_")
    try:
        cmd = [prof, "--kernel-trace", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--child-trace", "--n", str(n), "--ranks", str(rank)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if done.returncode != 0 or not files:
            print(f"trace: rocprofv3 returned {done.returncode}, {len(files)} trace files\n{done.stdout[-2000:]}")
            return None
        total, count = {}, {}
        for path in files:
            with open(path, newline="") as f:
                for r in csv.DictReader(f):
                    name = r.get("Kernel_Name", "").split("(")[0].split("<")[0].split()[-1].split("::")[-1]
                    total[name] = total.get(name, 0.0) + (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3
                    count[name] = count.get(name, 0) + 1
        applies = count.get("pc_finish_kernel", 0)
        products = count.get("cg_cast_kernel", 0)  # one per operator application
        if not applies or not products:
            return None
        build = sum(v for k, v in total.items() if k.startswith("pc_") and k not in APPLY_KERNELS)
        operator = sum(v for k, v in total.items() if not k.startswith("pc_") and not k.startswith(VECTOR_KERNELS))
        return {"applies": applies, "operator_applications": products,
                "apply_us": {k: total.get(k, 0.0) / applies for k in APPLY_KERNELS},
                "apply_us_total": sum(total.get(k, 0.0) for k in APPLY_KERNELS) / applies,
                "operator_us": operator / products, "build_kernels_us": build,
                "kernels": {k: [count[k], total[k]] for k in sorted(total)}}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--ranks", type=int, nargs="+", default=[0, 16, 64, 128])
    ap.add_argument("--rtol", type=float, default=1e-6)
    ap.add_argument("--maxit", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--json", default=None)
    ap.add_argument("--package-root", default=here, help=argparse.SUPPRESS)
    ap.add_argument("--plain-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--child-trace", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    _lib = load(args.package_root)
    if args.child_trace:
        child_trace(_lib, args.n, args.ranks[0])
        return

    y, a = inputs(args.n)
    report = {"n": args.n, "rtol": args.rtol, "reps": args.reps, "systems": {}}
    for kernel, ridge in SYSTEMS:
        rows = {}
        for rank in ([0] if args.plain_only else args.ranks):
            rows[str(rank)] = run_rank(_lib, y, a, kernel, ridge, rank, args.rtol, args.maxit, args.reps)
            if "0" in rows and rank:
                rows[str(rank)]["apply_ms"] = rows[str(rank)]["ms_per_iteration"] - rows["0"]["ms_per_iteration"]
            print(f"{kernel} ridge {ridge} rank {rank}: " + json.dumps(rows[str(rank)]), flush=True)
        report["systems"][f"{kernel}, ridge {ridge}"] = rows
    if args.plain_only:
        print("PLAIN " + json.dumps(report))
        return
    if args.parent_tree:
        cmd = [sys.executable, os.path.abspath(__file__), "--plain-only", "--package-root", os.path.abspath(args.parent_tree),
               "--n", str(args.n), "--rtol", str(args.rtol), "--maxit", str(args.maxit), "--reps", str(args.reps)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1200)
        lines = [l for l in done.stdout.splitlines() if l.startswith("PLAIN ")]
        if done.returncode != 0 or not lines:
            print(f"parent: the child returned {done.returncode}\n{done.stdout[-2000:]}")
        else:
            for name, rows in json.loads(lines[-1][6:])["systems"].items():
                report["systems"][name]["parent"] = rows["0"]
                print(f"{name} parent commit: " + json.dumps(rows["0"]), flush=True)
    if args.trace:
        report["trace"] = traced(args.n, max(args.ranks))
        print("trace: " + json.dumps(report["trace"]), flush=True)
    print(json.dumps(report))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
