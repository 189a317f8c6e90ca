#!/usr/bin/env python3
"""The preconditioned Lanczos quadrature (kmvp_<kernel>_lanczos_quadrature_precond) beside the plain one on one shape, and
the plain one on a build of the parent commit.  LAB_NOTES.md section 24 and the README row take their numbers from this.

    python tools/precond_lanczos_time.py [--n 100000] [--probes 16] [--ranks 16 64 128] [--rtol 1e-3] [--reps 1]
                                         [--parent-tree DIR] [--trace] [--json out.json]

Needs the GPU.  Config 5's cloud (uniform cube, D = 3, seed n + 3), float64, two systems: Gaussian with ridge 0.1 and
Matern 5/2 with ridge 0.01 (tools/precond_time.py's).  The plain arm runs kmvp_<kernel>_lanczos_quadrature on `probes`
Rademacher columns (seed 0); every rank runs the new entry on Rademacher (g, h) of the same seed, on one context: a first
call, which builds the factor, then `reps` more, which reuse it.  Reported per arm:
  steps               per column: smallest .. largest
  applications        operator applications: the call launches whole bursts of 8 iterations, 8 ceil(max steps / 8)
  wall_ms             median wall clock of the calls that reuse the factor (upload, probes, iteration, download, quadrature)
  ms_per_application  wall_ms / applications
  apply_share         (ms_per_application - the plain arm's) / ms_per_application: what the apply's three launches add to an
                      application, as far as the wall clock resolves it (--trace measures it directly)
  logquad_sd          sample standard deviation of logquad over the probes; logdet = [logdet_p +] mean logquad, its
                      standard error logquad_sd / sqrt(probes)
--parent-tree DIR: a checkout of the parent commit with its library built.  The plain arm is repeated in a child process
that imports the package from DIR, and reported as "parent".
--trace: one more Gaussian call at the largest rank, 16 iterations, in a child process under `rocprofv3 --kernel-trace`:
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
VECTOR_KERNELS = ("cg_", "lanczos_")  # the iteration's own kernels; everything else that is not pc_* is the operator's


def load(package_root):
    sys.path.insert(0, package_root)
    from kernel_matrix_benchmarks_amd import _lib
    return _lib


def signs(rows, probes, seed=0):
    return np.where(np.random.RandomState(seed).rand(rows, probes) < 0.5, -1.0, 1.0)


def summary(out, wall, probes):
    steps = out["steps"]
    apps = 8 * -(-int(steps.max()) // 8)
    wall_ms = float(np.median(wall))
    sd = float(np.std(out["logquad"], ddof=1))
    return {"steps": [int(steps.min()), int(steps.max())], "converged": bool(out["converged"]), "applications": apps,
            "wall_ms": wall_ms, "wall_ms_all": wall, "ms_per_application": wall_ms / apps, "logquad_sd": sd,
            "logdet": float(out.get("logdet_p", 0.0) + np.mean(out["logquad"])), "logdet_stderr": sd / np.sqrt(probes),
            "trace_inverse": float(np.mean(out["invquad"]))}


def run_arm(_lib, y, kernel, ridge, rank, probes, rtol, maxit, reps):
    n = y.shape[0]
    ctx = _lib.Context(0)
    try:
        ctx.set_points(y, None, _lib.KMVP_F64)
        ctx.fit(kernel)
        ctx.set_solver_diagonal(None, ridge)
        if rank:
            ctx.set_solver_preconditioner(rank)
            s = signs(n + rank, probes)
            g, h = np.ascontiguousarray(s[:n]), np.ascontiguousarray(s[n:])
            call = lambda: ctx.lanczos_quadrature_precond(kernel, g, h, rtol, maxit)
        else:
            z = np.ascontiguousarray(signs(n, probes))
            call = lambda: ctx.lanczos_quadrature(kernel, z, rtol, maxit)
        t0 = time.perf_counter()
        first = call()
        first_ms = (time.perf_counter() - t0) * 1e3
        extra = {"first_wall_ms": first_ms}
        if rank:
            extra.update(build_ms=ctx.last_preconditioner_ms, rank_built=ctx.last_preconditioner_rank,
                         logdet_p=first["logdet_p"])
        wall = []
        for _ in range(reps):
            t0 = time.perf_counter()
            out = call()
            wall.append((time.perf_counter() - t0) * 1e3)
            assert np.array_equal(out["steps"], first["steps"]) and (not rank or ctx.last_preconditioner_ms == 0.0)
        row = summary(out, wall, probes)
        row.update(extra, device_kernel=ctx.last_kernel_name, device_bytes=ctx.device_bytes)
        return row
    finally:
        ctx.close()


def child_trace(_lib, n, rank, probes):
    y = np.random.RandomState(n + 3).rand(n, 3)
    kernel, ridge = SYSTEMS[0]
    s = signs(n + rank, probes)
    ctx = _lib.Context(0)
    try:
        ctx.set_points(y, None, _lib.KMVP_F64)
        ctx.fit(kernel)
        ctx.set_solver_diagonal(None, ridge)
        ctx.set_solver_preconditioner(rank)
        ctx.lanczos_quadrature_precond(kernel, np.ascontiguousarray(s[:n]), np.ascontiguousarray(s[n:]), 1e-30, 16)
    finally:
        ctx.close()


def traced(n, rank, probes):
    """Kernel times of child_trace() in microseconds: per operator application and per apply."""
    prof = shutil.which("rocprofv3")
    if prof is None:
        return None
    tmp = tempfile.mkdtemp(prefix="precond_lanczos_time_")
    try:
        cmd = [prof, "--kernel-trace", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--child-trace", "--n", str(n), "--ranks", str(rank), "--probes", str(probes)]
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
        operator = sum(v for k, v in total.items() if not k.startswith("pc_") and not k.startswith(VECTOR_KERNELS))
        vector = sum(v for k, v in total.items() if k.startswith(VECTOR_KERNELS))
        apply_us = sum(total.get(k, 0.0) for k in APPLY_KERNELS) / applies
        return {"applies": applies, "operator_applications": products,
                "apply_us": {k: total.get(k, 0.0) / applies for k in APPLY_KERNELS}, "apply_us_total": apply_us,
                "operator_us": operator / products, "vector_kernels_us": vector / products,
                "apply_share_of_an_iteration": apply_us / (apply_us + (operator + vector) / products),
                "probe_us": total.get("pc_probe_kernel", 0.0), "logd_us": total.get("pc_logd_kernel", 0.0) + total.get("pc_logd_fold_kernel", 0.0),
                "kernels": {k: [count[k], total[k]] for k in sorted(total)}}
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--probes", type=int, default=16)
    ap.add_argument("--ranks", type=int, nargs="+", default=[16, 64, 128])
    ap.add_argument("--rtol", type=float, default=1e-3)
    ap.add_argument("--maxit", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--json", default=None)
    ap.add_argument("--package-root", default=here, help=argparse.SUPPRESS)
    ap.add_argument("--plain-only", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--child-trace", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    _lib = load(args.package_root)
    if args.child_trace:
        child_trace(_lib, args.n, args.ranks[0], args.probes)
        return

    y = np.random.RandomState(args.n + 3).rand(args.n, 3)
    report = {"n": args.n, "probes": args.probes, "rtol": args.rtol, "reps": args.reps, "systems": {}}
    for kernel, ridge in SYSTEMS:
        rows = {}
        for rank in [0] + ([] if args.plain_only else args.ranks):
            key = "plain" if rank == 0 else str(rank)
            rows[key] = run_arm(_lib, y, kernel, ridge, rank, args.probes, args.rtol, args.maxit, args.reps)
            if rank:
                rows[key]["apply_share"] = 1.0 - rows["plain"]["ms_per_application"] / rows[key]["ms_per_application"]
            print(f"{kernel} ridge {ridge} {'plain' if rank == 0 else f'rank {rank}'}: " + json.dumps(rows[key]), flush=True)
        report["systems"][f"{kernel}, ridge {ridge}"] = rows
    if args.plain_only:
        print("PLAIN " + json.dumps(report))
        return
    if args.parent_tree:
        cmd = [sys.executable, os.path.abspath(__file__), "--plain-only", "--package-root", os.path.abspath(args.parent_tree),
               "--n", str(args.n), "--probes", str(args.probes), "--rtol", str(args.rtol), "--maxit", str(args.maxit),
               "--reps", str(args.reps)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1200)
        lines = [l for l in done.stdout.splitlines() if l.startswith("PLAIN ")]
        if done.returncode != 0 or not lines:
            print(f"parent: the child returned {done.returncode}\n{done.stdout[-2000:]}")
        else:
            for name, rows in json.loads(lines[-1][6:])["systems"].items():
                report["systems"][name]["parent"] = rows["plain"]
                print(f"{name} parent commit: " + json.dumps(rows["plain"]), flush=True)
    if args.trace:
        report["trace"] = traced(args.n, max(args.ranks), args.probes)
        print("trace: " + json.dumps(report["trace"]), flush=True)
    print(json.dumps(report))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
