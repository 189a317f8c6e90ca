#!/usr/bin/env python3
"""Per-iteration time of the device-resident Lloyd iteration (kmvp_kmeans) next to (a) one kmvp_nearest(K = 1) on the same
N x C and (b) the host Lloyd loop a caller had to write before it -- prepare_data with the new centroids, query_nearest(1),
np.add.at -- in one process.  LAB_NOTES.md section 22 and the README row take their numbers from this.

    python tools/kmeans_time.py [--n 1000000] [--clusters 64 1024] [--iters 20] [--reps 3] [--warmup 1] [--host-iters 3]
                                [--trace] [--json out.json]

Needs the GPU.  float32, D = 3, uniform points in the unit cube, initial centroids = the first C points, tol = 0 and
maxit = iters (Lloyd does not converge within 20 iterations at these sizes; the returned count divides the time).
Reported per C, medians over `reps` interleaved passes after `warmup`:
  solve          kmvp_last_total_ms of kmvp_kmeans(maxit = iters) / iterations: the upload of the centroids and the download
                 of centroids and N labels included
  marginal       (solve(iters) - solve(iters / 2)) / (iters / 2): what one more iteration costs
  nearest        kmvp_nearest(K = 1), centroids as sources: kmvp_last_kernel_ms (the pair loop alone) and kmvp_last_total_ms
                 (with the segment merge and the finish, on the device)
  host loop      wall time per iteration of the host loop on the plugin API (MI355XProduct)
--trace runs one more solve per C in a child process under `rocprofv3 --kernel-trace` and adds the kernels' own times per
iteration: the update's share (km_update_kernel + km_reduce_kernel) of the six launches.
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

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from kernel_matrix_benchmarks_amd import _lib  # noqa: E402
from kernel_matrix_benchmarks_amd.algorithms.mi355x import MI355XProduct  # noqa: E402

D = 3
KERNELS = ("km_records_kernel", "lowd_knn_kernel", "knn_merge_kernel", "km_update_kernel", "km_reduce_kernel", "km_scalars_kernel")


def points(n):
    return np.random.RandomState(0).rand(n, D).astype(np.float32)


def solve(ctx, C, c0, maxit):
    cent, labels, cw, iters, inertia, shift, converged = ctx.kmeans(C, c0, None, 0.0, maxit)
    assert ctx.last_kernel_name == "lowd_knn_kernel" and iters >= 1
    return float(ctx.last_total_ms), iters


def host_loop(x, c0, iters):
    """The loop on the parent commit's API: every iteration re-uploads and re-packs all N points."""
    algo = MI355XProduct(kernel="gaussian", dimension=D, precision="float32", device=0)
    cent = np.array(c0, dtype=np.float64)
    x64 = x.astype(np.float64)
    per = []
    try:
        for _ in range(iters + 1):  # the first one is the warm-up
            t0 = time.perf_counter()
            algo.prepare_data(source_points=cent, target_points=x, same_points=False)
            algo.query_nearest(1)
            idx, _sq = algo.get_nearest()
            lab = idx[:, 0]
            sums = np.zeros_like(cent)
            np.add.at(sums, lab, x64)
            count = np.bincount(lab, minlength=len(cent)).astype(np.float64)
            cent = np.where(count[:, None] > 0, sums / np.maximum(count, 1.0)[:, None], cent)
            per.append((time.perf_counter() - t0) * 1e3)
    finally:
        algo.done()
    return per[1:]


def child(n, C, iters):
    """One warm-up solve and one more, for the profiler."""
    x = points(n)
    ctx = _lib.Context(0)
    try:
        ctx.set_points(x, None, _lib.KMVP_F32)
        for _ in range(2):
            solve(ctx, C, x[:C], iters)
    finally:
        ctx.close()


def traced(n, C, iters):
    """{kernel: microseconds per iteration} from a kernel trace of child(); None when the profiler is not there."""
    prof = shutil.which("rocprofv3")
    if prof is None:
        return None
    tmp = tempfile.mkdtemp(prefix="kmeans_time_")
    try:
        cmd = [prof, "--kernel-trace", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--child", "--n", str(n), "--clusters", str(C), "--iters", str(iters)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if done.returncode != 0 or not files:
            print(f"trace: rocprofv3 returned {done.returncode}, {len(files)} trace files\n{done.stdout[-2000:]}")
            return None
        total = {k: 0.0 for k in KERNELS}
        count = {k: 0 for k in KERNELS}
        for path in files:
            with open(path, newline="") as f:
                for row in csv.DictReader(f):
                    name = row.get("Kernel_Name", "")
                    for k in KERNELS:
                        if k in name:
                            total[k] += (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-3
                            count[k] += 1
        if not count["km_update_kernel"]:
            return None
        return {k: total[k] / count["km_update_kernel"] for k in KERNELS}  # one km_update_kernel per iteration
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--clusters", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-iters", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.child:
        child(args.n, args.clusters[0], args.iters)
        return

    x = points(args.n)
    half = max(1, args.iters // 2)
    report = {"n": args.n, "D": D, "precision": "float32", "iters": args.iters, "reps": args.reps, "warmup": args.warmup,
              "clusters": {}}
    for C in args.clusters:
        c0 = x[:C]
        km = _lib.Context(0)
        nn = _lib.Context(0)
        times = {"solve": [], "half": [], "nearest_kernel": [], "nearest_total": []}
        try:
            km.set_points(x, None, _lib.KMVP_F32)
            nn.set_points(np.ascontiguousarray(c0), x, _lib.KMVP_F32)
            for rep in range(args.warmup + args.reps):
                full_ms, full_it = solve(km, C, c0, args.iters)
                nn.run_nearest(1)
                near = (float(nn.last_kernel_ms), float(nn.last_total_ms))
                half_ms, half_it = solve(km, C, c0, half)
                if rep >= args.warmup:
                    times["solve"].append(full_ms / full_it)
                    times["half"].append((full_ms - half_ms) / max(1, full_it - half_it))
                    times["nearest_kernel"].append(near[0])
                    times["nearest_total"].append(near[1])
        finally:
            km.close()
            nn.close()
        host = host_loop(x, c0, args.host_iters)
        med = {k: float(np.median(v)) for k, v in times.items()}
        row = {"iterations": full_it, "solve_ms_per_iteration": med["solve"], "marginal_ms_per_iteration": med["half"],
               "nearest_kernel_ms": med["nearest_kernel"], "nearest_total_ms": med["nearest_total"],
               "host_loop_ms_per_iteration": float(np.median(host)),
               "solve/nearest_total": med["solve"] / med["nearest_total"],
               "host_loop/solve": float(np.median(host)) / med["solve"]}
        print(f"C = {C}: kmvp_kmeans {med['solve']:.3f} ms per iteration over {full_it} (min {min(times['solve']):.3f}, max "
              f"{max(times['solve']):.3f}, {args.reps} runs), one more iteration {med['half']:.3f} ms")
        print(f"C = {C}: (a) kmvp_nearest(K = 1) pair loop {med['nearest_kernel']:.3f} ms, with merge and finish "
              f"{med['nearest_total']:.3f} ms  -> an iteration is {row['solve/nearest_total']:.2f} of them")
        print(f"C = {C}: (b) host loop {row['host_loop_ms_per_iteration']:.1f} ms per iteration (min {min(host):.1f}, max "
              f"{max(host):.1f}, {args.host_iters} iterations)  -> {row['host_loop/solve']:.0f} x the device-resident iteration")
        if args.trace:
            per = traced(args.n, C, args.iters)
            if per is None:
                print(f"C = {C}: kernel trace not available: the update's share is not measured")
            else:
                whole = sum(per.values())
                update = per["km_update_kernel"] + per["km_reduce_kernel"]
                row["kernel_us_per_iteration"] = per
                row["update_share_of_kernels"] = update / whole
                row["update/assignment"] = update / (per["lowd_knn_kernel"] + per["knn_merge_kernel"])
                print(f"C = {C}: kernels per iteration (us): " + ", ".join(f"{k} {v:.1f}" for k, v in per.items()))
                print(f"C = {C}: the update (km_update_kernel + km_reduce_kernel) is {update:.1f} us = {update / whole:.2f} of the "
                      f"six launches' {whole:.1f} us, {row['update/assignment']:.2f} of the assignment (pair loop + merge)")
        report["clusters"][str(C)] = row
    line = json.dumps(report)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
