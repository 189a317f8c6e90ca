#!/usr/bin/env python3
"""Time of the device-resident Gaussian mean-shift (kmvp_gaussian_meanshift) in three arms, in one process:
  (a) the solver;
  (b) the solver with "meanshift_compact" = 0: frozen points ride along, every sweep covers all N targets;
  (c) the host loop a caller had to write before it, on MI355XProduct: every sweep prepare_data with the moved targets,
      query_logsumexp_gradient, a download, the step in numpy -- all N targets every sweep, until the last one froze;
next to ONE bare kmvp_gaussian_logsumexp_grad at full N, the yardstick of a sweep in the same run.  LAB_NOTES.md section 27
and the README row take their numbers from this.

    python tools/meanshift_time.py [--n 200000] [--tol 1e-4] [--maxit 2000] [--reps 3] [--warmup 1] [--host-reps 3]
                                   [--trace] [--json out.json]

Needs the GPU.  float32, D = 3, N = M = n points of the test cloud (tests/meanshift_reference.py cloud()), seeds = the
points themselves.  Reported, medians over `reps` passes after `warmup`:
  sweeps, target_sweeps / (N sweeps)   the share of the naive loop's pair evaluations the solver spends
  total ms per arm                     (a), (b): kmvp_last_total_ms, upload of nothing, download of modes, iters, step2
                                       included; (c): wall time
  ms per sweep / bare gradient         total / sweeps over kmvp_last_total_ms of the bare gradient
--trace runs one more solve in a child process under `rocprofv3 --kernel-trace` and adds the kernels' own times: the
share of pack + step + compaction + state next to the pair loop (and its segment merge).
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import meanshift_reference as mr  # noqa: E402
from kernel_matrix_benchmarks_amd import _lib  # noqa: E402
from kernel_matrix_benchmarks_amd.algorithms.mi355x import MI355XProduct  # noqa: E402

D = 3
OWN = ("ms_pack_kernel", "ms_step_kernel", "ms_state_kernel", "ms_init_kernel")
PAIR = ("lowd_lse_grad_kernel", "lse_grad_reduce_kernel")


def points(n):
    return np.ascontiguousarray(mr.cloud(n, D), dtype=np.float32)


def context(x, compact):
    ctx = _lib.Context(0)
    if not compact:
        ctx.set_option("meanshift_compact", 0)
    ctx.set_points(x, None, _lib.KMVP_F32)
    ctx.set_signal(None)
    return ctx


def solve(ctx, tol, maxit):
    out = ctx.meanshift(tol, maxit)
    assert ctx.last_kernel_name == "lowd_lse_grad_kernel"
    return float(ctx.last_total_ms), out


def host_loop(x, tol, maxit):
    """The loop on the parent commit's API: every sweep re-uploads and re-packs all N targets and downloads all N rows."""
    algo = MI355XProduct(kernel="gaussian", dimension=D, precision="float32", device=0)
    zeros = np.zeros((x.shape[0], 1), dtype=np.float32)

    def grad(targets):
        algo.prepare_data(source_points=x, target_points=targets, same_points=False)
        algo.fit()
        algo.prepare_query(source_signal=zeros)
        algo.query_logsumexp_gradient()
        return algo.get_logsumexp_gradient()[:, 0, :]

    try:
        t0 = time.perf_counter()
        out = mr.meanshift(grad, x, tol, maxit, precision=np.float32, all_rows=True)
        return (time.perf_counter() - t0) * 1e3, out
    finally:
        algo.done()


def child(n, tol, maxit):
    """One warm-up solve and one more, for the profiler."""
    ctx = context(points(n), True)
    try:
        for _ in range(2):
            solve(ctx, tol, maxit)
    finally:
        ctx.close()


def traced(n, tol, maxit):
    """{kernel: milliseconds per solve} from a kernel trace of child(); None when the profiler is not there."""
    prof = shutil.which("rocprofv3")
    if prof is None:
        return None
    tmp = tempfile.mkdtemp(prefix="meanshift_time_")
    try:
        cmd = [prof, "--kernel-trace", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__),
               "--child", "--n", str(n), "--tol", repr(tol), "--maxit", str(maxit)]
        done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if done.returncode != 0 or not files:
            print(f"trace: rocprofv3 returned {done.returncode}, {len(files)} trace files\n{done.stdout[-2000:]}")
            return None
        total = {}
        for path in files:
            with open(path, newline="") as f:
                for row in csv.DictReader(f):
                    name = row.get("Kernel_Name", "")
                    key = next((k for k in OWN + PAIR if k in name), None)
                    if key is None:  # whatever else ran between the solver's launches: the stream compaction's kernels
                        key = "compaction" if ("rocprim" in name or "hipcub" in name or "select" in name.lower()) else "other"
                    total[key] = total.get(key, 0.0) + (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-6
        if "ms_step_kernel" not in total:
            return None
        return {k: v / 2 for k, v in total.items()}  # two solves in the child
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--tol", type=float, default=1e-4)
    ap.add_argument("--maxit", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--host-reps", type=int, default=None, help="passes of arm (c) after one warm-up (default: --reps)")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    if args.child:
        child(args.n, args.tol, args.maxit)
        return

    x = points(args.n)
    N = args.n
    a, b = context(x, True), context(x, False)
    bare = context(x, True)
    times = {"solver": [], "riding": [], "bare": []}
    try:
        for rep in range(args.warmup + args.reps):
            ms_a, out_a = solve(a, args.tol, args.maxit)
            ms_b, out_b = solve(b, args.tol, args.maxit)
            bare.run_lse_grad("gaussian")
            ms_bare = float(bare.last_total_ms)
            print(f"pass {rep}: solver {ms_a:.1f} ms, without compaction {ms_b:.1f} ms, bare gradient {ms_bare:.3f} ms", flush=True)
            if rep >= args.warmup:
                times["solver"].append(ms_a)
                times["riding"].append(ms_b)
                times["bare"].append(ms_bare)
        same = all(np.array_equal(out_a[k], out_b[k], equal_nan=True) for k in ("modes", "iters", "step2", "sweeps", "target_sweeps"))
    finally:
        a.close()
        b.close()
        bare.close()
    host_reps = args.reps if args.host_reps is None else args.host_reps
    host = []
    host_same = None
    for rep in range((1 if host_reps else 0) + host_reps):
        ms_c, out_c = host_loop(x, args.tol, args.maxit)
        print(f"host pass {rep}: {ms_c:.1f} ms over {out_c['sweeps']} sweeps", flush=True)
        host_same = all(np.array_equal(out_a[k], out_c[k], equal_nan=True) for k in ("modes", "iters", "step2", "sweeps", "target_sweeps"))
        if rep >= 1:
            host.append(ms_c)
    med = {k: float(np.median(v)) for k, v in times.items()}
    sweeps, ts = out_a["sweeps"], out_a["target_sweeps"]
    report = {"n": N, "D": D, "precision": "float32", "tol": args.tol, "maxit": args.maxit, "reps": args.reps, "warmup": args.warmup,
              "sweeps": sweeps, "target_sweeps": ts, "active_share": ts / (N * sweeps), "converged": bool(out_a["converged"]),
              "unconverged": int(np.sum(~(out_a["step2"] <= args.tol ** 2))),
              "solver_ms": med["solver"], "solver_ms_min_max": [min(times["solver"]), max(times["solver"])],
              "without_compaction_ms": med["riding"], "without_compaction_ms_min_max": [min(times["riding"]), max(times["riding"])],
              "bare_gradient_ms": med["bare"], "same_bits_without_compaction": bool(same),
              "solver_ms_per_sweep/bare": med["solver"] / sweeps / med["bare"],
              "without_compaction_ms_per_sweep/bare": med["riding"] / sweeps / med["bare"],
              "solver_ms_per_target_sweep_of_N/bare": med["solver"] / (ts / N) / med["bare"]}
    print(f"N = M = {N}: {sweeps} sweeps, target_sweeps / (N sweeps) = {report['active_share']:.4f}, converged {report['converged']} "
          f"({report['unconverged']} seeds open)")
    print(f"(a) solver {med['solver']:.1f} ms (min {min(times['solver']):.1f}, max {max(times['solver']):.1f}, {args.reps} runs) = "
          f"{med['solver'] / sweeps:.3f} ms per sweep = {report['solver_ms_per_sweep/bare']:.3f} bare gradients of {med['bare']:.3f} ms")
    print(f"(b) without compaction {med['riding']:.1f} ms (min {min(times['riding']):.1f}, max {max(times['riding']):.1f}) = "
          f"{med['riding'] / sweeps:.3f} ms per sweep = {report['without_compaction_ms_per_sweep/bare']:.3f} bare gradients; same bits: {same}")
    print(f"    per N active targets the solver spends {report['solver_ms_per_target_sweep_of_N/bare']:.3f} bare gradients: what the "
          "pinned geometry, the small launches of the tail and the solver's own kernels cost together")
    if host:
        report.update(host_loop_ms=float(np.median(host)), host_loop_ms_min_max=[min(host), max(host)], host_loop_same_bits=bool(host_same),
                      **{"host_loop/solver": float(np.median(host)) / med["solver"],
                         "host_loop_ms_per_sweep/bare": float(np.median(host)) / sweeps / med["bare"]})
        print(f"(c) host loop {np.median(host):.1f} ms (min {min(host):.1f}, max {max(host):.1f}, {len(host)} runs) = "
              f"{np.median(host) / sweeps:.3f} ms per sweep = {report['host_loop_ms_per_sweep/bare']:.2f} bare gradients, "
              f"{report['host_loop/solver']:.1f} x the solver; same bits: {host_same}")
    if args.trace:
        per = traced(N, args.tol, args.maxit)
        if per is None:
            print("kernel trace not available: the share of the solver's own kernels is not measured")
        else:
            own = sum(v for k, v in per.items() if k in OWN or k == "compaction")
            pair = sum(v for k, v in per.items() if k in PAIR)
            report["kernel_ms_per_solve"] = per
            report["own_kernels/pair_loop"] = own / pair
            print("kernels per solve (ms): " + ", ".join(f"{k} {v:.2f}" for k, v in sorted(per.items())))
            print(f"pack + step + compaction + state: {own:.2f} ms next to {pair:.2f} ms of the pair loop and its merge = {own / pair:.3f}")
    line = json.dumps(report)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
