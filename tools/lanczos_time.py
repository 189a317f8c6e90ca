#!/usr/bin/env python3
"""Time of the Lanczos quadrature (kmvp_gaussian_lanczos_quadrature) against kmvp_gaussian_cg_solve on the same columns to
the same tolerance, on one shape, in one process.  LAB_NOTES.md and the README row take their numbers from this.

    python tools/lanczos_time.py [--n 100000] [--probes 16] [--rtol 1e-3] [--ridge 0.1] [--reps 3] [--json out.json]

Needs the GPU.  Config 5's cloud (uniform_cube(n, 3), seed n + 3), Gaussian, float64, A = K + ridge I (the bare matrix is
numerically singular: no residual test could accept a solve with random right-hand sides), `probes` Rademacher columns.
Both entries run the same products, dot products and vector updates per iteration; the quadrature adds one history row
per iteration and a host eigenproblem of `steps` rows per column at the end, and saves the true-residual product
cg_solve ends with.  Each arm runs `reps` times after one warm-up; the median of kmvp_last_total_ms (lanczos: events
around the whole call) and of the wall clock is reported, with the iteration counts, so that the time per operator
application can be compared as well.  Stated, not asserted.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from kernel_matrix_benchmarks_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--probes", type=int, default=16)
    ap.add_argument("--rtol", type=float, default=1e-3)
    ap.add_argument("--ridge", type=float, default=0.1)
    ap.add_argument("--maxit", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    n = args.n
    y = np.random.RandomState(n + 3).rand(n, 3)
    z = np.where(np.random.RandomState(0).rand(n, args.probes) < 0.5, -1.0, 1.0)
    ctx = _lib.Context(0)
    rows = {}
    try:
        ctx.set_points(y, None, _lib.KMVP_F64)
        ctx.fit("gaussian")
        ctx.set_solver_diagonal(None, args.ridge)

        def lanczos():
            out = ctx.lanczos_quadrature("gaussian", z, args.rtol, args.maxit)
            return int(out["steps"].max()), bool(out["converged"]), out

        def cg():
            _, iters, resid, ok = ctx.cg_solve("gaussian", z, args.rtol, args.maxit)
            return int(iters), bool(ok), resid

        for name, arm in (("cg_solve", cg), ("lanczos_quadrature", lanczos), ("cg_solve again", cg),
                          ("lanczos_quadrature again", lanczos)):
            arm()  # warm-up
            wall, dev = [], []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                iters, ok, extra = arm()
                wall.append((time.perf_counter() - t0) * 1e3)
                dev.append(ctx.last_total_ms)
            # operator applications: cg_solve launches whole bursts of 8 and ends with the true-residual product
            applications = 8 * -(-iters // 8) + (1 if name.startswith("cg") else 0)
            rows[name] = {"iterations": iters, "converged": ok, "wall_ms": float(np.median(wall)),
                          "device_ms": float(np.median(dev)) if name.startswith("lanczos") else None,
                          "wall_ms_per_application": float(np.median(wall)) / applications}
            if name == "lanczos_quadrature":
                rows[name]["log_det_estimate"] = float(extra["logquad"].mean())
                rows[name]["log_det_stderr"] = float(extra["logquad"].std(ddof=1) / np.sqrt(args.probes))
                rows[name]["steps"] = extra["steps"].tolist()
            print(name, json.dumps(rows[name]), flush=True)
        kernel = ctx.last_kernel_name
    finally:
        ctx.close()
    ratio = [rows["lanczos_quadrature" + s]["wall_ms"] / rows["cg_solve" + s]["wall_ms"] for s in ("", " again")]
    report = {"n": n, "probes": args.probes, "rtol": args.rtol, "ridge": args.ridge, "device_kernel": kernel, "arms": rows,
              "lanczos_over_cg_wall": ratio}
    print(json.dumps(report))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
