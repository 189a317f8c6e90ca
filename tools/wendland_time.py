#!/usr/bin/env python3
"""Times of the Wendland entries (kmvp_wendland_c2_cutoff, kmvp_wendland_c2_cg_solve: lowd_cutoff_kernel with wendland_value on
a cell list) next to the Gaussian cutoff of the same library on the same cloud and radius, in one process.  LAB_NOTES.md
section 34 and the README row take their numbers from this.

    python tools/wendland_time.py [--reps 3] [--warmup 1] [--n 1000000] [--neighbours 32,128] [--precisions float32,float64]
                                  [--rtol 1e-6] [--ridge 1e-2] [--json out.json]

Needs the GPU.  C2, D = 3, N = n points uniform in the unit cube, one right-hand side; the support radius with a mean of k
sources inside, R = (3 k / (4 pi n))^(1/3).  Arms per (precision, radius), the conventions of tools/cutoff_time.py:
  (a) wendland, query      kmvp_wendland_c2_cutoff on the cached plan: the call alone
  (b) gaussian, query      kmvp_gaussian_cutoff at the same R on the same plan: what the polynomial costs against the exponential
  (c) solve                kmvp_wendland_c2_cg_solve of (K + ridge I) b = a to rtol on the cached plan
  (d) solve, stale plan    the same solve after the plan was invalidated (the cell factor moved by one part in 1e9): host plan
                           build + uploads + the packs + the solve.  (d) - (c) is the plan + pack cost on its own
After `warmup` passes over all arms, `reps` passes with the arms interleaved.  Reported per arm: the median wall time (a host
clock around synchronous calls); for the products the median device pair-loop time; for the solve its iterations and its wall
time per operator application, wall / (iterations + 1): the applications of the iteration and the true residual's one.
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--neighbours", default="32,128", help="comma-separated mean numbers of inside sources per point")
    ap.add_argument("--precisions", default="float32,float64")
    ap.add_argument("--rtol", type=float, default=1e-6)
    ap.add_argument("--ridge", type=float, default=1e-2)
    ap.add_argument("--maxit", type=int, default=2000)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    n = args.n
    rs = np.random.RandomState(0)
    y64, a64 = rs.rand(n, 3), rs.randn(n, 1)
    report = {"D": 3, "kernel": "wendland-c2", "n": n, "reps": args.reps, "warmup": args.warmup, "rtol": args.rtol,
              "ridge": args.ridge, "cases": {}}
    for precision in args.precisions.split(","):
        npdt = np.dtype(precision).type
        code = _lib.KMVP_F64 if precision == "float64" else _lib.KMVP_F32
        y, a = np.ascontiguousarray(y64, dtype=npdt), np.ascontiguousarray(a64, dtype=npdt)
        ctx = _lib.Context(0)
        try:
            ctx.set_points(y, None, code)
            ctx.set_solver_diagonal(None, args.ridge)
            for k in (float(v) for v in args.neighbours.split(",")):
                R = (3.0 * k / (4.0 * np.pi * n)) ** (1.0 / 3.0)
                nudge = [0]
                last = {}

                def product(kernel):
                    ctx.set_signal(a)      # (a solve leaves no signal behind)
                    t0 = time.perf_counter()
                    ctx.run_cutoff(kernel, R, False)
                    return time.perf_counter() - t0, float(ctx.last_kernel_ms)

                def solve(stale):
                    if stale:
                        nudge[0] ^= 1
                        ctx.set_option("cutoff_cell_factor", 1.0 + 1e-9 * nudge[0])
                    t0 = time.perf_counter()
                    _, iters, resid, ok = ctx.cg_solve("wendland-c2", a, args.rtol, args.maxit, support_radius=R)
                    wall = time.perf_counter() - t0
                    last.update(iterations=iters, residual=resid, converged=bool(ok))
                    return wall, wall / (iters + 1)

                arms = {"wendland, query": lambda: product("wendland-c2"), "gaussian, query": lambda: product("gaussian"),
                        "solve": lambda: solve(False), "solve, stale plan": lambda: solve(True)}
                names = tuple(arms)
                for _ in range(args.warmup):
                    for name in names:
                        arms[name]()
                times = {name: [] for name in names}
                for rep in range(args.reps):
                    shift = rep % len(names)
                    for name in names[shift:] + names[:shift]:
                        times[name].append(arms[name]())
                info = ctx.cutoff_info()
                out = {"radius": R, "info": info, "arms": {}, **last}
                for name in names:
                    wall, second = (float(np.median([t[i] for t in times[name]])) for i in range(2))
                    key = "wall_per_application_ms" if name.startswith("solve") else "device_kernel_ms"
                    out["arms"][name] = {"wall_ms": 1e3 * wall, key: 1e3 * second if name.startswith("solve") else second,
                                         "wall_ms_all": [1e3 * t[0] for t in times[name]]}
                    print(f"{precision} k = {k:5.0f} R = {R:.5f} {name:20s} wall {1e3 * wall:10.3f} ms  {key} {out['arms'][name][key]:9.4f}")
                out["plan_and_pack_ms"] = out["arms"]["solve, stale plan"]["wall_ms"] - out["arms"]["solve"]["wall_ms"]
                print(f"{precision} k = {k:5.0f} {last['iterations']} iterations, residual {last['residual']:.3g}, converged "
                      f"{last['converged']}; plan + pack {out['plan_and_pack_ms']:.1f} ms (host plan {info['plan_ms']} ms) next to a solve "
                      f"of {out['arms']['solve']['wall_ms']:.1f} ms; cells {info['cells']} walked {info['walked']}")
                report["cases"][f"{precision},{k:g}"] = out
        finally:
            ctx.close()
    line = json.dumps(report)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
