#!/usr/bin/env python3
"""Times of the cutoff-radius entries (kmvp_<kernel>_cutoff, kmvp_radius_count: lowd_cutoff_kernel, lowd_cutoff_count_kernel
on a cell list) next to the plain product of the same library on the same cloud, in one process.  LAB_NOTES.md section 33
and the README row take their numbers from this.

    python tools/cutoff_time.py [--reps 3] [--warmup 1] [--n 1000000] [--neighbours 32,128] [--json out.json]

Needs the GPU.  Gaussian, D = 3, float32, N = M = n points uniform in the unit cube, targets == sources, one signal column;
the radius with a mean of k inside sources per target, R = (3 k / (4 pi n))^(1/3).  Arms per radius:
  (a) cutoff, query          kmvp_gaussian_cutoff on the cached plan: the call alone
  (b) cutoff, stale plan     the same call after the plan was invalidated (the cell factor moved by one part in 1e9): host
                             plan build + uploads + the three packs + the call.  (b) - (a) is the plan + pack cost on its own;
                             the host's share of it is the info word plan_ms
  (c) count                  kmvp_radius_count on the cached plan
  (d) plain, default         kmvp_gaussian with the library's own dispatch (the kernel it took: reported)
  (e) plain, difference form kmvp_gaussian with fast_sqdists = 0 (lowd_kernel: the cutoff kernels' own pair arithmetic)
After `warmup` passes over all arms, `reps` passes with the arms interleaved.  Reported per arm: the median wall time (a host
clock around synchronous calls) and the median kmvp_last_total_ms / kmvp_last_kernel_ms (device events); from the info
words: walked pairs / (N M), walked pairs per inside pair, and the walked-pair rate of the pair loop.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from kernel_matrix_benchmarks_amd import _lib  # noqa: E402


def timed(fn, ctx):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0, float(ctx.last_total_ms), float(ctx.last_kernel_ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--neighbours", default="32,128", help="comma-separated mean numbers of inside sources per target")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    n = args.n
    rs = np.random.RandomState(0)
    y = rs.rand(n, 3).astype(np.float32)
    b = rs.randn(n, 1).astype(np.float32)
    cut, plain, diff = _lib.Context(0), _lib.Context(0), _lib.Context(0)
    report = {"D": 3, "precision": "float32", "kernel": "gaussian", "n": n, "reps": args.reps, "warmup": args.warmup, "radii": {}}
    try:
        diff.set_option("fast_sqdists", 0)
        for ctx in (cut, plain, diff):
            ctx.set_points(y, None, _lib.KMVP_F32)
            ctx.set_signal(b)
        plain_kernel = {}
        for k in (float(v) for v in args.neighbours.split(",")):
            R = (3.0 * k / (4.0 * np.pi * n)) ** (1.0 / 3.0)
            nudge = [0]

            def stale():
                nudge[0] ^= 1
                cut.set_option("cutoff_cell_factor", 1.0 + 1e-9 * nudge[0])
                cut.run_cutoff("gaussian", R, False)

            def plain_run(ctx, key):
                ctx.run("gaussian", False)
                plain_kernel[key] = ctx.last_kernel_name

            arms = {"cutoff, query": (lambda: cut.run_cutoff("gaussian", R, False), cut),
                    "cutoff, stale plan": (stale, cut),
                    "count": (lambda: cut.radius_count(R), cut),
                    "plain, default": (lambda: plain_run(plain, "default"), plain),
                    "plain, difference form": (lambda: plain_run(diff, "difference form"), diff)}
            names = tuple(arms)
            for _ in range(args.warmup):
                for name in names:
                    timed(*arms[name])
            times = {name: [] for name in names}
            for rep in range(args.reps):
                shift = rep % len(names)
                for name in names[shift:] + names[:shift]:
                    times[name].append(timed(*arms[name]))
            cut.run_cutoff("gaussian", R, False)
            info = cut.cutoff_info()
            inside = int(cut.radius_count(R).sum())
            out = {"radius": R, "info": info, "inside_pairs": inside, "walked_over_nm": info["walked"] / (float(n) * n),
                   "walked_per_inside": info["walked"] / max(inside, 1), "plain_kernels": dict(plain_kernel), "arms": {}}
            for name in names:
                wall, total, kernel = (float(np.median([t[i] for t in times[name]])) for i in range(3))
                out["arms"][name] = {"wall_ms": 1e3 * wall, "device_total_ms": total, "device_kernel_ms": kernel,
                                     "wall_ms_all": [1e3 * t[0] for t in times[name]]}
                print(f"k = {k:5.0f} R = {R:.5f} {name:24s} wall {1e3 * wall:10.3f} ms  device total {total:10.3f} ms  "
                      f"pair loop {kernel:10.3f} ms")
            q = out["arms"]["cutoff, query"]
            out["plan_and_pack_ms"] = out["arms"]["cutoff, stale plan"]["wall_ms"] - q["wall_ms"]
            out["walked_pairs_per_s"] = info["walked"] / (1e-3 * q["device_kernel_ms"]) if q["device_kernel_ms"] > 0 else None
            print(f"k = {k:5.0f} cells {info['cells']} tiles {info['tiles']} runs {info['runs']} walked / (N M) = "
                  f"{out['walked_over_nm']:.3e}, walked per inside pair = {out['walked_per_inside']:.2f} ({inside / n:.1f} inside per "
                  f"target), plan + pack {out['plan_and_pack_ms']:.1f} ms (host plan {info['plan_ms']} ms), "
                  f"{(out['walked_pairs_per_s'] or float('nan')) / 1e12:.2f}e12 walked pairs/s; plain: {plain_kernel}")
            report["radii"][str(k)] = out
    finally:
        for ctx in (cut, plain, diff):
            ctx.close()
    line = json.dumps(report)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
