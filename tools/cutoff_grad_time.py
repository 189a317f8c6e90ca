#!/usr/bin/env python3
"""Times of the cutoff-radius gradients (kmvp_<kernel>_cutoff_grad: lowd_cutoff_grad_kernel on the cell list) next to the
same kernel's cutoff product at the same radius on the same cached plan, in one process.  The LAB_NOTES.md section on the
cutoff gradients and the README row take their numbers from this.

    python tools/cutoff_grad_time.py [--reps 3] [--warmup 1] [--n 1000000] [--neighbours 32,128] [--plain-n 100000] [--json out.json]

Needs the GPU.  D = 3, N = M = n points uniform in the unit cube, targets == sources, one signal column, float32 and
float64; the radius with a mean of k inside sources per target, R = (3 k / (4 pi n))^(1/3).  Kernels: the Gaussian and
Wendland C2.  Arms per (precision, kernel, radius), on ONE context so that both read the same plan and the same records:
  (a) product    kmvp_<kernel>_cutoff
  (b) gradient   kmvp_<kernel>_cutoff_grad
After `warmup` passes over both arms, `reps` passes with the arms interleaved (the order alternates).  Reported per arm: the
median wall time (a host clock around synchronous calls) and the median kmvp_last_total_ms / kmvp_last_kernel_ms (device
events), and the ratio gradient / product of the pair loops.
Last, kmvp_gaussian_grad on ALL pairs of the first plain-n points in float32 (lowd_grad_kernel), same protocol: its pair
loop times (n / plain-n)^2 is an EXTRAPOLATION to the cloud's size by the pair count, printed as such.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from kernel_matrix_benchmarks_amd import _lib  # noqa: E402

KERNELS = ("gaussian", "wendland-c2")


def timed(fn, ctx):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0, float(ctx.last_total_ms), float(ctx.last_kernel_ms)


def medians(samples):
    return tuple(float(np.median([t[i] for t in samples])) for i in range(3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--neighbours", default="32,128", help="comma-separated mean numbers of inside sources per target")
    ap.add_argument("--plain-n", type=int, default=100000, help="points of the all-pairs kmvp_gaussian_grad arm")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    n = args.n
    rs = np.random.RandomState(0)
    y64 = rs.rand(n, 3)
    b64 = rs.randn(n, 1)
    report = {"D": 3, "E": 1, "n": n, "reps": args.reps, "warmup": args.warmup, "runs": []}
    for prec, code, npdt in (("float32", _lib.KMVP_F32, np.float32), ("float64", _lib.KMVP_F64, np.float64)):
        ctx = _lib.Context(0)
        try:
            ctx.set_points(np.ascontiguousarray(y64, dtype=npdt), None, code)
            ctx.set_signal(np.ascontiguousarray(b64, dtype=npdt))
            for k in (float(v) for v in args.neighbours.split(",")):
                R = (3.0 * k / (4.0 * np.pi * n)) ** (1.0 / 3.0)
                for kernel in KERNELS:
                    arms = {"product": lambda: ctx.run_cutoff(kernel, R, False), "gradient": lambda: ctx.run_cutoff_grad(kernel, R)}
                    names = tuple(arms)
                    for _ in range(args.warmup):
                        for name in names:
                            timed(arms[name], ctx)
                    times = {name: [] for name in names}
                    for rep in range(args.reps):
                        for name in (names if rep % 2 == 0 else names[::-1]):
                            times[name].append(timed(arms[name], ctx))
                            assert ctx.last_kernel_name == ("lowd_cutoff_kernel" if name == "product" else "lowd_cutoff_grad_kernel")
                    info = ctx.cutoff_info()
                    out = {"precision": prec, "kernel": kernel, "k": k, "radius": R, "info": info, "arms": {}}
                    for name in names:
                        wall, total, loop = medians(times[name])
                        out["arms"][name] = {"wall_ms": 1e3 * wall, "device_total_ms": total, "device_kernel_ms": loop,
                                             "device_kernel_ms_all": [t[2] for t in times[name]]}
                        print(f"{prec} {kernel:12s} k = {k:5.0f} R = {R:.5f} {name:9s} wall {1e3 * wall:9.3f} ms  device total "
                              f"{total:9.3f} ms  pair loop {loop:9.3f} ms")
                    out["gradient_over_product"] = out["arms"]["gradient"]["device_kernel_ms"] / out["arms"]["product"]["device_kernel_ms"]
                    print(f"{prec} {kernel:12s} k = {k:5.0f} gradient / product (pair loops) = {out['gradient_over_product']:.3f}, "
                          f"walked records {info['walked']}")
                    report["runs"].append(out)
        finally:
            ctx.close()
    # the all-pairs gradient at a size where it is affordable
    m = min(args.plain_n, n)
    ctx = _lib.Context(0)
    try:
        ctx.set_points(np.ascontiguousarray(y64[:m], dtype=np.float32), None, _lib.KMVP_F32)
        ctx.set_signal(np.ascontiguousarray(b64[:m], dtype=np.float32))
        run = lambda: ctx.run_grad("gaussian")  # noqa: E731
        for _ in range(args.warmup):
            timed(run, ctx)
        wall, total, loop = medians([timed(run, ctx) for _ in range(args.reps)])
        scale = (n / float(m)) ** 2
        report["plain_gradient"] = {"kernel": "gaussian", "precision": "float32", "n": m, "device_kernel": ctx.last_kernel_name,
                                    "wall_ms": 1e3 * wall, "device_total_ms": total, "device_kernel_ms": loop,
                                    "extrapolated_to_n_ms": loop * scale}
        print(f"float32 gaussian     all pairs, n = {m}: {ctx.last_kernel_name} wall {1e3 * wall:9.3f} ms  device total {total:9.3f} ms  "
              f"pair loop {loop:9.3f} ms; times (n / {m})^2 = {scale:.0f}: {loop * scale:.1f} ms at n = {n} (EXTRAPOLATED by the pair count)")
    finally:
        ctx.close()
    line = json.dumps(report)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
