#!/usr/bin/env python3
"""Kernel times of the length-scale derivative (lowd_dscale_kernel) next to the gradient (lowd_grad_kernel) on one
shape, in one process and on one context per kernel function: the Gaussian and exp(-r).  LAB_NOTES.md section 20 takes
its measured ratios from this.

    python tools/dscale_time.py [--n 200000] [--reps 3] [--warmup 1] [--json out.json]

Needs the GPU.  N = M = n, D = 3, E = 1, float32, fast_sqdists = 0 (the difference form).  The points and the signal
are packed once per context (both kernels read the product's LAYOUT_LOWD image); after `warmup` passes over both arms,
`reps` passes with the arms alternating, the starting arm rotating.  Reported: every kmvp_last_kernel_ms (the events
around the pair-loop kernel), the median per arm and the ratio dscale / gradient.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from kernel_matrix_benchmarks_amd import _lib  # noqa: E402

ARMS = ("gradient", "dscale")
EXPECTED = {"gradient": "lowd_grad_kernel", "dscale": "lowd_dscale_kernel"}


def run_arm(ctx, kernel, arm):
    (ctx.run_grad if arm == "gradient" else ctx.run_dscale)(kernel)
    assert ctx.last_kernel_name == EXPECTED[arm], (arm, ctx.last_kernel_name)
    return float(ctx.last_kernel_ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    rs = np.random.RandomState(0)
    y = rs.rand(args.n, 3).astype(np.float32)
    x = rs.rand(args.n, 3).astype(np.float32)
    b = rs.randn(args.n, 1).astype(np.float32)
    report = {"n": args.n, "D": 3, "E": 1, "precision": "float32", "reps": args.reps, "kernels": {}}
    for kernel in ("gaussian", "absolute-exponential"):
        ctx = _lib.Context(0)
        try:
            ctx.set_option("fast_sqdists", 0)
            ctx.set_points(y, x, _lib.KMVP_F32)
            ctx.set_signal(b)
            for _ in range(args.warmup):
                for arm in ARMS:
                    run_arm(ctx, kernel, arm)
            times = {arm: [] for arm in ARMS}
            for rep in range(args.reps):
                for arm in (ARMS if rep % 2 == 0 else ARMS[::-1]):
                    times[arm].append(run_arm(ctx, kernel, arm))
        finally:
            ctx.close()
        med = {arm: float(np.median(v)) for arm, v in times.items()}
        report["kernels"][kernel] = {"kernel_ms": times, "median_ms": med, "dscale/gradient": med["dscale"] / med["gradient"]}
        for arm in ARMS:
            print(f"{kernel:22s} {arm:9s} median {med[arm]:8.3f} ms  ({', '.join(f'{t:.3f}' for t in times[arm])})")
        print(f"{kernel:22s} dscale/gradient {med['dscale'] / med['gradient']:.3f}")
    line = json.dumps(report)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
