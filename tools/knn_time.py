#!/usr/bin/env python3
"""Kernel times of the K-nearest-neighbour reduction (lowd_knn_kernel) next to lowd_kernel's Gaussian density product on
the same clouds, in one process.  LAB_NOTES.md section 21 and the README row take their measured ratios from this.

    python tools/knn_time.py [--n 200000] [--reps 3] [--warmup 1] [--segments 0] [--json out.json]

Needs the GPU.  N = M = n, D = 3, float32, uniform points in the unit cube; targets == sources (one cloud) and != (two
clouds); K = 1, 4, 16 -- the three list capacities.  One context per cloud pair, fast_sqdists = 0 (the difference form) and
density estimation, so the product and the neighbour query read the SAME packed target image and source records.  After
`warmup` passes over all arms, `reps` passes with the arms interleaved; reported: the median kmvp_last_kernel_ms (the events
around the pair-loop kernel) per arm and its ratio to the product of the same cloud pair.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from kernel_matrix_benchmarks_amd import _lib  # noqa: E402

KS = (1, 4, 16)


def run_arm(ctx, arm):
    if arm == "product":
        ctx.run("gaussian", False)
        assert ctx.last_kernel_name == "lowd_kernel", ctx.last_kernel_name
    else:
        ctx.run_nearest(arm)
        assert ctx.last_kernel_name == "lowd_knn_kernel", ctx.last_kernel_name
    return float(ctx.last_kernel_ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--segments", type=int, default=0, help="source segments of every launch (0: each path's own rule)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    rs = np.random.RandomState(0)
    y = rs.rand(args.n, 3).astype(np.float32)
    x = rs.rand(args.n, 3).astype(np.float32)
    clouds = {"targets == sources": None, "targets != sources": x}
    arms = ("product",) + KS
    report = {"n": args.n, "D": 3, "precision": "float32", "reps": args.reps, "warmup": args.warmup, "segments": args.segments,
              "clouds": {}}
    for name, targets in clouds.items():
        ctx = _lib.Context(0)
        try:
            ctx.set_option("fast_sqdists", 0)
            if args.segments:
                ctx.set_option("segments", args.segments)
            ctx.set_points(y, targets, _lib.KMVP_F32)
            ctx.set_signal(None)
            for _ in range(args.warmup):
                for arm in arms:
                    run_arm(ctx, arm)
            times = {arm: [] for arm in arms}
            for rep in range(args.reps):
                shift = rep % len(arms)
                for arm in arms[shift:] + arms[:shift]:
                    times[arm].append(run_arm(ctx, arm))
        finally:
            ctx.close()
        med = {arm: float(np.median(v)) for arm, v in times.items()}
        row = {"product_kernel_ms": med["product"]}
        print(f"{name}: product (lowd_kernel, Gaussian density) median {med['product']:.3f} ms "
              f"(min {min(times['product']):.3f}, max {max(times['product']):.3f}, {args.reps} runs)")
        for K in KS:
            row[f"K={K}"] = {"kernel_ms": med[K], "nearest/product": med[K] / med["product"]}
            print(f"{name}: nearest K = {K:2d} (lowd_knn_kernel) median {med[K]:.3f} ms (min {min(times[K]):.3f}, max "
                  f"{max(times[K]):.3f})  nearest/product {med[K] / med['product']:.3f}")
        report["clouds"][name] = row
    line = json.dumps(report)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
