#!/usr/bin/env python3
"""Kernel times of the difference-form family on one shape, in one process: product (lowd_kernel), gradient
(lowd_grad_kernel), log-sum-exp (lowd_lse_kernel) and the log-sum-exp's gradient (lowd_lse_grad_kernel), for the Gaussian
and exp(-r).  LAB_NOTES.md sections 13, 15 and 16 take their measured ratios from this.

    python tools/lse_family_time.py [--n 200000] [--reps 25] [--rounds 2] [--warmup 5] [--json out.json]

Needs the GPU.  N = M = n, D = 3, E = 1, float32, fast_sqdists = 0 (the difference form).  One context per kernel
function, packed once; after `warmup` passes over all arms (clocks and code objects settled), `rounds` rounds of `reps`
passes with the arms INTERLEAVED (every pass runs each arm once, the starting arm rotating), so that drift of the clocks
or a neighbour's load falls on all arms alike.  Reported: the median device_kernel_ms (the events around the pair-loop
kernel) per arm and round, and the ratios to the product and to the gradient of the same kernel function.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from kernel_matrix_benchmarks_amd import _lib  # noqa: E402

ARMS = ("product", "gradient", "logsumexp", "logsumexp_gradient")
EXPECTED = {"product": "lowd_kernel", "gradient": "lowd_grad_kernel", "logsumexp": "lowd_lse_kernel",
            "logsumexp_gradient": "lowd_lse_grad_kernel"}


def run_arm(ctx, kernel, arm):
    if arm == "product":
        ctx.run(kernel, False)
    elif arm == "gradient":
        ctx.run_grad(kernel)
    elif arm == "logsumexp":
        ctx.run_lse(kernel)
    else:
        ctx.run_lse_grad(kernel)
    assert ctx.last_kernel_name == EXPECTED[arm], (arm, ctx.last_kernel_name)
    return float(ctx.last_kernel_ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=25, help="passes per round: 25 are about 2.4 s of kernel time")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert args.reps >= 5, "the median of at least 5 kernel times"

    rs = np.random.RandomState(0)
    y = rs.rand(args.n, 3).astype(np.float32)
    x = rs.rand(args.n, 3).astype(np.float32)
    b = rs.randn(args.n, 1).astype(np.float32)  # the signal of the products, the log-weights of the log-sum-exps
    kernels = ("gaussian", "absolute-exponential")
    ctxs = {}
    try:
        for kernel in kernels:
            ctx = _lib.Context(0)
            ctx.set_option("fast_sqdists", 0)
            ctx.set_points(y, x, _lib.KMVP_F32)
            ctx.set_signal(b)
            ctxs[kernel] = ctx
        order = [(kernel, arm) for kernel in kernels for arm in ARMS]
        for _ in range(args.warmup):
            for kernel, arm in order:
                run_arm(ctxs[kernel], kernel, arm)
        rounds = []
        for r in range(args.rounds):
            times = {key: [] for key in order}
            for rep in range(args.reps):
                shift = (r * args.reps + rep) % len(order)
                for kernel, arm in order[shift:] + order[:shift]:
                    times[(kernel, arm)].append(run_arm(ctxs[kernel], kernel, arm))
            rounds.append({key: float(np.median(v)) for key, v in times.items()})
            spread = {key: (min(v), max(v)) for key, v in times.items()}
            for kernel in kernels:
                for arm in ARMS:
                    lo, hi = spread[(kernel, arm)]
                    print(f"round {r} {kernel:22s} {arm:20s} median {rounds[-1][(kernel, arm)]:8.3f} ms  "
                          f"(min {lo:.3f}, max {hi:.3f}, {args.reps} runs)")
    finally:
        for ctx in ctxs.values():
            ctx.close()

    report = {"n": args.n, "D": 3, "E": 1, "precision": "float32", "reps": args.reps, "rounds": []}
    for r, med in enumerate(rounds):
        row = {}
        for kernel in kernels:
            p, g = med[(kernel, "product")], med[(kernel, "gradient")]
            row[kernel] = {"kernel_ms": {arm: med[(kernel, arm)] for arm in ARMS},
                           "gradient/product": g / p,
                           "logsumexp/product": med[(kernel, "logsumexp")] / p,
                           "logsumexp_gradient/gradient": med[(kernel, "logsumexp_gradient")] / g,
                           "logsumexp_gradient/logsumexp": med[(kernel, "logsumexp_gradient")] / med[(kernel, "logsumexp")]}
            print(f"round {r} {kernel:22s} gradient/product {row[kernel]['gradient/product']:.3f}  logsumexp/product "
                  f"{row[kernel]['logsumexp/product']:.3f}  logsumexp_gradient/gradient "
                  f"{row[kernel]['logsumexp_gradient/gradient']:.3f}")
        report["rounds"].append(row)
    line = json.dumps(report)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
