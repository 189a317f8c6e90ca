#!/usr/bin/env python3
"""Times of the batched clouds (kmvp_set_batches: lowd_batch_kernel, lowd_batch_knn_kernel) next to what a user does
without them, in one process.  LAB_NOTES.md section 28 and the README row take their numbers from this.

    python tools/batched_time.py [--reps 3] [--warmup 1] [--shapes 256x2048,16x32768] [--json out.json]

Needs the GPU.  B clouds of n points each, targets == sources, D = 3, float32, uniform points in the unit cube; the
Gaussian density product and the K = 1 nearest neighbour.  Three arms per shape and reduction:
  (a) batched   one context on the concatenation with the batches set: ONE call.  Timed: the call alone ("query"), and
                kmvp_set_points + kmvp_set_batches + kmvp_set_signal + the call ("prepare + query").
  (b) loop      the host loop over the clouds on one MI355XProduct with its default policy (whichever kernel it picks per
                cloud: reported), prepare_data + [prepare_query +] query per cloud: what users do today.  Timed: the whole loop.
  (c) plain     the plain call on the concatenation in the difference form (fast_sqdists = 0: lowd_kernel / lowd_knn_kernel,
                the batched kernels' own pair arithmetic) -- B times the pairs and another result: for the pair rate only.
After `warmup` passes over all arms, `reps` passes with the arms interleaved.  Reported per arm: the median wall time (a host
clock around synchronous calls) and the median of the summed kmvp_last_total_ms (device events), and the pair rates
pairs / device time of (a) and (c).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from kernel_matrix_benchmarks_amd import _lib  # noqa: E402
from kernel_matrix_benchmarks_amd.algorithms.mi355x import MI355XProduct  # noqa: E402

REDUCTIONS = ("density", "nearest")


def call(ctx, reduction, name):
    if reduction == "density":
        ctx.run("gaussian", False)
    else:
        ctx.run_nearest(1)
    assert ctx.last_kernel_name == name, (ctx.last_kernel_name, name)
    return float(ctx.last_total_ms), float(ctx.last_kernel_ms)


class Batched:
    def __init__(self, y, off):
        self.y, self.off, self.ctx = y, off, _lib.Context(0)
        self.prepare()

    def prepare(self):
        self.ctx.set_points(self.y, None, _lib.KMVP_F32)
        self.ctx.set_batches(self.off)
        self.ctx.set_signal(None)

    def run(self, reduction, prepare):
        t0 = time.perf_counter()
        if prepare:
            self.prepare()
        total, kernel = call(self.ctx, reduction, "lowd_batch_kernel" if reduction == "density" else "lowd_batch_knn_kernel")
        return time.perf_counter() - t0, total, kernel


class Loop:
    def __init__(self, y, off):
        self.y, self.off = y, off
        self.algo = MI355XProduct(kernel="gaussian", dimension=y.shape[1], precision=np.float32)
        self.kernels = set()

    def run(self, reduction):
        algo, total, kernel = self.algo, 0.0, 0.0
        t0 = time.perf_counter()
        for b in range(len(self.off) - 1):
            cloud = self.y[self.off[b]:self.off[b + 1]]
            algo.prepare_data(source_points=cloud, target_points=cloud, same_points=True, density_estimation=True)
            if reduction == "density":
                algo.prepare_query(source_signal=None)
                algo.query()
            else:
                algo.query_nearest(1)
            total += algo.device_total_ms
            kernel += algo.device_kernel_ms
            self.kernels.add(algo.device_kernel)
        return time.perf_counter() - t0, total, kernel


class Plain:
    def __init__(self, y):
        self.ctx = _lib.Context(0)
        self.ctx.set_option("fast_sqdists", 0)
        self.ctx.set_points(y, None, _lib.KMVP_F32)
        self.ctx.set_signal(None)

    def run(self, reduction):
        t0 = time.perf_counter()
        total, kernel = call(self.ctx, reduction, "lowd_kernel" if reduction == "density" else "lowd_knn_kernel")
        return time.perf_counter() - t0, total, kernel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shapes", default="256x2048,16x32768", help="comma-separated BxN: B clouds of N points")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    report = {"D": 3, "precision": "float32", "reps": args.reps, "warmup": args.warmup, "shapes": {}}
    for shape in args.shapes.split(","):
        B, n = (int(v) for v in shape.lower().split("x"))
        rs = np.random.RandomState(B)
        y = rs.rand(B * n, 3).astype(np.float32)
        off = np.arange(B + 1, dtype=np.int64) * n
        batched, loop, plain = Batched(y, off), Loop(y, off), Plain(y)
        arms = {"batched, query": lambda r: batched.run(r, False), "batched, prepare + query": lambda r: batched.run(r, True),
                "loop, prepare_data + query per cloud": loop.run, "plain call on the concatenation": plain.run}
        names = tuple(arms)
        row = {}
        try:
            for reduction in REDUCTIONS:
                for _ in range(args.warmup):
                    for name in names:
                        arms[name](reduction)
                times = {name: [] for name in names}
                for rep in range(args.reps):
                    shift = rep % len(names)
                    for name in names[shift:] + names[:shift]:
                        times[name].append(arms[name](reduction))
                out = {}
                for name in names:
                    wall, total, kernel = (float(np.median([t[i] for t in times[name]])) for i in range(3))
                    pairs = float(B) * n * n * (B if name.startswith("plain") else 1)
                    out[name] = {"wall_ms": 1e3 * wall, "device_total_ms": total, "device_kernel_ms": kernel,
                                 "wall_ms_all": [1e3 * t[0] for t in times[name]], "pairs": pairs,
                                 "pairs_per_s_device": pairs / (1e-3 * total) if total > 0 else None}
                    print(f"{B} x {n} {reduction:8s} {name:38s} wall {1e3 * wall:10.3f} ms  device total {total:10.3f} ms  "
                          f"pair loop {kernel:10.3f} ms  {pairs / (1e-3 * total) / 1e9 if total > 0 else float('nan'):8.1f} Gpairs/s")
                row[reduction] = out
            row["loop_kernels"] = sorted(loop.kernels)
        finally:
            batched.ctx.close()
            plain.ctx.close()
            loop.algo.done()
        report["shapes"][shape] = row
    line = json.dumps(report)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
