#!/usr/bin/env python3
"""Times of the batched Sinkhorn solve (kmvp_<kernel>_sinkhorn_batched: lowd_batch_lse_kernel) next to what a user does
without it, in one process.  The LAB_NOTES.md section on the batched Sinkhorn and the README row take their numbers from this.

    python tools/sinkhorn_batched_time.py [--reps 3] [--warmup 1] [--shapes 256x2048,16x32768] [--iters 100] [--json out.json]

Needs the GPU.  B pairs of clouds of n points each (targets != sources), D = 3, float32, uniform points in the unit cube
(the sources shifted by 0.25 along x), Gaussian cost at eps = 0.01 -- far from converged after `iters` iterations, so
tol = 0 and maxit = iters run exactly that many in every arm (asserted).  Arms per shape:
  (a) batched   one context on the concatenation with the batches set: ONE call of kmvp_gaussian_sinkhorn_batched.  Timed: the
                call alone ("solve": the layouts are packed), and kmvp_set_points + kmvp_set_batches + the call ("prepare +
                solve": both directions are planned and packed inside).
  (b) loop      the host loop over the clouds on ONE context: kmvp_set_points + kmvp_gaussian_sinkhorn per cloud -- what
                users do today.  Timed: the whole loop.
  (c) retire    the first shape only: the clouds of batch b scaled by a factor that grows with b (1 .. 8 times, so the
                batches converge at very different k), tol = 1e-4, maxit = 1000, with "sinkhorn_retire" 1 and 0.  The results
                are asserted bitwise equal; the times say what retirement saves.
After `warmup` passes over all arms, `reps` passes with the arms interleaved.  Reported per arm: the median wall time (a host
clock around synchronous calls), the median of the summed kmvp_last_total_ms (device events), and pairs / wall time with
pairs = 2 B n^2 per iteration.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from kernel_matrix_benchmarks_amd import _lib  # noqa: E402

EPS = 0.01
KERNEL = "gaussian"


def clouds(B, n, spread=None):
    rs = np.random.RandomState(B)
    x = rs.rand(B * n, 3)
    y = rs.rand(B * n, 3) + np.array([0.25, 0.0, 0.0])
    scale = np.full(B * n, 1.0 / np.sqrt(EPS)) if spread is None else np.repeat(spread, n)
    return (x * scale[:, None]).astype(np.float32), (y * scale[:, None]).astype(np.float32)


class Batched:
    def __init__(self, x, y, off, tol, maxit, retire=-1):
        self.x, self.y, self.off, self.tol, self.maxit = x, y, off, tol, maxit
        self.ctx = _lib.Context(0)
        self.ctx.set_option("sinkhorn_retire", retire)
        self.prepare()
        self.last = None

    def prepare(self):
        self.ctx.set_points(self.y, self.x, _lib.KMVP_F32)
        self.ctx.set_batches(self.off, self.off)

    def run(self, prepare):
        t0 = time.perf_counter()
        if prepare:
            self.prepare()
        self.last = self.ctx.sinkhorn_batched(KERNEL, None, None, self.tol, self.maxit)
        wall = time.perf_counter() - t0
        assert self.ctx.last_kernel_name == "lowd_batch_lse_kernel"
        return wall, float(self.ctx.last_total_ms), int(self.last[2].sum())


class Loop:
    def __init__(self, x, y, off, tol, maxit):
        self.x, self.y, self.off, self.tol, self.maxit = x, y, off, tol, maxit
        self.ctx = _lib.Context(0)

    def run(self):
        total, iters = 0.0, 0
        t0 = time.perf_counter()
        for b in range(len(self.off) - 1):
            s = slice(self.off[b], self.off[b + 1])
            self.ctx.set_points(self.y[s], self.x[s], _lib.KMVP_F32)
            got = self.ctx.sinkhorn(KERNEL, None, None, self.tol, self.maxit)
            total += float(self.ctx.last_total_ms)
            iters += got[2]
        wall = time.perf_counter() - t0
        assert self.ctx.last_kernel_name == "lowd_lse_kernel"
        return wall, total, iters


def timed(arms, warmup, reps):
    names = tuple(arms)
    for _ in range(warmup):
        for name in names:
            arms[name]()
    times = {name: [] for name in names}
    for rep in range(reps):
        shift = rep % len(names)
        for name in names[shift:] + names[:shift]:
            times[name].append(arms[name]())
    return times


def summarise(label, times, n):
    out = {}
    for name, runs in times.items():
        wall, total = (float(np.median([t[i] for t in runs])) for i in range(2))
        iters = runs[0][2]
        assert all(t[2] == iters for t in runs), (name, [t[2] for t in runs])
        pairs = 2.0 * iters * n * n   # iters is summed over the batches: 2 n^2 pairs per batch and iteration
        out[name] = {"wall_ms": 1e3 * wall, "device_total_ms": total, "wall_ms_all": [1e3 * t[0] for t in runs],
                     "iterations_summed": iters, "pairs": pairs, "pairs_per_s_wall": pairs / wall}
        print(f"{label} {name:28s} wall {1e3 * wall:10.2f} ms  device total {total:10.2f} ms  iterations (summed) {iters:7d}  "
              f"{pairs / wall / 1e9:8.1f} Gpairs/s")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shapes", default="256x2048,16x32768", help="comma-separated BxN: B pairs of clouds of N points")
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--no-retire-case", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    report = {"D": 3, "precision": "float32", "kernel": KERNEL, "eps": EPS, "iters": args.iters, "reps": args.reps,
              "warmup": args.warmup, "shapes": {}}
    for q, shape in enumerate(args.shapes.split(",")):
        B, n = (int(v) for v in shape.lower().split("x"))
        off = np.arange(B + 1, dtype=np.int64) * n
        x, y = clouds(B, n)
        batched, loop = Batched(x, y, off, 0.0, args.iters), Loop(x, y, off, 0.0, args.iters)
        row = {}
        try:
            times = timed({"batched, solve": lambda: batched.run(False), "batched, prepare + solve": lambda: batched.run(True),
                           "loop, set_points + solve": loop.run}, args.warmup, args.reps)
            for name, runs in times.items():
                assert all(t[2] == B * args.iters for t in runs), (name, "an arm stopped early", [t[2] for t in runs])
            row["fixed iterations"] = summarise(f"{B} x {n}", times, n)
            row["speedup_wall_solve"] = row["fixed iterations"]["loop, set_points + solve"]["wall_ms"] / \
                row["fixed iterations"]["batched, solve"]["wall_ms"]
            row["speedup_wall_prepare_solve"] = row["fixed iterations"]["loop, set_points + solve"]["wall_ms"] / \
                row["fixed iterations"]["batched, prepare + solve"]["wall_ms"]
            print(f"{B} x {n}: loop / batched = x{row['speedup_wall_solve']:.2f} (solve), "
                  f"x{row['speedup_wall_prepare_solve']:.2f} (prepare + solve)")
        finally:
            batched.ctx.close()
            loop.ctx.close()
        if q == 0 and not args.no_retire_case:
            spread = np.geomspace(1.0, 8.0, B)
            xs, ys = clouds(B, n, spread)
            on, offarm = Batched(xs, ys, off, 1e-4, 1000, retire=1), Batched(xs, ys, off, 1e-4, 1000, retire=0)
            try:
                times = timed({"retire 1": lambda: on.run(False), "retire 0": lambda: offarm.run(False)}, args.warmup, args.reps)
                for p, r in zip(on.last, offarm.last):
                    assert np.array_equal(p, r), "sinkhorn_retire 0 and 1 disagree"
                its = on.last[2]
                row["retire"] = summarise(f"{B} x {n} spread 1..8", times, n)
                row["retire"]["iterations"] = {"min": int(its.min()), "median": float(np.median(its)), "max": int(its.max()),
                                               "status": sorted(set(int(s) for s in on.last[4]))}
                row["retire"]["saving_wall"] = row["retire"]["retire 0"]["wall_ms"] / row["retire"]["retire 1"]["wall_ms"]
                print(f"{B} x {n} spread 1..8: iterations {its.min()} .. {its.max()} (median {np.median(its):.0f}), "
                      f"retire 0 / retire 1 = x{row['retire']['saving_wall']:.2f}")
            finally:
                on.ctx.close()
                offarm.ctx.close()
        report["shapes"][shape] = row
    line = json.dumps(report)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
