#!/usr/bin/env python3
"""What a stale plan costs the cutoff-radius entries with the plan built on the host ("cutoff_plan" = 0, the default) and on the
device ("cutoff_plan" = 1; csrc/kmvp_cutoff_plan_device.hip), in one process.  LAB_NOTES.md section 37 and the README row take
their numbers from this.

    python tools/cutoff_plan_time.py [--reps 3] [--warmup 1] [--n 1000000] [--neighbours 32,128] [--json out.json]
    python tools/cutoff_plan_time.py --one-build [--n 1000000] [--neighbours 32]

Needs the GPU.  Gaussian, D = 3, float32, N = M = n points uniform in the unit cube, targets == sources, one signal column;
the radius with a mean of k inside sources per target, R = (3 k / (4 pi n))^(1/3).  Arms per radius, as tools/cutoff_time.py
forms them:
  (1) cutoff, cached plan         kmvp_gaussian_cutoff on the cached plan: the call alone
  (2) stale plan, host build      the same call after the plan was invalidated (the cell factor moved by one part in 1e9):
                                  copies back + host plan build + uploads + the packs + the call
  (3) stale plan, device build    the same with the plan built on the device: two small read-backs instead
Arms 2 and 3 run on contexts of their own, one per option value, with the same points.  After `warmup` passes over all arms,
`reps` passes with the arms interleaved; reported per arm: the median wall time (a host clock around synchronous calls), the
median kmvp_last_total_ms (device events) and the info word plan_ms.  The verdict line says whether arm 3 took less time than
arm 2 at every radius.

--one-build runs one warm-up call and then ONE stale-plan call with the device build and nothing else: the process to put
under `rocprofv3 --kernel-trace --stats -- python tools/cutoff_plan_time.py --one-build` for the per-kernel split (a run of
its own: no counters with it).
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
    return time.perf_counter() - t0, float(ctx.last_total_ms), float(ctx.cutoff_info()["plan_ms"])


def radius(k, n):
    return (3.0 * k / (4.0 * np.pi * n)) ** (1.0 / 3.0)


def stale_call(ctx, R):
    nudge = [0]

    def call():
        nudge[0] ^= 1
        ctx.set_option("cutoff_cell_factor", 1.0 + 1e-9 * nudge[0])
        ctx.run_cutoff("gaussian", R, False)

    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--neighbours", default="32,128", help="comma-separated mean numbers of inside sources per target")
    ap.add_argument("--one-build", action="store_true", help="one warm-up and one stale-plan call with the device build, for a kernel trace")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    n = args.n
    rs = np.random.RandomState(0)
    y = rs.rand(n, 3).astype(np.float32)
    b = rs.randn(n, 1).astype(np.float32)
    ks = [float(v) for v in args.neighbours.split(",")]
    if args.one_build:
        ctx = _lib.Context(0)
        try:
            ctx.set_option("cutoff_plan", 1)
            ctx.set_points(y, None, _lib.KMVP_F32)
            ctx.set_signal(b)
            call = stale_call(ctx, radius(ks[0], n))
            call()
            wall, total, plan_ms = timed(call, ctx)
            print(f"one device build: wall {1e3 * wall:.3f} ms, device total {total:.3f} ms, plan_ms {plan_ms:.0f}, "
                  f"built on {ctx.cutoff_info()['built_on']}")
        finally:
            ctx.close()
        return

    cached, host, device = _lib.Context(0), _lib.Context(0), _lib.Context(0)
    report = {"D": 3, "precision": "float32", "kernel": "gaussian", "n": n, "reps": args.reps, "warmup": args.warmup, "radii": {}}
    verdict = True
    try:
        device.set_option("cutoff_plan", 1)
        for ctx in (cached, host, device):
            ctx.set_points(y, None, _lib.KMVP_F32)
            ctx.set_signal(b)
        for k in ks:
            R = radius(k, n)
            arms = {"cutoff, cached plan": (lambda: cached.run_cutoff("gaussian", R, False), cached),
                    "stale plan, host build": (stale_call(host, R), host),
                    "stale plan, device build": (stale_call(device, R), device)}
            names = tuple(arms)
            for _ in range(args.warmup):
                for name in names:
                    timed(*arms[name])
            times = {name: [] for name in names}
            for rep in range(args.reps):
                shift = rep % len(names)
                for name in names[shift:] + names[:shift]:
                    times[name].append(timed(*arms[name]))
            sides = (host.cutoff_info()["built_on"], device.cutoff_info()["built_on"])
            same = bool(np.array_equal(host.get_result(n, 1), device.get_result(n, 1)))
            out = {"radius": R, "info": device.cutoff_info(), "built_on": sides, "same_bits": same, "arms": {}}
            for name in names:
                wall, total, plan_ms = (float(np.median([t[i] for t in times[name]])) for i in range(3))
                out["arms"][name] = {"wall_ms": 1e3 * wall, "device_total_ms": total, "plan_ms": plan_ms,
                                     "wall_ms_all": [1e3 * t[0] for t in times[name]]}
                print(f"k = {k:5.0f} R = {R:.5f} {name:26s} wall {1e3 * wall:10.3f} ms  device total {total:10.3f} ms  plan_ms {plan_ms:4.0f}")
            less = out["arms"]["stale plan, device build"]["wall_ms"] < out["arms"]["stale plan, host build"]["wall_ms"]
            out["device_build_takes_less"] = less
            verdict = verdict and less and same and sides == ("host", "device")
            print(f"k = {k:5.0f} built on {sides}, same bits: {same}, stale-plan call with the device build takes less time: {less}")
            report["radii"][str(k)] = out
    finally:
        for ctx in (cached, host, device):
            ctx.close()
    report["acceptance"] = verdict
    print(f"acceptance (at every radius the stale-plan call takes less time with the device build, same bits): {verdict}")
    line = json.dumps(report)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
