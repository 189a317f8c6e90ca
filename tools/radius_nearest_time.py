#!/usr/bin/env python3
"""Times of the radius search (kmvp_radius_nearest: lowd_cutoff_knn_kernel on the cell list) next to its floor and to the
brute force of the same library, in one process per precision.  LAB_NOTES.md section 36 and the README row take their
numbers from this.

    python tools/radius_nearest_time.py [--precision float32] [--reps 3] [--warmup 1] [--n 1000000] [--neighbours 32,128]
                                        [--ks 1,4,8,16] [--brute-n 100000] [--json out.json]

Needs the GPU.  D = 3, N = M = n points uniform in the unit cube, targets == sources; the radius with a mean of k inside
sources per target, R = (3 k / (4 pi n))^(1/3).  Arms per radius:
  (a) count                 kmvp_radius_count at the same R on the same cached plan: the same walk with a counter in place
                            of the list -- the floor
  radius K = ...            kmvp_radius_nearest on the cached plan, one arm per K
  (b) brute K = ...         kmvp_nearest at the same K on the first brute-n points.  Scaled by the pair count,
                            (n / brute-n)^2, it is labelled an EXTRAPOLATION to n points: it is not a measurement
After `warmup` passes over all arms, `reps` passes with the arms interleaved.  Reported per arm: the median wall time (a host
clock around the synchronous call) and the median kmvp_last_kernel_ms (device events around the pair loop); walked records
per inside pair from the info words; and every radius arm's pair-loop ratio to (a).
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
    ap.add_argument("--precision", choices=("float32", "float64"), default="float32")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--neighbours", default="32,128", help="comma-separated mean numbers of inside sources per target")
    ap.add_argument("--ks", default="1,4,8,16", help="comma-separated K")
    ap.add_argument("--brute-n", type=int, default=100000, help="points of the brute-force arm (0: leave it out)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    n, ks = args.n, [int(v) for v in args.ks.split(",")]
    npdt, code = (np.float64, _lib.KMVP_F64) if args.precision == "float64" else (np.float32, _lib.KMVP_F32)
    y = np.random.RandomState(0).rand(n, 3).astype(npdt)
    nb = min(args.brute_n, n)
    scale = (n / nb) ** 2 if nb else None
    cut, brute = _lib.Context(0), _lib.Context(0)
    report = {"D": 3, "precision": args.precision, "n": n, "brute_n": nb, "reps": args.reps, "warmup": args.warmup, "radii": {}}
    try:
        cut.set_points(y, None, code)
        if nb:
            brute.set_points(np.ascontiguousarray(y[:nb]), None, code)
        for k in (float(v) for v in args.neighbours.split(",")):
            R = (3.0 * k / (4.0 * np.pi * n)) ** (1.0 / 3.0)
            arms = {"count": (lambda: cut.radius_count(R), cut)}
            for K in ks:
                arms[f"radius K = {K}"] = (lambda K=K: cut.radius_nearest(R, K), cut)
            for K in ks if nb else ():
                arms[f"brute K = {K}"] = (lambda K=K: brute.run_nearest(K), brute)
            names = tuple(arms)
            for _ in range(args.warmup):
                for name in names:
                    timed(*arms[name])
            times = {name: [] for name in names}
            for rep in range(args.reps):
                shift = rep % len(names)
                for name in names[shift:] + names[:shift]:
                    times[name].append(timed(*arms[name]))
            inside = int(cut.radius_count(R).sum())
            info = cut.cutoff_info()
            out = {"radius": R, "info": info, "inside_pairs": inside, "walked_per_inside": info["walked"] / max(inside, 1), "arms": {}}
            for name in names:
                wall, total, kernel = (float(np.median([t[i] for t in times[name]])) for i in range(3))
                out["arms"][name] = {"wall_ms": 1e3 * wall, "device_total_ms": total, "device_kernel_ms": kernel,
                                     "wall_ms_all": [1e3 * t[0] for t in times[name]]}
            floor = out["arms"]["count"]["device_kernel_ms"]
            for name in names:
                a = out["arms"][name]
                tail = ""
                if name.startswith("radius"):
                    a["pair_loop_over_count"] = a["device_kernel_ms"] / floor if floor > 0 else None
                    tail = f"  pair loop / count {a['pair_loop_over_count']:.2f}"
                elif name.startswith("brute"):
                    a["extrapolated_to_n_ms"] = a["device_kernel_ms"] * scale
                    tail = f"  x {scale:.0f} by the pair count = {a['extrapolated_to_n_ms']:.0f} ms at n (an extrapolation)"
                print(f"{args.precision} k = {k:5.0f} R = {R:.5f} {name:16s} wall {a['wall_ms']:10.3f} ms  pair loop "
                      f"{a['device_kernel_ms']:10.3f} ms{tail}")
            print(f"{args.precision} k = {k:5.0f} cells {info['cells']} tiles {info['tiles']} runs {info['runs']} walked {info['walked']:.3e} "
                  f"records, {out['walked_per_inside']:.2f} per inside pair ({inside / n:.1f} inside per target), host plan "
                  f"{info['plan_ms']} ms")
            report["radii"][str(k)] = out
    finally:
        cut.close()
        brute.close()
    line = json.dumps(report)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
