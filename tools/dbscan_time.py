#!/usr/bin/env python3
"""Times of DBSCAN on the cell list (kmvp_dbscan: lowd_cutoff_count_kernel once, lowd_cutoff_label_kernel per round) next
to the count's walk, in one process per precision.  LAB_NOTES.md section 38 and the README row take their numbers from this.

    python tools/dbscan_time.py [--precision float32] [--reps 3] [--warmup 1] [--n 1000000] [--neighbours 32,128]
                                [--sklearn-n 100000] [--lists-n 1000000] [--json out.json]

Needs the GPU.  D = 3, n points; per cloud and mean number k of points inside R (R = (3 k / (4 pi n))^(1/3), the radius that
holds k points of a uniform cloud), min_samples = k / 2.  Clouds: "uniform" in the unit cube; "blobs": five Gaussian blobs
(sigma 0.05 .. 0.15) on 70 % of the points over uniform noise.  Arms per case, on one context and its cached plan:
  count             kmvp_radius_count at R: one walk with a counter -- what a sweep is measured against
  dbscan            kmvp_dbscan(R, k / 2): rounds, walks, wall time, kmvp_last_kernel_ms (the sum of its walks)
  dbscan all-core   kmvp_dbscan(R, 1): every finite point is a core point, there is no border walk, so
                    (kernel_ms - count's pair loop) / rounds is the time of ONE SWEEP walk with every record labelled
After `warmup` passes over all arms, `reps` passes with the arms interleaved; medians are reported.
Where they import, two host-side routes are recorded, each at the size it can handle (stated; nothing is extrapolated):
  sklearn           sklearn.cluster.DBSCAN on the first sklearn-n points of the uniform cloud at the k = 32 radius of THAT size
  lists + scipy     kmvp_radius_nearest(16) copied back and scipy.sparse.csgraph.connected_components on the core graph, at a
                    radius with a mean of 3 inside -- the route only works while no point has more than 16 inside, which is
                    checked -- with kmvp_dbscan at the same radius beside it
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from kernel_matrix_benchmarks_amd import _lib  # noqa: E402


def make(cloud, n, npdt):
    rs = np.random.RandomState(0)
    if cloud == "uniform":
        return rs.rand(n, 3).astype(npdt)
    nb = int(0.7 * n)
    centres, width, which = 0.2 + 0.6 * rs.rand(5, 3), 0.05 + 0.10 * rs.rand(5), rs.randint(0, 5, size=nb)
    x = np.concatenate([centres[which] + width[which, None] * rs.randn(nb, 3), rs.rand(n - nb, 3)])
    return np.ascontiguousarray(x[rs.permutation(n)], dtype=npdt)


def radius_for(k, n):
    return (3.0 * k / (4.0 * np.pi * n)) ** (1.0 / 3.0)


def timed(fn, ctx):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, float(ctx.last_total_ms), float(ctx.last_kernel_ms), out


def med(rows, i):
    return float(np.median([r[i] for r in rows]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", choices=("float32", "float64"), default="float32")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--neighbours", default="32,128")
    ap.add_argument("--clouds", default="uniform,blobs")
    ap.add_argument("--sklearn-n", type=int, default=100000, help="points of the sklearn arm (0: leave it out)")
    ap.add_argument("--lists-n", type=int, default=1000000, help="points of the lists + scipy arm (0: leave it out)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    n = args.n
    npdt, code = (np.float64, _lib.KMVP_F64) if args.precision == "float64" else (np.float32, _lib.KMVP_F32)
    report = {"D": 3, "precision": args.precision, "n": n, "reps": args.reps, "warmup": args.warmup, "cases": {}}
    for cloud in args.clouds.split(","):
        x = make(cloud, n, npdt)
        ctx = _lib.Context(0)
        try:
            ctx.set_points(x, None, code)
            for k in (int(v) for v in args.neighbours.split(",")):
                R, ms = radius_for(k, n), max(k // 2, 1)
                arms = {"count": lambda: ctx.radius_count(R), "dbscan": lambda: ctx.dbscan(R, ms), "dbscan all-core": lambda: ctx.dbscan(R, 1)}
                names = tuple(arms)
                for _ in range(args.warmup):
                    for name in names:
                        timed(arms[name], ctx)
                rows = {name: [] for name in names}
                for rep in range(args.reps):
                    shift = rep % len(names)
                    for name in names[shift:] + names[:shift]:
                        rows[name].append(timed(arms[name], ctx))
                counts = rows["count"][0][3]
                count_ms = med(rows["count"], 2)
                out = {"radius": R, "min_samples": ms, "mean_inside": float(counts.mean()), "max_inside": int(counts.max()),
                       "info": ctx.cutoff_info(), "arms": {}}
                for name in names:
                    a = {"wall_ms": 1e3 * med(rows[name], 0), "device_total_ms": med(rows[name], 1), "device_kernel_ms": med(rows[name], 2)}
                    tail = ""
                    if name != "count":
                        info = rows[name][0][3][3]
                        assert all(r[3][3] == info for r in rows[name]), "the rounds differ run to run"
                        a["info"] = info
                        a["ms_per_walk"] = a["device_kernel_ms"] / info["walks"]
                        tail = (f"  {info['n_clusters']} clusters, {info['n_core']} core, {info['n_border']} border, {info['n_noise']} noise, "
                                f"{info['rounds']} rounds, {info['walks']} walks, {a['ms_per_walk']:.3f} ms per walk")
                    if name == "dbscan all-core" and a["info"]["rounds"] > 0:
                        a["sweep_ms"] = (a["device_kernel_ms"] - count_ms) / a["info"]["rounds"]
                        a["sweep_over_count"] = a["sweep_ms"] / count_ms
                        tail += f"; one sweep {a['sweep_ms']:.3f} ms = x{a['sweep_over_count']:.3f} of the count's walk"
                    out["arms"][name] = a
                    print(f"{args.precision} {cloud:8s} k = {k:4d} R = {R:.5f} {name:16s} wall {a['wall_ms']:9.3f} ms  walks "
                          f"{a['device_kernel_ms']:9.3f} ms{tail}", flush=True)
                print(f"{args.precision} {cloud:8s} k = {k:4d} mean inside {out['mean_inside']:.1f}, max {out['max_inside']}, "
                      f"cells {out['info']['cells']}, walked {out['info']['walked']:.3e} records", flush=True)
                report["cases"][f"{cloud} k={k}"] = out
        finally:
            ctx.close()

    # ---- the host-side routes, each at the size it can handle ----
    try:
        from sklearn.cluster import DBSCAN
    except ImportError:
        DBSCAN = None
    if DBSCAN is not None and args.sklearn_n > 0:
        m = min(args.sklearn_n, n)
        xs = np.random.RandomState(0).rand(m, 3).astype(npdt)
        R = radius_for(32, m)
        t0 = time.perf_counter()
        sk = DBSCAN(eps=R, min_samples=16).fit(xs)
        t_sk = time.perf_counter() - t0
        ctx = _lib.Context(0)
        try:
            ctx.set_points(xs, None, code)
            ctx.dbscan(R, 16)
            t_us, _, _, got = timed(lambda: ctx.dbscan(R, 16), ctx)
        finally:
            ctx.close()
        core = got[1] == np.arange(m)
        agree = bool(np.array_equal(sk.core_sample_indices_, np.flatnonzero(core)) and np.array_equal(sk.labels_[core], got[0][core])
                     and np.array_equal(sk.labels_ == -1, got[0] == -1))
        report["sklearn"] = {"n": m, "radius": R, "min_samples": 16, "sklearn_s": t_sk, "kmvp_dbscan_wall_ms": 1e3 * t_us,
                             "cores_core_labels_noise_agree": agree, "labels_differing": int((sk.labels_ != got[0]).sum())}
        print(f"sklearn DBSCAN at n = {m} (k = 32, min_samples 16): {t_sk:.2f} s; kmvp_dbscan on the same points {1e3 * t_us:.2f} ms "
              f"wall; core points, core labels and noise agree: {agree}; {report['sklearn']['labels_differing']} border labels differ",
              flush=True)
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        coo_matrix = None
    if coo_matrix is not None and args.lists_n > 0:
        m = min(args.lists_n, n)
        xs = np.random.RandomState(0).rand(m, 3).astype(npdt)
        R, ms = radius_for(3, m), 3
        ctx = _lib.Context(0)
        try:
            ctx.set_points(xs, None, code)
            top = int(ctx.radius_count(R).max())
            if top > 16:
                print(f"lists + scipy at n = {m}: a point has {top} > 16 inside, the route does not apply", flush=True)
                report["lists"] = {"n": m, "radius": R, "max_inside": top, "applies": False}
            else:
                def host_route():
                    counts = ctx.radius_count(R)
                    idx, _ = ctx.radius_nearest(R, 16)
                    core = counts >= ms
                    rows = np.repeat(np.arange(m), 16)
                    keep = (idx.ravel() >= 0) & core[rows] & core[np.maximum(idx.ravel(), 0)]
                    g = coo_matrix((np.ones(int(keep.sum()), dtype=np.int8), (rows[keep], idx.ravel()[keep])), shape=(m, m))
                    return connected_components(g, directed=False)[1], core

                host_route()
                t0 = time.perf_counter()
                comp, core = host_route()
                t_host = time.perf_counter() - t0
                ctx.dbscan(R, ms)
                t_us, _, _, got = timed(lambda: ctx.dbscan(R, ms), ctx)
                same = len(set(zip(comp[core].tolist(), got[0][core].tolist()))) == len(set(got[0][core].tolist()))
                report["lists"] = {"n": m, "radius": R, "min_samples": ms, "max_inside": top, "applies": True, "host_route_ms": 1e3 * t_host,
                                   "kmvp_dbscan_wall_ms": 1e3 * t_us, "info": got[3], "same_core_partition": bool(same)}
                print(f"lists + scipy at n = {m} (mean 3 inside, max {top}, min_samples {ms}; core components only, no border rule): "
                      f"{1e3 * t_host:.1f} ms; kmvp_dbscan at the same radius {1e3 * t_us:.2f} ms wall ({got[3]['rounds']} rounds); the same "
                      f"partition of the core points: {same}", flush=True)
        finally:
            ctx.close()
    line = json.dumps(report)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
