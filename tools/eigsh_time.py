#!/usr/bin/env python3
"""Time of the device-resident eigen-solver (kmvp_<kernel>_eigsh) on one shape, in one process, against the loops it
replaces.  LAB_NOTES.md section 30 and the README row take their numbers from this.

    python tools/eigsh_time.py [--n 100000] [--k 16] [--tol 1e-8] [--reps 3] [--kernels gaussian,matern-5/2] [--json out.json]
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/eigsh_time.py --device-only --reps 1
    python tools/eigsh_time.py --stats OUT/.../*_kernel_stats.csv --steps STEPS [--n 100000]

Needs the GPU (the --stats form only reads a file).  Config 5's cloud (uniform_cube(n, 3), seed n + 3), float64, the plain
kernel operator, v0 a normal draw from seed 0.  Arms, each `reps` times after one warm-up, median reported:
  device       Context.eigsh: steps, wall ms, kmvp_last_total_ms, ms per step
  product      one bare single-column product of the same context (kmvp_last_total_ms): what a step cannot go below
  host         the same algorithm (CGS2, the look schedule, X = V S and the k-column application for the true residuals)
               with its basis in numpy and MI355XProduct.query as the operator: one upload, one prepare_query and one
               download per step
  scipy        scipy.sparse.linalg.eigsh (implicitly restarted Lanczos) on the same operator, where scipy imports
The --stats form reads rocprofv3's kernel statistics of a --device-only run and reports the share of the four
reorthogonalisation passes (eig_proj_kernel, eig_sub_kernel) and their bytes per second, the bytes counted from the shapes:
pass p of step j reads j vectors of N doubles and w once (the subtraction also writes it).  Stated, not asserted.
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

LOOK, BREAKDOWN = 8, 1e-13


def reorth_bytes(n, steps):
    """Bytes the four passes of every step read and write: V_j once per pass, w read by all four and written by two."""
    return sum(4 * j * n * 8 + 6 * n * 8 for j in range(1, steps + 1))


def host_lanczos(apply, n, k, v0, tol, maxit):
    """include/kmvp.h's process with the basis on the host; returns (theta, steps, operator applications)."""
    V = np.zeros((maxit + 1, n))
    V[0] = v0 / np.linalg.norm(v0)
    alpha, beta = np.zeros(maxit), np.zeros(maxit)
    j, theta = 0, None
    while j < maxit:
        Vj = V[: j + 1]
        w = apply(V[j])
        h = Vj @ w
        w = w - Vj.T @ h
        h2 = Vj @ w
        w = w - Vj.T @ h2
        alpha[j], beta[j] = h[j] + h2[j], np.linalg.norm(w)
        j += 1
        breakdown = beta[j - 1] <= BREAKDOWN * np.max(np.abs(alpha[:j]))
        if not breakdown:
            V[j] = w / beta[j - 1]
        if not (breakdown or (j >= k and j % LOOK == 0) or j == maxit) or j < k:
            continue
        T = np.diag(alpha[:j]) + np.diag(beta[: j - 1], 1) + np.diag(beta[: j - 1], -1)
        lam, Z = np.linalg.eigh(T)
        theta, S = lam[::-1][:k], Z[:, ::-1][:, :k]
        if breakdown or np.all(beta[j - 1] * np.abs(S[-1]) <= tol * abs(theta[0])):
            break
    X = V[:j].T @ S  # and the true residuals from one more k-column application, as the library ends
    X /= np.linalg.norm(X, axis=0)
    resid = np.linalg.norm(apply(X) - X * theta, axis=0) / abs(theta[0])
    return theta, j, float(np.max(resid))


def median_of(fn, reps):
    fn()  # warm-up
    wall, extra = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        extra = fn()
        wall.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(wall)), [float(w) for w in wall], extra


def read_stats(path, n, steps):
    rows = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            total = float(row.get("TotalDurationNs") or row.get("TotalDuration(ns)") or 0.0)
            rows[name] = rows.get(name, 0.0) + total
    whole = sum(rows.values())
    reorth = sum(t for name, t in rows.items() if "eig_proj_kernel" in name or "eig_sub_kernel" in name)
    top = sorted(rows.items(), key=lambda kv: -kv[1])[:8]
    report = {"stats": path, "kernel_ns_total": whole, "reorth_ns": reorth, "reorth_share": reorth / whole if whole else None,
              "top_kernels": [[name[:80], t, t / whole] for name, t in top]}
    if steps:
        # the trace holds every call of the run (warm-up included): bytes of ONE call times the calls traced
        report["reorth_bytes_per_call"] = reorth_bytes(n, steps)
    return report


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=100000)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--maxit", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernels", default="gaussian,matern-5/2")
    ap.add_argument("--device-only", action="store_true", help="the device arm alone (for a profiler run)")
    ap.add_argument("--stats", default=None, help="a rocprofv3 kernel_stats.csv to summarise instead of running")
    ap.add_argument("--steps", type=int, default=0, help="with --stats: the steps of one call, for the byte count")
    ap.add_argument("--calls", type=int, default=2, help="with --stats: eigsh calls the trace holds (warm-up + reps)")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()

    if args.stats:
        report = read_stats(args.stats, args.n, args.steps)
        if args.steps and report["reorth_ns"]:
            report["reorth_bytes_per_second"] = report["reorth_bytes_per_call"] * args.calls / (report["reorth_ns"] * 1e-9)
        print(json.dumps(report))
        if args.json:
            with open(args.json, "w") as f:
                json.dump(report, f, indent=1)
        return

    from kernel_matrix_benchmarks_amd import _lib
    from kernel_matrix_benchmarks_amd.algorithms.mi355x import MI355XProduct

    n, k = args.n, args.k
    y = np.random.RandomState(n + 3).rand(n, 3)
    v0 = np.random.RandomState(0).standard_normal(n)
    maxit = min(args.maxit, n)
    report = {"n": n, "k": k, "tol": args.tol, "maxit": maxit, "reps": args.reps, "kernels": {}}
    for kernel in args.kernels.split(","):
        row = {}
        ctx = _lib.Context(0)
        try:
            ctx.set_points(y, None, _lib.KMVP_F64)
            ctx.fit(kernel)
            dev_ms = []

            def device():
                out = ctx.eigsh(kernel, k, "kernel", v0, args.tol, maxit)
                dev_ms.append(ctx.last_total_ms)
                return out

            wall, walls, out = median_of(device, args.reps)
            steps = int(out["steps"])
            row["device"] = {"steps": steps, "converged": bool(out["converged"]), "wall_ms": wall, "wall_ms_all": walls,
                             "device_ms": float(np.median(dev_ms[1:])), "ms_per_step": float(np.median(dev_ms[1:])) / steps,
                             "worst_resid": float(np.max(out["resid"])), "theta_1": float(out["eigenvalues"][0]),
                             "theta_k": float(out["eigenvalues"][-1]), "reorth_bytes": reorth_bytes(n, steps),
                             "basis_bytes": (steps + 1) * n * 8}
            print(kernel, "device", json.dumps(row["device"]), flush=True)
            if not args.device_only:
                b = np.ascontiguousarray(v0.reshape(-1, 1))
                prod_ms = []

                def product():
                    ctx.set_signal(b)
                    ctx.run(kernel, False)
                    prod_ms.append(ctx.last_total_ms)

                median_of(product, max(args.reps, 5))
                row["product"] = {"total_ms": float(np.median(prod_ms[1:])), "device_kernel": ctx.last_kernel_name}
                row["device"]["ms_per_step_over_product"] = row["device"]["ms_per_step"] / row["product"]["total_ms"]
                print(kernel, "product", json.dumps(row["product"]), flush=True)
        finally:
            ctx.close()
        if not args.device_only:
            algo = MI355XProduct(kernel=kernel, dimension=3, precision=np.float64)
            try:
                algo.prepare_data(source_points=y, target_points=y, same_points=True)
                algo.fit()

                def apply(v):  # one vector (N,) or a block (N, E)
                    algo.prepare_query(source_signal=np.ascontiguousarray(v.reshape(n, -1)))
                    algo.query()
                    return np.asarray(algo.get_result(), dtype=np.float64).reshape(v.shape)

                wall, walls, (theta, hsteps, hresid) = median_of(lambda: host_lanczos(apply, n, k, v0, args.tol, maxit), args.reps)
                row["host"] = {"steps": hsteps, "wall_ms": wall, "wall_ms_all": walls, "ms_per_step": wall / hsteps,
                               "theta_1": float(theta[0]), "worst_resid": hresid,
                               "wall_over_device": wall / row["device"]["wall_ms"]}
                print(kernel, "host", json.dumps(row["host"]), flush=True)
                try:
                    from scipy.sparse.linalg import LinearOperator, eigsh
                except ImportError:
                    row["scipy"] = "scipy does not import here"
                else:
                    count = [0]

                    def counted(v):
                        count[0] += 1
                        return apply(np.asarray(v, dtype=np.float64).reshape(-1))

                    def scipy_arm():
                        count[0] = 0
                        lam = eigsh(LinearOperator((n, n), matvec=counted, dtype=np.float64), k=k, which="LA", tol=args.tol, v0=v0,
                                    return_eigenvectors=True)[0]
                        return lam, count[0]

                    wall, walls, (lam, applications) = median_of(scipy_arm, args.reps)
                    row["scipy"] = {"applications": applications, "wall_ms": wall, "wall_ms_all": walls,
                                    "theta_1": float(np.max(lam)), "wall_over_device": wall / row["device"]["wall_ms"]}
                print(kernel, "scipy", json.dumps(row["scipy"]), flush=True)
            finally:
                algo.done()
        report["kernels"][kernel] = row
    print(json.dumps(report))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
