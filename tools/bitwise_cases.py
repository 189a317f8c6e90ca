"""Bitwise comparison of two builds of libkmvp.so over a fixed, seeded list of products.

    KMVP_LIB=/path/to/old/libkmvp.so python tools/bitwise_cases.py run old.npz
    KMVP_LIB=/path/to/new/libkmvp.so python tools/bitwise_cases.py run new.npz     (another process)
    python tools/bitwise_cases.py compare old.npz new.npz

`run` writes, per product, the SHA-256 of the result's bytes (equal digests: equal arrays, bit for bit), its first 4096
values, the kernel's name and the dispatch note -- or the error a product was refused with; `compare` requires equal
digests, names and notes, and that every product ran on the kernel of the runner it is listed for (a quiet dispatch
elsewhere would compare equal without reaching that runner), and exits with status 1 otherwise.  `time` prints, per path and size, the first
product after kmvp_set_points (total time, packing included) and a repeat product (kernel time).

The list reaches every runner of kmvp_product.hip that has a launch plan: the staged matrix-core paths (fast, fastmm,
cfast, cfastmm), the float32 cell paths (cell, cellmm) and cell64 -- every case with the segments option unset and 3
and at 2 000, 40 007 and 330 017 points (few targets: one tile per wave, single-stage segments; many: the big tiles), with a second product on the same context after a new signal (the re-pack rules),
and a few cases through the host exchange (a world of one rank: the real exchange path).
"""
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

SIZES = (2000, 40007, 330017)
G, A, I, X = "gaussian", "absolute-exponential", "inverse-distance", "exp-dot"


def spec(path, kernel, D, E=1, norm=False, fast=None, tiles=0, density=False, other_targets=False, dtype="float32",
         shape=-1, exchange=False, sizes=SIZES):
    return dict(path=path, kernel=kernel, D=D, E=E, norm=norm, fast=fast, tiles=tiles, density=density,
                other_targets=other_targets, dtype=dtype, shape=shape, exchange=exchange, sizes=sizes)


def specs():
    s = []
    # fast_kernel: D 2, 3, 7; tiles 1, 2, 4; every kernel; normalised; density
    s += [spec("fast", G, D, fast=1, tiles=t) for D in (2, 3, 7) for t in (0, 1, 2, 4)]
    s += [spec("fast", k, 3, fast=1, norm=n) for k in (A, I) for n in (False, True)]
    s += [spec("fast", G, 3, fast=1, density=True), spec("fast", G, 3, fast=1, exchange=True)]
    # fastmm_kernel: D 3, 16, 64; NE 1, 16, 17, 33, 70; both kernels; targets == and != sources; exp(<x,y>)
    s += [spec("fastmm", G, 64, E=1, fast=1)]
    s += [spec("fastmm", G, D, E=E, fast=1) for D in (3, 16, 64) for E in (16, 17, 33, 70)]
    s += [spec("fastmm", G, 3, E=16, norm=True, fast=1), spec("fastmm", G, 3, E=69, norm=True, fast=1, tiles=1)]
    s += [spec("fastmm", G, 3, E=8, fast=1, other_targets=True), spec("fastmm", G, 3, E=40, norm=True, fast=1, other_targets=True)]
    s += [spec("fastmm", A, 16, E=E, norm=n, fast=1) for E in (1, 17, 40) for n in (False, True)]
    s += [spec("fastmm", X, 8, E=E, norm=n, other_targets=True) for E in (4, 40) for n in (False, True)]
    s += [spec("fastmm", X, 8, E=4, norm=True, other_targets=True, exchange=True)]
    # cfast_kernel: three kernels, tiles
    s += [spec("cfast", k, 3, fast=2, norm=n) for k in (G, A, I) for n in (False, True)]
    s += [spec("cfast", A, 3, fast=2, tiles=t) for t in (1, 2, 4)]
    s += [spec("cfast", G, 2, fast=2, density=True)]
    # cfastmm_kernel: NE as for fastmm; exp(-r), 1/r, the Gaussian
    s += [spec("cfastmm", A, 3, E=E, fast=2) for E in (16, 17, 33, 70)]
    s += [spec("cfastmm", I, 3, E=E, norm=n, fast=2) for E in (4, 40) for n in (False, True)]
    s += [spec("cfastmm", G, 4, E=16, norm=True, fast=2), spec("cfastmm", A, 2, E=8, fast=2, other_targets=True, tiles=1)]
    s += [spec("cfastmm", A, 3, E=40, fast=2, exchange=True)]
    # cell_kernel (fast_sqdists 4) and cellmm_kernel (3), both MFMA shapes; tiles 0, 1, 2, 4, 8; E 1 and 3; normalised; density
    for fast, path in ((4, "cell"), (3, "cellmm")):
        s += [spec(path, G, 3, fast=fast, tiles=t) for t in (0, 1, 2, 4, 8)]
        s += [spec(path, G, 3, fast=fast, norm=True), spec(path, G, 2, fast=fast, density=True)]
        s += [spec(path, G, 3, fast=fast, other_targets=True), spec(path, G, 3, fast=fast, exchange=True)]
    s += [spec("cellmm", G, 3, E=3, norm=n, fast=3, shape=sh)
          for n in (False, True) for sh in (-1, 0, 1)]
    s += [spec("cellmm", G, 3, fast=3, shape=sh, tiles=8) for sh in (0, 1)]
    # cell64_kernel
    s += [spec("cell64", G, 3, fast=3, dtype="float64", norm=n) for n in (False, True)]
    s += [spec("cell64", G, 2, fast=3, dtype="float64", density=True)]
    return s


def reaches(sp, kernel_name):
    """the kernel's name belongs to the runner the case is listed for (cellmm_kernel / cellmm16_kernel: both shapes)"""
    return kernel_name.startswith("cellmm") if sp["path"] == "cellmm" else kernel_name.startswith(sp["path"] + "_kernel")


def case_id(sp, n, segments):
    keys = ("path", "kernel", "D", "E", "norm", "fast", "tiles", "density", "other_targets", "dtype", "shape", "exchange")
    return "|".join("%s=%s" % (k, sp[k]) for k in keys) + "|N=%d|segments=%d" % (n, segments)


def inputs(sp, n):
    rs = np.random.RandomState((sp["D"] * 1000003 + sp["E"] * 10007 + n) % (1 << 31))
    dt = np.dtype(sp["dtype"])
    # exp(<x,y>): logits of a few units; the distance kernels: a cube of a few length scales
    y = (rs.randn(n, sp["D"]) * 0.7 if sp["kernel"] == X else rs.rand(n, sp["D"]) * 2.0).astype(dt)
    x = None
    if sp["other_targets"]:
        m = max(1, (n * 3) // 4 + 5)
        x = (rs.randn(m, sp["D"]) * 0.7 if sp["kernel"] == X else rs.rand(m, sp["D"]) * 2.0).astype(dt)
    b1 = rs.randn(n, sp["E"]).astype(dt)
    b2 = (rs.rand(n, sp["E"]) * 100.0 - 3.0).astype(dt)
    return y, x, b1, b2


def open_context(sp, segments):
    from kernel_matrix_benchmarks_amd import _lib

    ctx = _lib.Context(0)
    if sp["fast"] is not None:
        ctx.set_option("fast_sqdists", sp["fast"])
    ctx.set_option("fast_tiles", sp["tiles"])
    ctx.set_option("segments", segments)
    ctx.set_option("cellmm_shape", sp["shape"])
    if sp["exchange"]:
        ctx.comm_init_host(lambda array, op: None, 0, 1)  # one rank: its sum is the sum
    return ctx


def run_case(sp, n, segments):
    from kernel_matrix_benchmarks_amd import _lib

    code, _ = _lib.dtype_code(sp["dtype"])
    y, x, b1, b2 = inputs(sp, n)
    ctx = open_context(sp, segments)
    out = []
    try:
        ctx.set_points(y, x, code)
        if sp["kernel"] != X:
            ctx.fit(sp["kernel"])
        for b in (b1, b2):
            try:
                ctx.set_signal(None if sp["density"] else b)
                ctx.run(sp["kernel"], sp["norm"])
                res = ctx.get_result(ctx.N, 1 if sp["density"] else sp["E"])
                out.append((res, ctx.last_kernel_name, ctx.last_dispatch_note, ctx.last_total_ms, ctx.last_kernel_ms))
            except _lib.KmvpError as e:  # a refusal is a result too: both builds must refuse alike
                out.append((np.zeros((0, 0)), "ERROR", str(e), 0.0, 0.0))
    finally:
        ctx.close()
    return out


def cmd_run(path):
    results, meta = {}, {}
    for sp in specs():
        for n in sp["sizes"]:
            for segments in (0, 3):
                cid = case_id(sp, n, segments)
                for k, (res, name, note, _, _) in enumerate(run_case(sp, n, segments)):
                    results["%s|product=%d" % (cid, k)] = res.ravel()[:4096]
                    meta["%s|product=%d" % (cid, k)] = [name, note, hashlib.sha256(np.ascontiguousarray(res).tobytes()).hexdigest(),
                                                        bool(np.any(np.isnan(res))), reaches(sp, name)]
                print(cid, meta[cid + "|product=0"][0], flush=True)
    np.savez_compressed(path, __meta__=np.array(json.dumps(meta)), **results)
    print("%d results written to %s" % (len(results), path))


def cmd_compare(a_path, b_path):
    a, b = np.load(a_path), np.load(b_path)
    ma, mb = json.loads(str(a["__meta__"])), json.loads(str(b["__meta__"]))
    bad = 0
    if set(ma) != set(mb):
        print("different case lists:", sorted(set(ma) ^ set(mb))[:5])
        bad += 1
    kernels = {}
    for cid in sorted(set(ma) & set(mb)):
        if ma[cid] != mb[cid] or ma[cid][3] or not ma[cid][4]:  # digest, name, note; a NaN or another runner's kernel too
            bad += 1
            diff = float(np.max(np.abs(a[cid] - b[cid]))) if a[cid].shape == b[cid].shape else float("nan")
            print("DIFFERENT", cid, ma[cid], mb[cid], "max |a - b| =", diff)
        kernels[ma[cid][0]] = kernels.get(ma[cid][0], 0) + 1
    print("%d results compared, %d differ; kernels reached: %s" % (len(ma), bad, json.dumps(kernels, sort_keys=True)))
    return 1 if bad else 0


def cmd_time(label):
    timed = [spec("fast", G, 3, fast=1), spec("fastmm", G, 3, E=16, fast=1), spec("cfast", A, 3, fast=2),
             spec("cfastmm", A, 3, E=16, fast=2), spec("cell", G, 3, fast=4), spec("cellmm", G, 3, fast=3),
             spec("cell64", G, 3, fast=3, dtype="float64", sizes=(2000, 200000))]
    for sp in timed:
        for n in (sp["sizes"][0], 1000000 if sp["dtype"] == "float32" else sp["sizes"][1]):
            first, again = run_case(sp, n, 0)
            print(json.dumps({"build": label, "path": sp["path"], "N": n, "kernel": first[1],
                              "first_total_ms": round(first[3], 4), "repeat_kernel_ms": round(again[4], 4)}), flush=True)


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "run":
        cmd_run(sys.argv[2])
    elif len(sys.argv) >= 4 and sys.argv[1] == "compare":
        sys.exit(cmd_compare(sys.argv[2], sys.argv[3]))
    elif len(sys.argv) >= 3 and sys.argv[1] == "time":
        cmd_time(sys.argv[2])
    else:
        sys.exit(__doc__)
