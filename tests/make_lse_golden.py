"""Records tests/golden/lse_parent.npz: lowd_lse_kernel's and lowd_lse_grad_kernel's results on
lse_model_cases.golden_cases() under 1 and 2 segments, from the library as built -- run on the commit BEFORE a change to
those kernels that must leave finite inputs bit for bit (tests/test_gpu_lse_arith.py).  Needs a GPU.

    python tests/make_lse_golden.py [output.npz]"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(os.path.dirname(HERE), "oracle"), os.path.dirname(HERE)]

import numpy as np  # noqa: E402

import lse_model_cases as lc  # noqa: E402
from kernel_matrix_benchmarks_amd import _lib  # noqa: E402

DTYPE = {np.dtype(np.float32): _lib.KMVP_F32, np.dtype(np.float64): _lib.KMVP_F64}


def main(path):
    out = {}
    for c in lc.golden_cases():
        dt = c["precision"]
        ctx = _lib.Context(0)
        try:
            ctx.set_points(np.ascontiguousarray(c["y"], dtype=dt), np.ascontiguousarray(c["x"], dtype=dt), DTYPE[dt])
            ctx.set_signal(np.ascontiguousarray(c["b"][:, :2]))
            N, D = c["x"].shape
            for which in lc.WHICH:
                for segments in (1, 2):
                    ctx.set_option("chunk", 512)
                    ctx.set_option("segments", segments)
                    (ctx.run_lse_grad if which == "grad" else ctx.run_lse)(c["kernel"])
                    assert ctx.last_kernel_name == lc.NAME[which]
                    got = ctx.get_result(N, 2 * D).reshape(N, 2, D) if which == "grad" else ctx.get_result(N, 2)
                    assert np.isfinite(got).all()
                    out[lc.golden_key(c, which) + f"|{segments}"] = got.copy()
        finally:
            ctx.close()
    np.savez(path, **out)
    print(f"{len(out)} arrays -> {path}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "golden", "lse_parent.npz"))
