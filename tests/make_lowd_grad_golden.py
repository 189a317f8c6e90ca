"""Writes ``tests/golden/lowd_grad_parent.npz``: lowd_grad_kernel's and lowd_dscale_kernel's results on
``lowd_grad_model_cases.golden_cases()``, for ``test_gpu_lowd_grad_arith.py``'s bit-for-bit check.

The file was recorded ONCE, on an MI355X, from the library of the commit BEFORE the guard's select and the NaN row of the
two kernels were changed (``KMVP_LIB=<that library> python tests/make_lowd_grad_golden.py``).  Run against a later
library it records that library's bits, which is not what the test is about: do so only after a change that is meant
to move them, and say so.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(HERE, "..", "oracle"), os.path.join(HERE, "..")]
sys.dont_write_bytecode = True

import lowd_grad_model_cases as gc  # noqa: E402
from kernel_matrix_benchmarks_amd import _lib  # noqa: E402


def main(path):
    out = {}
    for c in gc.golden_cases():
        dt = c["precision"]
        ctx = _lib.Context(0)
        try:
            ctx.set_points(np.ascontiguousarray(c["y"], dtype=dt), np.ascontiguousarray(c["x"], dtype=dt),
                           _lib.KMVP_F64 if dt == np.float64 else _lib.KMVP_F32)
            ctx.set_signal(np.ascontiguousarray(c["b"]))
            for which in gc.whiches(c["kernel"]):
                (ctx.run_dscale if which == "dscale" else ctx.run_grad)(c["kernel"])
                N, (E, D) = len(c["x"]), (c["b"].shape[1], c["y"].shape[1])
                got = ctx.get_result(N, E * D).reshape(N, E, D)
                assert np.isfinite(got).all()
                out[gc.golden_key(c, which)] = got
        finally:
            ctx.close()
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes, library {_lib.LIB_PATH}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "golden", "lowd_grad_parent.npz"))
