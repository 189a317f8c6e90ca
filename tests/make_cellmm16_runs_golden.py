"""Writes ``tests/golden/cellmm16_runs_parent.npz``: cellmm16_kernel's sums on ``cellmm16_runs_cases.cases()``, for
``test_cellmm16_runs.py``'s bit-for-bit check.

The file was recorded ONCE, on an MI355X, from the library of the commit BEFORE the tile loop was cut into cell runs
(``KMVP_LIB=<that library> python tests/make_cellmm16_runs_golden.py``), whose loop asked every tile for its key.  Per case
it holds the SHA-256 of the whole output (all rows, float64 bytes) and the rows of ``sample_rows`` in full.  Run against a
later library it records that library's bits, which is not what the test is about: do so only after a change that is
meant to move them, and say so.
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(HERE, "..", "oracle"), os.path.join(HERE, "..")]
sys.dont_write_bytecode = True

import cellmm16_runs_cases as rc  # noqa: E402
from kernel_matrix_benchmarks_amd import _lib  # noqa: E402


def product(y, b, options, norm):
    """the case's output (N, 1) float64, its layout and its lists"""
    ctx = _lib.Context(0)
    try:
        for k, v in {**rc.BASE, **options}.items():
            ctx.set_option(k, v)
        ctx.set_points(y, None, _lib.KMVP_F32)
        ctx.fit("gaussian")
        ctx.set_signal(b)
        ctx.run("gaussian", norm)
        assert ctx.last_kernel_name == "cellmm16_kernel", ctx.last_kernel_name
        return ctx.get_result(len(y), 1), ctx.cell_layout(), ctx.cell_lists()
    finally:
        ctx.close()


def digest(out):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(out, dtype=np.float64).tobytes()).digest(), dtype=np.uint8)


def main(path):
    clouds = {name: rc.make_cloud(name) for name in rc.CLOUDS}
    out = {}
    for cid, name, options, norm in rc.cases():
        y, b = clouds[name]
        got, _, lists = product(y, b, options, norm)
        assert np.isfinite(got).all(), cid
        out[cid + "/sha256"] = digest(got)
        out[cid + "/rows"] = got[rc.sample_rows(len(y)), 0]
        print(cid, lists["blocks"], lists["segments"], "fused" if lists["fused"] else "")
    np.savez_compressed(path, **out)
    print(f"{path}: {len(out)} arrays, {os.path.getsize(path)} bytes, library {_lib.LIB_PATH}")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "golden", "cellmm16_runs_parent.npz"))
