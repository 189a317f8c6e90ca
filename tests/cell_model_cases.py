"""Clouds, runs and numpy emulations shared by tests/test_cell_model.py (CPU) and tests/test_gpu_cell_arith.py (GPU): the
cell-form Gaussian kernels (cell_kernel, cellmm_kernel, cellmm16_kernel, cell64_kernel) against oracle/kmvp_cell_model.py.

A case is a dict: name, y (M, D) sources, x (N, D) targets or None (the same points), b (M, E) signal, precision, near (every
point within one cloud inside the radius rule: the sharpness rule applies) and runs, a list of (path, sig, E, options).
path is the kernel expected to run: "cell", "cellmm", "cellmm16" or "cell64"; sig is "product", "density" or "norm"; options
are (key, value) pairs for kmvp_set_option on top of the ones that force the path (OPTIONS).

lattice() is a Python restatement of the library's grid rule for the CPU tests ONLY: the GPU test takes the real layout
from kmvp_cell_layout, and the model itself restates no rule of the cells.

emulate() restates the kernels' own steps in numpy -- f16 operands rounded toward zero by truncating the significand, bf16
and fp32 to nearest, v_exp_f32 flushing below 2^-126, Kahan sums, the running accumulators and vprev, folds at the cell
ends and the segment's end -- with ONE defect on request (DEFECTS)."""
import numpy as np

import kmvp_cell_model as cm

F32, F64 = np.float32, np.float64
NAME = {"cell": "cell_kernel", "cellmm": "cellmm_kernel", "cellmm16": "cellmm16_kernel", "cell64": "cell64_kernel"}
# the options that force a path (include/kmvp.h): fast_sqdists 4 = cell_kernel, 3 = the cell form; cellmm_shape 0 / 1
OPTIONS = {"cell": (("fast_sqdists", 4),), "cellmm": (("fast_sqdists", 3), ("cellmm_shape", 0)),
           "cellmm16": (("fast_sqdists", 3), ("cellmm_shape", 1)), "cell64": (("fast_sqdists", 3),)}
DEFAULTS = (("fast_tiles", 0), ("segments", 0), ("cell_fused", -1), ("cell_shared_build", -1), ("cell_balance", -1), ("chunk", 512))
SIGS = ("product", "density", "norm")
DEFECTS = ("no-mid", "xz-for-yz", "no-kahan", "vprev-stale", "segment-end-unfolded", "sigma-times-2", "pad-b-one", "dm-of-v",
           "cell64-degree-5", "u-own-centre")
POPULATIONS = (1, 31, 32, 33, 8 * 32, 8 * 32 + 1, 12 * 32 + 5, 0)                 # of the 2^3 cells; one empty
POPULATIONS64 = (1, 127, 128, 129, 64, 0, 3, 130)


def case(name, y, x, b, runs, precision=F32, near=False):
    y = np.ascontiguousarray(y, dtype=precision)
    x = None if x is None else np.ascontiguousarray(x, dtype=precision)
    return dict(name=name, y=y, x=x, b=np.ascontiguousarray(b, dtype=precision), runs=runs, precision=np.dtype(precision), near=near)


def box_cloud(rs, D, side, populations, shift=0.0):
    """Points of a [0, side]^D box of 2^D cells with the given populations (cell index = bits of its position in the list);
    the box's two extreme corners are points of their own cells, so that the library's box-fitted grid IS this grid."""
    pts = []
    for c, n in enumerate(populations[:2 ** D]):
        lo = np.array([(c >> a) & 1 for a in range(D)]) * side / 2
        p = lo + (0.02 + 0.96 * rs.rand(n, D)) * side / 2
        if c == 0 and n:
            p[0] = 0.0
        if c == 2 ** D - 1 and n:
            p[0] = side
        pts.append(p)
    y = np.concatenate(pts)
    return y[rs.permutation(len(y))] + shift


def signal(rs, M, E):
    return rs.randn(M, E) + 0.25


def grid_runs(D):
    """Every instantiation: TT = 1, 2, 4, 8 x plain / density / normalised on the three float32 kernels, and cellmm's
    several columns (one launch per column): E = 2, 5."""
    runs = []
    for tt in (1, 2, 4, 8):
        for sig in SIGS:
            for path in ("cell", "cellmm", "cellmm16"):
                runs.append((path, sig, 1, (("fast_tiles", tt),)))
    for E in (2, 5):
        runs += [("cellmm", "product", E, (("fast_tiles", 2),)), ("cellmm16", "norm", E, (("fast_tiles", 8),))]
    return runs


def grid_cases():
    """D = 1, 2, 3; targets = sources and != sources; the chosen populations."""
    for D in (1, 2, 3):
        rs = np.random.RandomState(100 + D)
        pops = POPULATIONS if D == 3 else ((31, 32, 12 * 32 + 5, 1) if D == 2 else (33, 8 * 32 + 1))
        side = 0.2 if D == 3 else (0.24 if D == 2 else 0.34)
        y = box_cloud(rs, D, side, pops)
        yield case(("grid", D, "same"), y, None, signal(rs, len(y), 5), grid_runs(D), near=True)
        x = np.concatenate((rs.rand(75, D) * side, [[0.0] * D, [side] * D]))
        yield case(("grid", D, "other"), y, x, signal(rs, len(y), 5), grid_runs(D), near=True)


def plan_cases():
    """1 / 2 / 3 / 17 segments (6000 sources: 17 stages of twelve tiles), the REST list present and absent, fused against two
    launches, the shared build against every wavefront's own (a cell of 1100 points: whole one-cell workgroups at TT = 8),
    and count-cut cells: columns cut by the width cap and, in a dense slab, by the count."""
    rs = np.random.RandomState(7)
    y = box_cloud(rs, 3, 0.2, (1100, 300, 40, 5, 2048, 33, 1024, 1450))
    x = np.concatenate((rs.rand(318, 3) * 0.2, [[0.0] * 3, [0.2] * 3]))
    runs = []
    for seg in (1, 2, 3, 17):
        runs += [("cellmm16", "product", 1, (("fast_tiles", 8), ("segments", seg))), ("cellmm", "product", 1, (("fast_tiles", 4), ("segments", seg))),
                 ("cell", "product", 1, (("fast_tiles", 2), ("segments", seg)))]
    yield case(("plan", "segments"), y, x, signal(rs, len(y), 1), runs, near=True)
    y = box_cloud(rs, 3, 0.2, (1100, 300, 40, 5, 1024, 33, 64, 34))
    mm16 = [("cellmm16", "product", 1, (("fast_tiles", 8),) + o) for o in ((), (("cell_fused", 0),), (("cell_shared_build", 0),),
                                                                          (("cell_shared_build", 0), ("cell_fused", 0)))]
    runs = mm16 + [("cellmm16", "norm", 1, (("fast_tiles", 8), ("cell_shared_build", 0))), ("cellmm", "product", 1, (("fast_tiles", 8),)),
                   ("cell", "norm", 1, (("fast_tiles", 8), ("chunk", 128)))]
    yield case(("plan", "rest"), y, None, signal(rs, len(y), 1), runs, near=True)
    y = box_cloud(rs, 3, 0.2, (1024, 1024, 0, 0, 0, 0, 0, 1024))                   # whole workgroups only: no REST list
    yield case(("plan", "no-rest"), y, None, signal(rs, len(y), 1), mm16[:1] + mm16[2:3], near=True)
    for height in (1.0, 4.0):                                                      # columns cut along z; at 4 the width cap binds
        y = rs.rand(3000, 3) * [0.2, 0.2, height]
        y[:1400] = rs.rand(1400, 3) * [0.1, 0.1, 0.05] + [0.0, 0.0, 0.3]           # a dense slab in one column: cut by the count
        y[-2], y[-1] = 0.0, [0.2, 0.2, height]
        runs = [("cellmm16", sig, 1, (("fast_tiles", 8), ("cell_balance", 1))) for sig in ("product", "norm")]
        runs += [("cellmm", "product", 1, (("fast_tiles", 8), ("cell_balance", 1))), ("cell", "product", 1, (("fast_tiles", 8), ("cell_balance", 1)))]
        yield case(("plan", "count-cut", height), y, None, signal(rs, len(y), 1), runs, near=True)


def range_cases():
    rs = np.random.RandomState(11)
    three = [(p, "product", 1, (("fast_tiles", 2),)) for p in ("cell", "cellmm", "cellmm16")]
    # a line at the largest extent the radius rule admits (squared half-diagonal 8 / log2 e): the ends see each other at e^-22
    y = rs.rand(1500, 3) * [4.7, 0.1, 0.1]
    y[0], y[1] = 0.0, [4.7, 0.1, 0.1]
    yield case(("range", "line"), y, None, signal(rs, 1500, 1), three + [("cellmm16", "norm", 1, (("fast_tiles", 8),))])
    # targets whose whole row is far: the sources at one end, the targets at the other
    ys = rs.rand(700, 3) * [0.3, 0.1, 0.1]
    xs = rs.rand(300, 3) * [0.3, 0.1, 0.1] + [4.4, 0.0, 0.0]
    ys[0], xs[0] = 0.0, [4.7, 0.1, 0.1]
    yield case(("range", "far-rows"), ys, xs, signal(rs, 700, 1), three + [("cellmm", "density", 1, (("fast_tiles", 1),))])
    # cell_kernel outside the radius rule: rows from e^-2 down to e^-108, past the flush of U
    xs = np.concatenate([rs.rand(12, 3) * 0.1 + [r, 0.0, 0.0] for r in np.linspace(1.4, 10.6, 25)])
    ys = rs.rand(500, 3) * 0.2
    yield case(("range", "flush"), ys, xs, np.abs(signal(rs, 500, 1)) + 0.5, [("cell", sig, 1, (("fast_sqdists", 3), ("fast_tiles", 1))) for sig in ("product", "density")])
    # the worst corners: every point within 2 % of a cell side of the (-,-,-) or the (+,+,+) corner of its cell, one-signed b
    pts = []
    for c in range(8):
        lo = np.array([(c >> a) & 1 for a in range(3)]) * 0.1
        pts += [lo + rs.rand(60, 3) * 0.002, lo + 0.1 - rs.rand(60, 3) * 0.002]
    y = np.concatenate(pts)
    y[0], y[-1] = 0.0, 0.2
    yield case(("range", "corners"), y, None, np.abs(rs.randn(len(y), 1)) + 0.5, three, near=True)
    # one corner: every point within 2 % of the (+,-,+) corner of its cell, so that t = 2 d.e is 0.0144 for EVERY pair and of
    # one sign, and the monomials x z and y z differ in sign: nothing of the remainder cancels over the sources
    pts = [np.array([(c >> a) & 1 for a in range(3)]) * 0.1 + [0.1, 0.0, 0.1] + rs.rand(90, 3) * 0.002 * [-1, 1, -1] for c in range(8)]
    y = np.concatenate(pts + [[[0.0] * 3, [0.2] * 3]])
    yield case(("range", "one-corner"), y, None, np.abs(rs.randn(len(y), 1)) + 0.5, three, near=True)
    for shift in (100.0, 1000.0):
        y = box_cloud(rs, 3, 0.2, (40, 70, 33, 1, 0, 90, 64, 50), shift)
        yield case(("range", "moved", shift), y, None, signal(rs, len(y), 1), three)


def signal_cases():
    rs = np.random.RandomState(13)
    three = [(p, "product", 1, (("fast_tiles", 2),)) for p in ("cell", "cellmm", "cellmm16")]
    # |b| over 2^+-20: the small sources sit next to their own targets, 4.6 away from the large ones
    y = np.concatenate((rs.rand(400, 3) * 0.1, rs.rand(400, 3) * 0.1 + [4.6, 0.0, 0.0]))
    b = np.concatenate((rs.randn(400, 1) * 2.0 ** 20, rs.randn(400, 1) * 2.0 ** -20))
    yield case(("signal", "2^+-20"), y, None, b, three)
    y = box_cloud(rs, 3, 0.2, (100, 200, 33, 64, 1, 0, 150, 90))
    b = rs.randn(len(y), 1)
    b[17] = 1.0e6
    yield case(("signal", "spike"), y, None, b, three, near=True)
    b = rs.randn(len(y), 3)
    b[:, 1] = 0.0
    yield case(("signal", "zero-column"), y, None, b, [("cellmm", "product", 3, (("fast_tiles", 2),)), ("cellmm16", "norm", 3, (("fast_tiles", 4),))], near=True)
    # 3000 copies of one point with b of alternating sign beside an ordinary cell: cancellation in the Kahan sum
    y = np.concatenate((np.tile([[0.03, 0.04, 0.05]], (3000, 1)), rs.rand(200, 3) * 0.1 + 0.1, [[0.0] * 3, [0.2] * 3]))
    b = np.concatenate(((-1.0) ** np.arange(3000) * (1.0 + 0.25 * rs.rand(3000)), rs.randn(202)))[:, None]
    yield case(("signal", "copies"), y, None, b, [(p, "product", 1, (("fast_tiles", 8),)) for p in ("cell", "cellmm", "cellmm16")], near=True)


def cell64_cases():
    rs = np.random.RandomState(17)
    runs = [("cell64", sig, 1, (("segments", s),)) for sig in SIGS for s in (0, 3)]
    y = box_cloud(rs, 3, 0.36, POPULATIONS64)                                      # side sqrt(0.1 / 3) = 0.1826 >= 0.18
    yield case(("cell64", "grid"), y, None, signal(rs, len(y), 1), runs, F64, near=True)
    x = np.concatenate((rs.rand(150, 3) * 0.36, [[0.0] * 3, [0.36] * 3]))
    yield case(("cell64", "grid-other"), y, x, signal(rs, len(y), 1), runs[:3], F64, near=True)
    ys = rs.rand(300, 3) * [0.5, 0.18, 0.18]
    xs = rs.rand(200, 3) * [0.5, 0.18, 0.18] + [5.0, 0.0, 0.0]
    yield case(("cell64", "far-rows"), ys, xs, signal(rs, 300, 1), runs[:1] + runs[4:5], F64)


def state_cases():
    """Two small clouds for the second product on one context: a column cloud on which the count cut applies, then the 2^3 cells."""
    rs = np.random.RandomState(19)
    y = rs.rand(1500, 3) * [0.2, 0.2, 1.0]
    y[-2], y[-1] = 0.0, [0.2, 0.2, 1.0]
    yield case(("state", "column"), y, None, signal(rs, len(y), 1), [], near=True)
    yield case(("state", "grid"), box_cloud(rs, 3, 0.2, POPULATIONS), None, signal(rs, sum(POPULATIONS), 1), [], near=True)


def by_name(name):
    return [c for g in groups().values() for c in g if c["name"] == name][0]


def groups():
    return {"grid": list(grid_cases()), "plan": list(plan_cases()), "range": list(range_cases()), "signal": list(signal_cases()),
            "cell64": list(cell64_cases())}


def signal_of(c, sig, E):
    return None if sig == "density" else c["b"][:, :E]


def lattice(c, path):
    """The lattice of kmvp_product.hip's cell_make_grid in Python (CPU tests only): the bounding box of both clouds divided per
    axis into the fewest equal cells of side <= sqrt(2 T_MAX / D); a layout dict as kmvp_cell_layout returns it (without
    sigma_b: sigma_of() below), in float32 as the library computes box, side and centres."""
    y, x = c["y"], c["y"] if c["x"] is None else c["x"]
    D = y.shape[1]
    f64 = path == "cell64"
    t_max = cm.CELL64_T_MAX if f64 else cm.CELL_T_MAX
    h_max = F32(np.sqrt(2.0 * t_max / D)) if f64 else F32(np.sqrt(F32(2.0) * F32(t_max) / F32(D)))
    both = np.concatenate((y, x)).astype(F32)
    lo_box, hi_box = both.min(axis=0), both.max(axis=0)
    centre = F32(0.5) * (lo_box + hi_box)
    half = np.maximum(hi_box - centre, centre - lo_box).astype(F32)
    lo = (centre - half).astype(F32)
    g = np.maximum(1.0, np.ceil(2.0 * half.astype(F64) / float(h_max)))
    h = np.where(half > 0, (2.0 * half.astype(F64) / g).astype(F32), h_max).astype(F32)
    inv_h = (F32(1.0) / h).astype(F32)
    out = {}
    for side, p in (("source", y), ("target", x)):
        if f64:
            idx = np.floor((p.astype(F64) - lo.astype(F64)) * inv_h.astype(F64))
        else:
            idx = np.floor(((p.astype(F32) - lo).astype(F32) * inv_h).astype(F32))
        idx = np.clip(idx, 0, g - 1).astype(np.int64)
        if f64:
            cen = lo.astype(F64) + (idx + 0.5) * h.astype(F64)
        else:
            cen = (lo + ((idx.astype(F32) + F32(0.5)) * h).astype(F32)).astype(F32).astype(F64)
        key = (idx * (1024 ** np.arange(D))).sum(axis=1)
        keys, first, ids = np.unique(key, return_index=True, return_inverse=True)
        cen3 = np.zeros((len(keys), 3))
        cen3[:, :D] = cen[first]
        out[side + "_cell"], out[side + "_centres"] = ids.astype(np.int32), cen3
    out["count_cut"] = False
    return out


def sigma_of(c, sig, E, col, layout):
    """sigma_b of one launch by cellmm_scale_kernel's rule on the lattice (fmax = 0.104): CPU tests only."""
    y = c["y"]
    D = y.shape[1]
    both = np.concatenate((y, y if c["x"] is None else c["x"])).astype(F64)
    ext = both.max(axis=0) - both.min(axis=0)
    h_max = np.sqrt(2.0 * cm.CELL_T_MAX / D)
    h = np.where(ext > 0, ext / np.maximum(1, np.ceil(ext / h_max)), h_max)
    wlog2 = int(np.ceil((h * ext).sum() * 1.4426950408889634))
    bmax = 1.0 if (sig == "density" or col == E) else float(np.abs(c["b"][:, col]).max())
    ex = 0
    if np.isfinite(bmax) and bmax > 0:
        ex = int(np.clip(15 - np.frexp(F32(bmax) * F32(0.104))[1] - wlog2, -100, 100))
    return 2.0 ** ex


def model(c, path, sig, E, layout, chunk=512):
    return cm.cell_product(c["y"], c["x"], signal_of(c, sig, E), sig == "norm", path=path, layout=layout, chunk=chunk)


# ---- the kernels' steps in numpy ----------------------------------------------------------------------------------------

LOG2E = F32(1.4426950408889634)


def rtz_f16(v):
    """float32 -> f16 toward zero (v_cvt_pkrtz_f16_f32), as float64: the significand cut to 11 bits -- to a multiple of 2^-24
    in the denormal range -- and the largest finite f16 beyond it."""
    v = np.asarray(v, dtype=F64)
    m, ex = np.frexp(np.abs(v))
    q = np.ldexp(1.0, np.maximum(ex - 1, -14) - 10)
    out = np.sign(v) * np.minimum(np.floor(np.abs(v) / q) * q, 65504.0)
    return np.where(np.isfinite(v), out, v)


def rne_f16(v):
    with np.errstate(over="ignore"):
        return np.asarray(v, dtype=F32).astype(np.float16).astype(F64)


def rne_bf16(v):
    bits = np.ascontiguousarray(v, dtype=F32).view(np.uint32).astype(np.uint64)
    bits = (bits + 0x7FFF + ((bits >> 16) & 1)) & 0xFFFF0000
    return bits.astype(np.uint32).view(F32).astype(F64)


def exp2_f32(arg):
    """v_exp_f32: 2^arg to nearest (the model grants it TRANS), 0 below the smallest normal number."""
    with np.errstate(over="ignore", under="ignore"):
        r = np.exp2(np.asarray(arg, dtype=F64)).astype(F32)
    return np.where(r < F32(2.0 ** -126), F32(0), r)


def fma32(a, b, c):
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


def tree_sum32(v, axis):
    """fp32 sum by halving (the packed adds and swaps of the folds), one rounding per level"""
    v = np.moveaxis(np.asarray(v, dtype=F32), axis, -1)
    while v.shape[-1] > 1:
        if v.shape[-1] & 1:
            v = np.concatenate((v, np.zeros(v.shape[:-1] + (1,), F32)), axis=-1)
        v = (v[..., 0::2] + v[..., 1::2]).astype(F32)
    return v[..., 0]


def tiles_of(layout, pad=32):
    """The source tiles in the kernels' order: cell by cell, 32 a tile, the last one of a cell padded (index -1)."""
    scell = np.asarray(layout["source_cell"])
    out = []
    for s in range(len(layout["source_centres"])):
        idx = np.nonzero(scell == s)[0]
        for t0 in range(0, len(idx), pad):
            tile = np.full(pad, -1, dtype=np.int64)
            tile[:len(idx[t0:t0 + pad])] = idx[t0:t0 + pad]
            out.append((s, tile))
    return out


def emulate(c, path, sig, E, layout, sigma=None, segments=1, chunk=512, defect=None, rows=None):
    """The modelled kernels' own steps on one case; (N, E), or (len(rows), E) for the target rows asked for.  sigma: sigma_b
    per launch (cellmm paths): a function of the column (E: the denominator's launch)."""
    if rows is not None:
        x = c["y"] if c["x"] is None else c["x"]
        layout = dict(layout, target_cell=np.asarray(layout["target_cell"])[rows])
        c = dict(c, x=np.ascontiguousarray(x[rows]))
    b = signal_of(c, sig, E)
    bb = np.ones((len(c["y"]), 1), c["precision"]) if b is None else b
    cols = [bb[:, e] for e in range(bb.shape[1])] + ([np.ones(len(bb), c["precision"])] if sig == "norm" else [])
    if path == "cell64":
        res = _emulate64(c, layout, cols, defect)
    elif path == "cell":
        res = _emulate_cell(c, layout, cols, chunk, defect)
    else:
        res = np.stack([_emulate_mm(c, layout, col, sigma(e), segments, defect) for e, col in enumerate(cols)], axis=1)
    if sig == "norm":
        with np.errstate(divide="ignore", invalid="ignore"):
            return res[:, :-1] / res[:, -1:]
    return res


def _geometry(c, layout, precision):
    y, x = c["y"], c["y"] if c["x"] is None else c["x"]
    scen = np.asarray(layout["source_centres"])[:, :y.shape[1]]
    tcen = np.asarray(layout["target_centres"])[:, :y.shape[1]]
    e = cm.offsets(y, layout["source_cell"], layout["source_centres"], precision).astype(precision)
    d = cm.offsets(x, layout["target_cell"], layout["target_centres"], precision).astype(precision)
    cT = tcen[layout["target_cell"]].astype(precision)
    return d, e, cT, scen.astype(precision)


def _emulate_mm(c, layout, bcol, sigma, segments, defect):
    """cellmm_kernel / cellmm16_body on all targets at once: per source tile the operand A for every target's cell, the
    accumulating MFMA (one rounding per tile and row here), the Kahan sum of W b, the fold where the source cell changes."""
    d, e, cT, scen = _geometry(c, layout, F32)
    N, D = d.shape
    tiles = tiles_of(layout)
    per_seg = -(-len(tiles) // max(1, segments))
    sig32 = F32(sigma)
    # targets: s = 64 d, hi and mid to nearest, the quadratic monomials x 64 (cellmm_target_operand)
    d3 = np.zeros((N, 3), F32)
    d3[:, :D] = d
    s = (d3 * F32(64)).astype(F32)
    sh = rne_f16(s)
    sm = rne_f16((s.astype(F64) - sh).astype(F32))
    q = F32(64)
    quad_t = {"xx": rne_f16(((d3[:, 0] * d3[:, 0]).astype(F32) * (F32(0.5) * q)).astype(F32)), "yy": rne_f16(((d3[:, 1] * d3[:, 1]).astype(F32) * (F32(0.5) * q)).astype(F32)),
              "zz": rne_f16(((d3[:, 2] * d3[:, 2]).astype(F32) * (F32(0.5) * q)).astype(F32)), "xz": rne_f16(((d3[:, 0] * d3[:, 2]).astype(F32) * q).astype(F32)),
              "yz": rne_f16(((d3[:, 1] * d3[:, 2]).astype(F32) * q).astype(F32)), "xy": rne_f16(((d3[:, 0] * d3[:, 1]).astype(F32) * q).astype(F32))}
    out = np.zeros(N, F64)
    for seg0 in range(0, len(tiles), per_seg):
        acc = np.zeros((N, 32), F32)                       # per target and source row: the sixteen slots' running sum
        vprev = np.zeros(N, F32)
        S0, S0c = np.zeros((N, 32), F32), np.zeros((N, 32), F32)
        U, key = np.zeros(N, F32), -2
        seg_tiles = tiles[seg0:seg0 + per_seg]

        def fold():
            nonlocal vprev, S0, S0c, out
            s0 = (tree_sum32(S0, 1) * F32(64)).astype(F32)
            v = tree_sum32(acc, 1)
            share = ((v - vprev).astype(F32) + s0).astype(F32)
            with np.errstate(under="ignore"):
                out = out + (U * share).astype(F32).astype(F64)
            if defect != "vprev-stale":
                vprev = v
            S0, S0c = np.zeros((N, 32), F32), np.zeros((N, 32), F32)

        for ti, (sc, tile) in enumerate(seg_tiles):
            if sc != key:
                if key >= 0:
                    fold()
                key = sc
                delta = (cT - scen[sc][None, :]).astype(F32)                      # (N, D)
                D1 = np.zeros((N, 3), F32)
                D1[:, :D] = (delta * LOG2E).astype(F32)
                df = (d + (np.zeros_like(delta) if defect == "u-own-centre" else delta)).astype(F32)
                s2 = np.zeros(N, F32)
                for a in range(D):
                    s2 = fma32(df[:, a], df[:, a], s2)
                U = exp2_f32((s2 * -LOG2E).astype(F32))
            valid = tile >= 0
            ee = np.zeros((32, 3), F32)
            ee[valid, :D] = e[tile[valid]]
            bj = np.zeros(32, F32)
            bj[valid] = bcol[tile[valid]]
            if defect == "pad-b-one":
                bj[~valid] = 1
            ef = (F32(2) * ee).astype(F32)
            g = (((ee[:, 0] * ee[:, 0]).astype(F32) + (ee[:, 1] * ee[:, 1]).astype(F32)).astype(F32) + (ee[:, 2] * ee[:, 2]).astype(F32)).astype(F32)
            g = (g * -LOG2E).astype(F32)
            bq = (bj * sig32).astype(F32)
            arg = fma32(ef[None, :, 0], D1[:, None, 0], fma32(ef[None, :, 1], D1[:, None, 1], fma32(ef[None, :, 2], D1[:, None, 2], g[None, :])))
            wexp = exp2_f32(arg)                                                  # (N, 32)
            wb = (wexp * bq[None, :]).astype(F32)
            if defect == "no-kahan":
                S0 = (S0 + wb).astype(F32)
            else:
                yk = fma32(bq[None, :], wexp, -S0c)
                tk = (S0 + yk).astype(F32)
                S0c = ((tk - S0).astype(F32) - yk).astype(F32)
                S0 = tk
            prod = np.zeros((N, 32), F64)
            for a in range(3):                                                    # linear slots: hi x hi, hi x mid, mid x hi
                u1 = (ef[None, :, a] * wb).astype(F32)
                c1 = rtz_f16(u1)
                mid = np.zeros_like(c1) if defect == "no-mid" else rtz_f16(fma32(ef[None, :, a], wb, -c1))
                prod += sh[:, None, a] * c1 + sh[:, None, a] * mid + sm[:, None, a] * c1
            for name, (p, r) in {"xx": (0, 0), "yy": (1, 1), "zz": (2, 2), "xz": (0, 2), "yz": (1, 2), "xy": (0, 1)}.items():
                if defect == "xz-for-yz" and name == "yz":
                    p, r = 0, 2
                mono = (ef[:, p] * ef[:, r]).astype(F32)
                prod += quad_t[name][:, None] * rtz_f16((mono[None, :] * wb).astype(F32))
            acc = (acc.astype(F64) + prod).astype(F32)
        if key >= 0 and defect != "segment-end-unfolded":
            fold()
    inv = 1.0 / (float(sigma) * 64.0)
    return out * (0.5 * inv if defect == "sigma-times-2" else inv)


def _emulate_cell(c, layout, cols, chunk, defect):
    """cell_kernel on all targets at once: bf16 slots, one MFMA from zero per tile, two chains of eight per lane half, acc in
    fp32 folded into fp64 every chunk_stages stages of four tiles."""
    d, e, cT, scen = _geometry(c, layout, F32)
    N, D = d.shape
    tiles = tiles_of(layout)
    d3 = np.zeros((N, 3), F32)
    d3[:, :D] = d
    dh = rne_bf16(d3)
    dm = rne_bf16(d3 if defect == "dm-of-v" else (d3.astype(F64) - dh).astype(F32))
    xb = np.zeros((N, 16))
    xb[:, 0] = 1.0
    for a in range(3):
        xb[:, 1 + 3 * a], xb[:, 2 + 3 * a], xb[:, 3 + 3 * a] = dh[:, a], dh[:, a], dm[:, a]
    for k, (p, r) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
        xb[:, 10 + k] = rne_bf16((d3[:, p] * d3[:, r]).astype(F32))
    fold_tiles = max(1, chunk // 128) * 4
    half = np.array([(r % 8) >= 4 for r in range(32)])                            # rows 8 g + 4 h .. + 3 belong to lane half h
    outd = np.zeros((N, len(cols), 2), F64)
    acc = np.zeros((N, len(cols), 2), F32)
    key, U = -2, np.zeros(N, F32)
    for ti, (sc, tile) in enumerate(tiles):
        delta = (cT - scen[sc][None, :]).astype(F32)
        if sc != key:
            key = sc
            df = (d + (np.zeros_like(delta) if defect == "u-own-centre" else delta)).astype(F32)
            s2 = np.zeros(N, F32)
            for a in range(D):
                s2 = fma32(df[:, a], df[:, a], s2)
            U = exp2_f32((s2 * -LOG2E).astype(F32))
        valid = tile >= 0
        ee = np.zeros((32, 3), F32)
        ee[valid, :D] = e[tile[valid]]
        ya = np.zeros((32, 16))
        ya[:, 0] = valid
        for a in range(3):
            e2 = (F32(2) * ee[:, a]).astype(F32)
            eh = rne_bf16(e2)
            em = rne_bf16((e2.astype(F64) - eh).astype(F32))
            ya[:, 1 + 3 * a], ya[:, 2 + 3 * a], ya[:, 3 + 3 * a] = eh, em, eh
        for k, (p, r, f) in enumerate(((0, 0, 2), (1, 1, 2), (2, 2, 2), (0, 1, 4), (0, 2, 4), (1, 2, 4))):
            ya[:, 10 + k] = rne_bf16(((F32(f) * ee[:, p]).astype(F32) * ee[:, r]).astype(F32))
        poly = (xb @ ya.T).astype(F32)                                            # (N, 32): exact products, one rounding here
        arg = np.zeros((N, 32), F32)
        dl3 = np.zeros((N, 3), F32)
        dl3[:, :D] = delta
        for a in range(3):
            arg = fma32(ee[None, :, a], ((F32(2) * dl3[:, None, a]).astype(F32) - ee[None, :, a]).astype(F32), arg)
        w = exp2_f32((arg * LOG2E).astype(F32))
        for k, col in enumerate(cols):
            bj = np.zeros(32, F32)
            bj[valid] = col[tile[valid]]
            if defect == "pad-b-one":
                bj[~valid] = 1
            wv = (w * bj[None, :]).astype(F32)
            for h in (0, 1):
                p = (poly[:, half == bool(h)].astype(F64) * wv[:, half == bool(h)]).sum(axis=1).astype(F32)
                with np.errstate(under="ignore"):
                    acc[:, k, h] = fma32(U, p, acc[:, k, h])
        if (ti + 1) % fold_tiles == 0:
            outd += acc
            acc[:] = 0
    return (outd + acc).sum(axis=2)


def _emulate64(c, layout, cols, defect):
    """cell64_kernel in float64: t by FMAs, the Horner form of degree 7, fma(p, w, acc_c) over a cell, fma(U, acc_c, acc)."""
    d, e, cT, scen = _geometry(c, layout, F64)
    N = len(d)
    scell = np.asarray(layout["source_cell"])
    out = np.zeros((N, len(cols)))
    for sc in range(len(scen)):
        idx = np.nonzero(scell == sc)[0]
        if not len(idx):
            continue
        delta = cT - scen[sc][None, :]
        rec = 2.0 * e[idx]
        arg = (rec[None, :, :] * (delta[:, None, :] - 0.25 * rec[None, :, :])).sum(axis=2)
        w = np.exp(arg)
        t = d @ rec.T
        coef = [1.0 / 5040, 1.0 / 720, 1.0 / 120, 1.0 / 24, 1.0 / 6, 0.5, 1.0, 1.0]
        if defect == "cell64-degree-5":
            coef = coef[2:]
        p = np.full_like(t, coef[0])
        for cf in coef[1:]:
            p = p * t + cf
        df = d + (0.0 if defect == "u-own-centre" else delta)
        U = np.exp(-(df * df).sum(axis=1))
        for k, col in enumerate(cols):
            out[:, k] += U * (p * (w * col[idx][None, :])).sum(axis=1)
    return out
