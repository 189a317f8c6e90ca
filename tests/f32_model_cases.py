"""Clouds, signals and numpy emulations shared by tests/test_f32_model.py (CPU) and tests/test_gpu_f32_arith.py (GPU):
the GPU test runs fast_kernel / cfast_kernel on exactly the clouds whose model the CPU test holds to the flag cap and on
which the defect emulations must leave the band.

Clouds: Gaussian products on clusters whose kernel values within a row span about e^0 ... e^-6; exp(-r) and 1/r on
interleaved jittered lattices -- a random subset of g^D lattice sites, jitter of +- a quarter of the spacing, sources and
targets on distinct sites -- because fast_kernel has only absolute accuracy in s and uniform random points at low D put
pairs so close that their rows would be flagged."""
import numpy as np

import kmvp_f32_model as f1
import kmvp_f32mm_model as fm
from test_f32mm_model import _split3  # (the bf16 helpers of the fastmm emulation, shared)

KERNELS = ("gaussian", "absolute-exponential", "inverse-distance")
SIGS = ("product", "norm", "density")
FAST_MAX_D, FAST_MAX_D_FOUR_TILES, FAST_MAX_D_TWO_TILES = 39, 7, 23   # kmvp_internal.hpp
SPREAD = 2.0


def clustered(rs, n, D, spread=SPREAD, centres=None, k=6):
    if centres is None:
        centres = rs.randn(k, D) * np.sqrt(spread / D)
    lab = rs.randint(len(centres), size=n)
    pts = centres[lab] + rs.randn(n, D) * (0.35 * np.sqrt(spread / D))
    return pts.astype(np.float32), lab, centres


def signal(rs, lab):
    """One column of mixed sign with a nonzero mean and per-cluster offsets."""
    off = rs.randn(lab.max() + 1, 1) * 2.0
    return (rs.randn(len(lab), 1) + 1.0 + off[lab]).astype(np.float32)


def lattice(rs, D, M, N, diameter=3.0, spacing=None):
    """M sources and N targets on distinct sites of the smallest g^D lattice that holds them, jittered by +- a quarter of
    the spacing; the lattice's diagonal is `diameter`, unless the spacing is given."""
    g = 2
    while g ** D < M + N:
        g += 1
    if g ** D <= 4 * (M + N):
        flat = rs.permutation(g ** D)[:M + N]
        sites = np.stack(np.unravel_index(flat, (g,) * D), axis=1)
    else:                                   # far more sites than points: draw and keep the distinct ones
        sites = np.unique(rs.randint(g, size=(4 * (M + N), D)), axis=0)
        sites = sites[rs.permutation(len(sites))[:M + N]]
        assert len(sites) == M + N
    h = spacing if spacing else diameter / (g * np.sqrt(D))
    pts = ((sites + 0.5 + rs.uniform(-0.25, 0.25, size=sites.shape)) * h).astype(np.float32)
    return pts[:M], pts[M:]


def cloud(rs, kernel, D, M, N, same, diameter=3.0):
    """(y, x or None, lab) of the kind the kernel function's tests use."""
    if kernel == "gaussian":
        y, lab, cen = clustered(rs, M, D)
        x = None if same else clustered(rs, N, D, centres=cen)[0]
    else:
        y, x = lattice(rs, D, M, 0 if same else N, diameter)
        x = None if same else x
        lab = rs.randint(6, size=M)
    return y, x, lab


def case(name, kernel, path, y, x, b, **kw):
    return dict(name=name, kernel=kernel, path=path, y=y, x=x, b=b, kw=kw)


def model(c, sig, **more):
    """The model of a case for one signal mode."""
    kw = dict(c["kw"], **more)
    return f1.f32_product(c["kernel"], c["y"], c["x"], None if sig == "density" else c["b"], sig == "norm", path=c["path"], **kw)


def fast_tile_counts(D):
    return (1, 2, 4) if D <= FAST_MAX_D_FOUR_TILES else ((1, 2) if D <= FAST_MAX_D_TWO_TILES else (1,))


def fast_grid_cases():
    """Every kernel function at every D = 1 ... 39, N = 67 targets and M = 101 sources (ragged in both), same points and
    different points alternating over D.  exp(-r) with a signal beyond D = 4 goes to fastmm_kernel on clouds inside the
    radius rule (scaled squared half-diagonal <= 8), fast_sqdists = 1 or not: those clouds are wider, a lattice of
    diagonal 8."""
    for kernel in KERNELS:
        for D in range(1, FAST_MAX_D + 1):
            rs = np.random.RandomState(1000 * KERNELS.index(kernel) + D)
            same = D % 2 == 0
            y, x, lab = cloud(rs, kernel, D, 101, 67, same, 8.0 if kernel == "absolute-exponential" and D > 4 else 3.0)
            yield case(("grid", kernel, D), kernel, "fast", y, x, signal(rs, lab))


def cfast_grid_cases():
    """M = 301 (three groups, the last one padded), N = 130, D = 1 and 4; 1/r on the sources themselves."""
    for kernel in KERNELS:
        for D in (1, 4):
            rs = np.random.RandomState(77 * KERNELS.index(kernel) + D)
            y, x, lab = cloud(rs, kernel, D, 301, 130, kernel == "inverse-distance")
            yield case(("cgrid", kernel, D), kernel, "cfast", y, x, signal(rs, lab))


STRESS_SEGMENTS = (1, 2, 3, 17)
STRESS_CHUNK = 32


def stress_cases():
    """fast_kernel's stages, segments and folds: M = 3000 x N = 200 at D = 3 (24 stages of four tiles) and M = 330 at
    D = 24 (stages of two tiles: six, the last one with a single ragged tile); a quarter of the targets each 1.6, 4.2, 6.5
    and 9.0 beyond the cloud (Gaussian rows e^-2 ... e^-80); the sources sorted so that each target's largest terms
    come last."""
    for kernel in KERNELS:
        for D, M in ((3, 3000), (24, 330)):
            rs = np.random.RandomState(31 + D + KERNELS.index(kernel))
            N = 200
            if kernel == "gaussian":
                y = (rs.rand(M, D) * (0.6 if D == 3 else 0.25)).astype(np.float32)
                x = (rs.rand(N, D) * (0.6 if D == 3 else 0.25)).astype(np.float32)
            else:
                y, x = lattice(rs, D, M, N, diameter=1.0)
            x[:, 0] += np.repeat([1.6, 4.2, 6.5, 9.0], N // 4).astype(np.float32)
            y = np.ascontiguousarray(y[np.argsort(-np.linalg.norm(y - x.mean(0), axis=1))])  # the closest last
            b = signal(rs, rs.randint(6, size=M))
            yield case(("stress", kernel, D), kernel, "fast", y, x, b, chunk=STRESS_CHUNK)


def rare_cases():
    """cfast_kernel's rare branch, targets == sources: a tight cluster (pairs below tau_g, recomputed), a far cluster
    (skipped by the reach gate), a cluster translated by +100 in every coordinate.  1/r also with one off-diagonal
    coincident pair: exactly those two rows are non-finite."""
    for kernel in ("absolute-exponential", "inverse-distance"):
        for D in (2, 3):
            for dup in ((False, True) if kernel == "inverse-distance" else (False,)):
                rs = np.random.RandomState(50 + D)
                if kernel == "absolute-exponential":
                    wide = lattice(rs, D, 150, 0, diameter=2.0)[0]
                    tight = (wide[3] + lattice(rs, D, 60, 0, diameter=2e-3)[0]).astype(np.float32)
                    far = lattice(rs, D, 60, 0, diameter=1.0)[0]
                    moved = lattice(rs, D, 60, 0, diameter=1.5)[0]
                else:
                    # 1/r: the model bounds a group's radius by the sources' diameter (~100 sqrt D here) and so flags
                    # rows with a pair closer than ~0.13; the clusters keep their neighbours 0.2 apart, which the
                    # groups that straddle two clusters (tau_g = 0.03 R_g^2) still recompute
                    wide = lattice(rs, D, 150, 0, spacing=0.4)[0]
                    tight = lattice(rs, D, 60, 0, spacing=0.4)[0]
                    tight[:, 0] += wide[:, 0].max() + np.float32(0.5)
                    far = lattice(rs, D, 60, 0, spacing=0.4)[0]
                    moved = lattice(rs, D, 60, 0, spacing=0.4)[0]
                far = (far + np.float32(40.0)).astype(np.float32)
                moved = (moved + np.float32(100.0)).astype(np.float32)
                y = np.concatenate((wide, tight, far, moved))[rs.permutation(330)]
                if dup:
                    y[200] = y[17]
                yield case(("rare", kernel, D, dup), kernel, "cfast", np.ascontiguousarray(y), None,
                           signal(rs, rs.randint(6, size=330)))


SHARDS = ((0, 67), (67, 131), (131, 200))


def zero_rule_cases():
    """The zero rule and the own-pair rule.  fast_kernel: 1/r with N = 450 > M = 200 (the rule wraps), exp(-r) on the
    sources themselves; both also as three source slices (SHARDS).  The first two targets of the different-points cloud
    sit on the corners of the lattice's box, so that every slice sees the box -- hence the centre -- of the whole.
    cfast_kernel: exp(-r) and 1/r on the sources themselves, whole and sliced (same_points_global)."""
    rs = np.random.RandomState(91)
    y, x = lattice(rs, 3, 200, 450)
    x[0], x[1] = 0.0, np.float32(3.0 / np.sqrt(3.0))
    b = signal(rs, rs.randint(6, size=200))
    yield case(("wrap", "inverse-distance"), "inverse-distance", "fast", y, x, b)
    yield case(("own", "absolute-exponential"), "absolute-exponential", "fast", y, None, b)
    yield case(("own", "inverse-distance"), "inverse-distance", "fast", y, None, b)
    y2 = lattice(rs, 2, 200, 0)[0]
    yield case(("own-c", "absolute-exponential"), "absolute-exponential", "cfast", y2, None, b)
    yield case(("own-c", "inverse-distance"), "inverse-distance", "cfast", y2, None, b)


EDGE_SHAPES = ((1, 1), (1, 33), (33, 1), (31, 65), (97, 129))


def edge_cases():
    """(M, N) of 1 and not multiples of 32, different points (1/r on cfast_kernel: the sources themselves)."""
    for path, D in (("fast", 3), ("cfast", 2)):
        for kernel in KERNELS:
            for M, N in EDGE_SHAPES:
                rs = np.random.RandomState(5 + M + N + D)
                y, x, lab = cloud(rs, kernel, D, M, N, path == "cfast" and kernel == "inverse-distance")
                yield case(("edge", path, kernel, M, N), kernel, path, y, x, signal(rs, lab))


def nonfinite_cases():
    """A NaN target coordinate (row 5); on cfast_kernel also sources at +-inf.  (1/r on cfast_kernel needs the sources
    themselves as targets and is left to rare_cases.)"""
    for path, D in (("fast", 3), ("cfast", 2)):
        for kernel in KERNELS:
            if path == "cfast" and kernel == "inverse-distance":
                continue
            rs = np.random.RandomState(15 + D + KERNELS.index(kernel))
            y, x, lab = cloud(rs, kernel, D, 300, 64, False)
            x[5, D - 1] = np.nan
            if path == "cfast":
                y[7, 0], y[11, 0] = np.inf, -np.inf
            yield case(("nonfinite", path, kernel), kernel, path, y, x, signal(rs, lab))


def all_cases():
    for gen in (fast_grid_cases, cfast_grid_cases, stress_cases, rare_cases, zero_rule_cases, edge_cases, nonfinite_cases):
        yield from gen()


# ---- numpy emulations of the kernels' own steps ----------------------------------------------------------------------

f32 = np.float32
DEFECTS = ("xlyh-xhyl", "mm", "ynorm-lo", "half-chain", "no-own-pair", "no-wrap")


def _fma(a, b, c):
    return (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(f32)


def _kval(kernel, S):
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if kernel != "inverse-distance":                    # v_exp_f32: no denormal results
            k = np.exp2(-S if kernel == "gaussian" else -np.sqrt(np.abs(S)).astype(f32)).astype(f32)
            return np.where(k < f32(2.0 ** -126), f32(0), k)
        return (f32(1) / np.sqrt(np.abs(S)).astype(f32)).astype(f32)


def _chain_columns(tp, sp):
    """The six products per dimension: target pieces (x_h, x_m, x_h, x_l, x_m, x_h) against -2 (y_h, y_h, y_m, y_h, y_m,
    y_l) -- (N, M) each, exact in float32."""
    (xh, xm, xl), (yh, ym, yl) = tp, sp
    return [np.outer(t, (f32(-2) * s_).astype(f32)).astype(f32) for t, s_ in ((xh, yh), (xm, yh), (xh, ym), (xl, yh), (xm, ym), (xh, yl))]


def _accumulate(k, b, sig, ST, chunk_stages, seg_stages, defect=None):
    """fast_kernel's / cfast_kernel's sums of one column: per tile of 32 sources and lane half two fp32 chains over the
    registers (rows 8 (reg / 4) + 4 h + reg % 4), p0 + p1, acc +=, a fold into float64 every chunk_stages stages; lane
    halves and segments added in float64.  k (N, M), b (M,) or None (adds)."""
    N, M = k.shape
    m_tiles = -(-M // 32)
    pad = m_tiles * 32 - M
    k = np.concatenate((k, np.zeros((N, pad), f32)), axis=1)
    b = None if b is None else np.concatenate((b.astype(f32), np.zeros(pad, f32)))
    m_stages = -(-m_tiles // ST)
    total = np.zeros(N)
    for s0 in range(0, m_stages, seg_stages):
        for h in (0, 1):
            acc, accd, in_chunk = np.zeros(N, f32), np.zeros(N), 0
            for stage in range(s0, min(m_stages, s0 + seg_stages)):
                for t in range(stage * ST, min(m_tiles, (stage + 1) * ST)):
                    p = [np.zeros(N, f32), np.zeros(N, f32)]
                    for reg in range(16):
                        if defect == "half-chain" and t == 1 and h == 1 and reg % 2 == 1:
                            continue                        # one chain of eight sources left out
                        j = 32 * t + 8 * (reg // 4) + 4 * h + reg % 4
                        p[reg & 1] = (p[reg & 1] + k[:, j]).astype(f32) if b is None else _fma(k[:, j], b[j], p[reg & 1])
                    acc = (acc + (p[0] + p[1]).astype(f32)).astype(f32)
                in_chunk += 1
                if in_chunk == chunk_stages:
                    accd, acc, in_chunk = accd + acc, np.zeros(N, f32), 0
            total += accd + acc
    return total


def _finish(k, b, sig, *acc_args, **acc_kw):
    if sig == "density":
        return _accumulate(k, None, sig, *acc_args, **acc_kw)[:, None]
    num = _accumulate(k, b[:, 0], sig, *acc_args, **acc_kw)
    if sig == "norm":
        with np.errstate(divide="ignore", invalid="ignore"):
            return (num / _accumulate(k, None, sig, *acc_args, **acc_kw))[:, None]
    return num[:, None]


def emulate_fast(kernel, y, x, b, sig, *, same_global=False, chunk=512, segments=1, j_offset=0, M_total=None, defect=None):
    """fast_kernel's steps in numpy float32: pack (centre, scale, |.|^2 in double rounded once), the three-way bf16 split,
    K = 6 D + 6 exact products summed in k order in float32, the kernel function, the exact rules, the chains and folds."""
    y = np.asarray(y, f32)
    own = x is None or same_global
    xx = y if x is None else np.asarray(x, f32)
    M, D = y.shape
    N = xx.shape[0]
    M_total = M if M_total is None else M_total
    pts = y if x is None else np.concatenate((y, xx))
    centre = (f32(0.5) * (pts.min(0) + pts.max(0))).astype(f32)
    c = f32(fm.kernel_constant(kernel))
    xv = ((xx - centre).astype(f32) * c).astype(f32)
    yv = ((y - centre).astype(f32) * c).astype(f32)
    nx = (xv.astype(np.float64) ** 2).sum(1).astype(f32)
    ny = (yv.astype(np.float64) ** 2).sum(1).astype(f32)
    S = np.zeros((N, M), f32)
    for d in range(D):
        for role, col in enumerate(_chain_columns(_split3(xv[:, d]), _split3(yv[:, d]))):
            if (defect == "xlyh-xhyl" and role in (3, 5)) or (defect == "mm" and role == 4):
                continue
            S = (S + col).astype(f32)
    for i, piece in enumerate(_split3(ny)):                 # |y'|^2 h, m, l against ones
        if not (defect == "ynorm-lo" and i == 2):
            S = (S + piece[None, :]).astype(f32)
    for piece in _split3(nx):                               # ones against |x'|^2 h, m, l
        S = (S + piece[:, None]).astype(f32)
    k = _kval(kernel, S)
    i = np.arange(N)
    g = i if defect == "no-wrap" else i % (M_total + 1)
    jz = np.where(g < M_total, g - j_offset, -1)
    hit = (jz >= 0) & (jz < M)
    if kernel == "inverse-distance":
        k[i[hit], jz[hit]] = 0
    if kernel == "absolute-exponential" and own and defect != "no-own-pair":
        k[i[hit], jz[hit]] = 1
    ST = f1.fast_stage_tiles(f1.fast_ksteps(D))
    m_stages = -(-(-(-M // 32)) // ST)
    return _finish(k, b, sig, ST, max(1, chunk // (32 * ST)), -(-m_stages // segments), defect=defect)


def emulate_cfast_group(kernel, y, x, b, sig):
    """cfast_kernel on ONE group (M <= 128 sources; targets == sources when x is None): rows relative to the group's
    centre, the target operand rebuilt relative to it, K = 32 columns in k order, pairs at or below tau_g recomputed from
    the raw coordinates with the zero rule and the exact s = 0 of the diagonal."""
    y = np.asarray(y, f32)
    xx = y if x is None else np.asarray(x, f32)
    M, D = y.shape
    N = xx.shape[0]
    assert M <= fm.CF_GROUP and D <= 4
    y4 = np.concatenate((y, np.zeros((M, 4 - D), f32)), axis=1)
    x4 = np.concatenate((xx, np.zeros((N, 4 - D), f32)), axis=1)
    cen = (f32(0.5) * (y4.min(0) + y4.max(0))).astype(f32)
    c = f32(fm.kernel_constant(kernel))
    yr = ((y4 - cen).astype(f32) * c).astype(f32)
    ysq = (yr.astype(np.float64) ** 2).sum(1).astype(f32)
    tau = f32(fm.CF_KAPPA) * ysq.max()

    def sq4(v):                                             # fmaf(v3, v3, fmaf(v2, v2, fmaf(v1, v1, v0 v0)))
        s_ = (v[..., 0] * v[..., 0]).astype(f32)
        for d in (1, 2, 3):
            s_ = (v[..., d].astype(np.float64) ** 2 + s_.astype(np.float64)).astype(f32)
        return s_

    xr = ((x4 - cen).astype(f32) * c).astype(f32)
    xsq = sq4(xr)
    yn, xn = _split3(ysq), _split3(xsq)
    cols = []
    for d in range(4):
        cols += _chain_columns(_split3(xr[:, d]), _split3(yr[:, d]))
        cols += [(np.broadcast_to(yn[0][None, :], (N, M)), np.broadcast_to(yn[1][None, :], (N, M))),
                 (np.broadcast_to(yn[2][None, :], (N, M)), np.broadcast_to(xn[0][:, None], (N, M))),
                 (np.broadcast_to(xn[1][:, None], (N, M)), np.broadcast_to(xn[2][:, None], (N, M))), ()][d]
    S = np.zeros((N, M), f32)
    for col in cols:
        S = (S + col).astype(f32)
    e = ((x4[:, None, :] - y4[None, :, :]).astype(f32) * c).astype(f32)
    exact = sq4(e)
    if kernel == "inverse-distance":
        i = np.arange(N)
        jz = i % (M + 1)
        exact[i[jz < M], jz[jz < M]] = np.inf
    S = np.where(S > tau, S, exact)
    return _finish(_kval(kernel, S), b, sig, 4, 4, 1)
