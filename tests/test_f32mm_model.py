"""oracle/kmvp_f32mm_model.py on the CPU: the model with rounding disabled against the float64 oracle, a numpy emulation of
fastmm_kernel's steps inside the band, and the band's size against the row's mass."""
import numpy as np
import pytest

import kmvp_f32mm_model as fm
import kmvp_oracle

CASES = [  # (kernel, path, N, M, D, same)
    ("gaussian", "fastmm", 40, 40, 7, True),
    ("gaussian", "fastmm", 37, 53, 16, False),
    ("absolute-exponential", "fastmm", 30, 70, 9, False),
    ("exp-dot", "fastmm", 30, 45, 23, False),
    ("gaussian", "cfastmm", 33, 60, 3, False),
    ("absolute-exponential", "cfastmm", 40, 40, 4, True),
    ("inverse-distance", "cfastmm", 40, 40, 3, True),
]


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}-{c[1]}-N{c[2]}-M{c[3]}-D{c[4]}" for c in CASES])
@pytest.mark.parametrize("norm", [False, True])
def test_model_without_rounding_is_the_float64_product(case, norm):
    kernel, path, N, M, D, same = case
    rs = np.random.RandomState(N + M + D)
    y = rs.rand(M, D) / np.sqrt(D)
    x = None if same else rs.rand(N, D) / np.sqrt(D)
    b = rs.randn(M, 3) + 0.5
    got = fm.f32mm_product(kernel, y, x, b, norm, path=path, rounding=False).value
    if kernel == "exp-dot":
        want = kmvp_oracle.exp_dot_product(source_points=y, target_points=x, source_signal=b, normalize_rows=norm)
    else:
        want = kmvp_oracle.product(kernel=kernel, source_points=y, target_points=x, source_signal=b, normalize_rows=norm)
    assert got.shape == want.shape
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin)
    assert np.abs(got[fin] - want[fin]).max() <= 1e-12 * np.abs(want[fin]).max()


def test_model_of_exp_dot_with_large_logits_and_nan_rows():
    """Rows whose logits reach several hundred: the model's value stays finite relative to its own scale; a NaN target is
    a non-finite row and no other."""
    rs = np.random.RandomState(4)
    y, x, b = rs.randn(200, 8) * 6, rs.randn(30, 8) * 6, rs.randn(200, 2)
    x[3, 1] = np.nan
    for norm in (False, True):
        m = fm.f32mm_product("exp-dot", y, x, b, norm)
        ok = np.arange(30) != 3
        want = kmvp_oracle.exp_dot_product(source_points=y, target_points=x[ok], source_signal=b, normalize_rows=norm)
        assert m.nonfinite[3] and np.array_equal(m.nonfinite[ok], ~np.isfinite(want).all(axis=1))
        fin = np.isfinite(want).all(axis=1)
        scale = np.max(np.abs(want[fin]), axis=1, keepdims=True) if not norm else np.abs(want).max()
        assert (np.abs(m.value[ok][fin] - want[fin]) <= 1e-12 * scale).all()
        if not norm:  # rows of very different scales: relative to their own, and the mass bounds the value
            assert (np.abs(m.value[ok][fin]) <= m.mass[ok][fin] * (1 + 1e-12)).all()


def _bf16(v):
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    return u.view(np.float32)


def _split3(v):
    v = np.asarray(v, dtype=np.float32)
    hi = _bf16(v)
    r1 = (v - hi).astype(np.float32)
    mid = _bf16(r1)
    lo = _bf16((r1 - mid).astype(np.float32))
    return hi, mid, lo


def emulate_fastmm(kernel, y, x, b, norm, rs, chunk_sources=64):
    """fastmm_kernel's steps in numpy: centred, scaled float32 operands split three ways into bf16, the six products per
    dimension, norms and the shift column summed in float32 in a random order, T = 2^(15 + kop) k in float32 and split
    through float16, b sigma split through float16, the second product in float32 chains folded into float64 every
    `chunk_sources` sources.  kop: the row's final shift (floor of the smallest exponent)."""
    N, D = x.shape
    M = y.shape[0]
    E = b.shape[1]
    dot = kernel == "exp-dot"
    c = {"gaussian": fm.C_GAUSSIAN, "absolute-exponential": fm.C_ABSEXP, "exp-dot": np.float32(fm.LOG2E / 2)}[kernel]
    pts = np.concatenate((y, x))
    centre = (0.5 * (pts.min(0) + pts.max(0))).astype(np.float32)
    f32 = np.float32
    if dot:
        xv, yv = x.astype(f32), (y.astype(f32) * f32(c)).astype(f32)
    else:
        xv = ((x.astype(f32) - centre).astype(f32) * f32(c)).astype(f32)
        yv = ((y.astype(f32) - centre).astype(f32) * f32(c)).astype(f32)
    xh, xm, xl = _split3(xv)
    yh, ym, yl = _split3(yv)
    # the six products per dimension of the kernel's rows (-2 y pieces against x pieces)
    terms = [(-2 * yh)[None, :, :] * xh[:, None, :], (-2 * yh)[None, :, :] * xm[:, None, :],
             (-2 * ym)[None, :, :] * xh[:, None, :], (-2 * yh)[None, :, :] * xl[:, None, :],
             (-2 * ym)[None, :, :] * xm[:, None, :], (-2 * yl)[None, :, :] * xh[:, None, :]]
    parts = [t.astype(f32) for t in terms]
    if not dot:
        nx = np.sum(xv.astype(np.float64) ** 2, axis=1).astype(f32)
        ny = np.sum(yv.astype(np.float64) ** 2, axis=1).astype(f32)
        for p in _split3(nx):
            parts.append(np.broadcast_to(p[:, None, None], (N, M, 1)).astype(f32))
        for p in _split3(ny):
            parts.append(np.broadcast_to(p[None, :, None], (N, M, 1)).astype(f32))
    allp = np.concatenate(parts, axis=2)
    order = rs.permutation(allp.shape[2])
    S = np.zeros((N, M), dtype=f32)
    for k in order:
        S = (S + allp[:, :, k]).astype(f32)
    # the row's shift and T
    if kernel == "absolute-exponential":
        r = np.sqrt(np.abs(S)).astype(f32)
        kop = np.floor(r.min(axis=1, keepdims=True))
        T = np.exp2((f32(15) + kop.astype(f32) - r).astype(f32)).astype(f32)
    else:
        kop = np.floor(S.min(axis=1, keepdims=True))
        T = np.exp2((-(S - kop.astype(f32)) + f32(15)).astype(f32)).astype(f32)
    Th = T.astype(np.float16).astype(f32)
    Tl = (T - Th).astype(f32).astype(np.float16).astype(f32)
    # the signal, with the denominator column of ones
    bb = np.concatenate((b, np.ones((M, 1))), axis=1) if norm else b
    bmax = np.abs(bb).max(axis=0)
    eb = np.floor(np.log2(bmax)) + 1
    sigma = np.exp2(np.clip(14 - eb, -100, 100)).astype(f32)
    v = (bb.astype(f32) * sigma).astype(f32)
    bh = v.astype(np.float16).astype(f32)
    bl = (v - bh).astype(f32).astype(np.float16).astype(f32)
    acc = np.zeros((N, bb.shape[1]), dtype=np.float64)
    for j0 in range(0, M, chunk_sources):
        a32 = np.zeros((N, bb.shape[1]), dtype=f32)
        for j in range(j0, min(M, j0 + chunk_sources)):
            for p in (Th[:, j, None] * bh[j], Th[:, j, None] * bl[j], Tl[:, j, None] * bh[j]):
                a32 = (a32 + p.astype(f32)).astype(f32)
        acc += a32
    out = acc / sigma.astype(np.float64) * np.exp2(-15.0 - kop)
    if norm:
        return out[:, :E] / out[:, E:]
    if dot:
        return out * 1.0  # true scale: 2^-kop already applied
    return out


EMU = [("gaussian", 3, False), ("gaussian", 9, True), ("absolute-exponential", 6, False), ("exp-dot", 5, False)]


@pytest.mark.parametrize("kernel,D,same", EMU, ids=[f"{k}-D{d}" for k, d, _ in EMU])
@pytest.mark.parametrize("norm", [False, True])
def test_emulated_kernel_stays_inside_the_band(kernel, D, same, norm):
    rs = np.random.RandomState(11 + D)
    M, N, E = 150, 24, 3
    y = (rs.rand(M, D) * 1.2 / np.sqrt(D)).astype(np.float32).astype(np.float64)
    x = y[:N].copy() if same else (rs.rand(N, D) * 1.2 / np.sqrt(D)).astype(np.float32).astype(np.float64)
    if kernel == "exp-dot":
        y, x = y * 6, x * 6
    b = (rs.randn(M, E) + 0.7).astype(np.float32).astype(np.float64)
    model = fm.f32mm_product(kernel, y, None if same else x, b, norm, rows=np.arange(N), chunk=32)
    worst = 0.0
    for trial in range(3):
        got = emulate_fastmm(kernel, y, x, b, norm, rs, chunk_sources=64)
        err = np.abs(got - model.value)
        assert (err <= model.band).all(), (trial, float((err / model.band).max()))
        worst = max(worst, float((err / model.band).max()))
    assert worst > 1e-4  # the emulation's errors are not negligible against the band: the band is not vacuous


@pytest.mark.parametrize("kernel,path", [("gaussian", "fastmm"), ("absolute-exponential", "fastmm"), ("exp-dot", "fastmm"),
                                         ("gaussian", "cfastmm"), ("absolute-exponential", "cfastmm"),
                                         ("inverse-distance", "cfastmm")])
def test_band_is_far_below_the_suites_float32_yardstick(kernel, path):
    """band / mass on clouds inside the radius rule, printed: 2^-14 ... 2^-13 on fastmm_kernel's functions, where the S
    term charges the large constant columns once (k-ordered chain) and the fp32 chains of the second product weigh as
    much; cfastmm_kernel's bound on the group radius makes its band 2^-13 ... 2^-10.3."""
    rs = np.random.RandomState(3)
    D = 3 if path == "cfastmm" else 8
    y = rs.rand(400, D) * (1.5 / np.sqrt(D))
    x = None if kernel == "inverse-distance" else rs.rand(90, D) * (1.5 / np.sqrt(D))
    b = rs.randn(400, 4) + 1.0
    for norm in (False, True):
        m = fm.f32mm_product(kernel, y, x, b, norm, path=path)
        assert not m.flagged.any()
        ratio = float((m.band / m.mass).max())
        print(f"\nf32mm model {kernel:22s} {path:8s} norm={norm}: max band/mass {ratio:.3g} (2^{np.log2(ratio):.1f})")
        assert ratio < (2.0 ** -12.5 if path == "fastmm" else 2.0 ** -10), (kernel, path, norm, ratio)
