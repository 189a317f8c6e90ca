"""oracle/kmvp_bf16_model.py on the CPU: the bf16 rounding helper against torch's float32 -> bfloat16 cast, the model with
rounding disabled against the float64 oracle, and the shape of its ambiguity band."""
import numpy as np
import pytest

import kmvp_bf16_model as bm
import kmvp_oracle

torch = pytest.importorskip("torch")


def torch_bf16(v):
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def test_bf16_round_equals_torch_cast():
    bits = [0x3F808000, 0x3F818000,            # ties: even mantissa stays, odd one rounds up
            0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001,  # either side of a tie, odd and even mantissas
            0x7F7F7FFF, 0x7F7F8000, 0x7F7FFFFF,  # near the top: stays finite, ties to even (up to inf), rounds to inf
            0x7F800000, 0xFF800000,              # +-inf
            0x7FC00000, 0xFFC00000, 0x7F800001, 0x7FFFFFFF, 0x7FBFFFFF,  # NaNs, payloads whose increment would carry
            0x00000001, 0x00008000, 0x00018000, 0x007FFFFF, 0x00800000, 0x807FFFFF,  # subnormals, smallest normal
            0x00000000, 0x80000000]
    v = np.array(bits, dtype=np.uint32).view(np.float32)
    rs = np.random.RandomState(0)
    v = np.concatenate((v, rs.randint(0, 2 ** 32, 100000, dtype=np.uint64).astype(np.uint32).view(np.float32)))
    got = bm.bf16_round(v)
    want = torch_bf16(v).astype(np.float64)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan], want[~nan])
    assert np.array_equal(np.signbit(got[~nan]), np.signbit(want[~nan]))
    # with the scale: ONE float32 product, then the rounding
    a = rs.randn(1000).astype(np.float32)
    c = 1.4426950408889634
    assert np.array_equal(bm.bf16_round(a, c), torch_bf16(a * np.float32(c)).astype(np.float64) / c)


def test_bf16_of_f64_is_one_rounding_to_nearest_even():
    p = np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -40, 0.75, 2.0 ** -100 * (1 + 2.0 ** -8)])
    assert np.array_equal(bm.bf16_of_f64(p), [1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, 0.75, 2.0 ** -100])
    rs = np.random.RandomState(1)
    q = np.exp(-rs.rand(10000) * 50)
    r = bm.bf16_of_f64(q)
    assert np.all(np.abs(r - q) <= 2.0 ** -8 * q) and np.abs(r - q).max() > 2.0 ** -10 * q.min()
    # where float32 is exact on the way, torch's two-step cast agrees
    q32 = q.astype(np.float32).astype(np.float64)
    assert np.array_equal(bm.bf16_of_f64(q32), torch_bf16(q32))


CASES = [  # (kernel, N, M, D, same, j_offset, M_total)
    ("gaussian", 40, 40, 20, True, 0, None),
    ("absolute-exponential", 37, 53, 17, False, 0, None),
    ("inverse-distance", 40, 40, 20, True, 0, None),
    ("inverse-distance", 90, 30, 16, False, 0, None),     # N > M + 1: the zero rule wraps
    ("inverse-distance", 70, 25, 16, False, 20, 61),      # a source shard: global flat indices shifted by j_offset
    ("gaussian-shifted", 30, 45, 23, False, 0, None),
    ("exp-dot", 30, 45, 23, False, 0, None),
]


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}-N{c[1]}-M{c[2]}-j{c[5]}" for c in CASES])
@pytest.mark.parametrize("norm", [False, True])
def test_model_without_rounding_is_the_float64_product(case, norm):
    kernel, N, M, D, same, j_offset, M_total = case
    rs = np.random.RandomState(N + M + D)
    y = rs.rand(M, D) / np.sqrt(D)
    x = None if same else rs.rand(N, D) / np.sqrt(D)
    b = rs.randn(M, 3) + 0.5
    got = bm.mfma_product(kernel, y, x, b, norm, j_offset=j_offset, M_total=M_total, rounding=False).value
    if kernel == "exp-dot":
        want = kmvp_oracle.exp_dot_product(source_points=y, target_points=x, source_signal=b, normalize_rows=norm)
    else:
        k = "gaussian" if kernel == "gaussian-shifted" else kernel
        want = kmvp_oracle.product(kernel=k, source_points=y, target_points=x, source_signal=b, normalize_rows=norm,
                                   j_offset=j_offset, M_total=M_total)
    assert got.shape == want.shape
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin)
    assert np.abs(got[fin] - want[fin]).max() <= 1e-12 * np.abs(want[fin]).max()
    if kernel == "inverse-distance" and not same:
        # the zero rule is actually exercised: the model puts zeros where the oracle's kernel matrix has them
        K = kmvp_oracle.kernel_block(kernel, kmvp_oracle.sqdists_block(x, y, False), np.arange(N), M, j_offset, M_total)
        assert (K == 0).sum() > 0


def test_model_density_and_zero_rule_duplicates():
    rs = np.random.RandomState(5)
    y = rs.rand(50, 16)
    for kernel in ("gaussian", "inverse-distance"):
        got = bm.mfma_product(kernel, y, None, None, density=True, rounding=False).value
        want = kmvp_oracle.product(kernel=kernel, source_points=y, density_estimation=True)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    # 1/r: a duplicate off the zero rule is infinite in both; the rounded model flags its row
    y[7] = y[3]
    m = bm.mfma_product("inverse-distance", y, None, rs.randn(50, 1))
    assert m.nonfinite[3] and m.nonfinite[7] and m.nonfinite.sum() == 2
    assert m.flagged[3] and m.flagged[7]


@pytest.mark.parametrize("kernel", ["gaussian", "absolute-exponential", "inverse-distance", "gaussian-shifted", "exp-dot"])
def test_ambiguity_band_is_empty_at_eta_zero_and_grows_with_eta(kernel):
    rs = np.random.RandomState(7)
    y = rs.rand(300, 40) / 3
    x = None if kernel in ("gaussian", "absolute-exponential", "inverse-distance") else rs.rand(60, 40) / 3
    b = rs.randn(300, 2) + 1.0
    prev = None
    for eta in (0.0, 0.5, 1.0, 4.0, 64.0, 4096.0):
        m = bm.mfma_product(kernel, y, x, b, eta=eta)
        if eta == 0.0:
            assert not m.amb.any()
        else:
            assert np.all(m.amb >= prev)
        prev = m.amb
    assert prev.sum() > 0  # wide enough bounds do reach midpoints
    # the model's value does not depend on eta, and its mass is positive
    assert np.array_equal(bm.mfma_product(kernel, y, x, b, eta=0.0).value, bm.mfma_product(kernel, y, x, b).value)
    assert (bm.mfma_product(kernel, y, x, b).mass > 0).all()


def test_band_is_far_below_the_input_rounding_yardstick():
    """At eta = 1 the band is a small fraction of a row's mass: the model's yardstick is much tighter than 1e-2."""
    rs = np.random.RandomState(3)
    y = rs.rand(500, 64) / 8
    b = rs.randn(500, 4) + 1.0
    for kernel in ("gaussian", "absolute-exponential", "inverse-distance"):
        m = bm.mfma_product(kernel, y, None, b)
        assert not m.flagged.any()
        assert (m.band / m.mass).max() < 2e-3, kernel
