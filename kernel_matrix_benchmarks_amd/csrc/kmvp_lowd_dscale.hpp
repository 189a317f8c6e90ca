// Derivative of the low-dimensional product in the logarithm of a per-axis length scale (an extension: no reference
// method stands behind it; include/kmvp.h kmvp_<kernel>_dscale):
//   H[i, e, d] = sum_j h_d(x_i, y_j) b[j, e],   h_d = -w(s_ij) (x_{i,d} - y_{j,d})^2,   s = |x_i - y_j|^2
// with w = k'(r) / r the weight of the gradient (kmvp_lowd_grad.hpp: grad_weight, grad_constant).  h_d is
// d k(x / l, y / l) / d log l_d at l = 1: the length scales are the caller's scaling of the points, one per axis.
// gaussian, exp(-r), Matern 3/2 and 5/2; no 1/r (not a covariance, and its derivative is the kernel itself).
//
// lowd_grad_kernel's structure, statement by statement: lanes = targets, one target per lane, the product's own
// LAYOUT_LOWD target image and source records (product, gradient, log-sum-exp and this pack once), LDS-staged double-
// buffered tiles, batches of U = 4, E D fp32 sums folded into fp64 every chunk, one fp64 partial per (segment, column
// e D + d, target), summed in index order by reduce_and_finish.  The sign flip and the constant are applied once per
// partial sum.
//
// Per pair: s exactly as the gradient forms it (D differences, one product, D - 1 FMAs: the same bits), the kernel's
// transcendentals, then the squares go in as TWO factors:
//   E = 1 and density:  t_d = (w b) df_d,  acc_d += t_d df_d                  (1 + 2 D operations; the gradient: 1 + D)
//   E > 1:              u_d = (w df_d) df_d,  acc_{e,d} += u_d b_e            (2 D + E D; the gradient: E + E D)
// and never as a kept square df_d^2, which would save one operation at E = 1: a pair whose squared distance overflows
// (|x_d - y_d| > 1.8e19 in float32) has w = 0 and df_d^2 = inf, and 0 * inf is NaN, where (0 * df_d) * df_d is the
// exact 0 the convention asks for.  A NaN coordinate still spoils its row through either factor.
//
// Pairs that must contribute exactly 0:
//  * pad records (y = +inf: x - y = -inf is not finite, so both factors would fail).  They only exist among the
//    last 2 U records of the array: only those batches pay for the selects that zero w AND x - y (GUARD).  The select
//    is on the record's index (j >= M), as the gradient's: a source of the caller's is never taken for a pad record;
//  * exp(-r) at s = 0: the true limit (x_d - y_d)^2 / r -> 0, no convention; but rsq(0) = inf, so the select of
//    grad_interact (w for the positive NORMAL s only) is needed all the same.  It also covers s = inf, where
//    r = s rsq(s) = inf * 0 is NaN.
//
// Non-finite inputs: the gradient's rules (kmvp_lowd_grad.hpp, include/kmvp.h) -- a NaN target coordinate makes its row
// NaN in every component (nan_target, when the row is written); a NaN or +-inf source coordinate is not screened and
// makes the components of its axis non-finite in every row, wherever in the array the source sits.
#pragma once
#include "kmvp_lowd_grad.hpp"

namespace kmvp {

// One (target, source) interaction.
template <int KERNEL, int D, int E, int SIG, bool GUARD, typename real>
__device__ __forceinline__ void dscale_interact(const real (&x)[D], real (&acc)[GradLayout<D, E, SIG>::NC],
                                                const real* __restrict__ r, int64_t j_local, int64_t m,
                                                const double* __restrict__ tab) {
  static_assert(KERNEL != K_INVDIST, "no length-scale derivative for 1/r");
  real df[D];
  df[0] = x[0] - r[0];
  real s = df[0] * df[0];
#pragma unroll
  for (int d = 1; d < D; ++d) {
    df[d] = x[d] - r[d];
    s = fma(df[d], df[d], s);
  }
  real w = grad_weight<KERNEL>(s, tab);
  if constexpr (KERNEL == K_ABSEXP) w = positive_normal(s) ? w : (real)0;
  if constexpr (GUARD) {
    // a pad record: w = 0 is not enough, 0 * (x - y) = 0 * -inf is NaN -- the differences go to 0 with it
    const bool pad = j_local >= m;
    w = pad ? (real)0 : w;
#pragma unroll
    for (int d = 0; d < D; ++d) df[d] = pad ? (real)0 : df[d];
  }
  if constexpr (SIG == SIG_DENSITY || E == 1) {
    real wb = w;
    if constexpr (SIG != SIG_DENSITY) wb = w * r[D];
#pragma unroll
    for (int d = 0; d < D; ++d) acc[d] = fma(wb * df[d], df[d], acc[d]);
  } else {
    real u[D];
#pragma unroll
    for (int d = 0; d < D; ++d) u[d] = (w * df[d]) * df[d];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const real b = r[D + e];
#pragma unroll
      for (int d = 0; d < D; ++d) acc[e * D + d] = fma(u[d], b, acc[e * D + d]);
    }
  }
}

template <int KERNEL, int D, int E, int SIG, typename real>
__global__ void __launch_bounds__(BLOCK_THREADS) lowd_dscale_kernel(const LowdArgs<real> a) {
  constexpr int R = RecLayout<D, E, SIG>::R;
  constexpr int NC = GradLayout<D, E, SIG>::NC;
  constexpr int U = 4;  // sources per batch; segments start on batch boundaries
  constexpr bool F32 = sizeof(real) == 4;

  // fp64 only: table 2^(j/64) of kexp_neg_f64
  __shared__ double exp_tab_lds[F32 ? 1 : 64];
  const double* exp_tab = exp_tab_lds;
  if constexpr (!F32) {
    if (threadIdx.x < 64) exp_tab_lds[threadIdx.x] = exp2((double)threadIdx.x * (1.0 / 64.0));
    __syncthreads();
  }

  int tb, seg;
  block_to_work((int)blockIdx.x, a.segments, a.tile_blocks, tb, seg);
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t i0 = ((int64_t)tb * WAVES_PER_BLOCK + wave) * 64;  // first target of this wave's tile
  const int64_t i = i0 + lane;                                     // < n_pad by construction; pad targets are 0

  real x[D];
  bool x_nan = false;  // nan_target (kmvp_lowd.hpp)
#pragma unroll
  for (int d = 0; d < D; ++d) {
    x[d] = a.xs[(int64_t)d * a.n_pad + i];
    x_nan = x_nan || (x[d] != x[d]);
  }
  // pad records: the array is rounded up to two batches, so they sit among its last 2 U records
  const int64_t pad_from = a.m_pad - 2 * U;

  const int64_t seg_begin = (int64_t)seg * a.seg_len;
  int64_t seg_end = seg_begin + a.seg_len;
  if (seg_end > a.m_pad) seg_end = a.m_pad;

  double accd[NC];
  real acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    accd[c] = 0.0;
    acc[c] = 0;
  }
  auto fold = [&]() {
    if constexpr (F32) {
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        accd[c] += (double)acc[c];
        acc[c] = 0;
      }
    }
  };

  // ---- LDS-staged tiles, as lowd_grad_kernel: coalesced 16-byte loads of LDS_TILE records per block, double
  // buffered (one barrier per tile), broadcast reads in the pair loop.
  static_assert((LDS_TILE * R * sizeof(real)) % (16 * BLOCK_THREADS) == 0 ||
                    (LDS_TILE * R * sizeof(real)) < (16 * BLOCK_THREADS),
                "tile must be a whole number of 16-byte pieces per thread");
  constexpr int TILE_BYTES = LDS_TILE * R * (int)sizeof(real);
  constexpr int PIECES = (TILE_BYTES + 16 * BLOCK_THREADS - 1) / (16 * BLOCK_THREADS);
  __shared__ __attribute__((aligned(16))) unsigned char lds_raw[2][TILE_BYTES];
  const int64_t n_tiles = (seg_end - seg_begin + LDS_TILE - 1) / LDS_TILE;
  const unsigned char* gbase = reinterpret_cast<const unsigned char*>(a.rec + seg_begin * R);
  const int64_t seg_bytes = (seg_end - seg_begin) * R * (int64_t)sizeof(real);
  uint4 stage[PIECES];
  auto gload = [&](int64_t tile) {
#pragma unroll
    for (int p = 0; p < PIECES; ++p) {
      const int64_t off = tile * TILE_BYTES + ((int64_t)p * BLOCK_THREADS + threadIdx.x) * 16;
      stage[p] = (off < seg_bytes && (p * BLOCK_THREADS + (int)threadIdx.x) * 16 < TILE_BYTES)
                     ? *reinterpret_cast<const uint4*>(gbase + off)
                     : make_uint4(0, 0, 0, 0);
    }
  };
  gload(0);
  int since_fold = 0;
  for (int64_t tile = 0; tile < n_tiles; ++tile) {
    const int buf = (int)(tile & 1);
#pragma unroll
    for (int p = 0; p < PIECES; ++p) {
      const int o = (p * BLOCK_THREADS + (int)threadIdx.x) * 16;
      if (o < TILE_BYTES) *reinterpret_cast<uint4*>(&lds_raw[buf][o]) = stage[p];
    }
    __syncthreads();
    if (tile + 1 < n_tiles) gload(tile + 1);
    const int64_t jt = seg_begin + tile * LDS_TILE;
    int cnt = LDS_TILE;
    if (jt + cnt > seg_end) cnt = (int)(seg_end - jt);
    const real* lrec = reinterpret_cast<const real*>(&lds_raw[buf][0]);
    for (int jj = 0; jj < cnt; jj += U) {
      const int64_t j = jt + jj;
      if (j + U > pad_from) {
#pragma unroll
        for (int u = 0; u < U; ++u)
          dscale_interact<KERNEL, D, E, SIG, true, real>(x, acc, lrec + (jj + u) * R, j + u, a.m, exp_tab);
      } else {
#pragma unroll
        for (int u = 0; u < U; ++u)
          dscale_interact<KERNEL, D, E, SIG, false, real>(x, acc, lrec + (jj + u) * R, j + u, a.m, exp_tab);
      }
    }
    since_fold += LDS_TILE;
    if (since_fold >= a.chunk) {
      fold();
      since_fold = 0;
    }
  }
  fold();

  // ---- one fp64 partial per (segment, column, target); coalesced over targets.  h_d = -w (x_d - y_d)^2: the sums hold
  // |w| without its constant, and the constant is negative
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    double v;
    if constexpr (F32) v = accd[c];
    else v = (double)acc[c];
    a.part[((int64_t)seg * NC + c) * a.n_pad + i] = nan_target(x_nan, -grad_constant<KERNEL>() * v);
  }
}

}  // namespace kmvp
