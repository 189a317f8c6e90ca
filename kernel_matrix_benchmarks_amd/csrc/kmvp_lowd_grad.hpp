// Gradient of the low-dimensional product with respect to the target points (an extension: no reference method
// stands behind it; include/kmvp.h kmvp_<kernel>_grad):
//   G[i, e, :] = sum_j w(s_ij) (x_i - y_j) b[j, e],   s = |x_i - y_j|^2
//   gaussian exp(-s):  w = -2 k        absexp exp(-r):  w = -k / r        invdist 1/r:  w = -1 / r^3
//   Matern nu = 3/2, t = sqrt(3) r:  w = -3 e^{-t}        nu = 5/2, t = sqrt(5) r:  w = -(5/3) (1 + t) e^{-t}
//   (both finite and smooth at r = 0: no convention, no select; the own pair of same_points gives w * 0 = 0 by itself)
//
// lowd_kernel's structure (kmvp_lowd.hpp) with one variant per (D, E): lanes = targets, one target per lane,
// LDS-staged source records -- the SAME records and target image the product packs (LAYOUT_LOWD), so a product and
// a gradient on one context pack once.  Each lane keeps E D sums; fp32 inside a chunk, folded into fp64 between
// chunks; one fp64 partial per (segment, column e D + d, target), summed in index order by reduce_and_finish.
//
// Per pair at E = 1: the 3D-1 operations of s (the differences x - y are kept, not recomputed), the kernel's
// transcendentals -- q = rsq(s) serves 1/r^3 as q q q and exp(-r) as r = s q, w = k q --, one product with the
// signal and D FMAs.  The sign of w and the Gaussian's 2 are applied once per partial sum, not per pair.
//
// Pairs that must contribute exactly 0 although x - y is not finite or w is not:
//  * pad records (y = +inf: the product's k is 0 there, but 0 * (x - y) = 0 * -inf is NaN).  They only exist among
//    the last 2 U records of the array, so only those batches pay for the selects that zero w AND x - y (GUARD).  The
//    select is on the record's INDEX (j >= M), not on s: a source of the caller's is never taken for a pad record, and
//    a NaN squared distance stays NaN, wherever in the array the source sits;
//  * 1/r: the pairs of the reference's flat-index zero rule, in the batches that can hold one (GUARD, as the
//    product's CHECK_DIAG).  A coincident pair that is NOT zeroed gives inf * 0: that row is NaN in every component,
//    exactly the rows where the product is inf;
//  * exp(-r) at s = 0 (not differentiable; 0 is the symmetric subgradient, and the own pair of same_points must
//    vanish): rsq(0) = inf.  One v_cmp_class per pair keeps w for the positive NORMAL s only (x - y is 0 or tiny
//    there; a denormal s, r < 1.1e-19 in float32, is flushed by the hardware's rsq: it counts as coincident).
//
// Non-finite inputs (include/kmvp.h): a NaN target coordinate makes its row NaN in every component and touches no other
// row -- the row is restored when it is written (nan_target, kmvp_lowd.hpp: the clamps of kexp_neg_f64 and of the Matern
// exponents turn a NaN s into w = 0, which would leave the components of the other axes finite).  A source coordinate
// that is NaN or +-inf is NOT screened (it would cost the unguarded pair loop a select): w (x_d - y_d) is 0 * inf or
// NaN in the components of that axis, in every row, the same in a guarded batch as in any other.
#pragma once
#include "kmvp_lowd.hpp"

namespace kmvp {

__device__ __forceinline__ bool positive_normal(float s) { return __builtin_amdgcn_classf(s, 0x100); }
__device__ __forceinline__ bool positive_normal(double s) { return __builtin_amdgcn_class(s, 0x100); }

// |w(s)| without its constant: k (gaussian), q^3 (1/r), k q (exp(-r)), q = 1/sqrt(s) as kval<K_INVDIST> computes it;
// Matern: the polynomial of one degree less than the value's (matern_value, kmvp_lowd.hpp: exactly 0 at s = inf)
template <int KERNEL, typename real>
__device__ __forceinline__ real grad_weight(real s, const double* __restrict__ tab) {
  if constexpr (KERNEL == K_GAUSSIAN) {
    return kval<K_GAUSSIAN>(s, tab);
  } else if constexpr (KERNEL == K_MATERN32) {
    return matern_value<K_MATERN32, 0>(s, tab);
  } else if constexpr (KERNEL == K_MATERN52) {
    return matern_value<K_MATERN52, 1>(s, tab);
  } else {
    const real q = kval<K_INVDIST>(s, tab);
    if constexpr (KERNEL == K_INVDIST) return q * q * q;
    return kval<K_GAUSSIAN>(s * q, tab) * q;  // exp(-r) / r with r = s / sqrt(s)
  }
}
// the constant: applied to the partial sums
template <int KERNEL>
__device__ __forceinline__ constexpr double grad_constant() {
  return KERNEL == K_GAUSSIAN ? -2.0 : KERNEL == K_MATERN32 ? -3.0 : KERNEL == K_MATERN52 ? -5.0 / 3.0 : -1.0;
}

template <int D, int E, int SIG>
struct GradLayout {
  static constexpr int EC = (SIG == SIG_DENSITY) ? 1 : E;  // signal columns of the result
  static constexpr int NC = EC * D;                        // sums per target: column e D + d
};

// One (target, source) interaction.
template <int KERNEL, int D, int E, int SIG, bool GUARD, typename real>
__device__ __forceinline__ void grad_interact(const real (&x)[D], real (&acc)[GradLayout<D, E, SIG>::NC],
                                              const real* __restrict__ r, int64_t jz, int64_t j_local, int64_t m,
                                              const double* __restrict__ tab) {
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
    if constexpr (KERNEL == K_INVDIST) w = (j_local == jz) ? (real)0 : w;
  }
  if constexpr (SIG == SIG_DENSITY) {
#pragma unroll
    for (int d = 0; d < D; ++d) acc[d] = fma(w, df[d], acc[d]);
  } else {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const real wb = w * r[D + e];
#pragma unroll
      for (int d = 0; d < D; ++d) acc[e * D + d] = fma(wb, df[d], acc[e * D + d]);
    }
  }
}

template <int KERNEL, int D, int E, int SIG, typename real>
__global__ void __launch_bounds__(BLOCK_THREADS) lowd_grad_kernel(const LowdArgs<real> a) {
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
  // 1/r: the zero column of this target (bruteforce.py:13-14, as lowd_kernel) and the wave-uniform bounds of the
  // tile's zero columns (conservative when the mod wraps inside the tile: then every batch is guarded)
  int64_t jz = -1, jz_lo = 0, jz_hi = -1;
  if constexpr (KERNEL == K_INVDIST) {
    const int64_t g = i % (a.m_total + 1);
    jz = (g < a.m_total) ? g - a.j_offset : (int64_t)-1;
    const int64_t g_lo = i0 % (a.m_total + 1);
    const int64_t g_hi = g_lo + 63;
    if (g_hi <= a.m_total) {
      jz_lo = g_lo - a.j_offset;
      jz_hi = g_hi - a.j_offset;
    } else {
      jz_lo = INT64_MIN / 2;
      jz_hi = INT64_MAX / 2;
    }
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

  // ---- LDS-staged tiles, as lowd_kernel's FEED 1: coalesced 16-byte loads of LDS_TILE records per block, double
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
      bool guard = j + U > pad_from;
      if constexpr (KERNEL == K_INVDIST) guard = guard || ((j + U - 1 >= jz_lo) && (j <= jz_hi));
      if (guard) {
#pragma unroll
        for (int u = 0; u < U; ++u)
          grad_interact<KERNEL, D, E, SIG, true, real>(x, acc, lrec + (jj + u) * R, jz, j + u, a.m, exp_tab);
      } else {
#pragma unroll
        for (int u = 0; u < U; ++u)
          grad_interact<KERNEL, D, E, SIG, false, real>(x, acc, lrec + (jj + u) * R, jz, j + u, a.m, exp_tab);
      }
    }
    since_fold += LDS_TILE;
    if (since_fold >= a.chunk) {
      fold();
      since_fold = 0;
    }
  }
  fold();

  // ---- one fp64 partial per (segment, column, target); coalesced over targets
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    double v;
    if constexpr (F32) v = accd[c];
    else v = (double)acc[c];
    a.part[((int64_t)seg * NC + c) * a.n_pad + i] = nan_target(x_nan, grad_constant<KERNEL>() * v);
  }
}

}  // namespace kmvp
