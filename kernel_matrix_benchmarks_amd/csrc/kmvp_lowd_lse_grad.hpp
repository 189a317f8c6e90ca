// Gradient of the log-sum-exp reduction with respect to the target points (an extension: no reference method stands
// behind it; include/kmvp.h kmvp_<kernel>_logsumexp_grad):
//   G[i, e, :] = grad_{x_i} L[i, e] = sum_j p_ij^e g(x_i, y_j),   p_ij^e = exp(l_ij + c[j, e]) / sum_j' exp(l_ij' + c[j', e])
//   gaussian l = -|x - y|^2:  g = -2 (x - y)          absexp l = -|x - y|:  g = -(x - y) / r,  r = |x - y|
// a softmax-weighted sum: a vector numerator and a scalar denominator on ONE online shift, in one pass.
//
// lowd_lse_kernel's structure (kmvp_lowd_lse.hpp) with lowd_grad_kernel's E D accumulators (kmvp_lowd_grad.hpp): lanes =
// targets, one target per lane, LDS-staged double-buffered source records -- the SAME records and target image the
// product packs (LAYOUT_LOWD), so a product, a gradient, a log-sum-exp and this gradient on one context pack once.
//
// Per column every lane keeps the integer shift m of lowd_lse_kernel (log2 units, moved per batch of U sources behind the
// wave-uniform __any(rise) branch) and D + 1 sums at the common scale 2^m:
//   Z = sum 2^(u - m)        V[d] = sum 2^(u - m) (x_d - y_d)        (exp(-r): ... (x_d - y_d) / r)
// fp32 inside a chunk, folded into fp64 between chunks.  A rise multiplies all D + 1 fp32 and fp64 sums of the column by
// 2^(m - m') with ldexp: exact, so the result depends on the order of the additions only, which is fixed.  The constant
// (-2 / -1) is applied once, by the finish kernel (kmvp_product.hip), to V / Z.
//
// The differences x - y of a batch are KEPT across the max step (U D registers), not recomputed after it: the compiler's
// account (LAB_NOTES.md section 16) has no variant in scratch at four sources per batch -- the widest, D = 8, E = 4, hold
// part of their sums in accumulation registers -- and keeping them saves D subtractions per pair.
//
// Terms that must contribute exactly 0 to Z and to V: c = -inf, pairs whose squared distance overflowed, pad records.
// All have u = -inf and so the weight 2^-inf = 0 (m starts from lowd_lse_kernel's finite sentinel).  For the first two
// x - y is finite and 0 (x - y) = 0.  A pad record has x - y = -inf and 0 * -inf is NaN: pad records only exist among the
// last 2 U records of the array, and only the batches that reach into them zero x - y of the records from a.m on (GUARD,
// as lowd_grad_kernel's: by the record's INDEX, not by s < inf -- that select also took a real source with an infinite
// coordinate for a pad record, so the components include/kmvp.h calls NaN came out finite when, and only when, the
// source stood among the last 8 records).
// exp(-r) at s = 0 (not differentiable: 0 is the symmetric subgradient, and the own pair of same_points must drop out):
// 1 / r comes from rsq(s) kept for the positive NORMAL s only (lowd_grad_kernel's select), so a coincident pair adds 0
// to V and keeps its weight in Z.  The logit itself is lse_neg_logit's: L and G see the same weights.
// A NaN target coordinate: the lane is marked once and all its sums are NaN at the store, as lowd_lse_kernel.
// c = NaN or +inf: the weight of that pair is NaN (float64: by lse_exp2_neg's select on m - u), so Z and with it all
// D components of that column are NaN; the other columns are untouched.
//
// Each (segment, column, target) leaves the D + 1 fp64 sums and ONE exponent -m in the `kexp` convention (+inf: no live
// source; Z is 0 exactly then), in the partial-sum array as [segment][(D + 2) NC][n_pad]: sum k of column c in row
// k NC + c (k = 0: Z, k = 1 + d: V[d]), the exponents in rows (D + 1) NC + c.
#pragma once
#include "kmvp_lowd_grad.hpp"
#include "kmvp_lowd_lse.hpp"

namespace kmvp {

// 1 / r for the direction (x - y) / r of exp(-r): kval<K_INVDIST>'s 1 / sqrt(s), 0 where s is not a positive normal number
template <typename real>
__device__ __forceinline__ real lse_grad_rinv(real s, const double* __restrict__ tab) {
  const real q = kval<K_INVDIST>(s, tab);
  return positive_normal(s) ? q : (real)0;
}

// One batch of U sources against the lane's target: logits, the shift's move, the D + 1 sums per column.  GUARD: the
// batch's records from n_real on are pad records.
template <int KERNEL, int D, int E, int SIG, int U, bool GUARD, typename real>
__device__ __forceinline__ void lse_grad_batch_step(const real (&x)[D], const real* __restrict__ rec, int n_real,
                                                    real (&m)[LseLayout<E, SIG>::NC],
                                                    real (&acc)[LseLayout<E, SIG>::NC][D + 1],
                                                    double (&accd)[LseLayout<E, SIG>::NC][D + 1],
                                                    const double* __restrict__ tab) {
  constexpr int R = RecLayout<D, E, SIG>::R;
  constexpr int NC = LseLayout<E, SIG>::NC;
  constexpr real LOG2E = (real)1.4426950408889634;
  real df[U][D], u[U][NC];
  real q[KERNEL == K_ABSEXP ? U : 1];
#pragma unroll
  for (int k = 0; k < U; ++k) {
    const real* r = rec + k * R;
    df[k][0] = x[0] - r[0];
    real s = df[k][0] * df[k][0];
#pragma unroll
    for (int d = 1; d < D; ++d) {
      df[k][d] = x[d] - r[d];
      s = fma(df[k][d], df[k][d], s);
    }
    if constexpr (GUARD) {
      // a pad record: its weight is 0 by itself (u = -inf), but 0 * (x - y) = 0 * -inf is NaN -- the differences go to 0
      const bool live = k < n_real;
#pragma unroll
      for (int d = 0; d < D; ++d) df[k][d] = live ? df[k][d] : (real)0;
    }
    const real nl = lse_neg_logit<KERNEL>(s);
    if constexpr (KERNEL == K_ABSEXP) q[k] = lse_grad_rinv(s, tab);
    if constexpr (SIG == SIG_DENSITY) {
      u[k][0] = nl * -LOG2E;
    } else {
#pragma unroll
      for (int e = 0; e < E; ++e) u[k][e] = (r[D + e] - nl) * LOG2E;
    }
  }
  // the batch's largest logit per column (max drops NaN and never prefers -inf) against the running shift
  real bmax[NC];
  bool rise = false;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    bmax[c] = u[0][c];
#pragma unroll
    for (int k = 1; k < U; ++k) bmax[c] = fmax(bmax[c], u[k][c]);
    rise = rise || (bmax[c] > m[c]);
  }
  if (__any(rise)) {  // wave-uniform; rare once the nearest sources have been seen
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if (bmax[c] > m[c]) {
        const real m_new = ceil(bmax[c]);
        const real down = m[c] - m_new;  // <= 0, integer valued (-inf for a logit of +inf)
#pragma unroll
        for (int k = 0; k <= D; ++k) {
          acc[c][k] = lse_scale(acc[c][k], down);
          if constexpr (sizeof(real) == 4) accd[c][k] = lse_scale(accd[c][k], down);
        }
        m[c] = m_new;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < U; ++k)
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const real a = m[c] - u[k][c];
      // c = NaN, or c = +inf (m = +inf, a = inf - inf): the column must not come out finite -- lse_exp2_neg passes the NaN on
      const real w = lse_exp2_neg(a, tab);
      acc[c][0] += w;
      real wq = w;
      if constexpr (KERNEL == K_ABSEXP) wq = w * q[k];
#pragma unroll
      for (int d = 0; d < D; ++d) acc[c][1 + d] = fma(wq, df[k][d], acc[c][1 + d]);
    }
}

template <int KERNEL, int D, int E, int SIG, typename real>
__global__ void __launch_bounds__(BLOCK_THREADS) lowd_lse_grad_kernel(const LowdArgs<real> a) {
  constexpr int R = RecLayout<D, E, SIG>::R;
  constexpr int NC = LseLayout<E, SIG>::NC;
  constexpr int U = 4;          // sources per batch; segments start on batch boundaries
  constexpr int PAD_BATCH = 8;  // the record array is rounded up to two batches (kmvp_product.hip LOWD_BATCH)
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
  bool x_nan = false;  // (the float64 exp clamps its argument with a min, which drops NaN: the row is marked here)
#pragma unroll
  for (int d = 0; d < D; ++d) {
    x[d] = a.xs[(int64_t)d * a.n_pad + i];
    x_nan = x_nan || (x[d] != x[d]);
  }
  // pad records sit among the last PAD_BATCH records of the array
  const int64_t pad_from = a.m_pad - PAD_BATCH;

  const int64_t seg_begin = (int64_t)seg * a.seg_len;
  int64_t seg_end = seg_begin + a.seg_len;
  if (seg_end > a.m_pad) seg_end = a.m_pad;

  double accd[NC][D + 1];
  real acc[NC][D + 1], m[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
#pragma unroll
    for (int k = 0; k <= D; ++k) {
      accd[c][k] = 0.0;
      acc[c][k] = 0;
    }
    m[c] = lse_sentinel<real>();
  }
  auto fold = [&]() {
    if constexpr (F32) {
#pragma unroll
      for (int c = 0; c < NC; ++c)
#pragma unroll
        for (int k = 0; k <= D; ++k) {
          accd[c][k] += (double)acc[c][k];
          acc[c][k] = 0;
        }
    }
  };

  // ---- LDS-staged tiles, as lowd_lse_kernel: coalesced 16-byte loads of LDS_TILE records per block, double buffered
  // (one barrier per tile), broadcast reads in the pair loop.
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
    // two loops, not one with a branch per batch: the batches of this tile before the pad region, then the guarded ones
    int cnt_plain = cnt;
    if (jt + cnt > pad_from) cnt_plain = jt < pad_from ? (int)(pad_from - jt) : 0;
    int jj = 0;
    for (; jj < cnt_plain; jj += U)
      lse_grad_batch_step<KERNEL, D, E, SIG, U, false, real>(x, lrec + jj * R, U, m, acc, accd, exp_tab);
    for (; jj < cnt; jj += U) {
      const int64_t left = a.m - (jt + jj);  // real records from this batch's first on
      const int n_real = left < 0 ? 0 : left < U ? (int)left : U;
      lse_grad_batch_step<KERNEL, D, E, SIG, U, true, real>(x, lrec + jj * R, n_real, m, acc, accd, exp_tab);
    }
    since_fold += LDS_TILE;
    if (since_fold >= a.chunk) {
      fold();
      since_fold = 0;
    }
  }
  fold();

  // ---- D + 1 fp64 sums and one exponent per (segment, column, target); coalesced over targets
  constexpr int ROWS = (D + 2) * NC;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    double z = 0.0;
#pragma unroll
    for (int k = 0; k <= D; ++k) {
      double v;
      if constexpr (F32) v = accd[c][k];
      else v = (double)acc[c][k];
      if (x_nan) v = __builtin_nan("");
      if (k == 0) z = v;
      a.part[((int64_t)seg * ROWS + k * NC + c) * a.n_pad + i] = v;
    }
    a.part[((int64_t)seg * ROWS + (D + 1) * NC + c) * a.n_pad + i] = (z == 0.0) ? (double)INFINITY : -(double)m[c];
  }
}

}  // namespace kmvp
