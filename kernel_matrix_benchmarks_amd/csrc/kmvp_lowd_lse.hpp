// Log-sum-exp reduction of the Gaussian and exp(-r) kernels (an extension: no reference method stands behind it;
// include/kmvp.h kmvp_<kernel>_logsumexp):
//   L[i, e] = log sum_j exp( l(x_i, y_j) + c[j, e] ),   gaussian l = -|x - y|^2,   absexp l = -|x - y|
// with the signal read as log-weights c (density mode: c = 0, one column).
//
// lowd_grad_kernel's structure (kmvp_lowd_grad.hpp) with one variant per (D, E): lanes = targets, one target per lane,
// LDS-staged double-buffered source records -- the SAME records and target image the product packs (LAYOUT_LOWD), so a
// product, a gradient and a log-sum-exp on one context pack once.  What is new is the online shift of the pair loop.
//
// The shift.  Logits are taken in log2 units, u = log2(e) (l + c).  Every lane keeps, per column, an INTEGER shift m (held
// in the working precision) and sums 2^(u - m) <= 1: fp32 inside a chunk, folded into fp64 between chunks, as the
// product.  m is updated per batch of U sources, not per pair: the batch's largest u is compared with m, and only when it
// is larger on some lane of the wave (a wave-uniform branch: after the first tiles the running maximum rarely rises) does
// that lane move to m' = ceil(max u) and multiply both its fp32 and its fp64 sum by 2^(m - m') -- v_ldexp: an exact
// power of two, so the result does not depend on where the rescales happen to fall beyond the order of the additions,
// which is fixed.  Nothing ever forms exp(max logit).
//
// Terms that must contribute exactly 0: pad records (y = +inf), pairs whose squared distance overflowed, c = -inf.  All
// of them have u = -inf, and m starts from a FINITE sentinel below every logit the format can hold, so u - m = -inf and
// 2^-inf = 0; -inf never meets -inf.  max() drops them (and NaN) from the comparison with m.  A NaN target coordinate
// makes every u of its lane NaN and its m stays at the sentinel; the lane is marked once and its sums are set to NaN in
// every column at the store (float64's exp clamps its argument with a min, which would drop the NaN); no other lane is touched.
//
// Each (segment, column, target) leaves the fp64 sum and the exponent -m in fastmm_kernel's `kexp` convention (sums at the
// scale 2^-kexp, +inf: no live source), the exponents as fp64 in the columns NC .. 2 NC - 1 of the partial-sum array:
// a sum is 0 exactly when the segment had no live term (the largest live term is in (1/2, 1] at the final m).
#pragma once
#include "kmvp_lowd.hpp"

namespace kmvp {

template <int E, int SIG>
struct LseLayout {
  static constexpr int NC = (SIG == SIG_DENSITY) ? 1 : E;  // columns of the result
};

// the shift's start: finite, below every logit that counts (a logit at or below it is taken as -inf)
template <typename real>
__device__ __forceinline__ constexpr real lse_sentinel() {
  return sizeof(real) == 4 ? (real)-3.0e38 : (real)-1.0e299;
}

// -l(x, y) from the squared distance: s (gaussian), r = sqrt(s) (exp(-r)).  float32: v_sqrt_f32 as kval<K_ABSEXP>;
// float64: kval<K_ABSEXP>'s r = s rsq(s) with its one correction step, s = 0 and s = inf (rsq = inf / 0: 0 * inf) passed
// through by the same select
template <int KERNEL>
__device__ __forceinline__ float lse_neg_logit(float s) {
  if constexpr (KERNEL == K_GAUSSIAN) return s;
  else return __builtin_amdgcn_sqrtf(s);
}
template <int KERNEL>
__device__ __forceinline__ double lse_neg_logit(double s) {
  if constexpr (KERNEL == K_GAUSSIAN) {
    return s;
  } else {
    const double y0 = __builtin_amdgcn_rsq(s);
    const double e = fma(-s * y0, y0, 1.0);
    const double r = s * fma(y0 * e, fma(e, 0.375, 0.5), y0);
    return (s == 0.0 || s == (double)INFINITY) ? s : r;
  }
}

// 2^-a for a >= 0 (a = m - u; +inf and anything beyond the format's range give exactly 0; NaN stays NaN).  a is NaN for a
// log-weight of NaN, and for one of +inf (m = +inf, inf - inf): v_exp_f32 passes it on, so the column's sum is NaN and
// the column not finite, as include/kmvp.h says.  kexp_neg_f64 clamps its argument with a min, which returns its OTHER
// argument for a NaN: the weight came out exactly 0 and the column finite (c = +inf: finite wherever another segment had
// a live term) -- hence the select, which changes no result of a finite a.
__device__ __forceinline__ float lse_exp2_neg(float a, const double*) { return kexp2(-a); }
__device__ __forceinline__ double lse_exp2_neg(double a, const double* __restrict__ tab) {
  const double w = kexp_neg_f64(a * 0.6931471805599453, tab);
  return (a == a) ? w : a;
}

// x 2^d for an integer-valued d <= 0 held in floating point (-inf allowed): exact
__device__ __forceinline__ float lse_scale(float v, float d) { return ldexpf(v, (int)fmaxf(d, -300.0f)); }
__device__ __forceinline__ double lse_scale(double v, float d) { return ldexp(v, (int)fmaxf(d, -300.0f)); }
__device__ __forceinline__ double lse_scale(double v, double d) { return ldexp(v, (int)fmax(d, -4000.0)); }

// The finished value from a sum at the scale 2^-k and its exponent k (the `kexp` convention above; k = -m):
// (log2(sum) - k) ln 2, and exactly -inf for k = +inf (no live term).  finish_lse_kernel and lowd_batch_lse_kernel.
__device__ __forceinline__ double lse_value(double sum, double k) {
  return (k < 1.0e300) ? (log2(sum) - k) * 0.6931471805599453 : -(double)INFINITY;
}

// The logits u[e] of one (target, source) pair, in log2 units.
template <int KERNEL, int D, int E, int SIG, typename real>
__device__ __forceinline__ void lse_logits(const real (&x)[D], const real* __restrict__ r,
                                           real (&u)[LseLayout<E, SIG>::NC]) {
  constexpr real LOG2E = (real)1.4426950408889634;
  real df = x[0] - r[0];
  real s = df * df;
#pragma unroll
  for (int d = 1; d < D; ++d) {
    df = x[d] - r[d];
    s = fma(df, df, s);
  }
  const real nl = lse_neg_logit<KERNEL>(s);
  if constexpr (SIG == SIG_DENSITY) {
    u[0] = nl * -LOG2E;
  } else {
#pragma unroll
    for (int e = 0; e < E; ++e) u[e] = (r[D + e] - nl) * LOG2E;
  }
}

template <int KERNEL, int D, int E, int SIG, typename real>
__global__ void __launch_bounds__(BLOCK_THREADS) lowd_lse_kernel(const LowdArgs<real> a) {
  constexpr int R = RecLayout<D, E, SIG>::R;
  constexpr int NC = LseLayout<E, SIG>::NC;
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
  bool x_nan = false;  // (the float64 exp clamps its argument with a min, which drops NaN: the row is marked here)
#pragma unroll
  for (int d = 0; d < D; ++d) {
    x[d] = a.xs[(int64_t)d * a.n_pad + i];
    x_nan = x_nan || (x[d] != x[d]);
  }

  const int64_t seg_begin = (int64_t)seg * a.seg_len;
  int64_t seg_end = seg_begin + a.seg_len;
  if (seg_end > a.m_pad) seg_end = a.m_pad;

  double accd[NC];
  real acc[NC], m[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    accd[c] = 0.0;
    acc[c] = 0;
    m[c] = lse_sentinel<real>();
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

  // ---- LDS-staged tiles, as lowd_grad_kernel: coalesced 16-byte loads of LDS_TILE records per block, double buffered
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
    for (int jj = 0; jj < cnt; jj += U) {
      real u[U][NC];
#pragma unroll
      for (int k = 0; k < U; ++k) lse_logits<KERNEL, D, E, SIG, real>(x, lrec + (jj + k) * R, u[k]);
      // the batch's largest logit per column (max drops NaN and never prefers -inf) against the running shift
      real bmax[NC];
      bool rise = false;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        bmax[c] = fmax(fmax(u[0][c], u[1][c]), fmax(u[2][c], u[3][c]));
        rise = rise || (bmax[c] > m[c]);
      }
      if (__any(rise)) {  // wave-uniform; rare once the nearest sources have been seen
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          if (bmax[c] > m[c]) {
            const real m_new = ceil(bmax[c]);
            const real down = m[c] - m_new;  // <= 0, integer valued (-inf for a logit of +inf)
            acc[c] = lse_scale(acc[c], down);
            accd[c] = lse_scale(accd[c], down);
            m[c] = m_new;
          }
        }
      }
#pragma unroll
      for (int k = 0; k < U; ++k)
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[c] += lse_exp2_neg(m[c] - u[k][c], exp_tab);
    }
    since_fold += LDS_TILE;
    if (since_fold >= a.chunk) {
      fold();
      since_fold = 0;
    }
  }
  fold();

  // ---- one fp64 (sum, exponent) pair per (segment, column, target); coalesced over targets
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    double v;
    if constexpr (F32) v = accd[c];
    else v = (double)acc[c];
    if (x_nan) v = __builtin_nan("");
    a.part[((int64_t)seg * 2 * NC + c) * a.n_pad + i] = v;
    a.part[((int64_t)seg * 2 * NC + NC + c) * a.n_pad + i] = (v == 0.0) ? (double)INFINITY : -(double)m[c];
  }
}

}  // namespace kmvp
