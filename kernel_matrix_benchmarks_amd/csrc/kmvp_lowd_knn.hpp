// Brute-force K nearest neighbours: the arg-K-min reduction over the sources (an extension: no reference method stands
// behind it; include/kmvp.h kmvp_nearest) -- next to the sum (lowd_kernel) and the log-sum-exp (lowd_lse_kernel), and the
// eps -> 0 limit of the latter's soft-min.
//
// lowd_lse_kernel's structure (kmvp_lowd_lse.hpp): lanes = targets, one target per lane, LDS-staged double-buffered source
// records -- the product's own target image and its records in the density layout (no signal columns, R = 4 ceil(D / 4);
// record j IS source j, pads sit at +inf), so the pair loop knows every source's index for free.
//
// The list.  Every lane keeps KT candidates (s, j) in registers, sorted by s and, among equal s, by j; KT is a template
// parameter and every access is unrolled, so nothing is indexed dynamically and nothing goes to scratch.  It starts from
// (+inf, -1).  s is the family's squared distance in the working precision (difference form: one subtraction, one
// square, D - 1 fmas); j is the position within the segment while the loop runs and becomes the GLOBAL index
// j_offset + segment start + position at the store.
//
// Insertion.  A source enters only if s < s_list[KT - 1], STRICTLY, and takes its place behind every entry with s_list <= s.
// Sources are walked in ascending index, so ties resolve towards the smaller index with no extra work.  A batch of U = 4
// sources is compared with the lane's bound first; the insertion code runs under a wave-uniform __any(...), which
// becomes rare once the near sources have been seen (with a full list at position p of the segment a batch triggers with
// probability ~ 1 - (1 - KT / p)^256: every segment starts from an empty list, so short segments are expensive here).
// The insertion itself is one unrolled pass: entry t becomes the old entry t - 1 where s is below that one, s where it is
// below the old entry t only, and stays otherwise.  KT = 1 (k-means assignment, Chamfer distance) is nothing but one
// compare and two selects per pair: no list, no batch, no branch.
//
// What never qualifies: pad records (y = +inf: s = +inf), sources with a NaN coordinate (s = NaN) and pairs whose squared
// distance overflows the working precision (s = +inf) all fail the strict compare -- the family's rule that a pair at
// infinite distance contributes nothing.  A NaN target coordinate makes every s of its lane NaN: its list stays empty,
// the lane is marked (x_nan, as lowd_lse_kernel) and its distances are written as NaN; no other lane is touched.
//
// Each (segment, target) leaves its KT pairs as float64 -- the distance widened exactly, the index as a double (exact:
// M_total < 2^53): part[segment][2 KT][n_pad], distances in rows 0 .. KT - 1, indices in rows KT .. 2 KT - 1, coalesced
// over targets.  kmvp_knn_merge.hpp merges the segments.
#pragma once
#include "kmvp_lowd.hpp"

namespace kmvp {

// One candidate (s, j) into the lane's sorted list; a no-op for a lane whose bound it does not beat (and for NaN).
template <int KT, typename real>
__device__ __forceinline__ void knn_insert(real (&sl)[KT], int (&jl)[KT], real s, int j) {
  bool lt[KT];
#pragma unroll
  for (int t = 0; t < KT; ++t) lt[t] = s < sl[t];  // monotone in t: the list is sorted
#pragma unroll
  for (int t = KT - 1; t > 0; --t) {
    sl[t] = lt[t - 1] ? sl[t - 1] : (lt[t] ? s : sl[t]);
    jl[t] = lt[t - 1] ? jl[t - 1] : (lt[t] ? j : jl[t]);
  }
  sl[0] = lt[0] ? s : sl[0];
  jl[0] = lt[0] ? j : jl[0];
}

template <int D, typename real>
__device__ __forceinline__ real knn_sqdist(const real (&x)[D], const real* __restrict__ r) {
  real df = x[0] - r[0];
  real s = df * df;
#pragma unroll
  for (int d = 1; d < D; ++d) {
    df = x[d] - r[d];
    s = fma(df, df, s);
  }
  return s;
}

template <int D, int KT, typename real>
__global__ void __launch_bounds__(BLOCK_THREADS) lowd_knn_kernel(const LowdArgs<real> a) {
  constexpr int R = RecLayout<D, 1, SIG_DENSITY>::R;
  constexpr int U = 4;  // sources per batch; segments start on batch boundaries

  int tb, seg;
  block_to_work((int)blockIdx.x, a.segments, a.tile_blocks, tb, seg);
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t i0 = ((int64_t)tb * WAVES_PER_BLOCK + wave) * 64;  // first target of this wave's tile
  const int64_t i = i0 + lane;                                     // < n_pad by construction; pad targets are 0

  real x[D];
  bool x_nan = false;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    x[d] = a.xs[(int64_t)d * a.n_pad + i];
    x_nan = x_nan || (x[d] != x[d]);
  }

  const int64_t seg_begin = (int64_t)seg * a.seg_len;
  int64_t seg_end = seg_begin + a.seg_len;
  if (seg_end > a.m_pad) seg_end = a.m_pad;

  real sl[KT];
  int jl[KT];  // position within the segment (the host keeps seg_len below 2^31)
#pragma unroll
  for (int t = 0; t < KT; ++t) {
    sl[t] = (real)INFINITY;
    jl[t] = -1;
  }

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
    const int pos0 = (int)(tile * LDS_TILE);  // position of the tile's first record within the segment
    const real* lrec = reinterpret_cast<const real*>(&lds_raw[buf][0]);
    if constexpr (KT == 1) {
      for (int jj = 0; jj < cnt; jj += U) {
#pragma unroll
        for (int k = 0; k < U; ++k) {
          const real s = knn_sqdist<D, real>(x, lrec + (jj + k) * R);
          const bool lt = s < sl[0];
          sl[0] = lt ? s : sl[0];
          jl[0] = lt ? pos0 + jj + k : jl[0];
        }
      }
    } else {
      for (int jj = 0; jj < cnt; jj += U) {
        real s[U];
#pragma unroll
        for (int k = 0; k < U; ++k) s[k] = knn_sqdist<D, real>(x, lrec + (jj + k) * R);
        // the batch's smallest distance (min drops NaN) against the lane's bound
        const real bmin = fmin(fmin(s[0], s[1]), fmin(s[2], s[3]));
        if (__any(bmin < sl[KT - 1])) {  // wave-uniform; rare once the near sources have been seen
#pragma unroll
          for (int k = 0; k < U; ++k) knn_insert<KT, real>(sl, jl, s[k], pos0 + jj + k);
        }
      }
    }
  }

  // ---- KT float64 (distance, global index) pairs per (segment, target); coalesced over targets
  double* part = a.part + (int64_t)seg * 2 * KT * a.n_pad + i;
#pragma unroll
  for (int t = 0; t < KT; ++t) {
    part[(int64_t)t * a.n_pad] = x_nan ? __builtin_nan("") : (double)sl[t];
    part[(int64_t)(KT + t) * a.n_pad] = jl[t] < 0 ? -1.0 : (double)(a.j_offset + seg_begin + jl[t]);
  }
}

}  // namespace kmvp
