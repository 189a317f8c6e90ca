// Batched clouds (include/kmvp.h kmvp_set_batches): the block-diagonal product a[i, e] = sum_{j in batch(i)} k(x_i, y_j) b[j, e]
// and the K nearest sources of every target within its own batch, on the layout of kmvp_batch_plan.hpp.
//
// lowd_kernel's scalar-cache feed (kmvp_lowd.hpp, FEED 0) with one change: the source range is the WAVE's, read from its
// tile entry, not the workgroup's segment.  Lanes are targets, one per lane; every tile holds targets of one batch only;
// the wave walks its batch's records through two SGPR batches of U = 4 records in ping-pong.  The tile entry's address
// depends on blockIdx and the wave's number alone (made wave-uniform with readfirstlane), so the entry and every record
// arrive through the scalar data cache, as in lowd_kernel.  The four waves of a workgroup run loops of different lengths:
// nothing inside the loop synchronises the workgroup -- the float64 table of kexp_neg_f64 is filled, and its one
// barrier passed, before the loop.
//
// The pair arithmetic is lowd_kernel's own: interact<..., T = 1, CHECK_DIAG = false> and kval (product), knn_sqdist and
// knn_insert (nearest).  float32 sums fold into fp64 every `chunk` sources (a multiple of 8), float64 keeps one chain.
// There are no segments, hence no partial results and no merge: a lane writes its fp64 row straight to (N, E) in the
// caller's order (normalised rows divide by the lane's own denominator first), or its sorted list into the candidate
// layout [2 Kc][N] that knn_finish_kernel reads.
//
// Reads past a range.  The prefetch of the loop's last round reads the U records behind the range: the next batch's first
// records, or the spare batch at the array's end behind the last one (kmvp_batch_plan.hpp); they are never consumed.  A
// tile with an empty range (an empty batch; the filler tiles, at record 0) still issues the first prefetch of U records
// from its range's start, inside the array for the same reason, and consumes nothing.
#pragma once
#include "kmvp_batch_plan.hpp"
#include "kmvp_lowd_knn.hpp"

namespace kmvp {

template <typename real>
struct LowdBatchArgs {
  const real* xs;          // targets, SoA over the padded slots: xs[d * n_pad + slot]
  const real* rec;         // source records [m_alloc][R]
  const BatchTile* tiles;  // [n_pad / 64]
  double* out;             // product: (N, E) row-major; nearest: candidates [2 Kc][N]
  int64_t n_pad;           // target slots
  int64_t n;               // targets
  int chunk;               // sources per fp32 chunk, a multiple of 8
  int kc;                  // nearest: candidates stored per target (<= KT)
};

// The wave's tile entry through the scalar cache: the wave's number is uniform by construction, which readfirstlane tells
// the compiler.
__device__ __forceinline__ BatchTile batch_tile_of_wave(const BatchTile* __restrict__ tiles, int64_t& slot0) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t tile = (int64_t)blockIdx.x * WAVES_PER_BLOCK + wave;
  slot0 = tile * BATCH_TILE;
  return tiles[tile];
}

template <int KERNEL, int D, int E, int SIG, typename real>
__global__ void __launch_bounds__(BLOCK_THREADS) lowd_batch_kernel(const LowdBatchArgs<real> a) {
  using L = RecLayout<D, E, SIG>;
  constexpr int R = L::R;
  constexpr int NE = L::NE;
  constexpr int U = 4;  // records per SGPR batch; ranges hold a whole number of 2 U
  constexpr bool F32 = sizeof(real) == 4;
  static_assert(2 * U == BATCH_RECORDS, "two ping-pong batches per round");

  // fp64 only: table 2^(j/64) of kexp_neg_f64 -- the workgroup's only barrier, before any wave enters its loop
  __shared__ double exp_tab_lds[F32 ? 1 : 64];
  const double* exp_tab = exp_tab_lds;
  if constexpr (!F32) {
    if (threadIdx.x < 64) exp_tab_lds[threadIdx.x] = exp2((double)threadIdx.x * (1.0 / 64.0));
    __syncthreads();
  }

  const int lane = threadIdx.x & 63;
  int64_t slot0;
  const BatchTile t = batch_tile_of_wave(a.tiles, slot0);

  real x[1][D];
#pragma unroll
  for (int d = 0; d < D; ++d) x[0][d] = a.xs[(int64_t)d * a.n_pad + slot0 + lane];  // < n_pad by construction; pads are 0
  const int64_t jz[1] = {-1};  // (interact's zero-column rule: CHECK_DIAG is off)

  double accd[NE];
  real acc[1][NE];
#pragma unroll
  for (int e = 0; e < NE; ++e) {
    accd[e] = 0.0;
    acc[0][e] = 0;
  }
  auto fold = [&]() {
    if constexpr (F32) {
#pragma unroll
      for (int e = 0; e < NE; ++e) {
        accd[e] += (double)acc[0][e];
        acc[0][e] = 0;
      }
    }
  };

  const real* __restrict__ segp = a.rec + t.rec0 * R;
  const int seg_n = t.len;
  auto run_batch = [&](const real (&rb)[U * R]) {
#pragma unroll
    for (int u = 0; u < U; ++u) interact<KERNEL, D, E, SIG, 1, false, real>(x, acc, rb + u * R, jz, 0, exp_tab);
  };
  real ra[U * R], rb[U * R];
#pragma unroll
  for (int q = 0; q < U * R; ++q) ra[q] = segp[q];
  for (int c0 = 0; c0 < seg_n; c0 += a.chunk) {
    const int c1 = min(c0 + a.chunk, seg_n);
    for (int j = c0; j < c1; j += 2 * U) {
      const real* __restrict__ pb = segp + (int64_t)(j + U) * R;
#pragma unroll
      for (int q = 0; q < U * R; ++q) rb[q] = pb[q];
      run_batch(ra);
      const real* __restrict__ pa = segp + (int64_t)(j + 2 * U) * R;
#pragma unroll
      for (int q = 0; q < U * R; ++q) ra[q] = pa[q];
      run_batch(rb);
    }
    fold();
  }

  // ---- the lane's fp64 row, in the caller's order.  An empty range is the plain entry's M = 0: zeros (0 / 0 = NaN when
  // normalised), also for a NaN target; otherwise a NaN target coordinate gives a NaN row (nan_target).
  if (lane < t.live) {
    bool x_nan = false;
#pragma unroll
    for (int d = 0; d < D; ++d) x_nan |= x[0][d] != x[0][d];
    x_nan = x_nan && seg_n > 0;
    double v[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      if constexpr (F32) v[e] = accd[e];
      else v[e] = (double)acc[0][e];
      v[e] = nan_target(x_nan, v[e]);
    }
    constexpr int EO = SIG == SIG_DENSITY ? 1 : E;  // columns of the result
    double* __restrict__ row = a.out + (t.i0 + lane) * EO;
#pragma unroll
    for (int e = 0; e < EO; ++e) {
      if constexpr (SIG == SIG_NORM) row[e] = v[e] / v[E];
      else row[e] = v[e];
    }
  }
}

template <int D, int KT, typename real>
__global__ void __launch_bounds__(BLOCK_THREADS) lowd_batch_knn_kernel(const LowdBatchArgs<real> a) {
  constexpr int R = RecLayout<D, 1, SIG_DENSITY>::R;
  constexpr int U = 4;
  static_assert(2 * U == BATCH_RECORDS, "two ping-pong batches per round");

  const int lane = threadIdx.x & 63;
  int64_t slot0;
  const BatchTile t = batch_tile_of_wave(a.tiles, slot0);

  real x[D];
  bool x_nan = false;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    x[d] = a.xs[(int64_t)d * a.n_pad + slot0 + lane];
    x_nan = x_nan || (x[d] != x[d]);
  }

  real sl[KT];
  int jl[KT];  // position within the range (the plan keeps a range below 2^31 records)
#pragma unroll
  for (int k = 0; k < KT; ++k) {
    sl[k] = (real)INFINITY;
    jl[k] = -1;
  }

  const real* __restrict__ segp = a.rec + t.rec0 * R;
  const int seg_n = t.len;
  auto run_batch = [&](const real (&rb)[U * R], int j) {
    if constexpr (KT == 1) {  // one compare and two selects per pair: no list, no branch
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const real s = knn_sqdist<D, real>(x, rb + u * R);
        const bool lt = s < sl[0];
        sl[0] = lt ? s : sl[0];
        jl[0] = lt ? j + u : jl[0];
      }
    } else {
      real s[U];
#pragma unroll
      for (int u = 0; u < U; ++u) s[u] = knn_sqdist<D, real>(x, rb + u * R);
      // the batch's smallest distance (min drops NaN) against the lane's bound
      const real bmin = fmin(fmin(s[0], s[1]), fmin(s[2], s[3]));
      if (__any(bmin < sl[KT - 1])) {  // wave-uniform; rare once the near sources have been seen
#pragma unroll
        for (int u = 0; u < U; ++u) knn_insert<KT, real>(sl, jl, s[u], j + u);
      }
    }
  };
  real ra[U * R], rb[U * R];
#pragma unroll
  for (int q = 0; q < U * R; ++q) ra[q] = segp[q];
  for (int j = 0; j < seg_n; j += 2 * U) {
    const real* __restrict__ pb = segp + (int64_t)(j + U) * R;
#pragma unroll
    for (int q = 0; q < U * R; ++q) rb[q] = pb[q];
    run_batch(ra, j);
    const real* __restrict__ pa = segp + (int64_t)(j + 2 * U) * R;
#pragma unroll
    for (int q = 0; q < U * R; ++q) ra[q] = pa[q];
    run_batch(rb, j + U);
  }

  // ---- the first kc (distance, global index) pairs of the lane's list as float64, [2 kc][N] in the caller's order.  An
  // empty range is the plain entry's M = 0: an empty list, also for a NaN target.
  if (lane < t.live) {
    const bool nan_row = x_nan && seg_n > 0;
    double* __restrict__ cand = a.out + t.i0 + lane;
#pragma unroll
    for (int k = 0; k < KT; ++k) {
      if (k < a.kc) {
        cand[(int64_t)k * a.n] = nan_row ? __builtin_nan("") : (double)sl[k];
        cand[(int64_t)(a.kc + k) * a.n] = jl[k] < 0 ? -1.0 : (double)(t.j0 + jl[k]);
      }
    }
  }
}

// kmvp_lowd_batch_inst.hip, one unit per precision: the Gaussian, exp(-r) and the Matern kernels, D <= 8, E <= 4 in the
// three signal modes; list capacities KT = 1, 4, 16.  hipErrorInvalidValue where nothing is instantiated.
hipError_t launch_lowd_batch_f32(int kernel, int D, int E, int sig, const LowdBatchArgs<float>& args, dim3 grid, hipStream_t stream,
                                 const char** kernel_name);
hipError_t launch_lowd_batch_f64(int kernel, int D, int E, int sig, const LowdBatchArgs<double>& args, dim3 grid, hipStream_t stream,
                                 const char** kernel_name);
hipError_t launch_lowd_batch_knn_f32(int D, int KT, const LowdBatchArgs<float>& args, dim3 grid, hipStream_t stream,
                                     const char** kernel_name);
hipError_t launch_lowd_batch_knn_f64(int D, int KT, const LowdBatchArgs<double>& args, dim3 grid, hipStream_t stream,
                                     const char** kernel_name);

// targets (N, D) row-major -> SoA over the padded slots through the plan's map; pads are 0
template <typename real>
__global__ void batch_pack_targets_kernel(const real* __restrict__ x, const int64_t* __restrict__ tmap, real* __restrict__ xs,
                                          int64_t n_pad, int D) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_pad) return;
  const int64_t i = tmap[s];
  for (int d = 0; d < D; ++d) xs[(int64_t)d * n_pad + s] = i >= 0 ? x[i * D + d] : (real)0;
}

// sources (M, D) -> the coordinates of the records [m_alloc][R] through the plan's map, every other slot 0; pad records
// have y = +inf so that every kernel evaluates to exactly 0 for them
template <typename real>
__global__ void batch_pack_sources_kernel(const real* __restrict__ y, const int64_t* __restrict__ smap, real* __restrict__ rec,
                                          int64_t m_alloc, int D, int R) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= m_alloc) return;
  const int64_t j = smap[s];
  real* r = rec + s * R;
  for (int d = 0; d < D; ++d) r[d] = j >= 0 ? y[j * D + d] : (real)INFINITY;
  for (int q = D; q < R; ++q) r[q] = (real)0;
}

// signal (M, EB) -> the signal slots of the records, nothing else; pad records keep b = 0
template <typename real>
__global__ void batch_pack_signal_kernel(const real* __restrict__ b, const int64_t* __restrict__ smap, real* __restrict__ rec,
                                         int64_t m_alloc, int D, int EB, int R) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= m_alloc) return;
  const int64_t j = smap[s];
  real* r = rec + s * R;
  for (int e = 0; e < EB; ++e) r[D + e] = j >= 0 ? b[j * EB + e] : (real)0;
}

}  // namespace kmvp
