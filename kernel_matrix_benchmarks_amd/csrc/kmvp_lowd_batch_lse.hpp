// Log-sum-exp over batched clouds: L[i, e] = log sum_{j in batch(i)} exp( l(x_i, y_j) + c[j, e] ), the pair loop of the
// batched Sinkhorn solve (kmvp_sinkhorn_batched.hip; include/kmvp.h kmvp_<kernel>_sinkhorn_batched).
//
// Two kernels that exist meet here and neither is restated:
//  * the FEED is lowd_batch_kernel's (kmvp_lowd_batch.hpp): the wave's BatchTile through batch_tile_of_wave, the records of
//    the wave's own range through the scalar data cache in two SGPR batches of U = 4 in ping-pong, one target per lane, no
//    segments, no barrier inside the loop -- the float64 table of kexp_neg_f64 and its one barrier come first;
//  * the ARITHMETIC is lowd_lse_kernel's (kmvp_lowd_lse.hpp): lse_logits, lse_sentinel, lse_exp2_neg and lse_scale are
//    called as they are; per batch of 4 the largest logit bmax, the wave-uniform __any(rise), the integer shift
//    m' = ceil(bmax) and the rescale of both sums by the exact power of two 2^(m - m').  float32 folds into fp64 every
//    `chunk` sources (batch_args' rule: a multiple of 8), float64 keeps one chain.  A NaN target marks its lane.
//
// No segments, hence no partial sums and no merge: a live lane finishes its own row and writes L as float64 to (N, NC) in
// the caller's order with lse_value, the expression of finish_lse_kernel -- (log2(sum) + m) ln 2, exactly -inf where the sum
// is 0.  An empty range (an empty batch, a retired tile) gives the plain entry's M = 0: -inf, also for a NaN target.
//
// Reads past a range are lowd_batch_kernel's: the last prefetch reads the next batch's first records or the spare batch at
// the array's end and is never consumed; a tile with an empty range still issues the first prefetch from its range's
// start, inside the array.
//
// Freshness of what comes through the scalar cache.  Between launches other kernels rewrite, with ordinary vector stores,
// the records' signal slots and -- the solver retiring a stopped batch -- the `len` field of tile entries.  The next launch
// reads them through the scalar cache, which is as fresh as the dispatch boundary makes it: the reliance
// batch_pack_signal_kernel followed by lowd_batch_kernel already has.  Nothing a wave reads through the scalar cache is
// written within the same launch: this kernel writes `out` only.
#pragma once
#include "kmvp_lowd_batch.hpp"
#include "kmvp_lowd_lse.hpp"

namespace kmvp {

template <typename real>
struct LowdBatchLseArgs {
  const real* xs;          // targets, SoA over the padded slots: xs[d * n_pad + slot]
  const real* rec;         // source records [m_alloc][R], the log-weights c in the signal slots
  const BatchTile* tiles;  // [n_pad / 64]
  double* out;             // (N, NC) row-major, the caller's order
  int64_t n_pad;           // target slots
  int chunk;               // sources per fp32 chunk, a multiple of 8
};

template <int KERNEL, int D, int E, int SIG, typename real>
__global__ void __launch_bounds__(BLOCK_THREADS) lowd_batch_lse_kernel(const LowdBatchLseArgs<real> a) {
  constexpr int R = RecLayout<D, E, SIG>::R;
  constexpr int NC = LseLayout<E, SIG>::NC;
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

  real x[D];
  bool x_nan = false;  // (the float64 exp clamps its argument with a min, which drops NaN: the row is marked here)
#pragma unroll
  for (int d = 0; d < D; ++d) {
    x[d] = a.xs[(int64_t)d * a.n_pad + slot0 + lane];  // < n_pad by construction; pads are 0
    x_nan = x_nan || (x[d] != x[d]);
  }

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

  const real* __restrict__ segp = a.rec + t.rec0 * R;
  const int seg_n = t.len;
  // one batch of U records: lowd_lse_kernel's inner block, the records in SGPRs instead of LDS
  auto run_batch = [&](const real (&rb)[U * R]) {
    real u[U][NC];
#pragma unroll
    for (int k = 0; k < U; ++k) lse_logits<KERNEL, D, E, SIG, real>(x, rb + k * R, u[k]);
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

  // ---- the lane's own row, finished: no other wave holds a share of it
  if (lane < t.live) {
    const bool nan_row = x_nan && seg_n > 0;
    double* __restrict__ row = a.out + (t.i0 + lane) * NC;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      double v;
      if constexpr (F32) v = accd[c];
      else v = (double)acc[c];
      if (nan_row) v = __builtin_nan("");
      row[c] = lse_value(v, (v == 0.0) ? (double)INFINITY : -(double)m[c]);
    }
  }
}

// kmvp_lowd_batch_lse_inst.hip, one unit per precision: the Gaussian and exp(-r), D <= 8, E = 1, SIG_PRODUCT -- what the
// batched Sinkhorn solve uses.  hipErrorInvalidValue where nothing is instantiated.
hipError_t launch_lowd_batch_lse_f32(int kernel, int D, int E, int sig, const LowdBatchLseArgs<float>& args, dim3 grid,
                                     hipStream_t stream, const char** kernel_name);
hipError_t launch_lowd_batch_lse_f64(int kernel, int D, int E, int sig, const LowdBatchLseArgs<double>& args, dim3 grid,
                                     hipStream_t stream, const char** kernel_name);

}  // namespace kmvp
