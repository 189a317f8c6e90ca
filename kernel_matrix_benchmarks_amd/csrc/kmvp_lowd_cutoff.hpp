// Cutoff-radius products and neighbour counts (include/kmvp.h kmvp_<kernel>_cutoff, kmvp_radius_count) on the cell list of
// kmvp_cutoff_plan.hpp:  a[i, e] = sum_{j : s_ij <= r2} k(s_ij) b[j, e]  and  counts[i] = #{j : s_ij <= r2}.
//
// lowd_batch_kernel's feed (kmvp_lowd_batch.hpp) inside an outer loop over the wave tile's runs.  Lanes are targets, one
// per lane; the tile's entry is read at an address that depends on blockIdx and the wave's number alone (made wave-uniform
// with readfirstlane), so the entry, every run entry and every record arrive through the scalar data cache; a run's
// records come in two SGPR batches of U = 4 in ping-pong.  The four waves of a workgroup walk different runs of different
// lengths: nothing inside the loops synchronises the workgroup -- the float64 table of kexp_neg_f64 is filled, and its one
// barrier passed, before them.
//
// Per pair: s = knn_sqdist (the value kmvp_nearest compares), k = kval<KERNEL>(s), k = s <= r2 ? k : 0, then interact's
// accumulation lines -- cutoff_interact below.  The select also discards a NaN s (a NaN target) and the pad records
// (s = +inf).  float32 sums fold into fp64 every `chunk` walked records and at every run's end; float64 keeps one chain.
// A lane writes its fp64 row to the caller's index, read from tmap; a NaN target coordinate gives a NaN row, count -1.
//
// K_WENDLAND_C2 / K_WENDLAND_C4 (include/kmvp.h kmvp_wendland_<c>_cutoff) take their value from wendland_value below in
// place of kval: polynomials in t = sqrt(s) / R that vanish at t = 1, so the select removes nothing but rounding.  They
// read no exp table, so those instantiations have neither the table nor its barrier.
//
// Reads past a run are the batched kernel's: the first prefetch is U records at the run's start, the loop's last round
// prefetches the U records behind the run -- the next row's first records, or the spare batch at the array's end.  The plan
// keeps rec0 + len + U <= m_alloc for every run (tests/test_host_cutoff_plan.py).  A tile without runs reads no record.
#pragma once
#include "kmvp_cutoff_plan.hpp"
#include "kmvp_lowd_knn.hpp"

namespace kmvp {

constexpr int CUTOFF_MAX_D = 3;

template <typename real>
struct LowdCutoffArgs {
  const real* xs;           // targets, SoA over the padded slots: xs[d * n_pad + slot]
  const real* rec;          // source records [m_alloc][R]
  const CutoffTile* tiles;  // [n_pad / 64]
  const CutoffRun* runs;
  const int64_t* tmap;      // [n_pad] slot -> caller's target index
  double* out;              // product: (N, E) row-major in the caller's order
  int64_t* counts;          // count: N values in the caller's order
  int64_t n_pad;            // target slots
  real r2;                  // (real)(R R)
  int chunk;                // walked records per fp32 chunk, a multiple of 8
  int self_norm;            // density estimation with normalised rows: v / v
  int exclude_self;         // count: a finite target has its own pair subtracted
  real iR2;                 // Wendland kernels: (real)(1 / (R R)), the quotient formed in double; no other kernel reads it
  double gconst;            // lowd_cutoff_grad_kernel (kmvp_lowd_cutoff_grad.hpp): the gradient's constant c, applied once per row
  // lowd_cutoff_knn_kernel (kmvp_lowd_cutoff_knn.hpp) alone reads what follows; it takes exclude_self from above
  const int32_t* smap32;    // [m_alloc] record -> caller's source index, -1 for a pad
  int64_t* knn_idx;         // (N, knn_k) row-major in the caller's order
  double* knn_sqdist;       // (N, knn_k)
  int knn_k;                // entries per row
  int knn_nan_rows;         // a NaN target gets (-1, NaN): set unless there is no source at all
};

__device__ __forceinline__ CutoffTile cutoff_tile_of_wave(const CutoffTile* __restrict__ tiles, int64_t& slot0) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t tile = (int64_t)blockIdx.x * WAVES_PER_BLOCK + wave;
  slot0 = tile * CUTOFF_TILE;
  return tiles[tile];
}

template <int KERNEL>
constexpr bool KERNEL_IS_WENDLAND = KERNEL == K_WENDLAND_C2 || KERNEL == K_WENDLAND_C4;

// Wendland's functions of t = sqrt(s iR2), u = max(1 - t, 0):  C2: u^4 (4 t + 1);  C4: u^6 (35 t^2 + 18 t + 3) / 3.
// t is exp(-r)'s square root in each precision (kval<K_ABSEXP>): v_sqrt_f32, resp. v_rsq_f64 and one step with q = 0 and
// q = inf passed through.  q = inf (a pad record, an overflowed s) gives u = 0 and 0 * inf = NaN, a NaN s a NaN: the caller's
// select on s <= r2 removes both.  Per pair after s, float32: v_mul, v_sqrt, v_sub, v_max, 2 (3) v_mul, 1 (2) v_fma, v_mul.
__device__ __forceinline__ float wendland_sqrt(float q) { return __builtin_amdgcn_sqrtf(q); }
__device__ __forceinline__ double wendland_sqrt(double q) {
  const double y0 = __builtin_amdgcn_rsq(q);
  const double e = fma(-q * y0, y0, 1.0);
  const double r = q * fma(y0 * e, fma(e, 0.375, 0.5), y0);
  return (q == 0.0 || q == (double)INFINITY) ? q : r;
}
template <int KERNEL, typename real>
__device__ __forceinline__ real wendland_value(real s, real iR2) {
  const real q = s * iR2;
  const real t = wendland_sqrt(q);
  const real u = fmax((real)1 - t, (real)0);
  const real u2 = u * u;
  if constexpr (KERNEL == K_WENDLAND_C2) return (u2 * u2) * fma((real)4, t, (real)1);
  else return ((u2 * u2) * u2) * fma(t, fma(t, (real)(35.0 / 3.0), (real)6), (real)1);
}

// One (target, source) pair: interact's arithmetic (kmvp_lowd.hpp) with the inside test between kval and the accumulation.
template <int KERNEL, int D, int E, int SIG, typename real>
__device__ __forceinline__ void cutoff_interact(const real (&x)[D], real (&acc)[RecLayout<D, E, SIG>::NE], const real* __restrict__ r,
                                                real r2, real iR2, const double* __restrict__ tab) {
  const real s = knn_sqdist<D, real>(x, r);
  real k;
  if constexpr (KERNEL_IS_WENDLAND<KERNEL>) k = wendland_value<KERNEL, real>(s, iR2);
  else k = kval<KERNEL>(s, tab);
  k = s <= r2 ? k : (real)0;
  if constexpr (SIG == SIG_DENSITY) {
    acc[0] += k;
  } else {
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = fma(k, r[D + e], acc[e]);
    if constexpr (SIG == SIG_NORM) acc[E] += k;
  }
}

template <int KERNEL, int D, int E, int SIG, typename real>
__global__ void __launch_bounds__(BLOCK_THREADS) lowd_cutoff_kernel(const LowdCutoffArgs<real> a) {
  using L = RecLayout<D, E, SIG>;
  constexpr int R = L::R;
  constexpr int NE = L::NE;
  constexpr int U = 4;  // records per SGPR batch; runs hold a whole number of 2 U
  constexpr bool F32 = sizeof(real) == 4;
  constexpr bool TABLE = !F32 && !KERNEL_IS_WENDLAND<KERNEL>;
  static_assert(2 * U == CUTOFF_RECORDS, "two ping-pong batches per round");

  // fp64 only: table 2^(j/64) of kexp_neg_f64 -- the workgroup's only barrier, before any wave enters its loops
  const double* exp_tab = nullptr;
  if constexpr (TABLE) {
    __shared__ double exp_tab_lds[64];
    if (threadIdx.x < 64) exp_tab_lds[threadIdx.x] = exp2((double)threadIdx.x * (1.0 / 64.0));
    __syncthreads();
    exp_tab = exp_tab_lds;
  }

  const int lane = threadIdx.x & 63;
  int64_t slot0;
  const CutoffTile t = cutoff_tile_of_wave(a.tiles, slot0);

  real x[D];
#pragma unroll
  for (int d = 0; d < D; ++d) x[d] = a.xs[(int64_t)d * a.n_pad + slot0 + lane];  // < n_pad by construction; pads are 0

  double accd[NE];
  real acc[NE];
#pragma unroll
  for (int e = 0; e < NE; ++e) {
    accd[e] = 0.0;
    acc[e] = 0;
  }
  auto fold = [&]() {
    if constexpr (F32) {
#pragma unroll
      for (int e = 0; e < NE; ++e) {
        accd[e] += (double)acc[e];
        acc[e] = 0;
      }
    }
  };
  const real r2 = a.r2;
  const real iR2 = a.iR2;
  auto run_batch = [&](const real (&rb)[U * R]) {
#pragma unroll
    for (int u = 0; u < U; ++u) cutoff_interact<KERNEL, D, E, SIG, real>(x, acc, rb + u * R, r2, iR2, exp_tab);
  };

  for (int q = 0; q < t.nruns; ++q) {
    const CutoffRun run = a.runs[t.run0 + q];
    const real* __restrict__ segp = a.rec + run.rec0 * R;
    const int seg_n = run.len;
    real ra[U * R], rb[U * R];
#pragma unroll
    for (int i = 0; i < U * R; ++i) ra[i] = segp[i];
    for (int c0 = 0; c0 < seg_n; c0 += a.chunk) {
      const int c1 = min(c0 + a.chunk, seg_n);
      for (int j = c0; j < c1; j += 2 * U) {
        const real* __restrict__ pb = segp + (int64_t)(j + U) * R;
#pragma unroll
        for (int i = 0; i < U * R; ++i) rb[i] = pb[i];
        run_batch(ra);
        const real* __restrict__ pa = segp + (int64_t)(j + 2 * U) * R;
#pragma unroll
        for (int i = 0; i < U * R; ++i) ra[i] = pa[i];
        run_batch(rb);
      }
      fold();
    }
  }

  // ---- the lane's fp64 row at the caller's index.  A tile without runs leaves zeros (0 / 0 = NaN when normalised): the
  // plain entry's M = 0.  A NaN target coordinate gives a NaN row (every pair of it is NaN, hence outside: nan_target).
  if (lane < t.live) {
    bool x_nan = false;
#pragma unroll
    for (int d = 0; d < D; ++d) x_nan |= x[d] != x[d];
    double v[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) {
      if constexpr (F32) v[e] = accd[e];
      else v[e] = (double)acc[e];
      v[e] = nan_target(x_nan, v[e]);
    }
    constexpr int EO = SIG == SIG_DENSITY ? 1 : E;  // columns of the result
    double* __restrict__ row = a.out + a.tmap[slot0 + lane] * EO;
#pragma unroll
    for (int e = 0; e < EO; ++e) {
      if constexpr (SIG == SIG_NORM) row[e] = v[e] / v[E];
      else if constexpr (SIG == SIG_DENSITY) row[e] = a.self_norm ? v[e] / v[e] : v[e];
      else row[e] = v[e];
    }
  }
}

// The same walk with an int32 counter per lane (a tile walks fewer than 2^31 records: kmvp_cutoff_plan.hpp).
template <int D, typename real>
__global__ void __launch_bounds__(BLOCK_THREADS) lowd_cutoff_count_kernel(const LowdCutoffArgs<real> a) {
  constexpr int R = RecLayout<D, 1, SIG_DENSITY>::R;
  constexpr int U = 4;
  static_assert(2 * U == CUTOFF_RECORDS, "two ping-pong batches per round");

  const int lane = threadIdx.x & 63;
  int64_t slot0;
  const CutoffTile t = cutoff_tile_of_wave(a.tiles, slot0);

  real x[D];
  bool x_nan = false, x_fin = true;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    x[d] = a.xs[(int64_t)d * a.n_pad + slot0 + lane];
    x_nan = x_nan || (x[d] != x[d]);
    x_fin = x_fin && (x[d] - x[d] == (real)0);
  }
  const real r2 = a.r2;
  int cnt = 0;
  auto run_batch = [&](const real (&rb)[U * R]) {
#pragma unroll
    for (int u = 0; u < U; ++u) cnt += knn_sqdist<D, real>(x, rb + u * R) <= r2 ? 1 : 0;
  };
  for (int q = 0; q < t.nruns; ++q) {
    const CutoffRun run = a.runs[t.run0 + q];
    const real* __restrict__ segp = a.rec + run.rec0 * R;
    const int seg_n = run.len;
    real ra[U * R], rb[U * R];
#pragma unroll
    for (int i = 0; i < U * R; ++i) ra[i] = segp[i];
    for (int j = 0; j < seg_n; j += 2 * U) {
      const real* __restrict__ pb = segp + (int64_t)(j + U) * R;
#pragma unroll
      for (int i = 0; i < U * R; ++i) rb[i] = pb[i];
      run_batch(ra);
      const real* __restrict__ pa = segp + (int64_t)(j + 2 * U) * R;
#pragma unroll
      for (int i = 0; i < U * R; ++i) ra[i] = pa[i];
      run_batch(rb);
    }
  }
  if (lane < t.live)
    a.counts[a.tmap[slot0 + lane]] = x_nan ? (int64_t)-1 : (int64_t)cnt - ((a.exclude_self && x_fin) ? 1 : 0);
}

// kmvp_lowd_cutoff_inst.hip, one unit per precision: the Gaussian, exp(-r) and the two Matern kernels, D <= 3, E <= 4 in
// the three signal modes; the count per D.  kmvp_lowd_wendland_inst.hip, again one unit per precision: the two Wendland
// kernels in the same shapes.  hipErrorInvalidValue where nothing is instantiated.
hipError_t launch_lowd_cutoff_f32(int kernel, int D, int E, int sig, const LowdCutoffArgs<float>& args, dim3 grid, hipStream_t stream,
                                  const char** kernel_name);
hipError_t launch_lowd_cutoff_f64(int kernel, int D, int E, int sig, const LowdCutoffArgs<double>& args, dim3 grid, hipStream_t stream,
                                  const char** kernel_name);
hipError_t launch_lowd_wendland_f32(int kernel, int D, int E, int sig, const LowdCutoffArgs<float>& args, dim3 grid, hipStream_t stream,
                                    const char** kernel_name);
hipError_t launch_lowd_wendland_f64(int kernel, int D, int E, int sig, const LowdCutoffArgs<double>& args, dim3 grid, hipStream_t stream,
                                    const char** kernel_name);
hipError_t launch_lowd_cutoff_count_f32(int D, const LowdCutoffArgs<float>& args, dim3 grid, hipStream_t stream, const char** kernel_name);
hipError_t launch_lowd_cutoff_count_f64(int D, const LowdCutoffArgs<double>& args, dim3 grid, hipStream_t stream, const char** kernel_name);

}  // namespace kmvp
