// Gradient of the cutoff-radius product with respect to the target points (include/kmvp.h kmvp_<kernel>_cutoff_grad) on the
// cell list of kmvp_cutoff_plan.hpp:
//   G[i, e, :] = c sum_{j : s_ij <= r2} W(s_ij) (x_i - y_j) b[j, e]
// lowd_cutoff_kernel's walk (kmvp_lowd_cutoff.hpp) around grad_interact's pair body (kmvp_lowd_grad.hpp).  Lanes are
// targets, one per lane; the tile's entry is read at a wave-uniform address (readfirstlane), so the entry, every run entry
// and every record arrive through the scalar data cache, a run's records in two SGPR batches of U = 4 in ping-pong.  Nothing
// inside the loops synchronises the workgroup: the float64 table of kexp_neg_f64 is filled, and its one barrier passed,
// before them, and the Wendland instantiations have neither.  It reads the product's LowdCutoffArgs and ct_* buffers with
// the product's record length, so a product and a gradient on one context plan and pack once.
//
// Per pair: the D differences x - y are formed once and KEPT, s is one square and D - 1 fmas of them -- knn_sqdist's
// expression bit for bit, so a row's inside set is the set kmvp_radius_count counts (a pair at exactly r2 is inside, a NaN s
// is outside).  W is grad_weight<KERNEL>(s) for the Gaussian, exp(-r) and the two Matern kernels, wendland_grad_weight
// below for Wendland's; c is grad_constant<KERNEL>(), resp. -20 / R^2 (C2) and -56 / (3 R^2) (C4), formed in double by the
// host (LowdCutoffArgs::gconst) and applied once per row in float64, never per pair.
//
// For the four truncated kernels G is the sum of the plain gradient's terms over the inside set: it equals the derivative
// of the truncated sum wherever no pair sits on the boundary (the truncated sum jumps there).  Wendland's two gradients are
// continuous and vanish at the boundary: they are the exact gradients of the exact products.
//
// An outside pair that is walked adds exactly +0 to every component.  Zeroing W alone is not enough: pad records sit at
// y = +inf, so their kept differences are -inf and 0 * -inf is NaN (and Wendland C4 gives 0 * inf in W itself).  W AND the
// D differences are selected to 0 on the one inside condition: D + 1 v_cndmask per pair whatever E is.  Selecting the
// E D accumulations instead costs E D of them: up to 8 more at D = 3, E = 4, one fewer at E = 1 (density included).  By
// counted issue slots the select therefore sits on W and the differences for E >= 2; at E = 1 the other form counts one slot
// per pair less, was built and measured, and was not faster (LAB_NOTES.md section 35), so one form serves every shape.
// exp(-r) keeps lowd_grad_kernel's positive_normal(s) select, folded into the same condition: s <= r2 && positive_normal(s),
// so a coincident or denormal-s pair contributes 0, the own pair of same_points included; for the other five kernels the
// own pair vanishes as W * 0.
//
// float32 keeps E D sums per lane, folded into fp64 every `chunk` walked records and at every run's end; float64 keeps one
// chain.  A live lane writes its fp64 row at the caller's index, read from tmap: no segments, no partials, no atomics, the
// same bits run to run.  A target with nothing inside gets +0 (c * 0 = -0 is written as -0 + 0 = +0), a NaN target
// coordinate a NaN row in every component (every pair of it is outside: nan_target at the write), an infinite one zeros.
// A non-finite source is in no record (kmvp_cutoff_plan.hpp), so it touches no row -- unlike lowd_grad_kernel, which does
// not screen its sources.
//
// Reads past a run are lowd_cutoff_kernel's: rec0 + len + U <= m_alloc for every run (tests/test_host_cutoff_plan.py).
#pragma once
#include "kmvp_lowd_cutoff.hpp"
#include "kmvp_lowd_grad.hpp"

namespace kmvp {

// |dk/dx| / |x - y| without its constant, from wendland_value's t and u:  C2: u^3;  C4: u^5 (5 t + 1).  q = inf (a pad
// record) gives u = 0 and, in C4, 0 * inf = NaN, a NaN s a NaN: the caller's select on s <= r2 removes both.
// Per pair after s, float32: v_mul, v_sqrt, v_sub, v_max, 2 (3) v_mul, C4 alone: v_fma, v_mul.
template <int KERNEL, typename real>
__device__ __forceinline__ real wendland_grad_weight(real s, real iR2) {
  const real q = s * iR2;
  const real t = wendland_sqrt(q);
  const real u = fmax((real)1 - t, (real)0);
  const real u2 = u * u;
  if constexpr (KERNEL == K_WENDLAND_C2) return u2 * u;
  else return ((u2 * u2) * u) * fma((real)5, t, (real)1);
}

// One (target, source) pair: grad_interact's arithmetic (kmvp_lowd_grad.hpp) with the inside select between the weight and
// the accumulation.
template <int KERNEL, int D, int E, int SIG, typename real>
__device__ __forceinline__ void cutoff_grad_interact(const real (&x)[D], real (&acc)[GradLayout<D, E, SIG>::NC],
                                                     const real* __restrict__ r, real r2, real iR2, const double* __restrict__ tab) {
  real df[D];
  df[0] = x[0] - r[0];
  real s = df[0] * df[0];
#pragma unroll
  for (int d = 1; d < D; ++d) {
    df[d] = x[d] - r[d];
    s = fma(df[d], df[d], s);
  }
  real w;
  if constexpr (KERNEL_IS_WENDLAND<KERNEL>) w = wendland_grad_weight<KERNEL, real>(s, iR2);
  else w = grad_weight<KERNEL>(s, tab);
  bool inside = s <= r2;
  if constexpr (KERNEL == K_ABSEXP) inside = inside && positive_normal(s);
  w = inside ? w : (real)0;
#pragma unroll
  for (int d = 0; d < D; ++d) df[d] = inside ? df[d] : (real)0;
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

// lowd_cutoff_kernel's walk over the wave tile's runs with `pair(record)` as its body and `fold()` every `chunk` walked
// records and at every run's end.
template <int R, typename real, typename Pair, typename Fold>
__device__ __forceinline__ void cutoff_walk(const CutoffTile& t, const CutoffRun* __restrict__ runs, const real* __restrict__ rec,
                                            int chunk, Pair pair, Fold fold) {
  constexpr int U = 4;  // records per SGPR batch; runs hold a whole number of 2 U
  static_assert(2 * U == CUTOFF_RECORDS, "two ping-pong batches per round");
  for (int q = 0; q < t.nruns; ++q) {
    const CutoffRun run = runs[t.run0 + q];
    const real* __restrict__ segp = rec + run.rec0 * R;
    const int seg_n = run.len;
    real ra[U * R], rb[U * R];
#pragma unroll
    for (int i = 0; i < U * R; ++i) ra[i] = segp[i];
    for (int c0 = 0; c0 < seg_n; c0 += chunk) {
      const int c1 = min(c0 + chunk, seg_n);
      for (int j = c0; j < c1; j += 2 * U) {
        const real* __restrict__ pb = segp + (int64_t)(j + U) * R;
#pragma unroll
        for (int i = 0; i < U * R; ++i) rb[i] = pb[i];
#pragma unroll
        for (int u = 0; u < U; ++u) pair(ra + u * R);
        const real* __restrict__ pa = segp + (int64_t)(j + 2 * U) * R;
#pragma unroll
        for (int i = 0; i < U * R; ++i) ra[i] = pa[i];
#pragma unroll
        for (int u = 0; u < U; ++u) pair(rb + u * R);
      }
      fold();
    }
  }
}

template <int KERNEL, int D, int E, int SIG, typename real>
__global__ void __launch_bounds__(BLOCK_THREADS) lowd_cutoff_grad_kernel(const LowdCutoffArgs<real> a) {
  static_assert(SIG == SIG_PRODUCT || SIG == SIG_DENSITY, "the gradient of a ratio is not built");
  constexpr int R = RecLayout<D, E, SIG>::R;
  constexpr int NC = GradLayout<D, E, SIG>::NC;
  constexpr bool F32 = sizeof(real) == 4;
  constexpr bool TABLE = !F32 && !KERNEL_IS_WENDLAND<KERNEL>;

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

  double accd[NC];
  real acc[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    accd[c] = 0.0;
    acc[c] = 0;
  }
  const real r2 = a.r2;
  const real iR2 = a.iR2;
  cutoff_walk<R, real>(
      t, a.runs, a.rec, a.chunk,
      [&](const real* __restrict__ r) { cutoff_grad_interact<KERNEL, D, E, SIG, real>(x, acc, r, r2, iR2, exp_tab); },
      [&]() {
        if constexpr (F32) {
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            accd[c] += (double)acc[c];
            acc[c] = 0;
          }
        }
      });

  // ---- the lane's fp64 row (E D values, column e D + d) at the caller's index: c v + 0, so that a row with nothing inside
  // is +0.  A NaN target coordinate gives a NaN row (every pair of it is NaN, hence outside: nan_target).
  if (lane < t.live) {
    bool x_nan = false;
#pragma unroll
    for (int d = 0; d < D; ++d) x_nan |= x[d] != x[d];
    double* __restrict__ row = a.out + a.tmap[slot0 + lane] * NC;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      double v;
      if constexpr (F32) v = accd[c];
      else v = (double)acc[c];
      row[c] = nan_target(x_nan, fma(a.gconst, v, 0.0));
    }
  }
}

// kmvp_lowd_cutoff_grad_inst.hip, one unit per precision and family (the four truncated kernels; Wendland's two): D <= 3,
// E <= 4 as a product, density.  hipErrorInvalidValue where nothing is instantiated.
hipError_t launch_lowd_cutoff_grad_f32(int kernel, int D, int E, int sig, const LowdCutoffArgs<float>& args, dim3 grid, hipStream_t stream,
                                       const char** kernel_name);
hipError_t launch_lowd_cutoff_grad_f64(int kernel, int D, int E, int sig, const LowdCutoffArgs<double>& args, dim3 grid,
                                       hipStream_t stream, const char** kernel_name);
hipError_t launch_lowd_wendland_grad_f32(int kernel, int D, int E, int sig, const LowdCutoffArgs<float>& args, dim3 grid,
                                         hipStream_t stream, const char** kernel_name);
hipError_t launch_lowd_wendland_grad_f64(int kernel, int D, int E, int sig, const LowdCutoffArgs<double>& args, dim3 grid,
                                         hipStream_t stream, const char** kernel_name);

}  // namespace kmvp
