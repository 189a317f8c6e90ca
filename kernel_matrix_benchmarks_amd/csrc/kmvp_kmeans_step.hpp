// Per-cluster arithmetic and the verdict of one Lloyd iteration (include/kmvp.h kmvp_kmeans; iteration: kmvp_kmeans.hip).
//
// The centroid update leaves, per cluster, the float64 sums  sum w x_d (d < D)  and  sum w  over the points that carry its
// label.  km_step_cluster() turns them into the new centroid -- a cluster of total weight 0 keeps its position -- and
// returns the cluster's term |c_k - c_{k-1}|^2 of the shift; km_verdict() is the stop word of the iteration.
//
// Plain C++ with the device attributes behind a macro: the same text runs in km_scalars_kernel (kmvp_kmeans.hip) and,
// compiled with a host compiler alone, in tests/test_host_kmeans_step.py.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KMVP_HD __host__ __device__
#else
#define KMVP_HD
#endif

namespace kmvp {

// the stop word (the state words follow Sinkhorn's: stop, iterations, then the iteration's scalars)
enum : int { KM_RUNNING = 0, KM_CONVERGED = 1, KM_NONFINITE = 2, KM_MAXIT = 3 };

// One cluster.  sums[d * stride], d < D: sum w x_d;  sums[D * stride]: W = sum w.  cent[0 .. D): c_{k-1} on entry, c_k on
// return: sums / W where W > 0, untouched otherwise (no point of positive weight carries the label: the centroid stays
// where it is, bit for bit, and its term of the shift is exactly 0).  *weight = W.  Returns sum_d (c_k - c_{k-1})_d^2,
// accumulated in d order with one rounding per term (fma), the same on the host and on the device.
KMVP_HD inline double km_step_cluster(const double* sums, int64_t stride, int D, double* cent, double* weight) {
  const double W = sums[(int64_t)D * stride];
  *weight = W;
  double term = 0.0;
  if (!(W > 0.0)) return term;
  for (int d = 0; d < D; ++d) {
    const double c = sums[(int64_t)d * stride] / W;
    const double diff = c - cent[d];
    term = __builtin_fma(diff, diff, term);
    cent[d] = c;
  }
  return term;
}

// The verdict on iteration `iters` (already counted).  unlabelled: the points without a qualifying centroid (label -1).
// Non-finite input ends the solve before anything else is asked; the first iteration whose shift is within tol converges,
// also when it is the last one allowed.
KMVP_HD inline int km_verdict(double unlabelled, double inertia, double shift, double iters, double tol, int maxit) {
  const bool finite = inertia - inertia == 0.0 && shift - shift == 0.0;  // false for +-inf and NaN alike
  if (unlabelled != 0.0 || !finite) return KM_NONFINITE;
  if (shift <= tol) return KM_CONVERGED;
  if (iters >= (double)maxit) return KM_MAXIT;
  return KM_RUNNING;
}

}  // namespace kmvp
