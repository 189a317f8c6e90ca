// The rule of one mean-shift sweep for one point (include/kmvp.h kmvp_gaussian_meanshift; iteration: kmvp_meanshift.hip).
//
// For the Gaussian the gradient of the log-sum-exp is G = -2 (x - ybar), ybar the softmax-weighted barycentre of the
// sources, so x + G / 2 is the mean-shift update.  ms_step_point() takes the row G that the gradient returns for the point
// at base = (double) real(z_{k-1}) and leaves z_k = base + G / 2 and q = |G / 2|^2; its return value is the verdict on the
// point: it goes on, it froze within the tolerance, or it froze because G is not finite (z_k and q are NaN then).
//
// Every product and every sum is rounded on its own, d ascending: no fused multiply-add anywhere, so that a numpy
// restatement reproduces the bits.  ms_mul() / ms_add() are the equivalent of __dmul_rn / __dadd_rn that holds under hipcc:
// HIP spells those two as a plain x * y and x + y in a header compiled with contraction allowed, and the compiler fused
// them into v_fma_f64 here; `#pragma clang fp contract(off)` inside the function takes the licence away from the very
// instruction (host and device pass alike).  g++ has no such pragma and is given -ffp-contract=off by whoever compiles
// this header for a machine with fused multiply-add.
//
// Plain C++ with the device attributes behind a macro: the same text runs in ms_step_kernel (kmvp_meanshift.hip) and,
// compiled with a host compiler alone, in tests/test_host_meanshift_step.py.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KMVP_HD __host__ __device__
#else
#define KMVP_HD
#endif

namespace kmvp {

// the verdict on a point after a sweep
enum : int { MS_ACTIVE = 0, MS_FROZEN = 1, MS_NONFINITE = 2 };

KMVP_HD inline double ms_mul(double a, double b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return a * b;
}
KMVP_HD inline double ms_add(double a, double b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return a + b;
}

// One point, one sweep.  G[0 .. D): the gradient row; base[0 .. D): the position the gradient was taken at, already rounded
// to the working precision; z[0 .. D): the new position (may alias base); *q: the squared step.
//   every G[d] finite:  z[d] = base[d] + 0.5 G[d],  q = sum_d (0.5 G[d])^2,  MS_FROZEN if q <= tol * tol, else MS_ACTIVE
//   otherwise:          z[d] = NaN for all d,       q = NaN,                 MS_NONFINITE
// (q = +inf, from a finite but huge G, is neither: the point stays active, as the comparison says.)
KMVP_HD inline int ms_step_point(const double* G, const double* base, int D, double tol, double* z, double* q) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  bool finite = true;
  for (int d = 0; d < D; ++d) finite = finite && (G[d] - G[d] == 0.0);  // false for +-inf and NaN alike
  if (!finite) {
    for (int d = 0; d < D; ++d) z[d] = __builtin_nan("");
    *q = __builtin_nan("");
    return MS_NONFINITE;
  }
  double s = 0.0;
  for (int d = 0; d < D; ++d) {
    const double h = ms_mul(0.5, G[d]);
    z[d] = ms_add(base[d], h);
    s = ms_add(s, ms_mul(h, h));
  }
  *q = s;
  return s <= ms_mul(tol, tol) ? MS_FROZEN : MS_ACTIVE;
}

}  // namespace kmvp
