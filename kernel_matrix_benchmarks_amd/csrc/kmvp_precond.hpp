// The small dense routines of the pivoted-Cholesky preconditioner (include/kmvp.h kmvp_set_solver_preconditioner; build and
// apply: kmvp_precond.hip).
//
// P = L L' + D is applied through the Woodbury identity, P^-1 r = D^-1 r - D^-1 L C^-1 L' D^-1 r with the R x R matrix
// C = I + L' D^-1 L, R <= 128.  C is symmetric positive definite: pc_cholesky() factors it once per build, C = G G', and
// every apply solves C w = t by pc_forward() (G y = t) and pc_backward() (G' w = y); pc_logdet() reads log det C off G.
//
// Plain C++ with the device attributes behind a macro: the same text runs on the host for the build, in pc_solve_kernel
// (kmvp_precond.hip) for the apply -- there on the 16 x 16 diagonal blocks of the factor -- and, compiled with a host
// compiler alone, in tests/test_host_precond.py.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define KMVP_HD __host__ __device__
#else
#define KMVP_HD
#endif

namespace kmvp {

constexpr int PRECOND_MAX_RANK = 128;  // KMVP_PRECOND_MAX_RANK of include/kmvp.h

// a (order n, row-major, leading dimension ld) = G G' in place: G in the lower triangle, the strict upper triangle is
// neither read nor written.  Returns false at the first pivot that is not positive (NaN included): a is then not
// positive definite in float64 and holds a partial factor.
KMVP_HD inline bool pc_cholesky(double* a, int n, int ld) {
  for (int j = 0; j < n; ++j) {
    double piv = a[j * ld + j];
    for (int k = 0; k < j; ++k) piv = __builtin_fma(-a[j * ld + k], a[j * ld + k], piv);
    if (!(piv > 0.0)) return false;
    const double g = __builtin_sqrt(piv);
    a[j * ld + j] = g;
    for (int i = j + 1; i < n; ++i) {
      double v = a[i * ld + j];
      for (int k = 0; k < j; ++k) v = __builtin_fma(-a[i * ld + k], a[j * ld + k], v);
      a[i * ld + j] = v / g;
    }
  }
  return true;
}

// G y = v in place; v[i * stride], i < n
KMVP_HD inline void pc_forward(const double* g, int n, int ld, double* v, int stride) {
  for (int i = 0; i < n; ++i) {
    double s = v[i * stride];
    for (int k = 0; k < i; ++k) s = __builtin_fma(-g[i * ld + k], v[k * stride], s);
    v[i * stride] = s / g[i * ld + i];
  }
}

// G' w = v in place
KMVP_HD inline void pc_backward(const double* g, int n, int ld, double* v, int stride) {
  for (int i = n - 1; i >= 0; --i) {
    double s = v[i * stride];
    for (int k = i + 1; k < n; ++k) s = __builtin_fma(-g[k * ld + i], v[k * stride], s);
    v[i * stride] = s / g[i * ld + i];
  }
}

// log det (G G') = 2 sum_t log G_tt of a factor pc_cholesky() left, added in ascending t: the factor's share of
// log det P = sum_i log D_i + log det (I + L' D^-1 L) (the matrix-determinant lemma; kmvp_<kernel>_lanczos_quadrature_precond)
KMVP_HD inline double pc_logdet(const double* g, int n, int ld) {
  double s = 0.0;
  for (int t = 0; t < n; ++t) s += __builtin_log(g[t * ld + t]);
  return 2.0 * s;
}

}  // namespace kmvp
