// Gauss quadrature on the coefficients of conjugate gradients (stochastic Lanczos quadrature): plain C++, no HIP, so the
// host tests compile it on its own (tests/host_quadrature_shim.cpp).
//
// CG on A x = z started from x = 0 is the Lanczos process on (A, z): after m iterations with step lengths alpha_k and
// beta_k (k = 1 .. m) the Lanczos tridiagonal -- the Jacobi matrix of the measure z' dE(lambda) z / |z|^2 -- is
//     d_1 = 1 / alpha_1,   d_k = 1 / alpha_k + beta_{k-1} / alpha_{k-1},   e_k = sqrt(beta_k) / alpha_k  (k < m)
// and with theta_i its eigenvalues and tau_i the first components of its normalised eigenvectors (Golub & Welsch)
//     z' f(A) z  ~  |z|^2 sum_i tau_i^2 f(theta_i),
// the m-point Gauss rule: exact for polynomials of degree < 2m, and for f = log with an error of the order of the square
// of CG's relative residual after m iterations.  The eigenproblem is solved by the implicit QL iteration in float64,
// carrying the first row of the eigenvector matrix only; the library links no LAPACK.
#pragma once
#include <cmath>
#include <cstddef>
#include <limits>
#include <vector>

namespace kmvp {

// Eigenvalues (into d) of the symmetric tridiagonal matrix with diagonal d[0..m) and off-diagonal e[0..m-1) (e has m
// entries, the last is scratch), and into w the first components of the eigenvectors.  false: no convergence (60 sweeps
// on one eigenvalue) or a non-finite entry.
inline bool jacobi_nodes(std::vector<double>& d, std::vector<double>& e, std::vector<double>& w) {
  const int m = (int)d.size();
  w.assign(m, 0.0);
  if (m == 0) return true;
  w[0] = 1.0;
  e[m - 1] = 0.0;
  for (int i = 0; i < m; ++i)
    if (!std::isfinite(d[i]) || !std::isfinite(e[i])) return false;
  const double eps = std::numeric_limits<double>::epsilon();
  for (int l = 0; l < m; ++l) {
    for (int sweep = 0;; ++sweep) {
      int k = l;
      for (; k < m - 1; ++k)
        if (std::fabs(e[k]) <= eps * (std::fabs(d[k]) + std::fabs(d[k + 1]))) break;
      if (k == l) break;
      if (sweep == 60) return false;
      double g = (d[l + 1] - d[l]) / (2.0 * e[l]);
      double r = std::hypot(g, 1.0);
      g = d[k] - d[l] + e[l] / (g + std::copysign(r, g));
      double s = 1.0, c = 1.0, p = 0.0;
      int i = k - 1;
      for (; i >= l; --i) {
        double f = s * e[i];
        const double b = c * e[i];
        r = std::hypot(f, g);
        e[i + 1] = r;
        if (r == 0.0) {  // an exact split: recover and start the sweep again
          d[i + 1] -= p;
          e[k] = 0.0;
          break;
        }
        s = f / r;
        c = g / r;
        g = d[i + 1] - p;
        r = (d[i] - g) * s + 2.0 * c * b;
        p = s * r;
        d[i + 1] = g + p;
        g = c * r - b;
        f = w[i + 1];  // the same rotation on the first row of the eigenvector matrix
        w[i + 1] = s * w[i] + c * f;
        w[i] = c * w[i] - s * f;
      }
      if (r == 0.0 && i >= l) continue;
      d[l] -= p;
      e[l] = g;
      e[k] = 0.0;
    }
  }
  return true;
}

// sum_i tau_i^2 f(theta_i) for the first m coefficients of one column: alpha[k * stride], beta[k * stride], k = 0 .. m-1
// (the history is stored (iteration, column), so a column is read with stride = columns), for f defined on theta > 0.
// m = 0 gives 0; a non-finite coefficient or Jacobi entry, a failed eigen-iteration and an eigenvalue <= 0 (the operator
// was not positive definite) give NaN.
template <typename F>
inline double lanczos_quadrature(const double* alpha, const double* beta, int m, std::ptrdiff_t stride, F f) {
  if (m <= 0) return 0.0;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<double> d(m), e(m, 0.0), w;
  for (int k = 0; k < m; ++k) {
    const double a = alpha[k * stride], b = beta[k * stride];
    if (!std::isfinite(a) || !std::isfinite(b)) return nan;
    d[k] = 1.0 / a + (k ? beta[(k - 1) * stride] / alpha[(k - 1) * stride] : 0.0);
    if (k + 1 < m) e[k] = std::sqrt(b) / a;
  }
  if (!jacobi_nodes(d, e, w)) return nan;
  double sum = 0.0;
  for (int i = 0; i < m; ++i) {
    if (!(d[i] > 0.0)) return nan;
    sum += w[i] * w[i] * f(d[i]);
  }
  return sum;
}

// f = log: |z|^2 times this is the estimate of z' log(A) z
inline double lanczos_quadrature_log(const double* alpha, const double* beta, int m, std::ptrdiff_t stride) {
  return lanczos_quadrature(alpha, beta, m, stride, [](double t) { return std::log(t); });
}

}  // namespace kmvp
