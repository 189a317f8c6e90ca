// Eigenpairs of a symmetric tridiagonal matrix in float64 by the implicit QL iteration: plain C++, no HIP, so the host tests
// compile it on its own (tests/host_tridiag_shim.cpp).  The Lanczos eigen-solver (kmvp_eigsh.hip) calls it on the j x j
// matrix of its coefficients at every look of the host; the library links no LAPACK.
//
// It is jacobi_nodes (kmvp_quadrature.hpp) with the rotations carried on `rows` rows of the eigenvector matrix instead of
// on the first one only, and with the same failure rules: false for a non-finite entry or 60 sweeps on one eigenvalue.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <limits>
#include <numeric>
#include <vector>

namespace kmvp {

// Eigenvalues (into d, unsorted) of the symmetric tridiagonal matrix with diagonal d[0..m) and off-diagonal e[0..m-1) (e
// has m entries, the last is scratch), and into z (rows x m, row-major) the first `rows` rows of the matrix whose columns
// are the normalised eigenvectors: z[r * m + i] is component r of the eigenvector of d[i].  rows = 1: the first components,
// rows = m: every eigenvector.
inline bool tridiag_ql(std::vector<double>& d, std::vector<double>& e, std::vector<double>& z, int rows) {
  const int m = (int)d.size();
  z.assign((size_t)rows * m, 0.0);
  if (m == 0) return true;
  for (int r = 0; r < rows; ++r) z[(size_t)r * m + r] = 1.0;
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
        for (int q = 0; q < rows; ++q) {  // the same rotation on every row kept of the eigenvector matrix
          double* zr = z.data() + (size_t)q * m;
          f = zr[i + 1];
          zr[i + 1] = s * zr[i] + c * f;
          zr[i] = c * zr[i] - s * f;
        }
      }
      if (r == 0.0 && i >= l) continue;
      d[l] -= p;
      e[l] = g;
      e[k] = 0.0;
    }
  }
  return true;
}

// order[i] = index of the i-th largest of d (ties: the smaller index first)
inline std::vector<int> descending_order(const std::vector<double>& d) {
  std::vector<int> order(d.size());
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return d[a] > d[b]; });
  return order;
}

// All eigenpairs of the m x m symmetric tridiagonal with diagonal alpha[0..m) and off-diagonal beta[0..m-1): theta (m)
// descending, and z (m x m, row-major) with column i the normalised eigenvector of theta[i].
inline bool tridiag_eigen(const double* alpha, const double* beta, int m, std::vector<double>& theta, std::vector<double>& z) {
  std::vector<double> d(alpha, alpha + m), e(m, 0.0), zz;
  for (int i = 0; i + 1 < m; ++i) e[i] = beta[i];
  theta.assign(m, std::numeric_limits<double>::quiet_NaN());
  z.assign((size_t)m * m, std::numeric_limits<double>::quiet_NaN());
  if (!tridiag_ql(d, e, zz, m)) return false;
  const std::vector<int> order = descending_order(d);
  for (int i = 0; i < m; ++i) {
    theta[i] = d[order[i]];
    for (int r = 0; r < m; ++r) z[(size_t)r * m + i] = zz[(size_t)r * m + order[i]];
  }
  return true;
}

// The eigenvalues, descending, and the LAST components of the normalised eigenvectors: all a look of the Lanczos process
// needs.  The last row of the eigenvector matrix of T is the first row of that of the reversed matrix J T J, so one row is
// carried through the iteration.
inline bool tridiag_eigen_last(const double* alpha, const double* beta, int m, std::vector<double>& theta,
                               std::vector<double>& last) {
  std::vector<double> d(m), e(m, 0.0), w;
  for (int i = 0; i < m; ++i) d[i] = alpha[m - 1 - i];
  for (int i = 0; i + 1 < m; ++i) e[i] = beta[m - 2 - i];
  theta.assign(m, std::numeric_limits<double>::quiet_NaN());
  last.assign(m, std::numeric_limits<double>::quiet_NaN());
  if (!tridiag_ql(d, e, w, 1)) return false;
  const std::vector<int> order = descending_order(d);
  for (int i = 0; i < m; ++i) {
    theta[i] = d[order[i]];
    last[i] = w[order[i]];
  }
  return true;
}

}  // namespace kmvp
