// C surface of the tridiagonal eigen-solver of csrc/kmvp_tridiag.hpp for tests/test_host_tridiag.py (host compiler only, no
// HIP).
#include "kmvp_tridiag.hpp"

using namespace kmvp;

extern "C" {

// theta (m) descending and z (m x m row-major, column i the eigenvector of theta[i]); returns 1 on success, 0 on failure
int ht_eigen(const double* alpha, const double* beta, int m, double* theta, double* z) {
  std::vector<double> t, zz;
  const bool ok = tridiag_eigen(alpha, beta, m, t, zz);
  for (int i = 0; i < m; ++i) theta[i] = t[i];
  for (size_t i = 0; i < (size_t)m * m; ++i) z[i] = zz[i];
  return ok ? 1 : 0;
}

// theta (m) descending and the last components of the eigenvectors
int ht_eigen_last(const double* alpha, const double* beta, int m, double* theta, double* last) {
  std::vector<double> t, l;
  const bool ok = tridiag_eigen_last(alpha, beta, m, t, l);
  for (int i = 0; i < m; ++i) {
    theta[i] = t[i];
    last[i] = l[i];
  }
  return ok ? 1 : 0;
}
}
