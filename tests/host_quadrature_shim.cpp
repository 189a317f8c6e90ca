// C surface of the Gauss quadrature of csrc/kmvp_quadrature.hpp for tests/test_host_quadrature.py (host compiler only, no
// HIP).
#include "kmvp_quadrature.hpp"

using namespace kmvp;

extern "C" {

// sum tau^2 log(theta) of one column's first m coefficients (NaN for a theta <= 0 or a non-finite coefficient)
double hq_log(const double* alpha, const double* beta, int m, long stride) {
  return lanczos_quadrature_log(alpha, beta, m, (std::ptrdiff_t)stride);
}

// sum tau^2 / theta: the same nodes and weights under another function
double hq_inverse(const double* alpha, const double* beta, int m, long stride) {
  return lanczos_quadrature(alpha, beta, m, (std::ptrdiff_t)stride, [](double t) { return 1.0 / t; });
}

// sum tau^2 |log theta|: the scale the errors of hq_log are measured in
double hq_abs_log(const double* alpha, const double* beta, int m, long stride) {
  return lanczos_quadrature(alpha, beta, m, (std::ptrdiff_t)stride, [](double t) { return std::fabs(std::log(t)); });
}
}
