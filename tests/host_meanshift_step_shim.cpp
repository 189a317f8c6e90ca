// Host-side shim for tests/test_host_meanshift_step.py: csrc/kmvp_meanshift_step.hpp (the rule of one mean-shift sweep for
// one point) compiled with a host compiler alone, behind a C surface.
#include "kmvp_meanshift_step.hpp"

extern "C" {

int ms_code(int which) {
  const int codes[3] = {kmvp::MS_ACTIVE, kmvp::MS_FROZEN, kmvp::MS_NONFINITE};
  return codes[which];
}

// n points of D coordinates, row-major: verdict[i], z[i][:], q[i]
void ms_step_rows(const double* G, const double* base, long n, int D, double tol, double* z, double* q, int* verdict) {
  for (long i = 0; i < n; ++i) verdict[i] = kmvp::ms_step_point(G + i * D, base + i * D, D, tol, z + i * D, q + i);
}

}
