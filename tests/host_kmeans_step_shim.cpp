// Host-side shim for tests/test_host_kmeans_step.py: csrc/kmvp_kmeans_step.hpp (the per-cluster arithmetic and the verdict
// of one Lloyd iteration) compiled with a host compiler alone, behind a C surface.
#include "kmvp_kmeans_step.hpp"

extern "C" {

int hs_code(int which) {
  const int codes[4] = {kmvp::KM_RUNNING, kmvp::KM_CONVERGED, kmvp::KM_NONFINITE, kmvp::KM_MAXIT};
  return codes[which];
}

double hs_step_cluster(const double* sums, long stride, int D, double* cent, double* weight) {
  return kmvp::km_step_cluster(sums, stride, D, cent, weight);
}

int hs_verdict(double unlabelled, double inertia, double shift, double iters, double tol, int maxit) {
  return kmvp::km_verdict(unlabelled, inertia, shift, iters, tol, maxit);
}

}
