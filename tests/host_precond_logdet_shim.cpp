// pc_cholesky() and pc_logdet() of csrc/kmvp_precond.hpp behind a C interface, compiled with the host compiler alone
// (tests/test_host_precond_logdet.py): the header is plain C++ without the device attributes.
#include "kmvp_precond.hpp"

extern "C" {
int hl_cholesky(double* a, int n, int ld) { return kmvp::pc_cholesky(a, n, ld) ? 1 : 0; }
double hl_logdet(const double* g, int n, int ld) { return kmvp::pc_logdet(g, n, ld); }
}
