// C surface of the small dense routines of csrc/kmvp_precond.hpp for tests/test_host_precond.py (host compiler only, no
// HIP).
#include "kmvp_precond.hpp"

using namespace kmvp;

extern "C" {

int hp_max_rank(void) { return PRECOND_MAX_RANK; }

// a (n x n, leading dimension ld) = G G' in place; 1 on success, 0 at a pivot that is not positive
int hp_cholesky(double* a, int n, int ld) { return pc_cholesky(a, n, ld) ? 1 : 0; }

// G y = v, then G' w = y, in place on v[i * stride]
void hp_forward(const double* g, int n, int ld, double* v, int stride) { pc_forward(g, n, ld, v, stride); }
void hp_backward(const double* g, int n, int ld, double* v, int stride) { pc_backward(g, n, ld, v, stride); }
}
