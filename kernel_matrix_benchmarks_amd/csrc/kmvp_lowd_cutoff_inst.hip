// Instantiations of the cutoff-radius kernels (kmvp_lowd_cutoff.hpp) for ONE precision.
// Compiled twice (see Makefile):
//   -DKMVP_REAL={float,double}  -DKMVP_FN=launch_lowd_cutoff_<p>  -DKMVP_FN_COUNT=launch_lowd_cutoff_count_<p>
// lowd_cutoff_kernel: the Gaussian, exp(-r) and the two Matern kernels, D = 1 .. CUTOFF_MAX_D, the product and normalised
// rows at E = 1 .. LOWD_MAX_E, density.  lowd_cutoff_count_kernel: one variant per D.
#include "kmvp_internal.hpp"
#include "kmvp_lowd_cutoff.hpp"

#if !defined(KMVP_REAL) || !defined(KMVP_FN) || !defined(KMVP_FN_COUNT)
#error "KMVP_REAL, KMVP_FN and KMVP_FN_COUNT must be defined"
#endif

namespace kmvp {

using real = KMVP_REAL;

template <int KERNEL, int D, int E, int SIG>
static hipError_t launch_one(const LowdCutoffArgs<real>& args, dim3 grid, hipStream_t stream, const char** kernel_name) {
  hipLaunchKernelGGL((lowd_cutoff_kernel<KERNEL, D, E, SIG, real>), grid, dim3(BLOCK_THREADS), 0, stream, args);
  if (kernel_name) *kernel_name = "lowd_cutoff_kernel";
  return hipGetLastError();
}

template <int KERNEL, int D>
static hipError_t launch_e(int E, int sig, const LowdCutoffArgs<real>& args, dim3 grid, hipStream_t stream, const char** kernel_name) {
  if (sig == SIG_DENSITY) return launch_one<KERNEL, D, 1, SIG_DENSITY>(args, grid, stream, kernel_name);
#define KMVP_CUTOFF_E(EV)                                                                                    \
  case EV:                                                                                                   \
    return sig == SIG_NORM ? launch_one<KERNEL, D, EV, SIG_NORM>(args, grid, stream, kernel_name)            \
                           : launch_one<KERNEL, D, EV, SIG_PRODUCT>(args, grid, stream, kernel_name);
  switch (E) {
    KMVP_CUTOFF_E(1)
    KMVP_CUTOFF_E(2)
    KMVP_CUTOFF_E(3)
    KMVP_CUTOFF_E(4)
    default: return hipErrorInvalidValue;
  }
#undef KMVP_CUTOFF_E
}

template <int KERNEL>
static hipError_t launch_d(int D, int E, int sig, const LowdCutoffArgs<real>& args, dim3 grid, hipStream_t stream,
                           const char** kernel_name) {
  switch (D) {
    case 1: return launch_e<KERNEL, 1>(E, sig, args, grid, stream, kernel_name);
    case 2: return launch_e<KERNEL, 2>(E, sig, args, grid, stream, kernel_name);
    case 3: return launch_e<KERNEL, 3>(E, sig, args, grid, stream, kernel_name);
    default: return hipErrorInvalidValue;
  }
}

hipError_t KMVP_FN(int kernel, int D, int E, int sig, const LowdCutoffArgs<real>& args, dim3 grid, hipStream_t stream,
                   const char** kernel_name) {
  if (sig != SIG_PRODUCT && sig != SIG_NORM && sig != SIG_DENSITY) return hipErrorInvalidValue;
  switch (kernel) {
    case K_GAUSSIAN: return launch_d<K_GAUSSIAN>(D, E, sig, args, grid, stream, kernel_name);
    case K_ABSEXP: return launch_d<K_ABSEXP>(D, E, sig, args, grid, stream, kernel_name);
    case K_MATERN32: return launch_d<K_MATERN32>(D, E, sig, args, grid, stream, kernel_name);
    case K_MATERN52: return launch_d<K_MATERN52>(D, E, sig, args, grid, stream, kernel_name);
    default: return hipErrorInvalidValue;
  }
}

template <int D>
static hipError_t launch_count_one(const LowdCutoffArgs<real>& args, dim3 grid, hipStream_t stream, const char** kernel_name) {
  hipLaunchKernelGGL((lowd_cutoff_count_kernel<D, real>), grid, dim3(BLOCK_THREADS), 0, stream, args);
  if (kernel_name) *kernel_name = "lowd_cutoff_count_kernel";
  return hipGetLastError();
}

hipError_t KMVP_FN_COUNT(int D, const LowdCutoffArgs<real>& args, dim3 grid, hipStream_t stream, const char** kernel_name) {
  switch (D) {
    case 1: return launch_count_one<1>(args, grid, stream, kernel_name);
    case 2: return launch_count_one<2>(args, grid, stream, kernel_name);
    case 3: return launch_count_one<3>(args, grid, stream, kernel_name);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace kmvp
