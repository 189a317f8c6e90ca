// Instantiations of lowd_cutoff_grad_kernel (kmvp_lowd_cutoff_grad.hpp) for ONE precision and ONE family of kernels.
// Compiled four times (see Makefile):
//   -DKMVP_REAL={float,double}  -DKMVP_WENDLAND=0  -DKMVP_FN=launch_lowd_cutoff_grad_<p>     Gaussian, exp(-r), Matern 3/2, 5/2
//   -DKMVP_REAL={float,double}  -DKMVP_WENDLAND=1  -DKMVP_FN=launch_lowd_wendland_grad_<p>   Wendland C2, C4
// D = 1 .. CUTOFF_MAX_D, the product at E = 1 .. LOWD_MAX_E, density.  There are no normalised rows: the gradient of a
// ratio is not built.
#include "kmvp_internal.hpp"
#include "kmvp_lowd_cutoff_grad.hpp"

#if !defined(KMVP_REAL) || !defined(KMVP_FN) || !defined(KMVP_WENDLAND)
#error "KMVP_REAL, KMVP_FN and KMVP_WENDLAND must be defined"
#endif

namespace kmvp {

using real = KMVP_REAL;

template <int KERNEL, int D, int E, int SIG>
static hipError_t launch_one(const LowdCutoffArgs<real>& args, dim3 grid, hipStream_t stream, const char** kernel_name) {
  hipLaunchKernelGGL((lowd_cutoff_grad_kernel<KERNEL, D, E, SIG, real>), grid, dim3(BLOCK_THREADS), 0, stream, args);
  if (kernel_name) *kernel_name = "lowd_cutoff_grad_kernel";
  return hipGetLastError();
}

template <int KERNEL, int D>
static hipError_t launch_e(int E, int sig, const LowdCutoffArgs<real>& args, dim3 grid, hipStream_t stream, const char** kernel_name) {
  if (sig == SIG_DENSITY) return launch_one<KERNEL, D, 1, SIG_DENSITY>(args, grid, stream, kernel_name);
  switch (E) {
    case 1: return launch_one<KERNEL, D, 1, SIG_PRODUCT>(args, grid, stream, kernel_name);
    case 2: return launch_one<KERNEL, D, 2, SIG_PRODUCT>(args, grid, stream, kernel_name);
    case 3: return launch_one<KERNEL, D, 3, SIG_PRODUCT>(args, grid, stream, kernel_name);
    case 4: return launch_one<KERNEL, D, 4, SIG_PRODUCT>(args, grid, stream, kernel_name);
    default: return hipErrorInvalidValue;
  }
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
  if (sig != SIG_PRODUCT && sig != SIG_DENSITY) return hipErrorInvalidValue;
  switch (kernel) {
#if KMVP_WENDLAND
    case K_WENDLAND_C2: return launch_d<K_WENDLAND_C2>(D, E, sig, args, grid, stream, kernel_name);
    case K_WENDLAND_C4: return launch_d<K_WENDLAND_C4>(D, E, sig, args, grid, stream, kernel_name);
#else
    case K_GAUSSIAN: return launch_d<K_GAUSSIAN>(D, E, sig, args, grid, stream, kernel_name);
    case K_ABSEXP: return launch_d<K_ABSEXP>(D, E, sig, args, grid, stream, kernel_name);
    case K_MATERN32: return launch_d<K_MATERN32>(D, E, sig, args, grid, stream, kernel_name);
    case K_MATERN52: return launch_d<K_MATERN52>(D, E, sig, args, grid, stream, kernel_name);
#endif
    default: return hipErrorInvalidValue;
  }
}

}  // namespace kmvp
