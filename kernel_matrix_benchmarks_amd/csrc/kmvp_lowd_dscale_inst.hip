// Instantiations of the length-scale-derivative pair-loop kernel (kmvp_lowd_dscale.hpp) for ONE kernel function and ONE
// precision.  Compiled eight times (see Makefile), as kmvp_lowd_grad_inst.hip:
//   -DKMVP_KERNEL={0,1,5,6}  -DKMVP_REAL={float,double}  -DKMVP_FN=launch_lowd_dscale_<k>_<p>
// One variant per (D, E): D = 1 .. LOWD_MAX_D, E = 1 .. LOWD_MAX_E and density mode.
#include "kmvp_internal.hpp"
#include "kmvp_lowd_dscale.hpp"

#ifndef KMVP_KERNEL
#error "KMVP_KERNEL, KMVP_REAL and KMVP_FN must be defined"
#endif

namespace kmvp {

using real = KMVP_REAL;
constexpr int KERNEL = KMVP_KERNEL;

template <int D, int E, int SIG>
static hipError_t launch_one(const LowdArgs<real>& args, dim3 grid, hipStream_t stream, const char** kernel_name) {
  hipLaunchKernelGGL((lowd_dscale_kernel<KERNEL, D, E, SIG, real>), grid, dim3(BLOCK_THREADS), 0, stream, args);
  if (kernel_name) *kernel_name = "lowd_dscale_kernel";
  return hipGetLastError();
}

template <int D>
static hipError_t launch_e(int E, int sig, const LowdArgs<real>& args, dim3 grid, hipStream_t stream,
                           const char** kernel_name) {
  if (sig == SIG_DENSITY) return launch_one<D, 1, SIG_DENSITY>(args, grid, stream, kernel_name);
  if (sig != SIG_PRODUCT) return hipErrorInvalidValue;
  switch (E) {
    case 1: return launch_one<D, 1, SIG_PRODUCT>(args, grid, stream, kernel_name);
    case 2: return launch_one<D, 2, SIG_PRODUCT>(args, grid, stream, kernel_name);
    case 3: return launch_one<D, 3, SIG_PRODUCT>(args, grid, stream, kernel_name);
    case 4: return launch_one<D, 4, SIG_PRODUCT>(args, grid, stream, kernel_name);
    default: return hipErrorInvalidValue;
  }
}

hipError_t KMVP_FN(int D, int E, int sig, const LowdArgs<real>& args, dim3 grid, hipStream_t stream,
                   const char** kernel_name) {
  switch (D) {
    case 1: return launch_e<1>(E, sig, args, grid, stream, kernel_name);
    case 2: return launch_e<2>(E, sig, args, grid, stream, kernel_name);
    case 3: return launch_e<3>(E, sig, args, grid, stream, kernel_name);
    case 4: return launch_e<4>(E, sig, args, grid, stream, kernel_name);
    case 5: return launch_e<5>(E, sig, args, grid, stream, kernel_name);
    case 6: return launch_e<6>(E, sig, args, grid, stream, kernel_name);
    case 7: return launch_e<7>(E, sig, args, grid, stream, kernel_name);
    case 8: return launch_e<8>(E, sig, args, grid, stream, kernel_name);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace kmvp
