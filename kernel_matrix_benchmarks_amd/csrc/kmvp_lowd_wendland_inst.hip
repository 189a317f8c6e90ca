// Instantiations of lowd_cutoff_kernel (kmvp_lowd_cutoff.hpp) with Wendland's compactly supported kernels, for ONE precision.
// Compiled twice (see Makefile):  -DKMVP_REAL={float,double}  -DKMVP_FN=launch_lowd_wendland_<p>
// K_WENDLAND_C2 and K_WENDLAND_C4, D = 1 .. CUTOFF_MAX_D, the product and normalised rows at E = 1 .. LOWD_MAX_E, density --
// the shapes of kmvp_lowd_cutoff_inst.hip, in a unit of their own so that the two compile side by side.
#include "kmvp_internal.hpp"
#include "kmvp_lowd_cutoff.hpp"

#if !defined(KMVP_REAL) || !defined(KMVP_FN)
#error "KMVP_REAL and KMVP_FN must be defined"
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
    case K_WENDLAND_C2: return launch_d<K_WENDLAND_C2>(D, E, sig, args, grid, stream, kernel_name);
    case K_WENDLAND_C4: return launch_d<K_WENDLAND_C4>(D, E, sig, args, grid, stream, kernel_name);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace kmvp
