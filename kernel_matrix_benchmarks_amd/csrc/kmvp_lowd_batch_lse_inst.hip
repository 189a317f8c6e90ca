// Instantiations of the batched log-sum-exp pair loop (kmvp_lowd_batch_lse.hpp) for ONE precision.
// Compiled twice (see Makefile):  -DKMVP_REAL={float,double}  -DKMVP_FN=launch_lowd_batch_lse_<p>
// What the batched Sinkhorn solve uses: the Gaussian and exp(-r), D = 1 .. LOWD_MAX_D, E = 1, SIG_PRODUCT.  The template
// itself is general in E and SIG.
#include "kmvp_internal.hpp"
#include "kmvp_lowd_batch_lse.hpp"

#if !defined(KMVP_REAL) || !defined(KMVP_FN)
#error "KMVP_REAL and KMVP_FN must be defined"
#endif

namespace kmvp {

using real = KMVP_REAL;

template <int KERNEL, int D>
static hipError_t launch_one(const LowdBatchLseArgs<real>& args, dim3 grid, hipStream_t stream, const char** kernel_name) {
  hipLaunchKernelGGL((lowd_batch_lse_kernel<KERNEL, D, 1, SIG_PRODUCT, real>), grid, dim3(BLOCK_THREADS), 0, stream, args);
  if (kernel_name) *kernel_name = "lowd_batch_lse_kernel";
  return hipGetLastError();
}

template <int KERNEL>
static hipError_t launch_d(int D, const LowdBatchLseArgs<real>& args, dim3 grid, hipStream_t stream, const char** kernel_name) {
  switch (D) {
    case 1: return launch_one<KERNEL, 1>(args, grid, stream, kernel_name);
    case 2: return launch_one<KERNEL, 2>(args, grid, stream, kernel_name);
    case 3: return launch_one<KERNEL, 3>(args, grid, stream, kernel_name);
    case 4: return launch_one<KERNEL, 4>(args, grid, stream, kernel_name);
    case 5: return launch_one<KERNEL, 5>(args, grid, stream, kernel_name);
    case 6: return launch_one<KERNEL, 6>(args, grid, stream, kernel_name);
    case 7: return launch_one<KERNEL, 7>(args, grid, stream, kernel_name);
    case 8: return launch_one<KERNEL, 8>(args, grid, stream, kernel_name);
    default: return hipErrorInvalidValue;
  }
}

hipError_t KMVP_FN(int kernel, int D, int E, int sig, const LowdBatchLseArgs<real>& args, dim3 grid, hipStream_t stream,
                   const char** kernel_name) {
  if (E != 1 || sig != SIG_PRODUCT) return hipErrorInvalidValue;
  switch (kernel) {
    case K_GAUSSIAN: return launch_d<K_GAUSSIAN>(D, args, grid, stream, kernel_name);
    case K_ABSEXP: return launch_d<K_ABSEXP>(D, args, grid, stream, kernel_name);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace kmvp
