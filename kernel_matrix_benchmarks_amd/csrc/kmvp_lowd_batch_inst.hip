// Instantiations of the batched pair-loop kernels (kmvp_lowd_batch.hpp) for ONE precision.
// Compiled twice (see Makefile):
//   -DKMVP_REAL={float,double}  -DKMVP_FN=launch_lowd_batch_<p>  -DKMVP_FN_KNN=launch_lowd_batch_knn_<p>
// lowd_batch_kernel: the Gaussian, exp(-r) and the two Matern kernels, D = 1 .. LOWD_MAX_D, the product and normalised rows
// at E = 1 .. LOWD_MAX_E, density.  lowd_batch_knn_kernel: one variant per (D, KT), list capacities KT = 1, 4, 16.
#include "kmvp_internal.hpp"
#include "kmvp_lowd_batch.hpp"

#if !defined(KMVP_REAL) || !defined(KMVP_FN) || !defined(KMVP_FN_KNN)
#error "KMVP_REAL, KMVP_FN and KMVP_FN_KNN must be defined"
#endif

namespace kmvp {

using real = KMVP_REAL;

template <int KERNEL, int D, int E, int SIG>
static hipError_t launch_one(const LowdBatchArgs<real>& args, dim3 grid, hipStream_t stream, const char** kernel_name) {
  hipLaunchKernelGGL((lowd_batch_kernel<KERNEL, D, E, SIG, real>), grid, dim3(BLOCK_THREADS), 0, stream, args);
  if (kernel_name) *kernel_name = "lowd_batch_kernel";
  return hipGetLastError();
}

template <int KERNEL, int D>
static hipError_t launch_e(int E, int sig, const LowdBatchArgs<real>& args, dim3 grid, hipStream_t stream, const char** kernel_name) {
  if (sig == SIG_DENSITY) return launch_one<KERNEL, D, 1, SIG_DENSITY>(args, grid, stream, kernel_name);
#define KMVP_BATCH_E(EV)                                                                                     \
  case EV:                                                                                                   \
    return sig == SIG_NORM ? launch_one<KERNEL, D, EV, SIG_NORM>(args, grid, stream, kernel_name)            \
                           : launch_one<KERNEL, D, EV, SIG_PRODUCT>(args, grid, stream, kernel_name);
  switch (E) {
    KMVP_BATCH_E(1)
    KMVP_BATCH_E(2)
    KMVP_BATCH_E(3)
    KMVP_BATCH_E(4)
    default: return hipErrorInvalidValue;
  }
#undef KMVP_BATCH_E
}

template <int KERNEL>
static hipError_t launch_d(int D, int E, int sig, const LowdBatchArgs<real>& args, dim3 grid, hipStream_t stream,
                           const char** kernel_name) {
  switch (D) {
    case 1: return launch_e<KERNEL, 1>(E, sig, args, grid, stream, kernel_name);
    case 2: return launch_e<KERNEL, 2>(E, sig, args, grid, stream, kernel_name);
    case 3: return launch_e<KERNEL, 3>(E, sig, args, grid, stream, kernel_name);
    case 4: return launch_e<KERNEL, 4>(E, sig, args, grid, stream, kernel_name);
    case 5: return launch_e<KERNEL, 5>(E, sig, args, grid, stream, kernel_name);
    case 6: return launch_e<KERNEL, 6>(E, sig, args, grid, stream, kernel_name);
    case 7: return launch_e<KERNEL, 7>(E, sig, args, grid, stream, kernel_name);
    case 8: return launch_e<KERNEL, 8>(E, sig, args, grid, stream, kernel_name);
    default: return hipErrorInvalidValue;
  }
}

hipError_t KMVP_FN(int kernel, int D, int E, int sig, const LowdBatchArgs<real>& args, dim3 grid, hipStream_t stream,
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

template <int D, int KT>
static hipError_t launch_knn_one(const LowdBatchArgs<real>& args, dim3 grid, hipStream_t stream, const char** kernel_name) {
  hipLaunchKernelGGL((lowd_batch_knn_kernel<D, KT, real>), grid, dim3(BLOCK_THREADS), 0, stream, args);
  if (kernel_name) *kernel_name = "lowd_batch_knn_kernel";
  return hipGetLastError();
}

template <int D>
static hipError_t launch_knn_kt(int KT, const LowdBatchArgs<real>& args, dim3 grid, hipStream_t stream, const char** kernel_name) {
  switch (KT) {
    case 1: return launch_knn_one<D, 1>(args, grid, stream, kernel_name);
    case 4: return launch_knn_one<D, 4>(args, grid, stream, kernel_name);
    case 16: return launch_knn_one<D, 16>(args, grid, stream, kernel_name);
    default: return hipErrorInvalidValue;
  }
}

hipError_t KMVP_FN_KNN(int D, int KT, const LowdBatchArgs<real>& args, dim3 grid, hipStream_t stream, const char** kernel_name) {
  switch (D) {
    case 1: return launch_knn_kt<1>(KT, args, grid, stream, kernel_name);
    case 2: return launch_knn_kt<2>(KT, args, grid, stream, kernel_name);
    case 3: return launch_knn_kt<3>(KT, args, grid, stream, kernel_name);
    case 4: return launch_knn_kt<4>(KT, args, grid, stream, kernel_name);
    case 5: return launch_knn_kt<5>(KT, args, grid, stream, kernel_name);
    case 6: return launch_knn_kt<6>(KT, args, grid, stream, kernel_name);
    case 7: return launch_knn_kt<7>(KT, args, grid, stream, kernel_name);
    case 8: return launch_knn_kt<8>(KT, args, grid, stream, kernel_name);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace kmvp
