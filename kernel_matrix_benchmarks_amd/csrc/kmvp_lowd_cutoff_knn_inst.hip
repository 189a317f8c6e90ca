// Instantiations of the radius search's kernel (kmvp_lowd_cutoff_knn.hpp) for ONE precision.
// Compiled twice (see Makefile):
//   -DKMVP_REAL={float,double}  -DKMVP_FN=launch_lowd_cutoff_knn_<p>
// lowd_cutoff_knn_kernel: one variant per (D, KT), D = 1 .. CUTOFF_MAX_D, list capacities KT = 1, 4, 16.
#include "kmvp_internal.hpp"
#include "kmvp_lowd_cutoff_knn.hpp"

#if !defined(KMVP_REAL) || !defined(KMVP_FN)
#error "KMVP_REAL and KMVP_FN must be defined"
#endif

namespace kmvp {

using real = KMVP_REAL;

template <int D, int KT>
static hipError_t launch_one(const LowdCutoffArgs<real>& args, dim3 grid, hipStream_t stream, const char** kernel_name) {
  hipLaunchKernelGGL((lowd_cutoff_knn_kernel<D, KT, real>), grid, dim3(BLOCK_THREADS), 0, stream, args);
  if (kernel_name) *kernel_name = "lowd_cutoff_knn_kernel";
  return hipGetLastError();
}

template <int D>
static hipError_t launch_kt(int KT, const LowdCutoffArgs<real>& args, dim3 grid, hipStream_t stream, const char** kernel_name) {
  switch (KT) {
    case 1: return launch_one<D, 1>(args, grid, stream, kernel_name);
    case 4: return launch_one<D, 4>(args, grid, stream, kernel_name);
    case 16: return launch_one<D, 16>(args, grid, stream, kernel_name);
    default: return hipErrorInvalidValue;
  }
}

hipError_t KMVP_FN(int D, int KT, const LowdCutoffArgs<real>& args, dim3 grid, hipStream_t stream, const char** kernel_name) {
  switch (D) {
    case 1: return launch_kt<1>(KT, args, grid, stream, kernel_name);
    case 2: return launch_kt<2>(KT, args, grid, stream, kernel_name);
    case 3: return launch_kt<3>(KT, args, grid, stream, kernel_name);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace kmvp
