// Instantiations of the K-nearest-neighbour pair-loop kernel (kmvp_lowd_knn.hpp) for ONE precision.
// Compiled twice (see Makefile):
//   -DKMVP_REAL={float,double}  -DKMVP_FN=launch_lowd_knn_<p>
// One variant per (D, KT): D = 1 .. LOWD_MAX_D, list capacities KT = 1, 4, 16.
#include "kmvp_internal.hpp"
#include "kmvp_lowd_knn.hpp"

#ifndef KMVP_REAL
#error "KMVP_REAL and KMVP_FN must be defined"
#endif

namespace kmvp {

using real = KMVP_REAL;

template <int D, int KT>
static hipError_t launch_one(const LowdArgs<real>& args, dim3 grid, hipStream_t stream, const char** kernel_name) {
  hipLaunchKernelGGL((lowd_knn_kernel<D, KT, real>), grid, dim3(BLOCK_THREADS), 0, stream, args);
  if (kernel_name) *kernel_name = "lowd_knn_kernel";
  return hipGetLastError();
}

template <int D>
static hipError_t launch_kt(int KT, const LowdArgs<real>& args, dim3 grid, hipStream_t stream, const char** kernel_name) {
  switch (KT) {
    case 1: return launch_one<D, 1>(args, grid, stream, kernel_name);
    case 4: return launch_one<D, 4>(args, grid, stream, kernel_name);
    case 16: return launch_one<D, 16>(args, grid, stream, kernel_name);
    default: return hipErrorInvalidValue;
  }
}

hipError_t KMVP_FN(int D, int KT, const LowdArgs<real>& args, dim3 grid, hipStream_t stream, const char** kernel_name) {
  switch (D) {
    case 1: return launch_kt<1>(KT, args, grid, stream, kernel_name);
    case 2: return launch_kt<2>(KT, args, grid, stream, kernel_name);
    case 3: return launch_kt<3>(KT, args, grid, stream, kernel_name);
    case 4: return launch_kt<4>(KT, args, grid, stream, kernel_name);
    case 5: return launch_kt<5>(KT, args, grid, stream, kernel_name);
    case 6: return launch_kt<6>(KT, args, grid, stream, kernel_name);
    case 7: return launch_kt<7>(KT, args, grid, stream, kernel_name);
    case 8: return launch_kt<8>(KT, args, grid, stream, kernel_name);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace kmvp
