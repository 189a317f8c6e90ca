// Instantiations of DBSCAN's pair loops (kmvp_lowd_cutoff_label.hpp) for ONE precision.
// Compiled twice (see Makefile):
//   -DKMVP_REAL={float,double}  -DKMVP_FN=launch_lowd_cutoff_label_<p>
// lowd_cutoff_label_kernel: one variant per (D, MODE), D = 1 .. CUTOFF_MAX_D, MODE = LABEL_SWEEP, LABEL_BORDER.
#include "kmvp_internal.hpp"
#include "kmvp_lowd_cutoff_label.hpp"

#if !defined(KMVP_REAL) || !defined(KMVP_FN)
#error "KMVP_REAL and KMVP_FN must be defined"
#endif

namespace kmvp {

using real = KMVP_REAL;

template <int D, int MODE>
static hipError_t launch_one(const LowdCutoffLabelArgs<real>& args, dim3 grid, hipStream_t stream, const char** kernel_name) {
  hipLaunchKernelGGL((lowd_cutoff_label_kernel<D, MODE, real>), grid, dim3(BLOCK_THREADS), 0, stream, args);
  if (kernel_name) *kernel_name = "lowd_cutoff_label_kernel";
  return hipGetLastError();
}

template <int D>
static hipError_t launch_mode(int mode, const LowdCutoffLabelArgs<real>& args, dim3 grid, hipStream_t stream, const char** kernel_name) {
  switch (mode) {
    case LABEL_SWEEP: return launch_one<D, LABEL_SWEEP>(args, grid, stream, kernel_name);
    case LABEL_BORDER: return launch_one<D, LABEL_BORDER>(args, grid, stream, kernel_name);
    default: return hipErrorInvalidValue;
  }
}

hipError_t KMVP_FN(int D, int mode, const LowdCutoffLabelArgs<real>& args, dim3 grid, hipStream_t stream, const char** kernel_name) {
  switch (D) {
    case 1: return launch_mode<1>(mode, args, grid, stream, kernel_name);
    case 2: return launch_mode<2>(mode, args, grid, stream, kernel_name);
    case 3: return launch_mode<3>(mode, args, grid, stream, kernel_name);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace kmvp
