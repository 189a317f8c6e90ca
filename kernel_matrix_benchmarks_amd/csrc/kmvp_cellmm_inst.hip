// Instantiations of cellmm_kernel / cellmm16_kernel (kmvp_cellmm.hpp): TT = target tiles of 32 per wave.
#include <stdlib.h>
#include "kmvp_internal.hpp"
#include "kmvp_cellmm.hpp"

namespace kmvp {

// diagnostic: KMVP_DBG_LDS=<bytes> of unused dynamic LDS per workgroup lowers the number of resident workgroups per CU
// (tools/cellmm_occupancy.py: what a third wave per SIMD is worth to this loop)
static size_t cmm_dbg_lds() {
  static const size_t v = getenv("KMVP_DBG_LDS") ? (size_t)atol(getenv("KMVP_DBG_LDS")) : 0;
  return v;
}
template <typename K, typename... Rest>
static void cmm_launch(K kernel, const CellmmArgs& args, dim3 grid, hipStream_t stream, Rest... rest) {
  if (cmm_dbg_lds()) (void)hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)cmm_dbg_lds());
  hipLaunchKernelGGL(kernel, grid, dim3(BLOCK_THREADS), cmm_dbg_lds(), stream, args, rest...);
}

hipError_t launch_cellmm_gaussian(int TT, int shape, const CellmmArgs& args, dim3 grid, hipStream_t stream, const char** kernel_name) {
  if (kernel_name) *kernel_name = shape == 1 ? "cellmm16_kernel" : "cellmm_kernel";  // the names the profiler shows
  if (shape == 1) {  // one list alone: every workgroup is below main_grid
    const int all = (int)grid.x;
    switch (TT) {
      case 1: cmm_launch(cellmm16_kernel<1>, args, grid, stream, args, all, args, 0); break;
      case 2: cmm_launch(cellmm16_kernel<2>, args, grid, stream, args, all, args, 0); break;
      case 4: cmm_launch(cellmm16_kernel<4>, args, grid, stream, args, all, args, 0); break;
      case 8: cmm_launch(cellmm16_kernel<8>, args, grid, stream, args, all, args, 0); break;
      default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
  }
  switch (TT) {
    case 1: cmm_launch(cellmm_kernel<1>, args, grid, stream); break;
    case 2: cmm_launch(cellmm_kernel<2>, args, grid, stream); break;
    case 4: cmm_launch(cellmm_kernel<4>, args, grid, stream); break;
    case 8: cmm_launch(cellmm_kernel<8>, args, grid, stream); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_cellmm16_fused(int TT, const CellmmArgs& main, const CellmmArgs& rest, const CellmmArgs& tail, int64_t main_grid,
                                 int64_t tail_grid, int64_t rest_grid, hipStream_t stream, const char** kernel_name) {
  if (kernel_name) *kernel_name = "cellmm16_kernel";
  if (main_grid + tail_grid + rest_grid > MAX_GRID) return hipErrorInvalidConfiguration;
#if CMM16_WHOLE_ROUNDS
  const dim3 grid((unsigned)main_grid);
#else
  const dim3 grid((unsigned)(main_grid + tail_grid + rest_grid));
#endif
  switch (TT) {  // TT > CELL_REST_TT: the kernels that hold the second body
    case 4: cmm_launch(cellmm16_kernel<4>, main, grid, stream, rest, (int)main_grid, tail, (int)tail_grid); break;
    case 8: cmm_launch(cellmm16_kernel<8>, main, grid, stream, rest, (int)main_grid, tail, (int)tail_grid); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace kmvp
