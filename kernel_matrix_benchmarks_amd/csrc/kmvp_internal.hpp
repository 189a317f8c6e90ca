// Host-side declarations shared by the translation units of libkmvp.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kmvp_knn_merge.hpp"
#include "kmvp_lowd.hpp"

namespace kmvp {

// Tuning of a specialised low-D launch (host-side choice, compile-time in the kernel).
struct LowdTuning {
  int targets_per_lane;  // T
  int feed;              // 0 scalar-cache stream, 1 LDS tiles
};

// Largest shapes the specialised kernels are instantiated for; anything else goes
// to lowd_mid_kernel / lowd_big_kernel (or to the MFMA path for bf16).
constexpr int LOWD_MAX_D = 8;
constexpr int LOWD_MAX_E = 4;

// defaults, from the sweep on MI355X (profiles/): one target per lane, LDS-staged tiles
constexpr int DEFAULT_TARGETS_PER_LANE = 1;
constexpr int DEFAULT_FEED = 1;

// Returns hipErrorInvalidValue when (D, E, sig, tuning) has no instantiation.
// One function per kernel x precision: each lives in its own translation unit
// (kmvp_lowd_inst.hip compiled with -DKMVP_KERNEL / -DKMVP_REAL) and contains no
// kernel-selection branch in device code.
#define KMVP_DECLARE_LOWD(NAME, REAL)                                                           \
  hipError_t NAME(int D, int E, int sig, LowdTuning tune, const LowdArgs<REAL>& args, dim3 grid, \
                  hipStream_t stream, const char** kernel_name);                                \
  hipError_t NAME##_generic(int sig, const REAL* x, const REAL* y, const REAL* b, double* part,  \
                            int64_t n, int64_t n_pad, int64_t m, int D, int E, int NE,           \
                            int segments, int64_t seg_len, int64_t j_offset, int64_t m_total,    \
                            hipStream_t stream, const char** kernel_name);

KMVP_DECLARE_LOWD(launch_lowd_gaussian_f32, float)
KMVP_DECLARE_LOWD(launch_lowd_absexp_f32, float)
KMVP_DECLARE_LOWD(launch_lowd_invdist_f32, float)
KMVP_DECLARE_LOWD(launch_lowd_gaussian_f64, double)
KMVP_DECLARE_LOWD(launch_lowd_absexp_f64, double)
KMVP_DECLARE_LOWD(launch_lowd_invdist_f64, double)
KMVP_DECLARE_LOWD(launch_lowd_matern32_f32, float)
KMVP_DECLARE_LOWD(launch_lowd_matern52_f32, float)
KMVP_DECLARE_LOWD(launch_lowd_matern32_f64, double)
KMVP_DECLARE_LOWD(launch_lowd_matern52_f64, double)

// Gradient with respect to the targets (kmvp_lowd_grad.hpp; kmvp_lowd_grad_inst.hip, one unit per kernel x precision):
// D <= LOWD_MAX_D, E <= LOWD_MAX_E, sig SIG_PRODUCT or SIG_DENSITY; hipErrorInvalidValue otherwise.
#define KMVP_DECLARE_LOWD_GRAD(NAME, REAL)                                                                    \
  hipError_t NAME(int D, int E, int sig, const LowdArgs<REAL>& args, dim3 grid, hipStream_t stream, \
                  const char** kernel_name);
KMVP_DECLARE_LOWD_GRAD(launch_lowd_grad_gaussian_f32, float)
KMVP_DECLARE_LOWD_GRAD(launch_lowd_grad_absexp_f32, float)
KMVP_DECLARE_LOWD_GRAD(launch_lowd_grad_invdist_f32, float)
KMVP_DECLARE_LOWD_GRAD(launch_lowd_grad_gaussian_f64, double)
KMVP_DECLARE_LOWD_GRAD(launch_lowd_grad_absexp_f64, double)
KMVP_DECLARE_LOWD_GRAD(launch_lowd_grad_invdist_f64, double)
KMVP_DECLARE_LOWD_GRAD(launch_lowd_grad_matern32_f32, float)
KMVP_DECLARE_LOWD_GRAD(launch_lowd_grad_matern52_f32, float)
KMVP_DECLARE_LOWD_GRAD(launch_lowd_grad_matern32_f64, double)
KMVP_DECLARE_LOWD_GRAD(launch_lowd_grad_matern52_f64, double)

// Derivative in the logarithm of a per-axis length scale (kmvp_lowd_dscale.hpp; kmvp_lowd_dscale_inst.hip): the
// gradient's signature, shapes and partial sums; no 1/r.
KMVP_DECLARE_LOWD_GRAD(launch_lowd_dscale_gaussian_f32, float)
KMVP_DECLARE_LOWD_GRAD(launch_lowd_dscale_absexp_f32, float)
KMVP_DECLARE_LOWD_GRAD(launch_lowd_dscale_gaussian_f64, double)
KMVP_DECLARE_LOWD_GRAD(launch_lowd_dscale_absexp_f64, double)
KMVP_DECLARE_LOWD_GRAD(launch_lowd_dscale_matern32_f32, float)
KMVP_DECLARE_LOWD_GRAD(launch_lowd_dscale_matern52_f32, float)
KMVP_DECLARE_LOWD_GRAD(launch_lowd_dscale_matern32_f64, double)
KMVP_DECLARE_LOWD_GRAD(launch_lowd_dscale_matern52_f64, double)

// Log-sum-exp reduction (kmvp_lowd_lse.hpp; kmvp_lowd_lse_inst.hip, one unit per kernel x precision): the Gaussian and
// exp(-r), D <= LOWD_MAX_D, E <= LOWD_MAX_E, sig SIG_PRODUCT or SIG_DENSITY; hipErrorInvalidValue otherwise.
// args.part: [segments][2 NC][n_pad] -- NC columns of sums, then NC columns of exponents.
#define KMVP_DECLARE_LOWD_LSE(NAME, REAL)                                                            \
  hipError_t NAME(int D, int E, int sig, const LowdArgs<REAL>& args, dim3 grid, hipStream_t stream, \
                  const char** kernel_name);
KMVP_DECLARE_LOWD_LSE(launch_lowd_lse_gaussian_f32, float)
KMVP_DECLARE_LOWD_LSE(launch_lowd_lse_absexp_f32, float)
KMVP_DECLARE_LOWD_LSE(launch_lowd_lse_gaussian_f64, double)
KMVP_DECLARE_LOWD_LSE(launch_lowd_lse_absexp_f64, double)

// What the log-sum-exp (kmvp_product.hip run_logsumexp_t) and the Sinkhorn iteration on top of it (kmvp_sinkhorn.hip) share
// on the host side: the launch switch, the launch geometry and the segment merge.
inline hipError_t launch_lowd_lse(int kernel, int D, int E, int sig, const LowdArgs<float>& args, dim3 grid, hipStream_t s,
                                  const char** name) {
  switch (kernel) {
    case K_GAUSSIAN: return launch_lowd_lse_gaussian_f32(D, E, sig, args, grid, s, name);
    case K_ABSEXP: return launch_lowd_lse_absexp_f32(D, E, sig, args, grid, s, name);
    default: return hipErrorInvalidValue;
  }
}
inline hipError_t launch_lowd_lse(int kernel, int D, int E, int sig, const LowdArgs<double>& args, dim3 grid, hipStream_t s,
                                  const char** name) {
  switch (kernel) {
    case K_GAUSSIAN: return launch_lowd_lse_gaussian_f64(D, E, sig, args, grid, s, name);
    case K_ABSEXP: return launch_lowd_lse_absexp_f64(D, E, sig, args, grid, s, name);
    default: return hipErrorInvalidValue;
  }
}

// Geometry of the specialised difference-form kernels (kmvp_lowd.hpp) for N targets and M sources: tiles of 64 T targets
// per wave, source records of R reals in batches, segments of whole batches, `cols` columns of partial sums per segment.
// Everything but the buffers.  opt_segments / opt_chunk: the context's "segments" and "chunk" options.
constexpr int64_t LOWD_BATCH = 8;  // two ping-pong batches of 4 records
template <typename real>
LowdArgs<real> lowd_geometry(int64_t N, int64_t M, int opt_segments, int opt_chunk, int64_t j_offset, int64_t m_total, int T,
                             int R, int cols) {
  const int64_t tile = 64 * (int64_t)T * WAVES_PER_BLOCK;
  LowdArgs<real> a;
  a.xs = nullptr;
  a.rec = nullptr;
  a.part = nullptr;
  a.n = N;
  a.n_pad = round_up(N > 1 ? N : 1, tile);
  a.tile_blocks = (int)(a.n_pad / tile);
  a.m_pad = round_up(M > 1 ? M : 1, LOWD_BATCH);
  // few targets: short segments, so that the launch still covers the chip (n = 2000, fp64: 121 -> 9 us)
  const bool small = small_problem(N);
  SegmentRule rule((int64_t)R * sizeof(real), cols);
  rule.min_seg = small ? 32 : 1024;
  rule.small = small;
  const int segments = choose_segments(opt_segments, a.n_pad / tile, a.m_pad, a.n_pad, rule);
  a.seg_len = round_up((a.m_pad + segments - 1) / segments, LOWD_BATCH);
  a.segments = (int)((a.m_pad + a.seg_len - 1) / a.seg_len);
  a.chunk = (int)round_up(opt_chunk > 8 ? opt_chunk : 8, LOWD_BATCH);
  a.j_offset = j_offset;
  a.m_total = m_total;
  a.m = M;
  return a;
}

// The segment merge of lowd_lse_kernel's (sum, exponent) pairs, reduce_shifted_kernel's arithmetic with fp64 exponents per
// (column, target) q < count:
//   K_q = min_s k[s][q],   sums[q] = sum_s part[s][q] 2^(K_q - k[s][q])   (index order; every factor <= 1 and exact)
// (static: a kernel cannot be inline; each of the two units that launch it carries its own copy, the others none)
static __global__ void lse_reduce_kernel(const double* __restrict__ part, double* __restrict__ sums, double* __restrict__ kmin,
                                         int64_t count /* NC * n_pad */, int segments) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= count) return;
  double K = INFINITY;
  for (int s = 0; s < segments; ++s) K = fmin(K, part[((int64_t)2 * s + 1) * count + q]);
  double v = 0.0;
  for (int s = 0; s < segments; ++s) {
    const double ks = part[((int64_t)2 * s + 1) * count + q];
    if (ks < INFINITY) v += ldexp(part[(int64_t)2 * s * count + q], (int)fmax(K - ks, -100000.0));
  }
  sums[q] = v;
  kmin[q] = K;
}

// K nearest neighbours (kmvp_lowd_knn.hpp; kmvp_lowd_knn_inst.hip, one unit per precision): D <= LOWD_MAX_D, list capacity
// KT = 1, 4 or 16; hipErrorInvalidValue otherwise.  args.part: [segments][2 KT][n_pad] -- KT rows of squared distances, then
// KT rows of global source indices.
hipError_t launch_lowd_knn_f32(int D, int KT, const LowdArgs<float>& args, dim3 grid, hipStream_t stream, const char** kernel_name);
hipError_t launch_lowd_knn_f64(int D, int KT, const LowdArgs<double>& args, dim3 grid, hipStream_t stream, const char** kernel_name);
inline hipError_t launch_lowd_knn(int D, int KT, const LowdArgs<float>& args, dim3 grid, hipStream_t s, const char** name) {
  return launch_lowd_knn_f32(D, KT, args, grid, s, name);
}
inline hipError_t launch_lowd_knn(int D, int KT, const LowdArgs<double>& args, dim3 grid, hipStream_t s, const char** name) {
  return launch_lowd_knn_f64(D, KT, args, grid, s, name);
}
// Smallest instantiated list capacity that holds `need` candidates (need <= 16).
inline int knn_capacity(int need) { return need <= 1 ? 1 : need <= 4 ? 4 : 16; }
// Source segments of a nearest-neighbour launch; 0: the product's own rule (choose_segments).  Every segment starts from
// an empty list, and a wave enters the insertion code whenever any of its 64 lanes improves -- at KT = 16 almost every
// batch of a segment's first ~4000 sources -- so a short segment costs far more here than in the product, whose segments
// exist for L2 residency and for many rounds of workgroups.  Measured at N = M = 2e5, D = 3, float32 (LAB_NOTES.md
// section 21): KT = 16 takes 23.5 / 24.5 / 27.6 / 30.5 / 40.8 / 54.8 ms with 1 / 2 / 3 / 4 / 8 / 16 segments, KT = 1 takes
// 13.1 / 11.0 / 10.3 / 10.1 / 9.5 / 9.3 ms.  Hence: the short lists, whose insertion costs next to nothing, take the
// product's rule; KT = 16 takes only as many segments as two workgroups per CU ask for (none where the target tiles alone
// cover the device), none shorter than 4096 sources, within the product's bound on the partial-result buffer.
// opt_segments > 0 (the "segments" option) holds.
constexpr int64_t KNN_MIN_SEGMENT = 4096;
inline int knn_segments(int opt_segments, int KT, int64_t tile_blocks, int64_t m_pad, int64_t n_pad) {
  if (opt_segments > 0) return opt_segments;
  if (KT <= 4) return 0;
  const int64_t for_parallelism = (512 + tile_blocks - 1) / tile_blocks;
  const int64_t cap_len = std::max<int64_t>(1, m_pad / KNN_MIN_SEGMENT);
  const int64_t cap_mem = std::max<int64_t>(1, (int64_t)(4e9 / (2.0 * KT * n_pad * 8)));
  return (int)std::max<int64_t>(1, std::min(for_parallelism, std::min(cap_len, cap_mem)));
}
// The segment merge (kmvp_knn_merge.hpp): S lists of KT candidates per target, [list][2 KT][elem_stride], into the Kc
// smallest in the canonical unpadded layout cand[2 Kc][n] -- distances in rows 0 .. Kc - 1, indices behind them.  What
// kmvp_nearest (kmvp_product.hip) and the k-means iteration on top of it (kmvp_kmeans.hip) share.
// (static: a kernel cannot be inline; each of the two units that launch it carries its own copy, the others none)
static __global__ void knn_merge_kernel(const double* __restrict__ lists, double* __restrict__ cand, int64_t n, int64_t list_stride,
                                        int64_t elem_stride, int S, int KT, int Kc) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  knn_merge(lists + i, list_stride, elem_stride, S, KT, Kc, cand + i, cand + (int64_t)Kc * n + i, n);
}

// Last step of kmvp_nearest, plain (kmvp_product.hip) and batched (kmvp_batch.hip): cand [2 Kc][n] (modified in place by the exclude-self drop) -> idx (n, K) int64, sqdist (n, K) float64
// (static: a kernel cannot be inline; each of the two units that launch it carries its own copy, the others none)
static __global__ void knn_finish_kernel(double* __restrict__ cand, int64_t* __restrict__ idx, double* __restrict__ sqdist,
                                         int64_t n, int K, int exclude_self) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int Kc = K + (exclude_self ? 1 : 0);
  double* s = cand + i;
  double* j = cand + (int64_t)Kc * n + i;
  if (exclude_self) knn_drop_self(s, j, n, Kc, i);
  for (int k = 0; k < K; ++k) {
    sqdist[i * K + k] = s[(int64_t)k * n];
    idx[i * K + k] = (int64_t)j[(int64_t)k * n];
  }
}

// Gradient of the log-sum-exp with respect to the targets (kmvp_lowd_lse_grad.hpp; kmvp_lowd_lse_grad_inst.hip, one unit
// per kernel x precision): the same shapes.  args.part: [segments][(D + 2) NC][n_pad] -- row k NC + c holds sum k of
// column c (k = 0: the denominator, k = 1 + d: component d of the numerator), rows (D + 1) NC + c the exponents.
KMVP_DECLARE_LOWD_LSE(launch_lowd_lse_grad_gaussian_f32, float)
KMVP_DECLARE_LOWD_LSE(launch_lowd_lse_grad_absexp_f32, float)
KMVP_DECLARE_LOWD_LSE(launch_lowd_lse_grad_gaussian_f64, double)
KMVP_DECLARE_LOWD_LSE(launch_lowd_lse_grad_absexp_f64, double)

// What the gradient of the log-sum-exp (kmvp_product.hip run_logsumexp_grad_t) and the mean-shift iteration on top of it
// (kmvp_meanshift.hip) share: the launch switch, the segment merge and the quotient V / Z.
inline hipError_t launch_lowd_lse_grad(int kernel, int D, int E, int sig, const LowdArgs<float>& args, dim3 grid, hipStream_t s,
                                       const char** name) {
  switch (kernel) {
    case K_GAUSSIAN: return launch_lowd_lse_grad_gaussian_f32(D, E, sig, args, grid, s, name);
    case K_ABSEXP: return launch_lowd_lse_grad_absexp_f32(D, E, sig, args, grid, s, name);
    default: return hipErrorInvalidValue;
  }
}
inline hipError_t launch_lowd_lse_grad(int kernel, int D, int E, int sig, const LowdArgs<double>& args, dim3 grid, hipStream_t s,
                                       const char** name) {
  switch (kernel) {
    case K_GAUSSIAN: return launch_lowd_lse_grad_gaussian_f64(D, E, sig, args, grid, s, name);
    case K_ABSEXP: return launch_lowd_lse_grad_absexp_f64(D, E, sig, args, grid, s, name);
    default: return hipErrorInvalidValue;
  }
}

// The segment merge: K_q = min_s k[s][q],   sums[t][q] = sum_s part[s][t][q] 2^(K_q - k[s][q]) for the NS = D + 1 sums t
// that share the exponent (index order; every factor <= 1 and exact).  One thread per (t, q).
// (static: a kernel cannot be inline; each of the two units that launch it carries its own copy, the others none)
static __global__ void lse_grad_reduce_kernel(const double* __restrict__ part, double* __restrict__ sums, double* __restrict__ kmin,
                                              int64_t count /* NC * n_pad */, int NS, int segments) {
  const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (int64_t)NS * count) return;
  const int64_t q = idx % count;
  const int64_t stride = (int64_t)(NS + 1) * count;  // one segment
  const double* kexp = part + (int64_t)NS * count + q;
  double K = INFINITY;
  for (int s = 0; s < segments; ++s) K = fmin(K, kexp[s * stride]);
  double v = 0.0;
  for (int s = 0; s < segments; ++s) {
    const double ks = kexp[s * stride];
    if (ks < INFINITY) v += ldexp(part[s * stride + idx], (int)fmax(K - ks, -100000.0));
  }
  sums[idx] = v;
  if (idx < count) kmin[q] = K;
}

// One component of the gradient from the merged sums: constant V[d] / Z (the common scale cancels); `none`: no live term
// anywhere, the softmax does not exist.  finish_lse_grad_kernel (kmvp_product.hip) and the mean-shift step
// (kmvp_meanshift.hip) both go through this one expression, so the step sees the gradient's own bits.
__device__ __forceinline__ double lse_grad_value(bool none, double constant, double v, double z) {
  return none ? __builtin_nan("") : constant * v / z;
}

// bf16 MFMA path (kmvp_mfma.hpp): largest shapes instantiated
constexpr int MFMA_MAX_KS = 9;  // D <= 16*9 - 6 = 138
constexpr int MFMA_MAX_NT = 4;  // E <= 128
struct MfmaArgs;
hipError_t launch_mfma_gaussian(int KS, int NT, int TW, const MfmaArgs& args, dim3 grid, hipStream_t stream,
                                const char** kernel_name);
hipError_t launch_mfma_absexp(int KS, int NT, int TW, const MfmaArgs& args, dim3 grid, hipStream_t stream,
                              const char** kernel_name);
hipError_t launch_mfma_invdist(int KS, int NT, int TW, const MfmaArgs& args, dim3 grid, hipStream_t stream,
                               const char** kernel_name);
// exp(<x,y>) with the per-target running shift (kmvp_mfma.hpp; D <= 16 KS - 3)
hipError_t launch_mfma_expdot(int KS, int NT, int TW, const MfmaArgs& args, dim3 grid, hipStream_t stream,
                              const char** kernel_name);
// the Gaussian with the same shift (targets != sources; D <= 16 KS - 9)
hipError_t launch_mfma_gaussian_shifted(int KS, int NT, int TW, const MfmaArgs& args, dim3 grid, hipStream_t stream,
                                        const char** kernel_name);


// split-bf16 MFMA low-D path (kmvp_fast.hpp): 6 D + 6 <= 48, E == 1
constexpr int FAST_MAX_D = 39;             // K = 6 D + 6 <= 240 = 15 k-steps of 16
constexpr int FAST_MAX_D_FOUR_TILES = 7;  // four target tiles per wave up to K = 48
constexpr int FAST_MAX_D_TWO_TILES = 23;  // two up to K = 144, one beyond
constexpr int FAST_DEFAULT_TT = 4;
// auto mode: scaled squared radius of the clouds below which the expansion is used
constexpr float FAST_AUTO_RADIUS2 = 8.0f;
struct FastArgs;
hipError_t launch_fast_gaussian(int D, int sig, int TT, const FastArgs& args, dim3 grid,
                                hipStream_t stream, const char** kernel_name);
hipError_t launch_fast_absexp(int D, int sig, int TT, const FastArgs& args, dim3 grid,
                              hipStream_t stream, const char** kernel_name);
hipError_t launch_fast_invdist(int D, int sig, int TT, const FastArgs& args, dim3 grid,
                               hipStream_t stream, const char** kernel_name);


// both products on the matrix cores (kmvp_fastmm.hpp): Gaussian, float32, D <= 64, several signal columns (one column beyond D = 39)
// cost model of the auto choice between the two (ps per 32 x 32 tile of pairs, whole chip; tools/fmm_probe.py)
constexpr double FMM_PS_PER_TILE_16 = 180.0, FMM_PS_PER_TILE_32 = 225.0;
constexpr double CMM_PS_PER_TILE_MAIN = 26.0, CMM_PS_PER_TILE_TT4 = 30.0, CMM_PS_PER_TILE_REST = 48.0;
struct FastmmArgs;
// online != 0: per-target running shift (kmvp_fastmm.hpp "The shift")
hipError_t launch_fastmm_gaussian(int KS, int mode, int TT, int online, const FastmmArgs& args, dim3 grid, hipStream_t stream,
                                  const char** kernel_name);
// exp(-r) on the same expansion, closest pairs recomputed exactly (5 <= D <= 64; D <= 4: the centred forms)
hipError_t launch_fastmm_absexp(int KS, int mode, int TT, int online, const FastmmArgs& args, dim3 grid, hipStream_t stream,
                                const char** kernel_name);
// tau = FMM_ABSEXP_KAPPA R^4 (R^2: scaled squared radius of the clouds): below it the error ~1e-7 R^2 of s would show
// in 2^-sqrt(s) beyond 1e-6 -- sqrt(s) >= ln2 * 1e-7 R^2 / 2e-6 = 0.035 R^2; twice that for margin
constexpr float FMM_ABSEXP_KAPPA = 5.0e-3f;

// the same second product on cfast_kernel's distances (kmvp_cfastmm.hpp): Gaussian and exp(-r), float32, D <= 4
struct CfastmmArgs;
hipError_t launch_cfastmm(int kernel, int mode, int TT, int online, const CfastmmArgs& args, dim3 grid, hipStream_t stream,
                          const char** kernel_name);
constexpr int CFMM_AUTO_MIN_COLS = 4;  // auto: from four columns on (1e5 points, four columns: 3.0 ms against 3.7 ms of the difference form)

// centred split-bf16 MFMA path (kmvp_cfast.hpp): D <= 4, E == 1, every kernel
constexpr int CFAST_MAX_D = 4;
constexpr int CFAST_DEFAULT_TT = 2;
constexpr int LOWD_MID_MAX_D = 128;  // lowd_mid_kernel: coordinates in registers up to here (16 chunks of 8)
struct CfastArgs;
hipError_t launch_cfast_gaussian(int sig, int TT, const CfastArgs& args, dim3 grid, hipStream_t stream,
                                 const char** kernel_name);
hipError_t launch_cfast_absexp(int sig, int TT, const CfastArgs& args, dim3 grid, hipStream_t stream,
                               const char** kernel_name);
hipError_t launch_cfast_invdist(int sig, int TT, const CfastArgs& args, dim3 grid, hipStream_t stream,
                                const char** kernel_name);
// cell-reduced Gaussian path (kmvp_cell.hpp): float32, D <= 3, E == 1
constexpr int CELL_MAX_D = 3;
// auto mode: the path is taken when padding the cells' last tiles adds at most this share of slots
constexpr double CELL_AUTO_MAX_PAD = 1.30;
struct CellArgs;
hipError_t launch_cell_gaussian(int sig, int TT, const CellArgs& args, dim3 grid, hipStream_t stream,
                                const char** kernel_name);
struct CellmmArgs;
hipError_t launch_cellmm_gaussian(int TT, int shape, const CellmmArgs& args, dim3 grid, hipStream_t stream, const char** kernel_name);
struct Cell64Args;
hipError_t launch_cell64_gaussian(int sig, const Cell64Args& args, dim3 grid, hipStream_t stream, const char** kernel_name);
// kmvp_sort.hip: hipcub radix sort of (key, value) pairs; tmp == nullptr queries the scratch size
hipError_t sort_pairs_u32(void* tmp, size_t* tmp_bytes, const unsigned* keys_in, unsigned* keys_out,
                          const int* vals_in, int* vals_out, int64_t n, hipStream_t stream);

}  // namespace kmvp
