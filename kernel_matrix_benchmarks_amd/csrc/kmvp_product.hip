// The product a = K b [/ K 1]: kernel layouts, launch geometry, the host side of the pair-loop paths
// (difference form, split-bf16 / centred / cell forms, the matrix-core column products, bf16 MFMA),
// the policy that picks one of them, and their common epilogue
//   segment reduction -> [RCCL all-reduce over the source shards] -> normalise.
// Reference call this serves: BruteForceProductBLAS.query (bruteforce.py:130-153).
#include "kmvp_ctx.hpp"
#include <array>
#include <cstring>
#include <map>
#include <vector>
#include "kmvp_cell_pack.hpp"
#include "kmvp_cell64_pack.hpp"
#include "kmvp_cellmm_pack.hpp"
#include "kmvp_cfast_pack.hpp"
#include "kmvp_fast_pack.hpp"
#include "kmvp_fastmm_pack.hpp"
#include "kmvp_cfastmm_pack.hpp"
#include "kmvp_mfma_pack.hpp"
#include "kmvp_lowd_lse.hpp"

namespace kmvp {
namespace {

template <typename real>
hipError_t launch_lowd(int kernel, int D, int E, int sig, LowdTuning tune,
                       const LowdArgs<real>& args, dim3 grid, hipStream_t s, const char** name);
template <>
hipError_t launch_lowd<float>(int kernel, int D, int E, int sig, LowdTuning tune,
                              const LowdArgs<float>& args, dim3 grid, hipStream_t s,
                              const char** name) {
  switch (kernel) {
    case K_GAUSSIAN: return launch_lowd_gaussian_f32(D, E, sig, tune, args, grid, s, name);
    case K_ABSEXP: return launch_lowd_absexp_f32(D, E, sig, tune, args, grid, s, name);
    case K_INVDIST: return launch_lowd_invdist_f32(D, E, sig, tune, args, grid, s, name);
    case K_MATERN32: return launch_lowd_matern32_f32(D, E, sig, tune, args, grid, s, name);
    case K_MATERN52: return launch_lowd_matern52_f32(D, E, sig, tune, args, grid, s, name);
    default: return hipErrorInvalidValue;  // (an id without a difference-form unit never reaches a launch)
  }
}
template <>
hipError_t launch_lowd<double>(int kernel, int D, int E, int sig, LowdTuning tune,
                               const LowdArgs<double>& args, dim3 grid, hipStream_t s,
                               const char** name) {
  switch (kernel) {
    case K_GAUSSIAN: return launch_lowd_gaussian_f64(D, E, sig, tune, args, grid, s, name);
    case K_ABSEXP: return launch_lowd_absexp_f64(D, E, sig, tune, args, grid, s, name);
    case K_INVDIST: return launch_lowd_invdist_f64(D, E, sig, tune, args, grid, s, name);
    case K_MATERN32: return launch_lowd_matern32_f64(D, E, sig, tune, args, grid, s, name);
    case K_MATERN52: return launch_lowd_matern52_f64(D, E, sig, tune, args, grid, s, name);
    default: return hipErrorInvalidValue;  // (an id without a difference-form unit never reaches a launch)
  }
}

template <typename real>
hipError_t launch_generic(int kernel, int sig, const real* x, const real* y, const real* b,
                          double* part, int64_t n, int64_t n_pad, int64_t m, int D, int E, int NE,
                          int segments, int64_t seg_len, int64_t j_offset, int64_t m_total,
                          hipStream_t s, const char** name);
template <>
hipError_t launch_generic<float>(int kernel, int sig, const float* x, const float* y, const float* b,
                                 double* part, int64_t n, int64_t n_pad, int64_t m, int D, int E,
                                 int NE, int segments, int64_t seg_len, int64_t j_offset,
                                 int64_t m_total, hipStream_t s, const char** name) {
  switch (kernel) {
    case K_GAUSSIAN:
      return launch_lowd_gaussian_f32_generic(sig, x, y, b, part, n, n_pad, m, D, E, NE, segments,
                                              seg_len, j_offset, m_total, s, name);
    case K_ABSEXP:
      return launch_lowd_absexp_f32_generic(sig, x, y, b, part, n, n_pad, m, D, E, NE, segments,
                                            seg_len, j_offset, m_total, s, name);
    case K_INVDIST:
      return launch_lowd_invdist_f32_generic(sig, x, y, b, part, n, n_pad, m, D, E, NE, segments,
                                             seg_len, j_offset, m_total, s, name);
    case K_MATERN32:
      return launch_lowd_matern32_f32_generic(sig, x, y, b, part, n, n_pad, m, D, E, NE, segments,
                                              seg_len, j_offset, m_total, s, name);
    case K_MATERN52:
      return launch_lowd_matern52_f32_generic(sig, x, y, b, part, n, n_pad, m, D, E, NE, segments,
                                              seg_len, j_offset, m_total, s, name);
    default:
      return hipErrorInvalidValue;
  }
}
template <>
hipError_t launch_generic<double>(int kernel, int sig, const double* x, const double* y,
                                  const double* b, double* part, int64_t n, int64_t n_pad, int64_t m,
                                  int D, int E, int NE, int segments, int64_t seg_len,
                                  int64_t j_offset, int64_t m_total, hipStream_t s,
                                  const char** name) {
  switch (kernel) {
    case K_GAUSSIAN:
      return launch_lowd_gaussian_f64_generic(sig, x, y, b, part, n, n_pad, m, D, E, NE, segments,
                                              seg_len, j_offset, m_total, s, name);
    case K_ABSEXP:
      return launch_lowd_absexp_f64_generic(sig, x, y, b, part, n, n_pad, m, D, E, NE, segments,
                                            seg_len, j_offset, m_total, s, name);
    case K_INVDIST:
      return launch_lowd_invdist_f64_generic(sig, x, y, b, part, n, n_pad, m, D, E, NE, segments,
                                             seg_len, j_offset, m_total, s, name);
    case K_MATERN32:
      return launch_lowd_matern32_f64_generic(sig, x, y, b, part, n, n_pad, m, D, E, NE, segments,
                                              seg_len, j_offset, m_total, s, name);
    case K_MATERN52:
      return launch_lowd_matern52_f64_generic(sig, x, y, b, part, n, n_pad, m, D, E, NE, segments,
                                              seg_len, j_offset, m_total, s, name);
    default:
      return hipErrorInvalidValue;
  }
}

template <typename real>
real scale_for(int kernel) {
  switch (kernel) {
    case K_GAUSSIAN: return coord_scale<K_GAUSSIAN, real>();
    case K_ABSEXP: return coord_scale<K_ABSEXP, real>();
    default: return coord_scale<K_INVDIST, real>();
  }
}

// Sum over the segments of part[s * stride + q].  Few segments: one thread per sum, index order.  Many (small problems take
// ~100 segments to fill the chip, and one thread's chain of dependent loads then costs more than the pair loop of a 1e4-point
// product): SEG_SPLIT consecutive lanes share a sum -- lane g takes the segments s = g (mod SEG_SPLIT) in index order, a
// butterfly over the group adds the eight partial sums.  A fixed order either way: results stay bitwise reproducible, and
// reduce_segments_kernel (the exchange path) and reduce_finish_kernel (the plain one) add in the SAME order.
constexpr int SEG_SPLIT = 8;  // (taken from SEG_SPLIT_FROM segments on: kmvp_plan.hpp)
__device__ __forceinline__ double seg_sum_one(const double* __restrict__ part, int64_t stride, int64_t q, int segments) {
  double v = 0.0;
  for (int s = 0; s < segments; ++s) v += part[(int64_t)s * stride + q];
  return v;
}
__device__ __forceinline__ double seg_sum_split(const double* __restrict__ part, int64_t stride, int64_t q, int segments, int g) {
  double v = 0.0;
  for (int s = g; s < segments; s += SEG_SPLIT) v += part[(int64_t)s * stride + q];
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  return v;
}

// sums[e][i] = sum over segments of part[s][e][i]  (split != 0: SEG_SPLIT threads per sum, launched accordingly)
__global__ void reduce_segments_kernel(const double* __restrict__ part, double* __restrict__ sums,
                                       int64_t count /* NE*n_pad */, int segments, int split) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (split) {
    const int64_t q = t / SEG_SPLIT;
    if (q >= count) return;  // (whole groups leave together)
    const double v = seg_sum_split(part, count, q, segments, (int)(t % SEG_SPLIT));
    if (t % SEG_SPLIT == 0) sums[q] = v;
    return;
  }
  if (t >= count) return;
  sums[t] = seg_sum_one(part, count, t, segments);
}

// The same for one launch's REGION of partial sums [segment][column][region_slots] (the float32 cell kernels run two
// launches with different numbers of segments): sums[e][slot_base + sl] = sum over segments, sums being [column][n_slots].
__global__ void reduce_region_kernel(const double* __restrict__ part, double* __restrict__ sums, int64_t region_slots,
                                     int NE, int segments, int64_t n_slots, int64_t slot_base) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= (int64_t)NE * region_slots) return;
  const int64_t e = q / region_slots, sl = q % region_slots;
  double v = 0.0;
  for (int s = 0; s < segments; ++s) v += part[((int64_t)s * NE + e) * region_slots + sl];
  sums[e * n_slots + slot_base + sl] = v;
}

// One launch for the single-GPU epilogue: out[i*E + e] = sum over segments (index order) of
// part[s][e][i], divided by the same sum of column E when normalised.  Same additions in the
// same order as reduce_segments_kernel + finish_kernel.
__global__ void reduce_finish_kernel(const double* __restrict__ part, double* __restrict__ out, int64_t n,
                                     int64_t n_pad, int E, int NE, int segments, int normalise, int split) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t i = split ? t / SEG_SPLIT : t;
  const int g = split ? (int)(t % SEG_SPLIT) : 0;
  if (i >= n) return;  // (split: whole groups leave together)
  const int64_t count = (int64_t)NE * n_pad;
  double den = 1.0;
  if (normalise)
    den = split ? seg_sum_split(part, count, (int64_t)E * n_pad + i, segments, g) : seg_sum_one(part, count, (int64_t)E * n_pad + i, segments);
  for (int e = 0; e < E; ++e) {
    const double v = split ? seg_sum_split(part, count, (int64_t)e * n_pad + i, segments, g)
                           : seg_sum_one(part, count, (int64_t)e * n_pad + i, segments);
    if (g == 0) out[i * E + e] = normalise ? v / den : v;
  }
}

// Column-blocked products: block partials part[s][e][i] (e < NEk) summed over the segments into the
// full sums array: column e < Ek goes to col0 + e, the extra column (denominator) to den_col.
__global__ void reduce_block_kernel(const double* __restrict__ part, double* __restrict__ sums, int64_t n_pad,
                                    int NEk, int Ek, int segments, int col0, int den_col) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t count = (int64_t)NEk * n_pad;
  if (q >= count) return;
  const int e = (int)(q / n_pad);
  const int64_t i = q % n_pad;
  double v = 0.0;
  for (int s = 0; s < segments; ++s) v += part[(int64_t)s * count + q];
  sums[(int64_t)(e < Ek ? col0 + e : den_col) * n_pad + i] = v;
}

// out[i*E + e] = sums[e][i]  (/ sums[E][i] when normalised).  kshift (exp(<x,y>), or nullptr): the sums of target i are
// at the scale 2^-kshift[i] -- it cancels in normalised rows and is applied to plain ones here (+inf: no source at all).
__global__ void finish_kernel(const double* __restrict__ sums, double* __restrict__ out, int64_t n,
                              int64_t n_pad, int E, int normalise, const double* __restrict__ kshift) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double den = normalise ? sums[(int64_t)E * n_pad + i] : 1.0;
  int back = 0;
  bool none = false;
  if (kshift && !normalise) {
    const double k = kshift[i];
    none = !(k < 1.0e300);
    back = none ? 0 : (int)fmin(fmax(-k, -100000.0), 100000.0);
  }
  for (int e = 0; e < E; ++e) {
    const double v = sums[(int64_t)e * n_pad + i];
    out[i * E + e] = normalise ? v / den : (none ? 0.0 : (back ? ldexp(v, back) : v));
  }
}

// exp(<x,y>) (fastmm_kernel with FastmmArgs::kexp): partial sums part[s][e][i] at the scale 2^-kexp[s][i].
//   K_i = min_s kexp[s][i]  (the exponent of the row's largest term so far; +inf: segment s had no live source)
//   sums[col][i] = sum_s part[s][e][i] 2^(K_i - kexp[s][i])        (every factor <= 1: nothing overflows)
// Columns as in reduce_block_kernel (e < Ek -> col0 + e, the extra column -> den_col); kmin[i] = K_i.
__global__ void reduce_shifted_kernel(const double* __restrict__ part, const float* __restrict__ kexp,
                                      double* __restrict__ sums, double* __restrict__ kmin, int64_t n_pad, int NEk, int Ek,
                                      int segments, int col0, int den_col) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= (int64_t)NEk * n_pad) return;
  const int e = (int)(q / n_pad);
  const int64_t i = q % n_pad;
  float K = INFINITY;
  for (int s = 0; s < segments; ++s) K = fminf(K, kexp[(int64_t)s * n_pad + i]);
  double v = 0.0;
  for (int s = 0; s < segments; ++s) {
    const float ks = kexp[(int64_t)s * n_pad + i];
    if (ks < INFINITY) v += ldexp(part[((int64_t)s * NEk + e) * n_pad + i], (int)fmaxf(K - ks, -100000.f));
  }
  sums[(int64_t)(e < Ek ? col0 + e : den_col) * n_pad + i] = v;
  if (e == 0) kmin[i] = (double)K;
}

// after the all-reduce(min) of the exponents over the ranks: this rank's sums move to the common scale 2^-kglobal
__global__ void rescale_shifted_kernel(double* __restrict__ sums, const double* __restrict__ klocal,
                                       const double* __restrict__ kglobal, int64_t n, int64_t n_pad, int NE) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= (int64_t)NE * n) return;
  const int64_t e = q / n, i = q % n;
  const double kl = klocal[i], kg = kglobal[i];
  double& v = sums[e * n_pad + i];
  v = (kl < 1.0e300) ? ldexp(v, (int)fmax(kg - kl, -100000.0)) : 0.0;
}

// canon[e][i] = sums[e][i] for i < n: drops the path-specific padding before the all-reduce
__global__ void unpad_kernel(const double* __restrict__ sums, double* __restrict__ canon, int64_t n,
                             int64_t n_pad, int64_t NE) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= NE * n) return;
  canon[q] = sums[(q / n) * n_pad + q % n];
}

__global__ void fill_kernel(double* p, int64_t n, double v) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}


// Timing marks of a synchronous product; an asynchronous one (solver iteration, possibly inside a
// stream capture) records nothing.
inline hipError_t mark(kmvp_ctx* c, int i) { return c->async_product ? hipSuccess : hipEventRecord(c->ev[i], c->stream); }

// Last step of every product, once the (N, E) result is queued into c->out: an asynchronous product leaves it on the
// stream (the caller keeps working there); a synchronous one waits for it and reads the elapsed times of its marks.
int complete(kmvp_ctx* c, int64_t N, int E) {
  c->out_n = N;
  c->out_e = E;
  if (c->async_product) return KMVP_OK;
  HIP_TRY(c, hipEventRecord(c->ev[2], c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipEventElapsedTime(&c->last_kernel_ms, c->ev[0], c->ev[1]));
  HIP_TRY(c, hipEventElapsedTime(&c->last_total_ms, c->ev[0], c->ev[2]));
  c->last_allreduce_ms = 0.f;
  if (c->exchanges()) HIP_TRY(c, hipEventElapsedTime(&c->last_allreduce_ms, c->ev[3], c->ev[4]));
  return KMVP_OK;
}

// (PackKey, points_stale, signal_stale, record_packed: kmvp_ctx.hpp, shared with the mean-shift iteration.)

// In-place all-reduce of `count` doubles on the device over the ranks of the attached exchange: ncclAllReduce on the
// context's stream, or -- rehearsal transport (kmvp_comm_init_host) -- device -> host, the caller's callback (e.g. gloo),
// host -> device: same buffer, same place in the stream, only the wire differs.
int exchange_f64(kmvp_ctx* c, double* buf, int64_t count, int op) {
  if (c->comm) {
    ncclResult_t r = g_rccl.AllReduce(buf, buf, (size_t)count, ncclFloat64, op == KMVP_OP_MIN ? ncclMin : ncclSum, c->comm,
                                      c->stream);
    if (r != ncclSuccess) return fail(c, KMVP_E_COMM, std::string("ncclAllReduce: ") + g_rccl.GetErrorString(r));
    return KMVP_OK;
  }
  const size_t cnt = (size_t)count;
  c->host_buf.resize(std::max<size_t>(cnt, 1));
  HIP_TRY(c, hipMemcpyAsync(c->host_buf.data(), buf, cnt * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const int hr = c->host_xchg(c->host_user, c->host_buf.data(), (int64_t)cnt, op);
  if (hr != 0) return fail(c, KMVP_E_COMM, "host all-reduce callback failed with status " + std::to_string(hr));
  HIP_TRY(c, hipMemcpyAsync(buf, c->host_buf.data(), cnt * sizeof(double), hipMemcpyHostToDevice, c->stream));
  return KMVP_OK;
}

// Common tail of every path, after the path's own reduction has left sums[column][n_pad]
// (fp64) in c->sums: one RCCL all-reduce over the source shards when a communicator is
// attached, normalisation / transposition into (N,E), event bookkeeping, and the stream
// synchronisation that makes the entry point synchronous (runner.py:138-140 times it).
int finish_product(kmvp_ctx* c, int64_t count, int64_t N, int64_t n_pad, int E, int sig, const double* kshift = nullptr) {
  int rc;
  const double* sums = (const double*)c->sums.p;
  if (c->exchanges()) {  // also with world == 1: the one-GPU tests then run the real exchange path
    // The padded length n_pad belongs to the kernel a rank happened to choose (tile sizes differ
    // between the paths, and the auto policy looks at the rank's own clouds), so the exchange uses
    // the canonical unpadded layout [column][N]: every rank contributes exactly NE * N doubles.
    const int64_t NE = count / n_pad;
    if ((rc = ensure(c, c->xchg, (size_t)NE * std::max<int64_t>(N, 1) * sizeof(double)))) return rc;
    hipLaunchKernelGGL(unpad_kernel, dim3(blocks_for(NE * N)), dim3(256), 0, c->stream, sums, (double*)c->xchg.p,
                       N, n_pad, NE);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, mark(c, 3));
    if ((rc = exchange_f64(c, (double*)c->xchg.p, NE * N, KMVP_OP_SUM))) return rc;
    HIP_TRY(c, mark(c, 4));
    sums = (const double*)c->xchg.p;
    n_pad = N;
  }
  if ((rc = ensure(c, c->out, (size_t)std::max<int64_t>(N, 1) * E * sizeof(double)))) return rc;
  hipLaunchKernelGGL(finish_kernel, dim3(blocks_for(std::max<int64_t>(N, 1))), dim3(256), 0, c->stream,
                     sums, (double*)c->out.p, N, n_pad, E, sig == SIG_NORM ? 1 : 0, kshift);
  HIP_TRY(c, hipGetLastError());
  return complete(c, N, E);
}


// Tail of the exp(<x,y>) path: c->sums [NE][n_pad] at the per-target scale 2^-K_i with K in c->kshift [n_pad].  Sharded:
// the ranks first agree on K (all-reduce MIN: the flash-attention (m, l, o) merge with m an integer exponent), move their
// sums to it, and then take the common tail (all-reduce SUM, normalise).
// The per-target exponent is clamped at +-FMM_MAX_ONLINE_SHIFT binades (= MFMA_DOT_MAX_SHIFT: what the two bf16 operand
// columns of the shift hold).  A row whose exponent reached the clamp has its largest logit at or beyond
// 32000 ln 2 ~ 2.2e4 (its values overflow the f16 / bf16 pieces: inf or NaN), or -- row-normalised -- every logit at or
// below -2.2e4 (all its values underflow: 0 / 0).  flag = 1 for such a row (a plain row of tiny logits is 0, rightly).
static_assert(FMM_MAX_ONLINE_SHIFT == MFMA_DOT_MAX_SHIFT, "one shift range for both native exp(<x,y>) paths");
__global__ void check_shift_range_kernel(const double* __restrict__ kshift, int64_t n, int normalise, int* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double k = kshift[i];  // +inf: no source at all; a NaN row keeps a finite, unclamped exponent
  if (k <= -(double)FMM_MAX_ONLINE_SHIFT || (normalise && k >= (double)FMM_MAX_ONLINE_SHIFT && k < 1.0e300)) *flag = 1;
}

int finish_product_shifted(kmvp_ctx* c, int64_t N, int64_t n_pad, int E, int sig) {
  const int NE = sig == SIG_NORM ? E + 1 : E;
  int rc;
  const double* kshift = (const double*)c->kshift.p;
  if (c->exchanges()) {
    if ((rc = ensure(c, c->xchgk, (size_t)std::max<int64_t>(N, 1) * sizeof(double)))) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->xchgk.p, c->kshift.p, (size_t)N * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    if ((rc = exchange_f64(c, (double*)c->xchgk.p, N, KMVP_OP_MIN))) return rc;
    hipLaunchKernelGGL(rescale_shifted_kernel, dim3(blocks_for((int64_t)NE * N)), dim3(256), 0, c->stream, (double*)c->sums.p,
                       (const double*)c->kshift.p, (const double*)c->xchgk.p, N, n_pad, NE);
    HIP_TRY(c, hipGetLastError());
    kshift = (const double*)c->xchgk.p;
  }
  // the range of the shift (check_shift_range_kernel): an error, never inf / NaN rows as a result.  (Asynchronous
  // products -- the solvers' inner operator -- leave no point to report it at: unchecked.)
  const bool check = !c->async_product && N > 0;
  if (check) {
    if ((rc = ensure(c, c->kflag, 256))) return rc;
    HIP_TRY(c, hipMemsetAsync(c->kflag.p, 0, sizeof(int), c->stream));
    hipLaunchKernelGGL(check_shift_range_kernel, dim3(blocks_for(N)), dim3(256), 0, c->stream, kshift, N,
                       sig == SIG_NORM ? 1 : 0, (int*)c->kflag.p);
    HIP_TRY(c, hipGetLastError());
  }
  if ((rc = finish_product(c, (int64_t)NE * n_pad, N, n_pad, E, sig, kshift))) return rc;
  if (check) {
    int flag = 0;
    HIP_TRY(c, hipMemcpyAsync(&flag, c->kflag.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (flag)
      return fail(c, KMVP_E_UNSUPPORTED,
                  "exp(<x,y>): a row's logits reach the native kernels' range |<x, y>| < 32000 ln 2 ~ 2.2e4 (the per-target "
                  "exponent is clamped at 32000 binades); scale the inputs down");
  }
  return KMVP_OK;
}

// Epilogue of the paths with fp64 partials [segment][column][n_pad] in c->part.  Without a
// communicator one fused launch does it; with one, the segments are summed into c->sums first and
// finish_product() exchanges them.
int reduce_and_finish(kmvp_ctx* c, int segments, int NE, int64_t N, int64_t n_pad, int E, int sig) {
  int rc;
  const int64_t count = (int64_t)NE * n_pad;
  const int split = segments >= SEG_SPLIT_FROM ? 1 : 0;
  if (c->exchanges()) {
    if ((rc = ensure(c, c->sums, (size_t)count * sizeof(double)))) return rc;
    hipLaunchKernelGGL(reduce_segments_kernel, dim3(blocks_for(count * (split ? SEG_SPLIT : 1))), dim3(256), 0, c->stream,
                       (const double*)c->part.p, (double*)c->sums.p, count, segments, split);
    HIP_TRY(c, hipGetLastError());
    return finish_product(c, count, N, n_pad, E, sig);
  }
  if ((rc = ensure(c, c->out, (size_t)std::max<int64_t>(N, 1) * E * sizeof(double)))) return rc;
  hipLaunchKernelGGL(reduce_finish_kernel, dim3(blocks_for(std::max<int64_t>(N, 1) * (split ? SEG_SPLIT : 1))), dim3(256), 0, c->stream,
                     (const double*)c->part.p, (double*)c->out.p, N, n_pad, E, NE, segments, sig == SIG_NORM ? 1 : 0, split);
  HIP_TRY(c, hipGetLastError());
  return complete(c, N, E);
}

// Geometry of the specialised difference-form kernels for the context's own clouds and options (kmvp_internal.hpp).
template <typename real>
LowdArgs<real> lowd_geometry(const kmvp_ctx* c, int T, int R, int cols) {
  return kmvp::lowd_geometry<real>(c->N, c->M, c->opt_segments, c->opt_chunk, c->j_offset, c->m_total, T, R, cols);
}

// The whole product: everything query() times.  `sig` as in kmvp_lowd.hpp.
template <typename real>
int run_product_t(kmvp_ctx* c, int kernel, int sig) {
  const int D = c->D;
  const int E = sig == SIG_DENSITY ? 1 : c->E;
  const int NE = sig == SIG_NORM ? E + 1 : E;
  const int64_t N = c->N, M = c->M;
  const bool specialised = D <= LOWD_MAX_D && E <= LOWD_MAX_E;
  const real scale = (real)1;  // difference form: the caller's coordinates, untouched (kval scales s)
  const real* x_raw = (const real*)(c->same_points ? c->y_raw.p : c->x_raw.p);
  int rc;

  int64_t n_pad;
  int segments;
  HIP_TRY(c, mark(c, 0));
  if (specialised) {
    LowdTuning tune;
    tune.feed = c->opt_feed >= 0 ? c->opt_feed : DEFAULT_FEED;
    tune.targets_per_lane = c->opt_T > 0 ? c->opt_T : (tune.feed == 1 ? DEFAULT_TARGETS_PER_LANE : 2);
    if (!(D == 3 && E == 1)) {
      // only the headline shape carries the whole (T, feed) grid; elsewhere a requested T keeps its
      // instantiated feed (T = 1: LDS tiles, T = 2: scalar-cache stream), anything else is the default
      if (tune.targets_per_lane == 2 && c->opt_T > 0) tune.feed = 0;
      else if (tune.feed == 0 && c->opt_T <= 0) tune.targets_per_lane = 2;
      else {
        tune.targets_per_lane = DEFAULT_TARGETS_PER_LANE;
        tune.feed = DEFAULT_FEED;
      }
    }
    if (c->opt_T > 0 || c->opt_feed >= 0) {
      // a requested pair that is not instantiated was replaced above without an error: say which pair runs
      char buf[96];
      snprintf(buf, sizeof buf, "%slowd_kernel runs targets_per_lane = %d, feed = %d", c->note.empty() ? "" : "; ",
               tune.targets_per_lane, tune.feed);
      c->note += buf;
    }
    const int EB = sig == SIG_DENSITY ? 0 : E;
    const int R = (D + EB + 3) / 4 * 4;
    LowdArgs<real> a = lowd_geometry<real>(c, tune.targets_per_lane, R, NE);
    n_pad = a.n_pad;
    segments = a.segments;

    // (re)pack the kernel layouts when the points, the signal, the kernel or T changed
    const PackKey key = {LAYOUT_LOWD, kernel, tune.targets_per_lane};
    if (points_stale(c, key)) {
      if ((rc = ensure(c, c->xs, (size_t)D * n_pad * sizeof(real)))) return rc;
      hipLaunchKernelGGL((pack_targets_kernel<real>), dim3(blocks_for(n_pad)), dim3(256), 0,
                         c->stream, x_raw, (real*)c->xs.p, N, n_pad, D, scale);
    }
    if (signal_stale(c, key, sig)) {
      // one spare batch behind the last record keeps the prefetch in bounds
      if ((rc = ensure(c, c->rec, (size_t)(a.m_pad + LOWD_BATCH) * R * sizeof(real)))) return rc;
      hipLaunchKernelGGL((pack_sources_kernel<real>), dim3(blocks_for(a.m_pad + LOWD_BATCH)), dim3(256), 0,
                         c->stream, (const real*)c->y_raw.p, (const real*)c->b_raw.p,
                         (real*)c->rec.p, M, a.m_pad + LOWD_BATCH, D, EB, R, scale);
    }
    HIP_TRY(c, hipGetLastError());
    record_packed(c, key, sig);

    if ((rc = ensure(c, c->part, (size_t)segments * NE * n_pad * sizeof(double)))) return rc;
    a.xs = (const real*)c->xs.p;
    a.rec = (const real*)c->rec.p;
    a.part = (double*)c->part.p;
    const int64_t nblocks = (int64_t)a.tile_blocks * segments;
    if (nblocks > 0x7fffffff) return fail(c, KMVP_E_UNSUPPORTED, "launch grid too large");
    HIP_TRY(c, mark(c, 0));
    hipError_t le = launch_lowd<real>(kernel, D, E, sig, tune, a, dim3((unsigned)nblocks), c->stream,
                                      &c->last_kernel_name);
    if (le == hipErrorInvalidValue)
      return fail(c, KMVP_E_UNSUPPORTED, "no kernel instantiated for this (D, E, targets_per_lane, feed)");
    HIP_TRY(c, le);
  } else {
    // generic fallback: scaled copies of the points, one target per lane
    n_pad = round_up(std::max<int64_t>(N, 1), BLOCK_THREADS);
    // both clouds as rows of DP entries, zero padded: 8 ceil(D / 8) for lowd_mid_kernel, 32 ceil(D / 32) for
    // lowd_big_kernel
    const int DP = D <= LOWD_MID_MAX_D ? (D + 7) / 8 * 8 : (D + 31) / 32 * 32;  // lowd_big_kernel: chunks of 32
    if (c->gen_points_ver != c->points_ver || c->gen_kernel != kernel) {
      if ((rc = ensure(c, c->y_scaled, (size_t)M * DP * sizeof(real)))) return rc;
      hipLaunchKernelGGL((pad_rows_kernel<real>), dim3(blocks_for(M * DP)), dim3(256), 0, c->stream,
                         (const real*)c->y_raw.p, (real*)c->y_scaled.p, M, D, DP);
      if (!c->same_points) {
        if ((rc = ensure(c, c->x_scaled, (size_t)N * DP * sizeof(real)))) return rc;
        hipLaunchKernelGGL((pad_rows_kernel<real>), dim3(blocks_for(N * DP)), dim3(256), 0, c->stream, x_raw,
                           (real*)c->x_scaled.p, N, D, DP);
      }
      HIP_TRY(c, hipGetLastError());
      c->gen_points_ver = c->points_ver;
      c->gen_kernel = kernel;
    }
    const int64_t tile_blocks = n_pad / BLOCK_THREADS;
    SegmentRule rule((int64_t)D * sizeof(real), NE);
    rule.min_seg = 256;
    segments = choose_segments(c->opt_segments, tile_blocks, M, n_pad, rule);
    const int64_t seg_len = (M + segments - 1) / segments;
    segments = (int)((M + seg_len - 1) / seg_len);
    if ((rc = ensure(c, c->part, (size_t)segments * NE * n_pad * sizeof(double)))) return rc;
    const real* xg = (const real*)(c->same_points ? c->y_scaled.p : c->x_scaled.p);
    const real* bg = sig == SIG_DENSITY ? nullptr : (const real*)c->b_raw.p;
    if (sig != SIG_DENSITY) {  // signal rows padded to whole column blocks of the kernel (8, or 32: lowd_mid_colblock)
      const int cb = D <= LOWD_MID_MAX_D ? lowd_mid_colblock((int)sizeof(real), D, c->E) : 8;
      const int EP = (c->E + cb - 1) / cb * cb;
      if ((rc = ensure(c, c->rec, (size_t)M * EP * sizeof(real)))) return rc;
      hipLaunchKernelGGL((pad_rows_kernel<real>), dim3(blocks_for(M * EP)), dim3(256), 0, c->stream,
                         (const real*)c->b_raw.p, (real*)c->rec.p, M, c->E, EP);
      HIP_TRY(c, hipGetLastError());
      c->packed_layout = -1;  // rec no longer holds a specialised layout
      bg = (const real*)c->rec.p;
    }
    HIP_TRY(c, mark(c, 0));
    HIP_TRY(c, launch_generic<real>(kernel, sig, xg, (const real*)c->y_scaled.p, bg,
                                    (double*)c->part.p, N, n_pad, M, D, c->E, NE, segments, seg_len,
                                    c->j_offset, c->m_total, c->stream, &c->last_kernel_name));
  }
  HIP_TRY(c, mark(c, 1));

  // ---- epilogue: segments -> sums, [all-reduce over the source shards], normalise
  return reduce_and_finish(c, segments, NE, N, n_pad, E, sig);
}

// Gradient with respect to the targets (kmvp_lowd_grad.hpp): lowd_grad_kernel on the product's own target image and
// source records (LAYOUT_LOWD, one target per lane), E D columns of partial sums per segment, the product's epilogue.
hipError_t launch_lowd_grad(int kernel, int D, int E, int sig, const LowdArgs<float>& args, dim3 grid, hipStream_t s,
                            const char** name) {
  switch (kernel) {
    case K_GAUSSIAN: return launch_lowd_grad_gaussian_f32(D, E, sig, args, grid, s, name);
    case K_ABSEXP: return launch_lowd_grad_absexp_f32(D, E, sig, args, grid, s, name);
    case K_INVDIST: return launch_lowd_grad_invdist_f32(D, E, sig, args, grid, s, name);
    case K_MATERN32: return launch_lowd_grad_matern32_f32(D, E, sig, args, grid, s, name);
    case K_MATERN52: return launch_lowd_grad_matern52_f32(D, E, sig, args, grid, s, name);
    default: return hipErrorInvalidValue;
  }
}
hipError_t launch_lowd_grad(int kernel, int D, int E, int sig, const LowdArgs<double>& args, dim3 grid, hipStream_t s,
                            const char** name) {
  switch (kernel) {
    case K_GAUSSIAN: return launch_lowd_grad_gaussian_f64(D, E, sig, args, grid, s, name);
    case K_ABSEXP: return launch_lowd_grad_absexp_f64(D, E, sig, args, grid, s, name);
    case K_INVDIST: return launch_lowd_grad_invdist_f64(D, E, sig, args, grid, s, name);
    case K_MATERN32: return launch_lowd_grad_matern32_f64(D, E, sig, args, grid, s, name);
    case K_MATERN52: return launch_lowd_grad_matern52_f64(D, E, sig, args, grid, s, name);
    default: return hipErrorInvalidValue;
  }
}
// Its sibling in the logarithm of a per-axis length scale (kmvp_lowd_dscale.hpp): lowd_dscale_kernel, the same arguments,
// the same E D columns; no 1/r.
hipError_t launch_lowd_dscale(int kernel, int D, int E, int sig, const LowdArgs<float>& args, dim3 grid, hipStream_t s,
                              const char** name) {
  switch (kernel) {
    case K_GAUSSIAN: return launch_lowd_dscale_gaussian_f32(D, E, sig, args, grid, s, name);
    case K_ABSEXP: return launch_lowd_dscale_absexp_f32(D, E, sig, args, grid, s, name);
    case K_MATERN32: return launch_lowd_dscale_matern32_f32(D, E, sig, args, grid, s, name);
    case K_MATERN52: return launch_lowd_dscale_matern52_f32(D, E, sig, args, grid, s, name);
    default: return hipErrorInvalidValue;
  }
}
hipError_t launch_lowd_dscale(int kernel, int D, int E, int sig, const LowdArgs<double>& args, dim3 grid, hipStream_t s,
                              const char** name) {
  switch (kernel) {
    case K_GAUSSIAN: return launch_lowd_dscale_gaussian_f64(D, E, sig, args, grid, s, name);
    case K_ABSEXP: return launch_lowd_dscale_absexp_f64(D, E, sig, args, grid, s, name);
    case K_MATERN32: return launch_lowd_dscale_matern32_f64(D, E, sig, args, grid, s, name);
    case K_MATERN52: return launch_lowd_dscale_matern52_f64(D, E, sig, args, grid, s, name);
    default: return hipErrorInvalidValue;
  }
}

// dscale: lowd_dscale_kernel in lowd_grad_kernel's place (run_dscale), everything else is shared
template <typename real>
int run_gradient_t(kmvp_ctx* c, int kernel, int sig, bool dscale) {
  const int D = c->D;
  const int E = sig == SIG_DENSITY ? 1 : c->E;
  const int NC = E * D;  // columns of the result: e D + d
  const int64_t N = c->N, M = c->M;
  const real* x_raw = (const real*)(c->same_points ? c->y_raw.p : c->x_raw.p);
  int rc;
  const int EB = sig == SIG_DENSITY ? 0 : E;
  const int R = (D + EB + 3) / 4 * 4;
  LowdArgs<real> a = lowd_geometry<real>(c, 1, R, NC);

  HIP_TRY(c, mark(c, 0));
  // the product's layouts under the product's key: whichever of them runs first on these points and this signal packs
  const PackKey key = {LAYOUT_LOWD, kernel, 1};
  if (points_stale(c, key)) {
    if ((rc = ensure(c, c->xs, (size_t)D * a.n_pad * sizeof(real)))) return rc;
    hipLaunchKernelGGL((pack_targets_kernel<real>), dim3(blocks_for(a.n_pad)), dim3(256), 0, c->stream, x_raw,
                       (real*)c->xs.p, N, a.n_pad, D, (real)1);
  }
  if (signal_stale(c, key, sig)) {
    if ((rc = ensure(c, c->rec, (size_t)(a.m_pad + LOWD_BATCH) * R * sizeof(real)))) return rc;
    hipLaunchKernelGGL((pack_sources_kernel<real>), dim3(blocks_for(a.m_pad + LOWD_BATCH)), dim3(256), 0, c->stream,
                       (const real*)c->y_raw.p, (const real*)c->b_raw.p, (real*)c->rec.p, M, a.m_pad + LOWD_BATCH, D, EB,
                       R, (real)1);
  }
  HIP_TRY(c, hipGetLastError());
  record_packed(c, key, sig);

  if ((rc = ensure(c, c->part, (size_t)a.segments * NC * a.n_pad * sizeof(double)))) return rc;
  a.xs = (const real*)c->xs.p;
  a.rec = (const real*)c->rec.p;
  a.part = (double*)c->part.p;
  const int64_t nblocks = (int64_t)a.tile_blocks * a.segments;
  if (nblocks > 0x7fffffff) return fail(c, KMVP_E_UNSUPPORTED, "launch grid too large");
  HIP_TRY(c, mark(c, 0));
  HIP_TRY(c, dscale ? launch_lowd_dscale(kernel, D, E, sig, a, dim3((unsigned)nblocks), c->stream, &c->last_kernel_name)
                    : launch_lowd_grad(kernel, D, E, sig, a, dim3((unsigned)nblocks), c->stream, &c->last_kernel_name));
  HIP_TRY(c, mark(c, 1));
  return reduce_and_finish(c, a.segments, NC, N, a.n_pad, NC, SIG_PRODUCT);
}


// ---- log-sum-exp reduction (kmvp_lowd_lse.hpp) -----------------------------------------------------------------------
// lowd_lse_kernel leaves, per (segment, column, target), a sum at the scale 2^-k and its exponent k (+inf: no live source),
// both fp64: part[s][c][i] and part[s][NC + c][i].  Every column has its own exponents, so the tail below treats
// (column, target) as ONE index of NC * n_pad (sharded: NC * N) entries and is then exp(<x,y>)'s, step by step.
// The launch switch and the segment merge (lse_reduce_kernel) are in kmvp_internal.hpp: the Sinkhorn iteration shares them.

// out[i * NC + e] = (log2(sums[e][i]) - K[e][i]) ln 2;  K = +inf (no live term anywhere): exactly -inf
__global__ void finish_lse_kernel(const double* __restrict__ sums, const double* __restrict__ kshift, double* __restrict__ out,
                                  int64_t n, int64_t n_pad, int NC) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n * NC) return;
  const int64_t i = q / NC, e = q % NC;
  const double k = kshift[e * n_pad + i];
  out[q] = lse_value(sums[e * n_pad + i], k);
}

// Tail of the log-sum-exp: c->sums / c->kshift hold [NC][n_pad] sums and exponents.  Sharded: the canonical unpadded layout
// [NC][N] of both, all-reduce(MIN) of the exponents, this rank's sums moved to the common scale (rescale_shifted_kernel),
// all-reduce(SUM) -- finish_product_shifted's exchange without its range check: the shift here is unbounded.
int finish_lse(kmvp_ctx* c, int64_t N, int64_t n_pad, int NC) {
  int rc;
  const double* sums = (const double*)c->sums.p;
  const double* kshift = (const double*)c->kshift.p;
  if (c->exchanges()) {
    const int64_t cnt = (int64_t)NC * N;
    const size_t bytes = (size_t)std::max<int64_t>(cnt, 1) * sizeof(double);
    if ((rc = ensure(c, c->xchg, bytes))) return rc;
    if ((rc = ensure(c, c->xchgk, 2 * bytes))) return rc;  // the rank's own exponents, then the common ones
    double* klocal = (double*)c->xchgk.p;
    double* kglobal = klocal + std::max<int64_t>(cnt, 1);
    hipLaunchKernelGGL(unpad_kernel, dim3(blocks_for(cnt)), dim3(256), 0, c->stream, sums, (double*)c->xchg.p, N, n_pad, (int64_t)NC);
    hipLaunchKernelGGL(unpad_kernel, dim3(blocks_for(cnt)), dim3(256), 0, c->stream, kshift, klocal, N, n_pad, (int64_t)NC);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(kglobal, klocal, (size_t)cnt * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, mark(c, 3));
    if ((rc = exchange_f64(c, kglobal, cnt, KMVP_OP_MIN))) return rc;
    hipLaunchKernelGGL(rescale_shifted_kernel, dim3(blocks_for(cnt)), dim3(256), 0, c->stream, (double*)c->xchg.p,
                       (const double*)klocal, (const double*)kglobal, cnt, cnt, 1);
    HIP_TRY(c, hipGetLastError());
    if ((rc = exchange_f64(c, (double*)c->xchg.p, cnt, KMVP_OP_SUM))) return rc;
    HIP_TRY(c, mark(c, 4));
    sums = (const double*)c->xchg.p;
    kshift = kglobal;
    n_pad = N;
  }
  if ((rc = ensure(c, c->out, (size_t)std::max<int64_t>(N, 1) * NC * sizeof(double)))) return rc;
  hipLaunchKernelGGL(finish_lse_kernel, dim3(blocks_for(std::max<int64_t>(N * NC, 1))), dim3(256), 0, c->stream, sums, kshift,
                     (double*)c->out.p, N, n_pad, NC);
  HIP_TRY(c, hipGetLastError());
  return complete(c, N, NC);
}

template <typename real>
int run_logsumexp_t(kmvp_ctx* c, int kernel, int sig) {
  const int D = c->D;
  const int E = sig == SIG_DENSITY ? 1 : c->E;  // = NC, the columns of the result
  const int64_t N = c->N, M = c->M;
  const real* x_raw = (const real*)(c->same_points ? c->y_raw.p : c->x_raw.p);
  int rc;
  const int EB = sig == SIG_DENSITY ? 0 : E;
  const int R = (D + EB + 3) / 4 * 4;
  LowdArgs<real> a = lowd_geometry<real>(c, 1, R, 2 * E);

  HIP_TRY(c, mark(c, 0));
  // the product's layouts under the product's key (as run_gradient_t): whichever runs first on these points and this signal packs
  const PackKey key = {LAYOUT_LOWD, kernel, 1};
  if (points_stale(c, key)) {
    if ((rc = ensure(c, c->xs, (size_t)D * a.n_pad * sizeof(real)))) return rc;
    hipLaunchKernelGGL((pack_targets_kernel<real>), dim3(blocks_for(a.n_pad)), dim3(256), 0, c->stream, x_raw,
                       (real*)c->xs.p, N, a.n_pad, D, (real)1);
  }
  if (signal_stale(c, key, sig)) {
    if ((rc = ensure(c, c->rec, (size_t)(a.m_pad + LOWD_BATCH) * R * sizeof(real)))) return rc;
    hipLaunchKernelGGL((pack_sources_kernel<real>), dim3(blocks_for(a.m_pad + LOWD_BATCH)), dim3(256), 0, c->stream,
                       (const real*)c->y_raw.p, (const real*)c->b_raw.p, (real*)c->rec.p, M, a.m_pad + LOWD_BATCH, D, EB,
                       R, (real)1);
  }
  HIP_TRY(c, hipGetLastError());
  record_packed(c, key, sig);

  const int64_t count = (int64_t)E * a.n_pad;
  if ((rc = ensure(c, c->part, (size_t)a.segments * 2 * count * sizeof(double)))) return rc;
  if ((rc = ensure(c, c->sums, (size_t)count * sizeof(double)))) return rc;
  if ((rc = ensure(c, c->kshift, (size_t)count * sizeof(double)))) return rc;
  a.xs = (const real*)c->xs.p;
  a.rec = (const real*)c->rec.p;
  a.part = (double*)c->part.p;
  const int64_t nblocks = (int64_t)a.tile_blocks * a.segments;
  if (nblocks > 0x7fffffff) return fail(c, KMVP_E_UNSUPPORTED, "launch grid too large");
  HIP_TRY(c, mark(c, 0));
  HIP_TRY(c, launch_lowd_lse(kernel, D, E, sig, a, dim3((unsigned)nblocks), c->stream, &c->last_kernel_name));
  HIP_TRY(c, mark(c, 1));
  hipLaunchKernelGGL(lse_reduce_kernel, dim3(blocks_for(count)), dim3(256), 0, c->stream, (const double*)c->part.p,
                     (double*)c->sums.p, (double*)c->kshift.p, count, a.segments);
  HIP_TRY(c, hipGetLastError());
  return finish_lse(c, N, a.n_pad, E);
}

// ---- gradient of the log-sum-exp with respect to the targets (kmvp_lowd_lse_grad.hpp) ------------------------------------
// lowd_lse_grad_kernel leaves, per (segment, column c, target), D + 1 sums at the scale 2^-k and ONE exponent k (+inf: no
// live source), all fp64: part[s][k NC + c][i] for sum k (0: the denominator Z, 1 + d: the numerator V[d]) and
// part[s][(D + 1) NC + c][i].  With q = (column, target) as ONE index of NC * n_pad (sharded: NC * N) entries the sums are
// [D + 1][q] and the exponents [q]: lse_reduce_kernel's arithmetic and finish_lse's exchange with D + 1 sums per exponent.
// (launch_lowd_lse_grad and the segment merge lse_grad_reduce_kernel: kmvp_internal.hpp, shared with the mean-shift
// iteration.)

// out[i][e D + d] = constant V[d] / Z with Z = sums[0][e][i], V[d] = sums[1 + d][e][i]: the common scale cancels.
// K = +inf (no live term anywhere): NaN in all D components -- exactly the entries where the log-sum-exp is -inf.
// (The expression itself: lse_grad_value, kmvp_internal.hpp.)
__global__ void finish_lse_grad_kernel(const double* __restrict__ sums, const double* __restrict__ kshift,
                                       double* __restrict__ out, int64_t n, int64_t n_pad, int NC, int D, double constant) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= n * NC) return;
  const int64_t i = q / NC, e = q % NC;
  const int64_t count = (int64_t)NC * n_pad;
  const bool none = !(kshift[e * n_pad + i] < 1.0e300);
  const double z = sums[e * n_pad + i];
  for (int d = 0; d < D; ++d)
    out[q * D + d] = lse_grad_value(none, constant, sums[(int64_t)(1 + d) * count + e * n_pad + i], z);
}

// Tail of the gradient: c->sums [D + 1][NC][n_pad] and c->kshift [NC][n_pad].  Sharded as finish_lse: the canonical
// unpadded layouts, all-reduce(MIN) of the NC * N exponents, this rank's (D + 1) NC N sums moved to the common scale
// (rescale_shifted_kernel with (column, target) as its target index), ONE all-reduce(SUM) of them.
int finish_lse_grad(kmvp_ctx* c, int kernel, int64_t N, int64_t n_pad, int NC, int D) {
  int rc;
  const int NS = D + 1;
  const double* sums = (const double*)c->sums.p;
  const double* kshift = (const double*)c->kshift.p;
  if (c->exchanges()) {
    const int64_t cnt = (int64_t)NC * N;
    const size_t bytes = (size_t)std::max<int64_t>(cnt, 1) * sizeof(double);
    if ((rc = ensure(c, c->xchg, NS * bytes))) return rc;
    if ((rc = ensure(c, c->xchgk, 2 * bytes))) return rc;  // the rank's own exponents, then the common ones
    double* klocal = (double*)c->xchgk.p;
    double* kglobal = klocal + std::max<int64_t>(cnt, 1);
    hipLaunchKernelGGL(unpad_kernel, dim3(blocks_for(NS * cnt)), dim3(256), 0, c->stream, sums, (double*)c->xchg.p, N, n_pad,
                       (int64_t)NS * NC);
    hipLaunchKernelGGL(unpad_kernel, dim3(blocks_for(cnt)), dim3(256), 0, c->stream, kshift, klocal, N, n_pad, (int64_t)NC);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(kglobal, klocal, (size_t)cnt * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, mark(c, 3));
    if ((rc = exchange_f64(c, kglobal, cnt, KMVP_OP_MIN))) return rc;
    hipLaunchKernelGGL(rescale_shifted_kernel, dim3(blocks_for(NS * cnt)), dim3(256), 0, c->stream, (double*)c->xchg.p,
                       (const double*)klocal, (const double*)kglobal, cnt, cnt, NS);
    HIP_TRY(c, hipGetLastError());
    if ((rc = exchange_f64(c, (double*)c->xchg.p, NS * cnt, KMVP_OP_SUM))) return rc;
    HIP_TRY(c, mark(c, 4));
    sums = (const double*)c->xchg.p;
    kshift = kglobal;
    n_pad = N;
  }
  if ((rc = ensure(c, c->out, (size_t)std::max<int64_t>(N, 1) * NC * D * sizeof(double)))) return rc;
  const double constant = kernel == K_GAUSSIAN ? -2.0 : -1.0;  // g = -2 (x - y), -(x - y) / r
  hipLaunchKernelGGL(finish_lse_grad_kernel, dim3(blocks_for(std::max<int64_t>(N * NC, 1))), dim3(256), 0, c->stream, sums,
                     kshift, (double*)c->out.p, N, n_pad, NC, D, constant);
  HIP_TRY(c, hipGetLastError());
  return complete(c, N, NC * D);
}

template <typename real>
int run_logsumexp_grad_t(kmvp_ctx* c, int kernel, int sig) {
  const int D = c->D;
  const int E = sig == SIG_DENSITY ? 1 : c->E;  // = NC, the columns of the log-sum-exp
  const int NS = D + 1;
  const int64_t N = c->N, M = c->M;
  const real* x_raw = (const real*)(c->same_points ? c->y_raw.p : c->x_raw.p);
  int rc;
  const int EB = sig == SIG_DENSITY ? 0 : E;
  const int R = (D + EB + 3) / 4 * 4;
  LowdArgs<real> a = lowd_geometry<real>(c, 1, R, E * (D + 2));

  HIP_TRY(c, mark(c, 0));
  // the product's layouts under the product's key (as run_logsumexp_t): whichever runs first on these points and this signal packs
  const PackKey key = {LAYOUT_LOWD, kernel, 1};
  if (points_stale(c, key)) {
    if ((rc = ensure(c, c->xs, (size_t)D * a.n_pad * sizeof(real)))) return rc;
    hipLaunchKernelGGL((pack_targets_kernel<real>), dim3(blocks_for(a.n_pad)), dim3(256), 0, c->stream, x_raw,
                       (real*)c->xs.p, N, a.n_pad, D, (real)1);
  }
  if (signal_stale(c, key, sig)) {
    if ((rc = ensure(c, c->rec, (size_t)(a.m_pad + LOWD_BATCH) * R * sizeof(real)))) return rc;
    hipLaunchKernelGGL((pack_sources_kernel<real>), dim3(blocks_for(a.m_pad + LOWD_BATCH)), dim3(256), 0, c->stream,
                       (const real*)c->y_raw.p, (const real*)c->b_raw.p, (real*)c->rec.p, M, a.m_pad + LOWD_BATCH, D, EB,
                       R, (real)1);
  }
  HIP_TRY(c, hipGetLastError());
  record_packed(c, key, sig);

  const int64_t count = (int64_t)E * a.n_pad;
  if ((rc = ensure(c, c->part, (size_t)a.segments * (NS + 1) * count * sizeof(double)))) return rc;
  if ((rc = ensure(c, c->sums, (size_t)NS * count * sizeof(double)))) return rc;
  if ((rc = ensure(c, c->kshift, (size_t)count * sizeof(double)))) return rc;
  a.xs = (const real*)c->xs.p;
  a.rec = (const real*)c->rec.p;
  a.part = (double*)c->part.p;
  const int64_t nblocks = (int64_t)a.tile_blocks * a.segments;
  if (nblocks > 0x7fffffff) return fail(c, KMVP_E_UNSUPPORTED, "launch grid too large");
  HIP_TRY(c, mark(c, 0));
  HIP_TRY(c, launch_lowd_lse_grad(kernel, D, E, sig, a, dim3((unsigned)nblocks), c->stream, &c->last_kernel_name));
  HIP_TRY(c, mark(c, 1));
  hipLaunchKernelGGL(lse_grad_reduce_kernel, dim3(blocks_for(NS * count)), dim3(256), 0, c->stream, (const double*)c->part.p,
                     (double*)c->sums.p, (double*)c->kshift.p, count, NS, a.segments);
  HIP_TRY(c, hipGetLastError());
  return finish_lse_grad(c, kernel, N, a.n_pad, E, D);
}

// Low D, many signal columns (D <= LOWD_MAX_D, E > LOWD_MAX_E): the specialised pair loop run
// once per block of LOWD_MAX_E columns (the kernel values are recomputed per block: E = 16 costs
// four passes of 14 issue slots per pair, against a generic kernel that is 4-5x slower).  The
// denominator of normalised rows comes from the first block.
template <typename real>
int run_product_blocked(kmvp_ctx* c, int kernel, int sig) {
  const int D = c->D, E = c->E;
  const int NE = sig == SIG_NORM ? E + 1 : E;
  const int64_t N = c->N, M = c->M;
  const real* x_raw = (const real*)(c->same_points ? c->y_raw.p : c->x_raw.p);
  int rc;
  LowdTuning tune;
  tune.feed = DEFAULT_FEED;
  tune.targets_per_lane = DEFAULT_TARGETS_PER_LANE;
  const int R = (D + LOWD_MAX_E + 3) / 4 * 4;
  LowdArgs<real> a = lowd_geometry<real>(c, tune.targets_per_lane, R, LOWD_MAX_E + 1);
  const int64_t n_pad = a.n_pad, m_pad = a.m_pad;
  const int segments = a.segments;

  HIP_TRY(c, mark(c, 0));
  const PackKey key = {LAYOUT_LOWD, kernel, tune.targets_per_lane};
  if (points_stale(c, key)) {
    if ((rc = ensure(c, c->xs, (size_t)D * n_pad * sizeof(real)))) return rc;
    hipLaunchKernelGGL((pack_targets_kernel<real>), dim3(blocks_for(n_pad)), dim3(256), 0, c->stream, x_raw,
                       (real*)c->xs.p, N, n_pad, D, (real)1);
  }
  record_packed(c, key, -1);  // the source records below hold one column block: never reusable as they are
  if ((rc = ensure(c, c->rec, (size_t)(m_pad + LOWD_BATCH) * R * sizeof(real)))) return rc;
  if ((rc = ensure(c, c->part, (size_t)segments * (LOWD_MAX_E + 1) * n_pad * sizeof(double)))) return rc;
  if ((rc = ensure(c, c->sums, (size_t)NE * n_pad * sizeof(double)))) return rc;
  a.xs = (const real*)c->xs.p;
  a.rec = (const real*)c->rec.p;
  a.part = (double*)c->part.p;

  const int64_t nblocks = (int64_t)a.tile_blocks * segments;
  if (nblocks > 0x7fffffff) return fail(c, KMVP_E_UNSUPPORTED, "launch grid too large");
  HIP_TRY(c, mark(c, 0));
  for (int e0 = 0; e0 < E; e0 += LOWD_MAX_E) {
    const int Ek = std::min(LOWD_MAX_E, E - e0);
    const int sigk = (sig == SIG_NORM && e0 == 0) ? SIG_NORM : SIG_PRODUCT;
    const int NEk = sigk == SIG_NORM ? Ek + 1 : Ek;
    const int Rk = (D + Ek + 3) / 4 * 4;
    hipLaunchKernelGGL((pack_sources_kernel<real>), dim3(blocks_for(m_pad + LOWD_BATCH)), dim3(256), 0, c->stream,
                       (const real*)c->y_raw.p, (const real*)c->b_raw.p, (real*)c->rec.p, M, m_pad + LOWD_BATCH, D, Ek,
                       Rk, (real)1, E, e0);
    hipError_t le = launch_lowd<real>(kernel, D, Ek, sigk, tune, a, dim3((unsigned)nblocks), c->stream,
                                      &c->last_kernel_name);
    if (le == hipErrorInvalidValue) return fail(c, KMVP_E_UNSUPPORTED, "no kernel instantiated for this column block");
    HIP_TRY(c, le);
    hipLaunchKernelGGL(reduce_block_kernel, dim3(blocks_for((int64_t)NEk * n_pad)), dim3(256), 0, c->stream,
                       (const double*)c->part.p, (double*)c->sums.p, n_pad, NEk, Ek, segments, e0, E);
    HIP_TRY(c, hipGetLastError());
  }
  HIP_TRY(c, mark(c, 1));
  return finish_product(c, (int64_t)NE * n_pad, N, n_pad, E, sig);
}

// ---- the staged matrix-core paths: fast, fastmm, cfast, cfastmm ------------------------------------------------------

static_assert(FAST_TILE == STAGED_TILE, "plan_stages() pads the targets to the kernels' tiles");

// The launch plan of a staged path (kmvp_plan.hpp) for the context's targets and options -- up to tt_max tiles per wave,
// tt_default on big problems, segments of at least four stages there -- refused when no launch takes its grid.
int stage_plan(kmvp_ctx* c, int64_t m_stages, int tt_max, int tt_default, SegmentRule rule, StagePlan& p) {
  rule.min_seg = 4;
  p = plan_stages(c->N, m_stages, c->opt_fast_tiles, tt_max, tt_default, c->opt_segments, rule);
  return p.ok ? KMVP_OK : fail(c, KMVP_E_UNSUPPORTED, "launch grid too large");
}
template <class Args>
void plan_args(const StagePlan& p, Args& a) {
  a.n_pad = p.n_pad;
  a.m_stages = p.m_stages;
  a.seg_stages = p.seg_stages;
  a.segments = p.segments;
  a.tile_blocks = (int)p.tile_blocks;
}

// split-bf16 MFMA low-D path (kmvp_fast.hpp): float32, D <= 7, E == 1, selected by the
// "fast_sqdists" option (the reference's constructor flag of the same name).
int run_product_fast(kmvp_ctx* c, int kernel, int sig) {
  const int D = c->D;
  const int E = 1;
  const int NE = sig == SIG_NORM ? 2 : 1;
  const int EB = sig == SIG_DENSITY ? 0 : 1;
  const int64_t N = c->N, M = c->M;
  const int KS = fast_ksteps(D);
  const int tt_max = D > FAST_MAX_D_TWO_TILES ? 1 : (D > FAST_MAX_D_FOUR_TILES ? 2 : 4);  // what is instantiated
  const int64_t SB = fast_stage_bytes(KS, EB);
  const float scale = scale_for<float>(kernel);
  const float* x_raw = (const float*)(c->same_points ? c->y_raw.p : c->x_raw.p);
  const int64_t m_tiles = (M + FAST_TILE - 1) / FAST_TILE;
  const int ST = fast_stage_tiles(KS);
  int rc;

  StagePlan p;
  if ((rc = stage_plan(c, (m_tiles + ST - 1) / ST, tt_max, FAST_DEFAULT_TT, SegmentRule(SB, NE), p))) return rc;
  const int64_t n_pad = p.n_pad, m_stages = p.m_stages;
  const int TT = p.TT;

  const PackKey key = {LAYOUT_FAST, kernel, TT};
  float* centre = (float*)c->aux.p;  // written by kmvp_set_points
  if (points_stale(c, key)) {
    const int RD = fast_target_row(D);
    if ((rc = ensure(c, c->xs, (size_t)n_pad * RD * sizeof(float)))) return rc;
    hipLaunchKernelGGL(pack_fast_targets_kernel, dim3(blocks_for(n_pad)), dim3(256), 0, c->stream, x_raw,
                       centre, (float*)c->xs.p, N, n_pad, D, RD, scale);
  }
  if (signal_stale(c, key, sig)) {
    if ((rc = ensure(c, c->rec, (size_t)m_stages * SB))) return rc;
    hipLaunchKernelGGL(pack_fast_sources_kernel, dim3(blocks_for(m_stages * ST * FAST_TILE)),
                       dim3(256), 0, c->stream, (const float*)c->y_raw.p, (const float*)c->b_raw.p, centre,
                       (unsigned char*)c->rec.p, M, m_stages, D, EB, KS, scale);
  }
  HIP_TRY(c, hipGetLastError());
  record_packed(c, key, sig);

  if ((rc = ensure(c, c->part, (size_t)p.segments * NE * n_pad * sizeof(double)))) return rc;
  FastArgs a;
  plan_args(p, a);
  a.xr = (const float*)c->xs.p;
  a.img = (const unsigned char*)c->rec.p;
  a.part = (double*)c->part.p;
  a.m = M;
  a.m_tiles = m_tiles;
  a.chunk_stages = std::max(1, c->opt_chunk / (FAST_TILE * ST));
  a.j_offset = c->j_offset;
  a.m_total = c->m_total;
  a.same_points = (c->same_points || c->opt_same_global) ? 1 : 0;
  const dim3 grid((unsigned)p.grid);
  HIP_TRY(c, mark(c, 0));
  const auto launch = kernel == K_GAUSSIAN ? launch_fast_gaussian : (kernel == K_ABSEXP ? launch_fast_absexp : launch_fast_invdist);
  const hipError_t le = launch(D, sig, TT, a, grid, c->stream, &c->last_kernel_name);
  if (le == hipErrorInvalidValue) return fail(c, KMVP_E_UNSUPPORTED, "fast_tiles must be 1, 2 or 4");
  HIP_TRY(c, le);
  HIP_TRY(c, mark(c, 1));

  // ---- epilogue: segments -> sums, [all-reduce over the source shards], normalise
  return reduce_and_finish(c, p.segments, NE, N, n_pad, E, sig);
}

// The column blocks of the matrix-core column products (fastmm_kernel, cfastmm_kernel): NE columns -- the denominator of
// normalised rows being one more column -- in blocks of up to FMM_MAX_COLS.  The signal part of the source image holds
// ONE block, so with several blocks it is re-packed on every pass and never reusable as it is (image_sig = -1).
// sigma / unscale: the current block's column scales (fastmm_colscale_kernel), kept in c->cell_scale behind the slots
// cellmm_kernel uses there.
struct ColumnBlocks {
  int NE, image_sig;
  bool one_block, sig_stale;
  float* sigma;
  double* unscale;
};
// (before the points are packed and the image is recorded: sig_stale is about what the buffers held on entry)
int column_blocks(kmvp_ctx* c, PackKey key, int sig, ColumnBlocks& cb) {
  int rc;
  cb.NE = sig == SIG_NORM ? c->E + 1 : c->E;
  cb.one_block = cb.NE <= FMM_MAX_COLS;
  cb.image_sig = cb.one_block ? sig : -1;
  cb.sig_stale = signal_stale(c, key, cb.image_sig);
  if ((rc = ensure(c, c->cell_scale, 1024))) return rc;
  cb.sigma = (float*)((char*)c->cell_scale.p + 256);
  cb.unscale = (double*)((char*)c->cell_scale.p + 512);
  return KMVP_OK;
}

// One pass of the pair loop per block: [column scales, pack_signal(col0, nb)] when the image is stale, launch(nb, part),
// and -- several blocks, or partial sums that carry exponents (shifted) -- the block's segments summed into c->sums.
// Then the tail: the shifted one (finish_product_shifted), the fused reduce + finish of a single block, or finish_product.
// `note`: the dispatch note of a pass that ran (nullptr: none).
template <class PackSignal, class Launch>
int run_column_blocks(kmvp_ctx* c, PackKey key, int sig, const StagePlan& p, const ColumnBlocks& cb, bool shifted,
                      const char* note, PackSignal pack_signal, Launch launch) {
  const int E = c->E, NE = cb.NE;
  const int64_t n_pad = p.n_pad;
  int rc;
  record_packed(c, key, cb.image_sig);
  if ((rc = ensure(c, c->part, (size_t)p.segments * std::min(NE, FMM_MAX_COLS) * n_pad * sizeof(double)))) return rc;
  if ((!cb.one_block || shifted) && (rc = ensure(c, c->sums, (size_t)NE * n_pad * sizeof(double)))) return rc;
  if (shifted) {
    if ((rc = ensure(c, c->kexp, (size_t)p.segments * n_pad * sizeof(float)))) return rc;
    if ((rc = ensure(c, c->kshift, (size_t)n_pad * sizeof(double)))) return rc;
  }
  HIP_TRY(c, mark(c, 0));
  for (int col0 = 0; col0 < NE; col0 += FMM_MAX_COLS) {
    const int nb = std::min(FMM_MAX_COLS, NE - col0);
    if (cb.sig_stale) {
      hipLaunchKernelGGL(fastmm_colscale_kernel, dim3(FMM_MAX_COLS), dim3(256), 0, c->stream, (const float*)c->b_raw.p,
                         c->M, E, col0, nb, cb.sigma, cb.unscale);
      pack_signal(col0, nb);
      HIP_TRY(c, hipGetLastError());
    }
    if ((rc = launch(nb))) return rc;
    // signal columns of the block; the one beyond them is the denominator (col0 <= E: never negative)
    const int Ek = std::min(nb, E - col0);
    const dim3 blocks(blocks_for((int64_t)nb * n_pad));
    if (shifted) {
      // (every pass runs the same distances in the same order: its exponents are the previous pass's, bit for bit)
      hipLaunchKernelGGL(reduce_shifted_kernel, blocks, dim3(256), 0, c->stream, (const double*)c->part.p,
                         (const float*)c->kexp.p, (double*)c->sums.p, (double*)c->kshift.p, n_pad, nb, Ek, p.segments, col0, E);
      HIP_TRY(c, hipGetLastError());
    } else if (!cb.one_block) {
      hipLaunchKernelGGL(reduce_block_kernel, blocks, dim3(256), 0, c->stream, (const double*)c->part.p,
                         (double*)c->sums.p, n_pad, nb, Ek, p.segments, col0, E);
      HIP_TRY(c, hipGetLastError());
    }
  }
  HIP_TRY(c, mark(c, 1));
  if (note) c->note = note;
  if (shifted) return finish_product_shifted(c, c->N, n_pad, E, sig);
  if (cb.one_block) return reduce_and_finish(c, p.segments, NE, c->N, n_pad, E, sig);
  return finish_product(c, (int64_t)NE * n_pad, c->N, n_pad, E, sig);
}

// Gaussian products with several signal columns, both matrix products on the matrix cores (kmvp_fastmm.hpp): float32,
// D <= 64, any E (column blocks as above).
// dot: k = exp(<x,y>) -- the Gaussian instantiation on operands without norms (S = -log2(e) <x,y>), always with the
// online shift, partial sums as (mantissa, exponent) pairs (FastmmArgs::kexp) and the shifted tail.
int run_product_fastmm(kmvp_ctx* c, int kernel, int sig, bool dot = false) {
  const int D = c->D, E = c->E;
  const int NE = sig == SIG_NORM ? E + 1 : E;
  const int64_t N = c->N, M = c->M;
  const int KS = fmm_ksteps(D);
  const int MODE = NE > 16 ? 1 : 0;
  const int tt_max = KS <= FMM_MAX_KS_TWO_TILES ? 2 : 1;  // (four tiles: no faster, 256 VGPRs)
  const int64_t SB = fmm_stage_bytes(KS, MODE);
  const int ST = fmm_stage_tiles(KS);
  // dot: the source rows hold -2 (y scale), so scale = log2(e) / 2 gives S = -log2(e) <x, y>
  const float scale = dot ? 0.72134752044448170f : scale_for<float>(kernel);
  const float* x_raw = (const float*)(c->same_points ? c->y_raw.p : c->x_raw.p);
  const int64_t m_tiles = (M + FAST_TILE - 1) / FAST_TILE;
  // the fixed shift 2^15 assumes every target has a source at distance ~0, i.e. targets == sources (also when the
  // sources are sharded: the all-reduced row then contains the self term); otherwise the per-target running shift
  const int online = (dot || !(c->same_points || c->opt_same_global)) ? 1 : 0;
  int rc;

  // (the kernel's time does not depend on the segment count between 8 and 48 at 1e5 points, the fp64 partial sums --
  // segments x columns x N x 8 bytes -- and their reduction do: about 4096 workgroups instead of 16384)
  SegmentRule rule(SB, std::min(NE, FMM_MAX_COLS));
  rule.target_blocks = 4096;
  StagePlan p;
  if ((rc = stage_plan(c, (m_tiles + ST - 1) / ST, tt_max, tt_max, rule, p))) return rc;
  const int64_t n_pad = p.n_pad, m_stages = p.m_stages;
  const int TT = p.TT;

  const PackKey key = {LAYOUT_FASTMM, dot ? K_EXPDOT : kernel, TT + 16 * MODE};
  ColumnBlocks cb;
  if ((rc = column_blocks(c, key, sig, cb))) return rc;
  float* centre = (float*)c->aux.p;  // written by kmvp_set_points
  if (points_stale(c, key)) {
    if ((rc = ensure(c, c->xs, (size_t)n_pad * KS * 32))) return rc;
    if ((rc = ensure(c, c->rec, (size_t)m_stages * SB))) return rc;
    hipLaunchKernelGGL(pack_fastmm_targets_kernel, dim3(blocks_for(n_pad * KS * 2)), dim3(256), 0, c->stream, x_raw,
                       centre, (unsigned char*)c->xs.p, N, n_pad, D, KS, scale,
                       kernel == K_GAUSSIAN ? (float)FMM_SHIFT : 0.f, dot ? 1 : 0);
    hipLaunchKernelGGL(pack_fastmm_rows_kernel, dim3(blocks_for(m_stages * ST * FAST_TILE)), dim3(256), 0,
                       c->stream, (const float*)c->y_raw.p, centre, (unsigned char*)c->rec.p, M, m_stages, D, KS, MODE,
                       scale, dot ? 1 : 0);
    HIP_TRY(c, hipGetLastError());
  }

  FastmmArgs a;
  plan_args(p, a);
  a.xop = (const unsigned char*)c->xs.p;
  a.img = (const unsigned char*)c->rec.p;
  a.unscale = cb.unscale;
  a.chunk_stages = std::max(1, 2 * c->opt_chunk / (FAST_TILE * ST));
  a.xraw = x_raw;
  a.yraw = (const float*)c->y_raw.p;
  a.n = N;
  a.m = M;
  a.D = D;
  a.scale = scale;
  {
    const float r2 = c->cloud_radius2 * scale * scale;  // scaled squared radius of the clouds
    a.tau = kernel == K_ABSEXP ? FMM_ABSEXP_KAPPA * r2 * r2 : 0.f;
  }
  const dim3 grid((unsigned)p.grid);
  const int64_t pieces = m_stages * ST * (MODE ? 2 : 1) * 2 * 64;
  const char* note = dot      ? "exp(<x,y>): fastmm_kernel with the per-target online shift, (mantissa, exponent) partial sums"
                     : online ? "fastmm_kernel with the per-target online shift (targets != sources)"
                              : nullptr;
  return run_column_blocks(
      c, key, sig, p, cb, dot, note,
      [&](int col0, int nb) {
        hipLaunchKernelGGL(pack_fastmm_signal_kernel, dim3(blocks_for(pieces)), dim3(256), 0, c->stream,
                           (const float*)c->b_raw.p, (const float*)cb.sigma, (unsigned char*)c->rec.p, M, m_stages, E, col0,
                           nb, KS, MODE);
      },
      [&](int nb) {
        a.NE = nb;
        a.part = (double*)c->part.p;
        a.kexp = dot ? (float*)c->kexp.p : nullptr;
        hipError_t le = kernel == K_ABSEXP ? launch_fastmm_absexp(KS, MODE, TT, online, a, grid, c->stream, &c->last_kernel_name)
                                           : launch_fastmm_gaussian(KS, MODE, TT, online, a, grid, c->stream, &c->last_kernel_name);
        if (le == hipErrorInvalidValue) return fail(c, KMVP_E_UNSUPPORTED, "no fastmm_kernel for this dimension / tile count");
        HIP_TRY(c, le);
        return (int)KMVP_OK;
      });
}

// Scratch of one radix sort of n (key, value) pairs, carved out of c->sortbuf: keys in / out, values in, hipcub's own
struct SortBufs {
  unsigned *keys_in, *keys_out;
  int* vals_in;
  void* tmp;
  size_t tmp_bytes;
};
int sort_buffers(kmvp_ctx* c, int64_t n, SortBufs& b) {
  int rc;
  b.tmp_bytes = 0;
  HIP_TRY(c, sort_pairs_u32(nullptr, &b.tmp_bytes, nullptr, nullptr, nullptr, nullptr, n, c->stream));
  if ((rc = ensure(c, c->sortbuf, 3 * (size_t)n * sizeof(unsigned) + b.tmp_bytes + 256))) return rc;
  b.keys_in = (unsigned*)c->sortbuf.p;
  b.keys_out = b.keys_in + n;
  b.vals_in = (int*)(b.keys_out + n);
  b.tmp = (void*)((((uintptr_t)(b.vals_in + n)) + 255) & ~(uintptr_t)255);
  return KMVP_OK;
}

// Morton order of the sources (independent of the kernel; cfast_kernel and cfastmm_kernel): keys -> radix sort -> c->perm
int morton_order(kmvp_ctx* c, int64_t m_alloc) {
  int rc;
  const float* centre = (const float*)c->aux.p;  // written by measure_clouds()
  if (c->perm_ver == c->points_ver && c->perm.cap >= (size_t)m_alloc * sizeof(int)) return KMVP_OK;
  if ((rc = ensure(c, c->perm, (size_t)m_alloc * sizeof(int)))) return rc;
  SortBufs b;
  if ((rc = sort_buffers(c, m_alloc, b))) return rc;
  hipLaunchKernelGGL(cfast_morton_kernel, dim3(blocks_for(m_alloc)), dim3(256), 0, c->stream,
                     (const float*)c->y_raw.p, centre, b.keys_in, b.vals_in, c->M, m_alloc, c->D);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, sort_pairs_u32(b.tmp, &b.tmp_bytes, b.keys_in, b.keys_out, b.vals_in, (int*)c->perm.p, m_alloc, c->stream));
  c->perm_ver = c->points_ver;
  c->packed_layout = -1;  // force a re-pack
  return KMVP_OK;
}

// centred split-bf16 MFMA path (kmvp_cfast.hpp): float32, D <= 4, E == 1, every kernel.
int run_product_cfast(kmvp_ctx* c, int kernel, int sig) {
  const int D = c->D;
  const int E = 1;
  const int NE = sig == SIG_NORM ? 2 : 1;
  const int EB = sig == SIG_DENSITY ? 0 : 1;
  const int64_t N = c->N, M = c->M;
  const float scale = scale_for<float>(kernel);
  const float* x_raw = (const float*)(c->same_points ? c->y_raw.p : c->x_raw.p);
  const int64_t per_stage = (int64_t)CF_GROUP * CF_STAGE_GROUPS;
  if (c->m_total > 0x7fffffff) return fail(c, KMVP_E_UNSUPPORTED, "more than 2^31 sources");
  int rc;

  // No L2-residency pull here (l2_seg_bytes = infinity): cfast_kernel runs as fast on 8 segments as on 40 - 48 at 1e6 and at
  // 1e7 x 1.25e6 points (tools/c4_segments.py: 117.2 / 116.5 ms, 1442 / 1447 ms), and every segment costs N x 16 bytes of
  // partial sums written and read back -- config 4's shard: 48 -> 8 segments, 7.7 -> 1.3 GB.  Few targets still get more
  // segments for parallelism (2e5 points: 16).
  SegmentRule rule(CF_STAGE_BYTES, NE);
  rule.target_blocks = 24576;
  StagePlan p;
  if ((rc = stage_plan(c, (M + per_stage - 1) / per_stage, 4, CFAST_DEFAULT_TT, rule, p))) return rc;
  const int64_t n_pad = p.n_pad, m_stages = p.m_stages;
  const int TT = p.TT;
  const int64_t m_alloc = m_stages * per_stage;

  if ((rc = morton_order(c, m_alloc))) return rc;
  const PackKey key = {LAYOUT_CFAST, kernel, TT};
  if (points_stale(c, key)) {
    if ((rc = ensure(c, c->xs, (size_t)n_pad * 4 * sizeof(float)))) return rc;
    hipLaunchKernelGGL(pack_cfast_targets_kernel, dim3(blocks_for(n_pad)), dim3(256), 0, c->stream, x_raw,
                       (float*)c->xs.p, N, n_pad, D);
  }
  if (signal_stale(c, key, sig)) {
    if ((rc = ensure(c, c->rec, (size_t)m_stages * CF_STAGE_BYTES))) return rc;
    hipLaunchKernelGGL(pack_cfast_sources_kernel, dim3((unsigned)(m_alloc / CF_GROUP)), dim3(CF_GROUP), 0,
                       c->stream, (const float*)c->y_raw.p, (const float*)c->b_raw.p, (const int*)c->perm.p,
                       (unsigned char*)c->rec.p, M, D, EB, scale, c->j_offset);
  }
  HIP_TRY(c, hipGetLastError());
  record_packed(c, key, sig);

  if ((rc = ensure(c, c->part, (size_t)p.segments * NE * n_pad * sizeof(double)))) return rc;
  CfastArgs a;
  plan_args(p, a);
  a.xraw = (const float*)c->xs.p;
  a.scale = scale;
  a.img = (const unsigned char*)c->rec.p;
  a.part = (double*)c->part.p;
  a.chunk_stages = std::max<int>(1, c->opt_chunk / (int)per_stage);
  a.j_offset = c->j_offset;
  a.m_total = c->m_total;
  const dim3 grid((unsigned)p.grid);
  HIP_TRY(c, mark(c, 0));
  const auto launch = kernel == K_GAUSSIAN ? launch_cfast_gaussian : (kernel == K_ABSEXP ? launch_cfast_absexp : launch_cfast_invdist);
  const hipError_t le = launch(sig, TT, a, grid, c->stream, &c->last_kernel_name);
  if (le == hipErrorInvalidValue) return fail(c, KMVP_E_UNSUPPORTED, "fast_tiles must be 1, 2 or 4");
  HIP_TRY(c, le);
  HIP_TRY(c, mark(c, 1));

  // ---- epilogue: segments -> sums, [all-reduce over the source shards], normalise
  return reduce_and_finish(c, p.segments, NE, N, n_pad, E, sig);
}

// Several signal columns on cfast_kernel's distances (kmvp_cfastmm.hpp): exp(-r), and the Gaussian outside the radius
// rule; float32, D <= 4, any E (column blocks as for fastmm_kernel).
int run_product_cfastmm(kmvp_ctx* c, int kernel, int sig) {
  const int D = c->D, E = c->E;
  const int NE = sig == SIG_NORM ? E + 1 : E;
  const int64_t N = c->N, M = c->M;
  const int MODE = NE > 16 ? 1 : 0;
  const int64_t SB = cfm_stage_bytes(MODE);
  const float scale = scale_for<float>(kernel);
  const float* x_raw = (const float*)(c->same_points ? c->y_raw.p : c->x_raw.p);
  if (c->m_total > 0x7fffffff) return fail(c, KMVP_E_UNSUPPORTED, "more than 2^31 sources");
  const int online = (kernel == K_INVDIST || !(c->same_points || c->opt_same_global)) ? 1 : 0;  // see run_product_fastmm; 1/r: always
  int rc;

  SegmentRule rule(SB, std::min(NE, FMM_MAX_COLS));  // as run_product_fastmm
  rule.target_blocks = 4096;
  StagePlan p;
  if ((rc = stage_plan(c, (M + CF_GROUP - 1) / CF_GROUP, 2, 2, rule, p))) return rc;  // one group per stage
  const int64_t n_pad = p.n_pad, m_stages = p.m_stages;
  const int TT = p.TT;

  if ((rc = morton_order(c, m_stages * CF_GROUP))) return rc;
  const PackKey key = {LAYOUT_CFASTMM, kernel, TT + 16 * MODE};
  ColumnBlocks cb;
  if ((rc = column_blocks(c, key, sig, cb))) return rc;
  if (points_stale(c, key)) {
    if ((rc = ensure(c, c->xs, (size_t)n_pad * 4 * sizeof(float)))) return rc;
    if ((rc = ensure(c, c->rec, (size_t)m_stages * SB))) return rc;
    hipLaunchKernelGGL(pack_cfast_targets_kernel, dim3(blocks_for(n_pad)), dim3(256), 0, c->stream, x_raw,
                       (float*)c->xs.p, N, n_pad, D);
    hipLaunchKernelGGL(pack_cfastmm_points_kernel, dim3((unsigned)m_stages), dim3(CF_GROUP), 0, c->stream,
                       (const float*)c->y_raw.p, (const int*)c->perm.p, (unsigned char*)c->rec.p, M, D, MODE, scale, c->j_offset);
    HIP_TRY(c, hipGetLastError());
  }

  CfastmmArgs a;
  plan_args(p, a);
  a.xraw = (const float*)c->xs.p;
  a.img = (const unsigned char*)c->rec.p;
  a.unscale = cb.unscale;
  a.chunk_stages = std::max(1, 2 * c->opt_chunk / CF_GROUP);
  a.scale = scale;
  a.m_total = c->m_total;
  const dim3 grid((unsigned)p.grid);
  const int64_t pieces = m_stages * (CF_GROUP / 32) * (MODE ? 2 : 1) * 2 * 64;
  return run_column_blocks(
      c, key, sig, p, cb, false, online ? "cfastmm_kernel with the per-target online shift (targets != sources)" : nullptr,
      [&](int col0, int nb) {
        hipLaunchKernelGGL(pack_cfastmm_signal_kernel, dim3(blocks_for(pieces)), dim3(256), 0, c->stream,
                           (const float*)c->b_raw.p, (const float*)cb.sigma, (const int*)c->perm.p, (unsigned char*)c->rec.p,
                           M, m_stages, E, col0, nb, MODE);
      },
      [&](int nb) {
        a.NE = nb;
        a.part = (double*)c->part.p;
        hipError_t le = launch_cfastmm(kernel, MODE, TT, online, a, grid, c->stream, &c->last_kernel_name);
        if (le == hipErrorInvalidValue) return fail(c, KMVP_E_UNSUPPORTED, "no cfastmm_kernel for this kernel / tile count");
        HIP_TRY(c, le);
        return (int)KMVP_OK;
      });
}

// ---- the cell paths: cell order and tile lists ---------------------------------------------------------------------------

// Cell order of one cloud: keys -> radix sort; the sorted keys come back to the host, where the
// tile lists are built (one pass over n keys, once per kmvp_set_points).
// zq_per_unit > 0 (float32, D = 3): the fine keys of count_cut_cells (kmvp_plan.hpp) instead of the lattice's.
int cell_sort(kmvp_ctx* c, const void* pts, int64_t n, const CellGrid& grid, kmvp_ctx::DevBuf& perm,
              std::vector<unsigned>& keys, kmvp_ctx::DevBuf* keys_dev = nullptr, double zq_per_unit = 0.0) {
  int rc;
  const int D = c->D;
  const size_t keys_bytes = (size_t)n * sizeof(unsigned);
  SortBufs b;
  if ((rc = sort_buffers(c, n, b))) return rc;
  if ((rc = ensure(c, perm, (size_t)n * sizeof(int)))) return rc;
  if (c->dtype == KMVP_F64)
    hipLaunchKernelGGL(cell64_keys_kernel, dim3(blocks_for(n)), dim3(256), 0, c->stream, (const double*)pts, n, D, grid,
                       b.keys_in, b.vals_in);
  else if (zq_per_unit > 0.0)
    hipLaunchKernelGGL(cell_fine_keys_kernel, dim3(blocks_for(n)), dim3(256), 0, c->stream, (const float*)pts, n, grid,
                       zq_per_unit, b.keys_in, b.vals_in);
  else
    hipLaunchKernelGGL(cell_keys_kernel, dim3(blocks_for(n)), dim3(256), 0, c->stream, (const float*)pts, n, D, grid,
                       b.keys_in, b.vals_in);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, sort_pairs_u32(b.tmp, &b.tmp_bytes, b.keys_in, b.keys_out, b.vals_in, (int*)perm.p, n, c->stream));
  keys.resize((size_t)n);
  HIP_TRY(c, hipMemcpyAsync(keys.data(), b.keys_out, keys_bytes, hipMemcpyDeviceToHost, c->stream));
  if (keys_dev) {  // the float64 path keeps the sorted keys on the device too (source records are packed from them)
    if ((rc = ensure(c, *keys_dev, keys_bytes))) return rc;
    HIP_TRY(c, hipMemcpyAsync(keys_dev->p, b.keys_out, keys_bytes, hipMemcpyDeviceToDevice, c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return KMVP_OK;
}

// A tile list (kmvp_plan.hpp) in its device layout: [start][count][key], l.size() entries each
int upload_tiles(kmvp_ctx* c, const TileList& l, kmvp_ctx::DevBuf& grp) {
  const size_t G = l.size();
  int rc;
  if ((rc = ensure(c, grp, 3 * std::max<size_t>(G, 1) * sizeof(int)))) return rc;
  HIP_TRY(c, hipMemcpyAsync(grp.p, l.start.data(), G * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync((int*)grp.p + G, l.count.data(), G * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync((int*)grp.p + 2 * G, l.key.data(), G * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // the host vectors go out of scope
  return KMVP_OK;
}

// The grid of the cell paths: the bounding box (aux) divided, per axis, into the smallest number of equal cells
// whose side stays within h_max (so boundary cells are as full as the others).  false: more than 1024 cells on an axis.
bool cell_make_grid(const float* aux, int D, float h_max, CellGrid& grid) {
  for (int a = 0; a < 3; ++a) {
    grid.lo[a] = 0.f;
    grid.g[a] = 1;
    grid.h[a] = h_max;
    grid.inv_h[a] = 1.f / h_max;
  }
  for (int a = 0; a < D; ++a) {
    const float half = aux[FAST_AUX_HALF + a];
    grid.lo[a] = aux[a] - half;
    const double cells = std::max(1.0, std::ceil(2.0 * half / h_max));
    if (!(cells <= CELL_MAX_GRID)) return false;
    grid.g[a] = (int)cells;
    if (half > 0.f) {
      grid.h[a] = (float)(2.0 * half / cells);
      grid.inv_h[a] = 1.f / grid.h[a];
    }
  }
  return true;
}
void cell_store_grid(kmvp_ctx* c, const CellGrid& grid) {
  for (int a = 0; a < 3; ++a) {
    c->cell_lo[a] = grid.lo[a];
    c->cell_g[a] = grid.g[a];
    c->cell_hh[a] = grid.h[a];
  }
}
void cell_load_grid(const kmvp_ctx* c, CellGrid& grid) {
  for (int a = 0; a < 3; ++a) {
    grid.lo[a] = c->cell_lo[a];
    grid.g[a] = c->cell_g[a];
    grid.h[a] = c->cell_hh[a];
    grid.inv_h[a] = 1.f / c->cell_hh[a];
  }
  grid.centres = nullptr;
}
// The grid as the packers of one cloud take it: with that cloud's table of centres where the cells are count-cut (with
// same_points the sources' sort, cells and table serve both sides, as cell_sperm does)
CellGrid cell_side_grid(const kmvp_ctx* c, CellGrid grid, bool targets) {
  if (c->cell_balanced) grid.centres = (const float*)((targets && !c->same_points) ? c->cell_tcentre.p : c->cell_scentre32.p);
  return grid;
}

// ---- count-cut cells ("cell_balance": count_cut_cells, kmvp_plan.hpp) -------------------------------------------------------

// The bounds of a count-cut cell, stated once.  Accuracy: |t| = |2 d.e| <= sum_a h_a^T h_a^S / 2 with h_a the full widths
// of the target's and the source's cell, and both clouds' cells obey the same cap, so with the lattice's h_x and h_y the
// z-width may reach sqrt(2 CELL_T_MAX - h_x^2 - h_y^2) (>= the lattice's own bound: 0.1095 at h_x = h_y = 0.1).  Range:
// cellmm_scale_kernel sizes sigma_b from the real bound on |f| = 2 |e| (cellmm_fmax), so no first-order entry of A leaves
// f16 whatever the width; CELL_Z_WIDTH_MAX = 2^-3 keeps that bound in the binade of the lattice's 0.104, so that sigma_b --
// and with it the distance of the operands' mid parts from the subnormals -- is at most one power of two below the lattice's.
constexpr float CELL_Z_WIDTH_MAX = 0.125f;
constexpr float CMM_F_LATTICE = 0.104f;  // the lattice's bound on |f| in three dimensions: sqrt(2 CELL_T_MAX / 3) = 0.1033
// The cap in buckets (0: no room); *zq_per_unit buckets per unit length, *bucket the width of one
int cell_balance_cap(const CellGrid& grid, double* zq_per_unit, double* bucket) {
  const double room = 2.0 * CELL_T_MAX - (double)grid.h[0] * grid.h[0] - (double)grid.h[1] * grid.h[1];
  const double extent = (double)grid.g[2] * grid.h[2];
  *bucket = extent / CELL_ZQ;
  *zq_per_unit = CELL_ZQ / extent;
  if (!(room > 0.0) || !(extent > 0.0)) return 0;
  const double width = std::min(std::sqrt(room), (double)CELL_Z_WIDTH_MAX);
  return (int)std::min<double>(CELL_ZQ, std::floor(width / *bucket));
}

// [cell][4] floats: the lattice's x and y centres of the cell's column, the midpoint of its bucket range in z
int upload_cell_centres(kmvp_ctx* c, const CellGrid& grid, double bucket, const std::vector<CountCell>& cells, kmvp_ctx::DevBuf& buf) {
  std::vector<float> tab(4 * std::max<size_t>(cells.size(), 1), 0.f);
  for (size_t i = 0; i < cells.size(); ++i) {
    tab[4 * i + 0] = cell_centre(cells[i].column, 0, grid);
    tab[4 * i + 1] = cell_centre(cells[i].column, 1, grid);
    tab[4 * i + 2] = count_cell_zcentre(grid.lo[2], bucket, cells[i].zlo, cells[i].zhi);
  }
  int rc;
  if ((rc = ensure(c, buf, tab.size() * sizeof(float)))) return rc;
  HIP_TRY(c, hipMemcpyAsync(buf.p, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // the host vector goes out of scope
  return KMVP_OK;
}

// Cell order, cells, tables of centres and tile lists of both clouds, cut by point count, for TT tiles per wavefront: a
// second sort per cloud, with the fine keys, after the lattice sort has chosen TT.  Targets are cut to whole wavefronts
// (32 TT points) where the cap stops a cell; a cloud that is only a source to whole tiles.
int cell_prepare_balanced(kmvp_ctx* c, const CellGrid& grid, int TT, int cap, double zq_per_unit, double bucket) {
  const int64_t quantum = (int64_t)CELL_TILE * TT, full = quantum * WAVES_PER_BLOCK;
  int rc;
  std::vector<unsigned> keys;
  if ((rc = cell_sort(c, c->y_raw.p, c->M, grid, c->cell_sperm, keys, nullptr, zq_per_unit))) return rc;
  std::vector<CountCell> cells = count_cut_cells(keys.data(), c->M, cap, c->same_points ? quantum : (int64_t)CELL_TILE, full);
  const TileList sources = count_cell_source_tiles(cells);
  if ((rc = upload_tiles(c, sources, c->cell_sgrp))) return rc;
  c->cell_m_tiles = (int64_t)sources.size();
  if ((rc = upload_cell_centres(c, grid, bucket, cells, c->cell_scentre32))) return rc;
  if (!c->same_points) {
    if ((rc = cell_sort(c, c->x_raw.p, c->N, grid, c->cell_tperm, keys, nullptr, zq_per_unit))) return rc;
    cells = count_cut_cells(keys.data(), c->N, cap, quantum, full);
    if ((rc = upload_cell_centres(c, grid, bucket, cells, c->cell_tcentre))) return rc;
  }
  return upload_tiles(c, count_cell_target_tiles(cells, TT, &c->cell_n_main, &c->cell_n_rest), c->cell_tgrp);
}

// picoseconds per 32 x 32 tile of pairs of the float32 cell kernels, whole chip, by the tiles a wavefront owns
// (cellmm_kernel at the headline shape: TT = 8 / 4 / 2: 26.9 / 30.7 / 44.2 ms for 1.03e9 tiles)
inline double cell_ps_per_tile(int TT) { return TT >= 8 ? CMM_PS_PER_TILE_MAIN : (TT >= 4 ? CMM_PS_PER_TILE_TT4 : CMM_PS_PER_TILE_REST); }

// Grid and cell order of both clouds for the current points (cached per points version).
// TT > 0: target tiles per wavefront as requested; TT == 0: the largest of 8, 4, 2 whose padding of the
// target cells stays within CELL_AUTO_MAX_PAD (2 if none does).
// Leaves c->cell_state = 1 when the path can run, -1 when it cannot (D > 3, non-finite box, more
// than 1024 cells along an axis).
int cell_prepare(kmvp_ctx* c, int TT) {
  if (c->cell_ver == c->points_ver && c->cell_state != 0 && c->cell_balance_req == c->opt_cell_balance &&
      (c->cell_state < 0 || c->cell_tt_req == TT))
    return KMVP_OK;
  c->cell_tt_req = TT;
  c->cell_balance_req = c->opt_cell_balance;
  c->cell_ver = c->points_ver;
  c->cell_state = -1;
  const int D = c->D;
  if (D > CELL_MAX_D || !(c->cloud_radius2 < INFINITY) || c->N > 0x3fffffff || c->M > 0x3fffffff) return KMVP_OK;
  float aux[FAST_AUX_FLOATS];
  HIP_TRY(c, hipMemcpyAsync(aux, c->aux.p, sizeof(aux), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  CellGrid grid;
  if (!cell_make_grid(aux, D, (float)(std::sqrt(2.f * CELL_T_MAX / (float)D)), grid)) return KMVP_OK;  // |2 d.e| <= D h^2 / 2 <= the bound
  int rc;
  std::vector<unsigned> keys;
  if ((rc = cell_sort(c, c->y_raw.p, c->M, grid, c->cell_sperm, keys))) return rc;
  const TileList sources = cell_tiles(keys.data(), c->M);
  if ((rc = upload_tiles(c, sources, c->cell_sgrp))) return rc;
  c->cell_m_tiles = (int64_t)sources.size();
  if (!c->same_points && (rc = cell_sort(c, c->x_raw.p, c->N, grid, c->cell_tperm, keys))) return rc;
  if (TT == 0) {
    // auto: the group size whose two lists cost least (sparse cells of 3 - 5 tiles: groups of four and a leftover list
    // beat groups of two; dense cells: groups of eight)
    double best = INFINITY;
    for (int t : {8, 4, 2}) {
      int64_t nm, nr;
      cell_split_count(keys.data(), (int64_t)keys.size(), t, &nm, &nr);
      const double cost = cell_ps_per_tile(t) * (double)nm + cell_ps_per_tile(2) * (double)nr;
      if (cost < best) {
        best = cost;
        TT = t;
      }
    }
  }
  // count-cut cells where they apply and are asked for ("cell_balance"); otherwise the lattice's, as ever
  double zq_per_unit, bucket;
  const int cap = cell_balance_cap(grid, &zq_per_unit, &bucket);
  c->cell_balanced = false;
  if (cell_balance_taken(c->opt_cell_balance, cell_balance_applies(D, c->dtype == KMVP_F32, TT, cap), c->N, c->M)) {
    c->cell_balanced = true;  // (cell_state stays -1 until the lists are whole)
    c->cell_zw = (float)((double)cap * bucket);
    if ((rc = cell_prepare_balanced(c, grid, TT, cap, zq_per_unit, bucket))) return rc;
  } else if ((rc = upload_tiles(c, cell_tiles_split(keys.data(), (int64_t)keys.size(), TT, &c->cell_n_main, &c->cell_n_rest), c->cell_tgrp)))
    return rc;
  c->cell_n_tiles = c->cell_n_main + c->cell_n_rest;  // (both lists already padded to whole workgroups)
  c->cell_tt = TT;
  cell_store_grid(c, grid);
  c->cell_state = 1;
  c->packed_layout = -1;  // xs / rec are re-packed by whoever runs next
  return KMVP_OK;
}

// share of slots over points after padding the last tile of every cell (both clouds)
double cell_padding(const kmvp_ctx* c) {  // (empty tiles included)
  const double t = (double)c->cell_n_tiles * CELL_TILE / (double)std::max<int64_t>(c->N, 1);
  const double s = (double)c->cell_m_tiles * CELL_TILE / (double)std::max<int64_t>(c->M, 1);
  return std::max(t, s);
}

// The context's side of a CellSplit (kmvp_plan.hpp): the plan of the two grids (MAIN and REST list) of the float32 cell
// kernels for the current lists, a grid's region of c->part and its share of the kernel's arguments.
// Per path: the stage of its source image, and for the main launch the shortest segment on big problems, the L2 budget
// of a segment and the target number of workgroups.
CellSplit cell_plan(const kmvp_ctx* c, int stage_tiles, SegmentRule main) {
  return cell_split(c->N, c->cell_m_tiles, c->cell_n_main, c->cell_n_rest, c->cell_tt, c->opt_segments, stage_tiles, main);
}
double* cell_region(const kmvp_ctx* c, const CellSplit& s, int cols, int r) { return (double*)c->part.p + s.region_offset(cols, r); }
template <class Args>
void cell_args(const kmvp_ctx* c, const CellSplit& s, int cols, int r, Args& a) {
  a.part = cell_region(c, s, cols, r);
  a.n_slots = s.slots[r];
  a.tile_base = s.slot_base(r) / CELL_TILE;  // MAIN 0, TAIL behind the MAIN list's whole rounds, REST at cell_n_main
  a.seg_stages = s.seg_stages[r];
  a.segments = s.segments[r];
  a.tile_blocks = (int)s.blocks[r];
}
inline int cell_tt(const kmvp_ctx* c, int r) { return r == 1 ? CELL_REST_TT : c->cell_tt; }
// resident workgroups of cellmm16_kernel<tt> on this device (the TAIL plan's R): two per CU at eight tiles per wavefront
// (224 registers: two wavefronts per SIMD), four at four (118 registers); "cell_tail_resident" overrides it
inline int64_t cell_tail_resident(const kmvp_ctx* c, int tt) {
  return c->opt_cell_tail_resident > 0 ? c->opt_cell_tail_resident : (int64_t)c->device_cus * (tt >= 8 ? 2 : 4);
}

// The targets of the float32 cell kernels (cell_kernel, cellmm_kernel): coordinates in tile order (xs), tile centres
// (cell_tmeta), the slot of every target (cell_slot)
int pack_cell_targets(kmvp_ctx* c, const CellGrid& grid) {
  const int64_t n_tiles = c->cell_n_tiles;
  const float* x_raw = (const float*)(c->same_points ? c->y_raw.p : c->x_raw.p);
  const int* tperm = (const int*)(c->same_points ? c->cell_sperm.p : c->cell_tperm.p);
  const int* tgrp = (const int*)c->cell_tgrp.p;
  int rc;
  if ((rc = ensure(c, c->xs, (size_t)n_tiles * CELL_TILE * 4 * sizeof(float)))) return rc;
  if ((rc = ensure(c, c->cell_tmeta, (size_t)n_tiles * 4 * sizeof(float)))) return rc;
  if ((rc = ensure(c, c->cell_slot, (size_t)c->N * sizeof(int)))) return rc;
  hipLaunchKernelGGL(pack_cell_targets_kernel, dim3((unsigned)n_tiles), dim3(CELL_TILE), 0, c->stream, x_raw, tperm,
                     tgrp, tgrp + n_tiles, (const unsigned*)(tgrp + 2 * n_tiles), n_tiles, c->D,
                     cell_side_grid(c, grid, true), (float*)c->xs.p, (float*)c->cell_tmeta.p, (int*)c->cell_slot.p);
  return KMVP_OK;
}

// ---- cell-reduced Gaussian path (kmvp_cell.hpp): float32, D <= 3, E == 1 -----------------------------

int run_product_cell(kmvp_ctx* c, int sig) {
  const int D = c->D;
  const int E = 1;
  const int NE = sig == SIG_NORM ? 2 : 1;
  const int64_t N = c->N;
  // target tiles: whole groups of cell_tt, then leftover tiles in groups of 2 (cell_tiles_split)
  SegmentRule rule(CELL_STAGE_BYTES, NE);
  rule.min_seg = 4;
  const CellSplit s = cell_plan(c, CELL_STAGE_TILES, rule);
  const int64_t m_stages = s.m_stages, n_slots = s.n_slots;
  int rc;
  CellGrid grid;
  cell_load_grid(c, grid);

  const PackKey key = {LAYOUT_CELL, K_GAUSSIAN, c->cell_tt};
  const int* sgrp = (const int*)c->cell_sgrp.p;
  if (points_stale(c, key) && (rc = pack_cell_targets(c, grid))) return rc;
  if (signal_stale(c, key, sig)) {
    if ((rc = ensure(c, c->rec, (size_t)m_stages * CELL_STAGE_BYTES))) return rc;
    hipLaunchKernelGGL(pack_cell_sources_kernel, dim3((unsigned)(m_stages * CELL_STAGE_TILES)), dim3(CELL_TILE), 0,
                       c->stream, (const float*)c->y_raw.p,
                       sig == SIG_DENSITY ? (const float*)nullptr : (const float*)c->b_raw.p,
                       (const int*)c->cell_sperm.p, sgrp, sgrp + c->cell_m_tiles,
                       (const unsigned*)(sgrp + 2 * c->cell_m_tiles), c->cell_m_tiles, D, cell_side_grid(c, grid, false),
                       (unsigned char*)c->rec.p);
  }
  HIP_TRY(c, hipGetLastError());
  record_packed(c, key, sig);

  if ((rc = ensure(c, c->part, s.part_doubles(NE) * sizeof(double)))) return rc;
  CellArgs a;
  a.xd = (const float*)c->xs.p;
  a.tmeta = (const float*)c->cell_tmeta.p;
  a.img = (const unsigned char*)c->rec.p;
  a.m_stages = m_stages;
  a.chunk_stages = std::max(1, c->opt_chunk / (CELL_TILE * CELL_STAGE_TILES));
  HIP_TRY(c, mark(c, 0));
  hipError_t le = hipSuccess;
  for (int r = 0; r < CELL_LISTS && le == hipSuccess; ++r)  // (no TAIL list here: a launch per list)
    if (s.blocks[r] > 0) {
      cell_args(c, s, NE, r, a);
      le = launch_cell_gaussian(sig, cell_tt(c, r), a, dim3((unsigned)s.grid(r)), c->stream, &c->last_kernel_name);
    }
  if (le == hipErrorInvalidValue) return fail(c, KMVP_E_UNSUPPORTED, "fast_tiles must be 1, 2, 4 or 8");
  HIP_TRY(c, le);
  HIP_TRY(c, mark(c, 1));

  // ---- epilogue: segments -> sums in the caller's order, [all-reduce over the source shards], normalise
  if ((rc = ensure(c, c->sums, (size_t)NE * N * sizeof(double)))) return rc;
  if ((rc = ensure(c, c->cell_sums, (size_t)NE * n_slots * sizeof(double)))) return rc;
  for (int r = 0; r < CELL_LISTS; ++r)
    if (s.blocks[r] > 0)
      hipLaunchKernelGGL(reduce_region_kernel, dim3(blocks_for((int64_t)NE * s.slots[r])), dim3(256), 0, c->stream,
                         (const double*)cell_region(c, s, NE, r), (double*)c->cell_sums.p, s.slots[r], NE, s.segments[r], n_slots,
                         s.slot_base(r));
  hipLaunchKernelGGL(gather_cells_kernel, dim3(blocks_for((int64_t)NE * N)), dim3(256), 0, c->stream,
                     (const double*)c->cell_sums.p, (const int*)c->cell_slot.p, (double*)c->sums.p, N, n_slots, NE);
  HIP_TRY(c, hipGetLastError());
  return finish_product(c, (int64_t)NE * N, N, N, E, sig);
}

// ---- cell form with the sum over the sources in the MFMA accumulator (kmvp_cellmm.hpp): float32, D <= 3,
// E == 1, plain product / density.  Shares grid, cell order, tile lists and the target layout with cell_kernel.

// log2 of the largest W_j(T) = exp(e_j.(2 D - e_j)) on this grid: |e_a| <= w_a / 2, |D_a| <= g_a h_a, with w_a the cells'
// width: the lattice's h_a, or along z the cap of count-cut cells (both clouds obey it)
int cellmm_wlog2(const kmvp_ctx* c) {
  double arg = 0.0;
  for (int a = 0; a < c->D; ++a) {
    const double w = (c->cell_balanced && a == 2) ? (double)c->cell_zw : (double)c->cell_hh[a];
    arg += w * ((double)c->cell_g[a] * c->cell_hh[a]);
  }
  return (int)std::ceil(arg * 1.4426950408889634);
}
// The bound on |f| = 2 |e| over all axes that cellmm_scale_kernel sizes sigma_b from: the lattice's constant, or the width
// of count-cut cells along z where that is larger
float cellmm_fmax(const kmvp_ctx* c) { return c->cell_balanced ? std::max(CMM_F_LATTICE, c->cell_zw) : CMM_F_LATTICE; }

// One launch per signal column (and one with b = 1 for the denominator of normalised rows): the weights W_j b_j
// live in the MFMA's source operand, so a column is an operand, not an extra fma.  E columns cost E launches of
// ~27 us per 1e9 pairs each -- against 3.5 E VALU slots per pair for the column-blocked difference form.
int run_product_cellmm(kmvp_ctx* c, int sig) {
  const int D = c->D;
  const int E = sig == SIG_DENSITY ? 1 : c->E;
  const int NE = sig == SIG_NORM ? E + 1 : E;
  const int64_t N = c->N;
  const int TT = c->cell_tt;  // the target tile lists were built for it (cell_prepare)
  // segments of <= 3 MiB of source image (one per XCD at a time in its 4 MiB L2) and ~14 rounds of resident
  // workgroups: 8 at the headline shape.  tools/cellmm_segments.py: 8 ... 32 segments run alike (28.3-28.5 ms),
  // 4 is slower (29.0); every segment costs n_slots x 8 bytes of partial sums written and read back and one more
  // pass over the targets, so the fewest that keep the chip full are taken (HBM-side traffic 0.44 -> 0.25 GB).
  SegmentRule rule(CMM_STAGE_BYTES, 1);
  rule.min_seg = 2;
  rule.l2_seg_bytes = 3 << 20;
  rule.target_blocks = 7168;
  CellSplit s = cell_plan(c, CMM_STAGE_TILES, rule);
  const int64_t m_stages = s.m_stages, n_slots = s.n_slots;
  int rc;
  CellGrid grid;
  cell_load_grid(c, grid);
  // MFMA shape: 16x16x32 (cellmm16_kernel) sustains more under the power limit, but issues twice the MFMAs per flop:
  // 1e6 points 27.7 -> 26.6 ms, 5e5 equal, 2e5 (smaller cells' tile groups) 1.73 -> 1.96 ms (tools/cellmm_shapes.py).  What
  // counts is how full the TARGET cells are, not the pair count: one of eight ranks' share of config 2 (1e6 targets x 125 000
  // sources) gains 3 % as well (3.72 -> 3.60 ms, tools/c2_shard.py --shape)
  const int shape = c->opt_cellmm_shape >= 0 ? c->opt_cellmm_shape : ((TT >= 8 && c->N >= CELLMM16_AUTO_N && c->M >= CELLMM16_AUTO_M) ? 1 : 0);
  FusedCellGrid fg = fused_cell_grid(s, TT, c->opt_cell_fused);
  if (shape != 1) fg.fused = false;  // cellmm_kernel keeps its two launches
  // the fused grid's last, partial round of MAIN workgroups in short segments: the TAIL list (cell_tail_split, kmvp_plan.hpp)
  const int64_t resident = cell_tail_resident(c, TT);
  if ((CMM16_WHOLE_ROUNDS || cell_tail_taken(c->opt_cell_tail, TT, fg.fused, c->N, c->M)) && fg.fused &&
      cell_tail_split(s, TT, resident, small_problem(N) ? 1 : rule.min_seg)) {
    fg = fused_cell_grid(s, TT, 1);
    c->note = std::string(c->note.empty() ? "" : c->note + "; ") + "tail list: the last " + std::to_string(s.blocks[2]) +
              " target blocks in " + std::to_string(s.segments[2]) + " segments (cell_tail)";
  }
  {
    const int64_t info[8] = {s.blocks[0], s.blocks[2], s.blocks[1], s.segments[0], s.segments[2], s.segments[1], resident, fg.fused ? 1 : 0};
    memcpy(c->cell_list_info, info, sizeof info);
  }

  const PackKey key = {LAYOUT_CELLMM, K_GAUSSIAN, TT};
  // the image holds ONE column's signal: it can be reused only by single-column products
  const int image_sig = NE > 1 ? -1 : sig;
  const bool sig_stale = signal_stale(c, key, image_sig);
  const int* sgrp = (const int*)c->cell_sgrp.p;
  if ((rc = ensure(c, c->cell_scale, 64))) return rc;
  float* scale = (float*)c->cell_scale.p;
  unsigned* bmax = (unsigned*)c->cell_scale.p + 4;
  HIP_TRY(c, mark(c, 0));
  if (points_stale(c, key)) {
    if ((rc = pack_cell_targets(c, grid))) return rc;
    if ((rc = ensure(c, c->rec, (size_t)m_stages * CMM_STAGE_BYTES))) return rc;
    hipLaunchKernelGGL(pack_cellmm_points_kernel, dim3((unsigned)(m_stages * CMM_STAGE_TILES)), dim3(CELL_TILE), 0,
                       c->stream, (const float*)c->y_raw.p, (const int*)c->cell_sperm.p, sgrp, sgrp + c->cell_m_tiles,
                       (const unsigned*)(sgrp + 2 * c->cell_m_tiles), c->cell_m_tiles, D, cell_side_grid(c, grid, false),
                       (unsigned char*)c->rec.p);
    HIP_TRY(c, hipGetLastError());
  }
  record_packed(c, key, image_sig);

  if ((rc = ensure(c, c->part, s.part_doubles(1) * sizeof(double)))) return rc;
  if ((rc = ensure(c, c->sums, (size_t)NE * N * sizeof(double)))) return rc;
  if ((rc = ensure(c, c->cell_sums, (size_t)NE * n_slots * sizeof(double)))) return rc;
  CellmmArgs a;
  a.xd = (const float*)c->xs.p;
  a.tmeta = (const float*)c->cell_tmeta.p;
  a.img = (const unsigned char*)c->rec.p;
  a.scale = scale;
  a.m_stages = m_stages;
  a.shared_build = cell_shared_build(TT, c->opt_cell_shared_build) ? 1 : 0;  // the kernel decides per workgroup (cellmm16_one_cell)
  if (NE == 1 && !sig_stale) HIP_TRY(c, mark(c, 0));  // resident signal: the timed region is the pair loop alone
  for (int col = 0; col < NE; ++col) {
    if (sig_stale) {  // the signal part of the image: max |b| -> sigma_b -> b sigma_b in tile order
      const float* b = (sig == SIG_DENSITY || col == E) ? (const float*)nullptr : (const float*)c->b_raw.p;
      HIP_TRY(c, hipMemsetAsync(bmax, 0, sizeof(unsigned), c->stream));
      if (b)
        hipLaunchKernelGGL(cellmm_absmax_kernel, dim3((unsigned)std::min<int64_t>(1024, (c->M + 255) / 256)), dim3(256), 0,
                           c->stream, b, c->M, E, col, bmax);
      hipLaunchKernelGGL(cellmm_scale_kernel, dim3(1), dim3(1), 0, c->stream, (const unsigned*)bmax, cellmm_wlog2(c),
                         cellmm_fmax(c), b ? 0 : 1, scale);
      hipLaunchKernelGGL(pack_cellmm_signal_kernel, dim3((unsigned)(m_stages * CMM_STAGE_TILES)), dim3(CELL_TILE), 0,
                         c->stream, b, E, col, (const int*)c->cell_sperm.p, sgrp, sgrp + c->cell_m_tiles, c->cell_m_tiles,
                         (const float*)scale, (unsigned char*)c->rec.p);
      HIP_TRY(c, hipGetLastError());
      if (NE == 1) HIP_TRY(c, mark(c, 0));
    }
    // cellmm16_kernel takes all lists in ONE launch, the MAIN list's workgroups, then the TAIL list's (if any), then the REST
    // list's (fused_cell_grid, kmvp_plan.hpp); otherwise the MAIN list, then the REST list, a launch each
    hipError_t le = hipSuccess;
    if (fg.fused) {
      CellmmArgs ar = a, at = a;
      cell_args(c, s, 1, 0, a);
      cell_args(c, s, 1, 1, ar);
      cell_args(c, s, 1, 2, at);
      le = launch_cellmm16_fused(TT, a, ar, at, fg.main_grid, fg.tail_grid, fg.rest_grid, c->stream, &c->last_kernel_name);
    } else {
      for (int r = 0; r < CELL_LISTS && le == hipSuccess; ++r)
        if (s.blocks[r] > 0) {
          cell_args(c, s, 1, r, a);
          le = launch_cellmm_gaussian(cell_tt(c, r), shape, a, dim3((unsigned)s.grid(r)), c->stream, &c->last_kernel_name);
        }
    }
    if (le == hipErrorInvalidValue) return fail(c, KMVP_E_UNSUPPORTED, "fast_tiles must be 1, 2, 4 or 8");
    HIP_TRY(c, le);
    if (NE == 1) HIP_TRY(c, mark(c, 1));
    // segments -> this column's sums in cell order (each launch's region with its own number of segments)
    double* col_sums = (double*)c->cell_sums.p + (size_t)col * n_slots;
    for (int r = 0; r < CELL_LISTS; ++r)
      if (s.blocks[r] > 0)
        hipLaunchKernelGGL(reduce_segments_kernel, dim3(blocks_for(s.slots[r])), dim3(256), 0, c->stream,
                           (const double*)cell_region(c, s, 1, r), col_sums + s.slot_base(r), s.slots[r], s.segments[r], 0);
    HIP_TRY(c, hipGetLastError());
  }
  if (NE > 1) HIP_TRY(c, mark(c, 1));  // several columns: the "kernel" time covers every column's pack + pair loop

  // ---- epilogue: back to the caller's order, [all-reduce over the source shards], normalise
  hipLaunchKernelGGL(gather_cells_kernel, dim3(blocks_for((int64_t)NE * N)), dim3(256), 0, c->stream,
                     (const double*)c->cell_sums.p, (const int*)c->cell_slot.p, (double*)c->sums.p, N, n_slots, NE);
  HIP_TRY(c, hipGetLastError());
  return finish_product(c, (int64_t)NE * N, N, N, E, sig);
}

// ---- float64 cell path (kmvp_cell64.hpp): Gaussian, D <= 3, E == 1, plain product ----------------------

// Grid, cell order, target tiles of 64 and the list of source cells for the current points.
int cell64_prepare(kmvp_ctx* c) {
  if (c->cell_ver == c->points_ver && c->cell_state != 0) return KMVP_OK;
  c->cell_ver = c->points_ver;
  c->cell_state = -1;
  const int D = c->D;
  if (D > CELL_MAX_D || !(c->cloud_radius2 < INFINITY) || c->N > 0x3fffffff || c->M > 0x3fffffff) return KMVP_OK;
  float aux[FAST_AUX_FLOATS];
  HIP_TRY(c, hipMemcpyAsync(aux, c->aux.p, sizeof(aux), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  CellGrid grid;
  if (!cell_make_grid(aux, D, (float)((float)std::sqrt(2.0 * CELL64_T_MAX / (double)D)), grid)) return KMVP_OK;  // |2 d.e| <= D h^2 / 2 <= the bound
  int rc;
  std::vector<unsigned> keys;
  if ((rc = cell_sort(c, c->y_raw.p, c->M, grid, c->cell_sperm, keys, &c->cell_skey))) return rc;
  // source cells: [first record, count] and centres
  std::vector<int> runs;
  std::vector<double> centres;
  for_each_key_run(keys.data(), c->M, [&](int64_t first, int64_t count, unsigned key) {
    runs.push_back((int)first);
    runs.push_back((int)count);
    for (int a = 0; a < 3; ++a) centres.push_back(a < D ? cell64_centre(key, a, grid) : 0.0);
    centres.push_back(0.0);
  });
  c->cell_m_tiles = (int64_t)runs.size() / 2;  // number of source cells
  if ((rc = ensure(c, c->cell_sgrp, runs.size() * sizeof(int)))) return rc;
  if ((rc = ensure(c, c->cell_scentre, centres.size() * sizeof(double)))) return rc;
  HIP_TRY(c, hipMemcpyAsync(c->cell_sgrp.p, runs.data(), runs.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->cell_scentre.p, centres.data(), centres.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (!c->same_points && (rc = cell_sort(c, c->x_raw.p, c->N, grid, c->cell_tperm, keys))) return rc;
  const TileList targets = cell_tiles(keys.data(), (int64_t)keys.size(), CELL64_TILE);
  if ((rc = upload_tiles(c, targets, c->cell_tgrp))) return rc;
  c->cell_n_tiles = (int64_t)targets.size();
  c->cell_tt = 1;
  cell_store_grid(c, grid);
  c->cell_state = 1;
  c->packed_layout = -1;
  return KMVP_OK;
}

int run_product_cell64(kmvp_ctx* c, int sig) {
  const int D = c->D;
  const int NE = sig == SIG_NORM ? 2 : 1;
  const int64_t N = c->N, M = c->M;
  const int64_t n_tiles = round_up(c->cell_n_tiles, WAVES_PER_BLOCK);
  const int64_t n_slots = n_tiles * CELL64_TILE;
  const int64_t tile_blocks = n_tiles / WAVES_PER_BLOCK;
  const int n_scells = (int)c->cell_m_tiles;
  int rc;
  CellGrid grid;
  cell_load_grid(c, grid);
  // segments of whole source cells: enough workgroups for a few rounds of the chip
  int64_t seg = c->opt_segments > 0 ? c->opt_segments : (8192 + tile_blocks - 1) / tile_blocks;
  seg = std::max<int64_t>(1, std::min<int64_t>(seg, n_scells));
  const int seg_cells = (int)((n_scells + seg - 1) / seg);
  const int segments = (n_scells + seg_cells - 1) / seg_cells;

  const PackKey key = {LAYOUT_CELL64, K_GAUSSIAN, 1};  // (no tile count: T = 1)
  const double* x_raw = (const double*)(c->same_points ? c->y_raw.p : c->x_raw.p);
  const int* tperm = (const int*)(c->same_points ? c->cell_sperm.p : c->cell_tperm.p);
  const int* tgrp = (const int*)c->cell_tgrp.p;
  if (points_stale(c, key)) {
    if ((rc = ensure(c, c->xs, (size_t)n_slots * 4 * sizeof(double)))) return rc;
    if ((rc = ensure(c, c->cell_tmeta, (size_t)n_tiles * 4 * sizeof(double)))) return rc;
    if ((rc = ensure(c, c->cell_slot, (size_t)N * sizeof(int)))) return rc;
    hipLaunchKernelGGL(pack_cell64_targets_kernel, dim3((unsigned)n_tiles), dim3(CELL64_TILE), 0, c->stream, x_raw, tperm,
                       tgrp, tgrp + c->cell_n_tiles, (const unsigned*)(tgrp + 2 * c->cell_n_tiles), c->cell_n_tiles, D,
                       grid, (double*)c->xs.p, (double*)c->cell_tmeta.p, (int*)c->cell_slot.p);
  }
  if (signal_stale(c, key, sig)) {
    const int64_t m_alloc = M + 64;  // zero records behind the last cell: the W pass reads whole groups of 64
    if ((rc = ensure(c, c->rec, (size_t)m_alloc * 4 * sizeof(double)))) return rc;
    hipLaunchKernelGGL(pack_cell64_sources_kernel, dim3(blocks_for(m_alloc)), dim3(256), 0, c->stream,
                       (const double*)c->y_raw.p, sig == SIG_DENSITY ? (const double*)nullptr : (const double*)c->b_raw.p,
                       (const int*)c->cell_sperm.p, (const unsigned*)c->cell_skey.p, M, m_alloc, D, grid, (double*)c->rec.p);
  }
  HIP_TRY(c, hipGetLastError());
  record_packed(c, key, sig);

  if ((rc = ensure(c, c->part, (size_t)segments * NE * n_slots * sizeof(double)))) return rc;
  Cell64Args a;
  a.xd = (const double*)c->xs.p;
  a.tmeta = (const double*)c->cell_tmeta.p;
  a.srec = (const double*)c->rec.p;
  a.scell = (const int*)c->cell_sgrp.p;
  a.scentre = (const double*)c->cell_scentre.p;
  a.part = (double*)c->part.p;
  a.n_slots = n_slots;
  a.n_scells = n_scells;
  a.seg_cells = seg_cells;
  a.segments = segments;
  a.tile_blocks = (int)tile_blocks;
  const dim3 grid_dim((unsigned)(tile_blocks * segments));
  HIP_TRY(c, mark(c, 0));
  HIP_TRY(c, launch_cell64_gaussian(sig, a, grid_dim, c->stream, &c->last_kernel_name));
  HIP_TRY(c, mark(c, 1));

  if ((rc = ensure(c, c->sums, (size_t)NE * N * sizeof(double)))) return rc;
  if ((rc = ensure(c, c->cell_sums, (size_t)NE * n_slots * sizeof(double)))) return rc;
  hipLaunchKernelGGL(reduce_segments_kernel, dim3(blocks_for((int64_t)NE * n_slots)), dim3(256), 0, c->stream,
                     (const double*)c->part.p, (double*)c->cell_sums.p, (int64_t)NE * n_slots, segments, 0);
  hipLaunchKernelGGL(gather_cells_kernel, dim3(blocks_for((int64_t)NE * N)), dim3(256), 0, c->stream,
                     (const double*)c->cell_sums.p, (const int*)c->cell_slot.p, (double*)c->sums.p, N, n_slots, NE);
  HIP_TRY(c, hipGetLastError());
  return finish_product(c, (int64_t)NE * N, N, N, 1, sig);
}

// ---- the rules of the dispatch (run_product, prepare_points), each stated once

// The radius rule: the squared half-diagonal of the clouds' bounding box in the kernel's scaled coordinates is within
// FAST_AUTO_RADIUS2 -- where the expanded forms of the squared distance are as accurate as the difference form
float scaled_radius2(const kmvp_ctx* c, int kernel) {
  const float sc = scale_for<float>(kernel);
  return c->cloud_radius2 * sc * sc;
}
bool radius_ok(const kmvp_ctx* c, int kernel) { return scaled_radius2(c, kernel) <= FAST_AUTO_RADIUS2; }

bool big_clouds(const kmvp_ctx* c) { return c->N >= SMALL_PROBLEM_TARGETS && c->M >= SMALL_PROBLEM_TARGETS; }

// Target tiles per wavefront of the float32 cell lists: as requested ("fast_tiles"), else 1 for few targets, else 0
// (cell_prepare takes the cheapest grouping)
int cell_tiles_request(const kmvp_ctx* c) {
  return c->opt_fast_tiles > 0 ? c->opt_fast_tiles : (c->N < SMALL_PROBLEM_TARGETS ? 1 : 0);
}

// cellmm_kernel's f16 operands have the range: clouds inside the radius rule, weights W_j <= 2^CMM_MAX_WLOG2 on the grid
bool cellmm_in_range(const kmvp_ctx* c) { return radius_ok(c, K_GAUSSIAN) && cellmm_wlog2(c) <= CMM_MAX_WLOG2; }

// Whether the float32 cell form (Gaussian, D <= 3) is worth building: forced (fast_sqdists >= 3), or in auto for big
// clouds inside the radius rule.  Several signal columns have cellmm_kernel alone (no cell_kernel to fall back on): they
// need the radius rule even when forced, and fast_sqdists = 4 (cell_kernel) rules them out.
bool cells_considered(const kmvp_ctx* c, bool several) {
  if (several && (c->opt_fast == 4 || !radius_ok(c, K_GAUSSIAN))) return false;
  return c->opt_fast >= 3 || (c->opt_fast < 0 && radius_ok(c, K_GAUSSIAN) && big_clouds(c));
}

// ok: the float32 cell form serves this product -- it is considered, the cell lists of the current points apply
// (cell_prepare) and, unless forced, pad the tiles by at most CELL_AUTO_MAX_PAD; several columns also need cellmm_kernel's
// operand range.  A refusal leaves its reason in the dispatch note (kmvp_last_dispatch_note): the fastest paths are
// narrow, and a caller who gets 5e12 instead of 3.7e13 pairs/s should be told which condition failed.
int cells_usable(kmvp_ctx* c, bool several, bool& ok) {
  const bool forced = c->opt_fast >= 3;
  ok = false;
  if (cells_considered(c, several)) {
    const int rc = cell_prepare(c, cell_tiles_request(c));
    if (rc) return rc;
    ok = c->cell_state == 1 && (forced || cell_padding(c) <= CELL_AUTO_MAX_PAD) && (!several || cellmm_in_range(c));
    if (ok) return KMVP_OK;
  }
  char buf[256];
  if (c->opt_fast >= 0 && !forced) {
    snprintf(buf, sizeof buf, "cell form not considered: fast_sqdists = %d was requested", c->opt_fast);
  } else if (!radius_ok(c, K_GAUSSIAN)) {
    snprintf(buf, sizeof buf, "cell form not taken: squared half-diagonal of the clouds' bounding box %.3g > %.3g (radius rule)",
             (double)scaled_radius2(c, K_GAUSSIAN), (double)FAST_AUTO_RADIUS2);
  } else if (!big_clouds(c)) {
    snprintf(buf, sizeof buf, "cell form not taken: fewer than %lld points in a cloud (N = %lld, M = %lld)",
             (long long)SMALL_PROBLEM_TARGETS, (long long)c->N, (long long)c->M);
  } else if (c->cell_state != 1) {
    snprintf(buf, sizeof buf, "cell form not taken: the grid does not apply (non-finite box or more than %d cells along an axis)",
             CELL_MAX_GRID);
  } else {
    snprintf(buf, sizeof buf, "cell form not taken: padding the cells' tiles would use %.0f %% of the slots (limit %.0f %%): too few "
             "points per grid cell", 100.0 * cell_padding(c), 100.0 * CELL_AUTO_MAX_PAD);
  }
  c->note = buf;
  return KMVP_OK;
}

// Whether the float64 cell form (kmvp_cell64.hpp) is worth building: forced (fast_sqdists = 3), or in auto for big clouds
bool cells64_considered(const kmvp_ctx* c) { return c->opt_fast == 3 || (c->opt_fast < 0 && big_clouds(c)); }

// Whether the product ends in finish_product_shifted (per-target exponents: all-reduce MIN, then SUM): exp(<x,y>), and the
// bf16 Gaussian with targets != sources (K_GAUSSIAN_SHIFTED; an explicit "mfma_variant" asks for the plain kernel).  Every
// rank must agree, one with an empty source slice included.
bool takes_shifted_tail(const kmvp_ctx* c, int kernel) {
  return kernel == K_EXPDOT || (c->dtype == KMVP_BF16 && kernel == K_GAUSSIAN && !(c->same_points || c->opt_same_global) &&
                                c->opt_mfma_variant < 0 && mfma_ksteps_shifted(c->D) <= MFMA_MAX_KS);
}

// bf16 MFMA path (kmvp_mfma.hpp): host arrays are float32, points and signal are packed
// to augmented bf16 rows / LDS tile images, sums come back as fp32 partials.
int run_product_mfma(kmvp_ctx* c, int kernel, int sig) {
  const int D = c->D;
  const int E = sig == SIG_DENSITY ? 1 : c->E;
  const int NE = sig == SIG_NORM ? E + 1 : E;
  const int64_t N = c->N, M = c->M;
  // exp(<x,y>) (include/kmvp.h kmvp_expdot, bfloat16): S = X Y^T log2(e) straight from the matrix pipe, the per-target
  // running shift of kmvp_mfma.hpp, partial sums as (mantissa, exponent) pairs and the shifted tail
  // The Gaussian with targets != sources takes the same running shift (K_GAUSSIAN_SHIFTED): a target farther than ~9 kernel
  // lengths from every source would otherwise have its whole row under the float32 range (0, or 0/0 when normalised) -- the
  // bf16 counterpart of what fastmm_kernel / cfastmm_kernel do for float32.  Targets == sources keep the plain kernel (every
  // row contains k = 1); exp(-r) would need r > 87 and stays plain.
  const bool dot = takes_shifted_tail(c, kernel);  // (mantissa, exponent) partial sums and the shifted tail
  const bool shifted = dot && kernel == K_GAUSSIAN;
  if (shifted) kernel = K_GAUSSIAN_SHIFTED;
  const int KS = kernel == K_EXPDOT ? mfma_ksteps_dot(D) : (shifted ? mfma_ksteps_shifted(D) : mfma_ksteps(D));
  const int NT = (E + 31) / 32;
  if (KS > MFMA_MAX_KS || NT > MFMA_MAX_NT)
    return fail(c, KMVP_E_UNSUPPORTED, "bf16 MFMA path is instantiated for D <= 138 (exp(<x,y>): 141) and E <= 128");
  const int KD = 16 * KS;
  const int NEP = NT * 32;
  const int64_t IMG = mfma_image_bytes(KS, NT);
  const float scale = kernel == K_EXPDOT ? 1.2011224087864498f /* sqrt(log2 e) on both sides */
                                         : scale_for<float>(shifted ? (int)K_GAUSSIAN : kernel);
  const int pack_mode = kernel == K_EXPDOT ? 1 : (shifted ? 2 : 0);
  const float* x_raw = (const float*)(c->same_points ? c->y_raw.p : c->x_raw.p);
  // target tiles of 32 per wave ("targets_per_lane" option): 1, 2, or (default, where instantiated)
  // 2 with the software-pipelined kernel
  const int TW = c->opt_T == 1 ? 1 : 2;
  const bool pipelined = TW == 2 && c->opt_T != 2 && KS <= MFMA_PIPE_MAX_KS && NT <= MFMA_PIPE_MAX_NT;
  // variant of the pipelined kernel (kmvp_mfma.hpp VAR): exp(-r) (two transcendentals per pair) by default with the loop
  // rotated by one transcendental stage; the denominators stay on the VALU -- on the matrix pipe they save 2 % of the
  // cycles and nothing of the time under the power limit (profiles/r03_c3_variants.txt); the single-transcendental kernels
  // gain nothing from either
  const int variant = dot ? 0 : (c->opt_mfma_variant >= 0 ? c->opt_mfma_variant : (kernel == K_ABSEXP ? 4 : 0));
  const int64_t tile = (int64_t)MFMA_TILE * TW * WAVES_PER_BLOCK;
  const int64_t n_pad = round_up(N, tile);
  const int64_t tile_blocks = n_pad / tile;
  const int64_t m_tiles = (M + MFMA_TILE - 1) / MFMA_TILE;
  int rc;

  // segments: enough workgroups for >= 4 per CU, at least 8 source tiles each
  int64_t seg = c->opt_segments > 0 ? c->opt_segments : (1024 + tile_blocks - 1) / tile_blocks;
  seg = std::max<int64_t>(1, std::min<int64_t>(seg, std::max<int64_t>(1, m_tiles / 8)));
  if (seg >= 8) seg = seg / 8 * 8;
  const int64_t seg_tiles = (m_tiles + seg - 1) / seg;
  const int segments = (int)((m_tiles + seg_tiles - 1) / seg_tiles);

  const PackKey key = {LAYOUT_MFMA, kernel, TW};
  HIP_TRY(c, mark(c, 0));
  if (points_stale(c, key)) {
    if ((rc = ensure(c, c->xs, (size_t)n_pad * KD * 2))) return rc;
    hipLaunchKernelGGL(pack_mfma_targets_kernel, dim3(blocks_for(n_pad)), dim3(256), 0, c->stream,
                       x_raw, (__bf16*)c->xs.p, N, n_pad, D, KD, scale, pack_mode);
  }
  if (signal_stale(c, key, sig)) {
    if ((rc = ensure(c, c->rec, (size_t)m_tiles * IMG))) return rc;
    hipLaunchKernelGGL(pack_mfma_sources_kernel, dim3(blocks_for(m_tiles * MFMA_TILE)), dim3(256), 0,
                       c->stream, (const float*)c->y_raw.p,
                       sig == SIG_DENSITY ? (const float*)nullptr : (const float*)c->b_raw.p,
                       (unsigned char*)c->rec.p, M, m_tiles, D, E, KS, NT, scale, pack_mode);
  }
  HIP_TRY(c, hipGetLastError());
  record_packed(c, key, sig);

  if ((rc = ensure(c, c->part, (size_t)segments * n_pad * NEP * sizeof(float)))) return rc;
  if ((rc = ensure(c, c->partd, (size_t)segments * n_pad * sizeof(float)))) return rc;
  MfmaArgs a;
  a.xa = (const __bf16*)c->xs.p;
  a.img = (const unsigned char*)c->rec.p;
  a.part = (float*)c->part.p;
  a.partd = (float*)c->partd.p;
  a.n_pad = n_pad;
  a.m_tiles = m_tiles;
  a.seg_tiles = seg_tiles;
  a.segments = segments;
  a.tile_blocks = (int)tile_blocks;
  a.j_offset = c->j_offset;
  a.m_total = c->m_total;
  a.kexp = nullptr;
  if (dot) {
    if ((rc = ensure(c, c->kexp, (size_t)segments * n_pad * sizeof(float)))) return rc;
    if ((rc = ensure(c, c->kshift, (size_t)n_pad * sizeof(double)))) return rc;
    a.kexp = (float*)c->kexp.p;
  }
  const dim3 grid((unsigned)(tile_blocks * segments));
  HIP_TRY(c, mark(c, 0));
  hipError_t le;
  switch (kernel) {
    case K_EXPDOT: le = launch_mfma_expdot(KS, NT, pipelined ? 3 : TW, a, grid, c->stream, &c->last_kernel_name); break;
    case K_GAUSSIAN_SHIFTED: le = launch_mfma_gaussian_shifted(KS, NT, pipelined ? 3 : TW, a, grid, c->stream, &c->last_kernel_name); break;
    case K_GAUSSIAN: le = launch_mfma_gaussian(KS, NT, pipelined ? 3 + variant : TW, a, grid, c->stream, &c->last_kernel_name); break;
    case K_ABSEXP: le = launch_mfma_absexp(KS, NT, pipelined ? 3 + variant : TW, a, grid, c->stream, &c->last_kernel_name); break;
    default: le = launch_mfma_invdist(KS, NT, pipelined ? 3 + variant : TW, a, grid, c->stream, &c->last_kernel_name); break;
  }
  HIP_TRY(c, le);
  HIP_TRY(c, mark(c, 1));

  const int64_t count = (int64_t)NE * n_pad;
  if ((rc = ensure(c, c->sums, (size_t)count * sizeof(double)))) return rc;
  if (dot) {
    hipLaunchKernelGGL(mfma_reduce_shifted_kernel, dim3(blocks_for(count)), dim3(256), 0, c->stream,
                       (const float*)c->part.p, (const float*)c->partd.p, (const float*)c->kexp.p, (double*)c->sums.p,
                       (double*)c->kshift.p, n_pad, NEP, E, segments, sig == SIG_NORM ? 1 : 0);
    HIP_TRY(c, hipGetLastError());
    c->note = shifted ? "bf16 Gaussian with the per-target online shift (targets != sources)"
                      : "exp(<x,y>) on the bf16 matrix cores with the per-target online shift, (mantissa, exponent) partial sums";
    return finish_product_shifted(c, N, n_pad, E, sig);
  }
  hipLaunchKernelGGL(mfma_reduce_kernel, dim3(blocks_for(count)), dim3(256), 0, c->stream,
                     (const float*)c->part.p, (const float*)c->partd.p, (double*)c->sums.p, n_pad, NEP,
                     E, segments, sig == SIG_NORM ? 1 : 0);
  HIP_TRY(c, hipGetLastError());
  return finish_product(c, count, N, n_pad, E, sig);
}

}  // namespace

// Centre and squared half-diagonal of the bounding box of the clouds just uploaded by
// kmvp_set_points (float32, D <= 7 only: the inputs of the split-bf16 path and of its "auto"
// rule).  The launch and the 4-byte read-back are queued on the context's stream; the caller
// synchronises.
int measure_clouds(kmvp_ctx* c, int dtype, int64_t M, int64_t N, int D) {
  c->cloud_radius2 = INFINITY;
  // float32: inputs of the split-bf16 paths and of their "auto" rule; float64: the grid of the cell path (D <= 3)
  const bool f64_cells = dtype == KMVP_F64 && D <= CELL_MAX_D;
  if ((dtype != KMVP_F32 && !f64_cells) || D > FMM_MAX_D || M <= 0 || N <= 0) return KMVP_OK;  // (aux holds D <= 64 centres)
  int rc;
  if ((rc = ensure(c, c->aux, (FAST_AUX_FLOATS + 2 * (size_t)FAST_BBOX_BLOCKS * D) * sizeof(float)))) return rc;
  float* part = (float*)c->aux.p + FAST_AUX_FLOATS;
  if (f64_cells)  // box in float32 (the cells only need it to a grid spacing), outward rounding is not needed: keys are clamped
    hipLaunchKernelGGL((fast_bbox_partial_kernel<double>), dim3(FAST_BBOX_BLOCKS), dim3(256), 0, c->stream,
                       (const double*)c->y_raw.p, M, c->same_points ? (const double*)nullptr : (const double*)c->x_raw.p, N,
                       D, part);
  else
    hipLaunchKernelGGL((fast_bbox_partial_kernel<float>), dim3(FAST_BBOX_BLOCKS), dim3(256), 0, c->stream,
                       (const float*)c->y_raw.p, M, c->same_points ? (const float*)nullptr : (const float*)c->x_raw.p, N,
                       D, part);
  hipLaunchKernelGGL(fast_center_kernel, dim3(1), dim3(FAST_BBOX_BLOCKS), 0, c->stream, (const float*)part, D,
                     (float*)c->aux.p);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(&c->cloud_radius2, (float*)c->aux.p + FAST_AUX_RADIUS2, sizeof(float),
                            hipMemcpyDeviceToHost, c->stream));
  c->centre_ver = c->points_ver + 1;  // kmvp_set_points bumps points_ver once the upload is complete
  return KMVP_OK;
}

// kmvp_fit: the cell structures of the Gaussian paths depend on the points only, so they can be built
// before any signal exists (the rules are those of run_product() with E = 1 assumed).
int prepare_points(kmvp_ctx* c, int kernel) {
  if (kernel != K_GAUSSIAN || c->D > CELL_MAX_D || c->N == 0 || c->M == 0 || c->centre_ver != c->points_ver) return KMVP_OK;
  if (c->dtype == KMVP_F32 && cells_considered(c, false)) return cell_prepare(c, cell_tiles_request(c));
  if (c->dtype == KMVP_F64 && cells64_considered(c)) return cell64_prepare(c);
  return KMVP_OK;
}

// kmvp_cell_layout: the cell structures of the last product on the cell form, read back from what its kernel read -- the
// stage headers of the source image (float64: the list of source cells), the target tiles' records and the slot of every
// target.  Nothing is recomputed from the grid, so a model that takes the answer as data restates no rule of the lists.
// Read-only: no buffer of the context is written.  A point that no tile holds keeps -1, one held twice gets -2.
int cell_layout_read(kmvp_ctx* c, int64_t* info, double* sigma_b, int32_t* source_cell, int32_t* target_cell,
                     double* source_centres, int64_t source_cap, double* target_centres, int64_t target_cap) {
  if (!info) return fail(c, KMVP_E_INVALID, "kmvp_cell_layout: info is NULL");
  const int layout = c->packed_layout;
  const bool f64 = layout == LAYOUT_CELL64;
  if (!c->have_points || c->cell_state != 1 || c->cell_ver != c->points_ver || c->packed_points_ver != c->points_ver ||
      (layout != LAYOUT_CELL && layout != LAYOUT_CELLMM && !f64) || f64 != (c->dtype == KMVP_F64))
    return fail(c, KMVP_E_INVALID, "kmvp_cell_layout: no product on the cell form has run on the current points");
  const int64_t M = c->M, N = c->N;
  const int tile = f64 ? CELL64_TILE : CELL_TILE;
  const int* sperm_d = (const int*)c->cell_sperm.p;
  std::vector<int> sperm((size_t)M);
  HIP_TRY(c, hipMemcpyAsync(sperm.data(), sperm_d, (size_t)M * sizeof(int), hipMemcpyDeviceToHost, c->stream));

  // ---- sources: cell of every source and the centres, in the order the kernels walk the cells
  std::vector<int32_t> scell((size_t)M, -1);
  std::vector<double> scen;
  auto assign = [](std::vector<int32_t>& of, int64_t idx, int64_t n, int32_t id) {
    if (idx < 0 || idx >= n) return false;
    of[(size_t)idx] = of[(size_t)idx] == -1 ? id : -2;
    return true;
  };
  bool sound = true;
  if (f64) {
    const int64_t cells = c->cell_m_tiles;  // (cell64_prepare: the number of source cells)
    std::vector<int> runs((size_t)cells * 2);
    std::vector<double> cen((size_t)cells * 4);
    HIP_TRY(c, hipMemcpyAsync(runs.data(), c->cell_sgrp.p, runs.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(cen.data(), c->cell_scentre.p, cen.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int64_t sc = 0; sc < cells; ++sc) {
      for (int a = 0; a < 3; ++a) scen.push_back(cen[(size_t)sc * 4 + a]);
      for (int64_t p = runs[2 * sc]; p < (int64_t)runs[2 * sc] + runs[2 * sc + 1]; ++p)
        sound = sound && p >= 0 && p < M && assign(scell, sperm[(size_t)p], M, (int32_t)sc);
    }
  } else {
    const int stage_tiles = layout == LAYOUT_CELL ? CELL_STAGE_TILES : CMM_STAGE_TILES;
    const int hdr_off = layout == LAYOUT_CELL ? CELL_HDR_OFF : CMM_HDR_OFF;
    const int stage_bytes = layout == LAYOUT_CELL ? CELL_STAGE_BYTES : CMM_STAGE_BYTES;
    const int64_t m_tiles = c->cell_m_tiles, m_stages = (m_tiles + stage_tiles - 1) / stage_tiles;
    std::vector<int> grp((size_t)m_tiles * 3);
    std::vector<float> hdr((size_t)m_stages * stage_tiles * 4);
    HIP_TRY(c, hipMemcpyAsync(grp.data(), c->cell_sgrp.p, grp.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (m_stages > 0)
      HIP_TRY(c, hipMemcpy2DAsync(hdr.data(), (size_t)stage_tiles * 16, (const unsigned char*)c->rec.p + hdr_off, (size_t)stage_bytes,
                                  (size_t)stage_tiles * 16, (size_t)m_stages, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    int key_s = -2;  // a new cell begins where the kernels see the key change
    for (int64_t t = 0; t < m_tiles; ++t) {
      const float* h = &hdr[(size_t)t * 4];
      int key;
      memcpy(&key, h + 3, sizeof key);
      if (key != key_s) {
        key_s = key;
        for (int a = 0; a < 3; ++a) scen.push_back((double)h[a]);
      }
      const int32_t id = (int32_t)(scen.size() / 3) - 1;
      const int64_t start = grp[(size_t)t], count = grp[(size_t)m_tiles + t];
      sound = sound && key >= 0 && count >= 0 && count <= CELL_TILE && start >= 0 && start + count <= M;
      for (int64_t k = 0; sound && k < count; ++k) sound = assign(scell, sperm[(size_t)(start + k)], M, id);
    }
  }
  if (!sound) return fail(c, KMVP_E_DEVICE, "kmvp_cell_layout: the source tile list points outside the cloud");

  // ---- targets: the tile of every target's slot, cells named by their stored centre
  const int64_t n_tiles = f64 ? round_up(c->cell_n_tiles, WAVES_PER_BLOCK) : c->cell_n_tiles;
  std::vector<int> slot((size_t)N);
  std::vector<double> tmeta((size_t)n_tiles * 4);
  HIP_TRY(c, hipMemcpyAsync(slot.data(), c->cell_slot.p, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (f64) {
    HIP_TRY(c, hipMemcpyAsync(tmeta.data(), c->cell_tmeta.p, tmeta.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  } else {
    std::vector<float> m32((size_t)n_tiles * 4);
    HIP_TRY(c, hipMemcpyAsync(m32.data(), c->cell_tmeta.p, m32.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (size_t q = 0; q < m32.size(); ++q) tmeta[q] = (q & 3) == 3 ? 0.0 : (double)m32[q];
  }
  std::vector<int32_t> tcell((size_t)N, -1);
  std::vector<double> tcen;
  std::map<std::array<double, 3>, int32_t> ids;
  std::vector<char> taken((size_t)n_tiles * tile, 0);
  for (int64_t i = 0; i < N; ++i) {
    const int64_t sl = slot[(size_t)i];
    if (sl < 0 || sl >= n_tiles * tile) continue;  // stays -1
    const double* m = &tmeta[(size_t)(sl / tile) * 4];
    const std::array<double, 3> key = {m[0], m[1], m[2]};
    auto it = ids.find(key);
    if (it == ids.end()) {
      it = ids.emplace(key, (int32_t)(tcen.size() / 3)).first;
      tcen.insert(tcen.end(), key.begin(), key.end());
    }
    tcell[(size_t)i] = taken[(size_t)sl] ? -2 : it->second;
    taken[(size_t)sl] = 1;
  }

  const int64_t ns = (int64_t)scen.size() / 3, nt = (int64_t)tcen.size() / 3;
  info[0] = ns;
  info[1] = nt;
  info[2] = c->cell_balanced ? 1 : 0;
  info[3] = c->cell_tt;
  info[4] = tile;
  info[5] = layout == LAYOUT_CELL ? 0 : (layout == LAYOUT_CELLMM ? 1 : 2);
  info[6] = f64 ? 0 : c->cell_n_main;
  info[7] = f64 ? 0 : c->cell_n_rest;
  if (sigma_b) {
    float sc = 0.f;  // of the last column cellmm_kernel / cellmm16_kernel ran
    if (layout == LAYOUT_CELLMM) {
      HIP_TRY(c, hipMemcpyAsync(&sc, c->cell_scale.p, sizeof sc, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    *sigma_b = (double)sc;
  }
  if ((source_centres && source_cap < ns) || (target_centres && target_cap < nt))
    return fail(c, KMVP_E_INVALID, "kmvp_cell_layout: room for fewer centres than there are cells (info[0], info[1])");
  if (source_cell) memcpy(source_cell, scell.data(), (size_t)M * sizeof(int32_t));
  if (target_cell) memcpy(target_cell, tcell.data(), (size_t)N * sizeof(int32_t));
  if (source_centres) memcpy(source_centres, scen.data(), scen.size() * sizeof(double));
  if (target_centres) memcpy(target_centres, tcen.data(), tcen.size() * sizeof(double));
  return KMVP_OK;
}

// kmvp_cell_lists: the lists of target tiles of the last product on cellmm_kernel / cellmm16_kernel and the list of every
// target's slot.  Read-only.
int cell_lists_read(kmvp_ctx* c, int64_t* info, int32_t* target_list) {
  if (!info) return fail(c, KMVP_E_INVALID, "kmvp_cell_lists: info is NULL");
  if (!c->have_points || c->cell_state != 1 || c->cell_ver != c->points_ver || c->packed_points_ver != c->points_ver ||
      c->packed_layout != LAYOUT_CELLMM)
    return fail(c, KMVP_E_INVALID, "kmvp_cell_lists: no product on cellmm_kernel / cellmm16_kernel has run on the current points");
  memcpy(info, c->cell_list_info, sizeof c->cell_list_info);
  if (!target_list) return KMVP_OK;
  std::vector<int> slot((size_t)c->N);
  HIP_TRY(c, hipMemcpyAsync(slot.data(), c->cell_slot.p, (size_t)c->N * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const int64_t block_slots = (int64_t)c->cell_tt * WAVES_PER_BLOCK * CELL_TILE;
  const int64_t main_end = info[0] * block_slots, tail_end = main_end + info[1] * block_slots;
  for (int64_t i = 0; i < c->N; ++i) target_list[i] = slot[(size_t)i] < main_end ? 0 : (slot[(size_t)i] < tail_end ? 2 : 1);
  return KMVP_OK;
}

int run_product(kmvp_ctx* c, int kernel, bool normalise) {
  if (!c) return KMVP_E_INVALID;
  c->note.clear();
  if (!c->have_points) return fail(c, KMVP_E_INVALID, "kmvp_set_points has not been called");
  if (!c->have_signal) return fail(c, KMVP_E_INVALID, "kmvp_set_signal has not been called");
  HIP_TRY(c, hipSetDevice(c->device));
  const bool matern = kernel == K_MATERN32 || kernel == K_MATERN52;
  if (matern) {
    // Matern 3/2, 5/2: the difference form only (lowd_kernel, lowd_mid_kernel, lowd_big_kernel).  What is not built is
    // refused, never served by another kernel's path
    if (c->dtype == KMVP_BF16)
      return fail(c, KMVP_E_UNSUPPORTED, "Matern kernels: built for float32 and float64 contexts, not for bfloat16");
    if (c->opt_fast >= 1)
      return fail(c, KMVP_E_UNSUPPORTED, "Matern kernels: fast_sqdists = " + std::to_string(c->opt_fast) +
                                             " asks for a matrix-core form that is not built for them (-1 or 0: the difference form)");
  }
  if (c->M < c->m_total && !(c->exchanges() && c->world > 1) && !c->opt_partial)
    // a slice of the sources and nobody to sum the shards with: the result would be this rank's partial
    // sums passed off as the product
    return fail(c, KMVP_E_INVALID,
                "the sources are a shard (M < M_total) but no multi-rank communicator is attached: call kmvp_comm_init, "
                "or set option partial_shard = 1 to get this shard's partial sums on purpose");
  const int sig = c->density ? SIG_DENSITY : (normalise ? SIG_NORM : SIG_PRODUCT);
  if (c->M == 0 && c->N > 0 && c->exchanges() && c->world > 1) {
    // a rank whose source slice is empty still owes the other ranks its (zero) share of the sums, through the same tail
    const int E = c->density ? 1 : c->E;
    const int64_t NE = sig == SIG_NORM ? E + 1 : E;
    int rc = ensure(c, c->sums, (size_t)NE * c->N * sizeof(double));
    if (rc) return rc;
    HIP_TRY(c, mark(c, 0));
    HIP_TRY(c, hipMemsetAsync(c->sums.p, 0, (size_t)NE * c->N * sizeof(double), c->stream));
    HIP_TRY(c, mark(c, 1));
    c->last_kernel_name = "none";
    if (c->density && normalise) {  // every rank takes the all-ones shortcut below: no exchange
    } else if (takes_shifted_tail(c, kernel)) {  // ... and its (absent) exponents: +inf loses every all-reduce(min)
      if ((rc = ensure(c, c->kshift, (size_t)c->N * sizeof(double)))) return rc;
      hipLaunchKernelGGL(fill_kernel, dim3(blocks_for(c->N)), dim3(256), 0, c->stream, (double*)c->kshift.p, c->N,
                         (double)INFINITY);
      HIP_TRY(c, hipGetLastError());
      return finish_product_shifted(c, c->N, c->N, E, sig);
    } else {
      return finish_product(c, NE * c->N, c->N, c->N, E, sig);
    }
  }
  if (c->N == 0 || c->M == 0) {
    // empty clouds: a = 0 (N,E); nothing to launch
    const int E = c->density ? 1 : c->E;
    int rc = ensure(c, c->out, (size_t)std::max<int64_t>(c->N, 1) * E * sizeof(double));
    if (rc) return rc;
    if (c->N > 0) {
      hipLaunchKernelGGL(fill_kernel, dim3(blocks_for(c->N * E)), dim3(256), 0, c->stream,
                         (double*)c->out.p, c->N * E,
                         normalise ? std::nan("") : 0.0);  // 0/0 in the reference
      HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    c->out_n = c->N;
    c->out_e = E;
    c->last_kernel_ms = c->last_total_ms = 0.f;
    return KMVP_OK;
  }
  if (c->density && normalise) {
    // bruteforce.py:134-138: the rows of a normalised matrix sum to one
    int rc = ensure(c, c->out, (size_t)c->N * sizeof(double));
    if (rc) return rc;
    hipLaunchKernelGGL(fill_kernel, dim3(blocks_for(c->N)), dim3(256), 0, c->stream,
                       (double*)c->out.p, c->N, 1.0);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->out_n = c->N;
    c->out_e = 1;
    c->last_kernel_ms = c->last_total_ms = 0.f;
    c->last_kernel_name = "fill_kernel";
    return KMVP_OK;
  }
  if (kernel == K_EXPDOT) {
    // k = exp(<x,y>) (include/kmvp.h kmvp_expdot): float32 on fastmm_kernel's matrix-core path only
    if (c->density) return fail(c, KMVP_E_UNSUPPORTED, "exp(<x,y>): pass a signal of ones for density estimation");
    if (c->dtype == KMVP_BF16) return run_product_mfma(c, K_EXPDOT, sig);  // D <= 141, E <= 128
    if (c->dtype != KMVP_F32 || c->D > FMM_MAX_D)
      return fail(c, KMVP_E_UNSUPPORTED,
                  "exp(<x,y>) is built for float32 at D <= 64 and for bfloat16 (other cases: the plugin's Gaussian identity)");
    return run_product_fastmm(c, K_GAUSSIAN, sig, true);
  }
  if (c->dtype == KMVP_BF16) return run_product_mfma(c, kernel, sig);
  if (matern) {  // always the difference form, with an empty dispatch note: no faster form exists that could have applied
    if (c->D <= LOWD_MAX_D && !c->density && c->E > LOWD_MAX_E)
      return c->dtype == KMVP_F64 ? run_product_blocked<double>(c, kernel, sig) : run_product_blocked<float>(c, kernel, sig);
    return c->dtype == KMVP_F64 ? run_product_t<double>(c, kernel, sig) : run_product_t<float>(c, kernel, sig);
  }
  const bool f32 = c->dtype == KMVP_F32 && c->centre_ver == c->points_ver;  // float32, clouds measured (measure_clouds)
  bool cells = false;  // the float32 Gaussian's cell form serves this product (cells_usable)
  if (f32 && kernel == K_GAUSSIAN && c->D <= CELL_MAX_D) {
    const int rc = cells_usable(c, !c->density && c->E > 1, cells);
    if (rc) return rc;
  }
  if (f32 && kernel == K_GAUSSIAN && !c->density && (c->E > 1 || c->D > FAST_MAX_D) &&
      (c->opt_fast < 0 || c->opt_fast == 1 || c->opt_fast == 3)) {
    // Several signal columns (low-D attention with E value channels) -- and single columns beyond fast_kernel's D = 39,
    // which fastmm_kernel serves up to D = 64.  Two forms on the matrix cores:
    //   fastmm_kernel  the tile of kernel values goes back to the matrix pipe for the product with the signal: up to 32
    //                  columns per pass at a cost per pair that does not depend on the column count (D <= 64);
    //   cellmm_kernel  one launch per column where the cell form applies (D <= 3) -- a seventh of fastmm's cost per
    //                  pair and column where the cells are well filled.
    // auto takes the cheaper one by the tile counts (picoseconds per 32 x 32 tile on the whole chip, measured at
    // 1e5 .. 1e6 points: tools/fmm_probe.py); fast_sqdists 1 / 3 force one of them.
    const int cols = c->E + (normalise ? 1 : 0);
    const bool fmm_ok = c->D <= FMM_MAX_D && (c->opt_fast == 1 || (c->opt_fast < 0 && radius_ok(c, kernel)));
    const double t_cell = cells ? (double)cols * (double)c->cell_m_tiles *
                                      (cell_ps_per_tile(c->cell_tt) * (double)c->cell_n_main + cell_ps_per_tile(2) * (double)c->cell_n_rest)
                                : INFINITY;
    // (the inputs of the choice go into the dispatch note: the constants were measured on one power-limited box)
    char cost[224];
    double t_fmm = INFINITY;
    if (fmm_ok) {
      const double tiles = std::ceil((double)c->N / FAST_TILE) * std::ceil((double)c->M / FAST_TILE);
      t_fmm = tiles * ((cols + FMM_MAX_COLS - 1) / FMM_MAX_COLS) * (cols > 16 ? FMM_PS_PER_TILE_32 : FMM_PS_PER_TILE_16);
    }
    snprintf(cost, sizeof cost, " [cost model, %d columns: fastmm_kernel %.3g ms, cellmm_kernel %.3g ms (%lld + %lld target x %lld source tiles)]",
             cols, t_fmm * 1e-9, t_cell * 1e-9, (long long)c->cell_n_main, (long long)c->cell_n_rest, (long long)c->cell_m_tiles);
    if (fmm_ok && (c->opt_fast == 1 || t_fmm <= t_cell)) {
      c->note.clear();
      const int rc = run_product_fastmm(c, K_GAUSSIAN, sig);
      if (c->opt_fast < 0) c->note += cost;
      return rc;
    }
    if (cells) {
      c->note.clear();
      const int rc = run_product_cellmm(c, sig);
      if (c->opt_fast < 0) c->note += cost;
      return rc;
    }
  }
  if (f32 && kernel == K_ABSEXP && !c->density && c->D > CFAST_MAX_D && c->D <= FMM_MAX_D && (c->opt_fast < 0 || c->opt_fast == 1)) {
    // exp(-r) beyond the centred forms' D = 4: fastmm_kernel's expansion around one centre with the closest pairs
    // recomputed exactly (any number of signal columns, one included), on clouds inside the radius rule
    // (auto: beyond the specialised difference form's D = 8, or where that form would go column by column -- at
    // D = 5 with up to four columns the two are equally fast)
    const bool pays = c->D > LOWD_MAX_D || c->E + (normalise ? 1 : 0) > LOWD_MAX_E;
    if (radius_ok(c, kernel) && (c->opt_fast == 1 || pays)) {
      c->note.clear();
      return run_product_fastmm(c, K_ABSEXP, sig);
    }
  }
  // (1/r: cfast_kernel's zero rule drops the pair with the target's own index among the COINCIDENT pairs, so the targets
  // must be the sources -- all of them, also when the sources are sharded)
  const bool invdist_square = kernel == K_INVDIST && (c->same_points || c->opt_same_global) && c->N == c->m_total;
  if (f32 && (kernel == K_GAUSSIAN || kernel == K_ABSEXP || invdist_square) && !c->density && c->E > 1 && c->D <= CFAST_MAX_D &&
      (c->opt_fast == 2 || (c->opt_fast < 0 && c->E + (normalise ? 1 : 0) >= CFMM_AUTO_MIN_COLS))) {
    // several signal columns where fastmm_kernel does not apply: exp(-r) and 1/r, which need relative accuracy in s, and
    // the Gaussian on clouds outside the radius rule -- cfast_kernel's distances, the same second product
    c->note.clear();
    return run_product_cfastmm(c, kernel, sig);
  }
  if (f32 && c->D <= FAST_MAX_D && (c->density || c->E == 1)) {
    // "fast_sqdists": squared distances in the expanded form on the matrix cores.
    //   fast_kernel  one centre for the whole cloud: absolute error eps32 (|x'|^2 + |y'|^2) in s
    //                -> as accurate as the difference form only for the Gaussian (smooth in s)
    //                on clouds of small scaled radius;
    //   cfast_kernel centre per source group + exact recomputation of the closest pairs:
    //                relative accuracy in s -> every kernel, any radius (D <= 4).  The
    //                inverse-distance zero rule is applied there to coincident pairs only, so
    //                it needs targets == sources.
    // auto (-1) picks the cheapest form that is as accurate as the difference form.
    const bool global_ok = kernel == K_GAUSSIAN && radius_ok(c, kernel);
    const bool centred_ok = c->D <= CFAST_MAX_D && (kernel != K_INVDIST || invdist_square);
    // cell_kernel: exp() range-reduced by grid cells, the polynomial remainder on the matrix cores
    // (Gaussian, D <= 3).  auto: when the clouds fill the cells well enough that padding stays small.
    // (also inside a solver iteration: grid, cell order and tile lists belong to the points and were built by
    // kmvp_fit or by the first product -- long before a burst of iterations is captured into a hipGraph -- and the
    // launches of the cell paths themselves are asynchronous)
    if (cells) {
      // cellmm_kernel (weights in the operand, sum in the accumulator) where its f16 operands have the range:
      // clouds inside the radius rule; cell_kernel otherwise (wide clouds) or on request (fast_sqdists = 4)
      c->note = c->cell_balanced ? "count-cut cells: the lattice's columns cut along z by point count (cell_balance)" : "";
      if (c->opt_fast != 4 && cellmm_in_range(c))
        return run_product_cellmm(c, sig);  // normalised rows: a second launch with b = 1 for the denominator
      if (c->opt_fast != 4)
        c->note = std::string(c->note.empty() ? "" : c->note + "; ") +
                  "cell_kernel instead of cellmm_kernel: the clouds are outside the radius rule (f16 operand range)";
      return run_product_cell(c, sig);
    }
    if (c->opt_fast == 1 || (c->opt_fast < 0 && global_ok)) return run_product_fast(c, kernel, sig);
    if (centred_ok && (c->opt_fast == 2 || c->opt_fast < 0)) return run_product_cfast(c, kernel, sig);
  }
  if (c->dtype == KMVP_F64 && kernel == K_GAUSSIAN && c->D <= CELL_MAX_D && (c->density || c->E == 1) &&
      c->centre_ver == c->points_ver && cells64_considered(c)) {
    // float64 cell form (kmvp_cell64.hpp): 12 fp64 instructions per pair instead of ~23
    int rc = cell64_prepare(c);
    if (rc) return rc;
    if (c->cell_state == 1 &&
        (c->opt_fast == 3 || (double)c->cell_n_tiles * CELL64_TILE <= CELL_AUTO_MAX_PAD * (double)c->N))
      return run_product_cell64(c, sig);
  }
  if (c->D <= LOWD_MAX_D && !c->density && c->E > LOWD_MAX_E) {  // low D, many signal columns
    if (c->note.empty()) c->note = "E > 4 signal columns: the difference form runs once per block of four columns";
    return c->dtype == KMVP_F64 ? run_product_blocked<double>(c, kernel, sig) : run_product_blocked<float>(c, kernel, sig);
  }
  if (c->dtype == KMVP_F64) return run_product_t<double>(c, kernel, sig);
  return run_product_t<float>(c, kernel, sig);
}


// kmvp_<kernel>_grad: G[i, e, :] = sum_j w(s_ij) (x_i - y_j) b[j, e], left as (N, E D) in c->out.  Linear in the sources,
// so shards, the exchange and the empty cases go through the product's tail with E D plain columns.
// kmvp_<kernel>_dscale: H[i, e, d] = sum_j -w(s_ij) (x_{i,d} - y_{j,d})^2 b[j, e], the same shape, the same tail, the same
// refusals and empty cases: one driver, `what` names the entry point in its messages.
static int run_target_columns(kmvp_ctx* c, int kernel, const std::string& what, bool dscale) {
  if (!c) return KMVP_E_INVALID;
  c->note.clear();
  if (!c->have_points) return fail(c, KMVP_E_INVALID, "kmvp_set_points has not been called");
  if (!c->have_signal) return fail(c, KMVP_E_INVALID, "kmvp_set_signal has not been called");
  HIP_TRY(c, hipSetDevice(c->device));
  if (c->M < c->m_total && !(c->exchanges() && c->world > 1) && !c->opt_partial)
    return fail(c, KMVP_E_INVALID,
                "the sources are a shard (M < M_total) but no multi-rank communicator is attached: call kmvp_comm_init, "
                "or set option partial_shard = 1 to get this shard's partial sums on purpose");
  if (c->dtype == KMVP_BF16)
    return fail(c, KMVP_E_UNSUPPORTED, what + ": built for float32 and float64 contexts, not for bfloat16");
  const int E = c->density ? 1 : c->E;
  if (c->D > LOWD_MAX_D)
    return fail(c, KMVP_E_UNSUPPORTED, what + ": D = " + std::to_string(c->D) + " is beyond the kernels' D <= " +
                                           std::to_string(LOWD_MAX_D));
  if (E > LOWD_MAX_E)
    return fail(c, KMVP_E_UNSUPPORTED, what + ": E = " + std::to_string(E) + " signal columns are beyond the kernels' E <= " +
                                           std::to_string(LOWD_MAX_E) + " (run it per block of columns)");
  const int64_t NC = (int64_t)E * c->D;
  if (c->N == 0 || c->M == 0) {
    int rc;
    if (c->N > 0 && c->exchanges() && c->world > 1) {
      // a rank whose source slice is empty still owes the other ranks its (zero) share of the sums
      if ((rc = ensure(c, c->sums, (size_t)NC * c->N * sizeof(double)))) return rc;
      HIP_TRY(c, mark(c, 0));
      HIP_TRY(c, hipMemsetAsync(c->sums.p, 0, (size_t)NC * c->N * sizeof(double), c->stream));
      HIP_TRY(c, mark(c, 1));
      c->last_kernel_name = "none";
      return finish_product(c, NC * c->N, c->N, c->N, (int)NC, SIG_PRODUCT);
    }
    if ((rc = ensure(c, c->out, (size_t)std::max<int64_t>(c->N, 1) * NC * sizeof(double)))) return rc;
    if (c->N > 0) {
      HIP_TRY(c, hipMemsetAsync(c->out.p, 0, (size_t)c->N * NC * sizeof(double), c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    c->out_n = c->N;
    c->out_e = (int)NC;
    c->last_kernel_ms = c->last_total_ms = 0.f;
    c->last_kernel_name = "none";
    return KMVP_OK;
  }
  const int sig = c->density ? SIG_DENSITY : SIG_PRODUCT;
  return c->dtype == KMVP_F64 ? run_gradient_t<double>(c, kernel, sig, dscale) : run_gradient_t<float>(c, kernel, sig, dscale);
}
int run_gradient(kmvp_ctx* c, int kernel) { return run_target_columns(c, kernel, "gradient", false); }
int run_dscale(kmvp_ctx* c, int kernel) { return run_target_columns(c, kernel, "length-scale derivative", true); }

// kmvp_<kernel>_logsumexp: L[i, e] = log sum_j exp(l(x_i, y_j) + c[j, e]) with the signal read as log-weights, left as
// (N, E) in c->out.  Not linear in the sources: shards merge as (sum, exponent) pairs (finish_lse), an empty slice owes
// the other ranks the same two collectives with no live term.
int run_logsumexp(kmvp_ctx* c, int kernel) {
  if (!c) return KMVP_E_INVALID;
  c->note.clear();
  if (!c->have_points) return fail(c, KMVP_E_INVALID, "kmvp_set_points has not been called");
  if (!c->have_signal) return fail(c, KMVP_E_INVALID, "kmvp_set_signal has not been called");
  HIP_TRY(c, hipSetDevice(c->device));
  if (c->M < c->m_total && !(c->exchanges() && c->world > 1) && !c->opt_partial)
    return fail(c, KMVP_E_INVALID,
                "the sources are a shard (M < M_total) but no multi-rank communicator is attached: call kmvp_comm_init, "
                "or set option partial_shard = 1 to get this shard's own log-sum-exp on purpose");
  if (c->dtype == KMVP_BF16)
    return fail(c, KMVP_E_UNSUPPORTED, "log-sum-exp: built for float32 and float64 contexts, not for bfloat16");
  const int E = c->density ? 1 : c->E;
  if (c->D > LOWD_MAX_D)
    return fail(c, KMVP_E_UNSUPPORTED, "log-sum-exp: D = " + std::to_string(c->D) + " is beyond the kernels' D <= " +
                                           std::to_string(LOWD_MAX_D));
  if (E > LOWD_MAX_E)
    return fail(c, KMVP_E_UNSUPPORTED, "log-sum-exp: E = " + std::to_string(E) + " columns are beyond the kernels' E <= " +
                                           std::to_string(LOWD_MAX_E) + " (columns are independent: run it per block of columns)");
  if (c->opt_fast >= 1)
    return fail(c, KMVP_E_UNSUPPORTED, "log-sum-exp: fast_sqdists = " + std::to_string(c->opt_fast) +
                                           " asks for a matrix-core form that is not built for it (-1 or 0: the difference form)");
  if (c->N == 0 || c->M == 0) {
    int rc;
    const int64_t cnt = (int64_t)E * c->N;
    c->last_kernel_name = "none";
    if (c->N > 0 && c->exchanges() && c->world > 1) {
      if ((rc = ensure(c, c->sums, (size_t)cnt * sizeof(double)))) return rc;
      if ((rc = ensure(c, c->kshift, (size_t)cnt * sizeof(double)))) return rc;
      HIP_TRY(c, mark(c, 0));
      HIP_TRY(c, hipMemsetAsync(c->sums.p, 0, (size_t)cnt * sizeof(double), c->stream));
      hipLaunchKernelGGL(fill_kernel, dim3(blocks_for(cnt)), dim3(256), 0, c->stream, (double*)c->kshift.p, cnt, (double)INFINITY);
      HIP_TRY(c, hipGetLastError());
      HIP_TRY(c, mark(c, 1));
      return finish_lse(c, c->N, c->N, E);
    }
    if ((rc = ensure(c, c->out, (size_t)std::max<int64_t>(cnt, 1) * sizeof(double)))) return rc;
    if (c->N > 0) {  // no source: every row is log 0
      hipLaunchKernelGGL(fill_kernel, dim3(blocks_for(cnt)), dim3(256), 0, c->stream, (double*)c->out.p, cnt, -(double)INFINITY);
      HIP_TRY(c, hipGetLastError());
      HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    c->out_n = c->N;
    c->out_e = E;
    c->last_kernel_ms = c->last_total_ms = 0.f;
    return KMVP_OK;
  }
  const int sig = c->density ? SIG_DENSITY : SIG_PRODUCT;
  return c->dtype == KMVP_F64 ? run_logsumexp_t<double>(c, kernel, sig) : run_logsumexp_t<float>(c, kernel, sig);
}

// kmvp_<kernel>_logsumexp_grad: G[i, e, :] = grad_{x_i} L[i, e], a softmax-weighted sum of g(x_i, y_j), left as (N, E D) in
// c->out.  Shards merge as (D + 1 sums, exponent) tuples (finish_lse_grad); an empty slice owes the other ranks the same two
// collectives with no live term.  Without any live term the softmax does not exist: NaN.
int run_logsumexp_grad(kmvp_ctx* c, int kernel) {
  if (!c) return KMVP_E_INVALID;
  c->note.clear();
  if (!c->have_points) return fail(c, KMVP_E_INVALID, "kmvp_set_points has not been called");
  if (!c->have_signal) return fail(c, KMVP_E_INVALID, "kmvp_set_signal has not been called");
  HIP_TRY(c, hipSetDevice(c->device));
  if (c->M < c->m_total && !(c->exchanges() && c->world > 1) && !c->opt_partial)
    return fail(c, KMVP_E_INVALID,
                "the sources are a shard (M < M_total) but no multi-rank communicator is attached: call kmvp_comm_init, "
                "or set option partial_shard = 1 to get this shard's own gradient of the log-sum-exp on purpose");
  if (c->dtype == KMVP_BF16)
    return fail(c, KMVP_E_UNSUPPORTED, "log-sum-exp gradient: built for float32 and float64 contexts, not for bfloat16");
  const int E = c->density ? 1 : c->E;
  const int D = c->D;
  if (D > LOWD_MAX_D)
    return fail(c, KMVP_E_UNSUPPORTED, "log-sum-exp gradient: D = " + std::to_string(D) + " is beyond the kernels' D <= " +
                                           std::to_string(LOWD_MAX_D));
  if (E > LOWD_MAX_E)
    return fail(c, KMVP_E_UNSUPPORTED, "log-sum-exp gradient: E = " + std::to_string(E) + " columns are beyond the kernels' E <= " +
                                           std::to_string(LOWD_MAX_E) + " (columns are independent: run it per block of columns)");
  if (c->opt_fast >= 1)
    return fail(c, KMVP_E_UNSUPPORTED, "log-sum-exp gradient: fast_sqdists = " + std::to_string(c->opt_fast) +
                                           " asks for a matrix-core form that is not built for it (-1 or 0: the difference form)");
  if (c->N == 0 || c->M == 0) {
    int rc;
    const int64_t cnt = (int64_t)E * c->N;
    c->last_kernel_name = "none";
    if (c->N > 0 && c->exchanges() && c->world > 1) {
      if ((rc = ensure(c, c->sums, (size_t)(D + 1) * cnt * sizeof(double)))) return rc;
      if ((rc = ensure(c, c->kshift, (size_t)cnt * sizeof(double)))) return rc;
      HIP_TRY(c, mark(c, 0));
      HIP_TRY(c, hipMemsetAsync(c->sums.p, 0, (size_t)(D + 1) * cnt * sizeof(double), c->stream));
      hipLaunchKernelGGL(fill_kernel, dim3(blocks_for(cnt)), dim3(256), 0, c->stream, (double*)c->kshift.p, cnt, (double)INFINITY);
      HIP_TRY(c, hipGetLastError());
      HIP_TRY(c, mark(c, 1));
      return finish_lse_grad(c, kernel, c->N, c->N, E, D);
    }
    if ((rc = ensure(c, c->out, (size_t)std::max<int64_t>(cnt * D, 1) * sizeof(double)))) return rc;
    if (c->N > 0) {  // no source: no softmax
      hipLaunchKernelGGL(fill_kernel, dim3(blocks_for(cnt * D)), dim3(256), 0, c->stream, (double*)c->out.p, cnt * D,
                         (double)NAN);
      HIP_TRY(c, hipGetLastError());
      HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    c->out_n = c->N;
    c->out_e = E * D;
    c->last_kernel_ms = c->last_total_ms = 0.f;
    return KMVP_OK;
  }
  const int sig = c->density ? SIG_DENSITY : SIG_PRODUCT;
  return c->dtype == KMVP_F64 ? run_logsumexp_grad_t<double>(c, kernel, sig) : run_logsumexp_grad_t<float>(c, kernel, sig);
}

// ---- K nearest neighbours (kmvp_lowd_knn.hpp, kmvp_knn_merge.hpp) ------------------------------------------------------
// lowd_knn_kernel leaves KT sorted candidates per (segment, target): part[s][2 KT][n_pad].  knn_merge_kernel folds S lists
// of one target into Kc = K (+ 1 with exclude_self) candidates in the canonical unpadded layout [2 Kc][N] -- the segments
// first, then, sharded, the ranks' lists after ONE all-reduce; knn_finish_kernel drops the own index and writes (N, K).
// (knn_merge_kernel: kmvp_internal.hpp, shared with the k-means iteration.)
static __global__ void knn_fill_kernel(double* __restrict__ cand, int64_t n, int Kc) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= 2 * (int64_t)Kc * n) return;
  cand[q] = q < (int64_t)Kc * n ? (double)INFINITY : -1.0;
}

// (knn_finish_kernel: kmvp_internal.hpp, shared with the batched clouds.)

template <typename real>
static int run_nearest_t(kmvp_ctx* c, int Kc) {
  const int D = c->D;
  const int64_t N = c->N, M = c->M;
  const real* x_raw = (const real*)(c->same_points ? c->y_raw.p : c->x_raw.p);
  int rc;
  const int KT = knn_capacity(Kc);
  const int R = (D + 3) / 4 * 4;  // density layout: no signal columns
  const int64_t tile = 64 * (int64_t)WAVES_PER_BLOCK;
  const int64_t n_pad0 = round_up(std::max<int64_t>(N, 1), tile), m_pad0 = round_up(std::max<int64_t>(M, 1), LOWD_BATCH);
  LowdArgs<real> a = kmvp::lowd_geometry<real>(N, M, knn_segments(c->opt_segments, KT, n_pad0 / tile, m_pad0, n_pad0),
                                              c->opt_chunk, c->j_offset, c->m_total, 1, R, 2 * KT);
  if (a.seg_len > 0x7fffffff) return fail(c, KMVP_E_UNSUPPORTED, "nearest: a source segment of 2^31 records or more (raise \"segments\")");

  // the product's layouts in the density form through the context's own bookkeeping (no kernel constant enters them):
  // a product with a signal before or after repacks its records, as it does after a density product
  const PackKey key = {LAYOUT_LOWD, K_GAUSSIAN, 1};
  if (points_stale(c, key)) {
    if ((rc = ensure(c, c->xs, (size_t)D * a.n_pad * sizeof(real)))) return rc;
    hipLaunchKernelGGL((pack_targets_kernel<real>), dim3(blocks_for(a.n_pad)), dim3(256), 0, c->stream, x_raw,
                       (real*)c->xs.p, N, a.n_pad, D, (real)1);
  }
  if (points_stale(c, key) || c->packed_sig != SIG_DENSITY) {
    if ((rc = ensure(c, c->rec, (size_t)(a.m_pad + LOWD_BATCH) * R * sizeof(real)))) return rc;
    hipLaunchKernelGGL((pack_sources_kernel<real>), dim3(blocks_for(a.m_pad + LOWD_BATCH)), dim3(256), 0, c->stream,
                       (const real*)c->y_raw.p, (const real*)nullptr, (real*)c->rec.p, M, a.m_pad + LOWD_BATCH, D, 0, R, (real)1);
  }
  HIP_TRY(c, hipGetLastError());
  record_packed(c, key, SIG_DENSITY);

  if ((rc = ensure(c, c->part, (size_t)a.segments * 2 * KT * a.n_pad * sizeof(double)))) return rc;
  a.xs = (const real*)c->xs.p;
  a.rec = (const real*)c->rec.p;
  a.part = (double*)c->part.p;
  const int64_t nblocks = (int64_t)a.tile_blocks * a.segments;
  if (nblocks > 0x7fffffff) return fail(c, KMVP_E_UNSUPPORTED, "launch grid too large");
  HIP_TRY(c, mark(c, 0));
  HIP_TRY(c, launch_lowd_knn(D, KT, a, dim3((unsigned)nblocks), c->stream, &c->last_kernel_name));
  HIP_TRY(c, mark(c, 1));
  hipLaunchKernelGGL(knn_merge_kernel, dim3(blocks_for(N)), dim3(256), 0, c->stream, (const double*)c->part.p, (double*)c->sums.p,
                     N, (int64_t)2 * KT * a.n_pad, a.n_pad, a.segments, KT, Kc);
  HIP_TRY(c, hipGetLastError());
  return KMVP_OK;
}

// kmvp_nearest: the K smallest squared distances of every target and their global source indices, into the caller's
// arrays.  Not a sum over the sources: shards merge as candidate lists (one all-reduce that adds zeros to every slot but
// the rank's own); an empty slice owes the other ranks the same collective with an all-pad slot.
int run_nearest(kmvp_ctx* c, int K, int exclude_self, int64_t* out_idx, double* out_sqdist) {
  if (!c) return KMVP_E_INVALID;
  c->note.clear();
  if (!c->have_points) return fail(c, KMVP_E_INVALID, "kmvp_set_points has not been called");
  if (K < 1) return fail(c, KMVP_E_INVALID, "nearest: K must be >= 1");
  if (exclude_self && !c->same_points && !c->opt_same_global)
    return fail(c, KMVP_E_INVALID, "nearest: exclude_self needs the targets to be the sources (same_points, or option "
                                   "same_points_global = 1 when the sources are a shard and x is the full cloud)");
  if (c->N > 0 && (!out_idx || !out_sqdist)) return fail(c, KMVP_E_INVALID, "nearest: a NULL output");
  HIP_TRY(c, hipSetDevice(c->device));
  if (c->M < c->m_total && !(c->exchanges() && c->world > 1) && !c->opt_partial)
    return fail(c, KMVP_E_INVALID,
                "the sources are a shard (M < M_total) but no multi-rank communicator is attached: call kmvp_comm_init, "
                "or set option partial_shard = 1 to get this shard's own neighbours on purpose");
  if (c->dtype == KMVP_BF16)
    return fail(c, KMVP_E_UNSUPPORTED, "nearest: built for float32 and float64 contexts, not for bfloat16");
  if (c->D > LOWD_MAX_D)
    return fail(c, KMVP_E_UNSUPPORTED, "nearest: D = " + std::to_string(c->D) + " is beyond the kernels' D <= " +
                                           std::to_string(LOWD_MAX_D));
  const int Kc = K + (exclude_self ? 1 : 0);  // candidates collected per target
  if (K > KNN_MAX_K || Kc > KNN_MAX_K)
    return fail(c, KMVP_E_UNSUPPORTED, "nearest: K = " + std::to_string(K) + (exclude_self ? " with exclude_self" : "") +
                                           " is beyond the lists' K <= 16 (15 with exclude_self)");
  if (c->opt_fast >= 1)
    return fail(c, KMVP_E_UNSUPPORTED, "nearest: fast_sqdists = " + std::to_string(c->opt_fast) +
                                           " asks for a matrix-core form that is not built for it (-1 or 0: the difference form)");
  const int64_t N = c->N;
  c->last_kernel_ms = c->last_total_ms = c->last_allreduce_ms = 0.f;
  c->last_kernel_name = "none";
  if (N == 0) return KMVP_OK;

  int rc;
  const int64_t cnt = (int64_t)2 * Kc * N;  // one rank's candidates, [2 Kc][N]
  if ((rc = ensure(c, c->sums, (size_t)cnt * sizeof(double)))) return rc;
  HIP_TRY(c, mark(c, 0));
  if (c->M == 0) {  // no source here: every list is empty
    HIP_TRY(c, mark(c, 0));
    hipLaunchKernelGGL(knn_fill_kernel, dim3(blocks_for(cnt)), dim3(256), 0, c->stream, (double*)c->sums.p, N, Kc);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, mark(c, 1));
  } else if ((rc = c->dtype == KMVP_F64 ? run_nearest_t<double>(c, Kc) : run_nearest_t<float>(c, Kc))) {
    return rc;
  }
  double* cand = (double*)c->sums.p;
  if (c->exchanges()) {  // also with world == 1, as the product's tail
    const int world = c->world;
    if ((rc = ensure(c, c->xchg, (size_t)(world + 1) * cnt * sizeof(double)))) return rc;
    double* slots = (double*)c->xchg.p;  // [world][2 Kc][N], then the merged [2 Kc][N]
    HIP_TRY(c, hipMemsetAsync(slots, 0, (size_t)world * cnt * sizeof(double), c->stream));
    HIP_TRY(c, hipMemcpyAsync(slots + (int64_t)c->rank * cnt, cand, (size_t)cnt * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, mark(c, 3));
    if ((rc = exchange_f64(c, slots, (int64_t)world * cnt, KMVP_OP_SUM))) return rc;  // adding zeros is exact, also for inf, NaN, -1
    HIP_TRY(c, mark(c, 4));
    cand = slots + (int64_t)world * cnt;
    hipLaunchKernelGGL(knn_merge_kernel, dim3(blocks_for(N)), dim3(256), 0, c->stream, (const double*)slots, cand, N, cnt, N,
                       world, Kc, Kc);
    HIP_TRY(c, hipGetLastError());
  }
  const size_t nk = (size_t)N * K;
  if ((rc = ensure(c, c->knn, nk * (sizeof(int64_t) + sizeof(double))))) return rc;
  int64_t* d_idx = (int64_t*)c->knn.p;
  double* d_sq = (double*)(d_idx + nk);
  hipLaunchKernelGGL(knn_finish_kernel, dim3(blocks_for(N)), dim3(256), 0, c->stream, cand, d_idx, d_sq, N, K, exclude_self ? 1 : 0);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipEventRecord(c->ev[2], c->stream));
  HIP_TRY(c, hipMemcpyAsync(out_idx, d_idx, nk * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(out_sqdist, d_sq, nk * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipEventElapsedTime(&c->last_kernel_ms, c->ev[0], c->ev[1]));
  HIP_TRY(c, hipEventElapsedTime(&c->last_total_ms, c->ev[0], c->ev[2]));
  if (c->exchanges()) HIP_TRY(c, hipEventElapsedTime(&c->last_allreduce_ms, c->ev[3], c->ev[4]));
  return KMVP_OK;
}

}  // namespace kmvp
