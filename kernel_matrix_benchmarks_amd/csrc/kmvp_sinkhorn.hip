// Sinkhorn iteration of entropic optimal transport on the log-sum-exp (include/kmvp.h kmvp_<kernel>_sinkhorn): what
// kmvp_solvers.hip is to the product.  The pair loop is lowd_lse_kernel, untouched; this file is the iteration around it.
//
// Two packed layouts live side by side in buffers of the solver's own (the product's xs / rec and their PackKey
// bookkeeping are never touched): direction 1 = target image of x with records of y (T1: the new u from v), direction 2 =
// target image of y with records of x (T2: the new v from u).  Both are packed once per kmvp_set_points; an iteration only
// rewrites the ONE signal slot of each record, rec[j R + D] = (real)(potential_j + log weight_j) -- the potentials and the
// log-weights themselves stay fp64 on the device.
//
// One iteration k, eight launches, no atomics:
//   lowd_lse_kernel (direction 2), lse_reduce_kernel, sk_finish_kernel:   v_k = T2(u_{k-1}) and the slots of y's records
//   lowd_lse_kernel (direction 1), lse_reduce_kernel, sk_finish_kernel:   ut = T1(v_k), per-block partial sums of
//                                                                         a_i |exp(u_i - ut_i) - 1| (fixed tree order)
//   sk_scalars_kernel (one block):  err_k = the partials in index order; iterations += 1; the stop word:
//                                   2 a non-finite potential or error, 1 err_k <= tol, 3 maxit reached, else 0
//   sk_commit_kernel:               only while the stop word is 0: u_k = ut and the slots of x's records
// so (u, v) on the device is always the plan err describes, whatever ends the solve.  The host reads the three state words
// after every iteration (the decision has been taken on the device by then: it only learns whether to launch another).
#include "kmvp_ctx.hpp"

namespace kmvp {
namespace {

constexpr int SK_THREADS = 256;
enum : int { SK_RUNNING = 0, SK_CONVERGED = 1, SK_NONFINITE = 2, SK_MAXIT = 3 };
// the state words behind the vectors: stop, iterations, err
constexpr size_t SK_STATE_WORDS = 3;

// Sum over the block in a fixed tree order; every thread gets it.
__device__ __forceinline__ double sk_block_sum(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int s = SK_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

// rec[j R + D] = (real)(pot_j + logw_j) for the m real records; pad records stay as packed (y = +inf, slot 0)
template <typename real>
__global__ void sk_slot_kernel(const double* __restrict__ pot, const double* __restrict__ logw, real* __restrict__ rec,
                               int64_t m, int R, int D) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j < m) rec[j * R + D] = (real)(pot[j] + logw[j]);
}

// After lse_reduce_kernel, for the n targets of one direction: pot_i = -(log2(sums_i) - K_i) ln 2, finish_lse_kernel's
// arithmetic with the sign flipped (K = +inf, no live term: +inf).  bad[block] counts its non-finite potentials.
//   rec != nullptr (T2): the potential goes straight into the slot of the records the OTHER direction reads.
//   prev != nullptr (T1): perr[block] = sum over the block of a_i |exp(prev_i - pot_i) - 1|, a_i = exp(logw_i); a point of
//   mass 0 (logw = -inf) contributes exactly 0 whatever its potentials are.
template <typename real>
__global__ void __launch_bounds__(SK_THREADS) sk_finish_kernel(const double* __restrict__ sums, const double* __restrict__ kshift,
                                                               int64_t n, double* __restrict__ pot, const double* __restrict__ logw,
                                                               const double* __restrict__ prev, real* __restrict__ rec, int R, int D,
                                                               double* __restrict__ perr, double* __restrict__ bad) {
  __shared__ double sh[SK_THREADS];
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double term = 0.0, flag = 0.0;
  if (i < n) {
    const double k = kshift[i];
    const double p = (k < 1.0e300) ? (k - log2(sums[i])) * 0.6931471805599453 : (double)INFINITY;
    pot[i] = p;
    if (!(fabs(p) < (double)INFINITY)) flag = 1.0;
    const double lw = logw[i];
    if (rec) rec[i * R + D] = (real)(p + lw);
    if (prev && lw > -(double)INFINITY) term = exp(lw) * fabs(expm1(prev[i] - p));
  }
  const double f = sk_block_sum(flag, sh);
  if (threadIdx.x == 0) bad[blockIdx.x] = f;
  if (prev) {
    const double e = sk_block_sum(term, sh);
    if (threadIdx.x == 0) perr[blockIdx.x] = e;
  }
}

// One block: err = the nb_u partials (thread t adds t, t + 256, ... in index order, then the tree), the non-finite counts of
// both directions, and the verdict on this iteration.  st = [stop | iterations | err]
__global__ void __launch_bounds__(SK_THREADS) sk_scalars_kernel(const double* __restrict__ perr, const double* __restrict__ bad_u,
                                                                int nb_u, const double* __restrict__ bad_v, int nb_v,
                                                                double* __restrict__ st, double tol, int maxit) {
  __shared__ double sh[SK_THREADS];
  double e = 0.0, b = 0.0;
  for (int q = threadIdx.x; q < nb_u; q += SK_THREADS) {
    e += perr[q];
    b += bad_u[q];
  }
  for (int q = threadIdx.x; q < nb_v; q += SK_THREADS) b += bad_v[q];
  const double err = sk_block_sum(e, sh);
  const double nbad = sk_block_sum(b, sh);
  if (threadIdx.x == 0) {
    const double it = st[1] + 1.0;
    int stop = SK_RUNNING;
    if (nbad != 0.0 || !(fabs(err) < (double)INFINITY)) stop = SK_NONFINITE;
    else if (err <= tol) stop = SK_CONVERGED;
    else if (it >= (double)maxit) stop = SK_MAXIT;
    st[0] = (double)stop;
    st[1] = it;
    st[2] = err;
  }
}

// u = ut and the slots of x's records, only while the iteration goes on
template <typename real>
__global__ void sk_commit_kernel(const double* __restrict__ st, const double* __restrict__ ut, const double* __restrict__ logw,
                                 double* __restrict__ u, real* __restrict__ rec, int64_t n, int R, int D) {
  if (st[0] != 0.0) return;  // uniform: written by sk_scalars_kernel, the launch before this one
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double p = ut[i];
  u[i] = p;
  rec[i * R + D] = (real)(p + logw[i]);
}

template <typename real>
int sinkhorn_t(kmvp_ctx* c, int kernel, const double* log_a, const double* log_b, double tol, int maxit, double* u_io,
               double* v_out, int* iters, double* err) {
  const int D = c->D;
  const int64_t N = c->N, M = c->M;
  const int R = (D + 1 + 3) / 4 * 4;  // RecLayout<D, 1, SIG_PRODUCT>::R: coordinates, one signal slot, padding
  int rc;
  // direction 1: targets x, sources y (T1); direction 2: targets y, sources x (T2).  Neither is a slice.
  LowdArgs<real> a1 = lowd_geometry<real>(N, M, c->opt_segments, c->opt_chunk, 0, M, 1, R, 2);
  LowdArgs<real> a2 = lowd_geometry<real>(M, N, c->opt_segments, c->opt_chunk, 0, N, 1, R, 2);
  const int64_t grid1 = (int64_t)a1.tile_blocks * a1.segments, grid2 = (int64_t)a2.tile_blocks * a2.segments;
  if (grid1 > 0x7fffffff || grid2 > 0x7fffffff) return fail(c, KMVP_E_UNSUPPORTED, "launch grid too large");

  HIP_TRY(c, hipEventRecord(c->ev[0], c->stream));
  // ---- the layouts, once per kmvp_set_points.  same_points: one cloud, one target image; the records still come twice,
  // their slots carry different potentials.
  DevBuf& xs_y = c->same_points ? c->sk_xs_x : c->sk_xs_y;
  if (c->sk_points_ver != c->points_ver) {
    const real* x_raw = (const real*)(c->same_points ? c->y_raw.p : c->x_raw.p);
    const real* y_raw = (const real*)c->y_raw.p;
    const int64_t rows1 = a1.m_pad + LOWD_BATCH, rows2 = a2.m_pad + LOWD_BATCH;
    if ((rc = ensure(c, c->sk_xs_x, (size_t)D * a1.n_pad * sizeof(real)))) return rc;
    if ((rc = ensure(c, c->sk_rec_y, (size_t)rows1 * R * sizeof(real)))) return rc;
    if ((rc = ensure(c, c->sk_rec_x, (size_t)rows2 * R * sizeof(real)))) return rc;
    hipLaunchKernelGGL((pack_targets_kernel<real>), dim3(blocks_for(a1.n_pad)), dim3(256), 0, c->stream, x_raw,
                       (real*)c->sk_xs_x.p, N, a1.n_pad, D, (real)1);
    hipLaunchKernelGGL((pack_sources_kernel<real>), dim3(blocks_for(rows1)), dim3(256), 0, c->stream, y_raw, (const real*)nullptr,
                       (real*)c->sk_rec_y.p, M, rows1, D, 0, R, (real)1, -1, 0);
    hipLaunchKernelGGL((pack_sources_kernel<real>), dim3(blocks_for(rows2)), dim3(256), 0, c->stream, x_raw, (const real*)nullptr,
                       (real*)c->sk_rec_x.p, N, rows2, D, 0, R, (real)1, -1, 0);
    if (!c->same_points) {
      if ((rc = ensure(c, c->sk_xs_y, (size_t)D * a2.n_pad * sizeof(real)))) return rc;
      hipLaunchKernelGGL((pack_targets_kernel<real>), dim3(blocks_for(a2.n_pad)), dim3(256), 0, c->stream, y_raw,
                         (real*)c->sk_xs_y.p, M, a2.n_pad, D, (real)1);
    }
    HIP_TRY(c, hipGetLastError());
    c->sk_points_ver = c->points_ver;
  }

  // ---- scratch of one half-step (shared with the log-sum-exp: rewritten by every call) and the solver's state
  const int64_t np = std::max(a1.n_pad, a2.n_pad);
  const size_t part_count = (size_t)std::max((int64_t)a1.segments * 2 * a1.n_pad, (int64_t)a2.segments * 2 * a2.n_pad);
  if ((rc = ensure(c, c->part, part_count * sizeof(double)))) return rc;
  if ((rc = ensure(c, c->sums, (size_t)np * sizeof(double)))) return rc;
  if ((rc = ensure(c, c->kshift, (size_t)np * sizeof(double)))) return rc;
  const int nb_u = (int)blocks_for(N, SK_THREADS), nb_v = (int)blocks_for(M, SK_THREADS);
  // [u N | ut N | log_a N | v M | log_b M | perr nb_u | bad_u nb_u | bad_v nb_v | state]
  const size_t words = 3 * (size_t)N + 2 * (size_t)M + 2 * (size_t)nb_u + nb_v + SK_STATE_WORDS;
  if ((rc = ensure(c, c->sk_state, words * sizeof(double)))) return rc;
  double* u = (double*)c->sk_state.p;
  double* ut = u + N;
  double* la = ut + N;
  double* v = la + N;
  double* lb = v + M;
  double* perr = lb + M;
  double* bad_u = perr + nb_u;
  double* bad_v = bad_u + nb_u;
  double* st = bad_v + nb_v;

  // u_0 and the log-weights (NULL: uniform); ut and v are written by the first iteration before anything reads them
  const std::vector<double> uniform_a(log_a ? 0 : (size_t)N, -std::log((double)N));
  const std::vector<double> uniform_b(log_b ? 0 : (size_t)M, -std::log((double)M));
  HIP_TRY(c, hipMemcpyAsync(u, u_io, (size_t)N * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(la, log_a ? log_a : uniform_a.data(), (size_t)N * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(lb, log_b ? log_b : uniform_b.data(), (size_t)M * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemsetAsync(st, 0, SK_STATE_WORDS * sizeof(double), c->stream));
  hipLaunchKernelGGL((sk_slot_kernel<real>), dim3(blocks_for(N)), dim3(256), 0, c->stream, (const double*)u, (const double*)la,
                     (real*)c->sk_rec_x.p, N, R, D);
  HIP_TRY(c, hipGetLastError());

  a1.xs = (const real*)c->sk_xs_x.p;
  a1.rec = (const real*)c->sk_rec_y.p;
  a2.xs = (const real*)xs_y.p;
  a2.rec = (const real*)c->sk_rec_x.p;
  a1.part = a2.part = (double*)c->part.p;
  double* sums = (double*)c->sums.p;
  double* kshift = (double*)c->kshift.p;

  // ---- the iteration
  double state[SK_STATE_WORDS] = {0.0, 0.0, 0.0};
  while (state[0] == 0.0) {
    // v = T2(u): targets y, records of x with u + log_a in the slot; the finish writes v + log_b into y's records
    HIP_TRY(c, launch_lowd_lse(kernel, D, 1, SIG_PRODUCT, a2, dim3((unsigned)grid2), c->stream, &c->last_kernel_name));
    hipLaunchKernelGGL(lse_reduce_kernel, dim3(blocks_for(a2.n_pad)), dim3(256), 0, c->stream, (const double*)a2.part, sums,
                       kshift, a2.n_pad, a2.segments);
    hipLaunchKernelGGL((sk_finish_kernel<real>), dim3(nb_v), dim3(SK_THREADS), 0, c->stream, (const double*)sums,
                       (const double*)kshift, M, v, (const double*)lb, (const double*)nullptr, (real*)c->sk_rec_y.p, R, D,
                       (double*)nullptr, bad_v);
    // ut = T1(v): targets x, records of y; the finish leaves the partial sums of the row marginal's violation
    HIP_TRY(c, launch_lowd_lse(kernel, D, 1, SIG_PRODUCT, a1, dim3((unsigned)grid1), c->stream, &c->last_kernel_name));
    hipLaunchKernelGGL(lse_reduce_kernel, dim3(blocks_for(a1.n_pad)), dim3(256), 0, c->stream, (const double*)a1.part, sums,
                       kshift, a1.n_pad, a1.segments);
    hipLaunchKernelGGL((sk_finish_kernel<real>), dim3(nb_u), dim3(SK_THREADS), 0, c->stream, (const double*)sums,
                       (const double*)kshift, N, ut, (const double*)la, (const double*)u, (real*)nullptr, R, D, perr, bad_u);
    hipLaunchKernelGGL(sk_scalars_kernel, dim3(1), dim3(SK_THREADS), 0, c->stream, (const double*)perr, (const double*)bad_u,
                       nb_u, (const double*)bad_v, nb_v, st, tol, maxit);
    hipLaunchKernelGGL((sk_commit_kernel<real>), dim3(blocks_for(N)), dim3(256), 0, c->stream, (const double*)st,
                       (const double*)ut, (const double*)la, u, (real*)c->sk_rec_x.p, N, R, D);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(state, st, sizeof(state), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }

  HIP_TRY(c, hipMemcpyAsync(u_io, u, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(v_out, v, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipEventRecord(c->ev[2], c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipEventElapsedTime(&c->last_total_ms, c->ev[0], c->ev[2]));
  c->last_kernel_ms = c->last_total_ms;  // both cover the whole solve (include/kmvp.h)
  c->last_allreduce_ms = 0.f;
  *iters = (int)state[1];
  *err = state[2];
  if ((int)state[0] == SK_CONVERGED) return KMVP_OK;
  c->err = (int)state[0] == SK_NONFINITE
               ? "Sinkhorn: a potential or the marginal error is not finite (a row without a live term, a non-finite "
                 "coordinate, weight or starting potential)"
               : "Sinkhorn stopped at maxit before the marginal error reached the requested tolerance";
  return KMVP_E_NOT_CONVERGED;
}

}  // namespace

int sinkhorn_solve(kmvp_ctx* c, int kernel, const double* log_a, const double* log_b, double tol, int maxit, double* u,
                   double* v, int* iters, double* err) {
  if (!c) return KMVP_E_INVALID;
  c->note.clear();
  if (!c->have_points) return fail(c, KMVP_E_INVALID, "kmvp_set_points has not been called");
  if (!(tol >= 0.0) || maxit < 1 || !u || !v || !iters || !err)
    return fail(c, KMVP_E_INVALID, "bad Sinkhorn arguments (tol >= 0, maxit >= 1, u, v, iters and err are all required)");
  if (c->dtype == KMVP_BF16)
    return fail(c, KMVP_E_UNSUPPORTED, "Sinkhorn: built for float32 and float64 contexts, not for bfloat16");
  if (c->D > LOWD_MAX_D)
    return fail(c, KMVP_E_UNSUPPORTED, "Sinkhorn: D = " + std::to_string(c->D) + " is beyond the log-sum-exp kernels' D <= " +
                                           std::to_string(LOWD_MAX_D));
  if (c->opt_fast >= 1)
    return fail(c, KMVP_E_UNSUPPORTED, "Sinkhorn: fast_sqdists = " + std::to_string(c->opt_fast) +
                                           " asks for a matrix-core form that is not built for it (-1 or 0: the difference form)");
  if (c->exchanges())
    return fail(c, KMVP_E_UNSUPPORTED, "Sinkhorn: a communicator is attached, and the sharded iteration is not built");
  if (c->M < c->m_total)
    return fail(c, KMVP_E_UNSUPPORTED, "Sinkhorn: the sources are a slice (M < M_total), and the sharded iteration is not built");
  if (c->N < 1 || c->M < 1) return fail(c, KMVP_E_INVALID, "Sinkhorn needs at least one point on each side");
  HIP_TRY(c, hipSetDevice(c->device));
  return c->dtype == KMVP_F64 ? sinkhorn_t<double>(c, kernel, log_a, log_b, tol, maxit, u, v, iters, err)
                              : sinkhorn_t<float>(c, kernel, log_a, log_b, tol, maxit, u, v, iters, err);
}

}  // namespace kmvp
