// Gaussian mean-shift on the gradient of the log-sum-exp (include/kmvp.h kmvp_gaussian_meanshift): what kmvp_sinkhorn.hip is
// to the log-sum-exp and kmvp_kmeans.hip to the arg-K-min.  The pair loop is lowd_lse_grad_kernel<K_GAUSSIAN, D, 1, sig>,
// untouched, with its segment merge and the quotient V / Z of its finish kernel; this file is the iteration around it.
//
// For the Gaussian G = -2 (x - ybar), ybar the softmax-weighted barycentre of the sources, so x + G / 2 IS the mean-shift
// update, on the integer shift of the log-sum-exp: finite for a seed so far from the data that the float32 product is 0 / 0.
//
// The seeds are the context's targets.  Their positions z (N, D) stay fp64 on the device; what moves through the pair loop
// is a target image of the ACTIVE points only, in a buffer of the solver's own.  The source records are the product's own
// (c->rec under the product's PackKey and signal bookkeeping, packed only if stale, exactly as run_logsumexp_grad_t does).
//
// One sweep k with n_act active points (known to the host from the previous look), seven launches, no atomics of ours:
//   ms_pack_kernel         real(z[act[slot]]) into the target image, SoA [d][n_pad(n_act)], pad targets 0
//   lowd_lse_grad_kernel   the grid covers the active tiles times the PINNED segments (below)
//   lse_grad_reduce_kernel the segments: sums [D + 1][n_pad], exponents [n_pad]
//   ms_step_kernel         G = lse_grad_value(...) -- finish_lse_grad_kernel's own expression --, then the rule of
//                          kmvp_meanshift_step.hpp: z_k, q, the freeze, iters and step2, and one keep flag per slot
//   DeviceSelect::Flagged  hipcub's order-preserving, deterministic stream compaction of the index list by the keep flags
//                          into the other list of the ping-pong pair, and the number kept
//   ms_state_kernel        [stop, sweeps, n_active, target_sweeps]
// The host reads those four words after every sweep and sizes the next launch from them; nothing else crosses the bus
// until the end.
//
// What enters the bits of a point's trajectory is its own arithmetic (lanes are targets, the shift moves per lane) and the
// geometry of the SOURCE axis: segment count, seg_len, chunk.  That geometry is pinned at the first sweep to what
// lowd_geometry gives kmvp_gaussian_logsumexp_grad for these (N, M, options), and kept while the active set shrinks: only
// n, n_pad and tile_blocks follow the active count.  So the solve walks through the bits of a host loop that calls
// kmvp_gaussian_logsumexp_grad with all N targets every sweep, whatever the other points do.
//
// "meanshift_compact" = 0 never swaps the lists: all N slots ride through every sweep, the step ignores the frozen ones
// (iters != 0), and the selection still runs for the count.  Same bits, by the independence above; it exists to measure what
// compaction saves.
#include <hipcub/hipcub.hpp>

#include "kmvp_ctx.hpp"
#include "kmvp_meanshift_step.hpp"

namespace kmvp {
namespace {

// the state words: stop, sweeps, n_active, target_sweeps
constexpr size_t MS_STATE_WORDS = 4;

// positions from the seeds, the identity list, nobody frozen
template <typename real>
__global__ void ms_init_kernel(const real* __restrict__ x, double* __restrict__ z, double* __restrict__ step2, int* __restrict__ iters,
                               int* __restrict__ act, int64_t n, int D) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  for (int d = 0; d < D; ++d) z[i * D + d] = (double)x[i * D + d];
  step2[i] = 0.0;
  iters[i] = 0;
  act[i] = (int)i;
}

// the target image of the active points: xs[d * n_pad + slot] = real(z[act[slot]][d]); pad targets are 0 (pack_targets_kernel)
template <typename real>
__global__ void ms_pack_kernel(const double* __restrict__ z, const int* __restrict__ act, real* __restrict__ xs, int64_t n_act,
                               int64_t n_pad, int D) {
  const int64_t slot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= n_pad) return;
  const int64_t i = slot < n_act ? act[slot] : 0;
  for (int d = 0; d < D; ++d) xs[(int64_t)d * n_pad + slot] = slot < n_act ? (real)z[i * D + d] : (real)0;
}

// One thread per slot of the active list.  sums [D + 1][n_pad] and kshift [n_pad] are the segment merge's; keep[slot] = 1
// where the point goes on.  A slot whose point froze in an earlier sweep (only without compaction) is left alone.
template <int D, typename real>
__global__ void __launch_bounds__(256) ms_step_kernel(const double* __restrict__ sums, const double* __restrict__ kshift,
                                                      int64_t n_pad, const int* __restrict__ act, int64_t n_act, int sweep,
                                                      double tol, double* __restrict__ z, double* __restrict__ step2,
                                                      int* __restrict__ iters, unsigned char* __restrict__ keep) {
  const int64_t slot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (slot >= n_act) return;
  const int64_t i = act[slot];
  if (iters[i] != 0) {
    keep[slot] = 0;
    return;
  }
  const bool none = !(kshift[slot] < 1.0e300);
  const double zsum = sums[slot];
  double G[D], base[D], zn[D], q;
#pragma unroll
  for (int d = 0; d < D; ++d) {
    G[d] = lse_grad_value(none, -2.0, sums[(int64_t)(1 + d) * n_pad + slot], zsum);
    base[d] = (double)(real)z[i * D + d];
  }
  const int verdict = ms_step_point(G, base, D, tol, zn, &q);
#pragma unroll
  for (int d = 0; d < D; ++d) z[i * D + d] = zn[d];
  step2[i] = q;
  if (verdict != MS_ACTIVE) iters[i] = sweep;
  keep[slot] = verdict == MS_ACTIVE ? 1 : 0;
}

template <typename real>
void launch_ms_step(int D, dim3 grid, hipStream_t stream, const double* sums, const double* kshift, int64_t n_pad, const int* act,
                    int64_t n_act, int sweep, double tol, double* z, double* step2, int* iters, unsigned char* keep) {
#define KMVP_MS_CASE(DD)                                                                                                      \
  case DD:                                                                                                                    \
    hipLaunchKernelGGL((ms_step_kernel<DD, real>), grid, dim3(256), 0, stream, sums, kshift, n_pad, act, n_act, sweep, tol, z, \
                       step2, iters, keep);                                                                                   \
    break;
  switch (D) {
    KMVP_MS_CASE(1) KMVP_MS_CASE(2) KMVP_MS_CASE(3) KMVP_MS_CASE(4) KMVP_MS_CASE(5) KMVP_MS_CASE(6) KMVP_MS_CASE(7) KMVP_MS_CASE(8)
  }
#undef KMVP_MS_CASE
}

// st = [stop | sweeps | n_active | target_sweeps]: the sweep that just ran had st[2] active points; *kept go on
__global__ void ms_state_kernel(int64_t* __restrict__ st, const int* __restrict__ kept, int maxit) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  const int64_t sweeps = st[1] + 1, n = *kept;
  st[3] += st[2];
  st[2] = n;
  st[1] = sweeps;
  st[0] = (n == 0 || sweeps >= (int64_t)maxit) ? 1 : 0;
}

template <typename real>
int meanshift_t(kmvp_ctx* c, double tol, int maxit, double* modes, int* iters, double* step2, int* sweeps, int64_t* target_sweeps) {
  const int D = c->D, NS = D + 1;
  const int64_t N = c->N, M = c->M;
  const int sig = c->density ? SIG_DENSITY : SIG_PRODUCT;
  const int EB = sig == SIG_DENSITY ? 0 : 1;
  const int R = (D + EB + 3) / 4 * 4;
  const bool compact = c->opt_meanshift_compact != 0;
  int rc;
  // the launch of kmvp_gaussian_logsumexp_grad for all N targets: its source axis is the pinned one
  LowdArgs<real> a = lowd_geometry<real>(N, M, c->opt_segments, c->opt_chunk, c->j_offset, c->m_total, 1, R, D + 2);
  const int64_t tile = 64 * (int64_t)WAVES_PER_BLOCK;
  const int64_t n_pad_all = a.n_pad;
  if ((int64_t)a.tile_blocks * a.segments > 0x7fffffff) return fail(c, KMVP_E_UNSUPPORTED, "launch grid too large");

  HIP_TRY(c, hipEventRecord(c->ev[0], c->stream));
  // ---- the product's layouts under the product's key, as run_logsumexp_grad_t: whichever runs first on these points and
  // this signal packs.  (Only the records are read here; the product's target image is packed with them so that the
  // bookkeeping stays true.)
  const real* x_raw = (const real*)(c->same_points ? c->y_raw.p : c->x_raw.p);
  const PackKey key = {LAYOUT_LOWD, K_GAUSSIAN, 1};
  if (points_stale(c, key)) {
    if ((rc = ensure(c, c->xs, (size_t)D * n_pad_all * sizeof(real)))) return rc;
    hipLaunchKernelGGL((pack_targets_kernel<real>), dim3(blocks_for(n_pad_all)), dim3(256), 0, c->stream, x_raw, (real*)c->xs.p, N,
                       n_pad_all, D, (real)1);
  }
  if (signal_stale(c, key, sig)) {
    if ((rc = ensure(c, c->rec, (size_t)(a.m_pad + LOWD_BATCH) * R * sizeof(real)))) return rc;
    hipLaunchKernelGGL((pack_sources_kernel<real>), dim3(blocks_for(a.m_pad + LOWD_BATCH)), dim3(256), 0, c->stream,
                       (const real*)c->y_raw.p, (const real*)c->b_raw.p, (real*)c->rec.p, M, a.m_pad + LOWD_BATCH, D, EB, R, (real)1);
  }
  HIP_TRY(c, hipGetLastError());
  record_packed(c, key, sig);

  // ---- buffers: the scratch of one gradient (shared with it: rewritten by every call), sized for all N targets, and the
  // solver's own
  if ((rc = ensure(c, c->part, (size_t)a.segments * (NS + 1) * n_pad_all * sizeof(double)))) return rc;
  if ((rc = ensure(c, c->sums, (size_t)NS * n_pad_all * sizeof(double)))) return rc;
  if ((rc = ensure(c, c->kshift, (size_t)n_pad_all * sizeof(double)))) return rc;
  if ((rc = ensure(c, c->ms_xs, (size_t)D * n_pad_all * sizeof(real)))) return rc;
  // [z N D | step2 N] doubles, [state] int64, [iters N | list N | list N | kept 1 (+ 1 pad)] ints, [keep N] bytes
  const size_t bytes = ((size_t)N * D + (size_t)N) * sizeof(double) + MS_STATE_WORDS * sizeof(int64_t) +
                       ((size_t)3 * N + 2) * sizeof(int) + (size_t)N;
  if ((rc = ensure(c, c->ms_state, bytes))) return rc;
  double* z = (double*)c->ms_state.p;
  double* d_step2 = z + (size_t)N * D;
  int64_t* st = (int64_t*)(d_step2 + N);
  int* d_iters = (int*)(st + MS_STATE_WORDS);
  int* list[2] = {d_iters + N, d_iters + 2 * N};
  int* kept = d_iters + 3 * N;
  unsigned char* keep = (unsigned char*)(kept + 2);
  size_t tmp_bytes = 0;
  HIP_TRY(c, hipcub::DeviceSelect::Flagged(nullptr, tmp_bytes, list[0], keep, list[1], kept, (int)N, c->stream));
  if ((rc = ensure(c, c->ms_tmp, std::max<size_t>(tmp_bytes, 16)))) return rc;

  hipLaunchKernelGGL((ms_init_kernel<real>), dim3(blocks_for(N)), dim3(256), 0, c->stream, x_raw, z, d_step2, d_iters, list[0], N, D);
  HIP_TRY(c, hipGetLastError());
  int64_t state[MS_STATE_WORDS] = {0, 0, N, 0};
  HIP_TRY(c, hipMemcpyAsync(st, state, sizeof(state), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // (state is reused as the landing place below)

  a.xs = (const real*)c->ms_xs.p;
  a.rec = (const real*)c->rec.p;
  a.part = (double*)c->part.p;

  // ---- the iteration
  int cur = 0;
  int64_t n_act = N;
  while (state[0] == 0) {
    a.n = n_act;
    a.n_pad = round_up(n_act, tile);
    a.tile_blocks = (int)(a.n_pad / tile);
    const int sweep = (int)state[1] + 1;
    hipLaunchKernelGGL((ms_pack_kernel<real>), dim3(blocks_for(a.n_pad)), dim3(256), 0, c->stream, (const double*)z,
                       (const int*)list[cur], (real*)c->ms_xs.p, n_act, a.n_pad, D);
    HIP_TRY(c, launch_lowd_lse_grad(K_GAUSSIAN, D, 1, sig, a, dim3((unsigned)(a.tile_blocks * a.segments)), c->stream,
                                    &c->last_kernel_name));
    hipLaunchKernelGGL(lse_grad_reduce_kernel, dim3(blocks_for(NS * a.n_pad)), dim3(256), 0, c->stream, (const double*)c->part.p,
                       (double*)c->sums.p, (double*)c->kshift.p, a.n_pad, NS, a.segments);
    launch_ms_step<real>(D, dim3(blocks_for(n_act)), c->stream, (const double*)c->sums.p, (const double*)c->kshift.p, a.n_pad,
                         (const int*)list[cur], n_act, sweep, tol, z, d_step2, d_iters, keep);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipcub::DeviceSelect::Flagged(c->ms_tmp.p, tmp_bytes, list[cur], keep, list[cur ^ 1], kept, (int)n_act, c->stream));
    hipLaunchKernelGGL(ms_state_kernel, dim3(1), dim3(64), 0, c->stream, st, (const int*)kept, maxit);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(state, st, sizeof(state), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (compact) {
      cur ^= 1;
      n_act = state[2];
    }
  }

  HIP_TRY(c, hipMemcpyAsync(modes, z, (size_t)N * D * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(step2, d_step2, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(iters, d_iters, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipEventRecord(c->ev[2], c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipEventElapsedTime(&c->last_total_ms, c->ev[0], c->ev[2]));
  c->last_kernel_ms = c->last_total_ms;  // both cover the whole solve (include/kmvp.h)
  c->last_allreduce_ms = 0.f;
  *sweeps = (int)state[1];
  *target_sweeps = state[3];
  // the points still active at the end carry the sweep count; converged: every point froze with a finite q <= tol^2
  const double tol2 = tol * tol;
  int64_t open = 0, nonfinite = 0;
  for (int64_t i = 0; i < N; ++i) {
    if (iters[i] == 0) {
      iters[i] = *sweeps;
      ++open;
    } else if (!(step2[i] <= tol2)) {
      ++nonfinite;
    }
  }
  if (open == 0 && nonfinite == 0) return KMVP_OK;
  c->err = nonfinite ? "mean-shift: " + std::to_string(nonfinite) +
                           " point(s) froze on a gradient that is not finite (no source of positive mass, a NaN coordinate, or an "
                           "overflowed difference): their rows are NaN"
                     : "mean-shift stopped at maxit with " + std::to_string(open) + " point(s) still moving by more than the tolerance";
  return KMVP_E_NOT_CONVERGED;
}

}  // namespace

int meanshift_solve(kmvp_ctx* c, double tol, int maxit, double* modes, int* iters, double* step2, int* sweeps,
                    int64_t* target_sweeps) {
  if (!c) return KMVP_E_INVALID;
  c->note.clear();
  if (!c->have_points) return fail(c, KMVP_E_INVALID, "kmvp_set_points has not been called");
  if (!c->have_signal) return fail(c, KMVP_E_INVALID, "kmvp_set_signal has not been called");
  if (!(tol >= 0.0) || maxit < 1 || !modes || !iters || !step2 || !sweeps || !target_sweeps)
    return fail(c, KMVP_E_INVALID, "bad mean-shift arguments (tol >= 0, maxit >= 1, modes, iters, step2, sweeps and target_sweeps "
                                   "are all required)");
  if (c->dtype == KMVP_BF16)
    return fail(c, KMVP_E_UNSUPPORTED, "mean-shift: built for float32 and float64 contexts, not for bfloat16");
  if (c->D > LOWD_MAX_D)
    return fail(c, KMVP_E_UNSUPPORTED, "mean-shift: D = " + std::to_string(c->D) + " is beyond the log-sum-exp gradient kernels' D <= " +
                                           std::to_string(LOWD_MAX_D));
  if (!c->density && c->E != 1)
    return fail(c, KMVP_E_UNSUPPORTED, "mean-shift: the signal has " + std::to_string(c->E) + " columns; the log-weights are one column");
  if (c->opt_fast >= 1)
    return fail(c, KMVP_E_UNSUPPORTED, "mean-shift: fast_sqdists = " + std::to_string(c->opt_fast) +
                                           " asks for a matrix-core form that is not built for it (-1 or 0: the difference form)");
  if (c->exchanges())
    return fail(c, KMVP_E_UNSUPPORTED, "mean-shift: a communicator is attached, and the sharded iteration is not built");
  if (c->M < c->m_total)
    return fail(c, KMVP_E_UNSUPPORTED, "mean-shift: the sources are a slice (M < M_total), and the sharded iteration is not built");
  if (c->N < 1 || c->M < 1) return fail(c, KMVP_E_INVALID, "mean-shift needs at least one seed and one source");
  if (c->N > 0x7fffffff) return fail(c, KMVP_E_UNSUPPORTED, "mean-shift: more than 2^31 - 1 seeds");
  HIP_TRY(c, hipSetDevice(c->device));
  return c->dtype == KMVP_F64 ? meanshift_t<double>(c, tol, maxit, modes, iters, step2, sweeps, target_sweeps)
                              : meanshift_t<float>(c, tol, maxit, modes, iters, step2, sweeps, target_sweeps);
}

}  // namespace kmvp
