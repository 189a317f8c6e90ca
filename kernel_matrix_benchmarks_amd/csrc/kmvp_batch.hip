// Batched clouds (include/kmvp.h kmvp_set_batches): many small clouds in one pair of arrays, one launch for all of them.
//   set_batches           checks the offsets, builds the plan (kmvp_batch_plan.hpp) and uploads its tile table and maps
//   run_product_batched   the block-diagonal product on lowd_batch_kernel
//   run_nearest_batched   the K nearest sources of every target within its own batch on lowd_batch_knn_kernel
// Target image, records, tile table and maps live in buffers of their own (bt_*): the product's pack bookkeeping
// (points_stale, record_packed) and its xs / rec buffers are never touched, so the plain entries return the same bits with
// batches off whatever ran in between.  The coordinates are packed once per (kmvp_set_points, kmvp_set_batches) and record
// length; a new signal rewrites the records' signal slots only.
#include "kmvp_ctx.hpp"
#include "kmvp_lowd_batch.hpp"

namespace kmvp {

namespace {

const char* const OFF_HINT = " (kmvp_set_batches with B = 0 switches the batches off)";

// Packs whatever of the batched layouts is stale for records of R reals with EB signal columns (0: the density layout).
template <typename real>
int pack_batched(kmvp_ctx* c, int R, int EB) {
  const int D = c->D;
  int rc;
  const real* x_raw = (const real*)(c->same_points ? c->y_raw.p : c->x_raw.p);
  if (c->bt_xs_points_ver != c->points_ver || c->bt_xs_ver != c->bt_ver) {
    if ((rc = ensure(c, c->bt_xs, (size_t)D * c->bt_n_pad * sizeof(real)))) return rc;
    hipLaunchKernelGGL((batch_pack_targets_kernel<real>), dim3(blocks_for(c->bt_n_pad)), dim3(256), 0, c->stream, x_raw,
                       (const int64_t*)c->bt_tmap.p, (real*)c->bt_xs.p, c->bt_n_pad, D);
    HIP_TRY(c, hipGetLastError());
    c->bt_xs_points_ver = c->points_ver;
    c->bt_xs_ver = c->bt_ver;
  }
  if (c->bt_rec_points_ver != c->points_ver || c->bt_rec_ver != c->bt_ver || c->bt_rec_R != R) {
    if ((rc = ensure(c, c->bt_rec, (size_t)c->bt_m_alloc * R * sizeof(real)))) return rc;
    hipLaunchKernelGGL((batch_pack_sources_kernel<real>), dim3(blocks_for(c->bt_m_alloc)), dim3(256), 0, c->stream,
                       (const real*)c->y_raw.p, (const int64_t*)c->bt_smap.p, (real*)c->bt_rec.p, c->bt_m_alloc, D, R);
    HIP_TRY(c, hipGetLastError());
    c->bt_rec_points_ver = c->points_ver;
    c->bt_rec_ver = c->bt_ver;
    c->bt_rec_R = R;
    c->bt_sig_ver = 0;  // the signal slots were zeroed
    c->bt_sig_EB = 0;
  }
  if (EB > 0 && (c->bt_sig_ver != c->signal_ver || c->bt_sig_EB != EB)) {
    hipLaunchKernelGGL((batch_pack_signal_kernel<real>), dim3(blocks_for(c->bt_m_alloc)), dim3(256), 0, c->stream,
                       (const real*)c->b_raw.p, (const int64_t*)c->bt_smap.p, (real*)c->bt_rec.p, c->bt_m_alloc, D, EB, R);
    HIP_TRY(c, hipGetLastError());
    c->bt_sig_ver = c->signal_ver;
    c->bt_sig_EB = EB;
  }
  return KMVP_OK;
}

template <typename real>
LowdBatchArgs<real> batch_args(const kmvp_ctx* c, double* out, int kc) {
  LowdBatchArgs<real> a;
  a.xs = (const real*)c->bt_xs.p;
  a.rec = (const real*)c->bt_rec.p;
  a.tiles = (const BatchTile*)c->bt_tiles.p;
  a.out = out;
  a.n_pad = c->bt_n_pad;
  a.n = c->N;
  a.chunk = (int)round_up(c->opt_chunk > 8 ? c->opt_chunk : 8, LOWD_BATCH);  // lowd_geometry's rule
  a.kc = kc;
  return a;
}

inline hipError_t launch_batch(int kernel, int D, int E, int sig, const LowdBatchArgs<float>& a, dim3 grid, hipStream_t s,
                               const char** name) {
  return launch_lowd_batch_f32(kernel, D, E, sig, a, grid, s, name);
}
inline hipError_t launch_batch(int kernel, int D, int E, int sig, const LowdBatchArgs<double>& a, dim3 grid, hipStream_t s,
                               const char** name) {
  return launch_lowd_batch_f64(kernel, D, E, sig, a, grid, s, name);
}
inline hipError_t launch_batch_knn(int D, int KT, const LowdBatchArgs<float>& a, dim3 grid, hipStream_t s, const char** name) {
  return launch_lowd_batch_knn_f32(D, KT, a, grid, s, name);
}
inline hipError_t launch_batch_knn(int D, int KT, const LowdBatchArgs<double>& a, dim3 grid, hipStream_t s, const char** name) {
  return launch_lowd_batch_knn_f64(D, KT, a, grid, s, name);
}

// Normalised density: the rows of a normalised matrix sum to one (bruteforce.py:134-138) -- where the batch has a source;
// 0 / 0 where it has none, as the plain entry's M = 0.  One thread per target slot.
__global__ void batch_ones_kernel(const BatchTile* __restrict__ tiles, double* __restrict__ out, int64_t n_pad) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= n_pad) return;
  const BatchTile t = tiles[s / BATCH_TILE];
  const int l = (int)(s % BATCH_TILE);
  if (l < t.live) out[t.i0 + l] = t.len > 0 ? 1.0 : __builtin_nan("");
}

template <typename real>
int run_product_batched_t(kmvp_ctx* c, int kernel, int sig) {
  const int D = c->D;
  const int E = sig == SIG_DENSITY ? 1 : c->E;
  const int EB = sig == SIG_DENSITY ? 0 : E;
  const int R = (D + EB + 3) / 4 * 4;
  int rc;
  HIP_TRY(c, hipEventRecord(c->ev[0], c->stream));
  if ((rc = pack_batched<real>(c, R, EB))) return rc;
  if ((rc = ensure(c, c->out, (size_t)c->N * E * sizeof(double)))) return rc;
  const LowdBatchArgs<real> a = batch_args<real>(c, (double*)c->out.p, 0);
  HIP_TRY(c, hipEventRecord(c->ev[0], c->stream));
  hipError_t le = launch_batch(kernel, D, E, sig, a, dim3((unsigned)(c->bt_n_pad / (BATCH_TILE * BATCH_WAVES))), c->stream,
                               &c->last_kernel_name);
  if (le == hipErrorInvalidValue) return fail(c, KMVP_E_UNSUPPORTED, "batched clouds: no kernel instantiated for this (kernel, D, E)");
  HIP_TRY(c, le);
  HIP_TRY(c, hipEventRecord(c->ev[1], c->stream));
  HIP_TRY(c, hipEventRecord(c->ev[2], c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipEventElapsedTime(&c->last_kernel_ms, c->ev[0], c->ev[1]));
  HIP_TRY(c, hipEventElapsedTime(&c->last_total_ms, c->ev[0], c->ev[2]));
  c->last_allreduce_ms = 0.f;
  c->out_n = c->N;
  c->out_e = E;
  return KMVP_OK;
}

template <typename real>
int run_nearest_batched_t(kmvp_ctx* c, int K, double* cand) {
  const int D = c->D;
  const int R = (D + 3) / 4 * 4;  // density layout: no signal columns
  int rc;
  if ((rc = pack_batched<real>(c, R, 0))) return rc;
  const LowdBatchArgs<real> a = batch_args<real>(c, cand, K);
  HIP_TRY(c, hipEventRecord(c->ev[0], c->stream));
  hipError_t le = launch_batch_knn(D, knn_capacity(K), a, dim3((unsigned)(c->bt_n_pad / (BATCH_TILE * BATCH_WAVES))), c->stream,
                                   &c->last_kernel_name);
  if (le == hipErrorInvalidValue) return fail(c, KMVP_E_UNSUPPORTED, "batched clouds: no kernel instantiated for this (D, K)");
  HIP_TRY(c, le);
  HIP_TRY(c, hipEventRecord(c->ev[1], c->stream));
  return KMVP_OK;
}

}  // namespace

// What the batched entries are not built for, beyond their own arguments; `what` opens the message.
int batched_unsupported(kmvp_ctx* c, const std::string& what) {
  const std::string tail = std::string(" (batched clouds, kmvp_set_batches)") + OFF_HINT;
  if (c->dtype == KMVP_BF16)
    return fail(c, KMVP_E_UNSUPPORTED, what + ": the batches are built for float32 and float64 contexts, not for bfloat16" + tail);
  if (c->D > LOWD_MAX_D)
    return fail(c, KMVP_E_UNSUPPORTED, what + ": D = " + std::to_string(c->D) + " is beyond the batches' kernels' D <= " +
                                           std::to_string(LOWD_MAX_D) + tail);
  if (c->opt_fast >= 1)
    return fail(c, KMVP_E_UNSUPPORTED, what + ": fast_sqdists = " + std::to_string(c->opt_fast) +
                                           " asks for a matrix-core form that is not built for the batches (-1 or 0: the difference form)" + tail);
  if (c->exchanges())
    return fail(c, KMVP_E_UNSUPPORTED, what + ": the batches are not built for a context with a communicator attached" + tail);
  if (c->M < c->m_total)
    return fail(c, KMVP_E_UNSUPPORTED, what + ": the batches are not built for a source slice (M < M_total)" + tail);
  return KMVP_OK;
}

int batches_refuse(kmvp_ctx* c, const char* what) {
  if (!c || !c->bt_on) return KMVP_OK;
  return fail(c, KMVP_E_UNSUPPORTED, std::string(what) + " is not built for batched clouds (kmvp_set_batches): the batches serve the "
                                         "Gaussian, exp(-r) and Matern products and kmvp_nearest without exclude_self" + OFF_HINT);
}

int set_batches(kmvp_ctx* c, int B, const int64_t* y_off, const int64_t* x_off) {
  if (!c) return KMVP_E_INVALID;
  if (!c->have_points) return fail(c, KMVP_E_INVALID, "batches: kmvp_set_points has not been called");
  if (B < 0) return fail(c, KMVP_E_INVALID, "batches: B must be >= 0");
  if (B == 0) {
    if (y_off || x_off) return fail(c, KMVP_E_INVALID, "batches: B = 0 (off) takes NULL offsets");
    c->bt_on = false;
    c->bt_B = 0;
    return KMVP_OK;
  }
  if (!y_off) return fail(c, KMVP_E_INVALID, "batches: y_offsets is NULL");
  if (!x_off && !c->same_points)
    return fail(c, KMVP_E_INVALID, "batches: x_offsets may be NULL only when the targets are the sources (x == NULL at kmvp_set_points)");
  if (!x_off) x_off = y_off;
  static const char* const why[] = {"", "do not start at 0", "are not monotone", "do not end at the number of points"};
  int bad;
  if ((bad = batch_offsets_check(B, y_off, c->M)))
    return fail(c, KMVP_E_INVALID, std::string("batches: y_offsets ") + why[bad] + " (B + 1 non-decreasing values from 0 to M = " +
                                       std::to_string(c->M) + ")");
  if ((bad = batch_offsets_check(B, x_off, c->N)))
    return fail(c, KMVP_E_INVALID, std::string("batches: x_offsets ") + why[bad] + " (B + 1 non-decreasing values from 0 to N = " +
                                       std::to_string(c->N) + ")");
  BatchPlan p;
  if (!batch_plan_build(B, y_off, x_off, p))
    return fail(c, KMVP_E_UNSUPPORTED, "batches: a batch of 2^31 sources or more (the pair loop counts positions within a batch in 32 bits)");
  if (p.n_pad / (BATCH_TILE * BATCH_WAVES) > MAX_GRID) return fail(c, KMVP_E_UNSUPPORTED, "batches: launch grid too large");
  HIP_TRY(c, hipSetDevice(c->device));
  // (the previous setting survives every refusal above; a device failure from here on leaves the batches off)
  c->bt_on = false;
  int rc;
  if ((rc = ensure(c, c->bt_tiles, p.tiles.size() * sizeof(BatchTile)))) return rc;
  if ((rc = ensure(c, c->bt_tmap, p.tmap.size() * sizeof(int64_t)))) return rc;
  if ((rc = ensure(c, c->bt_smap, p.smap.size() * sizeof(int64_t)))) return rc;
  if (!p.tiles.empty())
    HIP_TRY(c, hipMemcpyAsync(c->bt_tiles.p, p.tiles.data(), p.tiles.size() * sizeof(BatchTile), hipMemcpyHostToDevice, c->stream));
  if (!p.tmap.empty())
    HIP_TRY(c, hipMemcpyAsync(c->bt_tmap.p, p.tmap.data(), p.tmap.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->bt_smap.p, p.smap.data(), p.smap.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // the plan's vectors are only read during the call
  c->bt_n_pad = p.n_pad;
  c->bt_m_alloc = p.m_alloc;
  c->bt_B = B;
  c->bt_y_off.assign(y_off, y_off + B + 1);
  c->bt_x_off.assign(x_off, x_off + B + 1);
  ++c->bt_ver;
  c->bt_on = true;
  return KMVP_OK;
}

int run_product_batched(kmvp_ctx* c, int kernel, bool normalise) {
  if (!c) return KMVP_E_INVALID;
  c->note.clear();
  if (!c->have_points) return fail(c, KMVP_E_INVALID, "kmvp_set_points has not been called");
  if (!c->have_signal) return fail(c, KMVP_E_INVALID, "kmvp_set_signal has not been called");
  HIP_TRY(c, hipSetDevice(c->device));
  int rc;
  if ((rc = batched_unsupported(c, "product"))) return rc;
  const int E = c->density ? 1 : c->E;
  if (E > LOWD_MAX_E)
    return fail(c, KMVP_E_UNSUPPORTED, "product: E = " + std::to_string(E) + " signal columns are beyond the batches' kernels' E <= " +
                                           std::to_string(LOWD_MAX_E) + " (batched clouds, kmvp_set_batches: run it per block of columns)");
  c->last_kernel_ms = c->last_total_ms = c->last_allreduce_ms = 0.f;
  if (c->N == 0) {
    if ((rc = ensure(c, c->out, 16))) return rc;
    c->out_n = 0;
    c->out_e = E;
    c->last_kernel_name = "none";
    return KMVP_OK;
  }
  if (c->density && normalise) {
    if ((rc = ensure(c, c->out, (size_t)c->N * sizeof(double)))) return rc;
    hipLaunchKernelGGL(batch_ones_kernel, dim3(blocks_for(c->bt_n_pad)), dim3(256), 0, c->stream, (const BatchTile*)c->bt_tiles.p,
                       (double*)c->out.p, c->bt_n_pad);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->out_n = c->N;
    c->out_e = 1;
    c->last_kernel_name = "fill_kernel";
    return KMVP_OK;
  }
  const int sig = c->density ? SIG_DENSITY : (normalise ? SIG_NORM : SIG_PRODUCT);
  return c->dtype == KMVP_F64 ? run_product_batched_t<double>(c, kernel, sig) : run_product_batched_t<float>(c, kernel, sig);
}

int run_nearest_batched(kmvp_ctx* c, int K, int exclude_self, int64_t* out_idx, double* out_sqdist) {
  if (!c) return KMVP_E_INVALID;
  c->note.clear();
  if (!c->have_points) return fail(c, KMVP_E_INVALID, "kmvp_set_points has not been called");
  if (K < 1) return fail(c, KMVP_E_INVALID, "nearest: K must be >= 1");
  if (exclude_self)
    return fail(c, KMVP_E_UNSUPPORTED, std::string("nearest: exclude_self is not built for batched clouds (kmvp_set_batches)") + OFF_HINT);
  if (c->N > 0 && (!out_idx || !out_sqdist)) return fail(c, KMVP_E_INVALID, "nearest: a NULL output");
  HIP_TRY(c, hipSetDevice(c->device));
  int rc;
  if ((rc = batched_unsupported(c, "nearest"))) return rc;
  if (K > KNN_MAX_K)
    return fail(c, KMVP_E_UNSUPPORTED, "nearest: K = " + std::to_string(K) + " is beyond the lists' K <= 16");
  const int64_t N = c->N;
  c->last_kernel_ms = c->last_total_ms = c->last_allreduce_ms = 0.f;
  c->last_kernel_name = "none";
  if (N == 0) return KMVP_OK;

  // candidates [2 K][N] in c->sums, as the plain entry: scratch of the context that no entry expects to survive a call
  const int64_t cnt = (int64_t)2 * K * N;
  if ((rc = ensure(c, c->sums, (size_t)cnt * sizeof(double)))) return rc;
  double* cand = (double*)c->sums.p;
  if ((rc = c->dtype == KMVP_F64 ? run_nearest_batched_t<double>(c, K, cand) : run_nearest_batched_t<float>(c, K, cand))) return rc;
  const size_t nk = (size_t)N * K;
  if ((rc = ensure(c, c->knn, nk * (sizeof(int64_t) + sizeof(double))))) return rc;
  int64_t* d_idx = (int64_t*)c->knn.p;
  double* d_sq = (double*)(d_idx + nk);
  hipLaunchKernelGGL(knn_finish_kernel, dim3(blocks_for(N)), dim3(256), 0, c->stream, cand, d_idx, d_sq, N, K, 0);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipEventRecord(c->ev[2], c->stream));
  HIP_TRY(c, hipMemcpyAsync(out_idx, d_idx, nk * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(out_sqdist, d_sq, nk * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipEventElapsedTime(&c->last_kernel_ms, c->ev[0], c->ev[1]));
  HIP_TRY(c, hipEventElapsedTime(&c->last_total_ms, c->ev[0], c->ev[2]));
  return KMVP_OK;
}

}  // namespace kmvp
