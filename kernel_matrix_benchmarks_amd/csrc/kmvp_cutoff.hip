// Cutoff-radius products and neighbour counts (include/kmvp.h kmvp_<kernel>_cutoff, kmvp_radius_count, kmvp_cutoff_info).
//   cutoff_prepare   the cell-list plan, once per (points, radius, factor, "cutoff_plan"): on the host (cutoff_plan_host
//                    copies the points back, widens them exactly to double, runs kmvp_cutoff_plan.hpp's build and uploads
//                    its two tables and two maps) or, "cutoff_plan" = 1, on the device (kmvp_cutoff_plan_device.hip: the
//                    same entries with no transfer that grows with the clouds)
//   cutoff_plan_read the plan back from the buffers the kernels read (kmvp_cutoff_plan_read)
//   pack_cutoff      the gather-packs of the batched clouds (kmvp_lowd_batch.hpp) through the plan's maps
//   run_cutoff       the truncated product on lowd_cutoff_kernel
//   run_cutoff_grad  its gradient with respect to the targets on lowd_cutoff_grad_kernel: the same plan, the same packs
//   radius_count     the neighbour counts on lowd_cutoff_count_kernel
//   radius_nearest   the K nearest sources inside the radius on lowd_cutoff_knn_kernel: the count's plan and packs, and an
//                    int32 copy of the plan's source map, narrowed on the device once per plan
//   cutoff_count_device  the count's setup and walk with the counts left on the device: the first step of kmvp_dbscan.hip
//   wendland_cg_solve / cutoff_apply   conjugate gradients (kmvp_solvers.hip cg_solve) with the Wendland cutoff product as
//                    its operator: plan and packs once, then two launches per application
// Target image, records, tables and maps live in buffers of their own (ct_*): the product's pack bookkeeping
// (points_stale, record_packed), its xs / rec buffers and the batches' bt_* are never touched, so every other entry
// returns the same bits whatever ran in between.  The coordinates are packed once per plan and record length; a new
// signal rewrites the records' signal slots only.
#include <chrono>

#include "kmvp_ctx.hpp"
#include "kmvp_lowd_batch.hpp"
#include "kmvp_lowd_cutoff.hpp"
#include "kmvp_lowd_cutoff_grad.hpp"
#include "kmvp_lowd_cutoff_knn.hpp"

namespace kmvp {

namespace {

// What the cutoff entries are not built for, beyond their own arguments; `what` opens the message.
int cutoff_unsupported(kmvp_ctx* c, const std::string& what) {
  const std::string tail = " (cutoff radius: kmvp_<kernel>_cutoff, kmvp_radius_count)";
  if (c->dtype == KMVP_BF16)
    return fail(c, KMVP_E_UNSUPPORTED, what + ": the cutoff is built for float32 and float64 contexts, not for bfloat16" + tail);
  if (c->D > CUTOFF_MAX_D)
    return fail(c, KMVP_E_UNSUPPORTED, what + ": D = " + std::to_string(c->D) + " is beyond the cutoff's cell list, D <= " +
                                           std::to_string(CUTOFF_MAX_D) + tail);
  if (c->exchanges())
    return fail(c, KMVP_E_UNSUPPORTED, what + ": the cutoff is not built for a context with a communicator attached" + tail);
  if (c->M < c->m_total)
    return fail(c, KMVP_E_UNSUPPORTED, what + ": the cutoff is not built for a source slice (M < M_total)" + tail);
  return batches_refuse(c, (what + " with a cutoff radius").c_str());
}

template <typename real>
void widen(const std::vector<real>& in, std::vector<double>& out) {
  out.resize(in.size());
  for (size_t i = 0; i < in.size(); ++i) out[i] = (double)in[i];
}

// The host build: the points copied back and widened exactly to double, cutoff_plan_build, its two tables and two maps
// uploaded.
template <typename real>
int cutoff_plan_host(kmvp_ctx* c, double radius, CutoffBuilt* out, double* ms) {
  const int D = c->D;
  std::vector<real> yh((size_t)c->M * D), xh(c->same_points ? 0 : (size_t)c->N * D);
  if (!yh.empty()) HIP_TRY(c, hipMemcpyAsync(yh.data(), c->y_raw.p, yh.size() * sizeof(real), hipMemcpyDeviceToHost, c->stream));
  if (!xh.empty()) HIP_TRY(c, hipMemcpyAsync(xh.data(), c->x_raw.p, xh.size() * sizeof(real), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<double> yd, xd;
  widen(yh, yd);
  widen(xh, xd);
  CutoffPlan p;
  if (!cutoff_plan_build(yd.data(), c->M, c->same_points ? yd.data() : xd.data(), c->N, D, radius, c->opt_cutoff_factor, p))
    return fail(c, KMVP_E_UNSUPPORTED, "cutoff radius: 2^31 sources or more (the pair loop counts positions within a run in 32 bits)");
  *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (p.n_pad / (CUTOFF_TILE * CUTOFF_WAVES) > MAX_GRID) return fail(c, KMVP_E_UNSUPPORTED, "cutoff radius: launch grid too large");
  c->ct_plan_points_ver = 0;  // (a device failure from here on leaves no plan behind)
  int rc;
  if ((rc = ensure(c, c->ct_tiles, p.tiles.size() * sizeof(CutoffTile)))) return rc;
  if ((rc = ensure(c, c->ct_runs, p.runs.size() * sizeof(CutoffRun)))) return rc;
  if ((rc = ensure(c, c->ct_tmap, p.tmap.size() * sizeof(int64_t)))) return rc;
  if ((rc = ensure(c, c->ct_smap, p.smap.size() * sizeof(int64_t)))) return rc;
  if (!p.tiles.empty())
    HIP_TRY(c, hipMemcpyAsync(c->ct_tiles.p, p.tiles.data(), p.tiles.size() * sizeof(CutoffTile), hipMemcpyHostToDevice, c->stream));
  if (!p.runs.empty())
    HIP_TRY(c, hipMemcpyAsync(c->ct_runs.p, p.runs.data(), p.runs.size() * sizeof(CutoffRun), hipMemcpyHostToDevice, c->stream));
  if (!p.tmap.empty())
    HIP_TRY(c, hipMemcpyAsync(c->ct_tmap.p, p.tmap.data(), p.tmap.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(c->ct_smap.p, p.smap.data(), p.smap.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // the plan's vectors are only read during the call
  for (int d = 0; d < 3; ++d) {
    out->g[d] = p.g[d];
    out->lo[d] = p.lo[d];
  }
  out->h = p.h;
  out->n_pad = p.n_pad;
  out->m_pad = p.m_pad;
  out->m_alloc = p.m_alloc;
  out->live_tiles = p.live_tiles;
  out->walked = p.walked;
  out->tiles = (int64_t)p.tiles.size();
  out->runs = (int64_t)p.runs.size();
  return KMVP_OK;
}

// The plan for (points, radius, factor, "cutoff_plan"), built unless the context holds it: on the host and uploaded, or on
// the device where the option asks for it and the cloud fits the device build's 32-bit keys.
template <typename real>
int cutoff_prepare(kmvp_ctx* c, double radius) {
  uint64_t bits;
  memcpy(&bits, &radius, sizeof(bits));
  if (c->ct_plan_points_ver == c->points_ver && c->ct_radius_bits == bits && c->ct_factor == c->opt_cutoff_factor &&
      c->ct_plan_opt == c->opt_cutoff_plan)
    return KMVP_OK;
  CutoffBuilt b;
  double ms = 0.0;
  int rc, built_on = 0;
  if (c->opt_cutoff_plan == 1) {
    bool fits = false;
    const auto t0 = std::chrono::steady_clock::now();
    c->ct_plan_points_ver = 0;  // (a device failure from here on leaves no plan behind)
    if ((rc = cutoff_plan_device(c, radius, &b, &fits))) return rc;
    ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (fits) {
      built_on = 1;
      if (b.n_pad / (CUTOFF_TILE * CUTOFF_WAVES) > MAX_GRID) return fail(c, KMVP_E_UNSUPPORTED, "cutoff radius: launch grid too large");
    }
  }
  if (!built_on && (rc = cutoff_plan_host<real>(c, radius, &b, &ms))) return rc;
  c->ct_n_pad = b.n_pad;
  c->ct_m_alloc = b.m_alloc;
  const int64_t info[8] = {b.g[0], b.g[1], b.g[2], b.live_tiles, b.runs, b.walked, b.m_pad, (int64_t)std::llround(ms)};
  memcpy(c->ct_info, info, sizeof(info));
  const double grid[4] = {b.lo[0], b.lo[1], b.lo[2], b.h};
  memcpy(c->ct_grid, grid, sizeof(grid));
  c->ct_tiles_n = b.tiles;
  c->ct_built_on = built_on;
  ++c->ct_ver;
  c->ct_plan_points_ver = c->points_ver;
  c->ct_radius_bits = bits;
  c->ct_factor = c->opt_cutoff_factor;
  c->ct_plan_opt = c->opt_cutoff_plan;
  return KMVP_OK;
}

// Packs whatever of the cutoff layouts is stale for records of R reals with EB signal columns (0: the density layout).
template <typename real>
int pack_cutoff(kmvp_ctx* c, int R, int EB) {
  const int D = c->D;
  int rc;
  const real* x_raw = (const real*)(c->same_points ? c->y_raw.p : c->x_raw.p);
  if (c->ct_xs_ver != c->ct_ver) {
    if ((rc = ensure(c, c->ct_xs, (size_t)D * c->ct_n_pad * sizeof(real)))) return rc;
    if (c->ct_n_pad > 0) {
      hipLaunchKernelGGL((batch_pack_targets_kernel<real>), dim3(blocks_for(c->ct_n_pad)), dim3(256), 0, c->stream, x_raw,
                         (const int64_t*)c->ct_tmap.p, (real*)c->ct_xs.p, c->ct_n_pad, D);
      HIP_TRY(c, hipGetLastError());
    }
    c->ct_xs_ver = c->ct_ver;
  }
  if (c->ct_rec_ver != c->ct_ver || c->ct_rec_R != R) {
    if ((rc = ensure(c, c->ct_rec, (size_t)c->ct_m_alloc * R * sizeof(real)))) return rc;
    hipLaunchKernelGGL((batch_pack_sources_kernel<real>), dim3(blocks_for(c->ct_m_alloc)), dim3(256), 0, c->stream,
                       (const real*)c->y_raw.p, (const int64_t*)c->ct_smap.p, (real*)c->ct_rec.p, c->ct_m_alloc, D, R);
    HIP_TRY(c, hipGetLastError());
    c->ct_rec_ver = c->ct_ver;
    c->ct_rec_R = R;
    c->ct_sig_ver = 0;  // the signal slots were zeroed
    c->ct_sig_EB = 0;
  }
  if (EB > 0 && (c->ct_sig_ver != c->signal_ver || c->ct_sig_EB != EB)) {
    hipLaunchKernelGGL((batch_pack_signal_kernel<real>), dim3(blocks_for(c->ct_m_alloc)), dim3(256), 0, c->stream,
                       (const real*)c->b_raw.p, (const int64_t*)c->ct_smap.p, (real*)c->ct_rec.p, c->ct_m_alloc, D, EB, R);
    HIP_TRY(c, hipGetLastError());
    c->ct_sig_ver = c->signal_ver;
    c->ct_sig_EB = EB;
  }
  return KMVP_OK;
}

template <typename real>
LowdCutoffArgs<real> cutoff_args(const kmvp_ctx* c, double radius) {
  LowdCutoffArgs<real> a;
  a.xs = (const real*)c->ct_xs.p;
  a.rec = (const real*)c->ct_rec.p;
  a.tiles = (const CutoffTile*)c->ct_tiles.p;
  a.runs = (const CutoffRun*)c->ct_runs.p;
  a.tmap = (const int64_t*)c->ct_tmap.p;
  a.out = nullptr;
  a.counts = nullptr;
  a.n_pad = c->ct_n_pad;
  a.r2 = (real)(radius * radius);
  a.chunk = (int)round_up(c->opt_chunk > 8 ? c->opt_chunk : 8, LOWD_BATCH);  // lowd_geometry's rule
  a.self_norm = 0;
  a.exclude_self = 0;
  a.iR2 = (real)(1.0 / (radius * radius));
  a.gconst = 0.0;
  a.smap32 = nullptr;
  a.knn_idx = nullptr;
  a.knn_sqdist = nullptr;
  a.knn_k = 0;
  a.knn_nan_rows = 0;
  return a;
}

inline hipError_t launch_cutoff(int kernel, int D, int E, int sig, const LowdCutoffArgs<float>& a, dim3 grid, hipStream_t s,
                                const char** name) {
  return is_wendland(kernel) ? launch_lowd_wendland_f32(kernel, D, E, sig, a, grid, s, name)
                             : launch_lowd_cutoff_f32(kernel, D, E, sig, a, grid, s, name);
}
inline hipError_t launch_cutoff(int kernel, int D, int E, int sig, const LowdCutoffArgs<double>& a, dim3 grid, hipStream_t s,
                                const char** name) {
  return is_wendland(kernel) ? launch_lowd_wendland_f64(kernel, D, E, sig, a, grid, s, name)
                             : launch_lowd_cutoff_f64(kernel, D, E, sig, a, grid, s, name);
}
inline hipError_t launch_cutoff_count(int D, const LowdCutoffArgs<float>& a, dim3 grid, hipStream_t s, const char** name) {
  return launch_lowd_cutoff_count_f32(D, a, grid, s, name);
}
inline hipError_t launch_cutoff_count(int D, const LowdCutoffArgs<double>& a, dim3 grid, hipStream_t s, const char** name) {
  return launch_lowd_cutoff_count_f64(D, a, grid, s, name);
}

template <typename real>
int run_cutoff_t(kmvp_ctx* c, int kernel, double radius, bool normalise) {
  const int D = c->D;
  const int sig = c->density ? SIG_DENSITY : (normalise ? SIG_NORM : SIG_PRODUCT);
  const int E = c->density ? 1 : c->E;
  const int EB = c->density ? 0 : E;
  const int R = (D + EB + 3) / 4 * 4;
  int rc;
  HIP_TRY(c, hipEventRecord(c->ev[0], c->stream));
  if ((rc = cutoff_prepare<real>(c, radius))) return rc;
  if ((rc = pack_cutoff<real>(c, R, EB))) return rc;
  if ((rc = ensure(c, c->out, (size_t)c->N * E * sizeof(double)))) return rc;
  LowdCutoffArgs<real> a = cutoff_args<real>(c, radius);
  a.out = (double*)c->out.p;
  a.self_norm = c->density && normalise;
  HIP_TRY(c, hipEventRecord(c->ev[3], c->stream));
  hipError_t le = launch_cutoff(kernel, D, E, sig, a, dim3((unsigned)(c->ct_n_pad / (CUTOFF_TILE * CUTOFF_WAVES))), c->stream,
                                &c->last_kernel_name);
  if (le == hipErrorInvalidValue) return fail(c, KMVP_E_UNSUPPORTED, "cutoff radius: no kernel instantiated for this (kernel, D, E)");
  HIP_TRY(c, le);
  HIP_TRY(c, hipEventRecord(c->ev[1], c->stream));
  HIP_TRY(c, hipEventRecord(c->ev[2], c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipEventElapsedTime(&c->last_kernel_ms, c->ev[3], c->ev[1]));
  HIP_TRY(c, hipEventElapsedTime(&c->last_total_ms, c->ev[0], c->ev[2]));
  c->out_n = c->N;
  c->out_e = E;
  return KMVP_OK;
}

inline hipError_t launch_cutoff_grad(int kernel, int D, int E, int sig, const LowdCutoffArgs<float>& a, dim3 grid, hipStream_t s,
                                     const char** name) {
  return is_wendland(kernel) ? launch_lowd_wendland_grad_f32(kernel, D, E, sig, a, grid, s, name)
                             : launch_lowd_cutoff_grad_f32(kernel, D, E, sig, a, grid, s, name);
}
inline hipError_t launch_cutoff_grad(int kernel, int D, int E, int sig, const LowdCutoffArgs<double>& a, dim3 grid, hipStream_t s,
                                     const char** name) {
  return is_wendland(kernel) ? launch_lowd_wendland_grad_f64(kernel, D, E, sig, a, grid, s, name)
                             : launch_lowd_cutoff_grad_f64(kernel, D, E, sig, a, grid, s, name);
}

// The gradient's constant c (kmvp_lowd_cutoff_grad.hpp), in double: grad_constant<KERNEL>()'s values for the four truncated
// kernels, Wendland's from the radius.
double cutoff_grad_constant(int kernel, double radius) {
  switch (kernel) {
    case K_GAUSSIAN: return -2.0;
    case K_MATERN32: return -3.0;
    case K_MATERN52: return -5.0 / 3.0;
    case K_WENDLAND_C2: return -20.0 / (radius * radius);
    case K_WENDLAND_C4: return -56.0 / (3.0 * (radius * radius));
    default: return -1.0;  // exp(-r)
  }
}

// run_cutoff_t with the product's record length, so that the two share plan and packs, and (N, E D) in c->out.
template <typename real>
int run_cutoff_grad_t(kmvp_ctx* c, int kernel, double radius) {
  const int D = c->D;
  const int sig = c->density ? SIG_DENSITY : SIG_PRODUCT;
  const int E = c->density ? 1 : c->E;
  const int EB = c->density ? 0 : E;
  const int R = (D + EB + 3) / 4 * 4;
  int rc;
  HIP_TRY(c, hipEventRecord(c->ev[0], c->stream));
  if ((rc = cutoff_prepare<real>(c, radius))) return rc;
  if ((rc = pack_cutoff<real>(c, R, EB))) return rc;
  if ((rc = ensure(c, c->out, (size_t)c->N * E * D * sizeof(double)))) return rc;
  LowdCutoffArgs<real> a = cutoff_args<real>(c, radius);
  a.out = (double*)c->out.p;
  a.gconst = cutoff_grad_constant(kernel, radius);
  HIP_TRY(c, hipEventRecord(c->ev[3], c->stream));
  hipError_t le = launch_cutoff_grad(kernel, D, E, sig, a, dim3((unsigned)(c->ct_n_pad / (CUTOFF_TILE * CUTOFF_WAVES))), c->stream,
                                     &c->last_kernel_name);
  if (le == hipErrorInvalidValue)
    return fail(c, KMVP_E_UNSUPPORTED, "cutoff gradient: no kernel instantiated for this (kernel, D, E)");
  HIP_TRY(c, le);
  HIP_TRY(c, hipEventRecord(c->ev[1], c->stream));
  HIP_TRY(c, hipEventRecord(c->ev[2], c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipEventElapsedTime(&c->last_kernel_ms, c->ev[3], c->ev[1]));
  HIP_TRY(c, hipEventElapsedTime(&c->last_total_ms, c->ev[0], c->ev[2]));
  c->out_n = c->N;
  c->out_e = E * D;
  return KMVP_OK;
}

template <typename real>
int radius_count_t(kmvp_ctx* c, double radius, int exclude_self, int64_t* counts) {
  const int D = c->D;
  const int R = (D + 3) / 4 * 4;  // density layout: no signal columns
  int rc;
  HIP_TRY(c, hipEventRecord(c->ev[0], c->stream));
  if ((rc = cutoff_prepare<real>(c, radius))) return rc;
  if ((rc = pack_cutoff<real>(c, R, 0))) return rc;
  // counts in c->knn: scratch of the context that no entry expects to survive a call
  if ((rc = ensure(c, c->knn, (size_t)c->N * sizeof(int64_t)))) return rc;
  LowdCutoffArgs<real> a = cutoff_args<real>(c, radius);
  a.counts = (int64_t*)c->knn.p;
  a.exclude_self = exclude_self != 0;
  HIP_TRY(c, hipEventRecord(c->ev[3], c->stream));
  hipError_t le = launch_cutoff_count(D, a, dim3((unsigned)(c->ct_n_pad / (CUTOFF_TILE * CUTOFF_WAVES))), c->stream, &c->last_kernel_name);
  if (le == hipErrorInvalidValue) return fail(c, KMVP_E_UNSUPPORTED, "cutoff radius: no count kernel instantiated for this D");
  HIP_TRY(c, le);
  HIP_TRY(c, hipEventRecord(c->ev[1], c->stream));
  HIP_TRY(c, hipMemcpyAsync(counts, c->knn.p, (size_t)c->N * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipEventRecord(c->ev[2], c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipEventElapsedTime(&c->last_kernel_ms, c->ev[3], c->ev[1]));
  HIP_TRY(c, hipEventElapsedTime(&c->last_total_ms, c->ev[0], c->ev[2]));
  return KMVP_OK;
}

// The plan's smap narrowed to int32 (every index is below 2^31: cutoff_plan_build refuses more sources), once per plan.
__global__ void cutoff_narrow_smap_kernel(const int64_t* __restrict__ smap, int32_t* __restrict__ smap32, int64_t m_alloc) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s < m_alloc) smap32[s] = (int32_t)smap[s];
}

int cutoff_smap32(kmvp_ctx* c) {
  if (c->ct_smap32_ver == c->ct_ver) return KMVP_OK;
  int rc;
  if ((rc = ensure(c, c->ct_smap32, (size_t)c->ct_m_alloc * sizeof(int32_t)))) return rc;
  hipLaunchKernelGGL(cutoff_narrow_smap_kernel, dim3(blocks_for(c->ct_m_alloc)), dim3(256), 0, c->stream,
                     (const int64_t*)c->ct_smap.p, (int32_t*)c->ct_smap32.p, c->ct_m_alloc);
  HIP_TRY(c, hipGetLastError());
  c->ct_smap32_ver = c->ct_ver;
  return KMVP_OK;
}

inline hipError_t launch_cutoff_knn(int D, int KT, const LowdCutoffArgs<float>& a, dim3 grid, hipStream_t s, const char** name) {
  return launch_lowd_cutoff_knn_f32(D, KT, a, grid, s, name);
}
inline hipError_t launch_cutoff_knn(int D, int KT, const LowdCutoffArgs<double>& a, dim3 grid, hipStream_t s, const char** name) {
  return launch_lowd_cutoff_knn_f64(D, KT, a, grid, s, name);
}

// radius_count_t with the lists: the count's plan, target image and density-layout records, and the index copy.
template <typename real>
int radius_nearest_t(kmvp_ctx* c, double radius, int K, int exclude_self, int64_t* out_idx, double* out_sqdist) {
  const int D = c->D;
  const int R = (D + 3) / 4 * 4;  // density layout: no signal columns
  int rc;
  HIP_TRY(c, hipEventRecord(c->ev[0], c->stream));
  if ((rc = cutoff_prepare<real>(c, radius))) return rc;
  if ((rc = pack_cutoff<real>(c, R, 0))) return rc;
  if ((rc = cutoff_smap32(c))) return rc;
  // the rows in c->knn, as kmvp_nearest: (N, K) int64 indices, then (N, K) float64 squared distances
  const size_t nk = (size_t)c->N * K;
  if ((rc = ensure(c, c->knn, nk * (sizeof(int64_t) + sizeof(double))))) return rc;
  LowdCutoffArgs<real> a = cutoff_args<real>(c, radius);
  a.exclude_self = exclude_self != 0;
  a.smap32 = (const int32_t*)c->ct_smap32.p;
  a.knn_idx = (int64_t*)c->knn.p;
  a.knn_sqdist = (double*)(a.knn_idx + nk);
  a.knn_k = K;
  a.knn_nan_rows = c->M > 0;
  HIP_TRY(c, hipEventRecord(c->ev[3], c->stream));
  hipError_t le = launch_cutoff_knn(D, knn_capacity(K + (exclude_self ? 1 : 0)), a, dim3((unsigned)(c->ct_n_pad / (CUTOFF_TILE * CUTOFF_WAVES))),
                                    c->stream, &c->last_kernel_name);
  if (le == hipErrorInvalidValue) return fail(c, KMVP_E_UNSUPPORTED, "radius search: no kernel instantiated for this (D, K)");
  HIP_TRY(c, le);
  HIP_TRY(c, hipEventRecord(c->ev[1], c->stream));
  HIP_TRY(c, hipMemcpyAsync(out_idx, a.knn_idx, nk * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(out_sqdist, a.knn_sqdist, nk * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipEventRecord(c->ev[2], c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipEventElapsedTime(&c->last_kernel_ms, c->ev[3], c->ev[1]));
  HIP_TRY(c, hipEventElapsedTime(&c->last_total_ms, c->ev[0], c->ev[2]));
  return KMVP_OK;
}

int radius_checked(kmvp_ctx* c, double radius) {
  if (!std::isfinite(radius) || !(radius > 0.0)) return fail(c, KMVP_E_INVALID, "cutoff radius: the radius must be finite and > 0");
  return KMVP_OK;
}

// The solver's signal: the EB signal slots of the records in the working precision straight from the float64 (M, EB) vector
// v through the plan's map, nothing else; pad records keep b = 0.  (cg_cast_kernel + batch_pack_signal_kernel in one.)
template <typename real>
__global__ void cutoff_signal_f64_kernel(const double* __restrict__ v, const int64_t* __restrict__ smap, real* __restrict__ rec,
                                         int64_t m_alloc, int D, int EB, int R) {
  const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= m_alloc) return;
  const int64_t j = smap[s];
  real* r = rec + s * R;
  for (int e = 0; e < EB; ++e) r[D + e] = j >= 0 ? (real)v[j * EB + e] : (real)0;
}

template <typename real>
int cutoff_apply_t(kmvp_ctx* c, int kernel, const double* v, int E) {
  const int D = c->D;
  const int R = (D + E + 3) / 4 * 4;
  const bool sync = !c->async_product;
  if (sync) HIP_TRY(c, hipEventRecord(c->ev[0], c->stream));
  hipLaunchKernelGGL((cutoff_signal_f64_kernel<real>), dim3(blocks_for(c->ct_m_alloc)), dim3(256), 0, c->stream, v,
                     (const int64_t*)c->ct_smap.p, (real*)c->ct_rec.p, c->ct_m_alloc, D, E, R);
  c->ct_sig_ver = 0;  // the signal slots hold a Krylov vector, no version of kmvp_set_signal's
  c->ct_sig_EB = 0;
  LowdCutoffArgs<real> a = cutoff_args<real>(c, c->ct_solve_radius);
  a.out = (double*)c->out.p;
  if (sync) HIP_TRY(c, hipEventRecord(c->ev[3], c->stream));
  hipError_t le = launch_cutoff(kernel, D, E, SIG_PRODUCT, a, dim3((unsigned)(c->ct_n_pad / (CUTOFF_TILE * CUTOFF_WAVES))), c->stream,
                                &c->last_kernel_name);
  if (le == hipErrorInvalidValue) return fail(c, KMVP_E_UNSUPPORTED, "cutoff radius: no kernel instantiated for this (kernel, D, E)");
  HIP_TRY(c, le);
  c->out_n = c->N;
  c->out_e = E;
  if (!sync) return KMVP_OK;
  HIP_TRY(c, hipEventRecord(c->ev[1], c->stream));
  HIP_TRY(c, hipEventRecord(c->ev[2], c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipEventElapsedTime(&c->last_kernel_ms, c->ev[3], c->ev[1]));
  HIP_TRY(c, hipEventElapsedTime(&c->last_total_ms, c->ev[0], c->ev[2]));
  return KMVP_OK;
}

// Everything an application needs that is not a launch: the plan, the target image, the coordinates of records laid out
// for E signal columns, and c->out.
template <typename real>
int cutoff_solve_prepare(kmvp_ctx* c, double radius, int E) {
  const int R = (c->D + E + 3) / 4 * 4;
  int rc;
  if ((rc = cutoff_prepare<real>(c, radius))) return rc;
  if ((rc = pack_cutoff<real>(c, R, 0))) return rc;
  if ((rc = ensure(c, c->out, std::max<size_t>((size_t)c->N * E * sizeof(double), 16)))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return KMVP_OK;
}

// cutoff_count_device for one precision: radius_count_t's setup and launch, the index copy, nothing read back.
template <typename real>
int cutoff_count_device_t(kmvp_ctx* c, double radius, int64_t* counts) {
  const int D = c->D;
  const int R = (D + 3) / 4 * 4;  // density layout: no signal columns
  int rc;
  if ((rc = cutoff_prepare<real>(c, radius))) return rc;
  if (c->N == 0) return KMVP_OK;
  if ((rc = pack_cutoff<real>(c, R, 0))) return rc;
  if ((rc = cutoff_smap32(c))) return rc;
  LowdCutoffArgs<real> a = cutoff_args<real>(c, radius);
  a.counts = counts;
  HIP_TRY(c, hipEventRecord(c->ev[3], c->stream));
  hipError_t le = launch_cutoff_count(D, a, dim3((unsigned)(c->ct_n_pad / (CUTOFF_TILE * CUTOFF_WAVES))), c->stream, &c->last_kernel_name);
  if (le == hipErrorInvalidValue) return fail(c, KMVP_E_UNSUPPORTED, "cutoff radius: no count kernel instantiated for this D");
  HIP_TRY(c, le);
  HIP_TRY(c, hipEventRecord(c->ev[1], c->stream));
  return KMVP_OK;
}

}  // namespace

int cutoff_refuse(kmvp_ctx* c, const std::string& what) { return cutoff_unsupported(c, what); }

int cutoff_count_device(kmvp_ctx* c, double radius, int64_t* counts) {
  return c->dtype == KMVP_F64 ? cutoff_count_device_t<double>(c, radius, counts) : cutoff_count_device_t<float>(c, radius, counts);
}

int run_cutoff(kmvp_ctx* c, int kernel, double radius, bool normalise) {
  if (!c) return KMVP_E_INVALID;
  c->note.clear();
  int rc;
  if ((rc = radius_checked(c, radius))) return rc;
  if (!c->have_points) return fail(c, KMVP_E_INVALID, "cutoff radius: kmvp_set_points has not been called");
  if (!c->have_signal) return fail(c, KMVP_E_INVALID, "cutoff radius: kmvp_set_signal has not been called");
  HIP_TRY(c, hipSetDevice(c->device));
  if ((rc = cutoff_unsupported(c, "product"))) return rc;
  const int E = c->density ? 1 : c->E;
  if (E > LOWD_MAX_E)
    return fail(c, KMVP_E_UNSUPPORTED, "product: E = " + std::to_string(E) + " signal columns are beyond the cutoff's kernels' E <= " +
                                           std::to_string(LOWD_MAX_E) + " (cutoff radius: run it per block of columns)");
  c->last_kernel_ms = c->last_total_ms = c->last_allreduce_ms = 0.f;
  if (c->N == 0) {
    if ((rc = c->dtype == KMVP_F64 ? cutoff_prepare<double>(c, radius) : cutoff_prepare<float>(c, radius))) return rc;
    if ((rc = ensure(c, c->out, 16))) return rc;
    c->out_n = 0;
    c->out_e = E;
    c->last_kernel_name = "none";
    return KMVP_OK;
  }
  return c->dtype == KMVP_F64 ? run_cutoff_t<double>(c, kernel, radius, normalise) : run_cutoff_t<float>(c, kernel, radius, normalise);
}

int run_cutoff_grad(kmvp_ctx* c, int kernel, double radius) {
  if (!c) return KMVP_E_INVALID;
  c->note.clear();
  int rc;
  if ((rc = radius_checked(c, radius))) return rc;
  if (!c->have_points) return fail(c, KMVP_E_INVALID, "cutoff gradient: kmvp_set_points has not been called");
  if (!c->have_signal) return fail(c, KMVP_E_INVALID, "cutoff gradient: kmvp_set_signal has not been called");
  HIP_TRY(c, hipSetDevice(c->device));
  if ((rc = cutoff_unsupported(c, "cutoff gradient"))) return rc;
  const int E = c->density ? 1 : c->E;
  if (E > LOWD_MAX_E)
    return fail(c, KMVP_E_UNSUPPORTED, "cutoff gradient: E = " + std::to_string(E) + " signal columns are beyond the cutoff's kernels' E <= " +
                                           std::to_string(LOWD_MAX_E) + " (cutoff radius: run it per block of columns)");
  c->last_kernel_ms = c->last_total_ms = c->last_allreduce_ms = 0.f;
  if (c->N == 0) {
    if ((rc = c->dtype == KMVP_F64 ? cutoff_prepare<double>(c, radius) : cutoff_prepare<float>(c, radius))) return rc;
    if ((rc = ensure(c, c->out, 16))) return rc;
    c->out_n = 0;
    c->out_e = E * c->D;
    c->last_kernel_name = "none";
    return KMVP_OK;
  }
  return c->dtype == KMVP_F64 ? run_cutoff_grad_t<double>(c, kernel, radius) : run_cutoff_grad_t<float>(c, kernel, radius);
}

int cutoff_apply(kmvp_ctx* c, int kernel, const double* v, int E) {
  if (!(c->ct_solve_radius > 0.0) || c->ct_plan_points_ver != c->points_ver)
    return fail(c, KMVP_E_INVALID, "cutoff radius: the operator of a Wendland solve was applied outside kmvp_wendland_<c>_cg_solve");
  if (c->N == 0) return KMVP_OK;
  return c->dtype == KMVP_F64 ? cutoff_apply_t<double>(c, kernel, v, E) : cutoff_apply_t<float>(c, kernel, v, E);
}

int wendland_cg_solve(kmvp_ctx* c, int kernel, double radius, const void* a_host, int E, double rtol, int maxit, double* out_b,
                      int* iters, double* resid) {
  if (!c) return KMVP_E_INVALID;
  c->note.clear();
  int rc;
  if (!c->have_points) return fail(c, KMVP_E_INVALID, "kmvp_set_points has not been called");
  if ((rc = radius_checked(c, radius))) return rc;
  if (!a_host || !out_b || E < 1 || maxit < 0 || !(rtol > 0)) return fail(c, KMVP_E_INVALID, "bad solver arguments");
  HIP_TRY(c, hipSetDevice(c->device));
  if ((rc = cutoff_unsupported(c, "solve"))) return rc;
  if (!c->same_points)
    return fail(c, KMVP_E_INVALID, "cutoff radius: the solver needs the targets to be the sources (x == NULL at kmvp_set_points)");
  if (E > LOWD_MAX_E)
    return fail(c, KMVP_E_UNSUPPORTED, "solve: E = " + std::to_string(E) + " right-hand sides are beyond the cutoff's kernels' E <= " +
                                           std::to_string(LOWD_MAX_E) + " (cutoff radius: solve per block of columns)");
  if (c->precond_rank > 0)
    return fail(c, KMVP_E_UNSUPPORTED, "solve: the preconditioner is not built for the Wendland kernels (its column kernel knows none); "
                                       "set rank 0 (cutoff radius: kmvp_wendland_<c>_cg_solve)");
  c->last_kernel_ms = c->last_total_ms = c->last_allreduce_ms = 0.f;
  // as cg_apply leaves the context for the other kernels: E columns, no density, the signal replaced
  c->density = false;
  c->E = E;
  ++c->signal_ver;
  if ((rc = c->dtype == KMVP_F64 ? cutoff_solve_prepare<double>(c, radius, E) : cutoff_solve_prepare<float>(c, radius, E))) return rc;
  c->ct_solve_radius = radius;
  rc = cg_solve(c, kernel, a_host, E, rtol, maxit, out_b, iters, resid);
  c->ct_solve_radius = 0.0;
  c->have_signal = false;  // (also where cg_solve returned before its own guard)
  return rc;
}

int radius_count(kmvp_ctx* c, double radius, int exclude_self, int64_t* counts) {
  if (!c) return KMVP_E_INVALID;
  c->note.clear();
  int rc;
  if ((rc = radius_checked(c, radius))) return rc;
  if (!c->have_points) return fail(c, KMVP_E_INVALID, "cutoff radius: kmvp_set_points has not been called");
  if (exclude_self && !c->same_points)
    return fail(c, KMVP_E_INVALID, "cutoff radius: exclude_self needs the targets to be the sources (x == NULL at kmvp_set_points)");
  if (c->N > 0 && !counts) return fail(c, KMVP_E_INVALID, "cutoff radius: a NULL output");
  HIP_TRY(c, hipSetDevice(c->device));
  if ((rc = cutoff_unsupported(c, "neighbour count"))) return rc;
  c->last_kernel_ms = c->last_total_ms = c->last_allreduce_ms = 0.f;
  if (c->N == 0) {
    if ((rc = c->dtype == KMVP_F64 ? cutoff_prepare<double>(c, radius) : cutoff_prepare<float>(c, radius))) return rc;
    c->last_kernel_name = "none";
    return KMVP_OK;
  }
  return c->dtype == KMVP_F64 ? radius_count_t<double>(c, radius, exclude_self, counts)
                              : radius_count_t<float>(c, radius, exclude_self, counts);
}

int radius_nearest(kmvp_ctx* c, double radius, int K, int exclude_self, int64_t* out_idx, double* out_sqdist) {
  if (!c) return KMVP_E_INVALID;
  c->note.clear();
  int rc;
  if ((rc = radius_checked(c, radius))) return rc;
  if (!c->have_points) return fail(c, KMVP_E_INVALID, "radius search: kmvp_set_points has not been called");
  if (K < 1) return fail(c, KMVP_E_INVALID, "radius search: K must be >= 1");
  if (exclude_self && !c->same_points)
    return fail(c, KMVP_E_INVALID, "radius search: exclude_self needs the targets to be the sources (x == NULL at kmvp_set_points)");
  if (c->N > 0 && (!out_idx || !out_sqdist)) return fail(c, KMVP_E_INVALID, "radius search: a NULL output");
  HIP_TRY(c, hipSetDevice(c->device));
  if ((rc = cutoff_unsupported(c, "radius search"))) return rc;
  if (K + (exclude_self ? 1 : 0) > KNN_MAX_K)
    return fail(c, KMVP_E_UNSUPPORTED, "radius search: K = " + std::to_string(K) + (exclude_self ? " with exclude_self" : "") +
                                           " is beyond the lists' K <= 16 (15 with exclude_self)");
  c->last_kernel_ms = c->last_total_ms = c->last_allreduce_ms = 0.f;
  if (c->N == 0) {
    if ((rc = c->dtype == KMVP_F64 ? cutoff_prepare<double>(c, radius) : cutoff_prepare<float>(c, radius))) return rc;
    c->last_kernel_name = "none";
    return KMVP_OK;
  }
  return c->dtype == KMVP_F64 ? radius_nearest_t<double>(c, radius, K, exclude_self, out_idx, out_sqdist)
                              : radius_nearest_t<float>(c, radius, K, exclude_self, out_idx, out_sqdist);
}

int cutoff_info(kmvp_ctx* c, int64_t* out) {
  if (!c) return KMVP_E_INVALID;
  if (!out) return fail(c, KMVP_E_INVALID, "cutoff radius: a NULL output");
  if (c->ct_ver == 0) return fail(c, KMVP_E_INVALID, "cutoff radius: no cutoff call has built a plan on this context");
  memcpy(out, c->ct_info, sizeof(c->ct_info));
  return KMVP_OK;
}

// Tiles and runs widened to rows of int64 on the host: the tables come back as the kernels read them, 16 bytes an entry.
int cutoff_plan_read(kmvp_ctx* c, int64_t* sizes, double* grid, int64_t* tiles, int64_t* runs, int64_t* tmap, int64_t* smap) {
  if (!c) return KMVP_E_INVALID;
  if (c->ct_ver == 0 || c->ct_plan_points_ver == 0)
    return fail(c, KMVP_E_INVALID, "cutoff radius: no cutoff call has built a plan on this context");
  const int64_t ntiles = c->ct_tiles_n, nruns = c->ct_info[4];
  if (sizes) {
    const int64_t v[13] = {c->ct_info[0], c->ct_info[1], c->ct_info[2], c->ct_n_pad, c->ct_info[6], c->ct_m_alloc, c->ct_info[3],
                           c->ct_info[5],  ntiles,        nruns,         c->ct_n_pad, c->ct_m_alloc, c->ct_built_on};
    memcpy(sizes, v, sizeof(v));
  }
  if (grid) memcpy(grid, c->ct_grid, sizeof(c->ct_grid));
  if (!tiles && !runs && !tmap && !smap) return KMVP_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  std::vector<CutoffTile> th(tiles ? (size_t)ntiles : 0);
  std::vector<CutoffRun> rh(runs ? (size_t)nruns : 0);
  if (!th.empty()) HIP_TRY(c, hipMemcpyAsync(th.data(), c->ct_tiles.p, th.size() * sizeof(CutoffTile), hipMemcpyDeviceToHost, c->stream));
  if (!rh.empty()) HIP_TRY(c, hipMemcpyAsync(rh.data(), c->ct_runs.p, rh.size() * sizeof(CutoffRun), hipMemcpyDeviceToHost, c->stream));
  if (tmap && c->ct_n_pad > 0)
    HIP_TRY(c, hipMemcpyAsync(tmap, c->ct_tmap.p, (size_t)c->ct_n_pad * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  if (smap && c->ct_m_alloc > 0)
    HIP_TRY(c, hipMemcpyAsync(smap, c->ct_smap.p, (size_t)c->ct_m_alloc * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (size_t t = 0; t < th.size(); ++t) {
    tiles[3 * t + 0] = th[t].run0;
    tiles[3 * t + 1] = th[t].nruns;
    tiles[3 * t + 2] = th[t].live;
  }
  for (size_t r = 0; r < rh.size(); ++r) {
    runs[2 * r + 0] = rh[r].rec0;
    runs[2 * r + 1] = rh[r].len;
  }
  return KMVP_OK;
}

}  // namespace kmvp
