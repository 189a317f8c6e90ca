// libkmvp.so -- the extern "C" surface declared in include/kmvp.h.
//
// Owns the per-GPU context (device buffers, stream, events, RCCL communicator); the
// compute paths live in kmvp_product.hip and kmvp_solvers.hip.  Reference call order this
// serves: runner.py:70-148 (prepare_data, fit, prepare_query, query, get_result) through the
// plugin in kernel_matrix_benchmarks_amd/algorithms/mi355x.py.
#include "kmvp_ctx.hpp"

namespace kmvp {

Rccl g_rccl;

namespace {
thread_local std::string g_create_error;
}

int fail(kmvp_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  else g_create_error = msg;
  return code;
}
const char* create_error() { return g_create_error.c_str(); }

int ensure(kmvp_ctx* c, DevBuf& b, size_t bytes) {
  if (bytes <= b.cap && b.p) return KMVP_OK;
  if (b.p) {
    HIP_TRY(c, hipFree(b.p));
    b.p = nullptr;
    b.cap = 0;
  }
  if (bytes == 0) bytes = 16;
  HIP_TRY(c, hipMalloc(&b.p, bytes));
  b.cap = bytes;
  return KMVP_OK;
}

void release(DevBuf& b) {
  if (b.p) (void)hipFree(b.p);
  b.p = nullptr;
  b.cap = 0;
}

}  // namespace kmvp

using namespace kmvp;

// =====================================================================================
extern "C" {

int kmvp_abi_version(void) { return KMVP_ABI_VERSION; }

int kmvp_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return -KMVP_E_DEVICE;
  return n;
}

kmvp_ctx* kmvp_create(int device, int* status) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    fail(nullptr, KMVP_E_DEVICE, std::string("no HIP device: ") + hipGetErrorString(e));
    if (status) *status = KMVP_E_DEVICE;
    return nullptr;
  }
  if (device < 0 || device >= n) {
    fail(nullptr, KMVP_E_INVALID, "device index out of range");
    if (status) *status = KMVP_E_INVALID;
    return nullptr;
  }
  kmvp_ctx* c = new kmvp_ctx();
  c->device = device;
  bool ok = hipSetDevice(device) == hipSuccess &&
            hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess;
  for (int i = 0; ok && i < 5; ++i) ok = hipEventCreate(&c->ev[i]) == hipSuccess;
  ok = ok && hipDeviceGetAttribute(&c->device_cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess;
  if (!ok) {
    fail(nullptr, KMVP_E_DEVICE, "cannot create stream/events on the device");
    if (status) *status = KMVP_E_DEVICE;
    kmvp_destroy(c);
    return nullptr;
  }
  if (status) *status = KMVP_OK;
  return c;
}

void kmvp_destroy(kmvp_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(c->comm);
  for (DevBuf* b : {&c->y_raw, &c->x_raw, &c->b_raw, &c->xs, &c->rec, &c->x_scaled, &c->y_scaled,
                    &c->part, &c->partd, &c->aux, &c->sortbuf, &c->perm, &c->sums, &c->out, &c->scratch, &c->sdiag, &c->precond, &c->knn, &c->xchg, &c->kexp, &c->kshift, &c->xchgk, &c->kflag,
                    &c->sk_xs_x, &c->sk_rec_y, &c->sk_xs_y, &c->sk_rec_x, &c->sk_state, &c->km_xs, &c->km_rec, &c->km_part, &c->km_state, &c->ms_xs, &c->ms_state, &c->ms_tmp, &c->bt_tiles, &c->bt_tmap, &c->bt_smap, &c->bt_xs, &c->bt_rec, &c->skb_plan, &c->skb_xs, &c->skb_rec, &c->skb_state, &c->ct_tiles, &c->ct_runs, &c->ct_tmap, &c->ct_smap, &c->ct_xs, &c->ct_rec, &c->ct_smap32, &c->ct_work, &c->db_state, &c->db_rec, &c->db_tmp,
                    &c->cell_tperm, &c->cell_sperm, &c->cell_tgrp, &c->cell_sgrp, &c->cell_slot, &c->cell_tmeta, &c->cell_sums, &c->cell_skey, &c->cell_scentre, &c->cell_scale, &c->cell_tcentre, &c->cell_scentre32})
    release(*b);
  for (int i = 0; i < 5; ++i)
    if (c->ev[i]) (void)hipEventDestroy(c->ev[i]);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

const char* kmvp_last_error(const kmvp_ctx* c) { return c ? c->err.c_str() : create_error(); }

int kmvp_set_points(kmvp_ctx* c, const void* y, int64_t M, const void* x_or_null, int64_t N, int D,
                    int dtype, int64_t j_offset, int64_t M_total) {
  if (!c) return KMVP_E_INVALID;
  if (dtype != KMVP_F32 && dtype != KMVP_F64 && dtype != KMVP_BF16)
    return fail(c, KMVP_E_INVALID, "unknown dtype");
  if (M < 0 || N < 0 || D < 1) return fail(c, KMVP_E_INVALID, "bad shape");
  if ((M > 0 && !y) || (N > 0 && !x_or_null && N != M))
    return fail(c, KMVP_E_INVALID, "same_points (x == NULL) needs N == M");
  if (M_total < M || j_offset < 0 || j_offset + M > M_total)
    return fail(c, KMVP_E_INVALID, "shard [j_offset, j_offset+M) is outside [0, M_total)");
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t es = elem_size(dtype);
  int rc;
  if ((rc = ensure(c, c->y_raw, (size_t)M * D * es))) return rc;
  if (M > 0) HIP_TRY(c, hipMemcpyAsync(c->y_raw.p, y, (size_t)M * D * es, hipMemcpyHostToDevice, c->stream));
  c->same_points = (x_or_null == nullptr);
  if (!c->same_points) {
    if ((rc = ensure(c, c->x_raw, (size_t)N * D * es))) return rc;
    if (N > 0) HIP_TRY(c, hipMemcpyAsync(c->x_raw.p, x_or_null, (size_t)N * D * es, hipMemcpyHostToDevice, c->stream));
  }
  if ((rc = measure_clouds(c, dtype, M, N, D))) return rc;  // bounding box for the split-bf16 path
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // host buffers are only read during the call
  c->dtype = dtype;
  c->D = D;
  c->M = M;
  c->N = N;
  c->j_offset = j_offset;
  c->m_total = M_total;
  c->have_points = true;
  c->have_signal = false;
  c->diag_on = false;  // the solver's diagonal belongs to the points it was set for
  c->diag_n = 0;
  c->diag_ridge = c->diag_min = 0.0;
  c->precond_rank = 0;  // and so does the preconditioner, built from them and from that diagonal
  c->pc_used = 0;
  c->bt_on = false;  // and so do the batches (kmvp_set_batches): offsets into the previous clouds
  c->bt_B = 0;
  ++c->points_ver;
  return KMVP_OK;
}

int kmvp_fit(kmvp_ctx* c, int kernel) {
  if (!c) return KMVP_E_INVALID;
  if (!c->have_points) return fail(c, KMVP_E_INVALID, "kmvp_set_points has not been called");
  // 7, 8: Wendland C2, C4 (5 and 6 stay refused, as before these kernels existed)
  if (kernel < 0 || kernel > 8 || kernel == 5 || kernel == 6) return fail(c, KMVP_E_INVALID, "kernel must be 0, 1, 2, 3, 4, 7 or 8");
  // Matern 3/2, 5/2: the difference form has nothing the points alone determine; Wendland C2, C4: the cutoff's plan needs
  // the radius as well
  if (kernel > 2) return KMVP_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  return prepare_points(c, kernel);
}

int kmvp_set_signal(kmvp_ctx* c, const void* b_or_null, int E) {
  if (!c) return KMVP_E_INVALID;
  if (!c->have_points) return fail(c, KMVP_E_INVALID, "kmvp_set_points must come first");
  if (E < 1) return fail(c, KMVP_E_INVALID, "E must be >= 1");
  if (!b_or_null && E != 1) return fail(c, KMVP_E_INVALID, "density estimation (b == NULL) needs E == 1");
  HIP_TRY(c, hipSetDevice(c->device));
  c->density = (b_or_null == nullptr);
  c->E = E;
  if (!c->density) {
    const size_t bytes = (size_t)c->M * E * elem_size(c->dtype);
    int rc = ensure(c, c->b_raw, bytes);
    if (rc) return rc;
    if (bytes) HIP_TRY(c, hipMemcpyAsync(c->b_raw.p, b_or_null, bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  c->have_signal = true;
  ++c->signal_ver;
  return KMVP_OK;
}

// Batched clouds (kmvp_set_batches; kmvp_batch.hip): the four products below and kmvp_nearest go to their block-diagonal
// forms while batches are set; every other compute entry is refused with a message that names them.
static inline bool batched(const kmvp_ctx* c) { return c && c->bt_on; }
#define KMVP_NOT_BATCHED(c, what)                   \
  do {                                              \
    if (int rc_ = batches_refuse((c), (what))) return rc_; \
  } while (0)

int kmvp_set_batches(kmvp_ctx* c, int B, const int64_t* y_offsets, const int64_t* x_offsets_or_null) {
  return set_batches(c, B, y_offsets, x_offsets_or_null);
}

int kmvp_gaussian(kmvp_ctx* c) { return batched(c) ? run_product_batched(c, K_GAUSSIAN, false) : run_product(c, K_GAUSSIAN, false); }
int kmvp_gaussian_norm(kmvp_ctx* c) { return batched(c) ? run_product_batched(c, K_GAUSSIAN, true) : run_product(c, K_GAUSSIAN, true); }
int kmvp_absexp(kmvp_ctx* c) { return batched(c) ? run_product_batched(c, K_ABSEXP, false) : run_product(c, K_ABSEXP, false); }
int kmvp_absexp_norm(kmvp_ctx* c) { return batched(c) ? run_product_batched(c, K_ABSEXP, true) : run_product(c, K_ABSEXP, true); }
int kmvp_invdist(kmvp_ctx* c) { KMVP_NOT_BATCHED(c, "the inverse-distance product"); return run_product(c, K_INVDIST, false); }
int kmvp_invdist_norm(kmvp_ctx* c) { KMVP_NOT_BATCHED(c, "the inverse-distance product"); return run_product(c, K_INVDIST, true); }
int kmvp_expdot(kmvp_ctx* c) { KMVP_NOT_BATCHED(c, "exp(<x,y>)"); return run_product(c, K_EXPDOT, false); }
int kmvp_expdot_norm(kmvp_ctx* c) { KMVP_NOT_BATCHED(c, "exp(<x,y>)"); return run_product(c, K_EXPDOT, true); }
int kmvp_matern32(kmvp_ctx* c) { return batched(c) ? run_product_batched(c, K_MATERN32, false) : run_product(c, K_MATERN32, false); }
int kmvp_matern32_norm(kmvp_ctx* c) { return batched(c) ? run_product_batched(c, K_MATERN32, true) : run_product(c, K_MATERN32, true); }
int kmvp_matern52(kmvp_ctx* c) { return batched(c) ? run_product_batched(c, K_MATERN52, false) : run_product(c, K_MATERN52, false); }
int kmvp_matern52_norm(kmvp_ctx* c) { return batched(c) ? run_product_batched(c, K_MATERN52, true) : run_product(c, K_MATERN52, true); }
int kmvp_gaussian_grad(kmvp_ctx* c) { KMVP_NOT_BATCHED(c, "the gradient"); return run_gradient(c, K_GAUSSIAN); }
int kmvp_absexp_grad(kmvp_ctx* c) { KMVP_NOT_BATCHED(c, "the gradient"); return run_gradient(c, K_ABSEXP); }
int kmvp_invdist_grad(kmvp_ctx* c) { KMVP_NOT_BATCHED(c, "the gradient"); return run_gradient(c, K_INVDIST); }
int kmvp_matern32_grad(kmvp_ctx* c) { KMVP_NOT_BATCHED(c, "the gradient"); return run_gradient(c, K_MATERN32); }
int kmvp_matern52_grad(kmvp_ctx* c) { KMVP_NOT_BATCHED(c, "the gradient"); return run_gradient(c, K_MATERN52); }
int kmvp_gaussian_dscale(kmvp_ctx* c) { KMVP_NOT_BATCHED(c, "the length-scale derivative"); return run_dscale(c, K_GAUSSIAN); }
int kmvp_absexp_dscale(kmvp_ctx* c) { KMVP_NOT_BATCHED(c, "the length-scale derivative"); return run_dscale(c, K_ABSEXP); }
int kmvp_matern32_dscale(kmvp_ctx* c) { KMVP_NOT_BATCHED(c, "the length-scale derivative"); return run_dscale(c, K_MATERN32); }
int kmvp_matern52_dscale(kmvp_ctx* c) { KMVP_NOT_BATCHED(c, "the length-scale derivative"); return run_dscale(c, K_MATERN52); }
int kmvp_gaussian_logsumexp(kmvp_ctx* c) { KMVP_NOT_BATCHED(c, "the log-sum-exp"); return run_logsumexp(c, K_GAUSSIAN); }
int kmvp_absexp_logsumexp(kmvp_ctx* c) { KMVP_NOT_BATCHED(c, "the log-sum-exp"); return run_logsumexp(c, K_ABSEXP); }
int kmvp_gaussian_logsumexp_grad(kmvp_ctx* c) { KMVP_NOT_BATCHED(c, "the gradient of the log-sum-exp"); return run_logsumexp_grad(c, K_GAUSSIAN); }
int kmvp_absexp_logsumexp_grad(kmvp_ctx* c) { KMVP_NOT_BATCHED(c, "the gradient of the log-sum-exp"); return run_logsumexp_grad(c, K_ABSEXP); }
int kmvp_nearest(kmvp_ctx* c, int K, int exclude_self, int64_t* out_idx, double* out_sqdist) {
  if (batched(c)) return run_nearest_batched(c, K, exclude_self, out_idx, out_sqdist);
  return run_nearest(c, K, exclude_self, out_idx, out_sqdist);
}
int kmvp_gaussian_cutoff(kmvp_ctx* c, double radius, int normalise) { return run_cutoff(c, K_GAUSSIAN, radius, normalise != 0); }
int kmvp_absexp_cutoff(kmvp_ctx* c, double radius, int normalise) { return run_cutoff(c, K_ABSEXP, radius, normalise != 0); }
int kmvp_matern32_cutoff(kmvp_ctx* c, double radius, int normalise) { return run_cutoff(c, K_MATERN32, radius, normalise != 0); }
int kmvp_matern52_cutoff(kmvp_ctx* c, double radius, int normalise) { return run_cutoff(c, K_MATERN52, radius, normalise != 0); }
int kmvp_wendland_c2_cutoff(kmvp_ctx* c, double radius, int normalise) { return run_cutoff(c, K_WENDLAND_C2, radius, normalise != 0); }
int kmvp_wendland_c4_cutoff(kmvp_ctx* c, double radius, int normalise) { return run_cutoff(c, K_WENDLAND_C4, radius, normalise != 0); }
int kmvp_gaussian_cutoff_grad(kmvp_ctx* c, double radius) { return run_cutoff_grad(c, K_GAUSSIAN, radius); }
int kmvp_absexp_cutoff_grad(kmvp_ctx* c, double radius) { return run_cutoff_grad(c, K_ABSEXP, radius); }
int kmvp_matern32_cutoff_grad(kmvp_ctx* c, double radius) { return run_cutoff_grad(c, K_MATERN32, radius); }
int kmvp_matern52_cutoff_grad(kmvp_ctx* c, double radius) { return run_cutoff_grad(c, K_MATERN52, radius); }
int kmvp_wendland_c2_cutoff_grad(kmvp_ctx* c, double radius) { return run_cutoff_grad(c, K_WENDLAND_C2, radius); }
int kmvp_wendland_c4_cutoff_grad(kmvp_ctx* c, double radius) { return run_cutoff_grad(c, K_WENDLAND_C4, radius); }
int kmvp_radius_count(kmvp_ctx* c, double radius, int exclude_self, int64_t* counts) { return radius_count(c, radius, exclude_self, counts); }
int kmvp_radius_nearest(kmvp_ctx* c, double radius, int K, int exclude_self, int64_t* out_idx, double* out_sqdist) {
  return radius_nearest(c, radius, K, exclude_self, out_idx, out_sqdist);
}
int kmvp_dbscan(kmvp_ctx* c, double radius, int64_t min_samples, int64_t* labels, int64_t* core_of_or_null, int64_t* counts_or_null,
                int64_t* info) {
  return dbscan_solve(c, radius, min_samples, labels, core_of_or_null, counts_or_null, info);
}
int kmvp_cutoff_info(kmvp_ctx* c, int64_t* out) { return cutoff_info(c, out); }
int kmvp_cutoff_plan_read(kmvp_ctx* c, int64_t* sizes, double* grid, int64_t* tiles, int64_t* runs, int64_t* tmap, int64_t* smap) {
  return cutoff_plan_read(c, sizes, grid, tiles, runs, tmap, smap);
}
int kmvp_kmeans(kmvp_ctx* c, int C, const double* weights, double tol, int maxit, double* centroids, int64_t* labels,
                double* cluster_weight, int* iters, double* inertia, double* shift) {
  KMVP_NOT_BATCHED(c, "k-means");
  return kmeans_solve(c, C, weights, tol, maxit, centroids, labels, cluster_weight, iters, inertia, shift);
}
int kmvp_gaussian_meanshift(kmvp_ctx* c, double tol, int maxit, double* modes, int* iters, double* step2, int* sweeps,
                            int64_t* target_sweeps) {
  KMVP_NOT_BATCHED(c, "mean-shift");
  return meanshift_solve(c, tol, maxit, modes, iters, step2, sweeps, target_sweeps);
}

int kmvp_get_result(kmvp_ctx* c, double* out, int64_t out_len) {
  if (!c) return KMVP_E_INVALID;
  const int64_t n = c->out_n * c->out_e;
  if (!c->out.p && n > 0) return fail(c, KMVP_E_INVALID, "no result: run a product first");
  if (out_len < n || (n > 0 && !out)) return fail(c, KMVP_E_INVALID, "output buffer too small");
  HIP_TRY(c, hipSetDevice(c->device));
  if (n > 0) {
    HIP_TRY(c, hipMemcpyAsync(out, c->out.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  return KMVP_OK;
}

int kmvp_gaussian_cg_solve(kmvp_ctx* c, const void* a, int E, double rtol, int maxit, double* out_b,
                           int* iters, double* resid) {
  KMVP_NOT_BATCHED(c, "the solver");
  return cg_solve(c, K_GAUSSIAN, a, E, rtol, maxit, out_b, iters, resid);
}
int kmvp_absexp_cg_solve(kmvp_ctx* c, const void* a, int E, double rtol, int maxit, double* out_b,
                         int* iters, double* resid) {
  KMVP_NOT_BATCHED(c, "the solver");
  return cg_solve(c, K_ABSEXP, a, E, rtol, maxit, out_b, iters, resid);
}
int kmvp_matern32_cg_solve(kmvp_ctx* c, const void* a, int E, double rtol, int maxit, double* out_b,
                           int* iters, double* resid) {
  KMVP_NOT_BATCHED(c, "the solver");
  return cg_solve(c, K_MATERN32, a, E, rtol, maxit, out_b, iters, resid);
}
int kmvp_matern52_cg_solve(kmvp_ctx* c, const void* a, int E, double rtol, int maxit, double* out_b,
                           int* iters, double* resid) {
  KMVP_NOT_BATCHED(c, "the solver");
  return cg_solve(c, K_MATERN52, a, E, rtol, maxit, out_b, iters, resid);
}

int kmvp_wendland_c2_cg_solve(kmvp_ctx* c, double radius, const void* a, int E, double rtol, int maxit, double* out_b, int* iters,
                              double* resid) {
  return wendland_cg_solve(c, K_WENDLAND_C2, radius, a, E, rtol, maxit, out_b, iters, resid);
}
int kmvp_wendland_c4_cg_solve(kmvp_ctx* c, double radius, const void* a, int E, double rtol, int maxit, double* out_b, int* iters,
                              double* resid) {
  return wendland_cg_solve(c, K_WENDLAND_C4, radius, a, E, rtol, maxit, out_b, iters, resid);
}

int kmvp_invdist_minres_solve(kmvp_ctx* c, const void* a, int E, double rtol, int maxit, double* out_b,
                              int* iters, double* resid) {
  KMVP_NOT_BATCHED(c, "the solver");
  if (c && c->precond_rank > 0)
    return fail(c, KMVP_E_UNSUPPORTED, "preconditioner: MINRES has none (the inverse-distance matrix is indefinite); set rank 0");
  return minres_solve(c, K_INVDIST, a, E, rtol, maxit, out_b, iters, resid);
}

int kmvp_gaussian_lanczos_quadrature(kmvp_ctx* c, const void* z, int P, double rtol, int maxit, double* logquad,
                                     double* invquad, int* steps, double* x, double* alpha, double* beta) {
  KMVP_NOT_BATCHED(c, "the Lanczos quadrature");
  return cg_lanczos(c, K_GAUSSIAN, z, P, rtol, maxit, logquad, invquad, steps, x, alpha, beta);
}
int kmvp_absexp_lanczos_quadrature(kmvp_ctx* c, const void* z, int P, double rtol, int maxit, double* logquad,
                                   double* invquad, int* steps, double* x, double* alpha, double* beta) {
  KMVP_NOT_BATCHED(c, "the Lanczos quadrature");
  return cg_lanczos(c, K_ABSEXP, z, P, rtol, maxit, logquad, invquad, steps, x, alpha, beta);
}
int kmvp_matern32_lanczos_quadrature(kmvp_ctx* c, const void* z, int P, double rtol, int maxit, double* logquad,
                                     double* invquad, int* steps, double* x, double* alpha, double* beta) {
  KMVP_NOT_BATCHED(c, "the Lanczos quadrature");
  return cg_lanczos(c, K_MATERN32, z, P, rtol, maxit, logquad, invquad, steps, x, alpha, beta);
}
int kmvp_matern52_lanczos_quadrature(kmvp_ctx* c, const void* z, int P, double rtol, int maxit, double* logquad,
                                     double* invquad, int* steps, double* x, double* alpha, double* beta) {
  KMVP_NOT_BATCHED(c, "the Lanczos quadrature");
  return cg_lanczos(c, K_MATERN52, z, P, rtol, maxit, logquad, invquad, steps, x, alpha, beta);
}

#define KMVP_EIGSH_ENTRY(NAME, K)                                                                                          \
  int kmvp_##NAME##_eigsh(kmvp_ctx* c, int k, int op, const double* v0, double tol, int maxit, double* eigenvalues,        \
                          double* eigenvectors, double* resid, int* steps, double* alpha, double* beta, double* degree) { \
    KMVP_NOT_BATCHED(c, "the eigen-solver");                                                                              \
    return eigsh_solve(c, K, k, op, v0, tol, maxit, eigenvalues, eigenvectors, resid, steps, alpha, beta, degree);        \
  }
KMVP_EIGSH_ENTRY(gaussian, K_GAUSSIAN)
KMVP_EIGSH_ENTRY(absexp, K_ABSEXP)
KMVP_EIGSH_ENTRY(matern32, K_MATERN32)
KMVP_EIGSH_ENTRY(matern52, K_MATERN52)

#define KMVP_LANCZOS_PRECOND_ENTRY(NAME, K)                                                                                 \
  int kmvp_##NAME##_lanczos_quadrature_precond(kmvp_ctx* c, const double* g, const double* h, int P, double rtol, int maxit,  \
                                               double* logdet_p, double* logquad, double* invquad, double* wnorm2,           \
                                               int* steps, double* x, double* pz, double* alpha, double* beta) {             \
    KMVP_NOT_BATCHED(c, "the Lanczos quadrature");                                                                          \
    return cg_lanczos_precond(c, K, g, h, P, rtol, maxit, logdet_p, logquad, invquad, wnorm2, steps, x, pz, alpha, beta);    \
  }
KMVP_LANCZOS_PRECOND_ENTRY(gaussian, K_GAUSSIAN)
KMVP_LANCZOS_PRECOND_ENTRY(absexp, K_ABSEXP)
KMVP_LANCZOS_PRECOND_ENTRY(matern32, K_MATERN32)
KMVP_LANCZOS_PRECOND_ENTRY(matern52, K_MATERN52)
#undef KMVP_LANCZOS_PRECOND_ENTRY

int kmvp_gaussian_sinkhorn(kmvp_ctx* c, const double* log_a, const double* log_b, double tol, int maxit, double* u, double* v,
                           int* iters, double* err) {
  KMVP_NOT_BATCHED(c, "the Sinkhorn iteration");
  return sinkhorn_solve(c, K_GAUSSIAN, log_a, log_b, tol, maxit, u, v, iters, err);
}
int kmvp_absexp_sinkhorn(kmvp_ctx* c, const double* log_a, const double* log_b, double tol, int maxit, double* u, double* v,
                         int* iters, double* err) {
  KMVP_NOT_BATCHED(c, "the Sinkhorn iteration");
  return sinkhorn_solve(c, K_ABSEXP, log_a, log_b, tol, maxit, u, v, iters, err);
}

// (not refused while batches are set: these entries are the batches' own Sinkhorn; kmvp_sinkhorn_batched.hip)
int kmvp_gaussian_sinkhorn_batched(kmvp_ctx* c, const double* log_a, const double* log_b, double tol, int maxit, double* u,
                                   double* v, int* iters, double* err, int* status) {
  return sinkhorn_batched_solve(c, K_GAUSSIAN, log_a, log_b, tol, maxit, u, v, iters, err, status);
}
int kmvp_absexp_sinkhorn_batched(kmvp_ctx* c, const double* log_a, const double* log_b, double tol, int maxit, double* u,
                                 double* v, int* iters, double* err, int* status) {
  return sinkhorn_batched_solve(c, K_ABSEXP, log_a, log_b, tol, maxit, u, v, iters, err, status);
}

int kmvp_set_solver_diagonal(kmvp_ctx* c, const double* d, int64_t n, double ridge) {
  if (!c) return KMVP_E_INVALID;
  if (!std::isfinite(ridge)) return fail(c, KMVP_E_INVALID, "solver diagonal: ridge is not finite");
  if (n < 0 || (d == nullptr) != (n == 0)) return fail(c, KMVP_E_INVALID, "solver diagonal: pass n values, or NULL and n = 0");
  ++c->diag_ver;  // a preconditioner built with the previous diagonal is rebuilt
  if (!d) {
    c->diag_on = ridge != 0.0;
    c->diag_n = 0;
    c->diag_ridge = c->diag_min = ridge;
    return KMVP_OK;
  }
  // what the kernels read is ridge + d_i, formed once here (every rank forms the same values)
  std::vector<double> eff((size_t)n);
  double lo = INFINITY;
  for (int64_t i = 0; i < n; ++i) {
    eff[i] = ridge + d[i];
    if (!std::isfinite(eff[i])) return fail(c, KMVP_E_INVALID, "solver diagonal: d[" + std::to_string(i) + "] is not finite");
    lo = std::min(lo, eff[i]);
  }
  HIP_TRY(c, hipSetDevice(c->device));
  if (int rc = ensure(c, c->sdiag, sizeof(double) * (size_t)n)) return rc;
  c->diag_on = false;  // (a failed upload leaves no half-written diagonal behind)
  HIP_TRY(c, hipMemcpyAsync(c->sdiag.p, eff.data(), sizeof(double) * (size_t)n, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->diag_on = true;
  c->diag_n = n;
  c->diag_ridge = ridge;
  c->diag_min = lo;
  return KMVP_OK;
}

int kmvp_set_solver_preconditioner(kmvp_ctx* c, int rank) {
  if (!c) return KMVP_E_INVALID;
  if (rank < 0) return fail(c, KMVP_E_INVALID, "preconditioner: rank must be >= 0");
  if (rank > KMVP_PRECOND_MAX_RANK)
    return fail(c, KMVP_E_UNSUPPORTED, "preconditioner: rank " + std::to_string(rank) + " is beyond " + std::to_string(KMVP_PRECOND_MAX_RANK));
  c->precond_rank = rank;
  return KMVP_OK;
}
int kmvp_get_solver_preconditioner(kmvp_ctx* c, int* rank_built, int64_t* pivots, double* factor) {
  return precond_read(c, rank_built, pivots, factor);
}
double kmvp_last_preconditioner_ms(const kmvp_ctx* c) { return c ? c->last_precond_ms : 0.0; }

int kmvp_comm_get_unique_id(void* id128) {
  if (!id128) return KMVP_E_INVALID;
  if (!g_rccl.load()) return fail(nullptr, KMVP_E_COMM, g_rccl.error);
  static_assert(sizeof(ncclUniqueId) == KMVP_UNIQUE_ID_BYTES, "ncclUniqueId size");
  ncclUniqueId id;
  ncclResult_t r = g_rccl.GetUniqueId(&id);
  if (r != ncclSuccess) return fail(nullptr, KMVP_E_COMM, std::string("ncclGetUniqueId: ") + g_rccl.GetErrorString(r));
  memcpy(id128, &id, sizeof(id));
  return KMVP_OK;
}

int kmvp_comm_init(kmvp_ctx* c, const void* id128, int rank, int world) {
  if (!c || !id128 || world < 1 || rank < 0 || rank >= world) return fail(c, KMVP_E_INVALID, "bad communicator arguments");
  if (!g_rccl.load()) return fail(c, KMVP_E_COMM, g_rccl.error);
  HIP_TRY(c, hipSetDevice(c->device));
  if (c->comm) {
    g_rccl.CommDestroy(c->comm);
    c->comm = nullptr;
  }
  c->host_xchg = nullptr;
  c->host_user = nullptr;
  ncclUniqueId id;
  memcpy(&id, id128, sizeof(id));
  ncclResult_t r = g_rccl.CommInitRank(&c->comm, world, id, rank);
  if (r != ncclSuccess) {
    c->comm = nullptr;
    return fail(c, KMVP_E_COMM, std::string("ncclCommInitRank: ") + g_rccl.GetErrorString(r));
  }
  // what RCCL itself believes: a communicator whose size or rank differs from what the caller asked
  // for would hand back partial sums as results (or hang in the first all-reduce)
  int count = -1, user_rank = -1, dev = -1;
  ncclResult_t r1 = g_rccl.CommCount(c->comm, &count);
  ncclResult_t r2 = g_rccl.CommUserRank(c->comm, &user_rank);
  (void)g_rccl.CommCuDevice(c->comm, &dev);  // reported in the message only
  if (r1 != ncclSuccess || r2 != ncclSuccess || count != world || user_rank != rank) {
    g_rccl.CommDestroy(c->comm);
    c->comm = nullptr;
    c->comm_count = 1;
    c->rank = 0;
    c->world = 1;
    return fail(c, KMVP_E_COMM, "RCCL communicator mismatch: asked for rank " + std::to_string(rank) + " of " +
                                    std::to_string(world) + " on device " + std::to_string(c->device) + ", RCCL reports rank " +
                                    std::to_string(user_rank) + " of " + std::to_string(count) + " on device " +
                                    std::to_string(dev));
  }
  c->comm_count = count;
  c->rank = rank;
  c->world = world;
  return KMVP_OK;
}

int kmvp_comm_init_host(kmvp_ctx* c, kmvp_host_allreduce_fn fn, void* user, int rank, int world) {
  if (!c || !fn || world < 1 || rank < 0 || rank >= world) return fail(c, KMVP_E_INVALID, "bad communicator arguments");
  if (c->comm) {
    g_rccl.CommDestroy(c->comm);
    c->comm = nullptr;
  }
  c->host_xchg = fn;
  c->host_user = user;
  c->comm_count = world;
  c->rank = rank;
  c->world = world;
  return KMVP_OK;
}

int kmvp_comm_world(const kmvp_ctx* c) { return (c && c->exchanges()) ? c->comm_count : 1; }
int kmvp_comm_rank(const kmvp_ctx* c) { return (c && c->exchanges()) ? c->rank : 0; }

int kmvp_set_option(kmvp_ctx* c, const char* key, int64_t value) {
  if (!c || !key) return KMVP_E_INVALID;
  const std::string k(key);
  if (k == "feed") {
    if (value < -1 || value > 1) return fail(c, KMVP_E_INVALID, "feed must be -1 (auto), 0 or 1");
    c->opt_feed = (int)value;
  } else if (k == "targets_per_lane") {
    if (value != 0 && value != 1 && value != 2 && value != 4 && value != 8)
      return fail(c, KMVP_E_INVALID, "targets_per_lane must be 0 (auto), 1, 2, 4 or 8");
    c->opt_T = (int)value;
  } else if (k == "segments") {
    if (value < 0 || value > 65535) return fail(c, KMVP_E_INVALID, "segments out of range");
    c->opt_segments = (int)value;
  } else if (k == "fast_sqdists") {
    if (value < -1 || value > 4) return fail(c, KMVP_E_INVALID, "fast_sqdists must be -1 (auto), 0, 1, 2, 3 or 4");
    c->opt_fast = (int)value;
  } else if (k == "cellmm_shape") {
    if (value < -1 || value > 1) return fail(c, KMVP_E_INVALID, "cellmm_shape must be -1 (by size), 0 (32x32x16) or 1 (16x16x32)");
    c->opt_cellmm_shape = (int)value;
  } else if (k == "cell_fused") {
    if (value < -1 || value > 1) return fail(c, KMVP_E_INVALID, "cell_fused must be -1 (automatic), 0 (two launches) or 1 (one launch where it applies)");
    c->opt_cell_fused = (int)value;
  } else if (k == "cell_balance") {
    if (value < -1 || value > 1) return fail(c, KMVP_E_INVALID, "cell_balance must be -1 (automatic), 0 (never) or 1 (wherever count-cut cells apply)");
    c->opt_cell_balance = (int)value;
  } else if (k == "cell_tail") {
    if (value < -1 || value > 1) return fail(c, KMVP_E_INVALID, "cell_tail must be -1 (automatic), 0 (never) or 1 (wherever the fused grid has a partial last round)");
    c->opt_cell_tail = (int)value;
  } else if (k == "cell_tail_resident") {
    if (value < 0 || value > 65536) return fail(c, KMVP_E_INVALID, "cell_tail_resident must be 0 (the device's: two workgroups per compute unit) or a number of workgroups up to 65536");
    c->opt_cell_tail_resident = (int)value;
  } else if (k == "cell_shared_build") {
    if (value < -1 || value > 1) return fail(c, KMVP_E_INVALID, "cell_shared_build must be -1 (automatic), 0 (never) or 1 (wherever a workgroup is one-cell)");
    c->opt_cell_shared_build = (int)value;
  } else if (k == "mfma_variant") {
    if (value != -1 && value != 0 && value != 1 && value != 4 && value != 5)
      return fail(c, KMVP_E_INVALID, "mfma_variant must be -1 (by kernel), 0, 1, 4 or 5");
    c->opt_mfma_variant = (int)value;
  } else if (k == "same_points_global") {
    c->opt_same_global = value != 0;
  } else if (k == "partial_shard") {
    c->opt_partial = value != 0;
  } else if (k == "fast_tiles") {
    if (value != 0 && value != 1 && value != 2 && value != 4 && value != 8)
      return fail(c, KMVP_E_INVALID, "fast_tiles must be 0 (auto), 1, 2, 4 or 8");
    c->opt_fast_tiles = (int)value;
  } else if (k == "meanshift_compact") {
    if (value < -1 || value > 1) return fail(c, KMVP_E_INVALID, "meanshift_compact must be -1 (default), 0 or 1");
    c->opt_meanshift_compact = (int)value;
  } else if (k == "sinkhorn_retire") {
    if (value < -1 || value > 1) return fail(c, KMVP_E_INVALID, "sinkhorn_retire must be -1 (default), 0 or 1");
    c->opt_sinkhorn_retire = (int)value;
  } else if (k == "cutoff_plan") {
    if (value != 0 && value != 1) return fail(c, KMVP_E_INVALID, "cutoff_plan must be 0 (the plan is built on the host) or 1 (on the device)");
    c->opt_cutoff_plan = (int)value;
  } else if (k == "chunk") {
    if (value < 8 || value > (1 << 24)) return fail(c, KMVP_E_INVALID, "chunk out of range");
    c->opt_chunk = (int)value;
  } else {
    return fail(c, KMVP_E_INVALID, "unknown option " + k);
  }
  return KMVP_OK;
}

int kmvp_set_option_double(kmvp_ctx* c, const char* key, double value) {
  if (!c || !key) return KMVP_E_INVALID;
  const std::string k(key);
  if (k == "cutoff_cell_factor") {
    if (!(value >= 1.0) || !std::isfinite(value)) return fail(c, KMVP_E_INVALID, "cutoff_cell_factor must be a finite number >= 1");
    c->opt_cutoff_factor = value;
  } else {
    return fail(c, KMVP_E_INVALID, "unknown real-valued option " + k);
  }
  return KMVP_OK;
}

int64_t kmvp_device_bytes(const kmvp_ctx* c) {
  if (!c) return 0;
  size_t t = 0;
  for (const DevBuf* b : {&c->y_raw, &c->x_raw, &c->b_raw, &c->xs, &c->rec, &c->x_scaled,
                          &c->y_scaled, &c->part, &c->partd, &c->aux, &c->sortbuf, &c->perm, &c->sums, &c->out, &c->scratch, &c->sdiag, &c->precond, &c->knn, &c->xchg, &c->kexp, &c->kshift, &c->xchgk, &c->kflag,
                    &c->sk_xs_x, &c->sk_rec_y, &c->sk_xs_y, &c->sk_rec_x, &c->sk_state, &c->km_xs, &c->km_rec, &c->km_part, &c->km_state, &c->ms_xs, &c->ms_state, &c->ms_tmp, &c->bt_tiles, &c->bt_tmap, &c->bt_smap, &c->bt_xs, &c->bt_rec, &c->skb_plan, &c->skb_xs, &c->skb_rec, &c->skb_state, &c->ct_tiles, &c->ct_runs, &c->ct_tmap, &c->ct_smap, &c->ct_xs, &c->ct_rec, &c->ct_smap32, &c->ct_work, &c->db_state, &c->db_rec, &c->db_tmp,
                          &c->cell_tperm, &c->cell_sperm, &c->cell_tgrp, &c->cell_sgrp, &c->cell_slot, &c->cell_tmeta, &c->cell_sums, &c->cell_skey, &c->cell_scentre, &c->cell_scale, &c->cell_tcentre, &c->cell_scentre32})
    t += b->cap;
  return (int64_t)t;
}
double kmvp_last_kernel_ms(const kmvp_ctx* c) { return c ? c->last_kernel_ms : 0.0; }
double kmvp_last_total_ms(const kmvp_ctx* c) { return c ? c->last_total_ms : 0.0; }
double kmvp_last_allreduce_ms(const kmvp_ctx* c) { return c ? c->last_allreduce_ms : 0.0; }
int kmvp_cell_layout(kmvp_ctx* c, int64_t* info, double* sigma_b, int32_t* source_cell, int32_t* target_cell,
                     double* source_centres, int64_t source_cap, double* target_centres, int64_t target_cap) {
  if (!c) return KMVP_E_INVALID;
  return cell_layout_read(c, info, sigma_b, source_cell, target_cell, source_centres, source_cap, target_centres, target_cap);
}

int kmvp_cell_lists(kmvp_ctx* c, int64_t* info, int32_t* target_list) {
  if (!c) return KMVP_E_INVALID;
  return cell_lists_read(c, info, target_list);
}
const char* kmvp_last_kernel_name(const kmvp_ctx* c) { return c ? c->last_kernel_name : ""; }
const char* kmvp_last_dispatch_note(const kmvp_ctx* c) { return c ? c->note.c_str() : ""; }

}  // extern "C"
