// Lloyd's k-means on the arg-K-min at K = 1 (include/kmvp.h kmvp_kmeans): what kmvp_solvers.hip is to the product and
// kmvp_sinkhorn.hip to the log-sum-exp.  The pair loop is lowd_knn_kernel<D, 1>, untouched, with its segment merge; this
// file is the iteration around it.
//
// The points are the context's targets.  Their target image is packed once per kmvp_set_points into a buffer of the
// solver's own, the C centroid records (density layout of the difference form, R = 4 ceil(D / 4), pad records at +inf)
// into another: the product's xs / rec and their PackKey bookkeeping are never touched.  Centroids, sums, weights and
// labels stay fp64 / int64 on the device.
//
// One iteration k, six launches, no atomics:
//   km_records_kernel    the C records from the fp64 centroids c_{k-1}, rounded to the working precision
//   lowd_knn_kernel<D,1> (s_i, l_k(i)) per (segment, point)
//   knn_merge_kernel     the segments: cand[2][N], squared distances then labels, both as doubles
//   km_update_kernel     the new hot path.  A grid that depends on (N, C, D) only; workgroup g owns the contiguous run of
//                        points [g run, (g + 1) run).  It stages 256 points at a time in LDS (label; w x_d, w and w s as
//                        doubles, written by the thread that loaded the point) and then WALKS the 256 labels in index
//                        order, sixteen per round of broadcast reads: every thread owns the clusters of one residue modulo 256
//                        (km_owner_key), whose accumulators [D + 2][clusters of the pass] sit in LDS, and under a
//                        wave-uniform __any(owner) only the owning lane adds the point into its own accumulators.  One
//                        compare per point per thread whatever C is;
//                        no two threads ever touch the same accumulator, and every accumulator sees its points in index
//                        order.  Where C (D + 2) 8 B exceeds the LDS of a workgroup the clusters are taken in passes over
//                        ranges of CP, each pass rescanning the run.  Partials: part[g][D + 2][C].
//   km_reduce_kernel     tot[D + 2][C]: the partials in a fixed order that depends on the grid alone
//   km_scalars_kernel    one block: c_k in place of c_{k-1} (empty clusters stay), the cluster weights, shift_k and
//                        inertia_k (thread t adds the clusters t, t + 256, ... in index order, then a fixed tree),
//                        iterations += 1 and the stop word (kmvp_kmeans_step.hpp)
// The host reads the state words after every iteration (the decision has been taken on the device by then: it only
// learns whether to launch another).  Nothing but the fp64 centroids is carried from one iteration to the next, so a solve
// cut into calls of maxit = 1 walks through the same bits.
#include "kmvp_ctx.hpp"
#include "kmvp_kmeans_step.hpp"

namespace kmvp {
namespace {

constexpr int KM_THREADS = 256;
constexpr int KM_MAX_C = 65536;
constexpr int KM_GROUP = 16;  // labels the update examines per round of broadcast reads
// the state words behind the vectors: stop, iterations, inertia, shift
constexpr size_t KM_STATE_WORDS = 4;
// LDS of one update workgroup: at most 60 KiB (two workgroups and more per CU of 160 KiB; at D = 3 the accumulators of
// 1024 clusters, 40 KiB, and the staged points, 11 KiB, make one pass and three workgroups per CU)
constexpr size_t KM_LDS_BYTES = 60 * 1024;
// workgroups of the update: at most this many, and no more than keep the partials within KM_PART_BYTES
constexpr int64_t KM_MAX_GROUPS = 1024;
constexpr size_t KM_PART_BYTES = (size_t)128 << 20;

// Sum over the block in a fixed tree order; every thread gets it.
__device__ __forceinline__ double km_block_sum(double v, double* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int s = KM_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  const double r = sh[0];
  __syncthreads();
  return r;
}

// records [rows][R] from the centroids (C, D): pack_sources_kernel's density layout, coordinates rounded to `real`
template <typename real>
__global__ void km_records_kernel(const double* __restrict__ cent, real* __restrict__ rec, int C, int64_t rows, int D, int R) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= rows) return;
  real* r = rec + j * R;
  for (int d = 0; d < D; ++d) r[d] = j < C ? (real)cent[j * D + d] : (real)INFINITY;
  for (int q = D; q < R; ++q) r[q] = (real)0;
}

// LDS: lab [256] ints (read 16 bytes at a time: first) | acc [D + 2][CP] doubles | stage [D + 2][256] doubles
inline size_t km_lds_bytes(int D, int CP) { return ((size_t)(D + 2) * (CP + KM_THREADS)) * sizeof(double) + KM_THREADS * sizeof(int); }

// Thread t owns the clusters whose low eight bits are km_owner_key(t): bits 0-1 of the cluster pick the wave, bits 2-7 the
// lane, so that neighbouring clusters -- and all of them when C < 256 -- spread over the four waves of the workgroup.
__device__ __forceinline__ int km_owner_key(int t) { return ((t & 63) << 2) | (t >> 6); }

template <int D, typename real>
__global__ void __launch_bounds__(KM_THREADS) km_update_kernel(const real* __restrict__ xs, int64_t n_pad, int64_t n,
                                                               const double* __restrict__ cand, const double* __restrict__ w,
                                                               int C, int CP, int64_t run, double* __restrict__ part,
                                                               double* __restrict__ bad) {
  extern __shared__ __attribute__((aligned(16))) double km_lds[];
  constexpr int NK = D + 2;
  int* lab = reinterpret_cast<int*>(km_lds);
  double* acc = km_lds + KM_THREADS * sizeof(int) / sizeof(double);
  double* stage = acc + (size_t)NK * CP;
  const int t = threadIdx.x;
  const int key = km_owner_key(t);
  const int64_t p0 = (int64_t)blockIdx.x * run;
  const int64_t p1 = p0 + run < n ? p0 + run : n;
  double* mypart = part + (int64_t)blockIdx.x * NK * C;
  double unlabelled = 0.0;

  // point i as thread t holds it between the load and the stage: label, coordinates, weight, squared distance
  int nl = -1;
  real nx[D];
  double nw = 1.0, ns = 0.0;
  auto gload = [&](int64_t i) {
    nl = -1;
    if (i < p1) {
      nl = (int)cand[n + i];
      ns = cand[i];
      nw = w ? w[i] : 1.0;
#pragma unroll
      for (int d = 0; d < D; ++d) nx[d] = xs[(int64_t)d * n_pad + i];
    }
  };

  for (int c0 = 0; c0 < C; c0 += CP) {
    const int cp = C - c0 < CP ? C - c0 : CP;
    for (int q = t; q < NK * CP; q += KM_THREADS) acc[q] = 0.0;
    gload(p0 + t);
    for (int64_t base = p0; base < p1; base += KM_THREADS) {
      // ---- stage: thread t writes the point it loaded; one whose cluster is not of this pass is staged as label -1.
      // The loads of the next 256 points are issued before the walk and land during it.
      int l = nl;
      if (c0 == 0 && base + t < p1 && l < 0) unlabelled += 1.0;
      if ((unsigned)(l - c0) < (unsigned)cp) {
#pragma unroll
        for (int d = 0; d < D; ++d) stage[d * KM_THREADS + t] = nw * (double)nx[d];
        stage[D * KM_THREADS + t] = nw;
        stage[(D + 1) * KM_THREADS + t] = nw * ns;
      } else {
        l = -1;
      }
      lab[t] = l;
      __syncthreads();  // (the first one also covers the zeroed accumulators)
      gload(base + KM_THREADS + t);
      // ---- walk: the 256 labels in index order, sixteen per round of broadcast reads.  A lane that owns some of the
      // sixteen adds them into its own accumulators one after the other, in index order; lanes owning different ones do so
      // side by side.  All D + 2 reads of a point are issued before the first add: one LDS latency per point, not D + 2.
      const int4* lab4 = reinterpret_cast<const int4*>(lab);
      for (int q16 = 0; q16 < KM_THREADS / KM_GROUP; ++q16) {
        int L[KM_GROUP];
#pragma unroll
        for (int u = 0; u < KM_GROUP / 4; ++u) {
          const int4 v = lab4[q16 * (KM_GROUP / 4) + u];
          L[4 * u] = v.x;
          L[4 * u + 1] = v.y;
          L[4 * u + 2] = v.z;
          L[4 * u + 3] = v.w;
        }
        unsigned m = 0u;
#pragma unroll
        for (int u = 0; u < KM_GROUP; ++u) m |= (L[u] >= 0 && (L[u] & (KM_THREADS - 1)) == key) ? (1u << u) : 0u;
        while (__any(m != 0u)) {  // wave-uniform
          if (m != 0u) {
            const int j = __builtin_ctz(m);
            m &= m - 1u;
            int lj = L[0];
#pragma unroll
            for (int u = 1; u < KM_GROUP; ++u) lj = j == u ? L[u] : lj;
            const double* sp = stage + q16 * KM_GROUP + j;
            double* ap = acc + (lj - c0);
            double sv[NK], av[NK];
#pragma unroll
            for (int k = 0; k < NK; ++k) {
              sv[k] = sp[k * KM_THREADS];
              av[k] = ap[k * CP];
            }
#pragma unroll
            for (int k = 0; k < NK; ++k) ap[k * CP] = av[k] + sv[k];
          }
        }
      }
      __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < NK; ++k)
      for (int cl = t; cl < cp; cl += KM_THREADS) mypart[(int64_t)k * C + c0 + cl] = acc[k * CP + cl];
    __syncthreads();
  }
  // the block's points without a label (counted in the first pass), through the stage (at least 3 x 256 doubles)
  const double u = km_block_sum(unlabelled, stage);
  if (t == 0) bad[blockIdx.x] = u;
}

template <typename real>
void launch_km_update(int D, dim3 grid, size_t lds, hipStream_t stream, const real* xs, int64_t n_pad, int64_t n, const double* cand,
                      const double* w, int C, int CP, int64_t run, double* part, double* bad) {
#define KMVP_KM_CASE(DD)                                                                                                     \
  case DD:                                                                                                                   \
    hipLaunchKernelGGL((km_update_kernel<DD, real>), grid, dim3(KM_THREADS), lds, stream, xs, n_pad, n, cand, w, C, CP, run, \
                       part, bad);                                                                                          \
    break;
  switch (D) {
    KMVP_KM_CASE(1) KMVP_KM_CASE(2) KMVP_KM_CASE(3) KMVP_KM_CASE(4) KMVP_KM_CASE(5) KMVP_KM_CASE(6) KMVP_KM_CASE(7) KMVP_KM_CASE(8)
  }
#undef KMVP_KM_CASE
}

// tot[q] = sum_g part[g][q], q < (D + 2) C, in a fixed order that depends on G alone: sixteen threads per q add the
// workgroups g = r, r + 16, ... in order (r = 0 .. 15: sixteen loads in flight per q instead of one chain of G), then one of
// them adds the sixteen in order.  A block takes sixteen consecutive q.
constexpr int KM_RED = 16;
__global__ void __launch_bounds__(KM_RED * KM_RED) km_reduce_kernel(const double* __restrict__ part, double* __restrict__ tot,
                                                                    int64_t count, int G) {
  __shared__ double sh[KM_RED][KM_RED];
  const int ql = threadIdx.x & (KM_RED - 1), r = threadIdx.x / KM_RED;
  const int64_t q = (int64_t)blockIdx.x * KM_RED + ql;
  double v = 0.0;
  if (q < count) {
    int g = r;
    for (; g + 3 * KM_RED < G; g += 4 * KM_RED) {
      const double a0 = part[(int64_t)g * count + q], a1 = part[(int64_t)(g + KM_RED) * count + q];
      const double a2 = part[(int64_t)(g + 2 * KM_RED) * count + q], a3 = part[(int64_t)(g + 3 * KM_RED) * count + q];
      v += a0;
      v += a1;
      v += a2;
      v += a3;
    }
    for (; g < G; g += KM_RED) v += part[(int64_t)g * count + q];
  }
  sh[r][ql] = v;
  __syncthreads();
  if (r == 0 && q < count) {
    double s = sh[0][ql];
    for (int k = 1; k < KM_RED; ++k) s += sh[k][ql];
    tot[q] = s;
  }
}

// One block: the new centroids in place, the cluster weights, shift and inertia, and the verdict on this iteration.
// st = [stop | iterations | inertia | shift]
__global__ void __launch_bounds__(KM_THREADS) km_scalars_kernel(const double* __restrict__ tot, double* __restrict__ cent,
                                                                double* __restrict__ cw, int C, int D,
                                                                const double* __restrict__ bad, int G, double* __restrict__ st,
                                                                double tol, int maxit) {
  __shared__ double sh[KM_THREADS];
  double sterm = 0.0, iterm = 0.0, b = 0.0;
  for (int c = threadIdx.x; c < C; c += KM_THREADS) {
    sterm += km_step_cluster(tot + c, C, D, cent + (int64_t)c * D, cw + c);
    iterm += tot[(int64_t)(D + 1) * C + c];
  }
  for (int g = threadIdx.x; g < G; g += KM_THREADS) b += bad[g];
  const double shift = km_block_sum(sterm, sh);
  const double inertia = km_block_sum(iterm, sh);
  const double unlabelled = km_block_sum(b, sh);
  if (threadIdx.x == 0) {
    const double it = st[1] + 1.0;
    st[0] = (double)km_verdict(unlabelled, inertia, shift, it, tol, maxit);
    st[1] = it;
    st[2] = inertia;
    st[3] = shift;
  }
}

__global__ void km_labels_kernel(const double* __restrict__ cand, int64_t* __restrict__ labels, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) labels[i] = (int64_t)cand[n + i];
}

template <typename real>
int kmeans_t(kmvp_ctx* c, int C, const double* weights, double tol, int maxit, double* centroids, int64_t* labels,
             double* cluster_weight, int* iters, double* inertia, double* shift) {
  const int D = c->D, NK = D + 2;
  const int64_t N = c->N;
  const int R = (D + 3) / 4 * 4;  // density layout: no signal columns
  int rc;
  // the launch of kmvp_nearest(K = 1) with the centroids as sources
  const int64_t tile = 64 * (int64_t)WAVES_PER_BLOCK;
  const int64_t n_pad0 = round_up(N, tile), m_pad0 = round_up((int64_t)C, LOWD_BATCH);
  LowdArgs<real> a = lowd_geometry<real>(N, C, knn_segments(c->opt_segments, 1, n_pad0 / tile, m_pad0, n_pad0), c->opt_chunk, 0, C,
                                         1, R, 2);
  const int64_t grid = (int64_t)a.tile_blocks * a.segments;
  if (grid > 0x7fffffff) return fail(c, KMVP_E_UNSUPPORTED, "launch grid too large");

  // the update's geometry, a function of (N, C, D) alone: clusters per pass within the LDS of a workgroup, points per
  // workgroup in whole stages of 256, workgroups within KM_MAX_GROUPS and the partials' budget
  const int cp_max = (int)((KM_LDS_BYTES - KM_THREADS * sizeof(int)) / (NK * sizeof(double))) - KM_THREADS;
  const int CP = std::min(C, cp_max);
  const size_t lds = km_lds_bytes(D, CP);
  const size_t wg_bytes = (size_t)NK * C * sizeof(double);
  const int64_t g_max = std::max<int64_t>(1, std::min<int64_t>(KM_MAX_GROUPS, (int64_t)(KM_PART_BYTES / wg_bytes)));
  const int64_t run = round_up((N + g_max - 1) / g_max, (int64_t)KM_THREADS);
  const int G = (int)((N + run - 1) / run);

  HIP_TRY(c, hipEventRecord(c->ev[0], c->stream));
  // ---- the target image of the points, once per kmvp_set_points
  const int64_t rows = a.m_pad + LOWD_BATCH;
  if (c->km_points_ver != c->points_ver) {
    const real* x_raw = (const real*)(c->same_points ? c->y_raw.p : c->x_raw.p);
    if ((rc = ensure(c, c->km_xs, (size_t)D * a.n_pad * sizeof(real)))) return rc;
    hipLaunchKernelGGL((pack_targets_kernel<real>), dim3(blocks_for(a.n_pad)), dim3(256), 0, c->stream, x_raw, (real*)c->km_xs.p, N,
                       a.n_pad, D, (real)1);
    HIP_TRY(c, hipGetLastError());
    c->km_points_ver = c->points_ver;
  }
  if ((rc = ensure(c, c->km_rec, (size_t)rows * R * sizeof(real)))) return rc;
  if ((rc = ensure(c, c->km_part, (size_t)G * wg_bytes))) return rc;
  // scratch of one assignment (shared with kmvp_nearest: rewritten by every call)
  if ((rc = ensure(c, c->part, (size_t)a.segments * 2 * a.n_pad * sizeof(double)))) return rc;
  if ((rc = ensure(c, c->sums, (size_t)2 * N * sizeof(double)))) return rc;
  // [cent C D | tot (D + 2) C | cw C | bad G | state | w N (only with weights) | labels N (int64)]
  const size_t words = (size_t)C * D + (size_t)NK * C + C + G + KM_STATE_WORDS + (weights ? (size_t)N : 0) + (size_t)N;
  if ((rc = ensure(c, c->km_state, words * sizeof(double)))) return rc;
  double* cent = (double*)c->km_state.p;
  double* tot = cent + (size_t)C * D;
  double* cw = tot + (size_t)NK * C;
  double* bad = cw + C;
  double* st = bad + G;
  double* w = weights ? st + KM_STATE_WORDS : nullptr;
  int64_t* d_labels = (int64_t*)(st + KM_STATE_WORDS + (weights ? (size_t)N : 0));

  HIP_TRY(c, hipMemcpyAsync(cent, centroids, (size_t)C * D * sizeof(double), hipMemcpyHostToDevice, c->stream));
  if (weights) HIP_TRY(c, hipMemcpyAsync(w, weights, (size_t)N * sizeof(double), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemsetAsync(st, 0, KM_STATE_WORDS * sizeof(double), c->stream));

  a.xs = (const real*)c->km_xs.p;
  a.rec = (const real*)c->km_rec.p;
  a.part = (double*)c->part.p;
  double* cand = (double*)c->sums.p;
  const int64_t count = (int64_t)NK * C;

  // ---- the iteration
  double state[KM_STATE_WORDS] = {0.0, 0.0, 0.0, 0.0};
  while (state[0] == 0.0) {
    hipLaunchKernelGGL((km_records_kernel<real>), dim3(blocks_for(rows)), dim3(256), 0, c->stream, (const double*)cent,
                       (real*)c->km_rec.p, C, rows, D, R);
    HIP_TRY(c, launch_lowd_knn(D, 1, a, dim3((unsigned)grid), c->stream, &c->last_kernel_name));
    hipLaunchKernelGGL(knn_merge_kernel, dim3(blocks_for(N)), dim3(256), 0, c->stream, (const double*)a.part, cand, N,
                       (int64_t)2 * a.n_pad, a.n_pad, a.segments, 1, 1);
    launch_km_update<real>(D, dim3(G), lds, c->stream, a.xs, a.n_pad, N, (const double*)cand, (const double*)w, C, CP, run,
                           (double*)c->km_part.p, bad);
    hipLaunchKernelGGL(km_reduce_kernel, dim3(blocks_for(count, KM_RED)), dim3(KM_RED * KM_RED), 0, c->stream,
                       (const double*)c->km_part.p, tot, count, G);
    hipLaunchKernelGGL(km_scalars_kernel, dim3(1), dim3(KM_THREADS), 0, c->stream, (const double*)tot, cent, cw, C, D,
                       (const double*)bad, G, st, tol, maxit);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(state, st, sizeof(state), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }

  hipLaunchKernelGGL(km_labels_kernel, dim3(blocks_for(N)), dim3(256), 0, c->stream, (const double*)cand, d_labels, N);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(centroids, cent, (size_t)C * D * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(labels, d_labels, (size_t)N * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  if (cluster_weight) HIP_TRY(c, hipMemcpyAsync(cluster_weight, cw, (size_t)C * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipEventRecord(c->ev[2], c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipEventElapsedTime(&c->last_total_ms, c->ev[0], c->ev[2]));
  c->last_kernel_ms = c->last_total_ms;  // both cover the whole solve (include/kmvp.h)
  c->last_allreduce_ms = 0.f;
  *iters = (int)state[1];
  *inertia = state[2];
  *shift = state[3];
  if ((int)state[0] == KM_CONVERGED) return KMVP_OK;
  c->err = (int)state[0] == KM_NONFINITE
               ? "k-means: a point has no qualifying centroid (label -1: a NaN coordinate, or every distance overflowed), or "
                 "the inertia or the shift is not finite"
               : "k-means stopped at maxit before the shift of the centroids reached the requested tolerance";
  return KMVP_E_NOT_CONVERGED;
}

}  // namespace

int kmeans_solve(kmvp_ctx* c, int C, const double* weights, double tol, int maxit, double* centroids, int64_t* labels,
                 double* cluster_weight, int* iters, double* inertia, double* shift) {
  if (!c) return KMVP_E_INVALID;
  c->note.clear();
  if (!c->have_points) return fail(c, KMVP_E_INVALID, "kmvp_set_points has not been called");
  if (!(tol >= 0.0) || maxit < 1 || C < 1 || !centroids || !labels || !iters || !inertia || !shift)
    return fail(c, KMVP_E_INVALID, "bad k-means arguments (C >= 1, tol >= 0, maxit >= 1, centroids, labels, iters, inertia and "
                                   "shift are all required)");
  if (c->dtype == KMVP_BF16)
    return fail(c, KMVP_E_UNSUPPORTED, "k-means: built for float32 and float64 contexts, not for bfloat16");
  if (c->D > LOWD_MAX_D)
    return fail(c, KMVP_E_UNSUPPORTED, "k-means: D = " + std::to_string(c->D) + " is beyond the nearest-neighbour kernels' D <= " +
                                           std::to_string(LOWD_MAX_D));
  if (c->opt_fast >= 1)
    return fail(c, KMVP_E_UNSUPPORTED, "k-means: fast_sqdists = " + std::to_string(c->opt_fast) +
                                           " asks for a matrix-core form that is not built for it (-1 or 0: the difference form)");
  if (c->exchanges())
    return fail(c, KMVP_E_UNSUPPORTED, "k-means: a communicator is attached, and the sharded iteration is not built");
  if (c->M < c->m_total)
    return fail(c, KMVP_E_UNSUPPORTED, "k-means: the sources are a slice (M < M_total), and the sharded iteration is not built");
  if (C > KM_MAX_C)
    return fail(c, KMVP_E_UNSUPPORTED, "k-means: C = " + std::to_string(C) + " is beyond the update's C <= " + std::to_string(KM_MAX_C));
  if (c->N < 1) return fail(c, KMVP_E_INVALID, "k-means needs at least one point");
  for (int64_t q = 0; q < (int64_t)C * c->D; ++q)
    if (!std::isfinite(centroids[q]))
      return fail(c, KMVP_E_INVALID, "k-means: initial centroid " + std::to_string(q / c->D) + " is not finite");
  if (weights)
    for (int64_t i = 0; i < c->N; ++i)
      if (!(weights[i] >= 0.0) || !std::isfinite(weights[i]))
        return fail(c, KMVP_E_INVALID, "k-means: weights[" + std::to_string(i) + "] is negative or not finite");
  HIP_TRY(c, hipSetDevice(c->device));
  return c->dtype == KMVP_F64
             ? kmeans_t<double>(c, C, weights, tol, maxit, centroids, labels, cluster_weight, iters, inertia, shift)
             : kmeans_t<float>(c, C, weights, tol, maxit, centroids, labels, cluster_weight, iters, inertia, shift);
}

}  // namespace kmvp
