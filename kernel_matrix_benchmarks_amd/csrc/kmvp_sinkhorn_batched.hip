// Batched Sinkhorn (include/kmvp.h kmvp_<kernel>_sinkhorn_batched): one entropic transport problem per batch of
// kmvp_set_batches, all of them in one device-resident solve.  What kmvp_sinkhorn.hip is to lowd_lse_kernel this file is to
// lowd_batch_lse_kernel (kmvp_lowd_batch_lse.hpp), and its rules are that file's.
//
// Both directions live in buffers of the solver's own (skb_*; the batched product's bt_* and the plain Sinkhorn's sk_*
// buffers are never touched): direction 1 = target image of x with records of y (T1: the new u from v), direction 2 =
// target image of y with records of x (T2: the new v from u), whose plan is batch_plan_build with the offsets swapped
// (kmvp_sinkhorn_batch_plan.hpp).  Both are packed once per (kmvp_set_points, kmvp_set_batches); an iteration only rewrites
// the ONE signal slot of each record, (real)(potential + log weight) -- potentials and log-weights stay fp64 on the device.
//
// One iteration k, six launches and the retirement, no atomics:
//   lowd_batch_lse_kernel (direction 2), skb_finish_kernel:  v_k = T2(u_{k-1}) and the slots of y's records
//   lowd_batch_lse_kernel (direction 1), skb_finish_kernel:  ut = T1(v_k); per TILE the sum of a_i |exp(u_i - ut_i) - 1| over
//                                                            its 64 lanes in a fixed tree (dead lanes, points of mass 0: 0)
//   skb_scalars_kernel (one block):  per running batch err_k = its tiles' sums in ascending order, iterations += 1 and the
//                                    stop word (2 a non-finite potential or error, 1 err_k <= tol, 3 maxit reached, else
//                                    0); then how many batches still run, and the launch count
//   skb_commit_kernel:               per batch, only while its stop word is 0: u_k = ut and the slots of x's records
//   skb_retire_kernel:               len = 0 in the working copies of the tiles of stopped batches ("sinkhorn_retire")
// Every batch has its own state words [stop, iterations, err] and, once stopped, takes no further update: the finish kernels
// skip its lanes, so (u, v, iterations, err) of a batch always describe one plan -- with retirement (the pair loop consumes
// nothing for its tiles) or without (it rides along and is ignored), bit for bit.  The host reads two doubles per iteration
// (the decision has been taken on the device by then: it only learns whether to launch another).
#include "kmvp_ctx.hpp"
#include "kmvp_lowd_batch_lse.hpp"
#include "kmvp_sinkhorn_batch_plan.hpp"

namespace kmvp {
namespace {

constexpr int SKB_THREADS = 256;  // BATCH_WAVES tiles per block: n_pad is a whole number of them
static_assert(SKB_THREADS == BATCH_TILE * BATCH_WAVES, "the finish kernels walk the padded slots in whole workgroups");
enum : int { SKB_RUNNING = 0, SKB_CONVERGED = 1, SKB_NONFINITE = 2, SKB_MAXIT = 3 };

// What one direction's kernels read, all in skb_plan.
struct SkbDir {
  const BatchTile* tiles0;    // as planned: i0 and live of every tile, never rewritten
  BatchTile* tiles;           // the working copy the pair loop reads: len = 0 once the tile's batch has stopped
  const int32_t* tile_batch;  // [tiles]
  const int64_t* tile_begin;  // [B + 1]
  const int64_t* other_rec;   // [n_pad]
  const int64_t* tmap;        // [n_pad]
  const int64_t* smap;        // [m_alloc]
  int64_t nt, n_pad, m_alloc;
};

// Sum over each tile's 64 lanes in a fixed tree; lane 0 of every tile gets its tile's sum.
__device__ __forceinline__ double skb_tile_sum(double v, double* sh) {
  const int lane = threadIdx.x & 63;
  sh[threadIdx.x] = v;
  __syncthreads();
  for (int s = BATCH_TILE / 2; s > 0; s >>= 1) {
    if (lane < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  const double r = sh[threadIdx.x & ~63];
  __syncthreads();
  return r;
}

// rec[other_rec(slot) R + D] = (real)(pot_i + logw_i) for the live lanes of every tile: the start's u_0
template <typename real>
__global__ void __launch_bounds__(SKB_THREADS) skb_slot_kernel(const BatchTile* __restrict__ tiles0,
                                                               const int64_t* __restrict__ other_rec,
                                                               const double* __restrict__ pot, const double* __restrict__ logw,
                                                               real* __restrict__ rec, int R, int D) {
  const int64_t s = (int64_t)blockIdx.x * SKB_THREADS + threadIdx.x;
  const BatchTile t = tiles0[s / BATCH_TILE];
  const int lane = (int)(s % BATCH_TILE);
  if (lane >= t.live) return;
  const int64_t i = t.i0 + lane;
  rec[other_rec[s] * R + D] = (real)(pot[i] + logw[i]);
}

// After lowd_batch_lse_kernel, for the targets of one direction whose batch is still running: pot_i = -L_i (no live term:
// +inf).  tbad[tile] counts the tile's non-finite potentials.
//   rec != nullptr (T2): the potential goes straight into the slot of the record the OTHER direction reads.
//   prev != nullptr (T1): terr[tile] = sum over the tile of a_i |exp(prev_i - pot_i) - 1|, a_i = exp(logw_i); a point of mass 0
//   (logw = -inf) and a dead lane contribute exactly 0.
template <typename real>
__global__ void __launch_bounds__(SKB_THREADS) skb_finish_kernel(const BatchTile* __restrict__ tiles0,
                                                                 const int32_t* __restrict__ tile_batch,
                                                                 const int64_t* __restrict__ other_rec,
                                                                 const double* __restrict__ st, const double* __restrict__ L,
                                                                 double* __restrict__ pot, const double* __restrict__ logw,
                                                                 const double* __restrict__ prev, real* __restrict__ rec, int R,
                                                                 int D, double* __restrict__ terr, double* __restrict__ tbad) {
  __shared__ double sh[SKB_THREADS];
  const int64_t s = (int64_t)blockIdx.x * SKB_THREADS + threadIdx.x;
  const int64_t tile = s / BATCH_TILE;
  const int lane = (int)(s % BATCH_TILE);
  const BatchTile t = tiles0[tile];
  const int b = tile_batch[tile];
  const bool running = b >= 0 && st[3 * (int64_t)b] == 0.0;  // as the scalars kernel of the iteration before left it
  double term = 0.0, flag = 0.0;
  if (running && lane < t.live) {
    const int64_t i = t.i0 + lane;
    const double p = -L[i];
    pot[i] = p;
    if (!(fabs(p) < (double)INFINITY)) flag = 1.0;
    const double lw = logw[i];
    if (rec) rec[other_rec[s] * R + D] = (real)(p + lw);
    if (prev && lw > -(double)INFINITY) term = exp(lw) * fabs(expm1(prev[i] - p));
  }
  const double f = skb_tile_sum(flag, sh);
  if (lane == 0) tbad[tile] = f;
  if (prev) {
    const double e = skb_tile_sum(term, sh);
    if (lane == 0) terr[tile] = e;
  }
}

// One block.  Thread q takes the batches q, q + 256, ...: for a running batch, err = its direction-1 tiles' sums in
// ascending order, the non-finite counts of both directions, and the verdict on this iteration, st[b] = [stop | iterations
// | err].  glob = [batches still running | iterations launched].
__global__ void __launch_bounds__(SKB_THREADS) skb_scalars_kernel(const double* __restrict__ terr, const double* __restrict__ tbad_u,
                                                                  const int64_t* __restrict__ begin_u,
                                                                  const double* __restrict__ tbad_v,
                                                                  const int64_t* __restrict__ begin_v, int B,
                                                                  double* __restrict__ st, double* __restrict__ glob, double tol,
                                                                  int maxit) {
  __shared__ double sh[SKB_THREADS];
  double live = 0.0;
  for (int b = threadIdx.x; b < B; b += SKB_THREADS) {
    double* s = st + 3 * (int64_t)b;
    if (s[0] != 0.0) continue;
    double err = 0.0, nbad = 0.0;
    for (int64_t q = begin_u[b]; q < begin_u[b + 1]; ++q) {
      err += terr[q];
      nbad += tbad_u[q];
    }
    for (int64_t q = begin_v[b]; q < begin_v[b + 1]; ++q) nbad += tbad_v[q];
    const double it = s[1] + 1.0;
    int stop = SKB_RUNNING;
    if (nbad != 0.0 || !(fabs(err) < (double)INFINITY)) stop = SKB_NONFINITE;
    else if (err <= tol) stop = SKB_CONVERGED;
    else if (it >= (double)maxit) stop = SKB_MAXIT;
    s[0] = (double)stop;
    s[1] = it;
    s[2] = err;
    if (stop == SKB_RUNNING) live += 1.0;
  }
  // (a count: whole numbers, exact in any order)
  sh[threadIdx.x] = live;
  __syncthreads();
  for (int q = SKB_THREADS / 2; q > 0; q >>= 1) {
    if ((int)threadIdx.x < q) sh[threadIdx.x] += sh[threadIdx.x + q];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    glob[0] = sh[0];
    glob[1] += 1.0;
  }
}

// u = ut and the slots of x's records, per batch, only while its iteration goes on
template <typename real>
__global__ void __launch_bounds__(SKB_THREADS) skb_commit_kernel(const BatchTile* __restrict__ tiles0,
                                                                 const int32_t* __restrict__ tile_batch,
                                                                 const int64_t* __restrict__ other_rec,
                                                                 const double* __restrict__ st, const double* __restrict__ ut,
                                                                 const double* __restrict__ logw, double* __restrict__ u,
                                                                 real* __restrict__ rec, int R, int D) {
  const int64_t s = (int64_t)blockIdx.x * SKB_THREADS + threadIdx.x;
  const int64_t tile = s / BATCH_TILE;
  const int lane = (int)(s % BATCH_TILE);
  const int b = tile_batch[tile];
  if (b < 0 || st[3 * (int64_t)b] != 0.0) return;  // written by skb_scalars_kernel, the launch before this one
  const BatchTile t = tiles0[tile];
  if (lane >= t.live) return;
  const int64_t i = t.i0 + lane;
  const double p = ut[i];
  u[i] = p;
  rec[other_rec[s] * R + D] = (real)(p + logw[i]);
}

// The tiles of stopped batches in the working copies of both tables: len = 0, nothing else -- rec0 keeps pointing inside the
// record array, where the pair loop still issues its first prefetch.  Read by the NEXT launch of the pair loop.
__global__ void skb_retire_kernel(BatchTile* __restrict__ tiles_u, const int32_t* __restrict__ batch_u, int64_t nt_u,
                                  BatchTile* __restrict__ tiles_v, const int32_t* __restrict__ batch_v, int64_t nt_v,
                                  const double* __restrict__ st) {
  int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  BatchTile* tiles = tiles_u;
  const int32_t* batch = batch_u;
  if (q >= nt_u) {
    q -= nt_u;
    if (q >= nt_v) return;
    tiles = tiles_v;
    batch = batch_v;
  }
  const int b = batch[q];
  if (b >= 0 && st[3 * (int64_t)b] != 0.0) tiles[q].len = 0;
}

inline hipError_t launch_batch_lse(int kernel, int D, const LowdBatchLseArgs<float>& a, dim3 grid, hipStream_t s, const char** name) {
  return launch_lowd_batch_lse_f32(kernel, D, 1, SIG_PRODUCT, a, grid, s, name);
}
inline hipError_t launch_batch_lse(int kernel, int D, const LowdBatchLseArgs<double>& a, dim3 grid, hipStream_t s, const char** name) {
  return launch_lowd_batch_lse_f64(kernel, D, 1, SIG_PRODUCT, a, grid, s, name);
}

size_t round32(size_t v) { return (v + 31) / 32 * 32; }

// skb_plan's layout for one direction from byte offset `at` on (32-byte aligned pieces): the two tile tables, then the
// int64 arrays, then the tile-to-batch map.  Returns the offset behind it.
size_t skb_dir_layout(char* base, size_t at, int B, int64_t nt, int64_t n_pad, int64_t m_alloc, SkbDir& d) {
  auto take = [&](size_t bytes) {
    char* p = base + at;
    at += round32(bytes);
    return p;
  };
  d.nt = nt;
  d.n_pad = n_pad;
  d.m_alloc = m_alloc;
  d.tiles0 = (const BatchTile*)take((size_t)nt * sizeof(BatchTile));
  d.tiles = (BatchTile*)take((size_t)nt * sizeof(BatchTile));
  d.tile_begin = (const int64_t*)take((size_t)(B + 1) * sizeof(int64_t));
  d.other_rec = (const int64_t*)take((size_t)n_pad * sizeof(int64_t));
  d.tmap = (const int64_t*)take((size_t)n_pad * sizeof(int64_t));
  d.smap = (const int64_t*)take((size_t)m_alloc * sizeof(int64_t));
  d.tile_batch = (const int32_t*)take((size_t)nt * sizeof(int32_t));
  return at;
}

// The same layout filled on the host, for one upload.
void skb_dir_fill(std::vector<char>& host, const SkbDir& d, const char* base, const SinkhornDirection& s) {
  auto put = [&](const void* dst, const void* src, size_t bytes) {
    if (bytes) memcpy(host.data() + ((const char*)dst - base), src, bytes);
  };
  put(d.tiles0, s.plan.tiles.data(), s.plan.tiles.size() * sizeof(BatchTile));
  put(d.tiles, s.plan.tiles.data(), s.plan.tiles.size() * sizeof(BatchTile));
  put(d.tile_begin, s.tile_begin.data(), s.tile_begin.size() * sizeof(int64_t));
  put(d.other_rec, s.other_rec.data(), s.other_rec.size() * sizeof(int64_t));
  put(d.tmap, s.plan.tmap.data(), s.plan.tmap.size() * sizeof(int64_t));
  put(d.smap, s.plan.smap.data(), s.plan.smap.size() * sizeof(int64_t));
  put(d.tile_batch, s.tile_batch.data(), s.tile_batch.size() * sizeof(int32_t));
}

template <typename real>
int sinkhorn_batched_t(kmvp_ctx* c, int kernel, const double* log_a, const double* log_b, double tol, int maxit, double* u_io,
                       double* v_out, int* iters, double* err, int* status) {
  const int D = c->D, B = c->bt_B;
  const int64_t N = c->N, M = c->M;
  const int R = (D + 1 + 3) / 4 * 4;  // RecLayout<D, 1, SIG_PRODUCT>::R: coordinates, one signal slot, padding
  const int64_t* y_off = c->bt_y_off.data();
  const int64_t* x_off = c->bt_x_off.data();
  int rc;

  HIP_TRY(c, hipEventRecord(c->ev[0], c->stream));
  // ---- plans and layouts, once per (kmvp_set_points, kmvp_set_batches).  The sizes follow from the offsets alone.
  int64_t nt[2] = {0, 0}, m_pad[2] = {0, 0};
  for (int b = 0; b < B; ++b) {
    const int64_t n = x_off[b + 1] - x_off[b], m = y_off[b + 1] - y_off[b];
    nt[0] += (n + BATCH_TILE - 1) / BATCH_TILE;
    nt[1] += (m + BATCH_TILE - 1) / BATCH_TILE;
    m_pad[0] += batch_round_up(m, BATCH_RECORDS);
    m_pad[1] += batch_round_up(n, BATCH_RECORDS);
  }
  for (int d = 0; d < 2; ++d) nt[d] = batch_round_up(nt[d], BATCH_WAVES);
  if (nt[0] / BATCH_WAVES > MAX_GRID || nt[1] / BATCH_WAVES > MAX_GRID)
    return fail(c, KMVP_E_UNSUPPORTED, "batched Sinkhorn: launch grid too large");
  SkbDir d1, d2;
  size_t plan_bytes = skb_dir_layout(nullptr, 0, B, nt[0], nt[0] * BATCH_TILE, m_pad[0] + BATCH_RECORDS, d1);
  plan_bytes = skb_dir_layout(nullptr, plan_bytes, B, nt[1], nt[1] * BATCH_TILE, m_pad[1] + BATCH_RECORDS, d2);
  const bool stale = c->skb_points_ver != c->points_ver || c->skb_bt_ver != c->bt_ver;
  if ((rc = ensure(c, c->skb_plan, plan_bytes))) return rc;
  char* base = (char*)c->skb_plan.p;
  size_t at = skb_dir_layout(base, 0, B, nt[0], nt[0] * BATCH_TILE, m_pad[0] + BATCH_RECORDS, d1);
  skb_dir_layout(base, at, B, nt[1], nt[1] * BATCH_TILE, m_pad[1] + BATCH_RECORDS, d2);
  const size_t xs_reals = (size_t)D * (d1.n_pad + d2.n_pad);
  const size_t rec_reals = (size_t)(d1.m_alloc + d2.m_alloc) * R;
  if ((rc = ensure(c, c->skb_xs, std::max<size_t>(xs_reals, 1) * sizeof(real)))) return rc;
  if ((rc = ensure(c, c->skb_rec, rec_reals * sizeof(real)))) return rc;
  real* xs_x = (real*)c->skb_xs.p;
  real* xs_y = xs_x + (size_t)D * d1.n_pad;
  real* rec_y = (real*)c->skb_rec.p;                // direction 1 reads the records of y
  real* rec_x = rec_y + (size_t)d1.m_alloc * R;     // direction 2 reads the records of x
  if (stale) {
    c->skb_points_ver = c->skb_bt_ver = 0;  // (a failure below leaves nothing half-built behind)
    SinkhornBatchPlan p;
    if (!sinkhorn_batch_plan_build(B, y_off, x_off, p))
      return fail(c, KMVP_E_UNSUPPORTED, "batched Sinkhorn: a batch of 2^31 points or more (the pair loop counts positions within "
                                         "a batch in 32 bits)");
    if ((int64_t)p.d1.plan.tiles.size() != nt[0] || (int64_t)p.d2.plan.tiles.size() != nt[1] || p.d1.plan.m_alloc != d1.m_alloc ||
        p.d2.plan.m_alloc != d2.m_alloc)
      return fail(c, KMVP_E_DEVICE, "batched Sinkhorn: the plan's sizes disagree with the offsets'");
    std::vector<char> host(plan_bytes, 0);
    skb_dir_fill(host, d1, base, p.d1);
    skb_dir_fill(host, d2, base, p.d2);
    HIP_TRY(c, hipMemcpyAsync(base, host.data(), plan_bytes, hipMemcpyHostToDevice, c->stream));
    const real* x_raw = (const real*)(c->same_points ? c->y_raw.p : c->x_raw.p);
    const real* y_raw = (const real*)c->y_raw.p;
    if (d1.n_pad > 0)
      hipLaunchKernelGGL((batch_pack_targets_kernel<real>), dim3(blocks_for(d1.n_pad)), dim3(256), 0, c->stream, x_raw, d1.tmap,
                         xs_x, d1.n_pad, D);
    if (d2.n_pad > 0)
      hipLaunchKernelGGL((batch_pack_targets_kernel<real>), dim3(blocks_for(d2.n_pad)), dim3(256), 0, c->stream, y_raw, d2.tmap,
                         xs_y, d2.n_pad, D);
    hipLaunchKernelGGL((batch_pack_sources_kernel<real>), dim3(blocks_for(d1.m_alloc)), dim3(256), 0, c->stream, y_raw, d1.smap,
                       rec_y, d1.m_alloc, D, R);
    hipLaunchKernelGGL((batch_pack_sources_kernel<real>), dim3(blocks_for(d2.m_alloc)), dim3(256), 0, c->stream, x_raw, d2.smap,
                       rec_x, d2.m_alloc, D, R);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // the host image is only read during the upload
    c->skb_points_ver = c->points_ver;
    c->skb_bt_ver = c->bt_ver;
  } else {
    // the working copies of the tile tables start every solve as planned
    if (d1.nt > 0)
      HIP_TRY(c, hipMemcpyAsync(d1.tiles, d1.tiles0, (size_t)d1.nt * sizeof(BatchTile), hipMemcpyDeviceToDevice, c->stream));
    if (d2.nt > 0)
      HIP_TRY(c, hipMemcpyAsync(d2.tiles, d2.tiles0, (size_t)d2.nt * sizeof(BatchTile), hipMemcpyDeviceToDevice, c->stream));
  }

  // ---- the state: [u N | ut N | log_a N | v M | log_b M | L max(N, M) | terr nt1 | tbad_u nt1 | tbad_v nt2 | st 3 B | glob 2]
  const size_t words = 3 * (size_t)N + 2 * (size_t)M + (size_t)std::max(N, M) + 2 * (size_t)d1.nt + (size_t)d2.nt + 3 * (size_t)B + 2;
  if ((rc = ensure(c, c->skb_state, words * sizeof(double)))) return rc;
  double* u = (double*)c->skb_state.p;
  double* ut = u + N;
  double* la = ut + N;
  double* v = la + N;
  double* lb = v + M;
  double* L = lb + M;
  double* terr = L + std::max(N, M);
  double* tbad_u = terr + d1.nt;
  double* tbad_v = tbad_u + d1.nt;
  double* st = tbad_v + d2.nt;
  double* glob = st + 3 * (size_t)B;

  // u_0, the log-weights (NULL: uniform within each batch) and the batches' state words: a batch that is empty on both
  // sides has converged before the first iteration.  v of every batch with points is written by the first iteration.
  std::vector<double> uniform_a(log_a ? 0 : (size_t)N), uniform_b(log_b ? 0 : (size_t)M), st0(3 * (size_t)B + 2, 0.0);
  int running0 = 0;
  for (int b = 0; b < B; ++b) {
    const int64_t n = x_off[b + 1] - x_off[b], m = y_off[b + 1] - y_off[b];
    if (!log_a) std::fill(uniform_a.begin() + x_off[b], uniform_a.begin() + x_off[b + 1], -std::log((double)n));
    if (!log_b) std::fill(uniform_b.begin() + y_off[b], uniform_b.begin() + y_off[b + 1], -std::log((double)m));
    st0[3 * (size_t)b] = n == 0 ? (double)SKB_CONVERGED : (double)SKB_RUNNING;
    running0 += n > 0;
  }
  st0[3 * (size_t)B] = (double)running0;
  if (N > 0) {
    HIP_TRY(c, hipMemcpyAsync(u, u_io, (size_t)N * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(la, log_a ? log_a : uniform_a.data(), (size_t)N * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(lb, log_b ? log_b : uniform_b.data(), (size_t)M * sizeof(double), hipMemcpyHostToDevice, c->stream));
  }
  HIP_TRY(c, hipMemcpyAsync(st, st0.data(), st0.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
  const dim3 grid1((unsigned)(d1.nt / BATCH_WAVES)), grid2((unsigned)(d2.nt / BATCH_WAVES));
  if (running0 > 0) {
    hipLaunchKernelGGL((skb_slot_kernel<real>), grid1, dim3(SKB_THREADS), 0, c->stream, d1.tiles0, d1.other_rec, (const double*)u,
                       (const double*)la, rec_x, R, D);
    HIP_TRY(c, hipGetLastError());
  }

  LowdBatchLseArgs<real> a1, a2;
  a1.xs = xs_x;
  a1.rec = rec_y;
  a1.tiles = d1.tiles;
  a1.n_pad = d1.n_pad;
  a2.xs = xs_y;
  a2.rec = rec_x;
  a2.tiles = d2.tiles;
  a2.n_pad = d2.n_pad;
  a1.out = a2.out = L;
  a1.chunk = a2.chunk = (int)round_up(c->opt_chunk > 8 ? c->opt_chunk : 8, LOWD_BATCH);  // lowd_geometry's rule
  const bool retire = c->opt_sinkhorn_retire != 0;
  c->last_kernel_name = "lowd_batch_lse_kernel";

  // ---- the iteration
  double glob_h[2] = {(double)running0, 0.0};
  while (glob_h[0] > 0.0) {
    // v = T2(u): targets y, records of x with u + log_a in the slot; the finish writes v + log_b into y's records
    hipError_t le = launch_batch_lse(kernel, D, a2, grid2, c->stream, &c->last_kernel_name);
    if (le == hipErrorInvalidValue) return fail(c, KMVP_E_UNSUPPORTED, "batched Sinkhorn: no kernel instantiated for this (kernel, D)");
    HIP_TRY(c, le);
    hipLaunchKernelGGL((skb_finish_kernel<real>), grid2, dim3(SKB_THREADS), 0, c->stream, d2.tiles0, d2.tile_batch, d2.other_rec,
                       (const double*)st, (const double*)L, v, (const double*)lb, (const double*)nullptr, rec_y, R, D,
                       (double*)nullptr, tbad_v);
    // ut = T1(v): targets x, records of y; the finish leaves the tiles' sums of the row marginal's violation
    HIP_TRY(c, launch_batch_lse(kernel, D, a1, grid1, c->stream, &c->last_kernel_name));
    hipLaunchKernelGGL((skb_finish_kernel<real>), grid1, dim3(SKB_THREADS), 0, c->stream, d1.tiles0, d1.tile_batch, d1.other_rec,
                       (const double*)st, (const double*)L, ut, (const double*)la, (const double*)u, (real*)nullptr, R, D, terr,
                       tbad_u);
    hipLaunchKernelGGL(skb_scalars_kernel, dim3(1), dim3(SKB_THREADS), 0, c->stream, (const double*)terr, (const double*)tbad_u,
                       d1.tile_begin, (const double*)tbad_v, d2.tile_begin, B, st, glob, tol, maxit);
    hipLaunchKernelGGL((skb_commit_kernel<real>), grid1, dim3(SKB_THREADS), 0, c->stream, d1.tiles0, d1.tile_batch, d1.other_rec,
                       (const double*)st, (const double*)ut, (const double*)la, u, rec_x, R, D);
    if (retire)
      hipLaunchKernelGGL(skb_retire_kernel, dim3(blocks_for(d1.nt + d2.nt)), dim3(256), 0, c->stream, d1.tiles, d1.tile_batch,
                         d1.nt, d2.tiles, d2.tile_batch, d2.nt, (const double*)st);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(glob_h, glob, sizeof(glob_h), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }

  std::vector<double> st_h(3 * (size_t)B);
  if (N > 0) {
    HIP_TRY(c, hipMemcpyAsync(u_io, u, (size_t)N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(v_out, v, (size_t)M * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(c, hipMemcpyAsync(st_h.data(), st, st_h.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipEventRecord(c->ev[2], c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipEventElapsedTime(&c->last_total_ms, c->ev[0], c->ev[2]));
  c->last_kernel_ms = c->last_total_ms;  // both cover the whole solve (include/kmvp.h)
  c->last_allreduce_ms = 0.f;
  int nonfinite = 0, at_maxit = 0, first_bad = -1;
  for (int b = 0; b < B; ++b) {
    status[b] = (int)st_h[3 * (size_t)b];
    iters[b] = (int)st_h[3 * (size_t)b + 1];
    err[b] = st_h[3 * (size_t)b + 2];
    nonfinite += status[b] == SKB_NONFINITE;
    at_maxit += status[b] == SKB_MAXIT;
    if (status[b] != SKB_CONVERGED && first_bad < 0) first_bad = b;
  }
  if (first_bad < 0) return KMVP_OK;
  c->err = "batched Sinkhorn: " + std::to_string(nonfinite) + " of " + std::to_string(B) +
           " batches stopped on a potential or marginal error that is not finite (a row without a live term, a non-finite "
           "coordinate, weight or starting potential), " + std::to_string(at_maxit) +
           " at maxit before the marginal error reached the requested tolerance; the first is batch " + std::to_string(first_bad);
  return KMVP_E_NOT_CONVERGED;
}

}  // namespace

int sinkhorn_batched_solve(kmvp_ctx* c, int kernel, const double* log_a, const double* log_b, double tol, int maxit, double* u,
                           double* v, int* iters, double* err, int* status) {
  if (!c) return KMVP_E_INVALID;
  c->note.clear();
  if (!c->have_points) return fail(c, KMVP_E_INVALID, "kmvp_set_points has not been called");
  if (!c->bt_on)
    return fail(c, KMVP_E_INVALID, "batched Sinkhorn: batches are not set (kmvp_set_batches comes first; kmvp_<kernel>_sinkhorn "
                                   "solves one problem on the whole clouds)");
  if (!(tol >= 0.0) || maxit < 1 || !u || !v || !iters || !err || !status)
    return fail(c, KMVP_E_INVALID, "bad batched Sinkhorn arguments (tol >= 0, maxit >= 1, u, v, iters, err and status are all required)");
  int rc;
  if ((rc = batched_unsupported(c, "Sinkhorn"))) return rc;
  const int bad = sinkhorn_one_sided_batch(c->bt_B, c->bt_y_off.data(), c->bt_x_off.data());
  if (bad >= 0)
    return fail(c, KMVP_E_INVALID, "batched Sinkhorn: batch " + std::to_string(bad) + " has points on one side only (" +
                                       std::to_string(c->bt_x_off[bad + 1] - c->bt_x_off[bad]) + " targets, " +
                                       std::to_string(c->bt_y_off[bad + 1] - c->bt_y_off[bad]) + " sources)");
  HIP_TRY(c, hipSetDevice(c->device));
  return c->dtype == KMVP_F64 ? sinkhorn_batched_t<double>(c, kernel, log_a, log_b, tol, maxit, u, v, iters, err, status)
                              : sinkhorn_batched_t<float>(c, kernel, log_a, log_b, tol, maxit, u, v, iters, err, status);
}

}  // namespace kmvp
