// DBSCAN on the cell list, resident on the device (include/kmvp.h kmvp_dbscan).
//   1. the count (kmvp_cutoff.hip cutoff_count_device: kmvp_radius_count's plan, packs and walk), once
//   2. lab[i] = i for a core point (counts[i] >= min_samples), DB_NONE otherwise
//   3. rounds until one changes nothing:
//        db_round_begin_kernel  lab scattered through ct_smap32 into lab_rec (record order), par = lab, the changed word 0
//        lowd_cutoff_label_kernel<SWEEP>  nxt[i] = the smallest label among i's inside core points
//        db_hook_kernel         atomicMin(&par[lab[i]], nxt[i]) where nxt[i] < lab[i]; nobody reads par in this launch
//        db_chase_kernel        lab[i] = the root of i in par, which it only reads
//      the host reads the changed word, 4 bytes, once per round
//   4. lowd_cutoff_label_kernel<BORDER>: every point that is no core point gets its nearest inside core point, or -1
//   5. the roots flagged, an exclusive scan (hipcub) numbers the clusters, labels / core_of / the info words written
// The integer rules are kmvp_dbscan_step.hpp's.  Why the result is the definition's and independent of scheduling: the
// sweep reads labels no launch writes while it runs (a Jacobi step); the hook takes minima only, so par's final state is a
// pure minimum over the requests; the chase reads par and writes lab.  Labels only fall and every round but the last
// removes a root, so the rounds end by themselves; a guard of N rounds answers KMVP_E_DEVICE.
// All buffers are DBSCAN's own (db_state, db_rec, db_tmp) beside the cutoff's cached plan and packs, which it shares with
// kmvp_radius_count and kmvp_radius_nearest: every other entry returns the bits it returned before.
#include <hipcub/hipcub.hpp>

#include "kmvp_ctx.hpp"
#include "kmvp_dbscan_step.hpp"
#include "kmvp_lowd_cutoff_label.hpp"

namespace kmvp {

namespace {

static_assert(DB_NONE == LABEL_NONE, "one sentinel in the step rules and in the pair loop");

// the 64-bit state words
enum : int { DBW_CLUSTERS = 0, DBW_CORE = 1, DBW_BORDER = 2, DBW_NOISE = 3, DBW_N = 4 };

__device__ __forceinline__ void db_count_into(unsigned long long* word, bool mine) {
  const unsigned long long n = (unsigned long long)__popcll(__ballot(mine));
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(word, n);
}

__global__ void db_init_kernel(const int64_t* __restrict__ counts, int64_t min_samples, int32_t* __restrict__ lab, int64_t N,
                               unsigned long long* __restrict__ words) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int32_t l = DB_NONE;
  if (i < N) lab[i] = l = db_initial_label(counts[i], min_samples, i);
  db_count_into(words + DBW_CORE, l != DB_NONE);
}

__global__ void db_round_begin_kernel(const int32_t* __restrict__ lab, const int32_t* __restrict__ smap32, int32_t* __restrict__ lab_rec,
                                      int32_t* __restrict__ par, int64_t m_alloc, int64_t N, int32_t* __restrict__ changed) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t == 0) *changed = 0;
  if (t < m_alloc) {
    const int32_t j = smap32[t];
    lab_rec[t] = j >= 0 ? lab[j] : DB_NONE;
  }
  if (t < N) par[t] = lab[t];
}

__global__ void db_hook_kernel(const int32_t* __restrict__ lab, const int32_t* __restrict__ nxt, int32_t* par, int64_t N) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  const int32_t l = lab[i];
  int32_t slot, value;
  if (db_hook(l, l != DB_NONE ? nxt[i] : DB_NONE, &slot, &value)) atomicMin(par + slot, value);
}

__global__ void db_chase_kernel(const int32_t* __restrict__ par, int32_t* __restrict__ lab, int64_t N) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  if (par[i] != DB_NONE) lab[i] = db_chase(par, (int32_t)i);
}

__global__ void db_flag_kernel(const int32_t* __restrict__ lab, int32_t* __restrict__ flag, int64_t N) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N) flag[i] = db_root(lab[i], i);
}

// attach == nullptr: no border walk ran (there is no core point, or nothing else)
__global__ void db_finish_kernel(const int32_t* __restrict__ lab, const int32_t* __restrict__ attach, const int32_t* __restrict__ flag,
                                 const int32_t* __restrict__ cid, int64_t* __restrict__ labels, int64_t* __restrict__ core_of, int64_t N,
                                 unsigned long long* __restrict__ words) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool border = false, noise = false;
  if (i < N) {
    const int32_t l = lab[i];
    const int64_t co = db_core_of(l, (l == DB_NONE && attach) ? attach[i] : -1, i);
    core_of[i] = co;
    labels[i] = db_label(co, lab, cid);
    border = l == DB_NONE && co >= 0;
    noise = co < 0;
    if (i == N - 1) words[DBW_CLUSTERS] = (unsigned long long)(cid[i] + flag[i]);
  }
  db_count_into(words + DBW_BORDER, border);
  db_count_into(words + DBW_NOISE, noise);
}

inline hipError_t launch_label(int D, int mode, const LowdCutoffLabelArgs<float>& a, dim3 grid, hipStream_t s, const char** name) {
  return launch_lowd_cutoff_label_f32(D, mode, a, grid, s, name);
}
inline hipError_t launch_label(int D, int mode, const LowdCutoffLabelArgs<double>& a, dim3 grid, hipStream_t s, const char** name) {
  return launch_lowd_cutoff_label_f64(D, mode, a, grid, s, name);
}

inline size_t db_align(size_t bytes) { return (bytes + 255) / 256 * 256; }

template <typename real>
int dbscan_t(kmvp_ctx* c, double radius, int64_t min_samples, int64_t* labels, int64_t* core_of, int64_t* counts, int64_t* info) {
  const int D = c->D;
  const int64_t N = c->N;
  int rc;
  HIP_TRY(c, hipEventRecord(c->ev[0], c->stream));

  // db_state: counts, labels, core_of (int64), then lab, nxt, par, attach, flag, cid (int32), then the state words
  const size_t b64 = db_align((size_t)N * sizeof(int64_t)), b32 = db_align((size_t)N * sizeof(int32_t));
  if ((rc = ensure(c, c->db_state, 3 * b64 + 6 * b32 + 256))) return rc;
  char* base = (char*)c->db_state.p;
  int64_t* d_counts = (int64_t*)base;
  int64_t* d_labels = (int64_t*)(base + b64);
  int64_t* d_core_of = (int64_t*)(base + 2 * b64);
  int32_t* lab = (int32_t*)(base + 3 * b64);
  int32_t* nxt = (int32_t*)(base + 3 * b64 + b32);
  int32_t* par = (int32_t*)(base + 3 * b64 + 2 * b32);
  int32_t* attach = (int32_t*)(base + 3 * b64 + 3 * b32);
  int32_t* flag = (int32_t*)(base + 3 * b64 + 4 * b32);
  int32_t* cid = (int32_t*)(base + 3 * b64 + 5 * b32);
  unsigned long long* words = (unsigned long long*)(base + 3 * b64 + 6 * b32);
  int32_t* changed = (int32_t*)(words + DBW_N);

  float walk_ms = 0.f, ms = 0.f;
  int64_t walks = 0, rounds = 0;
  const dim3 pts(blocks_for(N)), tb(256);

  // 1. the count
  if ((rc = cutoff_count_device(c, radius, d_counts))) return rc;
  ++walks;
  // 2. the core points and their number
  HIP_TRY(c, hipMemsetAsync(words, 0, 256, c->stream));
  hipLaunchKernelGGL(db_init_kernel, pts, tb, 0, c->stream, (const int64_t*)d_counts, min_samples, lab, N, words);
  HIP_TRY(c, hipGetLastError());
  unsigned long long n_core = 0;
  HIP_TRY(c, hipMemcpyAsync(&n_core, words + DBW_CORE, sizeof(n_core), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[3], c->ev[1]));
  walk_ms += ms;

  LowdCutoffLabelArgs<real> a;
  a.xs = (const real*)c->ct_xs.p;
  a.rec = (const real*)c->ct_rec.p;
  a.tiles = (const CutoffTile*)c->ct_tiles.p;
  a.runs = (const CutoffRun*)c->ct_runs.p;
  a.tmap = (const int64_t*)c->ct_tmap.p;
  a.n_pad = c->ct_n_pad;
  a.r2 = (real)(radius * radius);
  a.smap32 = (const int32_t*)c->ct_smap32.p;
  a.lab = lab;
  a.nxt = nxt;
  a.changed = changed;
  a.attach = attach;
  const dim3 grid((unsigned)(c->ct_n_pad / (CUTOFF_TILE * CUTOFF_WAVES)));
  const int64_t m_alloc = c->ct_m_alloc;

  if (n_core > 0) {
    if ((rc = ensure(c, c->db_rec, (size_t)m_alloc * sizeof(int32_t)))) return rc;
    a.lab_rec = (const int32_t*)c->db_rec.p;
    // 3. the rounds
    for (;;) {
      if (rounds >= N) return fail(c, KMVP_E_DEVICE, "DBSCAN: the labels did not settle within N rounds (they can only fall: a device fault?)");
      ++rounds;
      hipLaunchKernelGGL(db_round_begin_kernel, dim3(blocks_for(std::max(N, m_alloc))), tb, 0, c->stream, (const int32_t*)lab, a.smap32,
                         (int32_t*)c->db_rec.p, par, m_alloc, N, changed);
      HIP_TRY(c, hipGetLastError());
      HIP_TRY(c, hipEventRecord(c->ev[3], c->stream));
      hipError_t le = launch_label(D, LABEL_SWEEP, a, grid, c->stream, &c->last_kernel_name);
      if (le == hipErrorInvalidValue) return fail(c, KMVP_E_UNSUPPORTED, "DBSCAN: no label kernel instantiated for this D");
      HIP_TRY(c, le);
      HIP_TRY(c, hipEventRecord(c->ev[1], c->stream));
      ++walks;
      hipLaunchKernelGGL(db_hook_kernel, pts, tb, 0, c->stream, (const int32_t*)lab, (const int32_t*)nxt, par, N);
      HIP_TRY(c, hipGetLastError());
      hipLaunchKernelGGL(db_chase_kernel, pts, tb, 0, c->stream, (const int32_t*)par, lab, N);
      HIP_TRY(c, hipGetLastError());
      int32_t fell = 0;
      HIP_TRY(c, hipMemcpyAsync(&fell, changed, sizeof(fell), hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[3], c->ev[1]));
      walk_ms += ms;
      if (!fell) break;
    }
    // 4. the border walk, unless every point is a core point: lab_rec holds the fixed point (the last round changed nothing)
    if ((int64_t)n_core < N) {
      HIP_TRY(c, hipEventRecord(c->ev[3], c->stream));
      hipError_t le = launch_label(D, LABEL_BORDER, a, grid, c->stream, &c->last_kernel_name);
      if (le == hipErrorInvalidValue) return fail(c, KMVP_E_UNSUPPORTED, "DBSCAN: no label kernel instantiated for this D");
      HIP_TRY(c, le);
      HIP_TRY(c, hipEventRecord(c->ev[1], c->stream));
      ++walks;
    }
  }
  const bool border_ran = n_core > 0 && (int64_t)n_core < N;

  // 5. the renumbering and the outputs
  hipLaunchKernelGGL(db_flag_kernel, pts, tb, 0, c->stream, (const int32_t*)lab, flag, N);
  HIP_TRY(c, hipGetLastError());
  size_t need = 0;
  HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(nullptr, need, (const int32_t*)flag, cid, (int)N, c->stream));
  if ((rc = ensure(c, c->db_tmp, need))) return rc;
  need = c->db_tmp.cap;
  HIP_TRY(c, hipcub::DeviceScan::ExclusiveSum(c->db_tmp.p, need, (const int32_t*)flag, cid, (int)N, c->stream));
  hipLaunchKernelGGL(db_finish_kernel, pts, tb, 0, c->stream, (const int32_t*)lab, border_ran ? (const int32_t*)attach : nullptr,
                     (const int32_t*)flag, (const int32_t*)cid, d_labels, d_core_of, N, words);
  HIP_TRY(c, hipGetLastError());
  unsigned long long w[DBW_N];
  HIP_TRY(c, hipMemcpyAsync(w, words, sizeof(w), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(labels, d_labels, (size_t)N * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  if (core_of) HIP_TRY(c, hipMemcpyAsync(core_of, d_core_of, (size_t)N * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  if (counts) HIP_TRY(c, hipMemcpyAsync(counts, d_counts, (size_t)N * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipEventRecord(c->ev[2], c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (border_ran) {
    HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[3], c->ev[1]));
    walk_ms += ms;
  }
  c->last_kernel_ms = walk_ms;
  HIP_TRY(c, hipEventElapsedTime(&c->last_total_ms, c->ev[0], c->ev[2]));
  c->last_kernel_name = "lowd_cutoff_label_kernel";
  info[0] = (int64_t)w[DBW_CLUSTERS];
  info[1] = (int64_t)w[DBW_CORE];
  info[2] = (int64_t)w[DBW_BORDER];
  info[3] = (int64_t)w[DBW_NOISE];
  info[4] = rounds;
  info[5] = walks;
  return KMVP_OK;
}

}  // namespace

int dbscan_solve(kmvp_ctx* c, double radius, int64_t min_samples, int64_t* labels, int64_t* core_of, int64_t* counts, int64_t* info) {
  if (!c) return KMVP_E_INVALID;
  c->note.clear();
  if (!std::isfinite(radius) || !(radius > 0.0)) return fail(c, KMVP_E_INVALID, "DBSCAN: the radius must be finite and > 0");
  if (min_samples < 1) return fail(c, KMVP_E_INVALID, "DBSCAN: min_samples must be >= 1");
  if (!c->have_points) return fail(c, KMVP_E_INVALID, "DBSCAN: kmvp_set_points has not been called");
  if (!c->same_points)
    return fail(c, KMVP_E_INVALID, "DBSCAN: the points are clustered among themselves, the targets must be the sources (x == NULL at kmvp_set_points)");
  if (c->N > 0 && (!labels || !info)) return fail(c, KMVP_E_INVALID, "DBSCAN: a NULL output");
  HIP_TRY(c, hipSetDevice(c->device));
  int rc;
  if ((rc = cutoff_refuse(c, "DBSCAN"))) return rc;
  c->last_kernel_ms = c->last_total_ms = c->last_allreduce_ms = 0.f;
  if (c->N == 0) {
    if ((rc = cutoff_count_device(c, radius, nullptr))) return rc;
    if (info) memset(info, 0, 6 * sizeof(int64_t));
    c->last_kernel_name = "none";
    return KMVP_OK;
  }
  return c->dtype == KMVP_F64 ? dbscan_t<double>(c, radius, min_samples, labels, core_of, counts, info)
                              : dbscan_t<float>(c, radius, min_samples, labels, core_of, counts, info);
}

}  // namespace kmvp
