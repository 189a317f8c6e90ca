// Shared host-side state of libkmvp.so: the per-GPU context, small helpers and the
// functions the translation units call across each other.
//   kmvp_api.hip      the extern "C" surface of include/kmvp.h
//   kmvp_product.hip  layouts, launch geometry, the pair-loop paths and the policy that picks one
//   kmvp_solvers.hip  conjugate gradients, MINRES and the Lanczos quadrature on the product
//   kmvp_eigsh.hip    the top-k eigenpairs by Lanczos with full reorthogonalisation on the same operator
//   kmvp_sinkhorn.hip the Sinkhorn iteration of entropic optimal transport on the log-sum-exp
//   kmvp_kmeans.hip   Lloyd's k-means on the arg-K-min at K = 1
//   kmvp_meanshift.hip Gaussian mean-shift on the gradient of the log-sum-exp
//   kmvp_batch.hip    batched clouds: block-diagonal products and nearest neighbours on layouts of their own
//   kmvp_precond.hip  the pivoted-Cholesky preconditioner of conjugate gradients: build, apply, read-back
//   kmvp_cutoff.hip   cutoff-radius products and neighbour counts on a cell list, on layouts of their own
//   kmvp_dbscan.hip   DBSCAN on that cell list: core counts, label sweeps, border attachment
#pragma once
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>  // types only: the library is dlopen'ed on first use
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/kmvp.h"
#include "kmvp_internal.hpp"

namespace kmvp {

// which path's layouts the shared xs / rec buffers hold
enum : int { LAYOUT_LOWD = 0, LAYOUT_FAST = 1, LAYOUT_MFMA = 2, LAYOUT_CFAST = 3, LAYOUT_CELL = 4, LAYOUT_CELL64 = 5, LAYOUT_CELLMM = 6, LAYOUT_FASTMM = 7, LAYOUT_CFASTMM = 8 };

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
};

// RCCL entry points, resolved lazily so that single-GPU use never loads the library
struct Rccl {
  void* handle = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t,
                            hipStream_t) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;
  ncclResult_t (*CommUserRank)(const ncclComm_t, int*) = nullptr;
  ncclResult_t (*CommCuDevice)(const ncclComm_t, int*) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  std::string error, path;
  bool load() {
    if (handle) return true;
    // RCCL must drive the SAME HIP runtime as this library: a process may hold two ROCm
    // stacks (e.g. the system one and the copy bundled with PyTorch), and a bare
    // dlopen("librccl.so.1") returns whichever copy happens to be loaded already.  So look
    // next to the libamdhip64 this library is bound to first, by absolute path.
    std::vector<std::string> names;
    Dl_info info;
    if (dladdr((void*)&hipGetDeviceCount, &info) && info.dli_fname) {
      char resolved[4096];
      std::string hip_path = realpath(info.dli_fname, resolved) ? resolved : info.dli_fname;
      const size_t slash = hip_path.rfind('/');
      if (slash != std::string::npos) {
        const std::string dir = hip_path.substr(0, slash + 1);
        names.push_back(dir + "librccl.so.1");
        names.push_back(dir + "librccl.so");
      }
    }
    names.push_back("librccl.so.1");
    names.push_back("librccl.so");
    names.push_back("/opt/rocm/lib/librccl.so.1");
    for (const std::string& n : names) {
      handle = dlopen(n.c_str(), RTLD_NOW | RTLD_LOCAL);
      if (handle) {
        path = n;
        break;
      }
    }
    if (!handle) {
      error = std::string("cannot load librccl: ") + dlerror();
      return false;
    }
    GetUniqueId = (decltype(GetUniqueId))dlsym(handle, "ncclGetUniqueId");
    CommInitRank = (decltype(CommInitRank))dlsym(handle, "ncclCommInitRank");
    AllReduce = (decltype(AllReduce))dlsym(handle, "ncclAllReduce");
    CommDestroy = (decltype(CommDestroy))dlsym(handle, "ncclCommDestroy");
    GetErrorString = (decltype(GetErrorString))dlsym(handle, "ncclGetErrorString");
    CommCount = (decltype(CommCount))dlsym(handle, "ncclCommCount");
    CommUserRank = (decltype(CommUserRank))dlsym(handle, "ncclCommUserRank");
    CommCuDevice = (decltype(CommCuDevice))dlsym(handle, "ncclCommCuDevice");
    if (!GetUniqueId || !CommInitRank || !AllReduce || !CommDestroy || !GetErrorString || !CommCount || !CommUserRank ||
        !CommCuDevice) {
      error = "librccl lacks an expected symbol";
      return false;
    }
    return true;
  }
};extern Rccl g_rccl;

}  // namespace kmvp

struct kmvp_ctx {
  using DevBuf = kmvp::DevBuf;
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // product start, pair loop end, end; all-reduce start, end
  std::string err;

  // problem
  int dtype = -1;
  int D = 0, E = 0;
  int64_t M = 0, N = 0, j_offset = 0, m_total = 0;
  bool same_points = false;
  bool have_points = false, have_signal = false, density = false;
  bool async_product = false;   // solvers: run_product() leaves the result on the stream, no host synchronisation
  // solvers: A = K + ridge I + diag(d) (kmvp_set_solver_diagonal).  diag_n > 0: sdiag holds ridge + d_i; else the scalar
  bool diag_on = false;
  int64_t diag_n = 0;
  double diag_ridge = 0.0, diag_min = 0.0;  // diag_min: the smallest ridge + d_i (CG refuses a negative one)

  DevBuf y_raw, x_raw, b_raw;   // caller's arrays in the working precision
  DevBuf xs, rec;               // kernel layouts (specialised path; bf16 path: augmented targets, tile images)
  DevBuf partd;                 // bf16 path: partial denominators
  DevBuf aux;                   // cloud centre, squared radius, half-widths (fast_center_kernel)
  DevBuf sortbuf, perm;         // centred path: radix-sort scratch, Morton order of the sources
  DevBuf x_scaled, y_scaled;    // scaled copies (generic path)
  // cell-reduced Gaussian path (kmvp_cell.hpp): cell order of targets / sources, their tiles
  // ([start][count][key] per tile), slot of every target in cell order, target tile centres,
  // segment-reduced sums in cell order
  DevBuf cell_tperm, cell_sperm, cell_tgrp, cell_sgrp, cell_slot, cell_tmeta, cell_sums, cell_skey, cell_scentre, cell_scale;
  DevBuf cell_tcentre, cell_scentre32;  // count-cut cells: [cell][4] float centres of the targets' / the sources' cells (same_points: the sources' serve both)
  DevBuf part, sums, out;       // fp64 partials, reduced sums, final (N,E)
  DevBuf xchg;                  // sharded runs: sums in the canonical unpadded layout [column][N] for the all-reduce
  DevBuf kexp, kshift, xchgk;   // exp(<x,y>): exponents per (segment, target) / per target / per target after the all-reduce(min)
                                // (log-sum-exp: kshift and xchgk per (column, target); xchgk holds the rank's own and the common ones)
  DevBuf kflag;                 // exp(<x,y>): set when a row's exponent reached the shift's clamp (check_shift_range_kernel)
  DevBuf scratch;               // CG vectors / dot products
  DevBuf knn;                   // kmvp_nearest: (N, K) int64 indices, then (N, K) float64 squared distances
  DevBuf sdiag;                 // solvers: the effective diagonal ridge + d_i, N doubles (kmvp_set_solver_diagonal)
  // conjugate gradients' pivoted-Cholesky preconditioner (kmvp_set_solver_preconditioner; layout: kmvp_precond.hip)
  DevBuf precond;               // residual diagonal, 1 / (ridge + d_i), the factor L [rank][N], pivots, Gram matrix and its factor
  int precond_rank = 0;         // as requested: 0 = off
  int pc_built = 0;             // columns the factor in `precond` holds (<= pc_rank)
  int pc_used = 0;              // columns the last kmvp_<kernel>_cg_solve or _lanczos_quadrature_precond applied (0: it ran unpreconditioned)
  int pc_kernel = -1, pc_rank = 0;  // what the factor was built for, with the versions below (pc_points_ver 0: no factor)
  uint64_t pc_points_ver = 0, pc_diag_ver = 0;
  uint64_t diag_ver = 0;        // counts kmvp_set_solver_diagonal
  float last_precond_ms = 0.f;  // the build inside the last kmvp_<kernel>_cg_solve or _lanczos_quadrature_precond (0: reused, or off)
  double pc_logdet_c = 0.0;     // log det (I + L' D^-1 L) of the factor in `precond`, from its Cholesky factor (pc_logdet)
  // Sinkhorn (kmvp_sinkhorn.hip): layouts of its own for both directions -- target image of x with records of y, target
  // image of y with records of x (the record's signal slot carries potential + log-weight) -- and the fp64 state
  DevBuf sk_xs_x, sk_rec_y, sk_xs_y, sk_rec_x, sk_state;
  uint64_t sk_points_ver = 0;   // points version the four layouts were packed from (0: none)
  // k-means (kmvp_kmeans.hip): the target image of the points, the centroid records, the workgroups' partial sums of the
  // centroid update, and the fp64 state (centroids, cluster sums, weights, labels, state words)
  DevBuf km_xs, km_rec, km_part, km_state;
  uint64_t km_points_ver = 0;   // points version km_xs was packed from (0: none)
  // mean-shift (kmvp_meanshift.hip): the moving target image of the active points, the fp64 state (positions, step2, the
  // state words, iters, the two index lists, the keep flags) and the scratch of the stream compaction
  DevBuf ms_xs, ms_state, ms_tmp;
  // batched clouds (kmvp_set_batches; kmvp_batch.hip): the plan's tile table and its two index maps, and layouts of their
  // own -- the target image over the padded slots and the source records of all ranges
  DevBuf bt_tiles, bt_tmap, bt_smap, bt_xs, bt_rec;
  bool bt_on = false;           // batches are set: the products and kmvp_nearest are block-diagonal, the rest is refused
  int bt_B = 0;
  int64_t bt_n_pad = 0, bt_m_alloc = 0;  // target slots and records of the plan
  uint64_t bt_ver = 0;          // counts accepted kmvp_set_batches calls with B > 0
  uint64_t bt_xs_points_ver = 0, bt_xs_ver = 0;    // points / plan version bt_xs was packed from (0: none)
  uint64_t bt_rec_points_ver = 0, bt_rec_ver = 0;  // the same for the coordinates in bt_rec, laid out for records of
  int bt_rec_R = 0;                                // bt_rec_R reals
  uint64_t bt_sig_ver = 0;      // signal version the records' signal slots hold (0: none), of
  int bt_sig_EB = -1;           // bt_sig_EB columns
  std::vector<int64_t> bt_y_off, bt_x_off;  // the accepted offsets (B + 1 each): the batched Sinkhorn plans its second direction from them
  // batched Sinkhorn (kmvp_sinkhorn_batched.hip): both directions' plans (tile tables in a pristine and a working copy,
  // tile-to-batch maps, tile ranges, index maps), their target images and records, and the fp64 state
  DevBuf skb_plan, skb_xs, skb_rec, skb_state;
  uint64_t skb_points_ver = 0, skb_bt_ver = 0;  // points / plan version the layouts were built and packed from (0: none)
  // cutoff radius (kmvp_<kernel>_cutoff, kmvp_radius_count; kmvp_cutoff.hip): the cell-list plan's tile and run tables and
  // its two index maps, and layouts of their own -- the target image over the padded slots and the source records
  DevBuf ct_tiles, ct_runs, ct_tmap, ct_smap, ct_xs, ct_rec;
  double opt_cutoff_factor = 1.0;  // "cutoff_cell_factor": the cells' side in units of the radius (>= 1)
  uint64_t ct_ver = 0;             // counts the plans built
  uint64_t ct_plan_points_ver = 0, ct_radius_bits = 0;  // what the plan in ct_* was built for (ct_plan_points_ver 0: none),
  double ct_factor = 0.0;                               // with this factor
  int64_t ct_n_pad = 0, ct_m_alloc = 0;  // target slots and records of the plan
  uint64_t ct_xs_ver = 0, ct_rec_ver = 0;  // plan version ct_xs / the coordinates in ct_rec were packed from (0: none), the
  int ct_rec_R = 0;                        // records laid out for ct_rec_R reals
  uint64_t ct_sig_ver = 0;      // signal version the records' signal slots hold (0: none), of
  int ct_sig_EB = -1;           // ct_sig_EB columns
  int64_t ct_info[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // kmvp_cutoff_info
  DevBuf ct_smap32;             // kmvp_radius_nearest: ct_smap narrowed to int32, what its kernel reads through the scalar cache,
  uint64_t ct_smap32_ver = 0;   // made from the plan of this version (0: none)
  int opt_cutoff_plan = 0;      // "cutoff_plan": 0 the plan is built on the host, 1 on the device (kmvp_cutoff_plan_device.hip)
  int ct_plan_opt = 0;          // ... the value the plan in ct_* was built under: part of its cache key
  int ct_built_on = 0;          // the side that built it (0 host, 1 device), and what kmvp_cutoff_plan_read reports beyond
  double ct_grid[4] = {0.0, 0.0, 0.0, 0.0};  // ct_info: lo[3] and h,
  int64_t ct_tiles_n = 0;                    // the tiles of the table (fillers included)
  DevBuf ct_work;               // the device build's keys, sorted clouds, scans and hipcub's scratch: nothing survives a build
  // DBSCAN (kmvp_dbscan.hip): the per-point state (counts, labels, the round's arrays, the outputs, the state words), the
  // labels in record order that the pair loop reads beside the records, and hipcub's scratch of the renumbering scan
  DevBuf db_state, db_rec, db_tmp;
  double ct_solve_radius = 0.0;  // kmvp_wendland_<c>_cg_solve: the support radius cg_apply's operator runs at (0: no such solve is running)
  uint64_t points_ver = 0, signal_ver = 0;
  // what xs / rec / scaled copies currently hold
  int packed_layout = -1;  // LAYOUT_* of the path that owns xs / rec right now
  int packed_kernel = -1, packed_sig = -1, packed_T = -1;
  uint64_t packed_points_ver = 0, packed_signal_ver = 0;
  int gen_kernel = -1;
  uint64_t gen_points_ver = 0;
  int64_t out_n = 0;
  int out_e = 0;

  // tuning (kmvp_set_option)
  int opt_feed = -1, opt_T = 0, opt_segments = 0, opt_chunk = 512;
  int opt_fast = -1, opt_fast_tiles = 0;  // fast_sqdists: -1 auto, 0 never, 1 always, 2 always the centred form, 3 always the cell form
  int opt_cellmm_shape = -1;              // cellmm_kernel's MFMA shape: 0 = 32x32x16, 1 = 16x16x32 (cellmm16_kernel), -1 = by size
  int opt_cell_shared_build = -1;         // cellmm16_kernel's one-cell workgroups build each source operand once: -1 / 1 = where the kernel holds that body (cell_shared_build), 0 = never
  int opt_cell_balance = -1;              // float32 cell lists: lattice columns cut along z by point count: -1 = where it applies at the sizes cellmm16_kernel is taken by itself, 1 = wherever it applies (cell_balance_applies), 0 = never
  int opt_cell_fused = -1;                // cellmm16_kernel's two tile lists: -1 / 1 = one launch where it applies (fused_cell_grid), 0 = two launches
  int opt_cell_tail = -1;                 // cellmm16_kernel's fused grid: the MAIN list's last, partial round in short segments (the TAIL list, cell_tail_split): -1 = automatic (cell_tail_taken), 0 = never, 1 = wherever it applies
  int opt_cell_tail_resident = 0;         // resident workgroups the TAIL plan assumes: 0 = two per CU of the device; > 0 = this many (tests)
  int device_cus = 0;                     // compute units of the device (kmvp_create)
  int64_t cell_list_info[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // the lists of the last product on cellmm_kernel / cellmm16_kernel: kmvp_cell_lists
  int opt_mfma_variant = -1;              // bf16 path: VAR of mfma_pipe_kernel (kmvp_mfma.hpp); -1 = by kernel
  int opt_meanshift_compact = -1;         // mean-shift: -1 / 1 = the active list is compacted after every sweep, 0 = never (frozen lanes ride along)
  int opt_sinkhorn_retire = -1;           // batched Sinkhorn: -1 / 1 = the tiles of stopped batches are retired (len = 0), 0 = never (stopped batches ride along)
  int opt_same_global = 0;               // the targets ARE the (unsharded) sources although x was passed explicitly
  int opt_partial = 0;                    // a source slice (M < M_total) may run WITHOUT a communicator: the caller sums the shards
  uint64_t perm_ver = 0;                  // points version the Morton order belongs to
  uint64_t cell_ver = 0;                  // points version the cell structures belong to
  int cell_state = 0;                     // for cell_ver: 0 not examined, 1 built, -1 the path does not apply
  int cell_balance_req = -1;              // the "cell_balance" option the cell structures were built under
  bool cell_balanced = false;             // the cells are count-cut (tile keys are cell ids, centres come from the tables)
  float cell_zw = 0.f;                    // count-cut cells: the cap on a cell's width along z
  int cell_tt = 0, cell_tt_req = 0;       // target tiles per wavefront the target tile list was padded for; as requested (0 = auto)
  float cell_lo[3] = {0.f, 0.f, 0.f}, cell_hh[3] = {1.f, 1.f, 1.f};  // grid origin and cell sides per axis
  int cell_g[3] = {1, 1, 1};
  int64_t cell_n_tiles = 0, cell_m_tiles = 0;  // tiles of 32 (targets: both lists, padded to workgroups / sources)
  int64_t cell_n_main = 0, cell_n_rest = 0;    // float32 cell kernels: target tiles in groups of cell_tt / leftover tiles in groups of 2
  float cloud_radius2 = INFINITY;          // squared half-diagonal of the clouds' bounding box
  uint64_t centre_ver = 0;

  // sharding
  ncclComm_t comm = nullptr;
  int rank = 0, world = 1;
  // rehearsal transport (kmvp_comm_init_host): the same exchange staged through host memory and summed by a callback
  kmvp_host_allreduce_fn host_xchg = nullptr;
  void* host_user = nullptr;
  std::vector<double> host_buf;
  bool exchanges() const { return comm != nullptr || host_xchg != nullptr; }

  int comm_count = 1;                      // ranks the RCCL communicator itself reports (ncclCommCount)
  float last_kernel_ms = 0.f, last_total_ms = 0.f, last_allreduce_ms = 0.f;
  const char* last_kernel_name = "";
  std::string note;  // why the last product did not take a faster form ("" when it did): kmvp_last_dispatch_note
};

namespace kmvp {

int fail(kmvp_ctx* c, int code, const std::string& msg);
const char* create_error();

#define HIP_TRY(c, expr)                                                                     \
  do {                                                                                       \
    hipError_t e_ = (expr);                                                                  \
    if (e_ != hipSuccess)                                                                    \
      return kmvp::fail((c), e_ == hipErrorOutOfMemory ? KMVP_E_NOMEM : KMVP_E_DEVICE,       \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                  \
  } while (0)

inline size_t elem_size(int dtype) { return dtype == KMVP_F64 ? 8 : 4; }
inline unsigned blocks_for(int64_t n, int threads = 256) { return (unsigned)((n + threads - 1) / threads); }

int ensure(kmvp_ctx* c, DevBuf& b, size_t bytes);  // grow-only device buffer
void release(DevBuf& b);

// What the shared xs / rec buffers hold: the layout of one path for one kernel and T (targets per lane or tiles per
// wavefront, and whatever else the layout depends on), packed from one version of the points, and -- the signal image --
// from one version of the signal for one product kind `sig` (-1: an image that is not reusable as it is).
struct PackKey {
  int layout, kernel, T;
};
inline bool points_stale(const kmvp_ctx* c, PackKey k) {
  return c->packed_points_ver != c->points_ver || c->packed_kernel != k.kernel || c->packed_layout != k.layout ||
         c->packed_T != k.T;
}
inline bool signal_stale(const kmvp_ctx* c, PackKey k, int sig) {
  return points_stale(c, k) || sig < 0 || c->packed_signal_ver != c->signal_ver || c->packed_sig != sig;
}
inline void record_packed(kmvp_ctx* c, PackKey k, int sig) {
  c->packed_points_ver = c->points_ver;
  c->packed_signal_ver = c->signal_ver;
  c->packed_layout = k.layout;
  c->packed_kernel = k.kernel;
  c->packed_T = k.T;
  c->packed_sig = sig;
}

// kmvp_product.hip: the product a = K b [/ K 1] with everything query() times, and the
// bounding box of the freshly uploaded clouds (asynchronous on the context's stream)
int run_product(kmvp_ctx* c, int kernel, bool normalise);
int measure_clouds(kmvp_ctx* c, int dtype, int64_t M, int64_t N, int D);
int prepare_points(kmvp_ctx* c, int kernel);  // kmvp_fit: whatever can be built from the points alone
int run_gradient(kmvp_ctx* c, int kernel);    // kmvp_<kernel>_grad: (N, E D) into c->out, synchronous
int run_dscale(kmvp_ctx* c, int kernel);      // kmvp_<kernel>_dscale: (N, E D) into c->out, synchronous
int run_logsumexp(kmvp_ctx* c, int kernel);   // kmvp_<kernel>_logsumexp: (N, E) into c->out, synchronous
int run_logsumexp_grad(kmvp_ctx* c, int kernel);  // kmvp_<kernel>_logsumexp_grad: (N, E D) into c->out, synchronous
int run_nearest(kmvp_ctx* c, int K, int exclude_self, int64_t* out_idx, double* out_sqdist);  // kmvp_nearest: synchronous, into the caller's arrays

// The solver's diagonal (kmvp_set_solver_diagonal) as the kernels take it: dg[i] = ridge + d_i per point, or nullptr and the
// scalar.  Both are fixed for a whole solve, so a captured burst stays valid.
struct Diag {
  const double* dg;
  double ridge;
  __device__ __forceinline__ double at(int64_t i) const { return dg ? dg[i] : ridge; }
};
inline Diag solver_diag(const kmvp_ctx* c) { return Diag{c->diag_n ? (const double*)c->sdiag.p : nullptr, c->diag_ridge}; }

// kmvp_precond.hip: P = L L' + D, L the rank-R pivoted Cholesky factor of the kernel matrix and D the solver's diagonal
// Builds the factor for (points, kernel, rank, diagonal) unless the context holds it; c->pc_built columns afterwards.
int precond_prepare(kmvp_ctx* c, int kernel);
constexpr int PC_APPLY_BLOCKS = 256;  // workgroups of the apply's first launch
// doubles of scratch one apply needs for E columns: the partial sums of L' D^-1 r, then w = C^-1 (L' D^-1 r)
inline size_t precond_scratch(int R, int E) { return (size_t)(PC_APPLY_BLOCKS + 1) * (size_t)R * (size_t)E; }
// z = P^-1 r for the (N, E) row-major r, and rz_partial[block][e] = the block's share of r . z (cg_dot_kernel's layout for
// `rz_blocks` workgroups of 256).  Three launches on the context's stream; nothing once *stop != 0.
void precond_apply(kmvp_ctx* c, const double* r, double* z, int E, double* scratch, double* rz_partial, int rz_blocks,
                   const double* stop);
// The probes of the preconditioned quadrature, z[i][e] = sqrt(D_i) g[i][e] + sum_t L[t][i] h[t][e] (t ascending over the
// columns built, one fma per term) for the device arrays g (N, P) and h (rank', P); one launch on the context's stream.
void precond_probes(kmvp_ctx* c, const double* g, const double* h, int P, double* z);
constexpr int PC_LOGD_BLOCKS = 64;  // workgroups of the partial sums of log D_i
// out[PC_LOGD_BLOCKS] = sum_i log D_i, the partial sums out[0 .. PC_LOGD_BLOCKS) added in workgroup order; two launches
void precond_logdiag(kmvp_ctx* c, double* out);
// kmvp_get_solver_preconditioner
int precond_read(kmvp_ctx* c, int* rank_built, int64_t* pivots, double* factor);

// kmvp_product.hip: kmvp_cell_layout, the cell structures the last product on the cell form ran on, read back
int cell_layout_read(kmvp_ctx* c, int64_t* info, double* sigma_b, int32_t* source_cell, int32_t* target_cell,
                     double* source_centres, int64_t source_cap, double* target_centres, int64_t target_cap);
int cell_lists_read(kmvp_ctx* c, int64_t* info, int32_t* target_list);  // kmvp_cell_lists

// kmvp_solvers.hip
int cg_solve(kmvp_ctx* c, int kernel, const void* a_host, int E, double rtol, int maxit, double* out_b,
             int* iters, double* resid);
int minres_solve(kmvp_ctx* c, int kernel, const void* a_host, int E, double rtol, int maxit,
                 double* out_b, int* iters, double* resid);
int cg_lanczos(kmvp_ctx* c, int kernel, const void* z_host, int P, double rtol, int maxit, double* logquad, double* invquad,
               int* steps, double* x_out, double* alpha_out, double* beta_out);
int cg_lanczos_precond(kmvp_ctx* c, int kernel, const double* g_host, const double* h_host, int P, double rtol, int maxit,
                       double* logdet_p, double* logquad, double* invquad, double* wnorm2, int* steps, double* x_out,
                       double* pz_out, double* alpha_out, double* beta_out);
// One solve's scratch block: `nvec` Krylov vectors of N x E doubles, the dot products' partial sums, then
// the device-resident iteration's state, with its stop word at `stop` and the iteration count after it, then `extra`
// doubles of the solver's own (cg_lanczos: the coefficient history).
struct Krylov {
  int64_t m = 0;  // length of the Krylov vectors: all points
  int E = 0;
  size_t n = 0;  // m * E
  size_t stop = 0;
  double *vecs = nullptr, *partial = nullptr, *state = nullptr;
  double* vec(int i) const { return vecs + (size_t)i * n; }
};
// However a solve ends, the product is synchronous again and no signal is left behind: b_raw held the
// right-hand side and the Krylov vectors, not what kmvp_set_signal uploaded.
struct SolveGuard {
  kmvp_ctx* c;
  ~SolveGuard() { c->async_product = false; c->have_signal = false; }
};
// What the eigen-solver (kmvp_eigsh.hip) shares with the solvers: the shape check (targets == sources, sharded or not) and
// the operator, K applied to the device-resident (N, k.E) float64 block v, the result in c->out (of `k` it reads E and n).
int solver_shape(kmvp_ctx* c);
int cg_apply(kmvp_ctx* c, int kernel, const double* v, const Krylov& k);

// kmvp_eigsh.hip: kmvp_<kernel>_eigsh, the device-resident Lanczos process with full reorthogonalisation
int eigsh_solve(kmvp_ctx* c, int kernel, int k, int op, const double* v0, double tol, int maxit, double* eigenvalues,
                double* eigenvectors, double* resid, int* steps, double* alpha_out, double* beta_out, double* degree_out);

// kmvp_sinkhorn.hip: kmvp_<kernel>_sinkhorn, the device-resident Sinkhorn iteration on lowd_lse_kernel
int sinkhorn_solve(kmvp_ctx* c, int kernel, const double* log_a, const double* log_b, double tol, int maxit, double* u,
                   double* v, int* iters, double* err);

// kmvp_kmeans.hip: kmvp_kmeans, the device-resident Lloyd iteration on lowd_knn_kernel<D, 1>
int kmeans_solve(kmvp_ctx* c, int C, const double* weights, double tol, int maxit, double* centroids, int64_t* labels,
                 double* cluster_weight, int* iters, double* inertia, double* shift);

// kmvp_batch.hip: batched clouds (kmvp_set_batches) -- the plan, the gather-packed layouts, the block-diagonal product
// and nearest neighbours on lowd_batch_kernel / lowd_batch_knn_kernel.  batches_refuse: KMVP_OK with batches off, else
// KMVP_E_UNSUPPORTED with a message that names `what` and the batches (the entries that are not built for them).
int set_batches(kmvp_ctx* c, int B, const int64_t* y_offsets, const int64_t* x_offsets_or_null);
int run_product_batched(kmvp_ctx* c, int kernel, bool normalise);
int run_nearest_batched(kmvp_ctx* c, int K, int exclude_self, int64_t* out_idx, double* out_sqdist);
int batches_refuse(kmvp_ctx* c, const char* what);
// What the batched entries are not built for, beyond their own arguments (bfloat16, D > 8, an explicit fast_sqdists, a
// communicator, a source slice): KMVP_E_UNSUPPORTED with a message that `what` opens, else KMVP_OK.
int batched_unsupported(kmvp_ctx* c, const std::string& what);

// kmvp_sinkhorn_batched.hip: kmvp_<kernel>_sinkhorn_batched, one Sinkhorn solve per batch on lowd_batch_lse_kernel
int sinkhorn_batched_solve(kmvp_ctx* c, int kernel, const double* log_a, const double* log_b, double tol, int maxit, double* u,
                           double* v, int* iters, double* err, int* status);

// kmvp_cutoff.hip: kmvp_<kernel>_cutoff, kmvp_radius_count and kmvp_cutoff_info -- the cell-list plan
// (kmvp_cutoff_plan.hpp), the gather-packed layouts, lowd_cutoff_kernel / lowd_cutoff_count_kernel
int run_cutoff(kmvp_ctx* c, int kernel, double radius, bool normalise);
// kmvp_<kernel>_cutoff_grad: the gradient with respect to the targets on the same plan and packs, lowd_cutoff_grad_kernel
int run_cutoff_grad(kmvp_ctx* c, int kernel, double radius);
int radius_count(kmvp_ctx* c, double radius, int exclude_self, int64_t* counts);
// kmvp_radius_nearest: the K nearest sources inside the radius on the same plan and the count's packs, lowd_cutoff_knn_kernel
int radius_nearest(kmvp_ctx* c, double radius, int K, int exclude_self, int64_t* out_idx, double* out_sqdist);
int cutoff_info(kmvp_ctx* c, int64_t* out);
// kmvp_cutoff_plan_read: the plan of the last cutoff call from the device buffers the kernels read
int cutoff_plan_read(kmvp_ctx* c, int64_t* sizes, double* grid, int64_t* tiles, int64_t* runs, int64_t* tmap, int64_t* smap);
// kmvp_cutoff_plan_device.hip: the plan for (points, radius, "cutoff_cell_factor") built on c->stream into ct_tiles, ct_runs,
// ct_tmap and ct_smap, and what cutoff_prepare keeps of it.  *fits false: nothing was built, the cloud is beyond the build's
// 32-bit keys and indices (kmvp_cutoff_plan_device.hpp cutoff_device_fits).
struct CutoffBuilt {
  int64_t g[3];
  double lo[3], h;
  int64_t n_pad, m_pad, m_alloc, live_tiles, walked, tiles, runs;
};
int cutoff_plan_device(kmvp_ctx* c, double radius, CutoffBuilt* out, bool* fits);
// kmvp_wendland_<c>_cg_solve: the checks, the plan and the packed layouts, then cg_solve with cutoff_apply as its operator
int wendland_cg_solve(kmvp_ctx* c, int kernel, double radius, const void* a_host, int E, double rtol, int maxit, double* out_b,
                      int* iters, double* resid);
// cg_apply's operator for the Wendland kernels: the E signal slots of the records straight from the float64 (M, E) vector v,
// then the pair loop into c->out -- two launches.  While c->async_product is set: no event, no synchronisation, no host check.
int cutoff_apply(kmvp_ctx* c, int kernel, const double* v, int E);

// kmvp_cutoff.hip, for kmvp_dbscan.hip: kmvp_radius_count's refusals under the name `what`; and its setup and walk -- the
// cached plan, the target image, the density-layout records, ct_smap32, then lowd_cutoff_count_kernel into the device
// array `counts` (N values) between ev[3] and ev[1], left on the stream.  N == 0: the plan alone.
int cutoff_refuse(kmvp_ctx* c, const std::string& what);
int cutoff_count_device(kmvp_ctx* c, double radius, int64_t* counts);
// kmvp_dbscan.hip: kmvp_dbscan, density clustering on the cell list -- the count, then sweeps of lowd_cutoff_label_kernel
// with an integer hook-and-chase step between them, one border walk and the renumbering, all resident on the device
int dbscan_solve(kmvp_ctx* c, double radius, int64_t min_samples, int64_t* labels, int64_t* core_of, int64_t* counts, int64_t* info);

// kmvp_meanshift.hip: kmvp_gaussian_meanshift, the device-resident mean-shift iteration on lowd_lse_grad_kernel
int meanshift_solve(kmvp_ctx* c, double tol, int maxit, double* modes, int* iters, double* step2, int* sweeps,
                    int64_t* target_sweeps);

}  // namespace kmvp
