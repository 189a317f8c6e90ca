// Krylov solvers for K b = a with the on-the-fly product as the operator: conjugate
// gradients (SPD Gaussian / exp(-r) matrices) and MINRES (symmetric indefinite
// inverse-distance matrix).  The reference solves densely with lstsq (bruteforce.py:205-207);
// parity is judged on the residual.
// With kmvp_set_solver_diagonal the operator of both is A = K + ridge I + diag(d): the product is untouched, the
// diagonal term is added to K v by the first kernel that consumes it (the *_diag_* variants below).
// cg_lanczos is conjugate gradients once more, for its coefficients rather than its iterate: every column on its own
// clock, the step lengths of every iteration kept, and the Gauss quadrature of log on them (kmvp_quadrature.hpp).
#include <cstdlib>

#include "kmvp_ctx.hpp"
#include "kmvp_quadrature.hpp"

namespace kmvp {

// ------------------------------------------------------------------------------------
// conjugate gradients on K b = a with the on-the-fly product as the operator

constexpr int CG_BLOCKS = 256;

// The system matrix is K(y, y) on ALL points.  Single GPU: x == y (x_or_null = NULL).  Sharded:
// every rank holds all points as targets and its slice of them as sources
// (same_points_global, N == M_total), and a communicator is attached.
int solver_shape(kmvp_ctx* c) {
  if (c->same_points && c->world == 1) return KMVP_OK;
  if (c->world > 1 && !c->exchanges()) return fail(c, KMVP_E_INVALID, "sharded solver without kmvp_comm_init");
  const bool sharded_square = c->opt_same_global && c->N == c->m_total && c->j_offset + c->M <= c->m_total &&
                             (c->world > 1 || c->M == c->m_total);  // one rank must hold every source
  if (c->same_points && c->world > 1)
    return fail(c, KMVP_E_INVALID, "sharded solver: pass all points as targets and this rank's slice as sources");
  if (!sharded_square) return fail(c, KMVP_E_INVALID, "the solver needs x == y (pass x_or_null = NULL)");
  return KMVP_OK;
}

// partial[block][e] = sum over the block's rows of u[i][e] * v[i][e]
__global__ void cg_dot_kernel(const double* __restrict__ u, const double* __restrict__ v, int64_t m,
                              int E, double* __restrict__ partial) {
  __shared__ double red[256];
  for (int e = 0; e < E; ++e) {
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m;
         i += (int64_t)gridDim.x * blockDim.x)
      acc += u[i * E + e] * v[i * E + e];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) partial[(int64_t)blockIdx.x * E + e] = red[0];
    __syncthreads();
  }
}

// CG's first consumer of K p with the diagonal on: Ap[i][e] += diag_i p[i][e] in place (Ap = K p on entry, the full
// replicated vector after the all-reduce), and partial[block][e] = sum of p . Ap in the same sweep -- the layout of
// cg_dot_kernel, so cg_scalars_kernel reads it unchanged.
__global__ void cg_diag_dot_kernel(const double* __restrict__ p, double* __restrict__ Ap, Diag diag, int64_t m, int E,
                                   double* __restrict__ partial) {
  __shared__ double red[256];
  for (int e = 0; e < E; ++e) {
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m;
         i += (int64_t)gridDim.x * blockDim.x) {
      const double pv = p[i * E + e];
      const double av = Ap[i * E + e] + diag.at(i) * pv;
      Ap[i * E + e] = av;
      acc += pv * av;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) partial[(int64_t)blockIdx.x * E + e] = red[0];
    __syncthreads();
  }
}

template <typename real>
__global__ void cg_cast_kernel(const double* __restrict__ in, real* __restrict__ out, int64_t n) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q < n) out[q] = (real)in[q];
}
template <typename real>
__global__ void cg_widen_kernel(const real* __restrict__ in, double* __restrict__ out, int64_t n) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q < n) out[q] = (double)in[q];
}
// out = a - K x: the right-hand side as uploaded (working precision), widened, minus the product
template <typename real>
__global__ void residual_kernel(const real* __restrict__ a, const double* __restrict__ Kx, double* __restrict__ out,
                                int64_t n) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q < n) out[q] = (double)a[q] - Kx[q];
}

// out = a - (K x + diag x): the residual of the regularised system
template <typename real>
__global__ void residual_diag_kernel(const real* __restrict__ a, const double* __restrict__ Kx, const double* __restrict__ x,
                                     Diag diag, double* __restrict__ out, int64_t n, int E) {
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q < n) out[q] = (double)a[q] - (Kx[q] + diag.at(q / E) * x[q]);
}

// Sum of the CG_BLOCKS partials of column e by the whole block (fixed tree order: deterministic).
// A single thread walking the 256 partials took ~9 us per call; this takes ~2.
__device__ __forceinline__ double block_sum_partials(const double* __restrict__ partial, int E, int e, double* red) {
  red[threadIdx.x] = threadIdx.x < CG_BLOCKS ? partial[(int64_t)threadIdx.x * E + e] : 0.0;
  __syncthreads();
  for (int s2 = CG_BLOCKS / 2; s2 > 0; s2 >>= 1) {
    if ((int)threadIdx.x < s2) red[threadIdx.x] += red[threadIdx.x + s2];
    __syncthreads();
  }
  const double v = red[0];
  __syncthreads();
  return v;
}

constexpr int CG_CHECK = 8;  // iterations between two looks at the residual on the host
constexpr int CG_GRAPH_AFTER = 64;  // bursts (512 iterations) before the burst is captured into a hipGraph

// One block.  mode 1: pAp[e] = sum of the partials -> alpha[e] = rs_old[e] / pAp[e];
// mode 2: rs_new[e] = sum -> beta[e] = rs_new[e] / rs_old[e], rs_old[e] = rs_new[e], iteration count + 1,
// and the stopping test max_e sqrt(rs_new / |a|^2) <= rtol: once it holds, `stop` is set and every
// later kernel of the burst returns at once, so the iterate the host reads is the one of the FIRST
// iteration that met the tolerance (the residual of an ill-conditioned system does not fall
// monotonically: at config 5 it meets 1e-6 at iteration 132 and not again before 240).
// scal = [rs_old | alpha | beta | |a|^2] x E, then stop, iterations.  Partials are added in block
// order, as the host would.
__global__ void __launch_bounds__(CG_BLOCKS) cg_scalars_kernel(const double* __restrict__ partial,
                                                              double* __restrict__ scal, int E, int mode,
                                                              double rtol) {
  __shared__ double red[CG_BLOCKS];
  double* stop = scal + 4 * E;
  if (*stop != 0.0) return;  // uniform: every thread reads the same word
  bool not_met = false;
  for (int e = 0; e < E; ++e) {
    const double v = block_sum_partials(partial, E, e, red);
    if (threadIdx.x != 0) continue;
    const double rs_old = scal[e];
    if (mode == 1) {
      scal[E + e] = (v != 0.0 && rs_old > 0.0) ? rs_old / v : 0.0;
    } else {
      scal[2 * E + e] = rs_old > 0.0 ? v / rs_old : 0.0;
      scal[e] = v;
      const double a2 = scal[3 * E + e];
      if (a2 > 0.0 && !(sqrt(v / a2) <= rtol)) not_met = true;  // NaN / inf: not met
    }
  }
  if (mode == 2 && threadIdx.x == 0) {
    scal[4 * E + 1] += 1.0;
    if (!not_met) *stop = 1.0;
  }
}

// x += alpha p ; r -= alpha Ap
__global__ void cg_update_xr_kernel(double* __restrict__ x, double* __restrict__ r, const double* __restrict__ p,
                                    const double* __restrict__ Ap, const double* __restrict__ scal, int64_t m,
                                    int E) {
  if (scal[4 * E] != 0.0) return;  // stopped
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= m * E) return;
  const double a = scal[E + q % E];
  x[q] = x[q] + a * p[q];
  r[q] = r[q] + (-a) * Ap[q];
}

// p = r + beta p
__global__ void cg_update_p_kernel(double* __restrict__ p, const double* __restrict__ r,
                                   const double* __restrict__ scal, int64_t m, int E) {
  if (scal[4 * E] != 0.0) return;  // stopped
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= m * E) return;
  p[q] = r[q] + scal[2 * E + q % E] * p[q];
}

// ------------------------------------------------------------------------------------
// host side shared by both solvers

// (Krylov, the solve's scratch block, and SolveGuard: kmvp_ctx.hpp, shared with the eigen-solver.)

// The checks both solvers make, the device, and the scratch layout.
static int solver_begin(kmvp_ctx* c, const void* a_host, int E, double rtol, int maxit, const double* out_b, int nvec,
                        size_t stop, Krylov& k, size_t extra = 0) {
  if (!c) return KMVP_E_INVALID;
  if (!c->have_points) return fail(c, KMVP_E_INVALID, "kmvp_set_points has not been called");
  if (int rc = solver_shape(c)) return rc;
  if (!a_host || !out_b || E < 1 || maxit < 0 || !(rtol > 0)) return fail(c, KMVP_E_INVALID, "bad solver arguments");
  if (c->diag_on && c->diag_n && c->diag_n != c->N)
    return fail(c, KMVP_E_INVALID, "solver diagonal: " + std::to_string(c->diag_n) + " values for " + std::to_string(c->N) +
                                       " points (pass the full vector, also on a source shard)");
  HIP_TRY(c, hipSetDevice(c->device));
  k.m = c->N;
  k.E = E;
  k.n = (size_t)k.m * E;
  k.stop = stop;
  if (int rc = ensure(c, c->scratch, sizeof(double) * (nvec * k.n + (size_t)CG_BLOCKS * E + stop + 2 + extra))) return rc;
  k.vecs = (double*)c->scratch.p;
  k.partial = k.vec(nvec);
  k.state = k.partial + (size_t)CG_BLOCKS * E;
  return KMVP_OK;
}

// out = sum over the CG_BLOCKS partials of u . v per column
static int cg_dots(kmvp_ctx* c, const double* u, const double* v, const Krylov& k, std::vector<double>& out) {
  const int E = k.E;
  std::vector<double> host_partial((size_t)CG_BLOCKS * E);
  hipLaunchKernelGGL(cg_dot_kernel, dim3(CG_BLOCKS), dim3(256), 0, c->stream, u, v, k.m, E, k.partial);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(host_partial.data(), k.partial, sizeof(double) * CG_BLOCKS * E, hipMemcpyDeviceToHost,
                            c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  out.assign(E, 0.0);
  for (int b = 0; b < CG_BLOCKS; ++b)
    for (int e = 0; e < E; ++e) out[e] += host_partial[(size_t)b * E + e];
  return KMVP_OK;
}

// K applied to the device vector v (N,E) double, N = all points; the result lands in c->out
// (N,E) double.  With source sharding the Krylov vectors are replicated on every
// rank, the operator is sharded: this rank's signal is its own slice v[j_offset .. j_offset+M)
// and run_product() ends with the all-reduce of the (N,E) sums, so every rank continues with
// bitwise the same vectors.  The solver's diagonal is NOT applied here: the first consumer of c->out adds it, once, on
// the full vector.
int cg_apply(kmvp_ctx* c, int kernel, const double* v, const Krylov& k) {
  // the Wendland kernels (kmvp_wendland_<c>_cg_solve): the cutoff product on its own layouts, b_raw and the pack
  // bookkeeping of the plain product untouched
  if (is_wendland(kernel)) return cutoff_apply(c, kernel, v, k.E);
  const int64_t n = c->M * k.E;  // this rank's sources
  v += (size_t)c->j_offset * k.E;
  int rc = ensure(c, c->b_raw, k.n * elem_size(c->dtype));  // also holds the right-hand side
  if (rc) return rc;
  if (c->dtype == KMVP_F64)
    hipLaunchKernelGGL((cg_cast_kernel<double>), dim3(blocks_for(n)), dim3(256), 0, c->stream, v, (double*)c->b_raw.p, n);
  else
    hipLaunchKernelGGL((cg_cast_kernel<float>), dim3(blocks_for(n)), dim3(256), 0, c->stream, v, (float*)c->b_raw.p, n);
  HIP_TRY(c, hipGetLastError());
  c->density = false;
  c->E = k.E;
  c->have_signal = true;
  ++c->signal_ver;
  return run_product(c, kernel, false);
}

// b_raw = the right-hand side as the caller passed it (N x E values in the working precision)
static int upload_rhs(kmvp_ctx* c, const void* a_host, const Krylov& k) {
  const size_t bytes = k.n * elem_size(c->dtype);
  if (int rc = ensure(c, c->b_raw, bytes)) return rc;
  HIP_TRY(c, hipMemcpyAsync(c->b_raw.p, a_host, bytes, hipMemcpyHostToDevice, c->stream));
  return KMVP_OK;
}

// out = the right-hand side widened to double
static int load_rhs(kmvp_ctx* c, const void* a_host, double* out, const Krylov& k) {
  if (int rc = upload_rhs(c, a_host, k)) return rc;
  const int64_t n = (int64_t)k.n;
  if (c->dtype == KMVP_F64)
    hipLaunchKernelGGL((cg_widen_kernel<double>), dim3(blocks_for(n)), dim3(256), 0, c->stream, (const double*)c->b_raw.p, out, n);
  else
    hipLaunchKernelGGL((cg_widen_kernel<float>), dim3(blocks_for(n)), dim3(256), 0, c->stream, (const float*)c->b_raw.p, out, n);
  HIP_TRY(c, hipGetLastError());
  return KMVP_OK;
}

// r = a - K x (with the diagonal on: a - K x - diag x) with one more product, and r2 = |r|^2 per column
static int true_residual(kmvp_ctx* c, int kernel, const void* a_host, const double* x, double* r, const Krylov& k,
                         std::vector<double>& r2) {
  int rc = cg_apply(c, kernel, x, k);
  if (!rc) rc = upload_rhs(c, a_host, k);  // after the product: b_raw held x
  if (rc) return rc;
  const int64_t n = (int64_t)k.n;
  const double* Kx = (const double*)c->out.p;
  if (c->diag_on) {
    if (c->dtype == KMVP_F64)
      hipLaunchKernelGGL((residual_diag_kernel<double>), dim3(blocks_for(n)), dim3(256), 0, c->stream, (const double*)c->b_raw.p, Kx, x, solver_diag(c), r, n, k.E);
    else
      hipLaunchKernelGGL((residual_diag_kernel<float>), dim3(blocks_for(n)), dim3(256), 0, c->stream, (const float*)c->b_raw.p, Kx, x, solver_diag(c), r, n, k.E);
  } else if (c->dtype == KMVP_F64)
    hipLaunchKernelGGL((residual_kernel<double>), dim3(blocks_for(n)), dim3(256), 0, c->stream, (const double*)c->b_raw.p, Kx, r, n);
  else
    hipLaunchKernelGGL((residual_kernel<float>), dim3(blocks_for(n)), dim3(256), 0, c->stream, (const float*)c->b_raw.p, Kx, r, n);
  HIP_TRY(c, hipGetLastError());
  return cg_dots(c, r, r, k, r2);
}

// One burst = CG_CHECK iterations of ~10 launches each.  A solve that is still running after
// CG_GRAPH_AFTER full bursts replays the burst as a hipGraph from then on (instantiating the 80-node
// graph costs ~70 ms on this stack, so short solves never pay for it; single GPU only: with a
// communicator the all-reduce stays out of graphs).  KMVP_NO_GRAPH=1 disables it; a refused capture
// falls back to plain launches for the rest of the solve.  One per solve, across its restarts.
struct BurstGraph {
  hipGraphExec_t exec = nullptr;
  int full_bursts = 0;
  bool try_graph;
  explicit BurstGraph(const kmvp_ctx* c) : try_graph(!c->exchanges() && getenv("KMVP_NO_GRAPH") == nullptr) {}
  BurstGraph(const BurstGraph&) = delete;
  BurstGraph& operator=(const BurstGraph&) = delete;
  ~BurstGraph() { if (exec) (void)hipGraphExecDestroy(exec); }
  int launch(kmvp_ctx* c) {
    return hipGraphLaunch(exec, c->stream) == hipSuccess ? KMVP_OK : fail(c, KMVP_E_DEVICE, "hipGraphLaunch failed");
  }
  template <typename Body>
  int run(kmvp_ctx* c, int burst, const Body& body) {
    if (burst != CG_CHECK) return body(burst);
    const bool capture = !exec && try_graph && full_bursts >= CG_GRAPH_AFTER;
    ++full_bursts;
    if (exec) return launch(c);
    if (!capture) return body(burst);
    // every buffer exists and every layout decision has been taken by the first burst: capture
    if (hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal) != hipSuccess) {
      (void)hipGetLastError();
      try_graph = false;
      return body(burst);
    }
    const int rc = body(burst);
    hipGraph_t graph = nullptr;
    const hipError_t ee = hipStreamEndCapture(c->stream, &graph);
    if (rc == KMVP_OK && ee == hipSuccess && graph && hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0) != hipSuccess)
      exec = nullptr;
    if (graph) (void)hipGraphDestroy(graph);
    if (rc) return rc;
    if (exec) return launch(c);
    (void)hipGetLastError();  // capture refused: nothing ran, go on launch by launch
    try_graph = false;
    return body(burst);
  }
};

// The host's part of a device-resident iteration: while it < maxit and rel > rtol, one burst of
// iterations (`body`, through `graph` when there is one), then a look at the device state (the k.stop + 2
// doubles and whatever the solver keeps behind them, read into `state`): the iteration count, `rel` as
// `rel_of` computes it from the state, and the stop word, set by the device once the tolerance was met
// inside the burst.
template <typename Body, typename Rel>
static int run_bursts(kmvp_ctx* c, const Krylov& k, int maxit, double rtol, int& it, double& rel,
                      std::vector<double>& state, const Body& body, const Rel& rel_of, BurstGraph* graph) {
  c->async_product = true;
  while (it < maxit && rel > rtol) {
    const int burst = std::min(CG_CHECK, maxit - it);
    if (int rc = graph ? graph->run(c, burst, body) : body(burst)) return rc;
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(state.data(), k.state, sizeof(double) * state.size(), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    it = (int)state[k.stop + 1];  // iterations that changed the iterate
    rel = rel_of();
    if (state[k.stop] != 0.0) break;
  }
  c->async_product = false;
  return KMVP_OK;
}

// wv = the worst of wv and one more column's relative residual v.  A NaN column makes the whole verdict NaN whichever
// column it is (std::max would drop it, and a plain !(v <= wv) lets the NEXT column overwrite it: with a NaN in one
// right-hand side of several the solve then ran on the others and was reported as converged).
static inline void fold_worst(double& wv, double v) {
  if (!std::isnan(wv) && !(v <= wv)) wv = v;
}

// Copies the solution out.  The verdict is on the TRUE residual (include/kmvp.h), with 1.5x slack for
// the rounding between it and the recurrence the iteration stops on; a non-finite residual
// (non-finite operator or right-hand side) is never a success.
static int solver_end(kmvp_ctx* c, const char* method, const double* x, const Krylov& k, double* out_b, int it,
                      double true_rel, double rtol, int* iters, double* resid) {
  HIP_TRY(c, hipMemcpyAsync(out_b, x, sizeof(double) * k.n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (iters) *iters = it;
  if (resid) *resid = true_rel;
  if (!(std::isfinite(true_rel) && true_rel <= rtol * 1.5)) {
    c->err = std::string(method) + (std::isfinite(true_rel)
                                         ? " stopped before the true residual reached the requested tolerance"
                                         : ": the residual is not finite (non-finite operator or right-hand side)");
    return KMVP_E_NOT_CONVERGED;
  }
  return KMVP_OK;
}

// ------------------------------------------------------------------------------------
// conjugate gradients

static int pcg_solve(kmvp_ctx* c, int kernel, const void* a_host, int E, double rtol, int maxit, double* out_b, int* iters,
                     double* resid);

int cg_solve(kmvp_ctx* c, int kernel, const void* a_host, int E, double rtol, int maxit,
             double* out_b, int* iters, double* resid) {
  if (c) {
    c->last_precond_ms = 0.f;
    c->pc_used = 0;
    if (c->precond_rank > 0 && c->N > 0) return pcg_solve(c, kernel, a_host, E, rtol, maxit, out_b, iters, resid);
  }
  Krylov k;  // x, r, p; state: scal = [rs_old | alpha | beta | |a|^2] x E, stop, iterations
  if (int rc = solver_begin(c, a_host, E, rtol, maxit, out_b, 3, 4 * (size_t)E, k)) return rc;
  if (c->diag_on && c->diag_min < 0.0)
    return fail(c, KMVP_E_INVALID, "solver diagonal: conjugate gradients needs ridge + d_i >= 0 everywhere (smallest: " +
                                       std::to_string(c->diag_min) + ")");
  SolveGuard guard{c};
  BurstGraph graph(c);
  const bool with_diag = c->diag_on;
  const Diag diag = solver_diag(c);
  const int64_t m = k.m;
  const size_t vec = k.n * sizeof(double);
  double *x = k.vec(0), *r = k.vec(1), *p = k.vec(2), *scal = k.state;

  // r = p = a (widened to double), x = 0
  int rc = load_rhs(c, a_host, r, k);
  if (rc) return rc;
  HIP_TRY(c, hipMemcpyAsync(p, r, vec, hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(c, hipMemsetAsync(x, 0, vec, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  std::vector<double> anorm2, rs_new;
  if ((rc = cg_dots(c, r, r, k, anorm2))) return rc;

  auto worst = [&](const double* r2) {
    double wv = 0.0;
    for (int e = 0; e < E; ++e) {
      const double v = anorm2[e] > 0 ? std::sqrt(r2[e] / anorm2[e]) : (anorm2[e] == 0 ? 0.0 : NAN);
      fold_worst(wv, v);
    }
    return wv;
  };

  // ---- the iteration lives on the device: the step lengths are computed by one-block kernels from
  // the dot products' partial sums (same additions in the same order as the host would do) and the
  // vector updates read them from device memory, so an iteration is a sequence of launches with no
  // host synchronisation; the host looks at the residual every CG_CHECK iterations only.
  std::vector<double> state(k.stop + 2, 0.0);
  for (int e = 0; e < E; ++e) {
    state[e] = anorm2[e];
    state[3 * E + e] = anorm2[e];
  }
  HIP_TRY(c, hipMemcpyAsync(scal, state.data(), sizeof(double) * state.size(), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const unsigned vblocks = blocks_for(m * E);
  auto body = [&](int burst) -> int {
    for (int i = 0; i < burst; ++i) {
      if (int rcb = cg_apply(c, kernel, p, k)) return rcb;
      double* Ap = (double*)c->out.p;
      if (with_diag)  // Ap = K p + diag p, and p . Ap
        hipLaunchKernelGGL(cg_diag_dot_kernel, dim3(CG_BLOCKS), dim3(256), 0, c->stream, p, Ap, diag, m, E, k.partial);
      else
        hipLaunchKernelGGL(cg_dot_kernel, dim3(CG_BLOCKS), dim3(256), 0, c->stream, p, Ap, m, E, k.partial);
      hipLaunchKernelGGL(cg_scalars_kernel, dim3(1), dim3(CG_BLOCKS), 0, c->stream, k.partial, scal, E, 1, rtol);
      hipLaunchKernelGGL(cg_update_xr_kernel, dim3(vblocks), dim3(256), 0, c->stream, x, r, p, Ap, scal, m, E);
      hipLaunchKernelGGL(cg_dot_kernel, dim3(CG_BLOCKS), dim3(256), 0, c->stream, r, r, m, E, k.partial);
      hipLaunchKernelGGL(cg_scalars_kernel, dim3(1), dim3(CG_BLOCKS), 0, c->stream, k.partial, scal, E, 2, rtol);
      hipLaunchKernelGGL(cg_update_p_kernel, dim3(vblocks), dim3(256), 0, c->stream, p, r, scal, m, E);
    }
    return KMVP_OK;
  };
  auto rel_of = [&] { return worst(state.data()); };  // rs_old heads the state
  int it = 0;
  double rel = worst(anorm2.data());
  double true_rel = NAN, prev_true = INFINITY;
  // The iteration stops on the RECURRENCE residual; the verdict is on the TRUE one, a - K x (- diag x), from one more
  // product.  Where the two have drifted apart (float32 operator, ill-conditioned Gaussian matrices) the
  // recurrence is restarted from the true residual (r = p = a - K x: "residual replacement"), at most
  // CG_MAX_RESTARTS times and only while that still halves the true residual.
  constexpr int CG_MAX_RESTARTS = 3;
  for (int pass = 0;; ++pass) {
    if ((rc = run_bursts(c, k, maxit, rtol, it, rel, state, body, rel_of, &graph))) return rc;
    if ((rc = true_residual(c, kernel, a_host, x, p, k, rs_new))) return rc;  // p = a - K x
    true_rel = worst(rs_new.data());
    const bool met = std::isfinite(true_rel) && true_rel <= rtol * 1.5;
    if (met || !std::isfinite(true_rel) || it >= maxit || pass >= CG_MAX_RESTARTS || !(true_rel <= 0.5 * prev_true)) break;
    // restart from the true residual: r = p = a - K x, rs_old = |r|^2, stop flag cleared (the count goes on)
    prev_true = true_rel;
    const double zero = 0.0;
    HIP_TRY(c, hipMemcpyAsync(r, p, vec, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(scal, rs_new.data(), sizeof(double) * E, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(scal + 4 * (size_t)E, &zero, sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    rel = true_rel;
  }
  return solver_end(c, "conjugate gradients", x, k, out_b, it, true_rel, rtol, iters, resid);
}

// ------------------------------------------------------------------------------------
// preconditioned conjugate gradients (kmvp_set_solver_preconditioner): cg_solve's driver around z = P^-1 r
//   x = 0, r = a, z = P^-1 r, p = z, rho = r . z
//   alpha = rho / pAp (cg_scalars_kernel's mode 1 and its guards);  x += alpha p;  r -= alpha Ap;  rs = r . r, the stop
//   test and the count exactly as cg_scalars_kernel's mode 2 makes them;  z = P^-1 r;  rho' = r . z;  beta = rho' / rho
//   (0 when rho <= 0);  p = z + beta p
// State: [rho | alpha | beta | |a|^2] x E, stop, iterations -- cg_solve's layout, with rho in the place of rs_old, so that
// cg_scalars_kernel (mode 1), cg_update_xr_kernel and cg_update_p_kernel (with z for r) serve unchanged -- then rs x E.

// One block.  mode 2 (after r . r): rs[e] = sum, the count and the stop word;  mode 3 (after r . z): beta and rho.
__global__ void __launch_bounds__(CG_BLOCKS) pcg_scalars_kernel(const double* __restrict__ partial, double* __restrict__ scal,
                                                               int E, int mode, double rtol) {
  __shared__ double red[CG_BLOCKS];
  double* stop = scal + 4 * E;
  if (*stop != 0.0) return;  // uniform: every thread reads the same word
  bool not_met = false;
  for (int e = 0; e < E; ++e) {
    const double v = block_sum_partials(partial, E, e, red);
    if (threadIdx.x != 0) continue;
    if (mode == 2) {
      scal[4 * E + 2 + e] = v;
      const double a2 = scal[3 * E + e];
      if (a2 > 0.0 && !(sqrt(v / a2) <= rtol)) not_met = true;  // NaN / inf: not met
    } else {
      const double rho = scal[e];
      scal[2 * E + e] = rho > 0.0 ? v / rho : 0.0;
      scal[e] = v;
    }
  }
  if (mode == 2 && threadIdx.x == 0) {
    scal[4 * E + 1] += 1.0;
    if (!not_met) *stop = 1.0;
  }
}

static int pcg_solve(kmvp_ctx* c, int kernel, const void* a_host, int E, double rtol, int maxit, double* out_b, int* iters,
                     double* resid) {
  Krylov k;  // x, r, p, z; state: see above; then the apply's scratch
  const int rank = c->precond_rank;
  const size_t rs_at = 4 * (size_t)std::max(E, 0) + 2;
  if (int rc = solver_begin(c, a_host, E, rtol, maxit, out_b, 4, 4 * (size_t)E, k, (size_t)E + precond_scratch(rank, std::max(E, 0))))
    return rc;
  if (!c->diag_on || !(c->diag_min > 0.0))
    return fail(c, KMVP_E_INVALID, "preconditioner: P = L L' + D needs a solver diagonal with ridge + d_i > 0 everywhere (" +
                                       (c->diag_on ? "smallest: " + std::to_string(c->diag_min) : std::string("none is set")) + ")");
  if (int rc = precond_prepare(c, kernel)) return rc;
  c->pc_used = c->pc_built;
  SolveGuard guard{c};
  BurstGraph graph(c);
  const Diag diag = solver_diag(c);
  const int64_t m = k.m;
  const size_t vec = k.n * sizeof(double);
  double *x = k.vec(0), *r = k.vec(1), *p = k.vec(2), *z = k.vec(3), *scal = k.state;
  double* pc_scratch = scal + rs_at + E;
  const double* stop = scal + 4 * (size_t)E;

  int rc = load_rhs(c, a_host, r, k);
  if (rc) return rc;
  HIP_TRY(c, hipMemsetAsync(x, 0, vec, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  std::vector<double> anorm2, rs_new;
  if ((rc = cg_dots(c, r, r, k, anorm2))) return rc;

  auto worst = [&](const double* r2) {
    double wv = 0.0;
    for (int e = 0; e < E; ++e) {
      const double v = anorm2[e] > 0 ? std::sqrt(r2[e] / anorm2[e]) : (anorm2[e] == 0 ? 0.0 : NAN);
      fold_worst(wv, v);
    }
    return wv;
  };

  std::vector<double> state(rs_at + E, 0.0);
  for (int e = 0; e < E; ++e) {
    state[3 * E + e] = anorm2[e];
    state[rs_at + e] = anorm2[e];
  }
  HIP_TRY(c, hipMemcpyAsync(scal, state.data(), sizeof(double) * state.size(), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const unsigned vblocks = blocks_for(m * E);
  // z = P^-1 r, rho = r . z (and beta, which the start does not use), on the stream
  auto precondition = [&] {
    precond_apply(c, r, z, E, pc_scratch, k.partial, CG_BLOCKS, stop);
    hipLaunchKernelGGL(pcg_scalars_kernel, dim3(1), dim3(CG_BLOCKS), 0, c->stream, k.partial, scal, E, 3, rtol);
  };
  // the start, and every restart: p = z = P^-1 r with rho = 0 on entry (beta = 0)
  auto start = [&]() -> int {
    precondition();
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(p, z, vec, hipMemcpyDeviceToDevice, c->stream));
    return KMVP_OK;
  };
  if ((rc = start())) return rc;
  auto body = [&](int burst) -> int {
    for (int i = 0; i < burst; ++i) {
      if (int rcb = cg_apply(c, kernel, p, k)) return rcb;
      double* Ap = (double*)c->out.p;
      hipLaunchKernelGGL(cg_diag_dot_kernel, dim3(CG_BLOCKS), dim3(256), 0, c->stream, p, Ap, diag, m, E, k.partial);
      hipLaunchKernelGGL(cg_scalars_kernel, dim3(1), dim3(CG_BLOCKS), 0, c->stream, k.partial, scal, E, 1, rtol);
      hipLaunchKernelGGL(cg_update_xr_kernel, dim3(vblocks), dim3(256), 0, c->stream, x, r, p, Ap, scal, m, E);
      hipLaunchKernelGGL(cg_dot_kernel, dim3(CG_BLOCKS), dim3(256), 0, c->stream, r, r, m, E, k.partial);
      hipLaunchKernelGGL(pcg_scalars_kernel, dim3(1), dim3(CG_BLOCKS), 0, c->stream, k.partial, scal, E, 2, rtol);
      precondition();
      hipLaunchKernelGGL(cg_update_p_kernel, dim3(vblocks), dim3(256), 0, c->stream, p, z, scal, m, E);
    }
    return KMVP_OK;
  };
  auto rel_of = [&] { return worst(state.data() + rs_at); };
  int it = 0;
  double rel = worst(anorm2.data());
  double true_rel = NAN, prev_true = INFINITY;
  constexpr int CG_MAX_RESTARTS = 3;  // residual replacement as in cg_solve, with z = P^-1 r, p = z at a restart
  for (int pass = 0;; ++pass) {
    if ((rc = run_bursts(c, k, maxit, rtol, it, rel, state, body, rel_of, &graph))) return rc;
    if ((rc = true_residual(c, kernel, a_host, x, p, k, rs_new))) return rc;  // p = a - A x
    true_rel = worst(rs_new.data());
    const bool met = std::isfinite(true_rel) && true_rel <= rtol * 1.5;
    if (met || !std::isfinite(true_rel) || it >= maxit || pass >= CG_MAX_RESTARTS || !(true_rel <= 0.5 * prev_true)) break;
    prev_true = true_rel;
    const double zero = 0.0;
    std::vector<double> rho0(E, 0.0);
    HIP_TRY(c, hipMemcpyAsync(r, p, vec, hipMemcpyDeviceToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(scal, rho0.data(), sizeof(double) * E, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(scal + rs_at, rs_new.data(), sizeof(double) * E, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(scal + 4 * (size_t)E, &zero, sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if ((rc = start())) return rc;
    rel = true_rel;
  }
  c->last_total_ms += c->last_precond_ms;  // the build, when it happened in this call
  return solver_end(c, "preconditioned conjugate gradients", x, k, out_b, it, true_rel, rtol, iters, resid);
}


// ------------------------------------------------------------------------------------
// conjugate gradients for its coefficients: stochastic Lanczos quadrature (include/kmvp.h kmvp_<kernel>_lanczos_quadrature)

// State per column e: see LZ_* ; then the stop word and the iteration count.  LZ_FROZEN says why a column takes no
// further update: on the tolerance, by a breakdown of the recurrence (pAp == 0 or rs_old <= 0), or as a zero column.
enum : int { LZ_RS = 0, LZ_ALPHA, LZ_BETA, LZ_Z2, LZ_FROZEN, LZ_STEPS, LZ_FIELDS };
constexpr double LZ_LIVE = 0.0, LZ_TOLERANCE = 1.0, LZ_BREAKDOWN = 2.0, LZ_ZERO = 3.0;

// cg_scalars_kernel with every column on its own clock.  One block; same guards on alpha and beta.  Iteration k = count + 1:
// mode 1 (after p . Ap): alpha, written to row `count` of the history; a column whose guard fires freezes here, with
//   steps = k - 1 and no row.
// mode 2 (after r . r): beta into row `count`, rs_old = rs_new, steps = k, and the column freezes once
//   sqrt(rs_new / |z|^2) <= rtol (NaN: never).  Then count + 1, and the stop word is set in the first iteration that
//   leaves every column frozen.
// The row is the DEVICE's count, so a replayed burst graph writes the rows of the iterations it replays.
__global__ void __launch_bounds__(CG_BLOCKS) lanczos_scalars_kernel(const double* __restrict__ partial,
                                                                   double* __restrict__ st, int P, int mode, double rtol,
                                                                   double* __restrict__ hist_alpha,
                                                                   double* __restrict__ hist_beta, int maxit) {
  __shared__ double red[CG_BLOCKS];
  double* stop = st + (size_t)LZ_FIELDS * P;
  if (*stop != 0.0) return;  // uniform: every thread reads the same word
  const int64_t row = (int64_t)stop[1];
  bool live = false;
  for (int e = 0; e < P; ++e) {
    const double v = block_sum_partials(partial, P, e, red);
    if (threadIdx.x != 0) continue;
    auto S = [&](int f) -> double& { return st[(size_t)f * P + e]; };
    if (S(LZ_FROZEN) != LZ_LIVE || row >= maxit) continue;
    const double rs_old = S(LZ_RS);
    if (mode == 1) {
      const double alpha = (v != 0.0 && rs_old > 0.0) ? rs_old / v : 0.0;
      S(LZ_ALPHA) = alpha;
      if (v == 0.0 || rs_old <= 0.0)
        S(LZ_FROZEN) = LZ_BREAKDOWN;
      else
        hist_alpha[row * P + e] = alpha;
    } else {
      const double beta = rs_old > 0.0 ? v / rs_old : 0.0;
      S(LZ_BETA) = beta;
      S(LZ_RS) = v;
      S(LZ_STEPS) = (double)(row + 1);
      hist_beta[row * P + e] = beta;
      if (sqrt(v / S(LZ_Z2)) <= rtol)
        S(LZ_FROZEN) = LZ_TOLERANCE;
      else
        live = true;
    }
  }
  if (mode == 2 && threadIdx.x == 0) {
    stop[1] += 1.0;
    if (!live) *stop = 1.0;
  }
}

// x += alpha p ; r -= alpha Ap in the columns that are live.  A frozen column is skipped, not multiplied by 0: whatever
// its p and Ap have become, its x and r stay.
__global__ void lanczos_update_xr_kernel(double* __restrict__ x, double* __restrict__ r, const double* __restrict__ p,
                                         const double* __restrict__ Ap, const double* __restrict__ st, int64_t m, int P) {
  if (st[(size_t)LZ_FIELDS * P] != 0.0) return;  // stopped
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= m * P) return;
  const int e = (int)(q % P);
  if (st[(size_t)LZ_FROZEN * P + e] != LZ_LIVE) return;
  const double a = st[(size_t)LZ_ALPHA * P + e];
  x[q] = x[q] + a * p[q];
  r[q] = r[q] + (-a) * Ap[q];
}

// p = r + beta p in the columns that are live
__global__ void lanczos_update_p_kernel(double* __restrict__ p, const double* __restrict__ r,
                                        const double* __restrict__ st, int64_t m, int P) {
  if (st[(size_t)LZ_FIELDS * P] != 0.0) return;  // stopped
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= m * P) return;
  const int e = (int)(q % P);
  if (st[(size_t)LZ_FROZEN * P + e] != LZ_LIVE) return;
  p[q] = r[q] + st[(size_t)LZ_BETA * P + e] * p[q];
}

// The recurrence of cg_solve from x = 0, r = p = z, without its residual replacement (a restart would break the three-term
// recurrence the coefficients stand for): the verdict is on the RECURRENCE residual.  Converged columns do not go on
// iterating as they do in cg_solve: their later coefficients would be rounding noise.
int cg_lanczos(kmvp_ctx* c, int kernel, const void* z_host, int P, double rtol, int maxit, double* logquad, double* invquad,
               int* steps, double* x_out, double* alpha_out, double* beta_out) {
  if (c && (!logquad || !invquad || !steps)) return fail(c, KMVP_E_INVALID, "bad solver arguments");
  if (c && c->dtype == KMVP_BF16 && c->have_points)
    return fail(c, KMVP_E_UNSUPPORTED, "the Lanczos quadrature needs a float32 or float64 context");
  Krylov k;  // x, r, p, z; state: LZ_FIELDS x P, stop, iterations; then alpha and beta of every iteration, (maxit, P) each
  const size_t rows = (size_t)std::max(maxit, 0) * (size_t)std::max(P, 0);
  if (int rc = solver_begin(c, z_host, P, rtol, maxit, logquad, 4, (size_t)LZ_FIELDS * P, k, 2 * rows)) return rc;
  if (c->diag_on && c->diag_min < 0.0)
    return fail(c, KMVP_E_INVALID, "solver diagonal: conjugate gradients needs ridge + d_i >= 0 everywhere (smallest: " +
                                       std::to_string(c->diag_min) + ")");
  SolveGuard guard{c};
  BurstGraph graph(c);
  const bool with_diag = c->diag_on;
  const Diag diag = solver_diag(c);
  const int64_t m = k.m;
  const size_t vec = k.n * sizeof(double);
  double *x = k.vec(0), *r = k.vec(1), *p = k.vec(2), *z = k.vec(3), *st = k.state;
  double *hist_alpha = st + k.stop + 2, *hist_beta = hist_alpha + rows;
  HIP_TRY(c, hipEventRecord(c->ev[0], c->stream));

  // z = r = p = the probes (widened to double), x = 0, history = 0
  int rc = load_rhs(c, z_host, z, k);
  if (rc) return rc;
  HIP_TRY(c, hipMemcpyAsync(r, z, vec, hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(p, z, vec, hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(c, hipMemsetAsync(x, 0, vec, c->stream));
  if (rows) HIP_TRY(c, hipMemsetAsync(hist_alpha, 0, sizeof(double) * 2 * rows, c->stream));
  std::vector<double> z2, zx;
  if ((rc = cg_dots(c, z, z, k, z2))) return rc;

  std::vector<double> state(k.stop + 2, 0.0);
  for (int e = 0; e < P; ++e) {
    state[(size_t)LZ_RS * P + e] = z2[e];
    state[(size_t)LZ_Z2 * P + e] = z2[e];
    state[(size_t)LZ_FROZEN * P + e] = z2[e] == 0.0 ? LZ_ZERO : LZ_LIVE;
  }
  HIP_TRY(c, hipMemcpyAsync(st, state.data(), sizeof(double) * state.size(), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const unsigned vblocks = blocks_for(m * P);
  auto body = [&](int burst) -> int {
    for (int i = 0; i < burst; ++i) {
      if (int rcb = cg_apply(c, kernel, p, k)) return rcb;
      double* Ap = (double*)c->out.p;
      if (with_diag)  // Ap = K p + diag p, and p . Ap
        hipLaunchKernelGGL(cg_diag_dot_kernel, dim3(CG_BLOCKS), dim3(256), 0, c->stream, p, Ap, diag, m, P, k.partial);
      else
        hipLaunchKernelGGL(cg_dot_kernel, dim3(CG_BLOCKS), dim3(256), 0, c->stream, p, Ap, m, P, k.partial);
      hipLaunchKernelGGL(lanczos_scalars_kernel, dim3(1), dim3(CG_BLOCKS), 0, c->stream, k.partial, st, P, 1, rtol, hist_alpha,
                         hist_beta, maxit);
      hipLaunchKernelGGL(lanczos_update_xr_kernel, dim3(vblocks), dim3(256), 0, c->stream, x, r, p, Ap, st, m, P);
      hipLaunchKernelGGL(cg_dot_kernel, dim3(CG_BLOCKS), dim3(256), 0, c->stream, r, r, m, P, k.partial);
      hipLaunchKernelGGL(lanczos_scalars_kernel, dim3(1), dim3(CG_BLOCKS), 0, c->stream, k.partial, st, P, 2, rtol, hist_alpha,
                         hist_beta, maxit);
      hipLaunchKernelGGL(lanczos_update_p_kernel, dim3(vblocks), dim3(256), 0, c->stream, p, r, st, m, P);
    }
    return KMVP_OK;
  };
  // run_bursts goes on while "rel" > rtol: infinite while a column is live
  auto rel_of = [&] {
    for (int e = 0; e < P; ++e)
      if (state[(size_t)LZ_FROZEN * P + e] == LZ_LIVE) return (double)INFINITY;
    return 0.0;
  };
  int it = 0;
  double rel = rel_of();
  if ((rc = run_bursts(c, k, maxit, rtol, it, rel, state, body, rel_of, &graph))) return rc;

  // z . x per column, then the history, the final state and the iterates in one pass over the stream
  if ((rc = cg_dots(c, z, x, k, zx))) return rc;
  std::vector<double> hist(2 * rows);
  HIP_TRY(c, hipMemcpyAsync(state.data(), st, sizeof(double) * state.size(), hipMemcpyDeviceToHost, c->stream));
  if (rows) HIP_TRY(c, hipMemcpyAsync(hist.data(), hist_alpha, sizeof(double) * 2 * rows, hipMemcpyDeviceToHost, c->stream));
  if (x_out) HIP_TRY(c, hipMemcpyAsync(x_out, x, vec, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipEventRecord(c->ev[2], c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipEventElapsedTime(&c->last_total_ms, c->ev[0], c->ev[2]));
  c->last_kernel_ms = c->last_total_ms;  // both cover the whole call (include/kmvp.h)

  bool ok = true;
  for (int e = 0; e < P; ++e) {
    const double frozen = state[(size_t)LZ_FROZEN * P + e];
    steps[e] = (int)state[(size_t)LZ_STEPS * P + e];
    logquad[e] = z2[e] * lanczos_quadrature_log(hist.data() + e, hist.data() + rows + e, steps[e], P);
    invquad[e] = zx[e];
    if (frozen != LZ_ZERO && !(frozen == LZ_TOLERANCE && std::isfinite(logquad[e]))) ok = false;
  }
  if (alpha_out && rows) memcpy(alpha_out, hist.data(), sizeof(double) * rows);
  if (beta_out && rows) memcpy(beta_out, hist.data() + rows, sizeof(double) * rows);
  if (!ok) {
    c->err = "Lanczos quadrature: a column did not reach the requested tolerance on the recurrence residual, or its "
             "quadrature is not finite (operator not positive definite, non-finite operator or probe)";
    return KMVP_E_NOT_CONVERGED;
  }
  return KMVP_OK;
}

// cg_lanczos around z = P^-1 r, as pcg_solve is cg_solve around it (include/kmvp.h kmvp_<kernel>_lanczos_quadrature_precond):
//   z = L h + D^1/2 g;  x = 0, r = z, pz = P^-1 z, p = pz, rho_0 = z . pz
//   alpha = rho / pAp;  x += alpha p;  r -= alpha Ap;  zr = P^-1 r;  rho' = r . zr;  beta = rho' / rho;  p = zr + beta p
// in the live columns.  These are the coefficients of conjugate gradients on M xh = w, M = P^-1/2 A P^-1/2, w = P^-1/2 z,
// whose residual norm is sqrt(rho): the state is LZ_* with rho in LZ_RS and rho_0 in LZ_Z2, so lanczos_scalars_kernel --
// mode 1 after p . Ap, mode 2 after the partials of r . zr that precond_apply leaves -- and the two update kernels (with zr
// for r in lanczos_update_p_kernel) serve unchanged, and the column freezes on sqrt(rho / rho_0) <= rtol without a dot
// product of its own.  Five Krylov vectors: pz is kept for invquad = pz . x and for the caller's trace estimates.
int cg_lanczos_precond(kmvp_ctx* c, int kernel, const double* g_host, const double* h_host, int P, double rtol, int maxit,
                       double* logdet_p, double* logquad, double* invquad, double* wnorm2, int* steps, double* x_out,
                       double* pz_out, double* alpha_out, double* beta_out) {
  if (c && (!h_host || !logdet_p || !logquad || !invquad || !wnorm2 || !steps)) return fail(c, KMVP_E_INVALID, "bad solver arguments");
  if (c && c->dtype == KMVP_BF16 && c->have_points)
    return fail(c, KMVP_E_UNSUPPORTED, "the Lanczos quadrature needs a float32 or float64 context");
  Krylov k;  // x, r, p, zr, pz; state: LZ_FIELDS x P, stop, iterations; alpha and beta of every iteration, (maxit, P) each; the
             // partial sums of log D_i and their sum; the apply's scratch
  const int rank = c ? c->precond_rank : 0;
  const size_t rows = (size_t)std::max(maxit, 0) * (size_t)std::max(P, 0);
  if (int rc = solver_begin(c, g_host, P, rtol, maxit, logquad, 5, (size_t)LZ_FIELDS * P, k,
                            2 * rows + PC_LOGD_BLOCKS + 1 + precond_scratch(rank, std::max(P, 0))))
    return rc;
  if (rank < 1)
    return fail(c, KMVP_E_INVALID, "preconditioner: the preconditioned Lanczos quadrature needs kmvp_set_solver_preconditioner with rank >= 1");
  if (!c->diag_on || !(c->diag_min > 0.0))
    return fail(c, KMVP_E_INVALID, "preconditioner: P = L L' + D needs a solver diagonal with ridge + d_i > 0 everywhere (" +
                                       (c->diag_on ? "smallest: " + std::to_string(c->diag_min) : std::string("none is set")) + ")");
  if (c->N < 1) return fail(c, KMVP_E_INVALID, "preconditioner: the cloud is empty");
  c->last_precond_ms = 0.f;
  if (int rc = precond_prepare(c, kernel)) return rc;
  c->pc_used = c->pc_built;
  SolveGuard guard{c};
  BurstGraph graph(c);
  const Diag diag = solver_diag(c);
  const int64_t m = k.m;
  const size_t vec = k.n * sizeof(double);
  double *x = k.vec(0), *r = k.vec(1), *p = k.vec(2), *zr = k.vec(3), *pz = k.vec(4), *st = k.state;
  double *hist_alpha = st + k.stop + 2, *hist_beta = hist_alpha + rows;
  double *logd = hist_alpha + 2 * rows, *pc_scratch = logd + PC_LOGD_BLOCKS + 1;
  const double* stop = st + k.stop;
  HIP_TRY(c, hipEventRecord(c->ev[0], c->stream));

  // g in x's place and the rows of h that have a column in the apply's scratch, until the probes are formed: r = z;
  // then x = 0, history = 0, the state's stop word = 0 (the apply reads it), pz = P^-1 z with the partials of z . pz, p = pz
  HIP_TRY(c, hipMemcpyAsync(x, g_host, vec, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(pc_scratch, h_host, sizeof(double) * (size_t)c->pc_built * P, hipMemcpyHostToDevice, c->stream));
  precond_probes(c, x, pc_scratch, P, r);
  precond_logdiag(c, logd);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemsetAsync(x, 0, vec, c->stream));
  HIP_TRY(c, hipMemsetAsync(st, 0, sizeof(double) * (k.stop + 2 + 2 * rows), c->stream));
  precond_apply(c, r, pz, P, pc_scratch, k.partial, CG_BLOCKS, stop);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(p, pz, vec, hipMemcpyDeviceToDevice, c->stream));
  std::vector<double> host_partial((size_t)CG_BLOCKS * P), rho0(P, 0.0), pzx;
  double sum_logd = 0.0;
  HIP_TRY(c, hipMemcpyAsync(host_partial.data(), k.partial, sizeof(double) * host_partial.size(), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(&sum_logd, logd + PC_LOGD_BLOCKS, sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (int b = 0; b < CG_BLOCKS; ++b)  // as cg_dots adds them
    for (int e = 0; e < P; ++e) rho0[e] += host_partial[(size_t)b * P + e];

  std::vector<double> state(k.stop + 2, 0.0);
  for (int e = 0; e < P; ++e) {
    state[(size_t)LZ_RS * P + e] = rho0[e];
    state[(size_t)LZ_Z2 * P + e] = rho0[e];
    state[(size_t)LZ_FROZEN * P + e] = rho0[e] == 0.0 ? LZ_ZERO : LZ_LIVE;
  }
  HIP_TRY(c, hipMemcpyAsync(st, state.data(), sizeof(double) * state.size(), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const unsigned vblocks = blocks_for(m * P);
  auto body = [&](int burst) -> int {
    for (int i = 0; i < burst; ++i) {
      if (int rcb = cg_apply(c, kernel, p, k)) return rcb;
      double* Ap = (double*)c->out.p;
      hipLaunchKernelGGL(cg_diag_dot_kernel, dim3(CG_BLOCKS), dim3(256), 0, c->stream, p, Ap, diag, m, P, k.partial);
      hipLaunchKernelGGL(lanczos_scalars_kernel, dim3(1), dim3(CG_BLOCKS), 0, c->stream, k.partial, st, P, 1, rtol, hist_alpha,
                         hist_beta, maxit);
      hipLaunchKernelGGL(lanczos_update_xr_kernel, dim3(vblocks), dim3(256), 0, c->stream, x, r, p, Ap, st, m, P);
      precond_apply(c, r, zr, P, pc_scratch, k.partial, CG_BLOCKS, stop);  // zr = P^-1 r and the partials of r . zr
      hipLaunchKernelGGL(lanczos_scalars_kernel, dim3(1), dim3(CG_BLOCKS), 0, c->stream, k.partial, st, P, 2, rtol, hist_alpha,
                         hist_beta, maxit);
      hipLaunchKernelGGL(lanczos_update_p_kernel, dim3(vblocks), dim3(256), 0, c->stream, p, zr, st, m, P);
    }
    return KMVP_OK;
  };
  auto rel_of = [&] {
    for (int e = 0; e < P; ++e)
      if (state[(size_t)LZ_FROZEN * P + e] == LZ_LIVE) return (double)INFINITY;
    return 0.0;
  };
  int it = 0;
  double rel = rel_of();
  if (int rc = run_bursts(c, k, maxit, rtol, it, rel, state, body, rel_of, &graph)) return rc;

  if (int rc = cg_dots(c, pz, x, k, pzx)) return rc;
  std::vector<double> hist(2 * rows);
  HIP_TRY(c, hipMemcpyAsync(state.data(), st, sizeof(double) * state.size(), hipMemcpyDeviceToHost, c->stream));
  if (rows) HIP_TRY(c, hipMemcpyAsync(hist.data(), hist_alpha, sizeof(double) * 2 * rows, hipMemcpyDeviceToHost, c->stream));
  if (x_out) HIP_TRY(c, hipMemcpyAsync(x_out, x, vec, hipMemcpyDeviceToHost, c->stream));
  if (pz_out) HIP_TRY(c, hipMemcpyAsync(pz_out, pz, vec, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipEventRecord(c->ev[2], c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipEventElapsedTime(&c->last_total_ms, c->ev[0], c->ev[2]));
  c->last_kernel_ms = c->last_total_ms;  // both cover the iteration; the total also the build, when it happened in this call
  c->last_total_ms += c->last_precond_ms;

  *logdet_p = sum_logd + c->pc_logdet_c;
  bool ok = true;
  for (int e = 0; e < P; ++e) {
    const double frozen = state[(size_t)LZ_FROZEN * P + e];
    steps[e] = (int)state[(size_t)LZ_STEPS * P + e];
    wnorm2[e] = rho0[e];
    logquad[e] = rho0[e] * lanczos_quadrature_log(hist.data() + e, hist.data() + rows + e, steps[e], P);
    invquad[e] = pzx[e];
    if (frozen != LZ_ZERO && !(frozen == LZ_TOLERANCE && std::isfinite(logquad[e]))) ok = false;
  }
  if (alpha_out && rows) memcpy(alpha_out, hist.data(), sizeof(double) * rows);
  if (beta_out && rows) memcpy(beta_out, hist.data() + rows, sizeof(double) * rows);
  if (!ok) {
    c->err = "preconditioned Lanczos quadrature: a column did not reach the requested tolerance on the recurrence residual, "
             "or its quadrature is not finite (operator not positive definite, non-finite operator or probe)";
    return KMVP_E_NOT_CONVERGED;
  }
  return KMVP_OK;
}


// ------------------------------------------------------------------------------------
// MINRES (Paige & Saunders) for the symmetric INDEFINITE inverse-distance systems (zero
// diagonal), where conjugate gradients does not apply.  One product per iteration.

// ---- MINRES on the device.  State per column e (doubles): see MS_* below; five coefficient
// triples [3E] feed vec_lin3_dev_kernel.  Same scalar arithmetic, in the same order, as the
// textbook recurrence on the host would do.
enum : int { MS_BETA1 = 0, MS_BETA, MS_OLDB, MS_ALFA, MS_DBAR, MS_EPSLN, MS_CS, MS_SN, MS_PHIBAR, MS_DONE, MS_FIELDS };
// layout: state[MS_FIELDS][E] | T0..T4 [5][3E] | stop | iterations
// The stop word: 0 while iterating; MS_MET once an iteration met the tolerance -- set by its scalar step, which comes BEFORE
// its x update, so that iteration's tail still runs (without it the host would read x of the iteration before, with the
// count and the phibar of this one); MS_STOPPED from the next scalar step on, and then the tail is off too.
constexpr double MS_MET = 2.0, MS_STOPPED = 1.0;
__host__ __device__ inline size_t ms_triple(int E, int t) { return (size_t)MS_FIELDS * E + (size_t)t * 3 * E; }
__host__ __device__ inline size_t ms_stop(int E) { return (size_t)MS_FIELDS * E + 15 * (size_t)E; }

// out = c0 a + c1 b + c2 c with the coefficient triple in device memory; nothing once stopped.  out2 (or nullptr): a second
// copy of the result -- it may be `a` itself (each thread reads its element before it writes it)
__global__ void vec_lin3_dev_kernel(double* __restrict__ out, const double* a,
                                    const double* __restrict__ b, const double* __restrict__ c,
                                    const double* __restrict__ coef, const double* __restrict__ stop, int64_t m,
                                    int E, double* out2) {
  if (*stop != 0.0) return;
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= m * E) return;
  const int e = (int)(q % E);
  double v = coef[e] * a[q];
  if (b) v += coef[E + e] * b[q];
  if (c) v += coef[2 * E + e] * c[q];
  out[q] = v;
  if (out2) out2[q] = v;
}

// MINRES' first consumer of K v with the solver's diagonal on: y = c0 (K v + diag v) + c1 r1, the Lanczos step of
// A = K + diag (vec_lin3_dev_kernel with the diagonal term folded into its first operand); nothing once stopped.
__global__ void minres_diag_lanczos_kernel(double* __restrict__ y, const double* __restrict__ Kv, const double* __restrict__ v,
                                           const double* __restrict__ r1, Diag diag, const double* __restrict__ coef,
                                           const double* __restrict__ stop, int64_t m, int E) {
  if (*stop != 0.0) return;
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= m * E) return;
  const int e = (int)(q % E);
  double yv = coef[e] * (Kv[q] + diag.at(q / E) * v[q]);
  yv += coef[E + e] * r1[q];
  y[q] = yv;
}

// The three vector updates that close a MINRES iteration (the stopping one included), in one launch (each was a ~4.5 us
// kernel of its own in a solve whose
// iteration is a chain of such kernels): w = T3 . (v, w1, w2);  x = T4 . (x, w);  v = T0 y  (the NEXT iteration's Lanczos vector;
// v is read for w before it is overwritten, element by element).  Same expressions, same order as vec_lin3_dev_kernel.
__global__ void minres_tail_kernel(double* __restrict__ w, double* __restrict__ v, const double* __restrict__ w1,
                                   const double* __restrict__ w2, double* __restrict__ x, const double* __restrict__ y,
                                   const double* __restrict__ T3, const double* __restrict__ T4, const double* __restrict__ T0,
                                   const double* __restrict__ stop, int64_t m, int E) {
  if (*stop == MS_STOPPED) return;  // MS_MET: the tolerance was met in THIS iteration, whose x is the one to return
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= m * E) return;
  const int e = (int)(q % E);
  double wv = T3[e] * v[q];
  wv += T3[E + e] * w1[q];
  wv += T3[2 * E + e] * w2[q];
  w[q] = wv;
  double xv = T4[e] * x[q];
  xv += T4[E + e] * wv;
  x[q] = xv;
  v[q] = T0[e] * y[q];
}

// mode 1 (after v.y): alfa, T2 = (1, -alfa/beta, 0).
// mode 2 (after r2.r2): the Givens step, T3 (w update), T4 (x update), the done flags, the stopping
// test max_e phibar/beta1 <= rtol, and the next iteration's T0 = (1/beta, 0, 0), T1 = (1, -beta/oldb, 0).
__global__ void __launch_bounds__(CG_BLOCKS) minres_scalars_kernel(const double* __restrict__ partial,
                                                                  double* __restrict__ st, int E, int mode,
                                                                  double rtol) {
#pragma clang fp contract(off)  // the rotation exactly as written (no fused multiply-adds)
  __shared__ double red[CG_BLOCKS];
  double* stop = st + ms_stop(E);
  if (*stop != 0.0) {  // uniform: a thread that reads the word after thread 0 rewrote it sees non-zero as well
    if (mode == 1 && threadIdx.x == 0 && *stop == MS_MET) *stop = MS_STOPPED;  // the stopping iteration's tail has run
    return;
  }
  bool not_met = false;
  double* T0 = st + ms_triple(E, 0);
  double* T1 = st + ms_triple(E, 1);
  double* T2 = st + ms_triple(E, 2);
  double* T3 = st + ms_triple(E, 3);
  double* T4 = st + ms_triple(E, 4);
  for (int e = 0; e < E; ++e) {
    const double dot = block_sum_partials(partial, E, e, red);
    if (threadIdx.x != 0) continue;
    auto S = [&](int f) -> double& { return st[(size_t)f * E + e]; };
    if (mode == 1) {
      S(MS_ALFA) = dot;
      T2[e] = 1.0;
      T2[E + e] = S(MS_BETA) > 0.0 ? -dot / S(MS_BETA) : 0.0;
      T2[2 * E + e] = 0.0;
    } else {
      const double alfa = S(MS_ALFA), cs0 = S(MS_CS), sn0 = S(MS_SN), dbar0 = S(MS_DBAR);
      const double oldb = S(MS_BETA);
      const double beta = sqrt(fmax(dot, 0.0));
      const double oldeps = S(MS_EPSLN);
      const double delta = cs0 * dbar0 + sn0 * alfa;
      const double gbar = sn0 * dbar0 - cs0 * alfa;
      const double epsln = sn0 * beta;
      const double dbar = -cs0 * beta;
      const double gamma = fmax(sqrt(gbar * gbar + beta * beta), 1e-300);
      const double cs = gbar / gamma, sn = beta / gamma;
      const double phi = cs * S(MS_PHIBAR);
      const double phibar = sn * S(MS_PHIBAR);
      const bool done0 = S(MS_DONE) != 0.0;
      const double dn = done0 ? 0.0 : 1.0 / gamma;
      T3[e] = dn;
      T3[E + e] = -oldeps * dn;
      T3[2 * E + e] = -delta * dn;
      T4[e] = 1.0;
      T4[E + e] = done0 ? 0.0 : phi;
      T4[2 * E + e] = 0.0;
      S(MS_OLDB) = oldb;
      S(MS_BETA) = beta;
      S(MS_EPSLN) = epsln;
      S(MS_DBAR) = dbar;
      S(MS_CS) = cs;
      S(MS_SN) = sn;
      S(MS_PHIBAR) = phibar;
      const bool done1 = done0 || phibar <= rtol * S(MS_BETA1) || beta == 0.0;
      S(MS_DONE) = done1 ? 1.0 : 0.0;
      // next iteration
      T0[e] = (!done1 && beta > 0.0) ? 1.0 / beta : 0.0;
      T0[E + e] = 0.0;
      T0[2 * E + e] = 0.0;
      T1[e] = 1.0;
      T1[E + e] = oldb > 0.0 ? -beta / oldb : 0.0;
      T1[2 * E + e] = 0.0;
      if (S(MS_BETA1) > 0.0 && !(phibar / S(MS_BETA1) <= rtol)) not_met = true;  // NaN / inf: not met
    }
  }
  if (mode == 2 && threadIdx.x == 0) {
    stop[1] += 1.0;
    if (!not_met) *stop = MS_MET;
  }
}

int minres_solve(kmvp_ctx* c, int kernel, const void* a_host, int E, double rtol, int maxit,
                 double* out_b, int* iters, double* resid) {
  Krylov k;  // x, r1, r2, y, v, w, w1, w2; state: see MS_* above
  if (int rc = solver_begin(c, a_host, E, rtol, maxit, out_b, 8, ms_stop(E), k)) return rc;
  SolveGuard guard{c};
  const bool with_diag = c->diag_on;
  const Diag diag = solver_diag(c);
  const int64_t m = k.m;
  const size_t vec = k.n * sizeof(double);
  double *x = k.vec(0), *r1 = k.vec(1), *r2 = k.vec(2), *y = k.vec(3), *v = k.vec(4);
  double *w = k.vec(5), *w1 = k.vec(6), *w2 = k.vec(7), *st = k.state;

  // r1 = r2 = y = a (widened), x = w = w2 = 0
  int rc = load_rhs(c, a_host, y, k);
  if (rc) return rc;
  HIP_TRY(c, hipMemcpyAsync(r1, y, vec, hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(c, hipMemcpyAsync(r2, y, vec, hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(c, hipMemsetAsync(x, 0, vec, c->stream));
  HIP_TRY(c, hipMemsetAsync(w, 0, vec, c->stream));
  HIP_TRY(c, hipMemsetAsync(w2, 0, vec, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  std::vector<double> dots;
  if ((rc = cg_dots(c, y, y, k, dots))) return rc;

  // ---- device-resident recurrence (see minres_scalars_kernel); the host rotates buffer pointers and
  // looks at the residual every CG_CHECK iterations
  std::vector<double> beta1(E), state(k.stop + 2, 0.0);
  for (int e = 0; e < E; ++e) {
    beta1[e] = std::sqrt(dots[e]);
    state[(size_t)MS_BETA1 * E + e] = beta1[e];
    state[(size_t)MS_BETA * E + e] = beta1[e];
    state[(size_t)MS_CS * E + e] = -1.0;
    state[(size_t)MS_PHIBAR * E + e] = beta1[e];
    const bool zero_rhs = !(beta1[e] > 0.0);  // x = 0
    state[(size_t)MS_DONE * E + e] = zero_rhs ? 1.0 : 0.0;
    state[ms_triple(E, 0) + e] = (!zero_rhs) ? 1.0 / beta1[e] : 0.0;  // T0 = (1/beta, 0, 0)
    state[ms_triple(E, 1) + e] = 1.0;                                   // T1 = (1, 0, 0): no r1 term in iteration 1
  }
  HIP_TRY(c, hipMemcpyAsync(st, state.data(), sizeof(double) * state.size(), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const double* stop = st + k.stop;
  const unsigned vb = blocks_for((int64_t)k.n);
  auto worst = [&]() {
    double wv = 0.0;
    for (int e = 0; e < E; ++e) {
      if (beta1[e] == 0.0) continue;  // zero right-hand side: x = 0
      const double v = state[(size_t)MS_PHIBAR * E + e] / beta1[e];
      fold_worst(wv, v);
    }
    return wv;
  };
  auto dlin3 = [&](double* out, const double* pa, const double* pb, const double* pc, int triple) {
    hipLaunchKernelGGL(vec_lin3_dev_kernel, dim3(vb), dim3(256), 0, c->stream, out, pa, pb, pc,
                       st + ms_triple(E, triple), stop, m, E, (double*)nullptr);
  };
  auto body = [&](int burst) -> int {
    for (int i = 0; i < burst; ++i) {
      // (v = y / beta was written by the previous iteration's tail, or before the first burst)
      if (int rcb = cg_apply(c, kernel, v, k)) return rcb;
      if (with_diag)  // y = (K v + diag v) - (beta / oldb) r1
        hipLaunchKernelGGL(minres_diag_lanczos_kernel, dim3(vb), dim3(256), 0, c->stream, y, (const double*)c->out.p,
                           (const double*)v, (const double*)r1, diag, st + ms_triple(E, 1), stop, m, E);
      else
        dlin3(y, (const double*)c->out.p, r1, nullptr, 1);  // y = K v - (beta / oldb) r1
      hipLaunchKernelGGL(cg_dot_kernel, dim3(CG_BLOCKS), dim3(256), 0, c->stream, v, y, m, E, k.partial);
      hipLaunchKernelGGL(minres_scalars_kernel, dim3(1), dim3(CG_BLOCKS), 0, c->stream, k.partial, st, E, 1, rtol);
      // y - (alfa / beta) r2, written into the old r1 buffer AND back into y
      hipLaunchKernelGGL(vec_lin3_dev_kernel, dim3(vb), dim3(256), 0, c->stream, r1, (const double*)y, (const double*)r2,
                         (const double*)nullptr, st + ms_triple(E, 2), stop, m, E, y);
      std::swap(r1, r2);             // r1 <- r2, r2 <- the new vector
      hipLaunchKernelGGL(cg_dot_kernel, dim3(CG_BLOCKS), dim3(256), 0, c->stream, r2, r2, m, E, k.partial);
      hipLaunchKernelGGL(minres_scalars_kernel, dim3(1), dim3(CG_BLOCKS), 0, c->stream, k.partial, st, E, 2, rtol);
      {  // w_new = (v - oldeps w1 - delta w2) / gamma with w1 <- w2, w2 <- w
        double* t = w1;
        w1 = w2;
        w2 = w;
        w = t;
      }
      // w = T3 . (v, w1, w2);  x = x + phi w;  v = y / beta for the next iteration
      hipLaunchKernelGGL(minres_tail_kernel, dim3(vb), dim3(256), 0, c->stream, w, v, (const double*)w1, (const double*)w2, x,
                         (const double*)y, st + ms_triple(E, 3), st + ms_triple(E, 4), st + ms_triple(E, 0), stop, m, E);
    }
    return KMVP_OK;
  };

  int it = 0;
  double rel = worst();
  dlin3(v, y, nullptr, nullptr, 0);  // v = y / beta of the first iteration
  if ((rc = run_bursts(c, k, maxit, rtol, it, rel, state, body, worst, nullptr))) return rc;

  // true residual ||a - K x (- diag x)|| / ||a||
  if ((rc = true_residual(c, kernel, a_host, x, v, k, dots))) return rc;
  double true_rel = 0.0;
  for (int e = 0; e < E; ++e) {
    if (beta1[e] == 0.0) continue;
    const double v = std::sqrt(dots[e]) / beta1[e];
    fold_worst(true_rel, v);
  }
  return solver_end(c, "MINRES", x, k, out_b, it, true_rel, rtol, iters, resid);
}

}  // namespace kmvp
