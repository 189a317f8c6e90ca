// Pivoted-Cholesky preconditioner of conjugate gradients (include/kmvp.h kmvp_set_solver_preconditioner).
//
// P = L L' + D with L (N, R) the first R <= 128 columns of the pivoted Cholesky factorisation of the kernel matrix K of
// the targets (the full cloud, also on a source shard: no communication, every rank holds the same bits) and D the
// solver's diagonal ridge + d_i > 0.  Everything here is float64 for every working precision; only the kernel column of a
// step is computed in the working precision, with the family's difference form and kval<KERNEL>.
//
// Build, resident on the device (no host look per step).  d = 1 exactly (k(x, x) = 1 for all four kernels); step m:
//   pc_fold_kernel   the argmax of d over the workgroups' partial argmaxes, ties to the smaller index.  d_max <= tau
//                    (tau = 256 unit roundoffs of the working precision: after 128 steps d carries about 128 of them
//                    from the working-precision columns) sets the stop word and the later launches return at once
//   pc_step_kernel   one thread per point: k(x_i, x_piv);  L[m][i] = (k - sum_{t<m} L[t][i] L[t][piv]) / sqrt(d_max);
//                    d[i] = max(d[i] - L[m][i]^2, 0), d[piv] = 0 exactly;  and the workgroup's partial argmax of the new d
// then C = I + L' D^-1 L from per-workgroup partial Gram sums added in workgroup order, copied to the host once, factored
// there (kmvp_precond.hpp) and uploaded.
//
// Apply, z = D^-1 r - D^-1 L C^-1 L' D^-1 r, three launches, no atomics, fixed orders:
//   pc_project_kernel  per-workgroup partials of L' D^-1 r
//   pc_solve_kernel    one workgroup: the partials added in workgroup order, C w = t per column by substitution, 16 rows
//                      at a time
//   pc_finish_kernel   z_i = (r_i - sum_t L[t][i] w_t) / D_i and the partials of r . z
//
// The preconditioned Lanczos quadrature (kmvp_<kernel>_lanczos_quadrature_precond; driver: cg_lanczos_precond) takes from here
//   pc_probe_kernel    the probes z = D^1/2 g + L h, whose covariance is P for Rademacher g and h
//   pc_logd_kernel, pc_logd_fold_kernel   sum_i log D_i, which with log det C off the Cholesky factor (pc_logdet, kept at the
//                      build) is log det P
#include <chrono>

#include "kmvp_ctx.hpp"
#include "kmvp_precond.hpp"

static_assert(kmvp::PRECOND_MAX_RANK == KMVP_PRECOND_MAX_RANK, "kmvp_precond.hpp and include/kmvp.h disagree");

namespace kmvp {

// the residual diagonal below which no further column is taken: 256 unit roundoffs of the working precision
constexpr double PC_TAU_F32 = 256.0 * 5.9604644775390625e-08;   // 2^-24
constexpr double PC_TAU_F64 = 256.0 * 1.1102230246251565e-16;  // 2^-53
constexpr int PC_THREADS = 256;
constexpr int PC_GRAM_BLOCKS = 64;  // workgroups of the Gram sums, each a contiguous run of points
constexpr int PC_GRAM_TILE = 32;    // points per LDS tile there
enum : int { PC_STOP = 0, PC_BUILT, PC_DMAX, PC_CTL };

// The layout of c->precond for N points and rank R, in doubles (the pivots and the argmax indices are int64 in place).
struct PcLayout {
  int64_t n;
  int R, nb;  // nb: workgroups of pc_step_kernel
  size_t dres, invd, L, piv, ctl, amax_v, amax_i, gram, chol, gpart, total;
  PcLayout(int64_t n_, int R_) : n(n_), R(R_), nb((int)blocks_for(n_, PC_THREADS)) {
    size_t o = 0;
    auto take = [&](size_t count) { const size_t at = o; o += count; return at; };
    dres = take((size_t)n);
    invd = take((size_t)n);
    L = take((size_t)R * (size_t)n);
    piv = take((size_t)R);
    ctl = take(PC_CTL);
    amax_v = take((size_t)nb);
    amax_i = take((size_t)nb);
    gram = take((size_t)R * R);
    chol = take((size_t)R * R);
    gpart = take((size_t)PC_GRAM_BLOCKS * R * R);
    total = o;
  }
};

// The larger value wins, ties go to the smaller index; a lane without a candidate passes (-1, INT64_MAX): d is never
// negative.  The result is in sv[0], si[0].
__device__ __forceinline__ void pc_block_argmax(double v, int64_t idx, double* sv, int64_t* si) {
  sv[threadIdx.x] = v;
  si[threadIdx.x] = idx;
  __syncthreads();
  for (int s = PC_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      const double ov = sv[threadIdx.x + s];
      const int64_t oi = si[threadIdx.x + s];
      if (ov > sv[threadIdx.x] || (ov == sv[threadIdx.x] && oi < si[threadIdx.x])) {
        sv[threadIdx.x] = ov;
        si[threadIdx.x] = oi;
      }
    }
    __syncthreads();
  }
}

// d = 1, invd = 1 / (ridge + d_i), and the partial argmaxes of the first step
__global__ void __launch_bounds__(PC_THREADS) pc_init_kernel(double* __restrict__ dres, double* __restrict__ invd, Diag diag,
                                                              int64_t n, double* __restrict__ amax_v,
                                                              int64_t* __restrict__ amax_i) {
  __shared__ double sv[PC_THREADS];
  __shared__ int64_t si[PC_THREADS];
  const int64_t i = (int64_t)blockIdx.x * PC_THREADS + threadIdx.x;
  if (i < n) {
    dres[i] = 1.0;
    invd[i] = 1.0 / diag.at(i);
  }
  pc_block_argmax(i < n ? 1.0 : -1.0, i < n ? i : INT64_MAX, sv, si);
  if (threadIdx.x == 0) {
    amax_v[blockIdx.x] = sv[0];
    amax_i[blockIdx.x] = si[0];
  }
}

// One workgroup: the argmax over the nb partial ones; takes step m or sets the stop word.
__global__ void __launch_bounds__(PC_THREADS) pc_fold_kernel(const double* __restrict__ amax_v,
                                                              const int64_t* __restrict__ amax_i, int nb, int m, double tau,
                                                              int64_t* __restrict__ piv, double* __restrict__ ctl) {
  __shared__ double sv[PC_THREADS];
  __shared__ int64_t si[PC_THREADS];
  if (ctl[PC_STOP] != 0.0) return;  // uniform: every thread reads the same word
  double v = -1.0;
  int64_t idx = INT64_MAX;
  for (int b = threadIdx.x; b < nb; b += PC_THREADS) {  // block order: a later block only wins with a larger value
    const double ov = amax_v[b];
    if (ov > v) {
      v = ov;
      idx = amax_i[b];
    }
  }
  pc_block_argmax(v, idx, sv, si);
  if (threadIdx.x != 0) return;
  if (!(sv[0] > tau)) {
    ctl[PC_STOP] = 1.0;
  } else {
    piv[m] = si[0];
    ctl[PC_DMAX] = sv[0];
    ctl[PC_BUILT] = (double)(m + 1);
  }
}

// Step m for one point per thread (x: the raw row-major targets; the loop over D is a runtime loop).
template <int KERNEL, typename real>
__global__ void __launch_bounds__(PC_THREADS) pc_step_kernel(const real* __restrict__ x, int D, int64_t n, int m,
                                                              double* __restrict__ dres, double* __restrict__ L,
                                                              const int64_t* __restrict__ piv, const double* __restrict__ ctl,
                                                              double* __restrict__ amax_v, int64_t* __restrict__ amax_i) {
  __shared__ double sv[PC_THREADS];
  __shared__ int64_t si[PC_THREADS];
  __shared__ double exp_tab_lds[sizeof(real) == 4 ? 1 : 64];
  const double* exp_tab = exp_tab_lds;
  if (ctl[PC_STOP] != 0.0) return;  // uniform; written by pc_fold_kernel alone
  if constexpr (sizeof(real) == 8) {
    if (threadIdx.x < 64) exp_tab_lds[threadIdx.x] = exp2((double)threadIdx.x * (1.0 / 64.0));
    __syncthreads();
  }
  const int64_t i = (int64_t)blockIdx.x * PC_THREADS + threadIdx.x;
  const int64_t p = piv[m];
  double dv = -1.0;
  int64_t di = INT64_MAX;
  if (i < n) {
    real df = x[i * D] - x[p * D];
    real s = df * df;
    for (int d = 1; d < D; ++d) {
      df = x[i * D + d] - x[p * D + d];
      s = fma(df, df, s);
    }
    const double k = (double)kval<KERNEL>(s, exp_tab);
    double sum = 0.0;
    for (int t = 0; t < m; ++t) sum = fma(L[(int64_t)t * n + i], L[(int64_t)t * n + p], sum);
    const double l = (k - sum) / sqrt(ctl[PC_DMAX]);
    L[(int64_t)m * n + i] = l;
    dv = i == p ? 0.0 : fmax(dres[i] - l * l, 0.0);
    dres[i] = dv;
    di = i;
  }
  pc_block_argmax(dv, di, sv, si);
  if (threadIdx.x == 0) {
    amax_v[blockIdx.x] = sv[0];
    amax_i[blockIdx.x] = si[0];
  }
}

// gpart[block][t][s] = sum over the block's run of points of L[t][i] L[s][i] / D_i, t, s < R.  256 threads as 16 x 16, each
// with an 8 x 8 tile of (t, s); rows R .. 127 of the LDS tile are 0.
__global__ void __launch_bounds__(PC_THREADS) pc_gram_kernel(const double* __restrict__ L, const double* __restrict__ invd,
                                                              int64_t n, int R, int64_t chunk, double* __restrict__ gpart) {
  __shared__ double ls[PC_GRAM_TILE][PRECOND_MAX_RANK + 1];
  __shared__ double wd[PC_GRAM_TILE];
  const int ty = threadIdx.x / 16, tx = threadIdx.x % 16;
  double acc[8][8];
#pragma unroll
  for (int a = 0; a < 8; ++a)
#pragma unroll
    for (int b = 0; b < 8; ++b) acc[a][b] = 0.0;
  const int64_t i0 = (int64_t)blockIdx.x * chunk;
  const int64_t i1 = i0 + chunk < n ? i0 + chunk : n;
  for (int64_t base = i0; base < i1; base += PC_GRAM_TILE) {
    for (int q = threadIdx.x; q < PC_GRAM_TILE * PRECOND_MAX_RANK; q += PC_THREADS) {
      const int r = q / PC_GRAM_TILE, pt = q % PC_GRAM_TILE;
      ls[pt][r] = (r < R && base + pt < i1) ? L[(int64_t)r * n + base + pt] : 0.0;
    }
    if (threadIdx.x < PC_GRAM_TILE) wd[threadIdx.x] = base + threadIdx.x < i1 ? invd[base + threadIdx.x] : 0.0;
    __syncthreads();
    for (int pt = 0; pt < PC_GRAM_TILE; ++pt) {
      double lt[8], lsv[8];
#pragma unroll
      for (int a = 0; a < 8; ++a) lt[a] = ls[pt][ty + 16 * a] * wd[pt];
#pragma unroll
      for (int b = 0; b < 8; ++b) lsv[b] = ls[pt][tx + 16 * b];
#pragma unroll
      for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) acc[a][b] = fma(lt[a], lsv[b], acc[a][b]);
    }
    __syncthreads();
  }
  double* out = gpart + (size_t)blockIdx.x * R * R;
#pragma unroll
  for (int a = 0; a < 8; ++a)
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const int t = ty + 16 * a, s = tx + 16 * b;
      if (t < R && s < R) out[t * R + s] = acc[a][b];
    }
}

// gram[t][s] = (t == s) + the partial sums in block order
__global__ void pc_gram_fold_kernel(const double* __restrict__ gpart, int R, double* __restrict__ gram) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= R * R) return;
  double v = 0.0;
  for (int b = 0; b < PC_GRAM_BLOCKS; ++b) v += gpart[(size_t)b * R * R + q];
  gram[q] = v + (q / R == q % R ? 1.0 : 0.0);
}

template <typename real>
static hipError_t launch_step(kmvp_ctx* c, int kernel, const PcLayout& lay, double* buf, int m) {
  const real* x = (const real*)(c->same_points ? c->y_raw.p : c->x_raw.p);
  double* amax_v = buf + lay.amax_v;
  int64_t* amax_i = (int64_t*)(buf + lay.amax_i);
  const int64_t* piv = (const int64_t*)(buf + lay.piv);
#define KMVP_PC_STEP(K)                                                                                               \
  hipLaunchKernelGGL((pc_step_kernel<K, real>), dim3(lay.nb), dim3(PC_THREADS), 0, c->stream, x, c->D, lay.n, m,       \
                     buf + lay.dres, buf + lay.L, piv, (const double*)(buf + lay.ctl), amax_v, amax_i)
  switch (kernel) {
    case K_GAUSSIAN: KMVP_PC_STEP(K_GAUSSIAN); break;
    case K_ABSEXP: KMVP_PC_STEP(K_ABSEXP); break;
    case K_MATERN32: KMVP_PC_STEP(K_MATERN32); break;
    case K_MATERN52: KMVP_PC_STEP(K_MATERN52); break;
    default: return hipErrorInvalidValue;
  }
#undef KMVP_PC_STEP
  return hipGetLastError();
}

int precond_prepare(kmvp_ctx* c, int kernel) {
  const int R = c->precond_rank;
  if (c->pc_points_ver == c->points_ver && c->pc_kernel == kernel && c->pc_rank == R && c->pc_diag_ver == c->diag_ver)
    return KMVP_OK;  // the factor is the one of this system
  const auto t0 = std::chrono::steady_clock::now();
  c->pc_points_ver = 0;  // no factor while it is being rebuilt
  c->pc_built = 0;
  const PcLayout lay(c->N, R);
  if (int rc = ensure(c, c->precond, sizeof(double) * lay.total)) return rc;
  double* buf = (double*)c->precond.p;
  const bool f64 = c->dtype == KMVP_F64;
  const double tau = f64 ? PC_TAU_F64 : PC_TAU_F32;
  // L = 0 (a build that stops early leaves its later rows 0), pivots and control words = 0
  HIP_TRY(c, hipMemsetAsync(buf + lay.L, 0, sizeof(double) * ((size_t)R * lay.n + R + PC_CTL), c->stream));
  hipLaunchKernelGGL(pc_init_kernel, dim3(lay.nb), dim3(PC_THREADS), 0, c->stream, buf + lay.dres, buf + lay.invd,
                     solver_diag(c), lay.n, buf + lay.amax_v, (int64_t*)(buf + lay.amax_i));
  HIP_TRY(c, hipGetLastError());
  for (int m = 0; m < R; ++m) {
    hipLaunchKernelGGL(pc_fold_kernel, dim3(1), dim3(PC_THREADS), 0, c->stream, (const double*)(buf + lay.amax_v),
                       (const int64_t*)(buf + lay.amax_i), lay.nb, m, tau, (int64_t*)(buf + lay.piv), buf + lay.ctl);
    HIP_TRY(c, f64 ? launch_step<double>(c, kernel, lay, buf, m) : launch_step<float>(c, kernel, lay, buf, m));
  }
  const int64_t chunk = (lay.n + PC_GRAM_BLOCKS - 1) / PC_GRAM_BLOCKS;
  hipLaunchKernelGGL(pc_gram_kernel, dim3(PC_GRAM_BLOCKS), dim3(PC_THREADS), 0, c->stream, (const double*)(buf + lay.L),
                     (const double*)(buf + lay.invd), lay.n, R, chunk, buf + lay.gpart);
  hipLaunchKernelGGL(pc_gram_fold_kernel, dim3(blocks_for((int64_t)R * R)), dim3(256), 0, c->stream,
                     (const double*)(buf + lay.gpart), R, buf + lay.gram);
  HIP_TRY(c, hipGetLastError());
  // the one look of the host: the control words and C
  std::vector<double> ctl(PC_CTL), gram((size_t)R * R);
  HIP_TRY(c, hipMemcpyAsync(ctl.data(), buf + lay.ctl, sizeof(double) * PC_CTL, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(gram.data(), buf + lay.gram, sizeof(double) * gram.size(), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const int built = (int)ctl[PC_BUILT];
  if (built < 0 || built > R) return fail(c, KMVP_E_DEVICE, "preconditioner: the build left an impossible column count");
  if (!pc_cholesky(gram.data(), built, R))
    return fail(c, KMVP_E_INVALID, "preconditioner: I + L' D^-1 L is not positive definite (non-finite points or diagonal?)");
  HIP_TRY(c, hipMemcpyAsync(buf + lay.chol, gram.data(), sizeof(double) * gram.size(), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // gram is a local
  c->pc_logdet_c = pc_logdet(gram.data(), built, R);
  c->pc_built = built;
  c->pc_kernel = kernel;
  c->pc_rank = R;
  c->pc_points_ver = c->points_ver;
  c->pc_diag_ver = c->diag_ver;
  c->last_precond_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return KMVP_OK;
}

// ------------------------------------------------------------------------------------
// apply

// part[block][t][e] = sum over the block's run of points of L[t][i] r[i][e] / D_i.  Every wavefront takes the rows
// t = wave, wave + 4, ...; its lanes stride over the points and fold by shuffles in a fixed order.
__global__ void __launch_bounds__(PC_THREADS) pc_project_kernel(const double* __restrict__ L, const double* __restrict__ invd,
                                                                 int64_t n, int R, const double* __restrict__ r, int E,
                                                                 const double* __restrict__ stop, double* __restrict__ part) {
  if (*stop != 0.0) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t chunk = (n + gridDim.x - 1) / gridDim.x;
  const int64_t i0 = (int64_t)blockIdx.x * chunk;
  const int64_t i1 = i0 + chunk < n ? i0 + chunk : n;
  for (int e = 0; e < E; ++e)
    for (int t = wave; t < R; t += PC_THREADS / 64) {
      const double* row = L + (int64_t)t * n;
      double acc = 0.0;
      for (int64_t i = i0 + lane; i < i1; i += 64) acc = fma(row[i], r[i * E + e] * invd[i], acc);
      for (int s = 32; s > 0; s >>= 1) acc += __shfl_down(acc, s);
      if (lane == 0) part[((size_t)blockIdx.x * R + t) * E + e] = acc;
    }
}

// One workgroup.  w[t][e] = the partials in block order; then C w = t per column with the uploaded factor G, C = G G'.
// One thread walking pc_forward() and pc_backward() over the whole factor in global memory took 914 us at rank 128 (a
// chain of 16 000 dependent loads), a fifth of the float64 Gaussian operator at N = 1e5.  Hence in blocks of 16 rows: the
// part of a block's right-hand side that the rows already solved determine is a matrix-vector product for all 256
// threads (coalesced reads of G, 16 partial sums per row added in a fixed order), and only the 16 x 16 diagonal block,
// copied to LDS, goes through pc_forward() / pc_backward() in one thread.
constexpr int PC_SOLVE_BLOCK = 16;
__global__ void __launch_bounds__(PC_THREADS) pc_solve_kernel(const double* __restrict__ part, int nblocks,
                                                               const double* __restrict__ chol, int R, int ld, int E,
                                                               const double* __restrict__ stop, double* __restrict__ w) {
  constexpr int B = PC_SOLVE_BLOCK;
  static_assert(B * B == PC_THREADS, "one thread per element of a diagonal block");
  __shared__ double gb[B][B + 1];
  __shared__ double red[B][B + 1];
  __shared__ double vv[PRECOND_MAX_RANK];
  if (*stop != 0.0) return;
  const int tid = threadIdx.x, hi = tid / B, lo = tid % B;
  const int nbk = (R + B - 1) / B;
  for (int e = 0; e < E; ++e) {
    if (tid < R) {
      double acc = 0.0;
      for (int b = 0; b < nblocks; ++b) acc += part[((size_t)b * R + tid) * E + e];
      vv[tid] = acc;
    }
    __syncthreads();
    for (int b = 0; b < nbk; ++b) {  // G y = t, top down
      const int i0 = b * B, rows = R - i0 < B ? R - i0 : B;
      double s = 0.0;  // row i0 + hi, columns lo, lo + 16, ... < i0
      if (hi < rows)
        for (int k = lo; k < i0; k += B) s = fma(chol[(i0 + hi) * ld + k], vv[k], s);
      red[hi][lo] = s;
      if (hi < rows && lo < rows) gb[hi][lo] = chol[(i0 + hi) * ld + i0 + lo];
      __syncthreads();
      if (tid < rows) {
        double t = 0.0;
        for (int q = 0; q < B; ++q) t += red[tid][q];
        vv[i0 + tid] -= t;
      }
      __syncthreads();
      if (tid == 0) pc_forward(&gb[0][0], rows, B + 1, vv + i0, 1);
      __syncthreads();
    }
    for (int b = nbk - 1; b >= 0; --b) {  // G' w = y, bottom up
      const int i0 = b * B, rows = R - i0 < B ? R - i0 : B;
      double s = 0.0;  // column i0 + lo of G, rows i0 + 16 + hi, + 16, ... < R
      if (lo < rows)
        for (int k = i0 + B + hi; k < R; k += B) s = fma(chol[k * ld + i0 + lo], vv[k], s);
      red[lo][hi] = s;
      if (hi < rows && lo < rows) gb[hi][lo] = chol[(i0 + hi) * ld + i0 + lo];
      __syncthreads();
      if (tid < rows) {
        double t = 0.0;
        for (int q = 0; q < B; ++q) t += red[tid][q];
        vv[i0 + tid] -= t;
      }
      __syncthreads();
      if (tid == 0) pc_backward(&gb[0][0], rows, B + 1, vv + i0, 1);
      __syncthreads();
    }
    if (tid < R) w[tid * E + e] = vv[tid];
    __syncthreads();
  }
}

// z[i][e] = (r[i][e] - sum_t L[t][i] w[t][e]) / D_i, and partial[block][e] = the block's share of r . z (cg_dot_kernel's
// layout and summation order)
__global__ void __launch_bounds__(PC_THREADS) pc_finish_kernel(const double* __restrict__ L, int64_t n, int R,
                                                                const double* __restrict__ r, const double* __restrict__ w,
                                                                Diag diag, int E, const double* __restrict__ stop,
                                                                double* __restrict__ z, double* __restrict__ partial) {
  __shared__ double red[PC_THREADS];
  __shared__ double we[PRECOND_MAX_RANK];
  if (*stop != 0.0) return;
  for (int e = 0; e < E; ++e) {
    if ((int)threadIdx.x < R) we[threadIdx.x] = w[threadIdx.x * E + e];
    __syncthreads();
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
      double s = 0.0;
      for (int t = 0; t < R; ++t) s = fma(L[(int64_t)t * n + i], we[t], s);
      const double rv = r[i * E + e];
      const double zv = (rv - s) / diag.at(i);
      z[i * E + e] = zv;
      acc += rv * zv;
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = PC_THREADS / 2; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) partial[(int64_t)blockIdx.x * E + e] = red[0];
    __syncthreads();
  }
}

void precond_apply(kmvp_ctx* c, const double* r, double* z, int E, double* scratch, double* rz_partial, int rz_blocks,
                   const double* stop) {
  const PcLayout lay(c->N, c->pc_rank);
  const double* buf = (const double*)c->precond.p;
  const int R = c->pc_built;
  double* part = scratch;
  double* w = scratch + (size_t)PC_APPLY_BLOCKS * R * E;
  hipLaunchKernelGGL(pc_project_kernel, dim3(PC_APPLY_BLOCKS), dim3(PC_THREADS), 0, c->stream, buf + lay.L, buf + lay.invd,
                     lay.n, R, r, E, stop, part);
  hipLaunchKernelGGL(pc_solve_kernel, dim3(1), dim3(PC_THREADS), 0, c->stream, (const double*)part, PC_APPLY_BLOCKS,
                     buf + lay.chol, R, lay.R, E, stop, w);
  hipLaunchKernelGGL(pc_finish_kernel, dim3(rz_blocks), dim3(PC_THREADS), 0, c->stream, buf + lay.L, lay.n, R, r,
                     (const double*)w, solver_diag(c), E, stop, z, rz_partial);
}

// ------------------------------------------------------------------------------------
// the preconditioned quadrature's share (kmvp_<kernel>_lanczos_quadrature_precond): probes with covariance P, log det D

// z[i][e] = sqrt(D_i) g[i][e] + sum_t L[t][i] h[t][e], t ascending, one fma per term.  One thread per (i, e): a workgroup
// is 256 consecutive points of one column (blockIdx.y), so a row of L is read coalesced and h[t][e] is uniform.
__global__ void __launch_bounds__(PC_THREADS) pc_probe_kernel(const double* __restrict__ L, int64_t n, int R, Diag diag,
                                                               const double* __restrict__ g, const double* __restrict__ h,
                                                               int P, double* __restrict__ z) {
  const int64_t i = (int64_t)blockIdx.x * PC_THREADS + threadIdx.x;
  const int e = blockIdx.y;
  if (i >= n) return;
  double acc = sqrt(diag.at(i)) * g[i * P + e];
  for (int t = 0; t < R; ++t) acc = fma(L[(int64_t)t * n + i], h[(int64_t)t * P + e], acc);
  z[i * P + e] = acc;
}

// part[block] = sum of log D_i over the block's contiguous run of points (pc_gram_kernel's mapping): every thread its
// strided share in ascending i, then the tree over the 256 threads.
__global__ void __launch_bounds__(PC_THREADS) pc_logd_kernel(Diag diag, int64_t n, int64_t chunk, double* __restrict__ part) {
  __shared__ double red[PC_THREADS];
  const int64_t i0 = (int64_t)blockIdx.x * chunk;
  const int64_t i1 = i0 + chunk < n ? i0 + chunk : n;
  double acc = 0.0;
  for (int64_t i = i0 + threadIdx.x; i < i1; i += PC_THREADS) acc += log(diag.at(i));
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = PC_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

// part[nblocks] = the partial sums in block order
__global__ void pc_logd_fold_kernel(double* __restrict__ part, int nblocks) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double v = 0.0;
  for (int b = 0; b < nblocks; ++b) v += part[b];
  part[nblocks] = v;
}

void precond_probes(kmvp_ctx* c, const double* g, const double* h, int P, double* z) {
  const PcLayout lay(c->N, c->pc_rank);
  const double* buf = (const double*)c->precond.p;
  hipLaunchKernelGGL(pc_probe_kernel, dim3(lay.nb, P), dim3(PC_THREADS), 0, c->stream, buf + lay.L, lay.n, c->pc_built,
                     solver_diag(c), g, h, P, z);
}

void precond_logdiag(kmvp_ctx* c, double* out) {
  const int64_t n = c->N;
  const int64_t chunk = (n + PC_LOGD_BLOCKS - 1) / PC_LOGD_BLOCKS;
  hipLaunchKernelGGL(pc_logd_kernel, dim3(PC_LOGD_BLOCKS), dim3(PC_THREADS), 0, c->stream, solver_diag(c), n, chunk, out);
  hipLaunchKernelGGL(pc_logd_fold_kernel, dim3(1), dim3(64), 0, c->stream, out, PC_LOGD_BLOCKS);
}

int precond_read(kmvp_ctx* c, int* rank_built, int64_t* pivots, double* factor) {
  if (!c) return KMVP_E_INVALID;
  if (!rank_built) return fail(c, KMVP_E_INVALID, "kmvp_get_solver_preconditioner: rank_built is NULL");
  *rank_built = c->pc_used;
  if (c->pc_used == 0 || (!pivots && !factor)) return KMVP_OK;
  if (c->pc_points_ver != c->points_ver || !c->precond.p)
    return fail(c, KMVP_E_INVALID, "kmvp_get_solver_preconditioner: the points changed since the solve that used the factor");
  HIP_TRY(c, hipSetDevice(c->device));
  const PcLayout lay(c->N, c->pc_rank);
  const double* buf = (const double*)c->precond.p;
  if (pivots)
    HIP_TRY(c, hipMemcpyAsync(pivots, buf + lay.piv, sizeof(int64_t) * c->pc_used, hipMemcpyDeviceToHost, c->stream));
  if (factor)
    HIP_TRY(c, hipMemcpyAsync(factor, buf + lay.L, sizeof(double) * (size_t)c->pc_used * lay.n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return KMVP_OK;
}

}  // namespace kmvp
