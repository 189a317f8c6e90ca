// kmvp_<kernel>_eigsh: the k algebraically largest eigenpairs of the kernel matrix (plain, centred or degree-normalised)
// by the Lanczos process with full reorthogonalisation, the iteration on the device (include/kmvp.h states the
// algorithm).  The operator is cg_apply (kmvp_solvers.hip), as for the Krylov solvers; what is new here is the basis
// that is kept, V [vector][ld] float64 with one Lanczos vector contiguous, and the tall-skinny work on it:
//   eig_proj_kernel   partial[block][vector] = the block's rows of V_j' w      } classical Gram-Schmidt, twice per step:
//   eig_reduce_kernel h[vector] = sum over the blocks, in block order          } four passes over the basis, each reading
//   eig_sub_kernel    w -= V_j h (and, in the second round, the block's |w|^2)  } it once, with the same row ownership
//   eig_scalar_kernel alpha_j, beta_j, the history, the breakdown test and the stop word
//   eig_normalize_kernel v_{j+1} = w / beta_j, beta read from device memory
// Between two looks of the host (kmvp_tridiag.hpp on the history) nothing crosses to it.  Every sum has a fixed order and
// there are no atomics: the same inputs give the same bits.
#include "kmvp_ctx.hpp"
#include "kmvp_tridiag.hpp"

namespace kmvp {

constexpr int EIG_BLOCKS = 256;   // workgroups of the passes over the basis: fixed, so the summation order is
constexpr int EIG_THREADS = 256;  // four wavefronts per workgroup
constexpr int EIG_CHUNK = 2 * EIG_THREADS;  // rows a workgroup holds in registers at a time: one 16-byte pair per lane
constexpr int EIG_MAX_STEPS = 512;
constexpr int EIG_UNROLL = 4;     // eig_sub_kernel: basis vectors whose loads are in flight together
constexpr int EIG_VB = 16;        // eig_proj_kernel: basis vectors per trip (the LDS reduction below is written for 16)
constexpr int EIG_LOOK = 8;       // steps between two looks of the host
constexpr double EIG_BREAKDOWN = 1e-13;
enum : int { ST_STOP = 0, ST_COUNT = 1, ST_AMAX = 2, ST_WORDS = 4 };
enum : int { STOP_NONE = 0, STOP_BREAKDOWN = 1, STOP_NONFINITE = 2 };

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// The block's rows [r0, r1) of V_j' w: a workgroup owns `rows_per_block` contiguous rows (even, so that every 16-byte pair
// lies inside one range; ld is even and the pad rows of V and w are zero), takes them EIG_CHUNK at a time with its piece
// of w in registers, and walks the nv vectors EIG_VB at a time with one coalesced 16-byte load per lane and vector, all
// EIG_VB loads in flight together.  A wavefront adds its 64 lanes through an LDS tile [vector][lane]: lane l adds 16
// lanes' terms of vector l mod 16 in lane order, two shuffles add the four quarters -- 16 LDS writes, 16 reads and 2
// shuffles per lane and 16 vectors (a shuffle tree per vector, 6 per vector, ran the pass at a third of eig_sub_kernel's
// rate).  The wavefronts' sums stay in LDS and are added in wavefront order at the end.
__global__ void __launch_bounds__(EIG_THREADS) eig_proj_kernel(const double* __restrict__ V, int64_t ld,
                                                              const double* __restrict__ w, int nv, int64_t rows_per_block,
                                                              int pl, double* __restrict__ partial,
                                                              const double* __restrict__ st) {
  if (st[ST_STOP] != 0.0) return;
  __shared__ double acc[4][EIG_MAX_STEPS + EIG_VB];
  __shared__ double tile[4][EIG_VB][65];  // 65: the quarter sums read down a column of lanes without bank conflicts
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int mine = lane & (EIG_VB - 1), quarter = lane >> 4;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < ld ? r0 + rows_per_block : ld;
  for (int64_t c0 = r0; c0 == r0 || c0 < r1; c0 += EIG_CHUNK) {  // a block past the end still writes its zeros
    const int64_t row = c0 + 2 * (int64_t)threadIdx.x;
    const bool in = row < r1;
    const double2 wp = in ? *reinterpret_cast<const double2*>(w + row) : make_double2(0.0, 0.0);
    for (int v = 0; v < nv; v += EIG_VB) {  // (every trip count here is uniform over the workgroup)
      double2 x[EIG_VB];
#pragma unroll
      for (int u = 0; u < EIG_VB; ++u)
        x[u] = v + u < nv && in ? *reinterpret_cast<const double2*>(V + (int64_t)(v + u) * ld + row) : make_double2(0.0, 0.0);
#pragma unroll
      for (int u = 0; u < EIG_VB; ++u) tile[wave][u][lane] = wp.x * x[u].x + wp.y * x[u].y;
      __syncthreads();
      double t = 0.0;
#pragma unroll
      for (int i = 0; i < 16; ++i) t += tile[wave][mine][quarter * 16 + i];
      t += __shfl_xor(t, 16);
      t += __shfl_xor(t, 32);
      if (lane < EIG_VB && v + lane < nv) acc[wave][v + lane] = (c0 == r0 ? 0.0 : acc[wave][v + lane]) + t;
      __syncthreads();
    }
  }
  __syncthreads();
  for (int v = threadIdx.x; v < nv; v += EIG_THREADS)
    partial[(int64_t)blockIdx.x * pl + v] = ((acc[0][v] + acc[1][v]) + acc[2][v]) + acc[3][v];
}

// h[v] = sum over the EIG_BLOCKS partials of vector v in a fixed order: one wavefront per vector, lane l adds blocks l,
// l + 64, ... in turn, then the 64 lanes are added by shuffles.  (One lane per vector walking the 256 partials took 13 us
// per launch at 32 vectors, more than the projection it finishes.)
__global__ void __launch_bounds__(EIG_THREADS) eig_reduce_kernel(const double* __restrict__ partial, int pl, int nv,
                                                                double* __restrict__ h, const double* __restrict__ st) {
  if (st[ST_STOP] != 0.0) return;
  const int lane = threadIdx.x & 63;
  const int v = blockIdx.x * (EIG_THREADS / 64) + (threadIdx.x >> 6);
  if (v >= nv) return;  // uniform over the wavefront
  double s = 0.0;
#pragma unroll
  for (int b = lane; b < EIG_BLOCKS; b += 64) s += partial[(int64_t)b * pl + v];
  s = wave_sum(s);
  if (lane == 0) h[v] = s;
}

// w -= V_j h on eig_proj_kernel's row ownership, h read through the scalar cache (its index is uniform), vectors in
// ascending order.  npartial != NULL: also the block's share of |w|^2 of the new w, for beta.
__global__ void __launch_bounds__(EIG_THREADS) eig_sub_kernel(const double* __restrict__ V, int64_t ld, double* __restrict__ w,
                                                             const double* __restrict__ h, int nv, int64_t rows_per_block,
                                                             double* __restrict__ npartial, const double* __restrict__ st) {
  if (st[ST_STOP] != 0.0) return;
  __shared__ double red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < ld ? r0 + rows_per_block : ld;
  double norm2 = 0.0;
  for (int64_t c0 = r0; c0 < r1; c0 += EIG_CHUNK) {
    const int64_t row = c0 + 2 * (int64_t)threadIdx.x;
    if (row >= r1) continue;
    double2 wp = *reinterpret_cast<const double2*>(w + row);
    for (int v = 0; v < nv; v += EIG_UNROLL) {
      double2 x[EIG_UNROLL];
#pragma unroll
      for (int u = 0; u < EIG_UNROLL; ++u)
        x[u] = v + u < nv ? *reinterpret_cast<const double2*>(V + (int64_t)(v + u) * ld + row) : make_double2(0.0, 0.0);
#pragma unroll
      for (int u = 0; u < EIG_UNROLL; ++u) {
        if (v + u >= nv) continue;
        const double hv = h[v + u];
        wp.x -= hv * x[u].x;
        wp.y -= hv * x[u].y;
      }
    }
    *reinterpret_cast<double2*>(w + row) = wp;
    norm2 += wp.x * wp.x + wp.y * wp.y;
  }
  if (!npartial) return;
  norm2 = wave_sum(norm2);
  if (lane == 0) red[wave] = norm2;
  __syncthreads();
  if (threadIdx.x == 0) npartial[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// One block.  alpha_j = h_j + h'_j, beta_j = sqrt(sum of the blocks' |w|^2) (fixed tree), both appended to the history at
// row jj = j - 1; the count; the breakdown test beta_j <= 1e-13 max_i |alpha_i| and the non-finite test set the stop word,
// after which every kernel of the burst returns at once (v_{j+1} is not formed).
__global__ void __launch_bounds__(EIG_BLOCKS) eig_scalar_kernel(const double* __restrict__ npartial, const double* __restrict__ h1,
                                                               const double* __restrict__ h2, int jj, double* __restrict__ st,
                                                               double* __restrict__ hist_alpha, double* __restrict__ hist_beta) {
  __shared__ double red[EIG_BLOCKS];
  if (st[ST_STOP] != 0.0) return;  // uniform: every thread reads the same word
  red[threadIdx.x] = npartial[threadIdx.x];
  __syncthreads();
  for (int s = EIG_BLOCKS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const double alpha = h1[jj] + h2[jj];
  const double beta = sqrt(red[0]);
  hist_alpha[jj] = alpha;
  hist_beta[jj] = beta;
  const double amax = fmax(st[ST_AMAX], fabs(alpha));
  st[ST_AMAX] = amax;
  st[ST_COUNT] = (double)(jj + 1);
  if (!(isfinite(alpha) && isfinite(beta)))
    st[ST_STOP] = (double)STOP_NONFINITE;
  else if (beta <= EIG_BREAKDOWN * amax)
    st[ST_STOP] = (double)STOP_BREAKDOWN;
}

// v_{j+1} = w / beta_j over the ld padded rows (the pad of w is zero)
__global__ void eig_normalize_kernel(const double* __restrict__ w, const double* __restrict__ beta, double* __restrict__ vnext,
                                     int64_t ld, const double* __restrict__ st) {
  if (st[ST_STOP] != 0.0) return;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < ld) vnext[i] = w[i] / *beta;
}

// ---- the operator around the product, on (n, E) row-major blocks: E = 1 in a step, E = k for the true residuals

// partial[block][e] = the block's share of the column sums of x (cg_dot_kernel's pattern)
__global__ void eig_colsum_kernel(const double* __restrict__ x, int64_t n, int E, double* __restrict__ partial,
                                  const double* __restrict__ st) {
  if (st[ST_STOP] != 0.0) return;
  __shared__ double red[256];
  for (int e = 0; e < E; ++e) {
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
      acc += x[i * E + e];
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

// One block.  mean[e] = (sum of the EIG_BLOCKS partials of column e, fixed tree) / n
__global__ void __launch_bounds__(EIG_BLOCKS) eig_mean_kernel(const double* __restrict__ partial, int E, int64_t n,
                                                             double* __restrict__ mean, const double* __restrict__ st) {
  __shared__ double red[EIG_BLOCKS];
  if (st[ST_STOP] != 0.0) return;
  for (int e = 0; e < E; ++e) {
    red[threadIdx.x] = partial[(int64_t)threadIdx.x * E + e];
    __syncthreads();
    for (int s = EIG_BLOCKS / 2; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) mean[e] = red[0] / (double)n;
    __syncthreads();
  }
}

// out = in - mean per column
__global__ void eig_center_kernel(const double* __restrict__ in, const double* __restrict__ mean, double* __restrict__ out,
                                  int64_t count, int E, const double* __restrict__ st) {
  if (st[ST_STOP] != 0.0) return;
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q < count) out[q] = in[q] - mean[q % E];
}

// out = s_i in per row (the degree scaling S = diag(q^-1/2))
__global__ void eig_rowscale_kernel(const double* __restrict__ in, const double* __restrict__ s, double* __restrict__ out,
                                    int64_t count, int E, const double* __restrict__ st) {
  if (st[ST_STOP] != 0.0) return;
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q < count) out[q] = s[q / E] * in[q];
}

// out = K x + diag x (the solver's diagonal), or the plain copy of K x
__global__ void eig_diag_kernel(const double* __restrict__ Kx, const double* __restrict__ x, Diag diag, int with_diag,
                                double* __restrict__ out, int64_t count, int E, const double* __restrict__ st) {
  if (st[ST_STOP] != 0.0) return;
  const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (q < count) out[q] = with_diag ? Kx[q] + diag.at(q / E) * x[q] : Kx[q];
}

// s = q^-1/2 of the degrees q = K 1
__global__ void eig_rsqrt_kernel(const double* __restrict__ q, double* __restrict__ s, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) s[i] = 1.0 / sqrt(q[i]);
}

// ---- after the stop

// X (n, k) = V_j S: one row per lane, eight columns at a time, the vectors in ascending order; S (nv, k) through the
// scalar cache
__global__ void eig_ritz_kernel(const double* __restrict__ V, int64_t ld, const double* __restrict__ S, int nv, int k,
                                double* __restrict__ X, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  for (int c0 = 0; c0 < k; c0 += 8) {
    double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int v = 0; v < nv; ++v) {
      const double x = V[(int64_t)v * ld + i];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (c0 + u < k) a[u] += x * S[(int64_t)v * k + c0 + u];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (c0 + u < k) X[i * k + c0 + u] = a[u];
  }
}

// One block per column: the column is divided by its norm and given the sign that makes its component of largest
// magnitude positive (a tie goes to the smallest index).
__global__ void __launch_bounds__(256) eig_colfix_kernel(double* __restrict__ X, int64_t n, int k) {
  __shared__ double red[256], big[256];
  __shared__ int64_t at[256];
  const int c = blockIdx.x;
  double ss = 0.0, best = -1.0;
  int64_t where = 0;
  for (int64_t i = threadIdx.x; i < n; i += 256) {
    const double x = X[i * k + c];
    ss += x * x;
    if (fabs(x) > best) {
      best = fabs(x);
      where = i;
    }
  }
  red[threadIdx.x] = ss;
  big[threadIdx.x] = best;
  at[threadIdx.x] = where;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      red[threadIdx.x] += red[threadIdx.x + s];
      const double ob = big[threadIdx.x + s];
      const int64_t oa = at[threadIdx.x + s];
      if (ob > big[threadIdx.x] || (ob == big[threadIdx.x] && oa < at[threadIdx.x])) {
        big[threadIdx.x] = ob;
        at[threadIdx.x] = oa;
      }
    }
    __syncthreads();
  }
  const double norm = sqrt(red[0]);
  const double sign = X[at[0] * k + c] < 0.0 ? -1.0 : 1.0;
  __syncthreads();
  for (int64_t i = threadIdx.x; i < n; i += 256) X[i * k + c] = sign * (X[i * k + c] / norm);
}

// One block per column: resid[c] = |A x_c - theta_c x_c| / (|theta_1| |x_c|)
__global__ void __launch_bounds__(256) eig_resid_kernel(const double* __restrict__ AX, const double* __restrict__ X,
                                                       const double* __restrict__ theta, int64_t n, int k,
                                                       double* __restrict__ resid) {
  __shared__ double r2[256], x2[256];
  const int c = blockIdx.x;
  const double th = theta[c];
  double a = 0.0, b = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 256) {
    const double x = X[i * k + c];
    const double r = AX[i * k + c] - th * x;
    a += r * r;
    b += x * x;
  }
  r2[threadIdx.x] = a;
  x2[threadIdx.x] = b;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      r2[threadIdx.x] += r2[threadIdx.x + s];
      x2[threadIdx.x] += x2[threadIdx.x + s];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) resid[c] = sqrt(r2[0]) / (fabs(theta[0]) * sqrt(x2[0]));
}

// ------------------------------------------------------------------------------------

namespace {

struct Eig {
  kmvp_ctx* c;
  int kernel, op;
  int64_t n, ld, rows_per_block;
  int pl;
  bool with_diag;
  Diag diag;
  double *V, *w, *t, *X, *R, *sq, *deg, *partial, *h1, *h2, *npartial, *cpartial, *mean, *st, *hist, *S, *theta, *resid;

  // out (n, E; for E == 1 it may be the padded w) = A x for the (n, E) block x
  int apply(const double* x, int E, double* out) {
    hipStream_t s = c->stream;
    const int64_t count = n * E;
    const unsigned blocks = blocks_for(count);
    Krylov k;
    k.m = n;
    k.E = E;
    k.n = (size_t)count;
    const double* in = x;
    if (op == KMVP_EIG_CENTERED) {
      hipLaunchKernelGGL(eig_colsum_kernel, dim3(EIG_BLOCKS), dim3(256), 0, s, x, n, E, cpartial, st);
      hipLaunchKernelGGL(eig_mean_kernel, dim3(1), dim3(EIG_BLOCKS), 0, s, cpartial, E, n, mean, st);
      hipLaunchKernelGGL(eig_center_kernel, dim3(blocks), dim3(256), 0, s, x, mean, t, count, E, st);
      in = t;
    } else if (op == KMVP_EIG_NORMALIZED) {
      hipLaunchKernelGGL(eig_rowscale_kernel, dim3(blocks), dim3(256), 0, s, x, sq, t, count, E, st);
      in = t;
    }
    HIP_TRY(c, hipGetLastError());
    if (int rc = cg_apply(c, kernel, in, k)) return rc;
    const double* Kx = (const double*)c->out.p;
    if (op == KMVP_EIG_CENTERED) {
      hipLaunchKernelGGL(eig_colsum_kernel, dim3(EIG_BLOCKS), dim3(256), 0, s, Kx, n, E, cpartial, st);
      hipLaunchKernelGGL(eig_mean_kernel, dim3(1), dim3(EIG_BLOCKS), 0, s, cpartial, E, n, mean, st);
      hipLaunchKernelGGL(eig_center_kernel, dim3(blocks), dim3(256), 0, s, Kx, mean, out, count, E, st);
    } else if (op == KMVP_EIG_NORMALIZED) {
      hipLaunchKernelGGL(eig_rowscale_kernel, dim3(blocks), dim3(256), 0, s, Kx, sq, out, count, E, st);
    } else {
      hipLaunchKernelGGL(eig_diag_kernel, dim3(blocks), dim3(256), 0, s, Kx, x, diag, with_diag ? 1 : 0, out, count, E, st);
    }
    HIP_TRY(c, hipGetLastError());
    return KMVP_OK;
  }

  // Lanczos step j = jj + 1: v_1 .. v_j are in V
  int step(int jj, int maxit) {
    hipStream_t s = c->stream;
    const int nv = jj + 1;
    if (int rc = apply(V + (size_t)jj * ld, 1, w)) return rc;
    for (int round = 0; round < 2; ++round) {
      double* h = round ? h2 : h1;
      hipLaunchKernelGGL(eig_proj_kernel, dim3(EIG_BLOCKS), dim3(EIG_THREADS), 0, s, V, ld, w, nv, rows_per_block, pl, partial, st);
      hipLaunchKernelGGL(eig_reduce_kernel, dim3(blocks_for(nv, EIG_THREADS / 64)), dim3(EIG_THREADS), 0, s, partial, pl, nv, h, st);
      hipLaunchKernelGGL(eig_sub_kernel, dim3(EIG_BLOCKS), dim3(EIG_THREADS), 0, s, V, ld, w, h, nv, rows_per_block,
                         round ? npartial : (double*)nullptr, st);
    }
    hipLaunchKernelGGL(eig_scalar_kernel, dim3(1), dim3(EIG_BLOCKS), 0, s, npartial, h1, h2, jj, st, hist, hist + maxit);
    hipLaunchKernelGGL(eig_normalize_kernel, dim3(blocks_for(ld)), dim3(256), 0, s, w, hist + maxit + jj,
                       V + (size_t)(jj + 1) * ld, ld, st);
    HIP_TRY(c, hipGetLastError());
    return KMVP_OK;
  }
};

}  // namespace

int eigsh_solve(kmvp_ctx* c, int kernel, int k, int op, const double* v0, double tol, int maxit, double* eigenvalues,
                double* eigenvectors, double* resid, int* steps, double* alpha_out, double* beta_out, double* degree_out) {
  if (!c) return KMVP_E_INVALID;
  if (!c->have_points) return fail(c, KMVP_E_INVALID, "kmvp_set_points has not been called");
  if (c->dtype == KMVP_BF16) return fail(c, KMVP_E_UNSUPPORTED, "the eigen-solver needs a float32 or float64 context");
  if (int rc = solver_shape(c)) return rc;
  const int64_t n = c->N;
  if (!v0 || !eigenvalues || !eigenvectors || !resid || !steps)
    return fail(c, KMVP_E_INVALID, "eigsh: v0, eigenvalues, eigenvectors, resid and steps must not be NULL");
  if (op != KMVP_EIG_KERNEL && op != KMVP_EIG_CENTERED && op != KMVP_EIG_NORMALIZED)
    return fail(c, KMVP_E_INVALID, "eigsh: unknown operator " + std::to_string(op));
  if (k < 1 || k > n) return fail(c, KMVP_E_INVALID, "eigsh: k = " + std::to_string(k) + " is not in 1 .. N = " + std::to_string(n));
  if (maxit < k || maxit > std::min<int64_t>(n, EIG_MAX_STEPS))
    return fail(c, KMVP_E_INVALID, "eigsh: maxit = " + std::to_string(maxit) + " is not in k .. min(N, " +
                                       std::to_string(EIG_MAX_STEPS) + ") (there is no restart)");
  if (!(tol > 0)) return fail(c, KMVP_E_INVALID, "eigsh: tol must be > 0");
  if (c->diag_on && op != KMVP_EIG_KERNEL)
    return fail(c, KMVP_E_INVALID, "eigsh: the solver diagonal goes with the plain kernel operator only (KMVP_EIG_KERNEL)");
  if (c->diag_on && c->diag_n && c->diag_n != n)
    return fail(c, KMVP_E_INVALID, "solver diagonal: " + std::to_string(c->diag_n) + " values for " + std::to_string(n) +
                                       " points (pass the full vector, also on a source shard)");
  const int64_t ld = round_up(n, 32);
  // v_1 = v0 / |v0|, in the centred operator of the centred v0
  std::vector<double> v1((size_t)ld, 0.0);
  double norm0 = 0.0, mean0 = 0.0;
  for (int64_t i = 0; i < n; ++i) {
    if (!std::isfinite(v0[i])) return fail(c, KMVP_E_INVALID, "eigsh: v0 is not finite");
    norm0 += v0[i] * v0[i];
    mean0 += v0[i];
  }
  mean0 = op == KMVP_EIG_CENTERED ? mean0 / (double)n : 0.0;
  double norm1 = 0.0;
  for (int64_t i = 0; i < n; ++i) {
    v1[i] = v0[i] - mean0;
    norm1 += v1[i] * v1[i];
  }
  norm0 = std::sqrt(norm0);
  norm1 = std::sqrt(norm1);
  if (!std::isfinite(norm1)) return fail(c, KMVP_E_INVALID, "eigsh: v0 is not finite");
  if (norm0 == 0.0) return fail(c, KMVP_E_INVALID, "eigsh: v0 is zero");
  if (norm1 <= 1e-13 * norm0) return fail(c, KMVP_E_INVALID, "eigsh: v0 is zero after centring (a constant vector)");
  for (int64_t i = 0; i < n; ++i) v1[i] /= norm1;

  HIP_TRY(c, hipSetDevice(c->device));
  Eig g;
  g.c = c;
  g.kernel = kernel;
  g.op = op;
  g.n = n;
  g.ld = ld;
  g.rows_per_block = round_up((ld + EIG_BLOCKS - 1) / EIG_BLOCKS, 2);
  g.pl = maxit + 1;
  g.with_diag = c->diag_on;
  g.diag = solver_diag(c);
  const size_t nk = (size_t)n * k;
  size_t words = 0;
  auto take = [&](size_t count) {
    const size_t at = words;
    words += (count + 31) / 32 * 32;
    return at;
  };
  const size_t oV = take((size_t)(maxit + 1) * ld), ow = take(ld), ot = take(nk), oX = take(nk), oR = take(nk), osq = take(n),
               odeg = take(n), opart = take((size_t)EIG_BLOCKS * g.pl), oh1 = take(g.pl), oh2 = take(g.pl),
               onp = take(EIG_BLOCKS), ocp = take((size_t)EIG_BLOCKS * k), omean = take(k), ost = take(ST_WORDS),
               ohist = take(2 * (size_t)maxit), oS = take((size_t)maxit * k), oth = take(k), ores = take(k);
  if (int rc = ensure(c, c->scratch, sizeof(double) * words)) return rc;  // KMVP_E_NOMEM: the basis does not fit
  double* base = (double*)c->scratch.p;
  g.V = base + oV, g.w = base + ow, g.t = base + ot, g.X = base + oX, g.R = base + oR, g.sq = base + osq, g.deg = base + odeg;
  g.partial = base + opart, g.h1 = base + oh1, g.h2 = base + oh2, g.npartial = base + onp, g.cpartial = base + ocp;
  g.mean = base + omean, g.st = base + ost, g.hist = base + ohist, g.S = base + oS, g.theta = base + oth, g.resid = base + ores;

  SolveGuard guard{c};
  hipStream_t s = c->stream;
  HIP_TRY(c, hipEventRecord(c->ev[0], s));
  c->async_product = true;  // every product of the call stays on the stream
  HIP_TRY(c, hipMemsetAsync(g.w, 0, sizeof(double) * ld, s));
  HIP_TRY(c, hipMemsetAsync(g.st, 0, sizeof(double) * ST_WORDS, s));
  HIP_TRY(c, hipMemsetAsync(g.hist, 0, sizeof(double) * 2 * maxit, s));
  HIP_TRY(c, hipMemcpyAsync(g.V, v1.data(), sizeof(double) * ld, hipMemcpyHostToDevice, s));
  if (op == KMVP_EIG_NORMALIZED) {  // q = K 1 with one density product
    c->density = true;
    c->E = 1;
    c->have_signal = true;
    ++c->signal_ver;
    if (int rc = run_product(c, kernel, false)) return rc;
    HIP_TRY(c, hipMemcpyAsync(g.deg, c->out.p, sizeof(double) * n, hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(eig_rsqrt_kernel, dim3(blocks_for(n)), dim3(256), 0, s, g.deg, g.sq, n);
    HIP_TRY(c, hipGetLastError());
    if (degree_out) HIP_TRY(c, hipMemcpyAsync(degree_out, g.deg, sizeof(double) * n, hipMemcpyDeviceToHost, s));
  }

  // ---- the process: bursts of steps up to the next look (every j >= k with j mod 8 == 0, and j == maxit)
  const double nan = std::numeric_limits<double>::quiet_NaN();
  std::vector<double> state(ST_WORDS, 0.0), hist(2 * (size_t)maxit, 0.0), theta, last;
  int j = 0, stop = STOP_NONE;
  bool solved = true;
  while (j < maxit && stop == STOP_NONE) {
    int look = (std::max(k, j + 1) + EIG_LOOK - 1) / EIG_LOOK * EIG_LOOK;
    look = std::min(look, maxit);
    for (int jj = j; jj < look; ++jj)
      if (int rc = g.step(jj, maxit)) return rc;
    HIP_TRY(c, hipMemcpyAsync(state.data(), g.st, sizeof(double) * ST_WORDS, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipMemcpyAsync(hist.data(), g.hist, sizeof(double) * 2 * maxit, hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
    j = (int)state[ST_COUNT];
    stop = (int)state[ST_STOP];
    if (stop == STOP_NONFINITE || j < 1) {
      solved = false;
      break;
    }
    if (j < k) continue;  // only after a breakdown, which ends the loop
    solved = tridiag_eigen_last(hist.data(), hist.data() + maxit, j, theta, last);
    if (!solved) break;
    bool met = true;
    for (int i = 0; i < k; ++i)
      if (!(hist[maxit + j - 1] * std::fabs(last[i]) <= tol * std::fabs(theta[0]))) met = false;
    if (met) break;
  }

  // ---- X = V_j S, unit columns with the sign rule, one more application of A for the true residuals
  const int m = std::max(j, 1);
  std::vector<double> zfull, S((size_t)m * k, nan), th(k, nan);
  if (solved && j >= 1) solved = tridiag_eigen(hist.data(), hist.data() + maxit, j, theta, zfull);
  if (solved)
    for (int i = 0; i < std::min(j, k); ++i) {
      th[i] = theta[i];
      for (int r = 0; r < j; ++r) S[(size_t)r * k + i] = zfull[(size_t)r * j + i];
    }
  const double zero = 0.0;
  HIP_TRY(c, hipMemcpyAsync(g.st, &zero, sizeof(double), hipMemcpyHostToDevice, s));  // the operator's kernels run again
  HIP_TRY(c, hipMemcpyAsync(g.S, S.data(), sizeof(double) * S.size(), hipMemcpyHostToDevice, s));
  HIP_TRY(c, hipMemcpyAsync(g.theta, th.data(), sizeof(double) * k, hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(eig_ritz_kernel, dim3(blocks_for(n)), dim3(256), 0, s, g.V, ld, g.S, m, k, g.X, n);
  hipLaunchKernelGGL(eig_colfix_kernel, dim3(k), dim3(256), 0, s, g.X, n, k);
  HIP_TRY(c, hipGetLastError());
  if (int rc = g.apply(g.X, k, g.R)) return rc;
  hipLaunchKernelGGL(eig_resid_kernel, dim3(k), dim3(256), 0, s, g.R, g.X, g.theta, n, k, g.resid);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(eigenvectors, g.X, sizeof(double) * nk, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipMemcpyAsync(resid, g.resid, sizeof(double) * k, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipEventRecord(c->ev[2], s));
  HIP_TRY(c, hipStreamSynchronize(s));
  c->async_product = false;
  HIP_TRY(c, hipEventElapsedTime(&c->last_total_ms, c->ev[0], c->ev[2]));
  c->last_kernel_ms = c->last_total_ms;  // both cover the whole call (include/kmvp.h)

  for (int i = 0; i < k; ++i) eigenvalues[i] = th[i];
  *steps = j;
  if (alpha_out) memcpy(alpha_out, hist.data(), sizeof(double) * maxit);
  if (beta_out) memcpy(beta_out, hist.data() + maxit, sizeof(double) * maxit);
  bool ok = solved && j >= k;
  for (int i = 0; i < k; ++i)
    if (!(std::isfinite(resid[i]) && std::isfinite(eigenvalues[i]) && resid[i] <= 1.5 * tol)) ok = false;
  if (!ok) {
    c->err = !solved ? "eigsh: the Lanczos coefficients are not finite (non-finite operator) or their eigen-iteration failed"
             : j < k ? "eigsh: the Krylov space of v0 is invariant after fewer than k steps"
                     : "eigsh stopped before the true residuals reached the requested tolerance";
    return KMVP_E_NOT_CONVERGED;
  }
  return KMVP_OK;
}

}  // namespace kmvp
