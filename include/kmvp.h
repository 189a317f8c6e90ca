/* kmvp.h -- C ABI of libkmvp.so, the MI355X (gfx950) kernel matrix-vector product
 * backend:   a_i = sum_j k(x_i, y_j) b_j   computed on the fly (no N x M matrix).
 *
 * The reference (kernel-matrix-benchmarks) has NO native interface: its plugin
 * boundary is the Python class API of
 *     kernel_matrix_benchmarks/algorithms/base.py:51-167   (BaseProduct / BaseSolver)
 * whose only computing implementation is
 *     kernel_matrix_benchmarks/algorithms/bruteforce.py:61-207.
 * This header is therefore what a ctypes binding of that class API binds; each
 * entry point cites the reference method it stands behind.  The Python plugin
 * (kernel_matrix_benchmarks_amd/algorithms/mi355x.py) is the reference-side
 * binding; INTEGRATION.md shows the stub a maintainer adds to the reference tree.
 *
 * Conventions
 *  - extern "C", plain C types only; no C++ exception crosses the boundary.
 *  - every int-returning function returns KMVP_OK (0) or a KMVP_E_* code; the
 *    message is available from kmvp_last_error(ctx) (ctx may be NULL for errors
 *    of kmvp_create).
 *  - host buffers are caller-owned, read during the call only and never
 *    modified (the runner reuses its numpy arrays across instances,
 *    runner.py:31-34,70-93); device buffers are ctx-owned.
 *  - a ctx is bound to ONE GPU and is not thread-safe (the reference's caller
 *    is single-threaded, main.py:303-308).  Nothing touches the GPU before
 *    kmvp_create (HIP contexts do not survive the runner's fork).
 *  - all compute entry points are synchronous: the result is complete in
 *    device memory when they return (runner.py:138-140 times query() with a
 *    wall clock).
 */
#ifndef KMVP_H
#define KMVP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KMVP_ABI_VERSION 1

enum kmvp_status {
  KMVP_OK = 0,
  KMVP_E_INVALID = 1,     /* bad argument or call order                     */
  KMVP_E_UNSUPPORTED = 2, /* shape / dtype this build has no kernel for     */
  KMVP_E_DEVICE = 3,      /* HIP runtime error                              */
  KMVP_E_COMM = 4,        /* RCCL error                                     */
  KMVP_E_NOMEM = 5,
  KMVP_E_NOT_CONVERGED = 6
};

/* working precision of the arithmetic; base.py:9 `precision`, algos.yaml:157-162 */
enum kmvp_dtype {
  KMVP_F32 = 0, /* host arrays float32, fp32 VALU kernels (fp64 cross-chunk sums)   */
  KMVP_F64 = 1, /* host arrays float64, fp64 VALU kernels                           */
  KMVP_BF16 = 2 /* host arrays float32, bf16 MFMA tiles with fp32 accumulation
                   (high-D path, D >= 16 only)                                      */
};

typedef struct kmvp_ctx kmvp_ctx;

int kmvp_abi_version(void);
/* number of visible GPUs, or a negative kmvp_status; does not create a context */
int kmvp_device_count(void);

/* BaseAlgorithm.__init__ (base.py:8-29) -- binds the ctx to GPU `device`. */
kmvp_ctx* kmvp_create(int device, int* status);
/* BaseAlgorithm.done (base.py:31-33) -- frees every device buffer and the communicator. */
void kmvp_destroy(kmvp_ctx* ctx);
const char* kmvp_last_error(const kmvp_ctx* ctx);

/* BaseProduct.prepare_data (base.py:56-80, bruteforce.py:89-111) and
 * BaseSolver.prepare_data (base.py:124-133).
 *   y: (M,D) row-major source points of THIS shard, x: (N,D) target points or
 *   NULL for same_points (then N must equal M_total and, when sharded, x is the
 *   FULL cloud passed explicitly -- see below).
 *   dtype: element type of the host arrays / working precision (kmvp_dtype).
 *   j_offset, M_total: global index of y[0] and global number of sources; pass
 *   0 and M when the sources are not sharded.  They only matter for the
 *   inverse-distance kernel, whose zero pattern is defined on the GLOBAL flat
 *   index (bruteforce.py:13-14).
 * Uploads and re-lays-out the points (untimed in the harness). */
int kmvp_set_points(kmvp_ctx* ctx, const void* y, int64_t M, const void* x_or_null, int64_t N,
                    int D, int dtype, int64_t j_offset, int64_t M_total);

/* BaseAlgorithm.fit (base.py:84, bruteforce.py:113-120: the reference builds its kernel matrix
 * there, timed as build_time).  Nothing of the matrix is ever built here; what CAN be built from the
 * points alone is: for the Gaussian on clouds that qualify for the cell form (fast_sqdists 3 / auto),
 * the grid, the cell order (radix sort) and the tile lists.  kernel: 0 gaussian, 1 absexp, 2 invdist, 3 matern32,
 * 4 matern52, 7 wendland_c2, 8 wendland_c4 (3, 4, 7, 8: accepted, nothing is built for them; 5 and 6 are not codes).
 * Optional: the first query does the same work when fit was not called. */
int kmvp_fit(kmvp_ctx* ctx, int kernel);

/* BaseProduct.prepare_query (base.py:86-98, bruteforce.py:122-128).
 *   b: (M,E) row-major signal of this shard in the dtype given to
 *   kmvp_set_points, or NULL for density estimation (b == 1, E must be 1). */
int kmvp_set_signal(kmvp_ctx* ctx, const void* b_or_null, int E);

/* BaseProduct.query (base.py:100-106, bruteforce.py:130-153): one entry point per
 * kernel x normalisation -- there is no kernel-selection branch in device code.
 *   kmvp_<kernel>       a = K b            (bruteforce.py:150,153)
 *   kmvp_<kernel>_norm  a = (K b) / (K 1)  (bruteforce.py:134-145)
 * kernels (bruteforce.py:18-22): gaussian exp(-s); absexp exp(-sqrt(s));
 * invdist 1/sqrt(s) with the flat-index diagonal zeroed (bruteforce.py:8-15).
 * With a communicator attached (kmvp_comm_init) the (N,E[+1]) partial sums of
 * all ranks are all-reduced over RCCL before the normalisation. */
int kmvp_gaussian(kmvp_ctx* ctx);
int kmvp_gaussian_norm(kmvp_ctx* ctx);
int kmvp_absexp(kmvp_ctx* ctx);
int kmvp_absexp_norm(kmvp_ctx* ctx);
int kmvp_invdist(kmvp_ctx* ctx);
int kmvp_invdist_norm(kmvp_ctx* ctx);
/* k(x, y) = exp(<x, y>): the attention kernel the reference's README defines (README.md:51-59; no reference plugin
 * computes it: parity unpinned).  float32 at D <= 64 or bfloat16 at D <= 141, E <= 128; a signal must be set (density
 * estimation: pass ones).  S = X Y^T comes straight from the matrix cores (float32: 3-way split bf16 operands, fp32
 * accuracy, kmvp_fastmm.hpp; bfloat16: plain bf16 operands and a bf16 second product, kmvp_mfma.hpp), the kernel values are
 * taken relative to a per-target running exponent (flash-attention recurrence with integer exponents) and leave the pair
 * loop as (mantissa sums, exponent) pairs, so that
 *   kmvp_expdot_norm  softmax attention  a_i = sum_j e^<x_i,y_j> b_j / sum_j e^<x_i,y_j>   never forms e^max<x,y>;
 *   kmvp_expdot       plain product: overflows to inf exactly where exp(<x, y>) leaves the float64 range.
 * Range: the exponent is an integer clamped at +-32000 binades, so a row's largest logit must stay below
 * 32000 ln 2 ~ 2.2e4 (row-normalised: above -2.2e4 as well); a product with such a row fails with KMVP_E_UNSUPPORTED
 * instead of returning inf / NaN rows.
 * Sharded: all-reduce(min) of the exponents, then the usual all-reduce(sum).  Other dtypes / D: KMVP_E_UNSUPPORTED
 * (the plugin then uses the Gaussian identity, with its range check). */
int kmvp_expdot(kmvp_ctx* ctx);
int kmvp_expdot_norm(kmvp_ctx* ctx);
/* Matern covariances nu = 3/2 and nu = 5/2 (an extension: the reference has exp(-r), which is nu = 1/2, and no other
 * member of the family).  With s = |x - y|^2, r = sqrt(s):
 *   kmvp_matern32  t = sqrt(3) r,  k = (1 + t) e^-t
 *   kmvp_matern52  t = sqrt(5) r,  k = (1 + t + t^2 / 3) e^-t
 * at length scale 1 -- sklearn.gaussian_process.kernels.Matern(length_scale=1, nu=1.5 / 2.5); a length scale l is the
 * caller's scaling of the points by 1 / l, as for the Gaussian.  Both matrices are symmetric positive definite.
 * A pair at infinite distance (a float32 squared distance that overflowed included) contributes exactly 0, never
 * inf * 0.
 * float32 and float64 contexts, any D and E, _norm and density estimation as for the other kernels, always in the
 * difference form (lowd_kernel up to D = 8, lowd_mid_kernel up to D = 128, lowd_big_kernel beyond; more than four
 * signal columns at D <= 8 in blocks of four); sharded like the others (no index-based rule: j_offset / M_total do not
 * enter the values).  KMVP_E_UNSUPPORTED for bfloat16 contexts and when "fast_sqdists" asks for a matrix-core form
 * (1 .. 4) explicitly: none is built for them; the default -1 and 0 take the difference form, and
 * kmvp_last_dispatch_note is "" (but for the pair it names when "targets_per_lane" or "feed" is set). */
int kmvp_matern32(kmvp_ctx* ctx);
int kmvp_matern32_norm(kmvp_ctx* ctx);
int kmvp_matern52(kmvp_ctx* ctx);
int kmvp_matern52_norm(kmvp_ctx* ctx);

/* Gradient of the product with respect to the target points (an extension: no reference method stands behind it --
 * the force field of an N-body sum, the gradient of a kernel density estimate, the derivative of a Kriging / GP mean).
 * For targets x (N,D), sources y (M,D) and signal b (M,E):
 *     G[i, e, :] = sum_j w(s_ij) (x_i - y_j) b[j, e],     s = |x_i - y_j|^2, r = sqrt(s), k the kernel value
 *   kmvp_gaussian_grad  w = -2 k
 *   kmvp_absexp_grad    w = -k / r.  A pair with s == 0 contributes exactly 0: exp(-r) is not differentiable there, 0 is
 *                       the symmetric subgradient, and the own pair of same_points vanishes as it must.  (float32: s below
 *                       the smallest normal number, r < 1.1e-19, counts as 0.)
 *   kmvp_invdist_grad   w = -1 / r^3.  The pairs zeroed by the flat-index rule (bruteforce.py:13-14; j_offset / M_total as
 *                       in the product) contribute 0.  A coincident pair that is NOT zeroed gives inf * 0: that row of G is
 *                       NaN in every component -- exactly the rows where kmvp_invdist is inf.
 *   kmvp_matern32_grad  w = -3 e^-t,  t = sqrt(3) r
 *   kmvp_matern52_grad  w = -(5/3) (1 + t) e^-t,  t = sqrt(5) r.  Both weights are finite and smooth at r = 0: a
 *                       coincident pair (the own pair of same_points) contributes w * 0 = 0 by itself; a pair at
 *                       infinite distance contributes exactly 0.
 * The targets are independent variables, also with same_points: this is the derivative in the first argument (a
 * caller who wants the total derivative of a symmetric sum adds the transpose term).  Density estimation (b == NULL)
 * means b = 1, E = 1.  Row normalisation is not differentiated.
 * Non-finite inputs, the same rules for kmvp_<kernel>_dscale below:
 *  - a NaN target coordinate makes that row NaN in every component, and touches no other row;
 *  - a pair whose squared distance overflows the working precision although x - y is finite contributes exactly 0;
 *  - a SOURCE coordinate that is NaN or +-inf is not screened (it would cost every pair a select): the components of
 *    that axis, G[:, :, d], are non-finite in EVERY row, wherever in the array the source sits.  The other components
 *    either hold the sum over the other sources or are non-finite too (float32 Gaussian, exp(-r) and 1/r on a NaN).
 *    Filter such sources before kmvp_set_points; the products, by contrast, count a source at infinity as 0;
 *  - a NaN signal entry b[j, e] makes column e non-finite in every row and leaves the other columns alone.
 * Synchronous like the products; the result is read with kmvp_get_result as (N, E D) float64 row-major, d fastest.
 * float32 and float64 contexts, D <= 8, E <= 4 (lowd_grad_kernel, difference form: as accurate far from the origin as
 * near it); KMVP_E_UNSUPPORTED beyond that and for bfloat16 contexts.  Honours "segments", "chunk" and "partial_shard";
 * with a communicator attached the (N, E D) sums of all ranks are all-reduced like a product's.  Results are bitwise
 * reproducible run to run (fixed summation order, no atomics). */
int kmvp_gaussian_grad(kmvp_ctx* ctx);
int kmvp_absexp_grad(kmvp_ctx* ctx);
int kmvp_invdist_grad(kmvp_ctx* ctx);
int kmvp_matern32_grad(kmvp_ctx* ctx);
int kmvp_matern52_grad(kmvp_ctx* ctx);

/* Derivative of the product in the logarithm of a per-axis length scale (an extension: no reference method stands
 * behind it -- the ARD length-scale gradient of a Gaussian-process likelihood, of a Kriging fit, of a bandwidth
 * selection).  A length scale is the caller's scaling of the points, x / l and y / l with one l_d per axis; at l = 1,
 * with w the weight of kmvp_<kernel>_grad above,
 *     d k(x_i, y_j) / d log l_d = -w(s_ij) (x_{i,d} - y_{j,d})^2 =: h_d(x_i, y_j)        (summed over d: -s w)
 *     H[i, e, d] = sum_j h_d(x_i, y_j) b[j, e]
 *   kmvp_gaussian_dscale   h_d = 2 k D_d^2                       D_d = x_{i,d} - y_{j,d}
 *   kmvp_absexp_dscale     h_d = k D_d^2 / r.  A coincident pair contributes exactly 0: the true limit D_d^2 / r -> 0,
 *                          not a convention.  (float32: s below the smallest normal number counts as 0, as above.)
 *   kmvp_matern32_dscale   h_d = 3 e^-t D_d^2,  t = sqrt(3) r
 *   kmvp_matern52_dscale   h_d = (5/3) (1 + t) e^-t D_d^2,  t = sqrt(5) r
 * There is no inverse-distance entry: that kernel is not a covariance, and its derivative is the kernel itself.
 * A pair whose squared distance overflows the working precision contributes exactly 0 as long as x - y itself is
 * finite.  A NaN target coordinate makes that row of H NaN in every component, and no other row; a NaN or +-inf source
 * coordinate makes H[:, :, d] of its axis non-finite in every row; a NaN signal entry its column: the rules stated for
 * kmvp_<kernel>_grad above.  Density estimation (b == NULL) means b = 1, E = 1.  Row normalisation is not
 * differentiated.
 * Synchronous like the products; the result is read with kmvp_get_result as (N, E D) float64 row-major, d fastest.
 * float32 and float64 contexts, D <= 8, E <= 4 (lowd_dscale_kernel, difference form on the product's own packed
 * layouts: as accurate far from the origin as near it); KMVP_E_UNSUPPORTED beyond that and for bfloat16 contexts.
 * Honours "segments", "chunk" and "partial_shard"; linear in the sources, so with a communicator attached the (N, E D)
 * sums of all ranks are all-reduced like a product's.  Results are bitwise reproducible run to run (fixed summation
 * order, no atomics). */
int kmvp_gaussian_dscale(kmvp_ctx* ctx);
int kmvp_absexp_dscale(kmvp_ctx* ctx);
int kmvp_matern32_dscale(kmvp_ctx* ctx);
int kmvp_matern52_dscale(kmvp_ctx* ctx);

/* Log-sum-exp reduction of the Gaussian and exp(-r) kernels (an extension: no reference method stands behind it -- the
 * half-iteration of entropic optimal transport (Sinkhorn), log-densities far from the data, the log-partition of a
 * kernel-attention row).  For targets x (N,D), sources y (M,D) and log-weights c (M,E):
 *     L[i, e] = log sum_j exp( l(x_i, y_j) + c[j, e] )            (natural logarithm)
 *   kmvp_gaussian_logsumexp  l = -|x - y|^2
 *   kmvp_absexp_logsumexp    l = -|x - y|
 * The signal given to kmvp_set_signal is READ AS c; density estimation (b == NULL) means c = 0, E = 1.  A temperature
 * eps -- L = log sum_j exp((g_j - C(x_i, y_j)) / eps) -- is the caller's scaling of the points (by 1 / sqrt(eps) for
 * C = |x - y|^2, by 1 / eps for C = |x - y|) and of c (= g / eps + log weight), as the length scale is for every other
 * kernel.  Every column has its own shift: columns are independent.  Row normalisation does not exist for this reduction,
 * and the other kernels have no such entry point.
 * Conventions
 *  - c[j, e] = -inf: source j has weight 0 in column e.
 *  - a row / column without a live term -- M == 0, every c = -inf, or (float32) every squared distance overflowed to
 *    inf -- is exactly -inf, never NaN.  Pad records and pairs at infinite distance contribute exactly 0.
 *  - a NaN target coordinate makes that row NaN in every column, and no other row.
 *  - c = +inf or NaN: the result of that column is unspecified but not finite.
 *  - the result never depends on exp(largest logit) being representable: the pair loop keeps a per-target, per-column
 *    integer shift in log2 units and sums 2^(u - shift) <= 1 (csrc/kmvp_lowd_lse.hpp); the shift is unbounded (no
 *    +-32000-binade range as for exp(<x, y>)).  Logits below -3e38 (float32) / -1e299 (float64) in log2 units count as -inf.
 *  - bitwise reproducible run to run: fixed summation order, no atomics, every rescale an exact power of two.
 * Synchronous like the products; the result is read with kmvp_get_result as (N, E) float64 row-major.
 * float32 and float64 contexts, D <= 8, E <= 4 (lowd_lse_kernel, difference form, on the product's own packed layouts);
 * KMVP_E_UNSUPPORTED beyond that, for bfloat16 contexts and when "fast_sqdists" asks for a matrix-core form (1 .. 4)
 * explicitly; kmvp_last_dispatch_note is "".  Honours "segments", "chunk" and "partial_shard" (the shard's own L is
 * returned: the caller merges shards with logaddexp).  With a communicator attached the ranks merge their
 * (sum, exponent) pairs: all-reduce(min) of the (N, E) exponents, then all-reduce(sum) -- also on a rank whose source
 * slice is empty. */
int kmvp_gaussian_logsumexp(kmvp_ctx* ctx);
int kmvp_absexp_logsumexp(kmvp_ctx* ctx);

/* Gradient of the log-sum-exp with respect to the target points (an extension, the companion of kmvp_<kernel>_logsumexp:
 * the barycentric map and the displacement field of entropic optimal transport, the gradient of a Sinkhorn loss with
 * respect to the points, the score grad log p of a kernel density, a mean-shift step).  A softmax-weighted sum:
 *     G[i, e, :] = grad_{x_i} L[i, e] = sum_j p_ij^e g(x_i, y_j)
 *     p_ij^e     = exp( l(x_i, y_j) + c[j, e] ) / sum_j' exp( l(x_i, y_j') + c[j', e] )
 *   kmvp_gaussian_logsumexp_grad  l = -|x - y|^2   g = -2 (x - y)          so G = -2 (x_i - ybar_i^e), ybar the
 *                                                                          softmax-weighted barycentre of the sources
 *   kmvp_absexp_logsumexp_grad    l = -|x - y|     g = -(x - y) / r,  r = |x - y|
 * The signal is READ AS log-weights c exactly as for kmvp_<kernel>_logsumexp (b == NULL: c = 0, E = 1); the targets are
 * independent variables, also with same_points (as for kmvp_<kernel>_grad).  Synchronous; the result is read with
 * kmvp_get_result as (N, E * D) float64 row-major, d fastest.  The other kernels have no such entry point, and row
 * normalisation does not exist for this reduction.
 * Conventions
 *  - exp(-r), a coincident pair (s = |x - y|^2 == 0; float32: s not a positive normal number, as for kmvp_absexp_grad):
 *    the pair contributes 0 to the numerator and keeps its weight in the denominator -- the symmetric subgradient; the
 *    own pair of same_points drops out of the numerator as it must.
 *  - c[j, e] = -inf, pad records and pairs whose squared distance overflowed contribute exactly 0 to both sums -- as
 *    long as the difference x - y itself is finite: a coordinate difference that overflows (float32: |x_d - y_d| > 3.4e38)
 *    or an infinite coordinate gives 0 * inf, and that row is NaN although other pairs are live.
 *  - a (row, column) without a live term -- M == 0, every c = -inf, or (float32) every squared distance overflowed -- is
 *    NaN in all D components: exactly the entries where kmvp_<kernel>_logsumexp is -inf.  Never finite, never inf.
 *  - a NaN target coordinate makes that row NaN in every column, and touches no other row.
 *  - c = +inf or NaN in one entry: no entry of that column is finite, for any target; the
 *    other columns are untouched.
 *  - the result never depends on exp(largest logit) being representable: numerator and denominator share the
 *    log-sum-exp's per-target, per-column integer shift (csrc/kmvp_lowd_lse_grad.hpp), which is unbounded.
 *  - bitwise reproducible run to run: fixed summation order, no atomics, every rescale an exact power of two.
 * float32 and float64 contexts, D <= 8, E <= 4 (lowd_lse_grad_kernel, difference form, on the product's own packed
 * layouts: one pack serves product, gradient, log-sum-exp and this); KMVP_E_UNSUPPORTED with a message beyond that, for
 * bfloat16 contexts and when "fast_sqdists" asks for a matrix-core form (1 .. 4) explicitly; kmvp_last_dispatch_note is
 * "".  Honours "segments", "chunk" and "partial_shard": a partial shard returns its OWN G_s, and the caller merges shards
 * as G = sum_s exp(L_s - L) G_s with the shards' L_s from kmvp_<kernel>_logsumexp and L their logaddexp (a shard whose
 * L_s is -inf has weight 0 and a NaN G_s: leave it out).  With a communicator attached the ranks merge (D + 1 sums,
 * exponent) tuples: all-reduce(min) of the (N, E) exponents, then ONE all-reduce(sum) of the (D + 1) E N sums -- also on
 * a rank whose source slice is empty. */
int kmvp_gaussian_logsumexp_grad(kmvp_ctx* ctx);
int kmvp_absexp_logsumexp_grad(kmvp_ctx* ctx);

/* Brute-force K nearest neighbours (an extension: no reference method stands behind it -- the third reduction over the
 * sources next to the sum and the log-sum-exp, KeOps' argKmin, and the eps -> 0 limit of the log-sum-exp's soft-min: the
 * assignment step of k-means and mean-shift, Chamfer and Hausdorff distances, the k-NN distance of an adaptive bandwidth or
 * a median heuristic, neighbour sets of Vecchia / nearest-neighbour Gaussian processes, a k-NN graph).  For every target
 * x_i the K sources with the smallest squared distance s = |x_i - y_j|^2, never forming the N x M matrix:
 *     out_idx[i, k]    GLOBAL index of the k-th nearest source (j_offset + position in y), int64
 *     out_sqdist[i, k] its squared distance, float64
 * both caller-owned, (N, K) row-major, written during the call (synchronous).  Neighbours come nearest first; equal
 * distances come in ascending index.  exclude_self != 0 leaves source j == i out of row i (same_points: a k-NN graph
 * without loops).  It is exact and costs the pair loop nothing: K + 1 candidates are collected, and the one with j == i
 * is dropped if it is there, the last one otherwise -- right also when more than K + 1 sources coincide with the target
 * (the K + 1 candidates are then all at distance 0 with indices below i).  Hence K <= 16, and K <= 15 with exclude_self.
 * Conventions
 *  - s is the family's difference form in the working precision (one subtraction, one square, D - 1 fmas), and
 *    out_sqdist is that very value -- the one the kernel compared -- widened to float64.
 *  - fewer than K qualifying sources (M == 0 included): the trailing entries are idx = -1, sqdist = +inf.  N == 0
 *    writes nothing and returns KMVP_OK.
 *  - a source with a NaN coordinate and a pair whose squared distance is not finite in the working precision (float32:
 *    it overflowed) never qualify: the family's rule that a pair at infinite distance contributes nothing.
 *  - a NaN target coordinate gives that row idx = -1, sqdist = NaN in all K entries, and touches no other row.
 *  - bitwise reproducible run to run, and independent of "segments".
 *  - kmvp_set_signal is neither needed nor consulted, and kmvp_get_result is not involved.  A product, gradient or
 *    log-sum-exp on the same context before and after the call returns the same bits as without it (the call goes through
 *    the context's pack bookkeeping with the density layout of the difference form).
 * float32 and float64 contexts, D <= 8 (lowd_knn_kernel: per-lane sorted lists of capacity 1, 4 or 16 in registers, the
 * smallest that holds K [+ 1]; csrc/kmvp_lowd_knn.hpp, merge: csrc/kmvp_knn_merge.hpp).  KMVP_E_UNSUPPORTED with a message
 * for bfloat16 contexts, D > 8, K > 16 (15 with exclude_self) and an explicit "fast_sqdists" of 1 .. 4.  KMVP_E_INVALID for
 * K < 1, a NULL output with N > 0, no points set, and exclude_self when the targets are not the sources (with a source
 * shard it is allowed when "same_points_global" is set and x is the full cloud).
 * kmvp_last_kernel_name is "lowd_knn_kernel", kmvp_last_dispatch_note is "", kmvp_last_kernel_ms / kmvp_last_total_ms as
 * for a product.  Honours "segments" (every segment starts from an empty list, which the lists of capacity 16 pay for:
 * the automatic choice gives them only the segments two workgroups per CU ask for, none shorter than 4096 sources; the
 * shorter lists take the product's rule), "chunk" (no meaning here: accepted, ignored) and
 * "partial_shard": a slice returns its own K with global indices, and the caller merges shards by (sqdist, idx).
 * With a communicator attached every rank places its [2 K'][N] candidates (K' = K, + 1 with exclude_self) into slot
 * `rank` of a zero-filled [world][2 K'][N] buffer; ONE all-reduce(sum) -- adding zeros is exact -- hands every rank all
 * lists, which it merges like segments: every rank returns the same bits, also a rank whose source slice is empty.  That
 * buffer is world * 2 K' * N doubles on every rank. */
int kmvp_nearest(kmvp_ctx* ctx, int K, int exclude_self, int64_t* out_idx, double* out_sqdist);

/* Batched clouds (an extension: KeOps' `ranges`, PyTorch3D's `lengths`): B clouds concatenated in the arrays of
 * kmvp_set_points, every reduction restricted to a target's own batch -- Chamfer distances and k-NN graphs on point-cloud
 * batches, per-sample kernel densities, per-group kernel regressions, in ONE launch instead of one upload, pack and launch
 * per cloud.  Called after kmvp_set_points:
 *     y_offsets, x_offsets   B + 1 int64 values each, non-decreasing, from 0 to M (respectively N): batch b owns sources
 *                            [y_offsets[b], y_offsets[b + 1]) and targets [x_offsets[b], x_offsets[b + 1]).  Empty batches
 *                            on either side are allowed.  Read during the call.
 *     x_offsets_or_null      NULL only when the targets are the sources (x_or_null == NULL at kmvp_set_points): it then
 *                            means x_offsets = y_offsets.
 *     B == 0 with NULL pointers switches batching off; kmvp_set_points switches it off too, as it clears the solver
 *     diagonal.  A refused call leaves the previous setting.
 * KMVP_E_INVALID for: no points set, B < 0, a NULL y_offsets with B > 0 (non-NULL offsets with B == 0), a NULL x_offsets
 * when the targets are not the sources, and offsets that are not monotone or do not start at 0 and end at M (respectively
 * N).  KMVP_E_UNSUPPORTED for a batch of more than 2^31 - 8 sources.
 * While batches are set
 *  - kmvp_gaussian[_norm], kmvp_absexp[_norm], kmvp_matern32[_norm], kmvp_matern52[_norm] compute the block-diagonal
 *    reduction a[i, e] = sum_{j in batch(i)} k(x_i, y_j) b[j, e].  The signal is set with kmvp_set_signal as usual: (M, E)
 *    over the concatenated sources, NULL for density estimation.  The normalised form divides by the batch's own
 *    sum_j k.  kmvp_get_result reads (N, E) float64 in the caller's order.  A batch without sources gives what the plain
 *    entry gives for M == 0: rows of 0, of NaN (0 / 0) when normalised; a NaN target coordinate gives a NaN row in every
 *    other batch.  Normalised density estimation is 1 (NaN in a batch without sources) and launches no pair loop.
 *  - kmvp_nearest(ctx, K, 0, idx, sqdist) returns every target's K nearest sources of its own batch: indices are positions
 *    in the concatenated y, nearest first, ties towards the smaller index; where the batch has fewer than K qualifying
 *    sources the tail is (-1, +inf); a NaN target row is (-1, NaN) -- all as documented for the plain entry (a batch
 *    without sources: (-1, +inf) throughout, the plain entry's M == 0).
 *  - every row depends on its own batch alone: it is the same bit for bit whatever the other batches hold, wherever the
 *    batch stands among them, alone (B = 1) and run to run.
 *  - everything else returns KMVP_E_UNSUPPORTED with a message that names the batches: kmvp_invdist[_norm] (its flat-index
 *    zero rule has no per-batch definition), kmvp_expdot[_norm], the gradients, the length-scale derivatives, the
 *    log-sum-exp and its gradient, the solvers, the Lanczos quadratures, kmvp_<kernel>_sinkhorn, k-means, mean-shift, and
 *    kmvp_nearest with exclude_self != 0.  Sinkhorn on batches has an entry of its own, kmvp_<kernel>_sinkhorn_batched (one
 *    transport problem per batch); the plain entry keeps refusing.  So do the products and kmvp_nearest themselves on a bfloat16 context, at D > 8, with E > 4
 *    signal columns (normalised rows included: the denominator rides along as lowd_kernel's does), with an explicit
 *    "fast_sqdists" of 1 .. 4, with a communicator attached and on a source slice (M < M_total).
 *  - kmvp_last_kernel_name is "lowd_batch_kernel" or "lowd_batch_knn_kernel" (csrc/kmvp_lowd_batch.hpp: lowd_kernel's
 *    scalar-cache feed with one source range per wavefront; plan and layout: csrc/kmvp_batch_plan.hpp),
 *    kmvp_last_dispatch_note is "", kmvp_last_kernel_ms / kmvp_last_total_ms as for a product.  "chunk" is honoured (the
 *    float32 chain between folds into float64, rounded up to 8); "segments", "feed" and "targets_per_lane" are accepted
 *    and ignored: a batch is never cut into segments, so a batch with few targets and very many sources runs on few waves.
 * With batches off every entry returns bit for bit what it returns without this call ever made: target image, records,
 * tile table and index maps of the batches live in buffers of their own on the context, and the product's pack
 * bookkeeping is not touched. */
int kmvp_set_batches(kmvp_ctx* ctx, int B, const int64_t* y_offsets, const int64_t* x_offsets_or_null);

/* Cutoff-radius products and neighbour counts on a cell list (an extension: short-range sums -- a Gaussian or Matern at a
 * length scale far below the cloud's size, SPH and molecular sums, densities with a fixed support, DBSCAN's core-point
 * counts, PyTorch3D's ball_query, KeOps' block-sparse ranges).  The caller knows a radius R beyond which a pair contributes
 * nothing; the work is O(N * neighbours), not O(N * M).  For targets x (N,D), sources y (M,D) in the working precision
 * `real`:
 *     r2   = (real)(R * R), R * R formed in double
 *     s_ij = the family's squared distance in the working precision: one subtraction, one square, D - 1 fmas (the value
 *            kmvp_nearest compares)
 *     the pair (i, j) is INSIDE iff s_ij <= r2: a pair at exactly r2 is inside, a NaN s is outside.
 *   kmvp_<kernel>_cutoff(ctx, R, normalise)   a[i, e] = sum_{j inside} k(s_ij) b[j, e] for the Gaussian, exp(-r) and the two
 *     Matern kernels, in the three signal modes of the plain product: the product, normalised rows (normalise != 0: divided
 *     by sum_{j inside} k) and density estimation (kmvp_set_signal(NULL)).  Read with kmvp_get_result as (N, E) float64.
 *     A target with no source inside gets 0, and NaN = 0 / 0 when normalised: the plain entry's M = 0 answer.  Normalised
 *     density estimation is v / v -- 1 where a source is inside and the sum did not flush to 0, NaN otherwise -- and runs
 *     the pair loop.
 *   kmvp_radius_count(ctx, R, exclude_self, counts)   counts[i] (N int64, caller-owned) = the number of sources inside.
 *     Needs kmvp_set_points only.  exclude_self != 0 is for targets == sources (x_or_null == NULL) only: a target whose
 *     coordinates are all finite counts itself once and has 1 subtracted; duplicates of it still count.
 *   kmvp_cutoff_info(ctx, out[8])   the plan the last of these calls ran on: [0], [1], [2] cells per axis (1 for unused
 *     axes); [3] wave tiles of 64 target slots that own a target; [4] source runs of all tiles; [5] records walked, the sum
 *     over the tiles of live lanes x the records of its runs; [6] padded source records; [7] wall milliseconds the last
 *     plan build took on whichever side ran it ("cutoff_plan": the host's build without its copies, the device's with its
 *     two read-backs), rounded (the plan is cached: 0 builds since do not reset it).  KMVP_E_INVALID before any such call.
 *   kmvp_cutoff_plan_read(ctx, sizes[13], grid[4], tiles, runs, tmap, smap)   that plan itself, copied from the device
 *     buffers the kernels read (so it checks the host build's upload as well as the device build): sizes[0 .. 3) cells per
 *     axis, [3] n_pad target slots, [4] m_pad and [5] m_alloc source records, [6] tiles with a live lane, [7] records walked,
 *     [8] tiles and [9] runs of the tables, [10] entries of tmap (= n_pad), [11] entries of smap (= m_alloc), [12] the side
 *     that built it: 0 the host, 1 the device; grid = the origin lo[3] and the cell side h; tiles as sizes[8] rows of three
 *     int64 (first run, runs, live lanes), runs as sizes[9] rows of two (first record, records), tmap and smap the padded
 *     slot -> caller index maps, -1 for a pad (csrc/kmvp_cutoff_plan.hpp).  Every pointer may be NULL: read the sizes
 *     first, then the arrays, as with kmvp_cell_layout.  KMVP_E_INVALID before any cutoff call has built a plan.
 * Non-finite coordinates
 *  - a source with a NaN or infinite coordinate is never inside;
 *  - a target with an infinite coordinate has nothing inside: a row of 0 (NaN when normalised), count 0;
 *  - a target with a NaN coordinate gets a NaN row (the family's rule) and count -1.  Neither disturbs any other row.
 * Signals must be finite.  An outside pair that the walk meets is removed by setting k to 0 -- one select per pair -- and
 * 0 * b is added: a non-finite b[j, e] therefore reaches column e of every row whose walk meets source j (its cell or a
 * neighbouring one), inside the radius or not.
 * How: both clouds are counting-sorted -- on the host, or with "cutoff_plan" = 1 by a radix sort on the device, which gives
 * the same plan entry for entry and hence the same bits from every entry here -- into cells of side h = "cutoff_cell_factor" * R * (1 + 2^-16) -- larger
 * where that would give more than 2^20 cells along an axis or more than 2 (N + M) cells -- and every wave tile of up to 64
 * targets of one row of cells walks the records of the 3^(D-1) neighbouring rows between its first cell - 1 and its last
 * cell + 1 (csrc/kmvp_cutoff_plan.hpp; kernels lowd_cutoff_kernel / lowd_cutoff_count_kernel, csrc/kmvp_lowd_cutoff.hpp:
 * lowd_batch_kernel's scalar-cache feed with several source ranges per wavefront).  The plan is cached on (points, R,
 * factor, "cutoff_plan"); target image, records, tables and maps live in buffers of the feature's own, so every other entry returns the
 * same bits before and after these calls.  float32 sums fold into float64 every "chunk" walked records and at the end of
 * every range; float64 keeps one chain.
 *  - bitwise reproducible run to run for the same points, radius and options.  The products depend on the grid (hence on
 *    "cutoff_cell_factor") in their float32 rounding: it decides where the chain is folded.  The counts do not.
 *  - kmvp_last_kernel_name is "lowd_cutoff_kernel" / "lowd_cutoff_count_kernel"; kmvp_last_kernel_ms is the pair loop,
 *    kmvp_last_total_ms includes the plan build's uploads and the packs.
 * KMVP_E_INVALID: a radius that is not finite or not > 0, no points set, no signal set (the products), a NULL counts with
 * N > 0, exclude_self when the targets are not the sources.  KMVP_E_UNSUPPORTED with a message that names the cutoff and
 * the cause: D > 3, E > 4 signal columns, a bfloat16 context, an attached communicator, a source slice (M < M_total), and
 * while batches are set (kmvp_set_batches).  float16 data: a float32 context of float16-rounded points, as everywhere.
 * Not built: log-sum-exp with a cutoff, the length-scale derivative with a cutoff (the gradient with respect to the
 * targets is kmvp_<kernel>_cutoff_grad below, the K nearest inside the radius kmvp_radius_nearest), solvers with a cutoff for the four truncated kernels (a
 * truncated Gaussian or Matern matrix is in general not positive definite), D > 3, source shards, batches combined with a
 * cutoff, caller-supplied block-sparse ranges. */
int kmvp_gaussian_cutoff(kmvp_ctx* ctx, double radius, int normalise);
int kmvp_absexp_cutoff(kmvp_ctx* ctx, double radius, int normalise);
int kmvp_matern32_cutoff(kmvp_ctx* ctx, double radius, int normalise);
int kmvp_matern52_cutoff(kmvp_ctx* ctx, double radius, int normalise);
int kmvp_radius_count(kmvp_ctx* ctx, double radius, int exclude_self, int64_t* counts);
int kmvp_cutoff_info(kmvp_ctx* ctx, int64_t out[8]);
int kmvp_cutoff_plan_read(kmvp_ctx* ctx, int64_t sizes[13], double grid[4], int64_t* tiles, int64_t* runs, int64_t* tmap, int64_t* smap);

/* K nearest sources within a radius on the cell list (an extension: PyTorch3D's ball_query with indices, fixed-radius
 * nearest neighbours, SPH and molecular-dynamics neighbour lists, DBSCAN's region query, Vecchia neighbour sets and a k-NN
 * graph on a cloud too large for the brute-force kmvp_nearest).  For every target the K sources with the smallest s_ij
 * among those INSIDE the radius -- kmvp_radius_count's rule exactly: r2 = (real)(R * R) with R * R formed in double, s_ij
 * the family's difference-form squared distance in the working precision, a pair at exactly r2 inside, a NaN s outside.
 * Outputs and conventions are kmvp_nearest's: out_idx / out_sqdist (N, K) row-major, caller-owned, written during the call;
 * nearest first, equal distances in ascending caller's source index; out_sqdist is the very value that was compared,
 * widened to float64; a row with fewer than K sources inside ends in (-1, +inf); N == 0 writes nothing and returns KMVP_OK.
 * exclude_self != 0 (targets == sources only) is kmvp_nearest's rule: K + 1 candidates are collected, the one with j == i
 * is dropped if it is there, else the last.  Hence K <= 16, and K <= 15 with exclude_self.
 * THE CONTRACT: row i equals, bit for bit, row i of kmvp_nearest(ctx, K, exclude_self, ...) with every entry whose
 * sqdist > r2 replaced by (-1, +inf).  That holds whatever "cutoff_cell_factor" is: the result does NOT depend on the grid
 * (unlike the float32 products), and it is bitwise reproducible.
 * Non-finite coordinates
 *  - a target with a NaN coordinate gets (-1, NaN) in all K entries (where there is a source at all: M == 0 gives
 *    (-1, +inf) everywhere, as kmvp_nearest does) and disturbs no other row;
 *  - a target with an infinite coordinate has nothing inside: (-1, +inf);
 *  - a source with a NaN or infinite coordinate is in no record and never appears.
 * How: lowd_cutoff_count_kernel's walk with a sorted list of 1, 4 or 16 candidates per lane in registers, the smallest
 * capacity that holds K [+ 1] (lowd_cutoff_knn_kernel, csrc/kmvp_lowd_cutoff_knn.hpp).  The walk does not meet the sources
 * in ascending index, so the list is ordered by the pair (s, caller's index) (csrc/kmvp_radius_knn_list.hpp); the indices
 * come from an int32 copy of the plan's source map, read through the scalar cache beside the records.
 *  - kmvp_set_signal is neither needed nor consulted, kmvp_get_result is not involved, kmvp_cutoff_info is valid afterwards;
 *  - the plan cache on (points, R, factor) and the density-layout pack are kmvp_radius_count's: a count and a radius search
 *    on one context plan and pack once; every other entry returns the same bits before and after the call;
 *  - kmvp_last_kernel_name is "lowd_cutoff_knn_kernel", kmvp_last_dispatch_note is "", kmvp_last_kernel_ms is the pair
 *    loop, kmvp_last_total_ms includes the plan build's uploads and the packs, as for the count.
 * KMVP_E_INVALID: a radius that is not finite or not > 0, K < 1, a NULL output with N > 0, no points set, exclude_self when
 * the targets are not the sources.  KMVP_E_UNSUPPORTED with a message that names the radius search and the cause: K > 16
 * (15 with exclude_self) and everything kmvp_radius_count refuses -- D > 3, a bfloat16 context, an attached communicator,
 * a source slice, batches.
 * Not built: all neighbours inside the radius without a bound K (a ragged result), D > 3, source shards, batches. */
int kmvp_radius_nearest(kmvp_ctx* ctx, double radius, int K, int exclude_self, int64_t* out_idx, double* out_sqdist);

/* DBSCAN on the cell list, resident on the device (an extension: the third clusterer beside kmvp_kmeans and
 * kmvp_gaussian_meanshift; sklearn.cluster.DBSCAN, density clustering without a cluster count).  The points are clustered
 * among themselves: the context's targets must be its sources (x == NULL at kmvp_set_points).
 * THE DEFINITION is canonical -- it does not depend on the order of the points, on the grid or on scheduling:
 *  - inside   pair (i, j) is inside iff s_ij <= r2: kmvp_radius_count's rule exactly -- s the family's difference-form
 *             squared distance in the working precision, r2 = (real)(R * R) with R * R formed in double, a pair at exactly
 *             r2 inside, a NaN s outside.  The difference form is symmetric bit for bit: the graph is undirected.
 *  - counts   counts[i] is what kmvp_radius_count(ctx, R, 0, .) returns, bit for bit: the point itself is included
 *             (sklearn's convention); a point with a NaN coordinate gets -1.
 *  - core     i is a core point iff counts[i] >= min_samples.
 *  - cluster  a connected component of the graph on the core points with the inside pairs as edges.  Its root is the
 *             smallest caller's index among its core points; clusters are numbered 0 .. C - 1 in ascending order of their
 *             roots.  That is the numbering sklearn's DBSCAN produces: core labels and the noise set agree with it exactly.
 *  - border   a point that is no core point and has a core point inside joins the cluster of its NEAREST inside core point,
 *             the minimum of the pair (s, caller's index) -- the order of kmvp_radius_nearest.  sklearn gives such a point
 *             to whichever cluster its traversal reaches first, which depends on the order of the points; this rule does not.
 *  - noise    every other point: label -1.  That covers the points with a NaN or infinite coordinate, which are inside of
 *             nothing (count -1, resp. 0) and join nothing.
 * Outputs, caller-owned, written during the call: labels (N int64); core_of_or_null (N int64: the point itself for a core
 * point, the core point it was attached to for a border point, -1 for noise); counts_or_null (N int64);
 * info = [n_clusters, n_core, n_border, n_noise, rounds, walks].  N == 0 writes zeros to info (if given) and returns KMVP_OK.
 * How (csrc/kmvp_dbscan.hip): the count's walk once; then rounds of one walk each (lowd_cutoff_label_kernel,
 * csrc/kmvp_lowd_cutoff_label.hpp: the count's pair loop with one select and one integer minimum per pair, the labels read
 * beside the records through the scalar cache) in which every core point takes the smallest label among its inside core
 * points, followed by an integer hook-and-chase step over O(N) words (csrc/kmvp_dbscan_step.hpp) that lets whole trees
 * fall at once; a round that changes nothing ends them -- labels only fall, so there is no maxit; the host reads one word
 * per round.  Then one walk attaches the border points, and a scan numbers the clusters.  `rounds` counts the rounds, the
 * last one included (0: there is no core point); `walks` the passes over the cell list: the count, the rounds, the border
 * walk (left out when there is no core point or nothing else).  O(N) integers of state never leave the device.
 *  - bitwise reproducible run to run, rounds included; independent of "cutoff_cell_factor" and of "cutoff_plan";
 *  - the plan cache on (points, R, factor, "cutoff_plan"), the target image, the density-layout records and the int32
 *    source map are kmvp_radius_count's and kmvp_radius_nearest's; the label buffers are its own: every other entry returns
 *    the same bits before and after the call.  kmvp_set_signal is neither needed nor consulted; kmvp_cutoff_info is valid
 *    afterwards;
 *  - kmvp_last_kernel_name is "lowd_cutoff_label_kernel", kmvp_last_kernel_ms is the sum of the walks, kmvp_last_total_ms
 *    the whole call.
 * KMVP_E_INVALID: a radius that is not finite or not > 0, min_samples < 1, a NULL labels or info with N > 0, no points set,
 * targets that are not the sources.  KMVP_E_UNSUPPORTED with a message that names DBSCAN and the cause: everything
 * kmvp_radius_count refuses -- a bfloat16 context, D > 3, an attached communicator, a source slice, batches.
 * KMVP_E_DEVICE should the labels not settle within N rounds (they cannot: every round but the last removes a root).
 * Not built: sample weights, targets != sources (predicting the cluster of new points), D > 3, shards, batches,
 * HDBSCAN / OPTICS, the unbounded neighbour list. */
int kmvp_dbscan(kmvp_ctx* ctx, double radius, int64_t min_samples, int64_t* labels, int64_t* core_of_or_null, int64_t* counts_or_null,
                int64_t info[6]);

/* Wendland's compactly supported kernels (an extension: the reference has none) -- the cutoff WITHOUT a truncation error,
 * and the library's first sparse operator for conjugate gradients.  With the support radius R, t = |x - y| / R and
 * u = max(1 - t, 0):
 *     wendland_c2   k = u^4 (4 t + 1)                    C^2, positive definite on R^D for D <= 3
 *     wendland_c4   k = u^6 (35 t^2 + 18 t + 3) / 3      C^4, positive definite on R^D for D <= 3
 * k(0) = 1 and k vanishes identically from t = 1 on, so the sum over the sources inside R IS the full product: there is no
 * plain (all-pairs) entry.  kmvp_fit accepts the kernel codes 7 (C2) and 8 (C4) and builds nothing.
 * Arithmetic per pair in the working precision `real` (csrc/kmvp_lowd_cutoff.hpp), after the cutoff's own s and r2:
 *     q = s * iR2, iR2 = (real)(1 / (R R)) formed in double;  t = sqrt(q), the square root exp(-r) uses in this precision;
 *     u = max(1 - t, 0);  u2 = u u;  C2: k = (u2 u2) fma(4, t, 1);  C4: k = ((u2 u2) u2) fma(t, fma(t, 35/3, 6), 1);
 *     k = s <= r2 ? k : 0.
 * k is continuous and 0 at t = 1: a pair that rounding puts on the other side of s <= r2 changes a sum by O(u^4), of the
 * order of (D 2^-24)^4 resp. (D 2^-53)^4 -- these kernels need no "inside set" in their definition.
 *   kmvp_wendland_<c>_cutoff(ctx, R, normalise)   every mode, convention, refusal and non-finite rule of
 *     kmvp_<kernel>_cutoff above (product, normalised rows, density, kmvp_cutoff_info, the plan cache on (points, R, factor));
 *     kmvp_last_kernel_name is "lowd_cutoff_kernel".
 *   kmvp_wendland_<c>_cg_solve(ctx, R, a, E, rtol, maxit, out_b, iters, resid)   (K + the solver's diagonal) b = a on the cloud
 *     given with x_or_null == NULL: kmvp_<kernel>_cg_solve's driver, stop test, residual replacement, graph replay, verdict
 *     and outputs (see there), with the cutoff product as the operator.  Before the first iteration the plan is built (or
 *     found cached) and the target image and the source coordinates are packed; every application of the operator is two
 *     launches -- the E signal slots of the records written in the working precision straight from the float64 Krylov
 *     vector, and the pair loop.  kmvp_set_solver_diagonal (ridge, per point) is honoured.  The cutoff's buffers stay its
 *     own: every other entry returns the same bits before and after.  No signal is left behind (as after every solve).
 *     KMVP_E_INVALID: a bad radius, targets that are not the sources, the solver's own argument checks.
 *     KMVP_E_UNSUPPORTED, naming the cause: E > 4, whatever kmvp_<kernel>_cutoff refuses (D > 3, bfloat16, a communicator,
 *     a source slice, batches), and a preconditioner of rank > 0 (its column kernel knows no Wendland function).
 * Not built: MINRES, the Lanczos quadrature, eigsh, the preconditioner, the length-scale derivative, source shards and
 * batches with these kernels.  Their gradient with respect to the targets is kmvp_wendland_<c>_cutoff_grad below. */
int kmvp_wendland_c2_cutoff(kmvp_ctx* ctx, double radius, int normalise);
int kmvp_wendland_c4_cutoff(kmvp_ctx* ctx, double radius, int normalise);
int kmvp_wendland_c2_cg_solve(kmvp_ctx* ctx, double radius, const void* a, int E, double rtol, int maxit, double* out_b,
                              int* iters, double* resid);
int kmvp_wendland_c4_cg_solve(kmvp_ctx* ctx, double radius, const void* a, int E, double rtol, int maxit, double* out_b,
                              int* iters, double* resid);

/* Gradient of the cutoff-radius product with respect to the target points (an extension: SPH's sum of m_j grad W, the
 * force of a short-range potential sum, the slope of a kriging mean with a tapered covariance), O(N * neighbours):
 *     G[i, e, :] = c * sum_{j : s_ij <= r2} W(s_ij) (x_i - y_j) b[j, e]
 * kmvp_<kernel>_grad's output on kmvp_<kernel>_cutoff's cell list: read with kmvp_get_result as (N, E * D) float64, column
 * e D + d, in the caller's order; in density mode (kmvp_set_signal(NULL)) b = 1 and E = 1.  r2 and the plan are the
 * cutoff's; kmvp_cutoff_info is valid afterwards.  s_ij is formed from the D differences x_i - y_j, computed once and kept:
 * one square and D - 1 fmas, the cutoff's expression bit for bit, so a row's inside set is exactly the set
 * kmvp_radius_count counts (a pair at exactly r2 is inside, a NaN s is outside).
 *   Gaussian, exp(-r), Matern 3/2 and 5/2: W and c are kmvp_<kernel>_grad's (c = -2, -1, -3, -5/3).  G is the sum of the
 *     plain gradient's terms over the inside set; it equals the derivative of the truncated sum wherever no pair sits on
 *     the boundary (the truncated sum jumps there).  exp(-r): a pair with s = 0 or a denormal s contributes 0, the own pair
 *     of targets == sources included (the plain gradient's subgradient rule).
 *   Wendland, t = sqrt(s iR2) and u = max(1 - t, 0) exactly as kmvp_wendland_<c>_cutoff forms them:
 *     wendland_c2   grad k = -(20 / R^2) u^3 (x - y)                 W = (u u) u                      c = -20 / R^2
 *     wendland_c4   grad k = -(56 / (3 R^2)) u^5 (5 t + 1) (x - y)   W = ((u2 u2) u) fma(5, t, 1)     c = -56 / (3 R^2)
 *     continuous and 0 at the boundary: the exact gradients of the exact products.
 * c is formed in double and applied once per row in float64, never per pair.
 *  - an outside pair that the walk meets adds exactly +0 to every component: W and the D differences are set to 0 on the
 *    inside condition (a pad record's difference is -inf, so W = 0 alone would give NaN);
 *  - a target with nothing inside gets a row of +0; a target with an infinite coordinate has nothing inside;
 *  - a target with a NaN coordinate gets a NaN row in every component and disturbs no other row;
 *  - a source with a NaN or infinite coordinate is in no record and touches no row.  kmvp_<kernel>_grad does NOT screen its
 *    sources: there such a source makes components of every row NaN;
 *  - signals must be finite, as for kmvp_<kernel>_cutoff: 0 * b is added for a walked outside pair;
 *  - float32 keeps E D sums per lane, folded into float64 every "chunk" walked records and at the end of every range;
 *    float64 keeps one chain.  Every row is written once by its own lane: no partial sums, no atomics; bitwise
 *    reproducible run to run for the same points, radius and options;
 *  - it reads the records and the target image that kmvp_<kernel>_cutoff packs: a product and a gradient on one context
 *    plan and pack once.  Every other entry returns the same bits before and after.
 *  - kmvp_last_kernel_name is "lowd_cutoff_grad_kernel" (csrc/kmvp_lowd_cutoff_grad.hpp); kmvp_last_kernel_ms is the pair
 *    loop.
 * KMVP_E_INVALID: a radius that is not finite or not > 0, no points set, no signal set.  KMVP_E_UNSUPPORTED with a message
 * that names the cutoff gradient and the cause: everything kmvp_<kernel>_cutoff refuses -- D > 3, E > 4 signal columns, a
 * bfloat16 context, an attached communicator, a source slice, batches.  There is no `normalise` argument (the gradient of
 * a ratio is not built) and no inverse-distance entry.
 * Not built: log-sum-exp with a cutoff, the length-scale derivative with a cutoff, D > 3, source shards,
 * batches. */
int kmvp_gaussian_cutoff_grad(kmvp_ctx* ctx, double radius);
int kmvp_absexp_cutoff_grad(kmvp_ctx* ctx, double radius);
int kmvp_matern32_cutoff_grad(kmvp_ctx* ctx, double radius);
int kmvp_matern52_cutoff_grad(kmvp_ctx* ctx, double radius);
int kmvp_wendland_c2_cutoff_grad(kmvp_ctx* ctx, double radius);
int kmvp_wendland_c4_cutoff_grad(kmvp_ctx* ctx, double radius);

/* Lloyd's k-means, resident on the device (an extension: the solver on top of the arg-K-min at K = 1, as the Krylov
 * solvers are on top of the product and Sinkhorn on top of the log-sum-exp).  Kernel-independent, like kmvp_nearest.  The
 * points are the TARGETS of the context -- x (N,D), or the cloud itself when x_or_null == NULL; the context's sources and
 * kmvp_set_signal are neither needed nor consulted.  weights_or_null: N doubles >= 0, NULL = every weight 1.
 * centroids: (C,D) float64 row-major, in: the caller's initial centroids c_0 (the library draws nothing), out: the final
 * ones.  With w the weights and x the points in the working precision, widened exactly:
 *   k = 1, 2, ...:  l_k(i)   = the nearest of c_{k-1} to x_i: exactly kmvp_nearest with K = 1 and the centroids, rounded to
 *                              the working precision, as sources (difference form; ties go to the smaller centroid index)
 *                   c_k[c]   = sum_{l_k(i) = c} w_i x_i / sum_{l_k(i) = c} w_i      (float64 sums, fixed order, no atomics)
 *                              a cluster of total weight 0 KEEPS ITS POSITION: c_k[c] = c_{k-1}[c]
 *                   inertia_k = sum_i w_i s_i, s_i the very value the kernel compared (the distance to c_{k-1}), widened
 *                   shift_k   = sum_c |c_k[c] - c_{k-1}[c]|^2
 *   the first k with shift_k <= tol (absolute) stops: KMVP_OK; k == maxit stops: KMVP_E_NOT_CONVERGED, everything written.
 * Outputs, the same in both cases: centroids = c_k, labels (N int64) = l_k, cluster_weight_or_null (C doubles) = the
 * weights of l_k's clusters, *iters = k, *inertia = inertia_k, *shift = shift_k.
 * Conventions
 *  - every returned centroid of positive weight is the weighted mean of the points that carry its label; every label is
 *    the nearest RETURNED centroid whenever *shift == 0, which is the only way tol = 0 converges -- and it is reached
 *    exactly, because equal labels give bitwise equal sums.
 *  - the stopping test is made on the device in every iteration (three state words cross to the host per iteration: it
 *    only learns whether to launch another); nothing depends on when the host looks.
 *  - chaining: maxit = 1 called k times, each call fed the previous call's centroids, gives the bits of one call with
 *    maxit = k (nothing but the float64 centroids is carried from one iteration to the next).
 *  - a point without a qualifying centroid (a NaN coordinate, or every distance overflowed) gets label -1, enters no sum
 *    and ends the solve; so does a non-finite inertia or shift: KMVP_E_NOT_CONVERGED with the outputs written.  A
 *    non-finite initial centroid and a negative or non-finite weight are KMVP_E_INVALID (host checks).
 *  - bitwise reproducible run to run, and independent of "segments" ("chunk": accepted, ignored).
 *  - a product, gradient, log-sum-exp or kmvp_nearest on the same context returns the same bits before and after the
 *    call as without it: the target image of the points (packed once per kmvp_set_points), the centroid records and the
 *    state live in buffers of the solver's own.
 * Per iteration six launches: the C centroid records rewritten from the float64 centroids, lowd_knn_kernel<D, 1>
 * (kmvp_last_kernel_name) and its segment merge, both untouched, the centroid update (csrc/kmvp_kmeans.hip: every
 * workgroup walks a contiguous run of labels in index order, every thread owning the clusters of one residue modulo 256
 * in LDS; then the workgroups' partial sums in a fixed order) and one block that forms the new centroids and the verdict
 * (csrc/kmvp_kmeans_step.hpp).  kmvp_last_dispatch_note is ""; kmvp_last_kernel_ms and kmvp_last_total_ms both cover the
 * whole solve.
 * float32 and float64 contexts (float16 data: a float32 context of float16-rounded points), D <= 8, C <= 65536.
 * KMVP_E_UNSUPPORTED with a message for bfloat16 contexts, D > 8, an explicit "fast_sqdists" of 1 .. 4, an attached
 * communicator, a source slice (M < M_total) and C > 65536.  KMVP_E_INVALID for no points set, N < 1, C < 1, tol < 0 or
 * NaN, maxit < 1 and a NULL centroids, labels, iters, inertia or shift. */
int kmvp_kmeans(kmvp_ctx* ctx, int C, const double* weights_or_null, double tol, int maxit, double* centroids,
                int64_t* labels, double* cluster_weight_or_null, int* iters, double* inertia, double* shift);

/* Gaussian mean-shift, resident on the device (an extension: the solver on top of the gradient of the log-sum-exp, as
 * Sinkhorn is on top of the log-sum-exp and k-means on top of the arg-K-min).  For the Gaussian G = -2 (x_i - ybar_i) with
 * ybar_i the softmax-weighted barycentre of the sources, so x_i + G_i / 2 IS the mean-shift update; it inherits the integer
 * shift of the log-sum-exp and is finite for a seed so far from the data that the float32 product is 0 / 0.
 * There is no exp(-r) entry: its mean-shift update is a Weiszfeld-type ratio sum p y / r over sum p / r, which the sums of
 * kmvp_absexp_logsumexp_grad (sum p (x - y) / r over sum p) do not give.
 * The sources y (M,D) and the signal come from the context as for kmvp_gaussian_logsumexp_grad; the signal is read as
 * log-weights c, ONE column (b == NULL: c = 0; -inf: mass 0).  The seeds are the context's TARGETS -- x (N,D), or the cloud
 * itself when x_or_null == NULL.  The bandwidth is the caller's scaling of the points, as everywhere in this family.
 * The positions z are float64 on the device, z_0 = the seeds; real() rounds to the working precision.  For k = 1, 2, ... and
 * every ACTIVE point i:
 *   base_i  = (double) real(z_{k-1,i})
 *   G_i     = the row kmvp_gaussian_logsumexp_grad returns for a target at real(z_{k-1,i}), bit for bit
 *   h_d     = 0.5 G_i[d],   z_{k,i}[d] = base_i[d] + h_d
 *   q_i     = sum_d h_d h_d   (d ascending from 0; every product and every sum rounded on its own, no fused multiply-add:
 *                              a numpy restatement reproduces the bits)
 *   point i FREEZES after the first sweep with q_i <= tol * tol: it keeps the z_k of that sweep, iters[i] = k, step2[i] = q_i.
 *   A point whose G has a non-finite component (a row without a live term, a NaN coordinate, an overflowed difference)
 *   freezes too: its modes row is NaN in all D components, step2[i] is NaN, iters[i] the sweep at which this happened.
 * The solve ends when no point is active, or after maxit sweeps; points still active then have iters = maxit and the q of
 * the last sweep.  Outputs (all required): modes (N,D) float64 row-major, iters (N ints), step2 (N doubles), *sweeps = the
 * sweeps run, *target_sweeps = sum_k (active points in sweep k): the solver's work in units of M pair evaluations.
 * KMVP_OK if and only if every point froze with a finite q <= tol^2; otherwise KMVP_E_NOT_CONVERGED with everything written.
 * Conventions
 *  - every target's arithmetic is its own (in lowd_lse_grad_kernel lanes are targets and the shift moves per lane): a
 *    point's trajectory depends neither on which other points are still active nor on where in the target image it sits.
 *    What does enter the bits is the geometry of the source axis -- segment count, segment length, "chunk" --, pinned at
 *    the first sweep to what kmvp_gaussian_logsumexp_grad takes for these (N, M, options) and kept while the active set
 *    shrinks.  So the solve gives the bits of a host loop that calls kmvp_gaussian_logsumexp_grad on all N moved targets
 *    every sweep.  Honours "segments" and "chunk".
 *  - the freeze is decided on the device in every sweep; four state words (stop, sweeps, active points, target_sweeps)
 *    cross to the host per sweep, and it sizes the next launch from them.  Nothing else crosses until the end.
 *  - "meanshift_compact" (kmvp_set_option) 0 keeps the frozen points in the launch; the results are the same bit for bit,
 *    and *target_sweeps does not depend on it.
 *  - bitwise reproducible run to run.  kmvp_get_result is not involved.
 *  - a product, gradient, log-sum-exp, kmvp_nearest or kmvp_kmeans on the same context returns the same bits before and
 *    after the call as without it: the moving target image, the positions, the index lists and the state live in buffers
 *    of the solver's own; the source records are the product's own, under its bookkeeping, packed only if stale.
 * Per sweep seven launches: the target image of the active points, lowd_lse_grad_kernel (kmvp_last_kernel_name) and its
 * segment merge, both untouched, the step (csrc/kmvp_meanshift.hip; the rule: csrc/kmvp_meanshift_step.hpp, on the quotient
 * V / Z of the gradient's own finish), an order-preserving stream compaction of the active index list, and the state words.
 * kmvp_last_dispatch_note is ""; kmvp_last_kernel_ms and kmvp_last_total_ms both cover the whole solve.
 * float32 and float64 contexts (float16 data: a float32 context of float16-rounded points), D <= 8.
 * KMVP_E_UNSUPPORTED with a message for bfloat16 contexts, D > 8, more than one signal column, an explicit "fast_sqdists"
 * of 1 .. 4, an attached communicator and a source slice (M < M_total).  KMVP_E_INVALID for no points or no signal set,
 * tol < 0 or NaN, maxit < 1, N < 1, M < 1 and a NULL output. */
int kmvp_gaussian_meanshift(kmvp_ctx* ctx, double tol, int maxit, double* modes, int* iters, double* step2, int* sweeps,
                            int64_t* target_sweeps);

/* BaseProduct.get_result (base.py:107-116): (N,E) float64 row-major. */
int kmvp_get_result(kmvp_ctx* ctx, double* out, int64_t out_len);

/* BaseSolver.prepare_query + query (base.py:140-156, bruteforce.py:201-207): solves
 * K b = a on the point cloud given to kmvp_set_points (x_or_null == NULL) by
 * conjugate gradients with the on-the-fly product as operator.  The reference
 * uses a dense lstsq; parity is judged on the residual.
 *   a: (M,E) in the ctx dtype.  rtol: target ||K b - a|| / ||a|| (per column).
 *   out_b (M,E) float64 receives the iterate; *iters / *resid the iteration
 *   count and the worst final TRUE relative residual (from one more product).  Returns KMVP_OK
 *   only if that residual is finite and <= 1.5 rtol (the iteration stops on the recurrence residual;
 *   where the two drift apart it is restarted from the true one); otherwise KMVP_E_NOT_CONVERGED with
 *   out_b still written -- also for a non-finite operator or right-hand side. */
int kmvp_gaussian_cg_solve(kmvp_ctx* ctx, const void* a, int E, double rtol, int maxit,
                           double* out_b, int* iters, double* resid);
int kmvp_absexp_cg_solve(kmvp_ctx* ctx, const void* a, int E, double rtol, int maxit,
                         double* out_b, int* iters, double* resid);
/* The Matern matrices are positive definite: conjugate gradients, same contract (float32 / float64 contexts). */
int kmvp_matern32_cg_solve(kmvp_ctx* ctx, const void* a, int E, double rtol, int maxit,
                           double* out_b, int* iters, double* resid);
int kmvp_matern52_cg_solve(kmvp_ctx* ctx, const void* a, int E, double rtol, int maxit,
                           double* out_b, int* iters, double* resid);
/* Same contract for the inverse-distance kernel, whose matrix (zero diagonal,
 * bruteforce.py:13-14) is symmetric but INDEFINITE: MINRES instead of CG. */
int kmvp_invdist_minres_solve(kmvp_ctx* ctx, const void* a, int E, double rtol, int maxit,
                              double* out_b, int* iters, double* resid);

/* Stochastic Lanczos quadrature (an extension: the other half of a Gaussian-process training objective,
 *     log p(a) = -1/2 a' A^-1 a - 1/2 log det A - n/2 log 2 pi,    A = K + ridge I + diag(d) as kmvp_set_solver_diagonal set it,
 * without the N x N matrix).  Conjugate gradients on A x_e = z_e for P probe columns z (N,P) in the ctx dtype, from
 * x = 0, keeping the step lengths alpha_k, beta_k of every iteration: they are the Lanczos tridiagonal of (A, z_e), and
 * with theta_i, tau_i its eigenvalues and the first components of its eigenvectors (csrc/kmvp_quadrature.hpp)
 *     logquad[e] = |z_e|^2 sum_i tau_i^2 log(theta_i)  ~  z_e' log(A) z_e        invquad[e] = z_e' x_e  ~  z_e' A^-1 z_e.
 * The estimator is the caller's: with Rademacher (+-1) columns z, (1/P) sum_e logquad[e] estimates log det A and
 * (1/P) sum_e invquad[e] estimates tr A^-1; their statistical error (sample standard deviation / sqrt(P)) is the
 * caller's too.  The library draws nothing: the same z give the same bits.  The quadrature's own error is of the order
 * of rtol^2 relative to |z_e|^2 sum tau^2 |log theta| (measured: <= 1.5 rtol^2 on the systems of
 * tests/lanczos_reference.py), far below the statistical one for any rtol <= 1e-2.
 *   Every column is on its own clock: it FREEZES after the first iteration with sqrt(rs / |z_e|^2) <= rtol on the
 *   RECURRENCE residual rs (there is no residual replacement and no final true residual: a restart would break the
 *   three-term recurrence the coefficients stand for), and takes no further update -- unlike kmvp_<kernel>_cg_solve,
 *   whose converged columns go on iterating until all have converged.  A column whose recurrence breaks down
 *   (p' A p == 0 or rs <= 0) freezes one step earlier; a zero column never starts; NaN never freezes a column.  The
 *   iteration ends once every column is frozen, or after maxit iterations.
 *   steps[e]: the iterations column e took (0 for a zero column: logquad = invquad = 0, x = 0).
 *   x (N,P) float64 or NULL: the iterates, each column as it was when it froze.
 *   alpha, beta (maxit,P) float64 or NULL: row k - 1 holds iteration k; rows >= steps[e] of column e are unspecified.
 * Returns KMVP_OK when every non-zero column froze on the tolerance with a finite logquad; otherwise
 * KMVP_E_NOT_CONVERGED with everything written (logquad is NaN where a theta_i <= 0 or a coefficient is not finite: the
 * operator was not positive definite in working precision).  KMVP_E_INVALID / KMVP_E_UNSUPPORTED as for the CG entries
 * (targets != sources, a diagonal of the wrong length, ridge + d_i < 0, P < 1, maxit < 0, rtol <= 0, a NULL z, logquad,
 * invquad or steps; a bfloat16 context is KMVP_E_UNSUPPORTED).  There is no inverse-distance entry: that matrix is
 * indefinite and log is not defined on its spectrum.
 * Device-resident like the solvers (one look of the host every 8 iterations, the burst replayed as a graph in long
 * runs, the operator sharded and the vectors replicated with a communicator: every rank returns bitwise the same
 * values); fixed summation order, no atomics: bitwise reproducible run to run.  The context is left as after a solve (no
 * signal).  kmvp_last_kernel_ms and kmvp_last_total_ms both cover the whole call. */
int kmvp_gaussian_lanczos_quadrature(kmvp_ctx* ctx, const void* z, int P, double rtol, int maxit, double* logquad,
                                     double* invquad, int* steps, double* x_or_null, double* alpha_or_null,
                                     double* beta_or_null);
int kmvp_absexp_lanczos_quadrature(kmvp_ctx* ctx, const void* z, int P, double rtol, int maxit, double* logquad,
                                   double* invquad, int* steps, double* x_or_null, double* alpha_or_null,
                                   double* beta_or_null);
int kmvp_matern32_lanczos_quadrature(kmvp_ctx* ctx, const void* z, int P, double rtol, int maxit, double* logquad,
                                     double* invquad, int* steps, double* x_or_null, double* alpha_or_null,
                                     double* beta_or_null);
int kmvp_matern52_lanczos_quadrature(kmvp_ctx* ctx, const void* z, int P, double rtol, int maxit, double* logquad,
                                     double* invquad, int* steps, double* x_or_null, double* alpha_or_null,
                                     double* beta_or_null);

/* Sinkhorn iteration of entropic optimal transport (an extension, the solver on top of kmvp_<kernel>_logsumexp as the
 * Krylov solvers are on top of the product): the iteration stays on the device, three doubles (stop word, iteration
 * count, error) cross to the host per iteration.  Targets x (N,D) and sources y (M,D) are the clouds given to kmvp_set_points (x_or_null == NULL:
 * the same cloud on both sides); kmvp_set_signal is not needed and not consulted.  Marginals a (N) and b (M) come as
 * log-weights; NULL means uniform (-log N, -log M).  The cost is |x - y|^2 (gaussian) or |x - y| (absexp); the
 * temperature eps is the caller's scaling of the points, as for kmvp_<kernel>_logsumexp, and the potentials are the
 * dimensionless u = f / eps, v = g / eps.  With l the kernel's logit:
 *     T2(u)_j = -log sum_i exp( l(x_i, y_j) + u_i + log_a_i )        T1(v)_i = -log sum_j exp( l(x_i, y_j) + v_j + log_b_j )
 *   k = 1, 2, ...:   v_k = T2(u_{k-1});   ut = T1(v_k);   err_k = sum_i a_i | exp(u_{k-1,i} - ut_i) - 1 |
 *                    err_k <= tol: stop with (u_{k-1}, v_k), *iters = k, *err = err_k;   otherwise u_k = ut
 * from u_0 = the caller's u (N doubles, read on entry: zeros, or a warm start -- an eps-scaling schedule is the caller's
 * loop over warm starts).  The plan is pi_ij = a_i b_j exp(u_i + v_j + l_ij); err_k is the L1 violation of the row marginal
 * of the plan of (u_{k-1}, v_k), whose column marginal is exact by construction.
 *   u (N, in: u_0, out), v (M, out), *iters, *err: ALWAYS the plan the reported error describes -- also when maxit is
 *   reached: KMVP_E_NOT_CONVERGED with all four written (u_{maxit-1}, v_maxit, maxit, err_maxit), as the solvers.
 * Conventions
 *  - the first k with err_k <= tol is the one returned: the stopping test and the commit u_k = ut are made on the device
 *    in every iteration, nothing depends on when the host looks.
 *  - log_a_i = -inf (log_b_j = -inf): a point of mass 0.  It contributes 0 to err and to every sum; its own potential
 *    is still returned (finite: the c-transform of the other side's potential).
 *  - a potential that becomes non-finite (a row without a live term, a NaN coordinate, a log-weight of +inf or NaN)
 *    stops the solve: KMVP_E_NOT_CONVERGED with the outputs written.
 *  - the masses of a and b are not compared here (the caller's business: the Python wrapper checks them).
 *  - potentials and log-weights are float64 on the device for every working precision; they are rounded to the
 *    context's precision only in the signal slot of the source records (potential + log-weight), which is all the pair
 *    loop reads of them.
 *  - bitwise reproducible run to run (u, v, iters, err): fixed summation order, no atomics.
 * Per iteration: lowd_lse_kernel twice (kmvp_last_kernel_name), each with its segment merge and a finish kernel that
 * forms the new potential and rewrites the signal slot of the OTHER direction's records; both packed layouts (target
 * image of x with records of y, target image of y with records of x) are built once per kmvp_set_points in buffers of
 * the solver's own, so a product, gradient or log-sum-exp on the same context before or after a solve is untouched.
 * kmvp_last_kernel_ms and kmvp_last_total_ms both cover the whole solve.  Honours "segments" and "chunk".
 * float32 and float64 contexts, D <= 8, one column of weights.  KMVP_E_UNSUPPORTED with a message for bfloat16 contexts,
 * D > 8, an explicit "fast_sqdists" of 1 .. 4, an attached communicator and a source slice (M < M_total): sharded
 * Sinkhorn is not built.  KMVP_E_INVALID for call-order errors, an empty cloud, tol < 0, maxit < 1 or a NULL output. */
int kmvp_gaussian_sinkhorn(kmvp_ctx* ctx, const double* log_a_or_null, const double* log_b_or_null, double tol, int maxit,
                           double* u, double* v, int* iters, double* err);
int kmvp_absexp_sinkhorn(kmvp_ctx* ctx, const double* log_a_or_null, const double* log_b_or_null, double tol, int maxit,
                         double* u, double* v, int* iters, double* err);

/* Batched Sinkhorn (an extension: where the device-resident solvers and the batched clouds meet): one entropic transport
 * problem per batch of kmvp_set_batches, all B of them in ONE device-resident solve -- a Sinkhorn loss on a minibatch of
 * cloud pairs.  Called after kmvp_set_points and kmvp_set_batches.  Batch b is the problem between the targets
 * [x_offsets[b], x_offsets[b + 1]) and the sources [y_offsets[b], y_offsets[b + 1]) with the cost, the temperature and the
 * dimensionless potentials of kmvp_<kernel>_sinkhorn.
 *     log_a (N), log_b (M)   log-weights, concatenated over the batches as the points are; NULL: uniform WITHIN each batch
 *                            (-log n_b, -log m_b)
 *     u (N, in: u_0, out), v (M, out)   concatenated likewise
 *     iters, err, status     B values each
 * Within every batch the iteration is exactly the one documented above (v_k = T2(u_{k-1}); ut = T1(v_k); err_k = sum over
 * the batch's targets of a_i |exp(u_{k-1,i} - ut_i) - 1|; the commit u_k = ut only while the batch runs), and every batch has
 * its own clock: it stops at the first k with err_b <= tol (status 1), on a non-finite potential or error of its own
 * (status 2), or at k == maxit (status 3).  A stopped batch takes no further update: (u, v, iters[b], err[b]) of a batch
 * ALWAYS describe one and the same plan -- (u_{k-1}, v_k) of the k at which it stopped.  A batch that is empty on both sides
 * has iters 0, err 0, status 1.  The conventions of the plain entry hold per batch (points of mass 0, what makes a
 * potential non-finite, fp64 potentials and log-weights rounded only into the signal slot of a record).
 * Returns KMVP_OK if and only if every batch has status 1; otherwise KMVP_E_NOT_CONVERGED with everything written.
 * Guarantees
 *  - bitwise reproducible run to run: fixed summation order, no atomics.  A batch's error is the sum, in ascending order,
 *    of its tiles' (64 targets') sums, each formed in a fixed tree.
 *  - a batch's (u, v, iters, err, status) are bit for bit what this entry returns for that batch alone (B = 1), the same
 *    wherever the batch stands among the others, whatever the others hold (batches that turn non-finite or run to maxit
 *    included), whenever the others stop, and with "sinkhorn_retire" 0 or 1.
 *  - bitwise equality with kmvp_<kernel>_sinkhorn on the same clouds is NOT promised: that entry folds at LDS tiles,
 *    merges segments and sums its error per block of 256.  The two agree to the accumulation bound of the log-sum-exp.
 *  - a product, batched product, kmvp_nearest, log-sum-exp or plain Sinkhorn on the same context returns the same bits
 *    before and after a batched solve: both directions' layouts (target image of x with records of y; target image of y
 *    with records of x, the batches' plan with the offsets swapped), the tile tables and the state live in buffers of the
 *    solver's own, packed once per (kmvp_set_points, kmvp_set_batches).
 * Per iteration: lowd_batch_lse_kernel twice (kmvp_last_kernel_name; csrc/kmvp_lowd_batch_lse.hpp: lowd_batch_kernel's
 * scalar-cache feed with lowd_lse_kernel's arithmetic, one source range per wavefront, every row finished by its own lane),
 * each with a finish kernel, then the per-batch verdicts, the commit and the retirement of stopped batches' tiles, all on
 * the device; two doubles (batches still running, iteration count) cross to the host per iteration.
 * kmvp_last_dispatch_note is "", kmvp_last_kernel_ms and kmvp_last_total_ms both cover the whole solve.  "chunk" is honoured;
 * "segments", "feed" and "targets_per_lane" are accepted and ignored, as for the batched product: a batch is never cut into
 * segments, so a batch with few targets and very many sources runs on few waves.
 * KMVP_E_INVALID: batches are not set (the message names kmvp_set_batches), tol < 0 or NaN, maxit < 1, a NULL u, v, iters,
 * err or status, a batch with points on one side only (the message names it).  KMVP_E_UNSUPPORTED, each with a message that
 * names the batches: a bfloat16 context, D > 8, an explicit "fast_sqdists" of 1 .. 4, an attached communicator, a source
 * slice (M < M_total). */
int kmvp_gaussian_sinkhorn_batched(kmvp_ctx* ctx, const double* log_a_or_null, const double* log_b_or_null, double tol,
                                   int maxit, double* u, double* v, int* iters, double* err, int* status);
int kmvp_absexp_sinkhorn_batched(kmvp_ctx* ctx, const double* log_a_or_null, const double* log_b_or_null, double tol,
                                 int maxit, double* u, double* v, int* iters, double* err, int* status);

/* Regularised systems (an extension: no reference method stands behind it -- the reference's lstsq solves the bare
 * K b = a; this is the `alpha` / nugget / noise term of kernel ridge regression, Kriging and Gaussian processes).
 * A = K + ridge I + diag(d) for the solvers that follow on this ctx.  d: n doubles (n = number of points of the
 * solve, i.e. N; always the FULL vector, also on a source shard) or NULL with n == 0.  (NULL, 0, 0.0) switches it
 * off.  Products (kmvp_gaussian ...) are not affected.  kmvp_set_points clears it.
 *   The effective diagonal ridge + d_i is kept in float64 on the device for every working precision (the Krylov
 *   vectors are float64) and is added to K v inside the device-resident iteration, after the all-reduce of a
 *   sharded product; rtol, *resid and the 1.5 rtol verdict of the solvers are then about A b = a.
 *   KMVP_E_INVALID: a non-finite ridge or d_i (here); at solve time, n != N, and for the CG entries (Gaussian,
 *   exp(-r), Matern: positive definite only with a non-negative shift) any ridge + d_i < 0.  MINRES takes any sign. */
int kmvp_set_solver_diagonal(kmvp_ctx* ctx, const double* d_or_null, int64_t n, double ridge);

/* Pivoted-Cholesky preconditioner for the conjugate-gradient entries (an extension, opt-in; what Gaussian-process
 * libraries that solve by CG use).  rank in 1 .. KMVP_PRECOND_MAX_RANK: the kmvp_<kernel>_cg_solve calls that follow on
 * this ctx (Gaussian, exp(-r), Matern 3/2 and 5/2) iterate with z = P^-1 r,
 *     P = L L' + D,   L (N, rank') the first rank' <= rank columns of the pivoted Cholesky factorisation of K,
 *                     D = diag(ridge + d_i) as kmvp_set_solver_diagonal set it,
 * applied exactly through the Woodbury identity (2 N rank' flops per column next to the N^2 pair evaluations of the
 * operator).  rank = 0 (the default) switches it off: the solve is then bit for bit the unpreconditioned one.
 * kmvp_set_points switches it off too, as it clears the solver diagonal.  rank < 0: KMVP_E_INVALID; rank >
 * KMVP_PRECOND_MAX_RANK: KMVP_E_UNSUPPORTED; a refused call leaves the previous setting.
 *   The factor is built inside the first solve that needs it (device-resident: argmax of the residual diagonal with ties
 *   to the smaller index, one kernel column in the working precision from the raw points by the difference form -- any D
 *   --, float64 update; no further column once the residual diagonal's maximum is <= 256 unit roundoffs of the working
 *   precision, hence rank' <= rank) and kept until the points, the kernel, the rank or the solver diagonal change.  On a
 *   source shard it is built from the targets, the full cloud on every rank: no communication, the same bits everywhere.
 *   The iteration stops on the same test as the plain one -- sqrt(|r|^2 / |a|^2) <= rtol on the recurrence residual -- so
 *   rtol, *resid and the 1.5 rtol verdict mean what they mean without it; stop word, first-iteration rule, residual
 *   replacement, bursts of 8 iterations and their graph replay carry over.  Bitwise reproducible run to run.
 *   At solve time rank > 0 needs a solver diagonal with ridge + d_i > 0 everywhere (P is positive definite only then):
 *   KMVP_E_INVALID with a message that names the preconditioner otherwise.
 *   kmvp_invdist_minres_solve with rank > 0 is KMVP_E_UNSUPPORTED (that matrix is indefinite).  The
 *   kmvp_<kernel>_lanczos_quadrature entries IGNORE the setting (a preconditioned quadrature needs the log det P
 *   correction: the kmvp_<kernel>_lanczos_quadrature_precond entries below make it); products, gradients and everything
 *   else are unaffected.
 * kmvp_get_solver_preconditioner: what the LAST kmvp_<kernel>_cg_solve (or kmvp_<kernel>_lanczos_quadrature_precond)
 * applied -- *rank_built = rank' (0 when it ran unpreconditioned, nothing else is written then), pivots_or_null (rank'
 * values: the point index of every column), factor_or_null ((rank', N) float64 row-major: row t = column t of L).
 * kmvp_last_preconditioner_ms: the build inside the last of those calls, host wall clock (0 when the factor was reused or
 * the preconditioner is off); kmvp_last_total_ms of that call includes it. */
#define KMVP_PRECOND_MAX_RANK 128
int kmvp_set_solver_preconditioner(kmvp_ctx* ctx, int rank);
int kmvp_get_solver_preconditioner(kmvp_ctx* ctx, int* rank_built, int64_t* pivots_or_null, double* factor_or_null);
double kmvp_last_preconditioner_ms(const kmvp_ctx* ctx);

/* Preconditioned stochastic Lanczos quadrature (an extension): log det A = log det P + tr log M with P = L L' + D the
 * preconditioner above (rank >= 1 set by kmvp_set_solver_preconditioner, a solver diagonal with ridge + d_i > 0) and
 * M = P^-1/2 A P^-1/2, which is close to I: fewer iterations than kmvp_<kernel>_lanczos_quadrature by the factor the
 * preconditioned solve gains, and a smaller variance, since only tr log M is estimated.
 *   *logdet_p = sum_i log D_i + 2 sum_t log G_tt, G the Cholesky factor of I + L' D^-1 L (matrix-determinant lemma): exact.
 *   Probes.  g (N,P) and h (rank,P), float64 row-major in every context, are the caller's (Rademacher: E gg' = I,
 *   E hh' = I); rows t >= rank' of h are not read.  On the device, in float64,
 *       z[i][e] = sqrt(D_i) g[i][e] + sum_t L[t][i] h[t][e]      (t ascending, one fma per term)
 *   so that cov z = P and w = P^-1/2 z has E ww' = I.
 *   Preconditioned conjugate gradients on A x_e = z_e from x = 0 is conjugate gradients on M xh = w: its coefficients
 *   alpha_k = rho_k / p'Ap, beta_k = rho_{k+1} / rho_k, rho = r' P^-1 r, are the Lanczos tridiagonal of (M, w_e), and
 *       wnorm2[e] = rho_0 = z_e' P^-1 z_e = |w_e|^2
 *       logquad[e] = rho_0 sum_i tau_i^2 log(theta_i)  ~  w_e' log(M) w_e      (mean over e: tr log M)
 *       invquad[e] = pz_e' x_e,  pz = P^-1 z                                    (mean over e: tr A^-1)
 *   and for any B, E pz' B x = tr(B A^-1).  x (N,P) or NULL: the iterates as they froze; pz (N,P) or NULL: P^-1 z.
 *   steps, alpha, beta: as kmvp_<kernel>_lanczos_quadrature.
 *   Every column is on its own clock as there, with rho in the place of rs: it freezes after the first iteration with
 *   sqrt(rho_k / rho_0) <= rtol -- the residual of the system whose tridiagonal is recorded --, one step earlier on a
 *   breakdown (p' A p == 0 or rho <= 0); a column with rho_0 == 0 never starts (steps = 0, logquad = invquad = 0, x = 0);
 *   NaN never freezes a column; no residual replacement, no true-residual product.
 * Returns KMVP_OK when every non-zero column froze on the tolerance with a finite logquad, otherwise
 * KMVP_E_NOT_CONVERGED with everything written.  KMVP_E_INVALID: rank == 0 (the message names the preconditioner), no
 * solver diagonal or ridge + d_i <= 0 somewhere, targets != sources, P < 1, maxit < 0, rtol <= 0, a NULL g, h, logdet_p,
 * logquad, invquad, wnorm2 or steps; a bfloat16 context is KMVP_E_UNSUPPORTED.  A refused call leaves the factor and the
 * setting in place.  The factor is built inside the call unless the context holds the current one;
 * kmvp_get_solver_preconditioner and kmvp_last_preconditioner_ms then speak of this call as they do of a solve.
 * Device-resident (one look of the host every 8 iterations, the burst replayed as a graph in long runs; the operator
 * sharded and the vectors replicated with a communicator, the factor built from the full cloud on every rank: every rank
 * returns the same bits); fixed summation order, no atomics: bitwise reproducible.  There is no inverse-distance entry. */
int kmvp_gaussian_lanczos_quadrature_precond(kmvp_ctx* ctx, const double* g, const double* h, int P, double rtol, int maxit,
                                             double* logdet_p, double* logquad, double* invquad, double* wnorm2, int* steps,
                                             double* x_or_null, double* pz_or_null, double* alpha_or_null,
                                             double* beta_or_null);
int kmvp_absexp_lanczos_quadrature_precond(kmvp_ctx* ctx, const double* g, const double* h, int P, double rtol, int maxit,
                                           double* logdet_p, double* logquad, double* invquad, double* wnorm2, int* steps,
                                           double* x_or_null, double* pz_or_null, double* alpha_or_null,
                                           double* beta_or_null);
int kmvp_matern32_lanczos_quadrature_precond(kmvp_ctx* ctx, const double* g, const double* h, int P, double rtol, int maxit,
                                             double* logdet_p, double* logquad, double* invquad, double* wnorm2, int* steps,
                                             double* x_or_null, double* pz_or_null, double* alpha_or_null,
                                             double* beta_or_null);
int kmvp_matern52_lanczos_quadrature_precond(kmvp_ctx* ctx, const double* g, const double* h, int P, double rtol, int maxit,
                                             double* logdet_p, double* logquad, double* invquad, double* wnorm2, int* steps,
                                             double* x_or_null, double* pz_or_null, double* alpha_or_null,
                                             double* beta_or_null);

/* Top-k eigenpairs (an extension: kernel PCA, spectral embedding, the largest eigenvalue for a condition estimate, the
 * exact top-k a low-rank approximation is judged against -- without the N x N matrix).  The k algebraically largest
 * eigenpairs of the symmetric operator A on the cloud given to kmvp_set_points (x_or_null == NULL, as for the solvers):
 *   KMVP_EIG_KERNEL      A = K + ridge I + diag(d) with the diagonal of kmvp_set_solver_diagonal when one is set, else A = K
 *   KMVP_EIG_CENTERED    A = H K H, H = I - 1 1'/N: kernel PCA
 *   KMVP_EIG_NORMALIZED  A = S K S, S = diag(q^-1/2), q = K 1 computed here by one density product at the start: spectral
 *                        embedding; the largest eigenvalue is 1 with eigenvector ~ q^1/2.  degree_or_null (N doubles)
 *                        receives q (untouched for the other operators).
 * A solver diagonal set together with op != KMVP_EIG_KERNEL is KMVP_E_INVALID.
 * The algorithm is the Lanczos process with FULL reorthogonalisation and no restart, held exactly as follows.
 *   v_1 = v0 / |v0| (N doubles; for the centred operator v0 is centred first).  The library draws nothing.
 *   j = 1, 2, ...:  w = A v_j      (the operator rounds its argument to the working precision exactly as the solvers do --
 *                                   for the centred and the normalised operator that argument is H v_j and S v_j;
 *                                   everything else is float64)
 *                   h = V_j' w,  w <- w - V_j h;   h' = V_j' w,  w <- w - V_j h'      (classical Gram-Schmidt, twice)
 *                   alpha_j = h_j + h'_j,   beta_j = |w|_2,   v_{j+1} = w / beta_j
 *   Breakdown: beta_j <= 1e-13 max_{i<=j} |alpha_i| -- v_{j+1} is not formed and the process ends at step j: the Krylov
 *   space of v0 is invariant to working accuracy.
 * The host looks at the process at fixed steps only -- every j >= k with j mod 8 == 0, at breakdown and at j == maxit --
 * so nothing depends on when it happens to look.  At a look it reads the history (alpha, beta), solves the j x j
 * tridiagonal (csrc/kmvp_tridiag.hpp), takes the k largest Ritz values theta_1 >= ... >= theta_k and the estimates
 * beta_j |s_{j,i}| from the last components of their eigenvectors, and stops when every estimate is <= tol |theta_1| (or
 * at breakdown, or at maxit).  Then X = V_j S[:, top k] is formed on the device and one more k-column application of A
 * gives the true residuals resid[i] = |A x_i - theta_i x_i|_2 / (|theta_1| |x_i|_2).  The verdict is on these, as for the
 * solvers: KMVP_OK if every one is finite and <= 1.5 tol, otherwise KMVP_E_NOT_CONVERGED with everything written (also for
 * a non-finite operator, e.g. a NaN coordinate: the outputs are then non-finite; and for a breakdown before step k).
 *   eigenvalues (k): the Ritz values, descending.   eigenvectors (N, k) float64 row-major: unit norm, the sign of each
 *   fixed so that its component of largest magnitude is positive (a tie goes to the smallest index).   resid (k).
 *   *steps: the steps taken.   alpha_or_null, beta_or_null (maxit each): row j - 1 holds step j; rows >= *steps unspecified.
 * Inside a burst of steps nothing crosses to the host: a device kernel forms alpha_j and beta_j, appends them to the
 * history and sets the stop word; the normalisation reads beta_j from device memory.  There is NO graph replay of the
 * burst (the reorthogonalisation grows with every step, so no two steps launch the same work).  Fixed summation orders,
 * no atomics: bitwise reproducible run to run.  With a communicator attached the operator is sharded and the basis
 * replicated, as for the quadrature: every rank returns the same bits.  The context is left as after a solve (no signal);
 * kmvp_last_kernel_ms and kmvp_last_total_ms both cover the whole call.  kmvp_set_solver_preconditioner is ignored.
 * KMVP_E_INVALID: no points set, targets != sources, k < 1 or k > N, maxit < k or maxit > min(N, 512), tol not > 0, a NULL
 * v0, eigenvalues, eigenvectors, resid or steps, a v0 that is non-finite or zero (for the centred operator also: constant,
 * |H v0| <= 1e-13 |v0|).  KMVP_E_UNSUPPORTED: a bfloat16 context; batches set (kmvp_set_batches).  KMVP_E_NOMEM: the basis
 * of (maxit + 1) N doubles does not fit.  There is no inverse-distance entry. */
enum kmvp_eig_operator { KMVP_EIG_KERNEL = 0, KMVP_EIG_CENTERED = 1, KMVP_EIG_NORMALIZED = 2 };
int kmvp_gaussian_eigsh(kmvp_ctx* ctx, int k, int op, const double* v0, double tol, int maxit, double* eigenvalues,
                        double* eigenvectors, double* resid, int* steps, double* alpha_or_null, double* beta_or_null,
                        double* degree_or_null);
int kmvp_absexp_eigsh(kmvp_ctx* ctx, int k, int op, const double* v0, double tol, int maxit, double* eigenvalues,
                      double* eigenvectors, double* resid, int* steps, double* alpha_or_null, double* beta_or_null,
                      double* degree_or_null);
int kmvp_matern32_eigsh(kmvp_ctx* ctx, int k, int op, const double* v0, double tol, int maxit, double* eigenvalues,
                        double* eigenvectors, double* resid, int* steps, double* alpha_or_null, double* beta_or_null,
                        double* degree_or_null);
int kmvp_matern52_eigsh(kmvp_ctx* ctx, int k, int op, const double* v0, double tol, int maxit, double* eigenvalues,
                        double* eigenvectors, double* resid, int* steps, double* alpha_or_null, double* beta_or_null,
                        double* degree_or_null);

/* Source sharding over the GPUs of one node, one process per GPU:
 * rank 0 calls kmvp_comm_get_unique_id and hands the 128 bytes to every rank
 * out of band; every rank then calls kmvp_comm_init.  world == 1 is allowed. */
#define KMVP_UNIQUE_ID_BYTES 128
int kmvp_comm_get_unique_id(void* id128);
int kmvp_comm_init(kmvp_ctx* ctx, const void* id128, int rank, int world);
/* What the attached RCCL communicator ITSELF reports (ncclCommCount / ncclCommUserRank; kmvp_comm_init
 * fails with KMVP_E_COMM when they differ from what it was asked for).  1 / 0 without a communicator.
 * bench.py prints the count as "rccl_ranks" so that a multi-GPU line shows the collective really spanned
 * N ranks. */
int kmvp_comm_world(const kmvp_ctx* ctx);
int kmvp_comm_rank(const kmvp_ctx* ctx);
/* REHEARSAL transport for the same exchange (not the product: RCCL is).  RCCL refuses two ranks on one device,
 * so the multi-rank path of this library -- shard-local kernels with j_offset / M_total, the canonical unpadded
 * [column][N] layout, exchange, normalisation, the sharded solvers -- cannot be exercised with world > 1 on a
 * one-GPU box through kmvp_comm_init.  With this entry the all-reduce is staged through host memory instead:
 * `fn(user, buf, count, op)` must reduce `count` doubles in place over all ranks -- op = KMVP_OP_SUM, or KMVP_OP_MIN
 * (the exponents of the exp(<x,y>) path) -- e.g. by torch.distributed.all_reduce over gloo, and return 0.  Everything else -- what is exchanged, where in the stream, what happens before and
 * after -- is the code path kmvp_comm_init uses.  Never selected implicitly. */
enum kmvp_reduce_op { KMVP_OP_SUM = 0, KMVP_OP_MIN = 1 };
typedef int (*kmvp_host_allreduce_fn)(void* user, double* buf, int64_t count, int op);
int kmvp_comm_init_host(kmvp_ctx* ctx, kmvp_host_allreduce_fn fn, void* user, int rank, int world);

/* BaseAlgorithm.set_query_arguments (base.py:40-42): tuning knobs, all optional.
 *   "feed"             -1 = auto (default), 0 = scalar-cache source stream, 1 = LDS-staged tiles
 *   "targets_per_lane" 0 = auto (default), 1, 2, 4 or 8 (difference form); bf16 path: 1 or 2 target
 *                      tiles per wavefront without software pipelining, 0 = pipelined where instantiated
 *   "segments"         number of source segments a launch is split into (0 = auto)
 *   "chunk"            sources summed in fp32 before folding into the fp64 sum
 *   "fast_sqdists"     squared distances in the expanded form |x|^2+|y|^2-2x.y on the matrix
 *                      cores (bruteforce.py:36-49 `fast_sqdists`; float32):
 *                      1 = always, around one centre for the whole cloud: fast_kernel (E == 1, D <= 39); with several
 *                          signal columns, or beyond D = 39 (Gaussian, D <= 64; exp(-r) at 5 <= D <= 64 inside the
 *                          radius rule, closest pairs recomputed exactly): fastmm_kernel, where the tile of kernel values goes
 *                          back to the matrix cores for the product with the signal, up to 32 columns per pass
 *                          (the denominator of normalised rows is one more column);
 *                      2 = always, around per-group centres of Morton-sorted sources with exact
 *                          recomputation of the closest pairs (cfast_kernel, D <= 4; with several signal
 *                          columns, Gaussian and exp(-r): cfastmm_kernel, the second product of fastmm_kernel
 *                          on these distances);
 *                      3 = always the cell form (Gaussian, D <= 3): exp() is range-reduced by the cells
 *                          of a regular grid, exp(-|x-y|^2) = U_i(S) W_j(T) exp(2 d.e), and the remainder
 *                          polynomial 1 + t + t^2/2 of t = 2 d.e (|t| <= 0.016) comes out of one MFMA per
 *                          32 x 32 pairs -- cellmm_kernel: f16 MFMA that also carries the weights W_j b_j
 *                          and the sum over the sources (any E: one launch per signal column; normalised
 *                          rows: one more with b = 1), on clouds inside the radius rule; cell_kernel
 *                          (bf16 MFMA for the polynomial, one VALU fma per pair; E == 1) otherwise;
 *                          float64 (cell64_kernel, E == 1): the degree-7 polynomial on the VALU;
 *                      4 = as 3 but always cell_kernel (float32);
 *                      0 = never (difference form, bruteforce.py:53-54);
 *                      -1 = auto (default): the cheapest form that is as accurate as the difference form for the
 *                          shape at hand -- which one that is: docs/DISPATCH.md (generated by asking the library),
 *                          the rules themselves: csrc/kmvp_product.hip run_product()
 *   "same_points_global" 1 when the targets passed to kmvp_set_points are the unsharded
 *                      sources (sharded same_points): enables form 2 for inverse-distance
 *   "partial_shard"    1: a source slice (M < M_total) may be run WITHOUT a multi-rank communicator and
 *                      returns that shard's partial sums (the caller adds the shards up); default 0: such
 *                      a call fails with KMVP_E_INVALID instead of passing partial sums off as the product
 *   "fast_tiles"       target tiles of 32 per wavefront in that kernel: 0 = auto, 1, 2, 4, 8
 *                      (clamped to what is instantiated: fast_kernel 4 up to D = 7, 2 up to D = 23,
 *                      1 beyond; cfast_kernel 4; cell_kernel and cellmm_kernel 8) */
/*   "cellmm_shape"     MFMA shape of the float32 cell form: -1 = by size (default: 16x16x32 from 5e5 targets and 1e5 sources
 *                      on with eight target tiles per wave, else 32x32x16), 0 = 32x32x16 (cellmm_kernel), 1 = 16x16x32
 *                      (cellmm16_kernel)
 *   "cell_fused"       cellmm16_kernel's two lists of target tiles (whole groups per cell; the cells' leftover tiles): -1 =
 *                      automatic (default) and 1 = ONE launch, the leftover list's workgroups behind the others, where both
 *                      lists fit one grid; 0 = always two launches.  The sums are the same bit for bit either way
 *   "cell_balance"     the cells of the float32 cell form: 1 = the lattice is kept in x and y and every (x, y) column is cut
 *                      along z by point count (1024 points, one workgroup of target tiles, per cell; shorter only where the
 *                      accuracy bound on a cell's width or the column ends), wherever that applies: D = 3, float32, eight
 *                      target tiles per wavefront, at most ~256 lattice cells along z; -1 = automatic (default): as 1 from the
 *                      sizes at which cellmm16_kernel is taken by itself (N >= 500000, M >= 100000); 0 = never, the lattice's
 *                      cells.  Results agree to the cell form's accuracy, not bit for bit: the cells differ
 *   "cell_shared_build" cellmm16_kernel's workgroups whose four wavefronts own target tiles of ONE cell: -1 = automatic
 *                      (default) and 1 = such a workgroup builds every source operand once and shares it through LDS,
 *                      wherever the kernel holds that body (eight target tiles per wavefront); 0 = never, every wavefront
 *                      builds its own.  The sums are the same bit for bit either way
 *   "cell_tail"        cellmm16_kernel's one launch: 1 = where the workgroups of the list of whole groups do not fill whole
 *                      rounds of resident workgroups (two per compute unit at eight target tiles per wavefront), the target
 *                      blocks of the last, partial round take k times as many, k times shorter source segments, as many as
 *                      run at once beside the leftover list (a third list, TAIL: csrc/kmvp_plan.hpp cell_tail_plan); 0 =
 *                      never; -1 = automatic (default): as 1 at eight target tiles per wavefront from the sizes at which
 *                      cellmm16_kernel is taken by itself (N >= 500000, M >= 100000).  Rows of the TAIL blocks see other
 *                      segment cuts and agree with 0 to the cell form's accuracy; all other rows are the same bit for bit
 *   "cell_tail_resident" the resident workgroups that plan assumes: 0 (default) = the device's; > 0 = this many (tests)
 *   "meanshift_compact" kmvp_gaussian_meanshift: -1 (default) and 1 = the list of active points is compacted after every
 *                      sweep, so the pair loop covers the points still moving; 0 = never, frozen points ride along and are
 *                      ignored.  The results are the same bit for bit either way: it exists to measure what compaction saves
 *   "sinkhorn_retire"  kmvp_<kernel>_sinkhorn_batched: -1 (default) and 1 = the tiles of a stopped batch are retired (their source
 *                      range set to empty), so the pair loop covers the batches still running; 0 = never, stopped batches ride
 *                      along and are ignored.  The results are the same bit for bit either way: it exists to measure what
 *                      retirement saves
 *   "cutoff_plan"      where the cell-list plan of the cutoff entries (kmvp_<kernel>_cutoff, kmvp_<kernel>_cutoff_grad,
 *                      kmvp_radius_count, kmvp_radius_nearest, kmvp_wendland_<c>_cg_solve) is built: 0 (default) = on the host,
 *                      from a copy of the points; 1 = on the device (csrc/kmvp_cutoff_plan_device.hip: radix sort, scans and
 *                      one thread per table entry; two small read-backs, no transfer that grows with the clouds), for a
 *                      cloud that moves every call.  The plan is the same entry for entry (kmvp_cutoff_plan_read) and every
 *                      result the same bit for bit; the value is part of the plan's cache key.  Clouds beyond the device
 *                      build's 32-bit keys (2^31 - 1 points or cells) are planned on the host whatever the option says
 *   "mfma_variant"     bf16 path, software-pipelined kernel: -1 = by kernel (default: exp(-r) 4, others 0), 0 = plain,
 *                      1 = denominators on the matrix pipe (one more accumulator tile per target tile), 4 = loop rotated by one
 *                      transcendental stage, 5 = both (csrc/kmvp_mfma.hpp, mfma_pipe_kernel VAR) */
int kmvp_set_option(kmvp_ctx* ctx, const char* key, int64_t value);
/* Options whose value is a real number:
 *   "cutoff_cell_factor"  the side of the cutoff entries' cells in units of the radius: a finite double >= 1, default 1.
 *                      Larger cells are always correct (counts are identical, products agree to their float32 rounding)
 *                      and walk more pairs: it is there to test and to measure */
int kmvp_set_option_double(kmvp_ctx* ctx, const char* key, double value);

/* BaseAlgorithm.get_memory_usage / get_additional (base.py:35-46): bytes of device
 * memory the ctx holds, and HIP-event timings of the last compute call:
 *   kmvp_last_kernel_ms  the dominant (pair-loop) kernel alone
 *   kmvp_last_total_ms   every launch of the call incl. reduction + all-reduce */
int64_t kmvp_device_bytes(const kmvp_ctx* ctx);
double kmvp_last_kernel_ms(const kmvp_ctx* ctx);
double kmvp_last_total_ms(const kmvp_ctx* ctx);
/*   kmvp_last_allreduce_ms  the RCCL all-reduce of the (N,E[+1]) sums alone (0 without a communicator) */
double kmvp_last_allreduce_ms(const kmvp_ctx* ctx);
/* name of the pair-loop kernel the last compute call launched (for rocprof matching) */
const char* kmvp_last_kernel_name(const kmvp_ctx* ctx);
/* The fastest forms are narrow (kmvp_set_option "fast_sqdists").  When the last product did NOT take the cell form
 * although kernel, precision and dimension would allow it, this says which condition failed (too few points per
 * cloud, too few points per grid cell, the radius rule, ...); "" when nothing faster applied.  get_additional()
 * stores it as "dispatch_note".  When "targets_per_lane" or "feed" is set and lowd_kernel serves the product, the note
 * also ends in "lowd_kernel runs targets_per_lane = T, feed = F": only D = 3 with one column carries every pair, and a
 * pair that is not built is replaced by (1, 1) or (2, 0) without an error. */
const char* kmvp_last_dispatch_note(const kmvp_ctx* ctx);


/* The cell layout of the last product on the cell form (cell_kernel, cellmm_kernel, cellmm16_kernel, cell64_kernel), read
 * back from the structures that kernel read: test infrastructure (oracle/kmvp_cell_model.py takes it as data), read-only.
 * KMVP_E_INVALID unless such a product has run on the current points.
 *   info[8]          [0] source cells, in the order the kernels walk them; [1] target cells; [2] 1 = the cells are
 *                    count-cut ("cell_balance"), 0 = the lattice's; [3] target tiles per wavefront in use; [4] points per
 *                    target tile (32; float64: 128); [5] whose source image: 0 = cell_kernel's, 1 = cellmm_kernel's /
 *                    cellmm16_kernel's, 2 = cell64_kernel's records; [6], [7] target tiles of the list of whole groups and
 *                    of the leftover list (float32)
 *   sigma_b          the power of two the signal of the LAST column was scaled by (cellmm_kernel, cellmm16_kernel; else 0)
 *   source_cell [M], target_cell [N]   the cell of every point: an index into the centres below; -1 = in no tile, -2 = in
 *                    more than one.  A cell of the leftover list is the cell of the same centre in the list of whole groups
 *   source_centres [3 source_cap], target_centres [3 target_cap]   the stored centres (the float32 kernels' are float32
 *                    values); KMVP_E_INVALID when a capacity is below the number of cells, which info then holds
 * Every pointer but info may be NULL: ask for the counts first. */
int kmvp_cell_layout(kmvp_ctx* ctx, int64_t* info, double* sigma_b, int32_t* source_cell, int32_t* target_cell,
                     double* source_centres, int64_t source_cap, double* target_centres, int64_t target_cap);

/* The lists of target tiles of the last product on cellmm_kernel / cellmm16_kernel (float32 cell form), as that product
 * planned them: test infrastructure, read-only.  KMVP_E_INVALID unless such a product has run on the current points.
 *   info[8]          [0], [1], [2] workgroups of target tiles (target blocks) of the MAIN, TAIL and REST list; [3], [4], [5]
 *                    their source segments; [6] the resident workgroups the TAIL plan assumed ("cell_tail_resident"); [7] 1 =
 *                    the lists ran in one launch
 *   target_list [N]  the list whose workgroups computed the target's row: 0 MAIN, 1 REST, 2 TAIL; may be NULL */
int kmvp_cell_lists(kmvp_ctx* ctx, int64_t* info, int32_t* target_list);

#ifdef __cplusplus
}
#endif
#endif /* KMVP_H */
