"""MI355X plugins: the on-the-fly kernel product and the CG solver built on it (and, beyond the reference's plugin
roles, ``MI355XSinkhorn``: entropic optimal transport on the product's log-sum-exp reduction).

Drop-in counterparts of the reference's ``BruteForceProductBLAS``
(bruteforce.py:61-153) and ``BruteForceSolverLAPACK`` (bruteforce.py:156-207):
same constructor keywords, same method order, same result type.  All arithmetic
happens in ``libkmvp.so`` (hand-written HIP kernels for gfx950) behind the C ABI
of ``include/kmvp.h``.  There is no CPU path: without the library or a GPU the
calls raise.

Differences a user should know about
 * ``fit()`` never forms the N x M matrix; it builds what the points alone determine
   (``kmvp_fit``: grid, cell order and tile lists of the Gaussian cell kernels, a few ms
   at 1e6 points; nothing for the other kernels).  Compare on build_time + query_time,
   which is the harness' default axis (plot.py:128).
 * The HIP context is created in ``prepare_data`` -- never at import or
   construction -- because the harness imports plugins in its parent process
   before forking the worker (main.py:262-308).
 * The solver is conjugate gradients on the product operator with a residual
   stopping rule; the dense ``lstsq`` of the reference cannot be matched
   vector-for-vector on these numerically singular matrices, so it
   reports (and is tested on) the relative residual.  ``MI355XSolver(ridge=...)``
   solves the regularised system (K + ridge I) b = a instead, which is well posed
   and is tested against a dense solve on the solution vector.
"""
import collections

import numpy as np

from kernel_matrix_benchmarks_amd import _lib
from kernel_matrix_benchmarks_amd.algorithms.base import BaseProduct, BaseSolver
from kernel_matrix_benchmarks_amd import sharding

SUPPORTED_KERNELS = ("gaussian", "absolute-exponential", "inverse-distance", "exp-dot", "matern-3/2", "matern-5/2")
# "matern-3/2", "matern-5/2": the Matern covariances (1 + t) e^-t, t = sqrt(3) r, and (1 + t + t^2/3) e^-t, t = sqrt(5) r,
# at length scale 1 (sklearn's Matern(length_scale=1, nu=1.5 / 2.5); a length scale is the caller's scaling of the
# points).  An extension -- the reference has nu = 1/2 only, as "absolute-exponential" -- checked against the
# definition (the tests' matern_reference).  float16 / float32 / float64, difference form only: bfloat16 and an
# explicit fast_sqdists are refused.
MATERN_KERNELS = ("matern-3/2", "matern-5/2")
# "wendland-c2", "wendland-c4": Wendland's compactly supported functions u^4 (4 t + 1) and u^6 (35 t^2 + 18 t + 3) / 3 of
# t = |x - y| / R, u = max(1 - t, 0): positive definite for D <= 3, identically 0 beyond the support radius R.  An
# extension -- the reference has no such kernel.  The support radius is an argument of the call, so the product runs
# through MI355XProduct.query_cutoff(R) alone (it IS the full product) and the solve through
# MI355XSolver(support_radius=R); float16 / float32 / float64, D <= 3.
WENDLAND_KERNELS = ("wendland-c2", "wendland-c4")
# "exp-dot": k(x, y) = exp(<x, y>), the transformer attention kernel the reference's README defines
# (README.md:51-59) but its plugins do not implement (bruteforce.py:18-22 has the other three): parity
# unpinned, checked against a direct numpy evaluation only (the tests' exp_dot_product).  Two routes:
#  * NATIVE (float32 / float16 inputs at D <= 64, bfloat16 at D <= 141; include/kmvp.h kmvp_expdot[_norm]): S = X Y^T
#    straight from the matrix cores, kernel values relative to a per-target running exponent (the flash-attention
#    recurrence), partial sums merged as (mantissa, exponent) pairs -- softmax attention never forms exp(max logit),
#    up to |largest logit| < 32000 ln 2 ~ 2.2e4 (the clamp of the integer exponent; beyond it the library refuses the
#    product); plain products overflow where exp(<x, y>) leaves float64, as numpy's would.
#  * IDENTITY (float64, float32 at D > 64, and the solver):
#        exp(<x, y>) = exp(|x|^2 / 2) * exp(-|x/sqrt2 - y/sqrt2|^2) * exp(|y|^2 / 2)
#    i.e. a GAUSSIAN product on the points / sqrt(2) with the signal weighted by w_j = exp(|y_j|^2/2 - c)
#    (c = max_j |y_j|^2/2, so w <= 1) -- every Gaussian kernel of the library serves it.  Row-normalised: (K (w b)) /
#    (K w), the factor of the target cancels; plain products multiply it back in float64.  Valid while
#    |y_j|^2/2 spans less than the exponent range of the working precision: checked in prepare_data
#    (EXPDOT_IDENTITY_SPREAD), NotImplementedError beyond it -- never a silent zero weight.
SQRT_HALF = 0.7071067811865476
GRADIENT_MAX_D, GRADIENT_MAX_E = 8, 4  # lowd_grad_kernel's instantiations (csrc/kmvp_internal.hpp LOWD_MAX_D, LOWD_MAX_E)
# lowd_dscale_kernel: the derivative in the per-axis length scales, at the gradient's shapes; no 1/r (not a covariance)
SCALE_DERIVATIVE_KERNELS = ("gaussian", "absolute-exponential", "matern-3/2", "matern-5/2")
# lowd_lse_kernel: the log-sum-exp reduction is built for these kernels, at the gradient's shapes
LOGSUMEXP_KERNELS = ("gaussian", "absolute-exponential")
BATCHED_KERNELS = ("gaussian", "absolute-exponential", "matern-3/2", "matern-5/2")  # kmvp_set_batches
LOGSUMEXP_MAX_D, LOGSUMEXP_MAX_E = 8, 4
# lowd_knn_kernel: K nearest neighbours, at the gradient's dimensions; K + 1 candidates are collected with exclude_self
NEAREST_MAX_D, NEAREST_MAX_K = 8, 16
CUTOFF_KERNELS = BATCHED_KERNELS  # kmvp_<kernel>_cutoff
CUTOFF_MAX_D = 3                  # the cutoff entries' cell list


def _cutoff_plan_code(cutoff_plan):
    """cutoff_plan="host" | "device" -> the value of the library's "cutoff_plan" option (include/kmvp.h)."""
    if cutoff_plan not in _lib.CUTOFF_PLAN_SIDES:
        raise ValueError(f"cutoff_plan must be 'host' or 'device', not {cutoff_plan!r}")
    return _lib.CUTOFF_PLAN_SIDES.index(cutoff_plan)
EXPDOT_NATIVE_MAX_D = 64
EXPDOT_NATIVE_MAX_D_BF16 = 141  # 16 * 9 k-steps - 3 operand columns (kmvp_mfma.hpp MFMA_DOT_AUG)
# largest spread max_j |y_j|^2/2 - min_j |y_j|^2/2 the identity route accepts: the smallest weight is exp(-spread);
# float32 / bfloat16 (8-bit exponent): e^-80 = 2^-115 is still a normal number; float64: e^-700
EXPDOT_IDENTITY_SPREAD = {"float32": 80.0, "float64": 700.0}


def _sq_norms_on_device(p_scaled, bf16):
    """|p'|^2 in float64 of the SCALED points exactly as the device will see them (float32 / float64 values as cast;
    bfloat16: rounded to nearest even as the packing kernels round) -- so that the weights exp(|y'|^2) and the
    Gaussian exp(-|x' - y'|^2) are about the same points and the identity holds to rounding of the arithmetic only."""
    q = np.asarray(p_scaled)
    if bf16:
        u = np.ascontiguousarray(q, dtype=np.float32).view(np.uint32)
        u = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
        q = u.view(np.float32)
    q = q.astype(np.float64)
    return np.sum(q * q, axis=1)


def _precision_name(precision):
    if isinstance(precision, str):
        return precision
    return np.dtype(precision).name


class MI355XProduct(BaseProduct):
    """a_i = sum_j k(x_i, y_j) b_j on one MI355X, or on several with the sources
    sharded over ranks (``comm`` = a ``sharding.Communicator``)."""

    def __init__(self, *, kernel, dimension, normalize_rows=False, precision=np.float32,
                 fast_sqdists=None, device=0, comm=None, targets_per_lane=0, feed=None, segments=0,
                 chunk=0, fast_tiles=0, cutoff_plan="host"):
        super().__init__(kernel=kernel, dimension=dimension, normalize_rows=normalize_rows,
                         precision=precision)
        if kernel not in SUPPORTED_KERNELS + WENDLAND_KERNELS:
            # same failure mode as bruteforce.py:82-85
            raise NotImplementedError(f"MI355XProduct doesn't support kernel {kernel}.")
        self._dot = kernel == "exp-dot"
        self._dot_native = False  # decided in prepare_data (needs D)
        self._device_kernel_fn = "gaussian" if self._dot else kernel
        self._dtype_code, self._host_dtype = _lib.dtype_code(precision)  # NotImplementedError if unknown
        # precision="float16" (algos.yaml:157): inputs rounded to float16 as the reference casts them
        # (bruteforce.py:103-111,126), arithmetic in float32 on the GPU
        self._round = _lib.input_rounding(precision)
        self.device = device
        self.comm = comm
        # fast_sqdists mirrors the reference's flag (bruteforce.py:70,36-49): True = expanded
        # |x|^2+|y|^2-2x.y form around one centre (matrix cores), False = difference form,
        # "centred" = expanded around per-group centres with exact recomputation of the closest
        # pairs; "cells" = the Gaussian's exp() range-reduced by grid cells, polynomial remainder
        # on the matrix cores (D <= 3: cellmm_kernel, which also sums over the sources in the MFMA
        # accumulator, where it applies; "cells-valu" = always cell_kernel, which sums on the VALU);
        # None lets the library pick the cheapest form that is as accurate as the difference form.
        if fast_sqdists not in (None, False, True, "centred", "cells", "cells-valu"):
            raise ValueError("fast_sqdists must be None, False, True, 'centred', 'cells' or 'cells-valu'")
        if kernel in WENDLAND_KERNELS:
            if self._dtype_code == _lib.KMVP_BF16:
                raise NotImplementedError(f"MI355XProduct doesn't support kernel {kernel} with precision='bfloat16' "
                                          "(float16, float32 and float64 only).")
            if fast_sqdists not in (None, False):
                raise NotImplementedError(f"MI355XProduct doesn't support kernel {kernel} with fast_sqdists={fast_sqdists!r}: "
                                          "the Wendland kernels run through query_cutoff alone (None or False).")
        if kernel in MATERN_KERNELS:
            # what the library has no kernel for (it would answer KMVP_E_UNSUPPORTED), refused before it is called
            if self._dtype_code == _lib.KMVP_BF16:
                raise NotImplementedError(f"MI355XProduct doesn't support kernel {kernel} with precision='bfloat16' "
                                          "(float16, float32 and float64 only).")
            if fast_sqdists not in (None, False):
                raise NotImplementedError(f"MI355XProduct doesn't support kernel {kernel} with fast_sqdists={fast_sqdists!r}: "
                                          "the Matern kernels run in the difference form only (None or False).")
        self.fast_sqdists = fast_sqdists
        self._options = dict(targets_per_lane=targets_per_lane, feed=feed, segments=segments,
                             chunk=chunk, fast_tiles=fast_tiles,
                             # the query_cutoff* / query_radius_* calls: their cell-list plan built on the host (default)
                             # or on the device -- same plan, same bits; for points that move every call
                             cutoff_plan=_cutoff_plan_code(cutoff_plan))
        self._ctx = None
        self.res = None
        self.name = f"MI355XProduct({_precision_name(precision)})" if fast_sqdists is None else (
            f"MI355XProduct({_precision_name(precision)}, fast_sqdists={fast_sqdists})")

    def _cast(self, a):
        if self._round is not None:
            a = np.asarray(a, dtype=self._round)
        return np.ascontiguousarray(a, dtype=self._host_dtype)

    # -- untimed -------------------------------------------------------------------
    def prepare_data(self, *, source_points, target_points, same_points=False,
                     density_estimation=False, source_batches=None, target_batches=None):
        """source_batches / target_batches: B + 1 offsets each into the concatenated sources / targets -- batched clouds
        (include/kmvp.h kmvp_set_batches): query() is then the block-diagonal product and query_nearest() stays within a
        target's own batch; the other query_* methods raise the library's error.  target_batches=None with
        same_points=True means the sources' offsets."""
        # h5py hands numpy.bool_ attributes over (runner.py:41-43)
        self.same_points = bool(same_points)
        self.density_estimation = bool(density_estimation)
        batches = self._check_batches(source_points, target_points, source_batches, target_batches)
        self._dot_note = ""
        if self._dot:
            d_in = np.asarray(source_points).shape[1]
            self._dot_native = ((self._dtype_code == _lib.KMVP_F32 and d_in <= EXPDOT_NATIVE_MAX_D) or
                                (self._dtype_code == _lib.KMVP_BF16 and d_in <= EXPDOT_NATIVE_MAX_D_BF16))
            self._device_kernel_fn = "exp-dot" if self._dot_native else "gaussian"
        if self._dot and not self._dot_native:
            # the caller's points in the working precision first (what the kernel is defined on), then the identity
            ys = np.asarray(self._cast(source_points), dtype=np.float64)
            xs = ys if self.same_points else np.asarray(self._cast(target_points), dtype=np.float64)
            source_points = ys * SQRT_HALF
            target_points = xs * SQRT_HALF
            bf16 = self._dtype_code == _lib.KMVP_BF16
            hy = _sq_norms_on_device(self._cast(source_points), bf16)   # |y/sqrt2|^2 = |y|^2 / 2
            hx = hy if self.same_points else _sq_norms_on_device(self._cast(target_points), bf16)
            shift = float(np.max(hy)) if len(hy) else 0.0
            spread = float(shift - np.min(hy)) if len(hy) else 0.0
            budget = EXPDOT_IDENTITY_SPREAD["float64" if self._dtype_code == _lib.KMVP_F64 else "float32"]
            self._dot_note = (f"exp-dot through the Gaussian identity ({_precision_name(self.precision)}, D = {ys.shape[1]}): "
                              f"|y|^2/2 spans {spread:.3g} of the {budget:g} this precision's exponent range allows")
            if not spread <= budget:
                raise NotImplementedError(
                    f"exp-dot through the Gaussian identity: |y_j|^2/2 spans {spread:.4g} > {budget:g}; sources of small norm "
                    f"would silently get weight 0 in {_precision_name(self.precision)}.  Use precision='float32' with D <= "
                    f"{EXPDOT_NATIVE_MAX_D} (native online-max kernel, logits up to ~2.2e4) or float64 (spread <= "
                    f"{EXPDOT_IDENTITY_SPREAD['float64']:g}).")
            self._w = np.exp(hy - shift).reshape(-1, 1)   # source weights, <= 1
            self._hx = hx + shift                         # log of the target factor exp(|x|^2/2 + c)
        y = self._cast(source_points)
        self.M, self.D = y.shape
        if self.same_points:
            x = None
            self.N = self.M
        else:
            x = self._cast(target_points)
            self.N = x.shape[0]
        if self._ctx is None:
            self._ctx = _lib.Context(self.device)
            for key, value in self._options.items():
                if value:
                    self._ctx.set_option(key, value)
            if self.fast_sqdists is not None:
                code = {"centred": 2, "cells": 3, "cells-valu": 4}.get(self.fast_sqdists, int(bool(self.fast_sqdists)))
                self._ctx.set_option("fast_sqdists", code)
        world = 1 if self.comm is None else self.comm.world
        if world > 1:
            # every rank keeps all targets and one contiguous slice of the sources
            self._shard = sharding.shard_range(self.M, self.comm.rank, world)
            lo, hi = self._shard
            # Gaussian (no index-based rule): shard the sources cell by cell instead of in the caller's
            # order -- every rank derives the same permutation from the full cloud it was handed
            # (every other kernel, the Matern kernels included, keeps the caller's source order)
            self._order = (sharding.spatial_order(y) if self._device_kernel_fn == "gaussian" and self._host_dtype == np.float32
                           else None)
            if self._order is not None:
                targets = y if x is None else x
                y = y[self._order]
                x = targets
            self.comm.attach(self._ctx)
            # the context sees the targets as an explicit array; tell it when they ARE the
            # (unsharded) sources, which the inverse-distance zero rule of the centred form needs
            self._ctx.set_option("same_points_global", 1 if x is None else 0)
            self._ctx.set_points(np.ascontiguousarray(y[lo:hi]), y if x is None else x,
                                 self._dtype_code, j_offset=lo, M_total=self.M)
        else:
            self._shard = (0, self.M)
            self._order = None
            self._ctx.set_points(y, x, self._dtype_code)
        self._batched = batches is not None
        if batches is not None:
            self._ctx.set_batches(*batches)

    def _check_batches(self, source_points, target_points, source_batches, target_batches):
        """The offsets of batched clouds as (source offsets, target offsets or None), or None without batches: everything
        the host can decide (shape, dtype, monotonicity, what the batches are not built for) is refused here, before any
        device call."""
        if source_batches is None and target_batches is None:
            return None
        if source_batches is None:
            raise ValueError("target_batches needs source_batches")
        if target_batches is None and not self.same_points:
            raise ValueError("target_batches=None needs same_points=True (the sources' offsets then serve both)")
        M = np.asarray(source_points).shape[0]
        yb = _lib.batch_offsets(source_batches, "source_batches", M)
        xb = None
        if target_batches is not None:
            N = M if self.same_points else np.asarray(target_points).shape[0]
            xb = _lib.batch_offsets(target_batches, "target_batches", N)
            if xb.size != yb.size:
                raise ValueError(f"target_batches has {xb.size} offsets, source_batches {yb.size}: both hold B + 1")
        what = None
        if self.kernel not in BATCHED_KERNELS:
            what = f"kernel={self.kernel!r} (gaussian, absolute-exponential, matern-3/2 and matern-5/2 only)"
        elif self._dtype_code == _lib.KMVP_BF16:
            what = "precision='bfloat16' (float16, float32 and float64 only)"
        elif self.fast_sqdists not in (None, False):
            what = f"fast_sqdists={self.fast_sqdists!r} (the difference form only: None or False)"
        elif self.comm is not None and self.comm.world > 1:
            what = "sources sharded over ranks (comm=)"
        if what is not None:
            raise NotImplementedError(f"MI355XProduct doesn't support batched clouds with {what}.")
        return yb, xb

    def prepare_query(self, *, source_signal):
        if self._dot_native and self.density_estimation:
            source_signal = np.ones((self.M, 1))  # the library's exp(<x,y>) entry takes an explicit signal
        if self._dot and not self._dot_native:
            # weighted signal [w b | w]: numerator columns and (normalised rows) the denominator column
            b = np.ones((self.M, 1)) if self.density_estimation else np.asarray(self._cast(source_signal), dtype=np.float64)
            if b.ndim == 1:
                b = b.reshape(-1, 1)
            if b.ndim != 2 or b.shape[0] != self.M:
                raise ValueError(f"source_signal has shape {b.shape}, expected ({self.M}, E)")
            self.E = b.shape[1]
            cols = [self._w * b] + ([self._w] if self.normalize_rows else [])
            wb = np.ascontiguousarray(np.concatenate(cols, axis=1), dtype=self._host_dtype)
            lo, hi = self._shard
            if self._order is not None:
                wb = wb[self._order]
            self._ctx.set_signal(np.ascontiguousarray(wb[lo:hi]))
            return
        if self.density_estimation and not self._dot_native:
            self._ctx.set_signal(None)
            self.E = 1
            return
        b = self._cast(source_signal)
        if b.ndim == 1:
            b = b.reshape(-1, 1)
        if b.ndim != 2 or b.shape[0] != self.M:
            # the reference fails in its matmul (bruteforce.py:150); here a short array would be read past its end
            raise ValueError(f"source_signal has shape {b.shape}, expected ({self.M}, E)")
        self.E = b.shape[1]
        lo, hi = self._shard
        if self._order is not None:
            b = b[self._order]  # the sources were sharded in cell order (prepare_data)
        self._ctx.set_signal(np.ascontiguousarray(b[lo:hi]))

    def get_result(self):
        if self._dot and not self._dot_native:
            if self.normalize_rows:
                res = self._ctx.get_result(self.N, self.E + 1)
                return np.ascontiguousarray(res[:, : self.E] / res[:, self.E:])  # exp(|x_i|^2/2) cancels
            res = self._ctx.get_result(self.N, self.E)
            hx = self._hx.reshape(-1, 1)
            with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
                out = res * np.exp(hx)
                # exp(|x|^2/2 + c) alone may leave float64 where the product does not (the Gaussian factor is tiny
                # there): those rows are put together in the log domain.  (A Gaussian factor that underflowed to 0 under
                # an infinite target factor stays NaN: nothing is known about that entry, and 0 would be a guess.)
                late = ~np.isfinite(out) & np.isfinite(res) & (res != 0)
                if late.any():
                    out = np.where(late, np.sign(res) * np.exp(np.log(np.abs(res)) + hx), out)
            return np.ascontiguousarray(out)
        return self._ctx.get_result(self.N, self.E)

    # -- timed ---------------------------------------------------------------------
    def fit(self):
        """The kernel matrix is never formed; what the points alone determine (grid, cell order and tile
        lists of the Gaussian cell kernels) is built here, as the reference builds its structure in fit()."""
        if not self._dot_native:  # (the native exp(<x,y>) path has nothing the points alone determine)
            self._ctx.fit(self._device_kernel_fn)

    def _refuse_wendland(self, method):
        """The Wendland kernels live in query_cutoff(R) alone: R is their support, and the call's argument."""
        if self.kernel in WENDLAND_KERNELS:
            raise NotImplementedError(f"MI355XProduct.{method} doesn't support kernel={self.kernel!r}: the kernel vanishes beyond "
                                      "its support radius, which is an argument of query_cutoff(radius) -- use query_cutoff.")

    def query(self):
        self._refuse_wendland("query")
        # synchronous: the device (and the all-reduce) is done when this returns
        self._ctx.run(self._device_kernel_fn, self.normalize_rows and (self._dot_native or not self._dot))
        self.res = None  # the result stays on the device until get_result()

    def query_gradient(self):
        """G[i, e, :] = grad_{x_i} sum_j k(x_i, y_j) b[j, e] (include/kmvp.h kmvp_<kernel>_grad): the timed part, like
        query().  The targets are independent variables, also with same_points.  Synchronous."""
        self._refuse_wendland("query_gradient")
        self._check_gradient_supported()
        self._ctx.run_grad(self.kernel)
        self.res = None

    def _check_gradient_supported(self):
        """What lowd_grad_kernel is not built for, refused before the library is called."""
        what = None
        if self.normalize_rows:
            what = "normalize_rows=True (the gradient of a ratio of sums is not built)"
        elif self.kernel == "exp-dot":
            what = "kernel='exp-dot'"
        elif self._dtype_code == _lib.KMVP_BF16:
            what = "precision='bfloat16' (float16, float32 and float64 only)"
        elif self.D > GRADIENT_MAX_D:
            what = f"D = {self.D} > {GRADIENT_MAX_D}"
        elif self.E > GRADIENT_MAX_E:
            what = f"E = {self.E} > {GRADIENT_MAX_E} signal columns (pass them in blocks of {GRADIENT_MAX_E})"
        if what is not None:
            raise NotImplementedError(f"MI355XProduct.query_gradient doesn't support {what}.")

    def get_gradient(self):
        """(N, E, D) float64, C-contiguous: the result of the last query_gradient()."""
        return np.ascontiguousarray(self._ctx.get_result(self.N, self.E * self.D).reshape(self.N, self.E, self.D))

    def query_scale_derivative(self):
        """H[i, e, d] = d/d log l_d of sum_j k(x_i / l, y_j / l) b[j, e] at l = 1, one length scale per axis (include/kmvp.h
        kmvp_<kernel>_dscale): -w (x_{i,d} - y_{j,d})^2 with the gradient's weight w.  The length scales are the caller's
        scaling of the points; H.sum(axis=2) is the derivative in one isotropic length scale.  The timed part, like
        query().  Synchronous."""
        self._refuse_wendland("query_scale_derivative")
        self._check_scale_derivative_supported()
        self._ctx.run_dscale(self.kernel)
        self.res = None

    def _check_scale_derivative_supported(self):
        """What lowd_dscale_kernel is not built for, refused before the library is called -- the kernel, the precision and
        the normalisation before prepare_data() too."""
        what = None
        if self.kernel not in SCALE_DERIVATIVE_KERNELS:
            what = f"kernel={self.kernel!r} (gaussian, absolute-exponential, matern-3/2 and matern-5/2 only)"
        elif self.normalize_rows:
            what = "normalize_rows=True (the derivative of a ratio of sums is not built)"
        elif self._dtype_code == _lib.KMVP_BF16:
            what = "precision='bfloat16' (float16, float32 and float64 only)"
        if what is None and self._ctx is None:
            raise RuntimeError("query_scale_derivative() needs prepare_data() and prepare_query() first")
        if what is None and self.D > GRADIENT_MAX_D:
            what = f"D = {self.D} > {GRADIENT_MAX_D}"
        elif what is None and self.E > GRADIENT_MAX_E:
            what = f"E = {self.E} > {GRADIENT_MAX_E} signal columns (pass them in blocks of {GRADIENT_MAX_E})"
        if what is not None:
            raise NotImplementedError(f"MI355XProduct.query_scale_derivative doesn't support {what}.")

    def get_scale_derivative(self):
        """(N, E, D) float64, C-contiguous: the result of the last query_scale_derivative()."""
        return np.ascontiguousarray(self._ctx.get_result(self.N, self.E * self.D).reshape(self.N, self.E, self.D))

    def query_logsumexp(self):
        """L[i, e] = log sum_j exp(l(x_i, y_j) + c[j, e]), l = -|x - y|^2 (gaussian) or -|x - y| (absolute-exponential),
        with the array given to prepare_query(source_signal=c) read as LOG-weights (density estimation: c = 0; c = -inf:
        weight 0); include/kmvp.h kmvp_<kernel>_logsumexp.  A temperature is the caller's scaling of the points and of
        c.  The timed part, like query().  Synchronous."""
        self._refuse_wendland("query_logsumexp")
        self._check_logsumexp_supported()
        self._ctx.run_lse(self.kernel)
        self.res = None

    def _check_logsumexp_supported(self, method="query_logsumexp"):
        """What lowd_lse_kernel and lowd_lse_grad_kernel are not built for, refused before the library is called."""
        what = None
        if self.kernel not in LOGSUMEXP_KERNELS:
            what = f"kernel={self.kernel!r} (gaussian and absolute-exponential only)"
        elif self.normalize_rows:
            what = "normalize_rows=True (row normalisation does not exist for this reduction)"
        elif self._dtype_code == _lib.KMVP_BF16:
            what = "precision='bfloat16' (float16, float32 and float64 only)"
        elif self.D > LOGSUMEXP_MAX_D:
            what = f"D = {self.D} > {LOGSUMEXP_MAX_D}"
        elif self.E > LOGSUMEXP_MAX_E:
            what = f"E = {self.E} > {LOGSUMEXP_MAX_E} columns (they are independent: pass them in blocks of {LOGSUMEXP_MAX_E})"
        elif self.fast_sqdists not in (None, False):
            what = f"fast_sqdists={self.fast_sqdists!r} (the difference form only: None or False)"
        if what is not None:
            raise NotImplementedError(f"MI355XProduct.{method} doesn't support {what}.")

    def get_logsumexp(self):
        """(N, E) float64, C-contiguous: the result of the last query_logsumexp()."""
        return np.ascontiguousarray(self._ctx.get_result(self.N, self.E))

    def query_logsumexp_gradient(self):
        """G[i, e, :] = grad_{x_i} L[i, e] of query_logsumexp()'s L: the softmax-weighted sum of -2 (x_i - y_j) (gaussian:
        G = -2 (x_i - barycentre)) or -(x_i - y_j) / |x_i - y_j| (absolute-exponential), with the array given to
        prepare_query(source_signal=c) read as LOG-weights; include/kmvp.h kmvp_<kernel>_logsumexp_grad.  The targets
        are independent variables, also with same_points.  A (row, column) without a live term is NaN.  The timed part,
        like query().  Synchronous."""
        self._refuse_wendland("query_logsumexp_gradient")
        self._check_logsumexp_supported("query_logsumexp_gradient")
        self._ctx.run_lse_grad(self.kernel)
        self.res = None

    def get_logsumexp_gradient(self):
        """(N, E, D) float64, C-contiguous: the result of the last query_logsumexp_gradient()."""
        return np.ascontiguousarray(self._ctx.get_result(self.N, self.E * self.D).reshape(self.N, self.E, self.D))

    def query_nearest(self, k, exclude_self=False):
        """The k sources nearest to every target and their squared distances (include/kmvp.h kmvp_nearest): nearest first,
        ties in ascending index, indices into source_points as given to prepare_data(); where fewer than k sources qualify
        the tail is (-1, +inf).  exclude_self (same_points only) leaves point i out of its own row.  Needs prepare_data()
        only: no signal is read, and the plugin's kernel function does not enter.  The timed part, like query().
        Synchronous; a sharded plugin merges the ranks' candidates, and every rank gets the same result."""
        k = int(k)
        what = None
        if self._dtype_code == _lib.KMVP_BF16:
            what = "precision='bfloat16' (float16, float32 and float64 only)"
        elif self._ctx is None:
            raise RuntimeError("query_nearest() needs prepare_data() first")
        elif self._dot and not self._dot_native:
            what = "kernel='exp-dot' through the Gaussian identity (the context holds rescaled points)"
        elif self.D > NEAREST_MAX_D:
            what = f"D = {self.D} > {NEAREST_MAX_D}"
        elif k + bool(exclude_self) > NEAREST_MAX_K:
            what = f"k = {k} > {NEAREST_MAX_K - bool(exclude_self)}" + (" with exclude_self" if exclude_self else "")
        elif self.fast_sqdists not in (None, False):
            what = f"fast_sqdists={self.fast_sqdists!r} (the difference form only: None or False)"
        elif self._order is not None:
            what = ("a sharded float32 Gaussian plugin, whose sources were dealt to the ranks in cell order: ties would no "
                    "longer resolve towards the smaller index of the caller's order (use another kernel= for the neighbour query)")
        if what is not None:
            raise NotImplementedError(f"MI355XProduct.query_nearest doesn't support {what}.")
        if exclude_self and not self.same_points:
            raise ValueError("exclude_self needs same_points=True")
        self._nearest = self._ctx.run_nearest(k, exclude_self)

    def get_nearest(self):
        """(idx (N, k) int64, sqdist (N, k) float64), C-contiguous: the result of the last query_nearest() or
        query_radius_nearest()."""
        return self._nearest

    def _check_cutoff_supported(self, method):
        """What the cutoff-radius entries are not built for, refused before the library is called."""
        what = None
        if self._ctx is None:
            raise RuntimeError(f"{method}() needs prepare_data() first")
        if self._dtype_code == _lib.KMVP_BF16:
            what = "precision='bfloat16' (float16, float32 and float64 only)"
        elif self._dot and not self._dot_native:
            what = "kernel='exp-dot' through the Gaussian identity (the context holds rescaled points)"
        elif self.D > CUTOFF_MAX_D:
            what = f"D = {self.D} > {CUTOFF_MAX_D}"
        elif self.comm is not None and self.comm.world > 1:
            what = "sources sharded over ranks (comm=)"
        if what is not None:
            raise NotImplementedError(f"MI355XProduct.{method} doesn't support {what}.")

    def query_cutoff(self, radius):
        """The product over the sources within ``radius`` of every target (include/kmvp.h kmvp_<kernel>_cutoff), on a cell
        list: O(N x neighbours) instead of O(N M).  A pair is inside iff its squared distance in the working precision is
        <= radius^2; a target with nothing inside gets 0 (NaN with normalize_rows).  For kernel="wendland-c2" / "wendland-c4"
        ``radius`` is the support radius and nothing is truncated.  Honours normalize_rows and density estimation; read the result with get_result().  The timed part, like query().  Synchronous."""
        self._check_cutoff_supported("query_cutoff")
        if self.kernel not in CUTOFF_KERNELS + WENDLAND_KERNELS:
            raise NotImplementedError(f"MI355XProduct.query_cutoff doesn't support kernel={self.kernel!r} (gaussian, "
                                      "absolute-exponential, matern-3/2, matern-5/2, wendland-c2 and wendland-c4 only).")
        self._ctx.run_cutoff(self.kernel, radius, self.normalize_rows)
        self._cutoff_info = self._ctx.cutoff_info()
        self.res = None

    def query_cutoff_gradient(self, radius):
        """G[i, e, :] = the gradient with respect to x_i of the sum over the sources within ``radius`` (include/kmvp.h
        kmvp_<kernel>_cutoff_grad): query_gradient()'s terms over query_cutoff()'s inside set, on the same cell list and the
        same packed records.  For kernel="wendland-c2" / "wendland-c4" it is the exact gradient of the exact product.  A
        target with nothing inside gets zeros.  Honours density estimation; read the result with get_gradient().  The
        timed part, like query().  Synchronous."""
        self._check_cutoff_supported("query_cutoff_gradient")
        what = None
        if self.kernel not in CUTOFF_KERNELS + WENDLAND_KERNELS:
            what = (f"kernel={self.kernel!r} (gaussian, absolute-exponential, matern-3/2, matern-5/2, wendland-c2 and "
                    "wendland-c4 only)")
        elif self.normalize_rows:
            what = "normalize_rows=True (the gradient of a ratio of sums is not built)"
        elif self.E > GRADIENT_MAX_E:
            what = f"E = {self.E} > {GRADIENT_MAX_E} signal columns (pass them in blocks of {GRADIENT_MAX_E})"
        if what is not None:
            raise NotImplementedError(f"MI355XProduct.query_cutoff_gradient doesn't support {what}.")
        self._ctx.run_cutoff_grad(self.kernel, radius)
        self._cutoff_info = self._ctx.cutoff_info()
        self.res = None

    def query_radius_count(self, radius, exclude_self=False):
        """The number of sources within ``radius`` of every target (include/kmvp.h kmvp_radius_count): DBSCAN's core-point
        test, ball_query's lengths.  exclude_self (same_points only) leaves a point's own pair out.  Needs prepare_data()
        only: no signal is read, and the plugin's kernel function does not enter.  Synchronous."""
        self._check_cutoff_supported("query_radius_count")
        if exclude_self and not self.same_points:
            raise ValueError("exclude_self needs same_points=True")
        self._radius_count = self._ctx.radius_count(radius, exclude_self)
        self._cutoff_info = self._ctx.cutoff_info()

    def query_radius_nearest(self, k, radius, exclude_self=False):
        """The k nearest sources of every target among those within ``radius`` (include/kmvp.h kmvp_radius_nearest), on the
        cell list: ball_query with indices, a fixed-radius neighbour list, a k-NN graph on a cloud too large for
        query_nearest().  Row for row it is query_nearest(k, exclude_self) with every entry beyond radius^2 (in the working
        precision) replaced by (-1, +inf): nearest first, ties in ascending index, indices into source_points.  Needs
        prepare_data() only.  Read it with get_nearest().  Synchronous."""
        k = int(k)
        self._check_cutoff_supported("query_radius_nearest")
        if exclude_self and not self.same_points:
            raise ValueError("exclude_self needs same_points=True")
        if k + bool(exclude_self) > NEAREST_MAX_K:
            raise NotImplementedError(f"MI355XProduct.query_radius_nearest doesn't support k = {k} > {NEAREST_MAX_K - bool(exclude_self)}"
                                      + (" with exclude_self" if exclude_self else "") + ".")
        self._nearest = self._ctx.radius_nearest(radius, k, exclude_self)
        self._cutoff_info = self._ctx.cutoff_info()

    def get_radius_count(self):
        """(N,) int64, -1 for a target with a NaN coordinate: the result of the last query_radius_count()."""
        return self._radius_count

    # -- bookkeeping ---------------------------------------------------------------
    def set_query_arguments(self, **kwargs):
        for key, value in kwargs.items():
            self._ctx.set_option(key, value)

    def get_memory_usage(self):
        """Device kB held by the context (the RSS of the reference says nothing here)."""
        return 0.0 if self._ctx is None else self._ctx.device_bytes / 1024

    # HIP-event timings of the last query() (device side) and the source slice this rank owns
    @property
    def device_kernel_ms(self):
        return self._ctx.last_kernel_ms

    @property
    def device_total_ms(self):
        return self._ctx.last_total_ms

    @property
    def device_kernel(self):
        return self._ctx.last_kernel_name

    @property
    def shard(self):
        return self._shard

    def get_additional(self):
        if self._ctx is None:
            return {}
        extra = {
            "device_kernel_ms": self._ctx.last_kernel_ms,
            "device_total_ms": self._ctx.last_total_ms,
            "device_kernel": self._ctx.last_kernel_name,
            "n_gpus": 1 if self.comm is None else self.comm.world,
            "device_bytes": self._ctx.device_bytes,
            # what RCCL itself saw, and the all-reduce's share of device_total_ms (0 on one GPU)
            "rccl_ranks": self._ctx.rccl_ranks,
            "allreduce_ms": self._ctx.last_allreduce_ms,
            # "" or why a faster form was not taken (too few points per grid cell, the radius rule, ...)
            "dispatch_note": self._ctx.last_dispatch_note or getattr(self, "_dot_note", ""),
        }
        if self._ctx.last_kernel_name.startswith("lowd_cutoff"):  # the cell-list plan of the last cutoff call
            extra.update({"cutoff_" + key: value for key, value in getattr(self, "_cutoff_info", {}).items()})
        return extra

    def done(self):
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None

    def __del__(self):
        # the runner calls done() only on the best instance (runner.py:174-176)
        try:
            self.done()
        except Exception:
            pass


# What MI355XSolver.log_determinant returns: the estimates with their standard errors (sample standard deviation over
# the probes / sqrt(probes)), the iterations every probe column took, and whether every column met the tolerance.
LogDeterminant = collections.namedtuple("LogDeterminant", "value stderr trace_inverse trace_inverse_stderr steps converged")
# What MI355XSolver.log_marginal_likelihood_gradient returns: the objective, its derivatives in the logarithm of the D
# per-axis length scales and in a uniform shift of the diagonal, each with the standard error of its trace estimate.
MarginalLikelihoodGradient = collections.namedtuple(
    "MarginalLikelihoodGradient",
    "value value_stderr d_log_lengthscale d_log_lengthscale_stderr d_ridge d_ridge_stderr converged")


def _rademacher_probes(M, probes, seed):
    """The +-1 probe columns of the trace estimates: a function of (M, probes, seed) alone, so every rank of a sharded
    solver draws the same ones."""
    return np.where(np.random.RandomState(seed).rand(M, probes) < 0.5, -1.0, 1.0)


def _precond_probes(M, rank, probes, seed):
    """The Rademacher pair (g (M, probes), h (rank, probes)) of the preconditioned quadrature, z = L h + D^1/2 g: a function
    of (M, rank, probes, seed) alone, so every rank of a sharded solver draws the same ones."""
    signs = np.where(np.random.RandomState(seed).rand(M + rank, probes) < 0.5, -1.0, 1.0)
    return np.ascontiguousarray(signs[:M]), np.ascontiguousarray(signs[M:])


def _log_likelihood(a, b, logdet, M):
    """-1/2 sum_e a_e' b_e - E/2 log det A - E M / 2 log 2 pi with b = A^-1 a (M, E)."""
    E = a.shape[1]
    return -0.5 * float(np.sum(a * b)) - 0.5 * E * logdet - 0.5 * E * M * np.log(2.0 * np.pi)


def assemble_likelihood_gradient(a, alpha, x, h_z, h_alpha, logquad, invquad, converged=True):
    """The host side of MI355XSolver.log_marginal_likelihood_gradient, in float64 and without a device: from the data a
    (M, E), alpha = A^-1 a (M, E), the probes' solves x_p = A^-1 z_p (M, P), the products h_z[:, p, d] = (d_d A) z_p
    (M, P, D) and h_alpha[:, e, d] = (d_d A) alpha_e (M, E, D) with d_d A = dA / d log l_d, and the per-probe quadratures
    logquad_p = z_p' log(A) z_p, invquad_p = z_p' A^-1 z_p (P):
        tr(A^-1 d_d A) ~ 1/P sum_p x_p' (d_d A) z_p              quad_d = sum_e alpha_e' (d_d A) alpha_e
        dL/d log l_d  = 1/2 quad_d - E/2 tr(A^-1 d_d A)           dL/d ridge = 1/2 sum_e alpha_e' alpha_e - E/2 tr A^-1
    Standard errors: E/2 x the sample standard deviation of the per-probe terms / sqrt(P)."""
    a, alpha, x = (np.asarray(v, dtype=np.float64) for v in (a, alpha, x))
    h_z, h_alpha = np.asarray(h_z, dtype=np.float64), np.asarray(h_alpha, dtype=np.float64)
    logquad, invquad = np.asarray(logquad, dtype=np.float64), np.asarray(invquad, dtype=np.float64)
    M, E = a.shape
    P = x.shape[1]
    root = np.sqrt(P)
    terms = np.einsum("mp,mpd->pd", x, h_z)           # x_p' (d_d A) z_p
    quad = np.einsum("me,med->d", alpha, h_alpha)     # sum_e alpha_e' (d_d A) alpha_e
    return MarginalLikelihoodGradient(
        value=_log_likelihood(a, alpha, float(np.mean(logquad)), M),
        value_stderr=0.5 * E * float(np.std(logquad, ddof=1) / root),
        d_log_lengthscale=0.5 * quad - 0.5 * E * np.mean(terms, axis=0),
        d_log_lengthscale_stderr=0.5 * E * np.std(terms, axis=0, ddof=1) / root,
        d_ridge=0.5 * float(np.sum(alpha * alpha)) - 0.5 * E * float(np.mean(invquad)),
        d_ridge_stderr=0.5 * E * float(np.std(invquad, ddof=1) / root),
        converged=bool(converged))


class MI355XSolver(BaseSolver):
    """Solves K b = a with the HIP product as the operator: conjugate gradients for the positive
    definite Gaussian / exp(-r) / Matern matrices, MINRES for the symmetric indefinite inverse-distance
    matrix (zero diagonal, bruteforce.py:13-14).

    ``ridge`` (an extension: the reference's lstsq solves the bare system) regularises it: (K + ridge I) b = a with a
    float, (K + diag(ridge)) b = a with one value per point -- the nugget / noise / ``alpha`` of Kriging, Gaussian
    processes and kernel ridge regression.  Non-negative for the CG kernels, any sign for inverse-distance.  The
    residual, ``rtol`` and ``converged`` are then about the regularised system.

    ``preconditioner_rank`` (an extension, 0 = off): conjugate gradients preconditioned by a pivoted-Cholesky factor of
    that many columns plus the ridge (include/kmvp.h kmvp_set_solver_preconditioner); it needs ``ridge`` > 0 and changes
    the iteration count, not what ``rtol`` and ``converged`` mean.  log_determinant(), log_marginal_likelihood() and
    log_marginal_likelihood_gradient() use it only with ``preconditioned=True``."""

    def __init__(self, *, kernel, dimension, normalize_rows=False, precision=np.float64,
                 device=0, rtol=1e-6, maxit=10000, comm=None, refine=None, inner_rtol=1e-3, ridge=0.0,
                 preconditioner_rank=0, support_radius=None, cutoff_plan="host"):
        super().__init__(kernel=kernel, dimension=dimension, normalize_rows=normalize_rows,
                         precision=precision)
        if kernel not in SUPPORTED_KERNELS + WENDLAND_KERNELS:
            raise NotImplementedError(f"MI355XSolver doesn't support kernel {kernel}.")
        # the Wendland solve's cell-list plan: built on the host (default) or on the device, same plan and same bits
        self._cutoff_plan = _cutoff_plan_code(cutoff_plan)
        # kernel="wendland-c2" / "wendland-c4" (an extension): the sparse operator of kmvp_wendland_<c>_cg_solve, O(M x
        # neighbours) per iteration; support_radius is the R of t = |x - y| / R
        self._wendland = kernel in WENDLAND_KERNELS
        if self._wendland:
            if support_radius is None or not (np.isfinite(support_radius) and support_radius > 0):
                raise ValueError(f"MI355XSolver(kernel={kernel!r}) needs support_radius, a finite number > 0")
            what = ("refine" if refine else "comm (a sharded operator)" if comm is not None else
                    "preconditioner_rank > 0 (the preconditioner knows no Wendland kernel)" if int(preconditioner_rank) > 0 else None)
            if what:
                raise NotImplementedError(f"MI355XSolver doesn't support kernel {kernel} with {what}.")
        elif support_radius is not None:
            raise ValueError(f"support_radius is for the Wendland kernels only, not for kernel {kernel}")
        self.support_radius = None if support_radius is None else float(support_radius)
        # refine="float32" (float64 solves only, an extension: the reference has one dense lstsq): mixed-precision
        # iterative refinement -- the residual a - K x is formed with the FLOAT64 operator, the correction K d = r is
        # solved to `inner_rtol` by CG on the FLOAT32 operator (the matrix-core cell form: ~10x cheaper per product),
        # x += d, until the float64 residual meets rtol.  The answer is judged exactly like the plain float64 solve.
        if refine not in (None, "float32"):
            raise ValueError("refine must be None or 'float32'")
        if refine and (np.dtype(precision) != np.float64 or kernel == "inverse-distance" or comm is not None):
            raise NotImplementedError("refine='float32' is for single-GPU float64 CG solves (gaussian, absolute-exponential, exp-dot)")
        self.refine = refine
        self.inner_rtol = float(inner_rtol)
        self._ctx32 = None
        self.outer_iterations = 0
        self.comm = comm  # sharding.Communicator: operator sharded over the sources, vectors replicated
        self._dtype_code, self._host_dtype = _lib.dtype_code(precision)
        if self._dtype_code == _lib.KMVP_BF16:
            raise NotImplementedError("MI355XSolver needs float16, float32 or float64")
        self._round = _lib.input_rounding(precision)  # float16: rounded inputs, float32 operator (scipy promotes too)
        self.device = device
        self.rtol = rtol
        self.maxit = maxit
        self._ctx = None
        self.iterations = 0
        self.residual = float("nan")
        self.converged = False
        self._dot = kernel == "exp-dot"  # K = D G D with D = diag(exp(|x|^2/2)), G the Gaussian matrix of the points / sqrt(2)
        self._device_kernel_fn = "gaussian" if self._dot else kernel
        self.method = "minres" if kernel == "inverse-distance" else "cg"
        self._base_name = (f"MI355XSolver({_precision_name(precision)}, {self.method}, rtol={rtol:g}" if not refine else
                           f"MI355XSolver({_precision_name(precision)}, {self.method} + refinement on {refine}, rtol={rtol:g}")
        self._diag_in_ctx = False  # whether the contexts hold a diagonal right now (set_points clears it)
        self._set_ridge(ridge)
        self._precond_in_ctx = 0   # the rank the context holds right now (set_points clears it)
        self._set_preconditioner_rank(preconditioner_rank)
        self._check_preconditioner_ridge()

    def _set_preconditioner_rank(self, rank):
        """Validates and stores ``preconditioner_rank``; it reaches the library at the next query()."""
        rank = int(rank)
        if rank < 0:
            raise ValueError("preconditioner_rank must be >= 0")
        if rank > 0 and (self.method != "cg" or self._dot or self.refine or self._wendland):
            what = "refine" if self.refine else f"kernel {self.kernel}"
            raise NotImplementedError(f"MI355XSolver(preconditioner_rank > 0) doesn't support {what}.")
        self.preconditioner_rank = rank
        self._update_name()

    def _check_preconditioner_ridge(self):
        if self.preconditioner_rank > 0 and isinstance(self.ridge, float) and self.ridge == 0.0:
            raise ValueError("preconditioner_rank > 0 needs ridge > 0 (the preconditioner L L' + ridge is positive definite "
                             "only then)")

    def _set_ridge(self, ridge):
        """Validates and stores ``ridge`` (a float, or one value per point); it reaches the library at the next query()."""
        try:
            r = np.array(ridge, dtype=np.float64)
        except (TypeError, ValueError) as e:
            raise ValueError(f"ridge must be a number or an array of one value per point: {e}") from None
        if r.ndim > 1 or (r.ndim == 1 and r.size == 0):
            raise ValueError(f"ridge has shape {r.shape}: pass a number or a one-dimensional array of one value per point")
        if not np.isfinite(r).all():
            raise ValueError("ridge must be finite")
        if self.method == "cg" and (r < 0).any():
            raise ValueError(f"ridge must be non-negative for kernel {self.kernel} (conjugate gradients needs a positive "
                             "definite system); only inverse-distance (MINRES) takes a negative shift")
        if r.ndim == 1 and getattr(self, "M", None) is not None and r.size != self.M:
            raise ValueError(f"ridge has {r.size} values, the point cloud has {self.M} points")
        self.ridge = float(r) if r.ndim == 0 else r
        self._diag_dirty = True
        self._update_name()

    def _update_name(self):
        # (the name moves only when a ridge or a preconditioner is set: result files of runs without them keep theirs)
        if isinstance(self.ridge, float):
            name = self._base_name + (f", ridge={self.ridge:g}" if self.ridge != 0.0 else "")
        else:
            name = self._base_name + f", ridge=per-point up to {float(np.max(self.ridge)):g}"
        rank = getattr(self, "preconditioner_rank", 0)
        self.name = name + (f", preconditioner_rank={rank})" if rank else ")")

    def _library_diagonal(self):
        """(d or None, ridge) as kmvp_set_solver_diagonal takes them.  exp-dot: the library iterates on G z = D^-1 a
        (z = D b, D = diag(exp(|x|^2/2))), where (K + L) b = a reads (G + D^-1 L D^-1) z = D^-1 a: it is handed the
        per-point vector l_i exp(-|x_i|^2) = l_i exp(-2 hx_i)."""
        vector = not isinstance(self.ridge, float)
        if not vector and self.ridge == 0.0:
            return None, 0.0
        if self._dot:
            return np.ascontiguousarray(self.ridge * np.exp(-2.0 * self._hx), dtype=np.float64), 0.0
        return (self.ridge, 0.0) if vector else (None, self.ridge)

    def _apply_diagonal(self):
        """Hands the diagonal to the contexts when it changed since the last query() (or the points did)."""
        if not self._diag_dirty:
            return
        d, ridge = self._library_diagonal()
        on = d is not None or ridge != 0.0
        if on or self._diag_in_ctx:
            for ctx in (self._ctx, self._ctx32):
                if ctx is not None:
                    ctx.set_solver_diagonal(d, ridge)
        self._diag_in_ctx = on
        # what the host-side residuals (refinement, exp-dot verdict) multiply the iterate by
        self._host_diag = None if not on else (ridge if d is None else d.reshape(-1, 1))
        self._diag_dirty = False

    def _diag_term(self, x):
        """The diagonal's share of A x on the host, as the library applies it (0 without a ridge)."""
        return 0.0 if self._host_diag is None else self._host_diag * x

    def _cast(self, a):
        if self._round is not None:
            a = np.asarray(a, dtype=self._round)
        return np.ascontiguousarray(a, dtype=self._host_dtype)

    def prepare_data(self, *, source_points):
        self._prepare_data(source_points)
        if self.refine:
            # the same points (after the exp-dot scaling) as float32 in a second context: the inner operator
            if self._ctx32 is None:
                self._ctx32 = _lib.Context(self.device)
            self._ctx32.set_points(np.ascontiguousarray(self._y_device, dtype=np.float32), None, _lib.KMVP_F32)

    def _prepare_data(self, source_points):
        if self._dot:
            ys = np.asarray(self._cast(source_points), dtype=np.float64)
            source_points = ys * SQRT_HALF
            self._hx = _sq_norms_on_device(self._cast(source_points), False)
        y = self._cast(source_points)
        self._y_device = y
        self.M, self.D = y.shape
        if not isinstance(self.ridge, float) and self.ridge.size != self.M:
            raise ValueError(f"ridge has {self.ridge.size} values, the point cloud has {self.M} points")
        self._diag_in_ctx, self._diag_dirty = False, True  # kmvp_set_points clears the library's diagonal
        self._precond_in_ctx = 0                            # and its preconditioner
        if self._ctx is None:
            self._ctx = _lib.Context(self.device)
            if self._cutoff_plan:
                self._ctx.set_option("cutoff_plan", self._cutoff_plan)
        world = 1 if self.comm is None else self.comm.world
        if world > 1:
            # every rank iterates on the full (replicated) Krylov vectors; the operator
            # is sharded over the sources and summed by the product's own all-reduce
            self._shard = sharding.shard_range(self.M, self.comm.rank, world)
            lo, hi = self._shard
            # (the sources keep the caller's order here: a rank's signal is a slice of the replicated Krylov vector)
            self.comm.attach(self._ctx)
            self._ctx.set_option("same_points_global", 1)
            self._ctx.set_points(np.ascontiguousarray(y[lo:hi]), y, self._dtype_code, j_offset=lo, M_total=self.M)
        else:
            self._shard = (0, self.M)
            self._ctx.set_points(y, None, self._dtype_code)

    def fit(self):
        """Nothing to factorise; the cell order of the float64 Gaussian operator is built here (kmvp_fit)."""
        self._ctx.fit(self._device_kernel_fn)
        if self._ctx32 is not None:
            self._ctx32.fit(self._device_kernel_fn)

    def prepare_query(self, *, target_signal):
        if self._dot:  # G (D b) = D^-1 a
            target_signal = np.asarray(target_signal, dtype=np.float64).reshape(self.M, -1) * np.exp(-self._hx).reshape(-1, 1)
        a = self._cast(target_signal)
        self._a = a.reshape(-1, 1) if a.ndim == 1 else a
        if self._a.ndim != 2 or self._a.shape[0] != self.M:
            raise ValueError(f"target_signal has shape {a.shape}, expected ({self.M}, E)")

    def set_query_arguments(self, rtol=None, maxit=None, ridge=None, preconditioner_rank=None):
        if rtol is not None:
            self.rtol = rtol
        if maxit is not None:
            self.maxit = maxit
        before = (self.ridge, self.preconditioner_rank)
        try:
            if ridge is not None:
                self._set_ridge(ridge)  # takes effect at the next query()
            if preconditioner_rank is not None:
                self._set_preconditioner_rank(preconditioner_rank)  # likewise
            self._check_preconditioner_ridge()
        except Exception:  # a refused pair leaves the previous one
            self._set_ridge(before[0])
            self._set_preconditioner_rank(before[1])
            raise

    def _apply_preconditioner(self):
        """Hands the rank to the context when it differs from what the context holds."""
        self._check_preconditioner_ridge()
        if self.preconditioner_rank != self._precond_in_ctx:
            self._ctx.set_solver_preconditioner(self.preconditioner_rank)
            self._precond_in_ctx = self.preconditioner_rank

    def query(self):
        self._apply_diagonal()
        self._apply_preconditioner()
        if self.refine:
            self._query_refined()
        else:
            extra = dict(support_radius=self.support_radius) if self._wendland else {}
            self.res, self.iterations, self.residual, self.converged = self._ctx.cg_solve(
                self._device_kernel_fn, self._a, self.rtol, self.maxit, **extra)
        if self._dot:
            # The iteration ran on the SCALED system G z = D^-1 a (z = D b, D = diag(exp(|x|^2/2))); where D varies a lot
            # its residual says little about K b = a.  The verdict is therefore taken on the unscaled system, from one
            # more product:  a - K b = D (D^-1 a - G z); with a ridge L:  a - K b - L b = D (D^-1 a - G z - D^-2 L z).
            z = np.ascontiguousarray(self.res, dtype=self._host_dtype)
            self._ctx.set_signal(z)
            self._ctx.run(self._device_kernel_fn, False)
            r_scaled = np.asarray(self._a, dtype=np.float64) - (self._ctx.get_result(self.M, z.shape[1]) + self._diag_term(self.res))
            with np.errstate(over="ignore", invalid="ignore"):
                d = np.exp(self._hx).reshape(-1, 1)
                num = np.linalg.norm(d * r_scaled, axis=0)
                den = np.linalg.norm(d * np.asarray(self._a, dtype=np.float64), axis=0)
                den[den == 0] = 1.0
                self.scaled_residual = self.residual
                self.residual = float(np.max(num / den))
            self.converged = bool(np.isfinite(self.residual) and self.residual <= 1.5 * self.rtol)
            self.res = self.res * np.exp(-self._hx).reshape(-1, 1)  # b = D^-1 (D b)

    def _query_refined(self):
        """Mixed-precision iterative refinement (see __init__).  Every outer step: float64 residual (one product of
        the float64 context), float32 CG on the scaled residual, float64 update.  With a ridge the inner context
        iterates on the same regularised operator and the float64 residual is a - (K x + (ridge + d) x)."""
        a = np.asarray(self._a, dtype=np.float64)
        anorm = np.linalg.norm(a, axis=0)
        anorm[anorm == 0] = 1.0
        x = np.zeros_like(a)
        r = a.copy()
        self.iterations, self.outer_iterations, self.converged = 0, 0, False
        rel = float(np.max(np.linalg.norm(r, axis=0) / anorm))
        best = rel
        # why the outer loop ended (get_additional "refinement_stop_reason"): tolerance | stagnation | maxit |
        # outer-limit | non-finite; with the last inner solve's own verdict beside it, so that a stalled refinement
        # (inner solve converged, outer residual stuck) can be told from an exhausted iteration budget
        self.stop_reason, self.inner_residual, self.inner_converged = "outer-limit", float("nan"), None
        for _ in range(40):
            if rel <= self.rtol:
                self.stop_reason = "tolerance"
                break
            if self.iterations >= self.maxit:
                self.stop_reason = "maxit"
                break
            scale = np.max(np.abs(r), axis=0)
            scale[scale == 0] = 1.0  # (a power-of-two free scaling is not needed: float32 has the range, this keeps it centred)
            d, iters, inner_res, inner_ok = self._ctx32.cg_solve(
                self._device_kernel_fn, np.ascontiguousarray(r / scale, dtype=np.float32), self.inner_rtol,
                max(1, self.maxit - self.iterations))
            self.iterations += iters
            self.outer_iterations += 1
            self.inner_residual, self.inner_converged = float(inner_res), bool(inner_ok)
            x_new = x + d * scale
            self._ctx.set_signal(x_new)
            self._ctx.run(self._device_kernel_fn, False)
            r_new = a - (self._ctx.get_result(self.M, a.shape[1]) + self._diag_term(x_new))
            rel_new = float(np.max(np.linalg.norm(r_new, axis=0) / anorm))
            if not np.isfinite(rel_new):
                self.stop_reason = "non-finite"
                break
            if rel_new > 0.9 * best:
                # the float32 correction did not help (inner tolerance beyond what a float32 operator can reach on
                # this matrix): keep the last good iterate and say so through `converged`
                self.stop_reason = "stagnation"
                break
            x, r, rel = x_new, r_new, rel_new
            best = rel
        else:
            if rel <= self.rtol:
                self.stop_reason = "tolerance"
        self.res, self.residual = x, rel
        self.converged = bool(np.isfinite(rel) and rel <= 1.5 * self.rtol)

    def _precond_quadrature(self, probes, seed, rtol, maxit, **want):
        """The preconditioned quadrature on the probes of (M, preconditioner_rank, probes, seed)."""
        if self.preconditioner_rank < 1:
            raise ValueError("preconditioned=True needs preconditioner_rank > 0")
        g, h = _precond_probes(self.M, self.preconditioner_rank, probes, seed)
        self._apply_diagonal()
        self._apply_preconditioner()
        return self._ctx.lanczos_quadrature_precond(self._device_kernel_fn, g, h, rtol, maxit, **want)

    def log_determinant(self, probes=32, seed=0, rtol=None, maxit=None, preconditioned=False):
        """log det A and tr A^-1 of A = K + ridge (the matrix query() solves with), without the matrix: stochastic Lanczos
        quadrature on ``probes`` Rademacher columns (include/kmvp.h kmvp_<kernel>_lanczos_quadrature), after
        prepare_data().  ``value`` is the mean of the per-probe z' log(A) z and ``stderr`` their sample standard
        deviation / sqrt(probes) -- the statistical error, which more probes reduce and a tighter ``rtol`` (default: the
        solver's) does not; ``trace_inverse`` likewise from z' A^-1 z.  The probes depend on (M, probes, seed) alone, so
        every rank of a sharded solver draws the same ones and returns the same bits.
        ``preconditioned=True`` (needs ``preconditioner_rank`` > 0): log det A = log det P + tr log M with P the
        pivoted-Cholesky preconditioner and M = P^-1/2 A P^-1/2 (include/kmvp.h kmvp_<kernel>_lanczos_quadrature_precond).
        ``value`` is the exact log det P plus the mean of the per-probe w' log(M) w, ``stderr`` the latter's alone;
        ``trace_inverse`` from (P^-1 z)' A^-1 z.  Fewer iterations and a smaller standard error than without."""
        what = (f"kernel {self.kernel}" if self.method != "cg" or self._dot or self._wendland else "refine" if self.refine else
                "normalize_rows" if self.normalize_rows else None)
        if what:
            raise NotImplementedError(f"MI355XSolver.log_determinant doesn't support {what}.")
        if preconditioned and self.preconditioner_rank < 1:
            raise ValueError("log_determinant(preconditioned=True) needs preconditioner_rank > 0")
        if self._ctx is None:
            raise RuntimeError("log_determinant() needs prepare_data() first")
        probes = int(probes)
        if probes < 2:
            raise ValueError("log_determinant needs at least 2 probes (the standard error is a sample deviation)")
        rtol, maxit = self.rtol if rtol is None else rtol, self.maxit if maxit is None else maxit
        if preconditioned:
            out = self._precond_quadrature(probes, seed, rtol, maxit)
        else:
            z = _rademacher_probes(self.M, probes, seed)
            self._apply_diagonal()
            out = self._ctx.lanczos_quadrature(self._device_kernel_fn, np.ascontiguousarray(z, dtype=self._host_dtype), rtol, maxit)
        root = np.sqrt(probes)
        value = float(np.mean(out["logquad"]))
        if preconditioned:
            value = float(out["logdet_p"] + value)  # log det P is exact: the standard error is tr log M's alone
        return LogDeterminant(value=value, stderr=float(np.std(out["logquad"], ddof=1) / root),
                              trace_inverse=float(np.mean(out["invquad"])),
                              trace_inverse_stderr=float(np.std(out["invquad"], ddof=1) / root),
                              steps=out["steps"], converged=bool(out["converged"]))

    def log_marginal_likelihood(self, probes=32, seed=0, preconditioned=False):
        """log p(a) of a zero-mean Gaussian process with covariance A = K + ridge, summed over the E columns of the last
        query()'s target_signal a (b = A^-1 a is its result):
            -1/2 sum_e a_e' b_e  -  E/2 log det A  -  E M / 2 log 2 pi
        with log det A from log_determinant(probes, seed).  Returns (value, stderr); the standard error is the
        log-determinant's share, E/2 times its own (the quadratic term is exact to the solve's rtol).
        ``preconditioned``: as log_determinant's."""
        if getattr(self, "res", None) is None or getattr(self, "_a", None) is None:
            raise RuntimeError("log_marginal_likelihood() needs prepare_query() and query() first")
        if not self.converged:
            raise RuntimeError(f"log_marginal_likelihood(): the last solve did not converge (relative residual {self.residual:g})")
        logdet = self.log_determinant(probes=probes, seed=seed, preconditioned=True) if preconditioned else \
            self.log_determinant(probes=probes, seed=seed)
        if not logdet.converged:
            raise RuntimeError("log_marginal_likelihood(): the Lanczos quadrature did not converge")
        a = np.asarray(self._a, dtype=np.float64)
        return _log_likelihood(a, self.res, logdet.value, self.M), 0.5 * a.shape[1] * logdet.stderr

    def log_marginal_likelihood_gradient(self, probes=32, seed=0, preconditioned=False):
        """log_marginal_likelihood(probes, seed) with its gradient in the hyperparameters, after query(): a namedtuple
        (value, value_stderr, d_log_lengthscale (D,), d_log_lengthscale_stderr (D,), d_ridge, d_ridge_stderr, converged).
        ``d_log_lengthscale[d]`` is dL / d log l_d for the covariance k(x / l, y / l) at l = 1: the length scales are the
        caller's scaling of the points, one per axis (ARD); the derivative in ONE isotropic length scale is
        ``d_log_lengthscale.sum()``.  ``d_ridge`` is the derivative in a uniform shift of the diagonal, also when
        ``ridge`` is one value per point.  With alpha = A^-1 a the last query()'s result:
            dL/d log l_d = 1/2 sum_e alpha_e' (d_d A) alpha_e - E/2 tr(A^-1 d_d A)
            dL/d ridge   = 1/2 sum_e alpha_e' alpha_e         - E/2 tr A^-1
        The traces are estimated on the Rademacher probes z_p of log_determinant(probes, seed), from ONE Lanczos
        quadrature that also returns x_p = A^-1 z_p: tr(A^-1 d_d A) ~ mean_p x_p' (d_d A) z_p, and (d_d A) [z | alpha]
        from kmvp_<kernel>_dscale in blocks of four columns.  ``value`` is log_marginal_likelihood(probes, seed)'s, bit for
        bit; the standard errors are the trace estimates' share (E/2 x sample deviation / sqrt(probes)), the quadratic
        terms are exact to the solve's rtol.  Every rank of a sharded solver returns the same bits.
        ``preconditioned=True`` (needs ``preconditioner_rank`` > 0): the probes are z = L h + D^1/2 g with covariance P, and
        with pz = P^-1 z, E pz' B x = tr(B A^-1): tr(A^-1 d_d A) ~ mean_p x_p' (d_d A) pz_p, tr A^-1 ~ mean_p pz_p' x_p,
        (d_d A) [pz | alpha] from the same product, and log det A = log det P + mean_p w_p' log(M) w_p."""
        pieces = self._likelihood_gradient_pieces(probes, seed, preconditioned)
        return assemble_likelihood_gradient(self._a, self.res, **pieces)

    def _likelihood_gradient_pieces(self, probes, seed, preconditioned=False):
        """The device's share of log_marginal_likelihood_gradient(): what assemble_likelihood_gradient() takes beside a and
        alpha, as a dict."""
        what = (f"kernel {self.kernel}" if self.method != "cg" or self._dot or self._wendland else "refine" if self.refine else
                "normalize_rows" if self.normalize_rows else None)
        if what:
            raise NotImplementedError(f"MI355XSolver.log_marginal_likelihood_gradient doesn't support {what}.")
        if getattr(self, "res", None) is None or getattr(self, "_a", None) is None:
            raise RuntimeError("log_marginal_likelihood_gradient() needs prepare_query() and query() first")
        if self.D > GRADIENT_MAX_D:
            raise NotImplementedError(f"MI355XSolver.log_marginal_likelihood_gradient doesn't support D = {self.D} > {GRADIENT_MAX_D}.")
        if not self.converged:
            raise RuntimeError("log_marginal_likelihood_gradient(): the last solve did not converge "
                               f"(relative residual {self.residual:g})")
        probes = int(probes)
        if probes < 2:
            raise ValueError("log_marginal_likelihood_gradient needs at least 2 probes (the standard error is a sample deviation)")
        if preconditioned:
            # the signal of the dscale product is pz = P^-1 z (d_d K is symmetric: x' (d_d K) pz = pz' (d_d K) x), and the
            # exact log det P joins every probe's logquad, so the mean is log det A and the deviation tr log M's alone
            out = self._precond_quadrature(probes, seed, self.rtol, self.maxit, want_x=True, want_pz=True)
            z = np.ascontiguousarray(out["pz"], dtype=self._host_dtype)
            out["logquad"] = out["logdet_p"] + out["logquad"]
        else:
            z = np.ascontiguousarray(_rademacher_probes(self.M, probes, seed), dtype=self._host_dtype)  # +-1: exact
            self._apply_diagonal()
            out = self._ctx.lanczos_quadrature(self._device_kernel_fn, z, self.rtol, self.maxit, want_x=True)
        if not out["converged"]:
            raise RuntimeError("log_marginal_likelihood_gradient(): the Lanczos quadrature did not converge")
        # (d_d A) [z_1 .. z_P, alpha_1 .. alpha_E]: the operator's own context, a rank's signal its slice of the replicated
        # columns (as the solver's operator), summed over the ranks by the product's all-reduce
        cols = np.concatenate([z, np.asarray(self.res, dtype=self._host_dtype)], axis=1)
        lo, hi = self._shard
        h = np.empty((self.M, cols.shape[1], self.D), dtype=np.float64)
        for c0 in range(0, cols.shape[1], GRADIENT_MAX_E):
            block = np.ascontiguousarray(cols[lo:hi, c0:c0 + GRADIENT_MAX_E])
            self._ctx.set_signal(block)
            self._ctx.run_dscale(self._device_kernel_fn)
            h[:, c0:c0 + block.shape[1], :] = self._ctx.get_result(self.M, block.shape[1] * self.D).reshape(self.M, -1, self.D)
        return dict(x=out["x"], h_z=h[:, :probes], h_alpha=h[:, probes:], logquad=out["logquad"], invquad=out["invquad"])

    def get_memory_usage(self):
        return 0.0 if self._ctx is None else self._ctx.device_bytes / 1024

    def get_additional(self):
        # (with a ridge the residual keys describe the regularised system (K + ridge) b = a)
        extra = {"cg_iterations": self.iterations, "cg_relative_residual": self.residual,
                 "cg_converged": bool(self.converged), "n_gpus": 1 if self.comm is None else self.comm.world}
        if not isinstance(self.ridge, float) or self.ridge != 0.0:  # like the name: only when one is set
            extra["ridge"] = float(np.max(self.ridge))
        if self.preconditioner_rank > 0 and self._ctx is not None:  # like the ridge: only when one is set
            extra["preconditioner_rank"] = self._ctx.last_preconditioner_rank  # as built
            extra["preconditioner_ms"] = self._ctx.last_preconditioner_ms
        if self._ctx is not None:
            extra["device_kernel"] = self._ctx.last_kernel_name  # the operator's pair-loop kernel
            extra["rccl_ranks"] = self._ctx.rccl_ranks
            if self._wendland and self._ctx.last_kernel_name.startswith("lowd_cutoff"):
                extra["cutoff_built_on"] = self._ctx.cutoff_info()["built_on"]  # the side that built the solve's plan
        if self._dot and hasattr(self, "scaled_residual"):
            extra["cg_scaled_system_residual"] = self.scaled_residual  # of G (D b) = D^-1 a, what the iteration saw
        if self.refine and self._ctx32 is not None:
            extra["refinement_steps"] = self.outer_iterations
            extra["inner_device_kernel"] = self._ctx32.last_kernel_name
            extra["refinement_stop_reason"] = getattr(self, "stop_reason", "")
            extra["refinement_last_inner_residual"] = getattr(self, "inner_residual", float("nan"))
            extra["refinement_last_inner_converged"] = bool(getattr(self, "inner_converged", False))
        return extra

    def done(self):
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None
        if getattr(self, "_ctx32", None) is not None:
            self._ctx32.close()
            self._ctx32 = None

    def __del__(self):
        try:
            self.done()
        except Exception:
            pass


SINKHORN_KERNELS = ("gaussian", "absolute-exponential")  # the log-sum-exp's kernels: cost |x - y|^2 and |x - y|
SINKHORN_MASS_RTOL = 1e-6


class MI355XSinkhorn:
    """Entropic optimal transport between two weighted clouds on one MI355X: the Sinkhorn iteration in the log domain,
    resident on the device (include/kmvp.h kmvp_<kernel>_sinkhorn; the pair loop is lowd_lse_kernel).  An extension:
    the reference's plugin API has no such role, so the class is not registered in algos.yaml.

        minimise  <pi, C> + eps KL(pi | a x b)   over plans pi with marginals a (targets x) and b (sources y)
        C = |x - y|^2 (kernel="gaussian")  or  |x - y| (kernel="absolute-exponential")

    Same call order as MI355XSolver: prepare_data, fit, query, then get_potentials / dual_value / barycentric_map /
    get_additional, done.  The temperature is applied by scaling the points (by 1 / sqrt(eps) or 1 / eps); the library
    works on the dimensionless potentials u = f / eps, v = g / eps.  ``options``: device, segments, chunk, fast_sqdists
    (only None / False run: the difference form).

    Batched clouds: prepare_data(..., source_batches=, target_batches=) takes B + 1 offsets into the concatenated sources
    and targets, as MI355XProduct.prepare_data, and query() then solves one transport problem per batch in one
    device-resident solve (kmvp_<kernel>_sinkhorn_batched; the pair loop is lowd_batch_lse_kernel).  Weights are
    concatenated like the points and handled per batch (None: uniform within each batch; the masses are compared per
    batch); get_potentials() returns the concatenated (f, g), dual_value() one value per batch, get_additional() per-batch
    iterations, marginal_error and converged.  barycentric_map() is not built for batches."""

    def __init__(self, *, kernel, dimension, eps, precision=np.float32, tol=1e-6, maxit=1000, device=0, segments=0,
                 chunk=0, fast_sqdists=None):
        if kernel not in SINKHORN_KERNELS:
            raise NotImplementedError(f"MI355XSinkhorn doesn't support kernel {kernel}.")
        if not (np.isfinite(eps) and eps > 0):
            raise ValueError(f"eps must be a positive number, not {eps!r}")
        self.kernel, self.dimension, self.eps = kernel, int(dimension), float(eps)
        self.precision = precision
        self._dtype_code, self._host_dtype = _lib.dtype_code(precision)
        self.tol, self.maxit = float(tol), int(maxit)
        self.device = device
        self.fast_sqdists = fast_sqdists
        self._options = dict(segments=segments, chunk=chunk)
        # the points are multiplied by this before they are cast to the working precision
        self.scale = 1.0 / np.sqrt(self.eps) if kernel == "gaussian" else 1.0 / self.eps
        self._ctx = None
        self._batches = None
        self.u = self.v = None
        self.iterations, self.marginal_error, self.converged = 0, float("nan"), False
        self.name = f"MI355XSinkhorn({_precision_name(precision)}, eps={self.eps:g})"

    @staticmethod
    def _log_weights(w, n, what):
        if w is None:
            return np.full(n, 1.0 / n), None  # (the library's uniform default: log_w = NULL)
        w = np.asarray(w, dtype=np.float64).reshape(-1)
        if w.shape != (n,):
            raise ValueError(f"{what} has {w.size} entries for {n} points")
        if not np.all(w >= 0):  # (NaN fails this as well)
            raise ValueError(f"{what} must be non-negative")
        with np.errstate(divide="ignore"):
            return w, np.log(w)  # a weight of 0 is a point of mass 0: log weight -inf

    # -- untimed -------------------------------------------------------------------
    def prepare_data(self, *, source_points, target_points, same_points=False, source_weights=None, target_weights=None,
                     source_batches=None, target_batches=None):
        self.same_points = bool(same_points)
        if source_points is None or (target_points is None and not self.same_points):
            raise ValueError("source_points and target_points are both needed (target_points may be None only with "
                             "same_points=True)")
        y = np.ascontiguousarray(np.asarray(source_points, dtype=np.float64) * self.scale, dtype=self._host_dtype)
        if y.ndim != 2 or y.shape[1] != self.dimension:
            raise ValueError(f"source_points has shape {y.shape}, expected (M, {self.dimension})")
        self.M, self.D = y.shape
        if self.same_points:
            x = None
            self.N = self.M
        else:
            x = np.ascontiguousarray(np.asarray(target_points, dtype=np.float64) * self.scale, dtype=self._host_dtype)
            if x.ndim != 2 or x.shape[1] != self.D:
                raise ValueError(f"target_points has shape {x.shape}, expected (N, {self.D})")
            self.N = x.shape[0]
        self._batches = self._check_batches(source_batches, target_batches)
        self.b, self._log_b = self._log_weights(source_weights, self.M, "source_weights")
        self.a, self._log_a = self._log_weights(target_weights, self.N, "target_weights")
        if self._batches is None:
            ma, mb = float(np.sum(self.a)), float(np.sum(self.b))
            if not abs(ma - mb) <= SINKHORN_MASS_RTOL * max(ma, mb):
                raise ValueError(f"the total masses differ: target_weights sum to {ma!r}, source_weights to {mb!r}")
        else:
            yb, xb = self._batches
            for k in range(yb.size - 1):
                # the unbatched rule within every batch: uniform weights sum to one, given ones are compared
                if source_weights is None:
                    self.b[yb[k]:yb[k + 1]] = 1.0 / max(int(yb[k + 1] - yb[k]), 1)
                if target_weights is None:
                    self.a[xb[k]:xb[k + 1]] = 1.0 / max(int(xb[k + 1] - xb[k]), 1)
                ma, mb = float(np.sum(self.a[xb[k]:xb[k + 1]])), float(np.sum(self.b[yb[k]:yb[k + 1]]))
                if not abs(ma - mb) <= SINKHORN_MASS_RTOL * max(ma, mb):
                    raise ValueError(f"the total masses differ in batch {k}: target_weights sum to {ma!r}, source_weights to {mb!r}")
        self._y, self._x = y, (y if x is None else x)  # the scaled points as the device holds them
        if self._ctx is None:
            self._ctx = _lib.Context(self.device)
            for key, value in self._options.items():
                if value:
                    self._ctx.set_option(key, value)
            if self.fast_sqdists is not None:
                code = {"centred": 2, "cells": 3, "cells-valu": 4}.get(self.fast_sqdists, int(bool(self.fast_sqdists)))
                self._ctx.set_option("fast_sqdists", code)
        self._ctx.set_points(y, x, self._dtype_code)
        if self._batches is not None:
            self._ctx.set_batches(self._batches[0], None if self.same_points and target_batches is None else self._batches[1])
        self.u = self.v = None

    def _check_batches(self, source_batches, target_batches):
        """(source offsets, target offsets) of batched clouds, or None without batches; everything the host can decide is
        refused here, before any device call."""
        if source_batches is None and target_batches is None:
            return None
        if source_batches is None:
            raise ValueError("target_batches needs source_batches")
        if target_batches is None and not self.same_points:
            raise ValueError("target_batches=None needs same_points=True (the sources' offsets then serve both)")
        yb = _lib.batch_offsets(source_batches, "source_batches", self.M)
        xb = yb if target_batches is None else _lib.batch_offsets(target_batches, "target_batches", self.N)
        if xb.size != yb.size:
            raise ValueError(f"target_batches has {xb.size} offsets, source_batches {yb.size}: both hold B + 1")
        one_sided = np.nonzero((np.diff(yb) == 0) != (np.diff(xb) == 0))[0]
        if one_sided.size:
            raise ValueError(f"batch {int(one_sided[0])} has points on one side only")
        return yb, xb

    # -- timed ---------------------------------------------------------------------
    def fit(self):
        """Nothing to build ahead of the first solve: it packs both directions' layouts itself, once per prepare_data."""

    def query(self, warm_start=None):
        """Runs the iteration from f = warm_start (N values in the caller's units, e.g. get_potentials()[0] of a solve
        at a larger eps) or from zero.  Synchronous.  Not converged (maxit reached, or a non-finite potential) is a
        result, reported by get_additional()["converged"]; every other failure raises."""
        u0 = None if warm_start is None else np.asarray(warm_start, dtype=np.float64).reshape(-1) / self.eps
        if self._batches is not None:  # one solve per batch: iterations, marginal_error and converged hold B values
            self.u, self.v, self.iterations, self.marginal_error, status = self._ctx.sinkhorn_batched(
                self.kernel, self._log_a, self._log_b, self.tol, self.maxit, u0)
            self.converged = status == 1
            return
        self.u, self.v, self.iterations, self.marginal_error, self.converged = self._ctx.sinkhorn(
            self.kernel, self._log_a, self._log_b, self.tol, self.maxit, u0)

    def set_query_arguments(self, tol=None, maxit=None):
        if tol is not None:
            self.tol = float(tol)
        if maxit is not None:
            self.maxit = int(maxit)

    # -- results -------------------------------------------------------------------
    def _need_solution(self, method):
        if self.u is None:
            raise RuntimeError(f"MI355XSinkhorn.{method}: no solution yet -- call query() after prepare_data() first")

    def get_potentials(self):
        """(f, g) = eps (u, v): f on the N targets, g on the M sources; the plan is
        pi_ij = a_i b_j exp((f_i + g_j - C_ij) / eps)."""
        self._need_solution("get_potentials")
        return self.eps * self.u, self.eps * self.v

    def dual_value(self):
        """<a, f> + <b, g>: the dual objective at the returned potentials (the plan's mass term cancels when its
        marginals are met).  Batched clouds: an array of B values, one per batch."""
        f, g = self.get_potentials()
        if self._batches is not None:
            yb, xb = self._batches
            return np.array([np.dot(self.a[xb[k]:xb[k + 1]], f[xb[k]:xb[k + 1]]) + np.dot(self.b[yb[k]:yb[k + 1]], g[yb[k]:yb[k + 1]])
                             for k in range(yb.size - 1)], dtype=np.float64)
        return float(np.dot(self.a, f) + np.dot(self.b, g))

    def barycentric_map(self):
        """(N, D): sum_j pi_ij y_j / sum_j pi_ij in the caller's coordinates -- where the plan sends x_i on average.
        Gaussian only: G = grad_x L = -2 (x - barycentre) of the log-sum-exp with the signal v + log b
        (kmvp_gaussian_logsumexp_grad on the same context)."""
        if self._batches is not None:
            raise NotImplementedError("MI355XSinkhorn.barycentric_map is not built for batched clouds (the batched gradient of "
                                      "the log-sum-exp is not built).")
        if self.kernel != "gaussian":
            raise NotImplementedError("MI355XSinkhorn.barycentric_map is built for kernel='gaussian' only.")
        self._need_solution("barycentric_map")
        log_b = self._log_b if self._log_b is not None else np.full(self.M, -np.log(self.M))
        self._ctx.set_signal(np.ascontiguousarray((self.v + log_b).reshape(-1, 1), dtype=self._host_dtype))
        self._ctx.run_lse_grad("gaussian")
        grad = self._ctx.get_result(self.N, self.D)
        return np.ascontiguousarray((np.asarray(self._x, dtype=np.float64) + 0.5 * grad) / self.scale)

    def get_memory_usage(self):
        return 0.0 if self._ctx is None else self._ctx.device_bytes / 1024

    def get_additional(self):
        if self._batches is not None:
            extra = {"iterations": np.asarray(self.iterations), "marginal_error": np.asarray(self.marginal_error),
                     "converged": np.asarray(self.converged, dtype=bool)}
        else:
            extra = {"iterations": self.iterations, "marginal_error": self.marginal_error, "converged": bool(self.converged)}
        if self._ctx is not None:
            extra.update(device_kernel_ms=self._ctx.last_kernel_ms, device_total_ms=self._ctx.last_total_ms,
                         device_kernel=self._ctx.last_kernel_name, device_bytes=self._ctx.device_bytes)
        return extra

    def done(self):
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None

    def __del__(self):
        try:
            self.done()
        except Exception:
            pass


KMEANS_MAX_D = NEAREST_MAX_D
KMEANS_MAX_CLUSTERS = 65536
KMEANS_INITS = ("random", "k-means++")


class MI355XKMeans:
    """Lloyd's k-means on one MI355X, resident on the device (include/kmvp.h kmvp_kmeans; the pair loop is
    lowd_knn_kernel at K = 1, the centroid update a deterministic, atomics-free kernel of its own).  An extension: the
    reference's plugin API has no such role, so the class is not registered in algos.yaml.

        minimise  sum_i w_i |x_i - c_{l(i)}|^2   over n_clusters centroids c and the assignment l

    Call order: prepare_data, fit, query, then get_centroids / get_labels / get_cluster_weights / predict /
    get_additional, done.  ``tol`` is ABSOLUTE on sum_c |c_k - c_{k-1}|^2, the squared displacement of the centroids in
    one iteration, in the units of the points squared; tol = 0 (the default) stops at the fixed point, which Lloyd's
    iteration reaches exactly.  A cluster that no point of positive weight is assigned to keeps its position.

    Initialisation happens on the host, from ``seed`` (the library itself draws nothing):
      init="random"     n_clusters distinct points, drawn without replacement;
      init="k-means++"  D^2 sampling in numpy: every next centroid is a point drawn with probability proportional to its
                        weight times its squared distance to the nearest centroid chosen so far.  O(N * n_clusters) work
                        and n_clusters passes over the points ON THE HOST: meant for moderate n_clusters, not timed.
    query(init=array) takes explicit (n_clusters, D) centroids instead, which also serves as a warm start.
    ``options``: device, segments (the result does not depend on it)."""

    def __init__(self, *, n_clusters, dimension, precision=np.float32, tol=0.0, maxit=300, init="random", seed=0, device=0,
                 segments=0):
        if int(n_clusters) < 1:
            raise ValueError(f"n_clusters must be >= 1, not {n_clusters!r}")
        if init not in KMEANS_INITS:
            raise ValueError(f"init must be one of {KMEANS_INITS}, not {init!r}")
        if not float(tol) >= 0:
            raise ValueError(f"tol must be >= 0, not {tol!r}")
        self.n_clusters, self.dimension = int(n_clusters), int(dimension)
        self.precision = precision
        self._dtype_code, self._host_dtype = _lib.dtype_code(precision)
        self._round = _lib.input_rounding(precision)  # float16: rounded points, float32 arithmetic
        self.tol, self.maxit = float(tol), int(maxit)
        self.init, self.seed = init, seed
        self.device = device
        self._options = dict(segments=segments)
        self._ctx = self._predict_ctx = None
        self.centroids = self.labels = self.cluster_weights = None
        self.iterations, self.inertia, self.shift, self.converged = 0, float("nan"), float("nan"), False
        self.name = f"MI355XKMeans({_precision_name(precision)}, n_clusters={self.n_clusters})"

    def _as_device_points(self, points, what):
        p = np.asarray(points, dtype=np.float64)
        if p.ndim != 2 or p.shape[1] != self.dimension:
            raise ValueError(f"{what} has shape {p.shape}, expected (N, {self.dimension})")
        if self._round is not None:
            p = p.astype(self._round)
        return np.ascontiguousarray(p, dtype=self._host_dtype)

    def _new_context(self):
        ctx = _lib.Context(self.device)
        for key, value in self._options.items():
            if value:
                ctx.set_option(key, value)
        return ctx

    # -- untimed -------------------------------------------------------------------
    def prepare_data(self, *, points, weights=None):
        x = self._as_device_points(points, "points")
        self.N, self.D = x.shape
        if self.N < 1:
            raise ValueError("k-means needs at least one point")
        if weights is not None:
            weights = np.ascontiguousarray(np.asarray(weights, dtype=np.float64).reshape(-1))
            if weights.shape != (self.N,):
                raise ValueError(f"weights has {weights.size} entries for {self.N} points")
            if not (np.all(weights >= 0) and np.all(np.isfinite(weights))):  # (NaN fails the first)
                raise ValueError("weights must be non-negative and finite")
        self._x, self._w = x, weights  # the points as the device holds them
        if self._ctx is None:
            self._ctx = self._new_context()
        self._ctx.set_points(x, None, self._dtype_code)  # the cloud is its own target set: the points of kmvp_kmeans
        self.centroids = self.labels = self.cluster_weights = None

    def _initial_centroids(self):
        rs = np.random.RandomState(self.seed)
        x = np.asarray(self._x, dtype=np.float64)
        C = self.n_clusters
        if self.init == "random":
            if C > self.N:
                raise ValueError(f"init='random' draws {C} distinct points, and there are only {self.N}")
            return x[rs.choice(self.N, size=C, replace=False)]
        w = np.ones(self.N) if self._w is None else self._w
        if not np.sum(w) > 0:
            raise ValueError("init='k-means++' needs a point of positive weight")
        cent = np.empty((C, self.D))
        cent[0] = x[rs.choice(self.N, p=w / np.sum(w))]
        near = np.sum((x - cent[0]) ** 2, axis=1)
        for c in range(1, C):
            p = w * near
            total = float(np.sum(p))
            # every point of positive weight already coincides with a centroid: fall back to the weights themselves
            cent[c] = x[rs.choice(self.N, p=p / total if total > 0 else w / np.sum(w))]
            near = np.minimum(near, np.sum((x - cent[c]) ** 2, axis=1))
        return cent

    # -- timed ---------------------------------------------------------------------
    def fit(self):
        """Nothing to build ahead of the first solve: it packs the points' layout itself, once per prepare_data."""

    def query(self, init=None):
        """Runs Lloyd's iteration from ``init`` ((n_clusters, D) centroids: explicit initial centroids or a warm start,
        e.g. get_centroids() of an earlier solve) or from the constructor's init= rule.  Synchronous.  Not converged
        (maxit reached, or a point without a label / a non-finite inertia) is a result, reported by
        get_additional()["converged"]; every other failure raises."""
        if self._ctx is None:
            raise RuntimeError("MI355XKMeans.query() needs prepare_data() first")
        if init is None:
            c0 = self._initial_centroids()
        else:
            c0 = np.asarray(init, dtype=np.float64)
            if c0.shape != (self.n_clusters, self.D):
                raise ValueError(f"init has shape {c0.shape}, expected ({self.n_clusters}, {self.D})")
        (self.centroids, self.labels, self.cluster_weights, self.iterations, self.inertia, self.shift,
         self.converged) = self._ctx.kmeans(self.n_clusters, c0, self._w, self.tol, self.maxit)

    def set_query_arguments(self, tol=None, maxit=None):
        if tol is not None:
            self.tol = float(tol)
        if maxit is not None:
            self.maxit = int(maxit)

    # -- results -------------------------------------------------------------------
    def _need_solution(self, method):
        if self.centroids is None:
            raise RuntimeError(f"MI355XKMeans.{method}: no solution yet -- call query() after prepare_data() first")

    def get_centroids(self):
        """(n_clusters, D) float64: the weighted means of the points that carry each label."""
        self._need_solution("get_centroids")
        return self.centroids

    def get_labels(self):
        """(N,) int64: the cluster of every point (-1: a point without a qualifying centroid, e.g. a NaN coordinate)."""
        self._need_solution("get_labels")
        return self.labels

    def get_cluster_weights(self):
        """(n_clusters,) float64: the total weight of every cluster (the point count without weights)."""
        self._need_solution("get_cluster_weights")
        return self.cluster_weights

    def predict(self, points):
        """(M,) int64: the nearest final centroid of every row of ``points`` -- kmvp_nearest with K = 1 against the
        centroids rounded to the working precision, the rule the iteration itself assigns by (ties: the smaller index)."""
        self._need_solution("predict")
        x = self._as_device_points(points, "points")
        if self._predict_ctx is None:  # a context of its own: the solver's keeps the training points
            self._predict_ctx = self._new_context()
        self._predict_ctx.set_points(np.ascontiguousarray(self.centroids, dtype=self._host_dtype), x, self._dtype_code)
        idx, _ = self._predict_ctx.run_nearest(1, False)
        return np.ascontiguousarray(idx[:, 0])

    def get_memory_usage(self):
        """Device kB held by the contexts."""
        return sum(ctx.device_bytes for ctx in (self._ctx, self._predict_ctx) if ctx is not None) / 1024

    def get_additional(self):
        extra = {"iterations": self.iterations, "inertia": self.inertia, "shift": self.shift, "converged": bool(self.converged)}
        if self._ctx is not None:
            extra.update(device_kernel_ms=self._ctx.last_kernel_ms, device_total_ms=self._ctx.last_total_ms,
                         device_kernel=self._ctx.last_kernel_name, device_bytes=self._ctx.device_bytes)
        return extra

    def done(self):
        for ctx in (self._ctx, self._predict_ctx):
            if ctx is not None:
                ctx.close()
        self._ctx = self._predict_ctx = None

    def __del__(self):
        try:
            self.done()
        except Exception:
            pass


SPECTRAL_KERNELS = ("gaussian", "absolute-exponential", "matern-3/2", "matern-5/2")
SPECTRAL_OPERATORS = ("kernel", "centered", "normalized")
SPECTRAL_MAX_STEPS = 512  # csrc/kmvp_eigsh.hip EIG_MAX_STEPS: there is no restart


class MI355XSpectral:
    """The n_components largest eigenpairs of the kernel matrix on one MI355X, by a device-resident Lanczos process with
    full reorthogonalisation on the on-the-fly product (include/kmvp.h kmvp_<kernel>_eigsh).  An extension: the
    reference's plugin API has no such role, so the class is not registered in algos.yaml.

        operator="kernel"      A = K (+ ridge I, or + diag(ridge) with one value per point)
        operator="centered"    A = H K H, H = I - 1 1'/N: kernel PCA (sklearn.decomposition.KernelPCA)
        operator="normalized"  A = D^-1/2 K D^-1/2, D = diag(K 1): spectral embedding (Ng, Jordan and Weiss)

    Call order: prepare_data, fit, query, then get_eigenvalues / get_eigenvectors / get_residuals / get_degree /
    get_embedding / transform / get_additional, done.  ``tol`` bounds |A x - theta x| / (theta_1 |x|) of every pair
    (default: 1e-10 in float64, 1e-4 in float32 and float16); ``maxit`` caps the Lanczos steps (default and most:
    min(N, 512) -- there is no restart).  The start vector is a normal draw from ``seed`` on the host unless query(v0=)
    passes one: the library itself draws nothing.  Not converged is a result (get_additional()["converged"]); every
    other failure raises.  A single start vector finds one copy of a multiple eigenvalue."""

    def __init__(self, *, kernel, dimension, precision=np.float64, n_components, operator="kernel", tol=None, maxit=None,
                 seed=0, ridge=None, device=0):
        if kernel not in SPECTRAL_KERNELS:
            raise NotImplementedError(f"MI355XSpectral doesn't support kernel {kernel}.")
        if operator not in SPECTRAL_OPERATORS:
            raise ValueError(f"operator must be one of {SPECTRAL_OPERATORS}, not {operator!r}")
        if int(n_components) < 1:
            raise ValueError(f"n_components must be >= 1, not {n_components!r}")
        self._dtype_code, self._host_dtype = _lib.dtype_code(precision)
        if self._dtype_code == _lib.KMVP_BF16:
            raise NotImplementedError("MI355XSpectral needs float16, float32 or float64")
        if ridge is not None and operator != "kernel":
            raise ValueError("ridge goes with operator='kernel' only")
        if ridge is not None:
            ridge = np.array(ridge, dtype=np.float64)
            if ridge.ndim > 1 or not np.isfinite(ridge).all():
                raise ValueError("ridge must be a finite number or a one-dimensional array of one value per point")
        self.kernel, self.dimension, self.precision = kernel, int(dimension), precision
        self.n_components, self.operator = int(n_components), operator
        self._round = _lib.input_rounding(precision)  # float16: rounded points, float32 arithmetic
        self.tol = float(tol) if tol is not None else (1e-10 if self._dtype_code == _lib.KMVP_F64 else 1e-4)
        self.maxit = None if maxit is None else int(maxit)
        self.seed, self.ridge, self.device = seed, ridge, device
        self._ctx = self._transform_ctx = None
        self.eigenvalues = self.eigenvectors = self.residuals = self.degree = None
        self.steps, self.converged = 0, False
        self.name = f"MI355XSpectral({_precision_name(precision)}, {kernel}, {operator}, n_components={self.n_components})"

    def _as_device_points(self, points, what):
        p = np.asarray(points, dtype=np.float64)
        if p.ndim != 2 or p.shape[1] != self.dimension:
            raise ValueError(f"{what} has shape {p.shape}, expected (N, {self.dimension})")
        if self._round is not None:
            p = p.astype(self._round)
        return np.ascontiguousarray(p, dtype=self._host_dtype)

    # -- untimed -------------------------------------------------------------------
    def prepare_data(self, *, points):
        x = self._as_device_points(points, "points")
        self.N, self.D = x.shape
        if self.n_components > self.N:
            raise ValueError(f"n_components = {self.n_components} for {self.N} points")
        if self.ridge is not None and self.ridge.ndim == 1 and self.ridge.size != self.N:
            raise ValueError(f"ridge has {self.ridge.size} values, the point cloud has {self.N} points")
        self._x = x  # the points as the device holds them
        if self._ctx is None:
            self._ctx = _lib.Context(self.device)
        self._ctx.set_points(x, None, self._dtype_code)
        if self.ridge is not None:  # (kmvp_set_points cleared the library's diagonal)
            if self.ridge.ndim == 1:
                self._ctx.set_solver_diagonal(np.ascontiguousarray(self.ridge), 0.0)
            else:
                self._ctx.set_solver_diagonal(None, float(self.ridge))
        self.eigenvalues = self.eigenvectors = self.residuals = self.degree = None

    # -- timed ---------------------------------------------------------------------
    def fit(self):
        """Whatever the product builds from the points alone (kmvp_fit)."""
        if self._ctx is None:
            raise RuntimeError("MI355XSpectral.fit() needs prepare_data() first")
        self._ctx.fit(self.kernel)

    def set_query_arguments(self, tol=None, maxit=None):
        if tol is not None:
            self.tol = float(tol)
        if maxit is not None:
            self.maxit = int(maxit)

    def query(self, v0=None):
        """Runs the Lanczos process from ``v0`` (N values; default: a standard normal draw from ``seed``).  Synchronous."""
        if self._ctx is None:
            raise RuntimeError("MI355XSpectral.query() needs prepare_data() first")
        if v0 is None:
            v0 = np.random.RandomState(self.seed).standard_normal(self.N)
        maxit = min(self.N, SPECTRAL_MAX_STEPS) if self.maxit is None else self.maxit
        r = self._ctx.eigsh(self.kernel, self.n_components, self.operator, v0, self.tol, maxit)
        self.eigenvalues, self.eigenvectors, self.residuals = r["eigenvalues"], r["eigenvectors"], r["resid"]
        self.steps, self.converged = r["steps"], r["converged"]
        self._eigsh_ms = self._ctx.last_total_ms
        self.degree = r.get("degree")
        if self.operator == "centered":
            # the column sums of K, for transform(): one density product on the same context
            self._ctx.set_signal(None)
            self._ctx.run(self.kernel, False)
            self.degree = self._ctx.get_result(self.N, 1)[:, 0]

    # -- results -------------------------------------------------------------------
    def _need_solution(self, method):
        if self.eigenvalues is None:
            raise RuntimeError(f"MI355XSpectral.{method}: no solution yet -- call query() after prepare_data() first")

    def get_eigenvalues(self):
        """(n_components,) float64, descending: the Ritz values."""
        self._need_solution("get_eigenvalues")
        return self.eigenvalues

    def get_eigenvectors(self):
        """(N, n_components) float64: unit columns, each with its component of largest magnitude positive."""
        self._need_solution("get_eigenvectors")
        return self.eigenvectors

    def get_residuals(self):
        """(n_components,) float64: |A x_i - theta_i x_i| / (theta_1 |x_i|) from one more application of A."""
        self._need_solution("get_residuals")
        return self.residuals

    def get_degree(self):
        """(N,) float64: the row sums K 1 (operator "normalized": what the library scaled by; "centered": what
        transform() centres with); None for operator "kernel"."""
        self._need_solution("get_degree")
        return self.degree

    def get_embedding(self):
        """(N, n_components) float64.  "kernel" and "centered": X sqrt(max(theta, 0)), the convention of
        sklearn.decomposition.KernelPCA.fit_transform.  "normalized": the rows of X scaled to unit length (Ng, Jordan and
        Weiss); a row of zeros stays as it is."""
        self._need_solution("get_embedding")
        X = self.eigenvectors
        if self.operator != "normalized":
            return X * np.sqrt(np.maximum(self.eigenvalues, 0.0))
        norms = np.sqrt(np.sum(X * X, axis=1, keepdims=True))
        return X / np.where(norms > 0, norms, 1.0)

    def transform(self, points):
        """(M, n_components) float64: the embedding of new points, K(x, Y) (X theta^-1/2) with the library's own product
        -- for "centered" with K(x, Y) centred as sklearn's KernelCenterer does it, from the row means K(x, Y) 1 / N of
        the new points, the stored column means of the training matrix and its total mean.  Columns with theta <= 0 are
        zero.  Not defined for "normalized"."""
        self._need_solution("transform")
        if self.operator == "normalized":
            raise NotImplementedError("MI355XSpectral.transform is for operator 'kernel' and 'centered': the normalised "
                                      "embedding has no out-of-sample form here")
        x = self._as_device_points(points, "points")
        theta = self.eigenvalues
        scale = np.where(theta > 0, 1.0 / np.sqrt(np.where(theta > 0, theta, 1.0)), 0.0)
        A = self.eigenvectors * scale  # (N, k)
        signal = np.concatenate([A, np.ones((self.N, 1))], axis=1) if self.operator == "centered" else A
        if self._transform_ctx is None:  # a context of its own: the solver's keeps the square problem
            self._transform_ctx = _lib.Context(self.device)
        self._transform_ctx.set_points(self._x, x, self._dtype_code)
        self._transform_ctx.set_signal(np.ascontiguousarray(signal, dtype=self._host_dtype))
        self._transform_ctx.run(self.kernel, False)
        out = self._transform_ctx.get_result(x.shape[0], signal.shape[1])
        if self.operator != "centered":
            return out
        k = self.n_components
        col_mean = self.degree / self.N                  # (1/N) sum_i K(y_i, y_j)
        total = float(np.sum(self.degree)) / self.N ** 2
        row_mean = out[:, k:] / self.N                   # (1/N) sum_j K(x, y_j)
        ones_A = np.sum(A, axis=0)                       # 1' A (zero up to rounding: the eigenvectors are centred)
        return out[:, :k] - row_mean * ones_A - col_mean @ A + total * ones_A

    def get_memory_usage(self):
        """Device kB held by the contexts."""
        return sum(ctx.device_bytes for ctx in (self._ctx, self._transform_ctx) if ctx is not None) / 1024

    def get_additional(self):
        extra = {"steps": self.steps, "converged": bool(self.converged), "tol": self.tol,
                 "worst_residual": float("nan") if self.residuals is None else float(np.max(self.residuals))}
        if self._ctx is not None:
            extra.update(device_total_ms=getattr(self, "_eigsh_ms", 0.0), device_bytes=self._ctx.device_bytes)
        return extra

    def done(self):
        for ctx in (self._ctx, self._transform_ctx):
            if ctx is not None:
                ctx.close()
        self._ctx = self._transform_ctx = None

    def __del__(self):
        try:
            self.done()
        except Exception:
            pass


MEANSHIFT_MAX_D = NEAREST_MAX_D


class MI355XMeanShift:
    """Gaussian mean-shift on one MI355X, resident on the device (include/kmvp.h kmvp_gaussian_meanshift; the pair loop is
    lowd_lse_grad_kernel: for the Gaussian the gradient of the log-sum-exp is -2 (x - ybar), so x + G / 2 is the mean-shift
    update, on the integer shift of the log-sum-exp).  The mode-seeking counterpart of MI355XKMeans: clustering without a
    cluster count.  An extension: the reference's plugin API has no such role, so the class is not registered in
    algos.yaml.

        every seed x climbs   x <- sum_j w_j exp(-|x - y_j|^2) y_j / sum_j w_j exp(-|x - y_j|^2)

    until its step is within ``tol`` (absolute, in the units of the points) or ``maxit`` sweeps have run; a point that has
    arrived drops out of the launch.  The bandwidth is the caller's scaling of the points: a Gaussian of bandwidth h is
    exp(-|x - y|^2) on points divided by h.

    Call order: prepare_data, set_query_arguments, query, then get_modes / get_iterations / get_clusters /
    get_additional, done.  ``options``: device, segments, chunk, compact (False: frozen points ride along; the results are
    the same bit for bit)."""

    def __init__(self, *, dimension, precision=np.float32, tol=1e-4, maxit=1000, device=0, segments=0, chunk=0, compact=True):
        if not float(tol) >= 0:
            raise ValueError(f"tol must be >= 0, not {tol!r}")
        self.dimension = int(dimension)
        self.precision = precision
        self._dtype_code, self._host_dtype = _lib.dtype_code(precision)
        if self._dtype_code == _lib.KMVP_BF16:
            raise NotImplementedError("MI355XMeanShift: float32, float64 and float16 only")
        self._round = _lib.input_rounding(precision)  # float16: rounded points, float32 arithmetic
        self.tol, self.maxit = float(tol), int(maxit)
        self.device = device
        self._options = dict(segments=segments, chunk=chunk)
        self._compact = bool(compact)
        self._ctx = None
        self.modes = self.iterations = self.step2 = None
        self.sweeps, self.target_sweeps, self.converged = 0, 0, False
        self.name = f"MI355XMeanShift({_precision_name(precision)})"

    def _as_device_points(self, points, what):
        p = np.asarray(points, dtype=np.float64)
        if p.ndim != 2 or p.shape[1] != self.dimension:
            raise ValueError(f"{what} has shape {p.shape}, expected (N, {self.dimension})")
        if self._round is not None:
            p = p.astype(self._round)
        return np.ascontiguousarray(p, dtype=self._host_dtype)

    # -- untimed -------------------------------------------------------------------
    def prepare_data(self, *, points, weights=None, seeds=None):
        """points (M, D): the data; weights (M,) >= 0 and finite or None (every weight 1; 0: a point of mass 0); seeds
        (N, D) or None: the points themselves."""
        y = self._as_device_points(points, "points")
        self.M, self.D = y.shape
        if self.M < 1:
            raise ValueError("mean-shift needs at least one point")
        x = None if seeds is None else self._as_device_points(seeds, "seeds")
        self.N = self.M if x is None else x.shape[0]
        if self.N < 1:
            raise ValueError("mean-shift needs at least one seed")
        log_w = None
        if weights is not None:
            w = np.asarray(weights, dtype=np.float64).reshape(-1)
            if w.shape != (self.M,):
                raise ValueError(f"weights has {w.size} entries for {self.M} points")
            if not (np.all(w >= 0) and np.all(np.isfinite(w))):  # (NaN fails the first)
                raise ValueError("weights must be non-negative and finite")
            with np.errstate(divide="ignore"):
                log_w = np.ascontiguousarray(np.log(w).reshape(-1, 1), dtype=self._host_dtype)  # 0 -> -inf: mass 0
        if self._ctx is None:
            self._ctx = _lib.Context(self.device)
            for key, value in self._options.items():
                if value:
                    self._ctx.set_option(key, value)
            if not self._compact:
                self._ctx.set_option("meanshift_compact", 0)
        self._ctx.set_points(y, x, self._dtype_code)
        self._ctx.set_signal(log_w)
        self.modes = self.iterations = self.step2 = None

    def set_query_arguments(self, tol=None, maxit=None):
        if tol is not None:
            self.tol = float(tol)
        if maxit is not None:
            self.maxit = int(maxit)

    # -- timed ---------------------------------------------------------------------
    def fit(self):
        """Nothing to build ahead of the first solve: it packs the source records itself, once per prepare_data."""

    def query(self):
        """Runs the iteration from the seeds.  Synchronous.  Not converged (maxit reached, or a point whose gradient is
        not finite) is a result, reported by get_additional(); every other failure raises."""
        if self._ctx is None:
            raise RuntimeError("MI355XMeanShift.query() needs prepare_data() first")
        r = self._ctx.meanshift(self.tol, self.maxit)
        self.modes, self.iterations, self.step2 = r["modes"], r["iters"], r["step2"]
        self.sweeps, self.target_sweeps, self.converged = r["sweeps"], r["target_sweeps"], r["converged"]

    # -- results -------------------------------------------------------------------
    def _need_solution(self, method):
        if self.modes is None:
            raise RuntimeError(f"MI355XMeanShift.{method}: no solution yet -- call query() after prepare_data() first")

    def _arrived(self):
        with np.errstate(invalid="ignore"):
            return np.all(np.isfinite(self.modes), axis=1) & (self.step2 <= self.tol * self.tol)

    def get_modes(self):
        """(N, D) float64: where every seed ended up (a NaN row: its gradient was not finite)."""
        self._need_solution("get_modes")
        return self.modes

    def get_iterations(self):
        """(N,) int64: the sweep after which every seed froze (the sweeps run, for one still moving at the end)."""
        self._need_solution("get_iterations")
        return self.iterations

    def get_clusters(self, merge_radius):
        """(centres (C, D) float64, labels (N,) int64) by a host rule: walk the converged modes -- finite, last step within
        tol -- in ascending index; a mode founds a centre if no earlier centre lies within ``merge_radius`` of it
        (Euclidean distance in float64, the squares added with d ascending, <=).  Afterwards every converged point gets the label of its nearest centre, ties
        to the smaller label; unconverged or NaN points get -1.  One vectorised numpy pass over the points per centre."""
        self._need_solution("get_clusters")
        ok = self._arrived()
        idx = np.flatnonzero(ok)
        z = self.modes[idx]
        centres = []
        near = np.full(idx.size, np.inf)    # distance of every converged mode to its nearest centre so far
        label = np.full(idx.size, -1, dtype=np.int64)
        while True:
            # the first mode, in index order, that no centre founded so far covers (near only shrinks, so everything
            # before it stays covered: the walk never has to look back)
            open_ = np.flatnonzero(near > merge_radius)
            if open_.size == 0:
                break
            c = z[open_[0]]
            s = np.zeros(idx.size)
            for d in range(self.D):  # the squares added with d ascending
                s = s + (z[:, d] - c[d]) ** 2
            dist = np.sqrt(s)
            closer = dist < near  # strictly: a tie stays with the smaller label
            label[closer] = len(centres)
            near = np.where(closer, dist, near)
            centres.append(c.copy())
        labels = np.full(self.N, -1, dtype=np.int64)
        labels[idx] = label
        return np.array(centres, dtype=np.float64).reshape(len(centres), self.D), labels

    def get_memory_usage(self):
        """Device kB held by the context."""
        return (self._ctx.device_bytes if self._ctx is not None else 0) / 1024

    def get_additional(self):
        extra = {"sweeps": self.sweeps, "target_sweeps": self.target_sweeps, "converged": bool(self.converged)}
        if self.modes is not None:
            extra["unconverged"] = int(self.N - np.count_nonzero(self._arrived()))
        if self._ctx is not None:
            extra.update(device_kernel_ms=self._ctx.last_kernel_ms, device_total_ms=self._ctx.last_total_ms,
                         device_kernel=self._ctx.last_kernel_name, device_bytes=self._ctx.device_bytes)
        return extra

    def done(self):
        if self._ctx is not None:
            self._ctx.close()
        self._ctx = None

    def __del__(self):
        try:
            self.done()
        except Exception:
            pass


class MI355XDBSCAN:
    """DBSCAN on one MI355X, resident on the device (include/kmvp.h kmvp_dbscan; the pair loops are
    lowd_cutoff_count_kernel and lowd_cutoff_label_kernel on the cutoff's cell list).  The third clusterer beside
    MI355XKMeans and MI355XMeanShift: density clustering without a cluster count.  An extension: the reference's plugin API
    has no such role, so the class is not registered in algos.yaml.

        core point    at least min_samples points within eps, itself included (sklearn's convention)
        cluster       a connected component of the core points under "within eps", numbered in ascending order of its
                      smallest core index -- the numbering sklearn.cluster.DBSCAN gives
        border point  a point that is no core point with a core point within eps: it joins the cluster of the NEAREST one
                      (ties: the smaller index).  sklearn's choice depends on its traversal order, this one does not
        noise         everything else, label -1

    Call order: prepare_data, set_query_arguments, query, then get_labels / get_core_sample_indices / get_core_of /
    get_counts / get_additional, done.  D <= 3; float16 / float32 / float64.  ``options``: device, cutoff_plan ("host" or
    "device": the side that builds the cell-list plan; the same result), cutoff_cell_factor (the cells' side in units of
    eps, >= 1; the same result)."""

    def __init__(self, *, eps, min_samples, dimension, precision=np.float32, device=0, cutoff_plan="host", cutoff_cell_factor=None):
        self.dimension = int(dimension)
        self.precision = precision
        self._dtype_code, self._host_dtype = _lib.dtype_code(precision)
        if self._dtype_code == _lib.KMVP_BF16:
            raise NotImplementedError("MI355XDBSCAN: float32, float64 and float16 only")
        if self.dimension > 3:
            raise NotImplementedError(f"MI355XDBSCAN: dimension = {self.dimension} is beyond the cell list's D <= 3")
        self._round = _lib.input_rounding(precision)  # float16: rounded points, float32 arithmetic
        self.device = device
        self._cutoff_plan = _cutoff_plan_code(cutoff_plan)
        self._cell_factor = None if cutoff_cell_factor is None else float(cutoff_cell_factor)
        self._ctx = None
        self.labels = self.core_of = self.counts = self.info = None
        self.set_query_arguments(eps=eps, min_samples=min_samples)
        self.name = f"MI355XDBSCAN({_precision_name(precision)}, eps={self.eps}, min_samples={self.min_samples})"

    # -- untimed -------------------------------------------------------------------
    def prepare_data(self, *, points):
        p = np.asarray(points, dtype=np.float64)
        if p.ndim != 2 or p.shape[1] != self.dimension:
            raise ValueError(f"points has shape {p.shape}, expected (N, {self.dimension})")
        if self._round is not None:
            p = p.astype(self._round)
        x = np.ascontiguousarray(p, dtype=self._host_dtype)
        self.N, self.D = x.shape
        self._x = x  # the points as the device holds them
        if self._ctx is None:
            self._ctx = _lib.Context(self.device)
            if self._cutoff_plan:
                self._ctx.set_option("cutoff_plan", self._cutoff_plan)
            if self._cell_factor is not None:
                self._ctx.set_option("cutoff_cell_factor", self._cell_factor)
        self._ctx.set_points(x, None, self._dtype_code)  # the cloud is its own target set: the points of kmvp_dbscan
        self.labels = self.core_of = self.counts = self.info = None

    def set_query_arguments(self, eps=None, min_samples=None):
        if eps is not None:
            if not (np.isfinite(float(eps)) and float(eps) > 0):
                raise ValueError(f"eps must be finite and > 0, not {eps!r}")
            self.eps = float(eps)
        if min_samples is not None:
            if int(min_samples) != min_samples or int(min_samples) < 1:
                raise ValueError(f"min_samples must be an integer >= 1, not {min_samples!r}")
            self.min_samples = int(min_samples)

    # -- timed ---------------------------------------------------------------------
    def fit(self):
        """Nothing to build ahead of the first query: it plans and packs itself, once per (points, eps)."""

    def query(self):
        """Clusters the points.  Synchronous; every failure raises."""
        if self._ctx is None:
            raise RuntimeError("MI355XDBSCAN.query() needs prepare_data() first")
        self.labels, self.core_of, self.counts, self.info = self._ctx.dbscan(self.eps, self.min_samples)

    # -- results -------------------------------------------------------------------
    def _need_solution(self, method):
        if self.labels is None:
            raise RuntimeError(f"MI355XDBSCAN.{method}: no solution yet -- call query() after prepare_data() first")

    def get_labels(self):
        """(N,) int64: the cluster of every point, -1 for noise (sklearn's labels_ on the core points and the noise)."""
        self._need_solution("get_labels")
        return self.labels

    def get_core_sample_indices(self):
        """The indices of the core points in ascending order (sklearn's core_sample_indices_)."""
        self._need_solution("get_core_sample_indices")
        return np.flatnonzero(self.core_of == np.arange(self.N))

    def get_core_of(self):
        """(N,) int64: the point itself for a core point, the core point a border point was attached to, -1 for noise."""
        self._need_solution("get_core_of")
        return self.core_of

    def get_counts(self):
        """(N,) int64: the points within eps of every point, itself included; -1 for a point with a NaN coordinate."""
        self._need_solution("get_counts")
        return self.counts

    def get_memory_usage(self):
        """Device kB held by the context."""
        return (self._ctx.device_bytes if self._ctx is not None else 0) / 1024

    def get_additional(self):
        extra = dict(self.info or {})
        if self._ctx is not None:
            extra.update(device_kernel_ms=self._ctx.last_kernel_ms, device_total_ms=self._ctx.last_total_ms,
                         device_kernel=self._ctx.last_kernel_name, device_bytes=self._ctx.device_bytes)
        return extra

    def done(self):
        if self._ctx is not None:
            self._ctx.close()
        self._ctx = None

    def __del__(self):
        try:
            self.done()
        except Exception:
            pass
