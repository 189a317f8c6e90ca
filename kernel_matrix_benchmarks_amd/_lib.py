"""ctypes binding of libkmvp.so (include/kmvp.h).

The library is the product: there is NO fallback.  If it cannot be loaded, or no
GPU is present, every compute entry point raises.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KMVP_LIB", os.path.join(_HERE, "libkmvp.so"))

KMVP_F32, KMVP_F64, KMVP_BF16 = 0, 1, 2
STATUS = {
    0: "OK", 1: "INVALID", 2: "UNSUPPORTED", 3: "DEVICE", 4: "COMM", 5: "NOMEM", 6: "NOT_CONVERGED",
}
UNIQUE_ID_BYTES = 128

# every symbol include/kmvp.h declares: (name, restype, argtypes)
_c = ctypes
SYMBOLS = [
    ("kmvp_abi_version", _c.c_int, []),
    ("kmvp_device_count", _c.c_int, []),
    ("kmvp_create", _c.c_void_p, [_c.c_int, _c.POINTER(_c.c_int)]),
    ("kmvp_destroy", None, [_c.c_void_p]),
    ("kmvp_last_error", _c.c_char_p, [_c.c_void_p]),
    ("kmvp_set_points", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_void_p, _c.c_int64,
                                   _c.c_int, _c.c_int, _c.c_int64, _c.c_int64]),
    ("kmvp_fit", _c.c_int, [_c.c_void_p, _c.c_int]),
    ("kmvp_set_signal", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int]),
    ("kmvp_gaussian", _c.c_int, [_c.c_void_p]),
    ("kmvp_gaussian_norm", _c.c_int, [_c.c_void_p]),
    ("kmvp_absexp", _c.c_int, [_c.c_void_p]),
    ("kmvp_absexp_norm", _c.c_int, [_c.c_void_p]),
    ("kmvp_invdist", _c.c_int, [_c.c_void_p]),
    ("kmvp_invdist_norm", _c.c_int, [_c.c_void_p]),
    ("kmvp_expdot", _c.c_int, [_c.c_void_p]),
    ("kmvp_expdot_norm", _c.c_int, [_c.c_void_p]),
    ("kmvp_matern32", _c.c_int, [_c.c_void_p]),
    ("kmvp_matern32_norm", _c.c_int, [_c.c_void_p]),
    ("kmvp_matern52", _c.c_int, [_c.c_void_p]),
    ("kmvp_matern52_norm", _c.c_int, [_c.c_void_p]),
    ("kmvp_gaussian_grad", _c.c_int, [_c.c_void_p]),
    ("kmvp_absexp_grad", _c.c_int, [_c.c_void_p]),
    ("kmvp_invdist_grad", _c.c_int, [_c.c_void_p]),
    ("kmvp_matern32_grad", _c.c_int, [_c.c_void_p]),
    ("kmvp_matern52_grad", _c.c_int, [_c.c_void_p]),
    ("kmvp_gaussian_dscale", _c.c_int, [_c.c_void_p]),
    ("kmvp_absexp_dscale", _c.c_int, [_c.c_void_p]),
    ("kmvp_matern32_dscale", _c.c_int, [_c.c_void_p]),
    ("kmvp_matern52_dscale", _c.c_int, [_c.c_void_p]),
    ("kmvp_gaussian_logsumexp", _c.c_int, [_c.c_void_p]),
    ("kmvp_absexp_logsumexp", _c.c_int, [_c.c_void_p]),
    ("kmvp_gaussian_logsumexp_grad", _c.c_int, [_c.c_void_p]),
    ("kmvp_absexp_logsumexp_grad", _c.c_int, [_c.c_void_p]),
    ("kmvp_nearest", _c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p]),
    ("kmvp_set_batches", _c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_void_p]),
    ("kmvp_gaussian_cutoff", _c.c_int, [_c.c_void_p, _c.c_double, _c.c_int]),
    ("kmvp_absexp_cutoff", _c.c_int, [_c.c_void_p, _c.c_double, _c.c_int]),
    ("kmvp_matern32_cutoff", _c.c_int, [_c.c_void_p, _c.c_double, _c.c_int]),
    ("kmvp_matern52_cutoff", _c.c_int, [_c.c_void_p, _c.c_double, _c.c_int]),
    ("kmvp_wendland_c2_cutoff", _c.c_int, [_c.c_void_p, _c.c_double, _c.c_int]),
    ("kmvp_wendland_c4_cutoff", _c.c_int, [_c.c_void_p, _c.c_double, _c.c_int]),
    ("kmvp_gaussian_cutoff_grad", _c.c_int, [_c.c_void_p, _c.c_double]),
    ("kmvp_absexp_cutoff_grad", _c.c_int, [_c.c_void_p, _c.c_double]),
    ("kmvp_matern32_cutoff_grad", _c.c_int, [_c.c_void_p, _c.c_double]),
    ("kmvp_matern52_cutoff_grad", _c.c_int, [_c.c_void_p, _c.c_double]),
    ("kmvp_wendland_c2_cutoff_grad", _c.c_int, [_c.c_void_p, _c.c_double]),
    ("kmvp_wendland_c4_cutoff_grad", _c.c_int, [_c.c_void_p, _c.c_double]),
    ("kmvp_radius_count", _c.c_int, [_c.c_void_p, _c.c_double, _c.c_int, _c.c_void_p]),
    ("kmvp_radius_nearest", _c.c_int, [_c.c_void_p, _c.c_double, _c.c_int, _c.c_int, _c.c_void_p, _c.c_void_p]),
    ("kmvp_dbscan", _c.c_int, [_c.c_void_p, _c.c_double, _c.c_int64, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    ("kmvp_cutoff_info", _c.c_int, [_c.c_void_p, _c.c_void_p]),
    ("kmvp_cutoff_plan_read", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_void_p]),
    ("kmvp_kmeans", _c.c_int, [_c.c_void_p, _c.c_int, _c.c_void_p, _c.c_double, _c.c_int, _c.c_void_p, _c.c_void_p,
                               _c.c_void_p, _c.POINTER(_c.c_int), _c.POINTER(_c.c_double), _c.POINTER(_c.c_double)]),
    ("kmvp_gaussian_meanshift", _c.c_int, [_c.c_void_p, _c.c_double, _c.c_int, _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                           _c.POINTER(_c.c_int), _c.POINTER(_c.c_int64)]),
    ("kmvp_get_result", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int64]),
    ("kmvp_gaussian_cg_solve", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_double, _c.c_int,
                                          _c.c_void_p, _c.POINTER(_c.c_int), _c.POINTER(_c.c_double)]),
    ("kmvp_absexp_cg_solve", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_double, _c.c_int,
                                        _c.c_void_p, _c.POINTER(_c.c_int), _c.POINTER(_c.c_double)]),
    ("kmvp_matern32_cg_solve", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_double, _c.c_int,
                                          _c.c_void_p, _c.POINTER(_c.c_int), _c.POINTER(_c.c_double)]),
    ("kmvp_matern52_cg_solve", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_double, _c.c_int,
                                          _c.c_void_p, _c.POINTER(_c.c_int), _c.POINTER(_c.c_double)]),
    ("kmvp_wendland_c2_cg_solve", _c.c_int, [_c.c_void_p, _c.c_double, _c.c_void_p, _c.c_int, _c.c_double, _c.c_int,
                                             _c.c_void_p, _c.POINTER(_c.c_int), _c.POINTER(_c.c_double)]),
    ("kmvp_wendland_c4_cg_solve", _c.c_int, [_c.c_void_p, _c.c_double, _c.c_void_p, _c.c_int, _c.c_double, _c.c_int,
                                             _c.c_void_p, _c.POINTER(_c.c_int), _c.POINTER(_c.c_double)]),
    ("kmvp_invdist_minres_solve", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_double, _c.c_int,
                                             _c.c_void_p, _c.POINTER(_c.c_int), _c.POINTER(_c.c_double)]),
    ("kmvp_gaussian_lanczos_quadrature", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_double, _c.c_int] + [_c.c_void_p] * 6),
    ("kmvp_absexp_lanczos_quadrature", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_double, _c.c_int] + [_c.c_void_p] * 6),
    ("kmvp_matern32_lanczos_quadrature", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_double, _c.c_int] + [_c.c_void_p] * 6),
    ("kmvp_matern52_lanczos_quadrature", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_double, _c.c_int] + [_c.c_void_p] * 6),
    ("kmvp_gaussian_eigsh", _c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_double, _c.c_int] + [_c.c_void_p] * 7),
    ("kmvp_absexp_eigsh", _c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_double, _c.c_int] + [_c.c_void_p] * 7),
    ("kmvp_matern32_eigsh", _c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_double, _c.c_int] + [_c.c_void_p] * 7),
    ("kmvp_matern52_eigsh", _c.c_int, [_c.c_void_p, _c.c_int, _c.c_int, _c.c_void_p, _c.c_double, _c.c_int] + [_c.c_void_p] * 7),
    ("kmvp_gaussian_lanczos_quadrature_precond", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_double, _c.c_int] + [_c.c_void_p] * 9),
    ("kmvp_absexp_lanczos_quadrature_precond", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_double, _c.c_int] + [_c.c_void_p] * 9),
    ("kmvp_matern32_lanczos_quadrature_precond", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_double, _c.c_int] + [_c.c_void_p] * 9),
    ("kmvp_matern52_lanczos_quadrature_precond", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_double, _c.c_int] + [_c.c_void_p] * 9),
    ("kmvp_gaussian_sinkhorn", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_double, _c.c_int, _c.c_void_p,
                                          _c.c_void_p, _c.POINTER(_c.c_int), _c.POINTER(_c.c_double)]),
    ("kmvp_absexp_sinkhorn", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_double, _c.c_int, _c.c_void_p,
                                        _c.c_void_p, _c.POINTER(_c.c_int), _c.POINTER(_c.c_double)]),
    ("kmvp_gaussian_sinkhorn_batched", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_double, _c.c_int] + [_c.c_void_p] * 5),
    ("kmvp_absexp_sinkhorn_batched", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_double, _c.c_int] + [_c.c_void_p] * 5),
    ("kmvp_set_solver_diagonal", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int64, _c.c_double]),
    ("kmvp_set_solver_preconditioner", _c.c_int, [_c.c_void_p, _c.c_int]),
    ("kmvp_get_solver_preconditioner", _c.c_int, [_c.c_void_p, _c.POINTER(_c.c_int), _c.c_void_p, _c.c_void_p]),
    ("kmvp_last_preconditioner_ms", _c.c_double, [_c.c_void_p]),
    ("kmvp_comm_get_unique_id", _c.c_int, [_c.c_void_p]),
    ("kmvp_comm_init", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int]),
    ("kmvp_comm_init_host", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p, _c.c_int, _c.c_int]),
    ("kmvp_comm_world", _c.c_int, [_c.c_void_p]),
    ("kmvp_comm_rank", _c.c_int, [_c.c_void_p]),
    ("kmvp_last_allreduce_ms", _c.c_double, [_c.c_void_p]),
    ("kmvp_set_option", _c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_int64]),
    ("kmvp_set_option_double", _c.c_int, [_c.c_void_p, _c.c_char_p, _c.c_double]),
    ("kmvp_device_bytes", _c.c_int64, [_c.c_void_p]),
    ("kmvp_last_kernel_ms", _c.c_double, [_c.c_void_p]),
    ("kmvp_last_total_ms", _c.c_double, [_c.c_void_p]),
    ("kmvp_cell_layout", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.POINTER(_c.c_double), _c.c_void_p, _c.c_void_p, _c.c_void_p,
                                    _c.c_int64, _c.c_void_p, _c.c_int64]),
    ("kmvp_cell_lists", _c.c_int, [_c.c_void_p, _c.c_void_p, _c.c_void_p]),
    ("kmvp_last_kernel_name", _c.c_char_p, [_c.c_void_p]),
    ("kmvp_last_dispatch_note", _c.c_char_p, [_c.c_void_p]),
]

HOST_ALLREDUCE_FN = _c.CFUNCTYPE(_c.c_int, _c.c_void_p, _c.POINTER(_c.c_double), _c.c_int64, _c.c_int)
OP_SUM, OP_MIN = 0, 1
# kernel codes of kmvp_fit (include/kmvp.h)
FIT_CODES = {"gaussian": 0, "absolute-exponential": 1, "inverse-distance": 2, "matern-3/2": 3, "matern-5/2": 4,
             "wendland-c2": 7, "wendland-c4": 8}
# Wendland's compactly supported kernels (include/kmvp.h kmvp_wendland_<c>_cutoff): the cutoff entries and a CG solve only
WENDLAND = ("wendland-c2", "wendland-c4")

# options whose value is a real number (include/kmvp.h kmvp_set_option_double)
REAL_OPTIONS = ("cutoff_cell_factor",)
# sizes[12] of kmvp_cutoff_plan_read: the side that built the cutoff plan ("cutoff_plan" of kmvp_set_option: 0 / 1)
CUTOFF_PLAN_SIDES = ("host", "device")

# enum kmvp_eig_operator (include/kmvp.h)
EIG_OPERATORS = {"kernel": 0, "centered": 1, "normalized": 2}

_lib = None


class KmvpError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"libkmvp: {STATUS.get(code, code)}: {message}")
        self.code = code


def load():
    """Loads libkmvp.so and types every entry point.  Raises if the library is missing."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or make -C kernel_matrix_benchmarks_amd/csrc).  There is no CPU fallback."
            )
        lib = ctypes.CDLL(LIB_PATH)
        for name, restype, argtypes in SYMBOLS:
            fn = getattr(lib, name)
            fn.restype = restype
            fn.argtypes = argtypes
        _lib = lib
    return _lib


def dtype_code(precision):
    """numpy dtype / string ('float32', algos.yaml:157) / 'bfloat16' -> (kmvp_dtype, host numpy dtype).
    float16 (algos.yaml:157,160): the reference casts its inputs to float16 and lets numpy do float16 arithmetic;
    here the inputs are ROUNDED to float16 by the plugin (``input_rounding``) and the arithmetic is float32."""
    if isinstance(precision, str) and precision.lower() in ("bfloat16", "bf16"):
        return KMVP_BF16, np.dtype(np.float32)
    dt = np.dtype(precision)
    if dt == np.float16:
        return KMVP_F32, np.dtype(np.float32)
    if dt == np.float64:
        return KMVP_F64, dt
    if dt == np.float32:
        return KMVP_F32, dt
    raise NotImplementedError(f"precision {precision!r} is not supported by the MI355X backend")


def input_rounding(precision):
    """dtype the host arrays are rounded to BEFORE the cast to the working precision (None: no extra rounding)."""
    if isinstance(precision, str) and precision.lower() in ("bfloat16", "bf16"):
        return None
    return np.dtype(np.float16) if np.dtype(precision) == np.float16 else None


def batch_offsets(offsets, what, total=None):
    """Offsets of B >= 1 batches as a contiguous int64 array of B + 1 values: one-dimensional and of an integer dtype;
    with ``total`` also non-decreasing from 0 to ``total`` (None: left to the library, which answers KMVP_E_INVALID).
    ValueError otherwise -- decided on the host."""
    a = np.asarray(offsets)
    if a.ndim != 1 or a.size < 2:
        raise ValueError(f"{what} has shape {a.shape}, expected B + 1 offsets (B >= 1) in one dimension")
    if not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{what} has dtype {a.dtype}, expected integers")
    a = np.ascontiguousarray(a, dtype=np.int64)
    if total is not None and (a[0] != 0 or np.any(np.diff(a) < 0) or a[-1] != total):
        raise ValueError(f"{what} must be non-decreasing from 0 to {total}")
    return a


def _vector(a, n, what):
    """None, or ``a`` as n contiguous float64 values: the library reads n doubles from the pointer, so a shorter array
    must never reach it."""
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.shape != (n,):
        raise ValueError(f"{what} has shape {a.shape}, expected ({n},)")
    return a


class Context:
    """Owns one kmvp_ctx (one GPU).  Thin, typed wrappers; all errors raise KmvpError."""

    def __init__(self, device=0):
        self._lib = load()
        status = ctypes.c_int(0)
        self._ctx = self._lib.kmvp_create(int(device), ctypes.byref(status))
        if not self._ctx:
            msg = self._lib.kmvp_last_error(None)
            raise KmvpError(status.value, msg.decode() if msg else "kmvp_create failed")
        self.device = int(device)
        self.comm_world = 0  # ranks of the communicator attached to THIS context (0: none)

    def _check(self, rc):
        if rc != 0:
            msg = self._lib.kmvp_last_error(self._ctx)
            raise KmvpError(rc, msg.decode() if msg else "")

    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.kmvp_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_points(self, y, x, dtype_code_, j_offset=0, M_total=None):
        M, D = y.shape
        N = M if x is None else x.shape[0]
        if x is not None and x.shape[1] != D:
            raise ValueError(f"target points have {x.shape[1]} coordinates, source points {D}")
        self.M, self.N, self.D = M, N, D
        self.B = 0  # (kmvp_set_points switches the batches off)
        self._check(self._lib.kmvp_set_points(
            self._ctx, y.ctypes.data, M, None if x is None else x.ctypes.data, N, D, dtype_code_,
            int(j_offset), int(M if M_total is None else M_total)))

    def set_batches(self, y_offsets, x_offsets=None):
        """Batched clouds (include/kmvp.h kmvp_set_batches): offsets of B + 1 values over the sources and -- None: the
        sources' own, same points only -- over the targets.  set_batches(None) switches the batches off."""
        if y_offsets is None:
            if x_offsets is not None:
                raise ValueError("target offsets without source offsets")
            self._check(self._lib.kmvp_set_batches(self._ctx, 0, None, None))
            self.B = 0
            return
        # the library reads B + 1 values from each pointer: arrays of another length must never reach it
        y_offsets = batch_offsets(y_offsets, "source_batches")
        if x_offsets is not None:
            x_offsets = batch_offsets(x_offsets, "target_batches")
            if x_offsets.size != y_offsets.size:
                raise ValueError(f"target_batches has {x_offsets.size} offsets, source_batches {y_offsets.size}: both hold B + 1")
        self._check(self._lib.kmvp_set_batches(self._ctx, y_offsets.size - 1, y_offsets.ctypes.data,
                                               None if x_offsets is None else x_offsets.ctypes.data))
        self.B = y_offsets.size - 1  # (a refused call raised above and left the previous setting)

    def fit(self, kernel):
        self._check(self._lib.kmvp_fit(self._ctx, FIT_CODES[kernel]))

    def set_signal(self, b):
        if b is None:
            self._check(self._lib.kmvp_set_signal(self._ctx, None, 1))
        else:
            # the library copies M * E elements from the pointer: a shorter array must never reach it
            if b.ndim != 2 or b.shape[0] != getattr(self, "M", b.shape[0]):
                raise ValueError(f"source_signal has shape {b.shape}, expected ({getattr(self, 'M', '?')}, E): one row per "
                                 "source point")
            self._check(self._lib.kmvp_set_signal(self._ctx, b.ctypes.data, b.shape[1]))

    def run(self, kernel, normalize_rows):
        if kernel in WENDLAND:
            raise NotImplementedError(f"kernel {kernel} has no plain (all-pairs) product: its support is the radius, use run_cutoff")
        entry = {
            ("gaussian", False): self._lib.kmvp_gaussian,
            ("gaussian", True): self._lib.kmvp_gaussian_norm,
            ("absolute-exponential", False): self._lib.kmvp_absexp,
            ("absolute-exponential", True): self._lib.kmvp_absexp_norm,
            ("inverse-distance", False): self._lib.kmvp_invdist,
            ("inverse-distance", True): self._lib.kmvp_invdist_norm,
            ("exp-dot", False): self._lib.kmvp_expdot,
            ("exp-dot", True): self._lib.kmvp_expdot_norm,
            ("matern-3/2", False): self._lib.kmvp_matern32,
            ("matern-3/2", True): self._lib.kmvp_matern32_norm,
            ("matern-5/2", False): self._lib.kmvp_matern52,
            ("matern-5/2", True): self._lib.kmvp_matern52_norm,
        }[(kernel, bool(normalize_rows))]
        self._check(entry(self._ctx))

    def run_grad(self, kernel):
        """Gradient with respect to the targets (include/kmvp.h kmvp_<kernel>_grad); read it with get_result(N, E * D)."""
        entry = {
            "gaussian": self._lib.kmvp_gaussian_grad,
            "absolute-exponential": self._lib.kmvp_absexp_grad,
            "inverse-distance": self._lib.kmvp_invdist_grad,
            "matern-3/2": self._lib.kmvp_matern32_grad,
            "matern-5/2": self._lib.kmvp_matern52_grad,
        }.get(kernel)
        if entry is None:
            raise NotImplementedError(f"no gradient for kernel {kernel}")
        self._check(entry(self._ctx))

    def run_dscale(self, kernel):
        """Derivative in the logarithm of a per-axis length scale (include/kmvp.h kmvp_<kernel>_dscale); read it with
        get_result(N, E * D)."""
        entry = {
            "gaussian": self._lib.kmvp_gaussian_dscale,
            "absolute-exponential": self._lib.kmvp_absexp_dscale,
            "matern-3/2": self._lib.kmvp_matern32_dscale,
            "matern-5/2": self._lib.kmvp_matern52_dscale,
        }.get(kernel)
        if entry is None:
            raise NotImplementedError(f"no length-scale derivative for kernel {kernel}")
        self._check(entry(self._ctx))

    def run_lse(self, kernel):
        """Log-sum-exp with the signal read as log-weights (include/kmvp.h kmvp_<kernel>_logsumexp); read it with
        get_result(N, E)."""
        entry = {
            "gaussian": self._lib.kmvp_gaussian_logsumexp,
            "absolute-exponential": self._lib.kmvp_absexp_logsumexp,
        }.get(kernel)
        if entry is None:
            raise NotImplementedError(f"no log-sum-exp for kernel {kernel}")
        self._check(entry(self._ctx))

    def run_lse_grad(self, kernel):
        """Gradient of the log-sum-exp with respect to the target points (include/kmvp.h kmvp_<kernel>_logsumexp_grad);
        read it with get_result(N, E * D)."""
        entry = {
            "gaussian": self._lib.kmvp_gaussian_logsumexp_grad,
            "absolute-exponential": self._lib.kmvp_absexp_logsumexp_grad,
        }.get(kernel)
        if entry is None:
            raise NotImplementedError(f"no log-sum-exp gradient for kernel {kernel}")
        self._check(entry(self._ctx))

    def run_nearest(self, K, exclude_self=False):
        """The K nearest sources of every target (include/kmvp.h kmvp_nearest): (idx int64 (N, K), sqdist float64 (N, K)),
        nearest first, ties in ascending index, global indices; (-1, +inf) where fewer than K sources qualify."""
        K = int(K)
        N = int(getattr(self, "N", 0))
        # the library writes N * K elements through each pointer: the arrays are sized here, from the points it was given
        idx = np.empty((N, max(K, 0)), dtype=np.int64)
        sqdist = np.empty((N, max(K, 0)), dtype=np.float64)
        self._check(self._lib.kmvp_nearest(self._ctx, K, 1 if exclude_self else 0, idx.ctypes.data, sqdist.ctypes.data))
        return idx, sqdist

    def run_cutoff(self, kernel, radius, normalize_rows=False):
        """The product over the sources within ``radius`` of every target (include/kmvp.h kmvp_<kernel>_cutoff): a pair is
        inside iff its squared distance in the working precision is <= radius^2.  Read it with get_result(N, E)."""
        entry = {
            "gaussian": self._lib.kmvp_gaussian_cutoff,
            "absolute-exponential": self._lib.kmvp_absexp_cutoff,
            "matern-3/2": self._lib.kmvp_matern32_cutoff,
            "matern-5/2": self._lib.kmvp_matern52_cutoff,
            "wendland-c2": self._lib.kmvp_wendland_c2_cutoff,
            "wendland-c4": self._lib.kmvp_wendland_c4_cutoff,
        }.get(kernel)
        if entry is None:
            raise NotImplementedError(f"no cutoff-radius product for kernel {kernel}")
        self._check(entry(self._ctx, float(radius), 1 if normalize_rows else 0))

    def run_cutoff_grad(self, kernel, radius):
        """Gradient of the cutoff-radius product with respect to the targets (include/kmvp.h kmvp_<kernel>_cutoff_grad): the
        plain gradient's terms over the pairs inside ``radius``; read it with get_result(N, E * D)."""
        entry = {
            "gaussian": self._lib.kmvp_gaussian_cutoff_grad,
            "absolute-exponential": self._lib.kmvp_absexp_cutoff_grad,
            "matern-3/2": self._lib.kmvp_matern32_cutoff_grad,
            "matern-5/2": self._lib.kmvp_matern52_cutoff_grad,
            "wendland-c2": self._lib.kmvp_wendland_c2_cutoff_grad,
            "wendland-c4": self._lib.kmvp_wendland_c4_cutoff_grad,
        }.get(kernel)
        if entry is None:
            raise NotImplementedError(f"no cutoff-radius gradient for kernel {kernel}")
        self._check(entry(self._ctx, float(radius)))

    def radius_count(self, radius, exclude_self=False):
        """The number of sources within ``radius`` of every target (include/kmvp.h kmvp_radius_count): (N,) int64, -1 for a
        target with a NaN coordinate.  exclude_self (targets = sources only) leaves a point's own pair out."""
        # the library writes N values through the pointer: the array is sized here, from the points it was given
        counts = np.zeros(int(getattr(self, "N", 0)), dtype=np.int64)
        self._check(self._lib.kmvp_radius_count(self._ctx, float(radius), 1 if exclude_self else 0, counts.ctypes.data))
        return counts

    def radius_nearest(self, radius, K, exclude_self=False):
        """The K nearest sources of every target among those within ``radius`` (include/kmvp.h kmvp_radius_nearest):
        (idx int64 (N, K), sqdist float64 (N, K)), nearest first, ties in ascending index; (-1, +inf) where fewer than K
        sources are inside -- run_nearest()'s rows with every entry beyond radius^2 (in the working precision) emptied."""
        K = int(K)
        N = int(getattr(self, "N", 0))
        # the library writes N * K elements through each pointer: the arrays are sized here, from the points it was given
        idx = np.empty((N, max(K, 0)), dtype=np.int64)
        sqdist = np.empty((N, max(K, 0)), dtype=np.float64)
        self._check(self._lib.kmvp_radius_nearest(self._ctx, float(radius), K, 1 if exclude_self else 0, idx.ctypes.data,
                                                  sqdist.ctypes.data))
        return idx, sqdist

    def dbscan(self, radius, min_samples):
        """DBSCAN of the points among themselves (include/kmvp.h kmvp_dbscan): (labels, core_of, counts, info), three (N,)
        int64 arrays -- the cluster of every point (-1: noise), the core point it belongs to a cluster through (itself for
        a core point, -1 for noise), radius_count()'s counts -- and a dict of n_clusters, n_core, n_border, n_noise, rounds
        and walks."""
        # the library writes N values through each pointer: the arrays are sized here, from the points it was given
        N = int(getattr(self, "N", 0))
        labels, core_of, counts = (np.full(N, -1, dtype=np.int64) for _ in range(3))
        info = np.zeros(6, dtype=np.int64)
        self._check(self._lib.kmvp_dbscan(self._ctx, float(radius), int(min_samples), labels.ctypes.data, core_of.ctypes.data,
                                          counts.ctypes.data, info.ctypes.data))
        names = ("n_clusters", "n_core", "n_border", "n_noise", "rounds", "walks")
        return labels, core_of, counts, {k: int(v) for k, v in zip(names, info)}

    def cutoff_info(self):
        """The plan of the last cutoff call (include/kmvp.h kmvp_cutoff_info): a dict of cells (3 per-axis counts),
        tiles, runs, walked (records walked, summed over the tiles as live lanes x records), records (padded), plan_ms and
        built_on ("host" or "device": the side that built it, kmvp_cutoff_plan_read)."""
        info = np.zeros(8, dtype=np.int64)
        self._check(self._lib.kmvp_cutoff_info(self._ctx, info.ctypes.data))
        sizes = np.zeros(13, dtype=np.int64)
        self._check(self._lib.kmvp_cutoff_plan_read(self._ctx, sizes.ctypes.data, None, None, None, None, None))
        return {"cells": tuple(int(v) for v in info[:3]), "tiles": int(info[3]), "runs": int(info[4]), "walked": int(info[5]),
                "records": int(info[6]), "plan_ms": int(info[7]), "built_on": CUTOFF_PLAN_SIDES[int(sizes[12])]}

    def cutoff_plan(self):
        """The plan of the last cutoff call as the kernels read it (include/kmvp.h kmvp_cutoff_plan_read): the dict of
        tests/cutoff_reference.py plan() -- g (3,), lo (3,), h, n_pad, m_pad, m_alloc, live_tiles, walked, tiles (T, 3)
        [run0, nruns, live], runs (Q, 2) [rec0, len], tmap (n_pad,), smap (m_alloc,) -- and built_on, "host" or "device"."""
        sizes, grid = np.zeros(13, dtype=np.int64), np.zeros(4)
        self._check(self._lib.kmvp_cutoff_plan_read(self._ctx, sizes.ctypes.data, grid.ctypes.data, None, None, None, None))
        # the library writes sizes[8 .. 12) entries through the four pointers: the arrays are sized from its own answer
        tiles, runs = np.zeros((int(sizes[8]), 3), dtype=np.int64), np.zeros((int(sizes[9]), 2), dtype=np.int64)
        tmap, smap = np.zeros(int(sizes[10]), dtype=np.int64), np.zeros(int(sizes[11]), dtype=np.int64)
        self._check(self._lib.kmvp_cutoff_plan_read(self._ctx, None, None, tiles.ctypes.data, runs.ctypes.data, tmap.ctypes.data,
                                                    smap.ctypes.data))
        return dict(g=sizes[:3].copy(), lo=grid[:3].copy(), h=float(grid[3]), n_pad=int(sizes[3]), m_pad=int(sizes[4]),
                    m_alloc=int(sizes[5]), live_tiles=int(sizes[6]), walked=int(sizes[7]), tiles=tiles, runs=runs, tmap=tmap,
                    smap=smap, built_on=CUTOFF_PLAN_SIDES[int(sizes[12])])

    def get_result(self, N, E):
        out = np.empty((N, E), dtype=np.float64)
        self._check(self._lib.kmvp_get_result(self._ctx, out.ctypes.data, out.size))
        return out

    def cg_solve(self, kernel, a, rtol, maxit, support_radius=None):
        """``support_radius``: the Wendland kernels' support radius (include/kmvp.h kmvp_wendland_<c>_cg_solve) -- required
        for them, refused for every other kernel."""
        if a.ndim != 2 or a.shape[0] != getattr(self, "N", a.shape[0]):
            # the Krylov vectors have one row per point (all points are targets); the library reads N * E elements
            raise ValueError(f"target_signal has shape {a.shape}, the point cloud has {self.N} points")
        if (kernel in WENDLAND) != (support_radius is not None):
            raise ValueError(f"kernel {kernel}: support_radius is required for the Wendland kernels and refused for the others")
        entry = {
            "gaussian": self._lib.kmvp_gaussian_cg_solve,
            "absolute-exponential": self._lib.kmvp_absexp_cg_solve,
            "inverse-distance": self._lib.kmvp_invdist_minres_solve,  # indefinite: MINRES
            "matern-3/2": self._lib.kmvp_matern32_cg_solve,
            "matern-5/2": self._lib.kmvp_matern52_cg_solve,
            "wendland-c2": self._lib.kmvp_wendland_c2_cg_solve,
            "wendland-c4": self._lib.kmvp_wendland_c4_cg_solve,
        }.get(kernel)
        if entry is None:
            raise NotImplementedError(f"no solver for kernel {kernel}")
        M, E = a.shape
        out = np.empty((M, E), dtype=np.float64)
        iters = ctypes.c_int(0)
        resid = ctypes.c_double(0.0)
        head = (self._ctx,) if support_radius is None else (self._ctx, float(support_radius))
        rc = entry(*head, a.ctypes.data, E, float(rtol), int(maxit), out.ctypes.data,
                   ctypes.byref(iters), ctypes.byref(resid))
        if rc not in (0, 6):
            self._check(rc)
        return out, iters.value, resid.value, rc == 0

    def lanczos_quadrature(self, kernel, z, rtol, maxit, want_x=False, want_coefficients=False):
        """Stochastic Lanczos quadrature on the probe columns z (N, P) in the context's dtype (include/kmvp.h
        kmvp_<kernel>_lanczos_quadrature).  Returns a dict: logquad, invquad (P float64), steps (P int), converged, and x
        (N, P) / alpha, beta (maxit, P) when asked for; raises on every status but OK and NOT_CONVERGED."""
        entry = {
            "gaussian": self._lib.kmvp_gaussian_lanczos_quadrature,
            "absolute-exponential": self._lib.kmvp_absexp_lanczos_quadrature,
            "matern-3/2": self._lib.kmvp_matern32_lanczos_quadrature,
            "matern-5/2": self._lib.kmvp_matern52_lanczos_quadrature,
        }.get(kernel)
        if entry is None:
            raise NotImplementedError(f"no Lanczos quadrature for kernel {kernel}")
        if z.ndim != 2 or z.shape[0] != getattr(self, "N", z.shape[0]) or not z.flags.c_contiguous:
            # the library reads N * P elements from the pointer: a shorter array must never reach it
            raise ValueError(f"the probes have shape {z.shape}, expected a contiguous ({getattr(self, 'N', '?')}, P) array")
        N, P = z.shape
        maxit = int(maxit)
        logquad, invquad = np.empty(P, dtype=np.float64), np.empty(P, dtype=np.float64)
        steps = np.empty(P, dtype=np.intc)
        x = np.empty((N, P), dtype=np.float64) if want_x else None
        alpha = np.empty((max(maxit, 0), P), dtype=np.float64) if want_coefficients else None
        beta = np.empty((max(maxit, 0), P), dtype=np.float64) if want_coefficients else None
        ptr = lambda a: None if a is None else a.ctypes.data
        rc = entry(self._ctx, z.ctypes.data, P, float(rtol), maxit, logquad.ctypes.data, invquad.ctypes.data,
                   steps.ctypes.data, ptr(x), ptr(alpha), ptr(beta))
        if rc not in (0, 6):
            self._check(rc)
        out = {"logquad": logquad, "invquad": invquad, "steps": steps.astype(np.int64), "converged": rc == 0}
        if want_x:
            out["x"] = x
        if want_coefficients:
            out["alpha"], out["beta"] = alpha, beta
        return out

    def eigsh(self, kernel, k, op, v0, tol, maxit, want_coefficients=False):
        """The k algebraically largest eigenpairs of the kernel matrix (op "kernel"), its centred form ("centered") or its
        degree-normalised form ("normalized") by Lanczos with full reorthogonalisation from the start vector v0 (N
        float64): include/kmvp.h kmvp_<kernel>_eigsh.  Returns a dict: eigenvalues (k), eigenvectors (N, k), resid (k),
        steps, converged, degree (N; "normalized" only) and alpha, beta (maxit) when asked for; raises on every status but
        OK and NOT_CONVERGED."""
        entry = {
            "gaussian": self._lib.kmvp_gaussian_eigsh,
            "absolute-exponential": self._lib.kmvp_absexp_eigsh,
            "matern-3/2": self._lib.kmvp_matern32_eigsh,
            "matern-5/2": self._lib.kmvp_matern52_eigsh,
        }.get(kernel)
        if entry is None:
            raise NotImplementedError(f"no eigen-solver for kernel {kernel}")
        if op not in EIG_OPERATORS:
            raise ValueError(f"operator {op!r}: expected one of {sorted(EIG_OPERATORS)}")
        N = int(getattr(self, "N", 0))
        k, maxit = int(k), int(maxit)
        if v0 is not None:
            # the library reads N doubles from the pointer: anything else must never reach it
            v0 = np.ascontiguousarray(v0, dtype=np.float64)
            if v0.shape != (N,):
                raise ValueError(f"v0 has shape {v0.shape}, expected ({N},): one value per point")
        # the library writes k, N * k and maxit elements: the arrays are sized here, from the points it was given
        eigenvalues = np.full(max(k, 0), np.nan)
        eigenvectors = np.full((N, max(k, 0)), np.nan)
        resid = np.full(max(k, 0), np.nan)
        steps = ctypes.c_int(0)
        alpha = np.full(max(maxit, 0), np.nan) if want_coefficients else None
        beta = np.full(max(maxit, 0), np.nan) if want_coefficients else None
        degree = np.full(N, np.nan) if op == "normalized" else None
        ptr = lambda a: None if a is None else a.ctypes.data
        rc = entry(self._ctx, k, EIG_OPERATORS[op], ptr(v0), float(tol), maxit, eigenvalues.ctypes.data,
                   eigenvectors.ctypes.data, resid.ctypes.data, ctypes.addressof(steps), ptr(alpha), ptr(beta), ptr(degree))
        if rc not in (0, 6):
            self._check(rc)
        out = {"eigenvalues": eigenvalues, "eigenvectors": eigenvectors, "resid": resid, "steps": steps.value,
               "converged": rc == 0}
        if degree is not None:
            out["degree"] = degree
        if want_coefficients:
            out["alpha"], out["beta"] = alpha, beta
        return out

    def lanczos_quadrature_precond(self, kernel, g, h, rtol, maxit, want_x=False, want_pz=False, want_coefficients=False):
        """Preconditioned stochastic Lanczos quadrature (include/kmvp.h kmvp_<kernel>_lanczos_quadrature_precond) on the
        probes z = L h + D^1/2 g formed on the device from g (N, P) and h (rank, P), float64, with ``rank`` what
        set_solver_preconditioner was given (pass it as h's row count).  Returns a dict: logdet_p (float), logquad,
        invquad, wnorm2 (P float64), steps (P int), converged, and x, pz (N, P) / alpha, beta (maxit, P) when asked for;
        raises on every status but OK and NOT_CONVERGED."""
        entry = {
            "gaussian": self._lib.kmvp_gaussian_lanczos_quadrature_precond,
            "absolute-exponential": self._lib.kmvp_absexp_lanczos_quadrature_precond,
            "matern-3/2": self._lib.kmvp_matern32_lanczos_quadrature_precond,
            "matern-5/2": self._lib.kmvp_matern52_lanczos_quadrature_precond,
        }.get(kernel)
        if entry is None:
            raise NotImplementedError(f"no preconditioned Lanczos quadrature for kernel {kernel}")
        # the library reads N * P and (at most) rank * P doubles from the pointers: shorter arrays must never reach it
        g, h = np.asarray(g), np.asarray(h)
        if g.dtype != np.float64 or g.ndim != 2 or g.shape[0] != getattr(self, "N", g.shape[0]) or not g.flags.c_contiguous:
            raise ValueError(f"g has shape {g.shape} and dtype {g.dtype}, expected a contiguous float64 ({getattr(self, 'N', '?')}, P) array")
        N, P = g.shape
        if h.dtype != np.float64 or h.ndim != 2 or h.shape[1] != P or not h.flags.c_contiguous or h.shape[0] > 128:
            raise ValueError(f"h has shape {h.shape} and dtype {h.dtype}, expected a contiguous float64 (rank, {P}) array")
        if h.shape[0] < 128:  # the library reads as many rows as the factor has columns, at most the rank it was given (<= 128)
            h = np.concatenate([h, np.zeros((128 - h.shape[0], P))], axis=0)
        maxit = int(maxit)
        logdet_p = ctypes.c_double(0.0)
        logquad, invquad, wnorm2 = (np.empty(P, dtype=np.float64) for _ in range(3))
        steps = np.empty(P, dtype=np.intc)
        x = np.empty((N, P), dtype=np.float64) if want_x else None
        pz = np.empty((N, P), dtype=np.float64) if want_pz else None
        alpha = np.empty((max(maxit, 0), P), dtype=np.float64) if want_coefficients else None
        beta = np.empty((max(maxit, 0), P), dtype=np.float64) if want_coefficients else None
        ptr = lambda a: None if a is None else a.ctypes.data
        rc = entry(self._ctx, g.ctypes.data, h.ctypes.data, P, float(rtol), maxit, ctypes.addressof(logdet_p),
                   logquad.ctypes.data, invquad.ctypes.data, wnorm2.ctypes.data, steps.ctypes.data, ptr(x), ptr(pz), ptr(alpha),
                   ptr(beta))
        if rc not in (0, 6):
            self._check(rc)
        out = {"logdet_p": logdet_p.value, "logquad": logquad, "invquad": invquad, "wnorm2": wnorm2,
               "steps": steps.astype(np.int64), "converged": rc == 0}
        if want_x:
            out["x"] = x
        if want_pz:
            out["pz"] = pz
        if want_coefficients:
            out["alpha"], out["beta"] = alpha, beta
        return out

    def sinkhorn(self, kernel, log_a, log_b, tol, maxit, u0=None):
        """Sinkhorn iteration on the clouds of set_points (include/kmvp.h kmvp_<kernel>_sinkhorn): log_a (N) / log_b (M)
        float64 log-weights or None (uniform), u0 (N) the starting potential or None (zeros).  Returns
        (u, v, iterations, marginal error, converged); raises on every status but OK and NOT_CONVERGED."""
        entry = {
            "gaussian": self._lib.kmvp_gaussian_sinkhorn,
            "absolute-exponential": self._lib.kmvp_absexp_sinkhorn,
        }.get(kernel)
        if entry is None:
            raise NotImplementedError(f"no Sinkhorn iteration for kernel {kernel}")

        vector = _vector
        N, M = getattr(self, "N", 0), getattr(self, "M", 0)
        log_a, log_b = vector(log_a, N, "log_a"), vector(log_b, M, "log_b")
        u = np.zeros(N, dtype=np.float64) if u0 is None else vector(u0, N, "u0").copy()
        v = np.zeros(M, dtype=np.float64)
        iters = ctypes.c_int(0)
        err = ctypes.c_double(0.0)
        rc = entry(self._ctx, None if log_a is None else log_a.ctypes.data, None if log_b is None else log_b.ctypes.data,
                   float(tol), int(maxit), u.ctypes.data, v.ctypes.data, ctypes.byref(iters), ctypes.byref(err))
        if rc not in (0, 6):
            self._check(rc)
        return u, v, iters.value, err.value, rc == 0

    def sinkhorn_batched(self, kernel, log_a, log_b, tol, maxit, u0=None):
        """One Sinkhorn solve per batch of set_batches (include/kmvp.h kmvp_<kernel>_sinkhorn_batched): log_a (N) / log_b (M)
        float64 log-weights concatenated over the batches or None (uniform within each batch), u0 (N) the starting
        potential or None (zeros).  Returns (u, v, iterations, marginal errors, status) with B values in each of the
        last three (status 1 converged, 2 non-finite, 3 maxit); raises on every return but OK and NOT_CONVERGED."""
        entry = {
            "gaussian": self._lib.kmvp_gaussian_sinkhorn_batched,
            "absolute-exponential": self._lib.kmvp_absexp_sinkhorn_batched,
        }.get(kernel)
        if entry is None:
            raise NotImplementedError(f"no Sinkhorn iteration for kernel {kernel}")
        N, M, B = getattr(self, "N", 0), getattr(self, "M", 0), getattr(self, "B", 0)
        # the library reads N (M) doubles from the pointers and writes B values: a shorter array must never reach it
        log_a, log_b = _vector(log_a, N, "log_a"), _vector(log_b, M, "log_b")
        u = np.zeros(N, dtype=np.float64) if u0 is None else _vector(u0, N, "u0").copy()
        v = np.zeros(M, dtype=np.float64)
        iters = np.zeros(max(B, 1), dtype=np.int32)
        err = np.zeros(max(B, 1), dtype=np.float64)
        status = np.zeros(max(B, 1), dtype=np.int32)
        rc = entry(self._ctx, None if log_a is None else log_a.ctypes.data, None if log_b is None else log_b.ctypes.data,
                   float(tol), int(maxit), u.ctypes.data, v.ctypes.data, iters.ctypes.data, err.ctypes.data, status.ctypes.data)
        if rc not in (0, 6):
            self._check(rc)
        return u, v, iters[:B].astype(np.int64), err[:B], status[:B].astype(np.int64)

    def kmeans(self, C, centroids0, weights, tol, maxit):
        """Lloyd's k-means on the TARGETS of set_points (include/kmvp.h kmvp_kmeans): centroids0 (C, D) float64 initial
        centroids, weights (N) float64 >= 0 or None (every weight 1), tol absolute on sum_c |c_k - c_{k-1}|^2.  Returns
        (centroids, labels, cluster_weight, iterations, inertia, shift, converged); raises on every status but OK and
        NOT_CONVERGED."""
        C = int(C)
        N, D = getattr(self, "N", 0), getattr(self, "D", 0)
        # the library reads C * D and N doubles from the pointers: a shorter array must never reach it
        cent = np.array(centroids0, dtype=np.float64, order="C", ndmin=2)  # a copy: written in place by the library
        if C >= 1 and cent.shape != (C, D):  # (C < 1 is refused by the library before it reads anything)
            raise ValueError(f"the initial centroids have shape {cent.shape}, expected ({C}, {D})")
        if weights is not None:
            weights = np.ascontiguousarray(weights, dtype=np.float64)
            if weights.shape != (N,):
                raise ValueError(f"weights has shape {weights.shape}, expected ({N},)")
        labels = np.full(N, -1, dtype=np.int64)
        cluster_weight = np.zeros(max(C, 0), dtype=np.float64)
        iters = ctypes.c_int(0)
        inertia, shift = ctypes.c_double(0.0), ctypes.c_double(0.0)
        rc = self._lib.kmvp_kmeans(self._ctx, C, None if weights is None else weights.ctypes.data, float(tol), int(maxit),
                                   cent.ctypes.data, labels.ctypes.data, cluster_weight.ctypes.data, ctypes.byref(iters),
                                   ctypes.byref(inertia), ctypes.byref(shift))
        if rc not in (0, 6):
            self._check(rc)
        return cent, labels, cluster_weight, iters.value, inertia.value, shift.value, rc == 0

    def meanshift(self, tol, maxit):
        """Gaussian mean-shift of the TARGETS of set_points over the sources, the signal read as one column of log-weights
        (include/kmvp.h kmvp_gaussian_meanshift).  Returns a dict: modes (N, D) float64, iters (N) int64, step2 (N) float64,
        sweeps, target_sweeps, converged; raises on every status but OK and NOT_CONVERGED."""
        N, D = int(getattr(self, "N", 0)), int(getattr(self, "D", 0))
        # the library writes N * D, N and N elements through the pointers: the arrays are sized here, from the points it was given
        modes = np.full((N, D), np.nan, dtype=np.float64)
        iters = np.zeros(N, dtype=np.intc)
        step2 = np.full(N, np.nan, dtype=np.float64)
        sweeps = ctypes.c_int(0)
        target_sweeps = ctypes.c_int64(0)
        rc = self._lib.kmvp_gaussian_meanshift(self._ctx, float(tol), int(maxit), modes.ctypes.data, iters.ctypes.data,
                                               step2.ctypes.data, ctypes.byref(sweeps), ctypes.byref(target_sweeps))
        if rc not in (0, 6):
            self._check(rc)
        return {"modes": modes, "iters": iters.astype(np.int64), "step2": step2, "sweeps": sweeps.value,
                "target_sweeps": target_sweeps.value, "converged": rc == 0}

    def set_solver_diagonal(self, d_or_none, ridge=0.0):
        """A = K + ridge I + diag(d) for the solves that follow (include/kmvp.h kmvp_set_solver_diagonal); d: one float64
        value per point (the FULL vector, also on a source shard) or None.  (None, 0.0) switches it off; set_points
        clears it."""
        if d_or_none is None:
            self._check(self._lib.kmvp_set_solver_diagonal(self._ctx, None, 0, float(ridge)))
            return
        d = np.ascontiguousarray(d_or_none, dtype=np.float64)
        if d.ndim != 1:  # the library reads d.size doubles and compares the count with the points at solve time
            raise ValueError(f"the solver diagonal has shape {d.shape}, expected one value per point")
        self._check(self._lib.kmvp_set_solver_diagonal(self._ctx, d.ctypes.data, d.size, float(ridge)))

    def set_solver_preconditioner(self, rank):
        """Pivoted-Cholesky preconditioner of rank ``rank`` for the cg_solve calls that follow (include/kmvp.h
        kmvp_set_solver_preconditioner); 0 switches it off, set_points clears it."""
        self._check(self._lib.kmvp_set_solver_preconditioner(self._ctx, int(rank)))

    def get_solver_preconditioner(self):
        """What the last cg_solve applied (include/kmvp.h kmvp_get_solver_preconditioner): (rank_built, pivots int64
        (rank_built,), factor float64 (rank_built, N), row t = column t of L); (0, empty, empty) when it ran
        unpreconditioned."""
        built = ctypes.c_int(0)
        self._check(self._lib.kmvp_get_solver_preconditioner(self._ctx, ctypes.byref(built), None, None))
        # the library writes rank_built and rank_built * N elements through the pointers: the arrays are sized from its answer
        pivots = np.empty(built.value, dtype=np.int64)
        factor = np.empty((built.value, int(getattr(self, "N", 0))), dtype=np.float64)
        if built.value:
            self._check(self._lib.kmvp_get_solver_preconditioner(self._ctx, ctypes.byref(built), pivots.ctypes.data,
                                                                 factor.ctypes.data))
        return built.value, pivots, factor

    @property
    def last_preconditioner_rank(self):
        """Columns of the factor the last cg_solve applied (0: it ran unpreconditioned), without reading the factor."""
        built = ctypes.c_int(0)
        self._check(self._lib.kmvp_get_solver_preconditioner(self._ctx, ctypes.byref(built), None, None))
        return built.value

    @property
    def last_preconditioner_ms(self):
        return float(self._lib.kmvp_last_preconditioner_ms(self._ctx))

    def comm_init(self, unique_id, rank, world):
        buf = (ctypes.c_char * UNIQUE_ID_BYTES).from_buffer_copy(unique_id)
        self._check(self._lib.kmvp_comm_init(self._ctx, buf, int(rank), int(world)))
        self.comm_world = int(world)  # attachment is recorded on the context itself (sharding.Communicator.attach)

    def comm_init_host(self, allreduce, rank, world):
        """REHEARSAL transport (include/kmvp.h kmvp_comm_init_host): ``allreduce(array, op)`` must reduce a float64
        numpy array in place over all ranks (op: OP_SUM or OP_MIN).  The library stages the exchange buffer through
        host memory and calls it."""

        def trampoline(_user, buf, count, op):
            try:
                allreduce(np.ctypeslib.as_array(buf, shape=(int(count),)), int(op))
                return 0
            except Exception as e:  # never let a Python exception cross the C frame
                self._host_error = e
                return 1

        self._host_cb = HOST_ALLREDUCE_FN(trampoline)  # kept alive as long as the context
        self._check(self._lib.kmvp_comm_init_host(self._ctx, ctypes.cast(self._host_cb, ctypes.c_void_p), None,
                                                  int(rank), int(world)))
        self.comm_world = int(world)

    @property
    def rccl_ranks(self):
        """Ranks the attached communicator itself reports (1 without one)."""
        return int(self._lib.kmvp_comm_world(self._ctx))

    @property
    def last_allreduce_ms(self):
        return float(self._lib.kmvp_last_allreduce_ms(self._ctx))

    def set_option(self, key, value):
        if key in REAL_OPTIONS:
            self._check(self._lib.kmvp_set_option_double(self._ctx, key.encode(), float(value)))
            return
        self._check(self._lib.kmvp_set_option(self._ctx, key.encode(), int(value)))

    @property
    def device_bytes(self):
        return int(self._lib.kmvp_device_bytes(self._ctx))

    @property
    def last_kernel_ms(self):
        return float(self._lib.kmvp_last_kernel_ms(self._ctx))

    @property
    def last_total_ms(self):
        return float(self._lib.kmvp_last_total_ms(self._ctx))

    @property
    def last_kernel_name(self):
        return self._lib.kmvp_last_kernel_name(self._ctx).decode()

    @property
    def last_dispatch_note(self):
        return self._lib.kmvp_last_dispatch_note(self._ctx).decode()

    def cell_layout(self):
        """The cell layout of the last product on the cell form (include/kmvp.h kmvp_cell_layout), read-only: a dict of
        source_cell (M,) and target_cell (N,) int32 (an index into the centres; -1: in no tile, -2: in more than one),
        source_centres and target_centres (cells, 3) float64, count_cut, tiles_per_wavefront, tile_points, image (0
        cell_kernel, 1 cellmm_kernel / cellmm16_kernel, 2 cell64_kernel), main_tiles, rest_tiles and sigma_b."""
        if not self._ctx:
            raise ValueError("the context is closed")
        info = np.zeros(8, dtype=np.int64)
        sigma = ctypes.c_double(0.0)
        self._check(self._lib.kmvp_cell_layout(self._ctx, info.ctypes.data, ctypes.byref(sigma), None, None, None, 0, None, 0))
        ns, nt = int(info[0]), int(info[1])
        scell, tcell = np.empty(self.M, dtype=np.int32), np.empty(self.N, dtype=np.int32)
        scen, tcen = np.empty((max(ns, 1), 3)), np.empty((max(nt, 1), 3))
        self._check(self._lib.kmvp_cell_layout(self._ctx, info.ctypes.data, ctypes.byref(sigma), scell.ctypes.data,
                                               tcell.ctypes.data, scen.ctypes.data, ns, tcen.ctypes.data, nt))
        return {"source_cell": scell, "target_cell": tcell, "source_centres": scen[:ns], "target_centres": tcen[:nt],
                "count_cut": bool(info[2]), "tiles_per_wavefront": int(info[3]), "tile_points": int(info[4]),
                "image": int(info[5]), "main_tiles": int(info[6]), "rest_tiles": int(info[7]), "sigma_b": float(sigma.value)}

    def cell_lists(self):
        """The lists of target tiles of the last product on cellmm_kernel / cellmm16_kernel (include/kmvp.h kmvp_cell_lists),
        read-only: a dict of blocks and segments (MAIN, TAIL, REST), resident, fused and target_list (N,) int32 (0 MAIN, 1
        REST, 2 TAIL)."""
        if not self._ctx:
            raise ValueError("the context is closed")
        info = np.zeros(8, dtype=np.int64)
        lists = np.empty(self.N, dtype=np.int32)
        self._check(self._lib.kmvp_cell_lists(self._ctx, info.ctypes.data, lists.ctypes.data))
        return {"blocks": tuple(int(v) for v in info[0:3]), "segments": tuple(int(v) for v in info[3:6]),
                "resident": int(info[6]), "fused": bool(info[7]), "target_list": lists}


def comm_unique_id():
    buf = ctypes.create_string_buffer(UNIQUE_ID_BYTES)
    rc = load().kmvp_comm_get_unique_id(buf)
    if rc != 0:
        msg = load().kmvp_last_error(None)
        raise KmvpError(rc, msg.decode() if msg else "")
    return bytes(buf.raw)


def device_count():
    n = load().kmvp_device_count()
    return max(0, n)
