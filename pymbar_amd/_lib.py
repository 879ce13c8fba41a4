"""ctypes binding of libmbar_hip.so (include/mbar_hip.h), and the argument layer every Python face of it goes through: ``f64`` and
``labels_i32`` give an array its dtype, layout and checked shape before it crosses the ABI, ``ptr`` casts it, ``check`` reads the
return code.

The product path has exactly one compute backend -- the gfx950 library.  If it cannot be loaded,
or no MI355X is visible, every entry point raises :class:`BackendUnavailable`; there is no CPU
fallback (the numpy oracle under ``oracle/`` is test infrastructure and is never imported here).
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MBAR_HIP_LIBRARY") or os.path.join(HERE, "csrc", "libmbar_hip.so")  # (override: A/B builds)

MBAR_OK = 0
MBAR_ERR_ARG = -1  # the caller's input was bad
EVAL_GRAM = 1
EVAL_USE_OFFSET = 2
TIMER_LSE, TIMER_GRAM, TIMER_REDUCE, TIMER_OTHER, TIMER_FUSED, TIMER_NEWTON, TIMER_COMM = 0, 1, 2, 3, 4, 5, 6


class BackendUnavailable(RuntimeError):
    """libmbar_hip.so is missing / not loadable, or there is no gfx950 device."""


class MbarHipError(RuntimeError):
    """A libmbar_hip call returned an error code."""

    def __init__(self, code, message):
        super().__init__(f"libmbar_hip error {code}: {message}")
        self.code = code


class BarState(C.Structure):
    """``mbar_bar_state`` of include/mbar_hip.h: one problem's BAR root find."""
    _fields_ = [(n, C.c_double) for n in ("DeltaF", "DeltaF_old", "DeltaF_initial", "UpperB", "LowerB", "FUpperB", "FLowerB", "FNew",
                                          "relative_change", "relative_tolerance")] + [
        ("req", C.c_double * 2), ("moments", C.c_double * 4)] + [
        (n, C.c_int64) for n in ("method", "iterated", "maximum_iterations", "iteration", "phase", "status", "nreq", "nzero",
                                 "want_moments", "moments_pending")]


MBAR_BATCH_MAX_K = 64
MBAR_BATCH_CHUNK = 256
MBAR_BATCH_MAX_AUG = 128
MBAR_BATCH_EXT_RUN = 4


class BatchState(C.Structure):
    """``mbar_batch_state`` of include/mbar_hip.h: one problem's adaptive loop in ``mbar_batch``."""
    _fields_ = [(n, C.c_double * MBAR_BATCH_MAX_K) for n in ("f",)] + [("req", (C.c_double * MBAR_BATCH_MAX_K) * 2)] + [
        (n, C.c_double * MBAR_BATCH_MAX_K) for n in ("lognum", "psum", "Nk", "x")] + [
        (n, C.c_double) for n in ("tol", "gamma", "max_delta", "max_diff", "gnorm_sci", "gnorm_nr")] + [
        (n, C.c_int64) for n in ("K", "maxiter", "min_sc_iter", "iterations", "nr_iter", "sci_iter", "choices", "phase", "status",
                                 "success", "nreq", "gram_req", "gram_w", "newton_bad")]


class SolveResult(C.Structure):
    _fields_ = [
        ("iterations", C.c_int64),
        ("nr_iter", C.c_int64),
        ("sci_iter", C.c_int64),
        ("success", C.c_int32),
        ("gram_sweeps", C.c_int32),
        ("max_delta", C.c_double),
        ("gnorm", C.c_double),
        ("wall_ms", C.c_double),
        ("warm_starts", C.c_int32),
        ("builds", C.c_int32),
        ("light_sweeps", C.c_int32),
        ("fused_unit", C.c_int32),
    ]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.POINTER(C.c_double), C.c_int64, C.c_int, C.c_void_p)

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int64)
_i32p = C.POINTER(C.c_int32)
_u64p = C.POINTER(C.c_uint64)
_ctx = C.c_void_p

# name -> (restype, argtypes); this table is also what tests/test_capi_symbols.py checks against
# the declarations in include/mbar_hip.h
SIGNATURES = {
    "mbar_version": (C.c_int, []),
    "mbar_last_error": (C.c_char_p, [_ctx]),
    "mbar_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "mbar_device_info": (C.c_int, [C.c_int, C.c_char_p, C.c_int, C.POINTER(C.c_int), _ip]),
    "mbar_ctx_create": (C.c_int, [C.POINTER(_ctx), C.c_int, C.c_int64, C.c_int64]),
    "mbar_ctx_destroy": (None, [_ctx]),
    "mbar_ctx_synchronize": (C.c_int, [_ctx]),
    "mbar_device_synchronize": (C.c_int, [C.c_int]),
    "mbar_cache_trim": (C.c_int, []),
    "mbar_host_digest": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_uint64)]),
    "mbar_host_newton_direction": (C.c_int, [_dp, _dp, C.c_int, C.c_int, _dp]),
    "mbar_ctx_set_option": (C.c_int, [_ctx, C.c_char_p, C.c_int64]),
    "mbar_ctx_upload_u": (C.c_int, [_ctx, _dp, C.c_int64, C.c_int64, C.c_int64, C.c_int64]),
    "mbar_ctx_download_u": (C.c_int, [_ctx, _dp, C.c_int64]),
    "mbar_ctx_upload_rows": (C.c_int, [_ctx, C.c_int64, C.c_int64, _dp, C.c_int64]),
    "mbar_ctx_copy_rows": (C.c_int, [_ctx, C.c_int64, _ctx, C.c_int64, C.c_int64]),
    "mbar_ctx_row_sub": (C.c_int, [_ctx, C.c_int64, _dp]),
    "mbar_ctx_rows_sub": (C.c_int, [_ctx, C.c_int64, C.c_int64, C.c_int64, _dp]),
    "mbar_ctx_rows_rsub": (C.c_int, [_ctx, C.c_int64, C.c_int64, C.c_int64]),
    "mbar_ctx_rows_logshift": (C.c_int, [_ctx, C.c_int64, C.c_int64, _dp]),
    "mbar_ctx_vec_logshift": (C.c_int, [_ctx, _dp, _dp]),
    "mbar_ctx_fill_masked_rows": (C.c_int, [_ctx, C.c_int64, C.c_int64, _dp, C.POINTER(C.c_int32)]),
    "mbar_ctx_fill_linear_rows": (C.c_int, [_ctx, C.c_int64, C.c_int64, C.c_int64, _dp, C.c_int64, C.c_int64, _dp, _dp]),
    "mbar_ctx_fill_family_rows": (C.c_int, [_ctx, C.c_int64, C.c_int64, C.c_int64, _dp, C.c_int64, C.c_int64, _dp, _dp, _dp,
                                            C.POINTER(C.c_int32), _dp]),
    "mbar_ctx_generate_harmonic": (C.c_int, [_ctx, C.c_uint64, _dp, _dp, _ip, C.c_int64]),
    "mbar_ctx_set_Nk": (C.c_int, [_ctx, _dp]),
    "mbar_ctx_set_sample_weights": (C.c_int, [_ctx, _dp]),
    "mbar_ctx_weights_from_vec": (C.c_int, [_ctx, C.c_double]),
    "mbar_ctx_draw_bootstrap_weights": (C.c_int, [_ctx, C.c_uint64, C.c_int64, _ip, C.c_int64, _ip, C.c_int64]),
    "mbar_ctx_set_bootstrap_layout": (C.c_int, [_ctx, _ip, C.c_int64, _ip]),
    "mbar_bootstrap_draws": (C.c_int, [C.c_uint64, C.c_int64, _ip, C.c_int64, _ip, _ip]),
    "mbar_comm_unique_id": (C.c_int, [C.c_void_p]),
    "mbar_ctx_comm_init": (C.c_int, [_ctx, C.c_void_p, C.c_int, C.c_int]),
    "mbar_ctx_set_host_allreduce": (C.c_int, [_ctx, ALLREDUCE_FN, C.c_void_p, C.c_int, C.c_int]),
    "mbar_ctx_comm_destroy": (C.c_int, [_ctx]),
    "mbar_loopback_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int]),
    "mbar_loopback_destroy": (None, [C.c_void_p]),
    "mbar_ctx_set_loopback": (C.c_int, [_ctx, C.c_void_p, C.c_int]),
    "mbar_eval": (C.c_int, [_ctx, _dp, C.c_int, C.c_uint, _dp, _dp, _dp]),
    "mbar_ctx_set_objective_offset": (C.c_int, [_ctx, _dp]),
    "mbar_lognum": (C.c_int, [_ctx, _dp, _dp]),
    "mbar_logden": (C.c_int, [_ctx, _dp, _dp]),
    "mbar_logw": (C.c_int, [_ctx, _dp, _dp, C.c_int64]),
    "mbar_w": (C.c_int, [_ctx, _dp, _dp, C.c_int64]),
    "mbar_gram_w": (C.c_int, [_ctx, _dp, _dp, _dp]),
    "mbar_ctx_set_bins": (C.c_int, [_ctx, C.c_int64, C.POINTER(C.c_int32), _dp]),
    "mbar_ctx_bins_info": (C.c_int, [_ctx, _ip, _ip, _ip]),
    "mbar_bin_lognum": (C.c_int, [_ctx, _dp, _dp]),
    "mbar_bin_gram_w": (C.c_int, [_ctx, _dp, _dp, _dp, _dp, _dp]),
    "mbar_ctx_set_scan": (C.c_int, [_ctx, C.c_int64, _dp, C.c_int64, _dp]),
    "mbar_scan_lognum": (C.c_int, [_ctx, _dp, C.c_int64, _dp, _dp, _dp, _dp]),
    "mbar_scan_gram_w": (C.c_int, [_ctx, _dp, C.c_int64, _dp, _dp, _dp, C.c_int64, _dp, _dp, _dp, _dp]),
    "mbar_scan_energy_lognum": (C.c_int, [_ctx, _dp, C.c_int64, _dp, _dp, _dp, C.c_int64, _dp, _dp]),
    "mbar_scan_energy_gram_w": (C.c_int, [_ctx, _dp, C.c_int64, _dp, _dp, _dp, C.c_int64, _dp, C.c_int64, _dp, _dp, _dp, _dp]),
    "mbar_scan_pair_gram": (C.c_int, [_ctx, _dp, C.c_int64, _dp, _dp, _dp, C.c_int64, _ip, _dp]),
    "mbar_scan_moments": (C.c_int,[_ctx, _dp, C.c_int64, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "mbar_ctx_set_scan_obs": (C.c_int, [_ctx, C.c_int64, _dp, C.c_int64]),
    "mbar_scan_obs_sums": (C.c_int, [_ctx, _dp, C.c_int64, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp]),
    "mbar_ctx_set_scan_points": (C.c_int, [_ctx, C.c_int64, _dp, C.c_int64]),
    "mbar_scan_kde_sums": (C.c_int, [_ctx, _dp, C.c_int64, _dp, _dp, _dp, C.c_int64, _dp, C.c_double, _dp, _dp, _dp, _ip]),
    "mbar_ctx_set_scan_terms": (C.c_int, [_ctx, C.POINTER(C.c_int32), _dp]),
    "mbar_ctx_set_scan_centers": (C.c_int, [_ctx, C.c_int64, _dp]),
    "mbar_ctx_set_scan_bins": (C.c_int, [_ctx, C.c_int64, C.POINTER(C.c_int32)]),
    "mbar_scan_bins_table": (C.c_int, [C.c_int64, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _ip]),
    "mbar_scan_bin_lognum": (C.c_int, [_ctx, _dp, C.c_int64, _dp, _dp, _dp]),
    "mbar_scan_bin_gram_w": (C.c_int, [_ctx, _dp, C.c_int64, _dp, _dp, _dp, _dp, _dp, _dp]),
    "mbar_ctx_create_ext": (C.c_int, [C.POINTER(_ctx), _ctx, C.c_int64]),
    "mbar_ctx_rows_sub_from": (C.c_int, [_ctx, C.c_int64, _ctx, C.c_int64, C.c_int64, _dp]),
    "mbar_ctx_rows_rsub_from": (C.c_int, [_ctx, C.c_int64, _ctx, C.c_int64, C.c_int64]),
    "mbar_ctx_rows_obs_from": (C.c_int, [_ctx, C.c_int64, _ctx, C.c_int64, C.c_int64, C.c_int64, _dp, _dp, _dp]),
    "mbar_lognum_ext": (C.c_int, [_ctx, _ctx, _dp, _dp]),
    "mbar_gram_w_ext": (C.c_int, [_ctx, _ctx, _dp, _dp, _dp, _dp, _dp]),
    "mbar_solve_adaptive": (C.c_int, [_ctx, _dp, C.c_double, C.c_int64, C.c_int64, C.c_double, C.c_int,
                                      _dp, C.c_int64, C.POINTER(SolveResult)]),
    "mbar_ctx_last_solve_psum": (C.c_int, [_ctx, _dp]),
    "mbar_solve_sci": (C.c_int, [_ctx, _dp, C.c_double, C.c_int64, C.c_int, C.POINTER(SolveResult)]),
    "mbar_ctx_timing": (C.c_int, [_ctx, C.c_int, _dp, _ip]),
    "mbar_ctx_timing_reset": (C.c_int, [_ctx]),
    "mbar_mfma_f64_peak": (C.c_int, [_ctx, _dp]),
    "mbar_kde_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int64, _dp, C.c_double]),
    "mbar_kde_destroy": (None, [C.c_void_p]),
    "mbar_kde_set_weights": (C.c_int, [C.c_void_p, C.c_int64, _dp]),
    "mbar_kde_eval": (C.c_int, [C.c_void_p, C.c_int64, _dp, _dp]),
    "mbar_kde_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int64]),
    "mbar_kde_log_norm":(C.c_int, [C.c_int, C.c_int, C.c_double, _dp]),
    "mbar_acf_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int64, _dp, _dp, C.c_int64, _ip, C.c_double, C.c_double]),
    "mbar_acf_destroy": (None, [C.c_void_p]),
    "mbar_acf_suffix_g": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int, _dp, _ip, C.POINTER(C.c_int32)]),
    "mbar_acf_multiple_g": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, _dp, _ip, C.POINTER(C.c_int32), C.c_int64, _dp]),
    "mbar_acf_schedule_length": (C.c_int, [C.c_int, C.c_int64, _ip]),
    "mbar_acf_lag_sums": (C.c_int, [C.c_void_p, C.c_int64, _ip, C.c_int64, _ip, C.c_int, _dp, _dp]),
    "mbar_bar_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int64, _ip, _dp, _ip, _dp]),
    "mbar_bar_destroy": (None, [C.c_void_p]),
    "mbar_bar_zero": (C.c_int, [C.c_void_p, _dp, _dp]),
    "mbar_bar_solve": (C.c_int, [C.c_void_p, C.POINTER(BarState), _ip]),
    "mbar_bar_moments": (C.c_int, [C.c_void_p, _dp]),
    "mbar_bar_step_host": (C.c_int, [C.POINTER(BarState), _dp]),
    "mbar_bspline_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int64, _dp]),
    "mbar_bspline_destroy": (None, [C.c_void_p]),
    "mbar_bspline_set_groups": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_int32)]),
    "mbar_bspline_set_weights": (C.c_int, [C.c_void_p, C.c_int64, _dp]),
    "mbar_bspline_moments": (C.c_int, [C.c_void_p, C.c_int, C.c_int, _dp, _dp]),
    "mbar_bspline_kernel_ms": (C.c_int, [C.c_void_p, _dp]),
    "mbar_batch_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.c_int64, _ip, _ip, C.POINTER(_dp)]),
    "mbar_batch_destroy": (None, [C.c_void_p]),
    "mbar_batch_solve": (C.c_int, [C.c_void_p, C.POINTER(BatchState), _ip]),
    "mbar_batch_gram_w": (C.c_int, [C.c_void_p, _dp, C.POINTER(C.c_int32), _dp, _dp]),
    "mbar_batch_step_host": (C.c_int, [C.POINTER(BatchState), _dp, _dp]),
    "mbar_batch_set_replicas": (C.c_int, [C.c_void_p, C.c_int64, _ip, _ip]),
    "mbar_batch_replica_set_weights": (C.c_int, [C.c_void_p, C.c_int64, _dp]),
    "mbar_batch_replicas_draw": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.POINTER(C.c_uint64), _ip]),
    "mbar_batch_replicas_solve": (C.c_int, [C.c_void_p, C.POINTER(BatchState), _ip]),
    "mbar_batch_replicas_gram_w": (C.c_int, [C.c_void_p, _dp, C.POINTER(C.c_int32), _dp, _dp]),
    "mbar_batch_set_ext": (C.c_int, [C.c_void_p, _ip, C.POINTER(_dp)]),
    "mbar_batch_ext_lognum": (C.c_int, [C.c_void_p, _dp, C.POINTER(C.c_int32), _dp]),
    "mbar_batch_ext_gram": (C.c_int, [C.c_void_p, _dp, _dp, C.POINTER(C.c_int32), C.c_int64, _dp, _dp]),
}

_lib = None


def load_library():
    """Load libmbar_hip.so and attach signatures.  Does not touch the GPU."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BackendUnavailable(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  pymbar_amd has no CPU fallback.")
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as exc:  # pragma: no cover - depends on the ROCm install
        raise BackendUnavailable(f"cannot load {LIB_PATH}: {exc}") from exc
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def last_error(ctx=None):
    msg = load_library().mbar_last_error(ctx)
    return msg.decode("utf-8", "replace") if msg else ""


def check(code, ctx=None, arg_error=None):
    """Raise unless ``code`` is MBAR_OK: ``arg_error(message)`` for MBAR_ERR_ARG where the caller names one (the inputs were
    bad), :class:`MbarHipError` for everything else."""
    if code != MBAR_OK:
        if code == MBAR_ERR_ARG and arg_error is not None:
            raise arg_error(last_error(ctx))
        raise MbarHipError(code, last_error(ctx))


def host_digest(a, threads=0):
    """16-byte digest of every byte of a C-contiguous numpy array (``mbar_host_digest``; host only, no GPU needed)."""
    out = (C.c_uint64 * 2)()
    check(load_library().mbar_host_digest(C.c_void_p(a.ctypes.data), a.nbytes, int(threads), out))
    return bytes(out)


def bootstrap_draws(seed, replicate, cumN, order=None):
    """The draws of replicate ``replicate`` of the counter-based bootstrap stream ``seed`` as the reference's ``bootstrap_rints`` row
    (``mbar_bootstrap_draws``; host only, no GPU needed): ``rints[sample of slot j] = sample drawn``, state by state."""
    cumN = np.ascontiguousarray(cumN, dtype=np.int64)
    out = np.zeros(int(cumN[-1]), dtype=np.int64)
    order = None if order is None else np.ascontiguousarray(order, dtype=np.int64)
    check(load_library().mbar_bootstrap_draws(C.c_uint64(int(seed)), int(replicate), ptr(cumN, _ip), len(cumN) - 1, ptr(order, _ip),
                                              ptr(out, _ip)))
    return out


def host_newton_direction(H, g, threads=0):
    """``x = H^+ g - (H^+ g)[0]`` as the host-driven adaptive loop computes it (``mbar_host_newton_direction``; host only).
    ``threads > 0`` forces the blocked, threaded Cholesky factorisation with that team size (tests)."""
    g = f64(g, (None,), "g")
    m = g.shape[0]
    H = f64(H, (m, m), "H")
    x = np.empty(m, dtype=np.float64)
    check(load_library().mbar_host_newton_direction(ptr(H), ptr(g), m, int(threads), ptr(x)))
    return x


def trim_device_cache():
    """Hand every device / pinned block this library has parked for re-use back to the driver (``mbar_cache_trim``; the bound
    of the cache is ``MBAR_CACHE_MB``, see include/mbar_hip.h)."""
    check(load_library().mbar_cache_trim())


def device_count():
    lib = load_library()
    n = C.c_int(0)
    rc = lib.mbar_device_count(C.byref(n))
    return n.value if rc == MBAR_OK else 0


def require_device():
    """Raise BackendUnavailable unless a gfx950 GPU can be used."""
    if device_count() < 1:
        raise BackendUnavailable(
            "no HIP device visible: pymbar_amd computes only on an MI355X (gfx950) through "
            "libmbar_hip.so and has no CPU fallback")


def default_device(device=None):
    """``device``, or this process's GPU when it is None: the local rank modulo the visible devices."""
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0")) % max(1, device_count())
    return int(device)


def ptr(a, t=_dp):
    """ctypes pointer to the data of a numpy array (None for None)."""
    return a.ctypes.data_as(t) if a is not None else None


def _shape_text(shape):
    return "(" + ", ".join("*" if s is None else str(s) for s in shape) + ("," if len(shape) == 1 else "") + ")"


def f64(a, shape, name, error=ValueError, optional=False):
    """``a`` as a C-contiguous float64 array of shape ``shape`` (a tuple; ``None`` matches any extent), or ``error``.  An array that
    conforms already comes back as it is, without a copy.  ``None`` stays ``None`` with ``optional`` and is refused otherwise."""
    if a is None:
        if optional:
            return None
        raise error(f"{name} is required")
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.shape != shape and (a.ndim != len(shape) or any(s is not None and s != n for s, n in zip(shape, a.shape))):
        raise error(f"{name} must have shape {_shape_text(shape)}")
    return a


def labels_i32(label_n, nbins, n, name):
    """The ``n`` bin labels of the resident samples as a contiguous int32 array: every label in ``[-1, nbins)`` (-1: in no bin).
    Another dtype is range-checked before it is narrowed: a value that does not fit an int32 would wrap into the valid range."""
    label_n = np.asarray(label_n)
    if label_n.shape != (n,):
        raise ValueError(f"{name} must have shape ({n},)")
    if label_n.dtype != np.int32:
        if label_n.size and (label_n.min() < -1 or label_n.max() >= int(nbins)):
            raise ValueError("labels must lie in [-1, nbins)")
        label_n = label_n.astype(np.int32)
    return np.ascontiguousarray(label_n)


class Handle:
    """Owner of one library handle ``_h``: released by ``close``, at the end of a ``with`` block or when collected.
    Subclasses name the library function that releases it in ``_destroy``."""

    _destroy = None
    _h = None

    def close(self):
        if self._h:
            getattr(self._lib, self._destroy)(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
