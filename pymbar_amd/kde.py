"""Weighted kernel-density estimates on the MI355X: the ``fes_type="kde"`` path of ``pymbar.FES`` (pymbar/fes.py:602-699,
1523-1609), which in the reference is ``sklearn.neighbors.KernelDensity(...).fit(x_n, sample_weight=w_n).score_samples(x)``.

:class:`KernelDensity` is a device-backed subset of sklearn's estimator (same parameters, same ``score_samples``), and does not
need sklearn.  The sum behind it runs in ``csrc/libmbar_hip.so`` (``mbar_kde_*`` of include/mbar_hip.h, kernels in
``csrc/mbar_k_kde.hip``): every (query, sample) pair, in log space, so the result is the exact weighted log density -- also
where sklearn's tree is not (d >= 2 in sparse regions) and where every kernel term underflows (gaussian / exponential far from
the data).  ``algorithm``, ``leaf_size``, ``breadth_first``, ``atol`` and ``rtol`` are accepted and have no effect.

:meth:`KernelDensity.score_samples_columns` evaluates several weight columns over the same samples in one device call -- the
bootstrap replicates of a KDE free energy surface (pymbar_amd.fes.FES).
"""
import ctypes as C

import numpy as np

from . import _lib
from .utils import ParameterError

KERNELS = ("gaussian", "tophat", "epanechnikov", "exponential", "linear", "cosine")
_KERNEL_ID = {"gaussian": 0, "tophat": 1, "epanechnikov": 2, "exponential": 3, "linear": 4, "cosine": 5}  # MBAR_KDE_*
MAX_DIM = 8
# the constructor parameters of sklearn.neighbors.KernelDensity (what get_params returns)
SKLEARN_PARAMS = ("algorithm", "atol", "bandwidth", "breadth_first", "kernel", "leaf_size", "metric", "metric_params", "rtol")


def log_normaliser(kernel, d, bandwidth):
    """``log(1 / integral of k_h over R^d)``, the constant the library adds (``mbar_kde_log_norm``; host only, no GPU needed)."""
    out = C.c_double(0.0)
    _lib.check(_lib.load_library().mbar_kde_log_norm(_KERNEL_ID[kernel], int(d), float(bandwidth), C.byref(out)))
    return out.value


class DeviceKDE(_lib.Handle):
    """N samples of dimension d resident on one device with C columns of sample weights (an ``mbar_kde`` handle).

    ``log_density(Q)[m, c] = log sum_n V[n, c] k_h(|Q_m - X_n|) - log sum_n V[n, c] + log-normaliser``."""

    _destroy = "mbar_kde_destroy"

    def __init__(self, X, kernel, bandwidth, device=None):
        _lib.require_device()
        self._lib = _lib.load_library()
        X = _lib.f64(X, (None, None), "X")
        self.n_samples, self.dim = X.shape
        self.device = _lib.default_device(device)
        self._h = C.c_void_p()
        _lib.check(self._lib.mbar_kde_create(C.byref(self._h), self.device, _KERNEL_ID[kernel], self.dim, self.n_samples, _lib.ptr(X),
                                             float(bandwidth)))
        self.n_columns = 1

    def set_weights(self, V):
        """V: (N,) or (N, C), finite and non-negative."""
        V = np.asarray(V, dtype=np.float64)
        V = _lib.f64(V[:, None] if V.ndim == 1 else V, (self.n_samples, None), "V")
        _lib.check(self._lib.mbar_kde_set_weights(self._h, V.shape[1], _lib.ptr(V)))
        self.n_columns = V.shape[1]

    def set_option(self, key, value):
        """``mbar_kde_set_option``: ``"max_chunks"`` caps the number of sample chunks of the next calls (0: the default cut)."""
        _lib.check(self._lib.mbar_kde_set_option(self._h, key.encode(), int(value)))

    def log_density(self, Q):
        Q = _lib.f64(Q, (None, self.dim), "Q")
        out = np.empty((Q.shape[0], self.n_columns), dtype=np.float64)
        if Q.shape[0]:
            _lib.check(self._lib.mbar_kde_eval(self._h, Q.shape[0], _lib.ptr(Q), _lib.ptr(out)))
        return out


def _check_2d(X, what):
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError(f"{what} must be a 2-D array (n_samples, n_features); reshape 1-D data with reshape(-1, 1)")
    if X.shape[0] == 0 or X.shape[1] == 0:
        raise ValueError(f"{what} is empty")
    if not np.all(np.isfinite(X)):
        raise ValueError(f"{what} contains NaN or infinity")
    return X


class KernelDensity:
    """Device-backed ``sklearn.neighbors.KernelDensity`` (euclidean metric, exact sums; see the module docstring)."""

    def __init__(self, *, bandwidth=1.0, algorithm="auto", kernel="gaussian", metric="euclidean", atol=0, rtol=0,
                 breadth_first=True, leaf_size=40, metric_params=None):
        self.bandwidth = bandwidth
        self.algorithm = algorithm
        self.kernel = kernel
        self.metric = metric
        self.atol = atol
        self.rtol = rtol
        self.breadth_first = breadth_first
        self.leaf_size = leaf_size
        self.metric_params = metric_params
        self._dev = None

    def get_params(self, deep=True):
        return {k: getattr(self, k) for k in SKLEARN_PARAMS}

    def set_params(self, **params):
        for k, v in params.items():
            if k not in SKLEARN_PARAMS:
                raise ValueError(f"Invalid parameter {k!r} for estimator KernelDensity. Valid parameters are: {sorted(SKLEARN_PARAMS)}.")
            setattr(self, k, v)
        return self

    def _bandwidth_for(self, X):
        n, d = X.shape
        if isinstance(self.bandwidth, str):
            if self.bandwidth == "scott":  # (sklearn >= 1.2)
                return float(n ** (-1.0 / (d + 4)))
            if self.bandwidth == "silverman":
                return float((n * (d + 2) / 4.0) ** (-1.0 / (d + 4)))
            raise ValueError(f"bandwidth must be a positive float, 'scott' or 'silverman', got {self.bandwidth!r}")
        h = float(self.bandwidth)
        if not (h > 0.0 and np.isfinite(h)):
            raise ValueError(f"bandwidth must be a positive float, got {self.bandwidth!r}")
        return h

    def fit(self, X, y=None, sample_weight=None):
        if self.metric != "euclidean" or self.metric_params is not None:
            raise ParameterError(f"metric {self.metric!r} / metric_params are not supported on this backend (euclidean only)")
        if self.kernel not in KERNELS:
            raise ValueError(f"kernel must be one of {KERNELS}, got {self.kernel!r}")
        X = _check_2d(X, "X")
        if X.shape[1] > MAX_DIM:
            raise ParameterError(f"at most {MAX_DIM} dimensions are supported on this backend, got {X.shape[1]}")
        h = self._bandwidth_for(X)
        if sample_weight is None:
            w = np.ones(X.shape[0])
        else:
            w = np.asarray(sample_weight, dtype=np.float64)
            if w.ndim == 0:
                w = np.full(X.shape[0], float(w))
            if w.shape != (X.shape[0],):
                raise ValueError(f"sample_weight.shape == {w.shape}, expected {(X.shape[0],)}!")
            if not np.all(np.isfinite(w)):
                raise ValueError("sample_weight contains NaN or infinity")
            if np.any(w < 0):
                raise ValueError("Negative values in data passed to `sample_weight`")
            if not np.any(w > 0):
                raise ValueError("sample_weight has no positive entry")
        self.close()
        self._dev = DeviceKDE(X, self.kernel, h)
        self._dev.set_weights(w)
        self._weights = w
        self._columns = None  # (the weight columns the device holds: None = the fit weights)
        self.bandwidth_ = h
        self.n_features_in_ = X.shape[1]
        return self

    def _queries(self, X):
        if self._dev is None:
            raise ValueError("This KernelDensity instance is not fitted yet. Call 'fit' first.")
        X = _check_2d(X, "X")
        if X.shape[1] != self.n_features_in_:
            raise ValueError(f"X has {X.shape[1]} features, but KernelDensity is expecting {self.n_features_in_} features as input.")
        return X

    def score_samples(self, X):
        """Log density of the fitted (weighted) sample at each row of X."""
        X = self._queries(X)
        if self._columns is not None:
            self._dev.set_weights(self._weights)
            self._columns = None
        return self._dev.log_density(X)[:, 0]

    def score(self, X, y=None):
        return float(np.sum(self.score_samples(X)))

    def score_samples_columns(self, X, weight_columns):
        """Log densities of the fitted sample positions under each column of ``weight_columns`` (N x C, finite, >= 0), one
        device pass over the pairs for all columns: ``out[m, c]`` = ``score_samples`` of a fit with ``sample_weight=
        weight_columns[:, c]``.  The columns stay on the device while the same array is passed again."""
        X = self._queries(X)
        if self._columns is not weight_columns:
            V = np.asarray(weight_columns, dtype=np.float64)
            if V.ndim != 2 or V.shape[0] != self._dev.n_samples:
                raise ValueError("weight_columns must be (n_samples, C)")
            if not np.all(np.isfinite(V)) or np.any(V < 0):
                raise ValueError("weight_columns must be finite and non-negative")
            self._dev.set_weights(V)
            self._columns = weight_columns
        return self._dev.log_density(X)

    def close(self):
        """Release the device copy of the samples (also done when the estimator is garbage-collected or refitted)."""
        if self._dev is not None:
            self._dev.close()
            self._dev = None

    def __repr__(self):
        changed = {k: v for k, v in self.get_params().items() if v != KernelDensity.__init__.__kwdefaults__[k]}
        return "KernelDensity(" + ", ".join(f"{k}={v!r}" for k, v in changed.items()) + ")"
