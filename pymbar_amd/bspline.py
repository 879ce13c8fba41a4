"""Weighted B-spline moments on the MI355X: the data terms of the spline surfaces of ``pymbar.FES`` (pymbar/fes.py:701-1166,
1611-2477).

A spline surface ``s(x) = sum_i c_i B_i(x)`` is linear in its coefficients, so every sum over the samples the reference evaluates
-- ``sum_n w_n s(x_n)`` in the objective, ``sum_n w_n B_i(x_n)`` in the gradient, the log likelihood of every Monte Carlo step --
is a dot product with the moment vector ``m_i = sum_n w_n B_i(x_n)``.  :class:`DeviceBSplineMoments` computes those moments in
``csrc/libmbar_hip.so`` (``mbar_bspline_*`` of include/mbar_hip.h, kernels in ``csrc/mbar_k_bspline.hip``), per sample group
and per weight column, exactly and reproducibly; ``B_i`` is ``scipy.interpolate.BSpline(t, e_i, k)`` with extrapolation."""
import ctypes as C

import numpy as np

from . import _lib
from .utils import DataError, ParameterError

MAX_DEGREE = 7
MAX_BASIS = 1024
MAX_GROUPS = 1024


def check_spline_shape(t, k):
    """The knot vector and degree the device accepts: ``(t, k, nbasis)`` or ``ParameterError``."""
    t = np.ascontiguousarray(t, dtype=np.float64)
    k = int(k)
    if not 0 <= k <= MAX_DEGREE:
        raise ParameterError(f"spline degree k must be 0 .. {MAX_DEGREE} on this backend, got {k}")
    nbasis = len(t) - k - 1
    if not k + 1 <= nbasis <= MAX_BASIS:
        raise ParameterError(f"the number of basis functions must be {k + 1} .. {MAX_BASIS} on this backend, got {nbasis}")
    if not np.all(np.isfinite(t)) or np.any(np.diff(t) < 0):
        raise ParameterError("knots must be finite and non-decreasing")
    return t, k, nbasis


class DeviceBSplineMoments(_lib.Handle):
    """N samples resident on one device, with optional group labels and C weight columns (an ``mbar_bspline`` handle).

    ``moments(t, k)[g, c, i] = sum over the samples n of group g of V[n, c] B_{i,k,t}(x_n)``."""

    _destroy = "mbar_bspline_destroy"

    def __init__(self, x, groups=None, n_groups=None, device=None):
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1))
        if len(x) == 0:
            raise DataError("need at least one sample")
        if not np.all(np.isfinite(x)):
            raise DataError("sample coordinates must be finite")
        _lib.require_device()
        self._lib = _lib.load_library()
        self.n_samples = len(x)
        self.device = _lib.default_device(device)
        self._h = C.c_void_p()
        _lib.check(self._lib.mbar_bspline_create(C.byref(self._h), self.device, self.n_samples, _lib.ptr(x)))
        self.n_groups = 1
        self.n_columns = 1
        if groups is not None:
            self.set_groups(groups, n_groups)

    def set_groups(self, groups, n_groups=None):
        g = np.ascontiguousarray(np.asarray(groups).reshape(-1), dtype=np.int32)
        if g.shape != (self.n_samples,):
            raise ParameterError("one group label per sample is needed")
        G = int(g.max()) + 1 if n_groups is None else int(n_groups)
        if not 1 <= G <= MAX_GROUPS:
            raise ParameterError(f"the number of groups must be 1 .. {MAX_GROUPS} on this backend, got {G}")
        if np.any(g < 0) or np.any(g >= G):
            raise ParameterError("group labels must lie in [0, n_groups)")
        _lib.check(self._lib.mbar_bspline_set_groups(self._h, G, _lib.ptr(g, _lib._i32p)))
        self.n_groups = G

    def set_weights(self, V):
        """V: (N,) or (N, C), finite."""
        V = np.asarray(V, dtype=np.float64)
        V = _lib.f64(V[:, None] if V.ndim == 1 else V, (self.n_samples, None), "weights", error=ParameterError)
        if V.shape[1] < 1:
            raise ParameterError("weights must be (n_samples, C)")
        if not np.all(np.isfinite(V)):
            raise DataError("weights must be finite")
        _lib.check(self._lib.mbar_bspline_set_weights(self._h, V.shape[1], _lib.ptr(V)))
        self.n_columns = V.shape[1]

    def moments(self, t, k):
        t, k, nbasis = check_spline_shape(t, k)
        out = np.empty((self.n_groups, self.n_columns, nbasis), dtype=np.float64)
        _lib.check(self._lib.mbar_bspline_moments(self._h, k, nbasis, _lib.ptr(t), _lib.ptr(out)))
        return out

    def kernel_ms(self):
        """Device time of the last :meth:`moments` call (HIP events around its kernels), in ms."""
        ms = C.c_double(0.0)
        _lib.check(self._lib.mbar_bspline_kernel_ms(self._h, C.byref(ms)))
        return ms.value
