"""``pymbar.timeseries`` on the MI355X: statistical inefficiencies, equilibration detection, correlation functions and
subsampling, with the reference's names, signatures, defaults, return types and errors.

Every lagged fluctuation sum runs in ``csrc/libmbar_hip.so`` (``mbar_acf_*`` of include/mbar_hip.h, kernels in
``csrc/mbar_k_acf.hip``), double-double and in a fixed order.  The reference's stopping rule runs on the device, one thread per
origin, so :func:`detect_equilibration` computes the g of every suffix ``A_t[t:]`` in O(T * lags) work instead of the
reference's O(T^2 * lags) (:func:`statistical_inefficiency_suffixes`).  Import it as ``from pymbar_amd import timeseries``; the
package does not import it, and like the reference it logs :data:`LongWarning` when it is imported.

Deliberate deviations from the reference: inputs are promoted to fp64 before the mean; a suffix whose
values are all equal takes the zero-variance path (``ParameterError``, or ``T - t + 1`` in :func:`detect_equilibration`); non-finite
input raises ``ParameterError``; ``fft=True`` and :func:`statistical_inefficiency_fft` use the same exact lag sums (no FFT, no
statsmodels).  The fft formula's cost is O(N * ind): quadratic for a series whose correlation never drops to zero or below.
"""
import ctypes as C
import logging
import math

import numpy as np

from . import _lib
from .utils import ParameterError

__all__ = [
    "statistical_inefficiency", "statistical_inefficiency_multiple", "integrated_autocorrelation_time",
    "integrated_autocorrelation_timeMultiple", "normalized_fluctuation_correlation_function",
    "normalized_fluctuation_correlation_function_multiple", "subsample_correlated_data", "detect_equilibration",
    "statistical_inefficiency_fft", "detect_equilibration_binary_search", "statistical_inefficiency_suffixes", "LongWarning",
]

logger = logging.getLogger(__name__)
LongWarning = (
    "Warning on use of the timeseries module: If the inherent timescales of the system "
    "are long compared to those being analyzed, this statistical inefficiency may be an underestimate.  "
    "The estimate presumes the use of many statistically independent samples.  "
    "Tests should be performed to assess whether this condition is satisfied.   "
    "Be cautious in the interpretation of the data."
)
logger.warning(LongWarning)

# status codes of the device rule (include/mbar_hip.h, mbar_acf_suffix_g)
STOPPED, ZERO_VARIANCE, END = 1, 2, 3
_ZERO_COV = "Sample covariance sigma_AB^2 = 0 -- cannot compute statistical inefficiency"

_ip = _lib._ip


def lag_schedule(fast, tmax):
    """The reference's lags below ``tmax`` with their increments: (1, 1), (2, 1), (3, 1), ... or (fast) (1, 1), (2, 2), (4, 3), ..."""
    out, t, inc = [], 1, 1
    while t < tmax:
        out.append((t, inc))
        t += inc
        if fast:
            inc += 1
    return out


class DeviceACF(_lib.Handle):
    """One series (or the concatenation of K segments) resident on one device (an ``mbar_acf`` handle).

    ``a``, ``b``: fp64 values (``b`` None: the autocorrelation); ``seg``: segment lengths; the device holds ``a - shift_a`` and
    ``b - shift_b``."""

    _destroy = "mbar_acf_destroy"

    def __init__(self, a, b=None, seg=None, shift_a=0.0, shift_b=0.0, device=None):
        _lib.require_device()
        self._lib = _lib.load_library()
        self.a = _lib.f64(a, (None,), "a")
        self.T = self.a.size
        self.b = _lib.f64(b, (self.T,), "b", optional=True)
        self.seg = np.ascontiguousarray([self.T] if seg is None else seg, dtype=np.int64)  # (the library checks their sum against T)
        self.device = _lib.default_device(device)
        self._h = C.c_void_p()
        _lib.check(self._lib.mbar_acf_create(C.byref(self._h), self.device, self.T, _lib.ptr(self.a), _lib.ptr(self.b), self.seg.size,
                                             _lib.ptr(self.seg, _ip), float(shift_a), float(shift_b)))

    def suffix_g(self, nskip, fast, mintime, fft=False):
        """(g, stop, status) of the origins 0, nskip, ... < T - 1 (one segment)."""
        n = (self.T - 2) // nskip + 1
        g, stop, st = np.empty(n), np.empty(n, np.int64), np.empty(n, np.int32)
        _lib.check(self._lib.mbar_acf_suffix_g(self._h, int(nskip), int(bool(fast)), int(mintime), int(bool(fft)), _lib.ptr(g),
                                               _lib.ptr(stop, _ip), _lib.ptr(st, _lib._i32p)))
        return g, stop, st

    def multiple_g(self, fast, mintime, want_ct=False):
        """(g, stop, status, ct) of the K-segment rule; ct[k] = C at schedule entry k (entry 0: lag 0, not written)."""
        g, stop, st = np.empty(1), np.empty(1, np.int64), np.empty(1, np.int32)
        ct = None
        if want_ct:
            n = C.c_int64(0)
            _lib.check(self._lib.mbar_acf_schedule_length(int(bool(fast)), int(self.seg.max()), C.byref(n)))
            ct = np.zeros(n.value)
        _lib.check(self._lib.mbar_acf_multiple_g(self._h, int(bool(fast)), int(mintime), _lib.ptr(g), _lib.ptr(stop, _ip),
                                                 _lib.ptr(st, _lib._i32p), 0 if ct is None else ct.size, _lib.ptr(ct)))
        return float(g[0]), int(stop[0]), int(st[0]), ct

    def lag_sums(self, lags, origins, segments=False):
        """(xab, xba), each [len(lags)][len(origins)]: about the suffix means of each origin, or (segments) the sums over
        [o_i, o_i+1) about the shifts."""
        lags = np.ascontiguousarray(lags, dtype=np.int64)
        origins = np.ascontiguousarray(origins, dtype=np.int64)
        xab = np.empty((lags.size, origins.size))
        xba = np.empty((lags.size, origins.size))
        _lib.check(self._lib.mbar_acf_lag_sums(self._h, lags.size, _lib.ptr(lags, _ip), origins.size, _lib.ptr(origins, _ip),
                                               int(bool(segments)), _lib.ptr(xab), _lib.ptr(xba)))
        return xab, xba


def _f64(x):
    a = np.asarray(x, dtype=np.float64).ravel()
    if not np.all(np.isfinite(a)):
        raise ParameterError("the timeseries contains NaN or infinity")
    return a


def _constant(a):
    return a.size == 0 or bool(np.all(a == a[0]))


def statistical_inefficiency(A_n, B_n=None, fast=False, mintime=3, fft=False):
    """Compute the (cross) statistical inefficiency g = 1 + 2 tau of (two) timeseries; g >= 1 (``pymbar.timeseries``)."""
    A_n = np.array(A_n)
    if fft and B_n is None:
        return statistical_inefficiency_fft(A_n, mintime=mintime)
    cross = B_n is not None
    B_n = np.array(B_n) if cross else A_n
    if A_n.shape != B_n.shape:
        raise ParameterError("A_n and B_n must have same dimensions.")
    return _suffix_g(_f64(A_n), _f64(B_n) if cross else None, fast, mintime, fft=False, nskip=None)[0]


def _suffix_g(a, b, fast, mintime, fft, nskip):
    """g of the origins 0, nskip, ... < T - 1 (nskip None: origin 0 only); NaN for a zero-variance suffix (origin 0 alone: raise)."""
    T = a.size
    single = nskip is None
    if single and (_constant(a) or (b is not None and _constant(b))):
        raise ParameterError(_ZERO_COV)
    if T < 2:
        return np.zeros(0)
    with DeviceACF(a, b, shift_a=a.mean(), shift_b=0.0 if b is None else b.mean()) as dev:
        g, _, st = dev.suffix_g(T if single else int(nskip), fast, mintime, fft)
    if single and st[0] == ZERO_VARIANCE:
        raise ParameterError(_ZERO_COV)
    g = np.where(st == ZERO_VARIANCE, np.nan, g)
    return [float(g[0])] if single else g


def statistical_inefficiency_suffixes(A_t, fast=True, nskip=1, mintime=3):
    """fp64 g of every suffix ``A_t[t:]``, ``t = 0, nskip, ... < T - 1`` (what :func:`detect_equilibration` computes), with
    ``statistical_inefficiency(A_t[t:], fast=fast, mintime=mintime)``'s rule; NaN where the suffix has zero variance."""
    if int(nskip) < 1:
        raise ParameterError("nskip must be >= 1")
    return _suffix_g(_f64(A_t), None, fast, mintime, fft=False, nskip=int(nskip))


def _as_list(A_kn):
    if type(A_kn) == np.ndarray:
        if A_kn.ndim == 1:
            return [A_kn.copy()]
        return [A_kn[k, :].copy() for k in range(A_kn.shape[0])]
    return A_kn


def statistical_inefficiency_multiple(A_kn, fast=False, return_correlation_function=False):
    """Statistical inefficiency from multiple stationary timeseries of possibly different lengths (``pymbar.timeseries``);
    with ``return_correlation_function`` also ``Ct``, a list of ``(t, C)``."""
    A_kn = _as_list(A_kn)
    parts = [_f64(A_kn[k]) for k in range(len(A_kn))]
    N_k = np.array([p.size for p in parts], dtype=np.int64)
    if len(parts) == 0 or np.any(N_k < 1):
        raise ParameterError("every timeseries needs at least one value")
    a = np.concatenate(parts)
    mu = a.sum() / float(a.size)
    with DeviceACF(a, None, seg=N_k, shift_a=mu) as dev:
        g, stop, st, ct = dev.multiple_g(fast, 10, want_ct=return_correlation_function)
    if st == ZERO_VARIANCE:
        raise ParameterError("Sample variance sigma^2 = 0 -- cannot compute statistical inefficiency")
    if not return_correlation_function:
        return g
    Ct = []
    for k, (t, _) in enumerate(lag_schedule(fast, int(N_k.max()) - 1), start=1):
        if t > stop or (t == stop and st == END):
            break
        Ct.append((t, ct[k]))
    return g, Ct


def integrated_autocorrelation_time(A_n, B_n=None, fast=False, mintime=3):
    """Integrated autocorrelation time (g - 1) / 2; see :func:`statistical_inefficiency`."""
    g = statistical_inefficiency(A_n, B_n, fast, mintime)
    return (g - 1.0) / 2.0


def integrated_autocorrelation_timeMultiple(A_kn, fast=False):
    """Integrated autocorrelation time from multiple timeseries; see :func:`statistical_inefficiency_multiple`."""
    g = statistical_inefficiency_multiple(A_kn, fast, False)
    return (g - 1.0) / 2.0


def normalized_fluctuation_correlation_function(A_n, B_n=None, N_max=None, norm=True):
    """C(t) = (<A(t) B(t)> - <A><B>) / (<AB> - <A><B>) for t = 0 .. N_max (``pymbar.timeseries``)."""
    if B_n is None:
        B_n = A_n
    A_n = np.array(A_n)
    B_n = np.array(B_n)
    N = A_n.size
    if (not N_max) or (N_max > N - 1):
        N_max = N - 1
    if A_n.shape != B_n.shape:
        raise ParameterError("A_n and B_n must have same dimensions.")
    a, b = _f64(A_n), _f64(B_n)
    mu_A, mu_B = a.mean(), b.mean()
    if _constant(a) or _constant(b):
        raise ParameterError(_ZERO_COV)
    lags = np.arange(N_max + 1)
    with DeviceACF(a, None if B_n is A_n else b, shift_a=mu_A, shift_b=mu_B) as dev:
        xab, xba = dev.lag_sums(lags, [0])
    sigma2_AB = xab[0, 0] / N
    if sigma2_AB == 0:
        raise ParameterError(_ZERO_COV)
    C_n = (xab[:, 0] + xba[:, 0]) / (2.0 * (N - lags).astype(np.float64) * sigma2_AB)
    if norm:
        return C_n
    return C_n * sigma2_AB + mu_A * mu_B


def normalized_fluctuation_correlation_function_multiple(A_kn, B_kn=None, N_max=None, norm=True, truncate=False):
    """The normalized fluctuation (cross) correlation function from multiple timeseries (``pymbar.timeseries``), including the
    reference's ``C_n[:t]`` return."""
    if B_kn is None:
        B_kn = A_kn
    if (type(A_kn) is not list) or (type(B_kn) is not list):
        raise ParameterError("A_kn and B_kn must each be a list of numpy arrays.")
    if len(A_kn) != len(B_kn):
        raise ParameterError(
            "A_kn and B_kn must contain corresponding timeseries -- different numbers of timeseries detected in each.")
    K = len(A_kn)
    for k in range(K):
        if A_kn[k].size != B_kn[k].size:
            raise ParameterError(
                "A_kn and B_kn must contain corresponding timeseries -- lack of correspondence in timeseries lenghts detected.")
    N_k = np.array([A_kn[k].size for k in range(K)], dtype=np.int64)
    if K == 0 or np.any(N_k < 1):
        raise ParameterError("every timeseries needs at least one value")
    N = int(N_k.sum())
    if (not N_max) or (N_max > max(N_k) - 1):
        N_max = int(max(N_k)) - 1
    a = np.concatenate([_f64(x) for x in A_kn])
    b = a if B_kn is A_kn else np.concatenate([_f64(x) for x in B_kn])
    mu_A, mu_B = a.sum() / float(N), b.sum() / float(N)
    starts = np.concatenate([[0], np.cumsum(N_k)[:-1]])
    lags = np.arange(N_max + 1)
    with DeviceACF(a, None if b is a else b, seg=N_k, shift_a=mu_A, shift_b=mu_B) as dev:
        xab, _ = dev.lag_sums(lags, starts, segments=True)
    sigma2_AB = 0.0
    for k in range(K):
        sigma2_AB += xab[0, k]
    sigma2_AB /= float(N)
    C_n = np.zeros([N_max + 1], np.float64)
    t = 0
    negative = False
    for t in range(0, N_max + 1):
        numerator = 0.0
        denominator = 0.0
        for k in range(K):
            if t >= N_k[k]:
                continue
            numerator += xab[t, k]
            denominator += float(N_k[k] - t)
            if truncate and numerator < 0:
                negative = True
        C_n[t] = numerator / denominator / sigma2_AB
        if negative:
            break
    if norm:
        return C_n[:t]
    return C_n[:t] * sigma2_AB + mu_A * mu_B


def subsample_correlated_data(A_t, g=None, fast=False, conservative=False, verbose=False):
    """Indices of an uncorrelated subsample of the data (``pymbar.timeseries``): ``range(0, T, ceil(g))`` with
    ``conservative``, else the distinct ``round(n g)`` below T.  Host index arithmetic; g comes from the device."""
    A_t = np.array(A_t)
    T = A_t.size
    if not g:
        if verbose:
            logger.info("Computing statistical inefficiency...")
        g = statistical_inefficiency(A_t, A_t, fast=fast)
        if verbose:
            logger.info("g = {:f}".format(g))
    if conservative:
        stride = int(math.ceil(g))
        if verbose:
            logger.info("conservative subsampling: using stride of {:d}".format(stride))
        indices = range(0, T, stride)
    else:
        indices = []
        n = 0
        while int(round(n * g)) < T:
            t = int(round(n * g))
            if (n == 0) or (t != indices[-1]):
                indices.append(t)
            n += 1
        if verbose:
            logger.info("standard subsampling: using average stride of {:f}".format(g))
    if verbose:
        logger.info("The resulting subsampled set has {:d} samples (original timeseries had {:d}).".format(len(indices), T))
    return indices


def equilibration_bookkeeping(T, nskip, g):
    """The reference's float32 bookkeeping of :func:`detect_equilibration` from the fp64 g of the origins 0, nskip, ... < T - 1
    (NaN: zero variance, counted as ``T - t + 1``): returns (t, g, Neff_max) as the reference's loop does."""
    g_t = np.ones([T - 1], np.float32)
    Neff_t = np.ones([T - 1], np.float32)
    origins = np.arange(0, T - 1, nskip, dtype=np.int64)
    num = T - origins + 1
    zero = np.isnan(g)
    g_t[origins] = np.where(zero, num, g)
    # (T - t + 1) / g_t[t] with a Python int over a float32 scalar: float32 arithmetic under NumPy 2, float64 under NumPy 1
    dt = type((int(T) + 1) / np.float32(1.0))
    Neff_t[origins] = num.astype(dt) / g_t[origins].astype(dt)
    Neff_max = Neff_t.max()
    t = Neff_t.argmax()
    return t, g_t[t], Neff_max


def detect_equilibration(A_t, fast=True, nskip=1):
    """Start t of the equilibrated region, its g and its number of uncorrelated samples Neff_max, maximising Neff over every
    origin 0, nskip, ... (``pymbar.timeseries``; the g of every suffix is one device call)."""
    T = A_t.size
    if A_t.std() == 0.0:
        return 0, 1, 1
    g = statistical_inefficiency_suffixes(A_t, fast=fast, nskip=nskip)
    return equilibration_bookkeeping(T, int(nskip), g)


def statistical_inefficiency_fft(A_n, mintime=3):
    """g = max(1, 1 + sum_{t=1}^{ind-1} 2 C_t (1 - t/N)), ind the first t > mintime with C_t <= 0 (N if none), from the exact lag
    sums (no FFT, no statsmodels): O(N * ind) work."""
    A_n = np.array(A_n)
    return _suffix_g(_f64(A_n), None, False, mintime, fft=True, nskip=None)[0]


def detect_equilibration_binary_search(A_t, bs_nodes=10):
    """Equilibration detection by a binary search over geometrically spaced origins with :func:`statistical_inefficiency_fft`
    (``pymbar.timeseries``)."""
    assert bs_nodes > 4, "Number of nodes for binary search must be > 4"
    T = A_t.size
    if A_t.std() == 0.0:
        return 0, 1, T
    start = 1
    end = T - 1
    n_grid = min(bs_nodes, T)
    while True:
        time_grid = np.unique((10 ** np.linspace(np.log10(start), np.log10(end), n_grid)).round().astype("int"))
        g_t = np.ones(time_grid.size)
        Neff_t = np.ones(time_grid.size)
        for k, t in enumerate(time_grid):
            if t < T - 1:
                g_t[k] = statistical_inefficiency_fft(A_t[t:])
                Neff_t[k] = (T - t + 1) / g_t[k]
        Neff_max = Neff_t.max()
        k = Neff_t.argmax()
        t = time_grid[k]
        g = g_t[k]
        if end - start < 4:
            break
        if k == 0:
            start = time_grid[0]
            end = time_grid[1]
        elif k == time_grid.size - 1:
            start = time_grid[-2]
            end = time_grid[-1]
        else:
            start = time_grid[k - 1]
            end = time_grid[k + 1]
    return t, g, Neff_max
