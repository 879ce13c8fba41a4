"""``pymbar.other_estimators`` on the MI355X: BAR (``bar``, ``bar_zero``, ``bar_overlap``) and EXP (``exp``, ``exp_gauss``) with the
reference's names, signatures, defaults, return dicts and errors, plus :func:`bar_batch`, which solves P independent BAR problems
in one device call.

Every sum over work values runs in ``csrc/libmbar_hip.so`` (``mbar_bar_*`` of include/mbar_hip.h, kernels in
``csrc/mbar_k_bar.hip``) on a copy of the values uploaded once (:class:`DeviceBAR`).  The Fermi sums of ``bar_zero`` are exact in
log space for any finite input, in a fixed reduction order.  The reference's root find -- bracket from EXP, widening, false
position, bisection or self-consistent iteration, with its convergence and error outcomes -- is one state machine
(``bar_advance`` in ``csrc/mbar_bar.h``) that the device advances after every evaluation pass; the host only reads a status
block between groups of passes.  ``bar`` is ``bar_batch`` with P = 1, so a batch's entry p is bit-identical to the single call.

Deliberate deviations from the reference: ``+inf`` work values contribute a Fermi factor and an
``exp(-w)`` of exactly 0 instead of a NaN at the bracket; NaN and ``-inf`` values and empty sides raise ``ParameterError``; an
unknown ``uncertainty_method`` raises ``ParameterError`` (the reference's message formatting raises ``ValueError``); ``verbose``
logs only the final line; array-likes and float32 input are accepted (as fp64).
"""
import ctypes as C
import logging

import numpy as np

from . import _lib
from .utils import BoundsError, ConvergenceError, ParameterError

__all__ = ["bar_zero", "bar", "bar_batch", "bar_overlap", "exp", "exp_gauss", "DeviceBAR"]

logger = logging.getLogger(__name__)

# include/mbar_hip.h
CHUNK = 4096  # MBAR_BAR_CHUNK
RUNNING, DONE, NAN_BRACKET, BOUNDS, NOT_CONVERGED = 0, 1, 2, 3, 4
METHODS = {"false-position": 0, "bisection": 1, "self-consistent-iteration": 2}

_ip = _lib._ip
_POOR_OVERLAP = ("BAR is likely to be inaccurate because of poor overlap. Improve the sampling, or decrease the spacing between "
                 "states.  For now, guessing that the free energy difference is 0 with no uncertainty.")


def _work(w, what):
    """fp64 copy of one side's work values; NaN and -inf are errors (+inf is a factor of 0)."""
    a = np.ascontiguousarray(np.asarray(w, dtype=np.float64).ravel())
    if np.isnan(a).any() or np.isneginf(a).any():
        raise ParameterError(f"{what} holds NaN or -inf")
    return a


class DeviceBAR(_lib.Handle):
    """P problems' forward and reverse work values resident on one device (an ``mbar_bar`` handle).

    ``w_F_list``, ``w_R_list``: sequences of P arrays (``w_R_list`` None: one-sided, for the EXP moments only).  Values are
    uploaded once; every evaluation, the bracket, the uncertainty sums and the EXP moments read that copy."""

    _destroy = "mbar_bar_destroy"

    def __init__(self, w_F_list, w_R_list=None, device=None):
        self._setup(w_F_list, w_R_list)
        _lib.require_device()
        self._lib = _lib.load_library()
        self.device = _lib.default_device(device)
        wf = np.concatenate(self.w_F)
        wr = np.concatenate(self.w_R)
        self._h = C.c_void_p()
        _lib.check(self._lib.mbar_bar_create(C.byref(self._h), self.device, self.P, _lib.ptr(self.n_F, _ip), _lib.ptr(wf),
                                             _lib.ptr(self.n_R, _ip), _lib.ptr(wr) if wr.size else None))

    def _setup(self, w_F_list, w_R_list):
        """The input rules: fp64 copies, no NaN or -inf, no empty side (one-sided: no empty forward side)."""
        self.w_F = [_work(w, f"w_F of problem {p}") for p, w in enumerate(w_F_list)]
        self.P = len(self.w_F)
        if self.P < 1:
            raise ParameterError("need at least one problem")
        if w_R_list is None:
            self.w_R = [np.zeros(0) for _ in range(self.P)]
        else:
            self.w_R = [_work(w, f"w_R of problem {p}") for p, w in enumerate(w_R_list)]
            if len(self.w_R) != self.P:
                raise ParameterError("w_F_list and w_R_list must hold the same number of problems")
            for p in range(self.P):
                if self.w_F[p].size == 0 or self.w_R[p].size == 0:
                    raise ParameterError(f"problem {p}: w_F and w_R must each hold at least one value")
        for p in range(self.P):
            if self.w_F[p].size == 0:
                raise ParameterError(f"problem {p}: w_F must hold at least one value")
        self.n_F = np.array([w.size for w in self.w_F], dtype=np.int64)
        self.n_R = np.array([w.size for w in self.w_R], dtype=np.int64)

    def zero(self, DeltaF):
        """[P][5]: (F, log_numer, log_denom, log_numer2, log_denom2) at DeltaF[p], one pass."""
        d = np.asarray(DeltaF, dtype=np.float64)  # (one value for every problem, or one per problem)
        d = _lib.f64(np.full(self.P, d) if d.ndim == 0 else d, (self.P,), "DeltaF")
        out = np.empty((self.P, 5))
        _lib.check(self._lib.mbar_bar_zero(self._h, _lib.ptr(d), _lib.ptr(out)))
        return out

    def solve(self, states):
        """Runs the root find of every problem (``states``: a ``BarState * P`` array, updated in place); returns the passes."""
        n = C.c_int64(0)
        _lib.check(self._lib.mbar_bar_solve(self._h, states, C.byref(n)))
        return n.value

    def moments(self):
        """[P][2][5]: per side (forward, reverse) logsumexp(-w), sum x, sum (x - mean)^2 with x = exp(-w - max(-w)), sum w,
        sum (w - mean)^2."""
        out = np.empty((self.P, 2, 5))
        _lib.check(self._lib.mbar_bar_moments(self._h, _lib.ptr(out)))
        return out


def _exp_delta_f(lse, T):
    # DeltaF = -(logsumexp(-w) - log T), the reference's expression
    return -(np.float64(lse) - np.log(T))


def bar_zero(w_F, w_R, DeltaF):
    """The function of DeltaF whose zero is the BAR estimate: log sum_F f(M + w_F - DeltaF) - log sum_R f(-(M - w_R - DeltaF)),
    f(x) = 1 / (1 + exp(x)), M = log(T_F / T_R)."""
    with DeviceBAR([w_F], [w_R]) as h:
        return np.float64(h.zero([float(DeltaF)])[0, 0])


def _check_options(method, uncertainty_method, iterated_solution, maximum_iterations):
    if not iterated_solution:
        maximum_iterations = 1
        method = "self-consistent-iteration"
    if method not in METHODS:
        raise ParameterError("method {} is not defined for bar".format(method))
    if uncertainty_method not in ["BAR", "MBAR"]:
        raise ParameterError("uncertainty_method {} is not defined for bar".format(uncertainty_method))
    return method, int(maximum_iterations)


def _uncertainty(moments, T_F, T_R, uncertainty_method):
    # Bennett's variance ('BAR') or MBAR's two-state variance ('MBAR') from the sums of the Fermi factors and their squares
    lnN, lnD, lnN2, lnD2 = (np.float64(v) for v in moments)
    afF = np.exp(lnN) / T_F
    afR = np.exp(lnD) / T_R
    afF2 = np.exp(lnN2) / T_F
    afR2 = np.exp(lnD2) / T_R
    nrat = (T_F + T_R) / (T_F * T_R)
    if uncertainty_method == "BAR":
        variance = (afF2 / afF**2) / T_F + (afR2 / afR**2) / T_R - nrat
        return np.sqrt(variance)
    vartemp = (afF - afF2) * T_F + (afR - afR2) * T_R
    return np.sqrt(1.0 / vartemp - nrat)


def bar_batch(w_F_list, w_R_list, DeltaF=0.0, compute_uncertainty=True, uncertainty_method="BAR", maximum_iterations=500,
              relative_tolerance=1.0e-12, verbose=False, method="false-position", iterated_solution=True):
    """:func:`bar` of P independent problems (``w_F_list[p]``, ``w_R_list[p]``) in one device call.

    ``DeltaF`` is a scalar or one start per problem.  Returns ``{"Delta_f": (P,), "dDelta_f": (P,)}`` (``dDelta_f`` only with
    ``compute_uncertainty``); entry p is bit-identical to ``bar(w_F_list[p], w_R_list[p], ...)``.  A failing problem raises the
    reference's error, naming its index."""
    method, maximum_iterations = _check_options(method, uncertainty_method, iterated_solution, maximum_iterations)
    with DeviceBAR(w_F_list, w_R_list) as h:
        P = h.P
        start = np.broadcast_to(np.asarray(DeltaF, dtype=np.float64), (P,))
        T_F = h.n_F.astype(np.float64)
        T_R = h.n_R.astype(np.float64)
        states = (_lib.BarState * P)()
        bracketed = method != "self-consistent-iteration"
        m = h.moments() if bracketed else None
        for p in range(P):
            s = states[p]
            s.method = METHODS[method]
            s.iterated = int(bool(iterated_solution))
            s.maximum_iterations = maximum_iterations
            s.relative_tolerance = float(relative_tolerance)
            s.DeltaF = float(start[p])
            s.want_moments = int(bool(compute_uncertainty))
            if bracketed:
                s.UpperB = float(_exp_delta_f(m[p, 0, 0], T_F[p]))
                s.LowerB = float(-_exp_delta_f(m[p, 1, 0], T_R[p]))
        h.solve(states)
    Delta_f = np.zeros(P)
    dDelta_f = np.zeros(P)
    for p in range(P):
        s = states[p]
        if s.status == NAN_BRACKET:
            logger.warning(_POOR_OVERLAP)
            continue
        if s.status == BOUNDS:
            raise BoundsError(f"problem {p}: WARNING: Cannot determine bound on free energy")
        if s.status == NOT_CONVERGED:
            raise ConvergenceError(
                "problem {:d}: WARNING: Did not converge to within specified tolerance. max_delta = {:f}, TOLERANCE = {:f}, "
                "MAX_ITS = {:d}".format(p, s.relative_change, relative_tolerance, maximum_iterations))
        if s.status != DONE:
            raise RuntimeError(f"problem {p}: the root find ended with status {s.status}")
        Delta_f[p] = s.DeltaF
        if compute_uncertainty:
            dDelta_f[p] = _uncertainty(s.moments, T_F[p], T_R[p], uncertainty_method)
        if verbose:
            if compute_uncertainty:
                logger.info("DeltaF = {:8.3f} +- {:8.3f}".format(Delta_f[p], dDelta_f[p]))
            else:
                logger.info("DeltaF = {:8.3f}".format(Delta_f[p]))
    if compute_uncertainty:
        return {"Delta_f": Delta_f, "dDelta_f": dDelta_f}
    return {"Delta_f": Delta_f}


def bar(w_F, w_R, DeltaF=0.0, compute_uncertainty=True, uncertainty_method="BAR", maximum_iterations=500,
        relative_tolerance=1.0e-12, verbose=False, method="false-position", iterated_solution=True):
    """Compute the free energy difference with the Bennett acceptance ratio (``pymbar.other_estimators.bar``).

    Returns ``{"Delta_f": float, "dDelta_f": float}`` (``dDelta_f`` only with ``compute_uncertainty``)."""
    r = bar_batch([w_F], [w_R], DeltaF=DeltaF, compute_uncertainty=compute_uncertainty, uncertainty_method=uncertainty_method,
                  maximum_iterations=maximum_iterations, relative_tolerance=relative_tolerance, verbose=verbose, method=method,
                  iterated_solution=iterated_solution)
    return {k: np.float64(v[0]) for k, v in r.items()}


def bar_overlap(w_F, w_R):
    """Overlap between the forward and reverse ensembles, MBAR's definition (0: none, 1: complete)."""
    from .mbar import MBAR

    w_F = np.asarray(w_F)
    w_R = np.asarray(w_R)
    N_k = np.array([len(w_F), len(w_R)])
    N = N_k.sum()
    u_kn = np.zeros([2, N])
    u_kn[1, 0:N_k[0]] = w_F[:]
    u_kn[0, N_k[0]:N] = w_R[:]
    mbar = MBAR(u_kn, N_k)
    results = bar(w_F, w_R)
    bar_df = results["Delta_f"]
    bar_ddf = results["dDelta_f"]
    assert np.isclose(mbar.f_k[1] - mbar.f_k[0], bar_df), f"BAR: {bar_df} +- {bar_ddf} | MBAR: {mbar.f_k[1] - mbar.f_k[0]}"
    return mbar.compute_overlap()["scalar"]


def _one_sided(w_F):
    w = _work(w_F, "w_F")
    if w.size == 0:
        raise ParameterError("w_F must hold at least one value")
    with DeviceBAR([w]) as h:
        return w, h.moments()[0, 0]


def exp(w_F, compute_uncertainty=True, is_timeseries=False):
    """One-sided exponential averaging (Zwanzig): ``{"Delta_f", "dDelta_f"}`` (``pymbar.other_estimators.exp``)."""
    w, m = _one_sided(w_F)
    T = float(w.size)
    DeltaF = _exp_delta_f(m[0], T)
    if not compute_uncertainty:
        return {"Delta_f": DeltaF}
    Ex = np.float64(m[1]) / T
    g = 1.0
    if is_timeseries:
        from . import timeseries

        max_arg = np.max(-w)
        x = np.exp(-w - max_arg)
        g = timeseries.statistical_inefficiency(x, x)
    dx = np.sqrt(np.float64(m[2]) / T) / np.sqrt(T / g)
    return {"Delta_f": DeltaF, "dDelta_f": dx / Ex}


def exp_gauss(w_F, compute_uncertainty=True, is_timeseries=False):
    """Gaussian approximation to one-sided exponential averaging: ``{"Delta_f", "dDelta_f"}``
    (``pymbar.other_estimators.exp_gauss``)."""
    w, m = _one_sided(w_F)
    T = float(w.size)
    var = np.float64(m[4]) / T
    DeltaF = np.float64(m[3]) / T - 0.5 * var
    if not compute_uncertainty:
        return {"Delta_f": DeltaF}
    T_eff = T
    if is_timeseries:
        from . import timeseries

        g = timeseries.statistical_inefficiency(w, w)
        T_eff = T / g
    dx2 = var / T_eff + 0.5 * var * var / (T_eff - 1)
    return {"Delta_f": DeltaF, "dDelta_f": np.sqrt(dx2)}
