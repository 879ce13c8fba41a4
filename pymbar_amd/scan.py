"""Reweighting scans over a linear family of unsampled states (``MBAR.compute_scan``): solve once, then reweight to hundreds or
thousands of states that were never sampled -- a temperature, pressure or lambda grid, a sweep of a restraint centre -- and read
free energies, averages and their uncertainties along the scan.

Member ``l`` of the family is ``u_l(n) = sum_b coeff_lb[l, b] basis_bn[b, n] + offset_l[l]``: ``B`` coefficients, not a matrix
row of ``N`` doubles.  The free energies and averages come from pass A of the device (``mbar_scan_lognum``), which never reads the
resident matrix.  The analytical uncertainties follow DESIGN.md section 17: the members are weight columns with ``N = 0`` appended
to the resident ``W``, so ``Theta(z, z') = z . z' + y(z)^T diag(g) y(z')`` with the border ``(y, g)`` of
:func:`pymbar_amd.utils.bordered_theta_basis` -- the resident ``K x K`` Gram matrix, the ``K x L x J`` cross block and the members'
own products (``mbar_scan_gram_w``, pass B, the cross block on the fp64 matrix cores) replace the ``Theta`` of order ``K + 2 L``
that ``compute_perturbed_free_energies(u_ln)`` / ``compute_expectations(A_n, u_kn=u_ln)`` decompose.

Every member's numbers are computed by operations whose order does not depend on the other members of the call (the host sums
below run over states and eigen-directions in explicit loops, not through BLAS): member ``l`` scanned alone returns the bits it
returns inside a scan of thousands.
"""
import logging

import numpy as np

from .utils import DataError, ParameterError, bordered_theta_basis, check_w_sums

logger = logging.getLogger(__name__)

MAX_BASIS = 8
MAX_OBSERVABLES = 3
MAX_STATES = 128
_NOT_HERE = "not supported on this backend"


def _scan_matrix(mbar):
    """The mbar's resident matrix, if its handle has the scan passes (the single-rank :class:`pymbar_amd.device.DeviceMatrix`)."""
    dm = mbar._dm
    if getattr(dm, "nranks", 1) != 1 or not all(hasattr(dm, name) for name in ("set_scan", "scan_lognum", "scan_gram_w")):
        raise ParameterError(f"scans over a linear family need the scan passes of a single-rank device matrix and are {_NOT_HERE} for this handle")
    if mbar.K > MAX_STATES:
        raise ParameterError(f"scans over a linear family serve at most {MAX_STATES} states (this object has {mbar.K})")
    return dm


def _check_inputs(mbar, basis_bn, coeff_lb, offset_l, A_qn, reference):
    N = mbar.N
    basis_bn = np.ascontiguousarray(basis_bn, dtype=np.float64)
    coeff_lb = np.ascontiguousarray(coeff_lb, dtype=np.float64)
    if basis_bn.ndim != 2 or basis_bn.shape[1] != N or not 1 <= basis_bn.shape[0] <= MAX_BASIS:
        raise ParameterError(f"basis_bn must have shape (B, N) with 1 <= B <= {MAX_BASIS}")
    B = basis_bn.shape[0]
    if coeff_lb.ndim != 2 or coeff_lb.shape[1] != B or coeff_lb.shape[0] < 1:
        raise ParameterError("coeff_lb must have shape (L, B) with L >= 1")
    L = coeff_lb.shape[0]
    offset_l = np.zeros(L) if offset_l is None else np.ascontiguousarray(offset_l, dtype=np.float64)
    if offset_l.shape != (L,):
        raise ParameterError("offset_l must have shape (L,)")
    if A_qn is None:
        A_qn = np.zeros((0, N))
    A_qn = np.asarray(A_qn, dtype=np.float64)
    if A_qn.ndim == 1:
        A_qn = A_qn.reshape(1, -1)
    if A_qn.ndim != 2 or A_qn.shape[1] != N or A_qn.shape[0] > MAX_OBSERVABLES:
        raise ParameterError(f"A_qn must have shape (Q, N) with 0 <= Q <= {MAX_OBSERVABLES}, or (N,)")
    if not (isinstance(reference, (int, np.integer)) and 0 <= int(reference) < L):
        raise ParameterError("reference must be the index of a member of the family")
    if not (np.all(np.isfinite(basis_bn)) and np.all(np.isfinite(coeff_lb)) and np.all(np.isfinite(offset_l)) and np.all(np.isfinite(A_qn))):
        raise DataError("basis_bn, coeff_lb, offset_l and A_qn must be finite")
    return basis_bn, coeff_lb, offset_l, A_qn, L


def _shifted(A_qn):
    """``(t_qn, shift)``: the observables made positive as the reference does (mbar.py:858-878)."""
    if len(A_qn) == 0:
        return np.zeros_like(A_qn), np.zeros(0)
    amin = A_qn.min(axis=1)
    shift = amin - np.abs(4.0 * np.finfo(np.float64).eps * amin)
    return A_qn - shift[:, None], shift


def _sqrt_small_negative_zeroed(d2, warning_cutoff):
    """``sqrt`` of squared uncertainties; small negative ones are zeroed (mbar.py:1687-1715, elementwise)."""
    d2 = np.array(d2)
    cutoff = -abs(warning_cutoff)
    if np.any(d2 < 0.0):
        if np.any(d2 < cutoff):
            logger.warning("A squared uncertainty is negative. Largest Magnitude = {0:f}".format(abs(np.min(d2[d2 < cutoff]))))
        d2[np.logical_and(0 > d2, d2 > cutoff)] = 0.0
    with np.errstate(invalid="ignore"):
        return np.sqrt(d2)


def _border(mbar, cross):
    """``y[i, l, j]`` of the members' columns ``b_l t_j`` and ``g``: ``y = lam^(-1/2) V^T D^(1/2) C``, summed over the states in
    ascending order, element by element."""
    G, ws = mbar._gram_w()
    check_w_sums(ws, 0.0)
    rt, lam, V, g = bordered_theta_basis(G, mbar.N_k)
    y = np.zeros((len(lam),) + cross.shape[1:])
    for k in range(cross.shape[0]):
        y += (V[k] * rt[k])[:, None, None] * cross[k][None, :, :]
    y /= np.sqrt(lam)[:, None, None]
    return y, g


def _qform(g, a, b):
    """``sum_i g_i a_i b_i`` over the eigen-directions in ascending order, element by element (``a``, ``b``: ``(m, ...)``)."""
    out = np.zeros(np.broadcast(a[0], b[0]).shape)
    for i in range(len(g)):
        out += g[i] * a[i] * b[i]
    return out


def _analytical(mbar, dm, coeff_lb, offset_l, f, mean, reference, approximate, warning_cutoff, cen={}):
    """``(dDelta_f, sigma)`` from pass B.  Member ``l`` contributes the columns ``z_l0 = b_l`` and ``z_lj = b_l t_j / mean_lj``;
    the cross block is bilinear, so the ``1 / mean`` scaling happens here."""
    L, J = mean.shape
    r = int(reference)
    cross, within, refcol, wsum = dm.scan_gram_w(mbar.f_k, coeff_lb, offset_l, f, reference=r, cross=not approximate, **cen)
    check_w_sums(wsum, 0.0)
    # z . z' of the columns that meet: b_l b_l, b_l b_r, (b_l t_j)(b_l t_j), (b_l t_j) b_l
    bb, br, rr = within[:, 0, 0], refcol[:, 0], within[r, 0, 0]
    if approximate:
        qbb = qbr = qrr = 0.0
    else:
        y, g = _border(mbar, cross)
        yb = y[:, :, 0]
        qbb, qbr, qrr = _qform(g, yb, yb), _qform(g, yb, yb[:, r:r + 1]), _qform(g, yb[:, r], yb[:, r])
    d2 = (bb + qbb) + (rr + qrr) - 2.0 * (br + qbr)
    d2[r] = 0.0
    dDelta_f = _sqrt_small_negative_zeroed(d2, warning_cutoff)
    sigma = np.zeros((J - 1, L))
    for j in range(1, J):
        m = mean[:, j]
        zz, zb = within[:, j, j] / (m * m), within[:, 0, j] / m
        if not approximate:
            yz = y[:, :, j] / m[None, :]
            zz, zb = zz + _qform(g, yz, yz), zb + _qform(g, yz, yb)
        var = (m * m) * (zz + (bb + qbb) - 2.0 * zb)
        with np.errstate(invalid="ignore"):
            sigma[j - 1] = np.sqrt(var)  # (as the reference: sqrt of the covariance's diagonal, mbar.py:1287)
    return dDelta_f, sigma


def _family_basis(mbar, basis_bn, coeff_lb):
    """``basis_bn`` of a scan call: None stands for the basis an object made by ``MBAR.from_linear`` was built from."""
    if coeff_lb is None:
        raise ParameterError("coeff_lb must have shape (L, B) with L >= 1")
    if basis_bn is not None:
        return basis_bn
    if getattr(mbar, "basis_bn", None) is None:
        raise ParameterError("basis_bn=None stands for the basis of an object made by MBAR.from_linear; this object was built from "
                             "a dense u_kn and has none: pass basis_bn")
    return mbar.basis_bn


def _family_kinds(mbar, basis_given, B, L, center_lb, harmonic_b, period_b):
    """``(set_scan keywords, scan_* keywords)`` of a scan call's term kinds and centres: empty for the linear family (the handle
    is then driven exactly as before the harmonic kind existed).  With ``basis_bn=None`` and no kinds given they are those of
    the object ``MBAR.from_family`` made; the centres are the call's own, required whenever a term is harmonic."""
    from .device import family_centers, family_terms

    if basis_given is None and harmonic_b is None and period_b is None:
        harmonic_b, period_b = getattr(mbar, "harmonic_b", None), getattr(mbar, "period_b", None)
    harmonic_b, period_b = family_terms(B, harmonic_b, period_b, error=ParameterError)
    if harmonic_b is None:
        if center_lb is not None and np.shape(center_lb) != (L, B):
            raise ParameterError("center_lb must have shape (L, B)")
        return {}, {}
    center_lb = family_centers(center_lb, L, B, harmonic_b, error=ParameterError, name="center_lb")
    return dict(harmonic_b=harmonic_b, period_b=period_b), dict(center_lb=center_lb)


def compute_scan(mbar, basis_bn=None, coeff_lb=None, offset_l=None, A_qn=None, reference=0, compute_uncertainty=True, uncertainty_method=None,
                 warning_cutoff=1.0e-10, center_lb=None, harmonic_b=None, period_b=None):
    """Free energies, averages and their uncertainties along a linear family of unsampled states.

    Member ``l`` is the state ``u_l(n) = sum_b coeff_lb[l, b] basis_bn[b, n] + offset_l[l]``; ``basis_bn`` is ``(B, N)`` with ``1 <=
    B <= 8`` (None: the basis of an object made by ``MBAR.from_linear``; on any other object None is a ``ParameterError``), ``coeff_lb`` ``(L, B)`` with any ``L >= 1``, ``A_qn`` optional, ``(Q, N)`` with ``Q <= 3`` or ``(N,)``.  Returns a
    dict: ``f`` ``(L,)`` in the gauge of ``mbar.f_k``; ``Delta_f = f - f[reference]`` and its uncertainty ``dDelta_f`` -- row
    ``reference`` of what ``compute_perturbed_free_energies(u_ln)`` returns for the dense ``u_ln``; with observables ``mu`` and
    ``sigma`` ``(Q, L)`` -- entry ``l`` of ``compute_expectations(A_qn[q], u_kn=u_ln, state_dependent=False)``.
    ``uncertainty_method``: None / "svd-ew" (the bordered form), "approximate", "bootstrap" (adds ``bootstrapped_f`` ``(n_bootstraps,
    L)`` and ``bootstrapped_observables`` ``(n_bootstraps, Q, L)``; the uncertainties are the ``std`` over replicates as
    ``compute_perturbed_free_energies`` and ``compute_expectations`` take it); "svd" needs the weight matrix itself and is not
    offered.

    ``center_lb`` ``(L, B)``, ``harmonic_b``, ``period_b`` ``(B,)``: a family with harmonic terms (``MBAR.from_family``) -- a sweep of
    a restraint centre on a torsion.  Term ``b`` of member ``l`` is then ``coeff_lb[l, b] w(basis_bn[b, n] - center_lb[l, b])^2``
    where ``harmonic_b[b]``, with the minimum image ``w`` for ``period_b[b] > 0``.  With ``basis_bn=None`` the kinds default to the
    constructor's; ``center_lb`` is required whenever a term is harmonic.  The uncertainties are formed as for a linear family."""
    basis_given = basis_bn
    if uncertainty_method == "svd":
        raise ParameterError("uncertainty_method 'svd' needs the weight matrix itself and is not offered for scans")
    if uncertainty_method not in (None, "svd-ew", "approximate", "bootstrap"):
        raise ParameterError(f"Method {uncertainty_method} unrecognized.")
    bootstrap = uncertainty_method == "bootstrap"
    if bootstrap and (mbar.n_bootstraps is None or mbar.n_bootstraps <= 0):
        raise ParameterError("Cannot request bootstrap sampling of expectations without any bootstraps.")
    basis_bn, coeff_lb, offset_l, A_qn, L = _check_inputs(mbar, _family_basis(mbar, basis_bn, coeff_lb), coeff_lb, offset_l, A_qn, reference)
    kinds, cen = _family_kinds(mbar, basis_given, basis_bn.shape[0], L, center_lb, harmonic_b, period_b)
    dm = _scan_matrix(mbar)
    Q = len(A_qn)
    t_qn, shift = _shifted(A_qn)
    dm.set_Nk(mbar.N_k)
    dm.set_scan(basis_bn, t_qn, **kinds)
    try:
        lognum, mean = dm.scan_lognum(mbar.f_k, coeff_lb, offset_l, **cen)
        f = -lognum
        out = dict(f=f, Delta_f=f - f[int(reference)])
        if Q:
            out["mu"] = mean[:, 1:].T + shift[:, None]
        if bootstrap:
            fb = np.zeros((mbar.n_bootstraps, L))
            Ab = np.zeros((mbar.n_bootstraps, Q, L))
            try:
                for b in range(mbar.n_bootstraps):
                    mbar._set_bootstrap_weights(dm, b)
                    ln_b, mean_b = dm.scan_lognum(mbar.f_k_boots[b, :], coeff_lb, offset_l, **cen)
                    fb[b] = -ln_b
                    Ab[b] = mean_b[:, 1:].T + shift[:, None]
            finally:
                dm.set_sample_weights(None)
            out["bootstrapped_f"], out["bootstrapped_observables"] = fb, Ab
            if compute_uncertainty:
                out["dDelta_f"] = np.std(fb, axis=0)  # (the per-state spread, as the reference returns it: mbar.py:1514)
                if Q:
                    out["sigma"] = np.std(Ab, axis=0)
        elif compute_uncertainty:
            out["dDelta_f"], sigma = _analytical(mbar, dm, coeff_lb, offset_l, f, mean, reference, uncertainty_method == "approximate",
                                                 warning_cutoff, cen)
            if Q:
                out["sigma"] = sigma
    finally:
        dm.set_scan(None)
    return out


# ---- many observables along a scan --------------------------------------------------------------------------------------------------
def _obs_matrix(mbar):
    dm = _scan_matrix(mbar)
    if not all(hasattr(dm, name) for name in ("set_scan_observables", "scan_obs_sums")):
        raise ParameterError(f"many observables along a scan need the observable pass of a single-rank device matrix and are {_NOT_HERE} for this handle")
    return dm


def _centred_observables(mbar, A_qn):
    """``(A_qn - s_q, s_q)`` with ``s_q`` the row's plain mean, or a ``ParameterError`` / ``DataError``."""
    A_qn = np.asarray(A_qn, dtype=np.float64)
    if A_qn.ndim == 1:
        A_qn = A_qn.reshape(1, -1)
    if A_qn.ndim != 2 or A_qn.shape[1] != mbar.N or A_qn.shape[0] < 1:
        raise ParameterError("A_qn must have shape (Q, N) with Q >= 1, or (N,)")
    if not np.all(np.isfinite(A_qn)):
        raise DataError("A_qn must be finite")
    shift = np.zeros(A_qn.shape[0])
    for q in range(A_qn.shape[0]):  # (row by row: an observable's centre does not depend on the others)
        shift[q] = np.sum(A_qn[q]) / A_qn.shape[1]
    return A_qn - shift[:, None], shift


def set_scan_observables(mbar, A_qn=None):
    """Keep ``A_qn`` -- ``(Q, N)`` with any ``Q >= 1``, or ``(N,)`` -- resident on the device for :func:`compute_scan_expectations`: a fit
    iterates over trial parameters hundreds of times against the same observables.  Stored is ``A_qn - s_q`` with ``s_q`` the row's
    plain mean (kept on the object), so that the variance expansion does not cancel against a large offset.  ``None`` releases them.
    The block survives the other scan methods."""
    dm = _obs_matrix(mbar)
    if A_qn is None:
        dm.set_scan_observables(None)
        mbar._scan_obs_shift = None
        return
    a_qn, shift = _centred_observables(mbar, A_qn)
    mbar._scan_obs_shift = None
    dm.set_scan_observables(a_qn)
    mbar._scan_obs_shift = shift


def _expectation_numbers(s1, t1, t2, w2sum, shift):
    """``(mu, sigma)`` ``(Q, L)`` from the sums: ``mu = s1 + s`` and, with ``m = s1``, ``sigma^2 = t2 - 2 m t1 + m^2 w2sum = sum c b^2 (a -
    m)^2``, the Kong estimate; element by element, so that an entry depends on its own member and observable alone."""
    mu = s1.T + shift[:, None]
    if t1 is None:
        return mu, None
    m = s1.T
    var = (t2.T - 2.0 * m * t1.T) + (m * m) * w2sum[None, :]
    with np.errstate(invalid="ignore"):
        sigma = np.sqrt(np.maximum(var, 0.0))
    return mu, sigma


def compute_scan_expectations(mbar, A_qn=None, basis_bn=None, coeff_lb=None, offset_l=None, compute_uncertainty=True,
                              uncertainty_method="approximate", center_lb=None, harmonic_b=None, period_b=None):
    """Averages of MANY observables along a family of unsampled states: a force-field fit against hundreds of experimental numbers, a
    distribution function with one observable per bin, per-residue quantities along a temperature ladder.

    ``A_qn``: ``(Q, N)`` with any ``Q >= 1`` or ``(N,)``, uploaded for this call and released afterwards; None: the observables
    :meth:`set_scan_observables` keeps resident (none set: a ``ParameterError``).  The family (``basis_bn``, ``coeff_lb``, ``offset_l``,
    ``center_lb``, ``harmonic_b``, ``period_b``) is that of :func:`compute_scan`.  Returns a dict: ``f`` ``(L,)``, the bits
    :func:`compute_scan` returns; ``mu`` ``(Q, L)``, entry ``l`` of ``compute_expectations(A_qn[q], u_kn=u_ln, state_dependent=False)``;
    ``n_eff`` ``(L,)``, Kish's effective sample number ``1 / sum_n w_ln^2`` of every member; with ``compute_uncertainty`` ``sigma``
    ``(Q, L)``.

    The sums are one ``(L x N)(N x Q)`` product on the fp64 matrix cores (``DeviceMatrix.scan_obs_sums``): every member weight is
    evaluated once per 128 observables, where ``ceil(Q / 3)`` calls of :func:`compute_scan` evaluate it once per 3.

    ``uncertainty_method``: "approximate" (the default: ``sigma^2 = sum_n w_ln^2 (A_qn - mu)^2``, what the reference's "approximate"
    returns) or "bootstrap" (the ``std`` over the replicates; adds ``bootstrapped_f`` ``(n_bootstraps, L)`` and
    ``bootstrapped_observables`` ``(n_bootstraps, Q, L)``).  The bordered forms need a ``K x L x Q`` cross block and stay with
    :func:`compute_scan` (``Q <= 3``)."""
    basis_given = basis_bn
    if uncertainty_method in (None, "svd-ew", "svd"):
        raise ParameterError(f"uncertainty_method {uncertainty_method!r}: the bordered uncertainty needs a K x L x Q cross block and stays "
                             f"with compute_scan (Q <= {MAX_OBSERVABLES}); compute_scan_expectations offers 'approximate' and 'bootstrap'")
    if uncertainty_method not in ("approximate", "bootstrap"):
        raise ParameterError(f"Method {uncertainty_method} unrecognized.")
    bootstrap = uncertainty_method == "bootstrap"
    if bootstrap and (mbar.n_bootstraps is None or mbar.n_bootstraps <= 0):
        raise ParameterError("Cannot request bootstrap sampling of expectations without any bootstraps.")
    basis_bn, coeff_lb, offset_l, _, L = _check_inputs(mbar, _family_basis(mbar, basis_bn, coeff_lb), coeff_lb, offset_l, None, 0)
    kinds, cen = _family_kinds(mbar, basis_given, basis_bn.shape[0], L, center_lb, harmonic_b, period_b)
    dm = _obs_matrix(mbar)
    resident = A_qn is None
    if resident:
        shift = getattr(mbar, "_scan_obs_shift", None)
        if shift is None:
            raise ParameterError("A_qn=None stands for the resident observables and none are set (set_scan_observables first)")
    else:
        a_qn, shift = _centred_observables(mbar, A_qn)
        if getattr(mbar, "_scan_obs_shift", None) is not None:
            raise ParameterError("observables are resident on this object (set_scan_observables): pass A_qn=None, or release them first")
    Q = len(shift)
    dm.set_Nk(mbar.N_k)
    dm.set_scan(basis_bn, None, **kinds)
    try:
        if not resident:
            dm.set_scan_observables(a_qn)
        lognum, _ = dm.scan_lognum(mbar.f_k, coeff_lb, offset_l, **cen)
        f = -lognum
        second = compute_uncertainty and not bootstrap
        s1, t1, t2, wsum, w2sum = dm.scan_obs_sums(mbar.f_k, coeff_lb, offset_l, f, second=second, **cen)
        check_w_sums(wsum, 0.0)
        if not second:  # (n_eff alone: the members' own products of pass B, without its cross block)
            w2sum = dm.scan_gram_w(mbar.f_k, coeff_lb, offset_l, f, reference=0, cross=False, **cen)[1][:, 0, 0]
        mu, sigma = _expectation_numbers(s1, t1, t2, w2sum, shift)
        out = dict(f=f, mu=mu, n_eff=1.0 / w2sum)
        if second:
            out["sigma"] = sigma
        if bootstrap:
            fb = np.zeros((mbar.n_bootstraps, L))
            Ab = np.zeros((mbar.n_bootstraps, Q, L))
            try:
                for b in range(mbar.n_bootstraps):
                    mbar._set_bootstrap_weights(dm, b)
                    ln_b, _ = dm.scan_lognum(mbar.f_k_boots[b, :], coeff_lb, offset_l, **cen)
                    fb[b] = -ln_b
                    s1_b = dm.scan_obs_sums(mbar.f_k_boots[b, :], coeff_lb, offset_l, fb[b], second=False, **cen)[0]
                    Ab[b] = s1_b.T + shift[:, None]
            finally:
                dm.set_sample_weights(None)
            out["bootstrapped_f"], out["bootstrapped_observables"] = fb, Ab
            if compute_uncertainty:
                out["sigma"] = np.std(Ab, axis=0)
    finally:
        if not resident:
            dm.set_scan_observables(None)
        dm.set_scan(None)
    return out


# ---- kernel-density surfaces along a scan -------------------------------------------------------------------------------------------
def _kde_matrix(mbar):
    dm = _scan_matrix(mbar)
    if not all(hasattr(dm, name) for name in ("set_scan_points", "scan_kde_sums")):
        raise ParameterError(f"kernel-density surfaces along a scan need the density pass of a single-rank device matrix and are {_NOT_HERE} for this handle")
    return dm


def _kde_points(mbar, x_n, queries, fes_reference, reference_point):
    """``(x_dn, q_dm, d, M)``: the samples and the queries coordinate-major, the point of "from-specified" appended as one more query."""
    x_n = np.asarray(x_n, dtype=np.float64)
    if x_n.ndim == 1:
        x_n = x_n.reshape(-1, 1)
    if x_n.ndim != 2 or x_n.shape[0] != mbar.N or x_n.shape[1] not in (1, 2):
        raise ParameterError("x_n must have shape (N,) or (N, d) with d = 1 or 2: kernel-density surfaces along a scan serve one or two dimensions")
    d = x_n.shape[1]
    queries = np.asarray(queries, dtype=np.float64)
    if queries.ndim == 1 and (d == 1 or queries.size == 0):
        queries = queries.reshape(-1, 1)
    if queries.ndim != 2 or queries.shape[1] != d or queries.shape[0] < 1:
        raise ParameterError(f"queries must have shape (M, {d}) with M >= 1" + (" or (M,)" if d == 1 else ""))
    M = queries.shape[0]
    if reference_point == "from-specified":
        if fes_reference is None:
            raise ParameterError("Specified reference point for FES not given")
        ref = np.array(fes_reference, dtype=np.float64).reshape(1, -1)
        if ref.shape[1] != d:
            raise DataError("fes_reference has inconsistent dimension with the data the FES is fit to.")
        queries = np.vstack([queries, ref])
    if not (np.all(np.isfinite(x_n)) and np.all(np.isfinite(queries))):
        raise DataError("x_n, queries and fes_reference must be finite")
    return np.ascontiguousarray(x_n.T), np.ascontiguousarray(queries.T), d, M


def _kde_surface(log_density, M, reference_point):
    """``(f_i, reference)`` of every member from its log densities at the queries (and, behind them, at the point of
    "from-specified"): ``FES._get_fes_kde``'s rule, row by row."""
    f_all = -log_density
    f_i = f_all[:, :M]
    L = len(f_i)
    reference = np.full(L, -1, dtype=np.int64)
    if reference_point == "from-lowest":
        reference = np.argmin(f_i, axis=1).astype(np.int64)
        f_i = f_i - f_i[np.arange(L), reference][:, None]
    elif reference_point == "from-specified":
        f_i = f_i - f_all[:, M][:, None]
    return np.ascontiguousarray(f_i), reference


def _kde_bootstrap_spread(fb, reference, reference_point, M):
    """``df_i`` ``(L, M)``: the ``std`` over the replicates of ``f^b_lm - f^b_l,ref`` with the reference query of the main estimate
    (column ``M`` for "from-specified", none for "from-normalization").  A replicate in which either is not finite is left out of
    that entry; fewer than two usable replicates give NaN."""
    nb, L, _ = fb.shape
    rows = np.arange(L)
    with np.errstate(invalid="ignore"):
        if reference_point == "from-lowest":
            fall = fb[:, :, :M] - fb[:, rows, reference][:, :, None]
        elif reference_point == "from-specified":
            fall = fb[:, :, :M] - fb[:, :, M][:, :, None]
        else:
            fall = fb[:, :, :M].copy()
    fall[~np.isfinite(fall)] = np.nan
    usable = np.sum(~np.isnan(fall), axis=0)
    df = np.full((L, M), np.nan)
    ok = usable >= 2
    if np.any(ok):
        df[ok] = np.nanstd(fall[:, ok], axis=0)
    return df


def compute_scan_kde(mbar, x_n, queries, bandwidth, basis_bn=None, coeff_lb=None, offset_l=None, kernel="gaussian", period=None,
                     reference_point="from-lowest", fes_reference=None, uncertainty_method=None, center_lb=None, harmonic_b=None,
                     period_b=None):
    """Kernel-density free energy surfaces of EVERY member of a family of unsampled states: F(x; T) on a temperature ladder, F(phi,
    psi; restraint centre) -- row ``l`` of every returned array is what ``FES(...).generate_fes(u_n=u_l, x_n, fes_type="kde",
    kde_parameters={"bandwidth": bandwidth})`` and ``get_fes(queries, reference_point, fes_reference)`` return for the dense member
    ``u_l``, without a dense ``u_l``, an upload or a weight evaluation per member, and, unlike :func:`compute_scan_fes`, without bins
    that must all hold samples.

    ``x_n``: ``(N,)`` or ``(N, d)`` with ``d`` 1 or 2; ``queries``: ``(M,)`` or ``(M, d)``, any ``M >= 1``; ``bandwidth`` positive and
    finite.  The family (``basis_bn``, ``coeff_lb``, ``offset_l``, ``center_lb``, ``harmonic_b``, ``period_b``) is that of
    :func:`compute_scan`.  ``kernel``: "gaussian" only (the other sklearn kernels are offered by ``FES(fes_type="kde")``).  ``period``:
    ``(d,)``, 0 = not periodic; where positive, the displacement of that coordinate is the minimum image ``dl - P rint(dl / P)``, formed
    by the operations of a periodic harmonic term, so a torsion surface is continuous over the +-180 degree seam.  The normaliser stays
    the unwrapped kernel's: exact to ``erfc(P / (2 sqrt(2) h))`` per periodic coordinate, i.e. for ``h << P``.  ``period=None`` is
    ``zeros(d)``, to the bit.

    Returns a dict: ``f`` ``(L,)``, the bits of :func:`compute_scan`; ``log_density`` ``(L, M)``, what
    ``KernelDensity(bandwidth=h).fit(x_n, sample_weight=w_l).score_samples(queries)`` gives for the dense member's weights ``w_l``;
    ``f_i`` ``(L, M)`` and ``reference`` ``(L,)`` by ``reference_point`` as ``FES.get_fes`` applies it per member -- "from-lowest" (the
    member's lowest query, its index in ``reference``), "from-specified" (the density at ``fes_reference``, evaluated as one more query;
    ``reference`` -1), "from-normalization" (``f_i = -log_density``; -1); ``n_exact``: the (member, query) pairs whose kernel terms
    all underflowed and that the device recomputed in log space.

    ``uncertainty_method``: None or "bootstrap" -- adds ``bootstrapped_log_density`` ``(n_bootstraps, L, M)`` and ``df_i``, the ``std``
    over the replicates of ``f^b_lm - f^b_l,ref`` with the reference query taken from the main estimate.  A replicate is what it is in
    :func:`compute_scan_fes`: that replicate's multiplicities and ``f_k_boots[b]``.  (Deliberately not the reference's KDE replicate,
    which refits resampled positions with the weights of the full sample.)

    The sums are one ``(M x N)(N x L)`` product on the fp64 matrix cores with both operands generated on the device
    (``DeviceMatrix.scan_kde_sums``): one member exponential serves up to 128 queries, one kernel exponential every member of a panel."""
    from .kde import KERNELS, log_normaliser

    basis_given = basis_bn
    if kernel != "gaussian":
        if kernel in KERNELS:
            raise ParameterError(f"kernel {kernel!r} is offered by FES(fes_type=\"kde\") only: kernel-density surfaces along a scan are gaussian")
        raise ParameterError(f"kernel must be one of {KERNELS}, got {kernel!r}")
    if reference_point not in ("from-lowest", "from-specified", "from-normalization"):
        raise ParameterError(f"reference point choice {reference_point} for kde is unavailable")
    if uncertainty_method not in (None, "bootstrap"):
        raise ParameterError(f"Uncertainty method {uncertainty_method} for kde is not implemented")
    bootstrap = uncertainty_method == "bootstrap"
    if bootstrap and (mbar.n_bootstraps is None or mbar.n_bootstraps <= 0):
        raise ParameterError("Cannot request bootstrap sampling of expectations without any bootstraps.")
    try:
        h = float(bandwidth)
    except (TypeError, ValueError):
        raise ParameterError(f"bandwidth must be a positive float, got {bandwidth!r}") from None
    if not (h > 0.0 and np.isfinite(h)):
        raise ParameterError(f"bandwidth must be a positive float, got {bandwidth!r}")
    x_dn, q_dm, d, M = _kde_points(mbar, x_n, queries, fes_reference, reference_point)
    if period is not None:
        period = np.ascontiguousarray(period, dtype=np.float64)
        if period.shape != (d,) or not np.all(np.isfinite(period)) or np.any(period < 0.0):
            raise ParameterError(f"period must have shape ({d},): 0 for a coordinate that is not periodic, its period otherwise")
    basis_bn, coeff_lb, offset_l, _, L = _check_inputs(mbar, _family_basis(mbar, basis_bn, coeff_lb), coeff_lb, offset_l, None, 0)
    kinds, cen = _family_kinds(mbar, basis_given, basis_bn.shape[0], L, center_lb, harmonic_b, period_b)
    dm = _kde_matrix(mbar)
    lognorm = log_normaliser("gaussian", d, h)

    def densities(f_k, f):
        logsum, wsum, n_exact = dm.scan_kde_sums(f_k, coeff_lb, offset_l, f, q_dm, h, period=period, **cen)
        with np.errstate(divide="ignore", invalid="ignore"):
            return (logsum - np.log(wsum)[:, None]) + lognorm, wsum, n_exact

    dm.set_Nk(mbar.N_k)
    dm.set_scan(basis_bn, None, **kinds)
    try:
        dm.set_scan_points(x_dn)
        lognum, _ = dm.scan_lognum(mbar.f_k, coeff_lb, offset_l, **cen)
        f = -lognum
        log_density, wsum, n_exact = densities(mbar.f_k, f)
        check_w_sums(wsum, 0.0)
        f_i, reference = _kde_surface(log_density, M, reference_point)
        out = dict(f=f, log_density=np.ascontiguousarray(log_density[:, :M]), f_i=f_i, reference=reference, n_exact=int(n_exact))
        if bootstrap:
            Lb = np.zeros((mbar.n_bootstraps,) + log_density.shape)
            try:
                for b in range(mbar.n_bootstraps):
                    mbar._set_bootstrap_weights(dm, b)
                    ln_b, _ = dm.scan_lognum(mbar.f_k_boots[b, :], coeff_lb, offset_l, **cen)
                    Lb[b] = densities(mbar.f_k_boots[b, :], -ln_b)[0]
            finally:
                dm.set_sample_weights(None)
            out["bootstrapped_log_density"] = np.ascontiguousarray(Lb[:, :, :M])
            out["df_i"] = _kde_bootstrap_spread(-Lb, reference, reference_point, M)
    finally:
        dm.set_scan_points(None)
        dm.set_scan(None)
    return out


# ---- differences between any two members of a scan --------------------------------------------------------------------------------
def _pairs_matrix(mbar):
    dm = _scan_matrix(mbar)
    if not hasattr(dm, "scan_pair_gram"):
        raise ParameterError(f"differences between the members of a scan need the pair pass of a single-rank device matrix and are {_NOT_HERE} for this handle")
    return dm


def _reference_members(reference_members, L):
    if reference_members is None:
        return np.arange(L, dtype=np.int64)
    members = np.asarray(reference_members)
    if members.ndim != 1 or members.size < 1 or members.dtype.kind not in "iu":
        raise ParameterError("reference_members must be None or a 1-D integer array of at least one member index")
    members = members.astype(np.int64)
    if members.min() < 0 or members.max() >= L or len(np.unique(members)) != len(members):
        raise ParameterError("reference_members must be distinct indices of members of the family")
    return members


def _pairs_analytical(mbar, dm, coeff_lb, offset_l, f, mean, members, approximate, warning_cutoff, cen={}):
    """``(cov_f, dDelta_f, cov_mu, dDelta_mu)`` of DESIGN.md section 23: ``Theta(z_ri, z_lj) = z_ri . z_lj + y(z_ri)^T diag(g) y(z_lj)``
    with ``z_l0 = b_l``, ``z_lq = b_l t_q / mean_lq``; the ``z . z'`` of two different members come from the pair block, a member's own
    from ``within`` as in :func:`_analytical`, the border from the one cross block.  Every entry is formed element by element, the
    eigen-directions summed in ascending order."""
    L, J = mean.shape
    R = len(members)
    cross, within, _, wsum = dm.scan_gram_w(mbar.f_k, coeff_lb, offset_l, f, reference=int(members[0]), cross=not approximate, **cen)
    check_w_sums(wsum, 0.0)
    pair = dm.scan_pair_gram(mbar.f_k, coeff_lb, offset_l, f, members, **cen)
    y = g = None
    if not approximate:
        y, g = _border(mbar, cross)
    scale = np.ones((J, L))  # z_lj = b_l t_j / scale[j, l]
    scale[1:] = mean[:, 1:].T

    def theta(i, j):
        """``Theta(z_ri, z_lj)``, ``(R, L)``"""
        si, sj = scale[i][members], scale[j]
        out = pair[:, :, i, j] / (si[:, None] * sj[None, :])
        if y is not None:
            out = out + _qform(g, (y[:, members, i] / si[None, :])[:, :, None], (y[:, :, j] / sj[None, :])[:, None, :])
        return out

    def own(i, j):
        """``Theta(z_li, z_lj)`` of every member with itself, ``(L,)``"""
        out = within[:, i, j] / (scale[i] * scale[j])
        if y is not None:
            out = out + _qform(g, y[:, :, i] / scale[i][None, :], y[:, :, j] / scale[j][None, :])
        return out

    at_self = (np.arange(R), members)
    t00, d00 = theta(0, 0), own(0, 0)
    d2 = (d00[None, :] + d00[members][:, None]) - 2.0 * t00
    d2[at_self] = 0.0
    cov_mu = np.zeros((J - 1, R, L))
    dmu = np.zeros((J - 1, R, L))
    for q in range(1, J):
        m = mean[:, q]
        var = (m * m) * (own(q, q) + d00 - 2.0 * own(0, q))
        cov_mu[q - 1] = (m[members][:, None] * m[None, :]) * (theta(q, q) - theta(q, 0) - theta(0, q) + t00)
        dq2 = (var[None, :] + var[members][:, None]) - 2.0 * cov_mu[q - 1]
        dq2[at_self] = 0.0
        dmu[q - 1] = _sqrt_small_negative_zeroed(dq2, warning_cutoff)
    return t00, _sqrt_small_negative_zeroed(d2, warning_cutoff), cov_mu, dmu


def _std_of_differences(x_bl, members):
    """``std`` over the replicates of ``x[b, l] - x[b, members[r]]``: ``(R, L)`` (the rule of the reference's
    ``compute_free_energy_differences`` and ``compute_expectations(output="differences")``)."""
    return np.std(x_bl[:, None, :] - x_bl[:, members][:, :, None], axis=0)


def compute_scan_pairs(mbar, basis_bn=None, coeff_lb=None, offset_l=None, A_qn=None, reference_members=None, compute_uncertainty=True,
                       uncertainty_method=None, warning_cutoff=1.0e-10, center_lb=None, harmonic_b=None, period_b=None):
    """Differences between ANY two members of a scan, and their uncertainties: the rows ``reference_members`` of the full ``L x L``
    matrices ``compute_perturbed_free_energies(u_ln)`` and ``compute_expectations(A, u_kn=u_ln, state_dependent=False,
    output="differences")`` return for the dense ``u_ln`` -- the uncertainty of ``f(T_1) - f(T_2)`` between two arbitrary grid points, of
    a finite difference along the grid, of ``Delta f`` between adjacent members.

    The family (``basis_bn``, ``coeff_lb``, ``offset_l``, ``center_lb``, ``harmonic_b``, ``period_b``), ``A_qn``, the limits and the errors
    are those of :func:`compute_scan`.  ``reference_members``: None (all ``L`` members) or a 1-D integer array of ``R`` distinct member
    indices.  Returns a dict, ``r`` running over ``reference_members``: ``f`` ``(L,)`` and with observables ``mu`` ``(Q, L)`` (the bits
    of :func:`compute_scan`); ``members`` ``(R,)``; ``Delta_f[r, l] = f[l] - f[members[r]]`` (the reference's sign); ``cov_f[r, l]``,
    the covariance of ``-f`` of the two members, and ``dDelta_f[r, l] = sqrt(cov_f[r, r'] + cov_f[l, l] - 2 cov_f[r, l])`` with both
    diagonal entries the members' own (exactly 0 for a member with itself); with observables ``Delta_mu``, ``cov_mu``, ``dDelta_mu``
    ``(Q, R, L)`` likewise for ``<A_q>``.  The members' products come from one pass of the device that generates both operands of the
    Gram block from the ``B`` numbers per sample (``DeviceMatrix.scan_pair_gram``) instead of one pass B per reference member.

    ``uncertainty_method``: None / "svd-ew" (the bordered form), "approximate" (``Theta = z . z'``), "bootstrap" (the ``std`` over the
    replicates of the differences; adds ``bootstrapped_f`` and ``bootstrapped_observables`` as :func:`compute_scan` does; no ``cov_f`` /
    ``cov_mu``); "svd" is not offered."""
    basis_given = basis_bn
    if uncertainty_method == "svd":
        raise ParameterError("uncertainty_method 'svd' needs the weight matrix itself and is not offered for scans")
    if uncertainty_method not in (None, "svd-ew", "approximate", "bootstrap"):
        raise ParameterError(f"Method {uncertainty_method} unrecognized.")
    bootstrap = uncertainty_method == "bootstrap"
    if bootstrap and (mbar.n_bootstraps is None or mbar.n_bootstraps <= 0):
        raise ParameterError("Cannot request bootstrap sampling of expectations without any bootstraps.")
    basis_bn, coeff_lb, offset_l, A_qn, L = _check_inputs(mbar, _family_basis(mbar, basis_bn, coeff_lb), coeff_lb, offset_l, A_qn, 0)
    members = _reference_members(reference_members, L)
    kinds, cen = _family_kinds(mbar, basis_given, basis_bn.shape[0], L, center_lb, harmonic_b, period_b)
    dm = _pairs_matrix(mbar)
    Q = len(A_qn)
    t_qn, shift = _shifted(A_qn)
    dm.set_Nk(mbar.N_k)
    dm.set_scan(basis_bn, t_qn, **kinds)
    try:
        lognum, mean = dm.scan_lognum(mbar.f_k, coeff_lb, offset_l, **cen)
        f = -lognum
        out = dict(f=f, members=members, Delta_f=f[None, :] - f[members][:, None])
        if Q:
            mu = mean[:, 1:].T + shift[:, None]
            out["mu"] = mu
            out["Delta_mu"] = mu[:, None, :] - mu[:, members][:, :, None]
        if bootstrap:
            fb = np.zeros((mbar.n_bootstraps, L))
            Ab = np.zeros((mbar.n_bootstraps, Q, L))
            try:
                for b in range(mbar.n_bootstraps):
                    mbar._set_bootstrap_weights(dm, b)
                    ln_b, mean_b = dm.scan_lognum(mbar.f_k_boots[b, :], coeff_lb, offset_l, **cen)
                    fb[b] = -ln_b
                    Ab[b] = mean_b[:, 1:].T + shift[:, None]
            finally:
                dm.set_sample_weights(None)
            out["bootstrapped_f"], out["bootstrapped_observables"] = fb, Ab
            if compute_uncertainty:
                out["dDelta_f"] = _std_of_differences(fb, members)
                if Q:
                    out["dDelta_mu"] = np.stack([_std_of_differences(Ab[:, q, :], members) for q in range(Q)])
        elif compute_uncertainty:
            cov_f, ddf, cov_mu, dmu = _pairs_analytical(mbar, dm, coeff_lb, offset_l, f, mean, members, uncertainty_method == "approximate",
                                                        warning_cutoff, cen)
            out["cov_f"], out["dDelta_f"] = cov_f, ddf
            if Q:
                out["cov_mu"], out["dDelta_mu"] = cov_mu, dmu
    finally:
        dm.set_scan(None)
    return out


# ---- entropy, enthalpy and heat capacity along a scan -----------------------------------------------------------------------------
def _thermo_matrix(mbar):
    dm = _scan_matrix(mbar)
    if not all(hasattr(dm, name) for name in ("scan_energy_lognum", "scan_energy_gram_w")):
        raise ParameterError(f"entropy and enthalpy along a scan need the energy passes of a single-rank device matrix and are {_NOT_HERE} for this handle")
    return dm


def _moments(center, mean):
    """``(u, var_u)`` from the centred moments of pass A: ``u = c + <t_1>``, ``var_u = <t_2> - <t_1>^2`` (None at ``J = 2``)."""
    m1 = mean[:, 1]
    return center + m1, (mean[:, 2] - m1 * m1 if mean.shape[1] > 2 else None)


def _theta_pairs(alpha, within, refblock, y, g, r, pairs=True):
    """``Theta(v_l, v_l)``, ``Theta(v_l, v_r)``, ``Theta(v_r, v_r)`` of the columns ``v_l = sum_j alpha[l, j] b_l t_lj`` (DESIGN.md
    section 21): ``v . v'`` from ``within`` (same member) and ``refblock`` (``refblock[l, i, j] = (b_r t_ri) . (b_l t_lj)``; the
    columns that meet the reference member's have ``alpha[r, 2] = 0``), plus the border ``y(v)^T diag(g) y(v')`` with ``y`` linear in
    the column.  ``y=None``: the ``v . v'`` terms alone ("approximate").  Sums over ``i``, ``j`` and the eigen-directions in
    ascending order, element by element.  ``pairs=False``: ``Theta(v_l, v_l)`` only."""
    L, J = alpha.shape
    ll = np.zeros(L)
    for i in range(J):
        for j in range(J):
            ll += alpha[:, i] * alpha[:, j] * within[:, i, j]
    yv = None
    if y is not None:
        yv = np.zeros(y.shape[:2])
        for j in range(J):
            yv += alpha[None, :, j] * y[:, :, j]
        ll = ll + _qform(g, yv, yv)
    if not pairs:
        return ll
    lr = np.zeros(L)
    for i in range(2):
        for j in range(J):
            lr += alpha[r, i] * alpha[:, j] * refblock[:, i, j]
    rr = ll[r]
    if yv is not None:
        lr = lr + _qform(g, yv, yv[:, r:r + 1])
    return ll, lr, rr


def _thermo_analytical(mbar, dm, coeff_lb, offset_l, f, center, mean, reference, approximate, warning_cutoff, cen={}):
    """The uncertainties of section 21 from pass B with the energy observable.  With ``a_l = b_l`` and ``d_lj = b_l t_lj - mean_lj
    b_l`` the columns are ``a`` (``ln c``: the free energy), ``d_1`` (``u``), ``d_1 + a`` (``s = u - f``) and, for the fluctuation,
    ``d_2 - 2 mean_1 d_1`` (the delta method); none of them divides by a mean, which is ~ 0 by construction here."""
    L, J = mean.shape
    r = int(reference)
    cross, within, refblock, wsum = dm.scan_energy_gram_w(mbar.f_k, coeff_lb, offset_l, f, center_u=center, J=J, reference=r,
                                                          cross=not approximate, **cen)
    check_w_sums(wsum, 0.0)
    y = g = None
    if not approximate:
        y, g = _border(mbar, cross)
    m1 = mean[:, 1]
    zero, one = np.zeros(L), np.ones(L)
    pad = [zero] * (J - 2)
    columns = dict(f=np.stack([one, zero] + pad, axis=1), u=np.stack([-m1, one] + pad, axis=1), s=np.stack([one - m1, one] + pad, axis=1))
    out = {}
    for name, alpha in columns.items():
        ll, lr, rr = _theta_pairs(alpha, within, refblock, y, g, r)
        d2 = ll + rr - 2.0 * lr
        d2[r] = 0.0
        out["dDelta_" + name] = _sqrt_small_negative_zeroed(d2, warning_cutoff)
    if J > 2:
        alpha = np.stack([2.0 * m1 * m1 - mean[:, 2], -2.0 * m1, one], axis=1)
        with np.errstate(invalid="ignore"):
            out["dvar_u"] = np.sqrt(_theta_pairs(alpha, within, refblock, y, g, r, pairs=False))
    out["n_eff"] = 1.0 / within[:, 0, 0]  # Kish's effective sample number of the member
    return out


def compute_scan_entropy_and_enthalpy(mbar, basis_bn=None, coeff_lb=None, offset_l=None, reference=0, fluctuation=True, compute_uncertainty=True,
                                      uncertainty_method=None, warning_cutoff=1.0e-10, center_lb=None, harmonic_b=None, period_b=None):
    """Free energy, reduced enthalpy, entropy and the fluctuation of the reduced potential along a family of unsampled states.

    The family (``basis_bn``, ``coeff_lb``, ``offset_l``, ``center_lb``, ``harmonic_b``, ``period_b``) and ``reference`` are those of
    :func:`compute_scan`; the observable is each member's own reduced potential ``u_l(n)``, which the device forms from the chain it
    evaluates anyway -- nothing of size ``L x N`` is built.  Returns a dict of ``(L,)`` arrays: ``f``, ``u = <u_l>_l``, ``s = u - f``,
    their differences to member ``reference`` ``Delta_f``, ``Delta_u``, ``Delta_s`` with the uncertainties ``dDelta_f``,
    ``dDelta_u``, ``dDelta_s`` -- row ``reference`` of ``compute_entropy_and_enthalpy(u_kn=u_ln)`` for the dense ``u_ln`` --, and with
    ``fluctuation`` ``var_u = <u_l^2>_l - <u_l>_l^2`` (``C_v / k_B`` on a temperature ladder) and ``dvar_u``.  With analytical
    uncertainties also ``n_eff``, Kish's effective sample number ``1 / sum_n b_ln^2`` of every member.

    ``uncertainty_method``: None / "svd-ew" (the bordered form), "approximate", "bootstrap" (the ``std`` over replicates of the
    differences, as ``compute_entropy_and_enthalpy`` takes it, and of ``var_u``; adds ``bootstrapped_f``, ``bootstrapped_u`` and
    ``bootstrapped_var_u`` ``(n_bootstraps, L)``); "svd" is not offered."""
    basis_given = basis_bn
    if uncertainty_method == "svd":
        raise ParameterError("uncertainty_method 'svd' needs the weight matrix itself and is not offered for scans")
    if uncertainty_method not in (None, "svd-ew", "approximate", "bootstrap"):
        raise ParameterError(f"Method {uncertainty_method} unrecognized.")
    bootstrap = uncertainty_method == "bootstrap"
    if bootstrap and (mbar.n_bootstraps is None or mbar.n_bootstraps <= 0):
        raise ParameterError("Cannot request bootstrap sampling of expectations without any bootstraps.")
    basis_bn, coeff_lb, offset_l, _, L = _check_inputs(mbar, _family_basis(mbar, basis_bn, coeff_lb), coeff_lb, offset_l, None, reference)
    kinds, cen = _family_kinds(mbar, basis_given, basis_bn.shape[0], L, center_lb, harmonic_b, period_b)
    dm = _thermo_matrix(mbar)
    r = int(reference)
    J = 3 if fluctuation else 2
    dm.set_Nk(mbar.N_k)
    dm.set_scan(basis_bn, None, **kinds)
    try:
        # pass A twice: about zero for <u_l>, then about that mean, so that neither u nor var_u carries a cancellation of order <u>^2
        _, mean0 = dm.scan_energy_lognum(mbar.f_k, coeff_lb, offset_l, center_u=None, J=2, **cen)
        center = mean0[:, 1].copy()
        lognum, mean = dm.scan_energy_lognum(mbar.f_k, coeff_lb, offset_l, center_u=center, J=J, **cen)
        f = -lognum
        u, var_u = _moments(center, mean)
        s = u - f
        out = dict(f=f, Delta_f=f - f[r], u=u, Delta_u=u - u[r], s=s, Delta_s=s - s[r])
        if fluctuation:
            out["var_u"] = var_u
        if bootstrap:
            nb = mbar.n_bootstraps
            fb, ub, vb = np.zeros((nb, L)), np.zeros((nb, L)), np.zeros((nb, L))
            try:
                for b in range(nb):
                    mbar._set_bootstrap_weights(dm, b)
                    ln_b, mean_b = dm.scan_energy_lognum(mbar.f_k_boots[b, :], coeff_lb, offset_l, center_u=center, J=J, **cen)
                    fb[b] = -ln_b
                    ub[b], v = _moments(center, mean_b)
                    if fluctuation:
                        vb[b] = v
            finally:
                dm.set_sample_weights(None)
            out["bootstrapped_f"], out["bootstrapped_u"] = fb, ub
            if fluctuation:
                out["bootstrapped_var_u"] = vb
            if compute_uncertainty:
                for name, arr in (("dDelta_f", fb), ("dDelta_u", ub), ("dDelta_s", ub - fb)):
                    out[name] = np.std(arr - arr[:, r:r + 1], axis=0)
                if fluctuation:
                    out["dvar_u"] = np.std(vb, axis=0)
        elif compute_uncertainty:
            out.update(_thermo_analytical(mbar, dm, coeff_lb, offset_l, f, center, mean, r, uncertainty_method == "approximate",
                                          warning_cutoff, cen))
    finally:
        dm.set_scan(None)
    return out


# ---- derivatives of f and of the averages along a scan ----------------------------------------------------------------------------
def _gradient_matrix(mbar):
    dm = _scan_matrix(mbar)
    if not hasattr(dm, "scan_moments"):
        raise ParameterError(f"derivatives along a scan need the moments pass of a single-rank device matrix and are {_NOT_HERE} for this handle")
    return dm


def gradient_layout(B, harmonic_b=None):
    """``(features, params)`` of a family of ``B`` terms.  ``features``: ``(b, kind)`` of every feature the moments pass returns, in
    its order -- ``(b, "basis")`` of a linear term, ``(b, "dl")`` then ``(b, "dl2")`` of a harmonic one.  ``params``: ``("coeff", b)``
    for every ``b``, then ``("center", b)`` for the harmonic ``b`` ascending."""
    harmonic = np.zeros(B, dtype=bool) if harmonic_b is None else np.asarray(harmonic_b, dtype=bool)
    features = []
    for b in range(B):
        features += [(b, "dl"), (b, "dl2")] if harmonic[b] else [(b, "basis")]
    params = [("coeff", b) for b in range(B)] + [("center", b) for b in range(B) if harmonic[b]]
    return features, params


def gradient_from_moments(coeff_lb, harmonic_b, center_phi, m1, m2, ma=None, mean=None, hessian=True):
    """The chain rule on the centred moments of one moments pass (``center_phi``, ``m1``, ``m2``, ``ma``, ``mean`` as
    ``DeviceMatrix.scan_moments`` takes and returns them): a dict with ``feature_mean = center_phi + m1``, ``feature_cov = m2 - m1
    m1^T``, ``grad_f`` ``(L, P)``, ``hess_f`` ``(L, P, P)`` and, with observables, ``grad_mu`` ``(Q, L, P)``.  Every parameter's
    ``g = du/dp`` is one feature times a factor -- a linear ``coeff_b``: ``basis_b``; a harmonic ``coeff_b``: ``dl_b^2``; ``center_b``:
    ``-2 coeff_lb dl_b`` -- so ``grad_f = <g>``, ``hess_f = <h> - Cov(g, g')`` with ``h(center_b, center_b) = 2 coeff_lb``, ``h(coeff_b,
    center_b) = -2 dl_b`` and 0 otherwise, ``grad_mu = -Cov(A, g)``.  Explicit ascending loops, element by element over the members: a
    member's numbers do not depend on the others."""
    coeff_lb = np.asarray(coeff_lb, dtype=np.float64)
    L, B = coeff_lb.shape
    features, params = gradient_layout(B, harmonic_b)
    F, P = len(features), len(params)
    slot = {fk: i for i, fk in enumerate(features)}
    fmean = center_phi + m1
    fcov = np.empty((L, F, F))
    for i in range(F):
        for j in range(F):
            fcov[:, i, j] = m2[:, i, j] - m1[:, i] * m1[:, j]
    # g_p = scale[:, p] * feature idx[p]
    idx, scale = [], np.ones((L, P))
    for p, (kind, b) in enumerate(params):
        if kind == "coeff":
            idx.append(slot[(b, "dl2")] if (b, "dl2") in slot else slot[(b, "basis")])
        else:
            idx.append(slot[(b, "dl")])
            scale[:, p] = -2.0 * coeff_lb[:, b]
    out = dict(feature_mean=fmean, feature_cov=fcov)
    grad = np.empty((L, P))
    for p in range(P):
        grad[:, p] = scale[:, p] * fmean[:, idx[p]]
    out["grad_f"] = grad
    if hessian:
        hess = np.empty((L, P, P))
        for p in range(P):
            for r in range(p, P):
                h = -(scale[:, p] * scale[:, r]) * fcov[:, idx[p], idx[r]]
                (kp, bp), (kr, br) = params[p], params[r]
                if bp == br and kp == "center" and kr == "center":
                    h = 2.0 * coeff_lb[:, bp] + h
                elif bp == br and kp == "coeff" and kr == "center":
                    h = -2.0 * fmean[:, slot[(bp, "dl")]] + h
                hess[:, p, r] = h
                hess[:, r, p] = h
        out["hess_f"] = hess
    if ma is not None and ma.shape[1] > 0:
        Q = ma.shape[1]
        gmu = np.empty((Q, L, P))
        for q in range(Q):
            for p in range(P):
                gmu[q, :, p] = -scale[:, p] * (ma[:, q, idx[p]] - mean[:, 1 + q] * m1[:, idx[p]])
        out["grad_mu"] = gmu
    return out


def compute_scan_gradient(mbar, basis_bn=None, coeff_lb=None, offset_l=None, A_qn=None, hessian=True, uncertainty_method=None,
                          center_lb=None, harmonic_b=None, period_b=None):
    """The derivatives of the free energy and of the averages along a family of unsampled states with respect to the family's own
    parameters: which way ``f`` and ``<A>`` move.

    The family (``basis_bn``, ``coeff_lb``, ``offset_l``, ``center_lb``, ``harmonic_b``, ``period_b``) and ``A_qn`` are those of
    :func:`compute_scan`.  The parameters are listed in the returned ``params``: ``("coeff", b)`` for every ``b``, then ``("center",
    b)`` for the harmonic ``b`` ascending, ``P = B + H``.  With ``g = du_l/dp`` and ``h = d2u_l/dp dp'``, all averages in member ``l``:

    * ``f`` ``(L,)``: the bits of :func:`compute_scan`;
    * ``grad_f`` ``(L, P)``: ``df/dp = <g>``;
    * ``hess_f`` ``(L, P, P)`` (with ``hessian``): ``d2f/dp dp' = <h> - Cov(g, g')``, symmetric;
    * with observables ``mu`` ``(Q, L)``, the bits of :func:`compute_scan`, and ``grad_mu`` ``(Q, L, P)``: ``d<A>/dp = -Cov(A, g)``;
    * ``feature_mean`` ``(L, F)`` and ``feature_cov`` ``(L, F, F)``: the raw moments of the features ``features`` lists (``(b,
      "basis")`` of a linear term, ``(b, "dl")`` and ``(b, "dl2")`` -- the wrapped displacement from the member's centre and its square --
      of a harmonic one) from which the chain rule forms the rest.

    The offset is not a parameter: ``df/doffset = 1`` and every covariance with it vanishes.  The device evaluates ``u_l`` once per
    (member, sample) and accumulates the moments of what the chain is made of next to the sums of :func:`compute_scan`; nothing of
    size ``L x N`` is built.  The pass runs twice, about zero and then about the feature means, so that no covariance carries a
    cancellation of order ``<phi>^2``.

    The derivative with respect to the centre of a PERIODIC harmonic term is the almost-everywhere one: ``u`` is continuous where a
    sample crosses the seam ``dl = +-P / 2`` but its slope has a kink there, which the second derivative does not see.

    ``uncertainty_method``: None (no uncertainties) or "bootstrap" -- one pass per replicate under that replicate's multiplicities and
    free energies, about the centres of the full sample; adds ``bootstrapped_f``, ``bootstrapped_grad_f``, ``bootstrapped_hess_f``,
    ``bootstrapped_mu``, ``bootstrapped_grad_mu``, ``bootstrapped_feature_mean``, ``bootstrapped_feature_cov`` (replicate first) and
    ``df``, ``dgrad_f``, ``dhess_f``, ``dmu``, ``dgrad_mu``, the ``std`` over the replicates.  Analytical uncertainties are not offered."""
    basis_given = basis_bn
    if uncertainty_method not in (None, "bootstrap"):
        raise ParameterError(f"uncertainty_method {uncertainty_method} is not offered for the derivatives along a scan: None or 'bootstrap'")
    bootstrap = uncertainty_method == "bootstrap"
    if bootstrap and (mbar.n_bootstraps is None or mbar.n_bootstraps <= 0):
        raise ParameterError("Cannot request bootstrap sampling of expectations without any bootstraps.")
    basis_bn, coeff_lb, offset_l, A_qn, L = _check_inputs(mbar, _family_basis(mbar, basis_bn, coeff_lb), coeff_lb, offset_l, A_qn, 0)
    B = basis_bn.shape[0]
    kinds, cen = _family_kinds(mbar, basis_given, B, L, center_lb, harmonic_b, period_b)
    dm = _gradient_matrix(mbar)
    hb = kinds.get("harmonic_b")
    features, params = gradient_layout(B, hb)
    Q = len(A_qn)
    t_qn, shift = _shifted(A_qn)

    def derived(lognum, mean, m1, m2, ma, center):
        res = gradient_from_moments(coeff_lb, hb, center, m1, m2, ma, mean, hessian)
        res["f"] = -lognum
        if Q:
            res["mu"] = mean[:, 1:].T + shift[:, None]
        return res

    dm.set_Nk(mbar.N_k)
    dm.set_scan(basis_bn, t_qn, **kinds)
    try:
        _, _, m1_0, _, _ = dm.scan_moments(mbar.f_k, coeff_lb, offset_l, None, **cen)
        center = np.ascontiguousarray(m1_0)
        out = derived(*dm.scan_moments(mbar.f_k, coeff_lb, offset_l, center, **cen), center)
        out.update(params=params, features=features)
        if bootstrap:
            names = [k for k in ("f", "grad_f", "hess_f", "mu", "grad_mu", "feature_mean", "feature_cov") if k in out]
            boots = {k: np.zeros((mbar.n_bootstraps,) + out[k].shape) for k in names}
            try:
                for b in range(mbar.n_bootstraps):
                    mbar._set_bootstrap_weights(dm, b)
                    res_b = derived(*dm.scan_moments(mbar.f_k_boots[b, :], coeff_lb, offset_l, center, **cen), center)
                    for k in names:
                        boots[k][b] = res_b[k]
            finally:
                dm.set_sample_weights(None)
            for k in names:
                out["bootstrapped_" + k] = boots[k]
                if not k.startswith("feature"):
                    out["d" + k] = np.std(boots[k], axis=0)
    finally:
        dm.set_scan(None)
    return out


# ---- histogram free energy surfaces along a scan ----------------------------------------------------------------------------------
def _scan_fes_matrix(mbar):
    dm = _scan_matrix(mbar)
    if not all(hasattr(dm, name) for name in ("set_scan_bins", "scan_bin_lognum", "scan_bin_gram_w")):
        raise ParameterError(f"histogram surfaces along a scan need the binned scan passes of a single-rank device matrix and are {_NOT_HERE} for this handle")
    return dm


def _reference_bins(f_raw, reference, reference_label):
    """``j_l``: the reference bin of every member (``fes._reference_bin`` per row)."""
    if reference == "from-lowest":
        return np.argmin(f_raw, axis=1).astype(np.int64)
    return np.full(len(f_raw), int(reference_label), dtype=np.int64)


def _neg_logsumexp_neg(f_raw):
    """``-logsumexp_i(-f_raw[l, i])``, summed over the bins in ascending order, row by row."""
    m = np.max(-f_raw, axis=1)
    s = np.zeros(len(f_raw))
    for i in range(f_raw.shape[1]):
        s += np.exp(-f_raw[:, i] - m)
    return -(m + np.log(s))


def _fes_analytical(mbar, dm, coeff_lb, offset_l, f_raw, j_l, approximate, cen={}):
    """``df_i`` of every member from pass B: ``Theta_ij = delta_ij d_li + y_li^T diag(g) y_lj`` (DESIGN.md section 16's border,
    per member), ``df^2 = Theta_ii + Theta_jj - 2 Theta_ij``."""
    L = len(f_raw)
    rows = np.arange(L)
    cross, d, wsum = dm.scan_bin_gram_w(mbar.f_k, coeff_lb, offset_l, f_raw, cross=not approximate, **cen)
    check_w_sums(wsum.ravel(), 0.0)
    dj = d[rows, j_l][:, None]
    if approximate:
        var = d + dj
    else:
        y, g = _border(mbar, cross)  # (m, L, nbins)
        yj = y[:, rows, j_l][:, :, None]
        var = (d + _qform(g, y, y)) + (dj + _qform(g, yj, yj)) - 2.0 * _qform(g, y, yj)
    var[rows, j_l] = 0.0
    return np.sqrt(np.maximum(var, 0.0))


def compute_scan_fes(mbar, basis_bn=None, coeff_lb=None, offset_l=None, sample_label=None, reference="from-lowest", reference_label=None,
                     uncertainty_method=None, theta_method=None, warning_cutoff=1.0e-10, center_lb=None, harmonic_b=None, period_b=None):
    """Histogram free energy surfaces of every member of a linear family of unsampled states: row ``l`` of every returned array
    is what ``fes.histogram_fes_labels(mbar, coeff_lb[l] @ basis_bn + offset_l[l], sample_label, reference, reference_label, ...)``
    returns, without a dense ``u_l``, an upload or a read of the resident matrix per member.

    ``basis_bn`` (None: the constructor's basis of ``MBAR.from_linear``), ``coeff_lb``, ``offset_l`` as in :func:`compute_scan`; ``sample_label`` as :func:`pymbar_amd.fes.label_samples`
    returns it (``[-1, nbins)``, every label below ``nbins = max + 1`` occurring).  Returns a dict: ``f_raw`` ``(L, nbins)``, the
    bin free energies in the gauge of ``mbar.f_k``; ``reference`` ``(L,)``, the reference bin ``j_l`` of every member (its lowest
    bin for "from-lowest", ``reference_label`` for "from-specified"); ``f_i = f_raw - f_raw[l, j_l]``; ``f`` ``(L,)``, ``-logsumexp_i(
    -f_raw[l])``, the free energy of the member restricted to the binned samples.  ``uncertainty_method``: None, "analytical"
    (``df_i``; ``theta_method`` None / "svd-ew": the bordered form, "approximate": the bin block alone, "svd": not offered) or
    "bootstrap" (``bootstrapped_f_raw`` ``(n_bootstraps, L, nbins)`` and ``df_i``, the ``std`` over the replicates of ``f^b_li -
    f^b_lj`` with ``j`` from the main estimate; a replicate that emptied the bin or the reference bin is left out, fewer than two
    usable replicates give NaN).  ``center_lb``, ``harmonic_b``, ``period_b``: a family with harmonic terms, as in
    :func:`compute_scan`."""
    from .fes import _check_labels

    basis_given = basis_bn

    if uncertainty_method not in (None, "analytical", "bootstrap"):
        raise ParameterError(f"Uncertainty_method {uncertainty_method} is not a valid option")
    if theta_method == "bootstrap":
        theta_method = None
    if theta_method == "svd":
        raise ParameterError("theta_method 'svd' needs the weight matrix itself and is not offered on the label path")
    if theta_method not in (None, "svd-ew", "approximate"):
        raise ParameterError(f"Method {theta_method} unrecognized.")
    bootstrap = uncertainty_method == "bootstrap"
    if bootstrap and (mbar.n_bootstraps is None or mbar.n_bootstraps <= 0):
        raise ParameterError("Cannot request bootstrap sampling of expectations without any bootstraps.")
    basis_bn, coeff_lb, offset_l, _, L = _check_inputs(mbar, _family_basis(mbar, basis_bn, coeff_lb), coeff_lb, offset_l, None, 0)
    if sample_label is None:
        raise ParameterError("sample_label must have one entry per sample")
    _, sample_label, nbins = _check_labels(mbar, np.zeros(mbar.N), sample_label)
    counts = np.bincount(sample_label[sample_label >= 0], minlength=nbins)
    if np.any(counts == 0):
        raise DataError(f"WARNING: bin {int(np.where(counts == 0)[0][0])} has no samples -- all bins must have at least one sample.")
    if reference == "from-specified":
        if reference_label is None or not (0 <= int(reference_label) < nbins):
            raise ParameterError("Specified reference point for FES not given")
    elif reference != "from-lowest":
        raise ParameterError(f"reference point method {reference} is not supported for histogram surfaces here")
    kinds, cen = _family_kinds(mbar, basis_given, basis_bn.shape[0], L, center_lb, harmonic_b, period_b)
    dm = _scan_fes_matrix(mbar)
    dm.set_Nk(mbar.N_k)
    dm.set_scan(basis_bn, None, **kinds)
    try:
        dm.set_scan_bins(nbins, sample_label)
        f_raw = -dm.scan_bin_lognum(mbar.f_k, coeff_lb, offset_l, **cen)
        j_l = _reference_bins(f_raw, reference, reference_label)
        rows = np.arange(L)
        out = dict(f_raw=f_raw, f_i=f_raw - f_raw[rows, j_l][:, None], reference=j_l, f=_neg_logsumexp_neg(f_raw))
        if bootstrap:
            fb = np.zeros((mbar.n_bootstraps, L, nbins))
            try:
                for b in range(mbar.n_bootstraps):
                    mbar._set_bootstrap_weights(dm, b)
                    fb[b] = -dm.scan_bin_lognum(mbar.f_k_boots[b, :], coeff_lb, offset_l, **cen)
            finally:
                dm.set_sample_weights(None)
            out["bootstrapped_f_raw"] = fb
            with np.errstate(invalid="ignore"):
                fall = fb - fb[:, rows, j_l][:, :, None]  # (inf - inf = NaN: the reference bin was emptied)
            fall[~np.isfinite(fall)] = np.nan
            usable = np.sum(~np.isnan(fall), axis=0)
            df = np.full((L, nbins), np.nan)
            ok = usable >= 2
            if np.any(ok):
                df[ok] = np.nanstd(fall[:, ok], axis=0)
            out["df_i"] = df
        elif uncertainty_method == "analytical":
            out["df_i"] = _fes_analytical(mbar, dm, coeff_lb, offset_l, f_raw, j_l, theta_method == "approximate", cen)
    finally:
        dm.set_scan_bins(0)
        dm.set_scan(None)
    return out
