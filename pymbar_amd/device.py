"""Device-resident reduced-potential matrix: the Python face of one ``mbar_ctx`` (include/mbar_hip.h).

A :class:`DeviceMatrix` holds this rank's column shard of ``u_kn`` in HBM for as long as the object
lives, so the many sweeps of a solve touch PCIe only with K-sized vectors.  It can be passed to every
function of :mod:`pymbar_amd.mbar_solvers` in place of the numpy ``u_kn`` (they upload a temporary
one when handed a numpy array).  The reference keeps ``u_kn`` in host RAM and re-sends it on every
jitted call (pymbar/mbar_solvers.py:255-257).
"""
import ctypes as C

import numpy as np

from . import _lib


_dptr = _lib.ptr

MAX_BASIS = 8  # MBAR_SCAN_MAX_B: basis vectors of a linear family (scans, fill_linear_rows)


def linear_family_inputs(basis_bn, coeff_rb, offset_r=None, error=ValueError):
    """``(basis_bn, coeff_rb, offset_r)`` of a linear family ``u_r(n) = sum_b coeff_rb[r, b] basis_bn[b, n] + offset_r[r]`` as
    float64 C-contiguous arrays, under the rules of :func:`pymbar_amd.scan._check_inputs`: ``basis_bn`` ``(B, N)`` with ``1 <= B <=
    8``, ``coeff_rb`` ``(R, B)`` with ``R >= 1``, ``offset_r`` ``(R,)`` or None (zeros).  A wrong shape raises ``error``, a
    non-finite value :class:`pymbar_amd.utils.DataError`."""
    from .utils import DataError

    basis_bn = np.ascontiguousarray(basis_bn, dtype=np.float64)
    coeff_rb = np.ascontiguousarray(coeff_rb, dtype=np.float64)
    if basis_bn.ndim != 2 or not 1 <= basis_bn.shape[0] <= MAX_BASIS:
        raise error(f"basis_bn must have shape (B, N) with 1 <= B <= {MAX_BASIS}")
    B = basis_bn.shape[0]
    if coeff_rb.ndim != 2 or coeff_rb.shape[1] != B or coeff_rb.shape[0] < 1:
        raise error("the coefficients must have one row per state and one column per basis vector")
    R = coeff_rb.shape[0]
    offset_r = np.zeros(R) if offset_r is None else np.ascontiguousarray(offset_r, dtype=np.float64)
    if offset_r.shape != (R,):
        raise error("the offsets must have one entry per state")
    if not (np.all(np.isfinite(basis_bn)) and np.all(np.isfinite(coeff_rb)) and np.all(np.isfinite(offset_r))):
        raise DataError("basis_bn, the coefficients and the offsets must be finite")
    return basis_bn, coeff_rb, offset_r


MAX_HARMONIC = 4  # MBAR_SCAN_MAX_H: harmonic terms of a family


def family_terms(B, harmonic_b=None, period_b=None, error=ValueError):
    """``(harmonic_b, period_b)`` of a family of ``B`` terms as a bool mask and float64 periods of shape ``(B,)``, or ``(None,
    None)`` for the all-linear family (``harmonic_b`` None or all false).  Term ``b`` of member ``l`` is ``coeff[l, b] basis[b, n]``
    when linear and ``coeff[l, b] w(basis[b, n] - center[l, b])^2`` when harmonic, ``w(d) = d - P rint(d / P)`` the minimum image for
    ``P = period_b[b] > 0`` and ``d`` itself for 0 (``period_b`` None: no term is periodic).  At most 4 terms may be harmonic;
    periods are finite and not negative and read at the harmonic terms only."""
    if harmonic_b is None:
        if period_b is not None and np.any(np.asarray(period_b) != 0):
            raise error("period_b without harmonic_b: only a harmonic term can be periodic")
        return None, None
    harmonic_b = np.asarray(harmonic_b)
    if harmonic_b.shape != (B,) or harmonic_b.dtype != np.bool_:
        raise error("harmonic_b must be a bool mask with one entry per basis vector")
    period_b = np.zeros(B) if period_b is None else np.array(period_b, dtype=np.float64)
    if period_b.shape != (B,):
        raise error("period_b must have one entry per basis vector")
    if int(harmonic_b.sum()) > MAX_HARMONIC:
        raise error(f"at most {MAX_HARMONIC} terms of a family may be harmonic")
    if not np.all(np.isfinite(period_b[harmonic_b])) or np.any(period_b[harmonic_b] < 0):
        raise error("the period of a harmonic term must be finite and not negative (0: not periodic)")
    if not harmonic_b.any():
        return None, None
    period_b[~harmonic_b] = 0.0
    return np.ascontiguousarray(harmonic_b), period_b


def family_centers(center_rb, R, B, harmonic_b, error=ValueError, name="center_kb"):
    """The centres ``(R, B)`` of a family's members as a float64 C-contiguous array (entries of linear terms are not read);
    required whenever a term is harmonic, None otherwise."""
    from .utils import DataError

    if harmonic_b is None:
        return None
    if center_rb is None:
        raise error(f"{name} is required: the family has harmonic terms")
    center_rb = np.ascontiguousarray(center_rb, dtype=np.float64)
    if center_rb.shape != (R, B):
        raise error(f"{name} must have one row per member and one column per basis vector")
    if not np.all(np.isfinite(center_rb[:, harmonic_b])):
        raise DataError(f"{name} must be finite")
    if not np.all(np.isfinite(center_rb)):  # (what no term reads must still be a number the library accepts)
        center_rb = np.where(harmonic_b[None, :], center_rb, 0.0)
    return center_rb


def _solve_result(res):
    """A ``SolveResult`` as the dict the solver functions return."""
    out = {k: getattr(res, k) for k, _ in _lib.SolveResult._fields_}
    out["success"] = bool(res.success)
    return out


class _ContextMatrix:
    """What :class:`DeviceMatrix` and :class:`ExtendedMatrix` share: they own one ``mbar_ctx`` (``_ctx``) and write whole rows of
    it (the row-level assembly of the expectation family).  The two differ in three hooks: where a destination row lives
    (``_dst_row``), where a source run lives (``_src``) and what a write invalidates (``_touched``)."""

    _ctx = None  # (until the constructor has made one: close() of a half-built object has nothing to release)

    def _check(self, rc, arg_error=None):
        if rc != _lib.MBAR_OK:
            _lib.check(rc, self._ctx, arg_error)

    def _f(self, f):
        """The free energies of a call: one per row, as the library reads them."""
        return _lib.f64(f, (self.K,), "f")

    def close(self):
        if self._ctx:
            self._lib.mbar_ctx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- the hooks (these are DeviceMatrix's: every row is the context's own) --------------------------------
    def _dst_row(self, row, n=1):
        """Row of the context that holds row ``row`` of the matrix, the first of ``n`` to be written."""
        return int(row)

    def _src(self, row0, n):
        """(context, row) of a source run of ``n`` rows."""
        return self._ctx, int(row0)

    def _touched(self):
        """The rows are about to change."""

    # ---- row-level assembly of an augmented matrix on the device (expectation family) ----------------------
    def _vec(self, v_n, name):
        """A host vector of N_local entries for the staging vector, contiguous; None stays None (the vector staged before)."""
        return _lib.f64(v_n, (self.N_local,), name, optional=True)

    def upload_rows(self, row0, rows):
        """Whole rows ``[row0, row0 + len(rows))`` from a host array ``rows`` (R, N_local)."""
        rows = _lib.f64(np.atleast_2d(rows), (None, self.N_local), "rows")
        self._touched()
        self._check(self._lib.mbar_ctx_upload_rows(self._ctx, self._dst_row(row0, rows.shape[0]), rows.shape[0], _dptr(rows),
                                                   rows.shape[1]))

    def copy_rows_from(self, src, dst_row0=0, src_row0=0, nrows=None):
        """Device-to-device copy of rows of another resident matrix (same device, same N_local)."""
        self._touched()
        nrows = src.K - src_row0 if nrows is None else nrows
        self._check(self._lib.mbar_ctx_copy_rows(self._ctx, self._dst_row(dst_row0, nrows), src._ctx, int(src_row0), int(nrows)))

    def rows_sub(self, dst_row0, src_row0, nrows, v_n=None):
        """``u[dst_row0 + r, :] = u[src_row0 + r, :] - v_n`` for ``r < nrows`` in one launch (``v_n=None``: the vector of the
        previous call): an observable evaluated at a run of states, the state rows copied and shifted in the same pass."""
        self._touched()
        sctx, srow = self._src(src_row0, nrows)
        v_n = self._vec(v_n, "v_n")
        self._check(self._lib.mbar_ctx_rows_sub_from(self._ctx, self._dst_row(dst_row0, nrows), sctx, srow, int(nrows), _dptr(v_n)))

    def rows_rsub(self, dst_row0, src_row0, nrows):
        """``u[dst_row0 + r, :] = u[src_row0 + r, :] - u[dst_row0 + r, :]`` for ``r < nrows`` in one launch: rows uploaded as
        ``log A`` become observable rows ``u - log A``."""
        self._touched()
        sctx, srow = self._src(src_row0, nrows)
        self._check(self._lib.mbar_ctx_rows_rsub_from(self._ctx, self._dst_row(dst_row0, nrows), sctx, srow, int(nrows)))

    def rows_logshift(self, row0, nrows):
        """Rows ``[row0, row0 + nrows)`` hold raw observable values and become ``log(A - shift)`` in place, ``shift = min A -
        |4 eps min A|`` per row (returned): the reference's shift-to-positive + log (mbar.py:858-867, :886-903) on the device."""
        self._touched()
        shift = np.empty(int(nrows), dtype=np.float64)
        self._check(self._lib.mbar_ctx_rows_logshift(self._ctx, self._dst_row(row0, nrows), int(nrows), _dptr(shift)))
        return shift

    def vec_logshift(self, A_n):
        """One observable ``A_n`` (N_local,) into the staging vector as ``log(A - shift)``; returns ``shift``.  ``rows_sub`` /
        ``row_sub`` with ``v_n=None`` subtract it."""
        A_n = self._vec(A_n, "A_n")
        shift = np.empty(1, dtype=np.float64)
        self._check(self._lib.mbar_ctx_vec_logshift(self._ctx, _dptr(A_n), _dptr(shift)))
        return float(shift[0])


class DeviceMatrix(_ContextMatrix):
    """(K x N_local) fp64 matrix on one MI355X plus the solver state attached to it."""

    def __init__(self, K, N_local, device=None):
        _lib.require_device()
        self._lib = _lib.load_library()
        self.K = int(K)
        self.N_local = int(N_local)
        self.device = _lib.default_device(device)
        self._ctx = C.c_void_p()
        _lib.check(self._lib.mbar_ctx_create(C.byref(self._ctx), self.device, self.K, self.N_local))
        self._Nk = None
        self._version = 0  # bumped by everything that changes the matrix, N_k or the transport
        self._wtag = None  # None = unit sample multiplicities; otherwise a token of the weights last installed
        self._lognum_cache = None
        self._gram_w_cache = None
        self._rowmin_cache = None  # (key, minima) of a run of rows, kept for the ExtendedMatrix objects on this matrix
        self._nbins = 0  # set_bins
        self._scan = None  # (B, Q) of set_scan
        self._scan_harmonic = None  # the bool mask of the scan family's harmonic terms
        self._scan_nbins = 0  # set_scan_bins
        self._scan_obs = 0  # rows of set_scan_observables
        self._scan_pts = 0  # coordinates of set_scan_points
        self._boot_layout_key = None  # the caller's key of the bootstrap layout on the device
        self._cb = None  # keeps the host all-reduce callback alive
        self._loop = None  # keeps the loopback group alive
        self.nranks = 1
        self.rank = 0
        self.allreduce_kind = "none"

    # ---- construction ---------------------------------------------------------------------------
    @classmethod
    def empty(cls, K, N_local, device=None):
        """A zero-filled resident matrix, to be assembled row by row (upload_rows / copy_rows_from / row_sub)."""
        return cls(K, N_local, device=device)

    @classmethod
    def from_host(cls, u_kn, device=None, columns=None):
        """Upload a host ``u_kn`` (K, N) -- or only its ``columns=(n0, n1)`` slice (this rank's shard)."""
        u_kn = _lib.f64(u_kn, (None, None), "u_kn")
        K, N = u_kn.shape
        n0, n1 = (0, N) if columns is None else columns
        dm = cls(K, n1 - n0, device=device)
        dm._check(dm._lib.mbar_ctx_upload_u(dm._ctx, _dptr(u_kn), N, n0, n1 - n0, 0))
        return dm

    @classmethod
    def from_linear(cls, basis_bn, coeff_kb, offset_k=None, device=None, columns=None, validate=True):
        """The matrix ``u[k, n] = sum_b coeff_kb[k, b] basis_bn[b, n] + offset_k[k]`` of a linear family, built ON THE DEVICE from
        the ``B <= 8`` basis vectors: :meth:`from_family` without a harmonic term.  ``validate=False``: the three arrays are what
        :func:`linear_family_inputs` returned (no second pass over the basis)."""
        if validate:
            basis_bn, coeff_kb, offset_k = linear_family_inputs(basis_bn, coeff_kb, offset_k)
        return cls.from_family(basis_bn, coeff_kb, offset_k, device=device, columns=columns, validate=False)

    def fill_linear_rows(self, row0, basis_bn, coeff_rb, offset_r=None, col0=0, validate=True):
        """Rows ``[row0, row0 + R)`` become ``fma(coeff_rb[r, B-1], basis_bn[B-1, n], ... fma(coeff_rb[r, 0], basis_bn[0, n],
        offset_r[r]))`` -- the chain of the scan passes -- on the device: :meth:`fill_family_rows` without a harmonic term.
        ``validate=False`` as in :meth:`from_linear`."""
        if validate:
            basis_bn, coeff_rb, offset_r = linear_family_inputs(basis_bn, coeff_rb, offset_r)
        self.fill_family_rows(row0, basis_bn, coeff_rb, offset_r, col0=col0, validate=False)

    @classmethod
    def from_family(cls, basis_bn, coeff_kb, offset_k=None, center_kb=None, harmonic_b=None, period_b=None, device=None, columns=None,
                    validate=True):
        """The matrix of a family of states (:func:`family_terms`), ``u[k, n] = offset_k[k] + sum_b term_b``, built ON THE DEVICE
        from the ``B <= 8`` basis vectors (``mbar_ctx_fill_family_rows``): ``8 B N`` bytes cross the bus instead of ``8 K N``.  A
        linear term is ``coeff_kb[k, b] basis_bn[b, n]``, a harmonic one ``coeff_kb[k, b] w(basis_bn[b, n] - center_kb[k, b])^2``
        with its minimum image for ``period_b[b] > 0`` -- umbrella sampling on a torsion.  ``columns=(n0, n1)`` as in
        :meth:`from_host`: only that slice of the samples (this rank's shard).  ``validate=False``: the arrays are what
        :func:`linear_family_inputs`, :func:`family_terms` and :func:`family_centers` returned."""
        if validate:
            basis_bn, coeff_kb, offset_k = linear_family_inputs(basis_bn, coeff_kb, offset_k)
            harmonic_b, period_b = family_terms(basis_bn.shape[0], harmonic_b, period_b)
            center_kb = family_centers(center_kb, coeff_kb.shape[0], basis_bn.shape[0], harmonic_b)
        n0, n1 = (0, basis_bn.shape[1]) if columns is None else columns
        dm = cls(coeff_kb.shape[0], n1 - n0, device=device)
        try:
            dm.fill_family_rows(0, basis_bn, coeff_kb, offset_k, center_kb, harmonic_b, period_b, col0=n0, validate=False)
        except BaseException:
            dm.close()
            raise
        return dm

    def fill_family_rows(self, row0, basis_bn, coeff_rb, offset_r=None, center_rb=None, harmonic_b=None, period_b=None, col0=0,
                         validate=True):
        """Rows ``[row0, row0 + R)`` become the chain the scan passes evaluate -- from ``offset_r``, ``b`` ascending,
        ``fma(coeff, basis, u)`` at a linear term and ``d = basis - center; P > 0: d = fma(-P, rint(d (1 / P)), d); fma(coeff, d d,
        u)`` at a harmonic one, every operation rounded once -- on the device.  ``basis_bn`` is ``(B, >= col0 + N_local)``: its
        columns ``[col0, col0 + N_local)`` are this matrix's samples.  With no harmonic term the library runs the kernel of the
        linear family."""
        if validate:
            basis_bn, coeff_rb, offset_r = linear_family_inputs(basis_bn, coeff_rb, offset_r)
            harmonic_b, period_b = family_terms(basis_bn.shape[0], harmonic_b, period_b)
            center_rb = family_centers(center_rb, coeff_rb.shape[0], basis_bn.shape[0], harmonic_b, name="center_rb")
        # (what crosses the ABI is checked whether or not the caller validated: conforming arrays pass through as they are)
        basis_bn = _lib.f64(basis_bn, (None, None), "basis_bn")
        B = basis_bn.shape[0]
        coeff_rb = _lib.f64(coeff_rb, (None, B), "coeff_rb")
        R = coeff_rb.shape[0]
        offset_r = _lib.f64(offset_r, (R,), "offset_r", optional=True)
        center_rb = _lib.f64(center_rb, (R, B), "center_rb", optional=True)
        period_b = _lib.f64(period_b, (B,), "period_b", optional=True)
        col0 = int(col0)
        if col0 < 0 or col0 + self.N_local > basis_bn.shape[1]:
            raise ValueError("basis_bn must cover the columns [col0, col0 + N_local)")
        self._touched()
        kind = None if harmonic_b is None else np.ascontiguousarray(harmonic_b, dtype=np.int32)
        if kind is not None and kind.shape != (B,):
            raise ValueError(f"harmonic_b must have shape ({B},)")
        self._check(self._lib.mbar_ctx_fill_family_rows(self._ctx, int(row0), R, B, _dptr(basis_bn), basis_bn.shape[1], col0,
                                                        _dptr(coeff_rb), _dptr(center_rb), _dptr(offset_r), _dptr(kind, _lib._i32p),
                                                        _dptr(period_b)))

    @classmethod
    def harmonic(cls, O_k, K_k, N_k_global, seed=0, n_global0=0, N_local=None, device=None):
        """Generate the synthetic harmonic ladder of SURVEY.md 8(d) directly in HBM."""
        O_k = _lib.f64(O_k, (None,), "O_k")
        K = len(O_k)
        K_k = _lib.f64(K_k, (K,), "K_k")
        N_k_global = np.ascontiguousarray(N_k_global, dtype=np.int64)
        if N_k_global.shape != (K,):
            raise ValueError(f"N_k_global must have shape ({K},)")
        if N_local is None:
            N_local = int(N_k_global.sum()) - n_global0
        dm = cls(K, N_local, device=device)
        dm._check(dm._lib.mbar_ctx_generate_harmonic(dm._ctx, C.c_uint64(seed), _dptr(O_k), _dptr(K_k), _dptr(N_k_global, _lib._ip),
                                                     n_global0))
        return dm

    def _touched(self):
        self._version += 1  # (the caches of lognum_cached / gram_w_cached and the row minima are keyed by it)

    @property
    def shape(self):
        return (self.K, self.N_local)

    def row_sub(self, row, v_n=None):
        """``u[row, :] -= v_n`` on the device (v = log A_n turns a state row into an observable row).
        ``v_n=None`` subtracts the vector of the previous call again (no upload)."""
        self._touched()
        v_n = self._vec(v_n, "v_n")
        self._check(self._lib.mbar_ctx_row_sub(self._ctx, int(row), _dptr(v_n)))

    def fill_masked_rows(self, row0, nrows, v_n, label_n):
        """Rows ``row0 + i`` (``i < nrows``) become ``v_n`` on the samples with ``label_n == i`` and ``+inf`` (weight zero)
        elsewhere: one extra "state" per histogram bin of a free energy surface, built on the device."""
        v_n = _lib.f64(v_n, (self.N_local,), "v_n")
        label_n = np.ascontiguousarray(label_n, dtype=np.int32)  # (any label is allowed here: one of no row marks no row)
        if label_n.shape != (self.N_local,):
            raise ValueError(f"label_n must have shape ({self.N_local},)")
        self._touched()
        self._check(self._lib.mbar_ctx_fill_masked_rows(self._ctx, int(row0), int(nrows), _dptr(v_n), _dptr(label_n, _lib._i32p)))

    # ---- histogram bins by label (the label path of pymbar_amd.fes) ----------------------------------------------------------
    def set_bins(self, nbins, label_n=None, v_n=None):
        """Bins of a histogram surface as labels of the resident samples: ``label_n`` in ``[-1, nbins)`` (-1: in no bin) and the
        target potential ``v_n``, uploaded once (``mbar_ctx_set_bins``).  ``nbins=0`` releases them."""
        if int(nbins) == 0:
            self._check(self._lib.mbar_ctx_set_bins(self._ctx, 0, None, None))
            self._nbins = 0
            return
        v_n = _lib.f64(v_n, (self.N_local,), "v_n")
        label_n = _lib.labels_i32(label_n, nbins, self.N_local, "label_n")
        # (MBAR_ERR_ARG: a label outside [-1, nbins), or NaN / -inf in v_n)
        self._check(self._lib.mbar_ctx_set_bins(self._ctx, int(nbins), _dptr(label_n, _lib._i32p), _dptr(v_n)), ValueError)
        self._nbins = int(nbins)

    def bins_info(self):
        """``dict(sweeps, chunks, record_bytes)`` of the chunk table ``set_bins`` built."""
        vals = [C.c_int64(0) for _ in range(3)]
        self._check(self._lib.mbar_ctx_bins_info(self._ctx, *[C.byref(v) for v in vals]))
        return dict(sweeps=vals[0].value, chunks=vals[1].value, record_bytes=vals[2].value)

    def bin_lognum(self, f):
        """``log sum_{n in bin i} c_n exp(-v_n - logden_n(f))`` for every bin (``-inf``: no sample with ``c_n > 0``)."""
        f = self._f(f)
        out = np.empty(self._nbins, dtype=np.float64)
        self._check(self._lib.mbar_bin_lognum(self._ctx, _dptr(f), _dptr(out)))
        return out

    def bin_gram_w(self, f, f_bins, cross=True):
        """``(cross, diag, wsum)`` of the bins' normalised weights ``B_n = exp(f_bins[label_n] - v_n - logden_n(f))`` against the
        resident states' ``W``: ``cross[k, i] = sum_{n in i} c_n W_nk B_n`` (``None`` with ``cross=False``), ``diag[i] = sum c_n
        B_n^2``, ``wsum[i] = sum c_n B_n``."""
        f, nbins = self._f(f), self._nbins
        f_bins = _lib.f64(f_bins, (nbins,), "f_bins")
        X = np.empty((self.K, nbins), dtype=np.float64) if cross else None
        d = np.empty(nbins, dtype=np.float64)
        w = np.empty(nbins, dtype=np.float64)
        self._check(self._lib.mbar_bin_gram_w(self._ctx, _dptr(f), _dptr(f_bins), _dptr(X), _dptr(d), _dptr(w)))
        return X, d, w

    # ---- reweighting scans over a linear family of unsampled states (pymbar_amd.scan) -----------------------------------------
    def set_scan(self, basis_bn=None, t_qn=None, harmonic_b=None, period_b=None):
        """The ``B`` basis vectors (``B x N``, ``1 <= B <= 8``) and the ``Q`` shifted observables (``Q x N``, ``Q <= 3``, or
        None) of a scan, uploaded once (``mbar_ctx_set_scan``).  ``basis_bn=None`` releases them.  ``harmonic_b`` / ``period_b``
        (:func:`family_terms`): the kind of the family's terms (``mbar_ctx_set_scan_terms``); the four ``scan_*`` methods then
        need the members' centres ``center_lb``."""
        if basis_bn is not None:  # (what Python can refuse is refused before anything changes)
            basis_bn = _lib.f64(basis_bn, (None, self.N_local), "basis_bn")
            t_qn = np.zeros((0, self.N_local)) if t_qn is None else _lib.f64(t_qn, (None, self.N_local), "t_qn")
            B, Q = basis_bn.shape[0], t_qn.shape[0]
            harmonic_b, period_b = family_terms(B, harmonic_b, period_b)
        self._scan = None
        self._scan_harmonic = None
        if basis_bn is None:
            self._check(self._lib.mbar_ctx_set_scan(self._ctx, 0, None, 0, None))
            return
        # (MBAR_ERR_ARG: B or Q outside the limits)
        self._check(self._lib.mbar_ctx_set_scan(self._ctx, B, _dptr(basis_bn), Q, _dptr(t_qn) if Q else None), ValueError)
        if harmonic_b is not None:
            kind = np.ascontiguousarray(harmonic_b, dtype=np.int32)
            self._check(self._lib.mbar_ctx_set_scan_terms(self._ctx, _dptr(kind, _lib._i32p), _dptr(period_b)), ValueError)
            self._scan_harmonic = harmonic_b
        self._scan = (B, Q)

    def _scan_centers(self, center_lb, L):
        """The centres of the members of the next scan call go to the context (a family with harmonic terms needs them)."""
        harmonic_b = self._scan_harmonic
        if harmonic_b is None:
            if center_lb is not None and np.shape(center_lb) != (L, self._scan[0]):
                raise ValueError("center_lb must have one row per member and one column per basis vector")
            return
        center_lb = family_centers(center_lb, L, self._scan[0], harmonic_b, name="center_lb")
        self._check(self._lib.mbar_ctx_set_scan_centers(self._ctx, L, _dptr(center_lb)), ValueError)

    def _scan_members(self, coeff_lb, offset_l):
        if self._scan is None:
            raise ValueError("no basis on this matrix (set_scan first)")
        coeff_lb = _lib.f64(coeff_lb, (None, self._scan[0]), "coeff_lb")
        L = coeff_lb.shape[0]
        if L < 1:
            raise ValueError("coeff_lb must have one row per member and one column per basis vector")
        offset_l = np.zeros(L) if offset_l is None else _lib.f64(offset_l, (L,), "offset_l")
        return coeff_lb, offset_l, L, 1 + self._scan[1]

    def _scan_pass_a(self, f, coeff_lb, offset_l, center_lb, energy=None):
        """Pass A for the stored observables (``energy=None``) or the energy observable (``energy=(center_u, J)``)."""
        f = self._f(f)
        coeff_lb, offset_l, L, J = self._scan_members(coeff_lb, offset_l)
        head = (self._ctx, _dptr(f), L, _dptr(coeff_lb), _dptr(offset_l))
        if energy is not None:
            center_u, J = self._scan_energy(energy, L)
            head += (_dptr(center_u), J)
        self._scan_centers(center_lb, L)
        lognum = np.empty(L, dtype=np.float64)
        mean = np.empty((L, J), dtype=np.float64)
        call = self._lib.mbar_scan_lognum if energy is None else self._lib.mbar_scan_energy_lognum
        self._check(call(*head, _dptr(lognum), _dptr(mean)))
        return lognum, mean

    def _scan_pass_b(self, f, coeff_lb, offset_l, f_scan, reference, cross, center_lb, energy=None):
        """Pass B for either kind of observable: ``(cross, within, the rows of products with the reference member, wsum)``."""
        f = self._f(f)
        coeff_lb, offset_l, L, J = self._scan_members(coeff_lb, offset_l)
        f_scan = _lib.f64(f_scan, (L,), "f_scan")
        if not 0 <= int(reference) < L:
            raise ValueError("the reference must be a member")
        head = (self._ctx, _dptr(f), L, _dptr(coeff_lb), _dptr(offset_l))
        if energy is not None:
            center_u, J = self._scan_energy(energy, L)
            head += (_dptr(center_u), J)
        self._scan_centers(center_lb, L)
        X = np.empty((self.K, L, J), dtype=np.float64) if cross else None
        tri = np.empty((L, J * (J + 1) // 2), dtype=np.float64)
        ref = np.empty((L, J) if energy is None else (L, 2, J), dtype=np.float64)
        w = np.empty(L, dtype=np.float64)
        call = self._lib.mbar_scan_gram_w if energy is None else self._lib.mbar_scan_energy_gram_w
        self._check(call(*head, _dptr(f_scan), int(reference), _dptr(X), _dptr(tri), _dptr(ref), _dptr(w)))
        within = np.empty((L, J, J), dtype=np.float64)
        iu = np.triu_indices(J)
        within[:, iu[0], iu[1]] = tri
        within[:, iu[1], iu[0]] = tri
        return X, within, ref, w

    @staticmethod
    def _scan_energy(energy, L):
        center_u, J = energy
        if J not in (2, 3):
            raise ValueError("the energy observable takes J = 2 (1, t) or 3 (1, t, t^2)")
        return (np.zeros(L) if center_u is None else _lib.f64(center_u, (L,), "center_u")), int(J)

    def scan_lognum(self, f, coeff_lb, offset_l=None, center_lb=None):
        """Pass A of a scan: ``(lognum, mean)`` with ``lognum[l] = log sum_n c_n exp(-u_l(n) - logden_n(f))`` and ``mean[l, j]``
        the average of ``t_j`` (``t_0 = 1``) in member ``l`` (``L x (1 + Q)``)."""
        return self._scan_pass_a(f, coeff_lb, offset_l, center_lb)

    def scan_gram_w(self, f, coeff_lb, offset_l, f_scan, reference=0, cross=True, center_lb=None):
        """Pass B of a scan: ``(cross, within, refcol, wsum)`` of the members' normalised weights ``b_ln = exp(f_scan[l] - u_l(n) -
        logden_n(f))`` -- ``cross[k, l, j] = sum_n c_n W_nk b_ln t_jn`` (``None`` with ``cross=False``), ``within[l, i, j] = sum_n
        c_n b_ln^2 t_in t_jn`` (symmetric ``J x J``), ``refcol[l, j] = sum_n c_n b_rn b_ln t_jn`` for the reference member ``r``,
        ``wsum[l] = sum_n c_n b_ln``."""
        return self._scan_pass_b(f, coeff_lb, offset_l, f_scan, reference, cross, center_lb)

    SCAN_PAIR_BYTES = 1 << 28  # the pair block of one slab of reference members of scan_pair_gram stays under this

    def scan_pair_gram(self, f, coeff_lb, offset_l, f_scan, rows, center_lb=None, slab=None):
        """The members' own Gram block (``mbar_scan_pair_gram``): ``pair[r, l, i, j] = sum_n c_n (b_rows[r] n t_in)(b_ln t_jn)``, ``R x L
        x J x J``, for the reference members ``rows`` (``R`` indices into the ``L`` members) with ``b`` as in :meth:`scan_gram_w`:
        ``pair[r, :, 0, :]`` is the ``refcol`` of ``scan_gram_w(reference=rows[r])``.  The reference members go to the device in slabs
        (of ``slab`` of them; by default as many as keep a slab's block under 256 MiB): an entry's bits do not depend on the cut."""
        f = self._f(f)
        coeff_lb, offset_l, L, J = self._scan_members(coeff_lb, offset_l)
        f_scan = _lib.f64(f_scan, (L,), "f_scan")
        rows = np.asarray(rows)
        if rows.ndim != 1 or rows.size < 1 or rows.dtype.kind not in "iu" or rows.min() < 0 or rows.max() >= L:
            raise ValueError("rows must be a 1-D integer array of at least one member index in [0, L)")
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        R = rows.shape[0]
        if slab is None:
            slab = self.SCAN_PAIR_BYTES // (8 * L * J * J)
        slab = max(1, min(int(slab), R))
        self._scan_centers(center_lb, L)
        pair = np.empty((R, L, J, J), dtype=np.float64)
        for r0 in range(0, R, slab):
            r1 = min(R, r0 + slab)
            self._check(self._lib.mbar_scan_pair_gram(self._ctx, _dptr(f), L, _dptr(coeff_lb), _dptr(offset_l), _dptr(f_scan), r1 - r0,
                                                      _dptr(rows[r0:r1], _lib._ip), _dptr(pair[r0:r1])))
        return pair

    def scan_energy_lognum(self, f, coeff_lb, offset_l=None, center_u=None, J=3, center_lb=None):
        """Pass A with the member's own reduced potential as the observable (``mbar_scan_energy_lognum``): ``(lognum, mean)`` as
        :meth:`scan_lognum` with ``t_1 = u_l(n) - center_u[l]``, ``t_2 = t_1^2`` (``L x J``, ``J`` 2 or 3; ``center_u`` None: zeros).
        The stored observables of :meth:`set_scan` are ignored; ``lognum`` has the bits of :meth:`scan_lognum`."""
        return self._scan_pass_a(f, coeff_lb, offset_l, center_lb, energy=(center_u, J))

    def scan_energy_gram_w(self, f, coeff_lb, offset_l, f_scan, center_u=None, J=3, reference=0, cross=True, center_lb=None):
        """Pass B with the energy observable (``mbar_scan_energy_gram_w``): ``(cross, within, refblock, wsum)`` as
        :meth:`scan_gram_w` with the member's own ``t_j``; ``refblock[l, i, j] = sum_n c_n (b_rn t_ri)(b_ln t_lj)``, ``i`` 0 or 1."""
        return self._scan_pass_b(f, coeff_lb, offset_l, f_scan, reference, cross, center_lb, energy=(center_u, J))

    def scan_features(self):
        """``(B, H, F)`` of the family :meth:`set_scan` put on the matrix: terms, harmonic terms among them and the features
        :meth:`scan_moments` takes moments of (a linear term's basis vector; a harmonic term's wrapped displacement ``dl`` and
        ``dl^2``), ``F = B + H``."""
        if self._scan is None:
            raise ValueError("no basis on this matrix (set_scan first)")
        B = self._scan[0]
        H = 0 if self._scan_harmonic is None else int(np.count_nonzero(self._scan_harmonic))
        return B, H, B + H

    def scan_moments(self, f, coeff_lb, offset_l=None, center_phi=None, center_lb=None):
        """Pass A of a scan with the moments of the features the chain is made of (``mbar_scan_moments``): ``(lognum, mean, m1, m2,
        ma)``.  ``lognum`` and ``mean`` are :meth:`scan_lognum`'s, to the bit.  Walking the terms in ascending ``b``, a linear term
        contributes the feature ``basis_bn[b]``, a harmonic one ``dl_b`` then ``dl_b^2`` (the wrapped displacement from the member's
        centre, as the chain forms it): ``F = B + H`` features ``phi_i``.  About ``center_phi`` ``(L, F)`` (None: zeros), in member
        ``l``: ``m1[l, i] = <phi_i - c_i>``, ``m2[l, i, j] = <(phi_i - c_i)(phi_j - c_j)>`` (``L x F x F``, symmetric) and ``ma[l, q, i]
        = <t_q (phi_i - c_i)>`` (``L x Q x F``) for the ``Q`` observables of :meth:`set_scan`."""
        f = self._f(f)
        coeff_lb, offset_l, L, J = self._scan_members(coeff_lb, offset_l)
        _, _, F = self.scan_features()
        center_phi = _lib.f64(center_phi, (L, F), "center_phi", optional=True)
        self._scan_centers(center_lb, L)
        lognum = np.empty(L, dtype=np.float64)
        mean = np.empty((L, J), dtype=np.float64)
        m1 = np.empty((L, F), dtype=np.float64)
        tri = np.empty((L, F * (F + 1) // 2), dtype=np.float64)
        ma = np.empty((L, J - 1, F), dtype=np.float64)
        self._check(self._lib.mbar_scan_moments(self._ctx, _dptr(f), L, _dptr(coeff_lb), _dptr(offset_l), _dptr(center_phi), _dptr(lognum),
                                                _dptr(mean), _dptr(m1), _dptr(tri), _dptr(ma) if J > 1 else None), ValueError)
        m2 = np.empty((L, F, F), dtype=np.float64)
        iu = np.triu_indices(F)
        m2[:, iu[0], iu[1]] = tri
        m2[:, iu[1], iu[0]] = tri
        return lognum, mean, m1, m2, ma

    # ---- many observables along a scan (pymbar_amd.scan.compute_scan_expectations) ---------------------------------------------
    SCAN_OBS_BYTES = 1 << 28  # the three L x Q blocks of one slab of members of scan_obs_sums stay under this

    def set_scan_observables(self, a_qn=None):
        """``Q >= 1`` observables (``Q x N``) kept resident for :meth:`scan_obs_sums` (``mbar_ctx_set_scan_obs``), in a block of their
        own: it survives :meth:`set_scan`, a change of term kinds, centres and sample weights.  ``None`` releases it."""
        if a_qn is None:
            self._check(self._lib.mbar_ctx_set_scan_obs(self._ctx, 0, None, 0))
            self._scan_obs = 0
            return
        a_qn = _lib.f64(a_qn, (None, self.N_local), "a_qn")
        if a_qn.shape[0] < 1:
            raise ValueError("a_qn must have at least one row")
        # (MBAR_ERR_ARG: a non-finite entry.  A refused call leaves the library's block, and the count that sizes the outputs, as
        # they were.)
        self._check(self._lib.mbar_ctx_set_scan_obs(self._ctx, a_qn.shape[0], _dptr(a_qn), self.N_local), ValueError)
        self._scan_obs = a_qn.shape[0]

    def scan_obs_sums(self, f, coeff_lb, offset_l, f_scan, second=True, center_lb=None, slab=None):
        """The sums of the resident observables along a scan (``mbar_scan_obs_sums``): ``(s1, t1, t2, wsum, w2sum)`` with ``b_ln`` as in
        :meth:`scan_gram_w` -- ``s1[l, q] = sum_n c_n b_ln a_qn``, ``t1[l, q] = sum_n c_n b_ln^2 a_qn``, ``t2[l, q] = sum_n c_n b_ln^2
        a_qn^2`` (``L x Q``), ``wsum[l] = sum_n c_n b_ln``, ``w2sum[l] = sum_n c_n b_ln^2``; with ``second=False`` only the first-moment
        launches run and ``t1``, ``t2``, ``w2sum`` are None.  The members go to the device in slabs (of ``slab`` members; by default
        as many as keep a slab's blocks under 256 MiB): an entry's bits do not depend on the cut."""
        f = self._f(f)
        coeff_lb, offset_l, L, _ = self._scan_members(coeff_lb, offset_l)
        f_scan = _lib.f64(f_scan, (L,), "f_scan")
        Q = self._scan_obs
        if Q < 1:
            raise ValueError("no observables on this matrix (set_scan_observables first)")
        if center_lb is not None and np.shape(center_lb) != (L, self._scan[0]):
            raise ValueError("center_lb must have one row per member and one column per basis vector")
        if slab is None:
            slab = self.SCAN_OBS_BYTES // (24 * Q)
        slab = max(1, min(int(slab), L))
        s1 = np.empty((L, Q), dtype=np.float64)
        wsum = np.empty(L, dtype=np.float64)
        t1, t2, w2sum = (np.empty((L, Q)), np.empty((L, Q)), np.empty(L)) if second else (None, None, None)
        for l0 in range(0, L, slab):
            l1 = min(L, l0 + slab)
            self._scan_centers(None if center_lb is None else center_lb[l0:l1], l1 - l0)
            part = lambda a: None if a is None else _dptr(a[l0:l1])
            self._check(self._lib.mbar_scan_obs_sums(self._ctx, _dptr(f), l1 - l0, _dptr(coeff_lb[l0:l1]), _dptr(offset_l[l0:l1]),
                                                     _dptr(f_scan[l0:l1]), part(s1), part(t1), part(t2), part(wsum), part(w2sum)))
        return s1, t1, t2, wsum, w2sum

    # ---- kernel-density surfaces along a scan (pymbar_amd.scan.compute_scan_kde) -------------------------------------------------
    SCAN_KDE_BYTES = 1 << 28  # the L x M block of one slab of members of scan_kde_sums stays under this

    def set_scan_points(self, x_dn=None):
        """The ``d = 1`` or ``2`` coordinates of the samples (``d x N``, coordinate-major) kept resident for :meth:`scan_kde_sums`
        (``mbar_ctx_set_scan_points``), in a block of their own: it survives :meth:`set_scan` and the other scan methods.  ``None``
        releases it."""
        if x_dn is None:
            self._check(self._lib.mbar_ctx_set_scan_points(self._ctx, 0, None, 0))
            self._scan_pts = 0
            return
        x_dn = _lib.f64(x_dn, (None, self.N_local), "x_dn")
        if not 1 <= x_dn.shape[0] <= 2:
            raise ValueError("x_dn must have one or two rows of coordinates")
        # (MBAR_ERR_ARG: a non-finite entry.  A refused call leaves the library's block, and the dimension the queries are checked
        # against, as they were.)
        self._check(self._lib.mbar_ctx_set_scan_points(self._ctx, x_dn.shape[0], _dptr(x_dn), self.N_local), ValueError)
        self._scan_pts = x_dn.shape[0]

    def scan_kde_sums(self, f, coeff_lb, offset_l, f_scan, queries_dm, bandwidth, period=None, center_lb=None, slab=None):
        """The gaussian kernel sums of the resident points along a scan (``mbar_scan_kde_sums``): ``(logsum, wsum, n_exact)`` with
        ``b_ln`` as in :meth:`scan_gram_w` -- ``logsum[l, m] = log sum_n c_n b_ln exp(-r^2 / 2h^2)`` (``L x M``), ``r`` the distance from
        sample ``n`` to query ``m`` of ``queries_dm`` (``d x M``, coordinate-major), ``wsum[l] = sum_n c_n b_ln``, ``n_exact`` the number of
        pairs whose terms all underflowed and that were recomputed in log space.  ``period`` (``d`` entries, 0: not periodic): the
        minimum image of that coordinate; None is zeros.  The members go to the device in slabs (of ``slab`` members; by default as
        many as keep a slab's block under 256 MiB): an entry's bits do not depend on the cut."""
        f = self._f(f)
        coeff_lb, offset_l, L, _ = self._scan_members(coeff_lb, offset_l)
        f_scan = _lib.f64(f_scan, (L,), "f_scan")
        d = self._scan_pts
        if d < 1:
            raise ValueError("no points on this matrix (set_scan_points first)")
        queries_dm = _lib.f64(queries_dm, (d, None), "queries_dm")
        M = queries_dm.shape[1]
        if M < 1:
            raise ValueError("queries_dm must have at least one query")
        period = _lib.f64(period, (d,), "period", optional=True)
        if center_lb is not None and np.shape(center_lb) != (L, self._scan[0]):
            raise ValueError("center_lb must have one row per member and one column per basis vector")
        if slab is None:
            slab = self.SCAN_KDE_BYTES // (8 * M)
        slab = max(1, min(int(slab), L))
        logsum = np.empty((L, M), dtype=np.float64)
        wsum = np.empty(L, dtype=np.float64)
        n_exact = 0
        for l0 in range(0, L, slab):
            l1 = min(L, l0 + slab)
            self._scan_centers(None if center_lb is None else center_lb[l0:l1], l1 - l0)
            ne = C.c_int64(0)
            # (MBAR_ERR_ARG: a non-finite query, a bandwidth or a period out of range)
            self._check(self._lib.mbar_scan_kde_sums(self._ctx, _dptr(f), l1 - l0, _dptr(coeff_lb[l0:l1]), _dptr(offset_l[l0:l1]),
                                                     _dptr(f_scan[l0:l1]), M, _dptr(queries_dm), float(bandwidth), _dptr(period),
                                                     _dptr(logsum[l0:l1]), _dptr(wsum[l0:l1]), C.byref(ne)), ValueError)
            n_exact += ne.value
        return logsum, wsum, n_exact

    # ---- histogram surfaces along a scan (pymbar_amd.scan.compute_scan_fes) ---------------------------------------------------
    SCAN_BIN_CROSS_BYTES = 1 << 28  # the host cross block of one slab of members of scan_bin_gram_w stays under this

    def set_scan_bins(self, nbins, label_n=None):
        """Histogram bins as labels of the resident samples for the binned scan passes: ``label_n`` in ``[-1, nbins)`` (-1: in no
        bin), sorted by bin on the host and uploaded once (``mbar_ctx_set_scan_bins``).  ``nbins=0`` releases them."""
        if int(nbins) == 0:
            self._check(self._lib.mbar_ctx_set_scan_bins(self._ctx, 0, None))
            self._scan_nbins = 0
            return
        label_n = _lib.labels_i32(label_n, nbins, self.N_local, "label_n")
        # (MBAR_ERR_ARG: a label outside [-1, nbins).  A refused call leaves the library's bins as they were, so the count that
        # sizes the output of the binned passes changes only with them.)
        self._check(self._lib.mbar_ctx_set_scan_bins(self._ctx, int(nbins), _dptr(label_n, _lib._i32p)), ValueError)
        self._scan_nbins = int(nbins)

    def scan_bin_lognum(self, f, coeff_lb, offset_l=None, center_lb=None):
        """Pass A of a binned scan: ``lognum[l, i] = log sum_{n in bin i} c_n exp(-u_l(n) - logden_n(f))`` (``L x nbins``; ``-inf``
        where no sample of the bin has ``c_n > 0``)."""
        f = self._f(f)
        coeff_lb, offset_l, L, _ = self._scan_members(coeff_lb, offset_l)
        self._scan_centers(center_lb, L)
        lognum = np.empty((L, self._scan_nbins), dtype=np.float64)
        self._check(self._lib.mbar_scan_bin_lognum(self._ctx, _dptr(f), L, _dptr(coeff_lb), _dptr(offset_l), _dptr(lognum)))
        return lognum

    def scan_bin_gram_w(self, f, coeff_lb, offset_l, f_bins, cross=True, slab=None, center_lb=None):
        """Pass B of a binned scan: ``(cross, diag, wsum)`` of the normalised weights ``Bv = exp(f_bins[l, i] - u_l(n) -
        logden_n(f))`` of member ``l`` on the samples of bin ``i`` -- ``cross[k, l, i] = sum_{n in i} c_n W_nk Bv`` (``None`` with
        ``cross=False``), ``diag[l, i] = sum c_n Bv^2``, ``wsum[l, i] = sum c_n Bv``.  The members go to the device in slabs (of
        ``slab`` members; by default as many as keep a slab's ``cross`` block under 256 MiB): a (member, bin)'s bits do not depend
        on the cut."""
        f = self._f(f)
        coeff_lb, offset_l, L, _ = self._scan_members(coeff_lb, offset_l)
        nbins = self._scan_nbins
        f_bins = _lib.f64(f_bins, (L, nbins), "f_bins")
        if slab is None:
            slab = self.SCAN_BIN_CROSS_BYTES // (8 * self.K * max(nbins, 1)) if cross else L
        slab = max(1, min(int(slab), L))
        X = np.empty((self.K, L, nbins), dtype=np.float64) if cross else None
        d = np.empty((L, nbins), dtype=np.float64)
        w = np.empty((L, nbins), dtype=np.float64)
        for l0 in range(0, L, slab):
            l1 = min(L, l0 + slab)
            Xs = np.empty((self.K, l1 - l0, nbins), dtype=np.float64) if cross and (l0, l1) != (0, L) else X
            self._scan_centers(None if center_lb is None else center_lb[l0:l1], l1 - l0)
            self._check(self._lib.mbar_scan_bin_gram_w(self._ctx, _dptr(f), l1 - l0, _dptr(coeff_lb[l0:l1]), _dptr(offset_l[l0:l1]),
                                                       _dptr(f_bins[l0:l1]), _dptr(Xs), _dptr(d[l0:l1]), _dptr(w[l0:l1])))
            if cross and Xs is not X:
                X[:, l0:l1, :] = Xs
        return X, d, w

    def set_option(self, key, value):
        self._check(self._lib.mbar_ctx_set_option(self._ctx, key.encode(), int(value)))

    def synchronize(self):
        self._check(self._lib.mbar_ctx_synchronize(self._ctx))

    def to_host(self):
        from .utils import prefault

        out = prefault(np.empty((self.K, self.N_local), dtype=np.float64))
        self._check(self._lib.mbar_ctx_download_u(self._ctx, _dptr(out), self.N_local))
        return out

    def set_Nk(self, N_k):
        """GLOBAL sample counts (any numeric dtype; zeros allowed)."""
        Nk = _lib.f64(N_k, (self.K,), "N_k")
        if self._Nk is None or not np.array_equal(Nk, self._Nk):
            self._touched()
            self._check(self._lib.mbar_ctx_set_Nk(self._ctx, _dptr(Nk)))
            self._Nk = Nk.copy()

    def set_sample_weights(self, c_n):
        """Per-sample multiplicities (``None`` restores 1): every sum over samples becomes ``sum_n c_n (...)``.
        A bootstrap replicate is ``np.bincount(resampled_indices, minlength=N)``."""
        c_n = _lib.f64(c_n, (self.N_local,), "sample weights", optional=True)
        self._wtag = None if c_n is None else object()
        self._check(self._lib.mbar_ctx_set_sample_weights(self._ctx, _dptr(c_n)))

    def draw_bootstrap_weights(self, seed, replicate, cumN, order=None, n_global0=0, layout_key=None):
        """Per-sample multiplicities = draw counts of bootstrap replicate ``replicate`` of the counter-based stream ``seed``, drawn
        ON THE DEVICE (``mbar_ctx_draw_bootstrap_weights``; :func:`pymbar_amd._lib.bootstrap_draws` gives the same draws on the
        host).  ``cumN`` (K + 1): positions of the states' runs; ``order``: sample index of a position (``None``: the default layout).
        ``layout_key``: any object that identifies (cumN, order) for the caller -- the layout is uploaded when the key changes
        (``mbar_ctx_set_bootstrap_layout``) and replicates with the same key touch no host array of N integers; without a key the
        arrays travel with every call and the library digests them to see whether its device copy still matches."""
        layout = (None, 0, None)  # a known key: the layout on the device
        if layout_key is None or layout_key is not self._boot_layout_key:
            cumN = np.ascontiguousarray(cumN, dtype=np.int64)
            if cumN.ndim != 1 or len(cumN) < 2:
                raise ValueError("cumN must hold the K + 1 run boundaries of K >= 1 states")
            order = None if order is None else np.ascontiguousarray(order, dtype=np.int64)
            if order is not None and order.shape != (max(int(cumN[-1]), 0),):
                raise ValueError("order must have one entry per position: cumN[-1] of them")
            arrays = (_dptr(cumN, _lib._ip), len(cumN) - 1, _dptr(order, _lib._ip))
            if layout_key is None:  # the arrays travel with the draw
                layout = arrays
            else:  # a new key: uploaded now, the draw finds it there
                self._check(self._lib.mbar_ctx_set_bootstrap_layout(self._ctx, *arrays))
            self._boot_layout_key = layout_key
        self._wtag = object()
        self._check(self._lib.mbar_ctx_draw_bootstrap_weights(self._ctx, C.c_uint64(int(seed)), int(replicate), *layout, int(n_global0)))

    def weights_from_vec(self, power):
        """Per-sample weights ``(A_n - shift)**power`` from the observable ``vec_logshift`` left on the device (no upload, no host
        pass): the weighted sums of a single observable at the resident states.  ``set_sample_weights(None)`` restores 1."""
        self._wtag = object()
        self._check(self._lib.mbar_ctx_weights_from_vec(self._ctx, float(power)))

    # ---- multi-GPU --------------------------------------------------------------------------------
    def comm_init_rccl(self, unique_id, rank, nranks):
        self._touched()
        buf = C.create_string_buffer(bytes(unique_id), 128)
        self._check(self._lib.mbar_ctx_comm_init(self._ctx, buf, rank, nranks))
        self.rank, self.nranks, self.allreduce_kind = rank, nranks, "rccl"

    def set_host_allreduce(self, fn, rank, nranks):
        """``fn(array, op)`` must all-reduce the float64 numpy ``array`` in place (op 'sum'|'max')."""
        self._touched()

        def _cb(ptr, count, op, _user):
            try:
                arr = np.ctypeslib.as_array(ptr, shape=(count,))
                fn(arr, "sum" if op == 0 else "max")
                return 0
            except Exception:  # pragma: no cover
                return 1

        self._cb = _lib.ALLREDUCE_FN(_cb)
        self._check(self._lib.mbar_ctx_set_host_allreduce(self._ctx, self._cb, None, rank, nranks))
        self.rank, self.nranks, self.allreduce_kind = rank, nranks, "host"

    def set_loopback(self, group, rank):
        """Join the in-process transport ``group`` (:class:`LoopbackGroup`) as ``rank``: collectives run on the compute stream
        like RCCL's, between contexts of this process on one device (one caller thread per context)."""
        self._touched()
        self._check(self._lib.mbar_ctx_set_loopback(self._ctx, group._h, int(rank)))
        self._loop = group  # (keeps the group alive)
        self.rank, self.nranks, self.allreduce_kind = int(rank), group.nranks, "loopback"

    def comm_destroy(self):
        """Detach the cross-rank transport (destroys an RCCL communicator); the matrix is single-rank again."""
        self._touched()
        self._check(self._lib.mbar_ctx_comm_destroy(self._ctx))
        self._cb = None
        self.rank, self.nranks, self.allreduce_kind = 0, 1, "none"

    def device_synchronize(self):
        """``hipDeviceSynchronize`` on this matrix's GPU (all streams)."""
        _lib.check(self._lib.mbar_device_synchronize(self.device))

    # ---- L1 ---------------------------------------------------------------------------------------
    def eval(self, f, gram=False, use_offset=False):
        """One fused sweep for 1 or 2 free-energy vectors.  Returns ``(psum, sumlogden, gram)`` with
        ``psum[i, k] = sum_n N_k W_nk(f_i)``, ``sumlogden[i] = sum_n logden_n(f_i)`` and, if asked,
        ``gram = sum_n p p^T`` at ``f[0]`` (all summed over ranks)."""
        f = np.ascontiguousarray(np.atleast_2d(np.asarray(f, dtype=np.float64)))
        nf = f.shape[0]
        if f.ndim != 2 or f.shape[1] != self.K or nf not in (1, 2):
            raise ValueError("f must be (K,) or (1|2, K)")
        psum = np.empty((nf, self.K), dtype=np.float64)
        sld = np.empty(nf, dtype=np.float64)
        G = np.empty((self.K, self.K), dtype=np.float64) if gram else None
        flags = (_lib.EVAL_GRAM if gram else 0) | (_lib.EVAL_USE_OFFSET if use_offset else 0)
        self._check(self._lib.mbar_eval(self._ctx, _dptr(f), nf, flags, _dptr(psum), _dptr(sld),
                                        _dptr(G) if gram else None))
        return psum, sld, G

    def set_objective_offset(self, f0):
        f0 = _lib.f64(f0, (self.K,), "f0", optional=True)
        self._check(self._lib.mbar_ctx_set_objective_offset(self._ctx, _dptr(f0)))

    def lognum(self, f):
        f = self._f(f)
        out = np.empty(self.K, dtype=np.float64)
        self._check(self._lib.mbar_lognum(self._ctx, _dptr(f), _dptr(out)))
        return out

    def lognum_cached(self, f):
        """``lognum(f)``, kept while neither the matrix, N_k, the multiplicities nor ``f`` change (consecutive methods of the
        class at the same ``f_k``: one sweep of the resident rows instead of one per call)."""
        f = self._f(f)
        if self._wtag is not None:
            return self.lognum(f)
        key = (self._version, f.tobytes())
        if self._lognum_cache is None or self._lognum_cache[0] != key:
            self._lognum_cache = (key, self.lognum(f))
        return self._lognum_cache[1].copy()

    def gram_w_cached(self, f):
        """``gram_w(f)`` with unit multiplicities, kept like ``lognum_cached`` (the covariance of the free energies, overlap and
        every expectation at the same ``f_k`` start from the same ``W^T W`` of the resident states)."""
        f = self._f(f)
        if self._wtag is not None:
            return self.gram_w(f)
        key = (self._version, f.tobytes())
        if self._gram_w_cache is None or self._gram_w_cache[0] != key:
            self._gram_w_cache = (key, self.gram_w(f))
        G, ws = self._gram_w_cache[1]
        return G.copy(), ws.copy()

    def extend(self, nrows):
        """An :class:`ExtendedMatrix` of ``K + nrows`` rows whose first K rows ARE this matrix (no copy) -- or ``None`` when the
        library cannot sweep the two as one panel (more than 128 states here, fewer than 129 or more than 256 rows in total,
        several ranks): the caller then assembles an augmented copy."""
        if self.nranks != 1:
            return None
        ctx = C.c_void_p()
        rc = self._lib.mbar_ctx_create_ext(C.byref(ctx), self._ctx, int(nrows))
        if rc != _lib.MBAR_OK:
            return None
        return ExtendedMatrix(self, ctx, int(nrows))

    def logden(self, f):
        f = self._f(f)
        out = np.empty(self.N_local, dtype=np.float64)
        self._check(self._lib.mbar_logden(self._ctx, _dptr(f), _dptr(out)))
        return out

    def logw_kn(self, f):
        """``log W`` of this shard as a C-ordered (K, N_local) array; its ``.T`` is the reference's
        F-ordered (N, K) ``Log_W_nk``."""
        f = self._f(f)
        from .utils import prefault

        out = prefault(np.empty((self.K, self.N_local), dtype=np.float64))  # (pages touched by several threads first)
        self._check(self._lib.mbar_logw(self._ctx, _dptr(f), _dptr(out), self.N_local))
        return out

    def w_kn(self, f):
        """The weights ``W`` of this shard as a C-ordered (K, N_local) array (``exp`` taken on the device); its ``.T`` is the
        reference's (N, K) ``W_nk``."""
        from .utils import prefault

        f = self._f(f)
        out = prefault(np.empty((self.K, self.N_local), dtype=np.float64))
        self._check(self._lib.mbar_w(self._ctx, _dptr(f), _dptr(out), self.N_local))
        return out

    def gram_w(self, f):
        """``(W^T W, sum_n W_nk)`` over all states (MFMA), summed over ranks."""
        f = self._f(f)
        G = np.empty((self.K, self.K), dtype=np.float64)
        ws = np.empty(self.K, dtype=np.float64)
        self._check(self._lib.mbar_gram_w(self._ctx, _dptr(f), _dptr(G), _dptr(ws)))
        return G, ws

    # ---- solver loops -----------------------------------------------------------------------------
    def solve_adaptive(self, f, tol=1e-12, maxiter=10000, min_sc_iter=2, gamma=1.0, check_convergence=True,
                       history_rows=0):
        f = self._f(f).copy()  # (the library writes the solution over the start)
        res = _lib.SolveResult()
        hist = np.zeros((max(1, history_rows), 4), dtype=np.float64)
        self._check(self._lib.mbar_solve_adaptive(self._ctx, _dptr(f), tol, int(maxiter), int(min_sc_iter),
                                                  float(gamma), 1 if check_convergence else 0, _dptr(hist),
                                                  int(history_rows), C.byref(res)))
        out = _solve_result(res)
        out["history"] = hist[: min(history_rows, res.iterations)]
        # per-state sums at the returned f (the solver has them anyway): gradient norm and all-state update without another sweep
        psum = np.empty(self.K, dtype=np.float64)
        out["psum"] = psum if self._lib.mbar_ctx_last_solve_psum(self._ctx, _dptr(psum)) == _lib.MBAR_OK else None
        return f, out

    def solve_sci(self, f, tol=1e-12, maxiter=10000, check_convergence=True):
        f = self._f(f).copy()  # (the library writes the solution over the start)
        res = _lib.SolveResult()
        self._check(self._lib.mbar_solve_sci(self._ctx, _dptr(f), tol, int(maxiter),
                                             1 if check_convergence else 0, C.byref(res)))
        return f, _solve_result(res)

    # ---- measurement ------------------------------------------------------------------------------
    def timing(self):
        """{class: (total_ms, launches)} of HIP-event timed kernels since the last reset."""
        out = {}
        for name, which in (("lse", _lib.TIMER_LSE), ("gram", _lib.TIMER_GRAM), ("reduce", _lib.TIMER_REDUCE),
                            ("other", _lib.TIMER_OTHER), ("fused", _lib.TIMER_FUSED), ("newton", _lib.TIMER_NEWTON),
                            ("comm", _lib.TIMER_COMM)):
            ms = C.c_double(0.0)
            n = C.c_int64(0)
            self._check(self._lib.mbar_ctx_timing(self._ctx, which, C.byref(ms), C.byref(n)))
            out[name] = (ms.value, n.value)
        return out

    def timing_reset(self):
        self._check(self._lib.mbar_ctx_timing_reset(self._ctx))

    def mfma_f64_peak(self):
        t = C.c_double(0.0)
        self._check(self._lib.mbar_mfma_f64_peak(self._ctx, C.byref(t)))
        return t.value


class ExtendedMatrix(_ContextMatrix):
    """``[rows of a resident DeviceMatrix | rows appended to it]`` without a copy of the resident rows: the appended rows live in
    an extension context of the library (``mbar_ctx_create_ext``) and the sweeps read both matrices (``mbar_lognum_ext``,
    ``mbar_gram_w_ext``).  Row indices are those of the augmented matrix of pymbar/mbar.py:886-903 -- ``[0, K)`` the resident
    states, ``[K, K + R)`` the appended ones (N_k = 0) -- and the methods are the subset of :class:`DeviceMatrix` that the
    expectation family drives; rows below K are read-only."""

    def __init__(self, base, ctx, nrows):
        self.base = base
        self._lib = base._lib
        self._ctx = ctx
        self.Kb = base.K
        self.K = base.K + nrows
        self.N_local = base.N_local
        self.nranks = 1

    def _ext_row(self, row, n=1):
        if row < self.Kb or row + n > self.K:
            raise ValueError("only the appended rows can be written")
        return int(row - self.Kb)

    _dst_row = _ext_row

    def _src(self, row0, n):
        """(context, row) of a source run: the resident matrix below K, the extension from K on (a run does not straddle)."""
        if row0 + n <= self.Kb:
            return self.base._ctx, int(row0)
        if row0 >= self.Kb:
            return self._ctx, int(row0 - self.Kb)
        raise ValueError("a source run straddles the resident and the appended rows")

    def copy_rows_from(self, src, dst_row0=0, src_row0=0, nrows=None):
        nrows = src.K - src_row0 if nrows is None else nrows
        if src is self.base and dst_row0 == 0 and src_row0 == 0 and nrows == self.Kb:
            return  # (the resident rows ARE the first K rows)
        super().copy_rows_from(src, dst_row0, src_row0, nrows)

    def rows_obs_from_base(self, dst_row0, state_row0, obs_row0, nrows):
        """Appended rows ``dst`` = resident rows ``state`` - log(resident rows ``obs`` - shift); ``shift`` per row is returned."""
        shift = np.empty(int(nrows), dtype=np.float64)
        # (the minima of resident rows are a property of the resident matrix: kept on it, keyed by its version and the row run)
        key = (self.base._version, int(obs_row0), int(nrows))
        cache = self.base._rowmin_cache
        mins = cache[1] if cache is not None and cache[0] == key else None
        out = np.empty(int(nrows), dtype=np.float64) if mins is None else None
        self._check(self._lib.mbar_ctx_rows_obs_from(self._ctx, self._ext_row(dst_row0, nrows), self.base._ctx, int(state_row0),
                                                     int(obs_row0), int(nrows), _dptr(shift), None if mins is None else _dptr(mins),
                                                     None if out is None else _dptr(out)))
        if mins is None:
            self.base._rowmin_cache = (key, out)
        return shift

    def set_Nk(self, N_k):
        N_k = np.asarray(N_k, dtype=np.float64)
        if (N_k.shape != (self.K,) or np.any(N_k[self.Kb:] != 0) or self.base._Nk is None
                or not np.array_equal(N_k[:self.Kb], self.base._Nk)):
            raise ValueError("the appended rows are unsampled states of the resident matrix's mixture")

    def lognum(self, f):
        f = self._f(f)
        fb = f[:self.Kb]  # (a run of a contiguous vector is contiguous)
        out = np.empty(self.K, dtype=np.float64)
        out[:self.Kb] = self.base.lognum_cached(fb)
        self._check(self._lib.mbar_lognum_ext(self._ctx, self.base._ctx, _dptr(fb), _dptr(out[self.Kb:])))
        return out

    def gram_w(self, f):
        f = self._f(f)
        fb, fe = f[:self.Kb], f[self.Kb:]
        G = np.empty((self.K, self.K), dtype=np.float64)
        ws = np.empty(self.K, dtype=np.float64)
        # (a few appended rows: only their entries are swept for, the resident states' own W^T W is the one the class keeps)
        Gb = self.base.gram_w_cached(fb)[0] if self.K - self.Kb <= 16 else None  # (a copy: C-contiguous)
        self._check(self._lib.mbar_gram_w_ext(self._ctx, self.base._ctx, _dptr(fb), _dptr(fe), _dptr(Gb), _dptr(G), _dptr(ws)))
        return G, ws


class LoopbackGroup:
    """``mbar_loopback``: stream-ordered all-reduce between the contexts of several threads of this process on one GPU."""

    def __init__(self, nranks):
        self._lib = _lib.load_library()
        self.nranks = int(nranks)
        self._h = C.c_void_p()
        _lib.check(self._lib.mbar_loopback_create(C.byref(self._h), self.nranks))

    def close(self):
        if self._h:
            self._lib.mbar_loopback_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def device_info(device=0):
    lib = _lib.load_library()
    name = C.create_string_buffer(256)
    cu = C.c_int(0)
    mem = C.c_int64(0)
    rc = lib.mbar_device_info(device, name, 256, C.byref(cu), C.byref(mem))
    if rc != _lib.MBAR_OK:
        raise _lib.BackendUnavailable(_lib.last_error(None))
    return dict(name=name.value.decode(), compute_units=cu.value, total_mem_bytes=mem.value)
