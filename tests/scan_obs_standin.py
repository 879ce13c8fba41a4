"""CPU stand-in for the observable pass of ``pymbar_amd.device.DeviceMatrix`` (``set_scan_observables`` / ``scan_obs_sums``, the sums
behind ``MBAR.compute_scan_expectations``) -- TEST INFRASTRUCTURE ONLY: :class:`tests.scan_standin.ScanOracleMatrix` plus the two
methods in numpy long double, and the same on the stand-in of the families with harmonic terms
(:class:`tests.family_standin.FamilyOracleMatrix`).  ``scan_obs_abs_sums`` returns ``sum c b^P |a|`` (P = 1, 2), what the signed sums
are held against.

Also the builder of the cases the pass is tested at and the matrix of cases that reaches every instantiation of the kernel
(``obs_cases``): tests/test_gpu_scan_obs.py runs them on the device."""
import numpy as np

from tests.family_standin import FamilyOracleMatrix, build_family_case, harmonic_mb
from tests.scan_standin import ScanOracleMatrix, build_case, scan_mb, scan_nb_for


class _ObsSums:
    _obs = None

    def set_scan_observables(self, a_qn=None):
        if a_qn is None:
            self._obs = None
            return
        N = self.N_local if self._counts is None else len(self._counts)
        a_qn = np.array(a_qn, dtype=np.float64)
        if a_qn.ndim != 2 or a_qn.shape[1] != N or a_qn.shape[0] < 1:
            raise ValueError("a_qn must have shape (Q, N_local) with Q >= 1")
        if not np.all(np.isfinite(a_qn)):
            raise ValueError("the observables must be finite")
        self._obs = a_qn

    def _weights(self, f, coeff_lb, offset_l, f_scan):
        """``(b[l, n], a[q, n])`` over the (resampled) samples, in the stand-in's number format"""
        if self._scan is None:
            raise ValueError("no basis on this matrix (set_scan first)")
        if self._obs is None:
            raise ValueError("no observables on this matrix (set_scan_observables first)")
        L = np.shape(coeff_lb)[0]
        if np.shape(f_scan) != (L,) or (offset_l is not None and np.shape(offset_l) != (L,)):
            raise ValueError("offset_l and f_scan must have one entry per member")
        x, _, _ = self._members(f, coeff_lb, offset_l)
        a = self._obs if self._counts is None else np.repeat(self._obs, self._counts, axis=1)
        return np.exp(np.asarray(f_scan, dtype=self.real)[:, None] + x), a.astype(self.real)

    def _obs_sums(self, f, coeff_lb, offset_l, f_scan, second=True):
        b, a = self._weights(f, coeff_lb, offset_l, f_scan)
        out = lambda v: np.asarray(v, dtype=np.float64)
        if not second:
            return out(b @ a.T), None, None, out(b.sum(axis=1)), None
        b2 = b * b
        return out(b @ a.T), out(b2 @ a.T), out(b2 @ (a * a).T), out(b.sum(axis=1)), out(b2.sum(axis=1))

    def _obs_abs_sums(self, f, coeff_lb, offset_l, f_scan):
        b, a = self._weights(f, coeff_lb, offset_l, f_scan)
        return np.asarray(b @ np.abs(a).T, dtype=np.float64), np.asarray((b * b) @ np.abs(a).T, dtype=np.float64)


class ScanObsOracleMatrix(_ObsSums, ScanOracleMatrix):
    def scan_obs_sums(self, f, coeff_lb, offset_l, f_scan, second=True, center_lb=None, slab=None):
        return self._obs_sums(f, coeff_lb, offset_l, f_scan, second)

    def scan_obs_abs_sums(self, f, coeff_lb, offset_l, f_scan, center_lb=None):
        return self._obs_abs_sums(f, coeff_lb, offset_l, f_scan)


class ScanObsFloat64Matrix(ScanObsOracleMatrix):
    """The same formulas in plain float64: what separates it from the long-double stand-in bounds the stand-in's own error"""
    real = np.float64


class FamilyObsOracleMatrix(_ObsSums, FamilyOracleMatrix):
    def scan_obs_sums(self, f, coeff_lb, offset_l, f_scan, second=True, center_lb=None, slab=None):
        return self._call(center_lb, self._obs_sums, f, coeff_lb, offset_l, f_scan, second)

    def scan_obs_abs_sums(self, f, coeff_lb, offset_l, f_scan, center_lb=None):
        return self._call(center_lb, self._obs_abs_sums, f, coeff_lb, offset_l, f_scan)


# ---- the cases --------------------------------------------------------------------------------------------------------------------
OBS_PANEL = 128  # observables of one panel of the kernel (mbar_scan_obs_sums)


def obs_panels(Q):
    """``[(nb, rows)]`` of the observable panels a block of Q stored rows is cut into"""
    return [(scan_nb_for(min(OBS_PANEL, Q - q0)), min(OBS_PANEL, Q - q0)) for q0 in range(0, Q, OBS_PANEL)]


def obs_rows(y, Q):
    """Q observables of a coordinate ``y`` of unit scale, kinds in turn: sign-changing, positive, an indicator, a constant row, an
    oscillation whose frequency grows with the row, a small fluctuation on a large offset"""
    kinds = (lambda q: y, lambda q: y * y, lambda q: (y > 0.3).astype(np.float64), lambda q: np.full_like(y, 2.5),
             lambda q: np.cos((1.0 + 0.37 * q) * y), lambda q: 1000.0 + y)
    return np.stack([kinds[q % len(kinds)](q) for q in range(Q)])


def build_obs_case(spec):
    """``spec = (family, K, N, L, B, H, Q, hard)``: the case of tests/scan_standin.py (family "linear", H = 0) or of
    tests/family_standin.py ("harmonic") without stored observables of the scan's own, and Q observables to keep resident, made of
    the first basis vector brought to unit scale."""
    fam, K, N, L, B, H, Q, hard = spec
    if fam == "linear":
        case = build_case((K, N, L, B, 0), hard)
        case.update(center=None, harmonic_b=None, period_b=None)
    else:
        case = build_family_case((K, N, L, B, H, 0), hard)
    y = case["basis"][0]
    y = (y - y.mean()) / (y.std() if y.std() > 0.0 else 1.0)
    case["a"] = obs_rows(y, Q)
    case["family"] = fam
    return case


def load_obs_case(dm, case):
    dm.set_Nk(case["N_k"])
    dm.set_sample_weights(case["c"])
    if case["family"] == "linear":
        dm.set_scan(case["basis"], None)
    else:
        dm.set_scan(case["basis"], None, harmonic_b=case["harmonic_b"], period_b=case["period_b"])
    dm.set_scan_observables(case["a"])


def obs_oracle_for(case, u, cls=None):
    """The long-double stand-in (or ``cls`` of the same kind) loaded with the case on the matrix ``u``"""
    if cls is None:
        cls = ScanObsOracleMatrix if case["family"] == "linear" else FamilyObsOracleMatrix
    m = cls(u)
    load_obs_case(m, case)
    return m


def cen_of(case, members=slice(None)):
    return {} if case["center"] is None else dict(center_lb=case["center"][members])


def run_obs(dm, case, f_scan=None, members=slice(None), **kw):
    """``(f_scan, (s1, t1, t2, wsum, w2sum))`` of the case's members (or of ``members`` of them)"""
    coeff, offset = case["coeff"][members], case["offset"][members]
    cen = cen_of(case, members)
    if f_scan is None:
        f_scan = -dm.scan_lognum(case["f"], coeff, offset, **cen)[0]
    return f_scan, dm.scan_obs_sums(case["f"], coeff, offset, f_scan, **cen, **kw)


def obs_L(fam):
    """One full member panel of the widest launch (one operand column per member) plus 17: under two operand columns that is two
    full panels and a third of two blocks whose second block holds one member"""
    return 64 * (scan_mb(1) if fam == "linear" else harmonic_mb(1)) + 17


def obs_case_id(spec):
    fam, K, N, L, B, H, Q, hard = spec
    panels = "+".join("NB%dx%d" % p for p in obs_panels(Q))
    return "%s-%s-K%d-N%d-L%d-B%d-H%d-Q%d%s" % (fam, panels, K, N, L, B, H, Q, "-hard" if hard else "")


OBS_Q = (1, 16, 17, 32, 33, 64, 65, 100, 128, 129)


def obs_cases():
    """The matrix of the observable kernel.  Linear family: both ends of every NB (Q = 100: block 6 partial, block 7 all padding) and
    a second observable panel that holds one row (Q = 129), at K = 9 and K = 128 (the kernel reads the matrix only through logden),
    N = 77 (four full tiles of 16 samples and a tail of 13), L = one full member panel plus 17, B cycling over 1, 2, 5, 8.  The
    harmonic family (B = 3, two harmonic terms of which one is periodic) at three of the widths.  Then the edges of the sample axis at
    Q = 17 -- the tile edge (1, 15, 16, 17) and the chunk edge (8192, 8193) -- and the hard variant of the cases (multiplicities 0 ..
    3, +inf entries, a state without samples; the member 900 below the rest is in every case) in both families."""
    cases = []
    for i, Q in enumerate(OBS_Q):
        for j, K in enumerate((9, 128)):
            cases.append(("linear", K, 77, obs_L("linear"), (1, 2, 5, 8)[(i + j) % 4], 0, Q, False))
    cases += [("harmonic", 9, 77, obs_L("harmonic"), 3, 2, Q, False) for Q in (17, 100, 129)]
    cases += [("linear", 9, N, 20, 5, 0, 17, False) for N in (1, 15, 16, 17)]
    cases += [("linear", 9, 8192, 70, 2, 0, 17, False), ("linear", 9, 8193, 70, 8, 0, 17, True)]
    cases += [("linear", 9, 211, 37, 5, 0, 33, True), ("linear", 128, 300, 141, 2, 0, 129, True), ("harmonic", 9, 211, 37, 3, 2, 65, True)]
    return cases
