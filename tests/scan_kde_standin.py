"""CPU stand-in for the density pass of ``pymbar_amd.device.DeviceMatrix`` (``set_scan_points`` / ``scan_kde_sums``, the sums behind
``MBAR.compute_scan_kde``) -- TEST INFRASTRUCTURE ONLY: :class:`tests.scan_standin.ScanOracleMatrix` plus the two methods in numpy
long double, and the same on the stand-in of the families with harmonic terms (:class:`tests.family_standin.FamilyOracleMatrix`).
Everything is formed in log space, so a pair whose terms are all below the fp64 range has its finite answer; ``n_exact`` is what the
2^-900 rule of the device predicts from the plain sums.

Also :func:`log_density_oracle`, the long-double log density of a member from its log weights (the minimum image restated here), the
builder of the cases the pass is tested at and the matrix of cases that reaches every instantiation of the kernel (``kde_cases``):
tests/test_gpu_scan_kde.py runs them on the device."""
import numpy as np

from tests.family_standin import FamilyOracleMatrix
from tests.kde_oracle import LD, log_normaliser_ld
from tests.scan_obs_standin import build_obs_case
from tests.scan_standin import ScanOracleMatrix, scan_nb_for

FLAG_BELOW = LD(2.0) ** -900  # the merged sums not at or above this take the device's exact path
KDE_PANEL = 128              # queries of one panel of the kernel (mbar_scan_kde_sums)


def log_kernel_wrapped(x_dn, q_dm, h, period=None, real=LD):
    """``(M, N)`` ``-r^2 / 2h^2`` with the minimum image ``dl - P rint(dl / P)`` where ``period[k] > 0``: from the float64 coordinates,
    every step in ``real``"""
    x_dn, q_dm = np.asarray(x_dn, dtype=np.float64), np.asarray(q_dm, dtype=np.float64)
    r2 = np.zeros((q_dm.shape[1], x_dn.shape[1]), dtype=real)
    with np.errstate(over="ignore"):
        for k in range(x_dn.shape[0]):
            dl = q_dm[k][:, None].astype(real) - x_dn[k][None, :].astype(real)
            P = 0.0 if period is None else float(period[k])
            if P > 0.0:
                dl = dl - real(P) * np.rint(dl / real(P))
            r2 = r2 + dl * dl
        hl = real(h)
        return -r2 / (2 * hl * hl)


def logsumexp_rows(t):
    """``log sum_n exp(t[m, n])`` per row, about the row's own maximum; -inf for a row without a finite term"""
    tm = t.max(axis=1)
    fin = np.isfinite(tm)
    out = np.full(t.shape[0], -np.inf, dtype=t.dtype)
    out[fin] = tm[fin] + np.log(np.sum(np.exp(t[fin] - tm[fin, None]), axis=1))
    return out


def log_density_oracle(x_dn, logw_n, q_dm, h, period=None, real=LD):
    """``(log density (M,), log of the plain sum (M,), log of the total weight)`` of ONE member with log weights ``logw_n`` (-inf:
    a sample without weight) in ``real``: what ``tests.kde_oracle.log_density_ld`` computes from the weights themselves, for weights
    that need not be inside the fp64 range, and with the minimum image."""
    logw_n = np.asarray(logw_n, dtype=real)
    pos = np.isfinite(logw_n)
    lk = log_kernel_wrapped(np.asarray(x_dn)[:, pos], q_dm, h, period, real)
    logsum = logsumexp_rows(lk + logw_n[pos][None, :])
    logtot = logsumexp_rows(logw_n[pos][None, :])[0]
    return logsum - logtot + log_normaliser_ld("gaussian", np.shape(x_dn)[0], h).astype(real), logsum, logtot


class _KdeSums:
    _pts = None

    def set_scan_points(self, x_dn=None):
        if x_dn is None:
            self._pts = None
            return
        N = self.N_local if self._counts is None else len(self._counts)
        x_dn = np.array(x_dn, dtype=np.float64)
        if x_dn.ndim != 2 or x_dn.shape[1] != N or not 1 <= x_dn.shape[0] <= 2:
            raise ValueError("x_dn must have shape (d, N_local) with d = 1 or 2")
        if not np.all(np.isfinite(x_dn)):
            raise ValueError("the points must be finite")
        self._pts = x_dn

    def _kde_sums(self, f, coeff_lb, offset_l, f_scan, queries_dm, bandwidth, period):
        if self._scan is None:
            raise ValueError("no basis on this matrix (set_scan first)")
        if self._pts is None:
            raise ValueError("no points on this matrix (set_scan_points first)")
        L = np.shape(coeff_lb)[0]
        queries_dm = np.asarray(queries_dm, dtype=np.float64)
        d = self._pts.shape[0]
        if np.shape(f_scan) != (L,) or (offset_l is not None and np.shape(offset_l) != (L,)):
            raise ValueError("offset_l and f_scan must have one entry per member")
        if queries_dm.ndim != 2 or queries_dm.shape[0] != d or queries_dm.shape[1] < 1:
            raise ValueError("queries_dm must have shape (d, M) with M >= 1")
        if period is not None and np.shape(period) != (d,):
            raise ValueError("period must have one entry per coordinate")
        if not (bandwidth > 0.0 and np.isfinite(bandwidth)) or not np.all(np.isfinite(queries_dm)):
            raise ValueError("mbar_scan_kde_sums: the bandwidth must be positive and finite, the queries finite")
        M = queries_dm.shape[1]
        if np.any(np.isnan(f)) or np.any(np.isnan(f_scan)):
            return np.full((L, M), np.nan), np.full(L, np.nan), 0
        R = self.real
        x, _, _ = self._members(f, coeff_lb, offset_l)
        pts = self._pts if self._counts is None else np.repeat(self._pts, self._counts, axis=1)
        lk = log_kernel_wrapped(pts, queries_dm, bandwidth, period, R)
        logsum = np.empty((L, M), dtype=R)
        wsum = np.empty(L, dtype=R)
        for l in range(L):
            logb = np.asarray(f_scan, dtype=R)[l] + x[l]
            logsum[l] = logsumexp_rows(lk + logb[None, :])
            wsum[l] = np.sum(np.exp(logb))
        with np.errstate(over="ignore"):
            flagged = ~(np.exp(logsum) >= FLAG_BELOW) & (wsum > 0)[:, None]
            return logsum.astype(np.float64), wsum.astype(np.float64), int(np.sum(flagged))


class ScanKdeOracleMatrix(_KdeSums, ScanOracleMatrix):
    def scan_kde_sums(self, f, coeff_lb, offset_l, f_scan, queries_dm, bandwidth, period=None, center_lb=None, slab=None):
        return self._kde_sums(f, coeff_lb, offset_l, f_scan, queries_dm, bandwidth, period)


class ScanKdeFloat64Matrix(ScanKdeOracleMatrix):
    """The same formulas in plain float64: the numpy restatement the device is held against"""
    real = np.float64


class _OrderedKdeSums(_KdeSums):
    """Plain float64 in the ORDER the device is specified to sum in (include/mbar_hip.h): the multiplicities as factors c_n, chunks of
    8192 samples cut by N alone, inside a chunk one chain of additions over the positions in ascending order (``np.cumsum``), the
    chunks added in chunk order.  numpy's own ``sum`` is pairwise and loses ~log2(N) roundings where a chain of 8192 loses up to 8192
    of them, whatever the hardware: this restatement, not the pairwise one, is what tells a fault of the kernel from the price of the
    order contract."""
    real = np.float64
    CHUNK = 8192

    def _kde_sums(self, f, coeff_lb, offset_l, f_scan, queries_dm, bandwidth, period):
        if self._scan is None or self._pts is None:
            raise ValueError("no basis or no points on this matrix")
        L, M = np.shape(coeff_lb)[0], np.shape(queries_dm)[1]
        x, _, _ = self._members(f, coeff_lb, offset_l)
        counts = self._counts
        if counts is not None:  # (the stand-in repeats sample n c_n times: back to one column per sample, the first of its run)
            first = np.cumsum(counts) - counts
            x = np.where(counts[None, :] > 0, x[:, np.minimum(first, x.shape[1] - 1)], -np.inf)
        N = x.shape[1]
        c = np.ones(N) if counts is None else counts.astype(np.float64)
        k = np.exp(log_kernel_wrapped(self._pts, queries_dm, bandwidth, period, np.float64))
        logsum, wsum = np.empty((L, M)), np.empty(L)
        for l in range(L):
            with np.errstate(invalid="ignore"):
                cb = np.where(c > 0.0, c * np.exp(np.asarray(f_scan, dtype=np.float64)[l] + x[l]), 0.0)
            s, w = np.zeros(M), 0.0
            for n0 in range(0, N, self.CHUNK):
                s = s + np.cumsum(k[:, n0:n0 + self.CHUNK] * cb[None, n0:n0 + self.CHUNK], axis=1)[:, -1]
                w = w + np.cumsum(cb[n0:n0 + self.CHUNK])[-1]
            with np.errstate(divide="ignore"):
                logsum[l], wsum[l] = np.log(s), w
        return logsum, wsum, int(np.sum(~(np.exp(logsum) >= float(FLAG_BELOW)) & (wsum > 0)[:, None]))


class ScanKdeOrderedMatrix(_OrderedKdeSums, ScanOracleMatrix):
    def scan_kde_sums(self, f, coeff_lb, offset_l, f_scan, queries_dm, bandwidth, period=None, center_lb=None, slab=None):
        return self._kde_sums(f, coeff_lb, offset_l, f_scan, queries_dm, bandwidth, period)


class FamilyKdeOrderedMatrix(_OrderedKdeSums, FamilyOracleMatrix):
    def scan_kde_sums(self, f, coeff_lb, offset_l, f_scan, queries_dm, bandwidth, period=None, center_lb=None, slab=None):
        return self._call(center_lb, self._kde_sums, f, coeff_lb, offset_l, f_scan, queries_dm, bandwidth, period)


class FamilyKdeOracleMatrix(_KdeSums, FamilyOracleMatrix):
    def scan_kde_sums(self, f, coeff_lb, offset_l, f_scan, queries_dm, bandwidth, period=None, center_lb=None, slab=None):
        return self._call(center_lb, self._kde_sums, f, coeff_lb, offset_l, f_scan, queries_dm, bandwidth, period)


class FamilyKdeFloat64Matrix(FamilyKdeOracleMatrix):
    real = np.float64


# ---- the cases --------------------------------------------------------------------------------------------------------------------
KDE_N = 2 * 8192 + 37  # three chunks of the kernel, the last one ragged
KDE_L = 300            # past one member panel of either family (256 linear, 128 harmonic)
KDE_M = (1, 16, 150)   # NB = 1; a full block; a panel of 128 (NB = 8) and a second one of 22 (NB = 2, padded)
KDE_ORACLE_MEMBERS = (0, 63, 64, 127, 128, 131, 255, 256, 299)  # the members the long-double oracle is formed for: the panel edges


def kde_panels(M):
    """``[(nb, queries)]`` of the query panels a call of M queries is cut into"""
    return [(scan_nb_for(min(KDE_PANEL, M - q0)), min(KDE_PANEL, M - q0)) for q0 in range(0, M, KDE_PANEL)]


def build_kde_case(spec):
    """``spec = (family, d, M, periodic, L)``: the case of tests/scan_obs_standin.py at K = 9, N = KDE_N (family "linear": B = 5;
    "harmonic": B = 3 with two harmonic terms), the hard variant (multiplicities 0 .. 3, +inf entries, a state without samples, a
    member 900 below the rest).  The points are the first basis vector brought to unit scale and, for d = 2, the sine of 1.7 times
    it plus a tenth of the second basis vector; bandwidth 0.25.  ``periodic``: the first coordinate has period 2.5, so that the
    samples beyond +-1.25 are folded onto the others.  The queries run from inside the samples to one bandwidth outside them."""
    fam, d, M, periodic, L = spec
    case = build_obs_case((fam, 9, KDE_N, L, 5 if fam == "linear" else 3, 0 if fam == "linear" else 2, 1, True))
    y = case["basis"][0]
    y = (y - y.mean()) / (y.std() if y.std() > 0.0 else 1.0)
    pts = [y]
    if d == 2:
        z = case["basis"][1]
        pts.append(np.sin(1.7 * y) + 0.1 * (z - z.mean()) / (z.std() if z.std() > 0.0 else 1.0))
    case["x_dn"] = np.ascontiguousarray(np.stack(pts))
    h = 0.25
    lo, hi = (-1.25, 1.25) if periodic else (max(y.min(), -3.0) - h, min(y.max(), 3.0) + h)
    q = [np.linspace(lo, hi, M) if M > 1 else np.array([0.3])]
    if d == 2:
        q.append(np.sin(1.7 * q[0]) + 0.2 * np.cos(5.0 * np.arange(M)))
    case["q_dm"] = np.ascontiguousarray(np.stack(q))
    case["h"] = h
    case["period"] = (np.array([2.5, 0.0])[:d] if periodic else None)
    return case


def load_kde_case(dm, case):
    dm.set_Nk(case["N_k"])
    dm.set_sample_weights(case["c"])
    if case["family"] == "linear":
        dm.set_scan(case["basis"], None)
    else:
        dm.set_scan(case["basis"], None, harmonic_b=case["harmonic_b"], period_b=case["period_b"])
    dm.set_scan_points(case["x_dn"])


def kde_oracle_for(case, u, real=LD, ordered=False):
    """The long-double stand-in (``real=np.float64``: the same formulas in plain float64 with numpy's pairwise sums; ``ordered``: the
    float64 restatement in the device's order) loaded with the case on the matrix ``u``"""
    if case["family"] == "linear":
        cls = ScanKdeOrderedMatrix if ordered else ScanKdeOracleMatrix if real is LD else ScanKdeFloat64Matrix
    else:
        cls = FamilyKdeOrderedMatrix if ordered else FamilyKdeOracleMatrix if real is LD else FamilyKdeFloat64Matrix
    m = cls(u)
    load_kde_case(m, case)
    return m


def cen_of(case, members=slice(None)):
    return {} if case["center"] is None else dict(center_lb=case["center"][members])


def run_kde(dm, case, f_scan=None, members=slice(None), q_dm=None, **kw):
    """``(f_scan, (logsum, wsum, n_exact))`` of the case's members (or of ``members`` of them) at the case's queries (or ``q_dm``)"""
    coeff, offset = case["coeff"][members], case["offset"][members]
    cen = cen_of(case, members)
    if f_scan is None:
        f_scan = -dm.scan_lognum(case["f"], coeff, offset, **cen)[0]
    q_dm = case["q_dm"] if q_dm is None else q_dm
    return f_scan, dm.scan_kde_sums(case["f"], coeff, offset, f_scan, q_dm, case["h"], period=case["period"], **cen, **kw)


def kde_case_id(spec):
    fam, d, M, periodic, L = spec
    return "%s-d%d-%s-L%d%s" % (fam, d, "+".join("NB%dx%d" % p for p in kde_panels(M)), L, "-periodic" if periodic else "")


def kde_cases():
    """d in {1, 2} x both families x period off and on at M = 150 and L = 300; M = 1 and 16 (NB = 1) in both dimensions and
    families; L = 1."""
    cases = [(fam, d, 150, periodic, KDE_L) for fam in ("linear", "harmonic") for d in (1, 2) for periodic in (False, True)]
    cases += [("linear", 1, 1, False, KDE_L), ("harmonic", 2, 1, True, KDE_L), ("linear", 2, 16, True, KDE_L), ("harmonic", 1, 16, False, KDE_L)]
    cases += [("linear", 2, 150, False, 1), ("harmonic", 1, 150, True, 1)]
    return cases
