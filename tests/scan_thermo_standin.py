"""CPU stand-in for the energy passes of ``pymbar_amd.device.DeviceMatrix`` (``scan_energy_lognum`` / ``scan_energy_gram_w``) -- TEST
INFRASTRUCTURE ONLY: :class:`tests.scan_standin.ScanOracleMatrix` (and :class:`tests.family_standin.FamilyOracleMatrix` for the
families with harmonic terms) plus the two methods in numpy long double.  The observable of member ``l`` is its own reduced
potential, ``t_0 = 1``, ``t_1 = u_l(n) - center_u[l]``, ``t_2 = t_1^2``.

Also the cases the two passes are tested at: the shapes of ``instantiation_cases`` re-cut for the energy observable (K at both ends
of every NB, J = 2 and 3), and the positive centre ``min_n u_l(n) - 1e-3`` that makes every product a sum of positive terms, as the
shifted observables of tests/scan_standin.py are."""
import numpy as np

from tests.family_standin import FamilyOracleMatrix, build_family_case, u_model_family
from tests.scan_standin import ScanOracleMatrix, build_case, scan_nb_for

LD = np.longdouble


class EnergyPasses:
    """The two energy passes on whatever ``_members`` of the class evaluates."""

    def _energy_members(self, f, coeff_lb, offset_l, center_u, J):
        if J not in (2, 3):
            raise ValueError("the energy observable takes J = 2 (1, t) or 3 (1, t, t^2)")
        x, _, logden = self._members(f, coeff_lb, offset_l)
        L = x.shape[0]
        center_u = np.zeros(L, dtype=self.real) if center_u is None else np.asarray(center_u, dtype=self.real)
        if center_u.shape != (L,):
            raise ValueError("center_u must have one entry per member")
        t1 = -(x + logden[None, :]) - center_u[:, None]  # u_l(n) - c_l
        tj = np.stack([np.ones_like(t1), t1, t1 * t1][:J], axis=1)  # (L, J, n)
        return x, tj, logden

    def _energy_lognum(self, f, coeff_lb, offset_l, center_u, J):
        x, tj, _ = self._energy_members(f, coeff_lb, offset_l, center_u, J)
        M = x.max(axis=1)
        e = np.exp(x - M[:, None])
        S = np.einsum("ln,ljn->lj", e, tj)
        return (M + np.log(S[:, 0])).astype(np.float64), (S / S[:, :1]).astype(np.float64)

    def _energy_gram_w(self, f, coeff_lb, offset_l, f_scan, center_u, J, reference, cross):
        R = self.real
        x, tj, logden = self._energy_members(f, coeff_lb, offset_l, center_u, J)
        f = np.asarray(f, dtype=np.float64)
        b = np.exp(np.asarray(f_scan, dtype=R)[:, None] + x)
        W = np.exp(f.astype(R)[:, None] - self.u.astype(R) - logden[None, :])
        bt = b[:, None, :] * tj
        X = np.einsum("kn,ljn->klj", W, bt).astype(np.float64) if cross else None
        within = np.einsum("lin,ljn->lij", bt, bt).astype(np.float64)
        refblock = np.einsum("in,ljn->lij", bt[int(reference), :2], bt).astype(np.float64)
        return X, within, refblock, b.sum(axis=1).astype(np.float64)


class ScanThermoOracleMatrix(EnergyPasses, ScanOracleMatrix):
    def scan_energy_lognum(self, f, coeff_lb, offset_l=None, center_u=None, J=3, center_lb=None):
        return self._energy_lognum(f, coeff_lb, offset_l, center_u, J)

    def scan_energy_gram_w(self, f, coeff_lb, offset_l, f_scan, center_u=None, J=3, reference=0, cross=True, center_lb=None):
        return self._energy_gram_w(f, coeff_lb, offset_l, f_scan, center_u, J, reference, cross)


class FamilyThermoOracleMatrix(EnergyPasses, FamilyOracleMatrix):
    def scan_energy_lognum(self, f, coeff_lb, offset_l=None, center_u=None, J=3, center_lb=None):
        return self._call(center_lb, self._energy_lognum, f, coeff_lb, offset_l, center_u, J)

    def scan_energy_gram_w(self, f, coeff_lb, offset_l, f_scan, center_u=None, J=3, reference=0, cross=True, center_lb=None):
        return self._call(center_lb, self._energy_gram_w, f, coeff_lb, offset_l, f_scan, center_u, J, reference, cross)


class ScanOnlyMatrix(ScanOracleMatrix):
    """A handle with the scan passes but without the energy passes"""


# ---- the cases --------------------------------------------------------------------------------------------------------------------
N_CASE = 6001  # a ragged last tile (6001 = 375 x 16 + 1) and a ragged second chunk of pass B; chunks 0 .. 2 of pass A


def energy_mb(J, harmonic):
    """Blocks of 16 members one wave of the pass-B kernel owns under the energy observable (ScanEnergy::mb, mbar_scan.h)"""
    return 1 if harmonic or J > 2 else 2


def energy_L(J, harmonic):
    """A full panel of 64 energy_mb members and a ragged one of two blocks whose second holds one member"""
    return 64 * energy_mb(J, harmonic) + 17


def energy_cases():
    """``(family, K, J)``: both families x K at both ends of every NB x J = 2, 3"""
    return [(fam, K, J) for fam in ("linear", "harmonic") for K in (5, 16, 17, 32, 33, 64, 65, 128) for J in (2, 3)]


def energy_case_id(case):
    fam, K, J = case
    return "%s-NB%d-J%d-K%d" % (fam, scan_nb_for(K), J, K)


def build_energy_case(case):
    """The hard case of tests/scan_standin.py (multiplicities with zeros, +inf entries, a resident state without samples, a member
    900 below the others) or of tests/family_standin.py at the shape of ``case``; the reference member sits in the LAST panel."""
    fam, K, J = case
    L = energy_L(J, fam == "harmonic")
    if fam == "linear":
        c = build_case((K, N_CASE, L, (2, 5, 8, 3)[(K + J) % 4], 0), True)
        c.update(kinds={}, center=None)
    else:
        c = build_family_case((K, N_CASE, L, 3, 2, 0), True)
        c = dict(c)
        c.update(kinds=dict(harmonic_b=c["harmonic_b"], period_b=c["period_b"]), center=c["center"])
    c["ref"] = L - 3
    c["J"] = J
    c["u_members"] = u_model_family(c["basis"], c["coeff"], c["offset"], c["center"], **c["kinds"])
    return c


def positive_center(case):
    """``min_n u_l(n) - 1e-3``: t_1 > 0 at every sample, so that the products are sums of positive terms"""
    return case["u_members"].min(axis=1) - 1e-3


def run_energy_passes(dm, case, center_u, members=slice(None), ref=None, cross=True):
    coeff, offset = case["coeff"][members], case["offset"][members]
    cen = {} if case["center"] is None else dict(center_lb=case["center"][members])
    cu = None if center_u is None else center_u[members]
    lognum, mean = dm.scan_energy_lognum(case["f"], coeff, offset, center_u=cu, J=case["J"], **cen)
    X, within, refblock, w = dm.scan_energy_gram_w(case["f"], coeff, offset, -lognum, center_u=cu, J=case["J"],
                                                   reference=case["ref"] if ref is None else ref, cross=cross, **cen)
    return dict(lognum=lognum, mean=mean, cross=X, within=within, refblock=refblock, wsum=w)
