"""CPU stand-in for the pair pass of ``pymbar_amd.device.DeviceMatrix`` (``scan_pair_gram``, the members' own Gram block behind
``MBAR.compute_scan_pairs``) -- TEST INFRASTRUCTURE ONLY: :class:`tests.scan_standin.ScanOracleMatrix` plus the one method in numpy
long double, and the same on the stand-in of the families with harmonic terms (:class:`tests.family_standin.FamilyOracleMatrix`).

Also the builder of the cases the pass is tested at and the matrix of cases that reaches every instantiation of the kernel
(``pair_cases``): tests/test_gpu_scan_pairs.py runs them on the device, tests/test_scan_pairs_host.py checks on the CPU that they
suit the stand-in."""
import numpy as np

from tests.family_standin import FamilyOracleMatrix, build_family_case, harmonic_mb
from tests.scan_standin import ScanOracleMatrix, build_case, scan_mb


class _PairGram:
    def _pair_gram(self, f, coeff_lb, offset_l, f_scan, rows):
        R = self.real
        x, tj, _ = self._members(f, coeff_lb, offset_l)
        b = np.exp(np.asarray(f_scan, dtype=R)[:, None] + x)  # (L, n)
        bt = b[:, None, :] * tj[None, :, :]  # (L, J, n)
        return np.einsum("rin,ljn->rlij", bt[np.asarray(rows, dtype=np.int64)], bt).astype(np.float64)


class ScanPairsOracleMatrix(_PairGram, ScanOracleMatrix):
    def scan_pair_gram(self, f, coeff_lb, offset_l, f_scan, rows, center_lb=None, slab=None):
        return self._pair_gram(f, coeff_lb, offset_l, f_scan, rows)


class ScanPairsFloat64Matrix(ScanPairsOracleMatrix):
    """The same formulas in plain float64: what separates it from the long-double stand-in bounds the stand-in's own error"""
    real = np.float64


class FamilyPairsOracleMatrix(_PairGram, FamilyOracleMatrix):
    def scan_pair_gram(self, f, coeff_lb, offset_l, f_scan, rows, center_lb=None, slab=None):
        return self._call(center_lb, self._pair_gram, f, coeff_lb, offset_l, f_scan, rows)


class FamilyPairsFloat64Matrix(FamilyPairsOracleMatrix):
    real = np.float64


# ---- the cases --------------------------------------------------------------------------------------------------------------------
PAIR_NB = (2, 8)  # blocks of 16 rows the pair kernel is instantiated for (mbar_k_scan.hip)


def pair_rows(nb, J):
    """Reference members of a row panel of 16 nb rows (scan_pair_rows, mbar_scan.h)"""
    return 16 * nb // J


def pair_panels(R, J):
    """``[(nb, reference members)]`` of the row panels a call with R reference members is cut into (mbar_scan_pair_gram)"""
    out = []
    while R > 0:
        nb = 2 if R <= pair_rows(2, J) else 8
        rm = min(R, pair_rows(nb, J))
        out.append((nb, rm))
        R -= rm
    return out


def build_pair_case(spec):
    """``spec = (family, K, N, L, B, H, Q, R, hard)``: the case of tests/scan_standin.py (family "linear", H = 0) or of
    tests/family_standin.py ("harmonic"), with the normalisers of its members (``f_scan``, from the long-double pass A) and R
    reference members scattered over the call, not sorted."""
    fam, K, N, L, B, H, Q, R, hard = spec
    if fam == "linear":
        case = build_case((K, N, L, B, Q), hard)
        case.update(center=None, harmonic_b=None, period_b=None)
    else:
        case = build_family_case((K, N, L, B, H, Q), hard)
    rng = np.random.default_rng(1000 + R + L)
    case["rows"] = rng.permutation(L)[:R].astype(np.int64)
    case["family"] = fam
    return case


def oracle_for(case, u, cls=None):
    """The long-double stand-in (or ``cls`` of the same kind) loaded with the case on the matrix ``u``"""
    if cls is None:
        cls = ScanPairsOracleMatrix if case["family"] == "linear" else FamilyPairsOracleMatrix
    m = cls(u)
    load_pair_case(m, case)
    return m


def load_pair_case(dm, case):
    dm.set_Nk(case["N_k"])
    dm.set_sample_weights(case["c"])
    if case["family"] == "linear":
        dm.set_scan(case["basis"], case["t"])
    else:
        dm.set_scan(case["basis"], case["t"], harmonic_b=case["harmonic_b"], period_b=case["period_b"])


def cen_of(case, members=slice(None)):
    return {} if case["center"] is None else dict(center_lb=case["center"][members])


def run_pair(dm, case, f_scan=None, rows=None, members=slice(None), **kw):
    """``(f_scan, pair)`` of the case's members (or of ``members`` of them, ``rows`` then indexing into those)"""
    coeff, offset = case["coeff"][members], case["offset"][members]
    cen = cen_of(case, members)
    if f_scan is None:
        f_scan = -dm.scan_lognum(case["f"], coeff, offset, **cen)[0]
    rows = case["rows"] if rows is None else rows
    return f_scan, dm.scan_pair_gram(case["f"], coeff, offset, f_scan, rows, **cen, **kw)


def pair_mb(fam, J):
    return scan_mb(J) if fam == "linear" else harmonic_mb(J)


def pair_case_id(spec):
    fam, K, N, L, B, H, Q, R, hard = spec
    panels = "+".join("NB%dx%d" % p for p in pair_panels(R, 1 + Q))
    return "%s-J%d-%s-N%d-L%d-B%d-H%d-R%d%s" % (fam, 1 + Q, panels, N, L, B, H, R, "-hard" if hard else "")


def pair_cases():
    """The matrix of the pair kernel: both families x J = 1 .. 4 x both row-panel widths, K = 3 (the kernel reads the matrix only
    through logden).  Per (family, J): a narrow row panel that is exactly full (NB = 2) against one member panel plus 17 members at
    N = 77 (four full tiles of 16 samples and a tail of 13), and a wide row panel (NB = 8) one reference member short, exactly full
    and one over (the one over is a second, narrow panel of one member) at N = 45; B cycles over 1, 2, 5, 8 (the harmonic family:
    H = 1 .. 4 of B = H, H + 1, 8, 5).  Then the edges of the sample axis: the tile edge (1, 15, 16, 17) and the chunk edge (8191,
    8192, 8193), and the hard variant of the cases (multiplicities 0 .. 3, +inf entries, a state without samples) in both families,
    one of them with a periodic term whose centres are swept across the seam (build_family_case: the centres lie in [-200, 200]
    about a torsion of period 360)."""
    cases = []
    for fi, fam in enumerate(("linear", "harmonic")):
        for Q in range(4):
            J = 1 + Q
            Lp = 64 * pair_mb(fam, J) + 17
            Hs = [1 + (fi + Q + i) % 4 for i in range(4)]
            Bs = [(1, 2, 5, 8)[(Q + i) % 4] for i in range(4)] if fam == "linear" else [(h, h + 1, 8, 5)[(Q + i) % 4] for i, h in enumerate(Hs)]
            Hs = Hs if fam == "harmonic" else [0] * 4
            full2, full8 = pair_rows(2, J), pair_rows(8, J)
            cases.append((fam, 3, 77, Lp, Bs[0], Hs[0], Q, full2, False))
            for i, R in enumerate((full8 - 1, full8, full8 + 1)):
                cases.append((fam, 3, 45, max(Lp, R), Bs[1 + i], Hs[1 + i], Q, R, False))
    cases += [("linear", 3, N, 20, 8, 0, 1, 5, False) for N in (1, 15, 16, 17)]
    cases += [("linear", 3, 8191, 70, 2, 0, 0, 40, False), ("linear", 3, 8192, 20, 5, 0, 3, 9, True), ("harmonic", 3, 8193, 40, 3, 2, 1, 17, False)]
    cases += [("linear", 3, 211, 37, 5, 0, 2, 37, True), ("harmonic", 3, 211, 37, 4, 3, 2, 11, True), ("harmonic", 3, 300, 33, 2, 1, 0, 33, True)]
    return cases
