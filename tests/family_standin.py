"""CPU stand-in of the family builders and scan passes of ``pymbar_amd.device.DeviceMatrix`` -- TEST INFRASTRUCTURE ONLY.

``u_model_family`` is the exact statement of the chain the fill kernel and both scan passes evaluate (``family_term``,
pymbar_amd/csrc/mbar_scan_device.h): from the offset, ``b`` ascending, a linear term ``u = fma(cf, v, u)``, a harmonic one

    d = v - c;  P > 0: m = rint(d * rP), d = fma(-P, m, d)  (rP = 1.0 / P);  q = d * d;  u = fma(cf, q, u)

every operation rounded once: the exact vectorised ``fma`` of ``tests/device_math_model.py``, numpy's ``rint`` (ties to even) and
plain float64 ``-`` and ``*``.  ``u_model`` is its name without harmonic terms, the linear family: one fma per term.
``FamilyOracleMatrix`` feeds the long-double stand-ins of the passes (tests/scan_standin.py, tests/scan_fes_standin.py) the
model's ``u_l`` and gives the oracle handle ``from_family`` / ``fill_family_rows`` and, as forwards like the real class's,
``from_linear`` / ``fill_linear_rows``.  Nothing under ``pymbar_amd/`` imports this.

Also the builder of the cases the harmonic passes are tested at (``build_family_case``) and the instantiation matrix of the
harmonic policy's pass-B kernel (``family_instantiation_cases``)."""
import numpy as np

from pymbar_amd import testsystems
from tests.device_math_model import fma
from tests.scan_fes_standin import ScanFesOracleMatrix
from tests.scan_standin import scan_nb_for

LD = np.longdouble


def u_model_family(basis_bn, coeff_kb, offset_k=None, center_kb=None, harmonic_b=None, period_b=None):
    """The ``(K, N)`` float64 matrix the device writes for the family, to the bit."""
    basis_bn = np.asarray(basis_bn, dtype=np.float64)
    coeff_kb = np.asarray(coeff_kb, dtype=np.float64)
    K, B = coeff_kb.shape
    offset_k = np.zeros(K) if offset_k is None else np.asarray(offset_k, dtype=np.float64)
    harmonic_b = np.zeros(B, dtype=bool) if harmonic_b is None else np.asarray(harmonic_b, dtype=bool)
    period_b = np.zeros(B) if period_b is None else np.asarray(period_b, dtype=np.float64)
    u = np.repeat(offset_k[:, None], basis_bn.shape[1], axis=1)
    for b in range(B):
        cf, v = coeff_kb[:, b:b + 1], basis_bn[b][None, :]
        if harmonic_b[b]:
            d = v - np.asarray(center_kb, dtype=np.float64)[:, b:b + 1]
            P = float(period_b[b])
            if P > 0.0:
                rP = 1.0 / P
                m = np.rint(d * rP)
                d = fma(-P, m, d)
            q = d * d
            u = fma(cf, q, u)
        else:
            u = fma(cf, v, u)
    return np.ascontiguousarray(u)


def u_model(basis_bn, coeff_kb, offset_k=None):
    """``u[k, n] = fma(coeff[k, B-1], basis[B-1, n], ... fma(coeff[k, 0], basis[0, n], offset[k]))``, (K, N) float64: the model
    without harmonic terms."""
    return u_model_family(basis_bn, coeff_kb, offset_k)


class FamilyOracleMatrix(ScanFesOracleMatrix):
    """The long-double scan passes (whole and binned cut) on members whose ``u_l`` is the model's, and the family builders."""

    created = 0  # handles made since a test last reset it ("before any device matrix is created")

    def __init__(self, u_shard, allreduce=None):
        type(self).created += 1
        super().__init__(u_shard, allreduce=allreduce)
        self._kinds = None
        self._centers = None

    @classmethod
    def from_linear(cls, basis_bn, coeff_kb, offset_k=None, device=None, columns=None, validate=True):
        return cls.from_family(basis_bn, coeff_kb, offset_k, device=device, columns=columns, validate=validate)

    def fill_linear_rows(self, row0, basis_bn, coeff_rb, offset_r=None, col0=0, validate=True):
        self.fill_family_rows(row0, basis_bn, coeff_rb, offset_r, col0=col0, validate=validate)

    @classmethod
    def from_family(cls, basis_bn, coeff_kb, offset_k=None, center_kb=None, harmonic_b=None, period_b=None, device=None, columns=None,
                    validate=True):
        u = u_model_family(basis_bn, coeff_kb, offset_k, center_kb, harmonic_b, period_b)
        if columns is not None:
            u = u[:, columns[0]:columns[1]]
        return cls(np.array(u))

    def fill_family_rows(self, row0, basis_bn, coeff_rb, offset_r=None, center_rb=None, harmonic_b=None, period_b=None, col0=0,
                         validate=True):
        rows = u_model_family(basis_bn, coeff_rb, offset_r, center_rb, harmonic_b, period_b)[:, col0:col0 + self.N_local]
        self.u[row0:row0 + rows.shape[0]] = rows

    def set_scan(self, basis_bn=None, t_qn=None, harmonic_b=None, period_b=None):
        super().set_scan(basis_bn, t_qn)
        self._kinds = None
        if basis_bn is not None and harmonic_b is not None and np.any(harmonic_b):
            harmonic_b = np.asarray(harmonic_b, dtype=bool)
            if harmonic_b.sum() > 4 or np.any(np.asarray(period_b)[harmonic_b] < 0):
                raise ValueError("at most 4 harmonic terms, periods not negative")
            self._kinds = (harmonic_b, np.zeros(len(harmonic_b)) if period_b is None else np.asarray(period_b, dtype=np.float64))

    def _members(self, f, coeff_lb, offset_l):
        if self._kinds is None:
            return super()._members(f, coeff_lb, offset_l)
        center_lb = self._centers
        if center_lb is None or np.shape(center_lb) != np.shape(coeff_lb):
            raise ValueError("a family with harmonic terms needs the centres of its members")
        R = self.real
        basis, t = self._scan
        if self._counts is not None:
            basis, t = np.repeat(basis, self._counts, axis=1), np.repeat(t, self._counts, axis=1)
        logden = self._logden(np.asarray(f, dtype=np.float64)).astype(R)
        u = u_model_family(basis, coeff_lb, offset_l, center_lb, *self._kinds)
        x = -u.astype(R) - logden[None, :]
        tj = np.vstack([np.ones((1, basis.shape[1]), dtype=R), t.astype(R)])
        return x, tj, logden

    # the four passes: the base classes' formulas, on the members above
    def _call(self, center_lb, fn, *args):
        self._centers = center_lb
        try:
            return fn(*args)
        finally:
            self._centers = None

    def scan_lognum(self, f, coeff_lb, offset_l=None, center_lb=None):
        return self._call(center_lb, super().scan_lognum, f, coeff_lb, offset_l)

    def scan_gram_w(self, f, coeff_lb, offset_l, f_scan, reference=0, cross=True, center_lb=None):
        return self._call(center_lb, super().scan_gram_w, f, coeff_lb, offset_l, f_scan, reference, cross)

    def scan_bin_lognum(self, f, coeff_lb, offset_l=None, center_lb=None):
        return self._call(center_lb, super().scan_bin_lognum, f, coeff_lb, offset_l)

    def scan_bin_gram_w(self, f, coeff_lb, offset_l, f_bins, cross=True, slab=None, center_lb=None):
        return self._call(center_lb, super().scan_bin_gram_w, f, coeff_lb, offset_l, f_bins, cross, slab)


# ---- the cases --------------------------------------------------------------------------------------------------------------------
def harmonic_mb(J):
    """Blocks of 16 members one wave of the harmonic policy's pass-B kernel owns (ScanHarmonic::mb, mbar_scan.h)"""
    return 2 if J == 1 else 1


def build_family_case(shape, hard=True, seed=0):
    """``(K, N, L, B, H, Q)``: K periodic umbrellas on a torsion (period 360) with N samples in all, as the resident matrix; L members
    in a basis of B vectors of which H are harmonic -- the torsion itself (periodic), then sin / cos features of it taken as
    non-periodic and periodic coordinates in turn -- and B - H linear (the energy first).  hard: multiplicities 0 .. 3, an unsampled
    resident state.  The member L - 1 of a call with L >= 5 lies 900 below every other."""
    K, N, L, B, H, Q = shape
    rng = np.random.default_rng(seed + 31 * K + L)
    n_per = -(-N // K)
    basis2, coeff_k, center_k, hb, pb, offset_k, _ = testsystems.periodic_umbrella_family(K=K, n_per_state=n_per, seed=seed)
    pick = np.sort(rng.permutation(K * n_per)[:N])
    E, chi = basis2[0, pick], basis2[1, pick]
    N_k = np.bincount(pick // n_per, minlength=K).astype(np.int64)
    u = testsystems.family_u_kn(np.stack([E, chi]), coeff_k, offset_k, center_k, hb, pb)
    # the scan family: harmonic coordinates first chi (P = 360), then 40 sin(chi) (P = 0), 50 cos(chi) (P = 25), chi / 2 (P = 180);
    # linear ones E, then bounded features of chi
    rad = np.deg2rad(chi)
    hcoords = [(chi, 360.0), (40.0 * np.sin(rad), 0.0), (50.0 * np.cos(rad), 25.0), (0.5 * chi, 180.0)][:H]
    lcoords = [E, np.cos(2 * rad), np.sin(3 * rad), np.ones_like(chi), np.tanh(chi / 90.0), np.cos(rad), np.sin(rad), np.abs(chi) / 180.0][:B - H]
    basis, harmonic_b, period_b = [], [], []
    ih = il = 0
    for b in range(B):  # interleaved: linear and harmonic terms alternate while both last
        take_h = ih < H and (b % 2 == 1 or il >= B - H)
        if take_h:
            basis.append(hcoords[ih][0]), harmonic_b.append(True), period_b.append(hcoords[ih][1])
            ih += 1
        else:
            basis.append(lcoords[il]), harmonic_b.append(False), period_b.append(0.0)
            il += 1
    basis, harmonic_b, period_b = np.stack(basis), np.array(harmonic_b), np.array(period_b)
    coeff = np.where(harmonic_b[None, :], rng.uniform(0.001, 0.004, (L, B)), rng.normal(0.0, 0.3, (L, B)))
    coeff[:, 0] = np.where(harmonic_b[0], coeff[:, 0], rng.uniform(0.8, 1.2, L))
    center = np.where(harmonic_b[None, :], rng.uniform(-200.0, 200.0, (L, B)), 0.0)  # (some centres lie outside the period)
    offset = rng.normal(0.0, 0.5, L)
    if L >= 5:
        offset[L - 1] += 900.0
    t = np.stack([chi, chi * chi, np.cos(rad)])[:Q]
    t = t - (t.min(axis=1) - 1e-3)[:, None] if Q else t
    f = rng.normal(0.0, 0.3, K)
    c = None
    if hard:
        c = rng.integers(0, 4, N).astype(np.float64)
        if K >= 3:
            N_k = N_k.copy()
            N_k[0] += N_k[K - 1]
            N_k[K - 1] = 0
    return dict(u=u, N_k=N_k, f=f, basis=basis, coeff=coeff, center=center, offset=offset, harmonic_b=harmonic_b, period_b=period_b, t=t,
                c=c, ref=min(2, L - 1))


def load_family_case(dm, case, binned=None):
    dm.set_Nk(case["N_k"])
    dm.set_sample_weights(case["c"])
    dm.set_scan(case["basis"], None if binned is not None else case["t"], harmonic_b=case["harmonic_b"], period_b=case["period_b"])
    if binned is not None:
        dm.set_scan_bins(*binned)


def run_family_passes(dm, case, members=slice(None), ref=None):
    coeff, offset, center = case["coeff"][members], case["offset"][members], case["center"][members]
    lognum, mean = dm.scan_lognum(case["f"], coeff, offset, center_lb=center)
    X, within, refcol, w = dm.scan_gram_w(case["f"], coeff, offset, -lognum, reference=case["ref"] if ref is None else ref, center_lb=center)
    return dict(lognum=lognum, mean=mean, cross=X, within=within, refcol=refcol, wsum=w)


def run_family_fes_passes(dm, case, members=slice(None), cross=True, **kw):
    coeff, offset, center = case["coeff"][members], case["offset"][members], case["center"][members]
    lognum = dm.scan_bin_lognum(case["f"], coeff, offset, center_lb=center)
    X, d, w = dm.scan_bin_gram_w(case["f"], coeff, offset, -lognum, cross=cross, center_lb=center, **kw)
    return dict(lognum=lognum, cross=X, diag=d, wsum=w)


PASS_SHAPES = [(1, 63, 1, 1, 1, 0), (5, 5000, 70, 3, 1, 2), (17, 4099, 33, 8, 4, 3), (128, 6001, 130, 2, 1, 1), (3, 8193, 5, 2, 1, 1)]


def family_case_id(shape):
    K, N, L, B, H, Q = shape
    return "NB%d-J%d-K%d-N%d-L%d-B%d-H%d-Q%d" % (scan_nb_for(K), 1 + Q, K, N, L, B, H, Q)


def family_instantiation_cases():
    """(K, N, L, B, H, Q) reaching every (NB, J) the harmonic policy's pass-B kernel is compiled for: one K per NB in {1, 2, 4, 8} x
    every J, at N = 77 (four full tiles of 16 samples and a tail of 13), one full panel of 64 mb(J) members and a second one of two
    blocks whose second block holds one member, H cycling over 1 .. 4."""
    cases = []
    for i, K in enumerate((9, 32, 33, 100)):
        for Q in range(4):
            H = 1 + (i + Q) % 4
            cases.append((K, 77, 64 * harmonic_mb(1 + Q) + 17, (H, H + 1, 8, 5)[(i + Q) % 4], H, Q))
    return cases
