"""CPU stand-in for the moments pass of ``pymbar_amd.device.DeviceMatrix`` (``scan_moments``, ``scan_features``) -- TEST
INFRASTRUCTURE ONLY: the scan stand-ins (tests/scan_standin.py, and tests/family_standin.py for the families with harmonic terms)
plus the one method in numpy long double.  The features are the ones the device's chain is made of: a linear term's basis vector, a
harmonic term's wrapped displacement ``dl`` and ``dl^2``; the ``rint`` of the minimum image is taken in float64, on the float64
difference and the float64 reciprocal of the period as the device takes it, everything else -- the difference itself, the wrap, the
square, the centred products and their sums -- in long double.

Also the cases the pass is tested at on the device (``moment_cases`` / ``build_moment_case``), with what can go wrong in the kernel:
ragged chunks and member panels, every bucket of the feature slots, multiplicities with zeros and a whole chunk of zeros, an
unsampled state, a member 900 below the others, samples exactly at a tie of the minimum image and across the seam."""
import numpy as np

from pymbar_amd.scan import gradient_layout
from tests.family_standin import FamilyOracleMatrix, build_family_case
from tests.scan_standin import build_case

LD = np.longdouble


def features_ld(basis_bn, center_lb, harmonic_b, period_b, L):
    """``phi[l, i, n]`` in long double, in the order of ``gradient_layout``"""
    basis_bn = np.asarray(basis_bn, dtype=np.float64)
    B, N = basis_bn.shape
    harmonic = np.zeros(B, dtype=bool) if harmonic_b is None else np.asarray(harmonic_b, dtype=bool)
    period = np.zeros(B) if period_b is None else np.asarray(period_b, dtype=np.float64)
    features, _ = gradient_layout(B, harmonic)
    phi = np.empty((L, len(features), N), dtype=LD)
    for i, (b, kind) in enumerate(features):
        if kind == "basis":
            phi[:, i, :] = basis_bn[b].astype(LD)[None, :]
            continue
        c = np.asarray(center_lb, dtype=np.float64)[:, b:b + 1]
        dl = basis_bn[b].astype(LD)[None, :] - c.astype(LD)
        P = float(period[b])
        if P > 0.0:
            m = np.rint((basis_bn[b][None, :] - c) * (1.0 / P))  # float64, as the device
            dl = dl - LD(P) * m.astype(LD)
        phi[:, i, :] = dl if kind == "dl" else dl * dl
    return phi


class GradientOracleMatrix(FamilyOracleMatrix):
    """The long-double scan passes and ``scan_moments`` on members whose ``u_l`` is the model's"""

    def scan_features(self):
        B = self._scan[0].shape[0]
        H = 0 if self._kinds is None else int(np.count_nonzero(self._kinds[0]))
        return B, H, B + H

    def _moments(self, f, coeff_lb, offset_l, center_phi):
        R = self.real
        x, tj, _ = self._members(f, coeff_lb, offset_l)
        L = x.shape[0]
        basis = self._scan[0]
        hb, pb = (None, None) if self._kinds is None else self._kinds
        phi = features_ld(basis, self._centers, hb, pb, L)
        if self._counts is not None:
            phi = np.repeat(phi, self._counts, axis=2)
        F = phi.shape[1]
        center_phi = np.zeros((L, F)) if center_phi is None else np.asarray(center_phi, dtype=np.float64)
        if center_phi.shape != (L, F):
            raise ValueError("center_phi must have shape (L, F)")
        M = x.max(axis=1)
        e = np.exp(x - M[:, None])
        S = e @ tj.T  # (L, J)
        J = tj.shape[0]
        m1, m2, ma = np.empty((L, F)), np.empty((L, F, F)), np.empty((L, J - 1, F))
        for l in range(L):
            d = (phi[l] - center_phi[l].astype(R)[:, None]).astype(R)
            w = d * e[l][None, :]
            m1[l] = (w.sum(axis=1) / S[l, 0]).astype(np.float64)
            m2[l] = (np.einsum("in,jn->ij", w, d) / S[l, 0]).astype(np.float64)
            ma[l] = (np.einsum("qn,in->qi", tj[1:], w) / S[l, 0]).astype(np.float64)
        return (M + np.log(S[:, 0])).astype(np.float64), (S / S[:, :1]).astype(np.float64), m1, m2, ma

    def scan_moments(self, f, coeff_lb, offset_l=None, center_phi=None, center_lb=None):
        return self._call(center_lb, self._moments, f, coeff_lb, offset_l, center_phi)


class ScanOnlyMatrix(FamilyOracleMatrix):
    """A handle with the scan passes but without the moments pass"""


# ---- the cases --------------------------------------------------------------------------------------------------------------------
K_CASE = 5
FAMILIES = [(1, 0), (2, 0), (8, 0), (2, 1), (8, 4)]  # (B, H): both ends of the linear bucket of 2, the top of the one of 8, ...


def moment_cases():
    """``(N, L, B, H, Q)``: every (B, H) x every Q, with N in {4097, 6001} (a last chunk of one sample; a ragged third chunk) and L in
    {1, 64, 65, 130} (a lone member, a full panel of 64 lanes, one lane in the second, two full and a ragged one) going round so that
    every family meets every L and both N; then the families between the buckets' ends: (3, 0) -- the bottom of the linear bucket of 8
    --, (1, 1) and (3, 1) -- both ends of the small harmonic bucket --, (4, 1) and (2, 2), the bottom of the large one."""
    cases = []
    Ls, Ns = (1, 64, 65, 130), (4097, 6001)
    for i, (B, H) in enumerate(FAMILIES):
        for Q in (0, 1, 3):
            j = len(cases)
            cases.append((Ns[(i + j) % 2], Ls[(i + j) % 4], B, H, Q))
    # every family also at the L and N the round left out for it
    seen = {(c[1], c[2], c[3]) for c in cases}
    for B, H in FAMILIES:
        for k, Lx in enumerate(Ls):
            if (Lx, B, H) not in seen:
                cases.append((Ns[k % 2], Lx, B, H, (3, 0, 1, 3)[k]))
    cases += [(6001, 65, 3, 0, 1), (4097, 65, 1, 1, 3), (6001, 64, 3, 1, 0), (4097, 130, 4, 1, 1), (6001, 65, 2, 2, 3)]
    return cases


def moment_case_id(case):
    return "N%d-L%d-B%d-H%d-Q%d" % case


def build_moment_case(case):
    """The hard case of tests/scan_standin.py (linear) or tests/family_standin.py (harmonic) at the shape of ``case``, and on top of
    it: the multiplicities of the whole second chunk of 2048 samples are zero; in a harmonic family the first periodic coordinate has
    samples exactly at a tie of the minimum image of member 0 (dl = +-P / 2) and one ulp to either side of it."""
    N, L, B, H, Q = case
    if H == 0:
        c = dict(build_case((K_CASE, N, L, B, Q), True))
        c.update(kinds={}, center=None)
    else:
        c = dict(build_family_case((K_CASE, N, L, B, H, Q), True))
        hb, pb = c["harmonic_b"], c["period_b"]
        b = int(np.flatnonzero(hb & (pb > 0))[0])
        P, c0 = pb[b], c["center"][0, b]
        basis = c["basis"].copy()
        tie = c0 + 0.5 * P
        basis[b, 10:16] = [tie, c0 - 0.5 * P, np.nextafter(tie, np.inf), np.nextafter(tie, -np.inf), tie - P, tie + P]
        c["basis"] = basis
        c.update(kinds=dict(harmonic_b=hb, period_b=pb))
    w = c["c"].copy()
    w[2048:4096] = 0.0
    w[10:16] = 1.0  # (the tie samples count)
    c["c"] = w
    assert np.any(c["N_k"] == 0) and np.any(w[:2048] == 0) and np.all(np.isfinite(c["u"][0]))
    return c


def run_moments(dm, case, center_phi=None, members=slice(None)):
    cen = {} if case["center"] is None else dict(center_lb=case["center"][members])
    cphi = None if center_phi is None else center_phi[members]
    names = ("lognum", "mean", "m1", "m2", "ma")
    return dict(zip(names, dm.scan_moments(case["f"], case["coeff"][members], case["offset"][members], cphi, **cen)))


def scaled_gaps(got, want, t_max):
    """The worst error of every output of the pass in the unit that suits it: ``lognum`` absolute; ``mean`` relative (the shifted
    observables are positive); ``m1[i]`` in units of ``sqrt(m2[i, i])``, ``m2[i, j]`` of ``sqrt(m2[i, i] m2[j, j])`` and ``ma[q, i]`` of
    ``max_n t_q sqrt(m2[i, i])`` -- the bounds Cauchy-Schwarz gives the entries, from the stand-in's numbers: the features have either
    sign, so that an entry can be arbitrarily close to zero and a relative error of its own means nothing."""
    rms = np.sqrt(np.einsum("lii->li", want["m2"]))
    rms = np.where(rms > 0.0, rms, 1.0)
    out = dict(lognum=np.max(np.abs(got["lognum"] - want["lognum"])),
               mean=np.max(np.abs(got["mean"] - want["mean"]) / np.abs(want["mean"])),
               m1=np.max(np.abs(got["m1"] - want["m1"]) / rms),
               m2=np.max(np.abs(got["m2"] - want["m2"]) / (rms[:, :, None] * rms[:, None, :])))
    if want["ma"].shape[1]:
        out["ma"] = np.max(np.abs(got["ma"] - want["ma"]) / (np.asarray(t_max)[None, :, None] * rms[:, None, :]))
    return out
