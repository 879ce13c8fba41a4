"""CPU stand-in for the scan passes of ``pymbar_amd.device.DeviceMatrix`` (``set_scan`` / ``scan_lognum`` / ``scan_gram_w``) -- TEST
INFRASTRUCTURE ONLY: :class:`tests.cpu_standin.OracleMatrix` plus the three methods in numpy long double.  Sample multiplicities
are emulated as in the base class (column n repeated c_n times); basis and observable vectors are repeated alongside."""
import numpy as np

from tests.cpu_standin import OracleMatrix

LD = np.longdouble


class ScanOracleMatrix(OracleMatrix):
    def __init__(self, u_shard, allreduce=None):
        super().__init__(u_shard, allreduce=allreduce)
        self._counts = None
        self._scan = None

    def set_sample_weights(self, c_n):
        super().set_sample_weights(c_n)
        self._counts = None if c_n is None else np.asarray(c_n).astype(np.int64)

    def set_scan(self, basis_bn=None, t_qn=None):
        if basis_bn is None:
            self._scan = None
            return
        N = (self.u_full if hasattr(self, "u_full") else self.u).shape[1]
        basis_bn = np.array(basis_bn, dtype=np.float64)
        t_qn = np.zeros((0, N)) if t_qn is None else np.array(t_qn, dtype=np.float64)
        if basis_bn.ndim != 2 or t_qn.ndim != 2 or basis_bn.shape[1] != N or t_qn.shape[1] != N:
            raise ValueError("basis_bn and t_qn must have N_local columns")
        if not 1 <= basis_bn.shape[0] <= 8 or t_qn.shape[0] > 3:
            raise ValueError("1 <= B <= 8 basis vectors and 0 <= Q <= 3 observables")
        self._scan = (basis_bn, t_qn)

    def _members(self, f, coeff_lb, offset_l):
        """x[l, n] = -u_l(n) - logden_n and t[j, n] (t_0 = 1) over the (resampled) samples, in long double"""
        basis, t = self._scan
        if self._counts is not None:
            basis, t = np.repeat(basis, self._counts, axis=1), np.repeat(t, self._counts, axis=1)
        coeff_lb = np.asarray(coeff_lb, dtype=LD)
        L = coeff_lb.shape[0]
        offset_l = np.zeros(L, dtype=LD) if offset_l is None else np.asarray(offset_l, dtype=LD)
        logden = self._logden(np.asarray(f, dtype=np.float64)).astype(LD)
        x = -(coeff_lb @ basis.astype(LD) + offset_l[:, None]) - logden[None, :]
        tj = np.vstack([np.ones((1, basis.shape[1]), dtype=LD), t.astype(LD)])
        return x, tj, logden

    def scan_lognum(self, f, coeff_lb, offset_l=None):
        x, tj, _ = self._members(f, coeff_lb, offset_l)
        M = x.max(axis=1)
        e = np.exp(x - M[:, None])
        S = e @ tj.T  # (L, J)
        return (M + np.log(S[:, 0])).astype(np.float64), (S / S[:, :1]).astype(np.float64)

    def scan_gram_w(self, f, coeff_lb, offset_l, f_scan, reference=0, cross=True):
        x, tj, logden = self._members(f, coeff_lb, offset_l)
        f = np.asarray(f, dtype=np.float64)
        b = np.exp(np.asarray(f_scan, dtype=LD)[:, None] + x)  # (L, n)
        W = np.exp(f.astype(LD)[:, None] - self.u.astype(LD) - logden[None, :])  # (K, n)
        bt = b[:, None, :] * tj[None, :, :]  # (L, J, n)
        X = np.einsum("kn,ljn->klj", W, bt).astype(np.float64) if cross else None
        within = np.einsum("lin,ljn->lij", bt, bt).astype(np.float64)
        refcol = np.einsum("n,ljn->lj", b[int(reference)], bt).astype(np.float64)
        return X, within, refcol, b.sum(axis=1).astype(np.float64)
