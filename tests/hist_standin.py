"""CPU stand-in for the binned passes of ``pymbar_amd.device.DeviceMatrix`` (``set_bins`` / ``bin_lognum`` / ``bin_gram_w``) --
TEST INFRASTRUCTURE ONLY: :class:`tests.cpu_standin.OracleMatrix` plus the three methods in numpy long double.  Sample
multiplicities are emulated as in the base class (column n repeated c_n times); labels and target potential are repeated
alongside.  ``HistOracleMatrix.constructed`` counts constructions (the label path creates no second matrix)."""
import numpy as np

from tests.cpu_standin import OracleMatrix

LD = np.longdouble


def logsumexp_ld(x):
    x = np.asarray(x, dtype=LD)
    if x.size == 0:
        return -np.inf
    m = np.max(x)
    if not np.isfinite(m):
        return float(m)
    return float(m + np.log(np.sum(np.exp(x - m))))


class HistOracleMatrix(OracleMatrix):
    constructed = 0

    def __init__(self, u_shard, allreduce=None):
        super().__init__(u_shard, allreduce=allreduce)
        HistOracleMatrix.constructed += 1
        self._counts = None
        self._bins = None

    def set_sample_weights(self, c_n):
        super().set_sample_weights(c_n)
        self._counts = None if c_n is None else np.asarray(c_n).astype(np.int64)

    def set_bins(self, nbins, label_n=None, v_n=None):
        if int(nbins) == 0:
            self._bins = None
            return
        N = (self.u_full if hasattr(self, "u_full") else self.u).shape[1]
        label_n = np.asarray(label_n, dtype=np.int64)
        v_n = np.asarray(v_n, dtype=np.float64)
        if label_n.shape != (N,) or v_n.shape != (N,):
            raise ValueError("v_n and label_n must have N_local entries")
        if N and (label_n.min() < -1 or label_n.max() >= int(nbins)):
            raise ValueError("labels must lie in [-1, nbins)")
        self._bins = (int(nbins), label_n.copy(), v_n.copy())

    def bins_info(self):
        return dict(sweeps=1, chunks=1, record_bytes=0)

    def _binned(self):
        nbins, label, v = self._bins
        if self._counts is not None:
            label, v = np.repeat(label, self._counts), np.repeat(v, self._counts)
        return nbins, label, v

    def bin_lognum(self, f):
        nbins, label, v = self._binned()
        x = -(v.astype(LD) + self._logden(np.asarray(f, dtype=np.float64)).astype(LD))
        return np.array([logsumexp_ld(x[label == i]) for i in range(nbins)], dtype=np.float64)

    def bin_gram_w(self, f, f_bins, cross=True):
        nbins, label, v = self._binned()
        f = np.asarray(f, dtype=np.float64)
        logden = self._logden(f).astype(LD)
        live = label >= 0
        B = np.zeros(len(label), dtype=LD)
        B[live] = np.exp(np.asarray(f_bins, dtype=LD)[label[live]] - v[live].astype(LD) - logden[live])
        W = np.exp(f.astype(LD)[:, None] - self.u.astype(LD) - logden[None, :])  # (K, n)
        X = np.zeros((self.K, nbins), dtype=LD)
        d = np.zeros(nbins, dtype=LD)
        w = np.zeros(nbins, dtype=LD)
        for i in range(nbins):
            m = label == i
            d[i] = np.sum(B[m] * B[m])
            w[i] = np.sum(B[m])
            if cross:
                X[:, i] = W[:, m] @ B[m]
        return (X.astype(np.float64) if cross else None), d.astype(np.float64), w.astype(np.float64)
