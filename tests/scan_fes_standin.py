"""CPU stand-in for the binned scan passes of ``pymbar_amd.device.DeviceMatrix`` (``set_scan_bins`` / ``scan_bin_lognum`` /
``scan_bin_gram_w``) -- TEST INFRASTRUCTURE ONLY: :class:`tests.scan_standin.ScanOracleMatrix` (and the binned passes of
:class:`tests.hist_standin.HistOracleMatrix`, which the label path under comparison needs) plus the three methods in numpy long
double.  Sample multiplicities are emulated as in the base classes (column n repeated c_n times); the labels are repeated alongside.

Also the builder of the cases the passes are tested at (``build_fes_case``): tests/test_gpu_scan_fes.py runs them on the device,
tests/test_scan_fes_host.py checks on the CPU that they suit the stand-in."""
import numpy as np

from tests.hist_standin import HistOracleMatrix
from tests.scan_standin import ScanOracleMatrix, build_case


class ScanFesOracleMatrix(ScanOracleMatrix, HistOracleMatrix):
    def __init__(self, u_shard, allreduce=None):
        super().__init__(u_shard, allreduce=allreduce)
        self._scan_bins = None

    def set_scan_bins(self, nbins, label_n=None):
        if int(nbins) == 0:
            self._scan_bins = None
            return
        N = (self.u_full if hasattr(self, "u_full") else self.u).shape[1]
        label_n = np.asarray(label_n, dtype=np.int64)
        if label_n.shape != (N,):
            raise ValueError("label_n must have N_local entries")
        if N and (label_n.min() < -1 or label_n.max() >= int(nbins)):
            raise ValueError("labels must lie in [-1, nbins)")
        self._scan_bins = (int(nbins), label_n.copy())

    def _labels(self):
        nbins, label = self._scan_bins
        if self._counts is not None:
            label = np.repeat(label, self._counts)
        return nbins, label

    def scan_bin_lognum(self, f, coeff_lb, offset_l=None):
        nbins, label = self._labels()
        x, _, _ = self._members(f, coeff_lb, offset_l)
        out = np.full((x.shape[0], nbins), -np.inf)
        for i in range(nbins):
            xi = x[:, label == i]
            if xi.shape[1]:
                M = xi.max(axis=1)
                out[:, i] = (M + np.log(np.exp(xi - M[:, None]).sum(axis=1))).astype(np.float64)
        return out

    def scan_bin_gram_w(self, f, coeff_lb, offset_l, f_bins, cross=True, slab=None):
        R = self.real
        nbins, label = self._labels()
        x, _, logden = self._members(f, coeff_lb, offset_l)
        f = np.asarray(f, dtype=np.float64)
        f_bins = np.asarray(f_bins, dtype=R)
        L = x.shape[0]
        W = np.exp(f.astype(R)[:, None] - self.u.astype(R) - logden[None, :])  # (K, n)
        X = np.zeros((self.K, L, nbins)) if cross else None
        d = np.zeros((L, nbins))
        w = np.zeros((L, nbins))
        for i in range(nbins):
            m = label == i
            fin = np.isfinite(f_bins[:, i])  # (+inf: an empty bin of that member, exact zeros)
            Bv = np.zeros((L, int(m.sum())), dtype=R)
            Bv[fin] = np.exp(f_bins[fin, i][:, None] + x[fin][:, m])
            d[:, i] = (Bv * Bv).sum(axis=1).astype(np.float64)
            w[:, i] = Bv.sum(axis=1).astype(np.float64)
            if cross:
                X[:, :, i] = (W[:, m] @ Bv.T).astype(np.float64)
        return X, d, w


class ScanFesFloat64Matrix(ScanFesOracleMatrix):
    """The same formulas in plain float64: what separates it from the long-double stand-in bounds the stand-in's own error"""
    real = np.float64


# ---- the cases --------------------------------------------------------------------------------------------------------------------
EDGE_SIZES = (1, 16, 17, 2047, 2049, 8193)  # bins of exactly these sizes: a single sample, the tile, both chunk lengths and one more


def labels_for(N, nbins, rng, kind):
    """kind "mixed": every bin populated, about a tenth of the samples in no bin; "shuffled": every sample in a random bin;
    "sorted": bins as consecutive runs; "edges": bins of exactly EDGE_SIZES, interleaved, the rest in no bin"""
    if kind == "edges":
        assert nbins == len(EDGE_SIZES) and N >= sum(EDGE_SIZES)
        label = np.full(N, -1, dtype=np.int64)
        label[: sum(EDGE_SIZES)] = np.repeat(np.arange(nbins), EDGE_SIZES)
        return rng.permutation(label)
    if kind == "sorted":
        return np.sort(np.arange(N) % nbins)
    label = np.arange(N) % nbins  # (every bin occurs)
    label = rng.permutation(label)
    if kind == "mixed":
        label[rng.random(N) < 0.1] = -1
        label[:nbins] = np.arange(nbins)
    return label


def build_fes_case(shape, hard, kind="mixed", seed=0):
    """``(K, N, L, B, nbins)``: the case of tests.scan_standin.build_case (Q = 0; hard: multiplicities 0 .. 3, +inf entries in u, an
    unsampled state; a member 800 .. 900 below the others whenever L >= 5) with labels; hard also zeroes the multiplicities of the
    whole of one bin when there are at least two (``emptied``: that bin's number, else None; the last bin, or the bin of 16
    samples of the "edges" labels)."""
    K, N, L, B, nbins = shape
    case = build_case((K, N, L, B, 0), hard, seed=seed)
    rng = np.random.default_rng(seed + 1000 + nbins)
    label = labels_for(N, nbins, rng, kind)
    emptied = None
    if hard and K >= 3:
        # a bin of a few samples keeps finite potentials: its cross entries stay normal numbers (a relative bound means something)
        small = np.isin(label, np.flatnonzero(np.bincount(label[label >= 0], minlength=nbins) < 64))
        case["u"][:, small] = build_case((K, N, L, B, 0), False, seed=seed)["u"][:, small]
    if hard and nbins >= 2:
        emptied = 1 if kind == "edges" else nbins - 1
        case["c"] = case["c"].copy()
        case["c"][label == emptied] = 0.0
        for i in range(nbins):  # (every other bin keeps a sample)
            if i != emptied and not np.any(case["c"][label == i] > 0):
                case["c"][np.flatnonzero(label == i)[0]] = 1.0
    elif hard:
        case["c"][0] = max(case["c"][0], 1.0)
    case.update(label=label, nbins=nbins, emptied=emptied)
    return case


def run_fes_passes(dm, case, members=slice(None), cross=True, **kw):
    coeff, offset = case["coeff"][members], case["offset"][members]
    lognum = dm.scan_bin_lognum(case["f"], coeff, offset)
    X, d, w = dm.scan_bin_gram_w(case["f"], coeff, offset, -lognum, cross=cross, **kw)
    return dict(lognum=lognum, cross=X, diag=d, wsum=w)


def load_case(dm, case):
    dm.set_Nk(case["N_k"])
    dm.set_sample_weights(case["c"])
    dm.set_scan(case["basis"], None)
    dm.set_scan_bins(case["nbins"], case["label"])


PASS_CASES = [((1, 63, 1, 1, 1), "sorted"), ((5, 5000, 300, 3, 7), "mixed"), ((17, 4099, 33, 8, 64), "shuffled"),
              ((128, 6001, 130, 2, 3), "mixed"), ((3, 12400, 5, 2, 6), "edges")]


def check_passes(got, want, case):
    """The assertions of the passes against the long-double stand-in, shared by the GPU test and the float64 check on the CPU"""
    e = case["emptied"]
    live = np.ones(case["nbins"], dtype=bool)
    if e is not None:
        live[e] = False
        assert np.all(got["lognum"][:, e] == -np.inf)
        assert np.all(got["diag"][:, e] == 0.0) and np.all(got["wsum"][:, e] == 0.0) and np.all(got["cross"][:, :, e] == 0.0)
    np.testing.assert_allclose(got["lognum"][:, live], want["lognum"][:, live], rtol=0, atol=1e-11)
    np.testing.assert_allclose(got["wsum"][:, live], want["wsum"][:, live], rtol=0, atol=1e-11)
    np.testing.assert_allclose(got["wsum"][:, live], 1.0, rtol=0, atol=1e-11)
    np.testing.assert_allclose(got["cross"][:, :, live], want["cross"][:, :, live], rtol=1e-10, atol=0)
    np.testing.assert_allclose(got["diag"][:, live], want["diag"][:, live], rtol=1e-10, atol=0)


def check_row_against_label_path(res, l, one):
    """Row ``l`` of a ``compute_scan_fes`` result against ``histogram_fes_labels`` of the same member, at the tolerances of
    tests/test_gpu_scan.py::check_against_dense.  At the reference bin itself the exact ``df`` is 0 and the scan returns 0; the
    label path's bordered form returns ``sqrt(max(Theta_jj + Theta_jj - 2 Theta_jj, 0))`` with the two ``Theta_jj`` summed in
    different orders -- the square root of a rounding residue of a few ulp of ``Theta_jj``, up to about ``sqrt(4 eps Theta_jj)`` =
    3e-8 sqrt(Theta_jj) -- so that one entry is held to that bound instead of to the relative one."""
    j = int(res["reference"][l])
    assert one["reference"] == j
    np.testing.assert_allclose(res["f_raw"][l], one["f_raw"], rtol=0, atol=1e-11)
    np.testing.assert_allclose(res["f_i"][l], one["f_i"], rtol=0, atol=2e-11)
    if "df_i" in one:
        others = np.arange(len(one["df_i"])) != j
        np.testing.assert_allclose(res["df_i"][l][others], one["df_i"][others], rtol=1e-9, atol=1e-14)
        assert res["df_i"][l, j] == 0.0 and 0.0 <= one["df_i"][j] < 1e-7
