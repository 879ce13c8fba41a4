"""CPU stand-in for the scan passes of ``pymbar_amd.device.DeviceMatrix`` (``set_scan`` / ``scan_lognum`` / ``scan_gram_w``) -- TEST
INFRASTRUCTURE ONLY: :class:`tests.cpu_standin.OracleMatrix` plus the three methods in numpy long double.  Sample multiplicities
are emulated as in the base class (column n repeated c_n times); basis and observable vectors are repeated alongside.

Also the builder of the cases the passes are tested at (``build_case`` and what it is made of) and the matrix of cases that
reaches every instantiation of the pass-B kernel (``instantiation_cases``): tests/test_gpu_scan.py runs them on the device,
tests/test_scan_host.py checks on the CPU that they suit the stand-in."""
import numpy as np

from pymbar_amd import testsystems
from tests.cpu_standin import OracleMatrix

LD = np.longdouble


class ScanOracleMatrix(OracleMatrix):
    real = LD  # the number format of the three methods

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
        R = self.real
        basis, t = self._scan
        if self._counts is not None:
            basis, t = np.repeat(basis, self._counts, axis=1), np.repeat(t, self._counts, axis=1)
        coeff_lb = np.asarray(coeff_lb, dtype=R)
        L = coeff_lb.shape[0]
        offset_l = np.zeros(L, dtype=R) if offset_l is None else np.asarray(offset_l, dtype=R)
        logden = self._logden(np.asarray(f, dtype=np.float64)).astype(R)
        x = -(coeff_lb @ basis.astype(R) + offset_l[:, None]) - logden[None, :]
        tj = np.vstack([np.ones((1, basis.shape[1]), dtype=R), t.astype(R)])
        return x, tj, logden

    def scan_lognum(self, f, coeff_lb, offset_l=None):
        x, tj, _ = self._members(f, coeff_lb, offset_l)
        M = x.max(axis=1)
        e = np.exp(x - M[:, None])
        S = e @ tj.T  # (L, J)
        return (M + np.log(S[:, 0])).astype(np.float64), (S / S[:, :1]).astype(np.float64)

    def scan_gram_w(self, f, coeff_lb, offset_l, f_scan, reference=0, cross=True):
        R = self.real
        x, tj, logden = self._members(f, coeff_lb, offset_l)
        f = np.asarray(f, dtype=np.float64)
        b = np.exp(np.asarray(f_scan, dtype=R)[:, None] + x)  # (L, n)
        W = np.exp(f.astype(R)[:, None] - self.u.astype(R) - logden[None, :])  # (K, n)
        bt = b[:, None, :] * tj[None, :, :]  # (L, J, n)
        X = np.einsum("kn,ljn->klj", W, bt).astype(np.float64) if cross else None
        within = np.einsum("lin,ljn->lij", bt, bt).astype(np.float64)
        refcol = np.einsum("n,ljn->lj", b[int(reference)], bt).astype(np.float64)
        return X, within, refcol, b.sum(axis=1).astype(np.float64)


class ScanFloat64Matrix(ScanOracleMatrix):
    """The same formulas in plain float64: what separates it from the long-double stand-in bounds the stand-in's own error"""
    real = np.float64


# ---- the cases --------------------------------------------------------------------------------------------------------------------
FEATURES = (lambda x: x * x, lambda x: x, np.ones_like, np.cos, np.sin, np.abs, np.tanh, lambda x: 0.1 * x ** 3)


def ladder(K, N, seed):
    """A harmonic ladder of K states with N samples in all, and its (x_n, u_kn, N_k, O_k, K_k)"""
    O_k, K_k = np.linspace(0.0, 2.0, K), np.linspace(1.0, 3.0, K)
    N_k = np.full(K, N // K)
    N_k[: N - N_k.sum()] += 1
    x_n, u_kn, N_k, _ = testsystems.harmonic_u_kn(O_k, K_k, N_k, seed=seed)
    return x_n, u_kn, N_k, O_k, K_k


def family(x_n, O_k, K_k, L, B, rng):
    """L members inside the hull of the sampled oscillators in the basis FEATURES[:B] (B >= 3: the offset rides on the constant
    basis vector; beyond that small random admixtures of the other features)"""
    O_l, K_l = rng.uniform(O_k.min(), O_k.max(), L), rng.uniform(K_k.min(), K_k.max(), L)
    basis = np.stack([fn(x_n) for fn in FEATURES[:B]])
    coeff = np.zeros((L, B))
    offset = np.zeros(L)
    if B == 1:
        coeff[:, 0] = 0.5 * K_l
    else:
        _, c2, off = testsystems.harmonic_scan_family(x_n, O_l, K_l)
        coeff[:, :2] = c2
        if B >= 3:
            coeff[:, 2] = off
            coeff[:, 3:] = rng.normal(0.0, 0.2, (L, B - 3))
        else:
            offset = off
    return basis, coeff, offset


def observables(x_n, Q):
    return np.stack([x_n, x_n * x_n, np.cos(x_n)])[:Q]


def build_case(shape, hard, seed=0):
    K, N, L, B, Q = shape
    rng = np.random.default_rng(seed + 17 * K + L)
    x_n, u_kn, N_k, O_k, K_k = ladder(K, N, seed)
    basis, coeff, offset = family(x_n, O_k, K_k, L, B, rng)
    t = observables(x_n, Q)
    t = t - (t.min(axis=1) - 1e-3)[:, None] if Q else t
    f = rng.normal(0.0, 0.3, K)
    c = None
    if L >= 5:
        offset[L - 1] += 900.0  # a member whose x lies far below every other's: its lognum must be finite and right
    if hard:
        c = rng.integers(0, 4, N).astype(np.float64)  # multiplicities 0 .. 3, a quarter of them zero
        if K >= 3:
            u_kn = u_kn.copy()
            u_kn[rng.integers(1, K, N // 20), rng.integers(0, N, N // 20)] = np.inf  # +inf entries (never in row 0)
            N_k = N_k.copy()
            N_k[0] += N_k[K - 1]  # a resident state without samples
            N_k[K - 1] = 0
    return dict(u=u_kn, N_k=N_k, f=f, basis=basis, coeff=coeff, offset=offset, t=t, c=c, ref=min(2, L - 1))


def run_passes(dm, case, members=slice(None), ref=None):
    coeff, offset = case["coeff"][members], case["offset"][members]
    lognum, mean = dm.scan_lognum(case["f"], coeff, offset)
    X, within, refcol, w = dm.scan_gram_w(case["f"], coeff, offset, -lognum, reference=case["ref"] if ref is None else ref)
    return dict(lognum=lognum, mean=mean, cross=X, within=within, refcol=refcol, wsum=w)


def scan_mb(J):
    """Blocks of 16 members one wave of the pass-B kernel owns (mbar_scan.h)"""
    return {1: 4, 2: 2}.get(J, 1)


def scan_nb_for(K):
    """Blocks of 16 states the pass-B kernel is instantiated for (mbar_k_scan.hip)"""
    need = (K + 15) // 16
    return 1 if need <= 1 else 2 if need <= 2 else 4 if need <= 4 else 8


def matrix_L(Q):
    """One full panel of 64 scan_mb(J) members -- every mb round of every wave -- and a second one of two blocks whose second block
    holds one member (waves 2 and 3 of it own nothing)"""
    return 64 * scan_mb(1 + Q) + 17


def case_id(shape):
    K, N, L, B, Q = shape
    return "NB%d-J%d-K%d-N%d-L%d-B%d-Q%d" % (scan_nb_for(K), 1 + Q, K, N, L, B, Q)


def instantiation_cases():
    """(K, N, L, B, Q) of the pass-B instantiation matrix: both ends of every NB (K = 100: block 6 partial, block 7 all padding) x
    every J, at N = 77 (four full tiles of 16 samples and a tail of 13 in one chunk), B cycling over 1, 2, 5, 8; then the edges of
    the sample axis: a chunk edge of pass B (8192) under MB = 4 and under NB = 8, the tile edge (16), and the chunk edge of pass A
    (2048) with a second group of 64 members that holds one."""
    cases = []
    for i, K in enumerate((9, 17, 32, 33, 64, 65, 100, 128)):
        for Q in range(4):
            cases.append((K, 77, matrix_L(Q), (1, 2, 5, 8)[(i + Q) % 4], Q))
    for N in (8192, 8193):
        cases += [(33, N, matrix_L(0), 2, 0), (65, N, matrix_L(3), 5, 3)]
    cases += [(17, N, 20, 8, 1) for N in (1, 15, 16, 17)]
    cases += [(3, N, 65, 5, 3) for N in (2047, 2048, 2049)]
    return cases
