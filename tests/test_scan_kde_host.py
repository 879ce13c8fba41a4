"""Kernel-density surfaces along a scan (``MBAR.compute_scan_kde``), host logic on the CPU stand-in (tests/scan_kde_standin.py): the
reference's own numbers (tests/golden/scan_kde_ho_K5.npz from make_golden_scan_kde.py) at the three reference points, ``f`` against
``compute_scan``'s, the bootstrap spread on hand-made replicates, every refusal, and the new symbols of the built library."""
import ctypes

import numpy as np
import pytest

import pymbar_amd
from pymbar_amd import _lib, scan as scan_module, testsystems
from pymbar_amd.utils import DataError, ParameterError
from tests.conftest import load_golden
from tests.kde_oracle import log_density_ld
from tests.scan_kde_standin import FamilyKdeOracleMatrix, ScanKdeOracleMatrix, log_density_oracle


@pytest.fixture
def standin(monkeypatch):
    import pymbar_amd.device

    monkeypatch.setattr(pymbar_amd.device, "DeviceMatrix", ScanKdeOracleMatrix)


@pytest.fixture(scope="module")
def gold():
    return load_golden("scan_kde_ho_K5.npz")


@pytest.fixture(scope="module")
def config1():
    x_n, u_kn, N_k, _, _, _ = testsystems.config1(seed=0)
    np.testing.assert_array_equal(u_kn, load_golden("config1_ho_K5_N5000.npz")["u_kn"])
    return x_n, u_kn, N_k


def fixture_family_1d(gold, x_n):
    basis, coeff, offset = testsystems.harmonic_scan_family(x_n, gold["a_O_l"], gold["a_K_l"])
    np.testing.assert_array_equal(coeff, gold["a_coeff"])
    np.testing.assert_array_equal(offset, gold["a_offset"])
    return basis, coeff, offset


def fixture_system_2d(gold):
    """The umbrella system of fes_kde.npz (b) as a linear family, and the members of the fixture"""
    g = load_golden("fes_kde.npz")
    basis, coeff_k, offset_k = testsystems.umbrella_2d_family(g["b_x_n"], g["b_u_n"], g["b_umbrella_centers"], float(g["b_Ku"]))
    np.testing.assert_array_equal(gold["b_coeff"][len(gold["b_betas"]):], coeff_k[gold["b_sampled"]])
    return dict(x_n=g["b_x_n"], N_k=g["b_N_k"], basis=basis, coeff_k=coeff_k, offset_k=offset_k, h=float(g["b_bandwidth"]),
                queries=g["b_queries"], coeff=gold["b_coeff"], offset=gold["b_offset"])


def check_1d_against_fixture(mbar, gold, basis, coeff, offset, x_n):
    """The assertions on part (1) of the fixture, shared with the GPU test: the tolerance of
    tests/test_gpu_kde.py::test_fes_kde_1d_reproduces_reference for the same comparison"""
    h, q = float(gold["a_bandwidth"]), gold["a_queries"]
    lo = mbar.compute_scan_kde(x_n, q, h, basis, coeff, offset)
    sp = mbar.compute_scan_kde(x_n, q, h, basis, coeff, offset, reference_point="from-specified", fes_reference=float(gold["a_fes_reference"]))
    nz = mbar.compute_scan_kde(x_n, q, h, basis, coeff, offset, reference_point="from-normalization")
    # (the tree sum of the reference's sklearn is inexact where a member's density is negligible: its f_i are held where its own
    # exact sum -- logsumexp over every sample of its own weights, stored next to them -- says the same, the exact sum everywhere)
    exact = gold["a_exact_L"]
    tree_ok = np.abs(gold["a_f_normalization"] + exact[:, :-1]) <= 1e-9
    assert np.mean(tree_ok) > 0.9 and np.all(tree_ok[np.arange(len(coeff)), np.argmin(gold["a_f_normalization"], axis=1)])
    for res, name in ((lo, "lowest"), (sp, "specified"), (nz, "normalization")):
        print(name, "max |f_i - reference| where its tree sum is exact =", np.max(np.abs(res["f_i"] - gold["a_f_" + name])[tree_ok]))
        assert res["f_i"].shape == (len(coeff), len(q)) == res["log_density"].shape
        np.testing.assert_allclose(res["f_i"][tree_ok], gold["a_f_" + name][tree_ok], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(nz["log_density"], exact[:, :-1], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(sp["f_i"], -exact[:, :-1] + exact[:, -1:], rtol=1e-9, atol=1e-9)
    np.testing.assert_array_equal(lo["reference"], np.argmin(gold["a_f_normalization"], axis=1))
    assert np.all(sp["reference"] == -1) and np.all(nz["reference"] == -1)
    assert lo["log_density"].tobytes() == nz["log_density"].tobytes() == sp["log_density"].tobytes()
    np.testing.assert_array_equal(nz["f_i"], -nz["log_density"])
    assert lo["n_exact"] == 0
    return lo


def test_surfaces_reproduce_reference_1d(standin, gold, config1):
    x_n, u_kn, N_k = config1
    mbar = pymbar_amd.MBAR(u_kn, N_k, relative_tolerance=1e-12)
    basis, coeff, offset = fixture_family_1d(gold, x_n)
    lo = check_1d_against_fixture(mbar, gold, basis, coeff, offset, x_n)
    scan = mbar.compute_scan(basis, coeff, offset)
    assert lo["f"].tobytes() == scan["f"].tobytes()
    one = mbar.compute_scan_kde(x_n.reshape(-1, 1), gold["a_queries"][7:8].reshape(1, 1), float(gold["a_bandwidth"]), basis, coeff[3:4], offset[3:4],
                                reference_point="from-normalization")
    np.testing.assert_allclose(one["log_density"][0, 0], lo["log_density"][3, 7], rtol=1e-13, atol=0)
    assert mbar._dm._scan is None and mbar._dm._pts is None  # nothing is left on the matrix


def test_log_densities_reproduce_exact_reference_2d(standin, gold):
    s = fixture_system_2d(gold)
    u_kn = s["coeff_k"] @ s["basis"] + s["offset_k"][:, None]
    mbar = pymbar_amd.MBAR(u_kn, s["N_k"], relative_tolerance=1e-12)
    np.testing.assert_allclose(mbar.f_k, gold["b_f_k"], atol=1e-9)
    res = mbar.compute_scan_kde(s["x_n"], s["queries"], s["h"], s["basis"], s["coeff"], s["offset"], reference_point="from-specified",
                                fes_reference=[0.0, 0.0])
    exact = gold["b_exact_L"]
    print("max |L - exact| =", np.max(np.abs(res["log_density"] - exact[:, :-1])))
    np.testing.assert_allclose(res["log_density"], exact[:, :-1], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(res["f_i"], -exact[:, :-1] + exact[:, -1:], rtol=1e-9, atol=1e-9)
    # a member with a sampled state's parameters is that state: its free energy
    np.testing.assert_allclose(res["f"][len(gold["b_betas"]):], mbar.f_k[gold["b_sampled"]], rtol=0, atol=1e-10)


def test_oracle_of_the_standin_is_the_kde_oracle(gold, config1):
    """:func:`log_density_oracle` (log weights, minimum image) against tests/kde_oracle.py: log_density_ld where both apply"""
    x_n, u_kn, N_k = config1
    rng = np.random.default_rng(3)
    x_dn = np.stack([x_n[:400], np.cos(x_n[:400])])
    w = rng.random(400)
    w[::7] = 0.0
    q_dm = np.stack([np.linspace(-3, 6, 23), np.linspace(-1, 1, 23)])
    with np.errstate(divide="ignore"):
        got, _, _ = log_density_oracle(x_dn, np.log(w.astype(np.longdouble)), q_dm, 0.3)
    want, _ = log_density_ld(x_dn.T, w, q_dm.T, "gaussian", 0.3)
    np.testing.assert_allclose(got.astype(np.float64), want[:, 0], rtol=1e-15, atol=0)
    # the minimum image: a sample moved by whole periods is the same sample
    moved = x_dn.copy()
    moved[0] += 360.0 * rng.integers(-2, 3, size=400)
    per = np.array([360.0, 0.0])
    with np.errstate(divide="ignore"):
        a = log_density_oracle(x_dn, np.log(w.astype(np.longdouble)), q_dm, 0.3, per)[0]
        b = log_density_oracle(moved, np.log(w.astype(np.longdouble)), q_dm, 0.3, per)[0]
    np.testing.assert_allclose(a.astype(np.float64), b.astype(np.float64), rtol=1e-12, atol=0)


def test_period_none_is_zeros_and_the_seam_is_continuous(monkeypatch):
    import pymbar_amd.device

    monkeypatch.setattr(pymbar_amd.device, "DeviceMatrix", FamilyKdeOracleMatrix)
    basis, coeff_kb, center_kb, harmonic_b, period_b, offset_k, N_k = testsystems.periodic_umbrella_family(K=6, n_per_state=200, seed=2)
    u_kn = testsystems.family_u_kn(basis, coeff_kb, offset_k, center_kb, harmonic_b, period_b)
    mbar = pymbar_amd.MBAR(u_kn, N_k)
    chi = basis[1]
    centers = np.stack([np.zeros(5), np.array([150.0, 170.0, 180.0, -170.0, -150.0])], axis=1)
    coeff = np.tile(coeff_kb[0], (5, 1))
    kw = dict(basis_bn=basis, coeff_lb=coeff, center_lb=centers, harmonic_b=harmonic_b, period_b=period_b, reference_point="from-normalization")
    q = np.array([-180.0, 180.0, 179.999, -179.999, 0.0])
    off = mbar.compute_scan_kde(chi, q, 4.0, **kw)
    zeros = mbar.compute_scan_kde(chi, q, 4.0, period=np.zeros(1), **kw)
    on = mbar.compute_scan_kde(chi, q, 4.0, period=[360.0], **kw)
    assert off["log_density"].tobytes() == zeros["log_density"].tobytes()
    np.testing.assert_allclose(on["log_density"][:, 0], on["log_density"][:, 1], rtol=1e-12, atol=0)  # -180 is +180
    np.testing.assert_allclose(on["log_density"][:, 2], on["log_density"][:, 3], rtol=0, atol=1e-3)
    assert np.all(on["log_density"][:, 0] > off["log_density"][:, 0] + 0.3)  # without the image half the neighbours are missing
    np.testing.assert_allclose(on["log_density"][:, 4], off["log_density"][:, 4], rtol=1e-12, atol=0)  # far from the seam: the same


def test_bootstrap_spread_on_hand_made_replicates():
    spread = scan_module._kde_bootstrap_spread
    # L = 2 members, M = 3 queries and the point of "from-specified" behind them, 4 replicates
    fb = np.array([[[1.0, 2.0, 4.0, 0.5], [0.0, 1.0, 3.0, 1.0]],
                   [[1.5, 2.0, 3.0, 0.0], [0.5, np.inf, 3.5, 1.0]],
                   [[0.5, 2.5, 5.0, 1.0], [np.inf, 1.5, 2.0, 1.0]],
                   [[1.0, 1.0, 4.5, 0.5], [np.nan, np.inf, 2.5, np.inf]]])
    reference = np.array([0, 2])
    lo = spread(fb, reference, "from-lowest", 3)
    assert lo.shape == (2, 3)
    np.testing.assert_allclose(lo[0], np.std(fb[:, 0, :3] - fb[:, 0, 0:1], axis=0), rtol=1e-15)
    assert lo[0, 0] == 0.0
    # member 1: replicate 3 has a NaN / inf everywhere but at the reference query; query 0 has two usable replicates, query 1 two
    np.testing.assert_allclose(lo[1, 0], np.std([0.0 - 3.0, 0.5 - 3.5]), rtol=1e-15)
    np.testing.assert_allclose(lo[1, 1], np.std([1.0 - 3.0, 1.5 - 2.0]), rtol=1e-15)
    assert lo[1, 2] == 0.0
    sp = spread(fb, np.array([-1, -1]), "from-specified", 3)
    np.testing.assert_allclose(sp[0], np.std(fb[:, 0, :3] - fb[:, 0, 3:4], axis=0), rtol=1e-15)
    np.testing.assert_allclose(sp[1, 2], np.std([3.0 - 1.0, 3.5 - 1.0, 2.0 - 1.0]), rtol=1e-15)  # (replicate 3's reference is not finite)
    nz = spread(fb, np.array([-1, -1]), "from-normalization", 3)
    np.testing.assert_allclose(nz[1, 2], np.std(fb[:, 1, 2]), rtol=1e-15)
    np.testing.assert_allclose(nz[1, 0], np.std([0.0, 0.5]), rtol=1e-15)
    # fewer than two usable replicates: NaN
    fb[1, 1, 0] = np.inf
    assert np.isnan(spread(fb, reference, "from-lowest", 3)[1, 0]) and np.isnan(spread(fb, reference, "from-normalization", 3)[1, 0])


def test_bootstrap_rule(standin, gold, config1):
    x_n, u_kn, N_k = config1
    mbar = pymbar_amd.MBAR(u_kn, N_k, n_bootstraps=3, rseed=7)
    basis, coeff, offset = fixture_family_1d(gold, x_n)
    pick = np.array([0, 7, 11])
    q = gold["a_queries"][5:35:3]
    res = mbar.compute_scan_kde(x_n, q, 0.2, basis, coeff[pick], offset[pick], uncertainty_method="bootstrap")
    Lb = res["bootstrapped_log_density"]
    assert Lb.shape == (3, 3, len(q)) and res["df_i"].shape == (3, len(q))
    rows = np.arange(3)
    want = np.std(-Lb + Lb[:, rows, res["reference"]][:, :, None], axis=0)
    np.testing.assert_allclose(res["df_i"], want, rtol=1e-13, atol=1e-15)
    assert np.all(res["df_i"][rows, res["reference"]] == 0.0) and np.sum(res["df_i"] > 0.0) == res["df_i"].size - 3
    # a replicate is that replicate's draw counts and free energies: the dense weights of replicate 1, member 7
    b = 1
    counts = np.bincount(mbar._bootstrap_row(b), minlength=len(x_n))
    u_l = coeff[7] @ basis + offset[7]
    logden = np.log(np.sum(N_k[:, None] * np.exp(mbar.f_k_boots[b][:, None] - u_kn), axis=0))
    with np.errstate(divide="ignore"):
        logw = -u_l - logden + np.log(counts.astype(np.float64))
    ld = log_density_oracle(x_n[None, :], logw, q[None, :], 0.2)[0].astype(np.float64)
    np.testing.assert_allclose(Lb[b, 1], ld, rtol=1e-10, atol=1e-10)
    assert mbar._dm._counts is None and mbar._dm._scan is None and mbar._dm._pts is None


def test_error_paths(standin, gold, config1, monkeypatch):
    x_n, u_kn, N_k = config1
    mbar = pymbar_amd.MBAR(u_kn, N_k)
    basis, coeff, offset = fixture_family_1d(gold, x_n)
    coeff, offset = coeff[:4], offset[:4]
    q = gold["a_queries"]
    call = lambda x=x_n, queries=q, h=0.2, **kw: mbar.compute_scan_kde(x, queries, h, basis, coeff, offset, **kw)
    with pytest.raises(ParameterError, match="d = 1 or 2"):
        call(x=np.stack([x_n, x_n, x_n], axis=1), queries=np.zeros((4, 3)))
    for bad in (x_n[:-1], np.stack([x_n, x_n]), x_n.reshape(-1, 1, 1)):
        with pytest.raises(ParameterError, match="x_n"):
            call(x=bad)
    for bad in (q[:0], np.stack([q, q], axis=1), q.reshape(-1, 1, 1)):
        with pytest.raises(ParameterError, match="queries"):
            call(queries=bad)
    for kernel in ("tophat", "epanechnikov", "exponential", "linear", "cosine"):
        with pytest.raises(ParameterError, match=r'offered by FES\(fes_type="kde"\) only'):
            call(kernel=kernel)
    with pytest.raises(ParameterError, match="kernel must be one of"):
        call(kernel="box")
    for bad in (np.zeros(2), np.zeros((1, 1)), [-1.0], [np.nan], [np.inf]):
        with pytest.raises(ParameterError, match="period"):
            call(period=bad)
    for bad in (0.0, -0.2, np.nan, np.inf, -np.inf, "wide"):
        with pytest.raises(ParameterError, match="bandwidth"):
            call(h=bad)
    with pytest.raises(ParameterError, match="without any bootstraps"):
        call(uncertainty_method="bootstrap")
    with pytest.raises(ParameterError, match="not implemented"):
        call(uncertainty_method="analytical")
    with pytest.raises(ParameterError, match="unavailable"):
        call(reference_point="all-differences")
    with pytest.raises(ParameterError, match="reference point"):
        call(reference_point="from-specified")
    with pytest.raises(DataError, match="fes_reference"):
        call(reference_point="from-specified", fes_reference=[0.0, 1.0])
    for bad in (np.nan, np.inf):
        poisoned = x_n.copy()
        poisoned[11] = bad
        with pytest.raises(DataError):
            call(x=poisoned)
        poisoned = q.copy()
        poisoned[3] = bad
        with pytest.raises(DataError):
            call(queries=poisoned)
    with pytest.raises(ParameterError):
        mbar.compute_scan_kde(x_n, q, 0.2, None, coeff, offset)  # (an object built from a dense u_kn has no basis of its own)
    with pytest.raises(ParameterError):
        mbar.compute_scan_kde(x_n, q, 0.2, basis, coeff[:, :1], offset)
    assert mbar._dm._scan is None and mbar._dm._pts is None  # nothing is left after a refused call
    monkeypatch.setattr(mbar, "K", 129)
    with pytest.raises(ParameterError, match="at most 128 states"):
        call()


def test_handles_without_the_density_pass_are_refused(monkeypatch, config1):
    import pymbar_amd.device
    from tests.scan_standin import ScanOracleMatrix

    monkeypatch.setattr(pymbar_amd.device, "DeviceMatrix", ScanOracleMatrix)
    x_n, u_kn, N_k = config1
    mbar = pymbar_amd.MBAR(u_kn, N_k)
    with pytest.raises(ParameterError, match="not supported on this backend"):
        mbar.compute_scan_kde(x_n, x_n[:3], 0.2, np.stack([x_n * x_n, x_n]), np.ones((2, 2)))


def test_umbrella_2d_family_is_the_dense_system():
    g = load_golden("fes_kde.npz")
    x_n, u_n, xu, Ku = g["b_x_n"], g["b_u_n"], g["b_umbrella_centers"], float(g["b_Ku"])
    basis, coeff, offset = testsystems.umbrella_2d_family(x_n, u_n, xu, Ku)
    dense = np.array([u_n + (Ku / 2) * np.sum((x_n - xu[k]) ** 2, axis=1) for k in range(len(xu))])
    np.testing.assert_allclose(coeff @ basis + offset[:, None], dense, rtol=1e-12, atol=1e-10)
    assert basis.shape == (4, len(x_n)) and coeff.shape == (len(xu), 4)
    with pytest.raises(ValueError):
        testsystems.umbrella_2d_family(x_n[:, 0], u_n, xu, Ku)


def test_library_exports_the_new_symbols():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("mbar_ctx_set_scan_points", "mbar_scan_kde_sums"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["mbar_scan_kde_sums"][1]) == 13
