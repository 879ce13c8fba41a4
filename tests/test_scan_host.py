"""Scans over a linear family of unsampled states (``MBAR.compute_scan``), host logic on the CPU stand-in (tests/scan_standin.py):
the bordered covariance against the dense augmented ``Theta``, the reference's own numbers (tests/golden/scan_ho_K5_L300.npz from
make_golden_scan.py), "approximate", the bootstrap plumbing and the error paths."""
import numpy as np
import pytest

import pymbar_amd
from pymbar_amd import testsystems
from pymbar_amd.utils import DataError, ParameterError
from tests.conftest import load_golden
from tests.scan_standin import ScanFloat64Matrix, ScanOracleMatrix, build_case, case_id, instantiation_cases, run_passes


@pytest.fixture
def standin(monkeypatch):
    import pymbar_amd.device

    monkeypatch.setattr(pymbar_amd.device, "DeviceMatrix", ScanOracleMatrix)


@pytest.fixture(scope="module")
def gold():
    return load_golden("scan_ho_K5_L300.npz")


@pytest.fixture(scope="module")
def config1():
    x_n, u_kn, N_k, _, _, _ = testsystems.config1(seed=0)
    np.testing.assert_array_equal(u_kn, load_golden("config1_ho_K5_N5000.npz")["u_kn"])
    return x_n, u_kn, N_k


def fixture_family(gold, x_n):
    basis, coeff, offset = testsystems.harmonic_scan_family(x_n, gold["O_l"], gold["K_l"])
    np.testing.assert_array_equal(coeff, gold["coeff"])
    np.testing.assert_array_equal(offset, gold["offset"])
    return basis, coeff, offset


def test_harmonic_scan_family_is_the_dense_potential():
    x = np.linspace(-2.0, 5.0, 41)
    O_l, K_l = np.array([0.3, 2.0, 3.7]), np.array([1.5, 4.0, 9.0])
    basis, coeff, offset = testsystems.harmonic_scan_family(x, O_l, K_l)
    assert basis.shape == (2, 41) and coeff.shape == (3, 2) and offset.shape == (3,)
    np.testing.assert_allclose(coeff @ basis + offset[:, None], 0.5 * K_l[:, None] * (x[None, :] - O_l[:, None]) ** 2, rtol=1e-13, atol=1e-13)


def dense_theta_numbers(mbar, basis, coeff, offset, A_qn, res, reference):
    """dDelta_f and sigma from the dense augmented Theta: ``_theta_from_gram`` on ``[W | z]``, z_l0 = b_l, z_lj = b_l t_j / mean_lj"""
    W = mbar._dm.w_kn(mbar.f_k).T  # (N, K)
    logden = mbar._dm.logden(mbar.f_k)
    L, Q = len(coeff), len(A_qn)
    b = np.exp(res["f"][:, None] - (coeff @ basis + offset[:, None]) - logden[None, :])  # (L, N)
    amin = A_qn.min(axis=1) if Q else np.zeros(0)
    shift = amin - np.abs(4.0 * np.finfo(np.float64).eps * amin)
    cols = [b]
    for q in range(Q):
        t = A_qn[q] - shift[q]
        cols.append(b * t[None, :] / (res["mu"][q] - shift[q])[:, None])
    Z = np.vstack(cols).T  # (N, L (1 + Q))
    aug = np.hstack([W, Z])
    N_aug = np.concatenate([mbar.N_k, np.zeros(Z.shape[1], dtype=mbar.N_k.dtype)])
    Theta = mbar._theta_from_gram(aug.T @ aug, N_aug, "svd-ew")[mbar.K:, mbar.K:]
    i = np.arange(L)
    d2 = Theta[i, i] + Theta[reference, reference] - 2.0 * Theta[i, reference]
    d2[reference] = 0.0
    sig = []
    for q in range(Q):
        zi = (1 + q) * L + i
        m = res["mu"][q] - shift[q]
        sig.append(m * np.sqrt(Theta[zi, zi] + Theta[i, i] - 2.0 * Theta[zi, i]))
    return np.sqrt(np.maximum(d2, 0.0)), np.array(sig)


def _bordered_against_dense(mbar, basis, coeff, offset, A_qn, reference):
    res = mbar.compute_scan(basis, coeff, offset, A_qn=A_qn, reference=reference)
    d, s = dense_theta_numbers(mbar, basis, coeff, offset, A_qn, res, reference)
    print("max |dDelta_f - dense| =", np.max(np.abs(res["dDelta_f"] - d)), " max |sigma - dense| =", np.max(np.abs(res["sigma"] - s)))
    np.testing.assert_allclose(res["dDelta_f"], d, rtol=0, atol=1e-12)
    np.testing.assert_allclose(res["sigma"], s, rtol=0, atol=1e-12)


def test_bordered_equals_dense_theta(standin, gold, config1):
    x_n, u_kn, N_k = config1
    mbar = pymbar_amd.MBAR(u_kn, N_k, relative_tolerance=1e-12)
    basis, coeff, offset = fixture_family(gold, x_n)
    pick = np.arange(0, 300, 13)
    _bordered_against_dense(mbar, basis, coeff[pick], offset[pick], np.stack([x_n, x_n * x_n]), reference=3)


def test_bordered_equals_dense_theta_with_an_unsampled_state(standin):
    g = load_golden("ho_unsampled_K4_N2300.npz")
    assert np.any(g["N_k"] == 0)
    mbar = pymbar_amd.MBAR(g["u_kn"], g["N_k"], relative_tolerance=1e-12)
    # a family over the resident rows themselves: basis = three of the rows, members = mixtures of them
    rng = np.random.default_rng(3)
    basis = g["u_kn"][[0, 1, 3]]
    coeff = rng.dirichlet(np.ones(3), size=9)
    offset = rng.normal(0.0, 0.5, 9)
    A = np.stack([g["u_kn"][2], np.cos(g["u_kn"][0])])
    _bordered_against_dense(mbar, basis, coeff, offset, A, reference=0)


@pytest.fixture
def fixture_scan(standin, gold, config1):
    x_n, u_kn, N_k = config1
    mbar = pymbar_amd.MBAR(u_kn, N_k, relative_tolerance=1e-12)
    basis, coeff, offset = fixture_family(gold, x_n)
    return mbar, basis, coeff, offset, np.stack([x_n, x_n * x_n])


def check_against_fixture(res, gold):
    """The assertions on the fixture, shared with the GPU test"""
    np.testing.assert_allclose(res["Delta_f"], gold["Delta_f"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(res["f"] - res["f"][0], gold["Delta_f"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(res["dDelta_f"], gold["dDelta_f"], rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(res["mu"], np.stack([gold["mu_x"], gold["mu_x2"]]), rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(res["sigma"], np.stack([gold["sigma_x"], gold["sigma_x2"]]), rtol=1e-7, atol=1e-9)


def test_scan_reproduces_reference(fixture_scan, gold):
    mbar, basis, coeff, offset, A = fixture_scan
    res = mbar.compute_scan(basis, coeff, offset, A_qn=A)
    assert res["f"].shape == (300,) and res["mu"].shape == (2, 300) and res["sigma"].shape == (2, 300)
    check_against_fixture(res, gold)
    one = mbar.compute_scan(basis, coeff, offset, A_qn=A[1], compute_uncertainty=False)  # an (N,) observable, no uncertainties
    assert "dDelta_f" not in one and "sigma" not in one and one["mu"].shape == (1, 300)
    np.testing.assert_allclose(one["mu"][0], gold["mu_x2"], rtol=1e-9, atol=1e-9)
    free = mbar.compute_scan(basis, coeff, offset)  # free energies only
    assert "mu" not in free and "sigma" not in free
    np.testing.assert_allclose(free["dDelta_f"], gold["dDelta_f"], rtol=1e-7, atol=1e-9)
    other = mbar.compute_scan(basis, coeff, offset, reference=41)
    np.testing.assert_allclose(other["Delta_f"], gold["Delta_f"] - gold["Delta_f"][41], rtol=1e-9, atol=1e-9)
    assert other["dDelta_f"][41] == 0.0 and other["dDelta_f"][0] == pytest.approx(free["dDelta_f"][41], rel=1e-9)


def test_approximate_is_the_members_block_of_the_gram_matrix(fixture_scan):
    mbar, basis, coeff, offset, A = fixture_scan
    pick = np.arange(5, 300, 37)
    res = mbar.compute_scan(basis, coeff[pick], offset[pick], A_qn=A, uncertainty_method="approximate")
    u_ln = coeff[pick] @ basis + offset[pick][:, None]
    dense = mbar.compute_perturbed_free_energies(u_ln, uncertainty_method="approximate")
    np.testing.assert_allclose(res["Delta_f"], dense["Delta_f"][0], rtol=0, atol=1e-11)
    np.testing.assert_allclose(res["dDelta_f"], dense["dDelta_f"][0], rtol=1e-9, atol=1e-12)
    for q in range(2):
        ex = mbar.compute_expectations(A[q], u_kn=u_ln, state_dependent=False, uncertainty_method="approximate")
        np.testing.assert_allclose(res["mu"][q], ex["mu"], rtol=1e-11, atol=1e-11)
        np.testing.assert_allclose(res["sigma"][q], ex["sigma"], rtol=1e-9, atol=1e-12)


def test_bootstrap_plumbing(standin, gold, config1):
    x_n, u_kn, N_k = config1
    mbar = pymbar_amd.MBAR(u_kn, N_k, n_bootstraps=3, rseed=7)
    basis, coeff, offset = fixture_family(gold, x_n)
    pick = np.array([0, 17, 150, 299])
    A = np.stack([x_n, x_n * x_n])
    res = mbar.compute_scan(basis, coeff[pick], offset[pick], A_qn=A, uncertainty_method="bootstrap")
    assert res["bootstrapped_f"].shape == (3, 4) and res["bootstrapped_observables"].shape == (3, 2, 4)
    u_ln = coeff[pick] @ basis + offset[pick][:, None]
    dense = mbar.compute_perturbed_free_energies(u_ln, uncertainty_method="bootstrap")
    np.testing.assert_allclose(res["dDelta_f"], dense["dDelta_f"], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(res["dDelta_f"], np.std(res["bootstrapped_f"], axis=0), rtol=0, atol=0)
    for q in range(2):
        ex = mbar.compute_expectations(A[q], u_kn=u_ln, state_dependent=False, uncertainty_method="bootstrap")
        np.testing.assert_allclose(res["sigma"][q], ex["sigma"], rtol=1e-9, atol=1e-12)
    # the multiplicities are gone again: the resident matrix is the original one
    assert mbar._dm._counts is None and mbar._dm.u.shape == u_kn.shape and mbar._dm._scan is None


def test_error_paths(fixture_scan):
    mbar, basis, coeff, offset, A = fixture_scan
    coeff, offset = coeff[:6], offset[:6]
    with pytest.raises(ParameterError):
        mbar.compute_scan(basis, coeff, offset, uncertainty_method="svd")
    with pytest.raises(ParameterError):
        mbar.compute_scan(basis, coeff, offset, uncertainty_method="nonsense")
    with pytest.raises(ParameterError, match="without any bootstraps"):
        mbar.compute_scan(basis, coeff, offset, uncertainty_method="bootstrap")
    with pytest.raises(ParameterError):
        mbar.compute_scan(basis[:, :-1], coeff, offset)
    with pytest.raises(ParameterError):
        mbar.compute_scan(basis[0], coeff, offset)
    with pytest.raises(ParameterError):
        mbar.compute_scan(np.vstack([basis] * 5)[:9], np.ones((6, 9)), offset)  # B = 9
    with pytest.raises(ParameterError):
        mbar.compute_scan(basis, coeff[:, :1], offset)
    with pytest.raises(ParameterError):
        mbar.compute_scan(basis, coeff[:0], offset[:0])
    with pytest.raises(ParameterError):
        mbar.compute_scan(basis, coeff, offset[:-1])
    with pytest.raises(ParameterError):
        mbar.compute_scan(basis, coeff, offset, A_qn=A[:, :-1])
    with pytest.raises(ParameterError):
        mbar.compute_scan(basis, coeff, offset, A_qn=np.vstack([A, A]))  # Q = 4
    with pytest.raises(ParameterError):
        mbar.compute_scan(basis, coeff, offset, reference=6)
    with pytest.raises(ParameterError):
        mbar.compute_scan(basis, coeff, offset, reference=-1)
    for bad in (np.nan, np.inf):
        poisoned = basis.copy()
        poisoned[1, 3] = bad
        with pytest.raises(DataError):
            mbar.compute_scan(poisoned, coeff, offset)
        poisoned = coeff.copy()
        poisoned[2, 0] = bad
        with pytest.raises(DataError):
            mbar.compute_scan(basis, poisoned, offset)
        poisoned = A.copy()
        poisoned[0, 0] = bad
        with pytest.raises(DataError):
            mbar.compute_scan(basis, coeff, offset, A_qn=poisoned)
    assert mbar._dm._scan is None  # nothing is left on the matrix after a refused call


def test_handles_without_the_scan_passes_are_refused(monkeypatch, config1):
    import pymbar_amd.device
    from tests.cpu_standin import OracleMatrix

    monkeypatch.setattr(pymbar_amd.device, "DeviceMatrix", OracleMatrix)
    x_n, u_kn, N_k = config1
    mbar = pymbar_amd.MBAR(u_kn, N_k)
    with pytest.raises(ParameterError, match="not supported on this backend"):
        mbar.compute_scan(np.stack([x_n * x_n, x_n]), np.ones((2, 2)))


@pytest.mark.parametrize("shape", instantiation_cases(), ids=case_id)
def test_instantiation_cases_suit_the_standin(shape):
    """The cases tests/test_gpu_scan.py holds the device to (rtol 1e-10 with atol 0 on the products, 1e-11 absolute on lognum and
    wsum) are cases at which the long-double stand-in is a reference: everything is finite, the weights are normalised, no entry of
    a product is zero or negative (the shifted observables leave nothing to cancel, so a relative bound alone means something), and
    the same formulas in plain float64 give the same numbers to 1e-12 relative -- a factor 100 under the device's bound.  lognum is
    held to 1e-12 absolute (a factor 10 under the device's): the far member's is about -900, where one ulp is 1.1e-13."""
    case = build_case(shape, True)
    ref = shape[2] - 1
    out = []
    for cls in (ScanOracleMatrix, ScanFloat64Matrix):
        m = cls(case["u"])
        m.set_Nk(case["N_k"])
        m.set_sample_weights(case["c"])
        m.set_scan(case["basis"], case["t"])
        out.append(run_passes(m, case, ref=ref))
    want, plain = out
    for name, v in want.items():
        assert np.all(np.isfinite(v)), name
    np.testing.assert_allclose(want["wsum"], 1.0, rtol=0, atol=1e-13)
    for name in ("cross", "within", "refcol", "mean"):
        assert np.all(want[name] > 0.0), name
    np.testing.assert_allclose(plain["lognum"], want["lognum"], rtol=0, atol=1e-12)
    for name in ("mean", "cross", "within", "refcol", "wsum"):
        np.testing.assert_allclose(plain[name], want[name], rtol=1e-12, atol=0)
