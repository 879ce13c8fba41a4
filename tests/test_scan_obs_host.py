"""Many observables along a scan (``MBAR.compute_scan_expectations``), host logic on the CPU stand-in (tests/scan_obs_standin.py): the
reference's own numbers (tests/golden/scan_observables_ho_K5.npz from make_golden_scan_observables.py), the approximate sigma against
``compute_scan``'s for the same observables, the resident observables, the bootstrap rule and every refusal."""
import numpy as np
import pytest

import pymbar_amd
from pymbar_amd import testsystems
from pymbar_amd.utils import DataError, ParameterError
from tests.conftest import load_golden
from tests.scan_obs_standin import ScanObsOracleMatrix


@pytest.fixture
def standin(monkeypatch):
    import pymbar_amd.device

    monkeypatch.setattr(pymbar_amd.device, "DeviceMatrix", ScanObsOracleMatrix)


@pytest.fixture(scope="module")
def gold():
    return load_golden("scan_observables_ho_K5.npz")


@pytest.fixture(scope="module")
def config1():
    x_n, u_kn, N_k, _, _, _ = testsystems.config1(seed=0)
    np.testing.assert_array_equal(u_kn, load_golden("config1_ho_K5_N5000.npz")["u_kn"])
    return x_n, u_kn, N_k


def fixture_observables(x_n):
    """The observables of the fixture, in its order (make_golden_scan_observables.py)"""
    return np.stack([x_n, x_n * x_n, np.cos(x_n), np.sin(3.0 * x_n), np.abs(x_n), np.tanh(x_n), 1000.0 + x_n])


def fixture_family(gold, x_n):
    basis, coeff, offset = testsystems.harmonic_scan_family(x_n, gold["O_l"], gold["K_l"])
    np.testing.assert_array_equal(coeff, gold["coeff"])
    np.testing.assert_array_equal(offset, gold["offset"])
    return basis, coeff, offset


def check_expectations_against_fixture(res, gold):
    """The assertions on the fixture, shared with the GPU test: the project's reference-fixture tolerances (tests/test_scan_host.py)"""
    print("max |mu - reference| =", np.max(np.abs(res["mu"] - gold["mu"])), " max rel sigma gap =", np.max(np.abs(res["sigma"] / gold["sigma"] - 1.0)))
    assert res["mu"].shape == gold["mu"].shape == res["sigma"].shape
    np.testing.assert_allclose(res["mu"], gold["mu"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(res["sigma"], gold["sigma"], rtol=1e-7, atol=1e-9)
    assert np.all(res["n_eff"] > 900.0) and np.all(res["n_eff"] <= 5000.0)


@pytest.fixture
def fixture_scan(standin, gold, config1):
    x_n, u_kn, N_k = config1
    mbar = pymbar_amd.MBAR(u_kn, N_k, relative_tolerance=1e-12)
    basis, coeff, offset = fixture_family(gold, x_n)
    return mbar, basis, coeff, offset, fixture_observables(x_n)


def test_expectations_reproduce_reference(fixture_scan, gold):
    mbar, basis, coeff, offset, A = fixture_scan
    res = mbar.compute_scan_expectations(A, basis, coeff, offset)
    assert res["f"].shape == (24,) and res["mu"].shape == (7, 24) and res["n_eff"].shape == (24,)
    check_expectations_against_fixture(res, gold)
    scan = mbar.compute_scan(basis, coeff, offset)
    assert res["f"].tobytes() == scan["f"].tobytes()
    one = mbar.compute_scan_expectations(A[3], basis, coeff, offset, compute_uncertainty=False)  # an (N,) observable, means only
    assert "sigma" not in one and one["mu"].shape == (1, 24)
    np.testing.assert_allclose(one["mu"][0], gold["mu"][3], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(one["n_eff"], res["n_eff"], rtol=1e-12, atol=0)
    assert mbar._dm._scan is None and mbar._dm._obs is None  # nothing is left on the matrix


def test_indicator_and_constant_observables(fixture_scan):
    """What the reference cannot take (its shift makes an indicator log 0): the mean of an indicator is the probability of its set, its
    sigma that of a Bernoulli variable under the members' weights; a constant row has its value and sigma 0."""
    mbar, basis, coeff, offset, A = fixture_scan
    x_n = A[0]
    ind = (x_n > 1.0).astype(np.float64)
    res = mbar.compute_scan_expectations(np.stack([ind, np.full_like(x_n, -3.25)]), basis, coeff, offset)
    assert np.all(np.isfinite(res["mu"])) and np.all(np.isfinite(res["sigma"]))
    logden = mbar._dm.logden(mbar.f_k)
    w = np.exp(res["f"][:, None] - (coeff @ basis + offset[:, None]) - logden[None, :])
    p = w @ ind
    np.testing.assert_allclose(res["mu"][0], p, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(res["sigma"][0] ** 2, (w * w) @ (ind - 0.0) ** 2 - 2.0 * p * ((w * w) @ ind) + p * p * np.sum(w * w, axis=1),
                               rtol=1e-9, atol=1e-15)
    np.testing.assert_allclose(res["mu"][1], -3.25, rtol=1e-14, atol=0)
    np.testing.assert_allclose(res["sigma"][1], 0.0, rtol=0, atol=1e-12)


def test_approximate_sigma_is_compute_scans(fixture_scan):
    mbar, basis, coeff, offset, A = fixture_scan
    res = mbar.compute_scan_expectations(A[:3], basis, coeff, offset)
    scan = mbar.compute_scan(basis, coeff, offset, A_qn=A[:3], uncertainty_method="approximate")
    np.testing.assert_allclose(res["mu"], scan["mu"], rtol=1e-11, atol=1e-11)
    np.testing.assert_allclose(res["sigma"], scan["sigma"], rtol=1e-9, atol=1e-12)


def test_resident_observables(fixture_scan, gold):
    mbar, basis, coeff, offset, A = fixture_scan
    mbar.set_scan_observables(A)
    np.testing.assert_array_equal(mbar._scan_obs_shift, A.sum(axis=1) / A.shape[1])
    np.testing.assert_array_equal(mbar._dm._obs, A - mbar._scan_obs_shift[:, None])
    res = mbar.compute_scan_expectations(None, basis, coeff, offset)
    check_expectations_against_fixture(res, gold)
    mbar.compute_scan(basis, coeff[:5], offset[:5], A_qn=A[:2])  # (another scan method in between: the block stays)
    pick = np.array([20, 3, 11])
    sub = mbar.compute_scan_expectations(basis_bn=basis, coeff_lb=coeff[pick], offset_l=offset[pick])
    assert sub["mu"].tobytes() == np.ascontiguousarray(res["mu"][:, pick]).tobytes()
    assert sub["sigma"].tobytes() == np.ascontiguousarray(res["sigma"][:, pick]).tobytes()
    with pytest.raises(ParameterError, match="resident"):  # (an array would replace the resident block)
        mbar.compute_scan_expectations(A[:2], basis, coeff, offset)
    mbar.set_scan_observables(None)
    assert mbar._dm._obs is None
    with pytest.raises(ParameterError, match="none are set"):
        mbar.compute_scan_expectations(None, basis, coeff, offset)


def test_bootstrap_rule(standin, gold, config1):
    x_n, u_kn, N_k = config1
    mbar = pymbar_amd.MBAR(u_kn, N_k, n_bootstraps=3, rseed=7)
    basis, coeff, offset = fixture_family(gold, x_n)
    pick = np.array([0, 7, 23])
    A = fixture_observables(x_n)[:4]
    res = mbar.compute_scan_expectations(A, basis, coeff[pick], offset[pick], uncertainty_method="bootstrap")
    assert res["bootstrapped_f"].shape == (3, 3) and res["bootstrapped_observables"].shape == (3, 4, 3)
    np.testing.assert_allclose(res["sigma"], np.std(res["bootstrapped_observables"], axis=0), rtol=0, atol=0)
    u_ln = coeff[pick] @ basis + offset[pick][:, None]
    for q in range(4):
        ex = mbar.compute_expectations(A[q], u_kn=u_ln, state_dependent=False, uncertainty_method="bootstrap")
        np.testing.assert_allclose(res["sigma"][q], ex["sigma"], rtol=1e-9, atol=1e-12)
    means = mbar.compute_scan_expectations(A, basis, coeff[pick], offset[pick], uncertainty_method="bootstrap", compute_uncertainty=False)
    assert "sigma" not in means and means["bootstrapped_observables"].tobytes() == res["bootstrapped_observables"].tobytes()
    # the multiplicities are gone again: the resident matrix is the original one
    assert mbar._dm._counts is None and mbar._dm.u.shape == u_kn.shape and mbar._dm._scan is None and mbar._dm._obs is None


def test_error_paths(fixture_scan):
    mbar, basis, coeff, offset, A = fixture_scan
    coeff, offset = coeff[:6], offset[:6]
    for method in (None, "svd-ew", "svd"):
        with pytest.raises(ParameterError, match="K x L x Q cross block"):
            mbar.compute_scan_expectations(A, basis, coeff, offset, uncertainty_method=method)
    with pytest.raises(ParameterError, match="unrecognized"):
        mbar.compute_scan_expectations(A, basis, coeff, offset, uncertainty_method="nonsense")
    with pytest.raises(ParameterError, match="without any bootstraps"):
        mbar.compute_scan_expectations(A, basis, coeff, offset, uncertainty_method="bootstrap")
    with pytest.raises(ParameterError, match="none are set"):
        mbar.compute_scan_expectations(None, basis, coeff, offset)
    for bad in (A[:, :-1], np.hstack([A, A[:, :1]]), A[:0], A[None], A[0, :-1]):
        with pytest.raises(ParameterError, match="A_qn"):
            mbar.compute_scan_expectations(bad, basis, coeff, offset)
        with pytest.raises(ParameterError, match="A_qn"):
            mbar.set_scan_observables(bad)
    with pytest.raises(ParameterError):
        mbar.compute_scan_expectations(A, basis[:, :-1], coeff, offset)
    with pytest.raises(ParameterError):
        mbar.compute_scan_expectations(A, basis, coeff[:, :1], offset)
    with pytest.raises(ParameterError):
        mbar.compute_scan_expectations(A, basis, coeff[:0], offset[:0])
    with pytest.raises(ParameterError):
        mbar.compute_scan_expectations(A, basis, coeff, offset[:-1])
    with pytest.raises(ParameterError):
        mbar.compute_scan_expectations(A, None, coeff, offset)  # (an object built from a dense u_kn has no basis of its own)
    for bad in (np.nan, np.inf, -np.inf):
        poisoned = A.copy()
        poisoned[5, 17] = bad
        with pytest.raises(DataError):
            mbar.compute_scan_expectations(poisoned, basis, coeff, offset)
        with pytest.raises(DataError):
            mbar.set_scan_observables(poisoned)
        poisoned = coeff.copy()
        poisoned[2, 0] = bad
        with pytest.raises(DataError):
            mbar.compute_scan_expectations(A, basis, poisoned, offset)
    assert mbar._dm._scan is None and mbar._dm._obs is None and mbar._scan_obs_shift is None  # nothing is left after a refused call


def test_handles_without_the_observable_pass_are_refused(monkeypatch, config1):
    import pymbar_amd.device
    from tests.scan_standin import ScanOracleMatrix

    monkeypatch.setattr(pymbar_amd.device, "DeviceMatrix", ScanOracleMatrix)
    x_n, u_kn, N_k = config1
    mbar = pymbar_amd.MBAR(u_kn, N_k)
    with pytest.raises(ParameterError, match="not supported on this backend"):
        mbar.compute_scan_expectations(x_n, np.stack([x_n * x_n, x_n]), np.ones((2, 2)))
    with pytest.raises(ParameterError, match="not supported on this backend"):
        mbar.set_scan_observables(x_n)
