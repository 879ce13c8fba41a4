"""Differences between any two members of a scan (``MBAR.compute_scan_pairs``), host logic on the CPU stand-in
(tests/scan_pairs_standin.py): the reference's own full matrices (tests/golden/scan_pairs_ho_K5.npz from make_golden_scan_pairs.py),
every row against ``compute_scan`` with that reference member, the dense path's matrices, "approximate", the bootstrap rule, the
error paths, and that the cases of the instantiation matrix suit the stand-in."""
import numpy as np
import pytest

import pymbar_amd
from pymbar_amd import testsystems
from pymbar_amd.utils import DataError, ParameterError
from tests.conftest import load_golden
from tests.scan_pairs_standin import (FamilyPairsFloat64Matrix, ScanPairsFloat64Matrix, ScanPairsOracleMatrix, build_pair_case, oracle_for,
                                      pair_case_id, pair_cases, pair_panels, run_pair)

MEMBERS = np.arange(0, 300, 7)


@pytest.fixture
def standin(monkeypatch):
    import pymbar_amd.device

    monkeypatch.setattr(pymbar_amd.device, "DeviceMatrix", ScanPairsOracleMatrix)


@pytest.fixture(scope="module")
def gold():
    return load_golden("scan_pairs_ho_K5.npz")


@pytest.fixture(scope="module")
def system():
    scan = load_golden("scan_ho_K5_L300.npz")
    x_n, u_kn, N_k, _, _, _ = testsystems.config1(seed=0)
    np.testing.assert_array_equal(u_kn, load_golden("config1_ho_K5_N5000.npz")["u_kn"])
    basis, coeff, offset = testsystems.harmonic_scan_family(x_n, scan["O_l"][MEMBERS], scan["K_l"][MEMBERS])
    return dict(u_kn=u_kn, N_k=N_k, basis=basis, coeff=coeff, offset=offset, A=np.stack([x_n, x_n * x_n]))


@pytest.fixture
def fixture_pairs(standin, system):
    mbar = pymbar_amd.MBAR(system["u_kn"], system["N_k"], relative_tolerance=1e-12)
    return mbar, system["basis"], system["coeff"], system["offset"], system["A"]


def check_pairs_against_fixture(res, gold, rows=slice(None)):
    """The assertions on the fixture, shared with the GPU test: the tolerances of tests/test_scan_host.py::check_against_fixture for
    the same quantities"""
    np.testing.assert_array_equal(gold["members"], MEMBERS)
    np.testing.assert_allclose(res["Delta_f"], gold["Delta_f"][rows], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(res["dDelta_f"], gold["dDelta_f"][rows], rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(res["Delta_mu"], np.stack([gold["mu_x"][rows], gold["mu_x2"][rows]]), rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(res["dDelta_mu"], np.stack([gold["sigma_x"][rows], gold["sigma_x2"][rows]]), rtol=1e-7, atol=1e-9)


def test_pairs_reproduce_reference(fixture_pairs, gold):
    mbar, basis, coeff, offset, A = fixture_pairs
    res = mbar.compute_scan_pairs(basis, coeff, offset, A_qn=A)
    L = len(MEMBERS)
    assert res["f"].shape == (L,) and res["mu"].shape == (2, L) and res["Delta_f"].shape == (L, L) and res["dDelta_mu"].shape == (2, L, L)
    np.testing.assert_array_equal(res["members"], np.arange(L))
    check_pairs_against_fixture(res, gold)
    assert np.all(np.diag(res["dDelta_f"]) == 0.0) and np.all(np.diag(res["Delta_f"]) == 0.0)
    for q in range(2):
        assert np.all(np.diag(res["dDelta_mu"][q]) == 0.0)
    np.testing.assert_allclose(res["cov_f"], res["cov_f"].T, rtol=1e-12, atol=1e-15)
    # a scattered subset: rows of the same matrices; free energies only; no uncertainties
    rows = np.array([41, 3, 17])
    sub = mbar.compute_scan_pairs(basis, coeff, offset, A_qn=A, reference_members=rows)
    np.testing.assert_array_equal(sub["members"], rows)
    check_pairs_against_fixture(sub, gold, rows)
    free = mbar.compute_scan_pairs(basis, coeff, offset, reference_members=rows)
    assert "mu" not in free and "dDelta_mu" not in free and "cov_mu" not in free
    np.testing.assert_allclose(free["dDelta_f"], gold["dDelta_f"][rows], rtol=1e-7, atol=1e-9)
    bare = mbar.compute_scan_pairs(basis, coeff, offset, A_qn=A[0], compute_uncertainty=False)
    assert "dDelta_f" not in bare and "cov_f" not in bare and bare["Delta_mu"].shape == (1, L, L)
    assert mbar._dm._scan is None


def test_rows_are_compute_scan_with_that_reference(fixture_pairs):
    mbar, basis, coeff, offset, A = fixture_pairs
    rows = np.array([40, 0, 22])
    for method in (None, "approximate"):
        res = mbar.compute_scan_pairs(basis, coeff, offset, A_qn=A, reference_members=rows, uncertainty_method=method)
        for i, r in enumerate(rows):
            one = mbar.compute_scan(basis, coeff, offset, A_qn=A, reference=int(r), uncertainty_method=method)
            assert res["f"].tobytes() == one["f"].tobytes() and res["mu"].tobytes() == one["mu"].tobytes()
            assert res["Delta_f"][i].tobytes() == one["Delta_f"].tobytes()
            np.testing.assert_allclose(res["dDelta_f"][i], one["dDelta_f"], rtol=1e-9, atol=0)
            # the entry of a member with itself is exactly 0; its covariance with itself is the variance compute_scan reports
            assert res["dDelta_f"][i, r] == 0.0
            np.testing.assert_allclose(np.sqrt(res["cov_mu"][:, i, r]), one["sigma"][:, r], rtol=1e-9, atol=0)


def test_pairs_equal_the_dense_path(fixture_pairs):
    mbar, basis, coeff, offset, A = fixture_pairs
    pick = np.arange(2, 43, 5)
    u_ln = coeff[pick] @ basis + offset[pick][:, None]
    for method in (None, "approximate"):
        res = mbar.compute_scan_pairs(basis, coeff[pick], offset[pick], A_qn=A, uncertainty_method=method)
        dense = mbar.compute_perturbed_free_energies(u_ln, uncertainty_method=method)
        np.testing.assert_allclose(res["Delta_f"], dense["Delta_f"], rtol=0, atol=2e-11)
        np.testing.assert_allclose(res["dDelta_f"], dense["dDelta_f"], rtol=1e-9, atol=1e-12)
        for q in range(2):
            ex = mbar.compute_expectations(A[q], u_kn=u_ln, state_dependent=False, output="differences", uncertainty_method=method)
            np.testing.assert_allclose(res["Delta_mu"][q], ex["mu"], rtol=1e-10, atol=1e-11)
            np.testing.assert_allclose(res["dDelta_mu"][q], ex["sigma"], rtol=1e-9, atol=1e-12)


def test_an_entry_does_not_depend_on_the_other_entries(fixture_pairs):
    mbar, basis, coeff, offset, A = fixture_pairs
    full = mbar.compute_scan_pairs(basis, coeff, offset, A_qn=A)
    two = [5, 31]
    lone = mbar.compute_scan_pairs(basis, coeff[two], offset[two], A_qn=A, reference_members=np.array([0]))
    # (the stand-in's einsum sums every entry on its own: what is pinned here is the host algebra)
    for key in ("Delta_f", "cov_f", "dDelta_f"):
        assert lone[key][0, 1] == full[key][5, 31], key
    for key in ("Delta_mu", "cov_mu", "dDelta_mu"):
        assert lone[key][:, 0, 1].tobytes() == full[key][:, 5, 31].tobytes(), key


def test_bootstrap_is_the_std_of_the_differences(standin, system):
    mbar = pymbar_amd.MBAR(system["u_kn"], system["N_k"], n_bootstraps=4, rseed=7)
    # hand-made replicates: what is checked is the rule, not the solver
    rng = np.random.default_rng(5)
    mbar.f_k_boots = mbar.f_k[None, :] + rng.normal(0.0, 0.05, (4, mbar.K))
    mbar.f_k_boots[:, 0] = 0.0
    pick = np.array([0, 9, 20, 42])
    rows = np.array([2, 0])
    basis, coeff, offset, A = system["basis"], system["coeff"][pick], system["offset"][pick], system["A"]
    res = mbar.compute_scan_pairs(basis, coeff, offset, A_qn=A, reference_members=rows, uncertainty_method="bootstrap")
    one = mbar.compute_scan(basis, coeff, offset, A_qn=A, uncertainty_method="bootstrap")
    assert "cov_f" not in res and "cov_mu" not in res
    fb, Ab = res["bootstrapped_f"], res["bootstrapped_observables"]
    assert fb.shape == (4, 4) and Ab.shape == (4, 2, 4)
    assert fb.tobytes() == one["bootstrapped_f"].tobytes() and Ab.tobytes() == one["bootstrapped_observables"].tobytes()
    for i, r in enumerate(rows):
        for l in range(4):
            assert res["dDelta_f"][i, l] == np.std(fb[:, l] - fb[:, r])
            for q in range(2):
                assert res["dDelta_mu"][q, i, l] == np.std(Ab[:, q, l] - Ab[:, q, r])
        assert res["dDelta_f"][i, r] == 0.0
    # the spread of a difference is not the per-state spread compute_scan reports
    assert np.all(res["dDelta_f"][0, [0, 1, 3]] > 0.0) and not np.allclose(res["dDelta_f"][0], one["dDelta_f"])
    assert mbar._dm._counts is None and mbar._dm._scan is None
    with pytest.raises(ParameterError, match="without any bootstraps"):
        pymbar_amd.MBAR(system["u_kn"], system["N_k"]).compute_scan_pairs(basis, coeff, offset, uncertainty_method="bootstrap")


def test_error_paths(fixture_pairs):
    mbar, basis, coeff, offset, A = fixture_pairs
    coeff, offset = coeff[:6], offset[:6]
    with pytest.raises(ParameterError):
        mbar.compute_scan_pairs(basis, coeff, offset, uncertainty_method="svd")
    with pytest.raises(ParameterError):
        mbar.compute_scan_pairs(basis, coeff, offset, uncertainty_method="nonsense")
    for bad in (np.array([0, 0]), np.array([6]), np.array([-1]), np.array([], dtype=np.int64), np.array([[0, 1]]), np.array([0.0, 1.0]), 3):
        with pytest.raises(ParameterError, match="reference_members"):
            mbar.compute_scan_pairs(basis, coeff, offset, reference_members=bad)
    with pytest.raises(ParameterError):
        mbar.compute_scan_pairs(basis[:, :-1], coeff, offset)
    with pytest.raises(ParameterError):
        mbar.compute_scan_pairs(np.vstack([basis] * 5)[:9], np.ones((6, 9)), offset)  # B = 9
    with pytest.raises(ParameterError):
        mbar.compute_scan_pairs(basis, coeff[:, :1], offset)
    with pytest.raises(ParameterError):
        mbar.compute_scan_pairs(basis, coeff[:0], offset[:0])
    with pytest.raises(ParameterError):
        mbar.compute_scan_pairs(basis, coeff, offset[:-1])
    with pytest.raises(ParameterError):
        mbar.compute_scan_pairs(basis, coeff, offset, A_qn=A[:, :-1])
    with pytest.raises(ParameterError):
        mbar.compute_scan_pairs(basis, coeff, offset, A_qn=np.vstack([A, A]))  # Q = 4
    with pytest.raises(ParameterError):
        mbar.compute_scan_pairs(None, coeff, offset)  # (not an object made from a family)
    poisoned = coeff.copy()
    poisoned[2, 0] = np.nan
    with pytest.raises(DataError):
        mbar.compute_scan_pairs(basis, poisoned, offset)
    assert mbar._dm._scan is None  # nothing is left on the matrix after a refused call


def test_handles_without_the_pair_pass_are_refused(monkeypatch, system):
    import pymbar_amd.device
    from tests.scan_standin import ScanOracleMatrix

    monkeypatch.setattr(pymbar_amd.device, "DeviceMatrix", ScanOracleMatrix)
    mbar = pymbar_amd.MBAR(system["u_kn"], system["N_k"])
    with pytest.raises(ParameterError, match="not supported on this backend"):
        mbar.compute_scan_pairs(system["basis"], system["coeff"][:3], system["offset"][:3])


def test_the_matrix_reaches_every_instantiation():
    """Both families x J = 1 .. 4 x both row-panel widths (the kernel's template arguments), and every panel edge the issue names"""
    reached = set()
    for spec in pair_cases():
        fam, Q, R = spec[0], spec[6], spec[7]
        for nb, rm in pair_panels(R, 1 + Q):
            reached.add((fam, 1 + Q, nb))
    assert reached == {(fam, J, nb) for fam in ("linear", "harmonic") for J in (1, 2, 3, 4) for nb in (2, 8)}


@pytest.mark.parametrize("spec", pair_cases(), ids=pair_case_id)
def test_pair_cases_suit_the_standin(spec):
    """The cases tests/test_gpu_scan_pairs.py holds the device to (rtol 1e-10 with atol 0) are cases at which the long-double
    stand-in is a reference: every entry is finite and above 1e-280 (the shifted observables leave nothing to cancel, so a relative
    bound alone means something), and the same formulas in plain float64 give the same numbers to 1e-11 relative -- a tenth of the
    device's bound."""
    case = build_pair_case(spec)
    want_m = oracle_for(case, case["u"])
    f_scan, want = run_pair(want_m, case)
    plain_cls = ScanPairsFloat64Matrix if case["family"] == "linear" else FamilyPairsFloat64Matrix
    _, plain = run_pair(oracle_for(case, case["u"], plain_cls), case, f_scan=f_scan)
    L, J = len(case["coeff"]), 1 + spec[6]
    assert want.shape == (spec[7], L, J, J)
    assert np.all(np.isfinite(f_scan)) and np.all(np.isfinite(want))
    assert np.all(want > 1e-280)
    np.testing.assert_allclose(plain, want, rtol=1e-11, atol=0)
    # what ties the block to pass B: row 0 of every reference member is that member's refcol, its own block its within
    r0 = int(case["rows"][0])
    _, within, refcol, _ = want_m.scan_gram_w(case["f"], case["coeff"], case["offset"], f_scan, reference=r0,
                                              **({} if case["center"] is None else dict(center_lb=case["center"])))
    np.testing.assert_allclose(want[0, :, 0, :], refcol, rtol=1e-13, atol=0)
    np.testing.assert_allclose(want[0, r0], within[r0], rtol=1e-13, atol=0)
