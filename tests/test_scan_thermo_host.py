"""Entropy, enthalpy and heat capacity along a scan (``MBAR.compute_scan_entropy_and_enthalpy``), host logic on the CPU stand-in
(tests/scan_thermo_standin.py): the reference's own numbers (tests/golden/scan_thermo_ho_K5.npz from make_golden_scan_thermo.py), the
dense augmented ``Theta`` of this project's ``compute_entropy_and_enthalpy(u_kn=u_ln)``, the gauge of the offsets, a member with a
sampled state's parameters, "approximate", the bootstrap plumbing and the error paths.

Tolerances.  A quantity with a twin in tests/test_scan_host.py takes that test's tolerance for the same comparison (``f`` /
``Delta_f``; ``u`` as a ``mu``; ``dDelta_u`` as a ``sigma``).  ``Delta_s = Delta_u - Delta_f`` is held to the sum of its parts'.
For ``var_u``, ``dvar_u`` and ``dDelta_s`` there is no twin: the bounds below are an order of magnitude above the worst gap seen
(profiles/scan_thermo_accuracy.txt), every test prints its gaps before it asserts."""
import numpy as np
import pytest

import pymbar_amd
from pymbar_amd import testsystems
from pymbar_amd.utils import DataError, ParameterError
from tests.conftest import load_golden
from tests.scan_thermo_standin import (ScanOnlyMatrix, ScanThermoOracleMatrix, FamilyThermoOracleMatrix,
                                       build_energy_case, energy_case_id, energy_cases, positive_center, run_energy_passes)

# ten times the worst gap seen, stand-in or device, either entry of the fixture (profiles/scan_thermo_accuracy.txt): against the
# fixture 7.4e-15 (var_u), 6.6e-15 (dvar_u), 1.4e-13 (dDelta_s) relative; against the dense path 4.6e-15 (var_u) and, on the stand-in,
# 7.2e-14 (dDelta_s)
FIXTURE_VAR_U = dict(rtol=8e-14, atol=0)
FIXTURE_DVAR_U = dict(rtol=7e-14, atol=0)
FIXTURE_DDELTA_S = dict(rtol=2e-12, atol=0)
DENSE_DDELTA_S = dict(rtol=8e-13, atol=0)
DENSE_VAR_U = dict(rtol=5e-14, atol=0)


def gap(name, got, want):
    got, want = np.asarray(got), np.asarray(want)
    a = np.max(np.abs(got - want))
    r = np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300))
    print("%-10s max abs gap %.3e  max rel gap %.3e" % (name, a, r))


@pytest.fixture
def standin(monkeypatch):
    import pymbar_amd.device

    monkeypatch.setattr(pymbar_amd.device, "DeviceMatrix", ScanThermoOracleMatrix)


@pytest.fixture(scope="module")
def gold():
    return load_golden("scan_thermo_ho_K5.npz")


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


def check_against_fixture(res, gold):
    """The assertions on the fixture, shared with the GPU test"""
    u0 = gold["pick_mu"][0, 0]  # (member 0 is the first of the picked members)
    assert gold["pick"][0] == 0
    u_ref = gold["Delta_u"] + u0
    var_ref = gold["mu_u2"] - u_ref * u_ref
    pick = gold["pick"]
    m1, C = gold["pick_mu"][:, 0], gold["pick_cov_obs"]
    dvar_ref = np.sqrt(4.0 * m1 * m1 * C[:, 0, 0] - 4.0 * m1 * C[:, 0, 1] + C[:, 1, 1])  # the delta method on the reference's covariance
    for name in ("Delta_f", "Delta_u", "Delta_s", "dDelta_f", "dDelta_u", "dDelta_s"):
        gap(name, res[name], gold[name])
    gap("u", res["u"], u_ref)
    gap("var_u", res["var_u"], var_ref)
    gap("var_u pick", res["var_u"][pick], gold["pick_mu"][:, 1] - m1 * m1)
    gap("dvar_u", res["dvar_u"][pick], dvar_ref)
    np.testing.assert_allclose(res["Delta_f"], gold["Delta_f"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(res["f"] - res["f"][0], gold["Delta_f"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(res["dDelta_f"], gold["dDelta_f"], rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(res["u"], u_ref, rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(res["Delta_u"], gold["Delta_u"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(res["dDelta_u"], gold["dDelta_u"], rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(res["Delta_s"], gold["Delta_s"], rtol=2e-9, atol=2e-9)
    np.testing.assert_allclose(res["s"], res["u"] - res["f"], rtol=0, atol=0)
    np.testing.assert_allclose(res["dDelta_s"], gold["dDelta_s"], **FIXTURE_DDELTA_S)
    np.testing.assert_allclose(res["var_u"], var_ref, **FIXTURE_VAR_U)
    np.testing.assert_allclose(res["dvar_u"][pick], dvar_ref, **FIXTURE_DVAR_U)


@pytest.fixture
def fixture_scan(standin, gold, config1):
    x_n, u_kn, N_k = config1
    mbar = pymbar_amd.MBAR(u_kn, N_k, relative_tolerance=1e-12)
    basis, coeff, offset = fixture_family(gold, x_n)
    return mbar, basis, coeff, offset


def test_method_reproduces_reference(fixture_scan, gold):
    mbar, basis, coeff, offset = fixture_scan
    res = mbar.compute_scan_entropy_and_enthalpy(basis, coeff, offset)
    assert set(res) == {"f", "Delta_f", "dDelta_f", "u", "Delta_u", "dDelta_u", "s", "Delta_s", "dDelta_s", "var_u", "dvar_u", "n_eff"}
    assert all(v.shape == (40,) for v in res.values())
    check_against_fixture(res, gold)
    assert np.all(res["n_eff"] > 1.0) and np.all(res["n_eff"] <= mbar.N)
    plain = mbar.compute_scan_entropy_and_enthalpy(basis, coeff, offset, fluctuation=False, compute_uncertainty=False)
    assert set(plain) == {"f", "Delta_f", "u", "Delta_u", "s", "Delta_s"}
    np.testing.assert_allclose(plain["u"], res["u"], rtol=1e-12, atol=1e-12)
    nofl = mbar.compute_scan_entropy_and_enthalpy(basis, coeff, offset, fluctuation=False)
    assert "var_u" not in nofl and "dvar_u" not in nofl
    for name in ("dDelta_f", "dDelta_u", "dDelta_s"):
        np.testing.assert_allclose(nofl[name], res[name], rtol=1e-9, atol=1e-12)
    other = mbar.compute_scan_entropy_and_enthalpy(basis, coeff, offset, reference=17)
    np.testing.assert_allclose(other["Delta_u"], gold["Delta_u"] - gold["Delta_u"][17], rtol=1e-9, atol=1e-9)
    for name in ("dDelta_f", "dDelta_u", "dDelta_s"):
        assert other[name][17] == 0.0 and other[name][0] == pytest.approx(res[name][17], rel=1e-9)
    # the scan's free energies are those of compute_scan (on the device: to the bit, tests/test_gpu_scan_thermo.py)
    scan = mbar.compute_scan(basis, coeff, offset)
    np.testing.assert_allclose(scan["f"], res["f"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(scan["dDelta_f"], res["dDelta_f"], rtol=1e-9, atol=1e-12)


def check_against_dense(mbar, basis, coeff, offset, reference, method=None, dtol=dict(rtol=0, atol=1e-12), stol=DENSE_DDELTA_S):
    """The method against row ``reference`` of this project's dense ``compute_entropy_and_enthalpy(u_kn=u_ln)`` (shared with the
    GPU test, which brings the device's tolerances of the uncertainties: ``dtol`` of those with a twin, ``stol`` of dDelta_s)"""
    res = mbar.compute_scan_entropy_and_enthalpy(basis, coeff, offset, reference=reference, uncertainty_method=method)
    u_ln = coeff @ basis + offset[:, None]
    dense = mbar.compute_entropy_and_enthalpy(u_kn=u_ln, uncertainty_method=method)
    sq = mbar.compute_expectations(u_ln ** 2, u_kn=u_ln, state_dependent=True, uncertainty_method=method)
    first = mbar.compute_expectations(u_ln, u_kn=u_ln, state_dependent=True, uncertainty_method=method)
    var_dense = sq["mu"] - first["mu"] ** 2
    for name in ("Delta_f", "Delta_u", "Delta_s", "dDelta_f", "dDelta_u", "dDelta_s"):
        gap(name, res[name], dense[name][reference])
    gap("u", res["u"], first["mu"])
    gap("var_u", res["var_u"], var_dense)
    np.testing.assert_allclose(res["Delta_f"], dense["Delta_f"][reference], rtol=0, atol=2e-11)
    np.testing.assert_allclose(res["dDelta_f"], dense["dDelta_f"][reference], **dtol)
    np.testing.assert_allclose(res["u"], first["mu"], rtol=1e-10, atol=1e-11)
    np.testing.assert_allclose(res["Delta_u"], dense["Delta_u"][reference], rtol=1e-10, atol=2e-11)
    np.testing.assert_allclose(res["dDelta_u"], dense["dDelta_u"][reference], **dtol)
    np.testing.assert_allclose(res["Delta_s"], dense["Delta_s"][reference], rtol=1e-10, atol=4e-11)
    np.testing.assert_allclose(res["dDelta_s"], dense["dDelta_s"][reference], **stol)
    np.testing.assert_allclose(res["var_u"], var_dense, **DENSE_VAR_U)
    return res


def test_bordered_equals_dense_theta(fixture_scan):
    mbar, basis, coeff, offset = fixture_scan
    check_against_dense(mbar, basis, coeff, offset, reference=3)


def test_bordered_equals_dense_theta_with_an_unsampled_state(standin):
    g = load_golden("ho_unsampled_K4_N2300.npz")
    assert np.any(g["N_k"] == 0)
    mbar = pymbar_amd.MBAR(g["u_kn"], g["N_k"], relative_tolerance=1e-12)
    rng = np.random.default_rng(3)
    basis = g["u_kn"][[0, 1, 3]]
    coeff = rng.dirichlet(np.ones(3), size=9)
    offset = rng.normal(0.0, 0.5, 9)
    check_against_dense(mbar, basis, coeff, offset, reference=0)


def test_approximate_is_the_members_block(fixture_scan):
    mbar, basis, coeff, offset = fixture_scan
    pick = np.arange(2, 40, 5)
    check_against_dense(mbar, basis, coeff[pick], offset[pick], reference=1, method="approximate", dtol=dict(rtol=1e-9, atol=1e-12))


def test_a_constant_in_every_offset_moves_u_and_f_alone(fixture_scan):
    mbar, basis, coeff, offset = fixture_scan
    res = mbar.compute_scan_entropy_and_enthalpy(basis, coeff, offset)
    for shift in (37.5, -1.0e3):
        moved = mbar.compute_scan_entropy_and_enthalpy(basis, coeff, offset + shift)
        for name in ("f", "u"):
            np.testing.assert_allclose(moved[name], res[name] + shift, rtol=0, atol=1e-12 * abs(shift) + 1e-11)
        for name in sorted(set(res) - {"f", "u"}):
            gap(name, moved[name], res[name])
        np.testing.assert_allclose(moved["s"], res["s"], rtol=0, atol=1e-12 * abs(shift) + 1e-11)
        for name in ("Delta_f", "Delta_u", "Delta_s"):
            np.testing.assert_allclose(moved[name], res[name], rtol=0, atol=1e-12 * abs(shift) + 1e-11)
        # the centred moments see the shift only through the rounding of u_l(n) - c_l: |shift| eps per sample
        np.testing.assert_allclose(moved["var_u"], res["var_u"], rtol=1e-12 * abs(shift) + 1e-11, atol=0)
        for name in ("dDelta_f", "dDelta_u", "dDelta_s", "dvar_u", "n_eff"):
            np.testing.assert_allclose(moved[name], res[name], rtol=1e-11 * abs(shift) + 1e-9, atol=1e-12)


def test_a_member_with_a_sampled_states_parameters_is_that_state(standin, config1):
    x_n, u_kn, N_k = config1
    _, _, _, _, O_k, K_k = testsystems.config1(seed=0)
    basis, coeff, offset = testsystems.harmonic_scan_family(x_n, O_k, K_k)
    mbar = pymbar_amd.MBAR(u_kn, N_k, relative_tolerance=1e-12)
    res = mbar.compute_scan_entropy_and_enthalpy(basis, coeff, offset, reference=2)
    own = mbar.compute_entropy_and_enthalpy()
    for name in ("Delta_f", "Delta_u", "Delta_s", "dDelta_f", "dDelta_u", "dDelta_s"):
        gap(name, res[name], own[name][2])
    # (the family's rows are the sampled rows up to the rounding of coeff @ basis + offset: 1e-12 on u of order 10)
    for name in ("Delta_f", "Delta_u", "Delta_s"):
        np.testing.assert_allclose(res[name], own[name][2], rtol=0, atol=1e-10)
    for name in ("dDelta_f", "dDelta_u", "dDelta_s"):
        np.testing.assert_allclose(res[name], own[name][2], rtol=1e-8, atol=1e-12)


def test_bootstrap_plumbing(standin, gold, config1):
    x_n, u_kn, N_k = config1
    mbar = pymbar_amd.MBAR(u_kn, N_k, n_bootstraps=3, rseed=7)
    basis, coeff, offset = fixture_family(gold, x_n)
    pick = np.array([0, 17, 25, 39])
    res = mbar.compute_scan_entropy_and_enthalpy(basis, coeff[pick], offset[pick], reference=1, uncertainty_method="bootstrap")
    for name in ("bootstrapped_f", "bootstrapped_u", "bootstrapped_var_u"):
        assert res[name].shape == (3, 4), name
    assert "n_eff" not in res
    u_ln = coeff[pick] @ basis + offset[pick][:, None]
    state_map = np.vstack([np.arange(4), np.arange(4)])
    inner = mbar.compute_expectations_inner(u_ln, u_ln, state_map, uncertainty_method="bootstrap")
    np.testing.assert_allclose(res["bootstrapped_f"], inner["bootstrapped_f"], rtol=0, atol=1e-11)
    np.testing.assert_allclose(res["bootstrapped_u"], inner["bootstrapped_observables"], rtol=1e-10, atol=1e-11)
    fb, ub = res["bootstrapped_f"], res["bootstrapped_u"]
    for name, arr in (("dDelta_f", fb), ("dDelta_u", ub), ("dDelta_s", ub - fb)):
        np.testing.assert_allclose(res[name], np.std(arr - arr[:, 1:2], axis=0), rtol=0, atol=0)
        assert res[name][1] == 0.0 and np.all(np.delete(res[name], 1) > 0.0)
    np.testing.assert_allclose(res["dvar_u"], np.std(res["bootstrapped_var_u"], axis=0), rtol=0, atol=0)
    assert np.all(res["bootstrapped_var_u"] > 0.0)
    assert mbar._dm._counts is None and mbar._dm.u.shape == u_kn.shape and mbar._dm._scan is None


def test_error_paths(fixture_scan):
    mbar, basis, coeff, offset = fixture_scan
    coeff, offset = coeff[:6], offset[:6]
    call = mbar.compute_scan_entropy_and_enthalpy
    with pytest.raises(ParameterError):
        call(basis, coeff, offset, uncertainty_method="svd")
    with pytest.raises(ParameterError):
        call(basis, coeff, offset, uncertainty_method="nonsense")
    with pytest.raises(ParameterError, match="without any bootstraps"):
        call(basis, coeff, offset, uncertainty_method="bootstrap")
    with pytest.raises(ParameterError):
        call(None, coeff, offset)  # (an object built from a dense u_kn has no basis of its own)
    with pytest.raises(ParameterError):
        call(basis, None, offset)
    with pytest.raises(ParameterError):
        call(basis[:, :-1], coeff, offset)
    with pytest.raises(ParameterError):
        call(np.vstack([basis] * 5)[:9], np.ones((6, 9)), offset)  # B = 9
    with pytest.raises(ParameterError):
        call(basis, coeff[:, :1], offset)
    with pytest.raises(ParameterError):
        call(basis, coeff[:0], offset[:0])
    with pytest.raises(ParameterError):
        call(basis, coeff, offset[:-1])
    with pytest.raises(ParameterError):
        call(basis, coeff, offset, reference=6)
    with pytest.raises(ParameterError):
        call(basis, coeff, offset, reference=-1)
    with pytest.raises(ParameterError):
        call(basis, coeff, offset, harmonic_b=[True, False])  # a harmonic term without centres
    for bad in (np.nan, np.inf):
        poisoned = basis.copy()
        poisoned[1, 3] = bad
        with pytest.raises(DataError):
            call(poisoned, coeff, offset)
        poisoned = coeff.copy()
        poisoned[2, 0] = bad
        with pytest.raises(DataError):
            call(basis, poisoned, offset)
    assert mbar._dm._scan is None  # nothing is left on the matrix after a refused call
    dm = mbar._dm
    dm.set_scan(basis)
    with pytest.raises(ValueError):
        dm.scan_energy_lognum(mbar.f_k, coeff, offset, J=4)
    with pytest.raises(ValueError):
        dm.scan_energy_lognum(mbar.f_k, coeff, offset, center_u=np.zeros(5))
    dm.set_scan(None)


@pytest.mark.parametrize("cls", ["no passes", "scan passes only"])
def test_handles_without_the_passes_are_refused(monkeypatch, config1, cls):
    import pymbar_amd.device
    from tests.cpu_standin import OracleMatrix

    monkeypatch.setattr(pymbar_amd.device, "DeviceMatrix", OracleMatrix if cls == "no passes" else ScanOnlyMatrix)
    x_n, u_kn, N_k = config1
    mbar = pymbar_amd.MBAR(u_kn, N_k)
    with pytest.raises(ParameterError, match="not supported on this backend"):
        mbar.compute_scan_entropy_and_enthalpy(np.stack([x_n * x_n, x_n]), np.ones((2, 2)))


@pytest.mark.parametrize("case", energy_cases(), ids=energy_case_id)
def test_energy_cases_suit_the_standin(case):
    """The cases tests/test_gpu_scan_thermo.py holds the device to (rtol 1e-10 with atol 0 on the products, 1e-11 absolute on lognum
    and wsum) are cases at which the long-double stand-in is a reference: with the positive centre everything is finite, the weights
    are normalised, no entry of a product is zero or negative (so a relative bound alone means something), and the same formulas in
    plain float64 give the same numbers to 1e-11 relative -- a factor 10 under the device's bound: u_l(n) - c_l is formed from a u of
    up to 2e3 (the far member), whose float64 rounding of 2e-13 stands against a t_1 of 1e-3 at the member's lowest sample."""
    c = build_energy_case(case)
    fam, K, J = case
    out = []
    for real in (np.longdouble, np.float64):
        cls = type("M", (FamilyThermoOracleMatrix if fam == "harmonic" else ScanThermoOracleMatrix,), dict(real=real))
        m = cls(c["u"])
        m.set_Nk(c["N_k"])
        m.set_sample_weights(c["c"])
        m.set_scan(c["basis"], None, **c["kinds"])
        out.append(run_energy_passes(m, c, positive_center(c)))
    want, plain = out
    for name, v in want.items():
        assert np.all(np.isfinite(v)), name
    np.testing.assert_allclose(want["wsum"], 1.0, rtol=0, atol=1e-13)
    for name in ("cross", "within", "refblock", "mean"):
        assert np.all(want[name] > 0.0), name
    np.testing.assert_allclose(plain["lognum"], want["lognum"], rtol=0, atol=1e-12)
    for name in ("mean", "cross", "within", "refblock", "wsum"):
        gap(name, plain[name], want[name])
        np.testing.assert_allclose(plain[name], want[name], rtol=1e-11, atol=0)


def test_temperature_ladder_family_gives_the_heat_capacity(standin):
    """Four harmonic oscillators sampled at beta = 1 .. 2.5 and scanned over beta: E = x^2 / 2 has <E> = 1 / (2 beta), so u = beta <E> =
    1 / 2 and var_u = C_v / k_B = 1 / 2 at every temperature."""
    rng = np.random.default_rng(12)
    beta_k = np.array([1.0, 1.5, 2.0, 2.5])
    N_k = np.full(4, 4000)
    x_n = np.concatenate([rng.normal(0.0, 1.0 / np.sqrt(b), n) for b, n in zip(beta_k, N_k)])
    E_n = 0.5 * x_n * x_n
    basis, coeff, offset = testsystems.temperature_ladder_family(E_n, np.linspace(1.1, 2.4, 14))
    assert basis.shape == (1, 16000) and coeff.shape == (14, 1) and not offset.any()
    mbar = pymbar_amd.MBAR(beta_k[:, None] * E_n[None, :], N_k)
    res = mbar.compute_scan_entropy_and_enthalpy(basis, coeff, offset)
    assert np.all(np.abs(res["u"] - 0.5) < 5.0 * np.hypot(res["dDelta_u"], 0.01))
    assert np.all(np.abs(res["var_u"] - 0.5) < 5.0 * res["dvar_u"]) and np.all(res["dvar_u"] < 0.05)
    with pytest.raises(ValueError):
        testsystems.temperature_ladder_family(basis, [1.0])


# ---- a sweep of a restraint centre across the +-180 degree seam (the system of periodic_umbrella_K6.npz) --------------------------

def seam_family():
    """The fixture's umbrellas as a family and its 40 unsampled centres (120 .. 240 degrees) as members"""
    g = load_golden("periodic_umbrella_K6.npz")
    basis, coeff, center, harmonic, period, offset, N_k = testsystems.periodic_umbrella_family(K=6, n_per_state=300, seed=0)
    assert np.array_equal(basis[1], g["chi_n"]) and np.array_equal(N_k, g["N_k"])
    L = len(g["chi0_l"])
    members = dict(coeff_lb=np.tile([1.0, 0.5 * g["spring_k"][0]], (L, 1)), center_lb=np.stack([np.zeros(L), g["chi0_l"]], axis=1))
    return dict(basis=basis, coeff=coeff, center=center, harmonic=harmonic, period=period, offset=offset, N_k=N_k), members


def check_against_seam_fixture(res, gold):
    """The assertions on the seam entry, shared with the GPU test: the tolerances of ``check_against_fixture``"""
    var_ref = gold["seam_mu_u2"] - gold["seam_mu_u"] ** 2
    for name in ("Delta_f", "Delta_u", "Delta_s", "dDelta_f", "dDelta_u", "dDelta_s"):
        gap("seam " + name, res[name], gold["seam_" + name])
    gap("seam u", res["u"], gold["seam_mu_u"])
    gap("seam var_u", res["var_u"], var_ref)
    np.testing.assert_allclose(res["Delta_f"], gold["seam_Delta_f"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(res["dDelta_f"], gold["seam_dDelta_f"], rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(res["u"], gold["seam_mu_u"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(res["Delta_u"], gold["seam_Delta_u"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(res["dDelta_u"], gold["seam_dDelta_u"], rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(res["Delta_s"], gold["seam_Delta_s"], rtol=2e-9, atol=2e-9)
    np.testing.assert_allclose(res["dDelta_s"], gold["seam_dDelta_s"], **FIXTURE_DDELTA_S)
    np.testing.assert_allclose(res["var_u"], var_ref, **FIXTURE_VAR_U)
    assert np.all(np.isfinite(res["dvar_u"])) and np.all(res["dvar_u"] > 0.0)


def test_sweep_across_the_seam_reproduces_reference(monkeypatch, gold):
    import pymbar_amd.device

    monkeypatch.setattr(pymbar_amd.device, "DeviceMatrix", FamilyThermoOracleMatrix)
    fam, members = seam_family()
    m = pymbar_amd.MBAR.from_family(fam["basis"], fam["coeff"], fam["N_k"], offset_k=fam["offset"], center_kb=fam["center"],
                                    harmonic_b=fam["harmonic"], period_b=fam["period"], relative_tolerance=1e-12)
    res = m.compute_scan_entropy_and_enthalpy(**members)  # basis and kinds: the constructor's
    check_against_seam_fixture(res, gold)
    explicit = m.compute_scan_entropy_and_enthalpy(fam["basis"], harmonic_b=fam["harmonic"], period_b=fam["period"], **members)
    for key in res:
        assert explicit[key].tobytes() == res[key].tobytes(), key
    with pytest.raises(ParameterError):
        m.compute_scan_entropy_and_enthalpy(coeff_lb=members["coeff_lb"])  # a harmonic term without centres
