"""Families with harmonic terms on the CPU stand-in (tests/family_standin.py): ``MBAR.from_family`` is the dense constructor on the
matrix the fill kernel is specified to write; ``compute_scan`` / ``compute_scan_fes`` with periodic members are the dense paths on
the dense ``u_ln``; the reference's own numbers (tests/golden/periodic_umbrella_K6.npz from make_golden_periodic_umbrella.py);
every validation error; the minimum image of the chain."""
import numpy as np
import pytest

import pymbar_amd
import pymbar_amd.device
from pymbar_amd import fes
from pymbar_amd import testsystems as ts
from pymbar_amd.utils import DataError, ParameterError
from tests.conftest import load_golden
from tests.family_standin import (PASS_SHAPES, FamilyOracleMatrix, build_family_case, family_case_id, family_instantiation_cases,
                                  load_family_case, run_family_passes, u_model_family)
from tests.scan_fes_standin import check_row_against_label_path
from tests.scan_standin import ScanOracleMatrix


@pytest.fixture(autouse=True)
def standin(monkeypatch):
    monkeypatch.setattr(pymbar_amd.device, "DeviceMatrix", FamilyOracleMatrix)


@pytest.fixture(scope="module")
def gold():
    return load_golden("periodic_umbrella_K6.npz")


@pytest.fixture(scope="module")
def umbrella(gold):
    """The fixture's system as a family: the samples are regenerated and asserted equal to the stored ones."""
    basis, coeff, center, harmonic, period, offset, N_k = ts.periodic_umbrella_family(K=6, n_per_state=300, seed=0)
    assert np.array_equal(basis[1], gold["chi_n"]) and np.array_equal(basis[0], gold["E_n"]) and np.array_equal(N_k, gold["N_k"])
    assert np.array_equal(center[:, 1], gold["chi0_k"]) and np.array_equal(coeff[:, 0], gold["beta_k"])
    u = u_model_family(basis, coeff, offset, center, harmonic, period)
    u.setflags(write=False)
    return dict(basis=basis, coeff=coeff, center=center, harmonic=harmonic, period=period, offset=offset, N_k=N_k, u_model=u)


def scan_members(gold, umbrella):
    """The fixture's 40 unsampled centres (120 .. 240 degrees: those above 180 lie outside the period) as members"""
    L = len(gold["chi0_l"])
    coeff = np.tile([1.0, 0.5 * gold["spring_k"][0]], (L, 1))
    center = np.stack([np.zeros(L), gold["chi0_l"]], axis=1)
    return coeff, center


def from_family(umbrella, **kw):
    return pymbar_amd.MBAR.from_family(umbrella["basis"], umbrella["coeff"], umbrella["N_k"], offset_k=umbrella["offset"],
                                       center_kb=umbrella["center"], harmonic_b=umbrella["harmonic"], period_b=umbrella["period"], **kw)


# ---- the chain -------------------------------------------------------------------------------------------------------------------
def test_wrap_model_is_the_minimum_image():
    """``(d - P rint(d / P))^2 = min(|d|, P - |d|)^2`` for ``|d| <= P``, the ties ``d = +-P / 2`` and the ends ``d = +-P`` included"""
    P = 360.0
    d = np.concatenate([np.linspace(-P, P, 2881), [0.0, 0.5 * P, -0.5 * P, P, -P, np.nextafter(0.5 * P, 0), np.nextafter(0.5 * P, P),
                                                    np.nextafter(-0.5 * P, 0), np.nextafter(-0.5 * P, -P)]])
    u = u_model_family(d[None, :], np.ones((1, 1)), None, np.zeros((1, 1)), [True], [P])[0]
    want = np.minimum(np.abs(d), P - np.abs(d)) ** 2
    np.testing.assert_allclose(u, want, rtol=4e-16, atol=1e-25)
    assert u[d == 0.5 * P][0] == u[d == -0.5 * P][0] == (0.5 * P) ** 2 and np.all(u[np.abs(d) == P] == 0.0)
    # a period of 0 is the plain harmonic term; the dense numpy statement says the same
    plain = u_model_family(d[None, :], np.ones((1, 1)), None, np.full((1, 1), 3.0), [True], [0.0])[0]
    assert np.array_equal(plain, (d - 3.0) ** 2)
    np.testing.assert_allclose(ts.family_u_kn(d[None, :], np.ones((1, 1)), None, np.zeros((1, 1)), [True], [P])[0], want, rtol=4e-16, atol=1e-25)


def test_model_without_harmonic_terms_is_the_linear_model(umbrella):
    from tests.device_math_model import fma
    from tests.family_standin import u_model

    a = u_model_family(umbrella["basis"], umbrella["coeff"], umbrella["offset"])
    assert np.array_equal(a, u_model(umbrella["basis"], umbrella["coeff"], umbrella["offset"]))
    chain = np.repeat(umbrella["offset"][:, None], umbrella["basis"].shape[1], axis=1)  # (the linear chain written out: one fma per term)
    for b in range(umbrella["basis"].shape[0]):
        chain = fma(umbrella["coeff"][:, b:b + 1], umbrella["basis"][b][None, :], chain)
    assert np.array_equal(a, chain)
    assert np.array_equal(a, u_model_family(umbrella["basis"], umbrella["coeff"], umbrella["offset"], umbrella["center"], [False, False], [0.0, 360.0]))


def test_testsystem_is_umbrella_sampling_across_the_seam(umbrella, gold):
    chi = umbrella["basis"][1]
    assert umbrella["basis"].shape == (2, 1800) and np.all(np.abs(chi) <= 180.0)
    last = chi[-300:]  # the umbrella centred at 150: samples on both sides of +-180
    assert np.any(last > 150.0) and np.any(last < -150.0)
    # the dense statement is the matrix the reference was given, up to the rounding of two formulas for the same number
    d = np.abs(chi[None, :] - gold["chi0_k"][:, None])
    d = np.where(d > 180.0, 360.0 - d, d)
    dense = gold["beta_k"][:, None] * (gold["E_n"][None, :] + 0.5 * gold["spring_k"][:, None] * d * d)
    fam = ts.family_u_kn(umbrella["basis"], umbrella["coeff"], umbrella["offset"], umbrella["center"], umbrella["harmonic"], umbrella["period"])
    np.testing.assert_allclose(fam, dense, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(umbrella["u_model"], dense, rtol=1e-13, atol=1e-13)


# ---- the constructor -------------------------------------------------------------------------------------------------------------
def test_from_family_is_the_dense_constructor(umbrella, gold):
    m = from_family(umbrella, relative_tolerance=1e-12)
    d = pymbar_amd.MBAR(umbrella["u_model"], umbrella["N_k"], relative_tolerance=1e-12)
    assert np.array_equal(m.f_k, d.f_k)
    for method in (None, "svd", "approximate"):
        rm, rd = m.compute_free_energy_differences(uncertainty_method=method), d.compute_free_energy_differences(uncertainty_method=method)
        assert np.array_equal(rm["Delta_f"], rd["Delta_f"]) and np.array_equal(rm["dDelta_f"], rd["dDelta_f"]), method
    # the dense numpy statement of the family gives the same object up to its own rounding
    n = pymbar_amd.MBAR(ts.family_u_kn(umbrella["basis"], umbrella["coeff"], umbrella["offset"], umbrella["center"], umbrella["harmonic"],
                                       umbrella["period"]), umbrella["N_k"], relative_tolerance=1e-12)
    np.testing.assert_allclose(m.f_k, n.f_k, rtol=0, atol=1e-10)
    # the reference's numbers
    np.testing.assert_allclose(m.f_k, gold["f_k"], rtol=0, atol=1e-9)
    r = m.compute_free_energy_differences()
    np.testing.assert_allclose(r["Delta_f"], gold["Delta_f"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(r["dDelta_f"], gold["dDelta_f"], rtol=1e-7, atol=1e-9)
    # what the object keeps
    for name, want in (("center_kb", umbrella["center"]), ("harmonic_b", umbrella["harmonic"]), ("period_b", umbrella["period"]),
                       ("basis_bn", umbrella["basis"]), ("coeff_kb", umbrella["coeff"])):
        got = getattr(m, name)
        assert np.array_equal(got, want) and got is not want and not got.flags.writeable, name
    assert d.center_kb is None and d.harmonic_b is None and d.period_b is None
    lin = pymbar_amd.MBAR.from_linear(umbrella["basis"], umbrella["coeff"], umbrella["N_k"])
    assert lin.center_kb is None and lin.harmonic_b is None and lin.period_b is None


def test_u_kn_is_lazy(umbrella):
    m = from_family(umbrella)
    m.compute_free_energy_differences()
    assert m._u_kn is None
    assert np.array_equal(m.u_kn, umbrella["u_model"]) and m._u_kn is m.u_kn


def test_without_harmonic_terms_it_is_from_linear(umbrella):
    a = pymbar_amd.MBAR.from_family(umbrella["basis"], umbrella["coeff"], umbrella["N_k"], harmonic_b=np.zeros(2, dtype=bool))
    b = pymbar_amd.MBAR.from_linear(umbrella["basis"], umbrella["coeff"], umbrella["N_k"])
    assert np.array_equal(a.f_k, b.f_k) and a.harmonic_b is None and a.center_kb is None


def test_constructor_errors_come_before_any_device_matrix(umbrella):
    b, c, N_k, cen, hb, pb = (umbrella[k] for k in ("basis", "coeff", "N_k", "center", "harmonic", "period"))
    five = np.tile(b[1:], (5, 1))
    nan_cen = cen.copy()
    nan_cen[2, 1] = np.nan
    cases = [
        (ParameterError, (b, c, N_k), dict(center_kb=cen, harmonic_b=hb, period_b=pb, copy=False)),
        (ParameterError, (five, np.ones((6, 5)), N_k), dict(center_kb=np.zeros((6, 5)), harmonic_b=np.ones(5, dtype=bool))),  # 5 harmonic terms
        (ParameterError, (b, c, N_k), dict(center_kb=cen, harmonic_b=hb, period_b=[0.0, -360.0])),                              # negative period
        (ParameterError, (b, c, N_k), dict(center_kb=cen, harmonic_b=hb, period_b=[0.0, np.inf])),
        (ParameterError, (b, c, N_k), dict(harmonic_b=hb, period_b=pb)),                                                        # centres missing
        (ParameterError, (b, c, N_k), dict(center_kb=cen[:5], harmonic_b=hb, period_b=pb)),                                     # wrong K
        (ParameterError, (b, c, N_k), dict(center_kb=cen, harmonic_b=[0, 1], period_b=pb)),                                     # not a bool mask
        (ParameterError, (b, c, N_k), dict(center_kb=cen, harmonic_b=hb[:1], period_b=pb)),
        (ParameterError, (b, c, N_k), dict(period_b=pb)),                                                                        # a period without a harmonic term
        (DataError, (b, c, N_k), dict(center_kb=nan_cen, harmonic_b=hb, period_b=pb)),
    ]
    FamilyOracleMatrix.created = 0
    for exc, args, kwargs in cases:
        with pytest.raises(exc):
            pymbar_amd.MBAR.from_family(*args, **kwargs)
    assert FamilyOracleMatrix.created == 0


# ---- the scans -------------------------------------------------------------------------------------------------------------------
def test_compute_scan_is_the_dense_path_and_the_reference(umbrella, gold):
    m = from_family(umbrella, relative_tolerance=1e-12, n_bootstraps=3, rseed=5)
    coeff, center = scan_members(gold, umbrella)
    res = m.compute_scan(coeff_lb=coeff, center_lb=center)  # basis and kinds: the constructor's
    assert res["f"].shape == (40,)
    # the reference (tolerances of tests/test_scan_host.py::check_against_fixture)
    np.testing.assert_allclose(res["Delta_f"], gold["pert_Delta_f"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(res["dDelta_f"], gold["pert_dDelta_f"], rtol=1e-7, atol=1e-9)
    # the dense path of this package on the dense u_ln
    u_ln = u_model_family(umbrella["basis"], coeff, None, center, umbrella["harmonic"], umbrella["period"])
    dense = m.compute_perturbed_free_energies(u_ln)
    np.testing.assert_allclose(res["Delta_f"], dense["Delta_f"][0], rtol=0, atol=1e-11)
    np.testing.assert_allclose(res["dDelta_f"], dense["dDelta_f"][0], rtol=1e-7, atol=1e-9)
    for method in ("approximate", "bootstrap"):
        a = m.compute_scan(umbrella["basis"], coeff, center_lb=center, harmonic_b=umbrella["harmonic"], period_b=umbrella["period"],
                           uncertainty_method=method)
        np.testing.assert_allclose(a["dDelta_f"], m.compute_perturbed_free_energies(u_ln, uncertainty_method=method)["dDelta_f"][0 if method == "approximate" else slice(None)],
                                   rtol=1e-9, atol=1e-12)
    # an observable along the scan
    A = np.cos(np.deg2rad(umbrella["basis"][1]))
    ob = m.compute_scan(coeff_lb=coeff[:7], center_lb=center[:7], A_qn=A)
    ex = m.compute_expectations(A, u_kn=u_ln[:7], state_dependent=False)
    np.testing.assert_allclose(ob["mu"][0], ex["mu"], rtol=1e-10, atol=1e-11)
    np.testing.assert_allclose(ob["sigma"][0], ex["sigma"], rtol=1e-7, atol=1e-9)
    assert m._dm._scan is None and m._dm._kinds is None


def test_a_member_with_a_sampled_states_parameters_is_that_state(umbrella):
    m = from_family(umbrella, relative_tolerance=1e-12)
    res = m.compute_scan(coeff_lb=umbrella["coeff"], offset_l=umbrella["offset"], center_lb=umbrella["center"])
    np.testing.assert_allclose(res["f"], m.f_k, rtol=0, atol=1e-11)


def test_compute_scan_fes_is_the_label_path_and_the_reference(umbrella, gold):
    m = from_family(umbrella, relative_tolerance=1e-12)
    coeff, center = scan_members(gold, umbrella)
    pick = gold["surface_members"]
    coeff = np.vstack([[1.0, 0.0], coeff[pick]])  # the unbiased potential (a harmonic term of coefficient 0), then three centres
    center = np.vstack([[0.0, 0.0], center[pick]])
    label = np.digitize(umbrella["basis"][1], gold["bin_edges"]) - 1  # (bins in grid order, as the fixture stores them)
    res = m.compute_scan_fes(coeff_lb=coeff, center_lb=center, sample_label=label, uncertainty_method="analytical")
    assert res["f_raw"].shape == (4, 30)
    np.testing.assert_allclose(res["f_i"], gold["fes_f_i"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(res["df_i"], gold["fes_df_i"], rtol=1e-7, atol=1e-7)
    np.testing.assert_allclose(res["f_raw"] - res["f_raw"][:, :1], gold["fes_f_raw"] - gold["fes_f_raw"][:, :1], rtol=1e-9, atol=1e-9)
    u_ln = u_model_family(umbrella["basis"], coeff, None, center, umbrella["harmonic"], umbrella["period"])
    for l in range(4):
        check_row_against_label_path(res, l, fes.histogram_fes_labels(m, u_ln[l], label, uncertainty_method="analytical"))
    assert m._dm._scan is None and m._dm._scan_bins is None


def test_scan_errors(umbrella, gold):
    m = from_family(umbrella)
    coeff, center = scan_members(gold, umbrella)
    b, hb, pb = umbrella["basis"], umbrella["harmonic"], umbrella["period"]
    label = np.zeros(1800, dtype=np.int32)
    for call, extra in ((m.compute_scan, {}), (m.compute_scan_fes, dict(sample_label=label))):
        with pytest.raises(ParameterError, match="center_lb is required"):
            call(coeff_lb=coeff, **extra)                                                    # centres missing
        with pytest.raises(ParameterError, match="center_lb"):
            call(coeff_lb=coeff, center_lb=center[:39], **extra)                             # centres with the wrong L
        with pytest.raises(ParameterError, match="at most 4"):
            call(np.tile(b[1:], (5, 1)), np.ones((40, 5)), center_lb=np.zeros((40, 5)), harmonic_b=np.ones(5, dtype=bool), **extra)
        with pytest.raises(ParameterError, match="period"):
            call(b, coeff, center_lb=center, harmonic_b=hb, period_b=[0.0, -1.0], **extra)   # negative period
        bad = center.copy()
        bad[3, 1] = np.inf
        with pytest.raises(DataError):
            call(coeff_lb=coeff, center_lb=bad, **extra)
    # a basis passed explicitly is a linear family unless the kinds come with it
    lin = m.compute_scan(b, coeff)
    np.testing.assert_allclose(lin["f"], pymbar_amd.MBAR(umbrella["u_model"], umbrella["N_k"]).compute_scan(b, coeff)["f"], rtol=0, atol=1e-9)
    assert m._dm._scan is None


def test_handles_without_the_family_are_refused(monkeypatch, umbrella, gold):
    monkeypatch.setattr(pymbar_amd.device, "DeviceMatrix", ScanOracleMatrix)
    m = pymbar_amd.MBAR(umbrella["u_model"], umbrella["N_k"])
    coeff, center = scan_members(gold, umbrella)
    with pytest.raises(TypeError):  # (a handle whose set_scan knows no term kinds)
        m.compute_scan(umbrella["basis"], coeff, center_lb=center, harmonic_b=umbrella["harmonic"], period_b=umbrella["period"])


# ---- the cases of the GPU tests suit the stand-in -----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", PASS_SHAPES + family_instantiation_cases(), ids=family_case_id)
def test_cases_suit_the_standin(shape):
    """The cases tests/test_gpu_family.py holds the device to (rtol 1e-10 on the products, 1e-11 absolute on lognum and wsum) are
    cases at which the long-double stand-in is a reference: everything is finite, the weights are normalised, no entry of a
    product is zero or negative, and the same formulas in plain float64 agree to 1e-12 relative (lognum: 1e-12 absolute)."""
    case = build_family_case(shape)
    assert case["harmonic_b"].sum() == shape[4] and len(case["harmonic_b"]) == shape[3]
    out = []
    for real in (np.longdouble, np.float64):
        dm = FamilyOracleMatrix(case["u"])
        dm.real = real
        load_family_case(dm, case)
        out.append(run_family_passes(dm, case, ref=shape[2] - 1))
    want, plain = out
    for name, v in want.items():
        assert np.all(np.isfinite(v)), name
    np.testing.assert_allclose(want["wsum"], 1.0, rtol=0, atol=1e-13)
    for name in ("cross", "within", "refcol", "mean"):
        assert np.all(want[name] > 0.0), name
    np.testing.assert_allclose(plain["lognum"], want["lognum"], rtol=0, atol=1e-12)
    for name in ("mean", "cross", "within", "refcol", "wsum"):
        np.testing.assert_allclose(plain[name], want[name], rtol=1e-12, atol=0)
