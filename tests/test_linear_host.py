"""``MBAR.from_linear`` on the CPU stand-in: the object built from a basis is the object the dense constructor builds from the
matrix the fill kernel is specified to write (``u_model``: the scan passes' fma chain, exact), bit for bit; the host matrix stays
absent until something reads it; argument errors come before any device matrix."""
import logging

import numpy as np
import pytest

import pymbar_amd
import pymbar_amd.device
from pymbar_amd import testsystems as ts
from pymbar_amd.utils import DataError, ParameterError
from tests.family_standin import FamilyOracleMatrix, u_model


@pytest.fixture(autouse=True)
def standin(monkeypatch):
    monkeypatch.setattr(pymbar_amd.device, "DeviceMatrix", FamilyOracleMatrix)


@pytest.fixture(scope="module")
def family():
    """Config 1 (K = 5, N = 5000) as a linear family over [x^2, x], and the matrix the kernel is specified to write from it."""
    x_n, u_kn, N_k, s_n, O_k, K_k = ts.config1(seed=0)
    basis, coeff, offset = ts.harmonic_scan_family(x_n, O_k, K_k)
    u = u_model(basis, coeff, offset)
    u.setflags(write=False)
    return dict(x_n=x_n, u_kn=u_kn, N_k=N_k, basis=basis, coeff=coeff, offset=offset, u_model=u, O_k=O_k, K_k=K_k)


def test_testsystems_helper_is_the_config1_family(family):
    basis, coeff, offset = ts.harmonic_linear_family(family["O_k"], family["K_k"], family["N_k"], seed=0)
    assert np.array_equal(basis, family["basis"]) and np.array_equal(coeff, family["coeff"]) and np.array_equal(offset, family["offset"])
    assert np.array_equal(basis[1], family["x_n"]) and np.array_equal(basis[0], family["x_n"] ** 2)
    # the model matrix is the golden matrix up to the rounding of two formulas for the same number (|u| <= 397)
    assert np.max(np.abs(family["u_model"] - family["u_kn"])) < 1e-12


def test_config1_matches_the_dense_constructor_bit_for_bit(family, golden):
    g = golden("config1_ho_K5_N5000.npz")
    m = pymbar_amd.MBAR.from_linear(family["basis"], family["coeff"], family["N_k"], offset_k=family["offset"])
    d = pymbar_amd.MBAR(family["u_model"], family["N_k"])
    assert np.array_equal(m.f_k, d.f_k)
    np.testing.assert_allclose(m.f_k, g["f_k"], atol=1e-10)
    for method in (None, "svd", "approximate"):
        rm = m.compute_free_energy_differences(uncertainty_method=method)
        rd = d.compute_free_energy_differences(uncertainty_method=method)
        assert np.array_equal(rm["Delta_f"], rd["Delta_f"]), method
        assert np.array_equal(rm["dDelta_f"], rd["dDelta_f"]), method
    # what the object keeps: private read-only copies of the family; a dense object has none
    assert np.array_equal(m.basis_bn, family["basis"]) and m.basis_bn is not family["basis"] and not m.basis_bn.flags.writeable
    assert np.array_equal(m.coeff_kb, family["coeff"]) and np.array_equal(m.offset_k, family["offset"])
    assert d.basis_bn is None and d.coeff_kb is None and d.offset_k is None
    assert set(m.upload_stats) == {"upload_s", "upload_GBps"}
    assert m.upload_stats["upload_GBps"] == pytest.approx(8.0 * 2 * 5000 / m.upload_stats["upload_s"] * 1e-9)


def test_offset_none_is_zeros(family):
    m = pymbar_amd.MBAR.from_linear(family["basis"], family["coeff"], family["N_k"])
    d = pymbar_amd.MBAR(u_model(family["basis"], family["coeff"], np.zeros(5)), family["N_k"])
    assert np.array_equal(m.f_k, d.f_k) and np.array_equal(m.offset_k, np.zeros(5))


def test_u_kn_is_lazy(family):
    m = pymbar_amd.MBAR.from_linear(family["basis"], family["coeff"], family["N_k"], offset_k=family["offset"])
    m.compute_free_energy_differences()
    m.compute_overlap()
    assert m._u_kn is None  # no K x N host array so far
    u = m.u_kn
    assert np.array_equal(u, family["u_model"]) and u.shape == (5, 5000)
    assert m.u_kn is u and m._u_kn is u
    # a dense object keeps its matrix as before
    d = pymbar_amd.MBAR(family["u_model"], family["N_k"])
    assert d._u_kn is d.u_kn and np.array_equal(d.u_kn, family["u_model"])


@pytest.mark.parametrize("initialize", ["BAR", "mean-reduced-potential"])
def test_initial_guesses_that_read_the_matrix(family, initialize):
    m = pymbar_amd.MBAR.from_linear(family["basis"], family["coeff"], family["N_k"], offset_k=family["offset"], initialize=initialize)
    d = pymbar_amd.MBAR(family["u_model"], family["N_k"], initialize=initialize)
    assert np.array_equal(m.f_k, d.f_k)
    assert m._u_kn is not None  # (these two trigger the download)


@pytest.mark.parametrize("initialize", ["zeros", "BAR"])
def test_bootstraps_are_the_dense_constructors(family, initialize):
    kw = dict(n_bootstraps=3, rseed=7, initialize=initialize)
    m = pymbar_amd.MBAR.from_linear(family["basis"], family["coeff"], family["N_k"], offset_k=family["offset"], **kw)
    d = pymbar_amd.MBAR(family["u_model"], family["N_k"], **kw)
    assert np.array_equal(m.bootstrap_rints, d.bootstrap_rints)
    assert np.array_equal(m.f_k_boots, d.f_k_boots)
    assert (m._u_kn is None) == (initialize == "zeros")
    rm = m.compute_free_energy_differences(uncertainty_method="bootstrap")
    rd = d.compute_free_energy_differences(uncertainty_method="bootstrap")
    assert np.array_equal(rm["dDelta_f"], rd["dDelta_f"])


def test_expectations_are_the_dense_objects(family):
    m = pymbar_amd.MBAR.from_linear(family["basis"], family["coeff"], family["N_k"], offset_k=family["offset"])
    d = pymbar_amd.MBAR(family["u_model"], family["N_k"])
    rm, rd = m.compute_expectations(family["x_n"]), d.compute_expectations(family["x_n"])
    for key in ("mu", "sigma"):
        assert np.array_equal(rm[key], rd[key]), key
    rm, rd = m.compute_entropy_and_enthalpy(), d.compute_entropy_and_enthalpy()
    for key in ("Delta_f", "dDelta_f", "Delta_u", "dDelta_u", "Delta_s", "dDelta_s"):
        assert np.array_equal(rm[key], rd[key]), key


def test_argument_errors_come_before_any_device_matrix(family):
    basis, coeff, offset, N_k = family["basis"], family["coeff"], family["offset"], family["N_k"]
    bad = basis.copy()
    bad[1, 17] = np.nan
    infc = coeff.copy()
    infc[2, 0] = np.inf
    nano = offset.copy()
    nano[4] = np.nan
    cases = [
        (ParameterError, (basis, coeff, N_k), dict(offset_k=offset, copy=False)),
        (ParameterError, (basis, coeff, N_k), dict(offset_k=offset, copy=True)),
        (ParameterError, (basis[:0], coeff[:, :0], N_k), dict()),                                      # B = 0
        (ParameterError, (np.tile(basis[:1], (9, 1)), np.tile(coeff[:, :1], (1, 9)), N_k), dict()),    # B = 9
        (ParameterError, (basis, np.tile(coeff[:, :1], (1, 3)), N_k), dict()),                         # coeff_kb: wrong second dimension
        (ParameterError, (basis, coeff, N_k), dict(offset_k=offset[:4])),                              # offset_k: wrong length
        (ParameterError, (basis, coeff, N_k + 1), dict(offset_k=offset)),                              # sum(N_k) != N
        (ParameterError, (basis, coeff, N_k), dict(bootstrap_rng="nonsense")),
        (DataError, (bad, coeff, N_k), dict(offset_k=offset)),
        (DataError, (basis, infc, N_k), dict(offset_k=offset)),
        (DataError, (basis, coeff, N_k), dict(offset_k=nano)),
    ]
    FamilyOracleMatrix.created = 0
    for exc, args, kwargs in cases:
        with pytest.raises(exc):
            pymbar_amd.MBAR.from_linear(*args, **kwargs)
    assert FamilyOracleMatrix.created == 0
    with pytest.raises(TypeError):
        pymbar_amd.MBAR.from_linear(basis, coeff, N_k, no_such_keyword=1)
    # the constructor's own errors keep their meaning
    with pytest.raises(ParameterError):
        pymbar_amd.MBAR.from_linear(basis, coeff, N_k, offset_k=offset, initial_f_k=np.zeros(4))
    with pytest.raises(ParameterError):
        pymbar_amd.MBAR.from_linear(basis, coeff, N_k, offset_k=offset, initialize="nonsense")


def test_scan_without_a_basis_needs_a_linear_object(family):
    d = pymbar_amd.MBAR(family["u_model"], family["N_k"])
    with pytest.raises(ParameterError, match="from_linear"):
        d.compute_scan(None, family["coeff"], family["offset"])
    with pytest.raises(ParameterError, match="from_linear"):
        d.compute_scan(coeff_lb=family["coeff"])
    with pytest.raises(ParameterError, match="from_linear"):
        d.compute_scan_fes(None, family["coeff"], family["offset"], sample_label=np.zeros(5000, dtype=np.int32))


def test_verbose_same_state_check_reads_the_basis_not_the_matrix(family, caplog):
    coeff = family["coeff"].copy()
    offset = family["offset"].copy()
    coeff[3], offset[3] = coeff[1], offset[1]  # states 1 and 3 are the same state
    with caplog.at_level(logging.INFO, logger="pymbar_amd.mbar"):
        m = pymbar_amd.MBAR.from_linear(family["basis"], coeff, family["N_k"], offset_k=offset, verbose=True, rseed=3)
    assert any("States 1 and 3 have the same energies" in r.getMessage() for r in caplog.records)
    assert [1, 3] in m.samestates and [3, 1] in m.samestates
    assert m._u_kn is None
    # the random draw of the check is the dense constructor's: same generator state afterwards
    d = pymbar_amd.MBAR(u_model(family["basis"], coeff, offset), family["N_k"], verbose=True, rseed=3)
    assert d.samestates == m.samestates
    assert m.rng.integers(1 << 30) == d.rng.integers(1 << 30)
