"""Spline surfaces on the CPU: the long-double moment oracle (tests/bspline_oracle.py) against scipy's design matrix, and the
whole ``pymbar_amd.FES`` spline path -- fits, bootstraps, information criteria, the Monte Carlo sampler and its confidence
intervals -- against the unmodified reference (tests/golden/fes_spline.npz, tests/golden/make_golden_fes_spline.py), with the
device pieces replaced by CPU stand-ins (``OracleMatrix``, ``OracleBSplineMoments``, ``OracleACF``).  Also the deviations from
the reference listed in INTEGRATION.md ("FES")."""
import numpy as np
import pytest
from scipy.interpolate import BSpline

import pymbar_amd
from pymbar_amd import bspline as amd_bspline
from pymbar_amd.utils import ConvergenceError, DataError, ParameterError
from tests import bspline_oracle as bo
from tests.conftest import load_golden


@pytest.fixture
def standins(monkeypatch):
    import pymbar_amd.device
    from pymbar_amd import timeseries
    from tests import timeseries_oracle
    from tests.cpu_standin import OracleMatrix

    monkeypatch.setattr(pymbar_amd.device, "DeviceMatrix", OracleMatrix)
    monkeypatch.setattr(amd_bspline, "DeviceBSplineMoments", bo.OracleBSplineMoments)
    monkeypatch.setattr(timeseries, "DeviceACF", timeseries_oracle.OracleACF)


@pytest.fixture(scope="module")
def gold():
    return load_golden("fes_spline.npz")


@pytest.fixture(scope="module")
def umb():
    return load_golden("fes_umbrella_1d.npz")


# the optimisers stop within their tolerance: CG with gtol 1e-6 (case c3) leaves coefficients a few 1e-6 from the optimum, and
# rounding-level differences in the data term move where it stops
FIT_TOL = {"c3": 1e-5}


def fit(umb, params, **kw):
    fes = pymbar_amd.FES(umb["u_kn"], umb["N_k"])
    fes.generate_fes(umb["u_n"], umb["x_n"], fes_type="spline", spline_parameters=params, **kw)
    return fes


# ---- the oracle --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(6))
def test_oracle_matches_scipy_design_matrix(k):
    rng = np.random.default_rng(k)
    inner = np.sort(rng.uniform(-1.0, 2.0, 9))
    inner[3] = inner[4]  # a repeated interior knot
    t = np.r_[[-1.0] * (k + 1), inner, [2.0] * (k + 1)]
    x = np.r_[rng.uniform(-1.5, 2.5, 400), t, 2.0, -1.0]  # outside xrange, on every knot, at both ends
    V = np.stack([np.ones(len(x)), rng.normal(size=len(x))], axis=1)
    D = BSpline.design_matrix(x, t, k, extrapolate=True).toarray()
    want = V.T @ D
    got = bo.moments(x, V, t, k)[0]
    scale = bo.abs_moments(x, V, t, k)[0].astype(np.float64)
    assert np.all(np.abs(got.astype(np.float64) - want) <= 1e-13 * scale + 1e-300)
    # and the intervals are scipy's (a value at a knot belongs to the interval it opens; at xrange[1], the last one)
    np.testing.assert_array_equal(bo.intervals(t, k, [2.0, 2.5, -1.5])[[0, 1]], [len(t) - k - 2] * 2)


@pytest.mark.parametrize("k", range(8))
def test_scipy_design_matrix_is_the_unfused_float64_recursion(k):
    """What the device's bases are held to bit for bit (tests/test_gpu_spline_fes.py): scipy's design matrix equals the Cox-de Boor
    recursion with every operation rounded to float64 and none fused, on the very case the device test uses."""
    x, t = bo.scipy_case(k)
    assert len(x) == 300 and x.min() < t[0] and x.max() > t[-1] and np.all(np.isin(t, x)) and np.any(np.diff(t[k:-k or None]) == 0)
    D = BSpline.design_matrix(x, t, k, extrapolate=True).toarray()
    h, l = bo.basis_values(t, k, x, dtype=np.float64)
    want = np.zeros_like(D)
    for j in range(k + 1):
        want[np.arange(len(x)), l - k + j] = h[:, j]
    np.testing.assert_array_equal(D, want)  # (equal values: the sign of a zero is not compared)


@pytest.mark.parametrize("C", list(bo.C_TO_CB))
def test_matrix_cases_cover_the_tile_seams(C):
    for k in range(8):
        for N in (700, 4096 + 300):
            x, V, t, g, G = bo.matrix_case(k, C, N)
            nbasis = len(t) - k - 1
            assert len(x) == N and V.shape == (N, C) and 1 <= G <= 1024 and g.min() >= 0 and g.max() < G
            assert np.all(np.isin(t, x)) and x.min() < t[0] and x.max() > t[-1] and np.any(np.diff(t[k:-k or None]) == 0)
            seams = bo.tile_seams(k, nbasis, G, C)
            assert 2 <= len(seams) + 1 <= 4  # several tiles, G nbasis a small multiple of the tile
            key = bo.cell_keys(x, g, t, k)
            for f0 in seams:
                i = f0 % nbasis
                assert np.any(key + k < f0) and np.any(key >= f0)
                if k >= 1 and 1 <= i <= nbasis - k:  # the seam lies inside a row: a sample's entries lie across it
                    assert np.any((key < f0) & (key + k >= f0)), (k, C, f0)


def test_oracle_groups_and_columns():
    rng = np.random.default_rng(3)
    x = rng.uniform(0, 1, 300)
    g = rng.integers(0, 4, 300)
    V = rng.normal(size=(300, 3))
    t = np.r_[[0.0] * 3, np.linspace(0, 1, 6), [1.0] * 3]
    M = bo.moments(x, V, t, 2, g, G=5)
    assert M.shape == (5, 3, len(t) - 3)
    assert np.all(M[4] == 0)
    D = BSpline.design_matrix(x, t, 2).toarray()
    for q in range(4):
        np.testing.assert_allclose(M[q].astype(float), V[g == q].T @ D[g == q], rtol=1e-12, atol=1e-12)


# ---- the fits against the reference ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "b", "c", "c2", "c3", "c4", "c5", "d"])
def test_fit_reproduces_reference(standins, gold, umb, name):
    fes = fit(umb, bo.spline_cases(gold)[name])
    np.testing.assert_allclose(fes.fes_function.t, gold[f"{name}_t"], rtol=0, atol=0)
    tol = FIT_TOL.get(name, 2e-6)
    np.testing.assert_allclose(fes.fes_function.c, gold[f"{name}_c"], rtol=1e-6, atol=tol)
    f = fes.get_fes(gold["grid"], reference_point="from-lowest")
    np.testing.assert_allclose(f["f_i"], gold[f"{name}_f_grid"], rtol=1e-6, atol=tol)
    assert f["df_i"] is None
    aic, bic = fes.get_information_criteria("aic"), fes.get_information_criteria("BIC")
    assert type(aic) is float and type(bic) is float  # (the reference: shape-(1,) arrays for unbiasedstate)
    np.testing.assert_allclose(aic, gold[f"{name}_aic"], rtol=1e-8)
    np.testing.assert_allclose(bic, gold[f"{name}_bic"], rtol=1e-8)
    np.testing.assert_allclose(fes.w_n, gold[f"{name}_w_n"], rtol=1e-9, atol=1e-15)


@pytest.mark.parametrize("name,base", [("e_u", "a"), ("e_b", "b")])
def test_bootstraps_reproduce_reference(standins, gold, umb, name, base):
    fes = fit(umb, bo.spline_cases(gold)[base], n_bootstraps=2, seed=int(gold[f"{name}_seed"]))
    np.testing.assert_allclose(fes.fes_function.c, gold[f"{name}_c"], rtol=1e-6, atol=2e-6)
    assert len(fes.fes_functions) == 2
    if name == "e_u":
        # f_b: re-solved on the resident matrix with the draw counts as multiplicities (the fixture: the resampled matrix to 1e-12)
        for f_b, want in zip(fes._spline_f_boots, gold[f"{name}_f_boots"]):
            np.testing.assert_allclose(f_b, want, rtol=0, atol=1e-8)
    # the reference solves each replicate's MBAR to relative tolerance 1e-7 only: its replicate surfaces carry that error
    tol = 1e-6 if name == "e_b" else 2e-5
    for fb, want in zip(fes.fes_functions, gold[f"{name}_c_boot"]):
        np.testing.assert_allclose(fb.c, want, rtol=tol, atol=tol)
    r = fes.get_fes(gold["grid"], reference_point="from-lowest", uncertainty_method="bootstrap")
    np.testing.assert_allclose(r["f_i"], gold[f"{name}_f_grid"], rtol=1e-6, atol=2e-6)
    np.testing.assert_allclose(r["df_i"], gold[f"{name}_df_grid"], rtol=1e-3, atol=tol * 10)


def test_bootstrap_stream_is_the_references(standins, gold, umb):
    """The draws of replicate b, per state, plus one int32 draw per skipped MBAR construction (seeded)."""
    np.random.seed(int(gold["e_u_seed"]))
    N_k = umb["N_k"]
    idx = np.arange(len(umb["u_n"]))
    for b in range(2):
        off = 0
        for n in N_k:
            idx[off:off + n] = off + np.random.randint(0, n, size=n)
            off += n
            np.random.randint(np.iinfo(np.int32).max)
        np.testing.assert_array_equal(idx, gold["e_u_idx"][b])


@pytest.mark.parametrize("name,base", [("f_u", "a"), ("f_b", "b")])
def test_mc_chain_reproduces_reference_step_for_step(standins, gold, umb, name, base):
    fes = fit(umb, bo.spline_cases(gold)[base])
    # start the chain where the reference's started: its fitted coefficients and weights (the fits agree to the optimiser's tol)
    t, k = fes.fes_function.t, fes.fes_function.k
    fitted = fes.fes_function
    fes.fes_function = BSpline(t, gold[f"{name}_c_start"].copy(), k)
    fes.w_n = gold[f"{base}_w_n"]
    np.random.seed(int(gold[f"{name}_seed"]))
    mc_parameters = dict(niterations=300, fraction_change=0.02, sample_every=10, print_every=1000)
    fes.sample_parameter_distribution(umb["x_n"], mc_parameters=mc_parameters, decorrelate=True, verbose=False)
    mc = fes.get_mc_data()
    assert round(mc["acceptance_ratio"] * 300) == round(float(gold[f"{name}_acceptance"]) * 300)
    assert mc["nequil"] == int(gold[f"{name}_nequil"])
    np.testing.assert_allclose(mc["samples"], gold[f"{name}_samples"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(mc["logposteriors"], gold[f"{name}_logposteriors"], rtol=1e-9)
    np.testing.assert_allclose(mc["g_logposterior"], gold[f"{name}_g_logposterior"], rtol=1e-6)
    np.testing.assert_allclose(mc["g"], gold[f"{name}_g"], rtol=1e-6)
    np.testing.assert_allclose(mc["g_parameters"], gold[f"{name}_g_parameters"], rtol=1e-6)
    ci = fes.get_confidence_intervals(gold["grid"], 5, 95)
    for key in ("plow", "phigh", "median", "values"):
        np.testing.assert_allclose(ci[key], gold[f"{name}_ci_{key}"], rtol=1e-9, atol=1e-9)
    # deviation: the fitted surface is left alone (the reference's get_fes after MC returns the chain's last sample)
    assert fes.fes_function is not mc["bspline"]
    np.testing.assert_array_equal(fes.fes_function.c, gold[f"{name}_c_start"])
    assert fitted is not None


# ---- deviations from the reference ("FES") ----------------------------------------------------------------
def test_custom_nr_reaches_newton_cg_optimum(standins, gold, umb):
    p = bo.spline_cases(gold)["c3"]
    ref = fit(umb, dict(p, optimization_algorithm="Newton-CG", optimize_options={"disp": False, "tol": 1e-10}))
    nr = fit(umb, dict(p, optimization_algorithm="Custom-NR", optimize_options={"gtol": 1e-7}))
    np.testing.assert_allclose(nr.fes_function.c, ref.fes_function.c, rtol=1e-6, atol=1e-6)
    assert type(nr.get_information_criteria("aic")) is float


def test_custom_nr_iteration_cap_raises(standins, gold, umb, monkeypatch):
    import pymbar_amd.fes as fesmod

    monkeypatch.setattr(fesmod, "CUSTOM_NR_MAXITER", 1)
    p = bo.spline_cases(gold)["c4"]
    with pytest.raises(ConvergenceError):
        fit(umb, dict(p, optimization_algorithm="Custom-NR", optimize_options={"gtol": 1e-12}))


def test_from_specified_is_f_minus_f_ref(standins, gold, umb):
    fes = fit(umb, bo.spline_cases(gold)["a"])
    grid = gold["grid"]
    r = fes.get_fes(grid, reference_point="from-specified", fes_reference=0.0)
    assert r["f_i"].shape == grid.shape
    np.testing.assert_allclose(r["f_i"], fes.fes_function(grid) - fes.fes_function(0.0), rtol=0, atol=1e-14)
    # the reference's answer is f(x) + f(ref) (it subtracts -f(ref))
    np.testing.assert_allclose(gold["a_f_specified"] - 2.0 * float(BSpline(gold["a_t"], gold["a_c"], 3)(0.0)), r["f_i"],
                               rtol=1e-6, atol=2e-6)
    with pytest.raises(ParameterError):
        fes.get_fes(grid, reference_point="from-specified", fes_reference=None)
    with pytest.raises(ParameterError):
        fes.get_fes(grid, reference_point="from-normalization")
    with pytest.raises(DataError):
        fes.get_fes(np.zeros((3, 2)))
    with pytest.raises(ParameterError):
        fes.get_fes(grid, uncertainty_method="bootstrap")  # no replicates


def test_mc_without_decorrelation_and_raised_errors(standins, gold, umb):
    fes = fit(umb, bo.spline_cases(gold)["c4"])
    np.random.seed(5)
    fes.sample_parameter_distribution(umb["x_n"], mc_parameters=dict(niterations=40, sample_every=5), decorrelate=False,
                                      verbose=False)
    mc = fes.get_mc_data()
    assert mc["g_parameters"] is None and mc["g"] is None and mc["nequil"] == 0
    assert mc["samples"].shape == (6, 8)
    kde = pymbar_amd.FES(umb["u_kn"], umb["N_k"])
    with pytest.raises(ParameterError):
        kde.sample_parameter_distribution(umb["x_n"])
    with pytest.raises(DataError):
        kde.get_mc_data()
    with pytest.raises(ParameterError):
        kde.get_information_criteria()


def test_hessian_needs_no_preceding_gradient(standins, gold, umb):
    for name in ("c2", "c3"):
        fes = fit(umb, bo.spline_cases(gold)[name])
        xi = fes.spline_data["first_coefficients"] + 0.01
        fes._spline_cache.clear()
        h_alone = fes._bspline_calculate_h(xi)
        fes._spline_cache.clear()
        fes._bspline_calculate_f(xi + 0.3)
        fes._bspline_calculate_g(xi + 0.3)
        h_after = fes._bspline_calculate_h(xi)
        np.testing.assert_array_equal(h_alone, h_after)
        # and it is the derivative of the gradient
        eps = 1e-5
        num = np.stack([(fes._bspline_calculate_g(xi + eps * e) - fes._bspline_calculate_g(xi - eps * e)) / (2 * eps)
                        for e in np.eye(len(xi))], axis=1)
        np.testing.assert_allclose(h_alone, num, rtol=1e-5, atol=1e-4 * np.abs(h_alone).max())


def test_spline_input_rules(standins, gold, umb):
    fes = pymbar_amd.FES(umb["u_kn"], umb["N_k"])
    p = bo.spline_cases(gold)["b"]
    for key in ("spline_weights", "nspline", "kdegree", "xrange", "optimization_algorithm", "spline_initialize", "fkbias"):
        q = {k: v for k, v in p.items() if k != key}
        with pytest.raises(ParameterError, match=f"without '{key}' are not supported on this backend"):
            fes.generate_fes(umb["u_n"], umb["x_n"], fes_type="spline", spline_parameters=q)
    for bad in (dict(optimization_algorithm="Nelder-Mead"), dict(objective="mle"), dict(kdegree=8, nspline=12),
                dict(nspline=1025), dict(spline_initialize="random"), dict(objective="map"),
                dict(spline_initialize="explicit")):
        with pytest.raises(ParameterError):
            fes.generate_fes(umb["u_n"], umb["x_n"], fes_type="spline", spline_parameters=dict(p, **bad))
    with pytest.raises(DataError):
        fes.generate_fes(umb["u_n"], np.full_like(umb["x_n"], np.nan), fes_type="spline",
                         spline_parameters=bo.spline_cases(gold)["c4"])
    # the caller's dict is not completed in place
    q = bo.spline_cases(gold)["c4"]
    keys = set(q)
    fes.generate_fes(umb["u_n"], umb["x_n"], fes_type="spline", spline_parameters=q)
    assert set(q) == keys and q["map_data"] is None


def test_device_handle_checks_limits_without_gpu():
    with pytest.raises(ParameterError):
        amd_bspline.check_spline_shape(np.zeros(20), 8)
    with pytest.raises(ParameterError):
        amd_bspline.check_spline_shape(np.zeros(1030), 3)
    with pytest.raises(ParameterError):
        amd_bspline.check_spline_shape([0.0, 1.0, 0.5, 2.0], 1)
    with pytest.raises(DataError):
        amd_bspline.DeviceBSplineMoments([0.0, np.inf])
