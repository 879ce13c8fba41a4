"""Weighted B-spline moments on the MI355X (``mbar_bspline_*``) against the long-double oracle of tests/bspline_oracle.py (every
body of ``k_bspline<K, CB>`` among them, and the bases against scipy's design matrix bit for bit), and
the spline surfaces of ``pymbar_amd.FES`` through the device against the unmodified reference (tests/golden/fes_spline.npz)."""
import numpy as np
import pytest
from scipy.interpolate import BSpline

import pymbar_amd
from pymbar_amd import bspline as amd_bspline
from pymbar_amd.bspline import DeviceBSplineMoments
from tests import bspline_oracle as bo
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu


knots = bo.knots


def check(x, V, t, k, groups=None, G=1):
    with DeviceBSplineMoments(x, groups=groups, n_groups=G if groups is not None else None) as dev:
        dev.set_weights(V)
        got = dev.moments(t, k)
        again = dev.moments(t, k)
    assert got.tobytes() == again.tobytes()  # bitwise-identical repeat
    want = bo.moments(x, V, t, k, groups, G)
    scale = bo.abs_moments(x, V, t, k, groups, G)
    err = np.abs(got.astype(np.longdouble) - want)
    bound = 1e-14 * scale
    assert np.all(err <= bound), float(np.max(err - bound))
    return got


@pytest.mark.parametrize("k", range(8))
def test_moments_every_degree_random_x(k):
    rng = np.random.default_rng(k)
    nbasis = 12 + 3 * k
    t = knots(k, nbasis, rng=rng)
    x = np.r_[rng.uniform(-1.4, 1.4, 5003), t, 1.0]  # outside xrange, at the knots, at xrange[1]
    V = rng.normal(size=(len(x), 2))
    g = rng.integers(0, 5, len(x))
    check(x, V, t, k, g, G=7)  # (groups 5 and 6 empty)


@pytest.mark.parametrize("C", [1, 2, 33])
def test_moments_columns_and_pass_boundary(C):
    rng = np.random.default_rng(10 + C)
    t = knots(3, 40)
    x = rng.uniform(-1.2, 1.2, 3000)
    check(x, rng.normal(size=(len(x), C)), t, 3, rng.integers(0, 64, len(x)), G=64)


@pytest.mark.parametrize("N", [1, 255, 257, 4097, 9001])
def test_moments_ragged_sizes(N):
    rng = np.random.default_rng(N)
    t = knots(2, 9)
    check(rng.uniform(-1.1, 1.1, N), rng.uniform(0, 1, N), t, 2)


def test_moments_large_basis_and_many_cells_per_wave():
    rng = np.random.default_rng(5)
    t = knots(3, 1024, rng=rng)
    x = rng.uniform(-1, 1, 20000)  # random order: up to 64 cells per wave
    check(x, rng.normal(size=(len(x), 2)), t, 3, rng.integers(0, 16, len(x)), G=16)
    t7 = knots(7, 300)
    check(rng.uniform(-1, 1, 20000), np.ones(20000), t7, 7, rng.integers(0, 64, 20000), G=64)


def test_moments_state_sorted_7e6():
    rng = np.random.default_rng(7)
    centers = 0.2 * np.arange(-3, 4)
    n = 1_000_000
    x = np.concatenate([rng.normal(c, np.sqrt(1 / 120.0), n) for c in centers])
    g = np.repeat(np.arange(7), n)
    t = knots(3, 10, -0.7, 0.7)
    check(x, np.ones(len(x)), t, 3, g, G=7)


# ---- every body of k_bspline<K, CB>: K = 0 .. 7 x CB = 1, 2, 4, 8, 16, 32 (C = 1, 2, 3, 7, 13, 29) -------------------------------------
@pytest.mark.parametrize("C", list(bo.C_TO_CB))
@pytest.mark.parametrize("k", range(8))
def test_moments_every_body(k, C):
    """One sample chunk (N = 700: three batches for wave 0, a ragged last batch), about 2.5 output tiles with samples on both sides
    of and across every tile seam (tests/bspline_oracle.py: matrix_case; tests/test_spline_fes_host.py checks the coverage)."""
    x, V, t, g, G = bo.matrix_case(k, C)
    check(x, V, t, k, g, G)


@pytest.mark.parametrize("k,C", list(zip((2, 5, 3, 7, 1, 4), bo.C_TO_CB)))
def test_moments_every_width_two_chunks(k, C):
    x, V, t, g, G = bo.matrix_case(k, C, N=4096 + 300)
    check(x, V, t, k, g, G)


@pytest.mark.parametrize("k", range(8))
def test_bases_are_scipys_bits(k):
    """One sample per group and unit weights: row g of the moments is a single product through exact sums, so it must be row g of
    scipy's design matrix bit for bit (the claim of csrc/mbar_k_bspline.hip; scipy's matrix is the unfused float64 recursion,
    tests/test_spline_fes_host.py).  The device adds a product to zeros, so a zero comes out positive: values are compared, the
    sign of a zero is not.  With 13 columns (CB = 16), one of ones and the others powers of two, the scaling is exact too."""
    x, t = bo.scipy_case(k)
    N = len(x)
    D = BSpline.design_matrix(x, t, k, extrapolate=True).toarray()
    scale = 2.0 ** np.array([0, -3, 5, 1, -1, 10, -20, 2, 3, -2, 7, -7, 4])
    with DeviceBSplineMoments(x, groups=np.arange(N), n_groups=N) as dev:
        got = dev.moments(t, k)
        assert got.shape == (N, 1, D.shape[1])
        np.testing.assert_array_equal(got[:, 0, :], D)
        dev.set_weights(np.tile(scale, (N, 1)))
        got = dev.moments(t, k)
        np.testing.assert_array_equal(got, D[:, None, :] * scale[None, :, None])


def test_nonfinite_input_raises():
    from pymbar_amd.utils import DataError

    with pytest.raises(DataError):
        DeviceBSplineMoments([0.0, np.nan])
    with DeviceBSplineMoments([0.0, 1.0]) as dev:
        with pytest.raises(DataError):
            dev.set_weights([1.0, np.inf])


# ---- the surfaces through the device --------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("name", ["a", "b", "c", "c2", "c3", "c4", "c5", "d"])
def test_device_fit_reproduces_reference(gold, umb, name):
    fes = fit(umb, bo.spline_cases(gold)[name])
    tol = FIT_TOL.get(name, 2e-6)
    np.testing.assert_allclose(fes.fes_function.c, gold[f"{name}_c"], rtol=1e-6, atol=tol)
    np.testing.assert_allclose(fes.get_fes(gold["grid"])["f_i"], gold[f"{name}_f_grid"], rtol=1e-6, atol=tol)
    np.testing.assert_allclose(fes.get_information_criteria("aic"), gold[f"{name}_aic"], rtol=1e-8)
    np.testing.assert_allclose(fes.get_information_criteria("bic"), gold[f"{name}_bic"], rtol=1e-8)


@pytest.mark.parametrize("name,base", [("e_u", "a"), ("e_b", "b")])
def test_device_bootstraps_reproduce_reference(gold, umb, name, base):
    fes = fit(umb, bo.spline_cases(gold)[base], n_bootstraps=2, seed=int(gold[f"{name}_seed"]))
    tol = 1e-6 if name == "e_b" else 2e-5
    for fb, want in zip(fes.fes_functions, gold[f"{name}_c_boot"]):
        np.testing.assert_allclose(fb.c, want, rtol=tol, atol=tol)
    r = fes.get_fes(gold["grid"], uncertainty_method="bootstrap")
    np.testing.assert_allclose(r["df_i"], gold[f"{name}_df_grid"], rtol=1e-3, atol=tol * 10)


@pytest.mark.parametrize("name,base", [("f_u", "a"), ("f_b", "b")])
def test_device_mc_reproduces_reference(gold, umb, name, base):
    fes = fit(umb, bo.spline_cases(gold)[base])
    fes.fes_function = BSpline(fes.fes_function.t, gold[f"{name}_c_start"].copy(), fes.fes_function.k)
    fes.w_n = gold[f"{base}_w_n"]
    np.random.seed(int(gold[f"{name}_seed"]))
    fes.sample_parameter_distribution(umb["x_n"], mc_parameters=dict(niterations=300, fraction_change=0.02, sample_every=10),
                                      decorrelate=True, verbose=False)
    mc = fes.get_mc_data()
    assert round(mc["acceptance_ratio"] * 300) == round(float(gold[f"{name}_acceptance"]) * 300)
    assert mc["nequil"] == int(gold[f"{name}_nequil"])
    np.testing.assert_allclose(mc["samples"], gold[f"{name}_samples"], rtol=1e-9, atol=1e-9)
    ci = fes.get_confidence_intervals(gold["grid"], 5, 95)
    for key in ("plow", "phigh", "median", "values"):
        np.testing.assert_allclose(ci[key], gold[f"{name}_ci_{key}"], rtol=1e-9, atol=1e-9)


class _Float64Moments(bo.OracleBSplineMoments):
    """Host moments in plain float64 (scipy's design matrix): the comparison fit of the 7e6-sample test."""

    def moments(self, t, k):
        D = BSpline.design_matrix(self.x, t, k, extrapolate=True).tocsc()
        G = self.n_groups
        g = np.zeros(self.n_samples, dtype=np.int64) if self.groups is None else self.groups
        return np.stack([(self.V[g == q].T @ D[g == q]) for q in range(G)])


def test_fit_at_7e6_matches_host_moments(monkeypatch):
    rng = np.random.default_rng(1234)
    centers, K0, Ku, n = 0.2 * np.arange(-3, 4), 20.0, 100.0, 1_000_000
    x = np.concatenate([rng.normal(c * Ku / (K0 + Ku), np.sqrt(1 / (K0 + Ku)), n) for c in centers])
    u_n = 0.5 * K0 * x ** 2
    u_kn = np.stack([u_n + 0.5 * Ku * (x - c) ** 2 for c in centers])
    N_k = np.full(7, n)
    params = dict(spline_weights="biasedstates", nspline=10, kdegree=3, xrange=[-0.7, 0.7], optimization_algorithm="Newton-CG",
                  spline_initialize="zeros", optimize_options={"disp": False, "tol": 1e-10},
                  fkbias=bo.fkbias_list(centers, Ku))
    fes = pymbar_amd.FES(u_kn, N_k)
    fes.generate_fes(u_n, x, fes_type="spline", spline_parameters=dict(params))
    c_dev, M_dev = fes.fes_function.c.copy(), fes._spline_M.copy()
    monkeypatch.setattr(amd_bspline, "DeviceBSplineMoments", _Float64Moments)
    fes.generate_fes(u_n, x, fes_type="spline", spline_parameters=dict(params))
    np.testing.assert_allclose(M_dev, fes._spline_M, rtol=1e-12)
    # (the two fits differ where Newton-CG stops: 1.6e-7 at most, on the coefficient next to xrange[1])
    np.testing.assert_allclose(c_dev, fes.fes_function.c, rtol=1e-6, atol=1e-6)
