"""Weighted kernel-density sums on the MI355X (``mbar_kde_*``, csrc/mbar_k_kde.hip) against the exact numpy oracle
(tests/kde_oracle.py): every kernel in d = 1, 2, 3, 5, sample / query / column counts on and off the tile sizes, queries far
outside the data, the rescale branch of the running shift forced, zero weights, determinism, one large case, and the whole
``pymbar_amd.FES`` class against the reference's fixtures."""
import numpy as np
import pytest

import pymbar_amd
from pymbar_amd.kde import DeviceKDE, KernelDensity
from tests import kde_oracle
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
KERNELS = kde_oracle.KERNELS


def _close(dev, ora, tol=1e-11):
    assert dev.shape == ora.shape
    np.testing.assert_array_equal(np.isnan(dev), np.isnan(ora))
    np.testing.assert_array_equal(np.isneginf(dev), np.isneginf(ora))
    assert not np.any(np.isposinf(dev))
    fin = np.isfinite(ora)
    err = np.abs(dev[fin] - ora[fin]) / np.maximum(1.0, np.abs(ora[fin]))
    assert err.size == 0 or err.max() <= tol, f"max scaled error {err.max():.3e}"


def _case(kernel, d, N, M, C, seed):
    rng = np.random.RandomState(seed)
    h = 0.35
    X = rng.normal(size=(N, d))
    V = rng.uniform(0.0, 2.0, size=(N, C)) * (rng.uniform(size=(N, 1)) > 0.2)  # ~20 % zero-weight samples
    if C >= 2:
        V[:, 1] = 0.0  # a column without weight: NaN
    V[0] = rng.uniform(0.5, 1.0, size=C) * (np.arange(C) != 1)  # (at least one positive weight per live column)
    Q = rng.normal(scale=1.3, size=(M, d))
    if M >= 3:
        Q[-1] = X.max(axis=0) + 40 * h  # 40 h and 300 h away from all data: finite for gaussian / exponential
        Q[-2] = X.min(axis=0) - 300 * h
    return X, V, Q, h


def _grid():
    out = []
    for kernel in KERNELS:
        for d in (1, 2, 3, 5):
            out.append((kernel, d, 7, 4099, 65))
            out.append((kernel, d, 1, 17, 1))
            out.append((kernel, d, 1_000_003, 17 if d < 5 else 1, 2 if d % 2 else 17))
    return out


@pytest.mark.parametrize("kernel,d,N,M,C", _grid())
def test_device_matches_oracle(kernel, d, N, M, C):
    X, V, Q, h = _case(kernel, d, N, M, C, seed=d * 1000 + N % 97 + M + C)
    with DeviceKDE(X, kernel, h) as dk:
        dk.set_weights(V)
        got = dk.log_density(Q)
    _close(got, kde_oracle.log_density(X, V, Q, kernel, h))
    if kernel in ("gaussian", "exponential") and M >= 3:
        assert np.all(np.isfinite(got[-2:, 0]))


@pytest.mark.parametrize("kernel", ["gaussian", "exponential"])
def test_rescale_branch_forced(kernel):
    """Every 64-sample tile streams far samples first and its nearest sample last, and the tiles of a workgroup's chunk come in
    order of decreasing distance: the running shift of each query moves inside tiles and across tiles; in the second set the
    first tiles' largest term lies e^1000 below the last tile's."""
    rng = np.random.RandomState(3)
    h = 1.0
    M = 4099
    Q = rng.uniform(-0.2, 0.2, size=(M, 1))
    ntiles = 200
    far = 46.0 if kernel == "gaussian" else 1010.0  # first terms ~e^-1060 / e^-1010 against the last ones
    X = np.empty((ntiles, 64))
    for t in range(ntiles):
        X[t, :63] = far + rng.uniform(0.0, 5.0, size=63) + (ntiles - t) * 0.01
        X[t, 63] = (ntiles - t) * 0.02
    X = X.reshape(-1, 1)
    V = rng.uniform(0.5, 1.5, size=(len(X), 3))
    V[::7, 2] = 0.0
    for XX in (X, np.vstack([far + 10 + rng.uniform(size=(64 * 50, 1)), [[0.01]]])):
        VV = V[:len(XX)] if len(XX) <= len(V) else rng.uniform(0.5, 1.5, size=(len(XX), 3))
        with DeviceKDE(XX, kernel, h) as dk:
            dk.set_weights(VV)
            got = dk.log_density(Q)
        ora = kde_oracle.log_density(XX, VV, Q, kernel, h)
        assert np.all(np.isfinite(ora))
        _close(got, ora)


def test_far_queries_and_zero_weight_near_samples():
    """The nearest samples of a query carry no weight in one column: that column's terms all underflow against the shared shift,
    and the pair is recomputed with its own maximum (finite, exact)."""
    rng = np.random.RandomState(9)
    X = np.vstack([rng.normal(size=(500, 2)), rng.normal(size=(500, 2)) + 60.0])
    V = np.ones((1000, 3))
    V[500:, 1] = 0.0  # column 1: only the cluster at the origin
    V[:500, 2] = 0.0  # column 2: only the far cluster
    Q = np.vstack([rng.normal(size=(20, 2)) + 60.0, rng.normal(size=(20, 2))])
    for kernel in ("gaussian", "exponential", "tophat"):
        with DeviceKDE(X, kernel, 0.2) as dk:
            dk.set_weights(V)
            got = dk.log_density(Q)
        ora = kde_oracle.log_density(X, V, Q, kernel, 0.2)
        _close(got, ora)
        if kernel == "gaussian":
            assert np.all(np.isfinite(got))


def test_determinism_and_batched_columns():
    rng = np.random.RandomState(5)
    X = rng.normal(size=(300_001, 2))
    V = rng.uniform(size=(300_001, 40))
    Q = rng.normal(size=(1000, 2))
    with DeviceKDE(X, "gaussian", 0.1) as dk:
        dk.set_weights(V)
        a = dk.log_density(Q)
        b = dk.log_density(Q)
        np.testing.assert_array_equal(a.view(np.uint64), b.view(np.uint64))
        for c in (0, 17, 39):
            dk.set_weights(V[:, c])
            one = dk.log_density(Q)[:, 0]
            np.testing.assert_allclose(a[:, c], one, rtol=1e-13, atol=1e-13)


def test_at_scale_n4e6_d2_c21():
    rng = np.random.RandomState(11)
    N = 4_000_000
    X = rng.normal(size=(N, 2))
    V = rng.uniform(size=(N, 21))
    Q = rng.normal(scale=1.5, size=(64, 2))
    with DeviceKDE(X, "gaussian", 0.05) as dk:
        dk.set_weights(V)
        got = dk.log_density(Q)
    _close(got, kde_oracle.log_density(X, V, Q, "gaussian", 0.05))


def test_kernel_density_estimator_on_device():
    g = load_golden("fes_kde.npz")
    for data in ("int", "real"):
        X, w, Q, h = g[f"c_{data}_x"], g[f"c_{data}_w"], g[f"c_{data}_q"], float(g[f"c_{data}_h"])
        for kernel in KERNELS:
            got = KernelDensity(kernel=kernel, bandwidth=h).fit(X, sample_weight=w).score_samples(Q)
            want = g[f"c_{data}_{kernel}"]
            _close(got, want, tol=1e-12)


def test_fes_kde_1d_reproduces_reference():
    g = load_golden("fes_kde.npz")
    u = load_golden("fes_umbrella_1d.npz")
    fes = pymbar_amd.FES(u["u_kn"], u["N_k"])
    fes.generate_fes(u["u_n"], u["x_n"], fes_type="kde", kde_parameters={"bandwidth": float(g["a_bandwidth"])},
                     n_bootstraps=int(g["a_n_bootstraps"]), seed=int(g["a_seed"]))
    for name in ("centers", "grid"):
        q = g[f"a_{name}"]
        lo = fes.get_fes(q, reference_point="from-lowest", uncertainty_method="bootstrap")
        np.testing.assert_allclose(lo["f_i"], g[f"a_{name}_f_lowest"], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(lo["df_i"], g[f"a_{name}_df_lowest"], rtol=1e-9, atol=1e-9)
        sp = fes.get_fes(q, reference_point="from-specified", fes_reference=0.0, uncertainty_method="bootstrap")
        np.testing.assert_allclose(sp["f_i"], g[f"a_{name}_f_specified"], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(sp["df_i"], g[f"a_{name}_df_specified"], rtol=1e-9, atol=1e-9)
        nz = fes.get_fes(q, reference_point="from-normalization")
        np.testing.assert_allclose(nz["f_i"], g[f"a_{name}_f_normalization"], rtol=1e-9, atol=1e-9)
    fes.kde.close()
    fes.mbar.close()


def test_fes_kde_2d_reproduces_reference_where_it_is_exact():
    g = load_golden("fes_kde.npz")
    x_n, u_n, xu = g["b_x_n"], g["b_u_n"], g["b_umbrella_centers"]
    u_kn = np.array([u_n + g["b_beta"] * (g["b_Ku"] / 2) * np.sum((x_n - xu[k]) ** 2, axis=1) for k in range(len(xu))])
    fes = pymbar_amd.FES(u_kn, g["b_N_k"])
    fes.generate_fes(u_n, x_n, fes_type="kde", kde_parameters={"bandwidth": float(g["b_bandwidth"])},
                     n_bootstraps=int(g["b_n_bootstraps"]), seed=int(g["b_seed"]))
    np.testing.assert_allclose(fes.mbar.f_k, g["b_f_k"], atol=1e-9)
    q = g["b_queries"]
    L = fes.kde.score_samples_columns(np.vstack([q, [[0.0, 0.0]]]), fes.bootstrap_weights)
    exact, ref = g["b_exact_L"], g["b_ref_L"]
    _close(L, exact, tol=1e-9)  # (the MBAR weights themselves agree to ~1e-10)
    ok = np.abs(exact - ref) <= 1e-9 * np.maximum(1.0, np.abs(exact))
    if np.all(ok):  # the reference's tree sum is exact on this system: its answers are reproduced
        lo = fes.get_fes(q, reference_point="from-lowest", uncertainty_method="bootstrap")
        np.testing.assert_allclose(lo["f_i"], g["b_f_lowest"], rtol=1e-8, atol=1e-8)
        np.testing.assert_allclose(lo["df_i"], g["b_df_lowest"], rtol=1e-7, atol=1e-8)
        sp = fes.get_fes(q, reference_point="from-specified", fes_reference=[0, 0], uncertainty_method="bootstrap")
        np.testing.assert_allclose(sp["f_i"], g["b_f_specified"], rtol=1e-8, atol=1e-8)
        np.testing.assert_allclose(sp["df_i"], g["b_df_specified"], rtol=1e-7, atol=1e-8)
        nz = fes.get_fes(q, reference_point="from-normalization")
        np.testing.assert_allclose(nz["f_i"], g["b_f_normalization"], rtol=1e-8, atol=1e-8)
    fes.kde.close()
    fes.mbar.close()


def test_fes_histogram_class_on_device():
    u = load_golden("fes_umbrella_1d.npz")
    fes = pymbar_amd.FES(u["u_kn"], u["N_k"])
    fes.generate_fes(u["u_n"], u["x_n"], histogram_parameters={"bin_edges": u["bin_edges"]})
    e = u["bin_edges"]
    centers = 0.5 * (e[1:] + e[:-1])
    grid = u["grid_of_label"]
    in_grid = centers[grid[(grid >= 0) & (grid < len(centers))]]
    lo = fes.get_fes(in_grid, reference_point="from-lowest", uncertainty_method="analytical")
    np.testing.assert_allclose(lo["f_i"], u["f_lowest"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(lo["df_i"], u["df_lowest"], rtol=1e-7, atol=1e-9)
    sp = fes.get_fes(in_grid, reference_point="from-specified", fes_reference=0.0, uncertainty_method="analytical")
    np.testing.assert_allclose(sp["f_i"], u["f_specified"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(sp["df_i"], u["df_specified"], rtol=1e-7, atol=1e-9)
    fes.mbar.close()
