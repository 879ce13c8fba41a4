"""Kernel-density surfaces on the CPU: the exact numpy oracle (tests/kde_oracle.py) against sklearn's answers and the reference's
FES (tests/golden/fes_kde.npz, tests/golden/make_golden_fes_kde.py), the normalisers, parameter rules, the bootstrap draw
stream, and the whole ``pymbar_amd.FES`` class with the device pieces replaced by CPU stand-ins (``OracleMatrix`` for
``DeviceMatrix``, ``OracleKDE`` for ``DeviceKDE``)."""
import numpy as np
import pytest

import pymbar_amd
from pymbar_amd import kde as amd_kde
from pymbar_amd.utils import DataError, ParameterError
from tests import kde_cases, kde_oracle
from tests.conftest import load_golden

KERNELS = kde_oracle.KERNELS


@pytest.fixture
def standins(monkeypatch):
    import pymbar_amd.device
    from tests.cpu_standin import OracleMatrix

    monkeypatch.setattr(pymbar_amd.device, "DeviceMatrix", OracleMatrix)
    monkeypatch.setattr(amd_kde, "DeviceKDE", kde_oracle.OracleKDE)


# ---- the oracle against sklearn / the reference ---------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("data", ["int", "real"])
def test_oracle_reproduces_sklearn_all_kernels_1d(kernel, data):
    g = load_golden("fes_kde.npz")
    X, w, Q, h = g[f"c_{data}_x"], g[f"c_{data}_w"], g[f"c_{data}_q"], float(g[f"c_{data}_h"])
    want = g[f"c_{data}_{kernel}"]
    got = kde_oracle.log_density(X, w, Q, kernel, h)[:, 0]
    np.testing.assert_array_equal(np.isneginf(got), np.isneginf(want))  # the support boundary |r| == h decided as sklearn does
    fin = np.isfinite(want)
    np.testing.assert_allclose(got[fin], want[fin], rtol=1e-12, atol=1e-12)
    if data == "int" and kernel == "tophat":
        assert np.isneginf(want).any() and np.any(np.abs(Q[:, 0][:, None] - X[:, 0][None, :]) == h)


def _replicate_columns(w_n, N_k, seed, B):
    np.random.seed(seed)
    N = len(w_n)
    cols = np.empty((N, B + 1))
    cols[:, 0] = w_n
    idx = np.arange(N)
    for b in range(1, B + 1):
        off = 0
        for n in N_k:
            idx[off:off + n] = off + np.random.randint(0, n, size=n)
            off += n
            np.random.randint(np.iinfo(np.int32).max)  # the reference's per-state MBAR construction draws its seed
        cols[:, b] = np.bincount(idx, weights=w_n, minlength=N)
    return cols


def test_bootstrap_stream_matches_reference_replicate_1():
    g = load_golden("fes_kde.npz")
    u = load_golden("fes_umbrella_1d.npz")
    np.random.seed(int(g["a_seed"]))
    idx = np.arange(len(u["u_n"]))
    off = 0
    for n in u["N_k"]:
        idx[off:off + n] = off + np.random.randint(0, n, size=n)
        off += n
        np.random.randint(np.iinfo(np.int32).max)
    np.testing.assert_array_equal(idx, g["a_idx1"])


def test_oracle_reproduces_reference_kde_fes_1d():
    g = load_golden("fes_kde.npz")
    u = load_golden("fes_umbrella_1d.npz")
    h = float(g["a_bandwidth"])
    cols = _replicate_columns(g["a_w_n"], u["N_k"], int(g["a_seed"]), int(g["a_n_bootstraps"]))
    for name in ("centers", "grid"):
        q = g[f"a_{name}"][:, None]
        L = kde_oracle.log_density(u["x_n"], cols, np.vstack([q, [[0.0]]]), "gaussian", h)
        f = -L[:-1, 0]
        np.testing.assert_allclose(f, g[f"a_{name}_f_normalization"], rtol=1e-10, atol=1e-10)
        np.testing.assert_allclose(f - f.min(), g[f"a_{name}_f_lowest"], rtol=1e-10, atol=1e-10)
        np.testing.assert_allclose(f + L[-1, 0], g[f"a_{name}_f_specified"], rtol=1e-10, atol=1e-10)
        np.testing.assert_allclose(np.std(-L[:-1, 1:] - f.min(), axis=1), g[f"a_{name}_df_lowest"], rtol=1e-8, atol=1e-10)


def test_oracle_reproduces_exact_sums_of_2d_fixture():
    g = load_golden("fes_kde.npz")
    x_n, w_n, h = g["b_x_n"], g["b_w_n"], float(g["b_bandwidth"])
    cols = np.column_stack([w_n] + [np.bincount(i, weights=w_n, minlength=len(w_n)) for i in g["b_idx"]])
    q = np.vstack([g["b_queries"], [[0.0, 0.0]]])
    L = kde_oracle.log_density(x_n, cols, q, "gaussian", h)
    np.testing.assert_allclose(L, g["b_exact_L"], rtol=1e-11, atol=1e-11)


# ---- normalisers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", KERNELS)
def test_library_normaliser_matches_oracle(kernel):
    for d in range(1, 9):
        for h in (0.3, 1.0, 2.5):
            assert abs(amd_kde.log_normaliser(kernel, d, h) - kde_oracle.log_normaliser(kernel, d, h)) < 1e-12


@pytest.mark.parametrize("kernel", KERNELS)
def test_density_integrates_to_one_1d(kernel):
    h = 0.8
    R = (40.0 if kernel in ("gaussian", "exponential") else 1.5) * h
    n = 600_000
    edges = np.linspace(-R, R, n + 1)  # (cell edges at +-h for the compact kernels: R / h = 1.5 and n a multiple of 6)
    mid = 0.5 * (edges[1:] + edges[:-1])
    L = kde_oracle.log_density(np.zeros((1, 1)), np.ones(1), mid[:, None], kernel, h)[:, 0]
    assert abs(np.sum(np.exp(L)) * (2 * R / n) - 1.0) < 1e-6


@pytest.mark.parametrize("kernel", KERNELS)
def test_density_integrates_to_one_2d(kernel):
    # a fine polar grid around the one sample (ring edges at r = h for the compact kernels)
    h = 0.6
    R = (40.0 if kernel in ("gaussian", "exponential") else 1.5) * h
    nr, nt = 30000, 64
    re = np.linspace(0.0, R, nr + 1)
    rm = 0.5 * (re[1:] + re[:-1])
    th = (np.arange(nt) + 0.5) * 2 * np.pi / nt
    pts = np.stack([(rm[:, None] * np.cos(th)[None, :]).ravel(), (rm[:, None] * np.sin(th)[None, :]).ravel()], axis=1)
    p = np.exp(kde_oracle.log_density(np.array([[0.3, -0.2]]), np.ones(1), pts + [0.3, -0.2], kernel, h)[:, 0])
    total = np.sum(p.reshape(nr, nt) * rm[:, None]) * (R / nr) * (2 * np.pi / nt)
    assert abs(total - 1.0) < 1e-6


# ---- KernelDensity parameters ----------------------------------------------------------------------------------------------
def test_kernel_density_parameters(standins):
    kd = amd_kde.KernelDensity()
    assert sorted(kd.get_params()) == sorted(amd_kde.SKLEARN_PARAMS)
    assert kd.get_params()["bandwidth"] == 1.0 and kd.get_params()["kernel"] == "gaussian"
    kd.set_params(kernel="epanechnikov", atol=1e-3, rtol=1e-2, leaf_size=5, breadth_first=False, algorithm="ball_tree")
    X = np.random.RandomState(0).normal(size=(50, 2))
    kd.fit(X)
    # atol / rtol / algorithm ... change nothing: the sum is exact
    np.testing.assert_array_equal(kd.score_samples(X[:5]), kde_oracle.log_density(X, np.ones(50), X[:5], "epanechnikov", 1.0)[:, 0])
    assert kd.score(X[:5]) == pytest.approx(np.sum(kd.score_samples(X[:5])))
    with pytest.raises(ValueError):
        kd.set_params(nonsense=1)
    for bad in (dict(metric="manhattan"), dict(metric_params={"p": 3})):
        with pytest.raises(ParameterError):
            amd_kde.KernelDensity(**bad).fit(X)
    for w in (-np.ones(50), np.full(50, np.nan), np.r_[np.ones(49), np.inf]):
        with pytest.raises(ValueError):
            amd_kde.KernelDensity().fit(X, sample_weight=w)
    with pytest.raises(ValueError):
        amd_kde.KernelDensity(bandwidth=-1.0).fit(X)
    with pytest.raises(ValueError):
        amd_kde.KernelDensity(kernel="triangle").fit(X)
    with pytest.raises(ValueError):
        kd.score_samples(np.zeros((3, 3)))  # wrong dimension
    # zero weights are legal and contribute nothing
    w = np.r_[np.zeros(10), np.ones(40)]
    a = amd_kde.KernelDensity(kernel="gaussian", bandwidth=0.5).fit(X, sample_weight=w).score_samples(X[:7])
    b = amd_kde.KernelDensity(kernel="gaussian", bandwidth=0.5).fit(X[10:]).score_samples(X[:7])
    np.testing.assert_allclose(a, b, rtol=1e-13)


@pytest.mark.parametrize("rule", ["scott", "silverman"])
def test_bandwidth_rules(standins, rule):
    X = np.random.RandomState(1).normal(size=(300, 3))
    kd = amd_kde.KernelDensity(bandwidth=rule).fit(X)
    n, d = X.shape
    want = n ** (-1.0 / (d + 4)) if rule == "scott" else (n * (d + 2) / 4.0) ** (-1.0 / (d + 4))
    assert kd.bandwidth_ == pytest.approx(want, rel=1e-15)
    try:
        from sklearn.neighbors import KernelDensity as SkKD
    except ImportError:
        return
    sk = SkKD(bandwidth=rule).fit(X)
    if hasattr(sk, "bandwidth_"):
        assert kd.bandwidth_ == pytest.approx(sk.bandwidth_, rel=1e-15)


# ---- the FES class on CPU stand-ins ----------------------------------------------------------------------------------------
def test_fes_kde_class_reproduces_reference_1d(standins):
    g = load_golden("fes_kde.npz")
    u = load_golden("fes_umbrella_1d.npz")
    fes = pymbar_amd.FES(u["u_kn"], u["N_k"])
    r = fes.generate_fes(u["u_n"], u["x_n"], fes_type="kde", kde_parameters={"bandwidth": float(g["a_bandwidth"])},
                         n_bootstraps=int(g["a_n_bootstraps"]), seed=int(g["a_seed"]))
    assert "timing" in r
    np.testing.assert_allclose(fes.w_n, g["a_w_n"], rtol=1e-9, atol=1e-15)
    np.testing.assert_allclose(fes.bootstrap_weights[:, 1], np.bincount(g["a_idx1"], weights=fes.w_n, minlength=len(fes.w_n)),
                               rtol=1e-14, atol=0)
    assert fes._w_kn is None  # (no K x N host array unless asked for)
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
        assert nz["df_i"] is None
        # from-normalization with bootstrap (the reference fails on an unbound fmin): the spread, unshifted
        nb = fes.get_fes(q, reference_point="from-normalization", uncertainty_method="bootstrap")
        np.testing.assert_allclose(nb["df_i"], g[f"a_{name}_df_lowest"], rtol=1e-9, atol=1e-9)
    assert fes.get_kde() is fes.kde and fes.get_mbar() is fes.mbar
    with pytest.raises(DataError):
        fes.get_fes(np.zeros((3, 2)))
    np.testing.assert_allclose(fes.w_kn, np.exp(fes.mbar.Log_W_nk))


def test_fes_histogram_class_reproduces_reference(standins):
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
    out = fes.get_fes([e[0] - 1.0, e[-1] + 1.0])  # outside the grid
    assert np.all(np.isnan(out["f_i"])) and "df_i" not in out


def test_fes_input_rules(standins):
    u = load_golden("fes_umbrella_1d.npz")
    fes = pymbar_amd.FES(u["u_kn"], u["N_k"])
    for nb in (1, 2.0, "3"):
        with pytest.raises(ValueError):
            fes.generate_fes(u["u_n"], u["x_n"], fes_type="kde", n_bootstraps=nb)
    with pytest.raises(ParameterError):
        fes.generate_fes(u["u_n"], u["x_n"], fes_type="kde", kde_parameters={"bandwith": 0.1})
    with pytest.raises(ParameterError, match="not supported on this backend"):
        fes.generate_fes(u["u_n"], u["x_n"], fes_type="spline", spline_parameters={})
    with pytest.raises(ParameterError, match="not supported on this backend"):
        fes.generate_fes(u["u_n"], u["x_n"], histogram_parameters={"bin_edges": u["bin_edges"]}, n_bootstraps=2)
    fes.generate_fes(u["u_n"], u["x_n"], histogram_parameters={"bin_edges": u["bin_edges"]})
    for kw in (dict(reference_point="from-normalization"), dict(reference_point="all-differences"),
               dict(uncertainty_method="bootstrap")):
        with pytest.raises(ParameterError, match="not supported on this backend"):
            fes.get_fes([0.0], **kw)
    # a 2-D u_n (K x N layout of the samples' own states) goes through kn_to_n
    K = len(u["N_k"])
    u_kn_layout = np.zeros((K, int(u["N_k"].max())))
    off = 0
    for k, n in enumerate(u["N_k"]):
        u_kn_layout[k, :n] = u["u_n"][off:off + n]
        off += n
    fes.generate_fes(u_kn_layout, u["x_n"], fes_type="kde", kde_parameters={"bandwidth": 0.05})
    np.testing.assert_array_equal(fes.u_n, u["u_n"])


# ---- the long-double oracle and the cases of the instantiation tests (tests/kde_cases.py) ------------------------------------
def _same_pattern(a, b):
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
    np.testing.assert_array_equal(np.isneginf(a), np.isneginf(b))
    assert not np.any(np.isposinf(a)) and not np.any(np.isposinf(b))


@pytest.mark.parametrize("kernel", KERNELS)
def test_long_double_normaliser_matches_quadrature(kernel):
    assert np.finfo(np.longdouble).eps < 1.1e-19  # (the oracle needs the 64-bit mantissa of x87 long double)
    for d in range(1, 9):
        for h in (0.3, 1.0, 2.5):
            assert abs(float(kde_oracle.log_normaliser_ld(kernel, d, h)) - kde_oracle.log_normaliser(kernel, d, h)) < 1e-13
            # the library's own: a few ulps of a value of at most 20 (the cosine recursion in fp64 left 2.3e-13 at d = 8)
            assert abs(float(kde_oracle.log_normaliser_ld(kernel, d, h)) - amd_kde.log_normaliser(kernel, d, h)) < 1e-14


@pytest.mark.parametrize("kernel", KERNELS)
def test_matrix_cases_suit_both_oracles(kernel, capsys):
    """Every case of the device's instantiation matrix: finite input, finite answers where they are meant to be, the float64 and
    the long-double oracle with the same NaN / -inf pattern, and the float64 oracle's scaled error against the long-double one
    (printed: the baseline of profiles/kde_instantiation_matrix.txt) far below the 1e-11 the float64 oracle has been trusted to."""
    worst = 0.0
    for k, d, C in kde_cases.matrix_cases():
        if k != kernel:
            continue
        X, V, Q, h = kde_cases.matrix_case(k, d, C)
        assert X.shape == (197, d) and Q.shape == (259, d) and V.shape == (197, C)
        assert all(np.all(np.isfinite(a)) for a in (X, V, Q)) and np.all(V >= 0)
        assert 0.1 < np.mean(V.max(axis=1) == 0) < 0.3
        L, cond = kde_cases.matrix_oracle(k, d, C)
        L64 = kde_oracle.log_density(X, V, Q, k, h)
        _same_pattern(L64, L)
        live = np.ones(C, dtype=bool)
        if C >= 3:
            live[1] = False
            assert np.all(np.isnan(L[:, 1]))
        assert not np.any(np.isnan(L[:, live]))
        np.testing.assert_array_equal(np.isfinite(L[:, live]), cond[:, live] > 0)
        if k in kde_cases.UNBOUNDED:
            assert np.all(np.isfinite(L[:, live]))  # the far queries too
        else:  # queries with and without a weighted sample inside the support, the far ones without
            assert np.any(np.isfinite(L[:-2, live])) and np.all(np.isneginf(L[-2:, live]))
        err = kde_cases.scaled_error(L64, L)
        with capsys.disabled():
            print(f"\nfloat64-oracle {k:13s} d={d} C={C:2d} scaled error vs long double {err:.3e}", end="")
        worst = max(worst, err)
    assert worst < 1e-12


def test_chunk_ranges_follow_the_host_cut():
    assert kde_oracle.chunk_ranges(197, 1) == [(0, 197)]
    assert kde_oracle.chunk_ranges(197, 2) == [(0, 128), (128, 197)]
    assert kde_oracle.chunk_ranges(197, 3) == [(0, 128), (128, 197)]  # ceil(4 / 3) = 2 tiles per chunk
    assert kde_oracle.chunk_ranges(192, 3) == [(0, 64), (64, 128), (128, 192)]
    assert kde_oracle.chunk_ranges(197, 7) == [(0, 64), (64, 128), (128, 192), (192, 197)]


@pytest.mark.parametrize("kernel", KERNELS)
def test_exact_cases_hold_the_pairs_they_are_built_for(kernel):
    for d in kde_cases.EXACT_DIMS:
        X, V, Q, h = kde_cases.exact_case(kernel, d)
        L, cond = kde_oracle.log_density_ld(X, V, Q, kernel, h)
        _same_pattern(kde_oracle.log_density(X, V, Q, kernel, h), L)
        assert not np.any(np.isnan(L))
        if kernel in kde_cases.UNBOUNDED:
            assert np.all(np.isfinite(L))
            assert np.all(L[:10, 2] < L[:10, 1] - 900 * np.log(2))  # flagged: far below the shared shift
        else:
            assert np.all(np.isneginf(L[:10, 2])) and np.all(np.isneginf(L[20:]))  # zero-weight inside / nothing inside
            assert np.all(np.isfinite(L[:10, 3])) and np.all(cond[:10, 3] >= 1)  # positive sum below 2^-900
            assert np.all(L[:10, 3] < L[:10, 1] + np.log(1e-280))


@pytest.mark.parametrize("kernel", kde_cases.UNBOUNDED)
def test_combine_cases_order_the_chunk_shifts(kernel):
    for order, want in ((("far", "mid", "near"), (0, 1, 2)), (("near", "far", "mid"), (1, 2, 0))):
        X, V, Q, h = kde_cases.combine_case(kernel, order)
        mx = kde_cases.chunk_maxima_doublings(X, Q, kernel, h, 3)
        assert mx.shape == (len(Q), 3)
        lo, mid, hi = (mx[:, i] for i in want)
        assert np.all(hi - lo > 960 + 2 * 256) and np.all(hi - mid > 256) and np.all(hi - mid < 960 - 256) and np.all(mid - lo > 256)
        assert np.all(np.isfinite(kde_oracle.log_density_ld(X, V, Q, kernel, h)[0]))


@pytest.mark.parametrize("kernel", kde_cases.COMPACT)
def test_boundary_cases_sit_on_the_boundary(kernel):
    for name, (X, Q, h) in kde_cases.boundary_cases().items():
        L = kde_oracle.log_density_ld(X, np.ones(1), Q, kernel, h)[0][:, 0]
        _same_pattern(kde_oracle.log_density(X, np.ones(1), Q, kernel, h)[:, 0], L)
        r2 = np.zeros(len(Q))
        for j in range(Q.shape[1]):
            r2 = r2 + Q[:, j] * Q[:, j]
        dist = np.sqrt(r2)
        assert dist[0] == dist[1] and np.isfinite(L[-1])
        if name.endswith("/h"):
            assert dist[0] == h and np.isneginf(L[0]) and np.isneginf(L[1])  # dist == h is outside
            assert np.any(np.isfinite(L[2:-1])) and np.any(np.isneginf(L[2:-1]))  # the neighbours fall on both sides
        elif name.endswith("/h_up"):
            assert dist[0] == np.nextafter(h, 0.0) and np.isfinite(L[0]) and np.isfinite(L[1])  # one ulp inside
        else:
            assert np.isneginf(L[0])


def test_overflow_cases_have_finite_long_double_answers():
    for name, (kernel, X, V, Q, h, far) in kde_cases.overflow_cases().items():
        L = kde_oracle.log_density_ld(X, V, Q, kernel, h)[0]
        assert not np.any(np.isnan(L)) and not np.any(np.isposinf(L))
        near = np.setdiff1d(np.arange(len(Q)), far)
        assert np.all(np.isfinite(L[near]))
        if name == "gaussian-d1":
            assert np.all(np.isneginf(L[far[:2]])) and np.all(np.isfinite(L[far[2]])) and np.all(L[far[2]] < -1e307)
        elif kernel == "gaussian":
            assert np.all(np.isneginf(L[far]))
        else:  # -r / h is inside the float64 range although r^2, or r times the coefficient, is not
            assert np.all(np.isfinite(L[far])) and np.all(L[far] < -1e150)


def test_kde_option_error_paths_without_device():
    from pymbar_amd import _lib

    lib = _lib.load_library()
    assert lib.mbar_kde_set_option(None, b"max_chunks", 2) == -1 and "NULL" in _lib.last_error(None)
    assert lib.mbar_kde_set_option(None, b"max_chunk", 2) == -1 and "unknown kde option" in _lib.last_error(None)
    assert lib.mbar_kde_set_option(None, None, 2) == -1 and "unknown kde option" in _lib.last_error(None)
    assert lib.mbar_kde_set_option(None, b"max_chunks", -1) == -1 and ">= 0" in _lib.last_error(None)
