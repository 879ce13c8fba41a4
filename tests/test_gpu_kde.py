"""Weighted kernel-density sums on the MI355X (``mbar_kde_*``, csrc/mbar_k_kde.hip) against the exact numpy oracle
(tests/kde_oracle.py): every kernel in d = 1, 2, 3, 5, sample / query / column counts on and off the tile sizes, queries far
outside the data, the rescale branch of the running shift forced, zero weights, determinism, one large case, and the whole
``pymbar_amd.FES`` class against the reference's fixtures; then every body of ``k_kde<KER, D, CB>`` and ``k_kde_exact<KER>`` and the
branches of ``k_kde_combine`` on small shapes against the long-double oracle (``kde_oracle.log_density_ld``, cases of
tests/kde_cases.py), the chunk cut chosen through the handle option ``"max_chunks"``."""
import numpy as np
import pytest

import pymbar_amd
from pymbar_amd._lib import MbarHipError
from pymbar_amd.kde import DeviceKDE, KernelDensity
from tests import kde_cases, kde_oracle
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


# ---- every body of k_kde<KER, D, CB>, k_kde_exact<KER> and the branches of k_kde_combine against the long-double oracle --------------
# (cases: tests/kde_cases.py, which also writes out the C -> CB and d -> D mapping; tests/test_kde_host.py checks on the CPU that
# the cases hold what they are built for)
# Bound on |device - long double| / max(1, |long double|) of the instantiation matrix.  MEASURED_MAX is the largest scaled error of
# each kernel over its bodies and both chunk cuts (profiles/kde_instantiation_matrix.txt, written by
# tools/kde_instantiation_matrix.py; the float64 numpy oracle's own error against the long-double one over the same cases is in
# the same file: 2.0e-15 .. 4.7e-14); the bound is TOL_MULTIPLE times it: room for another draw of the same distribution, orders
# of magnitude below a lost term, 50 to 2000 times tighter than the 1e-11 of the float64 comparison above.  (epanechnikov: one
# entry of the d = 8, C = 27 case whose only weighted sample inside the support has 1 - r^2 / h^2 = 6.8e-5, so that an ulp of one
# is 3e-12 of the term -- the float64 oracle has the same 4.7e-14 there; without that entry the kernel is at 2e-15 like the rest.)
TOL_MULTIPLE = 4.0
MEASURED_MAX = {"gaussian": 3.435e-15, "tophat": 1.110e-15, "epanechnikov": 4.910e-14, "exponential": 2.346e-15, "linear": 4.402e-15,
                "cosine": 2.647e-15}
LD_TOL = {k: TOL_MULTIPLE * v for k, v in MEASURED_MAX.items()}
assert max(LD_TOL.values()) <= 1e-11
# The cases outside the matrix (flagged pairs, chunks far apart, the support boundary, overflowing distances) are other
# distributions -- bandwidths of 0.01, a shift up to 256 doublings below a query's largest term -- so their bound is reasoned, not
# measured.  With the shift m that far from the terms that carry the sum: the exp2s argument fma(r, coef, -m) is rounded once at a
# magnitude of up to 2^19 units of 1/2048 doubling, half an ulp of which is 2^-35 units = 9.9e-15 in the natural log, and coef
# carries 2^-53 of the same magnitude (5e-15); the result is m ln2 / 2048 + log(sum), two numbers of up to 177 that cancel to
# order one, each rounded to half an ulp of 177 (1.4e-14 twice), the constant ln2 / 2048 carrying 2^-53 of 177 (2e-14); exp2s
# 3.4e-16, the column sum, the column total and the normaliser a few 1e-16.  That is 6e-14 at the worst against a result of order
# one, and the bound is 1.6 times it.  Every finite entry of the compact cases compared here has a sample with a kernel value
# above 0.7 (an ulp of 1 - r^2 / h^2 is 3e-16 of it).
OTHER_TOL = 1e-13


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _close_ld(dev, ora, kernel, what, tol=None):
    """NaN and -inf patterns exactly, every finite entry within the bound (none excluded); the figure is printed first."""
    assert dev.shape == ora.shape
    err = kde_cases.scaled_error(dev, np.where(np.isfinite(dev), ora, np.nan)) if np.isfinite(ora).any() else 0.0
    print(f"kde-ld {what} scaled_error {err:.3e}")
    np.testing.assert_array_equal(np.isnan(dev), np.isnan(ora))
    np.testing.assert_array_equal(np.isneginf(dev), np.isneginf(ora))
    assert not np.any(np.isposinf(dev))
    tol = LD_TOL[kernel] if tol is None else tol
    assert err <= tol, f"{what}: max scaled error {err:.3e} > {tol:.3e}"
    return err


@pytest.mark.parametrize("kernel,d,C", kde_cases.matrix_cases())
def test_every_body_matches_long_double(kernel, d, C):
    """N = 3 * 64 + 5, M = 256 + 3; max_chunks = 1 carries the four tiles inside one workgroup, 2 merges two chunks.  At one chunk a
    query block evaluated alone (M <= 256) returns the same bits: a query does not depend on its neighbours."""
    X, V, Q, h = kde_cases.matrix_case(kernel, d, C)
    L, _ = kde_cases.matrix_oracle(kernel, d, C)
    with DeviceKDE(X, kernel, h) as dk:
        dk.set_weights(V)
        for mc in (1, 2):
            dk.set_option("max_chunks", mc)
            got = dk.log_density(Q)
            _close_ld(got, L, kernel, f"matrix {kernel} d={d} CB={kde_cases.C_TO_CB[C]} max_chunks={mc}")
            if mc == 1:
                np.testing.assert_array_equal(_bits(dk.log_density(Q[:256])), _bits(got[:256]))
                np.testing.assert_array_equal(_bits(dk.log_density(Q[256:])), _bits(got[256:]))


@pytest.mark.parametrize("kernel,d", [("gaussian", 2), ("exponential", 3), ("gaussian", 8), ("epanechnikov", 4), ("cosine", 1)])
@pytest.mark.parametrize("C", [c for c in kde_cases.C_TO_CB if c > 1])
def test_column_of_a_batch_is_the_column_alone_bit_for_bit(kernel, d, C):
    """The column scale is a power of two and the accumulation order is per column: column c of a C-column call (CB = 4 .. 32)
    equals the same column evaluated at C = 1 (CB = 1) under the same chunk cut, the NaN of a zero-weight column included."""
    X, V, Q, h = kde_cases.matrix_case(kernel, d, C)
    with DeviceKDE(X, kernel, h) as dk:
        for mc in (1, 2):
            dk.set_option("max_chunks", mc)
            dk.set_weights(V)
            full = dk.log_density(Q)
            for c in range(C):
                dk.set_weights(V[:, c])
                np.testing.assert_array_equal(_bits(dk.log_density(Q)[:, 0]), _bits(full[:, c]), err_msg=f"column {c} max_chunks {mc}")


@pytest.mark.parametrize("d", kde_cases.EXACT_DIMS)
@pytest.mark.parametrize("kernel", KERNELS)
def test_flagged_pairs_every_kernel(kernel, d):
    """k_kde_exact<KER>: pairs whose own terms lie more than 900 doublings below the shared shift (the other cluster; weights of
    1e-290 beside a weight of one), and -inf where a compact support holds no sample, or only samples of zero weight."""
    X, V, Q, h = kde_cases.exact_case(kernel, d)
    L, _ = kde_oracle.log_density_ld(X, V, Q, kernel, h)
    with DeviceKDE(X, kernel, h) as dk:
        dk.set_weights(V)
        for mc in (0, 2):
            dk.set_option("max_chunks", mc)
            got = dk.log_density(Q)
            _close_ld(got, L, kernel, f"exact {kernel} d={d} max_chunks={mc}", tol=OTHER_TOL)
    if kernel in kde_cases.UNBOUNDED:
        assert np.all(np.isfinite(got))
    else:
        assert np.all(np.isfinite(got[:10, 3])) and np.all(np.isneginf(got[:10, 2])) and np.all(np.isneginf(got[20:]))


@pytest.mark.parametrize("order", [("far", "mid", "near"), ("near", "far", "mid")])
@pytest.mark.parametrize("kernel", kde_cases.UNBOUNDED)
def test_combine_chunks_far_apart(kernel, order):
    """max_chunks = 3, one tile per chunk: one chunk's shift more than 960 doublings below the largest (k_kde_combine scales it
    in log space), one in between, the largest shift last (every later chunk raises the maximum) or first."""
    X, V, Q, h = kde_cases.combine_case(kernel, order)
    assert kde_oracle.chunk_ranges(len(X), 3) == [(0, 64), (64, 128), (128, 192)]
    mx = kde_cases.chunk_maxima_doublings(X, Q, kernel, h, 3)
    lo, mid, hi = (mx[:, order.index(name)] for name in ("far", "mid", "near"))
    # (a chunk's device shift lies at most 256 doublings below its largest term)
    assert np.all(hi - lo > 960 + 2 * 256) and np.all(hi - mid > 256) and np.all(hi - mid < 960 - 256) and np.all(mid - lo > 256)
    L, _ = kde_oracle.log_density_ld(X, V, Q, kernel, h)
    assert np.all(np.isfinite(L))
    with DeviceKDE(X, kernel, h) as dk:
        dk.set_weights(V)
        for mc in (3, 1):
            dk.set_option("max_chunks", mc)
            _close_ld(dk.log_density(Q), L, kernel, f"combine {kernel} {'-'.join(order)} max_chunks={mc}", tol=OTHER_TOL)


@pytest.mark.parametrize("kernel", kde_cases.COMPACT)
def test_support_boundary_in_several_dimensions(kernel):
    """dist == h exactly ((3, 4) at 5, (1, 2, 2) at 3, (2, 3, 6) at 7, eight +-1 at sqrt(8)), neighbours one ulp and 2^-48 away,
    and the bandwidth one ulp up and down: -inf exactly where the oracle's float64 support test says, finite one ulp inside."""
    for name, (X, Q, h) in kde_cases.boundary_cases().items():
        L = kde_oracle.log_density_ld(X, np.ones(1), Q, kernel, h)[0]
        with DeviceKDE(X, kernel, h) as dk:
            got = dk.log_density(Q)
        np.testing.assert_array_equal(np.isneginf(got), np.isneginf(L), err_msg=name)
        assert not np.any(np.isnan(got)) and not np.any(np.isposinf(got))
        if name.endswith("/h_up"):
            assert np.isfinite(got[0, 0]) and np.isfinite(got[1, 0]), name  # the sample sits one ulp inside
        _close_ld(got[-1:], L[-1:], kernel, f"boundary {kernel} {name} (the query at v / 2)", tol=OTHER_TOL)


@pytest.mark.parametrize("name", list(kde_cases.overflow_cases()))
def test_distance_beyond_the_range_of_the_exponent(name):
    """|q - x|^2, or |q - x| times the exponent's coefficient, overflows float64 for the far queries: the answer is what the long
    double value rounds to (-inf below the range, never NaN), and the near queries of the same waves return the bits of a call
    without the far ones."""
    kernel, X, V, Q, h, far = kde_cases.overflow_cases()[name]
    L, _ = kde_oracle.log_density_ld(X, V, Q, kernel, h)
    with DeviceKDE(X, kernel, h) as dk:
        dk.set_weights(V)
        for mc in (1, 2):
            dk.set_option("max_chunks", mc)
            got = dk.log_density(Q)
            print(f"kde-ld overflow {name} max_chunks={mc} far rows: device {got[far].tolist()} oracle {L[far].tolist()}")
            assert not np.any(np.isnan(got))
            _close_ld(got, L, kernel, f"overflow {name} max_chunks={mc}", tol=OTHER_TOL)
            near = np.delete(np.arange(len(Q)), far)
            np.testing.assert_array_equal(_bits(dk.log_density(Q[near])), _bits(got[near]))


def test_max_chunks_option():
    kernel, d, C = "gaussian", 2, 7
    X, V, Q, h = kde_cases.matrix_case(kernel, d, C)
    L, _ = kde_cases.matrix_oracle(kernel, d, C)
    with DeviceKDE(X, kernel, h) as dk:
        dk.set_weights(V)
        default = dk.log_density(Q)
        seen = {}
        for mc in (1, 2, 7, 1000):  # (four tiles: 7 and 1000 both give one tile per chunk)
            dk.set_option("max_chunks", mc)
            seen[mc] = dk.log_density(Q)
            _close_ld(seen[mc], L, kernel, f"option max_chunks={mc}")
            np.testing.assert_array_equal(_bits(dk.log_density(Q)), _bits(seen[mc]))
        np.testing.assert_array_equal(_bits(seen[7]), _bits(seen[1000]))
        for key, value in (("max_chunk", 1), ("", 1), ("max_chunks", -1)):
            with pytest.raises(MbarHipError):
                dk.set_option(key, value)
        np.testing.assert_array_equal(_bits(dk.log_density(Q)), _bits(seen[1000]))  # (a refused call changes nothing)
        dk.set_option("max_chunks", 0)
        np.testing.assert_array_equal(_bits(dk.log_density(Q)), _bits(default))  # the default cut again: one tile per chunk here
        np.testing.assert_array_equal(_bits(default), _bits(seen[1000]))
