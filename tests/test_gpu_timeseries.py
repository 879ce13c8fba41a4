"""pymbar_amd.timeseries on the MI355X: the device lag sums and stopping rule against the long-double oracle
(tests/timeseries_oracle.py; accuracy contract |C_dev - C_exact| <= 1e-14 at every (origin, lag) pair the rule evaluates), the
public module against the reference's answers (tests/golden/timeseries.npz), the reference's own test assertions restated,
determinism, and one T = 1e7 equilibration detection."""
import numpy as np
import pytest

from pymbar_amd import testsystems
from tests import timeseries_oracle as orc
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
C_TOL = 1e-14


@pytest.fixture(scope="module")
def ts():
    from pymbar_amd import timeseries

    return timeseries


@pytest.fixture(scope="module")
def gold():
    return load_golden("timeseries.npz")


def ar1(T, tau, seed):
    rng = np.random.RandomState(seed)
    rho = np.exp(-1.0 / tau)
    e = rng.normal(size=T)
    x = np.empty(T)
    x[0] = e[0]
    for n in range(1, T):
        x[n] = rho * x[n - 1] + np.sqrt(1 - rho * rho) * e[n]
    return x


def check_origins(ts, a, origins, nskip, fast=True, mintime=3, b=None):
    """device rule and raw sums at the given origins (multiples of nskip) against the oracle's term-by-term rule."""
    a64 = np.asarray(a, dtype=np.float64)
    b64 = None if b is None else np.asarray(b, dtype=np.float64)
    with ts.DeviceACF(a64, b64, shift_a=a64.mean(), shift_b=0.0 if b is None else b64.mean()) as dev:
        g, stop, st = dev.suffix_g(nskip, fast, mintime)
        for s in origins:
            o = s // nskip
            gw, stw, sw, trace = orc.rule_trace(a64, s, fast, mintime, b=b64)
            assert st[o] == sw, (s, st[o], sw)
            assert stop[o] == stw, (s, stop[o], stw)
            assert g[o] == pytest.approx(gw, rel=1e-12, abs=0), s
            if not trace:
                continue
            lags = np.array([0] + [t for t, _ in trace])
            xab, xba = dev.lag_sums(lags, [s])
            N = a64.size - s
            sig2 = xab[0, 0] / N
            for k, (t, Cx) in enumerate(trace, start=1):
                Cd = (xab[k, 0] + xba[k, 0]) / (2.0 * (N - t) * sig2)
                assert abs(Cd - float(Cx)) <= C_TOL, (s, t, Cd, float(Cx))


# ---- device against the oracle --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [2, 3, 4, 5, 17, 2047, 2048, 2049, 4500])
@pytest.mark.parametrize("nskip", [1, 3, "big"])
def test_rule_and_sums_against_oracle(ts, T, nskip):
    a = ar1(T, 4.0, seed=T) + 0.25
    ns = T + 5 if nskip == "big" else nskip
    origins = np.arange(0, T - 1, ns)
    if origins.size > 40:
        origins = np.unique(np.concatenate([origins[:8], origins[-8:], np.random.RandomState(1).choice(origins, 24)]))
    check_origins(ts, a, origins, ns)


def test_float32_input(ts, gold):
    x = gold["cte_1"]
    assert x.dtype == np.float32
    check_origins(ts, x, [0, 1, 500, 1990, 1997], 1)
    g = ts.statistical_inefficiency(x)
    assert g == pytest.approx(orc.rule_trace(x.astype(np.float64), 0, False, 3)[0], rel=1e-12)


def test_cross_form(ts, gold):
    xa, xb = gold["xa"][:1500], gold["xb"][:1500]
    check_origins(ts, xa, [0, 3, 700, 1490], 1, fast=False, b=xb)


@pytest.mark.parametrize("fast", [False, True])
def test_ragged_segments(ts, gold, fast):
    rag = [gold[f"rag_{k}"] for k in range(5)]
    a = np.concatenate(rag)
    N_k = [x.size for x in rag]
    mu = a.sum() / a.size
    with ts.DeviceACF(a, seg=N_k, shift_a=mu) as dev, orc.OracleACF(a, seg=N_k, shift_a=mu) as ora:
        g, stop, st, ct = dev.multiple_g(fast, 10, want_ct=True)
        gw, stw, sw, ctw = ora.multiple_g(fast, 10, want_ct=True)
        assert (stop, st) == (stw, sw)
        assert g == pytest.approx(gw, rel=1e-12)
        n_eval = sum(1 for t, _ in ts.lag_schedule(fast, max(N_k) - 1) if t < stop or (t == stop and st == ts.STOPPED))
        np.testing.assert_allclose(ct[1:n_eval + 1], ctw[1:n_eval + 1], rtol=0, atol=C_TOL)
        starts = np.concatenate([[0], np.cumsum(N_k)[:-1]])
        lags = np.array([0, 1, 2, 5, 999, 1000, 1001, 4999, 5000])
        xab, _ = dev.lag_sums(lags, starts, segments=True)
        xw, _ = ora.lag_sums(lags, starts, segments=True)
        np.testing.assert_allclose(xab, xw, rtol=1e-13, atol=1e-10)


def test_adversarial_transient(ts, gold):
    tr = gold["tr"]
    origins = [0, 1, 299, 598, 599, 600, 601, 1500, 2990, 2997]
    check_origins(ts, tr, origins, 1)


# ---- against the reference's fixture --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["ar", "tr"])
def test_every_origin_against_reference(ts, gold, key):
    g = ts.statistical_inefficiency_suffixes(gold[key])
    np.testing.assert_allclose(g, gold[f"{key}_g_origins"], rtol=1e-10, atol=0)


@pytest.mark.parametrize("key,nskip", [("ar", 1), ("ar", 7), ("tr", 1), ("tr", 7), ("trend", 5), ("ct", 1)])
def test_detect_equilibration_against_reference(ts, gold, key, nskip):
    t, g, ne = ts.detect_equilibration(gold[key], nskip=nskip)
    want = gold[f"{key}_detect_{nskip}"]
    assert t == int(want[0])
    assert np.float32(g) == np.float32(want[1]) and np.float32(ne) == np.float32(want[2])


def test_module_against_reference(ts, gold):
    ar = gold["ar"]
    for fast in (False, True):
        for mt in (0, 3, 10):
            assert ts.statistical_inefficiency(ar, fast=fast, mintime=mt) == pytest.approx(
                float(gold[f"ar_g_fast{int(fast)}_mt{mt}"]), rel=1e-10)
    assert ts.statistical_inefficiency(gold["trend"]) == pytest.approx(float(gold["trend_g_slow"]), rel=1e-10)
    assert ts.statistical_inefficiency(gold["xa"], gold["xb"]) == pytest.approx(float(gold["x_g_slow"]), rel=1e-10)
    assert ts.statistical_inefficiency(gold["xa"], gold["xb"], fast=True) == pytest.approx(float(gold["x_g_fast"]), rel=1e-10)
    np.testing.assert_array_equal(ts.subsample_correlated_data(ar), gold["ar_sub"])
    np.testing.assert_array_equal(list(ts.subsample_correlated_data(ar, conservative=True)), gold["ar_sub_cons"])
    rag = [gold[f"rag_{k}"] for k in range(5)]
    for fast in (False, True):
        g, Ct = ts.statistical_inefficiency_multiple(rag, fast=fast, return_correlation_function=True)
        assert g == pytest.approx(float(gold[f"rag_g_fast{int(fast)}"]), rel=1e-10)
        want = gold[f"rag_ct_fast{int(fast)}"]
        np.testing.assert_array_equal([c[0] for c in Ct], want[:, 0])
        np.testing.assert_allclose([c[1] for c in Ct], want[:, 1], rtol=0, atol=1e-12)
    np.testing.assert_allclose(ts.normalized_fluctuation_correlation_function_multiple(rag, N_max=60), gold["rag_cf"], atol=1e-12)
    got = ts.normalized_fluctuation_correlation_function_multiple(rag, N_max=200, truncate=True)
    assert got.shape == gold["rag_cf_trunc"].shape
    np.testing.assert_allclose(got, gold["rag_cf_trunc"], atol=1e-12)
    np.testing.assert_allclose(ts.normalized_fluctuation_correlation_function_multiple(rag, N_max=40, norm=False),
                               gold["rag_cf_raw"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(ts.normalized_fluctuation_correlation_function(gold["xa"], gold["xb"], N_max=100), gold["x_cf"],
                               atol=1e-12)
    np.testing.assert_allclose(ts.normalized_fluctuation_correlation_function(ar[:600]), gold["ar_cf_full"], atol=1e-12)


def test_fft_and_binary_search_against_reference(ts, gold):
    assert ts.statistical_inefficiency_fft(gold["ar"]) == pytest.approx(float(gold["ar_g_fft"]), rel=1e-10)
    assert ts.statistical_inefficiency(gold["ar"], fft=True, mintime=10) == pytest.approx(float(gold["ar_g_fft_mt10"]), rel=1e-10)
    assert ts.statistical_inefficiency_fft(gold["trend"]) == pytest.approx(float(gold["trend_g_fft"]), rel=1e-10)
    t, g, ne = ts.detect_equilibration_binary_search(gold["tr"])
    want = gold["tr_bs"]
    assert t == int(want[0])
    assert g == pytest.approx(want[1], rel=1e-10) and ne == pytest.approx(want[2], rel=1e-10)


# ---- the reference's own timeseries test assertions, restated --------------------------------------------------------------------
def test_fft_against_direct(ts):
    for seed in (0, 1, 2):
        x = testsystems.correlated_timeseries_example(N=10000, tau=5.0, seed=seed)
        g0 = ts.statistical_inefficiency(x, fast=False, fft=False)
        g1 = ts.statistical_inefficiency(x, fast=False, fft=True)
        np.testing.assert_almost_equal(g0, g1, decimal=6)
        g2 = ts.statistical_inefficiency_fft(x)
        np.testing.assert_almost_equal(g1, g2, decimal=5)


def test_white_noise_and_repeat(ts):
    x = np.random.RandomState(5).normal(size=50000)
    assert abs(np.log(ts.statistical_inefficiency(x))) < 0.1
    y = np.repeat(x[:20000], 3)
    assert abs(np.log(ts.statistical_inefficiency(y)) - np.log(3.0)) < 0.1


def test_determinism(ts, gold):
    a = ts.statistical_inefficiency_suffixes(gold["tr"])
    b = ts.statistical_inefficiency_suffixes(gold["tr"])
    assert a.tobytes() == b.tobytes()
    rag = [gold[f"rag_{k}"] for k in range(5)]
    c1 = ts.normalized_fluctuation_correlation_function_multiple(rag, N_max=60)
    c2 = ts.normalized_fluctuation_correlation_function_multiple(rag, N_max=60)
    assert c1.tobytes() == c2.tobytes()


def test_large_detect_equilibration(ts):
    T = 10_000_000
    rng = np.random.RandomState(3)
    rho = np.exp(-1.0 / 10.0)
    e = rng.normal(size=T) * np.sqrt(1 - rho * rho)
    from scipy.signal import lfilter

    x = lfilter([1.0], [1.0, -rho], e)
    x[:200_000] += np.linspace(20.0, 0.0, 200_000)
    g = ts.statistical_inefficiency_suffixes(x)
    assert g.shape == (T - 1,)
    t, gt, ne = ts.detect_equilibration(x)
    assert 100_000 < t < 400_000 and np.isfinite(ne)
    origins = np.unique(np.concatenate([T - 2 - np.arange(0, 64 * 3000, 3000)[:48],
                                        np.random.RandomState(4).randint(T - 1_000_000, T - 200_000, 16)]))
    for s in origins:
        gw, stw, sw, _ = orc.rule_trace(x, int(s), True, 3)
        assert g[s] == pytest.approx(gw, rel=1e-12), s
