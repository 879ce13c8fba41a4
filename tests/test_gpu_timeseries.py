"""pymbar_amd.timeseries on the MI355X: the device lag sums and stopping rule against the long-double oracle
(tests/timeseries_oracle.py; accuracy contract |C_dev - C_exact| <= 1e-14 at every (origin, lag) pair the rule evaluates), the
public module against the reference's answers (tests/golden/timeseries.npz), the reference's own test assertions restated,
determinism, and one T = 1e7 equilibration detection.  The seam cases put origins, segment boundaries and lag blocks on and around
the tile boundary (ACF_TILE = 2048 positions) in both forms (auto, and cross with its second accumulator), run schedules of up to
727 lags (lag blocks of 8, 16, 32 and 64; tiles from the first running origin's on) and a constant tail."""
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


def check_origins(ts, a, origins, nskip, fast=True, mintime=3, b=None, fft=False, stats=None):
    """device rule and raw sums at the given origins (multiples of nskip) against the oracle's term-by-term rule; returns the
    number of origins whose trace is empty (rule checked, no lag sums to compare).  ``stats``: a dict that takes the worst
    figures (tools/hist_acf_branch_matrix.py)."""
    skipped = 0
    stats = {} if stats is None else stats
    a64 = np.asarray(a, dtype=np.float64)
    b64 = None if b is None else np.asarray(b, dtype=np.float64)
    with ts.DeviceACF(a64, b64, shift_a=a64.mean(), shift_b=0.0 if b is None else b64.mean()) as dev:
        g, stop, st = dev.suffix_g(nskip, fast, mintime, fft)
        for s in origins:
            o = s // nskip
            gw, stw, sw, trace = orc.rule_trace(a64, s, fast and not fft, mintime, fft=fft, b=b64)
            assert st[o] == sw, (s, st[o], sw)
            assert stop[o] == stw, (s, stop[o], stw)
            assert g[o] == pytest.approx(gw, rel=1e-12, abs=0), s
            stats["g"] = max(stats.get("g", 0.0), abs(g[o] - gw) / gw)
            stats["lags"] = max(stats.get("lags", 0), len(trace))
            if not trace:
                skipped += 1
                continue
            lags = np.array([0] + [t for t, _ in trace])
            xab, xba = dev.lag_sums(lags, [s])
            N = a64.size - s
            sig2 = xab[0, 0] / N
            for k, (t, Cx) in enumerate(trace, start=1):
                Cd = (xab[k, 0] + xba[k, 0]) / (2.0 * (N - t) * sig2)
                assert abs(Cd - float(Cx)) <= C_TOL, (s, t, Cd, float(Cx))
                stats["C"] = max(stats.get("C", 0.0), abs(Cd - float(Cx)))
    return skipped


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


# ---- tile seams, the second accumulator, long schedules, constant tails ----------------------------------------------------------
def seam_pair(T):
    a = ar1(T, 4, T) + 0.25
    return a, 0.7 * a + 0.7 * ar1(T, 4, T + 1) - 1.5


def seam_origins(T):
    return sorted({s for s in (0, 1, 2046, 2047, 2048, 4095, 4096, 4097, T - 40, T - 10, T - 3, T - 2) if 0 <= s < T - 1})


@pytest.mark.parametrize("T", [2047, 2048, 2049, 4500])
@pytest.mark.parametrize("fast", [False, True])
def test_cross_form_over_tile_seams(ts, T, fast):
    a, b = seam_pair(T)
    origins = seam_origins(T)
    thirds = [s for s in origins if s % 3 == 0]
    skipped = check_origins(ts, a, origins, 1, fast=fast, b=b)
    assert 6 * skipped <= len(origins)  # (only T - 2 has no lag to evaluate)
    assert check_origins(ts, a, thirds, 3, fast=fast, b=b) <= skipped  # the same origins again, as every third one


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("cross", [False, True])
def test_long_schedules(ts, seed, cross):
    """65 to 727 lags per origin: the rule's lag blocks of 8, 16, 32 and 64, several 64-lag blocks of lag_sums, and origins in the
    second tile (no tile before the first running origin's is summed)"""
    a = ar1(4500, 150, seed)
    b = 0.7 * a + 0.7 * ar1(4500, 150, seed + 10) if cross else None
    origins = [0, 2047, 2048, 3000]
    n_lags = [len(orc.rule_trace(a, s, False, 3, b=b)[3]) for s in (0, 3000)]
    assert min(n_lags) > ACF_MAX_LAGS
    assert check_origins(ts, a, origins, 1, fast=False, b=b) == 0


ACF_MAX_LAGS = 64


def assert_lag_sums(dev, ora, lags, origins, cross):
    """the contract of C, per (origin, lag) and accumulator: |x_dev - x_exact| <= C_TOL (N - t) sigma^2; exact zeros from t = N on"""
    T = dev.T
    xab, xba = dev.lag_sums(lags, origins)
    wab, wba = ora.lag_sums(lags, origins)
    var, _ = ora.lag_sums([0], origins)
    if not cross:
        assert xba.tobytes() == xab.tobytes()
    worst = 0.0
    for j, t in enumerate(lags):
        for i, s in enumerate(origins):
            N = T - s
            if t >= N:
                assert xab[j, i] == 0.0 and xba[j, i] == 0.0, (s, t)
                continue
            scale = (N - t) * abs(var[0, i]) / N
            if scale == 0.0:  # (an origin with one value left)
                assert xab[j, i] == 0.0 and xba[j, i] == 0.0, (s, t)
                continue
            worst = max(worst, abs(xab[j, i] - wab[j, i]) / scale, abs(xba[j, i] - wba[j, i]) / scale)
            assert abs(xab[j, i] - wab[j, i]) <= C_TOL * scale and abs(xba[j, i] - wba[j, i]) <= C_TOL * scale, (s, t)
    print("lag_sums: worst |x_dev - x_exact| / ((N - t) sigma^2) =", worst)
    return xab, xba


@pytest.mark.parametrize("cross", [False, True])
def test_lag_sums_blocks_and_first_tile(ts, cross):
    T = 4500
    a, b = seam_pair(T)
    b = b if cross else None
    rng = np.random.RandomState(6)
    lags = np.concatenate([[0, T - 1, T, 2 * T, 1, 2047, 2048, 2049, 2451, 2452], rng.choice(np.arange(2, 4400), 140, replace=False)])
    lags = lags[rng.permutation(lags.size)]
    assert lags.size == 150
    kw = dict(shift_a=a.mean(), shift_b=0.0 if b is None else b.mean())
    with ts.DeviceACF(a, b, **kw) as dev, orc.OracleACF(a, b, **kw) as ora:
        for origins in ([2048, 2049, 4499], [0, 2047, 2048, 4499]):
            first = assert_lag_sums(dev, ora, lags, origins, cross)
            again = dev.lag_sums(lags, origins)
            assert all(x.tobytes() == y.tobytes() for x, y in zip(first, again))


SEAM_SEGMENTS = [2048, 1, 2047, 2, 402]  # boundaries on a tile seam, lengths 1 and 2


@pytest.mark.parametrize("cross", [False, True])
def test_segment_sums_on_tile_seams(ts, cross):
    a, b = seam_pair(4500)
    b = b if cross else None
    kw = dict(seg=SEAM_SEGMENTS, shift_a=a.mean(), shift_b=0.0 if b is None else b.mean())
    starts = np.concatenate([[0], np.cumsum(SEAM_SEGMENTS)[:-1]])
    lags = np.array([0, 1, 2, 401, 402, 2046, 2047, 2048, 5000])
    with ts.DeviceACF(a, b, **kw) as dev, orc.OracleACF(a, b, **kw) as ora:
        xab, xba = dev.lag_sums(lags, starts, segments=True)
        wab, wba = ora.lag_sums(lags, starts, segments=True)
        np.testing.assert_allclose(xab, wab, rtol=1e-13, atol=1e-10)
        np.testing.assert_allclose(xba, wba, rtol=1e-13, atol=1e-10)  # (cross: the second accumulator's segment differences)
        if cross:
            assert np.max(np.abs(wab - wba)[1:3]) > 1e-3  # the two accumulators differ: xba is not a copy of xab
        else:
            assert xba.tobytes() == xab.tobytes()
        for j, t in enumerate(lags):  # a lag at or beyond a segment's length: exact zero
            for i, L in enumerate(SEAM_SEGMENTS):
                if t >= L:
                    assert xab[j, i] == 0.0 and xba[j, i] == 0.0, (t, L)
        again = dev.lag_sums(lags, starts, segments=True)
        assert again[0].tobytes() == xab.tobytes() and again[1].tobytes() == xba.tobytes()


@pytest.mark.parametrize("fast", [False, True])
def test_segment_rule_on_tile_seams(ts, fast):
    a = ar1(4500, 20, 5)
    mu = a.sum() / a.size
    with ts.DeviceACF(a, seg=SEAM_SEGMENTS, shift_a=mu) as dev, orc.OracleACF(a, seg=SEAM_SEGMENTS, shift_a=mu) as ora:
        g, stop, st, ct = dev.multiple_g(fast, 3, want_ct=True)
        gw, stw, sw, ctw = ora.multiple_g(fast, 3, want_ct=True)
        print("segment rule: stop", stw, "status", sw, "g", gw)
        assert sw == ts.STOPPED and stw > 24  # (past the lag blocks of 8 and 16)
        assert (stop, st) == (stw, sw)
        assert g == pytest.approx(gw, rel=1e-12)
        n_eval = sum(1 for t, _ in ts.lag_schedule(fast, max(SEAM_SEGMENTS) - 1) if t <= stop)
        np.testing.assert_allclose(ct[1:n_eval + 1], ctw[1:n_eval + 1], rtol=0, atol=C_TOL)
        again = dev.multiple_g(fast, 3, want_ct=True)
        assert (again[0], again[1], again[2]) == (g, stop, st) and again[3].tobytes() == ct.tobytes()


@pytest.mark.parametrize("T", [2049, 4500])
@pytest.mark.parametrize("cross", [False, True])
def test_fft_rule_over_tile_seams(ts, T, cross):
    a, b = seam_pair(T)
    assert check_origins(ts, a, seam_origins(T), 1, fast=False, b=b if cross else None, fft=True) == 0


@pytest.mark.parametrize("fast", [False, True])
def test_constant_tail(ts, fast):
    a = ar1(300, 4, 9)
    a[200:] = a[200]
    with ts.DeviceACF(a, shift_a=a.mean()) as dev, orc.OracleACF(a, shift_a=a.mean()) as ora:
        g, stop, st = dev.suffix_g(1, fast, 3)
        gw, stw, sw = ora.suffix_g(1, fast, 3)
    np.testing.assert_array_equal(st, sw)
    np.testing.assert_array_equal(stop, stw)
    np.testing.assert_allclose(g, gw, rtol=1e-12, atol=0)
    assert np.all(st[200:] == ts.ZERO_VARIANCE) and np.all(g[200:] == 1.0) and np.all(st[:200] != ts.ZERO_VARIANCE)


def test_constant_series_and_two_values(ts):
    for a in (np.full(50, 1.75), np.full(2, -3.0), np.full(2049, 0.1), np.array([1.0, 2.0])):
        with ts.DeviceACF(a, shift_a=a.mean()) as dev, orc.OracleACF(a, shift_a=a.mean()) as ora:
            g, stop, st = dev.suffix_g(1, True, 3)
            gw, stw, sw = ora.suffix_g(1, True, 3)
            np.testing.assert_array_equal(st, sw)
            np.testing.assert_array_equal(stop, stw)
            np.testing.assert_array_equal(g, gw)
            if a[0] == a[-1]:
                assert np.all(st == ts.ZERO_VARIANCE) and np.all(g == 1.0) and np.all(stop == 0)
                xab, _ = dev.lag_sums([0, 1], [0])
                assert np.all(np.abs(xab) <= 1e-28)  # (a - mean is held exactly as hi + lo)
    assert (int(st[0]), int(stop[0]), float(g[0])) == (ts.END, 1, 1.0)  # T = 2, two values: no lag to evaluate


def test_cross_rule_bits(ts):
    a, b = seam_pair(4500)
    with ts.DeviceACF(a, b, shift_a=a.mean(), shift_b=b.mean()) as dev:
        first = dev.suffix_g(1, False, 3)
        again = dev.suffix_g(1, False, 3)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(first, again))
