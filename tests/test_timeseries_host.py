"""pymbar_amd.timeseries on the CPU: the long-double oracle (tests/timeseries_oracle.py) against the reference's answers
(tests/golden/timeseries.npz, tests/golden/make_golden_timeseries.py), and the whole public module with the device handle replaced
by the oracle's stand-in (``OracleACF`` for ``DeviceACF``): outputs, return types, argument errors, short series and the float32
bookkeeping of ``detect_equilibration``."""
import numpy as np
import pytest

from pymbar_amd import testsystems
from pymbar_amd.utils import ParameterError
from tests import timeseries_oracle as orc
from tests.conftest import load_golden


@pytest.fixture(scope="module")
def gold():
    return load_golden("timeseries.npz")


@pytest.fixture
def ts(monkeypatch):
    from pymbar_amd import timeseries

    monkeypatch.setattr(timeseries, "DeviceACF", orc.OracleACF)
    return timeseries


def _rag(g):
    return [g[f"rag_{k}"] for k in range(5)]


def reference_bookkeeping(T, nskip, g_of):
    """detect_equilibration's loop as the reference writes it, over the given per-origin g (NaN: zero variance)."""
    g_t = np.ones([T - 1], np.float32)
    Neff_t = np.ones([T - 1], np.float32)
    for t in range(0, T - 1, nskip):
        g = g_of[t // nskip]
        g_t[t] = T - t + 1 if np.isnan(g) else g
        Neff_t[t] = (T - t + 1) / g_t[t]
    Neff_max = Neff_t.max()
    t = Neff_t.argmax()
    return t, g_t[t], Neff_max


# ---- the oracle against the fixture ---------------------------------------------------------------------------------------------
def test_oracle_rule_matches_reference_at_sampled_origins(gold):
    ar = gold["ar"]
    for s in (0, 1, 2, 100, 2500, 4990, 4997, 4998):
        g, _, _, _ = orc.rule_trace(ar, s, fast=True, mintime=3)
        assert g == pytest.approx(gold["ar_g_origins"][s], rel=1e-12)


def test_oracle_standin_every_origin_matches_reference(gold):
    for key in ("ar", "tr"):
        x = gold[key]
        g, stop, st = orc.OracleACF(x, shift_a=x.mean()).suffix_g(1, True, 3)
        np.testing.assert_allclose(g, gold[f"{key}_g_origins"], rtol=1e-10)
        assert gold[f"{key}_margin"].min() > 1e-9


def test_correlated_timeseries_example_bit_identical(gold):
    for seed in gold["cte_seeds"]:
        x = testsystems.correlated_timeseries_example(N=2000, tau=5.0, seed=int(seed))
        assert x.dtype == np.float32
        np.testing.assert_array_equal(x, gold[f"cte_{seed}"])


# ---- the public module on the stand-in ------------------------------------------------------------------------------------------
def test_module_logs_long_warning(caplog):
    import importlib

    import pymbar_amd.timeseries as m

    with caplog.at_level("WARNING"):
        importlib.reload(m)
    assert any("timeseries module" in r.getMessage() for r in caplog.records)


def test_package_does_not_import_timeseries():
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import sys, pymbar_amd; print('pymbar_amd.timeseries' in sys.modules)"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, check=True, cwd=root)
    assert r.stdout.strip() == "False"


def test_statistical_inefficiency_variants(ts, gold):
    ar = gold["ar"]
    for fast in (False, True):
        for mt in (0, 3, 10):
            g = ts.statistical_inefficiency(ar, fast=fast, mintime=mt)
            assert isinstance(g, float)
            assert g == pytest.approx(float(gold[f"ar_g_fast{int(fast)}_mt{mt}"]), rel=1e-10)
    assert ts.statistical_inefficiency(gold["trend"]) == pytest.approx(float(gold["trend_g_slow"]), rel=1e-10)
    assert ts.statistical_inefficiency(gold["trend"], fast=True) == pytest.approx(float(gold["trend_g_fast"]), rel=1e-10)
    assert ts.statistical_inefficiency(gold["xa"], gold["xb"]) == pytest.approx(float(gold["x_g_slow"]), rel=1e-10)
    assert ts.statistical_inefficiency(gold["xa"], gold["xb"], fast=True) == pytest.approx(float(gold["x_g_fast"]), rel=1e-10)
    assert ts.integrated_autocorrelation_time(ar) == pytest.approx((float(gold["ar_g_fast0_mt3"]) - 1) / 2, rel=1e-10)


def test_fft_forms(ts, gold):
    assert ts.statistical_inefficiency_fft(gold["ar"]) == pytest.approx(float(gold["ar_g_fft"]), rel=1e-10)
    assert ts.statistical_inefficiency(gold["ar"], fft=True, mintime=10) == pytest.approx(float(gold["ar_g_fft_mt10"]), rel=1e-10)
    assert ts.statistical_inefficiency_fft(gold["trend"]) == pytest.approx(float(gold["trend_g_fft"]), rel=1e-10)
    t, g, ne = ts.detect_equilibration_binary_search(gold["tr"])
    want = gold["tr_bs"]
    assert t == int(want[0])
    assert g == pytest.approx(want[1], rel=1e-10) and ne == pytest.approx(want[2], rel=1e-10)


def test_multiple_and_ct(ts, gold):
    rag = _rag(gold)
    for fast in (False, True):
        g, Ct = ts.statistical_inefficiency_multiple(rag, fast=fast, return_correlation_function=True)
        assert g == pytest.approx(float(gold[f"rag_g_fast{int(fast)}"]), rel=1e-10)
        want = gold[f"rag_ct_fast{int(fast)}"]
        assert isinstance(Ct, list) and len(Ct) == len(want)
        np.testing.assert_array_equal([c[0] for c in Ct], want[:, 0])
        np.testing.assert_allclose([c[1] for c in Ct], want[:, 1], rtol=0, atol=1e-12)
    assert ts.integrated_autocorrelation_timeMultiple(rag) == pytest.approx((float(gold["rag_g_fast0"]) - 1) / 2, rel=1e-10)
    A = np.stack([gold["ar"][:1000], gold["ar"][1000:2000]])
    assert ts.statistical_inefficiency_multiple(A) == pytest.approx(
        ts.statistical_inefficiency_multiple([A[0], A[1]]), rel=0, abs=0)


def test_correlation_functions(ts, gold):
    rag = _rag(gold)
    np.testing.assert_allclose(ts.normalized_fluctuation_correlation_function_multiple(rag, N_max=60), gold["rag_cf"], atol=1e-12)
    got = ts.normalized_fluctuation_correlation_function_multiple(rag, N_max=200, truncate=True)
    assert got.shape == gold["rag_cf_trunc"].shape
    np.testing.assert_allclose(got, gold["rag_cf_trunc"], atol=1e-12)
    np.testing.assert_allclose(ts.normalized_fluctuation_correlation_function_multiple(rag, N_max=40, norm=False),
                               gold["rag_cf_raw"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(ts.normalized_fluctuation_correlation_function(gold["xa"], gold["xb"], N_max=100), gold["x_cf"],
                               atol=1e-12)
    np.testing.assert_allclose(ts.normalized_fluctuation_correlation_function(gold["xa"], gold["xb"], N_max=30, norm=False),
                               gold["x_cf_raw"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(ts.normalized_fluctuation_correlation_function(gold["ar"][:600]), gold["ar_cf_full"], atol=1e-12)


def test_subsample_indices(ts, gold):
    idx = ts.subsample_correlated_data(gold["ar"])
    assert isinstance(idx, list)
    np.testing.assert_array_equal(idx, gold["ar_sub"])
    cons = ts.subsample_correlated_data(gold["ar"], conservative=True)
    assert isinstance(cons, range)
    np.testing.assert_array_equal(list(cons), gold["ar_sub_cons"])
    assert ts.subsample_correlated_data(np.arange(10.0), g=2.5) == [0, 2, 5, 8]


@pytest.mark.parametrize("key,nskip", [("ar", 1), ("ar", 7), ("tr", 1), ("tr", 7), ("trend", 5), ("ct", 1)])
def test_detect_equilibration(ts, gold, key, nskip):
    x = gold[key]
    t, g, ne = ts.detect_equilibration(x, nskip=nskip)
    want = gold[f"{key}_detect_{nskip}"]
    assert t == int(want[0])
    assert np.float32(g) == np.float32(want[1]) and np.float32(ne) == np.float32(want[2])
    assert isinstance(g, np.float32) and isinstance(ne, np.float32)
    # the bookkeeping equals the reference's loop bit for bit, over the same per-origin g
    gs = ts.statistical_inefficiency_suffixes(x, nskip=nskip)
    ref = reference_bookkeeping(x.size, nskip, gs)
    assert (t, g, ne) == ref and type(t) is type(ref[0])


def test_suffixes_constant_tail_is_nan(ts, gold):
    gs = ts.statistical_inefficiency_suffixes(gold["ct"])
    assert np.all(np.isnan(gs[1200:])) and not np.any(np.isnan(gs[:1199]))


# ---- errors and short series ----------------------------------------------------------------------------------------------------
def test_argument_errors(ts):
    with pytest.raises(ParameterError):
        ts.statistical_inefficiency(np.arange(5.0), np.arange(6.0))
    with pytest.raises(ParameterError):
        ts.normalized_fluctuation_correlation_function(np.arange(5.0), np.arange(6.0))
    with pytest.raises(ParameterError):
        ts.normalized_fluctuation_correlation_function_multiple(np.ones((2, 5)))
    with pytest.raises(ParameterError):
        ts.normalized_fluctuation_correlation_function_multiple([np.arange(5.0)], [np.arange(5.0), np.arange(4.0)])
    with pytest.raises(ParameterError):
        ts.normalized_fluctuation_correlation_function_multiple([np.arange(5.0)], [np.arange(4.0)])
    for bad in (np.nan, np.inf):
        x = np.arange(10.0)
        x[3] = bad
        with pytest.raises(ParameterError):
            ts.statistical_inefficiency(x)
        with pytest.raises(ParameterError):
            ts.detect_equilibration(x)
        with pytest.raises(ParameterError):
            ts.statistical_inefficiency_multiple([np.arange(4.0), x])
    with pytest.raises(ParameterError):
        ts.statistical_inefficiency(np.ones(10))


def test_short_series_without_device(monkeypatch):
    from pymbar_amd import timeseries

    def no_device(*a, **k):
        raise AssertionError("the device was touched")

    monkeypatch.setattr(timeseries, "DeviceACF", no_device)
    assert timeseries.detect_equilibration(np.ones(7)) == (0, 1, 1)
    assert timeseries.detect_equilibration(np.array([3.5])) == (0, 1, 1)


def test_two_values_one_origin(ts):
    t, g, ne = ts.detect_equilibration(np.array([0.0, 1.0]))
    assert t == 0 and g == np.float32(1.0) and ne == np.float32(3.0)
    assert ts.statistical_inefficiency(np.array([0.0, 1.0])) == 1.0
    np.testing.assert_array_equal(ts.statistical_inefficiency_suffixes(np.array([0.0, 1.0])), [1.0])
