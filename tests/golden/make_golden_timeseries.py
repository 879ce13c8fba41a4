"""Writes tests/golden/timeseries.npz: pymbar.timeseries answers of the unmodified reference on seeded series.

    PYTHONPATH=<reference checkout> python3 tests/golden/make_golden_timeseries.py

Series: an AR(1) in float64 (T = 5000, ``ar``), ``correlated_timeseries_example`` float32 outputs with seeds (``cte_<seed>``), a
large transient (mean offset 1e3 sigma over the first 20 %, ``tr``), a slow linear trend (the correlation function stays above
zero for long lags, ``trend``), a tail of exact zeros (``ct``; the reference also takes its zero-variance path), K = 5 ragged
series of 1000 .. 5000 values (``rag_<k>``) and a cross pair (``xa``, ``xb``).  Float32 series are handed to the reference
promoted to float64 (the project's documented deviation: it takes the mean in fp64).

For every origin of the per-origin arrays the generator also records the smallest |C| met in a stop test (``C <= 0 and t >
mintime``) and requires it to exceed 1e-9, so that rounding cannot flip a stop decision.

statsmodels is not importable next to numpy 1.26 here, so the reference's own ``statistical_inefficiency_fft`` and
``detect_equilibration_binary_search`` run against a small ``statsmodels.api`` stand-in injected into ``sys.modules``: its
``tsa.stattools.acf(x, fft=True, adjusted=True, nlags)`` uses numpy's FFT and the documented formula (autocovariance at lag t
divided by N - t, over the one at lag 0).
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "refshim"))


def _acf(x, adjusted=False, nlags=None, fft=True, **kw):
    x = np.asarray(x, dtype=np.float64)
    n = x.size
    d = x - x.mean()
    m = 1 << int(np.ceil(np.log2(2 * n - 1)))
    f = np.fft.rfft(d, m)
    acov = np.fft.irfft(f * np.conj(f), m)[:n]
    if adjusted:
        acov = acov / (n - np.arange(n))
    else:
        acov = acov / n
    nl = n - 1 if nlags is None else min(int(nlags), n - 1)
    return acov[:nl + 1] / acov[0]


def _install_statsmodels():
    sm = types.ModuleType("statsmodels")
    api = types.ModuleType("statsmodels.api")
    api.tsa = types.SimpleNamespace(stattools=types.SimpleNamespace(acf=_acf))
    sm.api = api
    sys.modules["statsmodels"] = sm
    sys.modules["statsmodels.api"] = api


def ar1(T, tau, seed):
    rng = np.random.RandomState(seed)
    rho = np.exp(-1.0 / tau)
    e = rng.normal(size=T)
    x = np.empty(T)
    x[0] = e[0]
    for n in range(1, T):
        x[n] = rho * x[n - 1] + np.sqrt(1 - rho * rho) * e[n]
    return x


def stop_margin(a, s, fast, mintime):
    """smallest |C| over the stop tests of origin s (float64 restatement; inf if there is none)."""
    x = a[s:] - a[s:].mean()
    N = x.size
    sig2 = np.dot(x, x) / N
    if sig2 == 0:
        return np.inf
    t, inc, m = 1, 1, np.inf
    while t < N - 1:
        C = np.dot(x[:N - t], x[t:]) / ((N - t) * sig2)
        if t > mintime:
            m = min(m, abs(C))
            if C <= 0:
                break
        t += inc
        if fast:
            inc += 1
    return m


def main():
    _install_statsmodels()
    from pymbar import timeseries as ts
    from pymbar.testsystems import timeseries as tsys
    from pymbar.utils import ParameterError

    out = {}
    # ---- correlated_timeseries_example, float32 recurrence
    for seed in (1, 7):
        out[f"cte_{seed}"] = tsys.correlated_timeseries_example(N=2000, tau=5.0, seed=seed)
    out["cte_seeds"] = np.array([1, 7])
    # ---- AR(1), float64, every origin
    ar = ar1(5000, 8.0, seed=11)
    out["ar"] = ar
    T = ar.size
    g_or = np.array([ts.statistical_inefficiency(ar[t:], fast=True) for t in range(T - 1)])
    out["ar_g_origins"] = g_or
    out["ar_margin"] = np.array([stop_margin(ar, t, True, 3) for t in range(T - 1)])
    for nskip in (1, 7):
        t, g, ne = ts.detect_equilibration(ar, fast=True, nskip=nskip)
        out[f"ar_detect_{nskip}"] = np.array([t, g, ne], dtype=np.float64)
    for fast in (False, True):
        for mt in (0, 3, 10):
            out[f"ar_g_fast{int(fast)}_mt{mt}"] = np.float64(ts.statistical_inefficiency(ar, fast=fast, mintime=mt))
    idx = ts.subsample_correlated_data(ar)
    out["ar_sub"] = np.array(idx)
    out["ar_sub_cons"] = np.array(list(ts.subsample_correlated_data(ar, conservative=True)))
    out["ar_g_fft"] = np.float64(ts.statistical_inefficiency_fft(ar))
    out["ar_g_fft_mt10"] = np.float64(ts.statistical_inefficiency_fft(ar, mintime=10))
    # ---- large transient: 1e3 sigma over the first 20 %
    tr = ar1(3000, 5.0, seed=23)
    tr[:600] += 1.0e3
    out["tr"] = tr
    out["tr_g_origins"] = np.array([ts.statistical_inefficiency(tr[t:], fast=True) for t in range(tr.size - 1)])
    out["tr_margin"] = np.array([stop_margin(tr, t, True, 3) for t in range(tr.size - 1)])
    for nskip in (1, 7):
        t, g, ne = ts.detect_equilibration(tr, fast=True, nskip=nskip)
        out[f"tr_detect_{nskip}"] = np.array([t, g, ne], dtype=np.float64)
    t, g, ne = ts.detect_equilibration_binary_search(tr)
    out["tr_bs"] = np.array([t, g, ne], dtype=np.float64)
    # ---- slow linear trend
    trend = ar1(2000, 3.0, seed=31) + np.linspace(0.0, 6.0, 2000)
    out["trend"] = trend
    out["trend_g_slow"] = np.float64(ts.statistical_inefficiency(trend))
    out["trend_g_fast"] = np.float64(ts.statistical_inefficiency(trend, fast=True))
    out["trend_g_fft"] = np.float64(ts.statistical_inefficiency_fft(trend))
    out["trend_g_origins"] = np.array([ts.statistical_inefficiency(trend[t:], fast=True) for t in range(0, trend.size - 1, 5)])
    out["trend_margin"] = np.array([stop_margin(trend, t, True, 3) for t in range(0, trend.size - 1, 5)])
    t, g, ne = ts.detect_equilibration(trend, fast=True, nskip=5)
    out["trend_detect_5"] = np.array([t, g, ne], dtype=np.float64)
    # ---- constant (exactly representable) tail
    ct = ar1(1500, 4.0, seed=41)
    ct[1200:] = 0.0
    out["ct"] = ct
    t, g, ne = ts.detect_equilibration(ct, fast=True, nskip=1)
    out["ct_detect_1"] = np.array([t, g, ne], dtype=np.float64)
    try:
        ts.statistical_inefficiency(ct[1300:])
        raise AssertionError("the reference should raise on the constant tail")
    except ParameterError:
        pass
    # ---- ragged multiple series
    N_k = [1000, 2000, 3000, 4000, 5000]
    rag = [ar1(n, 6.0, seed=50 + k) for k, n in enumerate(N_k)]
    for k, x in enumerate(rag):
        out[f"rag_{k}"] = x
    for fast in (False, True):
        g, Ct = ts.statistical_inefficiency_multiple(rag, fast=fast, return_correlation_function=True)
        out[f"rag_g_fast{int(fast)}"] = np.float64(g)
        out[f"rag_ct_fast{int(fast)}"] = np.array(Ct, dtype=np.float64)
    out["rag_cf"] = ts.normalized_fluctuation_correlation_function_multiple(rag, N_max=60)
    out["rag_cf_trunc"] = ts.normalized_fluctuation_correlation_function_multiple(rag, N_max=200, truncate=True)
    out["rag_cf_raw"] = ts.normalized_fluctuation_correlation_function_multiple(rag, N_max=40, norm=False)
    # ---- cross pair
    xa = ar1(4000, 6.0, seed=61)
    xb = 0.6 * xa + 0.8 * ar1(4000, 3.0, seed=62) + 2.5
    out["xa"], out["xb"] = xa, xb
    out["x_g_slow"] = np.float64(ts.statistical_inefficiency(xa, xb))
    out["x_g_fast"] = np.float64(ts.statistical_inefficiency(xa, xb, fast=True))
    out["x_cf"] = ts.normalized_fluctuation_correlation_function(xa, xb, N_max=100)
    out["x_cf_raw"] = ts.normalized_fluctuation_correlation_function(xa, xb, N_max=30, norm=False)
    out["ar_cf_full"] = ts.normalized_fluctuation_correlation_function(ar[:600])
    for key in ("ar_margin", "tr_margin", "trend_margin"):
        m = out[key]
        assert np.all(m > 1e-9), (key, m.min())
    np.savez_compressed(os.path.join(HERE, "timeseries.npz"), **out)
    print("wrote timeseries.npz:", os.path.getsize(os.path.join(HERE, "timeseries.npz")), "bytes")


if __name__ == "__main__":
    main()
