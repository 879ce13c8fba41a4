"""Throughput of the timeseries lag sums (pymbar_amd.timeseries, csrc/mbar_k_acf.hip) on one MI355X.

    python tools/bench_timeseries.py [--reps 3] [--cases detect_1e5,detect_1e6,detect_1e7,si_1e7,multiple]

Cases, on seeded AR(1) data: ``detect_equilibration(nskip=1)`` at T = 1e5, 1e6, 1e7 (correlation time 10, a linear transient over
the first 2 %), ``statistical_inefficiency(fast=False)`` at T = 1e7 with tau = 1000, and ``statistical_inefficiency_multiple`` on
K = 128 series of 1e5.  Prints ONE JSON line: per case the median ms per call (host clock around the blocking call, upload and
handle creation included, after one warm-up call) and the pair-products per second.  Pair-products are counted as the reference's
loops form them: sum over the evaluated (origin, lag) pairs of the number of products, N - t.

For the two single-origin cases (si_1e7, multiple) that is also what the device sweeps, and the line gives the fraction of an
instruction-count bound (an ESTIMATE, not a measured peak): F = 12 fp64 VALU instructions per product in k_acf_tiles (TwoProduct
with the two cross terms 4, compensated accumulation 8) at 5.6 cycles per wave-instruction per SIMD (the cost DESIGN.md uses for
the KDE bound), 1024 SIMDs at 2.4 GHz; block reductions, scans and the rule kernel are not counted.  For detect_equilibration the
device sweeps each lag once for all origins, so the reference-equivalent rate is not bounded by that estimate and no fraction is
given."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

F_PER_PAIR = 12


def bound_pairs_per_s():
    return 1024 * 2.4e9 / (F_PER_PAIR * 5.6 / 64.0)


def ar1(T, tau, seed):
    from scipy.signal import lfilter

    rho = np.exp(-1.0 / tau)
    e = np.random.RandomState(seed).normal(size=T) * np.sqrt(1 - rho * rho)
    return lfilter([1.0], [1.0, -rho], e)


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append(time.perf_counter() - t0)
    return r, ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", default="detect_1e5,detect_1e6,detect_1e7,si_1e7,multiple")
    a = ap.parse_args()
    from pymbar_amd import timeseries as ts

    out = dict(tool="bench_timeseries", bound_note="instruction-count ESTIMATE of k_acf_tiles, F = %d fp64 per product" % F_PER_PAIR,
               bound_pairs_per_s=bound_pairs_per_s(), cases=[])
    for case in a.cases.split(","):
        if case.startswith("detect_"):
            T = int(float(case.split("_")[1]))
            x = ar1(T, 10.0, seed=1)
            x[: T // 50] += np.linspace(20.0, 0.0, T // 50)
            r, tt = timed(lambda: ts.detect_equilibration(x, nskip=1), a.reps)
            with ts.DeviceACF(x, shift_a=x.mean()) as dev:
                g, stop, st = dev.suffix_g(1, True, 3)
            lags = np.array([t for t, _ in ts.lag_schedule(True, T)], dtype=np.int64)
            csum = np.concatenate([[0], np.cumsum(lags)])
            k = np.searchsorted(lags, stop, side="right")  # evaluated lags: <= stop (stopped by the test) or < stop (ran out)
            k = np.where(st == ts.END, np.searchsorted(lags, stop, side="left"), k)
            N = T - np.arange(stop.size)
            ref_pairs = float(np.sum(k * N - csum[k]))
            res = dict(t=int(r[0]), g=float(r[1]), Neff=float(r[2]), g_median=float(np.median(g)),
                       reference_pair_products=ref_pairs)
            pairs = None
        elif case == "si_1e7":
            T = 10_000_000
            x = ar1(T, 1000.0, seed=2)
            r, tt = timed(lambda: ts.statistical_inefficiency(x, fast=False), a.reps)
            with ts.DeviceACF(x, shift_a=x.mean()) as dev:
                _, stop, _ = dev.suffix_g(T, False, 3)
            res = dict(g=float(r), stop_lag=int(stop[0]))
            pairs = float(T) * float(stop[0])
        elif case == "multiple":
            A = [ar1(100_000, 10.0, seed=10 + k) for k in range(128)]
            r, tt = timed(lambda: ts.statistical_inefficiency_multiple(A), a.reps)
            with ts.DeviceACF(np.concatenate(A), seg=[100_000] * 128, shift_a=np.concatenate(A).mean()) as dev:
                _, stop, _, _ = dev.multiple_g(False, 10)
            res = dict(g=float(r), stop_lag=int(stop))
            pairs = 128e5 * float(stop)
        else:
            raise SystemExit(f"unknown case {case}")
        ms = 1e3 * float(np.median(tt))
        row = dict(case=case, ms=round(ms, 3), ms_all=[round(1e3 * t, 3) for t in tt], **res)
        if pairs is None:
            row.update(reference_pairs_per_s=res["reference_pair_products"] / (ms * 1e-3))
        else:
            rate = pairs / (ms * 1e-3)
            row.update(pair_products=pairs, pairs_per_s=rate, fraction_of_bound_estimate=rate / bound_pairs_per_s())
        out["cases"].append(row)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
