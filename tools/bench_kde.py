"""Throughput of the weighted kernel-density sum (pymbar_amd.kde.DeviceKDE, csrc/mbar_k_kde.hip) on one MI355X.

    python tools/bench_kde.py [--n 10000000] [--m 4096] [--reps 5] [--sklearn-n 100000 --sklearn-m 200]

Gaussian kernel, N samples, M queries, d = 1, 2, 3, C = 1 and C = 21 weight columns (one pass per call: 21 columns run in the
24-column body).  Prints ONE JSON line: per case the median ms per call (host clock around the blocking call, after one
warm-up call), pairs/s, pair-columns/s and the fraction of the instruction-count bound of DESIGN.md ("Kernel-density
surfaces"): fp64 VALU instructions per pair F = 2 d + 10 + CB at 5.6 cycles per wave-instruction per SIMD, 32-bit VALU
instructions I = 4 at 2 cycles, 1024 SIMDs at 2.4 GHz (an estimate, not a measured peak).  With sklearn importable it also
times sklearn.neighbors.KernelDensity(...).score_samples on the CPU at a reduced size (one thread, the reference's defaults)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def bound_pairs_per_s(d, cb):
    fp64, i32 = 2 * d + 10 + cb, 4
    cycles_per_pair_per_simd = (fp64 * 5.6 + i32 * 2.0) / 64.0
    return 1024 * 2.4e9 / cycles_per_pair_per_simd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--m", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sklearn-n", type=int, default=100_000)
    ap.add_argument("--sklearn-m", type=int, default=200)
    a = ap.parse_args()
    from pymbar_amd import _lib
    from pymbar_amd.kde import DeviceKDE

    rng = np.random.RandomState(0)
    out = dict(tool="bench_kde", kernel="gaussian", N=a.n, M=a.m, cases=[])
    for d in (1, 2, 3):
        X = rng.normal(size=(a.n, d))
        Q = rng.normal(scale=1.2, size=(a.m, d))
        h = 0.05
        with DeviceKDE(X, "gaussian", h) as dk:
            for C in (1, 21):
                V = rng.uniform(size=(a.n, C)) if C > 1 else np.ones((a.n, 1))
                dk.set_weights(V)
                dk.log_density(Q)  # warm-up
                _lib.load_library().mbar_device_synchronize(dk.device)
                ts = []
                for _ in range(a.reps):
                    t0 = time.perf_counter()
                    L = dk.log_density(Q)  # (blocking: the results are on the host when it returns)
                    ts.append(time.perf_counter() - t0)
                ms = 1e3 * float(np.median(ts))
                pairs = float(a.n) * a.m
                cb = 1 if C == 1 else 24
                rate = pairs / (ms * 1e-3)
                out["cases"].append(dict(d=d, C=C, pass_width=cb, ms=round(ms, 3), ms_all=[round(1e3 * t, 3) for t in ts],
                                         pairs_per_s=rate, pair_columns_per_s=rate * C,
                                         bound_pairs_per_s=bound_pairs_per_s(d, cb), fraction_of_bound=rate / bound_pairs_per_s(d, cb),
                                         finite=bool(np.all(np.isfinite(L)))))
                del V
    try:
        from sklearn.neighbors import KernelDensity as SkKD
    except ImportError:
        out["sklearn"] = "not importable"
    else:
        sk = []
        for d in (1, 2):
            X = rng.normal(size=(a.sklearn_n, d))
            Q = rng.normal(size=(a.sklearn_m, d))
            kd = SkKD(bandwidth=0.05).fit(X, sample_weight=rng.uniform(size=a.sklearn_n))
            t0 = time.perf_counter()
            kd.score_samples(Q)
            t = time.perf_counter() - t0
            sk.append(dict(d=d, N=a.sklearn_n, M=a.sklearn_m, s=round(t, 3), pairs_per_s=a.sklearn_n * a.sklearn_m / t))
        out["sklearn"] = sk
    print(json.dumps(out))


if __name__ == "__main__":
    main()
