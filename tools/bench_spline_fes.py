"""Spline free energy surfaces on one MI355X: the moment upload and kernel, generate_fes (unbiasedstate and biasedstates,
Newton-CG, nspline 10, cubic) and Monte Carlo steps, at N = 7e3, 7e5 and 7e6 on the 1-D umbrella system of
tests/golden/make_golden_fes.py (7 states, K0 = 20, Ku = 100), and the host data-term cost the moments replace: one
scipy BSpline(t, c, k)(x_n) over the samples.  Prints one JSON line.

    python tools/bench_spline_fes.py [--sizes 7000,700000,7000000] [--mc-steps 500]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pymbar_amd  # noqa: E402
from pymbar_amd.bspline import DeviceBSplineMoments  # noqa: E402

CENTERS, K0, KU = 0.2 * np.arange(-3, 4), 20.0, 100.0


def umbrella(N, seed=0):
    rng = np.random.default_rng(seed)
    n = N // len(CENTERS)
    x = np.concatenate([rng.normal(c * KU / (K0 + KU), np.sqrt(1.0 / (K0 + KU)), n) for c in CENTERS])
    u_n = 0.5 * K0 * x ** 2
    u_kn = np.stack([u_n + 0.5 * KU * (x - c) ** 2 for c in CENTERS])
    return x, u_n, u_kn, np.full(len(CENTERS), n)


def params(weights):
    return dict(spline_weights=weights, nspline=10, kdegree=3, xrange=[-0.7, 0.7], optimization_algorithm="Newton-CG",
                spline_initialize="zeros", optimize_options={"disp": False, "tol": 1e-7},
                fkbias=[lambda x, c=c: (KU / 2.0) * (x - c) ** 2 for c in CENTERS])


def main():
    from scipy.interpolate import BSpline

    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="7000,700000,7000000")
    ap.add_argument("--mc-steps", type=int, default=500)
    a = ap.parse_args()
    out = dict(bench="spline_fes", sizes={})
    for N in [int(s) for s in a.sizes.split(",")]:
        x, u_n, u_kn, N_k = umbrella(N)
        r = {}
        t = np.r_[[-0.7] * 3, np.linspace(-0.7, 0.7, 8), [0.7] * 3]
        g = np.repeat(np.arange(7), N_k)
        t0 = time.perf_counter()
        dev = DeviceBSplineMoments(x, groups=g, n_groups=7)
        r["upload_ms"] = 1e3 * (time.perf_counter() - t0)
        dev.moments(t, 3)  # (warm-up)
        ks, ws = [], []
        for _ in range(20):
            t0 = time.perf_counter()
            dev.moments(t, 3)
            ws.append(1e3 * (time.perf_counter() - t0))
            ks.append(dev.kernel_ms())
        dev.close()
        r["moment_kernel_ms_median"] = float(np.median(ks))
        r["moment_call_ms_median"] = float(np.median(ws))
        r["moment_kernel_GBps"] = (N * (8 + 4 + 8)) / (r["moment_kernel_ms_median"] * 1e-3) / 1e9
        c = np.linspace(0.0, 1.0, 10)
        hs = []
        for _ in range(3):
            t0 = time.perf_counter()
            BSpline(t, c, 3)(x)
            hs.append(1e3 * (time.perf_counter() - t0))
        r["host_bspline_eval_ms"] = float(np.median(hs))
        fes = pymbar_amd.FES(u_kn, N_k)
        for w in ("unbiasedstate", "biasedstates"):
            t0 = time.perf_counter()
            fes.generate_fes(u_n, x, fes_type="spline", spline_parameters=params(w))
            r[f"generate_fes_{w}_s"] = time.perf_counter() - t0
            np.random.seed(1)
            t0 = time.perf_counter()
            fes.sample_parameter_distribution(x, mc_parameters=dict(niterations=a.mc_steps, sample_every=10), decorrelate=False,
                                              verbose=False)
            r[f"mc_{w}_ms_per_step"] = 1e3 * (time.perf_counter() - t0) / a.mc_steps
            r[f"mc_{w}_acceptance"] = fes.get_mc_data()["acceptance_ratio"]
        fes.mbar.close() if hasattr(fes.mbar, "close") else None
        out["sizes"][str(N)] = r
        print(json.dumps({str(N): r}), file=sys.stderr)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
