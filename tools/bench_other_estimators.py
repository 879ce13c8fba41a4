"""Throughput of the BAR and EXP estimators (pymbar_amd.other_estimators, csrc/mbar_k_bar.hip) on one MI355X.

    python tools/bench_other_estimators.py [--reps 3] [--quick]

Data: ``gaussian_work_example(DeltaF=1, sigma_F=2, seed=0)`` with N values per side.  Prints ONE JSON line with, per case, the
median ms per call (host clock around the blocking call, after one warm-up call):
  * ``bar_<method>_<N>``: ``bar`` end to end at N = 1e6 and 1e7 per side (upload, bracket, root find, uncertainty), with the
    number of F evaluations (``evals``) and of device passes (``passes``);
  * ``upload_<N>``: creating the handle alone (validation, chunk minima, host-to-device copy);
  * ``eval_<N>``: one ``bar_zero`` pass on a resident handle (launch + sync included);
  * ``batch_127x1e5``: ``bar_batch`` over 127 adjacent pairs of 1e5 values per side;
  * ``exp_1e8``, ``exp_gauss_1e8``: EXP on 1e8 values.
Bounds of one evaluation (ESTIMATES, not measured peaks): fp64 issue at VALU_PER_VALUE instructions per value and request (counted
in the ISA of k_bar_eval: 3090 VALU instructions per 16 values), 5.6 cycles per wave-instruction per SIMD, 1024 SIMDs at 2.4 GHz;
HBM at 8 bytes per value and 6.29 TB/s (measured copy rate).  The kernel time per evaluation comes from a separate
``rocprofv3 --kernel-trace --stats`` run."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VALU_PER_VALUE = 3090 / 16


def issue_bound_values_per_s():
    return 1024 * 2.4e9 / (VALU_PER_VALUE * 5.6 / 64.0)


def hbm_bound_values_per_s():
    return 6.29e12 / 8.0


def timed(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        r = fn()
        ts.append(time.perf_counter() - t0)
    return r, float(np.median(ts)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--quick", action="store_true", help="N = 1e6 only, no 1e8 EXP (for a profiler run)")
    args = ap.parse_args()
    from pymbar_amd import other_estimators as oe
    from pymbar_amd import testsystems

    out = {"bounds_values_per_s": {"fp64_issue": issue_bound_values_per_s(), "hbm": hbm_bound_values_per_s()}}
    sizes = [10**6] if args.quick else [10**6, 10**7]
    for N in sizes:
        w_F, w_R = testsystems.gaussian_work_example(N_F=N, N_R=N, mu_F=None, DeltaF=1.0, sigma_F=2.0, seed=0)
        tag = f"1e{int(round(np.log10(N)))}"
        _, ms = timed(lambda: oe.DeviceBAR([w_F], [w_R]).close(), args.reps)
        out[f"upload_{tag}"] = {"ms": ms}
        with oe.DeviceBAR([w_F], [w_R]) as h:
            _, ms = timed(lambda: h.zero([1.0]), max(args.reps, 10))
            out[f"eval_{tag}"] = {"ms": ms, "values_per_s": 2 * N / (ms * 1e-3)}
        for method in ("false-position", "bisection", "self-consistent-iteration"):
            r, ms = timed(lambda: oe.bar(w_F, w_R, method=method), args.reps)
            with oe.DeviceBAR([w_F], [w_R]) as h:
                st = (oe._lib.BarState * 1)()
                s = st[0]
                s.method, s.iterated, s.maximum_iterations, s.relative_tolerance = oe.METHODS[method], 1, 500, 1e-12
                s.want_moments = 1
                m = h.moments()
                s.UpperB = float(oe._exp_delta_f(m[0, 0, 0], float(N)))
                s.LowerB = float(-oe._exp_delta_f(m[0, 1, 0], float(N)))
                passes = h.solve(st)
            out[f"bar_{method}_{tag}"] = {"ms": ms, "Delta_f": float(r["Delta_f"]), "dDelta_f": float(r["dDelta_f"]),
                                          "evals": int(st[0].nzero), "passes": int(passes)}
    rng = np.random.RandomState(1)
    wF = [rng.randn(10**5) * 2.0 + 2.0 + 0.01 * k for k in range(127)]
    wR = [rng.randn(10**5) * 2.0 - 2.0 for k in range(127)]
    r, ms = timed(lambda: oe.bar_batch(wF, wR), args.reps)
    out["batch_127x1e5"] = {"ms": ms, "ms_per_pair": ms / 127}
    if not args.quick:
        del wF, wR
        w = np.random.RandomState(2).randn(10**8) * 2.0 + 3.0
        _, ms = timed(lambda: oe.exp(w), args.reps)
        out["exp_1e8"] = {"ms": ms}
        _, ms = timed(lambda: oe.exp_gauss(w), args.reps)
        out["exp_gauss_1e8"] = {"ms": ms}
    e = out.get("eval_1e7", out.get("eval_1e6"))
    out["eval_fraction_of_issue_bound"] = e["values_per_s"] / issue_bound_values_per_s()
    out["binding_bound"] = "fp64_issue"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
