"""Many observables along a scan (``MBAR.compute_scan_expectations``) on one MI355X, all in ONE process: wall time of the method on
resident observables, means only and with the approximate sigma; kernel ms of the observable pass (``mbar_scan_obs_sums``) from the
library's event timers with the model of DESIGN.md section 24 next to it -- ``2 L Q N`` matrix flop per sum (one sum for the means,
three with sigma), ``L N ceil(Q / 128)`` exponentials per launch mode, the fraction of ``mbar_mfma_f64_peak`` reached, matrix flop
only --; and next to them the only route there was before: ``ceil(Q / 3)`` calls of ``compute_scan(..., uncertainty_method=
"approximate")``, timed in the same run.

The system is the harmonic ladder of tools/bench_histogram.py (K = 128 states generated and solved in HBM); the members are
oscillators with centres across the ladder, in the basis {x^2, x}; observable q is ``(1 + 0.37 q) x`` (the values do not matter to
the time), centred in place and handed to the device without a second host copy.

    python tools/bench_scan_obs.py [--reps 2] [--N 4000000] [--L 128,1024] [--Q 3,64,256,1024] [--loop 2] [--out profiles/scan_observables_bench.txt]

``--loop``: how many of the ``ceil(Q / 3)`` ``compute_scan`` calls of the old route are timed (every one costs the same; the route's
time is reported per call and for all of them)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_histogram import resident_mbar, timed  # noqa: E402
from bench_scan import kernel_ms  # noqa: E402
from pymbar_amd import testsystems as ts  # noqa: E402


def model(L, Q, N, sums):
    """Matrix flop that reach an output, matrix flop issued (whole blocks of 16 observables and of 16 members) and exponentials"""
    panels = [min(128, Q - q0) for q0 in range(0, Q, 128)]
    rows_issued = sum(16 * (1 if p <= 16 else 2 if p <= 32 else 4 if p <= 64 else 8) for p in panels)
    modes = 1 if sums == 1 else 2
    return dict(matrix_flop=2.0 * L * Q * N * sums, matrix_flop_issued=2.0 * (-(-L // 16) * 16) * rows_issued * N * sums,
                exponentials=float(L) * N * len(panels) * modes, observable_panels=len(panels))


def bench_case(m, x, A, O_k, L, Q, reps, loop, peak_tflops):
    dm, N = m._dm, m.N
    O_l = np.linspace(O_k[0], O_k[-1], L)
    K_l = np.full(L, 1.0 / (1.5 * (O_k[1] - O_k[0])) ** 2)
    basis, coeff, offset = ts.harmonic_scan_family(x, O_l, K_l)
    out = dict(K=m.K, N=N, L=L, B=2, Q=Q)
    t0 = time.perf_counter()
    dm.set_scan_observables(A[:Q])  # (centred already; the method's own set_scan_observables would make a second host copy)
    m._scan_obs_shift = np.zeros(Q)
    out["upload_ms"] = 1e3 * (time.perf_counter() - t0)
    dm.set_option("timing", 1)
    dm.set_scan(basis, None)
    f_scan = -dm.scan_lognum(m.f_k, coeff, offset)[0]
    for name, second, sums in (("means", False, 1), ("with_sigma", True, 3)):
        ms = kernel_ms(dm, lambda: dm.scan_obs_sums(m.f_k, coeff, offset, f_scan, second=second), reps)
        mod, med = model(L, Q, N, sums), float(np.median(ms))
        out[name] = dict(obs_kernel_ms=ms, obs_kernel_ms_median=med, **mod, matrix_tflops=mod["matrix_flop"] / (med * 1e-3) / 1e12,
                         fraction_of_mfma_f64_peak=mod["matrix_flop"] / (med * 1e-3) / 1e12 / peak_tflops,
                         issued_fraction_of_mfma_f64_peak=mod["matrix_flop_issued"] / (med * 1e-3) / 1e12 / peak_tflops)
    out["pass_a_kernel_ms"] = kernel_ms(dm, lambda: dm.scan_lognum(m.f_k, coeff, offset), reps)
    dm.set_option("timing", 0)
    dm.set_scan(None)
    out["means"]["method_wall_ms"] = timed(lambda: m.compute_scan_expectations(None, basis, coeff, offset, compute_uncertainty=False), reps)
    out["with_sigma"]["method_wall_ms"] = timed(lambda: m.compute_scan_expectations(None, basis, coeff, offset), reps)
    res = m.compute_scan_expectations(None, basis, coeff, offset)
    # the old route: ceil(Q / 3) calls of compute_scan with three observables each
    calls = -(-Q // 3)
    loop = min(loop, calls)
    rows = [A[3 * i:min(3 * i + 3, Q)] for i in range(loop)]
    old = timed(lambda: [m.compute_scan(basis, coeff, offset, A_qn=a, uncertainty_method="approximate") for a in rows], reps)
    old_means = timed(lambda: [m.compute_scan(basis, coeff, offset, A_qn=a, compute_uncertainty=False) for a in rows], reps)
    one = m.compute_scan(basis, coeff, offset, A_qn=rows[0], uncertainty_method="approximate")
    out["old_route"] = dict(calls=calls, calls_timed=loop, wall_ms_per_call=float(np.median(old)) / loop,
                            wall_ms_for_all=float(np.median(old)) / loop * calls, means_wall_ms_per_call=float(np.median(old_means)) / loop,
                            means_wall_ms_for_all=float(np.median(old_means)) / loop * calls)
    for name, key in (("means", "means_wall_ms_for_all"), ("with_sigma", "wall_ms_for_all")):
        out[name]["method_wall_ms_median"] = float(np.median(out[name]["method_wall_ms"]))
        out[name]["old_route_over_method"] = out["old_route"][key] / out[name]["method_wall_ms_median"]
    nq = len(rows[0])
    out["max_abs_mu_difference_to_old_route"] = float(np.max(np.abs(res["mu"][:nq] - one["mu"])))
    out["max_rel_sigma_difference_to_old_route"] = float(np.max(np.abs(res["sigma"][:nq] / one["sigma"] - 1.0)))
    out["finite"] = bool(np.all(np.isfinite(res["mu"])) and np.all(np.isfinite(res["sigma"])))
    out["min_n_eff"] = float(res["n_eff"].min())
    m.set_scan_observables(None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--N", type=int, default=4000000)
    ap.add_argument("--K", type=int, default=128)
    ap.add_argument("--L", default="128,1024")
    ap.add_argument("--Q", default="3,64,256,1024")
    ap.add_argument("--loop", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_observables_bench.txt"))
    a = ap.parse_args()
    Ls, Qs = [int(v) for v in a.L.split(",")], [int(v) for v in a.Q.split(",")]
    m, x, O_k = resident_mbar(a.K, a.N)
    m.u_kn, m.n_bootstraps = None, 0
    peak = m._dm.mfma_f64_peak()
    A = np.empty((max(Qs), m.N))
    for q in range(len(A)):  # (row by row, in place: the block is the only host copy)
        np.multiply(x, 1.0 + 0.37 * q, out=A[q])
        A[q] -= A[q].sum() / m.N
    print("observables ready", A.shape, file=sys.stderr, flush=True)
    lines = [json.dumps(dict(tool="bench_scan_obs", mfma_f64_peak_tflops=peak))]
    for L in Ls:
        for Q in Qs:
            r = bench_case(m, x, A, O_k, L, Q, a.reps, a.loop, peak)
            lines.append(json.dumps(r))
            print(lines[-1], file=sys.stderr, flush=True)
            with open(a.out, "w") as fh:  # (kept up to date case by case)
                fh.write("\n".join(lines) + "\n")
    m._dm.close()
    print(json.dumps(dict(bench="scan_obs", cases=len(lines) - 1, out=a.out)))


if __name__ == "__main__":
    main()
