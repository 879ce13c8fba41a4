"""Reweighting scans over a linear family (``MBAR.compute_scan``) on one MI355X, all in ONE process: kernel ms of pass A
(``mbar_scan_lognum``) and pass B (``mbar_scan_gram_w``, cross block on the fp64 matrix cores) from the library's event timers
(``mbar_ctx_timing``), pass B's achieved matrix flop/s -- ``2 K L J N`` over its kernel time -- against ``mbar_mfma_f64_peak``
measured in the same run, and at L = 128 the only baseline there is: ``compute_perturbed_free_energies`` on the materialised
``u_ln`` (wall time of the whole call, the upload of the L rows included, next to the whole ``compute_scan`` call).  At larger L
the dense path cannot run: the rows alone need ``8 L N`` bytes (80 GB at L = 1000, N = 1e7).

The system is the harmonic ladder of tools/bench_histogram.py (K = 128 states generated and solved in HBM); the family are
oscillators with centres across the ladder in the basis {x^2, x}; the observables, with Q = 2, are x and x^2.

    python tools/bench_scan.py [--reps 3] [--N 4000000,10000000] [--L 128,1024,8192]"""
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
from pymbar_amd import testsystems as ts  # noqa: E402


def kernel_ms(dm, fn, reps):
    fn()  # warm-up (also leaves logden(f_k) in place: the timed calls run the scan kernels only)
    out = []
    for _ in range(reps):
        dm.timing_reset()
        fn()
        out.append(dm.timing()["other"][0])
    return out


def bench_shape(m, x, O_k, L, Q, reps, peak_tflops, dense):
    K, N = m.K, m.N
    dm = m._dm
    O_l = np.linspace(O_k[0], O_k[-1], L)
    K_l = np.full(L, 1.0 / (1.5 * (O_k[1] - O_k[0])) ** 2)
    basis, coeff, offset = ts.harmonic_scan_family(x, O_l, K_l)
    A = np.stack([x, x * x])[:Q]
    t = A - (A.min(axis=1) - 1e-3)[:, None] if Q else None
    J = 1 + Q
    dm.set_scan(basis, t)
    dm.set_option("timing", 1)
    lognum, _ = dm.scan_lognum(m.f_k, coeff, offset)
    a_ms = kernel_ms(dm, lambda: dm.scan_lognum(m.f_k, coeff, offset), reps)
    b_ms = kernel_ms(dm, lambda: dm.scan_gram_w(m.f_k, coeff, offset, -lognum), reps)
    dm.set_option("timing", 0)
    dm.set_scan(None)
    b_med = float(np.median(b_ms))
    flop = 2.0 * K * L * J * N
    out = dict(K=K, N=N, L=L, Q=Q, pass_a_kernel_ms=a_ms, pass_b_kernel_ms=b_ms, pass_a_kernel_ms_median=float(np.median(a_ms)),
               pass_b_kernel_ms_median=b_med, pass_b_matrix_flop=flop, pass_b_tflops=flop / (b_med * 1e-3) / 1e12,
               pass_b_fraction_of_mfma_f64_peak=flop / (b_med * 1e-3) / 1e12 / peak_tflops)
    whole = timed(lambda: m.compute_scan(basis, coeff, offset, A_qn=A if Q else None), reps)
    out["compute_scan_wall_ms"] = whole
    if dense:
        u_ln = coeff @ basis + offset[:, None]
        d = timed(lambda: m.compute_perturbed_free_energies(u_ln), max(1, reps - 1))
        res, ref = m.compute_scan(basis, coeff, offset), m.compute_perturbed_free_energies(u_ln)
        out.update(dense_perturbed_wall_ms=d, dense_u_ln_bytes=int(u_ln.nbytes),
                   max_abs_Delta_f_difference=float(np.max(np.abs(res["Delta_f"] - ref["Delta_f"][0]))),
                   max_rel_dDelta_f_difference=float(np.max(np.abs(res["dDelta_f"][1:] / ref["dDelta_f"][0][1:] - 1.0))))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--N", default="4000000,10000000")
    ap.add_argument("--L", default="128,1024,8192")
    ap.add_argument("--K", type=int, default=128)
    a = ap.parse_args()
    out = dict(bench="scan", shapes=[])
    for N in [int(v) for v in a.N.split(",")]:
        m, x, O_k = resident_mbar(a.K, N)
        m.u_kn, m.n_bootstraps = None, 0
        peak = m._dm.mfma_f64_peak()
        out.setdefault("mfma_f64_peak_tflops", []).append(peak)
        for L in [int(v) for v in a.L.split(",")]:
            for Q in (0, 2):
                r = bench_shape(m, x, O_k, L, Q, a.reps, peak, dense=(L <= 128 and Q == 0))
                out["shapes"].append(r)
                print(json.dumps(r), file=sys.stderr, flush=True)
        m._dm.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
