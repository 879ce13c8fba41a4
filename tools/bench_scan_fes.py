"""Histogram free energy surfaces along a scan (``MBAR.compute_scan_fes``) on one MI355X, all in ONE process: kernel ms of pass A
(``mbar_scan_bin_lognum``) and pass B (``mbar_scan_bin_gram_w``, the gathered cross block on the fp64 matrix cores) from the
library's event timers (``mbar_ctx_timing``), the wall time of the whole ``compute_scan_fes`` call with analytical uncertainties,
and at L = 128 the only baseline there is: the loop of ``histogram_fes_labels`` over the same members (every member builds its
dense ``u_l``, uploads it, rebuilds the chunk table and reads the resident matrix once), in the same run.

The system is the harmonic ladder of tools/bench_histogram.py (K = 128 states generated and solved in HBM); the family is a sweep
of a restraint centre across the ladder in the basis {x^2, x}; the bins are 100 quantile bins of the sample coordinate, or the
populated cells of a 50 x 50 grid over it and a second coordinate localised per state (2-D umbrella sampling).  On the grid the
whole call is timed at L = 128 only: the host side of the bordered covariance holds the K x L x nbins cross block (2.6 GB at L =
1024), which is not what this tool measures.

    python tools/bench_scan_fes.py [--reps 3] [--N 4000000,10000000] [--L 128,1024]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_histogram import quantile_labels, resident_mbar, timed  # noqa: E402
from bench_scan import kernel_ms  # noqa: E402
from pymbar_amd import fes as amd_fes  # noqa: E402
from pymbar_amd import testsystems as ts  # noqa: E402


def grid_labels(x, O_k, side, rng):
    K, N = len(O_k), len(x)
    state = np.repeat(np.arange(K), N // K)
    y = O_k[(state * 37) % K] + rng.normal(0.0, 1.5 * (O_k[1] - O_k[0]), N)
    labels = quantile_labels(x, side) * side + quantile_labels(y, side)
    _, labels = np.unique(labels, return_inverse=True)  # (the populated cells, numbered)
    return labels.astype(np.int64)


def bench_shape(m, x, O_k, labels, tag, L, reps, whole, loop):
    K, N = m.K, m.N
    dm = m._dm
    nbins = int(labels.max()) + 1
    O_l = np.linspace(O_k[0], O_k[-1], L)
    K_l = np.full(L, 1.0 / (1.5 * (O_k[1] - O_k[0])) ** 2)
    basis, coeff, offset = ts.harmonic_scan_family(x, O_l, K_l)
    slab = max(1, min(L, dm.SCAN_BIN_CROSS_BYTES // (8 * K * nbins)))
    dm.set_scan(basis, None)
    t0 = time.perf_counter()
    dm.set_scan_bins(nbins, labels)
    set_bins_s = time.perf_counter() - t0
    dm.set_option("timing", 1)
    lognum = dm.scan_bin_lognum(m.f_k, coeff, offset)
    a_ms = kernel_ms(dm, lambda: dm.scan_bin_lognum(m.f_k, coeff, offset), reps)
    # pass B by slabs of the wrapper, without the host copy of the whole cross block: kernel time of all slabs of one call
    def pass_b():
        for l0 in range(0, L, slab):
            dm.scan_bin_gram_w(m.f_k, coeff[l0:l0 + slab], offset[l0:l0 + slab], -lognum[l0:l0 + slab], slab=slab)
    b_ms = kernel_ms(dm, pass_b, reps)
    dm.set_option("timing", 0)
    dm.set_scan_bins(0)
    dm.set_scan(None)
    out = dict(K=K, N=N, L=L, bins=tag, nbins=nbins, set_scan_bins_s=set_bins_s, members_per_slab=slab, pass_a_kernel_ms=a_ms,
               pass_b_kernel_ms=b_ms, pass_a_kernel_ms_median=float(np.median(a_ms)), pass_b_kernel_ms_median=float(np.median(b_ms)))
    res = None
    if whole:
        def call():
            nonlocal res
            res = m.compute_scan_fes(basis, coeff, offset, sample_label=labels, uncertainty_method="analytical")
        if nbins < 1000:
            out["compute_scan_fes_wall_ms"] = timed(call, reps)
        else:  # (tens of seconds of host algebra on the K x L x nbins cross block: one call, no warm-up)
            t0 = time.perf_counter()
            call()
            out["compute_scan_fes_wall_ms"] = [1e3 * (time.perf_counter() - t0)]
        t0 = time.perf_counter()
        m.compute_scan_fes(basis, coeff, offset, sample_label=labels)
        out["compute_scan_fes_no_uncertainty_wall_ms"] = [1e3 * (time.perf_counter() - t0)]
    if loop:
        t0 = time.perf_counter()
        rows = [amd_fes.histogram_fes_labels(m, coeff[l] @ basis + offset[l], labels) for l in range(L)]
        out["label_path_loop_wall_ms"] = [1e3 * (time.perf_counter() - t0)]
        t0 = time.perf_counter()
        for l in range(L):
            amd_fes.histogram_fes_labels(m, coeff[l] @ basis + offset[l], labels, uncertainty_method=None)
        out["label_path_loop_no_uncertainty_wall_ms"] = [1e3 * (time.perf_counter() - t0)]
        df = np.array([r["df_i"] for r in rows])
        off = np.arange(nbins)[None, :] != res["reference"][:, None]
        out.update(max_abs_f_i_difference=float(np.max(np.abs(res["f_i"] - np.array([r["f_i"] for r in rows])))),
                   max_rel_df_i_difference=float(np.max(np.abs(res["df_i"][off] / df[off] - 1.0))))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--N", default="4000000,10000000")
    ap.add_argument("--L", default="128,1024")
    ap.add_argument("--K", type=int, default=128)
    a = ap.parse_args()
    out = dict(bench="scan_fes", shapes=[])
    for N in [int(v) for v in a.N.split(",")]:
        m, x, O_k = resident_mbar(a.K, N)
        m.u_kn, m.n_bootstraps = None, 0
        rng = np.random.default_rng(2)
        for tag, labels in (("100 bins in one dimension", quantile_labels(x, 100)), ("50 x 50 grid localised per state", grid_labels(x, O_k, 50, rng))):
            for L in [int(v) for v in a.L.split(",")]:
                r = bench_shape(m, x, O_k, labels, tag, L, a.reps, whole=(L <= 128 or labels.max() < 1000), loop=(L <= 128))
                out["shapes"].append(r)
                print(json.dumps(r), file=sys.stderr, flush=True)
        m._dm.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
