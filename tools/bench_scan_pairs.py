"""Differences between any two members of a scan (``MBAR.compute_scan_pairs``) on one MI355X, all in ONE process: kernel ms of the
pair pass (``mbar_scan_pair_gram``) from the library's event timers with the model of DESIGN.md section 23 next to it -- ``2 R L J^2
N`` matrix flop, the exponentials of the (row panel, member panel) launches, the fraction of ``mbar_mfma_f64_peak`` reached, matrix
flop only --, the wall time of the method for 64 scattered reference members and for all pairs, and next to them the only route
there was before: one ``compute_scan(reference=r)`` per reference member, timed in the same run.

The system is the harmonic ladder of tools/bench_histogram.py (K = 128 states generated and solved in HBM); the members are
oscillators with centres across the ladder, in the basis {x^2, x}.

    python tools/bench_scan_pairs.py [--reps 3] [--N 4000000] [--L 1024] [--R 64] [--loop 64] [--out profiles/scan_pairs_bench.txt]

``--loop``: how many of the R ``compute_scan`` calls of the old route are timed (every one costs the same; the route's time is
reported per call and for all R)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_histogram import resident_mbar, timed  # noqa: E402
from bench_scan import kernel_ms  # noqa: E402
from pymbar_amd import testsystems as ts  # noqa: E402
from pymbar_amd.scan import _shifted  # noqa: E402


def panels(R, J):
    """``[(nb, reference members)]`` of the row panels of a call (mbar_scan_pair_gram)"""
    out = []
    while R > 0:
        nb = 2 if R <= 32 // J else 8
        rm = min(R, 16 * nb // J)
        out.append((nb, rm))
        R -= rm
    return out


def model(R, L, J, N, mb):
    """Matrix flop that reach an output, matrix flop issued (whole row panels, whole member blocks) and exponentials"""
    pw = 64 * mb
    mpanels = [min(pw, L - p0) for p0 in range(0, L, pw)]
    issued = sum(2.0 * 16 * nb * (-(-pl // 16) * 16) * J * N for nb, _ in panels(R, J) for pl in mpanels)
    exps = sum((rm + pl) * float(N) for _, rm in panels(R, J) for pl in mpanels)
    return dict(matrix_flop=2.0 * R * L * J * J * N, matrix_flop_issued=issued, exponentials=exps, row_panels=len(panels(R, J)),
                member_panels=len(mpanels))


def bench_case(m, x, O_k, L, R, Q, reps, loop, peak_tflops):
    dm, N = m._dm, m.N
    J = 1 + Q
    O_l = np.linspace(O_k[0], O_k[-1], L)
    K_l = np.full(L, 1.0 / (1.5 * (O_k[1] - O_k[0])) ** 2)
    basis, coeff, offset = ts.harmonic_scan_family(x, O_l, K_l)
    A = np.stack([x])[:Q] if Q else None
    scattered = np.sort(np.random.default_rng(L).permutation(L)[:R]).astype(np.int64)
    out = dict(K=m.K, N=N, L=L, B=2, Q=Q, J=J)
    dm.set_option("timing", 1)
    dm.set_scan(basis, None if A is None else _shifted(A)[0])
    f_scan = -dm.scan_lognum(m.f_k, coeff, offset)[0]
    mb = {1: 4, 2: 2}.get(J, 1)
    for name, rows in (("scattered", scattered), ("all", np.arange(L, dtype=np.int64))):
        ms = kernel_ms(dm, lambda: dm.scan_pair_gram(m.f_k, coeff, offset, f_scan, rows), reps)
        mod = model(len(rows), L, J, N, mb)
        med = float(np.median(ms))
        out[name] = dict(R=len(rows), pair_kernel_ms=ms, pair_kernel_ms_median=med, **mod,
                         matrix_tflops=mod["matrix_flop"] / (med * 1e-3) / 1e12,
                         fraction_of_mfma_f64_peak=mod["matrix_flop"] / (med * 1e-3) / 1e12 / peak_tflops,
                         issued_fraction_of_mfma_f64_peak=mod["matrix_flop_issued"] / (med * 1e-3) / 1e12 / peak_tflops)
    out["pass_b_one_reference_kernel_ms"] = kernel_ms(dm, lambda: dm.scan_gram_w(m.f_k, coeff, offset, f_scan, reference=0), reps)
    dm.set_option("timing", 0)
    dm.set_scan(None)
    out["scattered"]["method_wall_ms"] = timed(lambda: m.compute_scan_pairs(basis, coeff, offset, A_qn=A, reference_members=scattered), reps)
    out["all"]["method_wall_ms"] = timed(lambda: m.compute_scan_pairs(basis, coeff, offset, A_qn=A), max(1, reps - 1))
    # the old route: one compute_scan per reference member
    loop = min(loop, R)
    out["old_route_calls_timed"] = loop
    old = timed(lambda: [m.compute_scan(basis, coeff, offset, A_qn=A, reference=int(r)) for r in scattered[:loop]], max(1, reps - 1))
    out["old_route_wall_ms_per_call"] = [t / loop for t in old]
    out["old_route_wall_ms_for_R"] = float(np.median(old)) / loop * R
    for name in ("scattered", "all"):
        out[name]["method_wall_ms_median"] = float(np.median(out[name]["method_wall_ms"]))
    out["old_route_over_method_scattered"] = out["old_route_wall_ms_for_R"] / out["scattered"]["method_wall_ms_median"]
    res = m.compute_scan_pairs(basis, coeff, offset, A_qn=A, reference_members=scattered)
    one = m.compute_scan(basis, coeff, offset, A_qn=A, reference=int(scattered[1]))
    others = np.arange(L) != scattered[1]
    out["max_rel_dDelta_f_difference_to_old_route_row"] = float(np.max(np.abs(res["dDelta_f"][1][others] / one["dDelta_f"][others] - 1.0)))
    out["finite"] = bool(np.all(np.isfinite(res["dDelta_f"])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--N", type=int, default=4000000)
    ap.add_argument("--L", type=int, default=1024)
    ap.add_argument("--R", type=int, default=64)
    ap.add_argument("--K", type=int, default=128)
    ap.add_argument("--Q", default="0,1")
    ap.add_argument("--loop", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_pairs_bench.txt"))
    a = ap.parse_args()
    m, x, O_k = resident_mbar(a.K, a.N)
    m.u_kn, m.n_bootstraps = None, 0
    peak = m._dm.mfma_f64_peak()
    lines = [json.dumps(dict(tool="bench_scan_pairs", mfma_f64_peak_tflops=peak))]
    for Q in [int(v) for v in a.Q.split(",")]:
        r = bench_case(m, x, O_k, a.L, a.R, Q, a.reps, a.loop, peak)
        lines.append(json.dumps(r))
        print(lines[-1], file=sys.stderr, flush=True)
        with open(a.out, "w") as fh:  # (kept up to date case by case)
            fh.write("\n".join(lines) + "\n")
    m._dm.close()
    print(json.dumps(dict(bench="scan_pairs", cases=len(lines) - 1, out=a.out)))


if __name__ == "__main__":
    main()
