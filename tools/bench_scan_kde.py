"""Kernel-density surfaces along a scan (``MBAR.compute_scan_kde``) on one MI355X, all in ONE process: kernel ms of the density pass
(``mbar_scan_kde_sums``) from the library's event timers with the model of DESIGN.md section 25 next to it -- ``2 L M N`` matrix flop,
``L N ceil(M / 128)`` member exponentials and ``M N ceil(L / members of a panel)`` kernel exponentials, the fraction of
``mbar_mfma_f64_peak`` reached (measured in the same run; matrix flop only) --; the wall time of the method end to end; and next to
them the only route there was before: a loop over the members of ``FES.generate_fes(u_n=u_l, fes_type="kde")`` + ``get_fes``, of
which ``--loop`` members are timed and the figure is SCALED by L (every member costs the same).

The system is the harmonic ladder of tools/bench_histogram.py (K = 128 states generated and solved in HBM); the members are
oscillators with centres across the ladder, in the basis {x^2, x}; the points are the sample coordinate x and, for d = 2, cos 3x; the
queries a grid over the samples (a square grid for d = 2); the bandwidth a tenth of the spacing of the ladder's ends.

    python tools/bench_scan_kde.py [--reps 2] [--N 4000000] [--L 128,1024] [--M 256,4096] [--d 1,2] [--loop 2] [--out profiles/scan_kde_bench.txt]"""
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


def model(L, M, N, members_per_panel=256):
    """Matrix flop that reach an output, matrix flop issued (whole blocks of 16 queries and of 16 members) and exponentials"""
    panels = [min(128, M - q0) for q0 in range(0, M, 128)]
    rows_issued = sum(16 * (1 if p <= 16 else 2 if p <= 32 else 4 if p <= 64 else 8) for p in panels)
    return dict(matrix_flop=2.0 * L * M * N, matrix_flop_issued=2.0 * (-(-L // 16) * 16) * rows_issued * N,
                member_exponentials=float(L) * N * len(panels), kernel_exponentials=float(rows_issued) * N * -(-L // members_per_panel),
                query_panels=len(panels))


def queries_for(x, d, M):
    lo, hi = float(x.min()), float(x.max())
    if d == 1:
        return np.linspace(lo, hi, M)[:, None]
    side = int(round(np.sqrt(M)))
    gx, gy = np.meshgrid(np.linspace(lo, hi, side), np.linspace(-1.0, 1.0, M // side), indexing="ij")
    return np.stack([gx.ravel(), gy.ravel()], axis=1)


def old_route(m, basis, coeff, offset, pts, q, h, loop, reps):
    """``loop`` members through FES.generate_fes(u_n=u_l, fes_type="kde") + get_fes on the same resident object"""
    from pymbar_amd.fes import FES

    fes = FES.__new__(FES)
    fes.mbar, fes.N_k, fes.u_kn, fes.K, fes.N, fes.timings = m, np.asarray(m.N_k, dtype=np.int64), None, m.K, m.N, False

    def run():
        out = []
        for l in range(loop):
            fes.generate_fes(coeff[l] @ basis + offset[l], pts, fes_type="kde", kde_parameters={"bandwidth": h})
            out.append(fes.get_fes(q, reference_point="from-lowest")["f_i"])
            fes.kde.close()
        return out

    ms = timed(run, reps)
    return ms, run()


def bench_case(m, x, O_k, L, M, d, reps, loop, peak_tflops):
    dm, N = m._dm, m.N
    O_l = np.linspace(O_k[0], O_k[-1], L)
    K_l = np.full(L, 1.0 / (1.5 * (O_k[1] - O_k[0])) ** 2)
    basis, coeff, offset = ts.harmonic_scan_family(x, O_l, K_l)
    pts = np.stack([x, np.cos(3.0 * x)][:d], axis=1)
    q = queries_for(x, d, M)
    M = len(q)
    h = 0.1 * (O_k[-1] - O_k[0]) / 4.0
    out = dict(K=m.K, N=N, L=L, B=2, M=M, d=d, bandwidth=h)
    dm.set_option("timing", 1)
    dm.set_scan(basis, None)
    dm.set_scan_points(np.ascontiguousarray(pts.T))
    f_scan = -dm.scan_lognum(m.f_k, coeff, offset)[0]
    q_dm = np.ascontiguousarray(q.T)
    ms = kernel_ms(dm, lambda: dm.scan_kde_sums(m.f_k, coeff, offset, f_scan, q_dm, h), reps)
    sums_wall = timed(lambda: dm.scan_kde_sums(m.f_k, coeff, offset, f_scan, q_dm, h), reps)
    n_exact = dm.scan_kde_sums(m.f_k, coeff, offset, f_scan, q_dm, h)[2]
    dm.set_option("timing", 0)
    dm.set_scan_points(None)
    dm.set_scan(None)
    mod, med = model(L, M, N), float(np.median(ms))
    out["sums"] = dict(kernel_ms=ms, kernel_ms_median=med, wall_ms=sums_wall, n_exact=int(n_exact), **mod,
                       matrix_tflops=mod["matrix_flop"] / (med * 1e-3) / 1e12,
                       fraction_of_mfma_f64_peak=mod["matrix_flop"] / (med * 1e-3) / 1e12 / peak_tflops,
                       issued_fraction_of_mfma_f64_peak=mod["matrix_flop_issued"] / (med * 1e-3) / 1e12 / peak_tflops)
    wall = timed(lambda: m.compute_scan_kde(pts, q, h, basis, coeff, offset), reps)
    res = m.compute_scan_kde(pts, q, h, basis, coeff, offset)
    out["method"] = dict(wall_ms=wall, wall_ms_median=float(np.median(wall)), finite=bool(np.all(np.isfinite(res["f_i"]))))
    loop = min(loop, L)
    old_ms, old = old_route(m, basis, coeff, offset, pts, q, h, loop, reps)
    per_member = float(np.median(old_ms)) / loop
    out["old_route"] = dict(members_timed=loop, wall_ms_per_member=per_member, wall_ms_scaled_to_L=per_member * L, scaled=True,
                            over_method=per_member * L / out["method"]["wall_ms_median"],
                            max_abs_f_i_difference=float(max(np.max(np.abs(res["f_i"][l] - old[l])) for l in range(loop))))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--N", type=int, default=4000000)
    ap.add_argument("--K", type=int, default=128)
    ap.add_argument("--L", default="128,1024")
    ap.add_argument("--M", default="256,4096")
    ap.add_argument("--d", default="1,2")
    ap.add_argument("--loop", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_kde_bench.txt"))
    a = ap.parse_args()
    m, x, O_k = resident_mbar(a.K, a.N)
    m.u_kn, m.n_bootstraps = None, 0
    peak = m._dm.mfma_f64_peak()
    lines = [json.dumps(dict(tool="bench_scan_kde", mfma_f64_peak_tflops=peak, protocol="one process, one warm-up and %d timed repetitions per figure" % a.reps))]
    for d in [int(v) for v in a.d.split(",")]:
        for L in [int(v) for v in a.L.split(",")]:
            for M in [int(v) for v in a.M.split(",")]:
                lines.append(json.dumps(bench_case(m, x, O_k, L, M, d, a.reps, a.loop, peak)))
                print(lines[-1], file=sys.stderr, flush=True)
                with open(a.out, "w") as fh:  # (kept up to date case by case)
                    fh.write("\n".join(lines) + "\n")
    m._dm.close()
    print(json.dumps(dict(bench="scan_kde", cases=len(lines) - 1, out=a.out)))


if __name__ == "__main__":
    main()
