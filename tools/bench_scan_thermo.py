"""Entropy, enthalpy and heat capacity along a scan (``MBAR.compute_scan_entropy_and_enthalpy``) on one MI355X, all in ONE process:
kernel ms of pass A (``mbar_scan_energy_lognum``, J = 3) and pass B (``mbar_scan_energy_gram_w``, J = 3) from the library's event
timers, next to the same J = 3 sums with Q = 2 STORED observables (``mbar_scan_lognum`` / ``mbar_scan_gram_w``: the kernels
``compute_scan`` runs, whose instruction streams the energy policy leaves as they were), the wall time of the method and of
``compute_scan`` with Q = 2, and at L = 128 the dense ``compute_entropy_and_enthalpy(u_kn=u_ln)`` with its upload of the L rows.

The system is the harmonic ladder of tools/bench_histogram.py (K = 128 states generated and solved in HBM); the family are
oscillators with centres across the ladder in the basis {x^2, x}.

    python tools/bench_scan_thermo.py [--reps 3] [--N 4000000] [--L 128,1024]"""
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


def bench_shape(m, x, O_k, L, reps, dense):
    K, N = m.K, m.N
    dm = m._dm
    O_l = np.linspace(O_k[0], O_k[-1], L)
    K_l = np.full(L, 1.0 / (1.5 * (O_k[1] - O_k[0])) ** 2)
    basis, coeff, offset = ts.harmonic_scan_family(x, O_l, K_l)
    A = np.stack([x, x * x])
    t = A - (A.min(axis=1) - 1e-3)[:, None]
    out = dict(K=K, N=N, L=L, J=3)
    dm.set_option("timing", 1)
    dm.set_scan(basis, None)
    _, mean0 = dm.scan_energy_lognum(m.f_k, coeff, offset, center_u=None, J=2)
    cu = mean0[:, 1].copy()
    lognum, _ = dm.scan_energy_lognum(m.f_k, coeff, offset, center_u=cu, J=3)
    out["energy_pass_a_kernel_ms"] = kernel_ms(dm, lambda: dm.scan_energy_lognum(m.f_k, coeff, offset, center_u=cu, J=3), reps)
    out["energy_pass_a_J2_kernel_ms"] = kernel_ms(dm, lambda: dm.scan_energy_lognum(m.f_k, coeff, offset, center_u=None, J=2), reps)
    out["energy_pass_b_kernel_ms"] = kernel_ms(dm, lambda: dm.scan_energy_gram_w(m.f_k, coeff, offset, -lognum, center_u=cu, J=3), reps)
    dm.set_scan(basis, t)
    out["stored_pass_a_kernel_ms"] = kernel_ms(dm, lambda: dm.scan_lognum(m.f_k, coeff, offset), reps)
    out["stored_pass_b_kernel_ms"] = kernel_ms(dm, lambda: dm.scan_gram_w(m.f_k, coeff, offset, -lognum), reps)
    dm.set_option("timing", 0)
    dm.set_scan(None)
    for key in list(out):
        if key.endswith("_ms"):
            out[key + "_median"] = float(np.median(out[key]))
    out["energy_over_stored_pass_a"] = out["energy_pass_a_kernel_ms_median"] / out["stored_pass_a_kernel_ms_median"]
    out["energy_over_stored_pass_b"] = out["energy_pass_b_kernel_ms_median"] / out["stored_pass_b_kernel_ms_median"]
    out["method_wall_ms"] = timed(lambda: m.compute_scan_entropy_and_enthalpy(basis, coeff, offset), reps)
    out["compute_scan_Q2_wall_ms"] = timed(lambda: m.compute_scan(basis, coeff, offset, A_qn=A), reps)
    if dense:
        u_ln = coeff @ basis + offset[:, None]
        out["dense_entropy_and_enthalpy_wall_ms"] = timed(lambda: m.compute_entropy_and_enthalpy(u_kn=u_ln), max(1, reps - 1))
        out["dense_u_ln_bytes"] = int(u_ln.nbytes)
        res, ref = m.compute_scan_entropy_and_enthalpy(basis, coeff, offset), m.compute_entropy_and_enthalpy(u_kn=u_ln)
        for name in ("Delta_u", "Delta_s"):
            out["max_abs_%s_difference" % name] = float(np.max(np.abs(res[name] - ref[name][0])))
        for name in ("dDelta_u", "dDelta_s"):
            out["max_rel_%s_difference" % name] = float(np.max(np.abs(res[name][1:] / ref[name][0][1:] - 1.0)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--N", default="4000000")
    ap.add_argument("--L", default="128,1024")
    ap.add_argument("--K", type=int, default=128)
    a = ap.parse_args()
    out = dict(bench="scan_thermo", shapes=[])
    for N in [int(v) for v in a.N.split(",")]:
        m, x, O_k = resident_mbar(a.K, N)
        m.u_kn, m.n_bootstraps = None, 0
        for L in [int(v) for v in a.L.split(",")]:
            r = bench_shape(m, x, O_k, L, a.reps, dense=L <= 128)
            out["shapes"].append(r)
            print(json.dumps(r), file=sys.stderr, flush=True)
        m._dm.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
