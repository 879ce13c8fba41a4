"""End-to-end time of ``pymbar_amd.mbar_batch`` against a loop of ``MBAR(...)`` + ``compute_free_energy_differences()`` on the
same device; prints one JSON line.

    python tools/bench_mbar_batch.py [--sizes P,K,N ...] [--loop-max P] [--repeats R] [--bootstraps B]

Sizes default to (1000, 5, 5000), (4096, 12, 2e4) and (64, 40, 95000).  The loop runs on at most ``--loop-max`` problems of each
size and is scaled to P (its per-problem cost does not depend on P).  Reported per size: batch seconds (upload included, best
of R), its wall-clock split and the host share (input checks, host work between the device calls and the host covariance, over the
total), evaluation passes, the bytes one ``k_batch_eval`` pass reads
(every problem's K x N block once), and the loop's seconds.  Kernel times come from a separate
``rocprofv3 --kernel-trace --stats`` run of this script.

With ``--bootstraps B`` every problem also gets B bootstrap replicates (``mbar_batch(n_bootstraps=B,
uncertainty_method="bootstrap")``); the loop is then ``MBAR(u, N_k, n_bootstraps=B, bootstrap_rng="device")`` with the adaptive
protocol for the replicates too, and the seconds the replica slots took and their cost per slot are reported as well."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pymbar_amd  # noqa: E402
from pymbar_amd import testsystems as ts  # noqa: E402


def problems(P, K, N, seed=0):
    rng = np.random.default_rng(seed)
    N_k = np.full(K, N // K)
    N_k[: N - N_k.sum()] += 1
    base = ts.harmonic_u_kn(np.linspace(0, 2, K), np.linspace(1, 3, K), N_k, seed=1)[1]
    return [base + rng.normal(scale=1e-3, size=(K, 1)) * np.arange(K)[:, None] for _ in range(P)], [N_k] * P


def run_size(P, K, N, loop_max, repeats, B=0):
    us, Ns = problems(P, K, N)
    best, r = None, None
    for _ in range(repeats):
        t0 = time.perf_counter()
        ri = pymbar_amd.mbar_batch(us, Ns, n_bootstraps=B, rseed=0, uncertainty_method="bootstrap") if B else pymbar_amd.mbar_batch(us, Ns)
        dt = time.perf_counter() - t0
        if best is None or dt < best:
            best, r = dt, ri
    assert r["success"].all()
    nl = min(P, loop_max)
    t0 = time.perf_counter()
    proto = (dict(method="adaptive", tol=1e-12, options=dict(min_sc_iter=0)),)
    for p in range(nl):
        if B:
            m = pymbar_amd.MBAR(us[p], Ns[p], solver_protocol=proto, n_bootstraps=B, bootstrap_solver_protocol=proto,
                                bootstrap_rng="device", rseed=0)
            m.compute_free_energy_differences(uncertainty_method="bootstrap")
        else:
            m = pymbar_amd.MBAR(us[p], Ns[p], solver_protocol=proto)
            m.compute_free_energy_differences()
        m.close()
    loop = (time.perf_counter() - t0) * P / nl
    boot = {}
    if B:
        assert r["boot_success"].all()
        boot = dict(bootstraps=B, slots=P * B, bootstrap_s=round(r["timing"]["bootstrap"], 4),
                    us_per_slot=round(1e6 * r["timing"]["bootstrap"] / (P * B), 2), boot_passes=int(r["boot_passes"]),
                    boot_host_fallback=int(r["boot_host_fallback"].sum()), boot_iterations=int(np.max(r["boot_iterations"])))
    return dict(P=P, K=K, N=N, **boot, batch_s=round(best, 4), loop_s=round(loop, 3), speedup=round(loop / best, 1),
                passes=int(r["passes"]), split_s={k: round(v, 4) for k, v in r["timing"].items()},
                host_share=round((r["timing"]["checks"] + r["timing"]["host"] + r["timing"]["covariance"]) / best, 3),
                iterations=int(np.max(r["iterations"])), loop_problems_timed=nl,
                eval_pass_bytes=int(8 * K * N * P), data_GB=round(8e-9 * K * N * P, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="*", default=["1000,5,5000", "4096,12,20000", "64,40,95000"])
    ap.add_argument("--loop-max", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--bootstraps", type=int, default=0)
    a = ap.parse_args()
    out = []
    for s in a.sizes:
        P, K, N = (int(float(x)) for x in s.split(","))
        out.append(run_size(P, K, N, a.loop_max, a.repeats, a.bootstraps))
        print(json.dumps(out[-1]), file=sys.stderr, flush=True)
    print(json.dumps(dict(tool="bench_mbar_batch", device=pymbar_amd.device.device_info(0)["name"], sizes=out)))


if __name__ == "__main__":
    main()
