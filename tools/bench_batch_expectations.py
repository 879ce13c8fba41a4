"""Time of ``pymbar_amd.MBARBatch`` and of each of its methods against a loop of ``MBAR(...)`` (adaptive protocol) plus the same
method on the same device; prints one JSON line.

    python tools/bench_batch_expectations.py [--sizes P,K,N ...] [--loop-max P] [--repeats R]

Sizes default to the first two of DESIGN.md section 15's table, (1000, 5, 5000) and (4096, 12, 2e4).  Every figure is the median of
R runs after one warm-up.  Per size: the construction of the batch (checks, upload, solve), each method on the resident batch
with the split of its last run (rows built on the host / upload and device passes / host covariance), and per method the loop's
construction + method on at most ``--loop-max`` problems, scaled to P (its per-problem cost does not depend on P).
Every method is timed with the covariance pass at f_k not yet made, as its first call on a fresh object finds it.  Kernel times
come from a separate ``rocprofv3 --kernel-trace --stats`` run of this script."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pymbar_amd  # noqa: E402
from pymbar_amd import testsystems as ts  # noqa: E402

PROTO = (dict(method="adaptive", tol=1e-12, options=dict(min_sc_iter=0)),)
NEW_STATES = 3


def problems(P, K, N, seed=0):
    rng = np.random.default_rng(seed)
    N_k = np.full(K, N // K)
    N_k[: N - N_k.sum()] += 1
    x_n, base = ts.harmonic_u_kn(np.linspace(0, 2, K), np.linspace(1, 3, K), N_k, seed=1)[:2]
    return x_n, [base + rng.normal(scale=1e-3, size=(K, 1)) * np.arange(K)[:, None] for _ in range(P)], [N_k] * P


def median_s(fn, repeats):
    fn()
    ts_ = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts_.append(time.perf_counter() - t0)
    return statistics.median(ts_)


def run_size(P, K, N, loop_max, repeats):
    x_n, us, Ns = problems(P, K, N)
    xs = [x_n] * P
    news = [u[:NEW_STATES] * 1.1 + 0.3 for u in us]
    methods = {
        "compute_free_energy_differences": (lambda mb: mb.compute_free_energy_differences(),
                                            lambda m, p: m.compute_free_energy_differences()),
        "compute_overlap": (lambda mb: mb.compute_overlap(), lambda m, p: m.compute_overlap()),
        "compute_expectations": (lambda mb: mb.compute_expectations(xs), lambda m, p: m.compute_expectations(x_n)),
        "compute_expectations_new_states": (lambda mb: mb.compute_expectations(xs, u_kn_list=news),
                                            lambda m, p: m.compute_expectations(x_n, u_kn=news[p])),
        "compute_perturbed_free_energies": (lambda mb: mb.compute_perturbed_free_energies(news),
                                            lambda m, p: m.compute_perturbed_free_energies(news[p])),
        "compute_entropy_and_enthalpy": (lambda mb: mb.compute_entropy_and_enthalpy(), lambda m, p: m.compute_entropy_and_enthalpy()),
    }
    construct = median_s(lambda: pymbar_amd.MBARBatch(us, Ns).close(), repeats)
    nl = min(P, loop_max)

    def loop(single):
        for p in range(nl):
            m = pymbar_amd.MBAR(us[p], Ns[p], solver_protocol=PROTO)
            if single is not None:
                single(m, p)
            m.close()

    loop_construct = median_s(lambda: loop(None), repeats) * P / nl
    out = dict(P=P, K=K, N=N, loop_problems_timed=nl, repeats=repeats, batch_construct_s=round(construct, 4),
               loop_construct_s=round(loop_construct, 3), methods={})
    with pymbar_amd.MBARBatch(us, Ns) as mb:
        assert mb.success.all() and not mb.host_fallback.any()
        for name, (batched, single) in methods.items():
            def call():
                mb._gram = None   # (as on a fresh object: the covariance pass at f_k is part of the method that needs it)
                mb.timing = None
                batched(mb)

            t_b = median_s(call, repeats)
            t_l = median_s(lambda: loop(single), repeats) * P / nl
            row = dict(batch_method_s=round(t_b, 4), batch_total_s=round(construct + t_b, 4), loop_total_s=round(t_l, 3),
                       speedup=round(t_l / (construct + t_b), 1))
            if getattr(mb, "timing", None):
                row["split_s"] = {k: round(v, 4) for k, v in mb.timing.items()}
            out["methods"][name] = row
            print(json.dumps({name: row}), file=sys.stderr, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="*", default=["1000,5,5000", "4096,12,20000"])
    ap.add_argument("--loop-max", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    out = []
    for s in a.sizes:
        P, K, N = (int(float(x)) for x in s.split(","))
        out.append(run_size(P, K, N, a.loop_max, a.repeats))
    print(json.dumps(dict(tool="bench_batch_expectations", device=pymbar_amd.device.device_info(0)["name"], sizes=out)))


if __name__ == "__main__":
    main()
