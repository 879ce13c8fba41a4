#!/usr/bin/env python
"""A/B on ONE context: the fused sweep specialised for unit sample multiplicities (default) against the general kernel (option
"fused_general" = 1) in cold forced solves of 20 iterations from f = 0, the benchmark's timed region.  Alternating solves, the
HIP-event mean of the fused sweep (eager launches, timing level 1: what bench.py reports as roofline.avg_launch_ms) and the wall time per solve, median and
minimum of the repetitions after the first; the two arms must return the same bits.
    python tools/ab_fused_general.py [KxN ...] [--reps R]"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pymbar_amd import testsystems as ts  # noqa: E402
from pymbar_amd.device import DeviceMatrix  # noqa: E402


def main():
    argv = sys.argv[1:]
    reps = 8
    if "--reps" in argv:
        i = argv.index("--reps")
        reps = int(argv[i + 1])
        del argv[i:i + 2]
    cases = tuple(tuple(int(v) for v in a.split("x")) for a in argv) or ((128, 10_000_000),)
    for K, N in cases:
        O_k, K_k, N_k = ts.config3_params(K=K, N=N)
        with DeviceMatrix.harmonic(O_k, K_k, N_k, seed=0) as dm:
            dm.set_Nk(N_k)
            dm.set_option("pcache", 0)  # (cold solves: every one builds the probability matrix)
            dm.set_option("graph", 0)
            dm.set_option("timing", 1)
            sweep = {0: [], 1: []}
            wall = {0: [], 1: []}
            bits = {}
            for rep in range(reps + 1):
                for general in (0, 1):
                    dm.set_option("fused_general", general)
                    dm.timing_reset()
                    dm.synchronize()
                    t0 = time.perf_counter()
                    f, r = dm.solve_adaptive(np.zeros(K), maxiter=20, min_sc_iter=0, check_convergence=False)
                    dt = time.perf_counter() - t0
                    ms, n = dm.timing()["fused"]
                    if rep:
                        sweep[general].append(ms / max(n, 1))
                        wall[general].append(1e3 * dt)
                    bits[general] = (f.copy(), r["psum"].copy(), r["gnorm"], r["max_delta"], r["iterations"])
            same = all(np.array_equal(np.asarray(a), np.asarray(b)) for a, b in zip(bits[0], bits[1]))
            print(f"K={K} N={N}: {reps} alternations, results bit-identical: {same}")
            for general, name in ((0, "unit-weight kernel"), (1, "general kernel")):
                s, w = np.array(sweep[general]), np.array(wall[general])
                print(f"   {name:20s} fused sweep: median {np.median(s):.4f} ms min {s.min():.4f} max {s.max():.4f}   "
                      f"solve: median {np.median(w):.2f} ms min {w.min():.2f} max {w.max():.2f}", flush=True)
            assert same


if __name__ == "__main__":
    main()
