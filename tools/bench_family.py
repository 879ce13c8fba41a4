#!/usr/bin/env python
"""Families with harmonic terms (`MBAR.from_family`, scans over periodic members) against the linear family in the SAME run.

At K=128 N=1e7 (--quick: K=32 N=1e6), umbrellas on a torsion, basis [E, chi], B = 2:
  fill    k_fill_linear_rows (B = 2) against k_fill_family_rows (B = 2, one periodic term) on the same context: kernel time
          through mbar_ctx_timing, one warm-up, the median of REPEATS launches, min and max as the spread; store bandwidth 8 K N / t
  scan    pass A (mbar_scan_lognum) and pass B (mbar_scan_gram_w, with the cross block) of a 1024-member scan on the same
          resident matrix, linear members against periodic members: kernel time of the whole call (every launch of it)
  class   MBAR.from_family(...) + compute_free_energy_differences() against MBAR(u_kn_host, N_k) + the same call on the same
          matrix, default protocol, one warm-up construction each, the median of 3

The driver itself never opens the GPU: every step is a child process of its own under `timeout`, one at a time, and the first
step that fails ends the run.

Usage: python tools/bench_family.py [--out FILE] [--quick]"""
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

REPEATS = 7
L_SCAN = 1024
STEP_SECONDS = dict(fill=180, scan=300, cls=420)


def family(K, N):
    """K umbrellas on a torsion with N samples in all: chi spread over the circle around the umbrella that drew it, E the cosine
    potential (the kernels' time does not depend on the values)."""
    rng = np.random.default_rng(0)
    chi0 = -180.0 + 360.0 * (np.arange(K) + 0.5) / K
    N_k = np.full(K, N // K, dtype=np.int64)
    N_k[-1] += N - N_k.sum()
    chi = np.repeat(chi0, N_k) + rng.normal(0.0, 15.0, N)
    chi -= 360.0 * np.rint(chi / 360.0)
    basis = np.ascontiguousarray(np.stack([1.5 * (1.0 + np.cos(np.deg2rad(3.0 * chi))), chi]))
    coeff = np.ascontiguousarray(np.stack([np.ones(K), np.full(K, 0.001)], axis=1))
    center = np.ascontiguousarray(np.stack([np.zeros(K), chi0], axis=1))
    return basis, coeff, center, np.array([False, True]), np.array([0.0, 360.0]), N_k


def spread(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), n=len(ms))


def timed_other(dm, fn):
    """Kernel time of the launches `fn` books under the "other" timer: one warm-up, then REPEATS calls"""
    fn()
    out, launches = [], 0
    for _ in range(REPEATS):
        dm.timing_reset()
        fn()
        ms, launches = dm.timing()["other"]
        out.append(ms)
    return dict(spread(out), launches=launches)


def step_fill(K, N):
    from pymbar_amd.device import DeviceMatrix, device_info

    basis, coeff, center, hb, pb, _ = family(K, N)
    lin_coeff = np.ascontiguousarray(coeff * [1.0, 0.01])
    with DeviceMatrix.empty(K, N) as dm:
        dm.set_option("timing", 1)
        lin = timed_other(dm, lambda: dm.fill_linear_rows(0, basis, lin_coeff, None))
        fam = timed_other(dm, lambda: dm.fill_family_rows(0, basis, coeff, None, center, hb, pb))
        lin2 = timed_other(dm, lambda: dm.fill_family_rows(0, basis, lin_coeff, None, None, None, None))  # family kernel, no harmonic term
    gb = 8.0 * K * N * 1e-9
    return dict(step="fill", K=K, N=N, B=2, device=device_info(0)["name"], k_fill_linear_rows=lin, k_fill_family_rows_periodic=fam,
                k_fill_family_rows_all_linear=lin2, linear_store_GBps=gb / (lin["median_ms"] * 1e-3),
                family_store_GBps=gb / (fam["median_ms"] * 1e-3), family_over_linear_time=fam["median_ms"] / lin["median_ms"])


def step_scan(K, N):
    from pymbar_amd.device import DeviceMatrix

    basis, coeff, center, hb, pb, N_k = family(K, N)
    L = L_SCAN
    c_l = np.ascontiguousarray(np.tile([1.0, 0.001], (L, 1)))
    cen_l = np.ascontiguousarray(np.stack([np.zeros(L), np.linspace(-180.0, 180.0, L)], axis=1))
    lin_l = np.ascontiguousarray(np.stack([np.ones(L), np.linspace(-0.01, 0.01, L)], axis=1))
    f = np.zeros(K)
    out = dict(step="scan", K=K, N=N, L=L, B=2)
    with DeviceMatrix.from_family(basis, coeff, None, center, hb, pb) as dm:
        dm.set_Nk(N_k)
        dm.set_option("timing", 1)
        for tag, kinds, cf, cen in (("linear", {}, lin_l, {}), ("periodic", dict(harmonic_b=hb, period_b=pb), c_l, dict(center_lb=cen_l))):
            dm.set_scan(basis, None, **kinds)
            lognum, _ = dm.scan_lognum(f, cf, None, **cen)
            out[tag + "_pass_a"] = timed_other(dm, lambda: dm.scan_lognum(f, cf, None, **cen))
            out[tag + "_pass_b"] = timed_other(dm, lambda: dm.scan_gram_w(f, cf, None, -lognum, **cen))
        dm.set_scan(None)
    for p in ("pass_a", "pass_b"):
        out["periodic_over_linear_" + p] = out["periodic_" + p]["median_ms"] / out["linear_" + p]["median_ms"]
    return out


def step_class(K, N):
    import pymbar_amd

    basis, coeff, center, hb, pb, N_k = family(K, N)

    def fam():
        m = pymbar_amd.MBAR.from_family(basis, coeff, N_k, center_kb=center, harmonic_b=hb, period_b=pb)
        return m, m.compute_free_energy_differences()

    def dense(u):
        m = pymbar_amd.MBAR(u, N_k)
        return m, m.compute_free_energy_differences()

    m, r_fam = fam()  # warm-up, and the source of the dense host matrix: the same numbers to the bit
    u_host = np.array(m.u_kn)
    m.close()
    del m
    t_fam, t_dense = [], []
    for i in range(4):  # (the first dense construction is its warm-up)
        t0 = time.perf_counter()
        m, r = fam()
        t_fam.append(1e3 * (time.perf_counter() - t0))
        assert m._u_kn is None
        stats = dict(m.upload_stats)
        m.close()
        del m
        t0 = time.perf_counter()
        m, r_dense = dense(u_host)
        t_dense.append(1e3 * (time.perf_counter() - t0))
        m.close()
        del m
    same = bool(np.array_equal(r_fam["Delta_f"], r_dense["Delta_f"]) and np.array_equal(r_fam["dDelta_f"], r_dense["dDelta_f"]))
    a, b = spread(t_fam[1:]), spread(t_dense[1:])
    return dict(step="class", K=K, N=N, B=2, from_family_plus_differences=a, dense_plus_differences=b,
                ratio_dense_over_family=b["median_ms"] / a["median_ms"], same_bits=same, upload_stats=stats)


def run_step(argv):
    kind, nums = argv[0], [int(a) for a in argv[1:]]
    print(json.dumps({"fill": step_fill, "scan": step_scan, "class": step_class}[kind](*nums)), flush=True)


def main(argv):
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
    K, N = (32, 1_000_000) if "--quick" in argv else (128, 10_000_000)
    lines = []
    for step in (("fill", K, N), ("scan", K, N), ("class", K, N)):
        limit = STEP_SECONDS["cls" if step[0] == "class" else step[0]]
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step"] + [str(a) for a in step]
        res = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        line = res.stdout.strip().splitlines()[-1] if res.returncode == 0 and res.stdout.strip() else None
        if line is None:  # (a fault, an abort or a time limit: nothing more is started on the GPU)
            msg = json.dumps(dict(step=step[0], args=step[1:], failed=res.returncode, stderr=res.stderr[-2000:]))
            print(msg, flush=True)
            lines.append(msg)
            break
        print(line, flush=True)
        lines.append(line)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0 if lines and "failed" not in json.loads(lines[-1]) else 1


if __name__ == "__main__":
    if "--step" in sys.argv:
        run_step(sys.argv[sys.argv.index("--step") + 1:])
    else:
        sys.exit(main(sys.argv[1:]))
