#!/usr/bin/env python
"""The constructor from a linear family (`MBAR.from_linear`) against the dense constructor it replaces, and the kernel that makes
it possible against the device builder the project already had.

Per shape (K=128 N=1e7 with B=2 and B=8; K=32 N=1e6 with B=2 and B=8):
  kernel   k_fill_linear_rows through mbar_ctx_timing (one warm-up, the median of REPEATS launches, min and max as the spread), the
           store bandwidth 8 K N / t, and k_generate_harmonic -- same bytes, more arithmetic per element, 8-byte stores -- on the
           same context in the same process
  upload   mbar_ctx_upload_u of the dense K x N host matrix (wall time of the call): the path being replaced
  class    MBAR.from_linear(...) + compute_free_energy_differences() against MBAR(u_kn_host, N_k) + the same call, default
           protocol, one warm-up construction each (as tools/bench_class.py times its constructors), the median of 3

The driver itself never opens the GPU: every step is a child process of its own under `timeout`, one at a time, and the first
step that fails ends the run.

Usage: python tools/bench_linear.py [--out FILE] [--quick]      (--quick: K=32 N=1e6 only)"""
import ctypes as C
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
SHAPES = ((128, 10_000_000), (32, 1_000_000))
STEP_SECONDS = dict(kernel=120, upload=240, cls=360)


def family(K, N, B):
    """The harmonic ladder of the benchmark as a linear family over [x^2, x]; B > 2 pads the basis with seeded vectors whose
    coefficients are zero (the kernel's time does not depend on the values)."""
    from pymbar_amd import testsystems as ts

    O_k, K_k, N_k = ts.config3_params(K=K, N=N)
    N_k[-1] += N - N_k.sum()
    basis, coeff, offset = ts.harmonic_linear_family(O_k, K_k, N_k, seed=0)
    if B > 2:
        basis = np.concatenate([basis, np.random.default_rng(1).normal(size=(B - 2, N))])
        coeff = np.concatenate([coeff, np.zeros((K, B - 2))], axis=1)
    return np.ascontiguousarray(basis), np.ascontiguousarray(coeff), offset, N_k, O_k, K_k


def spread(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), n=len(ms))


def timed_other(dm, fn):
    """Kernel time of the launches `fn` books under the "other" timer: one warm-up, then REPEATS single launches."""
    fn()
    out = []
    for _ in range(REPEATS):
        dm.timing_reset()
        fn()
        ms, n = dm.timing()["other"]
        assert n == 1, n
        out.append(ms)
    return out


def step_kernel(K, N, B):
    from pymbar_amd.device import DeviceMatrix, _dptr, device_info

    basis, coeff, offset, N_k, O_k, K_k = family(K, N, B)
    with DeviceMatrix.empty(K, N) as dm:
        dm.set_option("timing", 1)
        fill = spread(timed_other(dm, lambda: dm.fill_linear_rows(0, basis, coeff, offset)))
        ctx_args = (np.ascontiguousarray(O_k), np.ascontiguousarray(K_k), np.ascontiguousarray(N_k, dtype=np.int64))

        def harmonic():
            dm._check(dm._lib.mbar_ctx_generate_harmonic(dm._ctx, C.c_uint64(0), _dptr(ctx_args[0]), _dptr(ctx_args[1]),
                                                         ctx_args[2].ctypes.data_as(C.POINTER(C.c_int64)), 0))

        harm = spread(timed_other(dm, harmonic))
    gb = 8.0 * K * N * 1e-9
    # "not slower beyond the spread between repeats": the medians compared with the wider of the two min-max ranges as the margin
    margin = max(fill["max_ms"] - fill["min_ms"], harm["max_ms"] - harm["min_ms"])
    return dict(step="kernel", K=K, N=N, B=B, device=device_info(0)["name"], k_fill_linear_rows=fill, k_generate_harmonic=harm,
                fill_store_GBps=gb / (fill["median_ms"] * 1e-3), harmonic_store_GBps=gb / (harm["median_ms"] * 1e-3),
                basis_read_fraction=B * ((K + 127) // 128) / K, fill_over_harmonic_time=fill["median_ms"] / harm["median_ms"],
                fill_over_harmonic_bytes=1.0 + B * ((K + 127) // 128) / K, margin_ms=margin,
                fill_not_slower=bool(fill["median_ms"] <= harm["median_ms"] + margin))


def step_upload(K, N):
    from pymbar_amd.device import DeviceMatrix

    basis, coeff, offset, *_ = family(K, N, 2)
    with DeviceMatrix.from_linear(basis, coeff, offset) as dm:
        u_host = dm.to_host()
    del basis
    ms = []
    for i in range(4):  # (the first is the warm-up)
        t0 = time.perf_counter()
        dm = DeviceMatrix.from_host(u_host)
        ms.append(1e3 * (time.perf_counter() - t0))
        dm.close()
    s = spread(ms[1:])
    return dict(step="upload", K=K, N=N, mbar_ctx_upload_u=s, GBps=8.0 * K * N * 1e-9 / (s["median_ms"] * 1e-3))


def step_class(K, N, B):
    import pymbar_amd

    basis, coeff, offset, N_k, *_ = family(K, N, B)

    def linear():
        m = pymbar_amd.MBAR.from_linear(basis, coeff, N_k, offset_k=offset)
        r = m.compute_free_energy_differences()
        return m, r

    def dense(u):
        m = pymbar_amd.MBAR(u, N_k)
        r = m.compute_free_energy_differences()
        return m, r

    m, r_lin = linear()  # warm-up, and the source of the dense host matrix: the same numbers to the bit
    u_host = np.array(m.u_kn)
    m.close()
    del m
    t_lin, t_dense = [], []
    for i in range(4):  # (the first dense construction is its warm-up)
        t0 = time.perf_counter()
        m, r = linear()
        t_lin.append(1e3 * (time.perf_counter() - t0))
        assert m._u_kn is None
        stats = dict(m.upload_stats)  # (of the last timed construction)
        m.close()
        del m
        t0 = time.perf_counter()
        m, r_dense = dense(u_host)
        t_dense.append(1e3 * (time.perf_counter() - t0))
        m.close()
        del m
    same = bool(np.array_equal(r_lin["Delta_f"], r_dense["Delta_f"]) and np.array_equal(r_lin["dDelta_f"], r_dense["dDelta_f"]))
    lin, den = spread(t_lin[1:]), spread(t_dense[1:])
    return dict(step="class", K=K, N=N, B=B, from_linear_plus_differences=lin, dense_plus_differences=den,
                ratio_dense_over_linear=den["median_ms"] / lin["median_ms"], same_bits=same, upload_stats=stats)


def run_step(argv):
    kind, nums = argv[0], [int(a) for a in argv[1:]]
    out = {"kernel": step_kernel, "upload": step_upload, "class": step_class}[kind](*nums)
    print(json.dumps(out), flush=True)


def main(argv):
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
    shapes = SHAPES[1:] if "--quick" in argv else SHAPES
    steps = []
    for K, N in shapes:
        steps += [("kernel", K, N, 2), ("kernel", K, N, 8), ("upload", K, N), ("class", K, N, 2)]
    lines = []
    for step in steps:
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
