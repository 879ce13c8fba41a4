#!/usr/bin/env python
"""The constructors from a family of states (`MBAR.from_linear`, `MBAR.from_family`) against the dense constructor they replace, the
two policies of the fill kernel against each other and against the device builder the project already had, and scans over
periodic members against linear ones -- all in the SAME run.

At K=128 N=1e7 (--quick: K=32 N=1e6):
  fill    B = 2 and B = 8: k_fill_rows<B, ScanLinear> (no harmonic term) and k_fill_rows<B, FamilyTerms> (max(1, B / 2) <= 4
          harmonic terms, the first periodic) on the same context, ALTERNATING launch by launch: kernel time through
          mbar_ctx_timing, one warm-up each, the median of REPEATS launches, min and max as the spread; store bandwidth 8 K N / t;
          then k_generate_harmonic -- same bytes, 8-byte stores -- on the same context as the yardstick
  upload  mbar_ctx_upload_u of the dense K x N host matrix (wall time of the call): the path being replaced
  scan    pass A (mbar_scan_lognum) and pass B (mbar_scan_gram_w, with the cross block) of a 1024-member scan on the same
          resident matrix, linear members against periodic members: kernel time of the whole call (every launch of it)
  class   MBAR.from_linear(...) and MBAR.from_family(...) + compute_free_energy_differences(), each against MBAR(u_kn_host, N_k)
          + the same call on the same matrix, default protocol, one warm-up construction each, the median of 3

The driver itself never opens the GPU: every step is a child process of its own under `timeout`, one at a time, and the first
step that fails ends the run.

Usage: python tools/bench_family.py [--out FILE] [--quick] [--steps fill,upload,scan,class]"""
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
L_SCAN = 1024
STEP_SECONDS = dict(fill=240, upload=240, scan=300, cls=600)


def family(K, N, B, harmonic):
    """`(basis, coeff, offset, center, harmonic_b, period_b, N_k)` of K states over N samples and B basis vectors (the kernels'
    time does not depend on the values).  harmonic False: the harmonic ladder of the benchmark as a linear family over [x^2, x], a
    B > 2 padded with seeded vectors whose coefficients are zero.  True: umbrellas on a torsion, basis [E, chi] -- chi spread over
    the circle around the umbrella that drew it, E the cosine potential -- a B > 2 padded with bounded features of chi, harmonic
    and linear in turn until max(1, B / 2) <= 4 terms are harmonic (B = 1: chi alone)."""
    from pymbar_amd import testsystems as ts

    N_k = np.full(K, N // K, dtype=np.int64)
    N_k[-1] += N - N_k.sum()
    rng = np.random.default_rng(1)
    if not harmonic:
        O_k, K_k = ts.ladder_params(K)
        basis, coeff, offset = ts.harmonic_linear_family(O_k, K_k, N_k, seed=0)
        if B > 2:
            basis = np.concatenate([basis, rng.normal(size=(B - 2, N))])
            coeff = np.concatenate([coeff, np.zeros((K, B - 2))], axis=1)
        return np.ascontiguousarray(basis[:B]), np.ascontiguousarray(coeff[:, :B]), offset, None, None, None, N_k
    chi0 = -180.0 + 360.0 * (np.arange(K) + 0.5) / K
    chi = np.repeat(chi0, N_k) + np.random.default_rng(0).normal(0.0, 15.0, N)
    chi -= 360.0 * np.rint(chi / 360.0)
    rad = np.deg2rad(chi)
    # (vector, period or None for a linear term, coefficient, centre)
    terms = [(1.5 * (1.0 + np.cos(3.0 * rad)), None, np.ones(K), 0.0), (chi, 360.0, np.full(K, 0.001), chi0)]
    extra = [(40.0 * np.sin(rad), 0.0), (np.cos(2.0 * rad), None), (50.0 * np.cos(rad), 25.0), (np.sin(3.0 * rad), None), (0.5 * chi, 180.0)]
    for v, P in extra + [(rng.normal(size=N), None)] * 8:
        if P is None or sum(t[1] is not None for t in terms) < min(4, max(1, B // 2)):
            terms.append((v, P, np.full(K, 1e-4), 0.0 if P is None else 0.5 * chi0))
    terms = terms[:B] if B > 1 else terms[1:2]
    basis = np.ascontiguousarray(np.stack([t[0] for t in terms]))
    coeff = np.ascontiguousarray(np.stack([t[2] for t in terms], axis=1))
    center = np.ascontiguousarray(np.stack([np.zeros(K) + t[3] for t in terms], axis=1))
    return (basis, coeff, None, center, np.array([t[1] is not None for t in terms]), np.array([t[1] or 0.0 for t in terms]), N_k)


def spread(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), n=len(ms))


def timed_other(dm, *fns):
    """Kernel time of the launches each of `fns` books under the "other" timer: one warm-up each, then REPEATS rounds in which
    they take turns."""
    for fn in fns:
        fn()
    out, launches = [[] for _ in fns], [0] * len(fns)
    for _ in range(REPEATS):
        for i, fn in enumerate(fns):
            dm.timing_reset()
            fn()
            ms, launches[i] = dm.timing()["other"]
            out[i].append(ms)
    res = [dict(spread(o), launches=n) for o, n in zip(out, launches)]
    return res[0] if len(fns) == 1 else res


def step_fill(K, N, B):
    from pymbar_amd import testsystems as ts
    from pymbar_amd.device import DeviceMatrix, _dptr, device_info

    lb, lc, lo, *_ = family(K, N, B, False)
    hbasis, hc, ho, cen, hb, pb, N_k = family(K, N, B, True)
    O_k, K_k = (np.ascontiguousarray(a) for a in ts.ladder_params(K))
    with DeviceMatrix.empty(K, N) as dm:
        dm.set_option("timing", 1)
        lin, fam = timed_other(dm, lambda: dm.fill_family_rows(0, lb, lc, lo), lambda: dm.fill_family_rows(0, hbasis, hc, ho, cen, hb, pb))
        harm = timed_other(dm, lambda: dm._check(dm._lib.mbar_ctx_generate_harmonic(
            dm._ctx, C.c_uint64(0), _dptr(O_k), _dptr(K_k), N_k.ctypes.data_as(C.POINTER(C.c_int64)), 0)))
    assert lin["launches"] == fam["launches"] == harm["launches"] == 1
    gb = 8.0 * K * N * 1e-9
    # "not slower beyond the spread between repeats": the medians compared with the wider of the two min-max ranges as the margin
    margin = max(lin["max_ms"] - lin["min_ms"], harm["max_ms"] - harm["min_ms"])
    return {"step": "fill", "K": K, "N": N, "B": B, "harmonic_terms": int(hb.sum()), "device": device_info(0)["name"],
            "k_fill_rows<%d, ScanLinear>" % B: lin, "k_fill_rows<%d, FamilyTerms>" % B: fam, "k_generate_harmonic": harm,
            "linear_store_GBps": gb / (lin["median_ms"] * 1e-3), "family_store_GBps": gb / (fam["median_ms"] * 1e-3),
            "harmonic_store_GBps": gb / (harm["median_ms"] * 1e-3), "family_over_linear_time": fam["median_ms"] / lin["median_ms"],
            "basis_read_fraction": B * ((K + 127) // 128) / K, "linear_over_harmonic_time": lin["median_ms"] / harm["median_ms"],
            "margin_ms": margin, "linear_not_slower": bool(lin["median_ms"] <= harm["median_ms"] + margin)}


def step_upload(K, N):
    from pymbar_amd.device import DeviceMatrix

    basis, coeff, offset, *_ = family(K, N, 2, False)
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


def step_scan(K, N):
    from pymbar_amd.device import DeviceMatrix

    basis, coeff, _, center, hb, pb, N_k = family(K, N, 2, True)
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

    def journey(make):
        """`make()` + differences against the dense constructor on the matrix `make()` built: the same numbers to the bit"""
        def run(ctor):
            m = ctor()
            return m, m.compute_free_energy_differences()

        m, r_fam = run(make)  # warm-up, and the source of the dense host matrix
        u_host, N_k = np.array(m.u_kn), m.N_k
        m.close()
        del m
        t_fam, t_dense = [], []
        for i in range(4):  # (the first dense construction is its warm-up)
            t0 = time.perf_counter()
            m, r = run(make)
            t_fam.append(1e3 * (time.perf_counter() - t0))
            assert m._u_kn is None
            stats = dict(m.upload_stats)  # (of the last timed construction)
            m.close()
            del m
            t0 = time.perf_counter()
            m, r_dense = run(lambda: pymbar_amd.MBAR(u_host, N_k))
            t_dense.append(1e3 * (time.perf_counter() - t0))
            m.close()
            del m
        same = bool(np.array_equal(r_fam["Delta_f"], r_dense["Delta_f"]) and np.array_equal(r_fam["dDelta_f"], r_dense["dDelta_f"]))
        a, b = spread(t_fam[1:]), spread(t_dense[1:])
        return dict(family_plus_differences=a, dense_plus_differences=b, ratio_dense_over_family=b["median_ms"] / a["median_ms"],
                    same_bits=same, upload_stats=stats)

    lb, lc, lo, _, _, _, N_k = family(K, N, 2, False)
    from_linear = journey(lambda: pymbar_amd.MBAR.from_linear(lb, lc, N_k, offset_k=lo))
    del lb
    hbasis, hc, _, cen, hb, pb, N_k = family(K, N, 2, True)
    from_family = journey(lambda: pymbar_amd.MBAR.from_family(hbasis, hc, N_k, center_kb=cen, harmonic_b=hb, period_b=pb))
    return dict(step="class", K=K, N=N, B=2, from_linear=from_linear, from_family=from_family)


def run_step(argv):
    kind, nums = argv[0], [int(a) for a in argv[1:]]
    print(json.dumps({"fill": step_fill, "upload": step_upload, "scan": step_scan, "class": step_class}[kind](*nums)), flush=True)


def main(argv):
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else None
    K, N = (32, 1_000_000) if "--quick" in argv else (128, 10_000_000)
    want = argv[argv.index("--steps") + 1].split(",") if "--steps" in argv else ["fill", "upload", "scan", "class"]
    steps = [s for s in (("fill", K, N, 2), ("fill", K, N, 8), ("upload", K, N), ("scan", K, N), ("class", K, N)) if s[0] in want]
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
