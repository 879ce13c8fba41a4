"""Histogram surfaces by bin label on one MI355X, three measurements in ONE process (boxes differ by a few percent: the two
sides of a comparison come from the same run):

 (i)   row path (``histogram_fes``: one matrix row per bin) against label path (``histogram_fes_labels``), f + analytical df, at
       K = 64, 64 populated bins, N = 4e6: harmonic ladder generated on the device, bins of the sample coordinate;
 (ii)  the label path alone at K = 128, N = 1e7 on a 50 x 50 grid, once with cells localised per state (2-D umbrella sampling) and
       once with random labels (the chunk table's worst case): kernel ms per pass (``mbar_ctx_timing``), sweeps and bytes of
       partial records, and the fraction of 8 TB/s that pass B's read(s) of the matrix reach;
 (iii) ``FES.generate_fes(fes_type="histogram", n_bootstraps=20)`` end to end at K = 32, N = 1e6.

    python tools/bench_histogram.py [--reps 5] [--skip ii]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import pymbar_amd  # noqa: E402
from pymbar_amd import fes as amd_fes  # noqa: E402
from pymbar_amd import testsystems as ts  # noqa: E402
from pymbar_amd.device import DeviceMatrix  # noqa: E402
from pymbar_amd.mbar import MBAR  # noqa: E402

HBM_BYTES_PER_S = 8.0e12


def resident_mbar(K, N):
    """An MBAR object around an umbrella-like harmonic ladder generated in HBM (centres 0 .. 4, every state 1.5 centre spacings
    wide, samples ordered by state), solved there; the sample coordinate, recovered from two rows of the matrix; the sample's state."""
    O_k, N_k = np.linspace(0.0, 4.0, K), np.full(K, N // K)
    K_k = np.full(K, 1.0 / (1.5 * (O_k[1] - O_k[0])) ** 2)
    dm = DeviceMatrix.harmonic(O_k, K_k, N_k, seed=1)
    dm.set_Nk(N_k)
    f_k, res = dm.solve_adaptive(np.zeros(K), tol=1e-10)
    assert res["success"]
    with DeviceMatrix.empty(2, dm.N_local) as two:
        two.copy_rows_from(dm, 0, 0, 2)
        u01 = two.to_host()
    x = (O_k[0] ** 2 - O_k[1] ** 2 - 2.0 * (u01[0] - u01[1]) / K_k[0]) / (2.0 * (O_k[0] - O_k[1]))
    m = MBAR.__new__(MBAR)  # (the attributes the histogram functions read; the matrix never exists on the host)
    m._dm, m.K, m.N, m.N_k, m.f_k, m._device = dm, K, dm.N_local, N_k, f_k, None
    m.states_with_samples = np.arange(K)
    m.basis_bn = m.coeff_kb = m.offset_k = None  # (not an object of MBAR.from_linear: u_kn is not rebuilt from a family)
    return m, x, O_k


def quantile_labels(x, nbins):
    edges = np.quantile(x, np.linspace(0.0, 1.0, nbins + 1)[1:-1])
    return np.searchsorted(edges, x).astype(np.int64)


def timed(fn, reps):
    fn()  # warm-up
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t0))
    return out


def part_i(reps):
    K, N, nbins = 64, 4_000_000, 64
    m, x, _ = resident_mbar(K, N)
    labels = quantile_labels(x, nbins)
    u_n = 0.5 * (x - 2.0) ** 2
    rows = timed(lambda: amd_fes.histogram_fes(m, u_n, labels), reps)
    labs = timed(lambda: amd_fes.histogram_fes_labels(m, u_n, labels), reps)
    a, b = amd_fes.histogram_fes(m, u_n, labels), amd_fes.histogram_fes_labels(m, u_n, labels)
    m._dm.close()
    return dict(K=K, N=N, nbins=nbins, row_path_ms=rows, label_path_ms=labs, row_path_ms_median=float(np.median(rows)),
                label_path_ms_median=float(np.median(labs)), max_abs_f_difference=float(np.max(np.abs(a["f_i"] - b["f_i"]))),
                max_rel_df_difference=float(np.max(np.abs(a["df_i"] - b["df_i"]) / np.maximum(a["df_i"], 1e-300))))


def part_ii(reps, shuffled):
    """shuffled=False: a second coordinate localised per state like the first (2-D umbrella sampling: a state covers a few grid
    cells); True: labels drawn at random, the worst case for the chunk table (a chunk closes on its 64th distinct bin)."""
    K, N, side = 128, 10_000_000, 50
    m, x, O_k = resident_mbar(K, N)
    rng = np.random.default_rng(2)
    nbins = side * side
    state = np.repeat(np.arange(K), N // K)
    y = O_k[(state * 37) % K] + rng.normal(0.0, 1.5 * (O_k[1] - O_k[0]), N)
    if shuffled:
        labels = rng.integers(0, nbins, N)
    else:
        labels = quantile_labels(x, side) * side + quantile_labels(y, side)
        _, labels = np.unique(labels, return_inverse=True)  # (the populated cells, numbered)
        nbins = int(labels.max()) + 1
    u_n = 0.5 * (x - 2.0) ** 2 + 0.5 * (y - 2.0) ** 2
    dm = m._dm
    t0 = time.perf_counter()
    dm.set_bins(nbins, labels, u_n)
    set_bins_s = time.perf_counter() - t0
    info = dm.bins_info()
    dm.set_option("timing", 1)
    f_raw = -dm.bin_lognum(m.f_k)  # (also leaves logden(f_k) in place: the timed calls below run the binned kernels only)
    dm.bin_gram_w(m.f_k, f_raw)
    a_ms, b_ms = [], []
    for _ in range(reps):
        dm.timing_reset()
        dm.bin_lognum(m.f_k)
        a_ms.append(dm.timing()["other"][0])
        dm.timing_reset()
        dm.bin_gram_w(m.f_k, f_raw)
        b_ms.append(dm.timing()["other"][0])
    dm.set_option("timing", 0)
    t0 = time.perf_counter()
    out = amd_fes.histogram_fes_labels(m, u_n, labels)
    whole_s = time.perf_counter() - t0
    dm.close()
    b_med = float(np.median(b_ms))
    return dict(K=K, N=N, grid=f"{side} x {side}", labels="random" if shuffled else "localised per state", nbins=nbins, set_bins_s=set_bins_s, **info, pass_a_kernel_ms=a_ms,
                pass_b_kernel_ms=b_ms, pass_a_kernel_ms_median=float(np.median(a_ms)), pass_b_kernel_ms_median=b_med,
                pass_b_matrix_bytes=8 * K * N, pass_b_fraction_of_8TBps=8.0 * K * N / (b_med * 1e-3) / HBM_BYTES_PER_S,
                pass_b_fraction_of_8TBps_per_sweep=info["sweeps"] * 8.0 * K * N / (b_med * 1e-3) / HBM_BYTES_PER_S,
                histogram_fes_labels_s=whole_s, df_max=float(np.max(out["df_i"])))


def part_iii():
    K, N, B = 32, 1_000_000, 20
    O_k, K_k, N_k = np.linspace(0.0, 4.0, K), np.ones(K), np.full(K, N // K)
    x_n, u_kn, N_k, _ = ts.harmonic_u_kn(O_k, K_k, N_k, seed=0)
    u_n = 0.5 * (x_n - 2.0) ** 2
    edges = np.linspace(-3.0, 7.0, 101)
    t0 = time.perf_counter()
    fes = pymbar_amd.FES(u_kn, N_k)
    init_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    fes.generate_fes(u_n, x_n, histogram_parameters={"bin_edges": edges})
    plain_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    fes.generate_fes(u_n, x_n, histogram_parameters={"bin_edges": edges}, n_bootstraps=B, seed=3)
    boot_s = time.perf_counter() - t0
    centers = 0.5 * (edges[1:] + edges[:-1])
    t0 = time.perf_counter()
    r = fes.get_fes(centers, uncertainty_method="bootstrap")
    get_s = time.perf_counter() - t0
    fes.mbar.close()
    return dict(K=K, N=N, n_bootstraps=B, populated_bins=int(len(fes.histogram_data["f"])), fes_init_s=init_s,
                generate_fes_no_bootstraps_s=plain_s, generate_fes_20_bootstraps_s=boot_s,
                s_per_replicate=(boot_s - plain_s) / B, get_fes_bootstrap_s=get_s, df_median=float(np.nanmedian(r["df_i"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--skip", default="")
    a = ap.parse_args()
    skip = set(a.skip.split(",")) if a.skip else set()
    out = dict(bench="histogram_labels")
    if "i" not in skip:
        out["i"] = part_i(a.reps)
        print(json.dumps({"i": out["i"]}), file=sys.stderr, flush=True)
    for name, shuffled in (("ii", False), ("ii_shuffled", True)):
        if name not in skip:
            out[name] = part_ii(a.reps, shuffled)
            print(json.dumps({name: out[name]}), file=sys.stderr, flush=True)
    if "iii" not in skip:
        out["iii"] = part_iii()
        print(json.dumps({"iii": out["iii"]}), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
