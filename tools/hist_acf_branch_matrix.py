"""Branch census and measured errors of the binned passes and of the lag sums (profiles/hist_acf_branch_matrix.txt).

Binned passes: for every case of tests/hist_cases.py (label pattern x N x K), every weighting (none / all ones / 0 .. 3) and
every sweep count of tests/test_gpu_fes_histogram.py, the model's census of the chunk table and of the step loop (chunks, their
lengths, chunks without bins, distinct slots and handed-over samples per 64-sample step, highest slot and lane) and the worst
error / bound of lognum, wsum, diag and cross against the long-double oracle (``bin_bound``; the tests assert a ratio <= 1).

Lag sums: for the seam, long-schedule and fft cases of tests/test_gpu_timeseries.py, the longest schedule, the worst
|C_dev - C_exact| over the (origin, lag) pairs the rule evaluates (contract 1e-14) and the worst relative error of g (1e-12).

    python tools/hist_acf_branch_matrix.py > profiles/hist_acf_branch_matrix.txt
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from pymbar_amd import timeseries as ts  # noqa: E402
from tests import hist_cases as hc  # noqa: E402
from tests import test_gpu_timeseries as tt  # noqa: E402


def hist_line(case, r, weighting):
    _, c = hc.weights_of(case, weighting)
    sweeps = r["info"]["sweeps"]
    cs = hc.step_census(case["labels"], c, case["nbins"], sweeps)
    assert r["info"]["chunks"] == len(cs["chunk_len"])
    q = hc.error_ratios(r, r["oracle"])
    print(f"{case['name']:24s} {weighting:5s} sweeps {sweeps:3d} {hc.census_line(cs)} | lognum {q['lognum']:.3f} wsum {q['wsum']:.3f} "
          f"diag {q['diag']:.3f} cross {q['cross']:.3f}")


def histogram_passes():
    print("binned passes: model census | worst error / bound against the long-double oracle")
    for key in hc.case_keys():
        case = hc.make_case(*key)
        with hc.open_matrix(case) as dm:
            for w in hc.WEIGHTINGS:
                hist_line(case, hc.run_weighting(dm, case, w), w)
    for pattern in ("nine", "gaps"):
        case = hc.make_case(pattern, 300, 4500, 17)
        for sweeps in (2, 4, case["nbins"]):
            with hc.open_matrix(case, hc.part_bytes_for(case, sweeps)) as dm:
                hist_line(case, hc.run_weighting(dm, case, "mult"), "mult")
    case = hc.make_case("nine", 300, 2049, 16)
    rng = np.random.default_rng(21)
    wide = dict(case, name="nine300 v to 1605", v=rng.choice([0.0, 800.0, 1600.0], case["nbins"])[case["labels"]] + rng.uniform(0.0, 5.0, case["N"]))
    big = hc.make_case("random", 300, 262221, 2)
    for case in (wide, big):
        with hc.open_matrix(case) as dm:
            hist_line(case, hc.run_weighting(dm, case, "mult"), "mult")


def lag_sums():
    print()
    print("lag sums: longest schedule | worst |C_dev - C_exact| | worst relative error of g")

    def line(name, a, origins, nskip, **kw):
        stats = {}
        tt.check_origins(ts, a, origins, nskip, stats=stats, **kw)
        print(f"{name:44s} lags {stats.get('lags', 0):4d}  C {stats.get('C', 0.0):.2e}  g {stats.get('g', 0.0):.2e}")

    for T in (2047, 2048, 2049, 4500):
        a, b = tt.seam_pair(T)
        origins = tt.seam_origins(T)
        for fast in (False, True):
            line(f"cross T={T} fast={int(fast)} nskip=1", a, origins, 1, fast=fast, b=b)
            line(f"cross T={T} fast={int(fast)} nskip=3", a, [s for s in origins if s % 3 == 0], 3, fast=fast, b=b)
    for seed in (1, 2, 3):
        a = tt.ar1(4500, 150, seed)
        b = 0.7 * a + 0.7 * tt.ar1(4500, 150, seed + 10)
        line(f"long schedule seed={seed} auto", a, [0, 2047, 2048, 3000], 1, fast=False)
        line(f"long schedule seed={seed} cross", a, [0, 2047, 2048, 3000], 1, fast=False, b=b)
    for T in (2049, 4500):
        a, b = tt.seam_pair(T)
        line(f"fft T={T} auto", a, tt.seam_origins(T), 1, fast=False, fft=True)
        line(f"fft T={T} cross", a, tt.seam_origins(T), 1, fast=False, fft=True, b=b)


if __name__ == "__main__":
    histogram_passes()
    lag_sums()
