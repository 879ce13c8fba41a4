"""Branch census and measured errors of the BAR and EXP sums, and the exits of the device root find
(profiles/bar_branch_matrix.txt).

Evaluation pass: for every case of tests/bar_cases.py (value pattern x side lengths) and every DeltaF of the case, the model's
census of both sides (chunks and their kinds -- all +inf, x_min > 0, x_min <= 0 without a positive x, straddling --, the elements
in each form of ``lin`` as positive / straddle / non-positive, the elements with x == 0, the largest shift difference of the
side, the padded slots of the last chunk, the trips of the strided merge loop) and the device's error / bound of F, log sum_F f,
log sum_R f and the two log sums of squares against the long-double oracle (the tests assert a ratio <= 1; 0 stands for an
oracle value of -inf or NaN that the device reproduces).

EXP moments: per case and side, the error / bound of logsumexp(-w), sum x, sum (x - mean)^2, sum w, sum (w - mean)^2.

Root find: per configuration (method, iterated, maximum_iterations, want_moments) of tests/test_gpu_other_estimators.py, the
passes of the device and of the host-driven lockstep run, the fields in which the final states differ (the test asserts none)
and how many problems reached each exit.

    python tools/bar_branch_matrix.py > profiles/bar_branch_matrix.txt
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

from pymbar_amd import other_estimators as oe  # noqa: E402
from tests import bar_cases as bc  # noqa: E402
from tests import test_gpu_other_estimators as tg  # noqa: E402
from tests.conftest import load_golden  # noqa: E402

METHODS = ("false-position", "bisection", "self-consistent")


def fmt(q):
    return " ".join(f"{v:.3f}" for v in q)


def evaluation_pass():
    print("evaluation pass: model census | error / bound of F, l1F, l1R, l2F, l2R against the long-double oracle")
    worst = np.zeros(5)
    for c in bc.cases():
        with oe.DeviceBAR([c["w_F"]], [c["w_R"]]) as h:
            for k, d in enumerate(c["dfs"]):
                q = bc.zero_ratios(c, k, h.zero([d])[0])
                worst = np.maximum(worst, q)
                _, cs = bc.model_zero(c["w_F"], c["w_R"], d)
                print(f"{c['name']:28s} DeltaF {d:<12g} {bc.census_line(cs)} | {fmt(q)}")
    print(f"worst: {fmt(worst)}")


def moments():
    print()
    print("EXP moments: chunks, merge trips, chunks of +inf, +inf values | error / bound of lse, sum x, sq x, sum w, sq w")
    cs = bc.cases()
    with oe.DeviceBAR([c["w_F"] for c in cs], [c["w_R"] for c in cs]) as h:
        m = h.moments()
    worst = np.zeros(5)
    for p, c in enumerate(cs):
        for side, (w, want) in enumerate(zip((c["w_F"], c["w_R"]), bc.oracle_moments(c))):
            q = bc.moment_ratios(w, m[p, side], want)
            worst = np.maximum(worst, q)
            mc = bc.model_moments(w)[1]
            print(f"{c['name']:28s} {'FR'[side]} chunks {mc['chunks']:3d} trips {mc['trips']} inf chunks {mc['all_inf']:3d} "
                  f"inf values {mc['n_inf']:5d} | {fmt(q)}")
    print(f"worst: {fmt(worst)}")


def root_find():
    print()
    print("root find: device passes / host-driven passes | differing fields | problems per exit")
    gold = load_golden("other_estimators.npz")
    gold["gw"] = json.loads(str(gold["gw"]))
    problems = tg.rootfind_problems(gold)
    print("problems:", " ".join(pr[0] for pr in problems))
    with oe.DeviceBAR([pr[1] for pr in problems], [pr[2] for pr in problems]) as h:
        for config in bc.rootfind_configs():
            dev = bc.make_states(problems, config)
            host = bc.copy_states(dev)
            passes = h.solve(dev)
            hpasses, widened = bc.drive_lockstep(h.zero, host)
            bad = sorted({f for p in range(len(problems)) for f in bc.state_mismatches(dev[p], host[p])})
            count = {}
            for p in range(len(problems)):
                for e in bc.exits_of(dev[p], widened[p]):
                    count[e] = count.get(e, 0) + 1
            print(f"{METHODS[config[0]]:15s} iterated {config[1]} maxit {config[2]:3d} moments {config[3]} passes {passes:4d} / {hpasses:4d}"
                  f" | differing: {bad or 'none'} | " + " ".join(f"{e} {count[e]}" for e in bc.EXITS if e in count))


if __name__ == "__main__":
    evaluation_pass()
    moments()
    root_find()
