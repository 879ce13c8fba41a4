"""pymbar_amd.other_estimators on the MI355X: the device against the reference's answers (tests/golden/other_estimators.npz) and
against the long-double oracle (tests/bar_oracle.py): bar_zero and the uncertainty sums within their bounds, identical bits for
identical calls and for a problem inside a ragged batch, +inf work values, NaN input; then the case set of tests/bar_cases.py
(every branch of the evaluation pass and of the moment stages, every chunk seam) within its derived bounds, and every exit of the
device root find bit for bit against the host-driven state machine."""
import json
import math

import numpy as np
import pytest

from pymbar_amd import other_estimators as oe
from pymbar_amd import testsystems
from pymbar_amd.utils import BoundsError, ConvergenceError, ParameterError
from tests import bar_cases as bc
from tests import bar_oracle as orc
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
ERRORS = {"ConvergenceError": ConvergenceError, "BoundsError": BoundsError}


@pytest.fixture(scope="module")
def gold():
    g = load_golden("other_estimators.npz")
    for k in ("cases", "exps", "overlaps", "gw"):
        g[k] = json.loads(str(g[k]))
    return g


def case_data(gold, key):
    if key in gold["gw"]:
        return testsystems.gaussian_work_example(**gold["gw"][key])
    return gold[f"{key}_wF"], gold[f"{key}_wR"]


def test_device_matches_reference_every_case(gold):
    by_data = {}
    for c in gold["cases"]:
        by_data.setdefault(c["data"], []).append(c)
    for key, cases in by_data.items():
        w_F, w_R = case_data(gold, key)
        for c in cases:
            if c["error"]:
                with pytest.raises(ERRORS[c["error"]], match="problem 0"):
                    oe.bar(w_F, w_R, **c["kwargs"])
                continue
            r = oe.bar(w_F, w_R, **c["kwargs"])
            assert r["Delta_f"] == pytest.approx(c["Delta_f"], rel=1e-11, abs=1e-13), c["name"]
            if c["dDelta_f"] is None:
                assert "dDelta_f" not in r
            elif math.isnan(c["dDelta_f"]):
                assert np.isfinite(r["dDelta_f"]) and r["dDelta_f"] > 0, c["name"]
            else:
                assert r["dDelta_f"] == pytest.approx(c["dDelta_f"], rel=1e-10), c["name"]
            if c["margin"] > 10 and c["fmin"] > 1e-13:
                # the evaluation count of the device's root find equals the reference's bar_zero calls
                with oe.DeviceBAR([w_F], [w_R]) as h:
                    st = _states_for(h, c["kwargs"])
                    h.solve(st)
                    assert st[0].nzero == c["calls"], c["name"]


def _states_for(h, kw):
    method, maxit = oe._check_options(kw.get("method", "false-position"), kw.get("uncertainty_method", "BAR"),
                                      kw.get("iterated_solution", True), kw.get("maximum_iterations", 500))
    st = (oe._lib.BarState * h.P)()
    m = h.moments()
    for p in range(h.P):
        s = st[p]
        s.method = oe.METHODS[method]
        s.iterated = int(bool(kw.get("iterated_solution", True)))
        s.maximum_iterations = maxit
        s.relative_tolerance = kw.get("relative_tolerance", 1e-12)
        s.DeltaF = kw.get("DeltaF", 0.0)
        s.UpperB = float(oe._exp_delta_f(m[p, 0, 0], float(h.n_F[p])))
        s.LowerB = float(-oe._exp_delta_f(m[p, 1, 0], float(h.n_R[p])))
    return st


def test_exp_matches_reference(gold):
    for e in gold["exps"]:
        w = gold[f"{e['data']}_w"]
        for fn, want in ((oe.exp, e["exp"]), (oe.exp_gauss, e["exp_gauss"])):
            r = fn(w, **e["kwargs"])
            assert r["Delta_f"] == pytest.approx(want[0], rel=1e-13, abs=1e-14), e["name"]
            if e["kwargs"].get("compute_uncertainty", True):
                tol = 1e-10 if e["kwargs"].get("is_timeseries") else 1e-13
                assert r["dDelta_f"] == pytest.approx(want[1], rel=tol), e["name"]


def test_bar_overlap_matches_reference(gold):
    for key, want in gold["overlaps"].items():
        w_F, w_R = case_data(gold, key)
        assert oe.bar_overlap(w_F, w_R) == pytest.approx(want, rel=1e-8)


@pytest.mark.parametrize("N", [1, 37, 4096, 100_000, 1_000_000])
def test_bar_zero_against_long_double_oracle(N):
    rng = np.random.RandomState(N)
    w_F = rng.randn(N) * 3.0 + 2.0
    w_R = rng.randn(N + N // 3) * 5.0 - 1.0
    dfs = [-800.0, -250.5, -37.0, -1.0, 0.0, 0.3, 2.0, 40.0, 333.3, 800.0]
    with oe.DeviceBAR([w_F], [w_R]) as h:
        for d in dfs:
            out = h.zero([d])[0]
            F, ln, ld, ln2, ld2 = orc.log_sums(w_F, w_R, d)
            bound = 1e-14 + 4e-16 * (abs(float(ln)) + abs(float(ld)))
            assert abs(out[0] - float(F)) <= bound, (N, d, out[0] - float(F), bound)
            for got, want in zip(out[1:], (ln, ld, ln2, ld2)):
                assert abs(got - float(want)) <= 1e-14 + 4e-16 * abs(float(want)), (N, d)


def test_uncertainty_moments_against_oracle():
    w_F, w_R = testsystems.gaussian_work_example(N_F=300_000, N_R=200_000, mu_F=None, DeltaF=1.0, sigma_F=2.0, seed=4)
    with oe.DeviceBAR([w_F], [w_R]) as h:
        for d in (0.0, 1.0, 7.5):
            out = h.zero([d])[0]
            _, ln, ld, ln2, ld2 = orc.log_sums(w_F, w_R, d)
            TF, TR = float(w_F.size), float(w_R.size)
            for got, want, T in zip(out[1:], (ln, ld, ln2, ld2), (TF, TR, TF, TR)):
                a = np.exp(got) / T
                b = float(np.exp(want) / T)
                assert a == pytest.approx(b, rel=1e-13)
        m = h.moments()
        for side, w in enumerate((w_F, w_R)):
            want = orc.side_moments(w)
            assert m[0, side, 0] == pytest.approx(float(want[0]), rel=1e-15, abs=1e-14)
            for k in range(1, 5):
                assert m[0, side, k] == pytest.approx(float(want[k]), rel=1e-13)


def test_identical_calls_identical_bits():
    w_F, w_R = testsystems.gaussian_work_example(N_F=2_000_000, N_R=1_500_000, mu_F=None, DeltaF=1.0, sigma_F=2.0, seed=9)
    a = [oe.bar(w_F, w_R, method=m) for m in ("false-position", "bisection", "self-consistent-iteration")]
    b = [oe.bar(w_F, w_R, method=m) for m in ("false-position", "bisection", "self-consistent-iteration")]
    for x, y in zip(a, b):
        assert x["Delta_f"].tobytes() == y["Delta_f"].tobytes() and x["dDelta_f"].tobytes() == y["dDelta_f"].tobytes()
    assert oe.exp(w_F)["dDelta_f"].tobytes() == oe.exp(w_F)["dDelta_f"].tobytes()


def test_ragged_batch_gives_single_call_bits():
    C = oe.CHUNK
    sizes = [1, 2, C - 1, C, C + 1, 1000, 1_000_000]
    rng = np.random.RandomState(5)
    w_F = [rng.randn(n) * 2.0 + 1.0 + 0.1 * k for k, n in enumerate(sizes)]
    w_R = [rng.randn(sizes[-1 - k]) * 2.0 - 1.0 for k in range(len(sizes))]
    for kw in ({}, {"method": "bisection", "uncertainty_method": "MBAR"}, {"method": "self-consistent-iteration"},
               {"iterated_solution": False}):
        r = oe.bar_batch(w_F, w_R, **kw)
        for p in range(len(sizes)):
            s = oe.bar(w_F[p], w_R[p], **kw)
            assert r["Delta_f"][p].tobytes() == s["Delta_f"].tobytes(), (p, kw)
            assert r["dDelta_f"][p].tobytes() == s["dDelta_f"].tobytes(), (p, kw)
    with oe.DeviceBAR(w_F, w_R) as h:
        z = h.zero(0.25)
    for p in range(len(sizes)):
        assert z[p, 0] == oe.bar_zero(w_F[p], w_R[p], 0.25)


def test_plus_inf_work_values_give_the_exact_answer():
    w_F, w_R = testsystems.gaussian_work_example(N_F=5000, N_R=5000, mu_F=None, DeltaF=1.0, sigma_F=1.5, seed=2)
    wi_F = np.concatenate([w_F[:2000], [np.inf] * 30, w_F[2000:]])
    wi_R = np.concatenate([w_R, [np.inf] * (2 * oe.CHUNK)])  # whole chunks of +inf too
    r = oe.bar(wi_F, wi_R)
    assert r["Delta_f"] != 0.0 and np.isfinite(r["dDelta_f"])
    assert abs(float(orc.log_sums(wi_F, wi_R, r["Delta_f"])[0])) < 1e-12
    e = oe.exp(wi_F)
    want = -(float(orc.side_moments(wi_F)[0]) - np.log(wi_F.size))
    assert e["Delta_f"] == pytest.approx(want, rel=1e-14)


def test_nan_and_minus_inf_raise():
    w = np.linspace(-1.0, 1.0, 100)
    for bad in (np.nan, -np.inf):
        x = w.copy()
        x[50] = bad
        with pytest.raises(ParameterError):
            oe.bar(x, w)
        with pytest.raises(ParameterError):
            oe.bar(w, x)
        with pytest.raises(ParameterError):
            oe.exp(x)
    with pytest.raises(ParameterError, match="problem 1"):
        oe.bar_batch([w, w], [w, []])


# ---- every branch, chunk seam and root-find exit (tests/bar_cases.py) ----------------------------------------------------------------
@pytest.fixture(scope="module")
def single_handle_zero():
    """h.zero(DeltaF) of every case and DeltaF in a handle of its own, once: {(case name, k): [5]}"""
    out = {}
    for c in bc.cases():
        with oe.DeviceBAR([c["w_F"]], [c["w_R"]]) as h:
            for k, d in enumerate(c["dfs"]):
                out[c["name"], k] = h.zero([d])[0]
    return out


def test_evaluation_pass_every_branch_against_oracle(single_handle_zero):
    """All five outputs of every case within their derived bounds of the long-double oracle (error / bound <= 1); where the
    oracle gives -inf or NaN the device gives the same class, and never a NaN where the oracle is finite."""
    worst = np.zeros(5)
    for c in bc.cases():
        for k, d in enumerate(c["dfs"]):
            q = bc.zero_ratios(c, k, single_handle_zero[c["name"], k])
            print(f"{c['name']:28s} DeltaF {d:<12g} error / bound", np.round(q, 3))
            worst = np.maximum(worst, q)
            assert np.all(q <= 1.0), (c["name"], d, q)
    print("worst error / bound (F, l1F, l1R, l2F, l2R):", worst)


def test_evaluation_pass_ragged_batch_gives_single_handle_bits(single_handle_zero):
    """All cases as ONE ragged handle, a DeltaF per problem: the bits of the single handles (which the test above holds to the
    oracle)."""
    cs = bc.cases()
    with oe.DeviceBAR([c["w_F"] for c in cs], [c["w_R"] for c in cs]) as h:
        for pick in (0, -1):
            z = h.zero(np.array([c["dfs"][pick] for c in cs]))
            for p, c in enumerate(cs):
                k = pick % len(c["dfs"])
                assert all(bc.same_bits(a, b) for a, b in zip(z[p], single_handle_zero[c["name"], k])), (c["name"], k)


def test_moments_every_stage_against_oracle():
    """h.moments() of every case, and of one-sided handles for the forward sides, within the bounds of bar_cases.moment_bounds;
    inf / NaN where the oracle has them (+inf work values: an infinite mean)."""
    cs = bc.cases()
    worst = np.zeros(5)
    with oe.DeviceBAR([c["w_F"] for c in cs], [c["w_R"] for c in cs]) as h:
        two = h.moments()
    with oe.DeviceBAR([c["w_F"] for c in cs]) as h:
        one = h.moments()
    for p, c in enumerate(cs):
        want = bc.oracle_moments(c)
        for label, w, got, wnt in (("F", c["w_F"], two[p, 0], want[0]), ("R", c["w_R"], two[p, 1], want[1]),
                                   ("one-sided", c["w_F"], one[p, 0], want[0])):
            q = bc.moment_ratios(w, got, wnt)
            print(f"{c['name']:28s} {label:9s} error / bound", np.round(q, 3))
            worst = np.maximum(worst, q)
            assert np.all(q <= 1.0), (c["name"], label, q, got, wnt)
        assert one[p, 1, 0] == -np.inf and np.all(one[p, 1, 1:] == 0.0)  # the empty reverse side
    # a handle of its own sees the same chunks: identical bits
    for c in (cs[0], cs[len(cs) // 2]):
        with oe.DeviceBAR([c["w_F"]], [c["w_R"]]) as h:
            m = h.moments()
        p = cs.index(c)
        assert all(bc.same_bits(a, b) for a, b in zip(m.ravel(), two[p].ravel())), c["name"]
    print("worst error / bound (lse, sum x, sq x, sum w, sq w):", worst)


def rootfind_problems(gold):
    """the golden data sets with their EXP bracket, a bracket above the root (it has to widen) and UpperB == LowerB == 0, and the
    dyadic problems with their hand-set brackets"""
    keys = ["ho", "ex", "uneq", "one", "poor", "widen"]
    data = [case_data(gold, k) for k in keys]
    with oe.DeviceBAR([d[0] for d in data], [d[1] for d in data]) as h:
        m = h.moments()
    out = []
    for p, (key, (w_F, w_R)) in enumerate(zip(keys, data)):
        U = float(oe._exp_delta_f(m[p, 0, 0], float(len(w_F))))
        L = float(-oe._exp_delta_f(m[p, 1, 0], float(len(w_R))))
        hi, gap = max(U, L), abs(U - L)
        out += [(f"{key}-exp", w_F, w_R, U, L), (f"{key}-above", w_F, w_R, hi + 3.0 * gap + 1.0, hi + 2.0 * gap + 0.5),
                (f"{key}-zero", w_F, w_R, 0.0, 0.0)]
    return out + bc.dyadic_problems()


# the exits each method has to reach on these problems (together: every name of bar_cases.EXITS)
ROOTFIND_EXITS = {0: {"DONE", "NOT_CONVERGED", "NAN_BRACKET", "FNew==0", "no-evaluation", "widened"},
                  1: {"DONE", "NOT_CONVERGED", "BOUNDS", "NAN_BRACKET", "widened"},
                  2: {"DONE", "NOT_CONVERGED"}}


@pytest.mark.parametrize("method", [0, 1, 2])
def test_root_find_every_exit_bit_for_bit(gold, method):
    """h.solve on hand-set states against mbar_bar_step_host driven in lockstep on copies of the same states, every request
    answered by h.zero: every field of the final state, and the moments against zero() at the final DeltaF, bit for bit."""
    problems = rootfind_problems(gold)
    rootfind_seen = set()
    with oe.DeviceBAR([pr[1] for pr in problems], [pr[2] for pr in problems]) as h:
        for config in [c for c in bc.rootfind_configs() if c[0] == method]:
            dev = bc.make_states(problems, config)
            host = bc.copy_states(dev)
            passes = h.solve(dev)
            hpasses, widened = bc.drive_lockstep(h.zero, host)
            final = h.zero(np.array([(s.DeltaF if s.iterated else s.DeltaF_initial) for s in host]))
            for p, pr in enumerate(problems):
                bad = bc.state_mismatches(dev[p], host[p])
                assert not bad, (pr[0], config, bad, [(getattr(dev[p], f), getattr(host[p], f)) for f in bad])
                want = final[p, 1:] if (config[3] and host[p].status == oe.DONE) else np.zeros(4)
                assert all(bc.same_bits(a, b) for a, b in zip(dev[p].moments, want)), (pr[0], config)
                assert dev[p].moments_pending == 0
                rootfind_seen.update(bc.exits_of(dev[p], widened[p]))
            assert passes >= hpasses  # (the device enqueues whole groups of passes)
    assert set.union(*ROOTFIND_EXITS.values()) == set(bc.EXITS)
    assert rootfind_seen >= ROOTFIND_EXITS[method], ROOTFIND_EXITS[method] - rootfind_seen


def test_bar_batch_error_names_the_failing_problem(gold):
    """One problem that does not converge among good ones: the error names its index, and without it the good problems get the
    bits they have alone."""
    keys = ["ho", "poor", "ex", "uneq"]
    data = [case_data(gold, k) for k in keys]
    kw = {"method": "self-consistent-iteration"}
    for order in ([0, 1, 2, 3], [1, 0, 2, 3], [0, 2, 3, 1]):
        with pytest.raises(ConvergenceError, match=f"problem {order.index(1)}:"):
            oe.bar_batch([data[i][0] for i in order], [data[i][1] for i in order], **kw)
    good = [0, 2, 3]
    r = oe.bar_batch([data[i][0] for i in good], [data[i][1] for i in good], **kw)
    for p, i in enumerate(good):
        s = oe.bar(data[i][0], data[i][1], **kw)
        assert r["Delta_f"][p].tobytes() == s["Delta_f"].tobytes() and r["dDelta_f"][p].tobytes() == s["dDelta_f"].tobytes()
    # BAR_BOUNDS: a bisection whose UpperB is the exact root, among good problems, through the handle
    problems = [(k,) + data[i] + (None, None) for k, i in zip(("ho", "ex"), (0, 2))]
    problems.insert(1, bc.dyadic_problems()[0])
    with oe.DeviceBAR([pr[1] for pr in problems], [pr[2] for pr in problems]) as h:
        m = h.moments()
        full = [(n, a, b, float(oe._exp_delta_f(m[p, 0, 0], float(len(a)))) if U is None else U,
                 float(-oe._exp_delta_f(m[p, 1, 0], float(len(b)))) if L is None else L) for p, (n, a, b, U, L) in enumerate(problems)]
        st = bc.make_states(full, (1, 1, 500, 1), starts=(0.0,))
        h.solve(st)
    assert [s.status for s in st] == [oe.DONE, oe.BOUNDS, oe.DONE]
    for p, i in ((0, 0), (2, 2)):
        s = oe.bar(data[i][0], data[i][1], method="bisection")
        assert st[p].DeltaF == s["Delta_f"] and oe._uncertainty(st[p].moments, *[float(len(x)) for x in data[i]], "BAR") == s["dDelta_f"]
