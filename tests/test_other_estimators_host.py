"""pymbar_amd.other_estimators on the CPU: the root find's state machine (the library's host entry point mbar_bar_step_host, the
code the device runs) against a fresh restatement of the reference's loop, and the whole public module with the device handle
replaced by the long-double stand-in (``OracleBAR`` for ``DeviceBAR``) against the reference's answers
(tests/golden/other_estimators.npz, tests/golden/make_golden_other_estimators.py); and the branch model of the device sums
(tests/bar_cases.py): its census over the case set, the model against the long-double oracle, its seeded errors, and the dyadic
root-find construction on the host."""
import json
import math

import numpy as np
import pytest

from pymbar_amd import testsystems
from pymbar_amd.utils import BoundsError, ConvergenceError, ParameterError
from tests import bar_oracle as orc
from tests.conftest import load_golden

METHODS = ("false-position", "bisection", "self-consistent-iteration")
ERRORS = {"ConvergenceError": ConvergenceError, "BoundsError": BoundsError}


@pytest.fixture(scope="module")
def gold():
    g = load_golden("other_estimators.npz")
    for k in ("cases", "exps", "overlaps", "gw"):
        g[k] = json.loads(str(g[k]))
    return g


@pytest.fixture
def oe(monkeypatch):
    from pymbar_amd import other_estimators

    monkeypatch.setattr(other_estimators, "DeviceBAR", orc.OracleBAR)
    return other_estimators


def case_data(gold, key):
    if key in gold["gw"]:
        return testsystems.gaussian_work_example(**gold["gw"][key])
    return gold[f"{key}_wF"], gold[f"{key}_wR"]


def small_cases(gold):
    return [c for c in gold["cases"] if not c["data"].startswith(("gw1e6", "gw1e7"))]


# ---- the state machine against the restatement ----------------------------------------------------------------------------------
def compare(F, method, **kw):
    with np.errstate(all="ignore"):
        return _compare(F, method, **kw)


def _compare(F, method, **kw):
    st, trace = orc.drive_host(F, orc.new_state(method, **kw))
    status, delta, rtrace = orc.restated_bar(F, method, **kw)
    # every evaluated DeltaF, bit for bit (NaN matches NaN)
    assert len(trace) == len(rtrace)
    assert all(a == b or (math.isnan(a) and math.isnan(b)) for a, b in zip(trace, rtrace))
    assert st.status == status
    assert st.nzero == len(rtrace)
    if status in (1, 4):
        assert st.DeltaF == delta or (math.isnan(st.DeltaF) and math.isnan(delta))
    return st


def exp_bounds(w_F, w_R):
    m = orc.OracleBAR([w_F], [w_R]).moments()
    TF, TR = float(len(w_F)), float(len(w_R))
    return -(np.float64(m[0, 0, 0]) - np.log(TF)), (np.float64(m[0, 1, 0]) - np.log(TR))


@pytest.mark.parametrize("key", ["ho", "ex", "uneq", "one", "poor", "widen"])
@pytest.mark.parametrize("method", METHODS)
def test_step_host_matches_restatement_on_oracle_F(gold, key, method):
    w_F, w_R = case_data(gold, key)
    U, L = exp_bounds(w_F, w_R)

    def F(x):
        return float(orc.log_sums(w_F, w_R, x)[0])

    compare(F, method, UpperB=U, LowerB=L)
    compare(F, method, UpperB=U, LowerB=L, maximum_iterations=2)
    compare(F, method, UpperB=U, LowerB=L, DeltaF=2.0, iterated=False)
    compare(F, method, UpperB=U, LowerB=L, relative_tolerance=1e-6)


SYNTH = {
    "linear": lambda x: 0.7 - 0.3 * x,
    "cubic": lambda x: float(-(np.float64(x) - 1.25) ** 3 - 0.1 * (np.float64(x) - 1.25)),
    "wiggly": lambda x: math.sin(3.0 * x) + 0.5 - 0.2 * x,
    "exact_zero": lambda x: 1.0 - x,
    "identity": lambda x: x,
    "shift": lambda x: x - 1.0,
    "flat": lambda x: 1.0 if x == x else float("nan"),  # (NaN at NaN, as bar_zero: the widening then ends)
    "nan_inside": lambda x: float("nan") if 0.2 < x < 0.8 else 1.0 - x,
    "nan": lambda x: float("nan"),
}


@pytest.mark.parametrize("name", sorted(SYNTH))
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("bounds", [(2.0, -1.0), (-1.0, 2.0), (0.0, 0.0), (3.0, 2.5), (0.5, 0.5)])
@pytest.mark.parametrize("maxit", [0, 1, 2, 500])
def test_step_host_matches_restatement_on_synthetic_F(name, method, bounds, maxit):
    for start in (0.0, 1.0, -0.3):
        for iterated in (True, False):
            compare(SYNTH[name], method, UpperB=bounds[0], LowerB=bounds[1], DeltaF=start, maximum_iterations=maxit,
                    iterated=iterated)


def test_step_host_reaches_every_outcome():
    """The branches of the reference's loop that the synthetic functions above are there to reach."""
    st = compare(SYNTH["exact_zero"], "false-position", UpperB=2.0, LowerB=0.0)  # FNew == 0
    assert st.status == 1 and st.DeltaF == 1.0 and st.relative_change == 1e-15
    st = compare(SYNTH["identity"], "false-position", UpperB=0.0, LowerB=0.0)  # both ends 0: no evaluation in the loop
    assert st.status == 1 and st.nzero == 2
    st = compare(SYNTH["identity"], "self-consistent-iteration", DeltaF=1.0)  # DeltaF == 0 breaks
    assert st.status == 1 and st.DeltaF == 0.0 and st.iteration == 0
    st = compare(SYNTH["shift"], "self-consistent-iteration", maximum_iterations=1)  # a break on the last pass still raises
    assert st.status == 4 and st.iteration == 1
    st = compare(SYNTH["shift"], "self-consistent-iteration", maximum_iterations=2)
    assert st.status == 1
    st = compare(SYNTH["nan"], "bisection", UpperB=1.0, LowerB=-1.0)
    assert st.status == 2 and st.nzero == 2
    st = compare(SYNTH["nan_inside"], "bisection", UpperB=2.0, LowerB=-1.0)
    assert st.status == 3
    st = compare(SYNTH["linear"], "bisection", UpperB=3.0, LowerB=2.5)  # widening (first narrowing: U > L)
    assert st.status == 1 and st.nzero > 6
    st = compare(SYNTH["flat"], "false-position", UpperB=1.0, LowerB=-1.0)  # widens until the bracket overflows to NaN
    assert st.status == 3 and st.nzero > 2000
    st = compare(SYNTH["linear"], "self-consistent-iteration", maximum_iterations=1, iterated=False)
    assert st.status == 1 and st.nzero == 2


# ---- the module on the stand-in against the reference ---------------------------------------------------------------------------
def run_case(oe, gold, c):
    w_F, w_R = case_data(gold, c["data"])
    if c["error"]:
        with pytest.raises(ERRORS[c["error"]], match="problem 0"):
            oe.bar(w_F, w_R, **c["kwargs"])
        return None
    return oe.bar(w_F, w_R, **c["kwargs"])


def check_case(r, c, nzero):
    if r is None:
        return
    assert r["Delta_f"] == pytest.approx(c["Delta_f"], rel=1e-11, abs=1e-13), c["name"]
    if c["dDelta_f"] is None:
        assert "dDelta_f" not in r
    elif math.isnan(c["dDelta_f"]):
        # the reference's uncertainty sums underflow (work spread of ~1e3 kT) and give NaN; the exact sums do not
        assert np.isfinite(r["dDelta_f"]) and r["dDelta_f"] > 0, c["name"]
    else:
        assert r["dDelta_f"] == pytest.approx(c["dDelta_f"], rel=1e-10), c["name"]
    if c["margin"] > 10 and c["fmin"] > 1e-13:
        assert nzero == c["calls"], c["name"]


def test_module_on_standin_matches_reference(oe, gold):
    for c in small_cases(gold):
        r = run_case(oe, gold, c)
        check_case(r, c, orc.OracleBAR.last_states[0].nzero if r is not None else None)


def test_bar_zero_on_standin(oe, gold):
    w_F, w_R = case_data(gold, "ho")
    for d in (-3.0, 0.0, 0.685, 5.0):
        assert oe.bar_zero(w_F, w_R, d) == float(orc.log_sums(w_F, w_R, d)[0])


def test_exp_on_standin_matches_reference(oe, gold, monkeypatch):
    from pymbar_amd import timeseries
    from tests import timeseries_oracle

    monkeypatch.setattr(timeseries, "DeviceACF", timeseries_oracle.OracleACF)
    for e in gold["exps"]:
        w = gold[f"{e['data']}_w"]
        for fn, want in ((oe.exp, e["exp"]), (oe.exp_gauss, e["exp_gauss"])):
            r = fn(w, **e["kwargs"])
            assert r["Delta_f"] == pytest.approx(want[0], rel=1e-13, abs=1e-14), e["name"]
            if e["kwargs"].get("compute_uncertainty", True):
                assert r["dDelta_f"] == pytest.approx(want[1], rel=1e-13 if "is_timeseries" not in e["kwargs"] else 1e-10), e["name"]
            else:
                assert "dDelta_f" not in r


def test_bar_batch_on_standin_equals_single_calls(oe, gold):
    keys = ["ho", "ex", "uneq", "one", "widen"]
    data = [case_data(gold, k) for k in keys]
    for kw in ({}, {"method": "bisection"}, {"method": "self-consistent-iteration", "uncertainty_method": "MBAR"}):
        r = oe.bar_batch([d[0] for d in data], [d[1] for d in data], **kw)
        for p, d in enumerate(data):
            s = oe.bar(d[0], d[1], **kw)
            assert r["Delta_f"][p] == s["Delta_f"] and r["dDelta_f"][p] == s["dDelta_f"]


def test_bar_batch_error_names_the_problem(oe, gold):
    w_F, w_R = case_data(gold, "ho")
    with pytest.raises(ConvergenceError, match="problem 1"):
        # a NaN start never converges; problem 0 does
        oe.bar_batch([w_F, w_F], [w_R, w_R], DeltaF=[0.0, np.nan], method="self-consistent-iteration")
    with pytest.raises(ParameterError, match="problem 2"):
        oe.bar_batch([w_F, w_F, w_F], [w_R, w_R, []])


def test_input_rules(oe, gold):
    w_F, w_R = case_data(gold, "ho")
    bad_nan = np.array(w_F, copy=True)
    bad_nan[3] = np.nan
    bad_inf = np.array(w_R, copy=True)
    bad_inf[7] = -np.inf
    for args in ((bad_nan, w_R), (w_F, bad_inf), ([], w_R), (w_F, [])):
        with pytest.raises(ParameterError):
            oe.bar(*args)
    with pytest.raises(ParameterError):
        oe.bar_zero(bad_nan, w_R, 0.0)
    with pytest.raises(ParameterError):
        oe.exp([])
    with pytest.raises(ParameterError):
        oe.exp_gauss([1.0, np.nan])
    with pytest.raises(ParameterError, match="method"):
        oe.bar(w_F, w_R, method="newton")
    with pytest.raises(ParameterError, match="uncertainty_method"):
        oe.bar(w_F, w_R, uncertainty_method="bootstrap")
    # float32 and lists are accepted as fp64
    r32 = oe.bar(np.asarray(w_F, np.float32), list(np.asarray(w_R, np.float32)))
    r64 = oe.bar(np.asarray(w_F, np.float32).astype(np.float64), np.asarray(w_R, np.float32).astype(np.float64))
    assert r32 == r64


def test_plus_inf_work_values_on_standin(oe, gold):
    w_F, w_R = case_data(gold, "ho")
    wi = np.concatenate([w_F, [np.inf, np.inf]])
    r = oe.bar(wi, w_R)
    # the root of the exact sums, with the two infinite values as factors of 0 (and in T_F)
    assert abs(orc.log_sums(wi, w_R, r["Delta_f"])[0]) < 1e-12
    assert r["Delta_f"] != 0.0 and np.isfinite(r["dDelta_f"])


def test_gaussian_work_example_is_the_reference_stream(gold):
    w_F, w_R = testsystems.gaussian_work_example(mu_F=None, DeltaF=1.0, seed=0)
    assert np.array_equal(w_F, gold["gwF_w"]) and np.array_equal(w_R, gold["gwR_w"])
    with pytest.raises(ValueError):
        testsystems.gaussian_work_example(mu_F=1.0, DeltaF=1.0)
    with pytest.raises(ValueError):
        testsystems.gaussian_work_example(mu_F=None, DeltaF=None)


def test_docstring_values_on_standin(oe):
    w_F, w_R = testsystems.gaussian_work_example(mu_F=None, DeltaF=1.0, seed=0)
    r = oe.bar(w_F, w_R)
    assert "{:.3f} +- {:.3f}".format(r["Delta_f"], r["dDelta_f"]) == "1.088 +- 0.050"
    r = oe.exp(w_F)
    assert "{:.3f} +- {:.3f}".format(r["Delta_f"], r["dDelta_f"]) == "1.088 +- 0.076"
    r = oe.exp_gauss(w_R)
    assert "{:.3f} +- {:.3f}".format(r["Delta_f"], r["dDelta_f"]) == "-1.073 +- 0.080"


def test_package_exports_without_touching_a_device():
    import pymbar_amd

    for name in ("bar", "bar_overlap", "bar_zero", "exp", "exp_gauss", "other_estimators"):
        assert name in pymbar_amd.__all__ and hasattr(pymbar_amd, name)


# ---- the branch model of the BAR / EXP sums (tests/bar_cases.py) --------------------------------------------------------------------
from tests import bar_cases as bc  # noqa: E402


@pytest.fixture(scope="module")
def model_runs():
    """the unmutated model on every case and DeltaF, once: [(case, k, values, census)]"""
    return [(c, k) + bc.model_zero(c["w_F"], c["w_R"], d) for c in bc.cases() for k, d in enumerate(c["dfs"])]


def test_case_set_census(model_runs):
    """Over the whole case set every chunk kind, every form of ``lin``, x == 0, a shift difference above 745, padded slots of 1
    and of 4095 and a second trip of the strided merge loop occur, and every side length occurs on both sides."""
    sides = [cs[s] for _, _, _, cs in model_runs for s in "FR"]
    for key in ("all_inf", "xmin_pos", "nonpos_only", "straddling", "n_pp", "n_straddle", "n_nonpos", "n_zero"):
        assert any(s[key] > 0 for s in sides), key
    assert any(s["shift_diff"] > 745.0 for s in sides)
    assert any(s["pad"] == 1 for s in sides) and any(s["pad"] == bc.CHUNK - 1 for s in sides)
    assert any(s["trips"] == 2 for s in sides) and all(s["trips"] in (1, 2) for s in sides)
    for side in ("w_F", "w_R"):
        assert {len(c[side]) for c in bc.cases()} >= set(bc.LENGTHS) | {bc.BIG}
    assert any(len(c["w_F"]) == len(c["w_R"]) for c in bc.cases()) and any(len(c["w_F"]) != len(c["w_R"]) for c in bc.cases())
    assert sum(len(c["w_F"]) + len(c["w_R"]) for c in bc.cases()) < 2_600_000
    # the patterns force what they are named for
    for c, k, _, cs in model_runs:
        for s in "FR":
            if c["pattern"] == "positive":
                assert cs[s]["n_straddle"] == cs[s]["n_nonpos"] == 0
            if c["pattern"] == "negative":
                assert cs[s]["n_pp"] == cs[s]["n_straddle"] == 0
            if c["pattern"] in ("zero", "straddle") and len(c["w_" + s]) > 1:
                assert cs[s]["n_zero" if c["pattern"] == "zero" else "n_straddle"] > 0
    # the moments' stages: a second merge trip, chunks of +inf, +inf inside a finite chunk
    mom = [bc.model_moments(c[side])[1] for c in bc.cases() for side in ("w_F", "w_R")]
    assert any(m["trips"] == 2 for m in mom) and any(m["all_inf"] > 0 for m in mom)
    assert any(m["n_inf"] > 0 and m["all_inf"] == 0 for m in mom) and any(m["all_inf"] == m["chunks"] for m in mom)
    # the depth of the moments' bound covers the device's tree at every length of the set
    for n in bc.LENGTHS + (bc.BIG,):
        assert bc.device_additions(n) + 1 <= 2 * bc.depth(n), n


def test_model_within_the_bounds_of_the_oracle(model_runs):
    worst = 0.0
    for c, k, got, _ in model_runs:
        q = bc.zero_ratios(c, k, got)
        worst = max(worst, q.max())
        assert np.all(q <= 1.0), (c["name"], c["dfs"][k], q)
    print("model_zero: worst error / bound", worst)
    worst = 0.0
    for c in bc.cases():
        for side, want in zip(("w_F", "w_R"), bc.oracle_moments(c)):
            q = bc.moment_ratios(c[side], bc.model_moments(c[side])[0], want)
            worst = max(worst, q.max())
            assert np.all(q <= 1.0), (c["name"], side, q)
    print("model_moments: worst error / bound", worst)


def test_every_mutation_of_the_model_is_detected():
    """Each deliberate error puts at least one case above its bound (the big pairs are left out: the others suffice)."""
    small = [c for c in bc.cases() if max(len(c["w_F"]), len(c["w_R"])) < bc.BIG]
    for mutate in bc.MUTATIONS:
        worst, where = 0.0, None
        for c in small:
            if mutate == "mom_chunkmin":
                q = max(bc.moment_ratios(c[s], bc.model_moments(c[s], mutate)[0], w).max()
                        for s, w in zip(("w_F", "w_R"), bc.oracle_moments(c)))
            else:
                q = max(bc.zero_ratios(c, k, bc.model_zero(c["w_F"], c["w_R"], d, mutate)[0]).max() for k, d in enumerate(c["dfs"]))
            if q > worst:
                worst, where = q, c["name"]
            if worst > 100.0:
                break
        print(f"mutation {mutate}: error / bound {worst:.3g} at {where}")
        assert worst > 1.0, mutate


def test_dropping_the_lo_word_of_the_shift_is_not_detectable(model_runs):
    """NOT covered, on record: without the ``lo`` word of the chunks' shifts (``mutate="nolo"``, not one of MUTATIONS) every case
    stays inside its bound, so neither this model nor the device tests can see that word."""
    worst = max(bc.zero_ratios(c, k, bc.model_zero(c["w_F"], c["w_R"], c["dfs"][k], "nolo")[0]).max() for c, k, _, _ in model_runs)
    print("without lo: worst error / bound", worst)
    assert worst <= 1.0


def test_step_host_reaches_every_exit_on_the_dyadic_construction():
    """The hand-set brackets on the dyadic pairs, F from the model: every exit the device test asserts is reached on the host."""
    problems = bc.dyadic_problems()

    def zero(d):
        with np.errstate(invalid="ignore"):
            return np.array([bc.model_zero(pr[1], pr[2], d[p])[0] for p, pr in enumerate(problems)])

    for p, (name, w_F, w_R, _, _) in enumerate(problems):
        if name.startswith("dyadic"):
            s = (w_F[0] - w_R[0]) / 2
            assert bc.model_zero(w_F, w_R, s)[0][0] == 0.0, name
            assert bc.model_zero(w_F, w_R, s + 1.0)[0][0] == -bc.model_zero(w_F, w_R, s - 1.0)[0][0], name
    seen = set()
    by_name = {}
    # (the moments pass is the device's; 0, 1 and 500 iterations reach every exit)
    for config in [c for c in bc.rootfind_configs() if c[3] == 0 and c[2] != 3]:
        st = bc.make_states(problems, config)
        _, widened = bc.drive_lockstep(zero, st)
        for p, pr in enumerate(problems):
            ex = bc.exits_of(st[p], widened[p])
            seen |= ex
            by_name.setdefault((pr[0], config[0]), set()).update(ex)
    assert seen >= set(bc.EXITS), set(bc.EXITS) - seen
    assert "BOUNDS" in by_name[("dyadic300-root", 1)] and "FNew==0" in by_name[("dyadic300-root", 0)]
    assert "FNew==0" in by_name[("dyadic4097-sym", 0)] and "widened" in by_name[("dyadic300-widen", 1)]
    assert "no-evaluation" in by_name[("dyadic64-zero", 0)] and "NAN_BRACKET" in by_name[("inf-both", 0)]
