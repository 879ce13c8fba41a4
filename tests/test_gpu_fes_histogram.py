"""The binned passes of the label path (``mbar_ctx_set_bins`` / ``mbar_bin_lognum`` / ``mbar_bin_gram_w``, mbar_k_hist.hip) on the
MI355X against a numpy long-double oracle, against the row path on the device, and through ``pymbar_amd.FES`` against the
unmodified reference (tests/golden/fes_histogram.npz).

The cases, the oracle, the bound (``bin_bound``) and the model of the chunk table and of the step loop are in tests/hist_cases.py.
The branch cases run every label pattern of that file (1, 8, 9 and 64 distinct slots per 64-sample step, slot 63, a one-sample
chunk, a chunk without bins), N around 64 and 2048, K around ``HIST_ROWS`` = 16, without multiplicities, with all ones and with
0 .. 3, against the oracle within the unchanged bound; the model's chunk count must be the device's."""
import numpy as np
import pytest

import pymbar_amd
from pymbar_amd import fes as amd_fes
from pymbar_amd.device import DeviceMatrix
from tests.conftest import load_golden
from tests.test_fes_histogram_host import check_bootstraps, record_draws, system_b

from tests import hist_cases as hc
from tests.hist_cases import assert_within, awkward_case, bin_bound, oracle, run_passes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def case():
    return awkward_case()


@pytest.fixture(scope="module")
def single_sweep(case):
    r = run_passes(case)
    r["oracle"] = oracle(r["u"], r["logden"], r["v"], case["f"], r["labels"], r["c"], case["nbins"])
    return r


def test_binned_passes_against_long_double_oracle(case, single_sweep):
    r, o = single_sweep, single_sweep["oracle"]
    assert r["info"]["sweeps"] == 1
    assert r["info"]["chunks"] >= 30  # (random labels: a chunk closes on its 64th distinct bin, long before 2048 samples)
    assert_within(r, o)
    # the bin without a drawn sample: -inf, and zeros in its cross column and diagonal
    assert np.isneginf(r["lognum"][299]) and np.all(r["cross"][:, 299] == 0) and r["diag"][299] == 0 and r["wsum"][299] == 0
    assert o["n_i"][298] == 1
    np.testing.assert_allclose(r["wsum"][o["n_i"] > 0], 1.0, rtol=0, atol=1e-12)


def test_same_sums_whatever_the_chunking(case, single_sweep):
    o = single_sweep["oracle"]
    tiled = run_passes(case, part_bytes=200 * 1024)
    assert tiled["info"]["sweeps"] >= 3
    assert_within(tiled, o)
    live = o["n_i"] > 0
    for name, n_exp in (("lognum", 1), ("wsum", 1), ("diag", 2)):
        scale = 1.0 if name == "lognum" else np.abs(o[name]).astype(np.float64)[live]
        assert np.all(np.abs(tiled[name][live] - single_sweep[name][live]) <= 2.0 * bin_bound(o, n_exp)[live] * scale)
    assert np.all(np.abs(tiled["cross"] - single_sweep["cross"]) <= 2.0 * bin_bound(o, 2)[None, :] * np.abs(o["cross"]).astype(np.float64))
    # labels sorted (few bins per chunk) against the same columns as they came
    perm = np.argsort(case["labels"], kind="stable")
    srt = run_passes(case, perm=perm)
    assert srt["info"]["chunks"] < single_sweep["info"]["chunks"]
    o2 = oracle(srt["u"], srt["logden"], srt["v"], case["f"], srt["labels"], srt["c"], case["nbins"])
    assert_within(srt, o2)
    assert np.all(np.abs(srt["lognum"][live] - single_sweep["lognum"][live]) <= 2.0 * bin_bound(o, 1)[live])
    assert np.all(np.abs(srt["cross"] - single_sweep["cross"]) <= 2.0 * bin_bound(o, 2)[None, :] * np.abs(o["cross"]).astype(np.float64))


def test_bit_reproducibility(single_sweep):
    r = single_sweep
    for other in (r["again"], r["third"]):  # the same call again; after set_bins with the same arrays
        assert other[0].tobytes() == r["lognum"].tobytes()
        for a, b in zip(other[1], (r["cross"], r["diag"], r["wsum"])):
            assert a.tobytes() == b.tobytes()


def test_label_path_against_row_path_on_the_device():
    rng = np.random.default_rng(8)
    K, nbins, N = 5, 200, 4000
    N_k = np.full(K, N // K)
    centers = np.linspace(-0.5, 0.5, K)
    x = np.concatenate([rng.normal(c, 1.0, n) for c, n in zip(centers, N_k)])
    u_kn = 0.5 * (x[None, :] - centers[:, None]) ** 2
    u_n = 0.5 * x ** 2 + 0.3 * np.cos(3 * x)
    labels = rng.permutation(np.arange(N) % nbins)
    mbar = pymbar_amd.MBAR(u_kn, N_k)
    try:
        rows = amd_fes.histogram_fes(mbar, u_n, labels, uncertainty_method=None)
        lab = amd_fes.histogram_fes_labels(mbar, u_n, labels, uncertainty_method=None)
        print("max |f_raw(label) - f_raw(row)| =", np.max(np.abs(lab["f_raw"] - rows["f_raw"])))
        np.testing.assert_allclose(lab["f_raw"], rows["f_raw"], rtol=0, atol=1e-11)
        f_full = np.concatenate([mbar.f_k, rows["f_raw"]])
        with DeviceMatrix.empty(K + nbins, N) as aug:
            aug.copy_rows_from(mbar._dm, 0, 0, K)
            aug.fill_masked_rows(K, nbins, u_n, labels)
            aug.set_Nk(np.concatenate([N_k, np.zeros(nbins)]))
            G, _ = aug.gram_w(f_full)
        dm = mbar._dm
        dm.set_bins(nbins, labels, u_n)
        X, d, w = dm.bin_gram_w(mbar.f_k, rows["f_raw"])
        dm.set_bins(0)
        np.testing.assert_allclose(X, G[:K, K:], rtol=1e-10, atol=0)
        np.testing.assert_allclose(d, np.diag(G)[K:], rtol=1e-10, atol=0)
        np.testing.assert_allclose(w, 1.0, rtol=0, atol=1e-11)
    finally:
        mbar.close()


def test_fes_bootstraps_reproduce_reference(monkeypatch):
    umb, gold = load_golden("fes_umbrella_1d.npz"), load_golden("fes_histogram.npz")
    drawn = record_draws(monkeypatch)
    fes = pymbar_amd.FES(umb["u_kn"], umb["N_k"])
    try:
        before = fes.mbar.compute_free_energy_differences()
        fes.generate_fes(umb["u_n"], umb["x_n"], histogram_parameters={"bin_edges": umb["bin_edges"]},
                         n_bootstraps=int(gold["a_n_bootstraps"]), seed=int(gold["a_seed"]))
        check_bootstraps(fes, umb, gold, drawn)
        # multiplicities do not leak: the context has c_n = 1 again and the class returns what it returned before
        assert fes.mbar._dm._wtag is None
        after = fes.mbar.compute_free_energy_differences()
        for key in ("Delta_f", "dDelta_f"):
            np.testing.assert_array_equal(after[key], before[key])
    finally:
        fes.mbar.close()


def test_fes_label_path_reproduces_reference_2d(monkeypatch):
    gold = load_golden("fes_histogram.npz")
    u_kn, u_n, x_n = system_b(gold)
    fes = pymbar_amd.FES(u_kn, gold["b_N_k"])
    made = []
    real_init = DeviceMatrix.__init__

    def counting_init(self, *a, **kw):
        made.append(1)
        real_init(self, *a, **kw)

    monkeypatch.setattr(DeviceMatrix, "__init__", counting_init)
    try:
        fes.generate_fes(u_n, x_n, histogram_parameters={"bin_edges": [gold["b_edges_x"], gold["b_edges_y"]]})
        hd = fes.histogram_data
        assert fes.K + len(hd["f"]) > amd_fes.ROW_PATH_MAX_ROWS
        np.testing.assert_allclose(hd["f"], gold["b_f"], rtol=1e-9, atol=1e-9)
        q = gold["b_queries"]
        lo = fes.get_fes(q, reference_point="from-lowest", uncertainty_method="analytical")
        sp = fes.get_fes(q, reference_point="from-specified", fes_reference=[0, 0], uncertainty_method="analytical")
        assert not made  # the label path: no second device matrix
        np.testing.assert_allclose(lo["f_i"], gold["b_f_lowest"], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(lo["df_i"], gold["b_df_lowest"], rtol=1e-7, atol=1e-9)
        np.testing.assert_allclose(sp["f_i"], gold["b_f_specified"], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(sp["df_i"], gold["b_df_specified"], rtol=1e-7, atol=1e-9)
    finally:
        fes.mbar.close()


# ---- every branch, seam and form of the binned passes (cases and model: tests/hist_cases.py) --------------------------------------
OUT = ("lognum", "cross", "diag", "wsum")


def bits(r):
    return tuple(r[k].tobytes() for k in OUT)


def check_run(case, r, label):
    """chunk count against the model, the four outputs against the oracle within ``bin_bound``, wsum = 1 at f_bins = -lognum,
    and cross=False against cross=True"""
    o = r["oracle"]
    assert r["info"]["chunks"] == hc.model_chunks(case["labels"], case["nbins"], r["info"]["sweeps"]), label
    assert_within(r, o, label=label)
    np.testing.assert_allclose(r["wsum"][o["n_i"] > 0], 1.0, rtol=0, atol=1e-12)
    assert r["diag_only"].tobytes() == r["diag"].tobytes() and r["wsum_only"].tobytes() == r["wsum"].tobytes(), label


@pytest.mark.parametrize("key", hc.case_keys(), ids=lambda k: f"{k[0]}{k[1]}-N{k[2]}-K{k[3]}")
def test_branch_cases_three_weightings(key):
    case = hc.make_case(*key)
    with hc.open_matrix(case) as dm:
        runs = {w: hc.run_weighting(dm, case, w) for w in hc.WEIGHTINGS}
    for w, r in runs.items():
        assert r["info"]["sweeps"] == 1
        check_run(case, r, f"{case['name']} {w}")
    # without multiplicities and with all ones: the same table, and a product with 1.0 is exact
    assert runs["none"]["logden"].tobytes() == runs["ones"]["logden"].tobytes(), "logden differs: a finding about the sweep"
    assert bits(runs["none"]) == bits(runs["ones"])
    if key[2] > 1:
        empty = np.unique(case["labels"][case["labels"] >= 0])[-1]  # the bin whose samples all have multiplicity 0
        assert runs["mult"]["oracle"]["n_i"][empty] == 0 and runs["none"]["oracle"]["n_i"][empty] > 0


@pytest.fixture(scope="module")
def nine():
    return hc.make_case("nine", 300, 2049, 16)


def run_mult(case, part_bytes=None, **changed):
    case = dict(case, **changed)
    with hc.open_matrix(case, part_bytes) as dm:
        return case, hc.run_weighting(dm, case, "mult")


def test_magnitudes_per_bin_maxima(nine):
    """v per bin from {0, 800, 1600} + uniform(0, 5): against one global maximum every term of two thirds of the bins underflows"""
    rng = np.random.default_rng(21)
    v = rng.choice([0.0, 800.0, 1600.0], nine["nbins"])[nine["labels"]] + rng.uniform(0.0, 5.0, nine["N"])
    case, r = run_mult(nine, v=v)
    live = r["oracle"]["n_i"] > 0
    assert np.all(np.isfinite(r["lognum"][live])) and r["lognum"][live].min() < -1500 and r["lognum"][live].max() > -100
    assert r["oracle"]["arg"].max() > 1500  # (the bound's argument term covers the rounding of 1600)
    check_run(case, r, "magnitudes")


def test_infinite_target_potential(nine):
    """v = +inf on every counted sample of one bin (lognum -inf; zeros in pass B at f_bins = +inf) and on some samples of another
    (those are ignored); no NaN anywhere"""
    lab, c = nine["labels"], nine["c"]
    whole, part = int(lab[5]), int(lab[7])
    v = nine["v"].copy()
    v[(lab == whole) & (c > 0)] = np.inf
    some = np.flatnonzero((lab == part) & (c > 0))
    assert some.size >= 2 and whole != part
    v[some[::2]] = np.inf
    case, r = run_mult(nine, v=v)
    o = r["oracle"]
    assert o["n_i"][whole] == 0 and o["n_i"][part] == some.size - some[::2].size
    assert np.isneginf(r["lognum"][whole]) and np.isposinf(r["f_bins"][whole])
    assert np.all(r["cross"][:, whole] == 0) and r["diag"][whole] == 0 and r["wsum"][whole] == 0
    check_run(case, r, "v = +inf")  # (asserts that no output holds a NaN)


def test_infinite_entries_of_the_matrix(nine):
    rng = np.random.default_rng(22)
    u = nine["u"].copy()
    hit = rng.random(u.shape) < 0.02
    hit[np.argmin(u, axis=0), np.arange(nine["N"])] = False  # never a whole column
    u[hit] = np.inf
    case, r = run_mult(nine, u=u)
    assert np.all(np.isfinite(r["logden"]))
    check_run(case, r, "u = +inf")


@pytest.mark.parametrize("pattern", ["nine", "gaps"])
def test_sweeps_two_four_and_one_bin_each(pattern):
    case = hc.make_case(pattern, 300, 4500, 17)
    _, single = run_mult(case)
    assert single["info"]["sweeps"] == 1
    check_run(case, single, f"{pattern} 1 sweep")
    o = single["oracle"]
    live = o["n_i"] > 0
    for sweeps in (2, 4, case["nbins"]):
        _, r = run_mult(case, hc.part_bytes_for(case, sweeps))
        assert r["info"]["sweeps"] == sweeps
        check_run(case, r, f"{pattern} {sweeps} sweeps")
        for name, n_exp in (("lognum", 1), ("wsum", 1), ("diag", 2)):
            scale = 1.0 if name == "lognum" else np.abs(o[name]).astype(np.float64)[live]
            assert np.all(np.abs(r[name][live] - single[name][live]) <= 2.0 * bin_bound(o, n_exp)[live] * scale)
        assert np.all(np.abs(r["cross"] - single["cross"]) <= 2.0 * bin_bound(o, 2)[None, :] * np.abs(o["cross"]).astype(np.float64))


def test_threaded_chunk_table():
    """129 blocks of 2048 samples: two or more builder threads; the table is the single-threaded model's"""
    case = hc.make_case("random", 300, 262221, 2)
    assert (case["N"] + 2047) // 2048 // 64 >= 2
    case, r = run_mult(case)
    assert r["info"]["sweeps"] == 1 and r["info"]["chunks"] > 3000
    check_run(case, r, "threaded table")


def test_state_between_and_around_the_passes(nine):
    case = nine
    rng = np.random.default_rng(23)
    other_f = case["f"] + rng.normal(0.0, 1.0, case["K"])
    other_Nk = case["N_k"][::-1] + np.arange(case["K"])
    with hc.open_matrix(case) as dm:
        first = hc.passes_on(dm, case, case["c"])
        fb = first["f_bins"]
        again = hc.passes_on(dm, case, case["c"])  # (set_bins with the same arrays, both passes again)
        assert bits(again) == bits(first)
        # logden(other_f) and gram_w write the log-denominators the passes read: each pass takes its own
        lognum = dm.bin_lognum(case["f"])
        dm.logden(other_f)
        after_logden = dm.bin_gram_w(case["f"], fb)
        dm.gram_w(other_f)
        after_gram = dm.bin_gram_w(case["f"], fb)
        for got in (after_logden, after_gram):
            assert (lognum.tobytes(),) + tuple(a.tobytes() for a in got) == bits(first)
        dm.set_Nk(other_Nk)
        moved = dm.bin_lognum(case["f"])
        assert moved.tobytes() != first["lognum"].tobytes()
        dm.set_Nk(case["N_k"])
        assert dm.bin_lognum(case["f"]).tobytes() == first["lognum"].tobytes()
        assert tuple(a.tobytes() for a in dm.bin_gram_w(case["f"], fb)) == bits(first)[1:]
        # other labels: their results, the ones of a fresh matrix
        relabelled = dict(case, labels=hc.pattern_labels("distinct", case["N"], case["nbins"]))
        second = hc.passes_on(dm, relabelled, case["c"])
        assert second["lognum"].tobytes() != first["lognum"].tobytes()
        with hc.open_matrix(relabelled) as fresh:
            assert bits(hc.passes_on(fresh, relabelled, case["c"])) == bits(second)
        # NaN in f or in f_bins: every output NaN
        bad_f = case["f"].copy()
        bad_f[3] = np.nan
        assert np.all(np.isnan(dm.bin_lognum(bad_f)))
        assert all(np.all(np.isnan(a)) for a in dm.bin_gram_w(bad_f, second["f_bins"]))
        bad_fb = second["f_bins"].copy()
        bad_fb[7] = np.nan
        assert all(np.all(np.isnan(a)) for a in dm.bin_gram_w(case["f"], bad_fb))
        assert all(np.all(np.isnan(a)) for a in dm.bin_gram_w(case["f"], bad_fb, cross=False)[1:])
        # refused arrays leave the earlier bins in place and usable
        for bad in (case["nbins"], -2):
            lab = relabelled["labels"].astype(np.int32)
            lab[100] = bad
            with pytest.raises(ValueError, match="labels must lie"):
                dm.set_bins(case["nbins"], lab, case["v"])
        for bad in (np.nan, -np.inf):
            v = case["v"].copy()
            v[100] = bad
            with pytest.raises(ValueError, match="must not hold NaN or -inf"):
                dm.set_bins(case["nbins"], relabelled["labels"], v)
        assert dm.bins_info() == second["info"]
        assert dm.bin_lognum(case["f"]).tobytes() == second["lognum"].tobytes()
        assert tuple(a.tobytes() for a in dm.bin_gram_w(case["f"], second["f_bins"])) == bits(second)[1:]
        dm.set_bins(0)
        with pytest.raises(Exception, match="no bins on this context"):
            dm.bin_lognum(case["f"])
        with pytest.raises(Exception, match="no bins on this context"):
            dm.bin_gram_w(case["f"], np.zeros(0))
