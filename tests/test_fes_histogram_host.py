"""Histogram surfaces by bin label and histogram bootstraps, host logic on the CPU stand-in (tests/hist_standin.py) against the
reference's own numbers (tests/golden/fes_umbrella_1d.npz, tests/golden/fes_histogram.npz from make_golden_fes_histogram.py)
and against the row path (``histogram_fes``) on the same stand-in."""
import numpy as np
import pytest

import pymbar_amd
from pymbar_amd import fes as amd_fes
from pymbar_amd.utils import ParameterError
from tests import hist_cases as hc
from tests.conftest import load_golden
from tests.hist_standin import HistOracleMatrix


@pytest.fixture
def standin(monkeypatch):
    import pymbar_amd.device

    monkeypatch.setattr(pymbar_amd.device, "DeviceMatrix", HistOracleMatrix)


@pytest.fixture(scope="module")
def umb():
    return load_golden("fes_umbrella_1d.npz")


@pytest.fixture(scope="module")
def gold():
    return load_golden("fes_histogram.npz")


def system_b(gold):
    """u_kn of fixture (b), rebuilt from the samples of fes_kde.npz by the generator's formula."""
    kde = load_golden("fes_kde.npz")
    x_n, u_n, xu = kde["b_x_n"], kde["b_u_n"], kde["b_umbrella_centers"]
    u_kn = np.array([u_n + (float(gold["b_Ku"]) / 2) * np.sum((x_n - xu[k]) ** 2, axis=1) for k in range(len(xu))])
    return u_kn, u_n, x_n


def test_labels_reproduce_reference_1d(standin, umb):
    g = umb
    mbar = pymbar_amd.MBAR(g["u_kn"], g["N_k"])
    labels, q = g["sample_label"], g["query"]
    low = amd_fes.histogram_fes_labels(mbar, g["u_n"], labels, reference="from-lowest")
    np.testing.assert_allclose(low["f_raw"], g["f_raw"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(low["f_i"][q], g["f_lowest"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(low["df_i"][q], g["df_lowest"], rtol=1e-7, atol=1e-9)
    assert "Theta_bins" not in low and "Theta" not in low
    spec = amd_fes.histogram_fes_labels(mbar, g["u_n"], labels, reference="from-specified", reference_label=int(g["specified_label"]))
    np.testing.assert_allclose(spec["f_i"][q], g["f_specified"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(spec["df_i"][q], g["df_specified"], rtol=1e-7, atol=1e-9)


def _against_rows(mbar, u_n, labels):
    K = mbar.K
    for method in (None, "approximate"):
        rows = amd_fes.histogram_fes(mbar, u_n, labels, theta_method=method)
        lab = amd_fes.histogram_fes_labels(mbar, u_n, labels, theta_method=method, return_theta=True)
        assert lab["reference"] == rows["reference"]
        np.testing.assert_allclose(lab["f_raw"], rows["f_raw"], rtol=0, atol=1e-11)
        print("max |Theta_bins - Theta[K:, K:]| =", np.max(np.abs(lab["Theta_bins"] - rows["Theta"][K:, K:])), "method", method)
        np.testing.assert_allclose(lab["Theta_bins"], rows["Theta"][K:, K:], rtol=0, atol=1e-12)
        np.testing.assert_allclose(lab["df_i"], rows["df_i"], rtol=1e-7, atol=1e-9)


def test_labels_against_rows_on_the_standin(standin, umb):
    mbar = pymbar_amd.MBAR(umb["u_kn"], umb["N_k"])
    _against_rows(mbar, umb["u_n"], umb["sample_label"])


def test_labels_with_an_unsampled_state(standin):
    g = load_golden("ho_unsampled_K4_N2300.npz")
    assert np.any(g["N_k"] == 0)
    mbar = pymbar_amd.MBAR(g["u_kn"], g["N_k"])
    rng = np.random.default_rng(5)
    u_n = g["u_kn"][int(np.argmin(g["N_k"]))]  # the surface of the state without samples
    labels = rng.integers(0, 9, size=mbar.N)
    labels[rng.random(mbar.N) < 0.05] = -1
    _against_rows(mbar, u_n, labels)


def test_fes_takes_the_label_path_above_256_rows(standin, gold):
    u_kn, u_n, x_n = system_b(gold)
    fes = pymbar_amd.FES(u_kn, gold["b_N_k"])
    before = HistOracleMatrix.constructed
    fes.generate_fes(u_n, x_n, histogram_parameters={"bin_edges": [gold["b_edges_x"], gold["b_edges_y"]]})
    hd = fes.histogram_data
    assert fes.K + len(hd["f"]) > amd_fes.ROW_PATH_MAX_ROWS
    np.testing.assert_array_equal(hd["sample_label"], gold["b_sample_label"])
    np.testing.assert_allclose(hd["f"], gold["b_f"], rtol=1e-9, atol=1e-9)
    q = gold["b_queries"]
    lo = fes.get_fes(q, reference_point="from-lowest", uncertainty_method="analytical")
    sp = fes.get_fes(q, reference_point="from-specified", fes_reference=[0, 0], uncertainty_method="analytical")
    assert HistOracleMatrix.constructed == before  # no second matrix: the bins are labels of the resident samples
    np.testing.assert_allclose(lo["f_i"], gold["b_f_lowest"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(lo["df_i"], gold["b_df_lowest"], rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(sp["f_i"], gold["b_f_specified"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(sp["df_i"], gold["b_df_specified"], rtol=1e-7, atol=1e-9)


def check_bootstraps(fes, umb, gold, drawn):
    """The assertions on fixture (a), shared with the GPU test: the stream, the replicates' f_k and bin free energies, df_i."""
    B = int(gold["a_n_bootstraps"])
    assert fes.n_bootstraps == B and len(fes.histogram_datas) == B and len(fes._hist_f_boots) == B
    np.testing.assert_array_equal(np.array(drawn), gold["a_idx"])  # the reference's draws, replicate by replicate
    for f_b, want in zip(fes._hist_f_boots, gold["a_tight_f_k"]):
        np.testing.assert_allclose(f_b, want, rtol=0, atol=1e-8)
    got = np.array([h["f"] for h in fes.histogram_datas])
    # against the tight solves: a bin free energy is a difference of two quantities that carry the solver's 1e-8
    print("max |f_b - tight| =", np.max(np.abs(got - gold["a_tight_f"])), " max |f_b - reference| =", np.max(np.abs(got - gold["a_ref_f"])))
    np.testing.assert_allclose(got, gold["a_tight_f"], rtol=0, atol=2e-8)
    # against the reference's own replicates, which sit within a_loose_gap (measured from the reference alone) of the tight ones
    bound = 2.0 * float(gold["a_loose_gap"]) + 2e-8
    np.testing.assert_allclose(got, gold["a_ref_f"], rtol=0, atol=bound)
    q = gold["a_queries"]
    lo = fes.get_fes(q, reference_point="from-lowest", uncertainty_method="bootstrap")
    sp = fes.get_fes(q, reference_point="from-specified", fes_reference=0.0, uncertainty_method="bootstrap")
    np.testing.assert_allclose(lo["f_i"], gold["a_f_lowest"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(sp["f_i"], gold["a_f_specified"], rtol=1e-9, atol=1e-9)
    # std over replicates moves by at most the largest change of a replicate's f_i - f_j: twice the replicate bound
    np.testing.assert_allclose(lo["df_i"], gold["a_df_lowest"], rtol=0, atol=2.0 * bound)
    np.testing.assert_allclose(sp["df_i"], gold["a_df_specified"], rtol=0, atol=2.0 * bound)


def record_draws(monkeypatch):
    drawn = []
    real = amd_fes._draw_bootstrap_indices

    def draw(N_k, idx):
        out = real(N_k, idx)
        drawn.append(out.copy())
        return out

    monkeypatch.setattr(amd_fes, "_draw_bootstrap_indices", draw)
    return drawn


def test_bootstraps_reproduce_reference(standin, monkeypatch, umb, gold):
    drawn = record_draws(monkeypatch)
    fes = pymbar_amd.FES(umb["u_kn"], umb["N_k"])
    fes.generate_fes(umb["u_n"], umb["x_n"], histogram_parameters={"bin_edges": umb["bin_edges"]},
                     n_bootstraps=int(gold["a_n_bootstraps"]), seed=int(gold["a_seed"]))
    check_bootstraps(fes, umb, gold, drawn)
    # the multiplicities are gone again: the resident matrix is the original one
    assert fes.mbar._dm._counts is None and fes.mbar._dm.u.shape == umb["u_kn"].shape


def _singleton_system():
    """Two harmonic states, 30 + 30 samples on a line; the last sample sits alone in the last bin."""
    rng = np.random.default_rng(11)
    x = np.concatenate([rng.normal(0.0, 0.4, 30), rng.normal(1.0, 0.4, 30)])
    x = np.clip(x, -1.4, 2.4)
    x[-1] = 2.8
    u_kn = np.array([0.5 * (x / 0.4) ** 2, 0.5 * ((x - 1.0) / 0.4) ** 2])
    edges = np.array([-1.5, 0.0, 0.5, 1.0, 2.5, 3.0])
    return u_kn, np.array([30, 30]), x, edges


@pytest.mark.parametrize("missing", [2, 3])
def test_replicate_without_the_bin_is_left_out(standin, monkeypatch, missing):
    u_kn, N_k, x, edges = _singleton_system()
    N = len(x)
    rounds = iter(range(4))

    def draw(N_k_, idx):  # the singleton (sample N - 1) is replaced by its neighbour in the first `missing` replicates
        b = next(rounds)
        idx[:] = np.arange(N)
        idx[0], idx[31] = b % 7 + 1, 31 + b % 5  # (so that the replicates differ)
        if b < missing:
            idx[N - 1] = N - 2
        return idx

    monkeypatch.setattr(amd_fes, "_draw_bootstrap_indices", draw)
    fes = pymbar_amd.FES(u_kn, N_k)
    fes.generate_fes(np.zeros(N), x, histogram_parameters={"bin_edges": edges}, n_bootstraps=4)
    hd = fes.histogram_data
    single = int(hd["sample_label"][N - 1])
    assert np.sum(hd["sample_label"] == single) == 1
    fb = np.array([h["f"] for h in fes.histogram_datas])
    assert np.all(np.isposinf(fb[:missing, single])) and np.all(np.isfinite(fb[missing:, single]))
    centers = 0.5 * (edges[1:] + edges[:-1])
    r = fes.get_fes(centers, reference_point="from-lowest", uncertainty_method="bootstrap")
    j = int(np.argmin(hd["f"]))
    seen = False
    for c, df in zip(centers, r["df_i"]):
        i = hd["label_of_grid"][(int(np.digitize(c, edges) - 1),)]
        usable = np.isfinite(fb[:, i]) & np.isfinite(fb[:, j])
        if i == single:
            seen = True
            assert list(usable) == [False] * missing + [True] * (4 - missing)
        if usable.sum() >= 2:  # the spread comes from the replicates that hold both bins
            np.testing.assert_allclose(df, np.std(fb[usable, i] - fb[usable, j]), rtol=1e-12, atol=1e-15)
        else:
            assert np.isnan(df)
    assert seen and np.isnan(r["df_i"][-1]) == (missing == 3)


def test_parameter_errors(standin, umb):
    g = umb
    mbar = pymbar_amd.MBAR(g["u_kn"], g["N_k"])
    labels = g["sample_label"]
    with pytest.raises(ParameterError):
        amd_fes.histogram_fes_labels(mbar, g["u_n"][:-1], labels)
    with pytest.raises(ParameterError):
        amd_fes.histogram_fes_labels(mbar, g["u_n"], labels[:-1])
    with pytest.raises(ParameterError):
        amd_fes.histogram_fes_labels(mbar, g["u_n"], labels, theta_method="svd")
    with pytest.raises(ParameterError):
        amd_fes.histogram_fes_labels(mbar, g["u_n"], labels, uncertainty_method="bootstrap")
    with pytest.raises(ParameterError):
        amd_fes.histogram_fes_labels(mbar, g["u_n"], np.where(labels == 0, -2, labels))
    with pytest.raises(ValueError):  # a label >= nbins is refused where the bins are uploaded
        mbar._dm.set_bins(int(labels.max()), labels, g["u_n"])
    with pytest.raises(Exception):
        amd_fes.histogram_fes_labels(mbar, g["u_n"], np.where(labels == 3, 2, labels))  # bin 3 emptied
    fes = pymbar_amd.FES(g["u_kn"], g["N_k"])
    fes.generate_fes(g["u_n"], g["x_n"], histogram_parameters={"bin_edges": g["bin_edges"]})
    with pytest.raises(ParameterError):
        fes.get_fes([0.0], uncertainty_method="bootstrap")  # no replicates


# ---- the branch model of the binned passes (tests/hist_cases.py): what the GPU cases reach, asserted from the model ----------------
@pytest.fixture(scope="module")
def branch_cases():
    return [hc.make_case(*key) for key in hc.case_keys()]


def test_model_constants_are_the_kernels():
    """the census describes the kernels only while the model's constants are theirs (HIST_ROUNDS = 7 would still sum correctly,
    with other steps handed over: no numeric check can see it)"""
    import os
    import re

    csrc = os.path.join(os.path.dirname(amd_fes.__file__), "csrc")
    text = open(os.path.join(csrc, "mbar_k_hist.hip")).read() + open(os.path.join(csrc, "mbar_hist.h")).read()
    for name, value in (("HIST_ROUNDS", hc.HIST_ROUNDS), ("HIST_SLOTS", hc.HIST_SLOTS), ("HIST_NO_SLOT", hc.NO_SLOT),
                        ("HIST_CHUNK_SAMPLES", hc.HIST_CHUNK_SAMPLES), ("HIST_ROWS", hc.HIST_ROWS)):
        found = re.findall(r"constexpr int %s = (\d+);" % name, text)
        assert found == [str(value)], (name, found)


def test_model_chunk_counts():
    counts = [hc.model_chunks(hc.pattern_labels(p, 4500, nb), nb, 1) for p, nb in hc.PATTERNS[:6]]
    assert tuple(counts) == hc.CHUNKS_AT_4500
    chunks, slot = hc.chunk_table(hc.pattern_labels("late65", 4500, 65), 0, 65)
    assert chunks == [(0, 2047, 64), (2047, 2048, 1), (2048, 4096, 64), (4096, 4500, 64)] and slot[2047] == 0
    # a tile of the bins sees the other labels as "no slot": 64-sample chunks of 300 distinct bins become 2048-sample ones
    lab = hc.pattern_labels("distinct", 4500, 300)
    assert hc.model_chunks(lab, 300, 300) == 300 * 3 and hc.model_chunks(lab, 300, 1) == 71


def test_case_set_reaches_every_branch(branch_cases):
    steps, lens, nbs, max_slot, max_lane = set(), set(), set(), -1, -1
    for case in branch_cases:
        for w in ("none", "mult"):
            cs = hc.step_census(case["labels"], hc.weights_of(case, w)[1], case["nbins"])
            steps |= set(cs["steps"])
            lens |= set(cs["chunk_len"])
            nbs |= set(cs["chunk_nb"])
            max_slot, max_lane = max(max_slot, cs["max_slot"]), max(max_lane, cs["max_lane"])
    distinct = {d for d, _ in steps}
    assert {0, 1, hc.HIST_ROUNDS, hc.HIST_ROUNDS + 1, 64} <= distinct
    assert (hc.HIST_ROUNDS, 0) in steps  # eight slots: the last butterfly leaves nothing
    assert any(d == hc.HIST_ROUNDS + 1 and left > 1 for d, left in steps)  # nine: one slot's several samples handed over
    assert (64, 56) in steps
    assert max_slot == 63 and max_lane == 63
    assert 1 in lens and 0 in nbs and hc.HIST_SLOTS in nbs
    # the patterns on their own terms, unit multiplicities, N = 4500
    def own(pattern, nbins):
        return set(hc.step_census(hc.pattern_labels(pattern, 4500, nbins), np.ones(4500), nbins)["steps"])

    assert own("sorted", 128) == {(1, 0), (2, 0), (3, 0)}
    assert own("eight", 300) == {(8, 0)}
    assert own("nine", 300) == {(1, 0), (9, 2), (9, 7), (10, 8)}  # (a chunk's short last step; 9 or 10 slots, 2, 7 or 8 handed over)
    assert own("distinct", 300) == own("distinct", 64) == {(20, 12), (64, 56)}
    assert (0, 0) in own("gaps", 300)  # a whole step of -1 inside a chunk with bins


def test_every_case_runs_on_the_standin(branch_cases):
    """every case and weighting through the CPU stand-in, whose sums the vectorised oracle of the GPU tests must reproduce"""
    for case in branch_cases:
        with np.errstate(divide="ignore"):  # (log N_k of a state without samples)
            dm = HistOracleMatrix(case["u"])
            dm.set_Nk(case["N_k"])
            for w in hc.WEIGHTINGS:
                weights, c = hc.weights_of(case, w)
                r = hc.passes_on(dm, case, weights)
                dm.set_sample_weights(None)
                o = hc.oracle(case["u"], dm.logden(case["f"]), case["v"], case["f"], case["labels"], c, case["nbins"])
                live = o["n_i"] > 0
                assert np.all(np.isneginf(r["lognum"][~live])) and np.all(r["wsum"][~live] == 0)
                np.testing.assert_allclose(r["lognum"][live], o["lognum"][live].astype(np.float64), rtol=0, atol=1e-13)
                for name in ("cross", "diag", "wsum"):
                    np.testing.assert_allclose(r[name], o[name].astype(np.float64), rtol=1e-13, atol=0)
