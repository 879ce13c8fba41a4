"""The binned passes of the label path (``mbar_ctx_set_bins`` / ``mbar_bin_lognum`` / ``mbar_bin_gram_w``, mbar_k_hist.hip) on the
MI355X against a numpy long-double oracle, against the row path on the device, and through ``pymbar_amd.FES`` against the
unmodified reference (tests/golden/fes_histogram.npz).

Error bound of a binned sum (``bin_bound``).  Every term is positive, so a bin's sum of ``n_i`` terms carries at most
``(n_i - 1) u`` relative (``u = 2^-53``; each term passes through at most ``n_i - 1`` additions however the chunks group them; the
compensated merges add less) plus the largest relative error of a term.  A term is a product of ``E`` device exponentials (``E = 1``
for lognum and wsum, 2 for cross and diag); each carries the pinned ``3.1 u`` of ``exp2s_fast``
(tests/test_device_math_tables.py, profiles/device_math_accuracy.txt) plus ``2^-52 max|argument|`` for its rounded argument,
the products and the multiplicity add one ``u`` per multiplication (``E + 1`` of them at most).  ``lognum = max + log(sum)`` gets the
same figure as an absolute error.  The oracle works on the device's own downloaded ``u``, ``logden(f)`` and ``v``, so only the binned
passes are under test."""
import numpy as np
import pytest

import pymbar_amd
from pymbar_amd import fes as amd_fes
from pymbar_amd.device import DeviceMatrix
from tests.conftest import load_golden
from tests.test_fes_histogram_host import check_bootstraps, record_draws, system_b

pytestmark = pytest.mark.gpu

LD = np.longdouble
U = 2.0 ** -53
E_EXP = 3.1  # (u) pinned relative error of the device exp


def awkward_case(seed=3):
    """K = 130 (two row blocks past 128, nine groups of 16 rows), N = 3001 (no multiple of 64), 300 bins with random labels so
    that chunks close on the 64-bin cap, 5 % of the labels -1, multiplicities 0 .. 3 with 30 % zeros, bin 298 with a single
    sample, bin 299 with three samples that all have multiplicity 0."""
    rng = np.random.default_rng(seed)
    K, N, nbins = 130, 3001, 300
    x = rng.normal(0.0, 1.0, N)
    centers = np.linspace(-2.0, 2.0, K)
    u = 0.5 * (x[None, :] - centers[:, None]) ** 2 * 4.0 + rng.normal(0.0, 0.05, (K, N))
    N_k = np.full(K, N // K)
    N_k[: N - N_k.sum()] += 1
    f = rng.normal(0.0, 0.5, K)
    v = rng.uniform(0.0, 5.0, N)
    labels = rng.integers(0, 298, N)
    labels[rng.random(N) < 0.05] = -1
    c = rng.integers(1, 4, N).astype(np.float64)
    c[rng.random(N) < 0.30] = 0.0
    labels[1234], c[1234] = 298, 2.0
    labels[[17, 1500, 2999]], c[[17, 1500, 2999]] = 299, 0.0
    return dict(K=K, N=N, nbins=nbins, u=u, N_k=N_k, f=f, v=v, labels=labels, c=c)


def oracle(u, logden, v, f, labels, c, nbins):
    """Long-double lognum, cross, diag, wsum with f_bins = -lognum, their bounds, from the device's own u / logden."""
    K = u.shape[0]
    x = -(v.astype(LD) + logden.astype(LD))
    logW = f.astype(LD)[:, None] - u.astype(LD) - logden.astype(LD)[None, :]
    lognum = np.full(nbins, -np.inf, dtype=LD)
    cross, diag, wsum = np.zeros((K, nbins), dtype=LD), np.zeros(nbins, dtype=LD), np.zeros(nbins, dtype=LD)
    n_i, arg = np.zeros(nbins), np.zeros(nbins)
    for i in range(nbins):
        m = (labels == i) & (c > 0)
        n_i[i] = m.sum()
        if not m.any():
            continue
        mx = x[m].max()
        lognum[i] = mx + np.log(np.sum(c[m] * np.exp(x[m] - mx)))
        b = x[m] - lognum[i]  # log B_n at f_bins = -lognum
        B = np.exp(b)
        wsum[i], diag[i] = np.sum(c[m] * B), np.sum(c[m] * B * B)
        cross[:, i] = np.exp(logW[:, m]) @ (c[m] * B)
        arg[i] = float(max(np.abs(x[m]).max(), np.abs(x[m] - mx).max(), np.abs(b).max(), np.abs(logW[:, m]).max(),
                           np.abs(f).max() + np.abs(u[:, m]).max()))
    return dict(lognum=lognum, cross=cross, diag=diag, wsum=wsum, n_i=n_i, arg=arg)


def bin_bound(o, n_exp):
    """Relative bound of a bin's sum whose terms hold n_exp exponentials (module docstring)."""
    return (np.maximum(o["n_i"] - 1, 0) + n_exp * (E_EXP + 2.0 * o["arg"]) + (n_exp + 1)) * U


def run_passes(case, part_bytes=None, perm=None):
    p = slice(None) if perm is None else perm
    with DeviceMatrix.from_host(case["u"][:, p]) as dm:
        dm.set_Nk(case["N_k"])
        if part_bytes is not None:
            dm.set_option("hist_part_bytes", part_bytes)
        labels, v, c = case["labels"][p], case["v"][p], case["c"][p]
        dm.set_sample_weights(c)
        dm.set_bins(case["nbins"], labels, v)
        info = dm.bins_info()
        lognum = dm.bin_lognum(case["f"])
        X, d, w = dm.bin_gram_w(case["f"], -lognum)
        again = (dm.bin_lognum(case["f"]), dm.bin_gram_w(case["f"], -lognum))
        dm.set_bins(case["nbins"], labels, v)
        third = (dm.bin_lognum(case["f"]), dm.bin_gram_w(case["f"], -lognum))
        dm.set_sample_weights(None)
        logden, u_dev = dm.logden(case["f"]), dm.to_host()
    return dict(lognum=lognum, cross=X, diag=d, wsum=w, info=info, again=again, third=third, logden=logden, u=u_dev, labels=labels, v=v, c=c)


@pytest.fixture(scope="module")
def case():
    return awkward_case()


@pytest.fixture(scope="module")
def single_sweep(case):
    r = run_passes(case)
    r["oracle"] = oracle(r["u"], r["logden"], r["v"], case["f"], r["labels"], r["c"], case["nbins"])
    return r


def assert_within(r, o, factor=1.0):
    live = o["n_i"] > 0
    err = np.abs(r["lognum"][live].astype(LD) - o["lognum"][live])
    print("lognum: worst error / bound", float(np.max(err / (factor * bin_bound(o, 1)[live]))))
    assert np.all(err <= factor * bin_bound(o, 1)[live])
    assert np.all(np.isneginf(r["lognum"][~live]))
    for name, n_exp in (("wsum", 1), ("diag", 2)):
        err = np.abs(r[name].astype(LD) - o[name])
        print(name, "worst error / bound", float(np.max(err[live] / (factor * bin_bound(o, n_exp) * np.abs(o[name]))[live])))
        assert np.all(err <= factor * bin_bound(o, n_exp) * np.abs(o[name]))
    err = np.abs(r["cross"].astype(LD) - o["cross"])
    bound = factor * bin_bound(o, 2)[None, :] * np.abs(o["cross"])
    print("cross worst error / bound", float(np.max(err[:, live] / bound[:, live])))
    assert np.all(err <= bound)


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
