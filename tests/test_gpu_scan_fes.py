"""Histogram free energy surfaces along a scan on the MI355X (``mbar_ctx_set_scan_bins`` / ``mbar_scan_bin_lognum`` /
``mbar_scan_bin_gram_w``, the binned cut of mbar_k_scan.hip; ``MBAR.compute_scan_fes``): the two passes against the long-double
stand-in (tests/scan_fes_standin.py; tests/test_scan_fes_host.py shows on the CPU that the cases suit it), every instantiation of
the pass-B kernel, the order contract bit for bit (the other members, the other bins, the bin's number, the record budget and the
slabs of the wrapper change nothing; one bin that holds every sample gives the bits of the scan passes), ``compute_scan_fes``
against the loop of ``histogram_fes_labels`` on the device and against the reference's fixture, the bootstrap replicates, and the
passes as consumers of the context's state.

Tolerances of the passes are those of tests/test_gpu_scan.py::test_passes_against_long_double_standin: lognum and wsum 1e-11
absolute, the products rtol 1e-10.  Shapes are (K, N, L, B, nbins)."""
import numpy as np
import pytest

import pymbar_amd
from pymbar_amd import _lib, fes, testsystems
from pymbar_amd.device import DeviceMatrix, LoopbackGroup, _dptr
from tests.conftest import load_golden
from tests.scan_fes_standin import (PASS_CASES, ScanFesOracleMatrix, build_fes_case, check_passes, check_row_against_label_path,
                                    load_case, run_fes_passes)
from tests.scan_standin import family, ladder, scan_nb_for
from tests.test_capi_context import PLAIN_STARTS, PLAIN_WRITERS, assert_same, same
from tests.test_gpu_parity import random_problem
from tests.test_scan_fes_host import check_against_fixture

pytestmark = pytest.mark.gpu


def shape_id(v):
    return v if isinstance(v, str) else "K%d-N%d-L%d-B%d-bins%d" % v


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def device_matrix(case):
    dm = DeviceMatrix.from_host(case["u"])
    load_case(dm, case)
    return dm


def standin_passes(case, u_dev):
    oracle = ScanFesOracleMatrix(u_dev)
    load_case(oracle, case)
    return run_fes_passes(oracle, case)


def report(got, want, case):
    live = np.arange(case["nbins"]) != (-1 if case["emptied"] is None else case["emptied"])
    for name in ("lognum", "cross", "diag", "wsum"):
        g, w = got[name][..., live], want[name][..., live]
        print(name, "max abs error", np.max(np.abs(g - w)), "max rel error", np.max(np.abs(g - w) / np.maximum(np.abs(w), 1e-300)))


# ---- 1. the passes against the long-double stand-in -----------------------------------------------------------------------------
@pytest.mark.parametrize("hard", [False, True], ids=["plain", "weights-inf-unsampled-emptied"])
@pytest.mark.parametrize("shape,kind", PASS_CASES, ids=shape_id)
def test_passes_against_long_double_standin(shape, kind, hard):
    case = build_fes_case(shape, hard, kind)
    with device_matrix(case) as dm:
        got = run_fes_passes(dm, case)
        u_dev = dm.to_host()
    want = standin_passes(case, u_dev)
    report(got, want, case)
    live = np.arange(case["nbins"]) != (-1 if case["emptied"] is None else case["emptied"])
    assert np.all(np.isfinite(got["lognum"][:, live]))
    if shape[2] >= 5:
        assert np.max(got["lognum"][:-1, live] - got["lognum"][-1, live]) > 800.0
    check_passes(got, want, case)


# ---- 2. every instantiation of the pass-B kernel --------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [256, 257], ids=["full-panel", "ragged-panel"])
@pytest.mark.parametrize("K", [16, 17, 32, 33, 64, 65, 128])
def test_every_instantiation_against_long_double_standin(K, L):
    """k_scan_cross<NB, 1, ScanBinned> for NB in {1, 2, 4, 8} at both ends of the state counts it serves, and <0> through
    cross=False, with one full panel of 256 members and with a second panel of one; N = 301 in 5 bins (tiles with a tail),
    multiplicities 0 .. 3, +inf entries, an unsampled state, an emptied bin."""
    B = {16: 1, 17: 2, 32: 5, 33: 8, 64: 3, 65: 2, 128: 4}[K]
    case = build_fes_case((K, 301, L, B, 5), True, "mixed")
    with device_matrix(case) as dm:
        got = run_fes_passes(dm, case)
        X, d, w = dm.scan_bin_gram_w(case["f"], case["coeff"], case["offset"], -got["lognum"], cross=False)
        u_dev = dm.to_host()
    want = standin_passes(case, u_dev)
    print("NB", scan_nb_for(K))
    report(got, want, case)
    check_passes(got, want, case)
    assert X is None and bits(d) == bits(got["diag"]) and bits(w) == bits(got["wsum"])


# ---- 3. bits --------------------------------------------------------------------------------------------------------------------
def test_order_contract_bit_for_bit():
    shape = (17, 4099, 33, 8, 12)
    case = build_fes_case(shape, True, "shuffled")
    L, nbins, label = shape[2], shape[4], case["label"]
    rng = np.random.default_rng(9)
    with device_matrix(case) as dm:
        got = run_fes_passes(dm, case)
        again = run_fes_passes(dm, case)
        lone = run_fes_passes(dm, case, members=slice(L - 1, L))
        slabs = [run_fes_passes(dm, case, slab=s) for s in (1, 7, 32)]
        dm.set_option("scan_part_bytes", 1)  # every bin a sweep of its own
        cut = run_fes_passes(dm, case)
        dm.set_option("scan_part_bytes", 1 << 28)
        # the bins renumbered: new number of bin i is sigma[i]
        sigma = rng.permutation(nbins)
        dm.set_scan_bins(nbins, np.where(label >= 0, sigma[np.maximum(label, 0)], -1))
        moved = run_fes_passes(dm, case)
        # every other bin's samples in no bin
        keep = 5
        dm.set_scan_bins(nbins, np.where(label == keep, keep, -1))
        alone = run_fes_passes(dm, case)
    assert np.all(np.isfinite(got["lognum"][:, :-1]))
    for name in got:
        assert bits(got[name]) == bits(again[name]), name  # two identical calls
        assert bits(got[name][..., L - 1:, :]) == bits(lone[name]), name  # the last member alone
        assert bits(got[name]) == bits(cut[name]), name  # the record budget
        for s in slabs:
            assert bits(got[name]) == bits(s[name]), name  # the slabs of the wrapper
        assert bits(got[name]) == bits(moved[name][..., sigma]), name  # the bins' numbers
        assert bits(got[name][..., keep]) == bits(alone[name][..., keep]), name  # the other bins
    assert np.all(alone["lognum"][:, np.arange(nbins) != keep] == -np.inf)


def test_pass_a_member_panels_do_not_change_a_bit():
    """Context option "scan_part_bytes" = 1: pass A in panels of 64 members (64 + 64 + 2), pass B one bin per sweep"""
    case = build_fes_case((5, 5000, 130, 3, 7), True, "mixed")
    with device_matrix(case) as dm:
        whole = run_fes_passes(dm, case)
        dm.set_option("scan_part_bytes", 1)
        cut = run_fes_passes(dm, case)
    for name in whole:
        assert bits(whole[name]) == bits(cut[name]), name


# ---- 4. one bin that holds every sample: the bits of the scan passes ------------------------------------------------------------
# K = 9, 17, 33, 128: NB = 1, 2, 4, 8; N on both sides of the chunk edges of pass A (2048) and of pass B (8192), for the smaller K
# just past each
ONE_BIN_CASES = [(N, K) for K in (33, 128) for N in (2047, 2049, 8191, 8193)] + [(N, K) for K in (9, 17) for N in (2049, 8193)]


@pytest.mark.parametrize("N,K", ONE_BIN_CASES)
def test_one_bin_is_the_scan_passes_bit_for_bit(N, K):
    """Both cuts of the samples are one kernel source (k_scan_vec<SUM, Cut>, k_scan_cross<NB, J, Cut> of mbar_k_scan.hip): with one
    bin that holds every sample the binned cut returns the bits of the whole cut at J = 1, in every instantiation the two share --
    NB = 1, 2, 4, 8 and, with cross=False, NB = 0, whose sums are also the bits of the calls with the cross block.  L = 70: one
    ragged panel."""
    L = 70
    case = build_fes_case((K, N, L, 3, 1), True, "sorted")
    assert np.all(case["label"] == 0)
    with device_matrix(case) as dm:
        got = run_fes_passes(dm, case)
        bare = run_fes_passes(dm, case, cross=False)
        lognum, mean = dm.scan_lognum(case["f"], case["coeff"], case["offset"])
        X, within, refcol, w = dm.scan_gram_w(case["f"], case["coeff"], case["offset"], -lognum, reference=0)
        X0, within0, refcol0, w0 = dm.scan_gram_w(case["f"], case["coeff"], case["offset"], -lognum, reference=0, cross=False)
    print("NB", scan_nb_for(K))
    assert np.all(np.isfinite(lognum)) and np.all(X > 0)
    assert bits(got["lognum"][:, 0]) == bits(lognum)
    assert bits(got["cross"][:, :, 0]) == bits(X[:, :, 0])
    assert bits(got["diag"][:, 0]) == bits(within[:, 0, 0])
    assert bits(got["wsum"][:, 0]) == bits(w)
    # NB = 0 on both sides: across the cuts, and against the calls with the cross block
    assert bare["cross"] is None and X0 is None
    assert bits(bare["diag"][:, 0]) == bits(within0[:, 0, 0]) and bits(bare["wsum"][:, 0]) == bits(w0)
    assert bits(bare["diag"]) == bits(got["diag"]) and bits(bare["wsum"]) == bits(got["wsum"])
    assert bits(within0) == bits(within) and bits(w0) == bits(w)


# ---- 5. compute_scan_fes against the loop of histogram_fes_labels ---------------------------------------------------------------
@pytest.mark.parametrize("shape", [(17, 4099, 33, 8, 12), (128, 6001, 40, 2, 30)], ids=shape_id)
def test_scan_fes_against_the_label_path(shape):
    K, N, L, B, nbins = shape
    rng = np.random.default_rng(K)
    x_n, u_kn, N_k, O_k, K_k = ladder(K, N, seed=1)
    basis, coeff, offset = family(x_n, O_k, K_k, L, B, rng)
    edges = np.quantile(x_n, np.linspace(0.0, 1.0, nbins + 1))
    edges[0], edges[-1] = edges[0] - 1.0, edges[-1] + 1.0
    label, grid = fes.label_samples(x_n, edges)
    assert len(grid) == nbins
    mbar = pymbar_amd.MBAR(u_kn, N_k, relative_tolerance=1e-12)
    try:
        for reference, rl in (("from-lowest", None), ("from-specified", nbins // 2)):
            for theta in (None, "approximate"):
                res = mbar.compute_scan_fes(basis, coeff, offset, sample_label=label, reference=reference, reference_label=rl,
                                            uncertainty_method="analytical", theta_method=theta)
                gap = 0.0
                for l in range(L):
                    one = fes.histogram_fes_labels(mbar, coeff[l] @ basis + offset[l], label, reference=reference, reference_label=rl,
                                                   theta_method=theta)
                    others = np.arange(nbins) != res["reference"][l]
                    gap = max(gap, np.max(np.abs(res["df_i"][l][others] / one["df_i"][others] - 1.0)))
                    check_row_against_label_path(res, l, one)
                print(reference, theta, "max rel df_i gap =", gap)
                low = res["f_raw"].min(axis=1)
                np.testing.assert_allclose(res["f"], low - np.log(np.sum(np.exp(low[:, None] - res["f_raw"]), axis=1)), rtol=0, atol=1e-12)
    finally:
        mbar.close()


def test_fixture_reproduces_reference():
    x_n, u_kn, N_k, _, _, _ = testsystems.config1(seed=0)
    mbar = pymbar_amd.MBAR(u_kn, N_k, relative_tolerance=1e-12)
    try:
        check_against_fixture(mbar, load_golden("scan_fes_ho_K5.npz"), x_n)
    finally:
        mbar.close()


# ---- 6. bootstrap ---------------------------------------------------------------------------------------------------------------
def test_bootstrap_replicates_are_the_label_path_under_the_replicates_weights():
    gold = load_golden("scan_fes_ho_K5.npz")
    x_n, u_kn, N_k, _, _, _ = testsystems.config1(seed=0)
    basis, coeff, offset = testsystems.harmonic_scan_family(x_n, gold["O_l"], gold["K_l"])
    label, grid = fes.label_samples(x_n, gold["bin_edges"])
    nbins, L = len(grid), len(coeff)
    mbar = pymbar_amd.MBAR(u_kn, N_k, n_bootstraps=4, bootstrap_rng="device", rseed=11)
    try:
        res = mbar.compute_scan_fes(basis, coeff, offset, sample_label=label, uncertainty_method="bootstrap")
        fb = res["bootstrapped_f_raw"]
        assert fb.shape == (4, L, nbins) and res["df_i"].shape == (L, nbins)
        dm = mbar._dm
        for b in range(4):
            mbar._set_bootstrap_weights(dm, b)
            try:
                for l in range(L):
                    dm.set_bins(nbins, label, coeff[l] @ basis + offset[l])
                    np.testing.assert_allclose(fb[b, l], -dm.bin_lognum(mbar.f_k_boots[b]), rtol=0, atol=1e-11)
                    dm.set_bins(0)
            finally:
                dm.set_sample_weights(None)
        usable = np.isfinite(fb - fb[:, np.arange(L), res["reference"]][:, :, None])
        full = usable.all(axis=0)
        diff = fb - fb[:, np.arange(L), res["reference"]][:, :, None]
        np.testing.assert_allclose(res["df_i"][full], np.std(diff, axis=0)[full], rtol=1e-12, atol=0)
        assert np.all(np.isnan(res["df_i"][usable.sum(axis=0) < 2]))
        assert np.all(res["df_i"][full] >= 0) and np.any(res["df_i"] > 0)
        assert mbar._dm._wtag is None  # the multiplicities do not leak
    finally:
        mbar.close()


# ---- 7. the passes as consumers of the context's state --------------------------------------------------------------------------
def small_scan(N, L=20, nbins=6):
    rng = np.random.default_rng(3)
    label = rng.integers(-1, nbins, N)
    label[:nbins] = np.arange(nbins)
    return dict(basis=rng.normal(0.0, 1.0, (2, N)), coeff=rng.uniform(0.0, 1.0, (L, 2)), offset=rng.normal(0.0, 1.0, L), label=label,
                nbins=nbins)


def fes_outputs(dm, f, s):
    """Both passes at f; pass B at f_bins = -lognum and at f_bins = 0 (finite whatever pass A returned)"""
    lognum = dm.scan_bin_lognum(f, s["coeff"], s["offset"])
    out = dict(lognum=lognum)
    for tag, f_bins in (("", -lognum), ("0 ", np.zeros_like(lognum))):
        X, d, w = dm.scan_bin_gram_w(f, s["coeff"], s["offset"], f_bins)
        out.update({tag + "cross": X, tag + "diag": d, tag + "wsum": w})
    return out


def fresh_fes_outputs(u, N_k, f, s, c=None):
    with DeviceMatrix.from_host(u) as fresh:
        fresh.set_Nk(N_k)
        fresh.set_sample_weights(c)
        fresh.set_scan(s["basis"], None)
        fresh.set_scan_bins(s["nbins"], s["label"])
        return fes_outputs(fresh, f, s)


@pytest.mark.parametrize("writer", sorted(PLAIN_WRITERS))
def test_passes_after_every_writer_of_the_matrix(writer):
    K, N = 5, 300
    u, N_k, f = random_problem(K, N, seed=31)
    rng = np.random.default_rng(5)
    start = PLAIN_STARTS.get(writer, lambda u: u)(u)
    s = small_scan(N)
    with DeviceMatrix.from_host(start) as dm:
        dm.set_Nk(N_k)
        dm.set_scan(s["basis"], None)
        dm.set_scan_bins(s["nbins"], s["label"])
        before = fes_outputs(dm, f, s)
        PLAIN_WRITERS[writer](dm, u, rng)
        got = fes_outputs(dm, f, s)
        final = dm.to_host()
    want = fresh_fes_outputs(final, N_k, f, s)
    assert_same(got, want, writer)
    for key in got:
        assert bool(np.isnan(before[key]).all()) == bool(np.isnan(start).any()), key
        assert bool(np.isnan(got[key]).all()) == bool(np.isnan(final).any()), key
        assert bool(np.isfinite(got[key]).all()) != bool(np.isnan(final).any()), key
        assert not same(got[key], before[key]), key


def test_passes_after_changes_of_what_slot_0_depends_on():
    K, N = 5, 300
    u, N_k, f = random_problem(K, N, seed=31)
    s = small_scan(N)
    rng = np.random.default_rng(8)
    N_k2 = np.roll(N_k, 2)
    c1 = rng.integers(1, 4, N).astype(np.float64)
    c1[rng.random(N) < 0.2] = 0.0
    c1[: s["nbins"]] = 1.0
    c2 = np.roll(c1, 1)
    c2[: s["nbins"]] = 1.0
    assert not np.array_equal(N_k2, N_k) and np.any((c1 == 0) != (c2 == 0))
    with DeviceMatrix.from_host(u) as dm:
        dm.set_Nk(N_k)
        dm.set_scan(s["basis"], None)
        dm.set_scan_bins(s["nbins"], s["label"])
        first = fes_outputs(dm, f, s)
        dm.set_Nk(N_k2)
        other_counts = fes_outputs(dm, f, s)
        dm.set_Nk(N_k)
        dm.set_sample_weights(c1)
        under_c1 = fes_outputs(dm, f, s)
        dm.set_sample_weights(c2)
        under_c2 = fes_outputs(dm, f, s)
        dm.set_sample_weights(None)
        dm.solve_adaptive(np.zeros(K), tol=1e-10, maxiter=200, min_sc_iter=0)  # (the device loop rotates the slots)
        after_solve = fes_outputs(dm, f, s)
    assert_same(first, fresh_fes_outputs(u, N_k, f, s), "first")
    assert_same(other_counts, fresh_fes_outputs(u, N_k2, f, s), "set_Nk")
    assert_same(under_c1, fresh_fes_outputs(u, N_k, f, s, c1), "weights")
    assert_same(under_c2, fresh_fes_outputs(u, N_k, f, s, c2), "other weights")
    assert_same(after_solve, first, "after a solve")
    for a, b in ((other_counts, first), (under_c1, first), (under_c2, under_c1)):
        assert not same(a["lognum"], b["lognum"]) and np.all(np.isfinite(a["lognum"]))


# ---- 8. NaN arguments -----------------------------------------------------------------------------------------------------------
def test_nan_arguments_make_nan_outputs():
    K, N = 5, 300
    u, N_k, f = random_problem(K, N, seed=31)
    s = small_scan(N)
    assert N_k[1] > 0
    with DeviceMatrix.from_host(u) as dm:
        dm.set_Nk(N_k)
        dm.set_scan(s["basis"], None)
        dm.set_scan_bins(s["nbins"], s["label"])
        good = fes_outputs(dm, f, s)
        f_bins = -good["lognum"]
        f_bins[11, 2] = np.nan  # one entry: every output of pass B
        for out in dm.scan_bin_gram_w(f, s["coeff"], s["offset"], f_bins):
            assert np.all(np.isnan(out))
        for bad in (np.nan, np.inf, -np.inf):  # f of a state with samples: every output of both passes
            f_bad = f.copy()
            f_bad[1] = bad
            for key, out in fes_outputs(dm, f_bad, s).items():
                assert np.all(np.isnan(out)), (bad, key)
        assert_same(fes_outputs(dm, f, s), good, "after the refused arguments")
    assert all(np.all(np.isfinite(v)) for v in good.values())


# ---- 9. refused contexts --------------------------------------------------------------------------------------------------------
MBAR_ERR_STATE = -4


def entry_points(owner, K, s, L, with_set=True):
    import ctypes as C

    lib, ctx = owner._lib, owner._ctx
    nbins = s["nbins"]
    f, f_bins = np.zeros(K), np.zeros((L, nbins))
    lognum = np.empty((L, nbins))
    X, d, w = np.empty((K, L, nbins)), np.empty((L, nbins)), np.empty((L, nbins))
    label = np.ascontiguousarray(s["label"], dtype=np.int32)
    if with_set:
        yield "mbar_ctx_set_scan_bins", lib.mbar_ctx_set_scan_bins(ctx, nbins, label.ctypes.data_as(C.POINTER(C.c_int32)))
    yield "mbar_scan_bin_lognum", lib.mbar_scan_bin_lognum(ctx, _dptr(f), L, _dptr(s["coeff"]), _dptr(s["offset"]), _dptr(lognum))
    yield "mbar_scan_bin_gram_w", lib.mbar_scan_bin_gram_w(ctx, _dptr(f), L, _dptr(s["coeff"]), _dptr(s["offset"]), _dptr(f_bins),
                                                           _dptr(X), _dptr(d), _dptr(w))


def assert_refused(owner, K, s, L, words, with_set=True):
    for name, rc in entry_points(owner, K, s, L, with_set):
        message = _lib.last_error(owner._ctx)
        assert rc == MBAR_ERR_STATE, (name, rc, message)
        assert name in message and words in message, message


def test_contexts_the_binned_scan_passes_do_not_serve_are_refused():
    N, L = 300, 4
    s = small_scan(N, L)
    u, N_k, _ = random_problem(129, N, seed=3)
    with DeviceMatrix.from_host(u) as wide:
        wide.set_Nk(N_k)
        assert_refused(wide, 129, s, L, "at most 128 states")
    u, N_k, f = random_problem(120, N, seed=77)
    with DeviceMatrix.from_host(u) as base:
        base.set_Nk(N_k)
        # before set_scan, before set_scan_bins, with observables on the family
        assert_refused(base, 120, s, L, "mbar_ctx_set_scan first", with_set=False)
        base.set_scan(s["basis"], None)
        assert_refused(base, 120, s, L, "mbar_ctx_set_scan_bins first", with_set=False)
        base.set_scan_bins(s["nbins"], s["label"])
        base.set_scan(s["basis"], np.ones((1, N)))
        assert_refused(base, 120, s, L, "Q = 0", with_set=False)
        base.set_scan(s["basis"], None)
        before = fes_outputs(base, f, s)
        e = base.extend(5)
        assert e is not None
        try:
            assert_refused(e, 125, s, L, "extension context")
        finally:
            e.close()
        with LoopbackGroup(1) as group:
            base.set_loopback(group, 0)
            assert_refused(base, 120, s, L, "transport")
            base.comm_destroy()
        assert_same(fes_outputs(base, f, s), before, "the base after the refusals")
        with pytest.raises(ValueError, match=r"\[-1, nbins\)"):
            base.set_scan_bins(3, np.where(s["label"] < 3, s["label"], 3))


def test_wide_pitch_contexts_are_refused():
    """A row pitch of 56 bytes x pitch >= 4 GiB (from 7.67e7 samples): one state, nothing uploaded -- the passes refuse before they
    read anything"""
    N, L = 76_700_000, 2  # (one state: 0.6 GB of matrix)
    s = dict(coeff=np.ones((L, 2)), offset=np.zeros(L), label=np.zeros(N, dtype=np.int32), nbins=1)
    with DeviceMatrix(1, N) as dm:
        assert_refused(dm, 1, s, L, "wide-pitch")
