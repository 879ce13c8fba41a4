"""Histogram free energy surfaces along a scan (``MBAR.compute_scan_fes``), host logic on the CPU stand-in
(tests/scan_fes_standin.py): the table builder of the C ABI (host only, no device), the bordered ``df_i`` against the dense
augmented ``Theta``, the reference's own numbers (tests/golden/scan_fes_ho_K5.npz from make_golden_scan_fes.py), "approximate",
the bootstrap plumbing, the error paths, and that the cases of tests/test_gpu_scan_fes.py suit the stand-in."""
import ctypes as C

import numpy as np
import pytest

import pymbar_amd
from pymbar_amd import _lib, fes, testsystems
from pymbar_amd.utils import DataError, ParameterError
from tests.conftest import load_golden
from tests.scan_fes_standin import (PASS_CASES, ScanFesFloat64Matrix, ScanFesOracleMatrix, build_fes_case, check_passes,
                                    check_row_against_label_path, labels_for, load_case, run_fes_passes)


@pytest.fixture
def standin(monkeypatch):
    import pymbar_amd.device

    monkeypatch.setattr(pymbar_amd.device, "DeviceMatrix", ScanFesOracleMatrix)


@pytest.fixture(scope="module")
def gold():
    return load_golden("scan_fes_ho_K5.npz")


@pytest.fixture(scope="module")
def config1():
    x_n, u_kn, N_k, _, _, _ = testsystems.config1(seed=0)
    np.testing.assert_array_equal(u_kn, load_golden("config1_ho_K5_N5000.npz")["u_kn"])
    return x_n, u_kn, N_k


# ---- the table builder ------------------------------------------------------------------------------------------------------------
def bins_table(label, nbins):
    lib = _lib.load_library()
    label = np.ascontiguousarray(label, dtype=np.int32)
    N = len(label)
    perm = np.full(max(N, 1), -7, dtype=np.int32)
    start = np.empty(nbins + 1, dtype=np.int64)
    rc = lib.mbar_scan_bins_table(N, nbins, label.ctypes.data_as(C.POINTER(C.c_int32)), perm.ctypes.data_as(C.POINTER(C.c_int32)),
                                  start.ctypes.data_as(C.POINTER(C.c_int64)))
    return rc, perm, start


@pytest.mark.parametrize("kind", ["shuffled", "sorted", "all-out", "one-bin", "mixed"])
@pytest.mark.parametrize("N", [1, 63, 4500, 262221])
def test_table_builder_is_a_stable_sort_by_bin(N, kind):
    rng = np.random.default_rng(N)
    nbins = 1 if kind == "one-bin" or N == 1 else min(37, N)
    if kind == "all-out":
        label = np.full(N, -1)
    elif kind == "one-bin":
        label = np.zeros(N, dtype=np.int64)
    else:
        label = labels_for(N, nbins, rng, kind)
    rc, perm, start = bins_table(label, nbins)
    assert rc == 0
    order = np.argsort(label, kind="stable")
    order = order[label[order] >= 0]
    np.testing.assert_array_equal(perm[: len(order)], order)
    assert np.all(perm[len(order):] == -7)  # nothing is written behind the last bin
    np.testing.assert_array_equal(start, np.concatenate([[0], np.cumsum(np.bincount(label[label >= 0], minlength=nbins))]))


def test_table_builder_refuses_bad_labels():
    for label, nbins in (([0, 1, 2], 2), ([0, -2, 1], 2)):
        rc, _, _ = bins_table(np.array(label), nbins)
        assert rc == -1 and "[-1, nbins)" in _lib.last_error(None)
    rc, _, _ = bins_table(np.array([0]), 0)
    assert rc == -1


# ---- the bordered covariance ----------------------------------------------------------------------------------------------------
def dense_df(mbar, u_l, label, f_raw_l, j):
    """df_i of one member from the dense augmented Theta: ``_theta_from_gram`` on ``[W | bins of the member]``"""
    W = mbar._dm.w_kn(mbar.f_k).T  # (N, K)
    logden = mbar._dm.logden(mbar.f_k)
    nbins = len(f_raw_l)
    Z = np.zeros((mbar.N, nbins))
    for i in range(nbins):
        m = label == i
        Z[m, i] = np.exp(f_raw_l[i] - u_l[m] - logden[m])
    aug = np.hstack([W, Z])
    N_aug = np.concatenate([mbar.N_k, np.zeros(nbins, dtype=mbar.N_k.dtype)])
    Theta = mbar._theta_from_gram(aug.T @ aug, N_aug, "svd-ew")[mbar.K:, mbar.K:]
    d = np.diag(Theta)
    return np.sqrt(np.maximum(d + d[j] - 2.0 * Theta[:, j], 0.0))


def _bordered_against_dense(mbar, basis, coeff, offset, label):
    for reference, ref_label in (("from-lowest", None), ("from-specified", 2)):
        res = mbar.compute_scan_fes(basis, coeff, offset, sample_label=label, reference=reference, reference_label=ref_label,
                                    uncertainty_method="analytical")
        for l in range(len(coeff)):
            want = dense_df(mbar, coeff[l] @ basis + offset[l], label, res["f_raw"][l], int(res["reference"][l]))
            print(reference, "member", l, "max |df_i - dense| =", np.max(np.abs(res["df_i"][l] - want)))
            np.testing.assert_allclose(res["df_i"][l], want, rtol=0, atol=1e-12)
            assert res["df_i"][l, res["reference"][l]] == 0.0


def fixture_family(gold, x_n):
    basis, coeff, offset = testsystems.harmonic_scan_family(x_n, gold["O_l"], gold["K_l"])
    np.testing.assert_array_equal(coeff, gold["coeff"])
    np.testing.assert_array_equal(offset, gold["offset"])
    label, grid = fes.label_samples(x_n, gold["bin_edges"])
    return basis, coeff, offset, label, np.array([g[0] for g in grid])


def test_bordered_equals_dense_theta(standin, gold, config1):
    x_n, u_kn, N_k = config1
    mbar = pymbar_amd.MBAR(u_kn, N_k, relative_tolerance=1e-12)
    basis, coeff, offset, label, _ = fixture_family(gold, x_n)
    _bordered_against_dense(mbar, basis, coeff[::3], offset[::3], label)


def test_bordered_equals_dense_theta_with_an_unsampled_state(standin):
    g = load_golden("ho_unsampled_K4_N2300.npz")
    assert np.any(g["N_k"] == 0)
    mbar = pymbar_amd.MBAR(g["u_kn"], g["N_k"], relative_tolerance=1e-12)
    rng = np.random.default_rng(3)
    basis = g["u_kn"][[0, 1, 3]]
    coeff = rng.dirichlet(np.ones(3), size=4)
    offset = rng.normal(0.0, 0.5, 4)
    label = labels_for(mbar.N, 9, rng, "mixed")
    _bordered_against_dense(mbar, basis, coeff, offset, label)


# ---- the fixture ----------------------------------------------------------------------------------------------------------------
def check_against_fixture(mbar, gold, x_n):
    """The assertions on the fixture, shared with the GPU test"""
    basis, coeff, offset, label, grid = fixture_family(gold, x_n)
    assert sorted(grid) == list(range(20))
    ref_label = int(np.flatnonzero(grid == np.digitize(gold["x_ref"], gold["bin_edges"]) - 1)[0])
    for reference, rl, tag in (("from-lowest", None, "lowest"), ("from-specified", ref_label, "specified")):
        res = mbar.compute_scan_fes(basis, coeff, offset, sample_label=label, reference=reference, reference_label=rl,
                                    uncertainty_method="analytical")
        assert res["f_raw"].shape == res["f_i"].shape == res["df_i"].shape == (8, 20) and res["f"].shape == res["reference"].shape == (8,)
        others = np.arange(20)[None, :] != res["reference"][:, None]
        print(tag, "max |f_i - reference| =", np.max(np.abs(res["f_i"] - gold["f_" + tag][:, grid])),
              " max rel df_i gap =", np.max(np.abs(res["df_i"][others] / gold["df_" + tag][:, grid][others] - 1.0)))
        np.testing.assert_allclose(res["f_raw"], gold["f_raw"][:, grid], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(res["f_i"], gold["f_" + tag][:, grid], rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(res["df_i"], gold["df_" + tag][:, grid], rtol=1e-7, atol=1e-9)
        np.testing.assert_allclose(res["f"], -np.log(np.sum(np.exp(-gold["f_raw"]), axis=1)), rtol=1e-9, atol=1e-9)
        if rl is not None:
            assert np.all(res["reference"] == rl)
    return res


def test_scan_fes_reproduces_reference(standin, gold, config1):
    x_n, u_kn, N_k = config1
    mbar = pymbar_amd.MBAR(u_kn, N_k, relative_tolerance=1e-12)
    check_against_fixture(mbar, gold, x_n)


def test_rows_are_the_label_path(standin, gold, config1):
    """Row l is what histogram_fes_labels returns for the dense u_l, for both references and theta methods"""
    x_n, u_kn, N_k = config1
    mbar = pymbar_amd.MBAR(u_kn, N_k, relative_tolerance=1e-12)
    basis, coeff, offset, label, _ = fixture_family(gold, x_n)
    for reference, rl in (("from-lowest", None), ("from-specified", 5)):
        for theta in (None, "approximate"):
            res = mbar.compute_scan_fes(basis, coeff, offset, sample_label=label, reference=reference, reference_label=rl,
                                        uncertainty_method="analytical", theta_method=theta)
            for l in range(len(coeff)):
                one = fes.histogram_fes_labels(mbar, coeff[l] @ basis + offset[l], label, reference=reference, reference_label=rl,
                                               theta_method=theta)
                check_row_against_label_path(res, l, one)
    none = mbar.compute_scan_fes(basis, coeff, offset, sample_label=label)
    assert "df_i" not in none and none["f_raw"].tobytes() == res["f_raw"].tobytes()
    assert mbar._dm._scan is None and mbar._dm._scan_bins is None


def test_approximate_is_the_bin_block(standin, gold, config1):
    x_n, u_kn, N_k = config1
    mbar = pymbar_amd.MBAR(u_kn, N_k, relative_tolerance=1e-12)
    basis, coeff, offset, label, _ = fixture_family(gold, x_n)
    res = mbar.compute_scan_fes(basis, coeff, offset, sample_label=label, uncertainty_method="analytical", theta_method="approximate")
    logden = mbar._dm.logden(mbar.f_k)
    for l in range(len(coeff)):
        Bv = np.exp(res["f_raw"][l][label] - (coeff[l] @ basis + offset[l]) - logden)
        d = np.bincount(label, weights=Bv * Bv, minlength=20)
        want = np.sqrt(d + d[res["reference"][l]])
        want[res["reference"][l]] = 0.0
        np.testing.assert_allclose(res["df_i"][l], want, rtol=1e-12, atol=0)


# ---- bootstrap ------------------------------------------------------------------------------------------------------------------
def test_bootstrap_plumbing(standin, gold, config1):
    x_n, u_kn, N_k = config1
    mbar = pymbar_amd.MBAR(u_kn, N_k, n_bootstraps=3, rseed=7)
    basis, coeff, offset, label, _ = fixture_family(gold, x_n)
    label = label.copy()
    lonely = int(label.max()) + 1
    label[np.argmax(x_n)] = lonely  # a bin of one sample: some replicate does not draw it
    nbins = lonely + 1
    res = mbar.compute_scan_fes(basis, coeff[:3], offset[:3], sample_label=label, uncertainty_method="bootstrap")
    fb = res["bootstrapped_f_raw"]
    assert fb.shape == (3, 3, nbins) and res["df_i"].shape == (3, nbins)
    emptied = np.isinf(fb[:, 0, lonely])
    assert emptied.any(), "no replicate emptied the bin of one sample: choose another rseed"
    assert np.all(np.isfinite(fb[:, :, :lonely]))
    dm = mbar._dm
    for b in range(3):  # every replicate is the label path under that replicate's weights
        mbar._set_bootstrap_weights(dm, b)
        try:
            for l in range(3):
                dm.set_bins(nbins, label, coeff[l] @ basis + offset[l])
                np.testing.assert_allclose(fb[b, l], -dm.bin_lognum(mbar.f_k_boots[b]), rtol=0, atol=1e-11)
                dm.set_bins(0)
        finally:
            dm.set_sample_weights(None)
    j = res["reference"]
    for l in range(3):
        diff = fb[:, l, :] - fb[:, l, j[l]][:, None]
        for i in range(nbins):
            use = np.isfinite(diff[:, i])
            if use.sum() >= 2:
                assert res["df_i"][l, i] == pytest.approx(np.std(diff[use, i]), rel=1e-12, abs=1e-15)
            else:
                assert np.isnan(res["df_i"][l, i])
    assert np.isnan(res["df_i"][0, lonely]) == (np.sum(~emptied) < 2)
    assert np.all(res["df_i"][np.arange(3), j] == 0.0)
    # the multiplicities are gone again: the resident matrix is the original one
    assert dm._counts is None and dm.u.shape == u_kn.shape and dm._scan is None and dm._scan_bins is None


# ---- error paths ----------------------------------------------------------------------------------------------------------------
def test_error_paths(standin, gold, config1):
    x_n, u_kn, N_k = config1
    mbar = pymbar_amd.MBAR(u_kn, N_k)
    basis, coeff, offset, label, _ = fixture_family(gold, x_n)
    call = mbar.compute_scan_fes
    with pytest.raises(ParameterError, match="svd"):
        call(basis, coeff, offset, sample_label=label, uncertainty_method="analytical", theta_method="svd")
    with pytest.raises(ParameterError):
        call(basis, coeff, offset, sample_label=label, uncertainty_method="analytical", theta_method="nonsense")
    with pytest.raises(ParameterError):
        call(basis, coeff, offset, sample_label=label, uncertainty_method="nonsense")
    with pytest.raises(ParameterError, match="without any bootstraps"):
        call(basis, coeff, offset, sample_label=label, uncertainty_method="bootstrap")
    with pytest.raises(ParameterError):
        call(basis[:, :-1], coeff, offset, sample_label=label)
    with pytest.raises(ParameterError):
        call(np.vstack([basis] * 5)[:9], np.ones((8, 9)), offset, sample_label=label)  # B = 9
    with pytest.raises(ParameterError):
        call(basis, coeff[:, :1], offset, sample_label=label)
    with pytest.raises(ParameterError):
        call(basis, coeff[:0], offset[:0], sample_label=label)
    with pytest.raises(ParameterError):
        call(basis, coeff, offset[:-1], sample_label=label)
    with pytest.raises(ParameterError):
        call(basis, coeff, offset)  # no labels
    with pytest.raises(ParameterError):
        call(basis, coeff, offset, sample_label=label[:-1])
    with pytest.raises(ParameterError):
        call(basis, coeff, offset, sample_label=np.where(label == 3, -2, label))
    with pytest.raises(DataError, match="no sample falls into any bin"):
        call(basis, coeff, offset, sample_label=np.full(len(label), -1))
    with pytest.raises(DataError, match="bin 3 has no samples"):
        call(basis, coeff, offset, sample_label=np.where(label == 3, -1, label))
    with pytest.raises(ParameterError, match="not given"):
        call(basis, coeff, offset, sample_label=label, reference="from-specified")
    with pytest.raises(ParameterError, match="not given"):
        call(basis, coeff, offset, sample_label=label, reference="from-specified", reference_label=20)
    with pytest.raises(ParameterError):
        call(basis, coeff, offset, sample_label=label, reference="from-normalization")
    for bad in (np.nan, np.inf):
        for which in range(3):
            args = [basis.copy(), coeff.copy(), offset.copy()]
            args[which].flat[3] = bad
            with pytest.raises(DataError):
                call(*args, sample_label=label)
    assert mbar._dm._scan is None and mbar._dm._scan_bins is None  # nothing is left on the matrix after a refused call


def test_handles_without_the_binned_scan_passes_are_refused(monkeypatch, config1):
    import pymbar_amd.device
    from tests.scan_standin import ScanOracleMatrix

    monkeypatch.setattr(pymbar_amd.device, "DeviceMatrix", ScanOracleMatrix)
    x_n, u_kn, N_k = config1
    mbar = pymbar_amd.MBAR(u_kn, N_k)
    with pytest.raises(ParameterError, match="not supported on this backend"):
        mbar.compute_scan_fes(np.stack([x_n * x_n, x_n]), np.ones((2, 2)), sample_label=np.zeros(len(x_n), dtype=int))


# ---- the cases of the GPU test --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hard", [False, True], ids=["plain", "hard"])
@pytest.mark.parametrize("shape,kind", PASS_CASES, ids=lambda v: v if isinstance(v, str) else "K%d-N%d-L%d-B%d-bins%d" % v)
def test_pass_cases_suit_the_standin(shape, kind, hard):
    """The cases tests/test_gpu_scan_fes.py holds the device to (rtol 1e-10 with atol 0 on the products, 1e-11 absolute on lognum
    and wsum) are cases at which the long-double stand-in is a reference: every compared entry is finite and a normal number, the
    weights are normalised, and the same formulas in plain float64 give the same numbers to 1e-12 relative (lognum: 1e-12
    absolute) -- a factor 100 (10) under the device's bound."""
    case = build_fes_case(shape, hard, kind)
    K, N, L, B, nbins = shape
    assert np.all(np.bincount(case["label"][case["label"] >= 0], minlength=nbins) > 0)
    if kind == "edges":
        assert sorted(np.bincount(case["label"][case["label"] >= 0])) == [1, 16, 17, 2047, 2049, 8193]
    out = []
    for cls in (ScanFesOracleMatrix, ScanFesFloat64Matrix):
        m = cls(case["u"])
        load_case(m, case)
        out.append(run_fes_passes(m, case))
    want, plain = out
    e = case["emptied"]
    assert (e is not None) == (hard and nbins >= 2)
    live = np.ones(nbins, dtype=bool)
    if e is not None:
        live[e] = False
    tiny = np.finfo(np.float64).tiny
    for name in ("lognum", "diag", "wsum"):
        assert np.all(np.isfinite(want[name][:, live])), name
    assert np.all(np.isfinite(want["cross"][:, :, live]))
    assert np.all(want["cross"][:, :, live] >= tiny) and np.all(want["diag"][:, live] >= tiny)
    if L >= 5:
        assert np.max(want["lognum"][:-1, live] - want["lognum"][-1, live]) > 800.0
    np.testing.assert_allclose(want["wsum"][:, live], 1.0, rtol=0, atol=1e-13)
    if e is not None:
        assert np.all(want["lognum"][:, e] == -np.inf) and np.all(want["wsum"][:, e] == 0.0)
        plain["lognum"][:, e], plain["cross"][:, :, e], plain["diag"][:, e], plain["wsum"][:, e] = -np.inf, 0.0, 0.0, 0.0
    np.testing.assert_allclose(plain["lognum"][:, live], want["lognum"][:, live], rtol=0, atol=1e-12)
    for name in ("diag", "wsum"):
        np.testing.assert_allclose(plain[name][:, live], want[name][:, live], rtol=1e-12, atol=0)
    np.testing.assert_allclose(plain["cross"][:, :, live], want["cross"][:, :, live], rtol=1e-12, atol=0)
    check_passes(plain, want, case)
