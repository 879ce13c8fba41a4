"""Scans over a linear family of unsampled states on the MI355X (``mbar_ctx_set_scan`` / ``mbar_scan_lognum`` / ``mbar_scan_gram_w``,
mbar_k_scan.hip; ``MBAR.compute_scan``): the two passes against the long-double stand-in (tests/scan_standin.py), the scan against
the dense path on the device, the reference's fixture (tests/golden/scan_ho_K5_L300.npz), bit reproducibility, independence of a
member from the others in the call, and the bootstrap replicates.

Tolerances of the passes are the label path's for the same quantities (tests/test_gpu_fes_histogram.py): lognum and wsum 1e-11
absolute, the products rtol 1e-10.  Shapes are (K, N, L, B, Q); 8191 / 8193 straddle the sample chunk of pass B (8192), 4099 and
6001 the chunk of pass A (2048).

The second half of the file takes the pass-B kernel through every instantiation it is compiled for (``instantiation_cases`` of
tests/scan_standin.py, the ids name NB and J), every member through every position of a call, pass A through its member-panel
cut (context option "scan_part_bytes"), and the passes through the context state they consume (slot 0, the poison flag, the
sample weights), with the same tolerances."""
import numpy as np
import pytest

import pymbar_amd
from pymbar_amd import _lib, testsystems
from pymbar_amd.device import DeviceMatrix, LoopbackGroup, _dptr
from tests.conftest import load_golden
from tests.scan_standin import (ScanOracleMatrix, build_case, case_id, family, instantiation_cases, ladder, matrix_L, observables,
                                run_passes, scan_nb_for)
from tests.test_capi_context import PLAIN_STARTS, PLAIN_WRITERS, assert_same, same
from tests.test_gpu_parity import random_problem
from tests.test_scan_host import check_against_fixture

pytestmark = pytest.mark.gpu

SHAPES = [(1, 63, 1, 1, 0), (5, 5000, 300, 3, 2), (17, 4099, 33, 8, 3), (128, 6001, 130, 2, 1), (3, 8191, 5, 2, 1), (3, 8193, 5, 2, 1)]


@pytest.mark.parametrize("hard", [False, True], ids=["plain", "weights-inf-unsampled"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "K%d-N%d-L%d-B%d-Q%d" % s)
def test_passes_against_long_double_standin(shape, hard):
    case = build_case(shape, hard)
    with DeviceMatrix.from_host(case["u"]) as dm:
        dm.set_Nk(case["N_k"])
        dm.set_sample_weights(case["c"])
        dm.set_scan(case["basis"], case["t"])
        got = run_passes(dm, case)
        again = run_passes(dm, case)
        lone = run_passes(dm, case, members=slice(shape[2] - 1, shape[2]), ref=0)
        u_dev = dm.to_host()
    oracle = ScanOracleMatrix(u_dev)
    oracle.set_Nk(case["N_k"])
    oracle.set_sample_weights(case["c"])
    oracle.set_scan(case["basis"], case["t"])
    want = run_passes(oracle, case)
    assert np.all(np.isfinite(got["lognum"]))
    if shape[2] >= 5:
        assert np.max(got["lognum"][:-1]) - got["lognum"][-1] > 800.0
    for name in ("lognum", "mean", "cross", "within", "refcol", "wsum"):
        scale = np.maximum(np.abs(want[name]), 1e-300)
        print(name, "max abs error", np.max(np.abs(got[name] - want[name])), "max rel error", np.max(np.abs(got[name] - want[name]) / scale))
    np.testing.assert_allclose(got["lognum"], want["lognum"], rtol=0, atol=1e-11)
    np.testing.assert_allclose(got["wsum"], want["wsum"], rtol=0, atol=1e-11)
    np.testing.assert_allclose(got["wsum"], 1.0, rtol=0, atol=1e-11)
    for name in ("mean", "cross", "within", "refcol"):
        np.testing.assert_allclose(got[name], want[name], rtol=1e-10, atol=0)
    for name in got:  # two identical calls: identical bits
        assert got[name].tobytes() == again[name].tobytes(), name
    for name in ("lognum", "mean", "wsum", "within"):  # the last member on its own: the bits it has inside the call
        assert lone[name][0].tobytes() == got[name][-1].tobytes(), name
    assert np.ascontiguousarray(lone["cross"][:, 0]).tobytes() == np.ascontiguousarray(got["cross"][:, -1]).tobytes()


def test_cross_block_is_optional():
    case = build_case((17, 4099, 33, 8, 3), False)
    with DeviceMatrix.from_host(case["u"]) as dm:
        dm.set_Nk(case["N_k"])
        dm.set_scan(case["basis"], case["t"])
        full = run_passes(dm, case)
        X, within, refcol, w = dm.scan_gram_w(case["f"], case["coeff"], case["offset"], -full["lognum"], reference=case["ref"], cross=False)
        dm.set_scan(None)
        with pytest.raises(Exception):
            dm.scan_lognum(case["f"], case["coeff"], case["offset"])
    assert X is None
    for a, b in ((within, full["within"]), (refcol, full["refcol"]), (w, full["wsum"])):
        assert a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def gold():
    return load_golden("scan_ho_K5_L300.npz")


@pytest.fixture(scope="module")
def fixture_scan(gold):
    x_n, u_kn, N_k, _, _, _ = testsystems.config1(seed=0)
    basis, coeff, offset = testsystems.harmonic_scan_family(x_n, gold["O_l"], gold["K_l"])
    A = np.stack([x_n, x_n * x_n])
    mbar = pymbar_amd.MBAR(u_kn, N_k, relative_tolerance=1e-12)
    res = mbar.compute_scan(basis, coeff, offset, A_qn=A)
    yield dict(mbar=mbar, basis=basis, coeff=coeff, offset=offset, A=A, res=res)
    mbar.close()


def test_fixture_reproduces_reference(fixture_scan, gold):
    res = fixture_scan["res"]
    check_against_fixture(res, gold)
    analytic = testsystems.harmonic_free_energies(gold["K_l"], subtract_component=0)
    z = np.abs(res["Delta_f"] - analytic)[1:] / res["dDelta_f"][1:]
    print("largest |Delta_f - analytic| / dDelta_f =", z.max())
    assert np.all(z < 5.0)


def test_scan_is_bit_reproducible_and_members_are_independent(fixture_scan):
    s = fixture_scan
    mbar, res = s["mbar"], s["res"]
    again = mbar.compute_scan(s["basis"], s["coeff"], s["offset"], A_qn=s["A"])
    for key in res:
        assert again[key].tobytes() == res[key].tobytes(), key
    # member 7 alone: its own quantities; Delta_f / dDelta_f need the reference member next to it
    lone = mbar.compute_scan(s["basis"], s["coeff"][7:8], s["offset"][7:8], A_qn=s["A"])
    assert lone["f"][0] == res["f"][7]
    for key in ("mu", "sigma"):
        assert lone[key][:, 0].tobytes() == res[key][:, 7].tobytes(), key
    pair = mbar.compute_scan(s["basis"], s["coeff"][[0, 7]], s["offset"][[0, 7]], A_qn=s["A"])
    for key in ("f", "Delta_f", "dDelta_f"):
        assert pair[key][1] == res[key][7], key
    for key in ("mu", "sigma"):
        assert pair[key][:, 1].tobytes() == res[key][:, 7].tobytes(), key


def dense_numbers(mbar, u_ln, A, method=None):
    pert = mbar.compute_perturbed_free_energies(u_ln, uncertainty_method=method)
    ex = [mbar.compute_expectations(a, u_kn=u_ln, state_dependent=False, uncertainty_method=method) for a in A]
    return pert, ex


def check_against_dense(mbar, basis, coeff, offset, A, reference, method=None):
    res = mbar.compute_scan(basis, coeff, offset, A_qn=A, reference=reference, uncertainty_method=method)
    u_ln = coeff @ basis + offset[:, None]
    pert, ex = dense_numbers(mbar, u_ln, [] if A is None else A, method)  # (no observables: free energies only)
    inner = mbar.compute_expectations_inner(np.array([0]), u_ln, np.arange(len(u_ln)))
    others = np.arange(len(u_ln)) != reference
    print("max |f - dense| =", np.max(np.abs(res["f"] - inner["f"])),
          " max rel dDelta_f gap =", np.max(np.abs(res["dDelta_f"][others] / pert["dDelta_f"][reference][others] - 1.0)),
          " max rel sigma gap =", max((np.max(np.abs(res["sigma"][q] / e["sigma"] - 1.0)) for q, e in enumerate(ex)), default=0.0))
    np.testing.assert_allclose(res["f"], inner["f"], rtol=0, atol=1e-11)
    np.testing.assert_allclose(res["Delta_f"], pert["Delta_f"][reference], rtol=0, atol=2e-11)
    np.testing.assert_allclose(res["dDelta_f"], pert["dDelta_f"][reference], rtol=1e-9, atol=1e-14)
    for q, e in enumerate(ex):
        np.testing.assert_allclose(res["mu"][q], e["mu"], rtol=1e-10, atol=1e-11)
        np.testing.assert_allclose(res["sigma"][q], e["sigma"], rtol=1e-9, atol=1e-14)
    return res


def test_fixture_scan_against_dense_path(fixture_scan):
    s = fixture_scan
    pick = np.arange(0, 300, 3)
    for method in (None, "approximate"):
        check_against_dense(s["mbar"], s["basis"], s["coeff"][pick], s["offset"][pick], s["A"], reference=0, method=method)


@pytest.mark.parametrize("shape", [(17, 4099, 33, 8, 3), (128, 6001, 40, 2, 1)], ids=lambda s: "K%d-N%d-L%d-B%d-Q%d" % s)
def test_scan_against_dense_path(shape):
    K, N, L, B, Q = shape
    rng = np.random.default_rng(K)
    x_n, u_kn, N_k, O_k, K_k = ladder(K, N, seed=1)
    basis, coeff, offset = family(x_n, O_k, K_k, L, B, rng)
    mbar = pymbar_amd.MBAR(u_kn, N_k, relative_tolerance=1e-12)
    try:
        check_against_dense(mbar, basis, coeff, offset, observables(x_n, Q), reference=4)
    finally:
        mbar.close()


def test_bootstrap_equals_dense_replicates(gold):
    x_n, u_kn, N_k, _, _, _ = testsystems.config1(seed=0)
    basis, coeff, offset = testsystems.harmonic_scan_family(x_n, gold["O_l"][::25], gold["K_l"][::25])
    A = np.stack([x_n, x_n * x_n])
    L = len(coeff)
    mbar = pymbar_amd.MBAR(u_kn, N_k, n_bootstraps=3, bootstrap_rng="device", rseed=11)
    try:
        res = mbar.compute_scan(basis, coeff, offset, A_qn=A, uncertainty_method="bootstrap")
        assert res["bootstrapped_f"].shape == (3, L) and res["bootstrapped_observables"].shape == (3, 2, L)
        u_ln = coeff @ basis + offset[:, None]
        state_map = np.zeros((2, L), int)
        state_map[0] = np.arange(L)
        for q in range(2):  # three dense-path evaluations at f_k_boots[b] with the same multiplicities
            inner = mbar.compute_expectations_inner(A[q], u_ln, state_map, uncertainty_method="bootstrap")
            np.testing.assert_allclose(res["bootstrapped_f"], inner["bootstrapped_f"], rtol=0, atol=1e-11)
            np.testing.assert_allclose(res["bootstrapped_observables"][:, q], inner["bootstrapped_observables"], rtol=1e-10, atol=1e-11)
            np.testing.assert_allclose(res["sigma"][q], np.std(inner["bootstrapped_observables"], axis=0), rtol=1e-7, atol=1e-12)
        np.testing.assert_allclose(res["dDelta_f"], np.std(res["bootstrapped_f"], axis=0), rtol=0, atol=0)
        assert np.all(np.std(res["bootstrapped_f"], axis=0) > 0)
        assert mbar._dm._wtag is None  # the multiplicities do not leak
    finally:
        mbar.close()


# ---- every instantiation of the pass-B kernel, every edge of a panel, every position of a member ----------------------------------

PRODUCTS = ("mean", "cross", "within", "refcol")


def device_matrix(case):
    dm = DeviceMatrix.from_host(case["u"])
    dm.set_Nk(case["N_k"])
    dm.set_sample_weights(case["c"])
    dm.set_scan(case["basis"], case["t"])
    return dm


def standin_matrix(case, u_dev):
    oracle = ScanOracleMatrix(u_dev)
    oracle.set_Nk(case["N_k"])
    oracle.set_sample_weights(case["c"])
    oracle.set_scan(case["basis"], case["t"])
    return oracle


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def matrix_case(K, Q):
    """The case of the instantiation matrix with K states and Q observables"""
    return next(s for s in instantiation_cases() if s[0] == K and s[4] == Q and s[1] == 77)


@pytest.mark.parametrize("shape", instantiation_cases(), ids=case_id)
def test_every_instantiation_against_long_double_standin(shape):
    """k_scan_cross<NB, J, ScanWhole> for every NB in {1, 2, 4, 8} and J in {1 .. 4} at both ends of the state counts NB serves, and
    <0, J> through cross=False, at the shapes of ``instantiation_cases`` (a full panel and a panel of 17 members; the sample, tile and chunk edges
    with more than one block), with multiplicities 0 .. 3, +inf entries, an unsampled state, and the reference member the last one
    of the last panel.  tests/test_scan_host.py shows on the CPU that these cases suit the stand-in."""
    K, N, L, B, Q = shape
    case = build_case(shape, True)
    ref = L - 1
    with device_matrix(case) as dm:
        got = run_passes(dm, case, ref=ref)
        again = run_passes(dm, case, ref=ref)
        X, within, refcol, w = dm.scan_gram_w(case["f"], case["coeff"], case["offset"], -got["lognum"], reference=ref, cross=False)
        u_dev = dm.to_host()
    want = run_passes(standin_matrix(case, u_dev), case, ref=ref)
    print(case_id(shape))
    for name in ("lognum", "mean", "cross", "within", "refcol", "wsum"):
        scale = np.maximum(np.abs(want[name]), 1e-300)
        print(name, "max abs error", np.max(np.abs(got[name] - want[name])), "max rel error", np.max(np.abs(got[name] - want[name]) / scale))
    assert np.all(np.isfinite(got["lognum"]))
    assert np.max(got["lognum"][:-1]) - got["lognum"][-1] > 800.0
    np.testing.assert_allclose(got["lognum"], want["lognum"], rtol=0, atol=1e-11)
    np.testing.assert_allclose(got["wsum"], want["wsum"], rtol=0, atol=1e-11)
    np.testing.assert_allclose(got["wsum"], 1.0, rtol=0, atol=1e-11)
    for name in PRODUCTS:
        np.testing.assert_allclose(got[name], want[name], rtol=1e-10, atol=0)
    for name in got:  # two identical calls: identical bits
        assert bits(got[name]) == bits(again[name]), name
    assert X is None  # the NB = 0 instantiation of the same J: the per-member sums are the same bits
    for name, a in (("within", within), ("refcol", refcol), ("wsum", w)):
        assert bits(a) == bits(got[name]), name


@pytest.mark.parametrize("K,Q", [(33, 0), (65, 1), (17, 2), (128, 3)], ids=lambda v: str(v))
def test_member_bits_do_not_depend_on_the_position(K, Q):
    """One (K, Q) per J.  The members in order and in a fixed random order (another lane column, wave, mb round and panel for nearly
    every one of them, the reference among them): every output of a member is the same bits in both calls."""
    shape = matrix_case(K, Q)
    L = shape[2]
    case = build_case(shape, True)
    ref = L - 1
    perm = np.random.default_rng(5).permutation(L)
    assert np.count_nonzero(perm // 16 != np.arange(L) // 16) > L // 2
    with device_matrix(case) as dm:
        first = run_passes(dm, case, ref=ref)
        second = run_passes(dm, case, members=perm, ref=int(np.flatnonzero(perm == ref)[0]))
    for name in ("lognum", "mean", "wsum", "within", "refcol"):
        assert bits(first[name][perm]) == bits(second[name]), name
    assert bits(first["cross"][:, perm]) == bits(second["cross"])
    assert np.all(np.isfinite(first["lognum"]))


@pytest.mark.parametrize("K,Q", [(33, 0), (65, 1), (17, 2), (128, 3)], ids=lambda v: str(v))
def test_reference_member_in_the_first_block_and_in_the_last_panel(K, Q):
    """The same members with the reference in block 0 of panel 0 and in the last block of the last panel: only refcol may change,
    and both are the stand-in's."""
    shape = matrix_case(K, Q)
    L = shape[2]
    case = build_case(shape, True)
    with device_matrix(case) as dm:
        got = {ref: run_passes(dm, case, ref=ref) for ref in (1, L - 1)}
        u_dev = dm.to_host()
    for name in ("lognum", "mean", "wsum", "within", "cross"):
        assert bits(got[1][name]) == bits(got[L - 1][name]), name
    assert bits(got[1]["refcol"]) != bits(got[L - 1]["refcol"])
    oracle = standin_matrix(case, u_dev)
    for ref in (1, L - 1):
        want = oracle.scan_gram_w(case["f"], case["coeff"], case["offset"], -got[ref]["lognum"], reference=ref, cross=False)[2]
        print("reference", ref, "refcol max rel error", np.max(np.abs(got[ref]["refcol"] - want) / np.abs(want)))
        np.testing.assert_allclose(got[ref]["refcol"], want, rtol=1e-10, atol=0)


def test_pass_a_member_panels_do_not_change_a_bit():
    """Context option "scan_part_bytes" = 1: panels of 64 members, here 64 + 64 + 2; at its default: one panel of 192."""
    shape = (5, 4099, 130, 3, 2)
    case = build_case(shape, True)
    with device_matrix(case) as dm:
        dm.set_option("scan_part_bytes", 1)
        cut = dm.scan_lognum(case["f"], case["coeff"], case["offset"])
        dm.set_option("scan_part_bytes", 1 << 28)
        whole = dm.scan_lognum(case["f"], case["coeff"], case["offset"])
        u_dev = dm.to_host()
    with device_matrix(case) as dm:  # the default of a context nobody set the option on
        default = dm.scan_lognum(case["f"], case["coeff"], case["offset"])
    for a, b, c in zip(cut, whole, default):
        assert bits(a) == bits(b) == bits(c)
    want = standin_matrix(case, u_dev).scan_lognum(case["f"], case["coeff"], case["offset"])
    print("lognum max abs error", np.max(np.abs(cut[0] - want[0])), "mean max rel error", np.max(np.abs(cut[1] - want[1]) / np.abs(want[1])))
    assert np.all(np.isfinite(cut[0]))
    np.testing.assert_allclose(cut[0], want[0], rtol=0, atol=1e-11)
    np.testing.assert_allclose(cut[1], want[1], rtol=1e-10, atol=0)


# ---- the passes as consumers of the context's state -----------------------------------------------------------------------------------

def small_scan(N, L=20):
    """B = 2, Q = 1 and L members on any matrix of N samples"""
    rng = np.random.default_rng(3)
    return dict(basis=rng.normal(0.0, 1.0, (2, N)), t=rng.uniform(0.5, 1.5, (1, N)), coeff=rng.uniform(0.0, 1.0, (L, 2)),
                offset=rng.normal(0.0, 1.0, L), ref=7 % L)


def scan_outputs(dm, f, s):
    """Both passes at f; pass B at f_scan = -lognum and at f_scan = 0 (finite whatever pass A returned: what pass B itself makes of
    the context's state)"""
    lognum, mean = dm.scan_lognum(f, s["coeff"], s["offset"])
    out = dict(lognum=lognum, mean=mean)
    for tag, f_scan in (("", -lognum), ("0 ", np.zeros(len(lognum)))):
        X, within, refcol, w = dm.scan_gram_w(f, s["coeff"], s["offset"], f_scan, reference=s["ref"])
        out.update({tag + "cross": X, tag + "within": within, tag + "refcol": refcol, tag + "wsum": w})
    return out


def fresh_scan_outputs(u, N_k, f, s, c=None):
    with DeviceMatrix.from_host(u) as fresh:
        fresh.set_Nk(N_k)
        fresh.set_sample_weights(c)
        fresh.set_scan(s["basis"], s["t"])
        return scan_outputs(fresh, f, s)


@pytest.mark.parametrize("writer", sorted(PLAIN_WRITERS))
def test_scan_passes_after_every_writer_of_the_matrix(writer):
    """K = 5, N = 300.  A context whose slot 0 holds the log-denominators of f (a scan at f left them there) is changed through one
    writer of the C ABI and scanned again at the same f: every output is that of a fresh context given the final matrix -- all NaN
    where the write made the matrix unusable, finite again where it repaired it."""
    K, N = 5, 300
    u, N_k, f = random_problem(K, N, seed=31)
    rng = np.random.default_rng(5)
    start = PLAIN_STARTS.get(writer, lambda u: u)(u)
    s = small_scan(N)
    with DeviceMatrix.from_host(start) as dm:
        dm.set_Nk(N_k)
        dm.set_scan(s["basis"], s["t"])
        before = scan_outputs(dm, f, s)
        PLAIN_WRITERS[writer](dm, u, rng)
        got = scan_outputs(dm, f, s)
        final = dm.to_host()
    want = fresh_scan_outputs(final, N_k, f, s)
    assert_same(got, want, writer)
    for key in got:
        assert bool(np.isnan(before[key]).all()) == bool(np.isnan(start).any()), key
        assert bool(np.isnan(got[key]).all()) == bool(np.isnan(final).any()), key
        assert bool(np.isfinite(got[key]).all()) != bool(np.isnan(final).any()), key
        assert not same(got[key], before[key]), key


def test_scan_passes_after_changes_of_what_slot_0_depends_on():
    """The log-denominators a scan leaves in slot 0 are those of (matrix, N_k, f); the sums also take the sample weights"""
    K, N = 5, 300
    u, N_k, f = random_problem(K, N, seed=31)
    s = small_scan(N)
    rng = np.random.default_rng(8)
    N_k2 = np.roll(N_k, 2)
    c1 = rng.integers(0, 3, N).astype(np.float64)
    c2 = np.roll(c1, 1)
    assert not np.array_equal(N_k2, N_k) and np.any((c1 == 0) != (c2 == 0))
    with DeviceMatrix.from_host(u) as dm:
        dm.set_Nk(N_k)
        dm.set_scan(s["basis"], s["t"])
        first = scan_outputs(dm, f, s)
        dm.set_Nk(N_k2)
        other_counts = scan_outputs(dm, f, s)
        dm.set_Nk(N_k)
        dm.set_sample_weights(c1)
        under_c1 = scan_outputs(dm, f, s)
        dm.set_sample_weights(c2)
        under_c2 = scan_outputs(dm, f, s)
        dm.set_sample_weights(None)
        dm.solve_adaptive(np.zeros(K), tol=1e-10, maxiter=200, min_sc_iter=0)  # (the device loop rotates the slots)
        after_solve = scan_outputs(dm, f, s)
    assert_same(first, fresh_scan_outputs(u, N_k, f, s), "first")
    assert_same(other_counts, fresh_scan_outputs(u, N_k2, f, s), "set_Nk")
    assert_same(under_c1, fresh_scan_outputs(u, N_k, f, s, c1), "weights")
    assert_same(under_c2, fresh_scan_outputs(u, N_k, f, s, c2), "other weights")
    assert_same(after_solve, first, "after a solve")
    for a, b in ((other_counts, first), (under_c1, first), (under_c2, under_c1)):
        assert not same(a["lognum"], b["lognum"]) and np.all(np.isfinite(a["lognum"]))


def test_nan_arguments_make_nan_outputs():
    K, N = 5, 300
    u, N_k, f = random_problem(K, N, seed=31)
    s = small_scan(N)
    assert N_k[1] > 0
    with DeviceMatrix.from_host(u) as dm:
        dm.set_Nk(N_k)
        dm.set_scan(s["basis"], s["t"])
        good = scan_outputs(dm, f, s)
        f_scan = -good["lognum"]
        f_scan[11] = np.nan  # one member's: every output of pass B
        for out in dm.scan_gram_w(f, s["coeff"], s["offset"], f_scan, reference=s["ref"]):
            assert np.all(np.isnan(out))
        for bad in (np.nan, np.inf, -np.inf):  # f of a state with samples: every output of both passes
            f_bad = f.copy()
            f_bad[1] = bad
            for key, out in scan_outputs(dm, f_bad, s).items():
                assert np.all(np.isnan(out)), (bad, key)
        assert_same(scan_outputs(dm, f, s), good, "after the refused arguments")
    assert all(np.all(np.isfinite(v)) for v in good.values())


def test_contexts_the_scan_passes_do_not_serve_are_refused():
    """More than 128 states, an extension context, a context with a transport: MBAR_ERR_STATE from all three entry points, before
    anything else is looked at"""
    MBAR_ERR_STATE = -4
    N, L = 300, 4
    s = small_scan(N, L)

    def entry_points(owner, K):
        lib, ctx = owner._lib, owner._ctx
        f, f_scan = np.zeros(K), np.zeros(L)
        lognum, mean = np.empty(L), np.empty((L, 2))
        X, tri, refcol, w = np.empty((K, L, 2)), np.empty((L, 3)), np.empty((L, 2)), np.empty(L)
        yield "mbar_ctx_set_scan", lib.mbar_ctx_set_scan(ctx, 2, _dptr(s["basis"]), 1, _dptr(s["t"]))
        yield "mbar_scan_lognum", lib.mbar_scan_lognum(ctx, _dptr(f), L, _dptr(s["coeff"]), _dptr(s["offset"]), _dptr(lognum), _dptr(mean))
        yield "mbar_scan_gram_w", lib.mbar_scan_gram_w(ctx, _dptr(f), L, _dptr(s["coeff"]), _dptr(s["offset"]), _dptr(f_scan), 0,
                                                       _dptr(X), _dptr(tri), _dptr(refcol), _dptr(w))

    def assert_refused(owner, K, words):
        for name, rc in entry_points(owner, K):
            message = _lib.last_error(owner._ctx)
            assert rc == MBAR_ERR_STATE, (name, rc, message)
            assert name in message and words in message, message

    u, N_k, _ = random_problem(129, N, seed=3)
    with DeviceMatrix.from_host(u) as wide:
        wide.set_Nk(N_k)
        assert_refused(wide, 129, "at most 128 states")
    u, N_k, f = random_problem(120, N, seed=77)
    with DeviceMatrix.from_host(u) as base:
        base.set_Nk(N_k)
        base.set_scan(s["basis"], s["t"])
        before = scan_outputs(base, f, small_scan(N))
        e = base.extend(5)
        assert e is not None
        try:
            assert_refused(e, 125, "extension context")
        finally:
            e.close()
        with LoopbackGroup(1) as group:
            base.set_loopback(group, 0)
            assert_refused(base, 120, "transport")
            base.comm_destroy()
        assert_same(scan_outputs(base, f, small_scan(N)), before, "the base after the refusals")


# ---- compute_scan: no observables, the reference member far from the first block ----------------------------------------------------

@pytest.mark.parametrize("shape", [(40, 4000, 273, 2, 0), (128, 4000, 81, 2, 3)], ids=case_id)
def test_scan_against_dense_path_with_the_last_member_as_reference(shape):
    """J = 1 (no observables: a free-energy curve) at NB = 4 with a full panel of 256 members and a second one, and J = 4 at NB = 8;
    the reference member is the last one of the last panel."""
    K, N, L, B, Q = shape
    rng = np.random.default_rng(K)
    x_n, u_kn, N_k, O_k, K_k = ladder(K, N, seed=1)
    basis, coeff, offset = family(x_n, O_k, K_k, L, B, rng)
    assert L == matrix_L(Q) and scan_nb_for(K) == (4 if Q == 0 else 8)
    mbar = pymbar_amd.MBAR(u_kn, N_k, relative_tolerance=1e-12)
    try:
        for method in (None, "approximate"):
            res = check_against_dense(mbar, basis, coeff, offset, observables(x_n, Q) if Q else None, reference=L - 1, method=method)
            assert ("mu" in res) == ("sigma" in res) == (Q > 0)
    finally:
        mbar.close()
