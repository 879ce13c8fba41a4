"""Scans over a linear family of unsampled states on the MI355X (``mbar_ctx_set_scan`` / ``mbar_scan_lognum`` / ``mbar_scan_gram_w``,
mbar_k_scan.hip; ``MBAR.compute_scan``): the two passes against the long-double stand-in (tests/scan_standin.py), the scan against
the dense path on the device, the reference's fixture (tests/golden/scan_ho_K5_L300.npz), bit reproducibility, independence of a
member from the others in the call, and the bootstrap replicates.

Tolerances of the passes are the label path's for the same quantities (tests/test_gpu_fes_histogram.py): lognum and wsum 1e-11
absolute, the products rtol 1e-10.  Shapes are (K, N, L, B, Q); 8191 / 8193 straddle the sample chunk of pass B (8192), 4099 and
6001 the chunk of pass A (2048)."""
import numpy as np
import pytest

import pymbar_amd
from pymbar_amd import testsystems
from pymbar_amd.device import DeviceMatrix
from tests.conftest import load_golden
from tests.scan_standin import ScanOracleMatrix
from tests.test_scan_host import check_against_fixture

pytestmark = pytest.mark.gpu

SHAPES = [(1, 63, 1, 1, 0), (5, 5000, 300, 3, 2), (17, 4099, 33, 8, 3), (128, 6001, 130, 2, 1), (3, 8191, 5, 2, 1), (3, 8193, 5, 2, 1)]
FEATURES = (lambda x: x * x, lambda x: x, np.ones_like, np.cos, np.sin, np.abs, np.tanh, lambda x: 0.1 * x ** 3)


def ladder(K, N, seed):
    """A harmonic ladder of K states with N samples in all, and its (x_n, u_kn, N_k, O_k, K_k)"""
    O_k, K_k = np.linspace(0.0, 2.0, K), np.linspace(1.0, 3.0, K)
    N_k = np.full(K, N // K)
    N_k[: N - N_k.sum()] += 1
    x_n, u_kn, N_k, _ = testsystems.harmonic_u_kn(O_k, K_k, N_k, seed=seed)
    return x_n, u_kn, N_k, O_k, K_k


def family(x_n, O_k, K_k, L, B, rng):
    """L members inside the hull of the sampled oscillators in the basis FEATURES[:B] (B >= 3: the offset rides on the constant
    basis vector; beyond that small random admixtures of the other features)"""
    O_l, K_l = rng.uniform(O_k.min(), O_k.max(), L), rng.uniform(K_k.min(), K_k.max(), L)
    basis = np.stack([fn(x_n) for fn in FEATURES[:B]])
    coeff = np.zeros((L, B))
    offset = np.zeros(L)
    if B == 1:
        coeff[:, 0] = 0.5 * K_l
    else:
        _, c2, off = testsystems.harmonic_scan_family(x_n, O_l, K_l)
        coeff[:, :2] = c2
        if B >= 3:
            coeff[:, 2] = off
            coeff[:, 3:] = rng.normal(0.0, 0.2, (L, B - 3))
        else:
            offset = off
    return basis, coeff, offset


def observables(x_n, Q):
    return np.stack([x_n, x_n * x_n, np.cos(x_n)])[:Q]


def build_case(shape, hard, seed=0):
    K, N, L, B, Q = shape
    rng = np.random.default_rng(seed + 17 * K + L)
    x_n, u_kn, N_k, O_k, K_k = ladder(K, N, seed)
    basis, coeff, offset = family(x_n, O_k, K_k, L, B, rng)
    t = observables(x_n, Q)
    t = t - (t.min(axis=1) - 1e-3)[:, None] if Q else t
    f = rng.normal(0.0, 0.3, K)
    c = None
    if L >= 5:
        offset[L - 1] += 900.0  # a member whose x lies far below every other's: its lognum must be finite and right
    if hard:
        c = rng.integers(0, 4, N).astype(np.float64)  # multiplicities 0 .. 3, a quarter of them zero
        if K >= 3:
            u_kn = u_kn.copy()
            u_kn[rng.integers(1, K, N // 20), rng.integers(0, N, N // 20)] = np.inf  # +inf entries (never in row 0)
            N_k = N_k.copy()
            N_k[0] += N_k[K - 1]  # a resident state without samples
            N_k[K - 1] = 0
    return dict(u=u_kn, N_k=N_k, f=f, basis=basis, coeff=coeff, offset=offset, t=t, c=c, ref=min(2, L - 1))


def run_passes(dm, case, members=slice(None), ref=None):
    coeff, offset = case["coeff"][members], case["offset"][members]
    lognum, mean = dm.scan_lognum(case["f"], coeff, offset)
    X, within, refcol, w = dm.scan_gram_w(case["f"], coeff, offset, -lognum, reference=case["ref"] if ref is None else ref)
    return dict(lognum=lognum, mean=mean, cross=X, within=within, refcol=refcol, wsum=w)


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
    pert, ex = dense_numbers(mbar, u_ln, A, method)
    inner = mbar.compute_expectations_inner(np.array([0]), u_ln, np.arange(len(u_ln)))
    others = np.arange(len(u_ln)) != reference
    print("max |f - dense| =", np.max(np.abs(res["f"] - inner["f"])),
          " max rel dDelta_f gap =", np.max(np.abs(res["dDelta_f"][others] / pert["dDelta_f"][reference][others] - 1.0)),
          " max rel sigma gap =", max(np.max(np.abs(res["sigma"][q] / e["sigma"] - 1.0)) for q, e in enumerate(ex)))
    np.testing.assert_allclose(res["f"], inner["f"], rtol=0, atol=1e-11)
    np.testing.assert_allclose(res["Delta_f"], pert["Delta_f"][reference], rtol=0, atol=2e-11)
    np.testing.assert_allclose(res["dDelta_f"], pert["dDelta_f"][reference], rtol=1e-9, atol=1e-14)
    for q, e in enumerate(ex):
        np.testing.assert_allclose(res["mu"][q], e["mu"], rtol=1e-10, atol=1e-11)
        np.testing.assert_allclose(res["sigma"][q], e["sigma"], rtol=1e-9, atol=1e-14)


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
