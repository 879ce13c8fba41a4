"""Families with harmonic terms on the MI355X (``mbar_ctx_fill_family_rows``, mbar_k_family.hip; ``mbar_ctx_set_scan_terms`` /
``mbar_ctx_set_scan_centers`` and the harmonic policy of mbar_k_scan.hip; ``MBAR.from_family``, ``compute_scan`` /
``compute_scan_fes`` with periodic members): the fill bit for bit against the model of the chain (tests/family_standin.py), the
all-linear family through either entry point and at every B, the passes against the long-double stand-in at
the tolerances of tests/test_gpu_scan.py (lognum and wsum 1e-11 absolute, the products rtol 1e-10) and at every (NB, J) the
harmonic policy is compiled for, fill and scan on one chain, the binned cut, the class journey, the reference's fixture and the
refusals of the library.  Shapes are (K, N, L, B, H, Q)."""
import ctypes as C

import numpy as np
import pytest

import pymbar_amd
from pymbar_amd import _lib, fes
from pymbar_amd import testsystems as ts
from pymbar_amd.device import DeviceMatrix, _dptr
from tests.conftest import load_golden
from tests.family_standin import (PASS_SHAPES, FamilyOracleMatrix, build_family_case, family_case_id, family_instantiation_cases,
                                  load_family_case, run_family_fes_passes, run_family_passes, u_model_family)
from tests.family_standin import u_model
from tests.scan_fes_standin import build_fes_case, check_passes, check_row_against_label_path, run_fes_passes
from tests.scan_fes_standin import load_case as load_fes_case
from tests.scan_standin import build_case, run_passes
from tests.test_gpu_scan import SHAPES as LINEAR_SHAPES

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -4  # MBAR_ERR_ARG, MBAR_ERR_STATE (include/mbar_hip.h)


def bits(a):
    return np.ascontiguousarray(a).tobytes()


# ---- the fill ----------------------------------------------------------------------------------------------------------------
P = 360.0
PROBES = np.array([0.0, 0.5 * P, -0.5 * P, np.nextafter(0.5 * P, 0), np.nextafter(0.5 * P, P), np.nextafter(-0.5 * P, 0),
                   np.nextafter(-0.5 * P, -P), P, -P, 7.3 * P, -7.3 * P])


def fill_family(R, N, B, seed=0):
    """R rows over N samples; B = 3: linear | periodic (P = 360) | harmonic (P = 0); B = 1: periodic.  Row 0's centre of the
    periodic term is 32 and the first columns hold 32 + d for the probe distances d (exact: 32 + d and back lose no bit for these
    d); rows 1 and 2 have their centres outside the period."""
    rng = np.random.default_rng(seed + R + N)
    harmonic = np.array([False, True, True][:B] if B == 3 else [True])
    period = np.array([0.0, P, 0.0][:B] if B == 3 else [P])
    hp = 1 if B == 3 else 0  # the periodic term
    basis = rng.uniform(-180.0, 180.0, (B, N))
    if B == 3:
        basis[0] = rng.normal(0.0, 2.0, N)
    n = min(N, len(PROBES))
    basis[hp, :n] = 32.0 + PROBES[:n]
    assert np.array_equal(basis[hp, :n] - 32.0, PROBES[:n])
    coeff = np.where(harmonic[None, :], rng.uniform(0.001, 0.01, (R, B)), rng.uniform(0.5, 1.5, (R, B)))
    center = np.where(harmonic[None, :], rng.uniform(-180.0, 180.0, (R, B)), 0.0)
    center[0, hp] = 32.0
    if R >= 3:
        center[1, hp], center[2, hp] = 500.0, -725.5
    return basis, coeff, center, rng.normal(0.0, 1.0, R), harmonic, period


EVERY_B = range(1, 9)  # every B the fill kernel is compiled for, under both policies


def every_b_family(B):
    """131 rows over 259 samples with H = min(B, 1 + B % 4) harmonic terms among the B: the row-group seam at 128 and a remainder of
    the row loop's unroll by 2 and by 4; 129 column pairs -- a second workgroup with one pair -- and the odd column."""
    case = build_family_case((3, 259, 131, B, min(B, 1 + B % 4), 0))
    return case["basis"], case["coeff"], case["center"], case["offset"], case["harmonic_b"], case["period_b"]


@pytest.mark.parametrize("shape", [(130, 1027, 3), (5, 1, 1)] + [(131, 259, "every%d" % B) for B in EVERY_B],
                         ids=lambda s: "R%d-N%d-B%s" % s)
def test_fill_has_the_models_bits(shape):
    """130 rows: the row-group seam at 128; N = 1027: two workgroups of column pairs and the odd column; N = 1: the odd column alone;
    every1 .. every8: the harmonic policy at every B it is compiled for (every_b_family)"""
    R, N, B = shape
    every = isinstance(B, str)
    basis, coeff, center, off, hb, pb = every_b_family(int(B[5:])) if every else fill_family(R, N, B)
    assert basis.shape[1] == N and coeff.shape[0] == R and hb.any()
    want = u_model_family(basis, coeff, off, center, hb, pb)
    with DeviceMatrix.from_family(basis, coeff, off, center, hb, pb) as dm:
        got = dm.to_host()
    diff = got != want
    print("entries that differ from the model:", int(diff.sum()), "of", diff.size)
    assert np.array_equal(got, want)
    # the probes are what they are there for: a tie gives (P / 2)^2 from either side, a whole period gives 0
    hp = 1 if B == 3 else 0
    if not every and N >= len(PROBES):
        one = u_model_family(basis[hp:hp + 1], np.ones((1, 1)), None, center[:1, hp:hp + 1], [True], [P])[0]
        assert one[1] == one[2] == (0.5 * P) ** 2 and one[7] == one[8] == 0.0 and one[3] < one[1] and one[4] < one[1]


def test_partial_fill_padding_and_shards():
    """Rows outside the call are untouched; what lies behind column N stays zero (the sweeps read whole tiles: they return the bits
    they return on an uploaded copy); a column shard is the matching slice."""
    R, N, B = 5, 301, 3
    basis, coeff, center, off, hb, pb = fill_family(R, N, B, seed=3)
    want = u_model_family(basis, coeff, off, center, hb, pb)
    host = np.random.default_rng(1).normal(size=(9, N))
    with DeviceMatrix.from_host(host) as dm:
        v0 = dm._version
        dm.fill_family_rows(2, basis, coeff, off, center, hb, pb)
        assert dm._version > v0
        got = dm.to_host()
    expect = host.copy()
    expect[2:7] = want
    assert np.array_equal(got, expect)
    N_k = np.full(R, N // R)
    N_k[0] += N - N_k.sum()
    f = np.random.default_rng(2).normal(size=R)
    out = []
    for make in (lambda: DeviceMatrix.from_family(basis, coeff, off, center, hb, pb), lambda: DeviceMatrix.from_host(want)):
        with make() as dm:
            dm.set_Nk(N_k)
            out.append((dm.eval(f, gram=True), dm.lognum(f), dm.gram_w(f)))
    (ea, la, ga), (eb, lb, gb) = out
    for a, b in zip(ea + (la,) + ga, eb + (lb,) + gb):
        assert np.array_equal(a, b)
    for n0, n1 in ((0, 129), (129, 301), (7, 8)):
        with DeviceMatrix.from_family(basis, coeff, off, center, hb, pb, columns=(n0, n1)) as dm:
            assert dm.shape == (R, n1 - n0) and np.array_equal(dm.to_host(), want[:, n0:n1])


# ---- the linear policy is what it was ---------------------------------------------------------------------------------------
def capi_fill(symbol, basis, coeff, off, *family):
    """The rows of one direct call of an exported fill entry point (``family``: center, kind, period behind the linear one's
    arguments) on an empty matrix."""
    ptr = lambda a, t=C.c_double: None if a is None else a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    R, (B, N) = coeff.shape[0], basis.shape
    with DeviceMatrix.empty(R, N) as dm:
        args = [dm._ctx, 0, R, B, ptr(basis), N, 0, ptr(coeff)]
        if family:
            center, kind, period = family
            args += [ptr(center), ptr(off), ptr(kind, C.c_int32), ptr(period)]
        else:
            args += [ptr(off)]
        dm._check(getattr(dm._lib, symbol)(*args))
        return dm.to_host()


def test_all_linear_family_returns_the_bits_of_the_linear_entry_points():
    shape = LINEAR_SHAPES[1]
    case = build_case(shape, True)
    K, N, L, B, Q = shape
    none = np.zeros(B, dtype=bool)
    zeros = np.zeros((L, B))
    # the fill: one direct call per exported symbol
    basis, coeff, off = (np.ascontiguousarray(case[k], dtype=np.float64) for k in ("basis", "coeff", "offset"))
    ua = capi_fill("mbar_ctx_fill_linear_rows", basis, coeff[:K].copy(), off[:K].copy())
    ub = capi_fill("mbar_ctx_fill_family_rows", basis, coeff[:K].copy(), off[:K].copy(), np.zeros((K, B)), np.zeros(B, dtype=np.int32), np.zeros(B))
    assert np.array_equal(ua, ub) and np.array_equal(ua, u_model(case["basis"], case["coeff"][:K], case["offset"][:K]))
    # and at every B the linear policy is compiled for, on the rows and columns of every_b_family: kind NULL, and kind all zero
    # with centres and periods set and ignored
    for b in EVERY_B:
        basis, coeff, center, off, _, pb = every_b_family(b)
        want = u_model(basis, coeff, off)
        lin = capi_fill("mbar_ctx_fill_linear_rows", basis, coeff, off)
        null = capi_fill("mbar_ctx_fill_family_rows", basis, coeff, off, None, None, None)
        zero = capi_fill("mbar_ctx_fill_family_rows", basis, coeff, off, center, np.zeros(b, dtype=np.int32), pb)
        assert bits(lin) == bits(want) and bits(null) == bits(want) and bits(zero) == bits(want), b
    fcase = build_fes_case((K, N, L, B, 7), True)
    with DeviceMatrix.from_host(case["u"]) as dm:
        dm.set_Nk(case["N_k"])
        dm.set_sample_weights(case["c"])
        dm.set_scan(case["basis"], case["t"])
        old = run_passes(dm, case)
        dm.set_scan(case["basis"], case["t"], harmonic_b=none, period_b=np.zeros(B))
        lognum, mean = dm.scan_lognum(case["f"], case["coeff"], case["offset"], center_lb=zeros)
        X, within, refcol, w = dm.scan_gram_w(case["f"], case["coeff"], case["offset"], -lognum, reference=case["ref"], center_lb=zeros)
        new = dict(lognum=lognum, mean=mean, cross=X, within=within, refcol=refcol, wsum=w)
        # through the C entry points themselves: terms that are all linear, centres set and ignored
        kind = np.zeros(B, dtype=np.int32)
        dm._check(dm._lib.mbar_ctx_set_scan_terms(dm._ctx, kind.ctypes.data_as(C.POINTER(C.c_int32)), _dptr(np.zeros(B))))
        dm._check(dm._lib.mbar_ctx_set_scan_centers(dm._ctx, L, _dptr(zeros)))
        capi = run_passes(dm, case)
    for name in old:
        assert bits(old[name]) == bits(new[name]) == bits(capi[name]), name
    with DeviceMatrix.from_host(fcase["u"]) as dm:
        load_fes_case(dm, fcase)
        old = run_fes_passes(dm, fcase)
        dm.set_scan(fcase["basis"], None, harmonic_b=none, period_b=np.zeros(B))
        lognum = dm.scan_bin_lognum(fcase["f"], fcase["coeff"], fcase["offset"], center_lb=zeros)
        X, d, w = dm.scan_bin_gram_w(fcase["f"], fcase["coeff"], fcase["offset"], -lognum, center_lb=zeros)
    for name, v in dict(lognum=lognum, cross=X, diag=d, wsum=w).items():
        assert bits(old[name]) == bits(v), name


# ---- the passes against the long-double stand-in ----------------------------------------------------------------------------
def check_family_passes(shape, lone=True):
    K, N, L, B, H, Q = shape
    case = build_family_case(shape)
    ref = L - 1 if not lone else None
    with DeviceMatrix.from_host(case["u"]) as dm:
        load_family_case(dm, case)
        got = run_family_passes(dm, case, ref=ref)
        again = run_family_passes(dm, case, ref=ref)
        alone = run_family_passes(dm, case, members=slice(L - 1, L), ref=0)
        X0, within0, refcol0, w0 = dm.scan_gram_w(case["f"], case["coeff"], case["offset"], -got["lognum"],
                                                  reference=case["ref"] if ref is None else ref, cross=False, center_lb=case["center"])
        u_dev = dm.to_host()
    oracle = FamilyOracleMatrix(u_dev)
    load_family_case(oracle, case)
    want = run_family_passes(oracle, case, ref=ref)
    print(family_case_id(shape))
    for name in ("lognum", "mean", "cross", "within", "refcol", "wsum"):
        scale = np.maximum(np.abs(want[name]), 1e-300)
        print(name, "max abs error", np.max(np.abs(got[name] - want[name])), "max rel error", np.max(np.abs(got[name] - want[name]) / scale))
    assert np.all(np.isfinite(got["lognum"]))
    if L >= 5:
        assert np.max(got["lognum"][:-1]) - got["lognum"][-1] > 800.0
    np.testing.assert_allclose(got["lognum"], want["lognum"], rtol=0, atol=1e-11)
    np.testing.assert_allclose(got["wsum"], want["wsum"], rtol=0, atol=1e-11)
    np.testing.assert_allclose(got["wsum"], 1.0, rtol=0, atol=1e-11)
    for name in ("mean", "cross", "within", "refcol"):
        np.testing.assert_allclose(got[name], want[name], rtol=1e-10, atol=0)
    for name in got:  # two identical calls: identical bits
        assert bits(got[name]) == bits(again[name]), name
    for name in ("lognum", "mean", "wsum", "within"):  # the last member on its own: the bits it has inside the call
        assert bits(alone[name][0]) == bits(got[name][-1]), name
    assert bits(alone["cross"][:, 0]) == bits(got["cross"][:, -1])
    assert X0 is None  # the NB = 0 instantiation of the same J: the per-member sums are the same bits
    for name, a in (("within", within0), ("refcol", refcol0), ("wsum", w0)):
        assert bits(a) == bits(got[name]), name


@pytest.mark.parametrize("shape", PASS_SHAPES, ids=family_case_id)
def test_passes_against_long_double_standin(shape):
    """Sample weights 0 .. 3 and an unsampled resident state; 4099 / 6001 straddle the chunk of pass A (2048), 8193 that of pass B
    (8192), 70 and 130 members the panels of 64 and 128."""
    check_family_passes(shape)


@pytest.mark.parametrize("shape", family_instantiation_cases(), ids=family_case_id)
def test_every_harmonic_instantiation(shape):
    """k_scan_cross<NB, J, ScanWhole, ScanHarmonic> for every NB in {1, 2, 4, 8} and J in {1 .. 4} (and <0, J> through
    cross=False): a full panel of 64 mb(J) members and one of 17, H = 1 .. 4, the reference member the last of the last panel."""
    check_family_passes(shape, lone=False)


# ---- fill and scan share one chain -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold():
    return load_golden("periodic_umbrella_K6.npz")


@pytest.fixture(scope="module")
def umbrella():
    basis, coeff, center, harmonic, period, offset, N_k = ts.periodic_umbrella_family(K=6, n_per_state=300, seed=0)
    kw = dict(offset_k=offset, center_kb=center, harmonic_b=harmonic, period_b=period)
    m = pymbar_amd.MBAR.from_family(basis, coeff, N_k, relative_tolerance=1e-12, n_bootstraps=3, rseed=7, **kw)
    yield dict(m=m, basis=basis, coeff=coeff, center=center, harmonic=harmonic, period=period, offset=offset, N_k=N_k, kw=kw)
    m.close()


def test_members_with_the_sampled_states_parameters_are_the_resident_rows(umbrella):
    """The scan's u_l is the row the fill wrote, to the bit: against the dense path on the DOWNLOADED matrix the scan agrees at the
    tolerances of tests/test_gpu_scan.py::test_scan_against_dense_path, and its f is f_k."""
    s = umbrella
    m = s["m"]
    res = m.compute_scan(coeff_lb=s["coeff"], offset_l=s["offset"], center_lb=s["center"], reference=1)
    u_dev = m._dm.to_host()
    assert np.array_equal(u_dev, u_model_family(s["basis"], s["coeff"], s["offset"], s["center"], s["harmonic"], s["period"]))
    pert = m.compute_perturbed_free_energies(u_dev)
    inner = m.compute_expectations_inner(np.array([0]), u_dev, np.arange(6))
    print("max |f - dense| =", np.max(np.abs(res["f"] - inner["f"])), " max |f - f_k| =", np.max(np.abs(res["f"] - m.f_k)))
    np.testing.assert_allclose(res["f"], inner["f"], rtol=0, atol=1e-11)
    np.testing.assert_allclose(res["Delta_f"], pert["Delta_f"][1], rtol=0, atol=2e-11)
    np.testing.assert_allclose(res["dDelta_f"], pert["dDelta_f"][1], rtol=1e-9, atol=1e-14)
    np.testing.assert_allclose(res["f"], m.f_k, rtol=0, atol=1e-11)


@pytest.mark.parametrize("method", [None, "approximate", "bootstrap"])
def test_scan_over_300_centres_across_the_seam(umbrella, method):
    s = umbrella
    m = s["m"]
    L = 300
    coeff = np.tile([1.0, s["coeff"][0, 1]], (L, 1))
    center = np.stack([np.zeros(L), np.linspace(60.0, 300.0, L)], axis=1)
    res = m.compute_scan(coeff_lb=coeff, center_lb=center, reference=4, uncertainty_method=method)
    u_ln = u_model_family(s["basis"], coeff, None, center, s["harmonic"], s["period"])
    pert = m.compute_perturbed_free_energies(u_ln, uncertainty_method=method)
    want_d = pert["dDelta_f"] if method == "bootstrap" else pert["dDelta_f"][4]
    print(method, "max |Delta_f - dense| =", np.max(np.abs(res["Delta_f"] - pert["Delta_f"][4])))
    np.testing.assert_allclose(res["Delta_f"], pert["Delta_f"][4], rtol=0, atol=2e-11)
    if method == "bootstrap":
        np.testing.assert_allclose(res["dDelta_f"], np.std(res["bootstrapped_f"], axis=0), rtol=0, atol=0)
        np.testing.assert_allclose(res["dDelta_f"], want_d, rtol=1e-9, atol=1e-12)
    else:
        np.testing.assert_allclose(res["dDelta_f"], want_d, rtol=1e-9, atol=1e-14)


def test_fixture_reproduces_reference(umbrella, gold):
    """tests/golden/periodic_umbrella_K6.npz at the tolerances of tests/test_scan_host.py::check_against_fixture"""
    s = umbrella
    m = s["m"]
    assert np.array_equal(s["basis"][1], gold["chi_n"])
    np.testing.assert_allclose(m.f_k, gold["f_k"], rtol=0, atol=1e-9)
    r = m.compute_free_energy_differences()
    np.testing.assert_allclose(r["Delta_f"], gold["Delta_f"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(r["dDelta_f"], gold["dDelta_f"], rtol=1e-7, atol=1e-9)
    L = len(gold["chi0_l"])
    coeff = np.tile([1.0, 0.5 * gold["spring_k"][0]], (L, 1))
    center = np.stack([np.zeros(L), gold["chi0_l"]], axis=1)
    res = m.compute_scan(coeff_lb=coeff, center_lb=center)
    np.testing.assert_allclose(res["Delta_f"], gold["pert_Delta_f"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(res["dDelta_f"], gold["pert_dDelta_f"], rtol=1e-7, atol=1e-9)
    pick = gold["surface_members"]
    coeff, center = np.vstack([[1.0, 0.0], coeff[pick]]), np.vstack([[0.0, 0.0], center[pick]])
    label = np.digitize(s["basis"][1], gold["bin_edges"]) - 1
    surf = m.compute_scan_fes(coeff_lb=coeff, center_lb=center, sample_label=label, uncertainty_method="analytical")
    np.testing.assert_allclose(surf["f_i"], gold["fes_f_i"], rtol=1e-9, atol=1e-9)
    np.testing.assert_allclose(surf["df_i"], gold["fes_df_i"], rtol=1e-7, atol=1e-7)


# ---- the binned cut ----------------------------------------------------------------------------------------------------------
def test_scan_fes_over_periodic_members_is_the_label_path(umbrella):
    s = umbrella
    m = s["m"]
    L = 9
    coeff = np.tile([1.0, s["coeff"][0, 1]], (L, 1))
    center = np.stack([np.zeros(L), np.linspace(100.0, 260.0, L)], axis=1)
    label = np.digitize(s["basis"][1], np.linspace(-180.0 - 1e-9, 180.0 + 1e-9, 25)) - 1
    res = m.compute_scan_fes(coeff_lb=coeff, center_lb=center, sample_label=label, uncertainty_method="analytical")
    u_ln = u_model_family(s["basis"], coeff, None, center, s["harmonic"], s["period"])
    for l in range(L):
        check_row_against_label_path(res, l, fes.histogram_fes_labels(m, u_ln[l], label, uncertainty_method="analytical"))


def test_binned_passes_one_bin_empty_bin_and_standin():
    shape = (17, 4099, 33, 8, 4, 0)
    case = build_family_case(shape)
    N = shape[1]
    rng = np.random.default_rng(9)
    with DeviceMatrix.from_host(case["u"]) as dm:
        load_family_case(dm, case)
        whole = run_family_passes(dm, case)
        # one bin that holds every sample: the bits of the whole cut
        load_family_case(dm, case, binned=(1, np.zeros(N, dtype=np.int32)))
        one = run_family_fes_passes(dm, case)
        # seven bins, the last one emptied of every multiplicity: exact zeros there; the others against the stand-in
        label = rng.integers(0, 7, N)
        label[:7] = np.arange(7)
        case["c"] = case["c"].copy()
        case["c"][label == 6] = 0.0
        for i in range(6):
            case["c"][np.flatnonzero(label == i)[0]] = 1.0
        case.update(nbins=7, emptied=6)
        load_family_case(dm, case, binned=(7, label))
        got = run_family_fes_passes(dm, case)
        u_dev = dm.to_host()
    assert bits(one["lognum"][:, 0]) == bits(whole["lognum"]) and bits(one["wsum"][:, 0]) == bits(whole["wsum"])
    assert bits(one["diag"][:, 0]) == bits(whole["within"][:, 0, 0]) and bits(one["cross"][:, :, 0]) == bits(whole["cross"][:, :, 0])
    oracle = FamilyOracleMatrix(u_dev)
    load_family_case(oracle, case, binned=(7, label))
    want = run_family_fes_passes(oracle, case)
    check_passes(got, want, case)  # (the tolerances of tests/test_gpu_scan_fes.py; the emptied bin: exact zeros and -inf)


# ---- the class journey ---------------------------------------------------------------------------------------------------------
def test_class_matches_the_dense_constructor_on_the_downloaded_matrix(umbrella):
    s = umbrella
    m = pymbar_amd.MBAR.from_family(s["basis"], s["coeff"], s["N_k"], **s["kw"])
    try:
        rm = m.compute_free_energy_differences()
        assert m._u_kn is None  # (nothing has downloaded the matrix so far)
        d = pymbar_amd.MBAR(m._dm.to_host(), s["N_k"])
        try:
            rd = d.compute_free_energy_differences()
            assert bits(m.f_k) == bits(d.f_k)
            assert bits(rm["Delta_f"]) == bits(rd["Delta_f"]) and bits(rm["dDelta_f"]) == bits(rd["dDelta_f"])
            assert np.array_equal(m.u_kn, d.u_kn) and m._u_kn is m.u_kn
        finally:
            d.close()
    finally:
        m.close()


# ---- refusals through the library ---------------------------------------------------------------------------------------------
def test_library_refusals():
    K, N, B = 4, 37, 2
    rng = np.random.default_rng(0)
    basis, coeff, center, off = rng.normal(size=(B, N)), rng.uniform(0.1, 1.0, (K, B)), rng.normal(size=(K, B)), np.zeros(K)
    ip = C.POINTER(C.c_int32)
    kind = np.array([0, 1], dtype=np.int32)
    five = np.ones(5, dtype=np.int32)
    with DeviceMatrix.from_host(rng.normal(size=(K, N))) as dm:
        lib, ctx = dm._lib, dm._ctx
        before = dm.to_host()

        def fill(B_, basis_, coeff_, center_, kind_, period_):
            return lib.mbar_ctx_fill_family_rows(ctx, 0, K, B_, _dptr(basis_), N, 0, _dptr(coeff_), _dptr(center_), _dptr(off),
                                                 None if kind_ is None else kind_.ctypes.data_as(ip), _dptr(period_))

        b5, c5 = np.ascontiguousarray(np.tile(basis[:1], (5, 1))), np.ones((K, 5))
        assert fill(5, b5, c5, np.zeros((K, 5)), five, np.zeros(5)) == ERR_ARG and "at most 4" in _lib.last_error(ctx)
        assert fill(B, basis, coeff, center, kind, np.array([0.0, -1.0])) == ERR_ARG and "period" in _lib.last_error(ctx)
        assert fill(B, basis, coeff, center, kind, np.array([0.0, np.nan])) == ERR_ARG
        assert fill(B, basis, coeff, None, kind, np.zeros(B)) == ERR_ARG and "centres" in _lib.last_error(ctx)
        for bad in (np.inf, np.nan):
            cbad, xbad = center.copy(), coeff.copy()
            cbad[1, 1] = xbad[2, 0] = bad
            assert fill(B, basis, coeff, cbad, kind, np.zeros(B)) == ERR_ARG
            assert fill(B, basis, xbad, center, kind, np.zeros(B)) == ERR_ARG
        assert np.array_equal(dm.to_host(), before)  # a refused call writes nothing
        # the scan side
        dm.set_Nk(np.array([10, 10, 10, 7]))
        f = np.zeros(K)
        assert lib.mbar_ctx_set_scan_terms(ctx, kind.ctypes.data_as(ip), _dptr(np.zeros(B))) == ERR_STATE  # no basis yet
        dm.set_scan(basis, None)
        assert lib.mbar_ctx_set_scan_terms(ctx, kind.ctypes.data_as(ip), _dptr(np.array([0.0, -360.0]))) == ERR_ARG
        assert lib.mbar_ctx_set_scan_terms(ctx, kind.ctypes.data_as(ip), _dptr(np.array([0.0, np.inf]))) == ERR_ARG
        dm.set_scan(b5, None)
        assert lib.mbar_ctx_set_scan_terms(ctx, five.ctypes.data_as(ip), _dptr(np.zeros(5))) == ERR_ARG
        dm.set_scan(basis, None)
        assert lib.mbar_ctx_set_scan_terms(ctx, kind.ctypes.data_as(ip), _dptr(np.array([0.0, 360.0]))) == _lib.MBAR_OK
        L = 3
        lognum = np.empty(L)
        args = (ctx, _dptr(f), L, _dptr(coeff[:L]), _dptr(off[:L]), _dptr(lognum), None)
        assert lib.mbar_scan_lognum(*args) == ERR_STATE                    # centres missing
        msg = _lib.last_error(ctx)
        assert "mbar_scan_lognum" in msg and "mbar_ctx_set_scan_centers" in msg
        assert lib.mbar_ctx_set_scan_centers(ctx, 4, _dptr(center)) == _lib.MBAR_OK
        assert lib.mbar_scan_lognum(*args) == ERR_STATE                    # centres of another L
        assert "mbar_scan_lognum" in _lib.last_error(ctx) and "4 members" in _lib.last_error(ctx)
        w = np.empty(L)
        assert lib.mbar_scan_gram_w(ctx, _dptr(f), L, _dptr(coeff[:L]), _dptr(off[:L]), _dptr(np.zeros(L)), 0, None, _dptr(np.empty(L)),
                                    _dptr(np.empty(L)), _dptr(w)) == ERR_STATE
        assert "mbar_scan_gram_w" in _lib.last_error(ctx)
        dm.set_scan_bins(1, np.zeros(N, dtype=np.int32))
        assert lib.mbar_scan_bin_lognum(ctx, _dptr(f), L, _dptr(coeff[:L]), _dptr(off[:L]), _dptr(lognum)) == ERR_STATE
        assert "mbar_scan_bin_lognum" in _lib.last_error(ctx)
        assert lib.mbar_scan_bin_gram_w(ctx, _dptr(f), L, _dptr(coeff[:L]), _dptr(off[:L]), _dptr(np.zeros((L, 1))), None,
                                        _dptr(np.empty((L, 1))), _dptr(np.empty((L, 1)))) == ERR_STATE
        assert "mbar_scan_bin_gram_w" in _lib.last_error(ctx)
        cbad = center[:L].copy()
        cbad[0, 1] = np.nan
        assert lib.mbar_ctx_set_scan_centers(ctx, L, _dptr(cbad)) == ERR_ARG
        assert lib.mbar_ctx_set_scan_centers(ctx, L, _dptr(np.ascontiguousarray(center[:L]))) == _lib.MBAR_OK
        xbad = coeff[:L].copy()
        xbad[1, 0] = np.inf
        assert lib.mbar_scan_lognum(ctx, _dptr(f), L, _dptr(xbad), _dptr(off[:L]), _dptr(lognum), None) == ERR_ARG
        assert lib.mbar_scan_lognum(*args) == _lib.MBAR_OK and np.all(np.isfinite(lognum))
        # another set_scan returns to the all-linear family: no centres asked for
        dm.set_scan(basis, None)
        assert lib.mbar_scan_lognum(*args) == _lib.MBAR_OK
        # the Python face: the same refusals as ValueError
        with pytest.raises(ValueError, match="at most 4"):
            dm.set_scan(b5, None, harmonic_b=np.ones(5, dtype=bool))
        dm.set_scan(basis, None, harmonic_b=np.array([False, True]), period_b=[0.0, 360.0])
        with pytest.raises(ValueError, match="center_lb is required"):
            dm.scan_lognum(f, coeff[:L], off[:L])
        with pytest.raises(ValueError, match="center_lb"):
            dm.scan_lognum(f, coeff[:L], off[:L], center_lb=center)
