"""Entropy, enthalpy and heat capacity along a scan on the MI355X (``mbar_scan_energy_lognum`` / ``mbar_scan_energy_gram_w``, the
ScanEnergy policy of mbar_k_scan.hip; ``MBAR.compute_scan_entropy_and_enthalpy``): every instantiation of the two sweeps against the
long-double stand-in (tests/scan_thermo_standin.py), the bits the passes promise (``lognum`` of ``mbar_scan_lognum``, two calls, a
member alone and at any position, any "scan_part_bytes"), the method against the reference's fixture
(tests/golden/scan_thermo_ho_K5.npz), against the dense path on the device and against dense bootstrap replicates, and the passes as
consumers of the context's state.

Tolerances.  Quantities with a twin in tests/test_gpu_scan.py take its tolerance for the same comparison: lognum and wsum 1e-11
absolute, mean / cross / within rtol 1e-10; f 1e-11, Delta_f 2e-11, dDelta_f (and dDelta_u, a sigma) rtol 1e-9 with atol 1e-14, u (a
mu) rtol 1e-10 with atol 1e-11.  refblock, var_u, dvar_u and dDelta_s have none: their bounds are an order of magnitude above the
worst error measured on the device (profiles/scan_thermo_accuracy.txt); every test prints its figures before it asserts."""
import numpy as np
import pytest

import pymbar_amd
from pymbar_amd import _lib, testsystems
from pymbar_amd.device import DeviceMatrix, LoopbackGroup, _dptr
from tests.conftest import load_golden
from tests.scan_standin import family, ladder
from tests.scan_thermo_standin import (FamilyThermoOracleMatrix, ScanThermoOracleMatrix, build_energy_case, energy_case_id, energy_cases,
                                       positive_center, run_energy_passes)
from tests.test_capi_context import PLAIN_STARTS, PLAIN_WRITERS, assert_same, same
from tests.test_gpu_parity import random_problem
from tests.test_scan_thermo_host import (DENSE_VAR_U, check_against_dense, check_against_fixture, check_against_seam_fixture, gap,
                                         seam_family)

pytestmark = pytest.mark.gpu

# no twin: ten times the worst error measured on the device (profiles/scan_thermo_accuracy.txt) -- refblock 1.8e-13 relative at the
# positive centre; at c = <u>: <t_1> 5.5e-14 absolute (about zero: an absolute bound, in units of u), <t_2> and var_u 3.9e-15
# relative; dDelta_s against the dense device path 1.0e-12 relative
REFBLOCK = dict(rtol=2e-12, atol=0)
CENTRED_MEAN_1 = dict(rtol=0, atol=6e-13)
CENTRED_MEAN_2 = dict(rtol=4e-14, atol=0)
DENSE_DDELTA_S = dict(rtol=1e-11, atol=0)


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def device_matrix(case):
    dm = DeviceMatrix.from_host(case["u"])
    dm.set_Nk(case["N_k"])
    dm.set_sample_weights(case["c"])
    dm.set_scan(case["basis"], None, **case["kinds"])
    return dm


def standin_matrix(case, u_dev):
    oracle = (FamilyThermoOracleMatrix if case["kinds"] else ScanThermoOracleMatrix)(u_dev)
    oracle.set_Nk(case["N_k"])
    oracle.set_sample_weights(case["c"])
    oracle.set_scan(case["basis"], None, **case["kinds"])
    return oracle


def plain_lognum(dm, case, members=slice(None)):
    cen = {} if case["center"] is None else dict(center_lb=case["center"][members])
    return dm.scan_lognum(case["f"], case["coeff"][members], case["offset"][members], **cen)[0]


@pytest.mark.parametrize("case", energy_cases(), ids=energy_case_id)
def test_every_energy_instantiation_against_long_double_standin(case):
    """k_scan_cross<NB, J, ScanWhole, Fam, ScanEnergy> for NB in {1, 2, 4, 8} at both ends of the state counts NB serves, J = 2 and 3,
    both families, and <0, J> through cross=False; k_scan_vec<true, ..., ScanEnergy> with them.  N = 6001 (a ragged last tile and
    chunk), multiplicities with zeros, +inf entries (linear cases), a resident state without samples, a member 900 below the others,
    a full and a ragged member panel with the reference member in the last one.  tests/test_scan_thermo_host.py shows on the CPU
    that these cases suit the stand-in."""
    c = build_energy_case(case)
    cu = positive_center(c)
    L = len(cu)
    with device_matrix(c) as dm:
        got = run_energy_passes(dm, c, cu)
        again = run_energy_passes(dm, c, cu)
        bare = run_energy_passes(dm, c, cu, cross=False)
        lone = run_energy_passes(dm, c, cu, members=slice(L - 1, L), ref=0)
        stored = plain_lognum(dm, c)
        u_dev = dm.to_host()
    want = run_energy_passes(standin_matrix(c, u_dev), c, cu)
    print(energy_case_id(case))
    for name in ("lognum", "mean", "cross", "within", "refblock", "wsum"):
        gap(name, got[name], want[name])
    assert np.all(np.isfinite(got["lognum"]))
    assert np.max(got["lognum"][:-1]) - got["lognum"][-1] > 800.0
    assert bits(got["lognum"]) == bits(stored)  # the bits of mbar_scan_lognum for the same members
    np.testing.assert_allclose(got["lognum"], want["lognum"], rtol=0, atol=1e-11)
    np.testing.assert_allclose(got["wsum"], want["wsum"], rtol=0, atol=1e-11)
    np.testing.assert_allclose(got["wsum"], 1.0, rtol=0, atol=1e-11)
    for name in ("mean", "cross", "within"):
        np.testing.assert_allclose(got[name], want[name], rtol=1e-10, atol=0)
    np.testing.assert_allclose(got["refblock"], want["refblock"], **REFBLOCK)
    for name in got:  # two identical calls: identical bits
        assert bits(got[name]) == bits(again[name]), name
    assert bare["cross"] is None  # the NB = 0 instantiation of the same J: the per-member sums are the same bits
    for name in ("within", "refblock", "wsum"):
        assert bits(bare[name]) == bits(got[name]), name
    for name in ("lognum", "mean", "wsum", "within"):  # the far member on its own: the bits it has inside the call
        assert bits(lone[name][0]) == bits(got[name][-1]), name
    assert bits(lone["cross"][:, 0]) == bits(got["cross"][:, -1])


@pytest.mark.parametrize("case", [("linear", 17, 3), ("harmonic", 65, 3), ("linear", 128, 2)], ids=energy_case_id)
def test_centred_moments_against_long_double_standin(case):
    """The method's second pass: the centre is the member's own mean (from the device's first pass), so <t_1> is about zero and
    <t_2> is the fluctuation.  The far member (900 below the others) keeps finite moments."""
    c = build_energy_case(case)
    with device_matrix(c) as dm:
        cen = {} if c["center"] is None else dict(center_lb=c["center"])
        _, mean0 = dm.scan_energy_lognum(c["f"], c["coeff"], c["offset"], center_u=None, J=2, **cen)
        cu = mean0[:, 1].copy()
        got = run_energy_passes(dm, c, cu)
        u_dev = dm.to_host()
    oracle = standin_matrix(c, u_dev)
    want0 = oracle.scan_energy_lognum(c["f"], c["coeff"], c["offset"], center_u=None, J=2, **cen)[1]
    want = run_energy_passes(oracle, c, cu)
    gap("u", mean0[:, 1], want0[:, 1])
    gap("mean_1", got["mean"][:, 1], want["mean"][:, 1])
    assert np.all(np.isfinite(got["mean"])) and cu[-1] > 800.0
    np.testing.assert_allclose(mean0[:, 1], want0[:, 1], rtol=1e-10, atol=1e-11)
    np.testing.assert_allclose(got["mean"][:, 1], want["mean"][:, 1], **CENTRED_MEAN_1)
    if case[2] > 2:
        gap("mean_2", got["mean"][:, 2], want["mean"][:, 2])
        var, var_want = got["mean"][:, 2] - got["mean"][:, 1] ** 2, want["mean"][:, 2] - want["mean"][:, 1] ** 2
        gap("var_u", var, var_want)
        assert np.all(var > 0.0)
        np.testing.assert_allclose(got["mean"][:, 2], want["mean"][:, 2], **CENTRED_MEAN_2)
        np.testing.assert_allclose(var, var_want, **CENTRED_MEAN_2)
    for name in ("within", "refblock", "cross"):  # (mixed signs: printed, the positive centre above is where they are held)
        gap(name, got[name], want[name])


@pytest.mark.parametrize("case", [("linear", 33, 3), ("harmonic", 17, 2)], ids=energy_case_id)
def test_member_bits_do_not_depend_on_the_position_or_the_company(case):
    """L = 300: the members in order and in a fixed random order (another lane column, wave and panel for nearly every one, the
    reference among them), and member 123 alone: every output of a member is the same bits."""
    fam, K, J = case
    c = build_energy_case(case)
    rng = np.random.default_rng(9)
    pick = rng.integers(0, len(c["coeff"]), 300)  # 300 members drawn from the case's
    for key in ("coeff", "offset", "center", "u_members"):
        if c[key] is not None:
            c[key] = c[key][pick]
    L, ref = 300, 299
    cu = positive_center(c)
    perm = rng.permutation(L)
    assert np.count_nonzero(perm // 16 != np.arange(L) // 16) > L // 2
    with device_matrix(c) as dm:
        first = run_energy_passes(dm, c, cu, ref=ref)
        second = run_energy_passes(dm, c, cu, members=perm, ref=int(np.flatnonzero(perm == ref)[0]))
        lone = run_energy_passes(dm, c, cu, members=slice(123, 124), ref=0)
    for name in ("lognum", "mean", "wsum", "within", "refblock"):
        assert bits(first[name][perm]) == bits(second[name]), name
    assert bits(first["cross"][:, perm]) == bits(second["cross"])
    for name in ("lognum", "mean", "wsum", "within"):
        assert bits(lone[name][0]) == bits(first[name][123]), name
    assert bits(lone["cross"][:, 0]) == bits(first["cross"][:, 123])
    assert np.all(np.isfinite(first["lognum"]))


def test_pass_a_member_panels_do_not_change_a_bit():
    """Context option "scan_part_bytes" = 1: panels of 64 members, here 64 + 64 + 17; at its default: one panel."""
    c = build_energy_case(("linear", 5, 2))
    cu = positive_center(c)
    c["J"] = 3

    def pass_a(dm):
        return dm.scan_energy_lognum(c["f"], c["coeff"], c["offset"], center_u=cu, J=3)

    with device_matrix(c) as dm:
        dm.set_option("scan_part_bytes", 1)
        cut = pass_a(dm)
        dm.set_option("scan_part_bytes", 1 << 28)
        whole = pass_a(dm)
    with device_matrix(c) as dm:
        default = pass_a(dm)
    assert len(cu) == 145
    for a, b, d in zip(cut, whole, default):
        assert bits(a) == bits(b) == bits(d) and np.all(np.isfinite(a))


# ---- the method ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gold():
    return load_golden("scan_thermo_ho_K5.npz")


@pytest.fixture(scope="module")
def fixture_scan(gold):
    x_n, u_kn, N_k, _, _, _ = testsystems.config1(seed=0)
    basis, coeff, offset = testsystems.harmonic_scan_family(x_n, gold["O_l"], gold["K_l"])
    mbar = pymbar_amd.MBAR(u_kn, N_k, relative_tolerance=1e-12)
    res = mbar.compute_scan_entropy_and_enthalpy(basis, coeff, offset)
    yield dict(mbar=mbar, basis=basis, coeff=coeff, offset=offset, res=res)
    mbar.close()


def test_fixture_reproduces_reference(fixture_scan, gold):
    check_against_fixture(fixture_scan["res"], gold)


def test_sweep_across_the_seam_reproduces_reference(gold):
    """The second entry of the fixture: the umbrellas of periodic_umbrella_K6.npz built by ``from_family`` on the device, 40
    unsampled restraint centres from 120 to 240 degrees (those above 180 lie outside the period)"""
    fam, members = seam_family()
    m = pymbar_amd.MBAR.from_family(fam["basis"], fam["coeff"], fam["N_k"], offset_k=fam["offset"], center_kb=fam["center"],
                                    harmonic_b=fam["harmonic"], period_b=fam["period"], relative_tolerance=1e-12)
    try:
        res = m.compute_scan_entropy_and_enthalpy(**members)
        check_against_seam_fixture(res, gold)
        lone = m.compute_scan_entropy_and_enthalpy(coeff_lb=members["coeff_lb"][21:22], center_lb=members["center_lb"][21:22])
        for key in ("f", "u", "s", "var_u", "dvar_u", "n_eff"):
            assert lone[key][0] == res[key][21], key
    finally:
        m.close()


def test_method_is_bit_reproducible_and_members_are_independent(fixture_scan):
    s = fixture_scan
    mbar, res = s["mbar"], s["res"]
    again = mbar.compute_scan_entropy_and_enthalpy(s["basis"], s["coeff"], s["offset"])
    for key in res:
        assert bits(again[key]) == bits(res[key]), key
    assert bits(mbar.compute_scan(s["basis"], s["coeff"], s["offset"], compute_uncertainty=False)["f"]) == bits(res["f"])
    lone = mbar.compute_scan_entropy_and_enthalpy(s["basis"], s["coeff"][7:8], s["offset"][7:8])
    for key in ("f", "u", "s", "var_u", "dvar_u", "n_eff"):
        assert lone[key][0] == res[key][7], key
    pair = mbar.compute_scan_entropy_and_enthalpy(s["basis"], s["coeff"][[0, 7]], s["offset"][[0, 7]])
    for key in res:
        assert pair[key][1] == res[key][7], key


def gpu_dense(mbar, basis, coeff, offset, reference, method=None):
    return check_against_dense(mbar, basis, coeff, offset, reference, method, dtol=dict(rtol=1e-9, atol=1e-14), stol=DENSE_DDELTA_S)


def test_fixture_method_against_dense_path(fixture_scan):
    s = fixture_scan
    for method in (None, "approximate"):
        gpu_dense(s["mbar"], s["basis"], s["coeff"], s["offset"], reference=0, method=method)


@pytest.mark.parametrize("shape", [(17, 4099, 40, 8), (128, 6001, 40, 2)], ids=lambda s: "K%d-N%d-L%d-B%d" % s)
def test_method_against_dense_path(shape):
    K, N, L, B = shape
    rng = np.random.default_rng(K)
    x_n, u_kn, N_k, O_k, K_k = ladder(K, N, seed=1)
    basis, coeff, offset = family(x_n, O_k, K_k, L, B, rng)
    mbar = pymbar_amd.MBAR(u_kn, N_k, relative_tolerance=1e-12)
    try:
        gpu_dense(mbar, basis, coeff, offset, reference=4)
    finally:
        mbar.close()


def test_bootstrap_equals_dense_replicates(gold):
    x_n, u_kn, N_k, _, _, _ = testsystems.config1(seed=0)
    basis, coeff, offset = testsystems.harmonic_scan_family(x_n, gold["O_l"][::5], gold["K_l"][::5])
    L = len(coeff)
    mbar = pymbar_amd.MBAR(u_kn, N_k, n_bootstraps=3, bootstrap_rng="device", rseed=11)
    try:
        res = mbar.compute_scan_entropy_and_enthalpy(basis, coeff, offset, uncertainty_method="bootstrap")
        for name in ("bootstrapped_f", "bootstrapped_u", "bootstrapped_var_u"):
            assert res[name].shape == (3, L), name
        u_ln = coeff @ basis + offset[:, None]
        state_map = np.vstack([np.arange(L), np.arange(L)])
        inner = mbar.compute_expectations_inner(u_ln, u_ln, state_map, uncertainty_method="bootstrap")
        inner2 = mbar.compute_expectations_inner(u_ln ** 2, u_ln, state_map, uncertainty_method="bootstrap")
        var_dense = inner2["bootstrapped_observables"] - inner["bootstrapped_observables"] ** 2
        gap("boot f", res["bootstrapped_f"], inner["bootstrapped_f"])
        gap("boot u", res["bootstrapped_u"], inner["bootstrapped_observables"])
        gap("boot var_u", res["bootstrapped_var_u"], var_dense)
        np.testing.assert_allclose(res["bootstrapped_f"], inner["bootstrapped_f"], rtol=0, atol=1e-11)
        np.testing.assert_allclose(res["bootstrapped_u"], inner["bootstrapped_observables"], rtol=1e-10, atol=1e-11)
        np.testing.assert_allclose(res["bootstrapped_var_u"], var_dense, **DENSE_VAR_U)
        # the spread of the differences, as compute_entropy_and_enthalpy takes it, from the dense replicates (the dense method
        # itself pairs the replicates of u_ln with f_k_boots of the K sampled states and serves u_ln of K rows only)
        fb, ub = inner["bootstrapped_f"], inner["bootstrapped_observables"]
        for name, arr in (("dDelta_f", fb), ("dDelta_u", ub), ("dDelta_s", ub - fb)):
            want = np.std(arr - arr[:, :1], axis=0)
            gap(name, res[name], want)
            np.testing.assert_allclose(res[name], want, rtol=1e-7, atol=1e-12)
        assert np.all(res["dvar_u"] > 0) and mbar._dm._wtag is None  # the multiplicities do not leak
    finally:
        mbar.close()


# ---- the passes as consumers of the context's state -----------------------------------------------------------------------------------

def small_scan(N, L=20):
    rng = np.random.default_rng(3)
    return dict(basis=rng.normal(0.0, 1.0, (2, N)), coeff=rng.uniform(0.0, 1.0, (L, 2)), offset=rng.normal(0.0, 1.0, L), ref=7 % L,
                center_u=rng.normal(0.0, 1.0, L))


def energy_outputs(dm, f, s, center_u=None):
    """Both passes at f; pass B at f_scan = -lognum and at f_scan = 0 (finite whatever pass A returned)"""
    cu = s["center_u"] if center_u is None else center_u
    lognum, mean = dm.scan_energy_lognum(f, s["coeff"], s["offset"], center_u=cu, J=3)
    out = dict(lognum=lognum, mean=mean)
    for tag, f_scan in (("", -lognum), ("0 ", np.zeros(len(lognum)))):
        X, within, refblock, w = dm.scan_energy_gram_w(f, s["coeff"], s["offset"], f_scan, center_u=cu, J=3, reference=s["ref"])
        out.update({tag + "cross": X, tag + "within": within, tag + "refblock": refblock, tag + "wsum": w})
    return out


def fresh_energy_outputs(u, N_k, f, s):
    with DeviceMatrix.from_host(u) as fresh:
        fresh.set_Nk(N_k)
        fresh.set_scan(s["basis"], None)
        return energy_outputs(fresh, f, s)


@pytest.mark.parametrize("writer", sorted(PLAIN_WRITERS))
def test_energy_passes_after_every_writer_of_the_matrix(writer):
    """As test_scan_passes_after_every_writer_of_the_matrix: a context scanned at f, changed through one writer of the C ABI and
    scanned again at the same f gives what a fresh context gives for the final matrix."""
    K, N = 5, 300
    u, N_k, f = random_problem(K, N, seed=31)
    rng = np.random.default_rng(5)
    start = PLAIN_STARTS.get(writer, lambda u: u)(u)
    s = small_scan(N)
    with DeviceMatrix.from_host(start) as dm:
        dm.set_Nk(N_k)
        dm.set_scan(s["basis"], None)
        before = energy_outputs(dm, f, s)
        PLAIN_WRITERS[writer](dm, u, rng)
        got = energy_outputs(dm, f, s)
        final = dm.to_host()
    want = fresh_energy_outputs(final, N_k, f, s)
    assert_same(got, want, writer)
    for key in got:
        assert bool(np.isnan(before[key]).all()) == bool(np.isnan(start).any()), key
        assert bool(np.isnan(got[key]).all()) == bool(np.isnan(final).any()), key
        assert bool(np.isfinite(got[key]).all()) != bool(np.isnan(final).any()), key
        assert not same(got[key], before[key]), key


def family_members(K, N, L, seed):
    """A family (linear or with a periodic harmonic term) and L members of it at the resident states' own parameters and between"""
    basis, coeff_k, center_k, hb, pb, offset_k, N_k = testsystems.periodic_umbrella_family(K=K, n_per_state=N // K, seed=seed)
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, K, L)
    idx[:K] = np.arange(K)
    center = center_k[idx] + np.where(np.arange(L)[:, None] < K, 0.0, rng.uniform(-20.0, 20.0, (L, center_k.shape[1])))
    return dict(basis=basis, coeff_k=coeff_k, center_k=center_k, hb=hb, pb=pb, offset_k=offset_k, N_k=N_k, coeff=coeff_k[idx],
                center=np.where(hb[None, :], center, 0.0), offset=offset_k[idx])


def test_after_from_family_a_member_with_a_states_parameters_is_that_state():
    """The other two writers of the matrix, ``from_family`` (and ``from_linear``, its all-linear case below) and a row update by
    ``fill_family_rows``: the energy observable of a member with a resident state's parameters is that state's row to the bit, so
    its centred first moment about the dense row's own mean and its free energy are those of the dense path on the same matrix; a
    sweep of the centre across the +-180 degree seam stays finite."""
    K, L = 6, 40
    m = family_members(K, 1800, L, seed=2)
    kinds = dict(harmonic_b=m["hb"], period_b=m["pb"])
    with DeviceMatrix.from_family(m["basis"], m["coeff_k"], m["offset_k"], center_kb=m["center_k"], **kinds) as dm:
        dm.set_Nk(m["N_k"])
        f = np.linspace(0.0, 1.0, K)
        dm.set_scan(m["basis"], None, **kinds)
        u_dev = dm.to_host()
        ln, mean = dm.scan_energy_lognum(f, m["coeff"], m["offset"], center_u=None, J=3, center_lb=m["center"])
        # a row update, then the same members again: rows 1 and 2 swapped, members 1 and 2 follow
        swap = np.array([2, 1])
        dm.fill_family_rows(1, m["basis"], m["coeff_k"][swap], m["offset_k"][swap], center_rb=m["center_k"][swap], **kinds)
        u_swapped = dm.to_host()
        ln2, mean2 = dm.scan_energy_lognum(f, m["coeff"], m["offset"], center_u=None, J=3, center_lb=m["center"])
        # the seam: the centre of member 0 swept from 170 to 190 degrees (= -170)
        sweep = np.repeat(m["center"][:1], 21, axis=0)
        sweep[:, m["hb"]] = np.linspace(170.0, 190.0, 21)[:, None]
        ln3, mean3 = dm.scan_energy_lognum(f, np.repeat(m["coeff"][:1], 21, axis=0), np.repeat(m["offset"][:1], 21), center_u=None, J=3,
                                           center_lb=sweep)
    assert np.array_equal(u_swapped[[1, 2]], u_dev[[2, 1]]) and np.array_equal(u_swapped[[0, 3, 4, 5]], u_dev[[0, 3, 4, 5]])
    for u_mat, lognum, mn, rows in ((u_dev, ln, mean, np.arange(K)), (u_swapped, ln2, mean2, np.array([0, 2, 1, 3, 4, 5]))):
        oracle = ScanThermoOracleMatrix(u_mat)
        oracle.set_Nk(m["N_k"])
        logden = oracle._logden(f).astype(np.longdouble)
        x = -u_mat[rows].astype(np.longdouble) - logden[None, :]
        M = x.max(axis=1)
        e = np.exp(x - M[:, None])
        want_ln = (M + np.log(e.sum(axis=1))).astype(np.float64)
        want_u = ((e * u_mat[rows]).sum(axis=1) / e.sum(axis=1)).astype(np.float64)
        want_u2 = ((e * u_mat[rows].astype(np.longdouble) ** 2).sum(axis=1) / e.sum(axis=1)).astype(np.float64)
        gap("lognum", lognum[:K], want_ln)
        gap("u", mn[:K, 1], want_u)
        gap("u2", mn[:K, 2], want_u2)
        np.testing.assert_allclose(lognum[:K], want_ln, rtol=0, atol=1e-11)
        np.testing.assert_allclose(mn[:K, 1], want_u, rtol=1e-10, atol=1e-11)
        np.testing.assert_allclose(mn[:K, 2], want_u2, rtol=1e-10, atol=1e-11)
    assert np.all(np.isfinite(ln3)) and np.all(np.isfinite(mean3))
    assert bits(ln3[1]) != bits(ln3[0])


def test_after_from_linear_a_member_with_a_states_parameters_is_that_state():
    K, N = 5, 1500
    x_n, u_kn, N_k, O_k, K_k = ladder(K, N, seed=4)
    basis, coeff, offset = testsystems.harmonic_scan_family(x_n, O_k, K_k)
    f = np.linspace(0.0, 0.5, K)
    with DeviceMatrix.from_linear(basis, coeff, offset) as dm:
        dm.set_Nk(N_k)
        dm.set_scan(basis, None)
        u_dev = dm.to_host()
        ln, mean = dm.scan_energy_lognum(f, coeff, offset, center_u=None, J=2)
    oracle = ScanThermoOracleMatrix(u_dev)
    oracle.set_Nk(N_k)
    logden = oracle._logden(f).astype(np.longdouble)
    x = -u_dev.astype(np.longdouble) - logden[None, :]
    e = np.exp(x - x.max(axis=1)[:, None])
    want_u = ((e * u_dev).sum(axis=1) / e.sum(axis=1)).astype(np.float64)
    gap("u", mean[:, 1], want_u)
    np.testing.assert_allclose(mean[:, 1], want_u, rtol=1e-10, atol=1e-11)


def test_nan_arguments_make_nan_outputs():
    K, N = 5, 300
    u, N_k, f = random_problem(K, N, seed=31)
    s = small_scan(N)
    assert N_k[1] > 0
    with DeviceMatrix.from_host(u) as dm:
        dm.set_Nk(N_k)
        dm.set_scan(s["basis"], None)
        good = energy_outputs(dm, f, s)
        f_scan = -good["lognum"]
        f_scan[11] = np.nan  # one member's normaliser: every output of pass B
        for out in dm.scan_energy_gram_w(f, s["coeff"], s["offset"], f_scan, center_u=s["center_u"], J=3, reference=s["ref"]):
            assert np.all(np.isnan(out))
        cu = s["center_u"].copy()
        cu[4] = np.nan  # one member's centre: every output of both passes
        for key, out in energy_outputs(dm, f, s, center_u=cu).items():
            assert np.all(np.isnan(out)), key
        for bad in (np.nan, np.inf, -np.inf):  # f of a state with samples: every output of both passes
            f_bad = f.copy()
            f_bad[1] = bad
            for key, out in energy_outputs(dm, f_bad, s).items():
                assert np.all(np.isnan(out)), (bad, key)
        cu[4] = np.inf
        with pytest.raises(Exception, match="finite"):
            dm.scan_energy_lognum(f, s["coeff"], s["offset"], center_u=cu, J=3)
        assert_same(energy_outputs(dm, f, s), good, "after the refused arguments")
    assert all(np.all(np.isfinite(v)) for v in good.values())


def test_nan_free_energies_make_a_nan_method_result():
    x_n, u_kn, N_k, _, O_k, K_k = testsystems.config1(seed=0)
    basis, coeff, offset = testsystems.harmonic_scan_family(x_n, O_k, K_k)
    mbar = pymbar_amd.MBAR(u_kn, N_k)
    try:
        mbar.f_k = mbar.f_k.copy()
        mbar.f_k[1] = np.nan
        res = mbar.compute_scan_entropy_and_enthalpy(basis, coeff, offset, compute_uncertainty=False)
        for key in ("f", "u", "s", "var_u"):
            assert np.all(np.isnan(res[key])), key
    finally:
        mbar.close()


def test_contexts_the_energy_passes_do_not_serve_are_refused():
    """More than 128 states, an extension context, a context with a transport: MBAR_ERR_STATE naming the limit; J outside {2, 3}:
    MBAR_ERR_ARG"""
    MBAR_ERR_STATE, MBAR_ERR_ARG = -4, -1
    N, L = 300, 4
    s = small_scan(N, L)

    def entry_points(owner, K, J=3):
        lib, ctx = owner._lib, owner._ctx
        f, f_scan = np.zeros(K), np.zeros(L)
        lognum, mean = np.empty(L), np.empty((L, 3))
        X, tri, ref, w = np.empty((K, L, 3)), np.empty((L, 6)), np.empty((L, 2, 3)), np.empty(L)
        yield "mbar_scan_energy_lognum", lib.mbar_scan_energy_lognum(ctx, _dptr(f), L, _dptr(s["coeff"]), _dptr(s["offset"]),
                                                                     _dptr(s["center_u"]), J, _dptr(lognum), _dptr(mean))
        yield "mbar_scan_energy_gram_w", lib.mbar_scan_energy_gram_w(ctx, _dptr(f), L, _dptr(s["coeff"]), _dptr(s["offset"]),
                                                                     _dptr(s["center_u"]), J, _dptr(f_scan), 0, _dptr(X), _dptr(tri),
                                                                     _dptr(ref), _dptr(w))

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
        for name, rc in entry_points(base, 120):  # no basis yet
            assert rc == MBAR_ERR_STATE and "mbar_ctx_set_scan first" in _lib.last_error(base._ctx), name
        base.set_scan(s["basis"], None)
        for J in (1, 4):
            for name, rc in entry_points(base, 120, J):
                assert rc == MBAR_ERR_ARG and name in _lib.last_error(base._ctx), (name, J)
        before = energy_outputs(base, f, small_scan(N))
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
        assert_same(energy_outputs(base, f, small_scan(N)), before, "the base after the refusals")
