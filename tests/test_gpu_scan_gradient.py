"""Derivatives of f and of the averages along a scan on the MI355X (``mbar_scan_moments``, k_scan_moments of mbar_k_scan.hip;
``DeviceMatrix.scan_moments``, ``MBAR.compute_scan_gradient``): every bucket of the kernel against the long-double stand-in
(tests/scan_gradient_standin.py) on every output array, the bits the pass promises (``lognum`` and ``mean`` of ``mbar_scan_lognum``,
two calls, a member alone and at any position, any "scan_part_bytes"), the method against the reference's fixture
(tests/golden/scan_gradient_ho_K5.npz) and ``compute_scan``, the bootstrap replicates against direct calls, a member with a sampled
state's parameters, and the refusals.

Tolerances.  ``lognum`` has a twin in tests/test_gpu_scan.py and takes its bound, 1e-11 absolute, and ``mean`` its rtol 1e-10.  The
moments have none: their bounds are ten times the worst error measured against the stand-in over the whole matrix of cases, in the
units of ``scaled_gaps`` (profiles/scan_gradient_accuracy.txt); every test prints its figures before it asserts."""
import numpy as np
import pytest

import pymbar_amd
from pymbar_amd import _lib, testsystems
from pymbar_amd.device import DeviceMatrix, _dptr
from pymbar_amd.scan import gradient_from_moments
from tests.conftest import load_golden
from tests.scan_gradient_standin import (GradientOracleMatrix, build_moment_case, moment_case_id, moment_cases, run_moments, scaled_gaps)
from tests.test_gpu_parity import random_problem
from tests.test_scan_gradient_host import (MOMENTS_TOL, SAMPLED_STATE_TOL, check_against_fixture, check_against_seam_fixture, fixture_family,
                                           seam_family)

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def device_matrix(case):
    dm = DeviceMatrix.from_host(case["u"])
    dm.set_Nk(case["N_k"])
    dm.set_sample_weights(case["c"])
    dm.set_scan(case["basis"], case["t"], **case["kinds"])
    return dm


def standin_matrix(case, u_dev):
    oracle = GradientOracleMatrix(u_dev)
    oracle.set_Nk(case["N_k"])
    oracle.set_sample_weights(case["c"])
    oracle.set_scan(case["basis"], case["t"], **case["kinds"])
    return oracle


def t_max(case):
    return case["t"].max(axis=1) if len(case["t"]) else np.zeros(0)


def assert_moments(got, want, case, what):
    gaps = scaled_gaps(got, want, t_max(case))
    print(what, " ".join("%s %.3e" % kv for kv in gaps.items()))
    for name, v in got.items():
        assert np.all(np.isfinite(v)), (what, name)
    assert gaps["lognum"] <= 1e-11 and gaps["mean"] <= 1e-10, (what, gaps)
    for name in ("m1", "m2", "ma"):
        if name in gaps:
            assert gaps[name] <= MOMENTS_TOL[name], (what, name, gaps[name])


@pytest.mark.parametrize("case", moment_cases(), ids=moment_case_id)
def test_every_bucket_against_long_double_standin(case):
    """k_scan_moments<HB, BB> for the buckets (0, 2), (0, 8), (1, 3), (4, 8) at both ends of the families each serves, Q = 0, 1, 3, N
    = 4097 (a last chunk of one sample) and 6001 (a ragged third chunk), L = 1, 64, 65, 130; multiplicities with zeros and a whole
    chunk of zeros, an unsampled resident state, a member 900 below the others, samples at a tie of the minimum image and across the
    seam; about zero and about the first call's means."""
    N, L, B, H, Q = case
    c = build_moment_case(case)
    cen = {} if c["center"] is None else dict(center_lb=c["center"])
    with device_matrix(c) as dm:
        got0 = run_moments(dm, c)
        again = run_moments(dm, c)
        centre = got0["m1"].copy()
        got1 = run_moments(dm, c, centre)
        plain = dm.scan_lognum(c["f"], c["coeff"], c["offset"], **cen)
        lone = run_moments(dm, c, centre, members=slice(L - 1, L))
        u_dev = dm.to_host()
    oracle = standin_matrix(c, u_dev)
    want0, want1 = run_moments(oracle, c), run_moments(oracle, c, centre)
    F = B + H
    assert got0["m1"].shape == (L, F) and got0["m2"].shape == (L, F, F) and got0["ma"].shape == (L, Q, F) and got0["mean"].shape == (L, 1 + Q)
    assert_moments(got0, want0, c, "about zero ")
    assert_moments(got1, want1, c, "about means")
    for got in (got0, got1):  # the bits of mbar_scan_lognum for the same call, whatever the centres
        assert bits(got["lognum"]) == bits(plain[0]) and bits(got["mean"]) == bits(plain[1])
        assert np.array_equal(got["m2"], np.swapaxes(got["m2"], 1, 2))
    if L >= 5:
        assert np.max(got0["lognum"][:-1]) - got0["lognum"][-1] > 800.0
    for name in got0:  # two identical calls: identical bits; the last member on its own: the bits it has inside the call
        assert bits(got0[name]) == bits(again[name]), name
        assert bits(lone[name][0]) == bits(got1[name][-1]), name


@pytest.mark.parametrize("case", [(6001, 130, 8, 0, 3), (4097, 130, 8, 4, 1), (4097, 130, 2, 1, 3)], ids=moment_case_id)
def test_member_bits_do_not_depend_on_the_position_or_the_company(case):
    """The 130 members in order and in a fixed random order (another lane and panel for nearly every one), and member 77 alone"""
    c = build_moment_case(case)
    L = case[1]
    perm = np.random.default_rng(9).permutation(L)
    assert np.count_nonzero(perm != np.arange(L)) > L // 2
    with device_matrix(c) as dm:
        centre = run_moments(dm, c)["m1"].copy()
        first = run_moments(dm, c, centre)
        second = run_moments(dm, c, centre, members=perm)
        lone = run_moments(dm, c, centre, members=slice(77, 78))
    for name in first:
        assert bits(first[name][perm]) == bits(second[name]), name
        assert bits(lone[name][0]) == bits(first[name][77]), name
        assert np.all(np.isfinite(first[name])), name


@pytest.mark.parametrize("case", [(6001, 130, 8, 0, 3), (6001, 130, 8, 4, 3)], ids=moment_case_id)
def test_member_panels_do_not_change_a_bit(case):
    """Context option "scan_part_bytes" = 1: panels of 64 members, here 64 + 64 + 2; at its default: one panel."""
    c = build_moment_case(case)
    with device_matrix(c) as dm:
        centre = run_moments(dm, c)["m1"].copy()
        dm.set_option("scan_part_bytes", 1)
        cut = run_moments(dm, c, centre)
        dm.set_option("scan_part_bytes", 1 << 28)
        whole = run_moments(dm, c, centre)
    with device_matrix(c) as dm:
        default = run_moments(dm, c, centre)
    for name in cut:
        assert bits(cut[name]) == bits(whole[name]) == bits(default[name]) and np.all(np.isfinite(cut[name])), name


# ---- the method -----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def gold():
    return load_golden("scan_gradient_ho_K5.npz")


@pytest.fixture(scope="module")
def fixture_scan(gold):
    x_n, u_kn, N_k, _, _, _ = testsystems.config1(seed=0)
    basis, coeff, offset, A_qn = fixture_family(gold, x_n)
    mbar = pymbar_amd.MBAR(u_kn, N_k, relative_tolerance=1e-12)
    res = mbar.compute_scan_gradient(basis, coeff, offset, A_qn)
    yield dict(mbar=mbar, basis=basis, coeff=coeff, offset=offset, A=A_qn, res=res)
    mbar.close()


def test_fixture_reproduces_reference(fixture_scan, gold):
    check_against_fixture(fixture_scan["res"], gold)


def test_method_has_the_bits_of_compute_scan_and_members_are_independent(fixture_scan):
    s = fixture_scan
    mbar, res = s["mbar"], s["res"]
    scan = mbar.compute_scan(s["basis"], s["coeff"], s["offset"], s["A"], compute_uncertainty=False)
    assert bits(scan["f"]) == bits(res["f"]) and bits(scan["mu"]) == bits(res["mu"])
    again = mbar.compute_scan_gradient(s["basis"], s["coeff"], s["offset"], s["A"])
    arrays = [k for k in res if k not in ("params", "features")]
    for key in arrays:
        assert bits(again[key]) == bits(res[key]), key
    lone = mbar.compute_scan_gradient(s["basis"], s["coeff"][7:8], s["offset"][7:8], s["A"])
    for key in arrays:
        axis = 1 if key in ("mu", "grad_mu") else 0
        assert bits(np.take(lone[key], 0, axis=axis)) == bits(np.take(res[key], 7, axis=axis)), key
    assert np.array_equal(res["hess_f"], np.swapaxes(res["hess_f"], 1, 2))
    assert "hess_f" not in mbar.compute_scan_gradient(s["basis"], s["coeff"], s["offset"], hessian=False)


def test_sweep_across_the_seam_reproduces_reference(gold):
    fam, members = seam_family()
    m = pymbar_amd.MBAR.from_family(fam["basis"], fam["coeff"], fam["N_k"], offset_k=fam["offset"], center_kb=fam["center"],
                                    harmonic_b=fam["harmonic"], period_b=fam["period"], relative_tolerance=1e-12)
    try:
        res = m.compute_scan_gradient(A_qn=fam["basis"][0], **members)
        check_against_seam_fixture(res, gold)
        lone = m.compute_scan_gradient(A_qn=fam["basis"][0], coeff_lb=members["coeff_lb"][21:22], center_lb=members["center_lb"][21:22])
        for key in ("f", "grad_f", "hess_f", "feature_mean", "feature_cov"):
            assert bits(lone[key][0]) == bits(res[key][21]), key
    finally:
        m.close()


def test_bootstrap_replicates_are_direct_calls_and_weights_do_not_leak(gold):
    x_n, u_kn, N_k, _, _, _ = testsystems.config1(seed=0)
    basis, coeff, offset, A_qn = fixture_family(gold, x_n)
    coeff, offset = coeff[::5], offset[::5]
    L = len(coeff)
    mbar = pymbar_amd.MBAR(u_kn, N_k, n_bootstraps=3, bootstrap_rng="device", rseed=11)
    try:
        before = mbar.compute_scan(basis, coeff, offset, A_qn, compute_uncertainty=False)
        res = mbar.compute_scan_gradient(basis, coeff, offset, A_qn, uncertainty_method="bootstrap")
        P = len(res["params"])
        assert res["bootstrapped_grad_f"].shape == (3, L, P) and res["bootstrapped_hess_f"].shape == (3, L, P, P)
        assert res["bootstrapped_grad_mu"].shape == (3, len(A_qn), L, P) and res["bootstrapped_f"].shape == (3, L)
        for name in ("f", "grad_f", "hess_f", "mu", "grad_mu"):
            assert bits(res["d" + name]) == bits(np.std(res["bootstrapped_" + name], axis=0)), name
        assert np.all(res["dgrad_f"] > 0.0)
        dm = mbar._dm
        t_qn, shift = pymbar_amd.scan._shifted(np.asarray(A_qn))
        dm.set_scan(basis, t_qn)
        try:
            first = dm.scan_moments(mbar.f_k, coeff, offset, None)[2]
            for b in range(3):
                mbar._set_bootstrap_weights(dm, b)
                lognum, mean, m1, m2, ma = dm.scan_moments(mbar.f_k_boots[b], coeff, offset, first)
                want = gradient_from_moments(coeff, None, first, m1, m2, ma, mean)
                assert bits(res["bootstrapped_f"][b]) == bits(-lognum)
                assert bits(res["bootstrapped_mu"][b]) == bits(mean[:, 1:].T + shift[:, None])
                for name in ("grad_f", "hess_f", "grad_mu", "feature_mean", "feature_cov"):
                    assert bits(res["bootstrapped_" + name][b]) == bits(want[name]), (b, name)
        finally:
            dm.set_sample_weights(None)
            dm.set_scan(None)
        assert mbar._dm._wtag is None
        after = mbar.compute_scan(basis, coeff, offset, A_qn, compute_uncertainty=False)
        assert bits(after["f"]) == bits(before["f"]) and bits(after["mu"]) == bits(before["mu"])
    finally:
        mbar.close()


def test_from_family_member_with_a_states_parameters_has_that_states_expectations():
    """``from_family`` with no arguments to the method but the members: a member with a sampled state's parameters is that state, so
    ``grad_f[("coeff", b)]`` is that state's ``compute_expectations`` of the feature -- the energy for the linear term, the squared
    wrapped displacement for the harmonic one"""
    basis, coeff_k, center_k, hb, pb, offset_k, N_k = testsystems.periodic_umbrella_family(K=6, n_per_state=300, seed=0)
    m = pymbar_amd.MBAR.from_family(basis, coeff_k, N_k, offset_k=offset_k, center_kb=center_k, harmonic_b=hb, period_b=pb,
                                    relative_tolerance=1e-12)
    try:
        res = m.compute_scan_gradient(coeff_lb=coeff_k, offset_l=offset_k, center_lb=center_k)
        assert res["params"] == [("coeff", 0), ("coeff", 1), ("center", 1)]
        d = basis[1][None, :] - center_k[:, 1:2]
        d = d - pb[1] * np.rint(d / pb[1])
        for p, A_kn in ((0, np.repeat(basis[:1], 6, axis=0)), (1, d * d), (2, -2.0 * coeff_k[:, 1:2] * d)):
            want = m.compute_expectations(A_kn, state_dependent=True, compute_uncertainty=False)["mu"]
            gap = np.max(np.abs(res["grad_f"][:, p] - want) / np.maximum(np.abs(want), 1.0))
            print(res["params"][p], "max gap %.3e" % gap)
            assert gap <= SAMPLED_STATE_TOL
    finally:
        m.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------

def small(N, L=4, seed=3):
    rng = np.random.default_rng(seed)
    return dict(basis=rng.normal(0.0, 1.0, (2, N)), t=rng.uniform(0.5, 1.5, (1, N)), coeff=rng.uniform(0.0, 1.0, (L, 2)),
                offset=rng.normal(0.0, 1.0, L))


def test_a_refused_array_leaves_the_handle_answering_with_a_fresh_objects_bits():
    """The pattern of tests/test_gpu_arg_refusals.py: every array of the face one entry short and one long is refused in Python,
    a non-finite centre by the library, and the handle then returns what a fresh one returns"""
    from tests.test_gpu_arg_refusals import assert_same, refused, wrong

    K, N, L = 3, 300, 4
    u, N_k, f = random_problem(K, N, seed=31)
    s = small(N, L)
    kinds = dict(harmonic_b=np.array([False, True]), period_b=np.array([0.0, 2.5]))
    center_lb = np.stack([np.zeros(L), np.linspace(-1.0, 1.0, L)], axis=1)

    def matrix():
        dm = DeviceMatrix.from_host(u)
        dm.set_Nk(N_k)
        dm.set_scan(s["basis"], s["t"], **kinds)
        return dm

    good = dict(f=f, coeff_lb=s["coeff"], offset_l=s["offset"], center_phi=np.full((L, 3), 0.25), center_lb=center_lb)
    with matrix() as dm, matrix() as fresh:
        assert dm.scan_features() == (2, 1, 3)
        for name, axes in (("f", (0,)), ("coeff_lb", (1,)), ("offset_l", (0,)), ("center_phi", (0, 1)), ("center_lb", (0, 1))):
            for bad in wrong(good[name], axes):
                with refused(dm):
                    dm.scan_moments(**dict(good, **{name: bad}))
        for bad in (np.nan, np.inf):
            cphi = good["center_phi"].copy()
            cphi[2, 1] = bad
            with pytest.raises(ValueError, match="finite"):
                dm.scan_moments(**dict(good, center_phi=cphi))
        assert_same(dm.scan_moments(**good), fresh.scan_moments(**good), "scan_moments")


def test_contexts_the_pass_does_not_serve_are_refused():
    """More than 128 states: MBAR_ERR_STATE naming the limit; no basis: MBAR_ERR_STATE; a harmonic family without centres:
    MBAR_ERR_STATE naming the call"""
    MBAR_ERR_STATE = -4
    N, L = 300, 4
    s = small(N, L)

    def entry(owner, K, F=2):
        lognum, mean, m1, m2, ma = np.empty(L), np.empty((L, 2)), np.empty((L, F)), np.empty((L, F * (F + 1) // 2)), np.empty((L, 1, F))
        rc = owner._lib.mbar_scan_moments(owner._ctx, _dptr(np.zeros(K)), L, _dptr(s["coeff"]), _dptr(s["offset"]), None, _dptr(lognum),
                                          _dptr(mean), _dptr(m1), _dptr(m2), _dptr(ma))
        return rc, _lib.last_error(owner._ctx)

    u, N_k, _ = random_problem(129, N, seed=3)
    with DeviceMatrix.from_host(u) as wide:
        wide.set_Nk(N_k)
        rc, message = entry(wide, 129)
        assert rc == MBAR_ERR_STATE and "mbar_scan_moments" in message and "at most 128 states" in message, message
    mbar = pymbar_amd.MBAR(u, N_k, maximum_iterations=1)
    try:
        with pytest.raises(pymbar_amd.utils.ParameterError, match="at most 128 states"):
            mbar.compute_scan_gradient(s["basis"], s["coeff"], s["offset"])
    finally:
        mbar.close()
    u, N_k, _ = random_problem(5, N, seed=7)
    with DeviceMatrix.from_host(u) as base:
        base.set_Nk(N_k)
        rc, message = entry(base, 5)
        assert rc == MBAR_ERR_STATE and "mbar_ctx_set_scan first" in message, message
        base.set_scan(s["basis"], s["t"], harmonic_b=np.array([True, False]), period_b=None)
        rc, message = entry(base, 5, F=3)
        assert rc == MBAR_ERR_STATE and "mbar_scan_moments" in message and "mbar_ctx_set_scan_centers first" in message, message
