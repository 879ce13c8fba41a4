"""Kernel-density surfaces along a scan on the MI355X (``mbar_ctx_set_scan_points`` / ``mbar_scan_kde_sums``, k_scan_kde of
mbar_k_scan.hip; ``DeviceMatrix.set_scan_points`` / ``scan_kde_sums``; ``MBAR.compute_scan_kde``): the log densities against the
long-double oracle (tests/scan_kde_standin.py) at every instantiation of the kernel -- d in {1, 2}, both families, period off and on, NB
= 1, 2 and 8, three chunks with a ragged last one, past one member panel --; the reference's fixture (tests/golden/scan_kde_ho_K5.npz);
the dense path on the device; the exact path; the bits; the bootstrap rule; the resident block; the refusals.

The bound.  ``err = |L - L_ld| / max(1, |L_ld|)`` of a log density ``L`` against the long-double oracle ``L_ld``.  Its maximum over the
matrix of cases below was measured on the device and for the oracle's formulas in plain float64 numpy (profiles/scan_kde_matrix.txt:
DEVICE_MAX and the restatement's figure next to it); the tests assert 4 x the device's measured maximum, the margin
profiles/kde_instantiation_matrix.txt set for k_kde and for the same reason -- rounding differs from box to box by less than that --
and that the device is no worse than 4 x the numpy restatement on the same case."""
import numpy as np
import pytest

import pymbar_amd
from pymbar_amd import _lib, testsystems
from pymbar_amd.device import DeviceMatrix, LoopbackGroup, _dptr
from pymbar_amd.kde import log_normaliser
from pymbar_amd.utils import ParameterError
from tests.conftest import load_golden
from tests.kde_oracle import LD
from tests.scan_kde_standin import (FLAG_BELOW, KDE_ORACLE_MEMBERS, build_kde_case, cen_of, kde_case_id, kde_cases, kde_oracle_for,
                                    load_kde_case, log_density_oracle, run_kde)
from tests.test_gpu_arg_refusals import COEFF, F, F_SCAN, N, OFFSET, assert_same, extended, matrix, refused, wrong
from tests.test_gpu_parity import random_problem
from tests.test_scan_kde_host import check_1d_against_fixture, fixture_family_1d, fixture_system_2d

pytestmark = pytest.mark.gpu

DEVICE_MAX = 1.96e-14  # the device's measured maximum of err over kde_cases() (profiles/scan_kde_matrix.txt)
BOUND = 4.0 * DEVICE_MAX


def device_matrix(case):
    dm = DeviceMatrix.from_host(case["u"])
    load_kde_case(dm, case)
    return dm


def same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def rel_err(L, L_ld):
    """``|L - L_ld| / max(1, |L_ld|)``, 0 where both are the same infinity"""
    L, L_ld = np.asarray(L, dtype=np.float64), np.asarray(L_ld, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        err = np.abs(L - L_ld) / np.maximum(1.0, np.abs(L_ld))
    return np.where(L == L_ld, 0.0, err)


def log_densities(sums, d, h):
    logsum, wsum, _ = sums
    return logsum - np.log(wsum)[:, None] + log_normaliser("gaussian", d, h)


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", kde_cases(), ids=kde_case_id)
def test_log_densities_against_long_double_oracle(spec):
    case = build_kde_case(spec)
    d, L = spec[1], spec[4]
    with device_matrix(case) as dm:
        f_scan, got = run_kde(dm, case)
        _, again = run_kde(dm, case, f_scan=f_scan)
        u_dev = dm.to_host()
    pick = np.array([l for l in KDE_ORACLE_MEMBERS if l < L])
    _, want = run_kde(kde_oracle_for(case, u_dev), case, f_scan=f_scan[pick], members=pick)
    _, plain = run_kde(kde_oracle_for(case, u_dev, ordered=True), case, f_scan=f_scan[pick], members=pick)
    _, pairwise = run_kde(kde_oracle_for(case, u_dev, real=np.float64), case, f_scan=f_scan[pick], members=pick)
    assert got[0].shape == (L, case["q_dm"].shape[1]) and got[1].shape == (L,)
    assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1]))
    L_dev = log_densities(got, d, case["h"])[pick]
    L_ld, L_np = log_densities(want, d, case["h"]), log_densities(plain, d, case["h"])
    e_dev, e_np = np.max(rel_err(L_dev, L_ld)), np.max(rel_err(L_np, L_ld))
    e_pw = np.max(rel_err(log_densities(pairwise, d, case["h"]), L_ld))
    print("KDEERR %s device %.3e numpy-in-device-order %.3e numpy-pairwise %.3e n_exact %d (oracle, picked members: %d)"
          % (kde_case_id(spec), e_dev, e_np, e_pw, got[2], want[2]))
    np.testing.assert_allclose(got[1], 1.0, rtol=0, atol=1e-11)  # (f_scan normalises the members)
    np.testing.assert_allclose(got[1][pick], want[1], rtol=1e-10, atol=0)
    assert same_bits(again[0], got[0]) and same_bits(again[1], got[1]) and again[2] == got[2]  # two identical calls
    assert e_dev <= BOUND
    assert e_dev <= 4.0 * e_np
    assert got[2] == 0 and want[2] == 0  # (in range: nothing took the exact path)


BIT_CASES = [("linear", 1, 150, False, 300), ("harmonic", 2, 150, True, 300)]


@pytest.mark.parametrize("spec", BIT_CASES, ids=kde_case_id)
def test_bits_do_not_depend_on_the_call(spec):
    """L = 300 members (more than one member panel of either family) against M = 150 queries (a panel of 128 under NB = 8 and one of 22
    under NB = 2).  A member computed alone, a query computed alone (NB = 1) or at row 21 of 40 (NB = 4), the call under another slab of
    members, and ``period=None`` against zeros, have the bits they have inside the call."""
    case = build_kde_case(spec)
    L, M = spec[4], spec[2]
    q_dm = case["q_dm"]
    with device_matrix(case) as dm:
        f_scan, full = run_kde(dm, case)
        for slab in (1, 37):
            _, cut = run_kde(dm, case, f_scan=f_scan, slab=slab)
            assert same_bits(cut[0], full[0]) and same_bits(cut[1], full[1]) and cut[2] == full[2], slab
        for l in (0, 131, L - 1):
            one = np.array([l])
            _, lone = run_kde(dm, case, f_scan=f_scan[one], members=one)
            assert same_bits(lone[0][0], full[0][l]) and same_bits(lone[1][0], full[1][l]), l
        for m in (0, 77, 127, 128, M - 1):
            _, lone = run_kde(dm, case, f_scan=f_scan, q_dm=np.ascontiguousarray(q_dm[:, m:m + 1]))
            cols = np.concatenate([np.arange(21), [m], np.arange(22, 40)])  # (query m at row 21 of 40)
            _, moved = run_kde(dm, case, f_scan=f_scan, q_dm=np.ascontiguousarray(q_dm[:, cols]))
            assert same_bits(lone[0][:, 0], full[0][:, m]), (m, "alone")
            assert same_bits(moved[0][:, 21], full[0][:, m]), (m, "at another row")
            assert same_bits(lone[1], full[1]) and same_bits(moved[1], full[1])
        if case["period"] is None:
            zeros = dict(case, period=np.zeros(spec[1]))
            _, z = run_kde(dm, zeros, f_scan=f_scan)
            assert same_bits(z[0], full[0]) and same_bits(z[1], full[1])


# ---- the exact path -------------------------------------------------------------------------------------------------------------------
def exact_system(d):
    """A harmonic-oscillator ladder (K = 5, N = 3000), points x (and cos 2x for d = 2), members: two of the hull and a COLD one -- K_l =
    100 four units above the query 0.0, so that the samples near that query carry weights around e^-800"""
    x_n, u_kn, N_k, _ = testsystems.harmonic_u_kn((0, 1, 2, 3, 4), (1, 2, 4, 8, 16), [600] * 5, seed=5)
    basis, coeff, offset = testsystems.harmonic_scan_family(x_n, [1.5, 2.5, 4.0], [2.0, 3.0, 100.0])
    pts = np.stack([x_n] + ([np.cos(2.0 * x_n)] if d == 2 else []))
    return x_n, u_kn, N_k, basis, coeff, offset, pts


def member_log_weights(u_kn, N_k, f_k, u_ln):
    """``log w_ln`` of the members in long double from ``u_kn, N_k, f_k``: ``-u_l(n) - log sum_k N_k exp(f_k - u_kn)``, normalised"""
    t = np.log(np.asarray(N_k, dtype=LD))[:, None] + np.asarray(f_k, dtype=LD)[:, None] - np.asarray(u_kn, dtype=LD)
    tm = t.max(axis=0)
    logden = tm + np.log(np.sum(np.exp(t - tm[None, :]), axis=0))
    lw = -np.asarray(u_ln, dtype=LD) - logden[None, :]
    lm = lw.max(axis=1)
    return lw - (lm + np.log(np.sum(np.exp(lw - lm[:, None]), axis=1)))[:, None]


@pytest.mark.parametrize("d", [1, 2])
def test_exact_path_far_queries_and_a_cold_member(d):
    x_n, u_kn, N_k, basis, coeff, offset, pts = exact_system(d)
    h = 0.04
    lo, hi = x_n.min(), x_n.max()
    q0 = np.array([0.0, 1.0, 2.0, hi + 50 * h, hi + 1000 * h, lo - 50 * h, lo - 1000 * h])
    q_dm = np.stack([q0] + ([np.full(len(q0), 5.0)] if d == 2 else []))  # (d = 2: cos 2x <= 1, so 5.0 is 100 h from every sample)
    mbar = pymbar_amd.MBAR(u_kn, N_k)
    try:
        res = mbar.compute_scan_kde(pts.T, q_dm.T, h, basis, coeff, offset, reference_point="from-normalization")
        poisoned = mbar.f_k.copy()
        poisoned[2] = np.nan
        dm = mbar._dm
        dm.set_scan(basis, None)
        dm.set_scan_points(pts)
        nan = dm.scan_kde_sums(poisoned, coeff, offset, res["f"], q_dm, h)
        dm.set_scan_points(None)
        dm.set_scan(None)
        f_k = mbar.f_k.copy()
    finally:
        mbar.close()
    assert np.all(np.isnan(nan[0])) and np.all(np.isnan(nan[1])) and nan[2] == 0
    lw = member_log_weights(u_kn, N_k, f_k, coeff @ basis + offset[:, None])
    want, flagged = np.empty((3, len(q0))), 0
    for l in range(3):
        Lld, logsum, logtot = log_density_oracle(pts, lw[l], q_dm, h)
        want[l] = Lld.astype(np.float64)
        flagged += int(np.sum(~(np.exp(logsum - logtot) >= FLAG_BELOW)))
    err = rel_err(res["log_density"], want)
    print("exact path d=%d: n_exact %d (oracle %d), max err %.3e" % (d, res["n_exact"], flagged, np.max(err)))
    assert np.all(np.isfinite(res["log_density"])) and np.all(np.isfinite(res["f_i"]))
    assert np.max(err) <= BOUND
    assert res["n_exact"] == flagged
    # what is flagged: every member at the far queries (all of them for d = 2), and the cold member near the samples it gives no weight
    assert flagged >= (3 * len(q0) if d == 2 else 3 * 4 + 1)


def test_exact_path_takes_a_distance_whose_square_overflows():
    """Coordinates of 1e160 against a bandwidth of 1e100: r^2 is beyond the fp64 range, r^2 / 2h^2 ~ 1e120 is not"""
    x_n, u_kn, N_k, basis, coeff, offset, pts = exact_system(2)
    q_dm = np.array([[1.0e160, -3.0e159], [2.5e159, 1.0e160]])
    h = 1.0e100
    mbar = pymbar_amd.MBAR(u_kn, N_k)
    try:
        res = mbar.compute_scan_kde(pts.T, q_dm.T, h, basis, coeff[:2], offset[:2], reference_point="from-normalization")
        f_k = mbar.f_k.copy()
    finally:
        mbar.close()
    lw = member_log_weights(u_kn, N_k, f_k, coeff[:2] @ basis + offset[:2, None])
    want = np.stack([log_density_oracle(pts, lw[l], q_dm, h)[0].astype(np.float64) for l in range(2)])
    print("overflowing r^2: L =", res["log_density"].ravel(), " max err %.3e" % np.max(rel_err(res["log_density"], want)))
    assert res["n_exact"] == 4 and np.all(np.isfinite(res["log_density"])) and np.all(res["log_density"] < -1.0e119)
    assert np.max(rel_err(res["log_density"], want)) <= BOUND


# ---- the method: the reference's fixture, the dense path, a centre family over the seam ------------------------------------------
def test_fixture_reproduces_reference():
    gold = load_golden("scan_kde_ho_K5.npz")
    x_n, u_kn, N_k, _, _, _ = testsystems.config1(seed=0)
    basis, coeff, offset = fixture_family_1d(gold, x_n)
    mbar = pymbar_amd.MBAR(u_kn, N_k, relative_tolerance=1e-12)
    try:
        lo = check_1d_against_fixture(mbar, gold, basis, coeff, offset, x_n)
        scan = mbar.compute_scan(basis, coeff, offset)
    finally:
        mbar.close()
    assert same_bits(lo["f"], scan["f"])
    s = fixture_system_2d(gold)
    mbar = pymbar_amd.MBAR.from_linear(s["basis"], s["coeff_k"], s["N_k"], offset_k=s["offset_k"], relative_tolerance=1e-12)
    try:
        res = mbar.compute_scan_kde(s["x_n"], s["queries"], s["h"], coeff_lb=s["coeff"], offset_l=s["offset"], reference_point="from-specified",
                                    fes_reference=[0.0, 0.0])
        scan = mbar.compute_scan(coeff_lb=s["coeff"], offset_l=s["offset"])
        f_k = mbar.f_k.copy()
    finally:
        mbar.close()
    np.testing.assert_allclose(f_k, gold["b_f_k"], atol=1e-9)
    exact = gold["b_exact_L"]
    err = rel_err(res["log_density"], exact[:, :-1])
    print("2-D fixture: max err against the stored exact log densities %.3e" % np.max(err))
    assert np.max(err) <= BOUND
    np.testing.assert_allclose(res["f_i"], -exact[:, :-1] + exact[:, -1:], rtol=1e-9, atol=1e-9)
    # a member with a sampled state's parameters: compute_scan's bits, and that state's free energy
    assert same_bits(res["f"], scan["f"])
    np.testing.assert_allclose(res["f"][len(gold["b_betas"]):], f_k[gold["b_sampled"]], rtol=0, atol=1e-10)


def test_method_against_the_dense_path_and_the_oracle():
    """A few members against ``pymbar_amd.FES(...).generate_fes(u_n=u_l, fes_type="kde")`` on the device, and against the oracle fed with
    long-double weights from ``u_kn, N_k, f_k``"""
    s = fixture_system_2d(load_golden("scan_kde_ho_K5.npz"))
    u_kn = s["coeff_k"] @ s["basis"] + s["offset_k"][:, None]
    pick = np.array([0, 2, 6])
    coeff, offset = s["coeff"][pick], s["offset"][pick]
    q = s["queries"][::3]
    mbar = pymbar_amd.MBAR(u_kn, s["N_k"])
    try:
        res = mbar.compute_scan_kde(s["x_n"], q, s["h"], s["basis"], coeff, offset, reference_point="from-normalization")
        f_k = mbar.f_k.copy()
    finally:
        mbar.close()
    fes = pymbar_amd.FES(u_kn, s["N_k"])
    dense = []
    try:
        for l in range(len(pick)):
            fes.generate_fes(coeff[l] @ s["basis"] + offset[l], s["x_n"], fes_type="kde", kde_parameters={"bandwidth": s["h"]})
            dense.append(-fes.get_fes(q, reference_point="from-normalization")["f_i"])
    finally:
        fes.kde.close()
        fes.mbar.close()
    lw = member_log_weights(u_kn, s["N_k"], f_k, coeff @ s["basis"] + offset[:, None])
    want = np.stack([log_density_oracle(s["x_n"].T, lw[l], q.T, s["h"])[0].astype(np.float64) for l in range(len(pick))])
    e_dense, e_ld = np.max(rel_err(res["log_density"], np.array(dense))), np.max(rel_err(res["log_density"], want))
    print("dense path: max err %.3e; oracle: %.3e" % (e_dense, e_ld))
    assert e_ld <= BOUND and e_dense <= BOUND
    assert res["n_exact"] == 0


def test_centre_family_over_the_seam():
    """``periodic_umbrella_family``: a sweep of the restraint centre across +-180 with ``period`` on, d = 1 (the torsion) and d = 2 (the
    torsion and its energy); one member has a sampled state's parameters"""
    basis, coeff_kb, center_kb, harmonic_b, period_b, offset_k, N_k = testsystems.periodic_umbrella_family(K=6, n_per_state=400, seed=2)
    chi0 = np.array([150.0, 170.0, 180.0, -170.0, center_kb[5, 1]])
    coeff = np.tile(coeff_kb[5], (len(chi0), 1))
    center = np.stack([np.zeros(len(chi0)), chi0], axis=1)
    u_kn = testsystems.family_u_kn(basis, coeff_kb, offset_k, center_kb, harmonic_b, period_b)
    u_ln = testsystems.family_u_kn(basis, coeff, None, center, harmonic_b, period_b)
    q1 = np.array([-180.0, 180.0, -179.5, 179.5, 120.0, 0.0])
    mbar = pymbar_amd.MBAR.from_family(basis, coeff_kb, N_k, offset_k=offset_k, center_kb=center_kb, harmonic_b=harmonic_b, period_b=period_b)
    try:
        f_k = mbar.f_k.copy()
        for d, h in ((1, 4.0), (2, 0.5)):
            pts = np.stack([basis[1], basis[0]][:d])
            e1 = np.linspace(0.2, 2.8, len(q1))
            e1[1] = e1[0]  # (the queries at -180 and +180 are one point)
            q_dm = np.stack([q1, e1][:d])
            period = np.array([360.0, 0.0])[:d]
            if d == 2:  # (one bandwidth for both coordinates: the torsion in units of 8 degrees)
                pts, q_dm, period = pts * np.array([[1 / 8.0], [1.0]]), q_dm * np.array([[1 / 8.0], [1.0]]), period / 8.0
            res = mbar.compute_scan_kde(pts.T, q_dm.T, h, coeff_lb=coeff, center_lb=center, period=period, reference_point="from-normalization")
            scan = mbar.compute_scan(coeff_lb=coeff, center_lb=center)
            lw = member_log_weights(u_kn, N_k, f_k, u_ln)
            want = np.stack([log_density_oracle(pts, lw[l], q_dm, h, period)[0].astype(np.float64) for l in range(len(chi0))])
            err = np.max(rel_err(res["log_density"], want))
            print("seam d=%d: max err %.3e" % (d, err))
            assert err <= BOUND
            assert same_bits(res["f"], scan["f"]) and res["n_exact"] == 0
            np.testing.assert_allclose(res["f"][4], f_k[5], rtol=0, atol=1e-10)  # the sampled state's parameters: that state
            np.testing.assert_allclose(res["log_density"][:, 0], res["log_density"][:, 1], rtol=1e-11, atol=1e-11)  # -180 is +180
    finally:
        mbar.close()


# ---- the bootstrap rule; the resident block ------------------------------------------------------------------------------------------
def test_bootstrap_replicates_against_the_oracle_and_the_weights_are_restored():
    gold = load_golden("scan_kde_ho_K5.npz")
    x_n, u_kn, N_k, _, _, _ = testsystems.config1(seed=0)
    basis, coeff, offset = fixture_family_1d(gold, x_n)
    pick = np.array([0, 7, 11])
    coeff, offset = coeff[pick], offset[pick]
    q = gold["a_queries"][6:34:3]
    mbar = pymbar_amd.MBAR(u_kn, N_k, n_bootstraps=4, rseed=11)
    try:
        before = mbar.compute_scan(basis, coeff, offset)
        res = mbar.compute_scan_kde(x_n, q, 0.2, basis, coeff, offset, uncertainty_method="bootstrap")
        assert mbar._dm._wtag is None and mbar._dm._scan is None and mbar._dm._scan_pts == 0  # nothing leaks
        after = mbar.compute_scan(basis, coeff, offset)
        rows = [np.bincount(mbar._bootstrap_row(b), minlength=len(x_n)) for b in range(4)]
        f_boots = mbar.f_k_boots.copy()
    finally:
        mbar.close()
    for key in before:
        assert same_bits(before[key], after[key]), key
    Lb = res["bootstrapped_log_density"]
    assert Lb.shape == (4, 3, len(q)) and res["df_i"].shape == (3, len(q))
    u_ln = coeff @ basis + offset[:, None]
    for b in range(4):
        with np.errstate(divide="ignore"):
            lw = member_log_weights(u_kn, N_k, f_boots[b], u_ln) + np.log(rows[b].astype(LD))[None, :]
        want = np.stack([log_density_oracle(x_n[None, :], lw[l], q[None, :], 0.2)[0].astype(np.float64) for l in range(3)])
        err = np.max(rel_err(Lb[b], want))
        print("replicate %d: max err %.3e" % (b, err))
        assert err <= BOUND
    r = np.arange(3)
    want_df = np.std(-Lb + Lb[:, r, res["reference"]][:, :, None], axis=0)
    np.testing.assert_allclose(res["df_i"], want_df, rtol=1e-13, atol=1e-15)
    assert np.sum(res["df_i"] > 0.0) == res["df_i"].size - 3


def test_points_stay_resident_across_the_other_scan_methods():
    gold = load_golden("scan_kde_ho_K5.npz")
    x_n, u_kn, N_k, _, _, _ = testsystems.config1(seed=0)
    basis, coeff, offset = fixture_family_1d(gold, x_n)
    q_dm = gold["a_queries"][None, 5:30]
    mbar = pymbar_amd.MBAR(u_kn, N_k)
    try:
        dm = mbar._dm
        dm.set_scan_points(x_n[None, :])
        dm.set_scan(basis, None)
        f_scan = -dm.scan_lognum(mbar.f_k, coeff, offset)[0]
        first = dm.scan_kde_sums(mbar.f_k, coeff, offset, f_scan, q_dm, 0.2)
        dm.set_scan(None)
        mbar.compute_scan(basis, coeff, offset, A_qn=x_n)
        mbar.compute_scan_expectations(np.stack([x_n, x_n * x_n]), basis, coeff, offset)
        dm.set_scan(basis, None)
        kept = dm.scan_kde_sums(mbar.f_k, coeff, offset, f_scan, q_dm, 0.2)
        dm.set_scan_points(None)
        with pytest.raises(ValueError, match="no points"):
            dm.scan_kde_sums(mbar.f_k, coeff, offset, f_scan, q_dm, 0.2)
        dm.set_scan(None)
    finally:
        mbar.close()
    assert_same(kept, first, "scan_kde_sums after other scan methods")


# ---- refusals -------------------------------------------------------------------------------------------------------------------
X_DN = np.random.default_rng(6).normal(size=(2, N))
Q_DM = np.array([[0.1, -0.4, 0.9], [0.0, 0.3, -0.2]])


def kde_matrix():
    dm = matrix()
    dm.set_scan_points(X_DN)
    return dm


def test_matrix_refuses_an_array_of_the_wrong_length():
    def call(dm, f=F, coeff_lb=COEFF, offset_l=OFFSET, f_scan=F_SCAN, queries_dm=Q_DM, period=None, center_lb=None):
        return dm.scan_kde_sums(f, coeff_lb, offset_l, f_scan, queries_dm, 0.7, period=period, center_lb=center_lb)

    good = dict(f=F, coeff_lb=COEFF, offset_l=OFFSET, f_scan=F_SCAN, queries_dm=Q_DM, period=np.zeros(2), center_lb=np.zeros_like(COEFF))
    axes = dict(f=(0,), coeff_lb=(1,), offset_l=(0,), f_scan=(0,), queries_dm=(0,), period=(0,), center_lb=(0, 1))
    with kde_matrix() as dm, kde_matrix() as fresh:
        for arg, ax in axes.items():
            for bad in wrong(good[arg], ax):
                with refused(dm):
                    call(dm, **{arg: bad})
        with refused(dm):
            call(dm, queries_dm=Q_DM[:, :0])
        for bad in list(wrong(X_DN, (1,))) + [X_DN[:0], X_DN[0], X_DN[None], np.vstack([X_DN, X_DN[:1]])]:
            with refused(dm):
                dm.set_scan_points(bad)
        got = call(dm)
        assert [np.shape(a) for a in got] == [(2, 3), (2,), ()]
        assert_same(got, call(fresh), "scan_kde_sums")
        # what only the library can see: an entry that is not a number, a bandwidth or a period out of range; the block stays
        for bad in (np.nan, np.inf):
            poisoned = X_DN.copy()
            poisoned[1, 3] = bad
            with pytest.raises(ValueError, match="mbar_ctx_set_scan_points"):
                dm.set_scan_points(poisoned)
            poisoned = Q_DM.copy()
            poisoned[0, 1] = bad
            with pytest.raises(ValueError, match="mbar_scan_kde_sums"):
                call(dm, queries_dm=poisoned)
            with pytest.raises(ValueError, match="mbar_scan_kde_sums"):
                call(dm, period=np.array([bad, 0.0]))
        with pytest.raises(ValueError, match="mbar_scan_kde_sums"):
            call(dm, period=np.array([-1.0, 0.0]))
        for h in (0.0, -1.0, np.nan, np.inf, 1e-170, 1e170):
            with pytest.raises(ValueError, match="mbar_scan_kde_sums"):
                dm.scan_kde_sums(F, COEFF, OFFSET, F_SCAN, Q_DM, h)
        assert_same(call(dm), call(fresh), "scan_kde_sums after the refusals")
        assert_same(call(dm, period=np.zeros(2)), call(fresh), "period zeros against None")
        dm.set_scan_points(None)
        with refused(dm):  # (no points: refused before the library is called)
            call(dm)
        dm.set_scan_points(X_DN)
        assert_same(call(dm), call(fresh), "scan_kde_sums after a release")
        dm.set_scan_points(X_DN[:1])
        with refused(dm):  # (the queries of another dimension)
            call(dm)
    with DeviceMatrix.from_host(np.zeros((3, 5))) as bare:
        bare.set_scan_points(X_DN)  # (the block does not need a basis)
        with pytest.raises(ValueError, match=r"no basis on this matrix \(set_scan first\)"):
            call(bare)


def test_library_refuses_bad_arguments_and_contexts():
    MBAR_ERR_STATE = -4
    L, M = 2, 3

    def sums(owner, K, logsum=True, wsum=True, n_exact=True, q=True, L=L, M=M):
        import ctypes as C

        out = lambda on, shape: _dptr(np.empty(shape)) if on else None
        ne = C.c_int64(0)
        rc = owner._lib.mbar_scan_kde_sums(owner._ctx, _dptr(np.zeros(K)), L, _dptr(COEFF), _dptr(OFFSET), _dptr(F_SCAN), M,
                                           _dptr(Q_DM) if q else None, 0.7, None, out(logsum, (L, 3)), out(wsum, L),
                                           C.byref(ne) if n_exact else None)
        return rc, _lib.last_error(owner._ctx)

    def upload(owner, d=2, x=X_DN, ld=N):
        rc = owner._lib.mbar_ctx_set_scan_points(owner._ctx, d, None if x is None else _dptr(np.ascontiguousarray(x)), ld)
        return rc, _lib.last_error(owner._ctx)

    with matrix() as dm:
        rc, message = sums(dm, 3)
        assert rc == MBAR_ERR_STATE and "mbar_scan_kde_sums" in message and "no points" in message, message
        for kw in (dict(d=-1), dict(d=3), dict(x=None), dict(ld=N - 1)):
            rc, message = upload(dm, **kw)
            assert rc == _lib.MBAR_ERR_ARG and "mbar_ctx_set_scan_points" in message, (kw, rc, message)
        assert upload(dm)[0] == _lib.MBAR_OK
        for kw in (dict(logsum=False), dict(wsum=False), dict(n_exact=False), dict(q=False), dict(L=0), dict(M=0)):
            rc, message = sums(dm, 3, **kw)
            assert rc == _lib.MBAR_ERR_ARG and "mbar_scan_kde_sums" in message, (kw, rc, message)
        # a refused upload leaves the block: the sums are a fresh object's
        dm._scan_pts = 2
        assert upload(dm, d=3)[0] == _lib.MBAR_ERR_ARG
        with kde_matrix() as fresh:
            want = fresh.scan_kde_sums(F, COEFF, OFFSET, F_SCAN, Q_DM, 0.7)
            assert_same(dm.scan_kde_sums(F, COEFF, OFFSET, F_SCAN, Q_DM, 0.7), want, "after a refused upload")
            with LoopbackGroup(1) as group:
                dm.set_loopback(group, 0)
                for rc, message in (sums(dm, 3), upload(dm)):
                    assert rc == MBAR_ERR_STATE and "mbar_" in message and "transport" in message, message
                dm.comm_destroy()
            assert sums(dm, 3)[0] == _lib.MBAR_OK
            # a pitch wider than N: the rows are taken at the pitch
            wide_rows = np.hstack([X_DN, np.full((2, 3), np.nan)])
            assert upload(dm, x=wide_rows, ld=N + 3)[0] == _lib.MBAR_OK
            assert_same(dm.scan_kde_sums(F, COEFF, OFFSET, F_SCAN, Q_DM, 0.7), want, "rows at a pitch")
        # a NaN among the free energies or the normalisers: NaN outputs, MBAR_OK
        logsum, wsum, n_exact = dm.scan_kde_sums(F, COEFF, OFFSET, np.array([0.2, np.nan]), Q_DM, 0.7)
        assert np.all(np.isnan(logsum)) and np.all(np.isnan(wsum)) and n_exact == 0
    u, N_k, _ = random_problem(129, 300, seed=3)
    with DeviceMatrix.from_host(u) as wide:
        wide.set_Nk(N_k)
        for rc, message in (sums(wide, 129), upload(wide, x=np.zeros((2, 300)), ld=300)):
            assert rc == MBAR_ERR_STATE and "at most 128 states" in message, message
    with extended() as ext:
        for rc, message in (sums(ext, 3), upload(ext)):
            assert rc == MBAR_ERR_STATE and "extension context" in message, message


def test_method_refuses_wide_and_sharded_objects():
    u, N_k, _ = random_problem(129, 600, seed=3)
    basis = np.stack([u[0], u[1]])
    coeff = np.array([[0.5, 0.5], [0.2, 0.8], [1.0, 0.0]])
    mbar = pymbar_amd.MBAR(u, N_k, maximum_iterations=1)
    try:
        with pytest.raises(ParameterError, match="at most 128 states"):
            mbar.compute_scan_kde(u[2], u[2][:4], 0.3, basis, coeff)
    finally:
        mbar.close()
    u, N_k, _ = random_problem(4, 600, seed=5)
    basis = np.stack([u[0], u[1]])
    mbar = pymbar_amd.MBAR(u, N_k)
    try:
        want = mbar.compute_scan_kde(u[2], u[2][:4], 0.3, basis, coeff)
        with LoopbackGroup(2) as group:
            mbar._dm.set_loopback(group, 0)
            try:
                with pytest.raises(ParameterError, match="single-rank"):
                    mbar.compute_scan_kde(u[2], u[2][:4], 0.3, basis, coeff)
            finally:
                mbar._dm.comm_destroy()
        got = mbar.compute_scan_kde(u[2], u[2][:4], 0.3, basis, coeff)
    finally:
        mbar.close()
    for key in want:
        assert same_bits(got[key], want[key]), key
