"""Differences between any two members of a scan on the MI355X (``mbar_scan_pair_gram``, k_scan_pair of mbar_k_scan.hip;
``DeviceMatrix.scan_pair_gram``; ``MBAR.compute_scan_pairs``): the members' own Gram block against the long-double stand-in
(tests/scan_pairs_standin.py) at every instantiation of the kernel and every edge of a panel, a tile and a chunk; against pass B
(``refcol``, ``within``); the bits (two calls, an entry alone and inside a call, the slab, the symmetry of the block without sample
weights); the method against the dense path on the device and against the reference's fixture (tests/golden/scan_pairs_ho_K5.npz);
the bootstrap rule; the refusals.

Tolerances are those of tests/test_gpu_scan.py for the same kinds of number: the products of pass B rtol 1e-10, f 1e-11 absolute,
Delta_f 2e-11 absolute, the uncertainties against the dense path rtol 1e-9 with atol 1e-14.  Delta_mu is a difference of two
averages each of which that file holds to rtol 1e-10 with atol 1e-11: it is held to the sum of the two bounds."""
import numpy as np
import pytest

import pymbar_amd
from pymbar_amd import _lib, testsystems
from pymbar_amd.device import DeviceMatrix, LoopbackGroup, _dptr
from pymbar_amd.utils import ParameterError
from tests.conftest import load_golden
from tests.scan_pairs_standin import build_pair_case, cen_of, load_pair_case, oracle_for, pair_case_id, pair_cases, run_pair
from tests.scan_standin import family, ladder, observables
from tests.test_gpu_arg_refusals import BASIS, COEFF, F, F_SCAN, OFFSET, assert_same, matrix, refused, wrong
from tests.test_gpu_parity import random_problem
from tests.test_scan_pairs_host import MEMBERS, check_pairs_against_fixture

pytestmark = pytest.mark.gpu


def device_matrix(case):
    dm = DeviceMatrix.from_host(case["u"])
    load_pair_case(dm, case)
    return dm


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", pair_cases(), ids=pair_case_id)
def test_pair_block_against_long_double_standin(spec):
    case = build_pair_case(spec)
    rows = case["rows"]
    with device_matrix(case) as dm:
        f_scan, got = run_pair(dm, case)
        _, again = run_pair(dm, case, f_scan=f_scan)
        passes = {int(r): dm.scan_gram_w(case["f"], case["coeff"], case["offset"], f_scan, reference=int(r), cross=False, **cen_of(case))
                  for r in (rows[0], rows[-1])}
        u_dev = dm.to_host()
    _, want = run_pair(oracle_for(case, u_dev), case, f_scan=f_scan)
    assert np.all(np.isfinite(got)) and np.all(want > 0.0)
    print("max rel error", np.max(np.abs(got - want) / want))
    np.testing.assert_allclose(got, want, rtol=1e-10, atol=0)
    assert got.tobytes() == again.tobytes()  # two identical calls: identical bits
    # row i = 0 of a reference member is the refcol pass B returns for it, its block with itself the member's within
    for at, r in ((0, int(rows[0])), (len(rows) - 1, int(rows[-1]))):
        _, within, refcol, _ = passes[r]
        np.testing.assert_allclose(got[at, :, 0, :], refcol, rtol=1e-10, atol=0)
        np.testing.assert_allclose(got[at, r], within[r], rtol=1e-10, atol=0)


BIT_CASES = [("linear", 3, 1000, 140, 5, 0, 1, 140, False), ("harmonic", 3, 1000, 70, 3, 2, 2, 70, False), ("linear", 3, 8193, 40, 2, 0, 3, 40, False)]


@pytest.mark.parametrize("spec", BIT_CASES, ids=pair_case_id)
def test_bits_do_not_depend_on_the_call(spec):
    """All pairs of a call that spans more than one member panel and more than one row panel, of both widths.  Without sample
    weights the block is symmetric to the bit: pair[r, l, i, j] and pair[l, r, j, i] are the same products with their factors in
    the other order -- this fails if the fill stage and the register path form a member's b differently.  An entry computed from
    its two members alone, or under another slab of reference members, has the bits it has inside the call."""
    case = build_pair_case(spec)
    L = spec[3]
    every = np.arange(L, dtype=np.int64)
    with device_matrix(case) as dm:
        f_scan, full = run_pair(dm, case, rows=every)
        for slab in (1, 37):
            _, cut = run_pair(dm, case, f_scan=f_scan, rows=every, slab=slab)
            assert cut.tobytes() == full.tobytes(), slab
        _, scattered = run_pair(dm, case, f_scan=f_scan)  # (the case's own rows: a shuffled subset)
        lone = []
        for r, l in ((3, L - 1), (L - 2, 0), (17, 17)):
            two = np.array([r, l])
            _, p = run_pair(dm, case, f_scan=f_scan[two], rows=np.array([0]), members=two)
            lone.append((r, l, p))
    assert np.ascontiguousarray(full.transpose(1, 0, 3, 2)).tobytes() == full.tobytes()
    assert scattered.tobytes() == np.ascontiguousarray(full[case["rows"]]).tobytes()
    for r, l, p in lone:
        assert p[0, 1].tobytes() == full[r, l].tobytes(), (r, l)
        assert p[0, 0].tobytes() == full[r, r].tobytes(), (r, l)


# ---- compute_scan_pairs against the dense path on the device ------------------------------------------------------------------------
def check_pairs_against_dense(mbar, basis, coeff, offset, A, members, method):
    res = mbar.compute_scan_pairs(basis, coeff, offset, A_qn=A, reference_members=members, uncertainty_method=method)
    rows = np.arange(len(coeff)) if members is None else members
    u_ln = coeff @ basis + offset[:, None]
    pert = mbar.compute_perturbed_free_energies(u_ln, uncertainty_method=method)
    inner = mbar.compute_expectations_inner(np.array([0]), u_ln, np.arange(len(u_ln)))
    np.testing.assert_array_equal(res["members"], rows)
    off = rows[:, None] != np.arange(len(coeff))[None, :]
    print("max |f - dense| =", np.max(np.abs(res["f"] - inner["f"])),
          " max rel dDelta_f gap =", np.max(np.abs(res["dDelta_f"][off] / pert["dDelta_f"][rows][off] - 1.0)))
    np.testing.assert_allclose(res["f"], inner["f"], rtol=0, atol=1e-11)
    np.testing.assert_allclose(res["Delta_f"], pert["Delta_f"][rows], rtol=0, atol=2e-11)
    np.testing.assert_allclose(res["dDelta_f"], pert["dDelta_f"][rows], rtol=1e-9, atol=1e-14)
    assert np.all(res["dDelta_f"][~off] == 0.0)
    for q, a in enumerate(A):
        ex = mbar.compute_expectations(a, u_kn=u_ln, state_dependent=False, output="differences", uncertainty_method=method)
        av = mbar.compute_expectations(a, u_kn=u_ln, state_dependent=False, compute_uncertainty=False)["mu"]
        print("observable", q, "max rel dDelta_mu gap =", np.max(np.abs(res["dDelta_mu"][q][off] / ex["sigma"][rows][off] - 1.0)))
        np.testing.assert_allclose(res["mu"][q], av, rtol=1e-10, atol=1e-11)
        bound = 2e-11 + 1e-10 * (np.abs(av)[None, :] + np.abs(av)[rows][:, None])
        assert np.all(np.abs(res["Delta_mu"][q] - ex["mu"][rows]) <= bound)
        np.testing.assert_allclose(res["dDelta_mu"][q], ex["sigma"][rows], rtol=1e-9, atol=1e-14)
    return res


@pytest.mark.parametrize("method", [None, "approximate"], ids=["svd-ew", "approximate"])
@pytest.mark.parametrize("shape", [(17, 4099, 33, 8, 3), (128, 6001, 40, 2, 1)], ids=lambda s: "K%d-N%d-L%d-B%d-Q%d" % s)
def test_pairs_against_dense_path(shape, method):
    K, N, L, B, Q = shape
    rng = np.random.default_rng(K)
    x_n, u_kn, N_k, O_k, K_k = ladder(K, N, seed=1)
    basis, coeff, offset = family(x_n, O_k, K_k, L, B, rng)
    mbar = pymbar_amd.MBAR(u_kn, N_k, relative_tolerance=1e-12)
    try:
        check_pairs_against_dense(mbar, basis, coeff, offset, observables(x_n, Q), None, method)
        check_pairs_against_dense(mbar, basis, coeff, offset, observables(x_n, Q), np.array([L - 1, 4, 19, 0, 11]), method)
    finally:
        mbar.close()


# ---- the reference's fixture, end to end ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture_system():
    scan = load_golden("scan_ho_K5_L300.npz")
    x_n, u_kn, N_k, _, _, _ = testsystems.config1(seed=0)
    basis, coeff, offset = testsystems.harmonic_scan_family(x_n, scan["O_l"][MEMBERS], scan["K_l"][MEMBERS])
    return dict(u_kn=u_kn, N_k=N_k, basis=basis, coeff=coeff, offset=offset, A=np.stack([x_n, x_n * x_n]))


def test_fixture_reproduces_reference(fixture_system):
    s = fixture_system
    gold = load_golden("scan_pairs_ho_K5.npz")
    mbar = pymbar_amd.MBAR(s["u_kn"], s["N_k"], relative_tolerance=1e-12)
    try:
        res = mbar.compute_scan_pairs(s["basis"], s["coeff"], s["offset"], A_qn=s["A"])
        check_pairs_against_fixture(res, gold)
        one = mbar.compute_scan(s["basis"], s["coeff"], s["offset"], A_qn=s["A"], reference=9)
        again = mbar.compute_scan_pairs(s["basis"], s["coeff"], s["offset"], A_qn=s["A"])
        rows = np.array([30, 2, 9])
        sub = mbar.compute_scan_pairs(s["basis"], s["coeff"], s["offset"], A_qn=s["A"], reference_members=rows)
    finally:
        mbar.close()
    # f and mu are compute_scan's bits; row 9 is compute_scan(reference=9)
    assert res["f"].tobytes() == one["f"].tobytes() and res["mu"].tobytes() == one["mu"].tobytes()
    assert res["Delta_f"][9].tobytes() == one["Delta_f"].tobytes()
    np.testing.assert_allclose(res["dDelta_f"][9], one["dDelta_f"], rtol=1e-9, atol=0)
    np.testing.assert_allclose(np.sqrt(res["cov_mu"][:, 9, 9]), one["sigma"][:, 9], rtol=1e-9, atol=0)
    # two identical calls: identical bits; an entry does not depend on the other reference members of the call
    for key in res:
        assert again[key].tobytes() == res[key].tobytes(), key
    for key in ("Delta_f", "cov_f", "dDelta_f"):
        assert sub[key].tobytes() == np.ascontiguousarray(res[key][rows]).tobytes(), key
    for key in ("Delta_mu", "cov_mu", "dDelta_mu"):
        assert sub[key].tobytes() == np.ascontiguousarray(res[key][:, rows]).tobytes(), key


def test_bootstrap_is_the_std_of_the_differences(fixture_system):
    s = fixture_system
    pick = np.arange(0, 43, 6)
    basis, coeff, offset, A = s["basis"], s["coeff"][pick], s["offset"][pick], s["A"]
    rows = np.array([5, 0, 2])
    mbar = pymbar_amd.MBAR(s["u_kn"], s["N_k"], n_bootstraps=3, bootstrap_rng="device", rseed=11)
    try:
        res = mbar.compute_scan_pairs(basis, coeff, offset, A_qn=A, reference_members=rows, uncertainty_method="bootstrap")
        one = mbar.compute_scan(basis, coeff, offset, A_qn=A, uncertainty_method="bootstrap")
        assert mbar._dm._wtag is None  # the multiplicities do not leak
    finally:
        mbar.close()
    fb, Ab = one["bootstrapped_f"], one["bootstrapped_observables"]
    assert res["bootstrapped_f"].tobytes() == fb.tobytes() and res["bootstrapped_observables"].tobytes() == Ab.tobytes()
    assert "cov_f" not in res and "cov_mu" not in res
    want = np.std(fb[:, None, :] - fb[:, rows][:, :, None], axis=0)
    assert res["dDelta_f"].tobytes() == want.tobytes()
    for q in range(2):
        want = np.std(Ab[:, q][:, None, :] - Ab[:, q][:, rows][:, :, None], axis=0)
        assert res["dDelta_mu"][q].tobytes() == want.tobytes()
    off = rows[:, None] != np.arange(len(pick))[None, :]
    assert np.all(res["dDelta_f"][off] > 0.0) and np.all(res["dDelta_f"][~off] == 0.0)


# ---- refusals -------------------------------------------------------------------------------------------------------------------
ROWS = np.array([1, 0])


def test_matrix_refuses_an_array_of_the_wrong_length():
    def call(dm, f=F, coeff_lb=COEFF, offset_l=OFFSET, f_scan=F_SCAN, rows=ROWS, center_lb=None):
        return dm.scan_pair_gram(f, coeff_lb, offset_l, f_scan, rows, center_lb=center_lb)

    good = dict(f=F, coeff_lb=COEFF, offset_l=OFFSET, f_scan=F_SCAN, center_lb=np.zeros_like(COEFF))
    axes = dict(f=(0,), coeff_lb=(1,), offset_l=(0,), f_scan=(0,), center_lb=(0, 1))
    with matrix() as dm, matrix() as fresh:
        for arg, ax in axes.items():
            for bad in wrong(good[arg], ax):
                with refused(dm):
                    call(dm, **{arg: bad})
        for bad in (np.array([0, 2]), np.array([-1]), np.array([], dtype=np.int64), np.array([[0, 1]]), np.array([0.0, 1.0])):
            with refused(dm):
                call(dm, rows=bad)
        assert call(dm).shape == (2, 2, 1, 1)
        assert_same(call(dm), call(fresh), "scan_pair_gram")
        # what only the library can see: a normaliser that is not a number
        for bad in (np.nan, np.inf):
            with pytest.raises(_lib.MbarHipError, match="mbar_scan_pair_gram") as err:
                call(dm, f_scan=np.array([0.2, bad]))
            assert err.value.code == _lib.MBAR_ERR_ARG
        assert_same(call(dm), call(fresh), "scan_pair_gram after the refusals")
    with DeviceMatrix.from_host(np.zeros((3, 5))) as bare:
        with pytest.raises(ValueError, match=r"no basis on this matrix \(set_scan first\)"):
            call(bare)


def test_library_refuses_bad_arguments_and_contexts():
    MBAR_ERR_STATE = -4
    L, R = 2, 2

    def entry(owner, K, rows=ROWS, R=R, f_scan=F_SCAN, pair=True):
        out = np.empty((2, L, 1, 1))
        rc = owner._lib.mbar_scan_pair_gram(owner._ctx, _dptr(np.zeros(K)), L, _dptr(COEFF), _dptr(OFFSET), _dptr(f_scan), R,
                                            _dptr(np.ascontiguousarray(rows, dtype=np.int64), _lib._ip), _dptr(out) if pair else None)
        return rc, _lib.last_error(owner._ctx)

    assert _lib.MBAR_ERR_ARG == -1
    with matrix() as dm:
        for kw in (dict(R=0), dict(rows=[0, 2]), dict(rows=[-1, 0]), dict(pair=False), dict(f_scan=np.array([np.nan, 0.0]))):
            rc, message = entry(dm, 3, **kw)
            assert rc == _lib.MBAR_ERR_ARG and "mbar_scan_pair_gram" in message, (kw, rc, message)
        with LoopbackGroup(1) as group:
            dm.set_loopback(group, 0)
            rc, message = entry(dm, 3)
            assert rc == MBAR_ERR_STATE and "mbar_scan_pair_gram" in message and "transport" in message, message
            dm.comm_destroy()
        rc, message = entry(dm, 3)
        assert rc == _lib.MBAR_OK, message
    u, N_k, _ = random_problem(129, 300, seed=3)
    with DeviceMatrix.from_host(u) as wide:
        wide.set_Nk(N_k)
        rc, message = entry(wide, 129)
        assert rc == MBAR_ERR_STATE and "mbar_scan_pair_gram" in message and "at most 128 states" in message, message


def test_method_refuses_wide_and_sharded_objects():
    u, N_k, _ = random_problem(129, 600, seed=3)
    basis = np.stack([u[0], u[1]])
    coeff = np.array([[0.5, 0.5], [0.2, 0.8], [1.0, 0.0]])
    mbar = pymbar_amd.MBAR(u, N_k, maximum_iterations=1)
    try:
        with pytest.raises(ParameterError, match="at most 128 states"):
            mbar.compute_scan_pairs(basis, coeff)
    finally:
        mbar.close()
    u, N_k, _ = random_problem(4, 600, seed=5)
    basis = np.stack([u[0], u[1]])
    mbar = pymbar_amd.MBAR(u, N_k)
    try:
        want = mbar.compute_scan_pairs(basis, coeff)
        with LoopbackGroup(2) as group:
            mbar._dm.set_loopback(group, 0)
            try:
                for call in (mbar.compute_scan_pairs, mbar.compute_scan):
                    with pytest.raises(ParameterError, match="single-rank"):
                        call(basis, coeff)
            finally:
                mbar._dm.comm_destroy()
        got = mbar.compute_scan_pairs(basis, coeff)
    finally:
        mbar.close()
    for key in want:
        assert got[key].tobytes() == want[key].tobytes(), key
