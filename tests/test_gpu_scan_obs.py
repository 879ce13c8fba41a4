"""Many observables along a scan on the MI355X (``mbar_ctx_set_scan_obs`` / ``mbar_scan_obs_sums``, k_scan_obs of mbar_k_scan.hip;
``DeviceMatrix.set_scan_observables`` / ``scan_obs_sums``; ``MBAR.compute_scan_expectations``): the sums against the long-double
stand-in (tests/scan_obs_standin.py) at every instantiation of the kernel and every edge of a panel, a tile and a chunk; the bits
(two calls, a member alone and inside a call, an observable alone, inside a block and at another row, the slab, with and without the
second moments); against pass A and pass B; the method against the dense path on the device and against the reference's fixture
(tests/golden/scan_observables_ho_K5.npz); the bootstrap rule; the resident block; the refusals.

Bounds.  The positive sums (t2, wsum, w2sum) rtol 1e-10, the project's for the products of pass B (tests/test_gpu_scan.py).  The signed
sums (s1, t1) cancel, so they are held to 1e-10 of the sum of the magnitudes of their terms, ``sum c b^P |a_q|`` from the stand-in.
Against the dense path mu is held to rtol 1e-10 with atol 1e-11 as the averages of that file, and the variance to 1e-9 of the sum of
the magnitudes of the three terms it is expanded into, ``t2 + 2 |m t1| + m^2 w2sum``: the dense path's tolerance for an uncertainty
(rtol 1e-9) applied to what the expansion can lose."""
import numpy as np
import pytest

import pymbar_amd
from pymbar_amd import _lib, scan as scan_module, testsystems
from pymbar_amd.device import DeviceMatrix, LoopbackGroup, _dptr
from pymbar_amd.utils import ParameterError
from tests.conftest import load_golden
from tests.scan_obs_standin import build_obs_case, cen_of, load_obs_case, obs_case_id, obs_cases, obs_oracle_for, obs_rows, run_obs
from tests.scan_standin import family, ladder
from tests.test_gpu_arg_refusals import BASIS, COEFF, F, F_SCAN, N, OFFSET, assert_same, extended, matrix, refused, wrong
from tests.test_gpu_parity import random_problem
from tests.test_scan_obs_host import check_expectations_against_fixture, fixture_family, fixture_observables

pytestmark = pytest.mark.gpu

NAMES = ("s1", "t1", "t2", "wsum", "w2sum")


def device_matrix(case):
    dm = DeviceMatrix.from_host(case["u"])
    load_obs_case(dm, case)
    return dm


def same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


# ---- the kernel ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", obs_cases(), ids=obs_case_id)
def test_sums_against_long_double_standin(spec):
    case = build_obs_case(spec)
    with device_matrix(case) as dm:
        f_scan, got = run_obs(dm, case)
        _, again = run_obs(dm, case, f_scan=f_scan)
        _, first = run_obs(dm, case, f_scan=f_scan, second=False)
        u_dev = dm.to_host()
    oracle = obs_oracle_for(case, u_dev)
    _, want = run_obs(oracle, case, f_scan=f_scan)
    abs1, abs2 = oracle.scan_obs_abs_sums(case["f"], case["coeff"], case["offset"], f_scan, **cen_of(case))
    got, want = dict(zip(NAMES, got)), dict(zip(NAMES, want))
    for name in NAMES:
        assert got[name].shape == want[name].shape and np.all(np.isfinite(got[name])), name
    for name in ("t2", "wsum", "w2sum"):
        live = want[name] > 0.0
        print(name, "max rel error", np.max(np.abs(got[name][live] - want[name][live]) / want[name][live]) if np.any(live) else 0.0)
        np.testing.assert_allclose(got[name], want[name], rtol=1e-10, atol=0)
    for name, scale in (("s1", abs1), ("t1", abs2)):
        live = scale > 0.0
        print(name, "worst |error| / sum of magnitudes", np.max(np.abs(got[name] - want[name])[live] / scale[live]) if np.any(live) else 0.0)
        assert np.all(np.abs(got[name] - want[name]) <= 1e-10 * scale), name
    np.testing.assert_allclose(got["wsum"], 1.0, rtol=0, atol=1e-11)  # (f_scan normalises the members)
    for a, b in zip(again, got.values()):  # two identical calls: identical bits
        assert same_bits(a, b)
    # the first moments alone: the bits they have next to the second moments
    assert same_bits(first[0], got["s1"]) and same_bits(first[3], got["wsum"]) and first[1] is None and first[2] is None and first[4] is None


BIT_CASES = [("linear", 9, 1000, 300, 5, 0, 200, False), ("harmonic", 9, 1000, 300, 3, 2, 200, False), ("linear", 9, 8193, 300, 2, 0, 200, True)]


@pytest.mark.parametrize("spec", BIT_CASES, ids=obs_case_id)
def test_bits_do_not_depend_on_the_call(spec):
    """L = 300 members (more than one member panel under either number of operand columns) against Q = 200 observables (a panel of
    128 under NB = 8 and one of 72 under NB = 8 with blocks of padding).  A member computed alone, an observable computed alone (NB =
    1) or at another row of another block (among 40 rows: NB = 4), and the call under another slab of members, have the bits they have
    inside the call."""
    case = build_obs_case(spec)
    L, Q = spec[3], spec[6]
    with device_matrix(case) as dm:
        f_scan, full = run_obs(dm, case)
        for slab in (1, 37):
            _, cut = run_obs(dm, case, f_scan=f_scan, slab=slab)
            for name, a, b in zip(NAMES, cut, full):
                assert same_bits(a, b), (slab, name)
        for l in (0, 131, L - 1):
            one = np.array([l])
            _, lone = run_obs(dm, case, f_scan=f_scan[one], members=one)
            for name, a, b in zip(NAMES, lone, full):
                assert same_bits(a[0], b[l]), (l, name)
        for q in (0, 77, 127, 128, Q - 1):
            dm.set_scan_observables(case["a"][q:q + 1])
            _, lone = run_obs(dm, case, f_scan=f_scan)
            rows = np.concatenate([np.arange(21), [q], np.arange(22, 40)])  # (row q of the block at row 21 of 40)
            dm.set_scan_observables(case["a"][rows])
            _, moved = run_obs(dm, case, f_scan=f_scan)
            for i, name in enumerate(NAMES[:3]):
                assert same_bits(lone[i][:, 0], full[i][:, q]), (q, name, "alone")
                assert same_bits(moved[i][:, 21], full[i][:, q]), (q, name, "at another row")
            assert same_bits(lone[3], full[3]) and same_bits(lone[4], full[4]) and same_bits(moved[3], full[3])


@pytest.mark.parametrize("spec", [("linear", 9, 1000, 150, 5, 0, 3, True), ("harmonic", 9, 1000, 70, 3, 2, 2, True),
                                  ("linear", 128, 8193, 40, 2, 0, 1, False)], ids=obs_case_id)
def test_sums_agree_with_pass_a_and_pass_b(spec):
    """s1 against pass A's ``mean`` of the same stored rows; w2sum and wsum against ``within[:, 0, 0]`` and ``wsum`` of pass B"""
    case = build_obs_case(spec)
    cen = cen_of(case)
    with device_matrix(case) as dm:
        f_scan, (s1, _, _, wsum, w2sum) = run_obs(dm, case)
        kinds = {} if case["family"] == "linear" else dict(harmonic_b=case["harmonic_b"], period_b=case["period_b"])
        dm.set_scan(case["basis"], case["a"], **kinds)  # (the same rows as the scan's own observables; the resident block stays)
        lognum, mean = dm.scan_lognum(case["f"], case["coeff"], case["offset"], **cen)
        _, within, _, w = dm.scan_gram_w(case["f"], case["coeff"], case["offset"], f_scan, cross=False, **cen)
        dm.set_scan(case["basis"], None, **kinds)
        _, after = run_obs(dm, case, f_scan=f_scan)
    assert same_bits(-lognum, f_scan)
    np.testing.assert_allclose(s1, mean[:, 1:], rtol=1e-10, atol=1e-11)
    np.testing.assert_allclose(w2sum, within[:, 0, 0], rtol=1e-10, atol=0)
    np.testing.assert_allclose(wsum, w, rtol=1e-10, atol=0)
    assert same_bits(after[0], s1)  # the block survived a change of basis


# ---- compute_scan_expectations against the dense path on the device -----------------------------------------------------------------
def dense_observables(x_n, Q):
    """Q observables the dense path takes (its shift needs a row that is not constant): x, x^2, a small fluctuation on a large
    offset, then oscillations of growing frequency"""
    y = (x_n - x_n.mean()) / x_n.std()
    return np.stack([x_n, x_n * x_n, 1000.0 + x_n][:Q] + [np.cos((1.0 + 0.37 * q) * y) for q in range(3, Q)])


@pytest.mark.parametrize("shape", [(17, 4099, 33, 8, 20), (128, 6001, 40, 2, 5)], ids=lambda s: "K%d-N%d-L%d-B%d-Q%d" % s)
def test_expectations_against_dense_path(shape):
    K, N_, L, B, Q = shape
    rng = np.random.default_rng(K)
    x_n, u_kn, N_k, O_k, K_k = ladder(K, N_, seed=1)
    basis, coeff, offset = family(x_n, O_k, K_k, L, B, rng)
    A = dense_observables(x_n, Q)
    u_ln = coeff @ basis + offset[:, None]
    mbar = pymbar_amd.MBAR(u_kn, N_k, relative_tolerance=1e-12)
    try:
        res = mbar.compute_scan_expectations(A, basis, coeff, offset)
        one = mbar.compute_scan(basis, coeff, offset, compute_uncertainty=False)
        means = mbar.compute_scan_expectations(A, basis, coeff, offset, compute_uncertainty=False)
        dense = [mbar.compute_expectations(a, u_kn=u_ln, state_dependent=False, uncertainty_method="approximate") for a in A]
        logden = mbar._dm.logden(mbar.f_k)
    finally:
        mbar.close()
    assert same_bits(res["f"], one["f"]) and same_bits(means["mu"], res["mu"]) and "sigma" not in means
    np.testing.assert_allclose(means["n_eff"], res["n_eff"], rtol=1e-10, atol=0)
    # the magnitudes of the three terms of the expansion, from the dense weights
    w = np.exp(res["f"][:, None] - u_ln - logden[None, :])
    w2 = w * w
    a = A - (A.sum(axis=1) / A.shape[1])[:, None]
    for q in range(Q):
        m = w @ a[q]
        scale = w2 @ (a[q] * a[q]) + 2.0 * np.abs(m * (w2 @ a[q])) + m * m * w2.sum(axis=1)
        dvar = np.abs(res["sigma"][q] ** 2 - dense[q]["sigma"] ** 2)
        print("observable", q, "max |mu - dense| =", np.max(np.abs(res["mu"][q] - dense[q]["mu"])), " worst |dvar| / scale =", np.max(dvar / scale))
        np.testing.assert_allclose(res["mu"][q], dense[q]["mu"], rtol=1e-10, atol=1e-11)
        assert np.all(dvar <= 1e-9 * scale), q
    np.testing.assert_allclose(res["n_eff"], 1.0 / w2.sum(axis=1), rtol=1e-10, atol=0)


# ---- the reference's fixture, end to end; the resident block; the bootstrap rule ----------------------------------------------------
@pytest.fixture(scope="module")
def fixture_system():
    gold = load_golden("scan_observables_ho_K5.npz")
    x_n, u_kn, N_k, _, _, _ = testsystems.config1(seed=0)
    basis, coeff, offset = fixture_family(gold, x_n)
    return dict(gold=gold, u_kn=u_kn, N_k=N_k, basis=basis, coeff=coeff, offset=offset, A=fixture_observables(x_n))


def test_fixture_reproduces_reference_and_the_observables_stay_resident(fixture_system):
    s = fixture_system
    basis, coeff, offset, A = s["basis"], s["coeff"], s["offset"], s["A"]
    mbar = pymbar_amd.MBAR(s["u_kn"], s["N_k"], relative_tolerance=1e-12)
    try:
        res = mbar.compute_scan_expectations(A, basis, coeff, offset)
        mbar.set_scan_observables(A)
        kept = mbar.compute_scan_expectations(None, basis, coeff, offset)
        scan = mbar.compute_scan(basis, coeff, offset, A_qn=A[:2])  # (another scan method, with observables of its own, in between)
        other = mbar.compute_scan_expectations(basis_bn=basis, coeff_lb=coeff[::-1] * 1.01, offset_l=offset[::-1])
        back = mbar.compute_scan_expectations(basis_bn=basis, coeff_lb=coeff, offset_l=offset)
        with pytest.raises(ParameterError, match="resident"):
            mbar.compute_scan_expectations(A[:2], basis, coeff, offset)
        mbar.set_scan_observables(None)
        with pytest.raises(ParameterError, match="none are set"):
            mbar.compute_scan_expectations(None, basis, coeff, offset)
    finally:
        mbar.close()
    check_expectations_against_fixture(res, s["gold"])
    assert same_bits(res["f"], scan["f"])
    np.testing.assert_allclose(res["mu"][:2], scan["mu"], rtol=1e-10, atol=1e-11)
    assert not np.allclose(other["mu"][:, ::-1], res["mu"], rtol=1e-6, atol=0)  # (other members: other numbers)
    for key in res:
        assert same_bits(kept[key], res[key]) and same_bits(back[key], res[key]), key


def test_bootstrap_is_the_std_of_the_replicates(fixture_system):
    s = fixture_system
    pick = np.array([0, 7, 23])
    basis, coeff, offset, A = s["basis"], s["coeff"][pick], s["offset"][pick], s["A"]
    mbar = pymbar_amd.MBAR(s["u_kn"], s["N_k"], n_bootstraps=3, bootstrap_rng="device", rseed=11)
    try:
        res = mbar.compute_scan_expectations(A, basis, coeff, offset, uncertainty_method="bootstrap")
        assert mbar._dm._wtag is None and mbar._dm._scan is None and mbar._dm._scan_obs == 0  # nothing leaks
        one = mbar.compute_scan(basis, coeff, offset, uncertainty_method="bootstrap")
        # the replicates, one by one
        dm = mbar._dm
        a_qn, shift = scan_module._centred_observables(mbar, A)
        dm.set_scan(basis, None)
        dm.set_scan_observables(a_qn)
        Ab = np.zeros((3, len(A), len(pick)))
        try:
            for b in range(3):
                mbar._set_bootstrap_weights(dm, b)
                f_b = -dm.scan_lognum(mbar.f_k_boots[b], coeff, offset)[0]
                Ab[b] = dm.scan_obs_sums(mbar.f_k_boots[b], coeff, offset, f_b)[0].T + shift[:, None]
        finally:
            dm.set_sample_weights(None)
            dm.set_scan_observables(None)
            dm.set_scan(None)
    finally:
        mbar.close()
    assert same_bits(res["bootstrapped_f"], one["bootstrapped_f"])
    assert same_bits(res["bootstrapped_observables"], Ab)
    assert same_bits(res["sigma"], np.std(Ab, axis=0)) and np.all(res["sigma"] > 0.0)
    assert "n_eff" in res and res["mu"].shape == (len(A), len(pick))


# ---- refusals -------------------------------------------------------------------------------------------------------------------
A_QN = np.random.default_rng(5).normal(size=(2, N))


def obs_matrix():
    dm = matrix()
    dm.set_scan_observables(A_QN)
    return dm


def test_matrix_refuses_an_array_of_the_wrong_length():
    def call(dm, f=F, coeff_lb=COEFF, offset_l=OFFSET, f_scan=F_SCAN, center_lb=None, second=True):
        return dm.scan_obs_sums(f, coeff_lb, offset_l, f_scan, second=second, center_lb=center_lb)

    good = dict(f=F, coeff_lb=COEFF, offset_l=OFFSET, f_scan=F_SCAN, center_lb=np.zeros_like(COEFF))
    axes = dict(f=(0,), coeff_lb=(1,), offset_l=(0,), f_scan=(0,), center_lb=(0, 1))
    with obs_matrix() as dm, obs_matrix() as fresh:
        for arg, ax in axes.items():
            for bad in wrong(good[arg], ax):
                with refused(dm):
                    call(dm, **{arg: bad})
        for bad in list(wrong(A_QN, (1,))) + [A_QN[:0], A_QN[0], A_QN[None]]:
            with refused(dm):
                dm.set_scan_observables(bad)
        assert [a.shape for a in call(dm)] == [(2, 2), (2, 2), (2, 2), (2,), (2,)]
        assert_same(call(dm), call(fresh), "scan_obs_sums")
        # what only the library can see: an entry that is not a number; the block stays as it was
        for bad in (np.nan, np.inf):
            poisoned = A_QN.copy()
            poisoned[1, 3] = bad
            with pytest.raises(ValueError, match="mbar_ctx_set_scan_obs"):
                dm.set_scan_observables(poisoned)
        assert_same(call(dm), call(fresh), "scan_obs_sums after the refusals")
        assert_same(call(dm, second=False), call(fresh, second=False), "the first moments after the refusals")
        dm.set_scan_observables(None)
        with refused(dm):  # (no observables: refused before the library is called)
            call(dm)
        dm.set_scan_observables(A_QN)
        assert_same(call(dm), call(fresh), "scan_obs_sums after a release")
    with DeviceMatrix.from_host(np.zeros((3, 5))) as bare:
        bare.set_scan_observables(A_QN)  # (the block does not need a basis)
        with pytest.raises(ValueError, match=r"no basis on this matrix \(set_scan first\)"):
            call(bare)


def test_library_refuses_bad_arguments_and_contexts():
    MBAR_ERR_STATE = -4
    L, Q = 2, 2

    def sums(owner, K, s1=True, t1=True, t2=True, wsum=True, w2sum=True, f_scan=F_SCAN, L=L):
        out = lambda on, shape: _dptr(np.empty(shape)) if on else None
        rc = owner._lib.mbar_scan_obs_sums(owner._ctx, _dptr(np.zeros(K)), L, _dptr(COEFF), _dptr(OFFSET), _dptr(f_scan), out(s1, (L, Q)),
                                           out(t1, (L, Q)), out(t2, (L, Q)), out(wsum, L), out(w2sum, L))
        return rc, _lib.last_error(owner._ctx)

    def upload(owner, Q=Q, a=A_QN, ld=N):
        rc = owner._lib.mbar_ctx_set_scan_obs(owner._ctx, Q, None if a is None else _dptr(np.ascontiguousarray(a)), ld)
        return rc, _lib.last_error(owner._ctx)

    with matrix() as dm:
        rc, message = sums(dm, 3)
        assert rc == MBAR_ERR_STATE and "mbar_scan_obs_sums" in message and "no observables" in message, message
        for kw in (dict(Q=-1), dict(a=None), dict(ld=N - 1)):
            rc, message = upload(dm, **kw)
            assert rc == _lib.MBAR_ERR_ARG and "mbar_ctx_set_scan_obs" in message, (kw, rc, message)
        assert upload(dm)[0] == _lib.MBAR_OK
        for kw in (dict(s1=False), dict(wsum=False), dict(t1=False), dict(t2=False), dict(w2sum=False), dict(t1=False, t2=False), dict(L=0)):
            rc, message = sums(dm, 3, **kw)
            assert rc == _lib.MBAR_ERR_ARG and "mbar_scan_obs_sums" in message, (kw, rc, message)
        with LoopbackGroup(1) as group:
            dm.set_loopback(group, 0)
            for rc, message in (sums(dm, 3), upload(dm)):
                assert rc == MBAR_ERR_STATE and "mbar_" in message and "transport" in message, message
            dm.comm_destroy()
        assert sums(dm, 3)[0] == _lib.MBAR_OK and sums(dm, 3, t1=False, t2=False, w2sum=False)[0] == _lib.MBAR_OK
        # a pitch wider than N: the rows are taken at the pitch
        wide_rows = np.hstack([A_QN, np.full((2, 3), np.nan)])
        assert upload(dm, a=wide_rows, ld=N + 3)[0] == _lib.MBAR_OK
        dm._scan_obs = 2
        got = dm.scan_obs_sums(F, COEFF, OFFSET, F_SCAN)
        with obs_matrix() as fresh:
            assert_same(got, fresh.scan_obs_sums(F, COEFF, OFFSET, F_SCAN), "rows at a pitch")
        # a NaN among the free energies or the normalisers: NaN outputs, MBAR_OK
        s1, t1, t2, wsum, w2sum = dm.scan_obs_sums(F, COEFF, OFFSET, np.array([0.2, np.nan]))
        assert all(np.all(np.isnan(a)) for a in (s1, t1, t2, wsum, w2sum))
    u, N_k, _ = random_problem(129, 300, seed=3)
    with DeviceMatrix.from_host(u) as wide:
        wide.set_Nk(N_k)
        for rc, message in (sums(wide, 129), upload(wide, a=np.zeros((2, 300)), ld=300)):
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
            mbar.compute_scan_expectations(u[2], basis, coeff)
    finally:
        mbar.close()
    u, N_k, _ = random_problem(4, 600, seed=5)
    basis = np.stack([u[0], u[1]])
    mbar = pymbar_amd.MBAR(u, N_k)
    try:
        want = mbar.compute_scan_expectations(u[2:], basis, coeff)
        with LoopbackGroup(2) as group:
            mbar._dm.set_loopback(group, 0)
            try:
                with pytest.raises(ParameterError, match="single-rank"):
                    mbar.compute_scan_expectations(u[2:], basis, coeff)
                with pytest.raises(ParameterError, match="single-rank"):
                    mbar.set_scan_observables(u[2:])
            finally:
                mbar._dm.comm_destroy()
        got = mbar.compute_scan_expectations(u[2:], basis, coeff)
    finally:
        mbar.close()
    for key in want:
        assert same_bits(got[key], want[key]), key
