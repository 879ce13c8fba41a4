"""Derivatives of f and of the averages along a scan (``MBAR.compute_scan_gradient``, ``DeviceMatrix.scan_moments``), host logic on
the CPU stand-in (tests/scan_gradient_standin.py): central differences of the stand-in's own long-double ``f`` and ``mu``, the
reference's raw moments (tests/golden/scan_gradient_ho_K5.npz from make_golden_scan_gradient.py), the argument layer of the new face
and the refusals.

Tolerances.  The finite differences: the step and the third derivative (``fd_bound``).  The fixture: ten times the worst error of
the stand-in against it, in units of ``sqrt(<phi_i^2>)`` for a mean and ``sqrt(<phi_i^2><phi_j^2>)`` for a covariance -- the raw-moment
route ``<phi phi'> - <phi><phi'>`` of the reference cancels, the centred one does not (profiles/scan_gradient_accuracy.txt).  The
device's bounds of tests/test_gpu_scan_gradient.py are kept here too, next to the figures they come from."""
import numpy as np
import pytest

import pymbar_amd
from pymbar_amd import testsystems
from pymbar_amd.device import DeviceMatrix
from pymbar_amd.scan import gradient_layout
from pymbar_amd.utils import ParameterError
from tests.conftest import load_golden
from tests.scan_gradient_standin import GradientOracleMatrix, ScanOnlyMatrix, features_ld

LD = np.longdouble

# ten times the worst error seen on the device against the long-double stand-in over the matrix of cases of
# tests/test_gpu_scan_gradient.py, about zero and about the means, in the units of scaled_gaps (profiles/scan_gradient_accuracy.txt):
# m1 3.6e-13, m2 4.9e-13, ma 3.2e-13 -- all three at members of the (8, 4) family whose weight sits on a few samples: one ulp of a
# feature dl^2 of 3e4 stands against a spread of a few units
MOMENTS_TOL = dict(m1=3.6e-12, m2=5.0e-12, ma=3.3e-12)
# ten times the worst error seen, stand-in or device, against the reference's raw moments, scaled as said above: config 1 -- grad_f
# 1.08e-14, hess_f 5.64e-13, grad_mu 1.13e-13; the seam -- grad_f 1.08e-14, hess_f 6.37e-13, grad_mu 6.74e-15
FIXTURE_TOL = dict(grad_f=1.1e-13, hess_f=5.7e-12, grad_mu=1.2e-12)
SEAM_TOL = dict(grad_f=1.1e-13, hess_f=6.4e-12, grad_mu=6.8e-14)
# a member with a sampled state's parameters against that state's compute_expectations on the device, relative to max(|mu|, 1):
# ten times the 1.11e-15 measured
SAMPLED_STATE_TOL = 1.2e-14


def gap(name, got, want, scale=1.0):
    g = float(np.max(np.abs(np.asarray(got) - np.asarray(want)) / scale))
    print("%-12s max scaled gap %.3e" % (name, g))
    return g


@pytest.fixture
def standin(monkeypatch):
    import pymbar_amd.device

    monkeypatch.setattr(pymbar_amd.device, "DeviceMatrix", GradientOracleMatrix)


@pytest.fixture(scope="module")
def gold():
    return load_golden("scan_gradient_ho_K5.npz")


def observables(x_n):
    return np.stack([np.cos(x_n), x_n * x_n * np.sin(x_n)])


def fixture_family(gold, x_n):
    basis, coeff, offset = testsystems.harmonic_scan_family(x_n, gold["O_l"], gold["K_l"])
    np.testing.assert_array_equal(coeff, gold["coeff"])
    np.testing.assert_array_equal(offset, gold["offset"])
    return basis, coeff, offset, observables(x_n)


def seam_family():
    """The umbrellas of periodic_umbrella_K6.npz as a family and its 40 unsampled centres (120 .. 240 degrees) as members"""
    g = load_golden("periodic_umbrella_K6.npz")
    basis, coeff, center, harmonic, period, offset, N_k = testsystems.periodic_umbrella_family(K=6, n_per_state=300, seed=0)
    assert np.array_equal(basis[1], g["chi_n"]) and np.array_equal(N_k, g["N_k"])
    L = len(g["chi0_l"])
    members = dict(coeff_lb=np.tile([1.0, 0.5 * g["spring_k"][0]], (L, 1)), center_lb=np.stack([np.zeros(L), g["chi0_l"]], axis=1))
    return dict(basis=basis, coeff=coeff, center=center, harmonic=harmonic, period=period, offset=offset, N_k=N_k), members


def fixture_gaps(res, mean, second, spec, extra={}, A_scale=None, second_A=None, mean_A=None):
    """The expected derivatives from the reference's raw moments ``mean[i]``, ``second[i, j]`` of the features (and ``mean_A[q]``,
    ``second_A[q, i]`` with the observables), by the identities, against ``res``.  ``spec``: (feature, factor) of every parameter's ``g
    = du/dp``, ``extra[(p, r)]``: ``<d2u/dp dr>`` where it is not zero -- written out by the caller, not taken from the code under test.
    Returns the worst gap of ``grad_f``, ``hess_f`` and ``grad_mu`` in units of ``sqrt(<phi_i^2>)`` per feature involved (times the
    factors, times ``max |A|``)."""
    rms = np.sqrt(np.stack([second[i, i] for i in range(len(mean))]))
    cov = second - mean[:, None, :] * mean[None, :, :]
    out = dict(grad_f=0.0, hess_f=0.0)
    for p, (i, s) in enumerate(spec):
        out["grad_f"] = max(out["grad_f"], gap("grad_f[%d]" % p, res["grad_f"][:, p], s * mean[i], np.abs(s) * rms[i]))
        for r, (j, t) in enumerate(spec):
            want = extra.get((p, r), 0.0) - (s * t) * cov[i, j]
            out["hess_f"] = max(out["hess_f"], gap("hess_f[%d,%d]" % (p, r), res["hess_f"][:, p, r], want, np.abs(s * t) * rms[i] * rms[j]))
    if second_A is not None:
        out["grad_mu"] = 0.0
        for q in range(len(mean_A)):
            for p, (i, s) in enumerate(spec):
                want = -s * (second_A[q, i] - mean_A[q] * mean[i])
                out["grad_mu"] = max(out["grad_mu"], gap("grad_mu[%d,%d]" % (q, p), res["grad_mu"][q, :, p], want,
                                                         np.abs(s) * A_scale[q] * rms[i]))
    return out


def check_against_fixture(res, gold, tol=None):
    """Config 1: parameters coeff_0 (x^2) and coeff_1 (x).  Shared with the GPU test."""
    tol = FIXTURE_TOL if tol is None else tol
    assert res["params"] == [("coeff", 0), ("coeff", 1)] and res["features"] == [(0, "basis"), (1, "basis")]
    x_n = testsystems.config1(seed=0)[0]
    pp = gold["mu_phiphi"]
    second = np.array([[pp[0], pp[1]], [pp[1], pp[2]]])
    ones = np.ones(len(gold["O_l"]))
    gaps = fixture_gaps(res, gold["mu_phi"], second, [(0, ones), (1, ones)], {}, np.abs(observables(x_n)).max(axis=1), gold["mu_Aphi"],
                        gold["mu_A"])
    g_mu = gap("mu", res["mu"], gold["mu_A"], np.abs(gold["mu_A"]))
    gaps["feature_mean"] = gap("feature_mean", res["feature_mean"], gold["mu_phi"].T, np.sqrt(np.stack([pp[0], pp[2]])).T)
    assert g_mu <= 1e-9 and gaps["feature_mean"] <= tol["grad_f"]
    for name in ("grad_f", "hess_f", "grad_mu"):
        assert gaps[name] <= tol[name], (name, gaps[name])
    return gaps


def check_against_seam_fixture(res, gold, tol=None):
    """The seam: features E, dl, dl^2; parameters coeff_0 (E), coeff_1 (dl^2), center_1 (-2 k dl); the observable is E.  Shared with
    the GPU test."""
    tol = SEAM_TOL if tol is None else tol
    assert res["params"] == [("coeff", 0), ("coeff", 1), ("center", 1)] and res["features"] == [(0, "basis"), (1, "dl"), (1, "dl2")]
    _, members = seam_family()
    k_l = members["coeff_lb"][:, 1]
    mean, second = gold["seam_mu"], gold["seam_mu2"]
    ones = np.ones(len(k_l))
    E = seam_family()[0]["basis"][0]
    extra = {(2, 2): 2.0 * k_l, (1, 2): -2.0 * mean[1], (2, 1): -2.0 * mean[1]}  # d2u/dc2 = 2 k, d2u/dk dc = -2 dl
    gaps = fixture_gaps(res, mean, second, [(0, ones), (2, ones), (1, -2.0 * k_l)], extra, [np.abs(E).max()], second[:1], mean[:1])
    for name in ("grad_f", "hess_f", "grad_mu"):
        assert gaps[name] <= tol[name], (name, gaps[name])
    assert np.all(np.isfinite(res["hess_f"])) and np.array_equal(res["hess_f"], np.swapaxes(res["hess_f"], 1, 2))
    return gaps


# ---- the reference ---------------------------------------------------------------------------------------------------------------------

def test_method_reproduces_reference(standin, gold):
    x_n, u_kn, N_k, _, _, _ = testsystems.config1(seed=0)
    basis, coeff, offset, A_qn = fixture_family(gold, x_n)
    mbar = pymbar_amd.MBAR(u_kn, N_k, relative_tolerance=1e-12)
    res = mbar.compute_scan_gradient(basis, coeff, offset, A_qn)
    assert set(res) == {"f", "mu", "grad_f", "hess_f", "grad_mu", "feature_mean", "feature_cov", "params", "features"}
    assert res["grad_f"].shape == (40, 2) and res["hess_f"].shape == (40, 2, 2) and res["grad_mu"].shape == (2, 40, 2)
    check_against_fixture(res, gold)
    scan = mbar.compute_scan(basis, coeff, offset, A_qn, compute_uncertainty=False)
    np.testing.assert_allclose(res["f"], scan["f"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(res["mu"], scan["mu"], rtol=1e-12, atol=0)
    plain = mbar.compute_scan_gradient(basis, coeff, offset, hessian=False)
    assert set(plain) == {"f", "grad_f", "feature_mean", "feature_cov", "params", "features"}
    assert mbar._dm._scan is None


def test_sweep_across_the_seam_reproduces_reference(standin, gold):
    fam, members = seam_family()
    m = pymbar_amd.MBAR.from_family(fam["basis"], fam["coeff"], fam["N_k"], offset_k=fam["offset"], center_kb=fam["center"],
                                    harmonic_b=fam["harmonic"], period_b=fam["period"], relative_tolerance=1e-12)
    res = m.compute_scan_gradient(A_qn=fam["basis"][0], **members)  # basis and kinds: the constructor's
    check_against_seam_fixture(res, gold)
    explicit = m.compute_scan_gradient(fam["basis"], A_qn=fam["basis"][0], harmonic_b=fam["harmonic"], period_b=fam["period"], **members)
    for key in ("f", "grad_f", "hess_f", "grad_mu"):
        assert explicit[key].tobytes() == res[key].tobytes(), key
    with pytest.raises(ParameterError):
        m.compute_scan_gradient(coeff_lb=members["coeff_lb"])  # a harmonic term without centres


# ---- finite differences on the stand-in ------------------------------------------------------------------------------------------------

def ld_f_mu(dm, f_k, coeff, offset, center, A_qn):
    """``f`` (L,) and ``mu`` (Q, L) of the members in long double, from the stand-in's own ``x_ln``"""
    def run():
        x, _, _ = dm._members(f_k, coeff, offset)
        M = x.max(axis=1)
        e = np.exp(x - M[:, None])
        S0 = e.sum(axis=1)
        return -(M + np.log(S0)), (e @ np.asarray(A_qn, dtype=LD).T / S0[:, None]).T, e / S0[:, None]

    return dm._call(center, run)


def fd_bound(w, g_p, curv, h, p, order, r=None, A=None):
    """What a central difference of step ``h`` along parameter ``p`` may miss: ``h^2 / 6`` times the third derivative of the differenced
    quantity, bounded over the step by twice its bound at the point.  The derivatives of ``f`` are joint cumulants of the ``g = du/dp``
    and, for a centre, of the constant ``d2u/dc2 = 2 k`` (``curv[p]``, of the size of ``g^2``).  A joint cumulant of ``k`` variables is
    bounded through Hoelder's inequality by ``2^k`` (the partitions of k <= 4 items number at most 15 < 2^4) times the product of their
    sizes ``s = (E|g - <g>|^k)^(1/k) + sqrt(curv)``.  ``order`` 3: differences of ``f``, ``s_p^3``; 4 with ``r``: differences of
    ``grad_f[r]``, ``s_r s_p^3``; 3 with ``A``: differences of ``mu``, ``2 max|A - <A>| s_p^3``.  ``w``: the members' normalised weights
    (L, n), ``g_p``: (P, L, n)."""
    def size(i):
        d = g_p[i] - (w * g_p[i]).sum(axis=1)[:, None]
        return (w * np.abs(d) ** order).sum(axis=1) ** (1.0 / order) + np.sqrt(curv[i])

    bound = 2.0 * h * h / 6.0 * 2.0 ** order * size(p) ** 3
    if r is not None:
        bound = bound * size(r)
    if A is not None:
        bound = bound * 2.0 * np.abs(A[None, :] - (w * A[None, :]).sum(axis=1)[:, None]).max(axis=1)
    return np.asarray(bound, dtype=np.float64)


def family_cases():
    x_n, u_kn, N_k, _, O_k, K_k = testsystems.config1(seed=0)
    rng = np.random.default_rng(5)
    basis, coeff, offset = testsystems.harmonic_scan_family(x_n, rng.uniform(0.5, 3.5, 6), rng.uniform(10.0, 30.0, 6))
    yield "linear", dict(u=u_kn, N_k=N_k, basis=basis, coeff=coeff, offset=offset, center=None, kinds={}, A=observables(x_n))
    fam, members = seam_family()
    u = testsystems.family_u_kn(fam["basis"], fam["coeff"], fam["offset"], fam["center"], fam["harmonic"], fam["period"])
    pick = slice(3, 40, 7)
    yield "harmonic", dict(u=u, N_k=fam["N_k"], basis=fam["basis"], coeff=members["coeff_lb"][pick], offset=np.zeros(6),
                           center=members["center_lb"][pick] + 0.37, kinds=dict(harmonic_b=fam["harmonic"], period_b=fam["period"]),
                           A=np.stack([fam["basis"][0], np.cos(np.deg2rad(fam["basis"][1]))]))


@pytest.mark.parametrize("name, c", list(family_cases()), ids=["linear", "harmonic"])
def test_gradient_and_hessian_against_central_differences_of_the_standin(standin, name, c):
    """``grad_f`` against central differences of the stand-in's long-double ``f``, ``hess_f`` against those of ``grad_f`` (the
    method's, at the displaced parameters: the columns of a Hessian are derivatives of the gradient), ``grad_mu`` against those of the
    long-double ``mu``.  No sample of the harmonic case sits within the step of a seam."""
    mbar = pymbar_amd.MBAR(c["u"], c["N_k"], relative_tolerance=1e-12)
    cen = {} if c["center"] is None else dict(center_lb=c["center"])
    res = mbar.compute_scan_gradient(c["basis"], c["coeff"], c["offset"], c["A"], **cen, **c["kinds"])
    dm = mbar._dm
    dm.set_Nk(mbar.N_k)
    dm.set_scan(c["basis"], None, **c["kinds"])
    L, B = c["coeff"].shape
    hb = c["kinds"].get("harmonic_b")
    features, params = gradient_layout(B, hb)
    assert res["params"] == params
    _, _, w = ld_f_mu(dm, mbar.f_k, c["coeff"], c["offset"], c["center"], c["A"])
    phi = features_ld(c["basis"], c["center"], hb, c["kinds"].get("period_b"), L)
    g_p = []
    for kind, b in params:
        if kind == "center":
            g_p.append(-2.0 * c["coeff"][:, b][:, None] * phi[:, features.index((b, "dl"))])
        else:
            g_p.append(phi[:, features.index((b, "dl2") if (b, "dl2") in features else (b, "basis"))])
    if hb is not None:  # the derivative is the almost-everywhere one: keep the step clear of the seam
        dl = np.abs(np.asarray(phi[:, features.index((1, "dl"))], dtype=np.float64))
        assert np.min(180.0 - dl) > 1e-3  # (the centre moves by 1e-4)
    worst = dict(grad_f=0.0, hess_f=0.0, grad_mu=0.0)
    for p, (kind, b) in enumerate(params):
        h = 1e-4 * (np.abs(c["coeff"][:, b]).max() if kind == "coeff" else 1.0)
        out = []
        for sign in (+1.0, -1.0):
            coeff, center = c["coeff"].copy(), None if c["center"] is None else c["center"].copy()
            (coeff if kind == "coeff" else center)[:, b] += sign * h
            f, mu, _ = ld_f_mu(dm, mbar.f_k, coeff, c["offset"], center, c["A"])
            cen_d = {} if center is None else dict(center_lb=center)
            dm.set_scan(None)
            grad = mbar.compute_scan_gradient(c["basis"], coeff, c["offset"], hessian=False, **cen_d, **c["kinds"])["grad_f"]
            dm.set_scan(c["basis"], None, **c["kinds"])
            out.append((f, mu, grad))
        fd_f = np.asarray((out[0][0] - out[1][0]) / (2.0 * h), dtype=np.float64)
        fd_mu = np.asarray((out[0][1] - out[1][1]) / (2.0 * h), dtype=np.float64)
        fd_grad = (out[0][2] - out[1][2]) / (2.0 * h)
        curv = [2.0 * np.abs(c["coeff"][:, bb]) if kk == "center" else np.zeros(L) for kk, bb in params]
        # (grad_f and the float64 parameters carry roundings that the step magnifies: eps |value| / h, with a factor 16 for the chain)
        eps = np.finfo(np.float64).eps
        round_f = 16.0 * np.finfo(LD).eps * np.abs(np.asarray(out[0][0], dtype=np.float64)) / h + 16.0 * eps * np.abs(res["grad_f"][:, p])
        worst["grad_f"] = max(worst["grad_f"], gap("grad_f %s" % (params[p],), res["grad_f"][:, p], fd_f, fd_bound(w, g_p, curv, h, p, 3) + round_f))
        for r in range(len(params)):
            round_g = 16.0 * eps * np.abs(res["grad_f"][:, r]) / h
            worst["hess_f"] = max(worst["hess_f"], gap("hess_f %s %s" % (params[r], params[p]), res["hess_f"][:, r, p], fd_grad[:, r],
                                                       fd_bound(w, g_p, curv, h, p, 4, r=r) + round_g))
        for q in range(len(c["A"])):
            worst["grad_mu"] = max(worst["grad_mu"], gap("grad_mu %d %s" % (q, params[p]), res["grad_mu"][q, :, p], fd_mu[q],
                                                         fd_bound(w, g_p, curv, h, p, 3, A=c["A"][q].astype(LD)) + 16.0 * eps * np.abs(fd_mu[q])))
    dm.set_scan(None)
    assert all(v <= 1.0 for v in worst.values()), worst
    assert np.max(np.abs(res["grad_f"])) > 1e-3 and np.max(np.abs(res["hess_f"])) > 1e-3 and np.max(np.abs(res["grad_mu"])) > 1e-3


# ---- the argument layer ----------------------------------------------------------------------------------------------------------------

class _NoCalls:
    def __getattr__(self, name):
        def call(*args):
            raise AssertionError(f"{name} was called with an argument that should have been refused")

        return call


def bare_matrix(K, N, B, Q, harmonic=None):
    """A ``DeviceMatrix`` as ``set_scan`` leaves it, without a device or a library: any call into the library fails the test"""
    dm = DeviceMatrix.__new__(DeviceMatrix)
    dm.K, dm.N_local, dm._lib, dm._scan, dm._scan_harmonic = K, N, _NoCalls(), (B, Q), harmonic
    return dm


def wrong(a, axes):
    for ax in axes:
        yield np.delete(a, -1, axis=ax)
        yield np.concatenate([a, np.take(a, [-1], axis=ax)], axis=ax)


@pytest.mark.parametrize("harmonic", [None, np.array([False, True])], ids=["linear", "harmonic"])
def test_every_array_of_the_face_is_refused_one_entry_short_and_one_long(harmonic):
    K, N, B, Q, L = 3, 5, 2, 1, 4
    F = B + (0 if harmonic is None else 1)
    dm = bare_matrix(K, N, B, Q, harmonic)
    assert dm.scan_features() == (B, F - B, F)
    good = dict(f=np.zeros(K), coeff_lb=np.ones((L, B)), offset_l=np.zeros(L), center_phi=np.zeros((L, F)), center_lb=np.zeros((L, B)))
    for name, axes in (("f", (0,)), ("coeff_lb", (1,)), ("offset_l", (0,)), ("center_phi", (0, 1)), ("center_lb", (0, 1))):
        for bad in wrong(good[name], axes):
            with pytest.raises(ValueError):
                dm.scan_moments(**dict(good, **{name: bad}))
    with pytest.raises(ValueError):
        dm.scan_moments(np.zeros(K), np.ones((0, B)))
    if harmonic is not None:
        with pytest.raises(ValueError, match="center_lb is required"):
            dm.scan_moments(**dict(good, center_lb=None))
    with pytest.raises(AssertionError, match="was called"):  # (the conforming call is the one that reaches the library)
        dm.scan_moments(**good)
    dm._scan = None
    with pytest.raises(ValueError, match="set_scan first"):
        dm.scan_moments(**good)
    with pytest.raises(ValueError, match="set_scan first"):
        dm.scan_features()


# ---- refusals --------------------------------------------------------------------------------------------------------------------------

def test_refusals(standin, gold):
    x_n, u_kn, N_k, _, _, _ = testsystems.config1(seed=0)
    basis, coeff, offset, A_qn = fixture_family(gold, x_n)
    coeff, offset = coeff[:6], offset[:6]
    mbar = pymbar_amd.MBAR(u_kn, N_k)
    call = mbar.compute_scan_gradient
    for method in ("svd", "svd-ew", "approximate", "analytical", "nonsense"):
        with pytest.raises(ParameterError, match="not offered"):
            call(basis, coeff, offset, uncertainty_method=method)
    with pytest.raises(ParameterError, match="without any bootstraps"):
        call(basis, coeff, offset, uncertainty_method="bootstrap")
    with pytest.raises(ParameterError, match="built from a dense u_kn"):
        call(None, coeff, offset)  # (an object built from a dense u_kn has no basis of its own)
    with pytest.raises(ParameterError):
        call(basis, None, offset)
    with pytest.raises(ParameterError):
        call(basis, coeff, offset[:-1])
    with pytest.raises(ParameterError):
        call(basis, coeff, offset, A_qn=np.zeros((4, len(x_n))))
    with pytest.raises(ParameterError):
        call(basis, coeff, offset, harmonic_b=[True, False])  # a harmonic term without centres
    assert mbar._dm._scan is None  # nothing is left on the matrix after a refused call


def test_more_than_128_states_are_refused(standin):
    rng = np.random.default_rng(1)
    K, N = 129, 258
    mbar = pymbar_amd.MBAR(rng.normal(0.0, 1.0, (K, N)), np.full(K, 2), maximum_iterations=1)
    with pytest.raises(ParameterError, match="at most 128 states"):
        mbar.compute_scan_gradient(rng.normal(0.0, 1.0, (1, N)), np.ones((2, 1)))


def test_handles_without_the_pass_are_refused(monkeypatch):
    import pymbar_amd.device

    monkeypatch.setattr(pymbar_amd.device, "DeviceMatrix", ScanOnlyMatrix)
    x_n, u_kn, N_k, _, _, _ = testsystems.config1(seed=0)
    mbar = pymbar_amd.MBAR(u_kn, N_k)
    with pytest.raises(ParameterError, match="not supported on this backend"):
        mbar.compute_scan_gradient(np.stack([x_n * x_n, x_n]), np.ones((2, 2)))


def test_bootstrap_plumbing(standin, gold):
    x_n, u_kn, N_k, _, _, _ = testsystems.config1(seed=0)
    basis, coeff, offset, A_qn = fixture_family(gold, x_n)
    pick = np.array([0, 17, 25, 39])
    mbar = pymbar_amd.MBAR(u_kn, N_k, n_bootstraps=3, rseed=7)
    res = mbar.compute_scan_gradient(basis, coeff[pick], offset[pick], A_qn, uncertainty_method="bootstrap")
    assert res["bootstrapped_grad_f"].shape == (3, 4, 2) and res["bootstrapped_hess_f"].shape == (3, 4, 2, 2)
    assert res["bootstrapped_grad_mu"].shape == (3, 2, 4, 2) and res["bootstrapped_mu"].shape == (3, 2, 4)
    for name in ("f", "grad_f", "hess_f", "mu", "grad_mu"):
        np.testing.assert_array_equal(res["d" + name], np.std(res["bootstrapped_" + name], axis=0))
        assert np.all(res["d" + name] > 0.0), name
    # a replicate's gradient is that replicate's own average of the feature
    scan = mbar.compute_scan(basis, coeff[pick], offset[pick], basis, uncertainty_method="bootstrap")
    np.testing.assert_allclose(res["bootstrapped_grad_f"], np.swapaxes(scan["bootstrapped_observables"], 1, 2), rtol=1e-10, atol=1e-12)
    assert mbar._dm._counts is None and mbar._dm._scan is None
