"""The state machine of ``pymbar_amd.mbar_batch`` on the host (``mbar_batch_step_host``, no GPU) against the oracle's adaptive
loop, and the input rules of ``mbar_batch`` (checked before any device work)."""
import numpy as np
import pytest
from scipy.special import logsumexp

import pymbar_amd
from oracle import mbar_oracle as oracle
from pymbar_amd import _lib
from pymbar_amd import batch
from pymbar_amd import testsystems as ts
from pymbar_amd.utils import ParameterError


def _lognum(u_kn, N_k, f):
    logden = oracle.log_denominator(u_kn, N_k, f)
    return logsumexp(-logden - u_kn, axis=1)


def _gram(u_kn, N_k, f):
    p = N_k * oracle.mbar_W_nk(u_kn, N_k, f)
    return p.T @ p


def drive(u_kn, N_k, f0, tol=1e-12, min_sc_iter=0, maxiter=10000, gamma=1.0):
    """Runs one problem's loop with every pass evaluated by the oracle; returns the final state and the choice per iteration."""
    K = u_kn.shape[0]
    N_k = np.asarray(N_k, dtype=np.float64)
    st = _lib.BatchState()
    st.K = K
    st.tol, st.gamma, st.maxiter, st.min_sc_iter = tol, gamma, maxiter, min_sc_iter
    for k in range(K):
        st.Nk[k] = N_k[k]
        st.f[k] = f0[k]
    batch.step_host(st)
    choices = []
    while st.status == batch.RUNNING:
        reqs = [np.array(st.req[r][:K]) for r in range(st.nreq)]
        ln = np.stack([_lognum(u_kn, N_k, f) for f in reqs])
        G = _gram(u_kn, N_k, reqs[st.gram_req]) if st.gram_req >= 0 else None
        before = st.iterations
        batch.step_host(st, ln, G)
        if st.iterations > before:
            choices.append("nr" if (st.choices >> before) & 1 else "sci")
    return st, choices


def _check_against_oracle(u_kn, N_k, f0, min_sc_iter):
    N_k = np.asarray(N_k)
    sws = np.where(N_k > 0)[0]
    hist = []
    f_ref, res = oracle.solve_mbar_once_adaptive(u_kn[sws], N_k[sws], f0[sws], tol=1e-12, min_sc_iter=min_sc_iter, history=hist)
    st, choices = drive(u_kn, N_k, f0, min_sc_iter=min_sc_iter)
    assert st.status == batch.DONE and st.success == 1
    assert st.iterations == res["iterations"]
    ref_choices = [h["choice"] for h in hist]
    # deviation 3 of INTEGRATION.md section 3: the last iteration's choice compares two round-off gradient norms
    assert choices[:-1] == ref_choices[:-1]
    assert abs(st.nr_iter - res["nr_iter"]) <= 1 and st.nr_iter + st.sci_iter == st.iterations
    f = np.array(st.f[: len(N_k)])
    np.testing.assert_allclose(f[sws], f_ref, rtol=1e-12, atol=1e-12)
    # the all-state update at the solution from the state's own lognum
    f_all = -np.array(st.lognum[: len(N_k)])
    f_all -= f_all[0]
    f_or, _ = oracle.solve_mbar_for_all_states(u_kn, N_k, f0, sws, tol=1e-12, min_sc_iter=min_sc_iter)
    np.testing.assert_allclose(f_all, f_or, rtol=1e-11, atol=1e-11)


@pytest.mark.parametrize("min_sc_iter", [0, 2])
def test_state_machine_config1(golden, min_sc_iter):
    g = golden("config1_ho_K5_N5000.npz")
    _check_against_oracle(g["u_kn"], g["N_k"], np.zeros(5), min_sc_iter)
    if min_sc_iter == 0:
        st, choices = drive(g["u_kn"], g["N_k"], np.zeros(5))
        assert st.iterations == int(g["adaptive_iters"])
        assert [1 if c == "nr" else 0 for c in choices][:-1] == list(g["adaptive_choices"])[:-1]
        np.testing.assert_allclose(np.array(st.f[:5]), g["f_adaptive"], rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("min_sc_iter", [0, 2])
def test_state_machine_exponentials_and_unsampled(golden, min_sc_iter):
    g = golden("exp_K20_N1000.npz")
    _check_against_oracle(g["u_kn"], g["N_k"], np.zeros(20), min_sc_iter)
    g = golden("ho_unsampled_K4_N2300.npz")
    _check_against_oracle(g["u_kn"], g["N_k"], np.zeros(4), min_sc_iter)


@pytest.mark.parametrize("min_sc_iter", [0, 2])
def test_state_machine_oscillators_from_a_start(min_sc_iter):
    x_n, u_kn, N_k, s_n = ts.harmonic_u_kn(np.linspace(0, 3, 9), np.linspace(1, 4, 9), [60, 0, 80, 50, 0, 70, 40, 90, 30], seed=11)
    f0 = np.linspace(0.0, 2.0, 9)
    _check_against_oracle(u_kn, N_k, f0 - f0[0], min_sc_iter)


def test_state_machine_edges():
    # one sampled state: no solve, one pass for the all-state update
    x_n, u_kn, N_k, s_n = ts.harmonic_u_kn(np.array([0.0, 1.0, 2.0]), np.array([1.0, 1.0, 1.0]), [0, 40, 0], seed=2)
    st, choices = drive(u_kn, N_k, np.array([0.0, 0.5, 1.0]))
    assert st.status == batch.DONE and st.success == 1 and st.iterations == 0 and st.f[1] == 0.0
    # no iterations allowed: the start comes back, not converged
    st, _ = drive(u_kn[:2, :40], np.array([20, 20]), np.array([0.0, 0.3]), maxiter=0)
    assert st.status == batch.DONE and st.success == 0 and st.iterations == 0 and st.f[1] == 0.3
    # an iteration limit ends the loop unconverged after that many iterations
    g = ts.harmonic_u_kn(np.linspace(0, 2, 4), np.ones(4), [30] * 4, seed=5)
    st, choices = drive(g[1], g[2], np.zeros(4), maxiter=2)
    assert st.status == batch.DONE and st.success == 0 and st.iterations == 2 and len(choices) == 2


def disconnected_problem():
    """States {0, 1} and {2} share no sample: the gauge-fixed Hessian has a zero pivot (state 2's row is zero)."""
    x_n, u_kn, N_k, s_n = ts.harmonic_u_kn(np.array([0.0, 0.5, 3.0]), np.array([1.0, 1.0, 1.0]), [30, 30, 30], seed=4)
    u_kn[2, :60] = np.inf
    u_kn[:2, 60:] = np.inf
    return u_kn, N_k


def test_state_machine_hands_back_a_singular_system():
    u_kn, N_k = disconnected_problem()
    st, _ = drive(u_kn, N_k, np.zeros(3))
    assert st.status == batch.FALLBACK and st.newton_bad == 1 and st.nreq == 0


def test_all_states_update_equals_the_formula_per_problem():
    """The shared all-state update on a whole state array against ``solve_mbar_for_all_states``'s update written out per problem:
    ragged widths, an unsampled state in one row, sums over hundreds of orders of magnitude (one subnormal), f of both signs.
    The same expression per element: no tolerance."""
    rng = np.random.default_rng(5)
    Ks = [1, 2, 8, 9, 64]
    states = (_lib.BatchState * len(Ks))()
    sv = batch._states_view(states)
    for name in ("f", "psum", "lognum", "Nk"):   # what lies behind column K must not matter
        sv[name] = rng.normal(size=sv[name].shape)
    Nks = []
    for e, K in enumerate(Ks):
        N_k = rng.integers(1, 1000, size=K)
        if K == 8:
            N_k[3] = 0                               # an unsampled state: this row takes -lognum
        Nks.append(N_k)
        sv["K"][e] = K
        sv["Nk"][e, :K] = N_k
        sv["f"][e, :K] = rng.normal(scale=30.0, size=K)
        sv["psum"][e, :K] = 10.0 ** rng.uniform(-300, 300, size=K)
        sv["lognum"][e, :K] = rng.normal(scale=30.0, size=K)
    sv["psum"][4, 7] = 1e-310                        # (subnormal, and still so after the division by N_k < 1000)
    assert (sv["f"] < 0).any() and (sv["f"] > 0).any()
    got = batch._all_states_update(sv)
    for e, K in enumerate(Ks):
        N_k = Nks[e]
        f = sv["f"][e, :K].copy()
        if np.all(N_k > 0):
            f = f - np.log(sv["psum"][e, :K] / N_k)
        else:
            f = -1.0 * sv["lognum"][e, :K]
        f -= f[0]
        assert np.all(np.isfinite(f)) and (K == 8) == (not np.all(N_k > 0))
        assert np.array_equal(got[e, :K], f), (K, got[e, :K] - f)


def test_input_rules():
    u = np.zeros((3, 10))
    with pytest.raises(ParameterError, match="at least one problem"):
        pymbar_amd.mbar_batch([], [])
    with pytest.raises(ParameterError, match="problem 1: K = 65"):
        pymbar_amd.mbar_batch([u, np.zeros((65, 65))], [[3, 3, 4], [1] * 65])
    with pytest.raises(ParameterError, match="problem 0: The sum of all N_k"):
        pymbar_amd.mbar_batch([u], [[3, 3, 3]])
    with pytest.raises(ParameterError, match="problem 1: N_k must have shape"):
        pymbar_amd.mbar_batch([u, u], [[3, 3, 4], [5, 5]])
    with pytest.raises(ParameterError, match="problem 0: initial_f_k must be a 3-dimensional"):
        pymbar_amd.mbar_batch([u], [[3, 3, 4]], initial_f_k=[np.zeros(4)])
    with pytest.raises(ParameterError, match="initial_f_k vectors"):
        pymbar_amd.mbar_batch([u, u], [[3, 3, 4]] * 2, initial_f_k=[np.zeros(3)])
    with pytest.raises(ParameterError, match="uncertainty_method"):
        pymbar_amd.mbar_batch([u], [[3, 3, 4]], uncertainty_method="svd")
