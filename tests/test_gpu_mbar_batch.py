"""``pymbar_amd.mbar_batch`` on the device: the reference's fixtures in one ragged batch, per-entry equality with the
single-problem ``MBAR``, bit-for-bit independence of the batch, a random ragged batch against the oracle, the host fallback and
a batch of 4096 problems.  Tolerances: those of tests/test_gpu_parity.py and tests/test_gpu_scale.py (Delta_f 1e-8 relative,
dDelta_f 1e-7 relative)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pymbar_amd  # noqa: E402
from oracle import mbar_oracle as oracle  # noqa: E402
from pymbar_amd import testsystems as ts  # noqa: E402

TOL = 1e-12


def _adaptive_mbar(u_kn, N_k, f0=None, tol=TOL, maxiter=10000, min_sc_iter=0):
    proto = (dict(method="adaptive", tol=tol, options=dict(min_sc_iter=min_sc_iter, maxiter=maxiter, gamma=1.0)),)
    return pymbar_amd.MBAR(u_kn, N_k, initial_f_k=f0, solver_protocol=proto, maximum_iterations=maxiter)


def _fixture_problems(golden):
    out = []
    g = golden("config1_ho_K5_N5000.npz")
    out.append(("config1", g["u_kn"], g["N_k"], g))
    g = golden("ho_unsampled_K4_N2300.npz")
    out.append(("unsampled", g["u_kn"], g["N_k"], g))
    g = golden("exp_K20_N1000.npz")
    out.append(("exp", g["u_kn"], g["N_k"], g))
    g = golden("ladder_K32_N32000.npz")
    x_n, u_kn, N_k, s_n, O_k, K_k = ts.config2(seed=0, K=32, N=32000)
    out.append(("ladder", u_kn, N_k, g))
    g = golden("config5_alch_K40_N95000.npz")
    x_n, u_kn, N_k, s_n, O_k, K_k = ts.config5(seed=0)
    assert np.array_equal(N_k, g["N_k"])
    out.append(("config5", u_kn, N_k, g))
    g = golden("osc_K50_N5000.npz")
    x_n, u_kn, N_k, s_n = ts.harmonic_u_kn(np.linspace(1, 5, 50), np.linspace(1, 3, 50), [100] * 50, seed=7)
    out.append(("osc", u_kn, N_k, g))
    return out


def _assert_delta_f(D, D_ref, what):
    rel = np.abs(D - D_ref) / np.maximum(np.abs(D_ref), 1e-3)
    assert rel.max() < 1e-8, (what, rel.max())


def test_fixtures_in_one_ragged_batch(golden):
    probs = _fixture_problems(golden)
    r = pymbar_amd.mbar_batch([p[1] for p in probs], [p[2] for p in probs])
    assert r["success"].all() and not r["host_fallback"].any()
    for i, (name, u_kn, N_k, g) in enumerate(probs):
        _assert_delta_f(r["Delta_f"][i], g["Delta_f"], name)
        np.testing.assert_allclose(r["f_k"][i], g["f_k"], rtol=1e-8, atol=1e-9, err_msg=name)
        np.testing.assert_allclose(r["dDelta_f"][i], g["dDelta_f_svd_ew"], rtol=1e-7, atol=1e-9, err_msg=name)
        if "adaptive_iters" in g:
            assert r["iterations"][i] == int(g["adaptive_iters"]), name
            assert abs(r["nr_iterations"][i] - int(g["adaptive_nr"])) <= 1, name
            assert abs(r["sci_iterations"][i] - int(g["adaptive_sci"])) <= 1, name
            # every choice but the last (deviation 3 of INTEGRATION.md section 3)
            assert list(r["choices"][i].astype(int))[:-1] == list(g["adaptive_choices"])[:-1], name
        if "f_adaptive" in g:
            sws = N_k > 0
            np.testing.assert_allclose(r["f_k"][i][sws] - r["f_k"][i][sws][0], g["f_adaptive"], rtol=1e-9, atol=1e-10)


def test_each_entry_equals_the_single_problem_path(golden):
    probs = _fixture_problems(golden)[:3]
    rng = np.random.default_rng(5)
    f0 = [rng.normal(size=len(p[2])) * 0.1 for p in probs]
    for msc in (0, 2):
        r = pymbar_amd.mbar_batch([p[1] for p in probs], [p[2] for p in probs], initial_f_k=f0, min_sc_iter=msc)
        for i, (name, u_kn, N_k, g) in enumerate(probs):
            m = _adaptive_mbar(u_kn, N_k, f0[i], min_sc_iter=msc)
            d = m.compute_free_energy_differences()
            _assert_delta_f(r["Delta_f"][i], d["Delta_f"], name)
            np.testing.assert_allclose(r["f_k"][i], m.f_k, rtol=1e-10, atol=1e-10)
            np.testing.assert_allclose(r["dDelta_f"][i], d["dDelta_f"], rtol=1e-7, atol=1e-10)
            m.close()
            sws = np.where(N_k > 0)[0]
            f_ref, res = oracle.solve_mbar_once_adaptive(u_kn[sws], N_k[sws], (f0[i] - f0[i][0])[sws] - (f0[i] - f0[i][0])[sws[0]],
                                                         tol=TOL, min_sc_iter=msc)
            assert r["iterations"][i] == res["iterations"], name
            assert abs(r["nr_iterations"][i] - res["nr_iter"]) <= 1, name


def test_bits_do_not_depend_on_the_batch(golden):
    probs = _fixture_problems(golden)
    us, Ns = [p[1] for p in probs], [p[2] for p in probs]
    a = pymbar_amd.mbar_batch(us, Ns)
    b = pymbar_amd.mbar_batch(us, Ns)
    for key in ("f_k", "Delta_f", "dDelta_f"):
        for x, y in zip(a[key], b[key]):
            assert np.array_equal(x, y), key
    assert np.array_equal(a["iterations"], b["iterations"])
    for i in (0, 2, 5):
        one = pymbar_amd.mbar_batch([us[i]], [Ns[i]])
        for key in ("f_k", "Delta_f", "dDelta_f"):
            assert np.array_equal(one[key][0], a[key][i]), (key, i)
        assert one["iterations"][0] == a["iterations"][i]


def _random_problem(rng, K, N):
    """A harmonic-oscillator problem with zero-sample states and scattered +inf entries (never a whole column)."""
    N_k = rng.multinomial(N, rng.dirichlet(np.ones(K)))
    if K > 2:
        N_k[rng.integers(1, K)] += N_k[0]  # (state 0 often unsampled)
        N_k[0] = 0
    if N_k.sum() == 0 or (N_k > 0).sum() == 0:
        N_k[-1] = N
    O_k = np.sort(rng.uniform(0, 2, K))
    K_k = rng.uniform(0.5, 4, K)
    x_n, u_kn, N_k, s_n = ts.harmonic_u_kn(O_k, K_k, N_k, seed=int(rng.integers(1 << 30)))
    if K > 3 and N > 20:
        # +inf on a state that did not draw the sample: a finite entry remains in every column
        n = rng.choice(N, size=max(1, N // 50), replace=False)
        k = rng.integers(0, K, size=n.size)
        keep = k != s_n[n]
        u_kn[k[keep], n[keep]] = np.inf
    return u_kn, N_k


def test_random_ragged_batch_against_the_oracle():
    rng = np.random.default_rng(2026)
    us, Ns = [], []
    for p in range(300):
        K = int(rng.integers(2, 65))
        N = int(rng.integers(1, 20001)) if p % 10 == 0 else (int(rng.integers(1, 5001)) if p % 3 else int(rng.integers(1, 300)))
        u, N_k = _random_problem(rng, K, N)
        us.append(u)
        Ns.append(N_k)
    us.append(np.array([[0.3, 1.2, -0.4]]))  # K = 1
    Ns.append(np.array([3]))
    r = pymbar_amd.mbar_batch(us, Ns, compute_uncertainty=False, maximum_iterations=200)
    checked = pinned = 0
    for p in range(len(us)):
        if r["host_fallback"][p]:
            continue
        u_kn, N_k = us[p], Ns[p]
        sws = np.where(N_k > 0)[0]
        hist = []
        f_ref, res = oracle.solve_mbar_for_all_states(u_kn, N_k, np.zeros(len(N_k)), sws, tol=TOL, min_sc_iter=0, maxiter=200,
                                                      history=hist)
        if res is not None:
            if not res["success"]:
                continue
            assert r["success"][p]
            # the iteration count is pinned where the reference's stop is clear: its last relative change below tol / 10 and the
            # one before above 100 tol.  Elsewhere the stop test compares round-off with tol (few samples per state, +inf
            # entries: f_k that carry ~1e-12 of noise), and any summation order may stop an iteration or more apart.
            clear = hist[-1]["max_delta"] < TOL / 10 and (len(hist) < 2 or hist[-2]["max_delta"] > 100 * TOL)
            if clear:
                assert r["iterations"][p] == res["iterations"], p
                pinned += 1
        scale = max(1.0, np.abs(f_ref).max())
        np.testing.assert_allclose(r["f_k"][p], f_ref, rtol=1e-8, atol=1e-8 * scale, err_msg=str(p))
        checked += 1
    assert checked >= 250 and pinned >= 80
    m = pymbar_amd.MBAR(us[-1], Ns[-1])
    assert np.array_equal(r["f_k"][-1], m.f_k) and r["iterations"][-1] == 0
    m.close()


def test_newton_fallback_is_flagged_and_matches_mbar():
    x_n, u_kn, N_k, s_n = ts.harmonic_u_kn(np.array([0.0, 0.5, 3.0]), np.array([1.0, 1.0, 1.0]), [30, 30, 30], seed=4)
    u_kn[2, :60] = np.inf
    u_kn[:2, 60:] = np.inf
    g = ts.config1(seed=0)
    r = pymbar_amd.mbar_batch([g[1], u_kn], [g[2], N_k], compute_uncertainty=False)
    assert list(r["host_fallback"]) == [False, True]
    m = _adaptive_mbar(u_kn, N_k)
    assert np.array_equal(r["f_k"][1], m.f_k)
    m.close()


def test_scale_4096_problems():
    P, K, N = 4096, 12, 20000
    rng = np.random.default_rng(7)
    O_k = np.linspace(0, 2, K)
    K_k = np.linspace(1, 3, K)
    N_k = np.full(K, N // K)
    N_k[: N - N_k.sum()] += 1
    base = ts.harmonic_u_kn(O_k, K_k, N_k, seed=1)[1]
    us = []
    for p in range(P):
        us.append(base + rng.normal(scale=1e-3, size=(K, 1)) * np.arange(K)[:, None])
    r = pymbar_amd.mbar_batch(us, [N_k] * P)
    assert r["success"].all()
    for p in (0, 1234, 4095):
        m = _adaptive_mbar(us[p], N_k)
        d = m.compute_free_energy_differences()
        _assert_delta_f(r["Delta_f"][p], d["Delta_f"], str(p))
        np.testing.assert_allclose(r["dDelta_f"][p], d["dDelta_f"], rtol=1e-7, atol=1e-10)
        m.close()
