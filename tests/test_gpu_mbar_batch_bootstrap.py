"""Bootstrap replicates in ``pymbar_amd.mbar_batch`` on the device: every replicate against the single-problem path with the same
draw counts and against the oracle on the gathered columns, the weighted evaluation kernel at the shapes where it can go wrong
(explicit multiplicities through ``mbar_batch_replica_set_weights``) against a long-double statement of ``sum_n c_n (...)``,
bit-for-bit independence of a replicate from the batch and from B, the host fallback, and 4096 replica slots in one call.
Tolerances: those of tests/test_gpu_mbar_batch.py (f_k 1e-8 / 1e-9 against the oracle, 1e-10 against the single-problem path,
dDelta_f 1e-7 relative)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pymbar_amd  # noqa: E402
from oracle import mbar_oracle as oracle  # noqa: E402
from pymbar_amd import _lib, batch, mbar_solvers  # noqa: E402
from pymbar_amd import testsystems as ts  # noqa: E402
from pymbar_amd.device import DeviceMatrix  # noqa: E402

TOL = 1e-12
PROTOCOL = (dict(method="adaptive", tol=TOL, continuation=None, options=dict(min_sc_iter=0, maxiter=10000, gamma=1.0, verbose=False)),)


def _fixture_problems(golden):
    out = []
    for name in ("config1_ho_K5_N5000.npz", "ho_unsampled_K4_N2300.npz", "exp_K20_N1000.npz"):
        g = golden(name)
        out.append((name, g["u_kn"], np.asarray(g["N_k"])))
    x_n, u_kn, N_k, s_n = ts.harmonic_u_kn(np.linspace(1, 5, 50), np.linspace(1, 3, 50), [100] * 50, seed=7)
    out.append(("osc_K50_N5000", u_kn, np.asarray(N_k)))
    return out


def _single_problem_replicate(u_kn, N_k, f_start, seed, b, weights=None):
    """The replicate by hand on the single-problem path: the draw counts on the device, then solve_mbar_for_all_states."""
    sws = np.where(N_k != 0)[0].astype(np.int64)
    cumN = np.concatenate(([0], np.cumsum(N_k))).astype(np.int64)
    results = []
    with DeviceMatrix.from_host(u_kn) as dm:
        if weights is None:
            dm.draw_bootstrap_weights(seed, b, cumN)
        else:
            dm.set_sample_weights(weights)
        f = mbar_solvers.solve_mbar_for_all_states(dm, N_k, f_start.copy(), sws, PROTOCOL, results_out=results)
    return f, results[-1]


def test_each_replicate_equals_the_single_problem_path_and_the_oracle(golden):
    probs = _fixture_problems(golden)
    seeds = [11, 2026, 7, 123456789]
    B = 3
    r = pymbar_amd.mbar_batch([p[1] for p in probs], [p[2] for p in probs], n_bootstraps=B, bootstrap_seeds=seeds,
                              uncertainty_method="bootstrap")
    assert r["success"].all() and r["boot_success"].all() and not r["boot_host_fallback"].any()
    assert np.array_equal(r["bootstrap_seeds"], np.array(seeds, dtype=np.uint64))
    for p, (name, u_kn, N_k) in enumerate(probs):
        K = len(N_k)
        assert r["f_k_boots"][p].shape == (B, K)
        sws = np.where(N_k > 0)[0]
        for b in range(B):
            f_dev, res = _single_problem_replicate(u_kn, N_k, r["f_k"][p], seeds[p], b)
            print(name, b, "iterations", r["boot_iterations"][p, b], res["iterations"],
                  "max |f - single|", np.abs(r["f_k_boots"][p][b] - f_dev).max())
            np.testing.assert_allclose(r["f_k_boots"][p][b], f_dev, rtol=1e-10, atol=1e-10, err_msg=f"{name} {b}")
            assert r["boot_iterations"][p, b] == res["iterations"], (name, b)
            draws = batch.bootstrap_indices(seeds[p], b, N_k)
            f_or, res_or = oracle.solve_mbar_for_all_states(u_kn[:, draws], N_k, r["f_k"][p], sws, tol=TOL, min_sc_iter=0)
            print(name, b, "oracle iterations", res_or["iterations"], "max |f - oracle|", np.abs(r["f_k_boots"][p][b] - f_or).max())
            np.testing.assert_allclose(r["f_k_boots"][p][b], f_or, rtol=1e-8, atol=1e-9, err_msg=f"{name} {b}")
            assert r["boot_iterations"][p, b] == res_or["iterations"], (name, b)
        fb = r["f_k_boots"][p]
        expect = np.std(fb[:, None, :] - fb[:, :, None], axis=0)
        np.testing.assert_allclose(r["dDelta_f"][p], expect, rtol=1e-7, atol=0.0)
    # the other methods: the analytical dDelta_f of the B = 0 call next to the same replicates
    a = pymbar_amd.mbar_batch([p[1] for p in probs], [p[2] for p in probs], n_bootstraps=B, bootstrap_seeds=seeds)
    z = pymbar_amd.mbar_batch([p[1] for p in probs], [p[2] for p in probs])
    for p in range(len(probs)):
        assert np.array_equal(a["dDelta_f"][p], z["dDelta_f"][p]) and np.array_equal(a["f_k_boots"][p], r["f_k_boots"][p])


# ---- the weighted evaluation kernel at its edges ------------------------------------------------------------------------

SHAPE_K = (3, 8, 9, 17, 33, 64)      # every width class (8, 16, 32, 64) and both sides of each boundary
SHAPE_N = (1, 255, 256, 257, 513)    # one sample, one short of / exactly / one past a chunk, three chunks with a short last one
PATTERNS = ("ones", "zero_chunk", "last_column", "thousands")


def _shape_problem(K, N, seed):
    N_k = np.zeros(K, dtype=np.int64)   # state 1 has no samples
    live = [k for k in range(K) if k != 1]
    for i in range(N):
        N_k[live[i % len(live)]] += 1
    x_n, u_kn, N_k, s_n = ts.harmonic_u_kn(np.linspace(0, 2, K), np.linspace(1, 3, K), N_k, seed=seed)
    return np.ascontiguousarray(u_kn), np.asarray(N_k)


def _multiplicities(pattern, N, rng):
    c = rng.integers(0, 4, size=N).astype(np.float64)
    if pattern == "ones":
        c[:] = 1.0
    elif pattern == "zero_chunk":       # a whole chunk of 256 samples not drawn (every sample, when there is one chunk only)
        c[:256] = 0.0
    elif pattern == "last_column":      # the first chunk's only drawn sample is its last column
        last = min(255, N - 1)
        c[:256] = 0.0
        c[last] = 2.0
    elif pattern == "thousands":
        c[rng.integers(0, N, size=max(1, N // 7))] = 1000.0
    return c


def _long_double_sums(u_kn, N_k, f, c):
    """lognum_k = log sum_n c_n exp(-logden_n - u_kn), wsum_k = sum_n c_n W_nk and gram = sum_n c_n W_ni W_nj in long double."""
    L = np.longdouble
    u, fl, cl = u_kn.astype(L), f.astype(L), c.astype(L)
    on = N_k > 0
    t = (fl[on, None] + np.log(N_k[on].astype(L))[:, None]) - u[on]
    m = t.max(axis=0)
    ld = m + np.log(np.exp(t - m).sum(axis=0))
    with np.errstate(divide="ignore"):
        lognum = np.log((cl[None, :] * np.exp(-ld[None, :] - u)).sum(axis=1))
    W = np.exp(fl[:, None] - u - ld[None, :])
    return lognum, (cl[None, :] * W).sum(axis=1), (cl[None, :] * W) @ W.T


@pytest.fixture(scope="module")
def shape_run():
    """Every (K, N) problem in one device batch, one replica slot per multiplicity pattern: the slots' per-state log sums (a solve
    that takes no iteration evaluates them at the start) and their covariance inputs at the same f; likewise the problems' own,
    once before the slots exist, again after the slots' calls, and once more after the slots are released."""
    rng = np.random.default_rng(31)
    probs = [_shape_problem(K, N, seed=100 + i) for i, (K, N) in enumerate((K, N) for K in SHAPE_K for N in SHAPE_N)]
    blocks = [p[0] for p in probs]
    Nks = [p[1] for p in probs]
    P = len(probs)
    fs = []
    for u, N_k in probs:
        f = rng.normal(scale=0.3, size=len(N_k))
        f[0] = 0.0
        fs.append(f)
    slots = [(p, pat) for p in range(P) for pat in PATTERNS]
    base = np.array([p for p, _ in slots], dtype=np.int64)
    cs = [_multiplicities(pat, blocks[p].shape[1], rng) for p, pat in slots]

    def states_for(idx):
        st = (_lib.BatchState * len(idx))()
        sv = batch._states_view(st)
        sv["tol"], sv["gamma"], sv["maxiter"], sv["min_sc_iter"] = TOL, 1.0, 0, 0
        F = np.zeros((len(idx), batch.MAX_K))
        for i, p in enumerate(idx):
            K = len(Nks[p])
            sv["K"][i] = K
            sv["Nk"][i, :K] = Nks[p]
            sv["f"][i, :K] = fs[p]
            F[i, :K] = fs[p]
        return st, F

    def problems_run(h):
        st, F = states_for(range(P))
        h.solve(st)
        return (batch._states_view(st)["lognum"].copy(),) + h.gram_w(F, np.ones(P, dtype=bool))

    with batch.DeviceBatch(blocks) as h:
        base_lognum, base_gram, base_wsum = problems_run(h)
        h.set_replicas(base, Nks)
        for s, c in enumerate(cs):
            h.replica_set_weights(s, c)
        with pytest.raises(pymbar_amd.utils.ParameterError, match="finite and >= 0"):
            h.replica_set_weights(0, np.full(blocks[0].shape[1], -1.0))
        st, F = states_for(base)
        h.replicas_solve(st)
        sv = batch._states_view(st)
        assert (sv["status"] == batch.DONE).all() and (sv["iterations"] == 0).all()
        lognum = sv["lognum"].copy()
        gram, wsum = h.replicas_gram_w(F, np.ones(len(slots), dtype=bool))
        repeats = [problems_run(h)]
        h.set_replicas(np.zeros(0, dtype=np.int64), Nks)
        repeats.append(problems_run(h))
    return dict(probs=probs, fs=fs, slots=slots, cs=cs, lognum=lognum, gram=gram, wsum=wsum, base_lognum=base_lognum,
                base_gram=base_gram, base_wsum=base_wsum, repeats=repeats)


def _unpack(Ks, gram, wsum):
    goff = np.concatenate(([0], np.cumsum(Ks * Ks)))
    woff = np.concatenate(([0], np.cumsum(Ks)))
    return [(gram[goff[i]:goff[i + 1]].reshape(Ks[i], Ks[i]), wsum[woff[i]:woff[i + 1]]) for i in range(len(Ks))]


def test_weighted_sums_at_the_edges_match_long_double(shape_run):
    """Bound: a sum of at most 513 positive terms, each an exp of an argument of magnitude < 200 built from a K <= 64 term
    log-sum-exp, carries at most (513 + 64 + 3 * 200 + 10) eps = 2.6e-13 of relative error, a Gram entry (products of two such
    factors) twice that: 1e-12 relative for the sums, 1e-12 absolute for their logarithms (plus eps of the logarithm itself)."""
    d = shape_run
    Ks = np.array([len(d["probs"][p][1]) for p, _ in d["slots"]], dtype=np.int64)
    for s, ((p, pat), (G, ws)) in enumerate(zip(d["slots"], _unpack(Ks, d["gram"], d["wsum"]))):
        u_kn, N_k = d["probs"][p]
        assert np.abs(u_kn).max() < 150.0 and np.abs(d["fs"][p]).max() < 50.0
        K, N = u_kn.shape
        what = f"K={K} N={N} {pat}"
        ln_ref, ws_ref, G_ref = _long_double_sums(u_kn, N_k, d["fs"][p], d["cs"][s])
        ln = d["lognum"][s, :K]
        assert np.array_equal(G, G.T), what
        if d["cs"][s].sum() == 0:       # nothing drawn: every chunk writes (-inf, 0)
            assert np.all(ln == -np.inf) and np.all(ws == 0.0) and np.all(G == 0.0), what
            continue
        err = np.abs(ln - ln_ref.astype(np.float64))
        assert err.max() <= 1e-12 + 4 * np.finfo(float).eps * np.abs(ln).max(), (what, err.max())
        np.testing.assert_allclose(ws, ws_ref.astype(np.float64), rtol=1e-12, atol=0.0, err_msg=what)
        np.testing.assert_allclose(G, G_ref.astype(np.float64), rtol=1e-12, atol=0.0, err_msg=what)


def test_unit_multiplicities_reproduce_the_unweighted_kernel(shape_run):
    d = shape_run
    P = len(d["probs"])
    Kp = np.array([len(p[1]) for p in d["probs"]], dtype=np.int64)
    Ks = np.array([len(d["probs"][p][1]) for p, _ in d["slots"]], dtype=np.int64)
    slots = _unpack(Ks, d["gram"], d["wsum"])
    plain = _unpack(Kp, d["base_gram"], d["base_wsum"])
    seen = 0
    for s, (p, pat) in enumerate(d["slots"]):
        if pat != "ones":
            continue
        K = Kp[p]
        np.testing.assert_allclose(d["lognum"][s, :K], d["base_lognum"][p, :K], rtol=1e-13, atol=0.0)
        np.testing.assert_allclose(slots[s][0], plain[p][0], rtol=1e-13, atol=0.0)
        np.testing.assert_allclose(slots[s][1], plain[p][1], rtol=1e-13, atol=0.0)
        seen += 1
    assert seen == P


def test_problems_and_slots_stay_apart_when_their_calls_interleave(shape_run):
    """The problems' records, states and outputs are their own: the same bits after the slots' solve and covariance pass, and
    after the slots are released."""
    d = shape_run
    for lognum, gram, wsum in d["repeats"]:
        assert np.array_equal(lognum, d["base_lognum"])
        assert np.array_equal(gram, d["base_gram"])
        assert np.array_equal(wsum, d["base_wsum"])


# ---- bits ----------------------------------------------------------------------------------------------------------------

def test_replicate_bits_depend_on_nothing_but_the_replicate(golden):
    probs = _fixture_problems(golden)[:3]
    us = [p[1] for p in probs] * 2
    Ns = [p[2] for p in probs] * 2
    seeds = [5, 6, 7, 8, 9, 10]
    a = pymbar_amd.mbar_batch(us, Ns, n_bootstraps=4, bootstrap_seeds=seeds, compute_uncertainty=False)
    b = pymbar_amd.mbar_batch(us, Ns, n_bootstraps=4, bootstrap_seeds=seeds, compute_uncertainty=False)
    z = pymbar_amd.mbar_batch(us, Ns, compute_uncertainty=False)
    for p in range(6):
        assert np.array_equal(a["f_k_boots"][p], b["f_k_boots"][p])
        assert np.array_equal(a["f_k"][p], z["f_k"][p]) and a["iterations"][p] == z["iterations"][p]
    assert np.array_equal(a["boot_iterations"], b["boot_iterations"])
    for p in (1, 5):
        alone = pymbar_amd.mbar_batch([us[p]], [Ns[p]], n_bootstraps=4, bootstrap_seeds=[seeds[p]], compute_uncertainty=False)
        assert np.array_equal(alone["f_k_boots"][0], a["f_k_boots"][p])
        fewer = pymbar_amd.mbar_batch([us[p]], [Ns[p]], n_bootstraps=2, bootstrap_seeds=[seeds[p]], compute_uncertainty=False)
        assert np.array_equal(fewer["f_k_boots"][0], a["f_k_boots"][p][:2])
    # rseed pins the seeds; the seeds that come back reproduce the call
    c = pymbar_amd.mbar_batch(us[:2], Ns[:2], n_bootstraps=2, rseed=3, compute_uncertainty=False)
    e = pymbar_amd.mbar_batch(us[:2], Ns[:2], n_bootstraps=2, bootstrap_seeds=c["bootstrap_seeds"], compute_uncertainty=False)
    assert np.array_equal(c["f_k_boots"][1], e["f_k_boots"][1])


def test_small_groups_give_the_same_bits(golden, monkeypatch):
    probs = _fixture_problems(golden)[:3]
    us, Ns = [p[1] for p in probs], [p[2] for p in probs]
    a = pymbar_amd.mbar_batch(us, Ns, n_bootstraps=3, bootstrap_seeds=[1, 2, 3], compute_uncertainty=False)
    monkeypatch.setattr(batch, "BOOTSTRAP_GROUP_BYTES", 100_000)   # two slots of config1, a few of the others
    b = pymbar_amd.mbar_batch(us, Ns, n_bootstraps=3, bootstrap_seeds=[1, 2, 3], compute_uncertainty=False)
    for p in range(3):
        assert np.array_equal(a["f_k_boots"][p], b["f_k_boots"][p])


# ---- fallback ------------------------------------------------------------------------------------------------------------

def test_replicates_of_a_singular_problem_take_the_host_path():
    x_n, u_kn, N_k, s_n = ts.harmonic_u_kn(np.array([0.0, 0.5, 3.0]), np.array([1.0, 1.0, 1.0]), [30, 30, 30], seed=4)
    u_kn[2, :60] = np.inf
    u_kn[:2, 60:] = np.inf
    N_k = np.asarray(N_k)
    g = ts.config1(seed=0)
    r = pymbar_amd.mbar_batch([g[1], u_kn], [g[2], N_k], n_bootstraps=2, bootstrap_seeds=[4, 5], compute_uncertainty=False)
    assert list(r["host_fallback"]) == [False, True]
    assert not r["boot_host_fallback"][0].any() and r["boot_host_fallback"][1].all()
    for b in range(2):
        c = np.bincount(batch.bootstrap_indices(5, b, N_k), minlength=u_kn.shape[1])
        f, res = _single_problem_replicate(u_kn, N_k, r["f_k"][1], 5, b, weights=c)
        assert np.array_equal(r["f_k_boots"][1][b], f)
    alone = pymbar_amd.mbar_batch([g[1]], [g[2]], n_bootstraps=2, bootstrap_seeds=[4], compute_uncertainty=False)
    assert np.array_equal(alone["f_k_boots"][0], r["f_k_boots"][0]) and np.array_equal(alone["f_k"][0], r["f_k"][0])


# ---- size ----------------------------------------------------------------------------------------------------------------

def test_scale_4096_replica_slots():
    P, K, N, B = 512, 12, 2000, 8
    rng = np.random.default_rng(7)
    N_k = np.full(K, N // K)
    N_k[: N - N_k.sum()] += 1
    base = ts.harmonic_u_kn(np.linspace(0, 2, K), np.linspace(1, 3, K), N_k, seed=1)[1]
    us = [base + rng.normal(scale=1e-3, size=(K, 1)) * np.arange(K)[:, None] for p in range(P)]
    r = pymbar_amd.mbar_batch(us, [N_k] * P, n_bootstraps=B, rseed=12, uncertainty_method="bootstrap")
    assert r["success"].all() and r["boot_success"].all() and not r["boot_host_fallback"].any()
    assert len(r["f_k_boots"]) == P and r["f_k_boots"][0].shape == (B, K) and r["dDelta_f"][P - 1].shape == (K, K)
    sws = np.arange(K)
    for s in rng.choice(P * B, size=5, replace=False):
        p, b = divmod(int(s), B)
        draws = batch.bootstrap_indices(int(r["bootstrap_seeds"][p]), b, N_k)
        f_or, res = oracle.solve_mbar_for_all_states(us[p][:, draws], N_k, r["f_k"][p], sws, tol=TOL, min_sc_iter=0)
        np.testing.assert_allclose(r["f_k_boots"][p][b], f_or, rtol=1e-8, atol=1e-9, err_msg=f"{p} {b}")
