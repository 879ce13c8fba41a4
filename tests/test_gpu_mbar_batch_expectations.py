"""``pymbar_amd.MBARBatch`` on the device: the extension-row passes of a batch handle against numpy, their determinism, the
reference's fixtures, per-entry equality with the single-problem ``MBAR`` and the host fallback.  Tolerances: those
tests/test_expectations.py holds the single-problem path to for the same quantities (G and wsum 1e-10 relative, lognum 1e-12;
the fixtures 2e-7 / 2e-6; the project's two expectation paths against each other 1e-7 relative, 1e-10 absolute)."""
import itertools

import numpy as np
import pytest
from scipy.special import logsumexp

pytestmark = pytest.mark.gpu

import pymbar_amd  # noqa: E402
from oracle import mbar_oracle as oracle  # noqa: E402
from pymbar_amd import batch  # noqa: E402
from pymbar_amd import testsystems as ts  # noqa: E402
from pymbar_amd.utils import ParameterError  # noqa: E402
from tests.test_mbar_batch_expectations_host import check_against_reference  # noqa: E402

KS, NS = (1, 3, 5, 17, 40, 64), (1, 255, 256, 257, 700, 5000)   # N: both sides of the chunk boundary, several runs of chunks


def _ragged_batch():
    """Every (K, R, N) of K in KS, R in {0, 1, 2, K, 128 - K}, N in NS: random oscillator problems and extension rows with
    scattered +inf entries; in problems of three rows or more the last row is +inf everywhere and the one before it everywhere
    but at one sample."""
    rng = np.random.default_rng(20)
    us, Nks, rows = [], [], []
    for K, N in itertools.product(KS, NS):
        for R in sorted({0, 1, 2, K, 128 - K}):
            x = rng.normal(scale=1.5, size=N)
            O, kk = rng.uniform(-1, 1, size=K), rng.uniform(0.5, 2.0, size=K)
            us.append(0.5 * kk[:, None] * (x[None, :] - O[:, None]) ** 2)
            N_k = rng.multinomial(N, np.full(K, 1.0 / K))
            Nks.append(N_k)
            e = 0.5 * rng.uniform(0.5, 2.0, size=(R, 1)) * (x[None, :] - rng.uniform(-1, 1, size=(R, 1))) ** 2 + rng.normal(size=(R, 1))
            e[rng.random(size=e.shape) < 0.05] = np.inf
            if R >= 3:
                e[R - 1] = np.inf
                e[R - 2] = np.inf
                e[R - 2, rng.integers(N)] = 0.7
            rows.append(e)
    return us, Nks, rows


@pytest.fixture(scope="module")
def ragged():
    us, Nks, rows = _ragged_batch()
    mb = pymbar_amd.MBARBatch(us, Nks, tol=1e-8, maximum_iterations=50)   # (the passes read N_k from the solved states)
    h = mb._h
    rng = np.random.default_rng(21)
    F = mb._F + np.where(mb._F != 0.0, rng.normal(scale=0.2, size=mb._F.shape), 0.0)   # (any finite f, not the solution)
    mask = np.ones(mb.P, dtype=bool)
    h.set_ext(rows)
    lognum = h.ext_lognum(F, mask)
    f_ext = np.where(np.isfinite(lognum), -lognum, 0.0)
    gram, wsum = h.ext_gram(F, f_ext, mask, 0)
    yield dict(mb=mb, h=h, us=us, Nks=Nks, rows=rows, F=F, mask=mask, lognum=lognum, f_ext=f_ext, gram=gram, wsum=wsum)
    mb.close()


def _offsets(h):
    A = h.K + h.R
    return (np.concatenate(([0], np.cumsum(h.R))), np.concatenate(([0], np.cumsum(A * A))), np.concatenate(([0], np.cumsum(A))))


def test_extension_passes_against_numpy(ragged):
    r = ragged
    h, F = r["h"], r["F"]
    roff, goff, woff = _offsets(h)
    assert h.P == len(KS) * len(NS) * 5 - 2 * len(NS)   # (K = 1: R = 1 and R = K are one case; K = 64: R = K and R = 128 - K)
    gw, ww = h.gram_w(F, r["mask"])
    g0 = np.concatenate(([0], np.cumsum(h.K * h.K)))
    n_inf = n_zero = 0
    worst = dict(lognum=0.0, G=0.0, wsum=0.0, gram_w=0.0)
    for p in range(h.P):
        K, R = int(h.K[p]), int(h.R[p])
        u, e, f = r["us"][p], r["rows"][p], F[p, :K]
        ld = oracle.log_denominator(u, r["Nks"][p].astype(np.float64), f)
        with np.errstate(divide="ignore", invalid="ignore"):
            ln_ref = logsumexp(-ld[None, :] - e, axis=1) if R else np.zeros(0)
            Q = np.exp(np.concatenate((f, r["f_ext"][roff[p]:roff[p + 1]]))[:, None] - np.vstack((u, e)) - ld[None, :]).T
        ln = r["lognum"][roff[p]:roff[p + 1]]
        G = r["gram"][goff[p]:goff[p + 1]].reshape(K + R, K + R)
        ws = r["wsum"][woff[p]:woff[p + 1]]
        fin = np.isfinite(ln_ref)
        assert np.array_equal(np.isneginf(ln), np.isneginf(ln_ref)) and not np.any(np.isnan(ln))
        n_inf += int((~fin).sum())
        if fin.any():
            worst["lognum"] = max(worst["lognum"], np.max(np.abs(ln[fin] - ln_ref[fin]) / (1.0 + np.abs(ln_ref[fin]))))
        np.testing.assert_allclose(ln[fin], ln_ref[fin], rtol=1e-12, atol=1e-12, err_msg=f"problem {p}: K={K} R={R} N={u.shape[1]}")
        G_ref, ws_ref = Q.T @ Q, Q.sum(0)
        worst["G"] = max(worst["G"], np.max(np.abs(G - G_ref) / np.maximum(np.abs(G_ref), 1e-300)))
        worst["wsum"] = max(worst["wsum"], np.max(np.abs(ws - ws_ref) / np.maximum(np.abs(ws_ref), 1e-300)))
        np.testing.assert_allclose(G, G_ref, rtol=1e-10, atol=1e-300, err_msg=f"problem {p}: K={K} R={R} N={u.shape[1]}")
        np.testing.assert_allclose(ws, ws_ref, rtol=1e-10, atol=1e-300, err_msg=f"problem {p}: K={K} R={R} N={u.shape[1]}")
        assert np.array_equal(G, G.T), f"problem {p}: G is not bit-symmetric"
        for c in np.where(~fin)[0]:   # (a row of +inf: a zero column of Q)
            assert not G[K + c].any() and not G[:, K + c].any() and ws[K + c] == 0.0
            n_zero += 1
        if R == 0:
            Gw = gw[g0[p]:g0[p + 1]].reshape(K, K)
            worst["gram_w"] = max(worst["gram_w"], np.max(np.abs(G - Gw) / np.maximum(np.abs(Gw), 1e-300)))
            np.testing.assert_allclose(G, Gw, rtol=1e-10, atol=1e-300)
            np.testing.assert_allclose(ws, ww[woff[p] - roff[p]:woff[p] - roff[p] + K], rtol=1e-10)
    print("worst relative deviations:", worst, "rows of -inf:", n_inf)
    assert n_inf == n_zero and n_inf >= 10


def test_extension_passes_are_deterministic(ragged):
    r = ragged
    h, F, mask = r["h"], r["F"], r["mask"]
    roff, goff, woff = _offsets(h)
    # the same calls again
    assert np.array_equal(h.ext_lognum(F, mask), r["lognum"], equal_nan=True)
    gram, wsum = h.ext_gram(F, r["f_ext"], mask, 0)
    assert np.array_equal(gram, r["gram"]) and np.array_equal(wsum, r["wsum"])
    # every problem a group of its own, and groups of a few problems
    for group_bytes in (1, 1 << 20):
        gram, wsum = h.ext_gram(F, r["f_ext"], mask, group_bytes)
        assert np.array_equal(gram, r["gram"]) and np.array_equal(wsum, r["wsum"]), group_bytes
    # masked-out problems are left untouched, the others do not notice
    half = np.arange(h.P) % 2 == 0
    gram, wsum = h.ext_gram(F, r["f_ext"], half, 0)
    ln = h.ext_lognum(F, half)
    for p in range(h.P):
        for got, want, off in ((gram, r["gram"], goff), (wsum, r["wsum"], woff), (ln, r["lognum"], roff)):
            if half[p]:
                assert np.array_equal(got[off[p]:off[p + 1]], want[off[p]:off[p + 1]], equal_nan=True)
            else:
                assert not got[off[p]:off[p + 1]].any()
    # a set of rows that is rejected leaves the earlier set in place
    bad = [None] * h.P
    bad[0] = np.full((1, int(h.N[0])), np.nan)
    with pytest.raises(ParameterError, match="problem 0: extension rows hold NaN"):
        h.set_ext(bad)
    assert np.array_equal(h.R, np.array([len(e) for e in r["rows"]]))
    assert np.array_equal(h.ext_lognum(F, mask), r["lognum"], equal_nan=True)
    # a problem alone: one of every width class of the Gram pass, N = 5000 (five runs of chunks) and N = 257
    picks = [p for p in range(h.P) if (int(h.K[p]), int(h.R[p]), int(h.N[p])) in
             {(3, 3, 5000), (17, 2, 5000), (40, 2, 257), (5, 123, 5000), (64, 64, 5000), (64, 0, 700)}]
    assert len(picks) == 6
    for p in picks:
        K = int(h.K[p])
        with pymbar_amd.MBARBatch([r["us"][p]], [r["Nks"][p]], tol=1e-8, maximum_iterations=50) as one:
            assert not one._h.R.any()
            one._h.set_ext([r["rows"][p]])
            one_mask = np.ones(1, dtype=bool)
            ln = one._h.ext_lognum(F[p:p + 1], one_mask)
            gram, wsum = one._h.ext_gram(F[p:p + 1], r["f_ext"][roff[p]:roff[p + 1]], one_mask, 0)
        assert np.array_equal(ln, r["lognum"][roff[p]:roff[p + 1]], equal_nan=True), (p, K)
        assert np.array_equal(gram, r["gram"][goff[p]:goff[p + 1]]) and np.array_equal(wsum, r["wsum"][woff[p]:woff[p + 1]]), (p, K)


def test_reference_fixtures_on_the_device(golden):
    check_against_reference(golden)


# ---- entry p equals the single-problem path ----
def _oscillator_problems():
    """40 harmonic-oscillator problems with overlapping states: K from 2 to 64, N from 50 to 20000, zero-sample states in some."""
    Ks = [2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15, 16, 17, 18, 20, 22, 24, 26, 28, 30, 31, 32, 33, 34, 36, 38, 40, 42, 44, 46, 48,
          50, 52, 56, 60, 62, 63, 64]
    rng = np.random.default_rng(3)
    out = []
    for i, K in enumerate(Ks):
        N = int(np.exp(rng.uniform(np.log(50), np.log(20000)))) if 0 < i < len(Ks) - 1 else (50 if i == 0 else 20000)
        N_k = np.full(K, N // K)
        N_k[: N - N_k.sum()] += 1
        if i % 4 == 1 and K > 2:   # (a state or two without samples; their samples go to the first state)
            for j in {K // 2, K - 1}:
                N_k[0] += N_k[j]
                N_k[j] = 0
        x_n, u_kn, N_k, _ = ts.harmonic_u_kn(np.linspace(0.0, 2.0, K), np.linspace(1.0, 2.0, K), N_k, seed=100 + i)
        out.append((x_n, u_kn, N_k))
    return out


def _new_states(u_kn):
    K = u_kn.shape[0]
    return u_kn[:min(K, (128 - K) // 2)] * 1.1 + 0.3   # (K + new states + their observables stay within 128 rows)


@pytest.fixture(scope="module")
def oscillators():
    probs = _oscillator_problems()
    proto = (dict(method="adaptive", tol=1e-12, options=dict(min_sc_iter=0, maxiter=10000, gamma=1.0)),)
    singles = [pymbar_amd.MBAR(u, N_k, solver_protocol=proto) for _, u, N_k in probs]
    mb = pymbar_amd.MBARBatch([u for _, u, _ in probs], [N_k for _, _, N_k in probs])
    assert not mb.host_fallback.any() and mb.success.all()
    yield probs, singles, mb
    mb.close()
    for m in singles:
        m.close()


def _assert_entries(got, want_of, singles, what):
    """``got``: the batch method's dict of lists; ``want_of(m, p)``: the single-problem method's dict."""
    worst = 0.0
    for p, m in enumerate(singles):
        want = want_of(m, p)
        assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
        for key in want:
            g, w = np.asarray(got[key][p]), np.asarray(want[key])
            assert g.shape == w.shape, (what, key, p)
            worst = max(worst, float(np.max(np.abs(g - w) / (1e-10 / 1e-7 + np.abs(w)))))
    print(f"{what}: worst deviation relative to 1e-3 + |MBAR's value|: {worst:.3e}")
    for p, m in enumerate(singles):
        want = want_of(m, p)
        for key in want:
            np.testing.assert_allclose(got[key][p], want[key], rtol=1e-7, atol=1e-10, equal_nan=True,
                                       err_msg=f"{what}: problem {p} (K = {m.K}, N = {m.N}) {key}")


def test_free_energy_differences_and_overlap_equal_mbar(oscillators):
    probs, singles, mb = oscillators
    for p, m in enumerate(singles):
        np.testing.assert_allclose(mb.f_k[p], m.f_k, rtol=0, atol=1e-10)
    _assert_entries(mb.compute_free_energy_differences(), lambda m, p: m.compute_free_energy_differences(), singles, "Delta_f")
    got = mb.compute_overlap()
    got["scalar"] = [np.real(s) for s in got["scalar"]]
    got["eigenvalues"] = [np.real(s) for s in got["eigenvalues"]]

    def want(m, p):
        r = m.compute_overlap()
        return dict(scalar=np.real(r["scalar"]), eigenvalues=np.real(r["eigenvalues"]), matrix=r["matrix"])

    _assert_entries(got, want, singles, "overlap")


@pytest.mark.parametrize("observable", ["x", "x2", "cos", "shifted"])
@pytest.mark.parametrize("output", ["averages", "differences"])
def test_expectations_equal_mbar(oscillators, observable, output):
    probs, singles, mb = oscillators
    fn = dict(x=lambda x: x, x2=lambda x: x ** 2, cos=np.cos, shifted=lambda x: x - 1e6)[observable]
    A = [fn(x) for x, _, _ in probs]
    _assert_entries(mb.compute_expectations(A, output=output), lambda m, p: m.compute_expectations(A[p], output=output), singles,
                    f"{observable} {output}")


@pytest.mark.parametrize("output", ["averages", "differences"])
def test_state_dependent_expectations_equal_mbar(oscillators, output):
    probs, singles, mb = oscillators
    A = [np.cos(x)[None, :] * np.linspace(1.0, 2.0, u.shape[0])[:, None] for x, u, _ in probs]
    _assert_entries(mb.compute_expectations(A, output=output, state_dependent=True),
                    lambda m, p: m.compute_expectations(A[p], output=output, state_dependent=True), singles, f"state dependent {output}")


@pytest.mark.parametrize("state_dependent", [False, True])
def test_expectations_at_new_states_equal_mbar(oscillators, state_dependent):
    probs, singles, mb = oscillators
    u_new = [_new_states(u) for _, u, _ in probs]
    A = [x ** 2 for x, _, _ in probs]
    if state_dependent:
        A = [a[None, :] * np.linspace(1.0, 2.0, un.shape[0])[:, None] for a, un in zip(A, u_new)]
    _assert_entries(mb.compute_expectations(A, u_kn_list=u_new, state_dependent=state_dependent),
                    lambda m, p: m.compute_expectations(A[p], u_kn=u_new[p], state_dependent=state_dependent), singles,
                    f"new states, state_dependent={state_dependent}")
    if not state_dependent:
        r = mb.compute_expectations(A, u_kn_list=u_new, compute_uncertainty=False, uncertainty_method="approximate")
        assert sorted(r) == ["mu"]


def test_perturbed_free_energies_equal_mbar(oscillators):
    probs, singles, mb = oscillators
    u_new = [_new_states(u) for _, u, _ in probs]
    _assert_entries(mb.compute_perturbed_free_energies(u_new), lambda m, p: m.compute_perturbed_free_energies(u_new[p]), singles,
                    "perturbed")
    _assert_entries(mb.compute_perturbed_free_energies(u_new, uncertainty_method="approximate"),
                    lambda m, p: m.compute_perturbed_free_energies(u_new[p], uncertainty_method="approximate"), singles,
                    "perturbed, approximate")


def test_entropy_and_enthalpy_equal_mbar(oscillators, monkeypatch):
    probs, singles, mb = oscillators
    got = mb.compute_entropy_and_enthalpy()
    _assert_entries(got, lambda m, p: m.compute_entropy_and_enthalpy(), singles, "entropy and enthalpy")
    # the grouping of the augmented Gram pass does not show in any bit
    monkeypatch.setattr(batch, "EXT_GRAM_GROUP_BYTES", 1 << 16)
    again = mb.compute_entropy_and_enthalpy()
    for key in got:
        for a, b in zip(got[key], again[key]):
            assert np.array_equal(a, b, equal_nan=True), key


def test_fallback_is_flagged_and_matches_mbar():
    x_n, u_kn, N_k, s_n = ts.harmonic_u_kn(np.array([0.0, 0.5, 3.0]), np.array([1.0, 1.0, 1.0]), [30, 30, 30], seed=4)
    u_kn[2, :60] = np.inf
    u_kn[:2, 60:] = np.inf
    g = ts.config1(seed=0)
    proto = (dict(method="adaptive", tol=1e-12, options=dict(min_sc_iter=0, maxiter=10000, gamma=1.0)),)
    with pymbar_amd.MBARBatch([g[1], u_kn], [g[2], N_k]) as mb:
        assert list(mb.host_fallback) == [False, True]
        m = pymbar_amd.MBAR(u_kn, N_k, solver_protocol=proto)
        assert np.array_equal(mb.f_k[1], m.f_k)
        xs = [g[0], x_n]
        u_new = [g[1][:2] * 1.1 + 0.3, np.array([(x_n - 0.2) ** 2, 2.0 * (x_n + 0.1) ** 2])]
        pairs = [
            (mb.compute_free_energy_differences(), m.compute_free_energy_differences()),
            (mb.compute_expectations(xs), m.compute_expectations(x_n)),
            (mb.compute_expectations([x ** 2 for x in xs], output="differences"), m.compute_expectations(x_n ** 2, output="differences")),
            (mb.compute_expectations(xs, u_kn_list=u_new), m.compute_expectations(x_n, u_kn=u_new[1])),
            (mb.compute_perturbed_free_energies(u_new), m.compute_perturbed_free_energies(u_new[1])),
        ]
        for got, want in pairs:
            assert sorted(got) == sorted(want)
            for key in want:
                np.testing.assert_allclose(got[key][1], want[key], rtol=1e-7, atol=1e-10, equal_nan=True, err_msg=key)
        np.testing.assert_allclose(mb.compute_overlap()["matrix"][1], m.compute_overlap()["matrix"], rtol=1e-7, atol=1e-10)
        # the entropy / enthalpy decomposition takes the potentials themselves as observables, and this problem's hold +inf: the
        # batch answers as MBAR does -- with its numbers, or with its error
        try:
            want = m.compute_entropy_and_enthalpy()
        except Exception as exc:  # noqa: BLE001
            with pytest.raises(type(exc)):
                mb.compute_entropy_and_enthalpy()
        else:
            got = mb.compute_entropy_and_enthalpy()
            for key in want:
                np.testing.assert_allclose(got[key][1], want[key], rtol=1e-7, atol=1e-10, equal_nan=True, err_msg=key)
        m.close()
