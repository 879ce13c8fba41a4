"""Bootstrap replicates of ``pymbar_amd.mbar_batch`` without a GPU: the batch state machine (``mbar_batch_step_host``) driven on a
replicate stated as draw counts over the ORIGINAL columns against the oracle's adaptive loop on the GATHERED columns, the input
rules of the bootstrap arguments (checked before any device work) and the bootstrap ``dDelta_f`` formula."""
import numpy as np
import pytest
from scipy.special import logsumexp

import pymbar_amd
from oracle import mbar_oracle as oracle
from pymbar_amd import _lib
from pymbar_amd import batch
from pymbar_amd.utils import ParameterError

SEED = 20261017


def _weighted_lognum(u_kn, N_k, f, c):
    """log sum_n c_n exp(-logden_n - u_kn): the log-denominator of a sample does not change, samples not drawn carry no term."""
    logden = oracle.log_denominator(u_kn, N_k, f)
    on = c > 0
    return logsumexp((-logden - u_kn)[:, on], b=c[on], axis=1)


def _weighted_gram(u_kn, N_k, f, c):
    p = N_k * oracle.mbar_W_nk(u_kn, N_k, f)
    return (p * c[:, None]).T @ p


def _drive_weighted(u_kn, N_k, f0, c, tol=1e-12):
    K = u_kn.shape[0]
    N_k = np.asarray(N_k, dtype=np.float64)
    st = _lib.BatchState()
    st.K = K
    st.tol, st.gamma, st.maxiter, st.min_sc_iter = tol, 1.0, 10000, 0
    for k in range(K):
        st.Nk[k] = N_k[k]
        st.f[k] = f0[k]
    batch.step_host(st)
    while st.status == batch.RUNNING:
        reqs = [np.array(st.req[r][:K]) for r in range(st.nreq)]
        ln = np.stack([_weighted_lognum(u_kn, N_k, f, c) for f in reqs])
        G = _weighted_gram(u_kn, N_k, reqs[st.gram_req], c) if st.gram_req >= 0 else None
        batch.step_host(st, ln, G)
    return st


@pytest.mark.parametrize("name", ["config1_ho_K5_N5000.npz", "ho_unsampled_K4_N2300.npz", "exp_K20_N1000.npz"])
def test_state_machine_on_a_replicate_equals_the_oracle_on_gathered_columns(golden, name):
    g = golden(name)
    u_kn, N_k = g["u_kn"], np.asarray(g["N_k"])
    K, N = u_kn.shape
    sws = np.where(N_k > 0)[0]
    f_base, _ = oracle.solve_mbar_for_all_states(u_kn, N_k, np.zeros(K), sws, tol=1e-12, min_sc_iter=0)
    for b in range(3):
        draws = batch.bootstrap_indices(SEED, b, N_k)
        assert draws.shape == (N,) and np.array_equal(draws, _lib.bootstrap_draws(SEED, b, np.concatenate(([0], np.cumsum(N_k)))))
        c = np.bincount(draws, minlength=N).astype(np.float64)
        assert c.sum() == N
        f_ref, res = oracle.solve_mbar_once_adaptive(u_kn[sws][:, draws], N_k[sws], f_base[sws], tol=1e-12, min_sc_iter=0)
        st = _drive_weighted(u_kn, N_k, f_base, c)
        assert st.status == batch.DONE and st.success == 1
        assert st.iterations == res["iterations"], (name, b)
        assert abs(st.nr_iter - res["nr_iter"]) <= 1 and st.nr_iter + st.sci_iter == st.iterations
        f = np.array(st.f[:K])
        np.testing.assert_allclose(f[sws], f_ref, rtol=1e-8, atol=1e-9, err_msg=f"{name} replicate {b}")


def test_bootstrap_input_rules():
    u = np.zeros((3, 10))
    N_k = [3, 3, 4]
    with pytest.raises(ParameterError, match="Cannot request bootstrap sampling of free energy differences without any bootstraps."):
        pymbar_amd.mbar_batch([u], [N_k], uncertainty_method="bootstrap")
    with pytest.raises(ParameterError, match="n_bootstraps"):
        pymbar_amd.mbar_batch([u], [N_k], n_bootstraps=1.5)
    with pytest.raises(ParameterError, match="n_bootstraps"):
        pymbar_amd.mbar_batch([u], [N_k], n_bootstraps=-1)
    with pytest.raises(ParameterError, match="bootstrap_seeds"):
        pymbar_amd.mbar_batch([u, u], [N_k, N_k], n_bootstraps=2, bootstrap_seeds=[1, 2, 3])
    with pytest.raises(ParameterError, match="bootstrap_seeds"):
        pymbar_amd.mbar_batch([u], [N_k], n_bootstraps=2, bootstrap_seeds=[0.5])


def test_bootstrap_ddelta_f_formula():
    f = np.array([[0.0, 1.0, 3.0], [0.0, 2.0, 3.0], [0.0, 3.0, 6.0], [0.0, 2.0, 4.0]])
    d = batch.bootstrap_ddelta_f(f)
    assert d.shape == (3, 3) and np.array_equal(d, d.T) and np.all(np.diag(d) == 0.0)
    # d[i, j]: the population standard deviation over the replicates of f_j - f_i
    assert d[0, 1] == pytest.approx(np.sqrt(0.5), rel=1e-15)           # 1, 2, 3, 2
    assert d[0, 2] == pytest.approx(np.sqrt(1.5), rel=1e-15)           # 3, 3, 6, 4
    assert d[1, 2] == pytest.approx(np.sqrt(0.5), rel=1e-15)           # 2, 1, 3, 2
    assert np.all(batch.bootstrap_ddelta_f(f[:1]) == 0.0)
