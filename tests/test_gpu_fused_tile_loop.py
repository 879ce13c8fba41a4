"""The tile loop of the fused sweep (k_fused, mbar_k_fused.hip) runs two tiles per trip -- buffer 0, then buffer 1 of a wave's pair,
so that every LDS address is a lane register plus an immediate -- and a wave with an odd number of tiles enters its first trip at
the second half.  What that can get wrong is a matter of how many tiles a wave has, so the grid is forced down to ONE workgroup
(option ``grid_blocks`` = 1: four waves) and N is chosen so that the waves get 0, 1, 2, 3, 4, 5 and 6 tiles, with a ragged last
tile on either parity and a wave whose stream ends one tile before its neighbour's:

    N     tiles   per wave          last tile
    1       1     1 0 0 0           1 sample
    15      1     1 0 0 0           15
    16      1     1 0 0 0           full
    17      2     1 1 0 0           1
    63      4     1 1 1 1           15
    64      4     1 1 1 1           full
    65      5     2 1 1 1           1
    128     8     2 2 2 2           full
    129     9     3 2 2 2           1
    192    12     3 3 3 3           full
    200    13     4 3 3 3           8
    319    20     5 5 5 5           15
    321    21     6 5 5 5           1

K = 16, 40, 128 are panels of 1, 3 and 8 blocks: accumulators the compiler places, and (8) pinned by hand.  Every case is three
forced adaptive iterations from f = 0 on a harmonic ladder.  The oracle's loop is the yardstick, at the tolerances
tests/test_gpu_parity.py sets for an adaptive solve against it (test_adaptive_solves_above_128_states_match_the_oracle: free
energies rtol = atol = 1e-9, the two gradient norms of every iteration rtol = 1e-9, atol = 1e-8).

The WIDE instantiations (64-bit lane offsets, a row pitch of 7.6e7 samples and more) are out of reach of a small case: only
test_gpu_parity.py's test_wide_row_pitch_matches_sum_of_shards runs them."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import mbar_oracle as oracle  # noqa: E402
from pymbar_amd import testsystems as ts  # noqa: E402

KS = [16, 40, 128]
NS = [1, 15, 16, 17, 63, 64, 65, 128, 129, 192, 200, 16 * 4 * 5 - 1, 16 * 4 * 5 + 1]
ITERATIONS = 3
F_TOL = dict(rtol=1e-9, atol=1e-9)        # tests/test_gpu_parity.py:470
GNORM_TOL = dict(rtol=1e-9, atol=1e-8)    # tests/test_gpu_parity.py:472


@functools.lru_cache(maxsize=None)
def problem(K, N):
    """A harmonic ladder of K states with N samples in all (states without samples where N is small), a bootstrap replicate of
    it (draws WITHIN each state; draw counts with zeros), and the oracle's three iterations on both."""
    rng = np.random.RandomState(1000 * K + N)
    N_k = rng.multinomial(N, np.ones(K) / K)
    O_k, K_k = ts.ladder_params(K)
    _, u_kn, N_k, _ = ts.harmonic_u_kn(O_k, K_k, N_k, seed=1000 * K + N)
    sws = np.where(N_k > 0)[0]
    rints = np.zeros(N, dtype=np.int64)
    start = 0
    for n_k in N_k:
        if n_k > 0:
            rints[start:start + n_k] = start + rng.randint(0, n_k, size=n_k)
        start += n_k
    c_n = np.bincount(rints, minlength=N).astype(np.float64)

    def reference(u):
        if len(sws) == 1:  # (one sampled state: f = 0 by the gauge, and the oracle's stopping measure is a maximum over nothing)
            return np.zeros(1), None
        hist = []
        r = oracle.adaptive(np.ascontiguousarray(u[sws]), N_k[sws].astype(float), np.zeros(len(sws)), tol=1e-30,
                            maxiter=ITERATIONS, min_sc_iter=0, history=hist)
        assert r["iterations"] == ITERATIONS
        return r["x"], np.array([[h["gnorm_sci"], h["gnorm_nr"]] for h in hist])

    for a in (u_kn, N_k, sws, c_n):
        a.setflags(write=False)
    return dict(u_kn=u_kn, N_k=N_k, sws=sws, c_n=c_n, plain=reference(u_kn), boot=reference(u_kn[:, rints]))


@functools.lru_cache(maxsize=None)
def device_runs(K, N):
    """The case's solves on the device, once: unit-weight form and general form on one workgroup, the unit-weight form on the
    default grid, and the bootstrap replicate (general form) on one workgroup."""
    from pymbar_amd.device import DeviceMatrix

    p = problem(K, N)
    kw = dict(maxiter=ITERATIONS, min_sc_iter=0, check_convergence=False, history_rows=ITERATIONS)
    out = {}
    with DeviceMatrix.from_host(p["u_kn"]) as dm:
        dm.set_Nk(p["N_k"])
        for k, v in dict(device_loop=1, pmode=1, fused=1, pcache=0).items():
            dm.set_option(k, v)
        try:
            dm.set_option("grid_blocks", 1)
            for name, general in (("unit", 0), ("general", 1)):
                dm.set_option("fused_general", general)
                out[name] = dm.solve_adaptive(np.zeros(K), **kw)
            dm.set_option("fused_general", 1)
            dm.set_sample_weights(p["c_n"])
            try:
                out["boot"] = dm.solve_adaptive(np.zeros(K), **kw)
            finally:
                dm.set_sample_weights(None)
            dm.set_option("fused_general", 0)
            dm.set_option("grid_blocks", 0)
            out["unit, default grid"] = dm.solve_adaptive(np.zeros(K), **kw)
        finally:
            dm.set_option("fused_general", 0)
            dm.set_option("grid_blocks", 0)
    return out


def assert_matches_oracle(run, ref, sws, tag):
    (f, r), (x, gn) = run, ref
    assert r["iterations"] == ITERATIONS, (tag, r)
    assert np.all(np.isfinite(f[sws])), tag
    print(tag, "max |f - f_oracle| =", np.max(np.abs(f[sws] - x)))
    np.testing.assert_allclose(f[sws], x, err_msg=tag, **F_TOL)
    if gn is not None:
        print(tag, "max |gnorm - gnorm_oracle| =", np.max(np.abs(r["history"][:, 1:3] - gn)))
        np.testing.assert_allclose(r["history"][:, 1:3], gn, err_msg=tag, **GNORM_TOL)


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_unit_weight_form_equals_the_general_form_to_the_bit(K, N):
    """Same grid, same partial records, same order of every sum, and x * 1.0 is exact: f, the per-state sums, the gradient norm
    and the last relative change are the same bits -- also with the broadcast of the first candidate's reciprocal inside the
    unit-weight form's fused multiply-add, and with the reciprocals of a ragged tile zeroed through the 32-bit sample count."""
    runs = device_runs(K, N)
    (fu, ru), (fg, rg) = runs["unit"], runs["general"]
    assert ru["fused_unit"] == 1 and rg["fused_unit"] == 0, (ru, rg)  # (which kernel the launcher was given)
    assert np.all(np.isfinite(fu))
    assert np.array_equal(fu, fg), np.max(np.abs(fu - fg))
    assert ru["psum"] is not None and np.array_equal(ru["psum"], rg["psum"])
    assert ru["gnorm"] == rg["gnorm"] and ru["max_delta"] == rg["max_delta"], (ru, rg)
    assert np.array_equal(ru["history"], rg["history"])


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_both_forms_match_the_oracle(K, N):
    """(Two forms broken alike would agree with each other.)"""
    p, runs = problem(K, N), device_runs(K, N)
    for name in ("unit", "general"):
        assert_matches_oracle(runs[name], p["plain"], p["sws"], f"K={K} N={N} {name}")


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_weighted_context_matches_the_oracle_on_the_gathered_replicate(K, N):
    """Bootstrap draw counts (with zeros) as per-sample multiplicities on the resident matrix: the general form, against the
    oracle's loop on the explicitly gathered columns."""
    p, runs = problem(K, N), device_runs(K, N)
    assert runs["boot"][1]["fused_unit"] == 0, runs["boot"][1]
    assert_matches_oracle(runs["boot"], p["boot"], p["sws"], f"K={K} N={N} bootstrap replicate")


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("K", KS)
def test_result_does_not_depend_on_the_grid(K, N):
    """The default grid (a workgroup for every four tiles, up to the device's size) against one workgroup: another order of the
    sums, so not the same bits -- the oracle's tolerance between the two, and the oracle itself for the default grid."""
    p, runs = problem(K, N), device_runs(K, N)
    (f1, r1), (fd, rd) = runs["unit"], runs["unit, default grid"]
    assert rd["fused_unit"] == 1 and rd["iterations"] == ITERATIONS, rd
    sws = p["sws"]
    np.testing.assert_allclose(fd[sws], f1[sws], **F_TOL)
    np.testing.assert_allclose(rd["history"][:, 1:3], r1["history"][:, 1:3], **GNORM_TOL)
    assert_matches_oracle(runs["unit, default grid"], p["plain"], sws, f"K={K} N={N} default grid")
