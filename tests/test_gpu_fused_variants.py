"""The two forms of the fused sweep up to 128 states (k_fused, mbar_k_fused.hip): the general kernel, which carries the per-sample
multiplicities through the tile, and the one specialised for unit multiplicities, which a context without sample weights runs
(no weights' piece, no multiplications by one, the multipliers of the 4x4x4 steps in registers).  Option ``fused_general`` = 1
forces the general kernel.  Multiplying by 1.0 is exact and nothing else differs -- same grid, same partial records, same order
of every sum -- so the two must agree to the BIT, and a weighted context (bootstrap draw counts) must still agree with the CPU
oracle at the tolerances of tests/test_gpu_parity.py (test_adaptive_solves_above_128_states_match_the_oracle: the same
quantities against the same oracle loop)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import mbar_oracle as oracle  # noqa: E402
from pymbar_amd import testsystems as ts  # noqa: E402

# every panel width NB = ceil(K / 16) of 1 .. 8, with K a multiple of 16 and not; some with states without samples
CASES = [(16, ()), (5, ()), (32, (3,)), (24, ()), (48, ()), (40, (7, 23)), (64, ()), (50, (1, 49)),
         (80, (11,)), (70, ()), (96, ()), (90, (5,)), (112, ()), (100, (17, 18)), (128, (5,)), (120, ())]
# N never a multiple of the 16-sample tile; 53 samples = 4 tiles: one workgroup whose waves get one tile each, 37 = 3 tiles: the
# last wave gets none; 3001 + K: every wave gets several and the tile count is not a multiple of the wave count
SIZES = [37, 53, 3001]


@pytest.fixture(scope="module")
def DM():
    from pymbar_amd.device import DeviceMatrix

    return DeviceMatrix


def problem(K, N, seed, unsampled):
    rng = np.random.RandomState(seed)
    N_k = rng.multinomial(N, np.ones(K) / K) if K > 1 else np.array([N])
    for k in unsampled:
        j = (k + 1) % K
        while j in unsampled:
            j = (j + 1) % K
        N_k[j] += N_k[k]
        N_k[k] = 0
    _, u_kn, N_k, _ = ts.harmonic_u_kn(np.linspace(0.0, 3.0, K), np.linspace(1.0, 2.5, K), N_k, seed=seed)
    return u_kn, N_k


def solve(dm, K, general, **kw):
    dm.set_option("fused_general", general)
    f, r = dm.solve_adaptive(np.zeros(K), history_rows=64, **kw)
    return f, r


def assert_same_bits(a, b, tag):
    (fa, ra), (fb, rb) = a, b
    assert np.all(np.isfinite(fa)), tag
    assert np.array_equal(fa, fb), (tag, np.max(np.abs(fa - fb)))
    assert ra["psum"] is not None and np.array_equal(ra["psum"], rb["psum"]), tag
    for key in ("gnorm", "max_delta", "iterations", "nr_iter", "sci_iter", "success", "gram_sweeps", "light_sweeps", "warm_starts",
                "builds"):
        assert ra[key] == rb[key], (tag, key, ra[key], rb[key])
    assert np.array_equal(ra["history"], rb["history"]), tag


@pytest.mark.parametrize("N0", SIZES)
@pytest.mark.parametrize("K,unsampled", CASES)
def test_unit_weight_kernel_matches_the_general_one_to_the_bit(DM, K, unsampled, N0):
    """Forced adaptive solves (a fixed number of iterations, like the benchmark's) of a context without sample weights, with the
    specialised kernel (default) and with the general one: free energies, per-state sums, stopping statistics, iteration counts
    and the per-iteration history are identical.  Cold solves (the sweep inside the loop), solves with forced self-consistent
    steps (every speculation of those rejected), eager launches and captured graphs, and warm starts on the cached probability matrix (the
    sweep in front of the loop)."""
    N = N0 + (K if N0 > 100 else 0)
    assert N % 16 != 0
    u_kn, N_k = problem(K, N, seed=100 * K + N0, unsampled=unsampled)
    with DM.from_host(u_kn) as dm:
        dm.set_Nk(N_k)
        for k, v in dict(device_loop=1, pmode=1, fused=1, pcache=0).items():
            dm.set_option(k, v)
        for graph, kw in ((1, dict(maxiter=12, min_sc_iter=0, check_convergence=False)),
                          (0, dict(maxiter=12, min_sc_iter=0, check_convergence=False)),
                          (1, dict(maxiter=20, min_sc_iter=3, check_convergence=False)),
                          (1, dict(maxiter=100, min_sc_iter=0, tol=1e-12))):
            dm.set_option("graph", graph)
            unit = solve(dm, K, 0, **kw)
            gen = solve(dm, K, 1, **kw)
            assert_same_bits(unit, gen, f"K={K} N={N} {kw} graph={graph}")
            # which kernel the launcher was given: the specialised one in the first arm, the general one in the second
            assert unit[1]["fused_unit"] == 1 and gen[1]["fused_unit"] == 0, (K, N, unit[1], gen[1])
        dm.set_option("graph", 1)
        # the fused sweep did run, in both forms (its launches are counted by the HIP-event timers)
        dm.set_option("timing", 1)
        for general in (0, 1):
            dm.timing_reset()
            timed = solve(dm, K, general, maxiter=12, min_sc_iter=0, check_convergence=False)
            assert timed[1]["iterations"] == 12 and dm.timing()["fused"][1] > 0, (K, N, general, dm.timing())
        dm.set_option("timing", 0)
        # warm starts: the first solve leaves the probability matrix, the next two start from it with one fused sweep
        dm.set_option("pcache", 1)
        solve(dm, K, 0, maxiter=100, min_sc_iter=0, tol=1e-12)
        f0 = 0.01 * np.cos(np.arange(K))
        f0[0] = 0.0
        warm = []
        for general in (0, 1):
            dm.set_option("fused_general", general)
            warm.append(dm.solve_adaptive(f0, maxiter=8, min_sc_iter=0, check_convergence=False, history_rows=64))
        assert warm[0][1]["warm_starts"] == 1, warm[0][1]
        assert warm[0][1]["fused_unit"] == 1 and warm[1][1]["fused_unit"] == 0, (warm[0][1], warm[1][1])
        assert_same_bits(warm[0], warm[1], f"K={K} N={N} warm start")
        dm.set_option("fused_general", 0)


@pytest.mark.parametrize("K,unsampled", CASES)
def test_unit_weight_kernel_on_a_matrix_whose_padding_columns_are_not_zero(DM, K, unsampled):
    """The two-sweep form of the loop (option fused = 0) builds the probability matrix with k_build_sweep, which normalises the
    zero energies behind the last sample like any other column: the padding of P is then NOT zero.  A fused solve that starts on
    this cached matrix must leave those columns out -- the general kernel does through their multiplicity of zero, the
    specialised one through their reciprocal: identical bits again, and the free energies of the two-sweep solve."""
    N = 3000 + 16 * (K // 16) + 5  # (the last tile holds 5 or 13 samples)
    assert N % 16 != 0
    u_kn, N_k = problem(K, N, seed=100 * K + 11, unsampled=unsampled)
    sws = np.where(N_k > 0)[0]
    with DM.from_host(u_kn) as dm:
        dm.set_Nk(N_k)
        for k, v in dict(device_loop=1, pmode=1, fused=0, pcache=1).items():
            dm.set_option(k, v)
        kw = dict(maxiter=100, min_sc_iter=0, tol=1e-12)
        f_two, r_two = dm.solve_adaptive(np.zeros(K), history_rows=64, **kw)
        assert r_two["success"]
        dm.set_option("fused", 1)
        unit = solve(dm, K, 0, **kw)
        gen = solve(dm, K, 1, **kw)
        assert unit[1]["warm_starts"] == 1 and gen[1]["warm_starts"] == 1, (unit[1], gen[1])  # (on the cached matrix: no rebuild)
        assert_same_bits(unit, gen, f"K={K} N={N} on the two-sweep form's matrix")
        assert r_two["fused_unit"] == 0 and unit[1]["fused_unit"] == 1 and gen[1]["fused_unit"] == 0, (r_two, unit[1], gen[1])
        assert unit[1]["success"] and unit[1]["iterations"] == r_two["iterations"]
        # (tolerance: tests/test_gpu_parity.py, test_adaptive_loop_variants_agree, for the same pair of loop forms)
        np.testing.assert_allclose(unit[0][sws], f_two[sws], rtol=1e-11, atol=1e-11)
        dm.set_option("fused_general", 0)


@pytest.mark.parametrize("K,unsampled", CASES)
def test_weighted_context_still_matches_the_oracle(DM, K, unsampled):
    """A bootstrap replicate (draw counts as per-sample multiplicities on the resident matrix) runs the general kernel whatever the
    option says, and agrees with the oracle's loop on the explicitly gathered columns: free energies, iteration counts and both
    gradient norms of every iteration, at the tolerances tests/test_gpu_parity.py sets for them."""
    N = 3001 + K
    tol = 1e-10
    u_kn, N_k = problem(K, N, seed=100 * K + 7, unsampled=unsampled)
    sws = np.where(N_k > 0)[0]
    Nf = N_k[sws].astype(float)
    rng = np.random.default_rng(K)
    rints = np.zeros(N, dtype=np.int64)
    start = 0
    for n_k in N_k:
        if n_k > 0:
            rints[start:start + n_k] = start + rng.integers(0, n_k, size=n_k)
        start += n_k
    hist = []
    r_or = oracle.adaptive(np.ascontiguousarray(u_kn[:, rints][sws]), Nf, np.zeros(len(sws)), tol=tol, min_sc_iter=0, history=hist)
    assert r_or["success"]
    gn = np.array([[h["gnorm_sci"], h["gnorm_nr"]] for h in hist])
    with DM.from_host(u_kn) as dm:
        dm.set_Nk(N_k)
        for k, v in dict(device_loop=1, pmode=1, fused=1, pcache=0).items():
            dm.set_option(k, v)
        out = []
        for general in (0, 1):
            dm.set_option("fused_general", general)
            dm.set_sample_weights(np.bincount(rints, minlength=N))
            try:
                fa, ra = dm.solve_adaptive(np.zeros(K), tol=tol, maxiter=300, min_sc_iter=0, history_rows=300)
            finally:
                dm.set_sample_weights(None)
            assert ra["success"] and ra["iterations"] == r_or["iterations"], (K, ra["iterations"], r_or["iterations"])
            assert ra["fused_unit"] == 0, ra  # (sample weights: never the specialised kernel)
            np.testing.assert_allclose(fa[sws], r_or["x"], rtol=1e-9, atol=1e-9)
            np.testing.assert_allclose(ra["history"][:, 1:3], gn, rtol=1e-9, atol=1e-8)
            out.append((fa, ra))
        assert_same_bits(out[0], out[1], f"K={K} weighted")  # (the same kernel twice)
        dm.set_option("fused_general", 0)
