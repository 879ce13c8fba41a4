"""``mbar_batch``: many independent small MBAR problems solved in one device call (INTEGRATION.md
section 7).

Entry p of the result is what ``MBAR(u_kn_list[p], N_k_list[p], initial_f_k=..., solver_protocol=(dict(method="adaptive",
tol=tol, options=dict(min_sc_iter=..., maxiter=..., gamma=...)),))`` followed by ``compute_free_energy_differences()`` gives:
the same iteration count and Newton / self-consistent choices, ``f_k`` within the tolerance of the solve, and unsampled
states filled in as ``solve_mbar_for_all_states`` does.  The adaptive loops of all problems run on the device
(``csrc/mbar_k_batch.hip``); the host reads one status int per problem between groups of passes.  A problem whose Newton system
has a pivot that counts as zero is finished on the host by the single-problem path and flagged in ``host_fallback``.

With ``n_bootstraps = B`` every problem's B bootstrap replicates are solved in the same call: a replicate is a replica slot of the
device batch -- the problem's resident block with per-sample draw counts, drawn on the device from the counter-based stream of
``MBAR(bootstrap_rng="device")`` -- started from the problem's solved ``f_k``; nothing is gathered and no block is copied.
"""
import ctypes as C
import logging
import os
import time

import numpy as np

from . import _lib
from .utils import ParameterError, check_w_sums

logger = logging.getLogger(__name__)

MAX_K = _lib.MBAR_BATCH_MAX_K
RUNNING, DONE, FALLBACK = 0, 1, 2
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int64)
# Device memory one group of replica slots may take for its multiplicities (8 N bytes per slot), chunk records and states
BOOTSTRAP_GROUP_BYTES = 2 << 30


def _check_inputs(rc):
    """MBAR_ERR_ARG is about the inputs (NaN / -inf entries, a batch larger than the device, bad weights): a ParameterError."""
    if rc == -1:
        raise ParameterError(_lib.last_error(None))
    _lib.check(rc)


class DeviceBatch(_lib.Handle):
    """P problems' reduced potentials resident on one device (``mbar_batch_*`` of include/mbar_hip.h)."""

    _destroy = "mbar_batch_destroy"

    def __init__(self, blocks, device=None):
        self._lib = _lib.load_library()
        _lib.require_device()
        self.device = _lib.default_device(device)
        self.P = len(blocks)
        self.K = np.array([b.shape[0] for b in blocks], dtype=np.int64)
        self.N = np.array([b.shape[1] for b in blocks], dtype=np.int64)
        ptrs = (_dp * self.P)(*[b.ctypes.data_as(_dp) for b in blocks])
        h = C.c_void_p()
        _check_inputs(self._lib.mbar_batch_create(C.byref(h), self.device, self.P, _lib.ptr(self.K, _ip), _lib.ptr(self.N, _ip), ptrs))
        self._h = h

    # The problems and the replica slots are two sets of solves over the same blocks: `fn` is the set's entry point, Ks its widths
    def _solve(self, fn, states):
        passes = C.c_int64(0)
        _lib.check(fn(self._h, states, C.byref(passes)))
        return passes.value

    def _gram_w(self, fn, Ks, F, mask):
        F = np.ascontiguousarray(F, dtype=np.float64)
        mask = np.ascontiguousarray(mask, dtype=np.int32)
        gram = np.zeros(int(np.sum(Ks * Ks)), dtype=np.float64)
        wsum = np.zeros(int(np.sum(Ks)), dtype=np.float64)
        _lib.check(fn(self._h, _lib.ptr(F), mask.ctypes.data_as(C.POINTER(C.c_int32)), _lib.ptr(gram), _lib.ptr(wsum)))
        return gram, wsum

    def solve(self, states):
        return self._solve(self._lib.mbar_batch_solve, states)

    def gram_w(self, F, mask):
        """Packed ``W^T W`` and ``sum_n W_nk`` at ``F[p, :K[p]]`` for the problems with ``mask[p]``."""
        return self._gram_w(self._lib.mbar_batch_gram_w, self.K, F, mask)

    # ---- replica slots (bootstrap replicates) ----
    def set_replicas(self, base, N_k_list):
        """Declares ``len(base)`` replica slots: slot s shares problem ``base[s]``'s block; ``N_k_list[p]`` (every problem's samples
        per state) fixes the layout of the draws.  An empty ``base`` releases the slots."""
        base = np.ascontiguousarray(base, dtype=np.int64)
        Nk = np.zeros((self.P, MAX_K), dtype=np.int64)
        for p in range(self.P):
            Nk[p, :self.K[p]] = N_k_list[p]
        _check_inputs(self._lib.mbar_batch_set_replicas(self._h, len(base), _lib.ptr(base, _ip), _lib.ptr(Nk, _ip)))
        self.base = base

    def replica_set_weights(self, slot, c_n):
        """Slot ``slot``'s per-sample multiplicities from a host vector (finite, >= 0)."""
        c_n = np.ascontiguousarray(c_n, dtype=np.float64)
        if c_n.shape != (int(self.N[self.base[slot]]),):
            raise ValueError(f"sample weights must have shape ({int(self.N[self.base[slot]])},)")
        _check_inputs(self._lib.mbar_batch_replica_set_weights(self._h, int(slot), _lib.ptr(c_n)))

    def replicas_draw(self, first, seeds, replicates):
        """Draw counts of the slots ``first .. first + len(seeds)`` on the device: replicate ``replicates[i]`` of stream ``seeds[i]``."""
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
        replicates = np.ascontiguousarray(replicates, dtype=np.int64)
        _lib.check(self._lib.mbar_batch_replicas_draw(self._h, int(first), len(seeds), seeds.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                      _lib.ptr(replicates, _ip)))

    def replicas_solve(self, states):
        return self._solve(self._lib.mbar_batch_replicas_solve, states)

    def replicas_gram_w(self, F, mask):
        """``gram_w`` of the slots: packed ``sum_n c_n W_ni W_nj`` and ``sum_n c_n W_nk`` at ``F[s, :K]``."""
        return self._gram_w(self._lib.mbar_batch_replicas_gram_w, self.K[self.base], F, mask)


def bootstrap_indices(seed, b, N_k):
    """The resampled sample indices of replicate ``b`` of the stream ``seed`` over the default layout (the states' runs in order):
    the reference's ``bootstrap_rints`` row, and the draws whose counts the device uses (``_lib.bootstrap_draws``; no GPU)."""
    cumN = np.concatenate(([0], np.cumsum(np.asarray(N_k, dtype=np.int64)))).astype(np.int64)
    return _lib.bootstrap_draws(seed, b, cumN)


def bootstrap_ddelta_f(f_k_boots):
    """``dDelta_f`` of ``MBAR.compute_free_energy_differences(uncertainty_method="bootstrap")`` from the (B, K) replicates."""
    f_k_boots = np.asarray(f_k_boots, dtype=np.float64)
    diffm = f_k_boots[:, np.newaxis, :] - f_k_boots[:, :, np.newaxis]
    return np.std(diffm, axis=0)


def _states_view(states):
    """A structured numpy view of a ctypes array of ``BatchState`` (no copy)."""
    return np.ctypeslib.as_array(states)


def _new_states(prob, Ks, Nks, fs, settings):
    """A ``BatchState`` array for one solve of a set: entry e is problem ``prob[e]``'s (ascending), with its K, N_k and start
    ``fs[prob[e]]``; ``settings``: tol, gamma, maxiter, min_sc_iter."""
    n = len(prob)
    states = (_lib.BatchState * n)()
    sv = _states_view(states)
    sv["K"] = Ks[prob]
    sv["tol"], sv["gamma"], sv["maxiter"], sv["min_sc_iter"] = settings
    cuts = np.concatenate(([0], np.flatnonzero(np.diff(prob)) + 1, [n]))  # (the entries of one problem are consecutive)
    for e0, e1 in zip(cuts[:-1], cuts[1:]):
        p = prob[e0]
        K = int(Ks[p])
        sv["Nk"][e0:e1, :K] = Nks[p]
        sv["f"][e0:e1, :K] = fs[p]
    return states


def _all_states_update(sv):
    """The all-state update of ``solve_mbar_for_all_states`` (mbar_solvers.py) on every entry of a solved state array: every
    state sampled -- f - log(psum / N_k) with the per-state sums at the solution; otherwise -lognum over all states; then
    f_0 = 0.  Returns (len(sv), MAX_K); row e is meaningful in its first K[e] columns."""
    cols = np.arange(MAX_K)[None, :] < sv["K"][:, None]
    Nk = np.where(cols, sv["Nk"], 1.0)
    sampled = np.all(Nk > 0, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        f_all = np.where(sampled[:, None], sv["f"] - np.log(np.where(cols, sv["psum"], 1.0) / Nk), -1.0 * sv["lognum"])
    return f_all - f_all[:, :1]


def step_host(state, lognum=None, gram=None):
    """One step of the batch state machine on the host (``mbar_batch_step_host``; no GPU): ``lognum`` (nreq, K) at the last
    pass's requests, ``gram`` (K, K) at ``req[gram_req]``.  Returns the status."""
    lib = _lib.load_library()
    K = int(state.K)
    ln = None if lognum is None else np.ascontiguousarray(np.asarray(lognum, dtype=np.float64).reshape(-1, K))
    g = None if gram is None else np.ascontiguousarray(np.asarray(gram, dtype=np.float64).reshape(K, K))
    rc = lib.mbar_batch_step_host(C.byref(state), _lib.ptr(ln), _lib.ptr(g))
    if rc < 0:
        raise _lib.MbarHipError(rc, _lib.last_error(None))
    return rc


def _check_problem(p, u_kn, N_k, f_init):
    from .mbar_solvers import validate_inputs

    u = np.ascontiguousarray(u_kn, dtype=np.float64)
    if u.ndim != 2:
        raise ParameterError(f"problem {p}: u_kn must be a K x N array")
    K, N = u.shape
    if not 1 <= K <= MAX_K:
        raise ParameterError(f"problem {p}: K = {K} states; mbar_batch handles 1 .. {MAX_K} (use MBAR for larger problems)")
    if N < 1:
        raise ParameterError(f"problem {p}: u_kn has no samples")
    N_k = np.array(N_k, dtype=np.int64)
    if N_k.shape != (K,):
        raise ParameterError(f"problem {p}: N_k must have shape ({K},)")
    if np.any(N_k < 0):
        raise ParameterError(f"problem {p}: N_k has a negative entry")
    if int(N_k.sum()) != N:
        raise ParameterError(f"problem {p}: The sum of all N_k must equal the total number of samples (length of second "
                             "dimension of u_kn).")
    f_k = np.zeros(K, dtype=np.float64)
    if f_init is not None:
        f_init = np.array(f_init, dtype=np.float64)
        if f_init.shape != (K,):
            raise ParameterError(f"problem {p}: initial_f_k must be a {K:d}-dimensional np array.")
        f_k = f_init - f_init[0]
    try:
        validate_inputs(u, N_k.astype(np.float64), f_k)
    except (TypeError, ValueError) as exc:
        raise ParameterError(f"problem {p}: {exc}") from exc
    return u, N_k, f_k


def _protocol(tol, maximum_iterations, min_sc_iter, gamma):
    return (dict(method="adaptive", tol=tol, continuation=None,
                 options=dict(min_sc_iter=min_sc_iter, maxiter=maximum_iterations, gamma=gamma, verbose=False)),)


def _host_solve(u, N_k, f_k, protocol, device):
    """The single-problem path for a problem the device loop handed back: ``solve_mbar_for_all_states`` on its own matrix,
    then ``(W^T W, sum_n W_nk)`` at the answer as ``MBAR`` takes them."""
    from . import mbar_solvers
    from .device import DeviceMatrix

    sws = np.where(N_k != 0)[0].astype(np.int64)
    results = []
    with DeviceMatrix.from_host(u, device=device) as dm:
        f = mbar_solvers.solve_mbar_for_all_states(dm, N_k, f_k, sws, protocol, results_out=results)
        dm.set_Nk(N_k)
        G, ws = dm.gram_w(f)
    res = results[-1] if results else dict(iterations=0, nr_iter=0, sci_iter=0, success=True)
    return f, G, ws, res


def _host_solve_replicas(u, N_k, f_start, protocol, device, seed, bs):
    """The single-problem path for the replicates ``bs`` of a problem: its own matrix with the draw counts as sample weights."""
    from . import mbar_solvers
    from .device import DeviceMatrix

    sws = np.where(N_k != 0)[0].astype(np.int64)
    out = []
    with DeviceMatrix.from_host(u, device=device) as dm:
        for b in bs:
            dm.set_sample_weights(np.bincount(bootstrap_indices(seed, b, N_k), minlength=u.shape[1]))
            results = []
            try:
                f = mbar_solvers.solve_mbar_for_all_states(dm, N_k, f_start.copy(), sws, protocol, results_out=results)
            finally:
                dm.set_sample_weights(None)
            res = results[-1] if results else dict(iterations=0, success=True)
            out.append((f, int(res["iterations"]), bool(res["success"])))
    return out


def _slot_bytes(K, N):
    chunks = -(-int(N) // _lib.MBAR_BATCH_CHUNK)
    return 8 * int(N) + chunks * (8 * (4 * K + K * K) + 32) + C.sizeof(_lib.BatchState) + 96


def _solve_replicas(h, blocks, Nks, f_out, fallback, seeds, B, settings, protocol):
    """The P x B replicates: slots on the device in groups of at most BOOTSTRAP_GROUP_BYTES, each started from its problem's f_k;
    slots the device hands back, and every replicate of a problem that itself fell back, go through the single-problem path."""
    P = len(blocks)
    f_boots = [np.zeros((B, b.shape[0])) for b in blocks]
    iters = np.zeros((P, B), dtype=np.int64)
    success = np.zeros((P, B), dtype=bool)
    host = np.zeros((P, B), dtype=bool)
    passes = 0
    slots = [(p, b) for p in range(P) if not fallback[p] for b in range(B)]
    cost = np.array([_slot_bytes(blocks[p].shape[0], blocks[p].shape[1]) for p, _ in slots], dtype=np.int64)
    start = 0
    while start < len(slots):
        end = start + max(1, int(np.searchsorted(np.cumsum(cost[start:]), BOOTSTRAP_GROUP_BYTES, side="right")))
        group = slots[start:end]
        R = len(group)
        gp = np.array([p for p, _ in group], dtype=np.int64)
        gb = np.array([b for _, b in group], dtype=np.int64)
        h.set_replicas(gp, Nks)
        h.replicas_draw(0, seeds[gp], gb)
        states = _new_states(gp, h.K, Nks, f_out, settings)
        passes += h.replicas_solve(states)
        sv = _states_view(states)
        f_all = _all_states_update(sv)  # (with the weighted psum and lognum)
        back = sv["status"] == FALLBACK
        cuts = np.concatenate(([0], np.flatnonzero(np.diff(gp)) + 1, [R]))  # (a problem's slots are consecutive)
        for s0, s1 in zip(cuts[:-1], cuts[1:]):
            p = gp[s0]
            ok = ~back[s0:s1]
            bs = gb[s0:s1][ok]
            f_boots[p][bs] = f_all[s0:s1][ok, :int(h.K[p])]
            iters[p, bs] = sv["iterations"][s0:s1][ok]
            success[p, bs] = sv["success"][s0:s1][ok] != 0
            host[p, gb[s0:s1][~ok]] = True
        start = end
    h.set_replicas(np.zeros(0, dtype=np.int64), Nks)
    host[fallback, :] = True
    for p in np.where(host.any(axis=1))[0]:
        bs = np.where(host[p])[0]
        for b, (f, it, ok) in zip(bs, _host_solve_replicas(blocks[p], Nks[p], f_out[p], protocol, h.device, int(seeds[p]), bs)):
            f_boots[p][b] = f
            iters[p, b] = it
            success[p, b] = ok
    if not success.all():
        logger.warning(f"{int((~success).sum())} bootstrap replicates did not converge to within specified tolerance.")
    return f_boots, iters, success, host, passes


def _pseudoinverse_stack(A, tol=1.0e-10):
    """``MBAR._pseudoinverse`` of every matrix of the stack ``A`` (B, K, K)."""
    out = np.empty_like(A)
    literal = os.environ.get("PYMBAR_AMD_PINV", "") == "svd"
    sym = np.array([not literal and np.allclose(a, a.T, rtol=0.0, atol=1e-12 * max(1.0, float(np.abs(a).max()))) for a in A],
                   dtype=bool)
    if sym.any():
        out[sym] = np.linalg.pinv(A[sym], rcond=tol, hermitian=True)
    if (~sym).any():
        out[~sym] = np.linalg.pinv(A[~sym], rcond=tol)
    return out


def _theta_stack(G, Nk, method):
    """``MBAR._theta_from_gram`` ("svd-ew" / "approximate") of a stack of problems with the same K: G (B, K, K), Nk (B, K)."""
    if method == "approximate":
        return G
    B, K, _ = G.shape
    S2, V = np.linalg.eigh(G)
    S2[np.where(S2 < 0.0)] = 0.0
    sg = np.sqrt(S2)
    VT = np.swapaxes(V, 1, 2)
    VS = V * sg[:, None, :]
    inner = ((sg[:, :, None] * VT) * Nk[:, None, :]) @ V * sg[:, None, :]
    ident = np.identity(K, dtype=np.float64)
    return ((VS @ _pseudoinverse_stack(ident - inner)) * sg[:, None, :]) @ VT


def _error_of_differences_stack(cov, warning_cutoff):
    """``MBAR._ErrorOfDifferences`` of every matrix of the stack ``cov`` (B, K, K)."""
    diag = np.diagonal(cov, axis1=1, axis2=2)
    d2 = diag[:, None, :] + diag[:, :, None] - 2 * cov
    cutoff = -abs(warning_cutoff)
    for b in range(d2.shape[0]):
        x = d2[b]
        if np.any(x < 0.0):
            if np.any(x < cutoff):
                logger.warning("A squared uncertainty is negative. Largest Magnitude = {0:f}".format(abs(np.min(x[x < cutoff]))))
            else:
                x[np.logical_and(0 > x, x > cutoff)] = 0.0
    return np.sqrt(d2)


def mbar_batch(u_kn_list, N_k_list, initial_f_k=None, tol=1e-12, maximum_iterations=10000, min_sc_iter=0, gamma=1.0,
               compute_uncertainty=True, uncertainty_method=None, warning_cutoff=1e-10, device=None, n_bootstraps=0, rseed=None,
               bootstrap_seeds=None):
    """Solve P independent MBAR problems (``u_kn_list[p]``: K_p x N_p, ``N_k_list[p]``: K_p, 1 <= K_p <= 64) in one device call.

    Returns a dict of per-problem entries: ``f_k``, ``Delta_f`` and ``dDelta_f`` (lists of arrays; ``dDelta_f`` only with
    ``compute_uncertainty``), ``iterations``, ``nr_iterations``, ``sci_iterations`` (int arrays), ``success`` and
    ``host_fallback`` (bool arrays), and ``choices`` (per problem the Newton-Raphson flag of each of the first 63 iterations).
    ``uncertainty_method``: None / "svd-ew", "approximate" or "bootstrap".

    ``n_bootstraps = B > 0``: after the P problems (solved exactly as with ``B = 0``) their P x B bootstrap replicates are solved
    on the device as well, each from its problem's ``f_k`` with the same ``tol``, ``maximum_iterations``, ``min_sc_iter`` and
    ``gamma``, in groups of replica slots that take at most ``BOOTSTRAP_GROUP_BYTES`` (2 GiB) of device memory for their draw counts
    (8 bytes per sample and slot), chunk records and states.  Replicate b of problem p is replicate b of the counter-based stream
    ``bootstrap_seeds[p]`` (``bootstrap_indices(seed, b, N_k)`` gives its resampled indices); without ``bootstrap_seeds`` the P seeds
    come from ``np.random.default_rng(rseed)``.  Added entries: ``bootstrap_seeds``, ``f_k_boots`` (list of (B, K_p) arrays),
    ``boot_iterations``, ``boot_success`` and ``boot_host_fallback`` ((P, B) arrays; replicates the device handed back, and all
    those of a problem in ``host_fallback``, are solved by the single-problem path).  ``uncertainty_method="bootstrap"`` gives
    ``dDelta_f`` as ``MBAR.compute_free_energy_differences`` does, the standard deviation over the replicates of every difference,
    and skips the covariance pass; the other methods give the analytical ``dDelta_f`` next to ``f_k_boots``."""
    P = len(u_kn_list)
    if P == 0:
        raise ParameterError("mbar_batch needs at least one problem")
    if len(N_k_list) != P:
        raise ParameterError(f"mbar_batch: {P} matrices but {len(N_k_list)} N_k vectors")
    if initial_f_k is not None and len(initial_f_k) != P:
        raise ParameterError(f"mbar_batch: {P} matrices but {len(initial_f_k)} initial_f_k vectors")
    if uncertainty_method not in (None, "svd-ew", "approximate", "bootstrap"):
        raise ParameterError(f"mbar_batch: uncertainty_method {uncertainty_method!r} is not supported (None, 'svd-ew', 'approximate', "
                             "'bootstrap')")
    if isinstance(n_bootstraps, bool) or not isinstance(n_bootstraps, (int, np.integer)) or n_bootstraps < 0:
        raise ParameterError(f"mbar_batch: n_bootstraps must be an integer >= 0, it was set to {n_bootstraps!r}")
    B = int(n_bootstraps)
    if uncertainty_method == "bootstrap" and B == 0:
        raise ParameterError("Cannot request bootstrap sampling of free energy differences without any bootstraps.")
    seeds = None
    if bootstrap_seeds is not None:
        seeds = np.asarray(bootstrap_seeds)
        if seeds.shape != (P,) or not np.issubdtype(seeds.dtype, np.integer) or np.any(seeds < 0):
            raise ParameterError(f"mbar_batch: bootstrap_seeds must be {P} non-negative integers, one per problem")
        seeds = seeds.astype(np.uint64)
    elif B > 0:
        seeds = np.random.default_rng(rseed).integers(np.iinfo(np.int64).max, size=P).astype(np.uint64)
    tol = float(tol)
    maximum_iterations = int(maximum_iterations)
    min_sc_iter = int(min_sc_iter)
    gamma = float(gamma)
    if tol < 4.0 * np.finfo(float).eps:
        logger.info("Tolerance may be too close to machine precision to converge.")
    t0 = time.perf_counter()
    blocks, Nks, f0s = [], [], []
    for p in range(P):
        u, N_k, f_k = _check_problem(p, u_kn_list[p], N_k_list[p], None if initial_f_k is None else initial_f_k[p])
        blocks.append(u)
        Nks.append(N_k)
        f0s.append(f_k)
    Ks = np.array([b.shape[0] for b in blocks], dtype=np.int64)

    settings = (tol, gamma, maximum_iterations, min_sc_iter)
    states = _new_states(np.arange(P), Ks, Nks, f0s, settings)

    t1 = time.perf_counter()
    with DeviceBatch(blocks, device=device) as h:
        t2 = time.perf_counter()
        passes = h.solve(states)
        t3 = time.perf_counter()
        sv = _states_view(states)
        status = sv["status"].copy()
        fallback = status == FALLBACK
        f_all = _all_states_update(sv)
        f_out, results = [], []
        F = np.zeros((P, MAX_K), dtype=np.float64)
        host_gram = {}
        protocol = _protocol(tol, maximum_iterations, min_sc_iter, gamma)
        for p in range(P):
            K = int(Ks[p])
            N_k = Nks[p]
            if fallback[p]:
                f, G, ws, res = _host_solve(blocks[p], N_k, f0s[p], protocol, h.device)
                host_gram[p] = (G, ws)
                results.append((int(res["iterations"]), int(res["nr_iter"]), int(res["sci_iter"]), bool(res["success"]), 0))
            else:
                f = f_all[p, :K].copy()
                results.append((int(sv["iterations"][p]), int(sv["nr_iter"][p]), int(sv["sci_iter"][p]), bool(sv["success"][p]),
                                int(sv["choices"][p])))
                if results[-1][3] is False:
                    logger.warning(f"problem {p}: WARNING: Did not converge to within specified tolerance.")
            F[p, :K] = f
            f_out.append(f)
        gram = wsum = None
        t4 = time.perf_counter()
        analytical = compute_uncertainty and uncertainty_method != "bootstrap"
        if analytical:
            gram, wsum = h.gram_w(F, ~fallback)
        t5 = time.perf_counter()
        boots = None
        if B > 0:
            boots = _solve_replicas(h, blocks, Nks, f_out, fallback, seeds, B, settings, protocol)
        t6 = time.perf_counter()

    out = dict(f_k=f_out, Delta_f=[np.array(f - np.vstack(f)) for f in f_out])
    out["iterations"] = np.array([r[0] for r in results], dtype=np.int64)
    out["nr_iterations"] = np.array([r[1] for r in results], dtype=np.int64)
    out["sci_iterations"] = np.array([r[2] for r in results], dtype=np.int64)
    out["success"] = np.array([r[3] for r in results], dtype=bool)
    out["host_fallback"] = fallback.copy()
    out["choices"] = [np.array([(r[4] >> i) & 1 for i in range(min(r[0], 63))], dtype=bool) for r in results]
    out["passes"] = int(passes)
    # wall-clock split (s): input checks, upload, the device loop, host work between them, the covariance pass, host covariance
    out["timing"] = dict(checks=t1 - t0, upload=t2 - t1, solve=t3 - t2, host=t4 - t3, gram=t5 - t4, covariance=0.0)
    if B > 0:
        out["bootstrap_seeds"] = seeds.copy()
        out["f_k_boots"], out["boot_iterations"], out["boot_success"], out["boot_host_fallback"], out["boot_passes"] = boots
        out["timing"]["bootstrap"] = t6 - t5
    if compute_uncertainty and uncertainty_method == "bootstrap":
        out["dDelta_f"] = [bootstrap_ddelta_f(fb) for fb in out["f_k_boots"]]
    if not analytical:
        return out
    goff = np.concatenate(([0], np.cumsum(Ks * Ks)))
    woff = np.concatenate(([0], np.cumsum(Ks)))
    Gs, Ws = [], []
    for p in range(P):
        K = int(Ks[p])
        if fallback[p]:
            G, ws = host_gram[p]
        else:
            G = gram[goff[p]:goff[p + 1]].reshape(K, K)
            ws = wsum[woff[p]:woff[p + 1]]
        try:
            check_w_sums(ws, 0.0)
        except ParameterError as exc:
            raise ParameterError(f"problem {p}: {exc}") from exc
        Gs.append(G)
        Ws.append(ws)
    method = "svd-ew" if uncertainty_method is None else uncertainty_method
    dDelta_f = [None] * P
    for K in np.unique(Ks):
        sel = np.where(Ks == K)[0]
        G = np.stack([Gs[p] for p in sel])
        Nk = np.stack([Nks[p] for p in sel]).astype(np.float64)
        theta = _theta_stack(G, Nk, method)
        err = _error_of_differences_stack(theta, warning_cutoff)
        for i, p in enumerate(sel):
            dDelta_f[p] = err[i]
    out["dDelta_f"] = dDelta_f
    out["timing"]["covariance"] = time.perf_counter() - (t6 if B > 0 else t5)
    return out
