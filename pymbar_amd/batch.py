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

``MBARBatch`` keeps the solved batch resident and answers the expectation family of ``MBAR`` for every problem at once: new states
and observables become extension rows of the resident blocks, swept by one device pass for their normalisers and one for the
augmented Gram matrices.
"""
import ctypes as C
import logging
import os
import time
from typing import NamedTuple

import numpy as np

from . import _lib
from .utils import ParameterError, check_w_sums

logger = logging.getLogger(__name__)

MAX_K = _lib.MBAR_BATCH_MAX_K
MAX_AUG = _lib.MBAR_BATCH_MAX_AUG
RUNNING, DONE, FALLBACK = 0, 1, 2
_dp, _ip, _i32p, _u64p = _lib._dp, _lib._ip, _lib._i32p, _lib._u64p
# Device memory one group of replica slots may take for its multiplicities (8 N bytes per slot), chunk records and states
BOOTSTRAP_GROUP_BYTES = 2 << 30
# Device memory the partial records of one group of problems may take in the augmented Gram pass of MBARBatch
EXT_GRAM_GROUP_BYTES = 1 << 30


def _check_inputs(rc):
    """MBAR_ERR_ARG is about the inputs (NaN / -inf entries, a batch larger than the device, bad weights): a ParameterError."""
    _lib.check(rc, arg_error=ParameterError)


def _at(F, mask, n):
    """Where a pass over ``n`` problems or slots evaluates: ``F`` (n, MAX_K), entry e's free energies in the first K columns of row
    e, and ``mask`` (n,) as int32."""
    mask = np.ascontiguousarray(mask, dtype=np.int32)
    if mask.shape != (n,):
        raise ValueError(f"mask must have shape ({n},)")
    return _lib.f64(F, (n, MAX_K), "F"), mask


class DeviceBatch(_lib.Handle):
    """P problems' reduced potentials resident on one device (``mbar_batch_*`` of include/mbar_hip.h)."""

    _destroy = "mbar_batch_destroy"

    def __init__(self, blocks, device=None):
        self._lib = _lib.load_library()
        _lib.require_device()
        self.device = _lib.default_device(device)
        blocks = [_lib.f64(b, (None, None), f"block {p}") for p, b in enumerate(blocks)]
        self.P = len(blocks)
        self.K = np.array([b.shape[0] for b in blocks], dtype=np.int64)
        self.N = np.array([b.shape[1] for b in blocks], dtype=np.int64)
        self.R = np.zeros(self.P, dtype=np.int64)  # extension rows per problem (set_ext)
        self.base = np.zeros(0, dtype=np.int64)  # the problem of every replica slot (set_replicas)
        ptrs = (_dp * self.P)(*[_lib.ptr(b) for b in blocks])
        h = C.c_void_p()
        _check_inputs(self._lib.mbar_batch_create(C.byref(h), self.device, self.P, _lib.ptr(self.K, _ip), _lib.ptr(self.N, _ip), ptrs))
        self._h = h

    # The problems and the replica slots are two sets of solves over the same blocks: `fn` is the set's entry point, Ks its widths
    def _solve(self, fn, states, n):
        if len(states) != n:
            raise ValueError(f"{n} states are needed, one per entry of the set")
        passes = C.c_int64(0)
        _lib.check(fn(self._h, states, C.byref(passes)))
        return passes.value

    def _gram_w(self, fn, Ks, F, mask):
        F, mask = _at(F, mask, len(Ks))
        gram = np.zeros(int(np.sum(Ks * Ks)), dtype=np.float64)
        wsum = np.zeros(int(np.sum(Ks)), dtype=np.float64)
        _lib.check(fn(self._h, _lib.ptr(F), _lib.ptr(mask, _i32p), _lib.ptr(gram), _lib.ptr(wsum)))
        return gram, wsum

    def solve(self, states):
        return self._solve(self._lib.mbar_batch_solve, states, self.P)

    def gram_w(self, F, mask):
        """Packed ``W^T W`` and ``sum_n W_nk`` at ``F[p, :K[p]]`` for the problems with ``mask[p]``."""
        return self._gram_w(self._lib.mbar_batch_gram_w, self.K, F, mask)

    # ---- replica slots (bootstrap replicates) ----
    def set_replicas(self, base, N_k_list):
        """Declares ``len(base)`` replica slots: slot s shares problem ``base[s]``'s block; ``N_k_list[p]`` (every problem's samples
        per state) fixes the layout of the draws.  An empty ``base`` releases the slots."""
        base = np.ascontiguousarray(base, dtype=np.int64)
        if base.ndim != 1 or len(N_k_list) != self.P:
            raise ValueError(f"base must be a vector of problems and N_k_list hold {self.P} vectors")
        Nk = np.zeros((self.P, MAX_K), dtype=np.int64)
        for p in range(self.P):
            if np.shape(N_k_list[p]) != (self.K[p],):
                raise ValueError(f"problem {p}: N_k must have shape ({int(self.K[p])},)")
            Nk[p, :self.K[p]] = N_k_list[p]
        _check_inputs(self._lib.mbar_batch_set_replicas(self._h, len(base), _lib.ptr(base, _ip), _lib.ptr(Nk, _ip)))
        self.base = base

    def replica_set_weights(self, slot, c_n):
        """Slot ``slot``'s per-sample multiplicities from a host vector (finite, >= 0)."""
        c_n = _lib.f64(c_n, (int(self.N[self.base[slot]]),), "sample weights")
        _check_inputs(self._lib.mbar_batch_replica_set_weights(self._h, int(slot), _lib.ptr(c_n)))

    def replicas_draw(self, first, seeds, replicates):
        """Draw counts of the slots ``first .. first + len(seeds)`` on the device: replicate ``replicates[i]`` of stream ``seeds[i]``."""
        seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
        replicates = np.ascontiguousarray(replicates, dtype=np.int64)
        if seeds.ndim != 1 or replicates.shape != seeds.shape:
            raise ValueError("seeds and replicates must be vectors of one length")
        _lib.check(self._lib.mbar_batch_replicas_draw(self._h, int(first), len(seeds), _lib.ptr(seeds, _u64p), _lib.ptr(replicates, _ip)))

    def replicas_solve(self, states):
        return self._solve(self._lib.mbar_batch_replicas_solve, states, len(self.base))

    def replicas_gram_w(self, F, mask):
        """``gram_w`` of the slots: packed ``sum_n c_n W_ni W_nj`` and ``sum_n c_n W_nk`` at ``F[s, :K]``."""
        return self._gram_w(self._lib.mbar_batch_replicas_gram_w, self.K[self.base], F, mask)

    # ---- extension rows (the expectation family) ----
    def set_ext(self, rows):
        """Problem p's extension rows ``rows[p]`` (R_p x N_p; None: no rows), resident until replaced; ``rows=None`` releases them."""
        if rows is None:
            self.R = np.zeros(self.P, dtype=np.int64)
            _check_inputs(self._lib.mbar_batch_set_ext(self._h, None, None))
            return
        if len(rows) != self.P:
            raise ValueError(f"rows must hold {self.P} entries, one per problem")
        rows = [None if r is None or len(r) == 0 else _lib.f64(r, (None, int(self.N[p])), f"problem {p}: extension rows")
                for p, r in enumerate(rows)]
        R = np.array([0 if r is None else r.shape[0] for r in rows], dtype=np.int64)
        ptrs = (_dp * self.P)(*[_lib.ptr(r) for r in rows])
        _check_inputs(self._lib.mbar_batch_set_ext(self._h, _lib.ptr(R, _ip), ptrs))  # (rejected: the earlier rows stay)
        self.R = R

    def ext_lognum(self, F, mask):
        """Packed ``log sum_n exp(-logden_n(F[p]) - e_rn)`` of the extension rows of the problems with ``mask[p]``."""
        F, mask = _at(F, mask, self.P)
        out = np.zeros(int(self.R.sum()), dtype=np.float64)
        if out.size:
            _check_inputs(self._lib.mbar_batch_ext_lognum(self._h, _lib.ptr(F), _lib.ptr(mask, _i32p), _lib.ptr(out)))
        return out

    def ext_gram(self, F, f_ext, mask, group_bytes=0):
        """Packed ``Q^T Q`` ((K + R)^2 per problem) and column sums of ``Q = [W | exp(f_ext_r - e_rn - logden_n)]`` at ``F`` for the
        problems with ``mask[p]``; the records of one group of problems take at most ``group_bytes`` of device memory."""
        F, mask = _at(F, mask, self.P)
        f_ext = _lib.f64(f_ext, (int(self.R.sum()),), "f_ext")
        A = self.K + self.R
        gram = np.zeros(int(np.sum(A * A)), dtype=np.float64)
        wsum = np.zeros(int(np.sum(A)), dtype=np.float64)
        _check_inputs(self._lib.mbar_batch_ext_gram(self._h, _lib.ptr(F), _lib.ptr(f_ext), _lib.ptr(mask, _i32p), int(group_bytes),
                                                    _lib.ptr(gram), _lib.ptr(wsum)))
        return gram, wsum


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


def _check_lengths(who, u_kn_list, N_k_list, initial_f_k):
    P = len(u_kn_list)
    if P == 0:
        raise ParameterError(f"{who} needs at least one problem")
    if len(N_k_list) != P:
        raise ParameterError(f"{who}: {P} matrices but {len(N_k_list)} N_k vectors")
    if initial_f_k is not None and len(initial_f_k) != P:
        raise ParameterError(f"{who}: {P} matrices but {len(initial_f_k)} initial_f_k vectors")
    return P


def _settings(tol, maximum_iterations, min_sc_iter, gamma):
    """The solver settings of a batch as the states take them, and as the protocol of the single-problem path."""
    tol = float(tol)
    maximum_iterations = int(maximum_iterations)
    min_sc_iter = int(min_sc_iter)
    gamma = float(gamma)
    if tol < 4.0 * np.finfo(float).eps:
        logger.info("Tolerance may be too close to machine precision to converge.")
    return (tol, gamma, maximum_iterations, min_sc_iter), _protocol(tol, maximum_iterations, min_sc_iter, gamma)


def _check_problems(u_kn_list, N_k_list, initial_f_k, settings):
    """Every problem checked and made contiguous (``_check_problem``), and the state array that starts their solves."""
    P = len(u_kn_list)
    blocks, Nks, f0s = [], [], []
    for p in range(P):
        u, N_k, f_k = _check_problem(p, u_kn_list[p], N_k_list[p], None if initial_f_k is None else initial_f_k[p])
        blocks.append(u)
        Nks.append(N_k)
        f0s.append(f_k)
    Ks = np.array([b.shape[0] for b in blocks], dtype=np.int64)
    return blocks, Nks, f0s, _new_states(np.arange(P), Ks, Nks, f0s, settings)


def _solve_problems(h, states, blocks, Nks, f0s, protocol):
    """The problems' solves on the handle ``h``, the all-state update, and the single-problem path for the problems the device
    handed back.  Returns (passes, time after the device loop, fallback, f_k per problem, the same in rows of MAX_K, per problem
    (iterations, nr, sci, success, choices), {p: (W^T W, sum_n W_nk)} of the problems that fell back)."""
    P = len(blocks)
    passes = h.solve(states)
    t3 = time.perf_counter()
    sv = _states_view(states)
    status = sv["status"].copy()
    fallback = status == FALLBACK
    f_all = _all_states_update(sv)
    f_out, results = [], []
    F = np.zeros((P, MAX_K), dtype=np.float64)
    host_gram = {}
    for p in range(P):
        K = blocks[p].shape[0]
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
    return passes, t3, fallback, f_out, F, results, host_gram


def _unpack_gram(Ks, gram, wsum, fallback, host_gram):
    """Per problem ``(W^T W, sum_n W_nk)`` from the packed covariance pass (or the single-problem path), the sums checked."""
    goff = np.concatenate(([0], np.cumsum(Ks * Ks)))
    woff = np.concatenate(([0], np.cumsum(Ks)))
    Gs, Ws = [], []
    for p in range(len(Ks)):
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
    return Gs, Ws


def _theta_stacks(Gs, Nks, method):
    """``_theta_stack`` of the problems, those of one size as one stack: ``Gs[p]`` (A_p, A_p), ``Nks[p]`` (A_p,).  Yields
    (the problems of a size, their Theta stack)."""
    sizes = np.array([G.shape[0] for G in Gs], dtype=np.int64)
    for A in np.unique(sizes):
        sel = np.where(sizes == A)[0]
        G = np.stack([Gs[p] for p in sel])
        Nk = np.stack([Nks[p] for p in sel]).astype(np.float64)
        yield sel, _theta_stack(G, Nk, method)


def _ddelta_f(Nks, Gs, uncertainty_method, warning_cutoff):
    dDelta_f = [None] * len(Gs)
    for sel, theta in _theta_stacks(Gs, Nks, "svd-ew" if uncertainty_method is None else uncertainty_method):
        err = _error_of_differences_stack(theta, warning_cutoff)
        for i, p in enumerate(sel):
            dDelta_f[p] = err[i]
    return dDelta_f


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
    P = _check_lengths("mbar_batch", u_kn_list, N_k_list, initial_f_k)
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
    t0 = time.perf_counter()
    settings, protocol = _settings(tol, maximum_iterations, min_sc_iter, gamma)
    blocks, Nks, f0s, states = _check_problems(u_kn_list, N_k_list, initial_f_k, settings)
    Ks = np.array([b.shape[0] for b in blocks], dtype=np.int64)

    t1 = time.perf_counter()
    with DeviceBatch(blocks, device=device) as h:
        t2 = time.perf_counter()
        passes, t3, fallback, f_out, F, results, host_gram = _solve_problems(h, states, blocks, Nks, f0s, protocol)
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
    Gs, Ws = _unpack_gram(Ks, gram, wsum, fallback, host_gram)
    out["dDelta_f"] = _ddelta_f(Nks, Gs, uncertainty_method, warning_cutoff)
    out["timing"]["covariance"] = time.perf_counter() - (t6 if B > 0 else t5)
    return out


def _check_method(who, uncertainty_method):
    if uncertainty_method not in (None, "svd-ew", "approximate"):
        raise ParameterError(f"{who}: uncertainty_method {uncertainty_method!r} is not supported (None, 'svd-ew', 'approximate')")
    return "svd-ew" if uncertainty_method is None else uncertainty_method


class MBARBatch:
    """P independent MBAR problems solved in one device call and kept resident for the expectation family (DESIGN.md section 15,
    INTEGRATION.md section 7).

    Construction checks, uploads and solves exactly as ``mbar_batch(..., n_bootstraps=0)`` does (the same ``f_k`` bits); the handle
    stays on the device until ``close()``, the end of a ``with`` block or collection.  Attributes: ``P``, ``K``, ``N`` (arrays),
    ``N_k``, ``f_k`` (lists), ``iterations``, ``success``, ``host_fallback``.  Every method returns a dict of per-problem lists
    under the key names of the ``MBAR`` method it mirrors; entry p is what ``MBAR(u_p, N_p, solver_protocol=<adaptive, tol>)``
    and the same method return.  New states and observables become extension rows of the resident blocks (states with no samples,
    as in expectations.py): their normalisers and the augmented Gram matrices of all problems come from one device pass each, the
    covariances from eigendecompositions stacked over the problems that share an augmented size.  ``uncertainty_method``: None /
    "svd-ew" or "approximate".  A problem in ``host_fallback`` is answered by the single-problem ``MBAR``."""

    def __init__(self, u_kn_list, N_k_list, initial_f_k=None, tol=1e-12, maximum_iterations=10000, min_sc_iter=0, gamma=1.0,
                 device=None):
        self._h = None
        self._mbars = {}
        P = _check_lengths("MBARBatch", u_kn_list, N_k_list, initial_f_k)
        settings, self._protocol = _settings(tol, maximum_iterations, min_sc_iter, gamma)
        self._maxiter = settings[2]
        self._blocks, self.N_k, self._f0s, states = _check_problems(u_kn_list, N_k_list, initial_f_k, settings)
        self.P = P
        self.K = np.array([b.shape[0] for b in self._blocks], dtype=np.int64)
        self.N = np.array([b.shape[1] for b in self._blocks], dtype=np.int64)
        self._h = DeviceBatch(self._blocks, device=device)
        try:
            _, _, self.host_fallback, self.f_k, self._F, results, self._host_gram = _solve_problems(
                self._h, states, self._blocks, self.N_k, self._f0s, self._protocol)
        except BaseException:
            self.close()
            raise
        self.iterations = np.array([r[0] for r in results], dtype=np.int64)
        self.success = np.array([r[3] for r in results], dtype=bool)
        self._gram = None

    # ---- lifetime ----
    def close(self):
        """Release the device copy of the problems (and the single-problem objects of those that fell back)."""
        if self._h is not None:
            self._h.close()
            self._h = None
        for m in self._mbars.values():
            m.close()
        self._mbars = {}

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if self._h is None:
            raise ParameterError("MBARBatch: the batch is closed")
        return self._h

    def _mbar(self, p):
        """The single-problem object of a problem that fell back."""
        from .mbar import MBAR

        if p not in self._mbars:
            self._mbars[p] = MBAR(self._blocks[p], self.N_k[p], initial_f_k=self._f0s[p], solver_protocol=self._protocol,
                                  maximum_iterations=self._maxiter, device=self._handle().device)
        return self._mbars[p]

    def _gram_w(self):
        """Per problem ``(W^T W, sum_n W_nk)`` at ``f_k`` (one device pass, kept)."""
        h = self._handle()
        if self._gram is None:
            gram, wsum = h.gram_w(self._F, ~self.host_fallback)
            self._gram = _unpack_gram(self.K, gram, wsum, self.host_fallback, self._host_gram)
        return self._gram

    def _ErrorOfDifferences(self, cov, warning_cutoff=1.0e-10):
        from .mbar import error_of_differences

        return error_of_differences(cov, warning_cutoff)

    # ---- the methods of MBAR ----
    def compute_free_energy_differences(self, compute_uncertainty=True, uncertainty_method=None, warning_cutoff=1.0e-10):
        """``Delta_f`` and ``dDelta_f`` per problem: the numbers of ``mbar_batch``."""
        _check_method("MBARBatch", uncertainty_method)
        self._handle()
        out = dict(Delta_f=[np.array(f - np.vstack(f)) for f in self.f_k])
        if compute_uncertainty:
            Gs, _ = self._gram_w()
            out["dDelta_f"] = _ddelta_f(self.N_k, Gs, uncertainty_method, warning_cutoff)
        return out

    def compute_overlap(self):
        """``scalar``, ``eigenvalues`` and ``matrix`` of ``MBAR.compute_overlap`` per problem."""
        Gs, _ = self._gram_w()
        out = dict(scalar=[], eigenvalues=[], matrix=[])
        for p in range(self.P):
            O = self.N_k[p] * Gs[p]
            eigenvals = np.sort(np.linalg.eigvals(O))[::-1]
            out["scalar"].append(1 - eigenvals[1])
            out["eigenvalues"].append(eigenvals)
            out["matrix"].append(O)
        return out

    def compute_expectations(self, A_n_list, u_kn_list=None, output="averages", state_dependent=False, compute_uncertainty=True,
                             uncertainty_method=None, warning_cutoff=1.0e-10):
        """``mu`` and ``sigma`` of ``MBAR.compute_expectations`` per problem: ``A_n_list[p]`` is (N_p,), or (K_p, N_p) with
        ``state_dependent`` (one observable per state); ``u_kn_list[p]`` optional new states (L_p, N_p)."""
        from . import expectations as ex

        _check_method("MBARBatch", uncertainty_method)
        if output not in ("averages", "differences"):
            raise ParameterError(f"MBARBatch: output must be 'averages' or 'differences', it was {output!r}")
        self._check_list("A_n_list", A_n_list)
        u_ln = self._check_new_states(u_kn_list)
        A, maps = [], []
        for p in range(self.P):
            Kout = int(self.K[p]) if u_ln[p] is None else u_ln[p].shape[0]
            a = np.asarray(A_n_list[p], dtype=np.float64)
            want = (Kout, int(self.N[p])) if state_dependent else (int(self.N[p]),)
            if a.shape != want:
                raise ParameterError(f"problem {p}: the observable must have shape {want}, it has {a.shape}")
            if not np.all(np.isfinite(a)):
                raise ParameterError(f"problem {p}: the observable is not finite")
            A.append(np.atleast_2d(a))
            sm = np.zeros([2, Kout], int)
            sm[0, :] = np.arange(Kout)
            if state_dependent:
                sm[1, :] = np.arange(Kout)
            maps.append(sm)
        inner = self.compute_expectations_inner(A, u_ln, maps, uncertainty_method=uncertainty_method, warning_cutoff=warning_cutoff,
                                                return_theta=compute_uncertainty)
        out = dict(mu=[])
        if compute_uncertainty:
            out["sigma"] = []
        for p in range(self.P):
            Kout = maps[p].shape[1]
            cov = ex._difference_covariance(inner[p], Kout)[1] if compute_uncertainty else None
            r = ex._expectations_result(self, inner[p], None, cov, Kout, output, compute_uncertainty, uncertainty_method,
                                        warning_cutoff)
            for key in out:
                out[key].append(r[key])
        return out

    def compute_perturbed_free_energies(self, u_ln_list, compute_uncertainty=True, uncertainty_method=None, warning_cutoff=1.0e-10):
        """``Delta_f`` and ``dDelta_f`` among the new states ``u_ln_list[p]`` (L_p, N_p) per problem."""
        from . import expectations as ex

        _check_method("MBARBatch", uncertainty_method)
        u_ln = self._check_new_states(u_ln_list, required=True)
        maps = [np.arange(u.shape[0]) for u in u_ln]
        inner = self.compute_expectations_inner([None] * self.P, u_ln, maps, uncertainty_method=uncertainty_method,
                                                warning_cutoff=warning_cutoff, return_theta=compute_uncertainty)
        out = dict(Delta_f=[])
        if compute_uncertainty:
            out["dDelta_f"] = []
        for p in range(self.P):
            r = ex._perturbed_result(self, inner[p], compute_uncertainty, uncertainty_method, warning_cutoff)
            for key in out:
                out[key].append(r[key])
        return out

    def compute_entropy_and_enthalpy(self, uncertainty_method=None, warning_cutoff=1.0e-10):
        """``Delta_f``, ``Delta_u``, ``Delta_s`` and their uncertainties per problem (``MBAR.compute_entropy_and_enthalpy``)."""
        from . import expectations as ex

        _check_method("MBARBatch", uncertainty_method)
        self._handle()
        for p in np.where(~self.host_fallback)[0]:   # (the potentials are the observables; a problem that fell back is MBAR's)
            if not np.all(np.isfinite(self._blocks[p])):
                raise ParameterError(f"problem {p}: the potentials hold +inf: no entropy / enthalpy decomposition")
        maps = [np.vstack([np.arange(K), np.arange(K)]) for K in self.K]
        inner = self.compute_expectations_inner(self._blocks, [None] * self.P, maps, uncertainty_method=uncertainty_method,
                                                warning_cutoff=warning_cutoff, return_theta=True)
        keys = ("Delta_f", "dDelta_f", "Delta_u", "dDelta_u", "Delta_s", "dDelta_s")
        out = {key: [] for key in keys}
        for p in range(self.P):
            r = ex._entropy_and_enthalpy_result(self, inner[p], int(self.K[p]), uncertainty_method, warning_cutoff)
            for key in keys:
                out[key].append(r[key])
        return out

    # ---- input rules ----
    def _check_list(self, name, lst):
        if len(lst) != self.P:
            raise ParameterError(f"MBARBatch: {self.P} problems but {len(lst)} entries in {name}")

    def _check_new_states(self, u_list, required=False):
        """Per problem the new states as a contiguous (L_p, N_p) array, or None for the resident states."""
        if u_list is None:
            if required:
                raise ParameterError("MBARBatch: the new states are missing")
            return [None] * self.P
        self._check_list("the list of new states", u_list)
        out = []
        for p in range(self.P):
            u = np.ascontiguousarray(u_list[p], dtype=np.float64)
            if u.ndim == 1:
                u = u.reshape(1, -1)
            if u.ndim != 2 or u.shape[0] < 1:
                raise ParameterError(f"problem {p}: the new states must be an L x N array")
            if u.shape[1] < self.N[p]:
                raise ParameterError(f"problem {p}: the new states have {u.shape[1]} columns, fewer than the {int(self.N[p])} samples: "
                                     "evaluate the new potentials at all of the samples used originally")
            if u.shape[1] != self.N[p]:
                raise ParameterError(f"problem {p}: the new states must have shape (L, {int(self.N[p])}), they have {u.shape}")
            if np.any(np.isnan(u)) or np.any(u == -np.inf):
                raise ParameterError(f"problem {p}: the new states hold NaN or -inf")
            out.append(u)
        return out

    # ---- the one pass underneath ----
    def compute_expectations_inner(self, A_list, u_ln_list, state_maps, uncertainty_method=None, warning_cutoff=1.0e-10,
                                   return_theta=False):
        """``expectations.compute_expectations_inner`` of every problem: ``A_list[p]`` the observables (n_obs, N_p) (None: no
        observables), ``u_ln_list[p]`` the states (L_p, N_p) (None: the resident states), ``state_maps[p]`` as there.  Returns
        per problem the dict of ``observables``, ``f``, ``Theta``, ``Amin``.

        The augmented matrix of problem p is its resident block plus extension rows, built as ``expectations._augmented_matrix``
        builds them: resident states are not duplicated (their copies of the reference's layout are columns scaled by
        exp(f_l - f_k[l]): the ``distinct`` case of ``expectations.assemble_inner``, which writes every result dict), new states
        are rows with N = 0, observable s is the row u_{l(s),n} - log(A_sn - shift_s) with the shift of ``rows_logshift`` taken
        on the host.  A problem that needs no rows at all (resident states, no observables) is answered from the kept covariance
        pass at ``f_k``.  ``self.timing`` holds the wall-clock split (s) of the last call: the rows built on the host, upload and
        device passes, covariances and results."""
        from .expectations import assemble_inner

        method = _check_method("MBARBatch", uncertainty_method)
        h = self._handle()
        plans = self._plan_inner(A_list, u_ln_list, state_maps)   # (every input rule, before any device work)
        device = ~self.host_fallback
        t0 = time.perf_counter()
        rows, shifts = [None] * self.P, [None] * self.P
        for p, pl in enumerate(plans):
            if device[p] and pl.R > 0:
                rows[p], shifts[p] = _extension_rows(pl)
        t1 = time.perf_counter()
        R = np.array([0 if r is None else r.shape[0] for r in rows], dtype=np.int64)
        mask = R > 0
        # the kept pass at f_k: the normalisers of resident states, and the Gram matrix of a problem without rows
        kept = any(device[p] and (pl.resident or (return_theta and pl.R == 0)) for p, pl in enumerate(plans))
        Gs, Ws = self._gram_w() if kept else (None, None)
        lognum_ext, gram, wsum = np.zeros(0), None, None
        if mask.any():
            h.set_ext(rows)
            try:
                lognum_ext = h.ext_lognum(self._F, mask)
                if return_theta:
                    if not np.all(np.isfinite(lognum_ext[np.repeat(mask, R)])):
                        roff = np.concatenate(([0], np.cumsum(R)))
                        bad = [p for p in np.where(mask)[0] if not np.all(np.isfinite(lognum_ext[roff[p]:roff[p + 1]]))]
                        raise ParameterError(f"problem {bad[0]}: a new state or an observable has no weight on any sample")
                    gram, wsum = h.ext_gram(self._F, -lognum_ext, mask, EXT_GRAM_GROUP_BYTES)
            finally:
                h.set_ext(None)
        t2 = time.perf_counter()
        roff = np.concatenate(([0], np.cumsum(R)))
        Aug = self.K + R
        goff = np.concatenate(([0], np.cumsum(Aug * Aug)))
        woff = np.concatenate(([0], np.cumsum(Aug)))
        sel = np.where(device)[0]
        thetas = {}
        if return_theta:
            Gaug, Naug = [], []
            for p in sel:
                if mask[p]:
                    a = int(Aug[p])
                    try:
                        check_w_sums(wsum[woff[p]:woff[p + 1]], 0.0)
                    except ParameterError as exc:
                        raise ParameterError(f"problem {p}: {exc}") from exc
                    Gaug.append(gram[goff[p]:goff[p + 1]].reshape(a, a))
                else:
                    Gaug.append(Gs[p])
                Naug.append(np.concatenate((self.N_k[p], np.zeros(int(R[p]), dtype=np.int64))))
            thetas = {sel[i]: t for idx, stack in _theta_stacks(Gaug, Naug, method) for i, t in zip(idx, stack)}
        out = [None] * self.P
        for p in sel:
            # the K + R columns of problem p are distinct: resident states are not duplicated (expectations.assemble_inner puts
            # their copies back), new states are the first NL extension rows; the observable rows follow
            plan, ln_ext = plans[p].plan, lognum_ext[roff[p]:roff[p + 1]]
            if plans[p].resident:
                with np.errstate(divide="ignore"):
                    ln_L = (np.log(Ws[p]) - self.f_k[p])[plan.L_list]   # (from sum_n W_nk = exp(f_k + lognum_k))
                ln_obs = ln_ext
            else:
                ln_L, ln_obs = ln_ext[:plan.NL], ln_ext[plan.NL:]
            out[p] = assemble_inner(plan, int(self.K[p]), self.f_k[p], ln_L, ln_obs, shifts[p], thetas.get(p),
                                    distinct=plans[p].resident)
        for p in np.where(self.host_fallback)[0]:
            pl, m = plans[p], self._mbar(p)
            A = np.array([0]) if pl.A is None else (m.u_kn if pl.A is self._blocks[p] else pl.A)
            out[p] = m.compute_expectations_inner(A, m.u_kn if pl.resident else pl.u_ln, state_maps[p],
                                                  uncertainty_method=uncertainty_method, warning_cutoff=warning_cutoff,
                                                  return_theta=return_theta)
        self.timing = dict(rows=t1 - t0, device=t2 - t1, covariance=time.perf_counter() - t2)
        return out

    def _plan_inner(self, A_list, u_ln_list, state_maps):
        """Per problem what ``compute_expectations_inner`` is asked for, checked: the plan of its state map
        (``expectations.plan_inner``), its states and observables, and the extension rows ``R`` it takes (the observables at
        resident states; the distinct new states and the observables otherwise)."""
        from .expectations import plan_inner

        self._check_list("A_list", A_list)
        self._check_list("u_ln_list", u_ln_list)
        self._check_list("state_maps", state_maps)
        plans = []
        for p in range(self.P):
            K, N = int(self.K[p]), int(self.N[p])
            resident = u_ln_list[p] is None
            u_ln = self._blocks[p] if resident else u_ln_list[p]
            A = A_list[p]
            n_states = u_ln.shape[0] if u_ln.ndim == 2 else 0   # (what is not an array of rows is refused below)
            n_obs = A.shape[0] if A is not None and A.ndim == 2 else 0
            plan = plan_inner(state_maps[p], n_states, n_obs)
            state_list, obs_list, S = plan.state_list, plan.obs_list, plan.S
            if u_ln.ndim != 2 or u_ln.shape[1] != N or (S > 0 and (A is None or A.ndim != 2 or A.shape[1] != N)):
                raise ParameterError(f"problem {p}: states and observables must be arrays of {N} columns")
            if np.any(state_list < 0) or np.any(state_list >= plan.n_states) or (
                    S > 0 and (np.any(obs_list < 0) or np.any(obs_list >= plan.n_obs))):
                raise ParameterError(f"problem {p}: the state map names a state or an observable that is not there")
            if not self.host_fallback[p]:   # (a problem that fell back is MBAR's, with MBAR's answer to such input)
                for i in np.unique(obs_list):
                    if not np.all(np.isfinite(A[i])):
                        raise ParameterError(f"problem {p}: observable {int(i)} is not finite")
            R = S if resident else plan.NL + S
            if K + R > MAX_AUG:
                raise ParameterError(f"problem {p}: K + extra rows = {K + R} > {MAX_AUG}: use MBAR")
            plans.append(_BatchPlan(plan, R, resident, u_ln, A))
        return plans


class _BatchPlan(NamedTuple):
    """One problem of ``MBARBatch.compute_expectations_inner``: the plan of its state map and what is the batch's own."""
    plan: "InnerPlan"   # (expectations.InnerPlan)
    R: int              # extension rows
    resident: bool      # the states are the resident ones
    u_ln: np.ndarray    # the states (L, N)
    A: np.ndarray       # the observables (n_obs, N), or None


def _extension_rows(bp):
    """``(rows, shift)`` of one planned problem: its extension rows -- the distinct new states (none where the states are
    resident), then per observable s the row u_{l(s),n} - log(A_sn - shift) -- and its observables' shifts, shift = amin -
    |4 eps amin|."""
    plan, A, u_ln = bp.plan, bp.A, bp.u_ln
    eps4 = 4.0 * np.finfo(np.float64).eps
    shift = np.zeros(plan.n_obs if plan.S > 0 else 0, dtype=np.float64)
    logA = {}
    for i in np.unique(plan.obs_list):
        amin = A[i].min()
        shift[i] = amin - np.abs(eps4 * amin)
        with np.errstate(divide="ignore"):
            logA[int(i)] = np.log(A[i] - shift[i])
    block = np.empty((bp.R, u_ln.shape[1]), dtype=np.float64)
    r0 = 0
    if not bp.resident:
        block[:plan.NL] = u_ln[plan.L_list]
        r0 = plan.NL
    for s in range(plan.S):
        block[r0 + s] = u_ln[plan.state_list[s]] - logA[int(plan.obs_list[s])]
    return block, shift
