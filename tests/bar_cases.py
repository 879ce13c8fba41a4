"""Cases, branch model, bounds and root-find drivers of the BAR and EXP sums (``mbar_bar_zero`` / ``mbar_bar_solve`` /
``mbar_bar_moments``; mbar_k_bar.hip, mbar_bar.cpp, ``bar_advance`` of mbar_bar.h) -- TEST INFRASTRUCTURE ONLY, shared by
tests/test_gpu_other_estimators.py (device), tests/test_other_estimators_host.py (the model's own checks, on the CPU) and
tools/bar_branch_matrix.py.  The oracle is tests/bar_oracle.py (numpy long double).

Cases.  A case is a pair ``(w_F, w_R)``, a tuple of ``DeltaF`` values and a name; ``cases()`` is the product of the side lengths
next to every chunk (4096), wave (64) and workgroup (256) seam with the value patterns below, thinned to every third pair per
pattern, plus two pairs with a side of 256 * 4096 + 1 values (257 chunks: the strided merge loops make a second trip).  A
pattern is named for the branch of ``k_bar_eval`` / ``merge_side`` / ``k_bar_mom_*`` it forces at the case's ``DeltaF``:
``positive`` (every x > 0), ``negative`` (every x <= 0), ``straddle`` (x_min <= 0 < x inside a chunk), ``zero`` (dyadic w, M = 0,
some x exactly 0), ``spread`` (sorted, scale 400: neighbouring chunks' shifts differ by more than 745, so the smaller chunk's
``exp(e)`` is 0), ``offset`` (w near +-1e6), ``inf_scattered`` / ``inf_chunks`` / ``inf_side*`` (+inf values inside chunks, as whole
chunks, as a whole side).

Branch model.  ``model_zero`` restates ``k_bar_eval`` + ``merge_side`` in numpy fp64: the chunk cut, the padding with +inf, the
two ``two_sum``s of x_min, the three forms of ``lin``, the ``hi + lo`` shift, the rescaling by ``exp(e)`` and ``exp(2 e)``.  Only
the ORDER of the additions inside a sum differs from the device (numpy's pairwise sums), so the model is held to the same bound
as the device, not to its bits.  It also returns the census of what the case reaches.  ``mutate`` names one deliberate error; the
CPU tests show that each puts a case above its bound.  NOT detectable at these bounds: dropping the ``lo`` word of the shift
(``mutate="nolo"``: at most 0.21 of the bound on this case set, asserted as NOT detected) -- the suite does not pin it.  ``model_moments`` does the same for the three stages of the EXP
moments.

Bounds (each a function of the inputs and of the oracle's values only).

* Log sums (``log_sum_bound``): the project's bound ``1e-14 + 4e-16 |want|`` plus ``2^-52 (max finite |w| of the side + |DeltaF| +
  |M|)``.  x = (w -+ DeltaF) +- M is formed with two fp64 roundings, each at most 2^-53 of a partial result that is at most
  ``max|w| + |DeltaF| + |M|``; ``|d log f / dx| <= 1`` and every term of a side moves by at most that much, so the log of the sum
  moves by at most the same amount.  About 1e-15 everywhere but in the ``offset`` cases.  ``F``: the two log-sum bounds added.
* EXP moments (``moment_bounds``).  logsumexp(-w): ``max(1e-14, 1e-15 |want|)``, the project's.  ``sum w``: ``1e-13 sum |w|`` over
  the finite values (the sum may cancel; its rounding error does not).  ``sum x``: 1e-13 of the value.  The centred squares,
  ``sum (v - mean)^2``: 1e-13 of the value plus ``n delta^2``: with the device's mean off by delta,
  ``sum (v - m - delta)^2 = sum (v - m)^2 - 2 delta sum (v - m) + n delta^2`` and the middle term vanishes at the true mean m.
  ``delta <= 2^-52 max|v| depth(n)``, ``depth(n) = ceil(log2 n) + 1``: every addition of the device's fixed tree rounds by at
  most 2^-53 of a partial sum <= n max|v|, i.e. 2^-53 max|v| of the mean, the division adds one more, and a value passes through
  at most ``device_additions(n) + 1 <= 2 depth(n)`` of them (15 in its thread, 6 in the wave, 3 across waves, then the same
  over the chunks; checked for every length of the case set in the CPU tests).  For x = exp(-w - max(-w)) in (0, 1] two more
  units of 2^-52 cover the one-ulp exponentials of the device and of numpy.  Where the oracle's value is inf or NaN (+inf work
  values: an infinite mean) the device's value has to be of the same class.
"""
import functools
import math
import struct

import numpy as np

from tests import bar_oracle as orc

LD = np.longdouble
EPS = 2.0 ** -52
CHUNK, WG = 4096, 256  # MBAR_BAR_CHUNK, BAR_WG
LENGTHS = (1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193, 3 * 4096 + 1)
BIG = 256 * 4096 + 1
MUTATIONS = ("straddle", "pad0", "s2e", "noshift", "mom_chunkmin")
STATE_FIELDS = ("status", "phase", "iteration", "nzero", "DeltaF", "DeltaF_initial", "UpperB", "LowerB", "FUpperB", "FLowerB",
                "FNew", "relative_change")


# ---- the case set ------------------------------------------------------------------------------------------------------------------
def length_pairs():
    """every length with itself (M exactly 0), then with the length five places on (M != 0): each length on both sides"""
    k = len(LENGTHS)
    return [(n, n) for n in LENGTHS] + [(LENGTHS[i], LENGTHS[(i + 5) % k]) for i in range(k)]


PATTERNS = ("positive", "negative", "straddle", "zero", "spread", "offset", "inf_scattered", "inf_chunks")
INF_SIDES = (("inf_side_F", 65, 65), ("inf_side_R", 4097, 257), ("inf_side_FR", 2, 4097), ("inf_side_FR", 256, 256))


def _inf_scattered(rng, n):
    w = rng.normal(1.0, 2.0, n)
    w[1::3] = np.inf
    k = min(5, n - 1)
    if k:
        w[n - k:] = np.inf  # the last values of the (short) last chunk
    return w


def _inf_chunks(rng, n):
    w = np.full(n, np.inf)
    w[-1] = rng.normal(1.0, 2.0)  # whole chunks of +inf first, one finite value last
    return w


def make_case(pattern, n_F, n_R, seed=11):
    """(w_F, w_R) and the DeltaF values at which the pattern forces its branch"""
    rng = np.random.default_rng([seed, n_F, n_R, sum(map(ord, pattern))])
    absM = abs(math.log(n_F / n_R))
    if pattern == "positive":
        w = [absM + 1.0 + rng.exponential(3.0, n) for n in (n_F, n_R)]
        dfs = (0.0, 0.5, -0.75)
    elif pattern == "negative":
        w = [-(absM + 1.0 + rng.exponential(3.0, n)) for n in (n_F, n_R)]
        dfs = (0.0, 0.5, -0.75)
    elif pattern == "straddle":
        w = [rng.normal(0.0, 3.0, n) for n in (n_F, n_R)]
        for a in w:
            if a.size > 1:
                a[0], a[-1] = -(absM + 2.0), absM + 2.0
        dfs = (0.0, 1.5)
    elif pattern == "zero":
        assert n_F == n_R
        w = [rng.integers(-4096, 4097, n) / 1024.0 for n in (n_F, n_R)]
        d = float(w[0][n_F // 2])  # x_F = w_F - d is exactly 0 there,
        w[1][0] = -d  # and x_R = w_R + d here
        dfs = (d,)
    elif pattern == "spread":
        w = [np.sort(rng.normal(0.0, 400.0, n)) for n in (n_F, n_R)]
        dfs = (0.0, 600.0, -600.0)
    elif pattern == "offset":
        w = [1e6 + rng.normal(0.0, 2.0, n_F), -1e6 + rng.normal(0.0, 2.0, n_R)]
        dfs = (1e6 + 0.3125, 0.0)
    elif pattern == "inf_scattered":
        w = [_inf_scattered(rng, n) for n in (n_F, n_R)]
        dfs = (0.0, 2.0)
    elif pattern == "inf_chunks":
        w = [_inf_chunks(rng, n) for n in (n_F, n_R)]
        dfs = (0.5,)
    elif pattern.startswith("inf_side_"):
        w = [rng.normal(0.0, 2.0, n) for n in (n_F, n_R)]
        for side, tag in enumerate("FR"):
            if tag in pattern[9:]:
                w[side][:] = np.inf
        dfs = (0.0,)
    else:
        raise ValueError(pattern)
    return dict(name=f"{pattern}-{n_F}x{n_R}", pattern=pattern, w_F=w[0], w_R=w[1], dfs=dfs)


def case_keys():
    """(pattern, n_F, n_R): pattern k takes every third length pair, starting at pair k (``zero``: pairs of equal lengths only);
    the +inf sides; the two pairs with the 257-chunk side"""
    pairs = length_pairs()
    keys = []
    for k, pattern in enumerate(PATTERNS):
        for j, (a, b) in enumerate(pairs):
            if pattern == "zero":
                if a == b and j % 2 == 0:
                    keys.append((pattern, a, b))
            elif (j + k) % 3 == 0:
                keys.append((pattern, a, b))
    keys += list(INF_SIDES)
    keys += [("spread", BIG, 1), ("straddle", 1, BIG)]
    return keys


@functools.lru_cache(maxsize=None)
def cases():
    """the whole set, generated once per process (about 2.5 million values); read-only"""
    out = [make_case(*key) for key in case_keys()]
    for c in out:
        c["w_F"].setflags(write=False)
        c["w_R"].setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _oracle_zero(name):
    c = next(c for c in cases() if c["name"] == name)
    return tuple(np.array(orc.log_sums(c["w_F"], c["w_R"], d), dtype=LD) for d in c["dfs"])


def oracle_zero(case):
    """[(F, l1F, l1R, l2F, l2R) in long double for every DeltaF of the case], computed once per process"""
    with np.errstate(invalid="ignore"):
        return _oracle_zero(case["name"])


@functools.lru_cache(maxsize=None)
def _oracle_moments(name):
    c = next(c for c in cases() if c["name"] == name)
    return tuple(orc.side_moments(w) for w in (c["w_F"], c["w_R"]))


def oracle_moments(case):
    with np.errstate(invalid="ignore", over="ignore"):
        return _oracle_moments(case["name"])


# ---- the model of k_bar_eval + merge_side ------------------------------------------------------------------------------------------
def two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def softplus_tail(x):
    return np.log1p(np.exp(-np.abs(x)))


def model_side(w, side, DeltaF, M, mutate=None):
    """(log sum f, log sum f^2) of one side as the device forms them, and the side's census"""
    w = np.asarray(w, dtype=np.float64)
    n = w.size
    nc = -(-n // CHUNK)
    pad = nc * CHUNK - n
    v = np.full(nc * CHUNK, np.inf)
    v[:n] = w
    real = np.zeros(nc * CHUNK, dtype=bool)
    real[:n] = True
    real = real.reshape(nc, CHUNK)
    wmin = v.reshape(nc, CHUNK).min(axis=1)  # of the real values: the host's chunk table
    if mutate == "pad0":
        v[n:] = 0.0
    v = v.reshape(nc, CHUNK)
    live = wmin != np.inf
    census = dict(chunks=nc, pad=pad, trips=-(-nc // WG), all_inf=int((~live).sum()), xmin_pos=0, nonpos_only=0, straddling=0,
                  n_pp=0, n_straddle=0, n_nonpos=0, n_zero=0, shift_diff=0.0)
    if not live.any():
        return -np.inf, -np.inf, census
    v, real, wmin = v[live], real[live], wmin[live]
    c1 = DeltaF if side else -DeltaF
    c2 = -M if side else M
    with np.errstate(invalid="ignore", over="ignore"):
        a_hi, a_lo = two_sum(wmin, c1)
        xmin, b_lo = two_sum(a_hi, c2)
        lmin = softplus_tail(xmin)
        x = (v + c1) + c2
        pos = x > 0.0
        minpos = (xmin > 0.0)[:, None]
        pp, st = pos & minpos, pos & ~minpos
        lin = np.where(pp, wmin[:, None] - v, np.where(st, 0.0 if mutate == "straddle" else -x, 0.0))
        t = np.exp(lin + (lmin[:, None] - softplus_tail(x)))
        s1 = t.sum(axis=1)
        s2 = (t * t).sum(axis=1)
        h_hi, h_lo = two_sum(xmin, lmin)
        hi = -np.where(xmin > 0.0, h_hi, lmin)  # the partial's shift -softplus(x_min) as hi + lo
        lo = -np.where(xmin > 0.0, h_lo + (a_lo + b_lo), 0.0) * (mutate != "nolo")
        L = hi.max()
        e = np.zeros_like(hi) if mutate == "noshift" else (hi - L) + lo
        keep = s1 != 0.0
        S1 = np.sum((s1 * np.exp(e))[keep])
        S2 = np.sum((s2 * np.exp(e if mutate == "s2e" else 2.0 * e))[keep])
        l1, l2 = L + np.log(S1), 2.0 * L + np.log(S2)
    any_pos = (pos & real).any(axis=1)
    census.update(xmin_pos=int((xmin > 0.0).sum()), nonpos_only=int(((xmin <= 0.0) & ~any_pos).sum()),
                  straddling=int(((xmin <= 0.0) & any_pos).sum()), n_pp=int((pp & real).sum()), n_straddle=int((st & real).sum()),
                  n_nonpos=int((~pos & real).sum()), n_zero=int(((x == 0.0) & real).sum()), shift_diff=float(hi.max() - hi.min()))
    return float(l1), float(l2), census


def model_zero(w_F, w_R, DeltaF, mutate=None):
    """((F, l1F, l1R, l2F, l2R) as fp64, {"F": census of the forward side, "R": of the reverse side})"""
    M = float(np.log(np.float64(len(w_F)) / np.float64(len(w_R))))
    l1F, l2F, cF = model_side(w_F, 0, float(DeltaF), M, mutate)
    l1R, l2R, cR = model_side(w_R, 1, float(DeltaF), M, mutate)
    with np.errstate(invalid="ignore"):
        F = np.float64(l1F) - np.float64(l1R)
    return np.array([F, l1F, l1R, l2F, l2R]), dict(F=cF, R=cR)


def census_line(cs):
    def one(c):
        return (f"chunks {c['chunks']:3d} (inf {c['all_inf']} pos {c['xmin_pos']} nonpos {c['nonpos_only']} straddle {c['straddling']})"
                f" lin {c['n_pp']}/{c['n_straddle']}/{c['n_nonpos']} x==0 {c['n_zero']} shift diff {c['shift_diff']:.4g} pad {c['pad']}"
                f" trips {c['trips']}")

    return f"F: {one(cs['F'])} | R: {one(cs['R'])}"


def model_moments(w, mutate=None):
    """(logsumexp(-w), sum x, sum (x - mean)^2, sum w, sum (w - mean)^2) of one side as the three stages of k_bar_mom_chunk /
    k_bar_mom_merge form them, and the census (chunks, merge trips, chunks of +inf, +inf values)"""
    w = np.asarray(w, dtype=np.float64)
    n = w.size
    nc = -(-n // CHUNK)
    v = np.full(nc * CHUNK, np.nan)
    v[:n] = w
    v = v.reshape(nc, CHUNK)  # (NaN marks the slots past the end: the device's loop stops there)
    real = ~np.isnan(v)
    with np.errstate(invalid="ignore", over="ignore"):
        wmin_c = np.nanmin(v, axis=1)
        census = dict(chunks=nc, trips=-(-nc // WG), all_inf=int((wmin_c == np.inf).sum()), n_inf=int(np.isinf(w).sum()))

        def chunk_sums(term):
            return np.where(real, term, 0.0).sum(axis=1)

        # stage 0: exp(-w) shifted by the chunk's largest, and w itself
        p0 = np.where(wmin_c == np.inf, 0.0, chunk_sums(np.exp(wmin_c[:, None] - v)))
        p1 = chunk_sums(v)
        wmin = wmin_c.min()
        if wmin != np.inf:
            fin = wmin_c != np.inf
            lse = -wmin + np.log(np.sum(p0[fin] * np.exp(wmin - wmin_c[fin])))
        else:
            lse = -np.inf
        sum_w = p1.sum()
        mw = sum_w / n
        # stage 1: x as the reference forms it, against the SIDE's minimum, and the centred squares of w
        shift = wmin_c[:, None] if mutate == "mom_chunkmin" else wmin
        x = np.exp(-v - (-shift))
        sum_x = chunk_sums(x).sum()
        sq_w = chunk_sums((v - mw) ** 2).sum()
        mx = sum_x / n
        # stage 2
        sq_x = chunk_sums((np.exp(-v - (-wmin)) - mx) ** 2).sum()
    return np.array([lse, sum_x, sq_x, sum_w, sq_w]), census


# ---- bounds --------------------------------------------------------------------------------------------------------------------------
def _max_finite(w):
    w = np.asarray(w)
    f = np.abs(w[np.isfinite(w)])
    return float(f.max()) if f.size else 0.0


def log_sum_bound(want, w_side, DeltaF, M):
    """bound of one log sum of a side (module docstring)"""
    return 1e-14 + 4e-16 * abs(float(want)) + EPS * (_max_finite(w_side) + abs(DeltaF) + abs(M))


def zero_bounds(case, DeltaF, want):
    """bounds of (F, l1F, l1R, l2F, l2R); where the oracle's value is not finite the entry is unused"""
    M = math.log(len(case["w_F"]) / len(case["w_R"]))
    with np.errstate(invalid="ignore"):
        b = [log_sum_bound(v if np.isfinite(v) else 0.0, w, DeltaF, M)
             for v, w in zip(want[1:], (case["w_F"], case["w_R"], case["w_F"], case["w_R"]))]
    return np.array([b[0] + b[1]] + b)


def kind(v):
    """finite / +inf / -inf / nan"""
    v = float(v)
    return "nan" if v != v else ("finite" if math.isfinite(v) else ("+inf" if v > 0 else "-inf"))


def ratios(got, want, bounds):
    """error / bound of every entry; where the oracle is not finite: 0 for the same class, inf otherwise (also for a NaN where
    the oracle is finite)"""
    out = np.zeros(len(got))
    for k, (g, w, b) in enumerate(zip(got, want, bounds)):
        if kind(w) != "finite" or kind(g) != "finite":
            out[k] = 0.0 if kind(g) == kind(w) else np.inf
        else:
            out[k] = float(abs(LD(g) - LD(w)) / LD(b))
    return out


def zero_ratios(case, k, got):
    want = oracle_zero(case)[k]
    return ratios(got, want, zero_bounds(case, case["dfs"][k], want))


def depth(n):
    return math.ceil(math.log2(n)) + 1 if n > 1 else 1


def device_additions(n):
    """the most additions a value passes through in the device's two-level fixed-order sum of n values"""
    def level(m, per_thread):
        # m values over 256 threads (per_thread each at most), a butterfly over the wave's 64 lanes, the waves in order
        serial = min(per_thread, -(-m // WG)) - 1
        return max(serial, 0) + min(6, math.ceil(math.log2(min(m, 64))) if m > 1 else 0) + min(3, -(-min(m, WG) // 64) - 1)

    nc = -(-n // CHUNK)
    return level(min(n, CHUNK), CHUNK // WG) + (level(nc, -(-nc // WG)) if nc > 1 else 0)


def moment_bounds(w, want):
    """bounds of the five moments of a side (module docstring); an entry whose oracle value is not finite is unused"""
    w = np.asarray(w, dtype=np.float64)
    n = w.size
    fin = np.abs(w[np.isfinite(w)])
    d_w = EPS * _max_finite(w) * depth(n)
    d_x = EPS * 1.0 * (depth(n) + 2)
    f = [float(v) if np.isfinite(v) else 0.0 for v in want]
    return np.array([max(1e-14, 1e-15 * abs(f[0])), 1e-13 * abs(f[1]), 1e-13 * abs(f[2]) + n * d_x ** 2, 1e-13 * float(fin.sum()),
                     1e-13 * abs(f[4]) + n * d_w ** 2])


def moment_ratios(w, got, want=None):
    with np.errstate(invalid="ignore", over="ignore"):
        want = orc.side_moments(w) if want is None else want
    return ratios(got, want, moment_bounds(w, want))


# ---- the root find: problems, configurations, the lockstep host drive --------------------------------------------------------------
def dyadic_pair(n, s, seed=5):
    """n_F == n_R, w_F = w + s, w_R = w - s with w and s multiples of 2^-10: M = 0, every x is exact, and both sides run the same
    arithmetic on the same numbers at DeltaF = s, so F(s) == 0.0 exactly (and F(s + t) == -F(s - t) for dyadic t)"""
    w = np.random.default_rng([seed, n]).integers(-2048, 2049, n) / 1024.0
    return w + s, w - s


def dyadic_problems():
    """(name, w_F, w_R, UpperB, LowerB): the hand-set brackets that force the exits the golden data sets do not reach"""
    out = []
    for n, s in ((300, 0.75), (4097, -1.5)):
        w_F, w_R = dyadic_pair(n, s)
        out += [(f"dyadic{n}-root", w_F, w_R, s, s - 2.0),  # UpperB is the exact root
                (f"dyadic{n}-sym", w_F, w_R, s + 1.0, s - 1.0),  # F(U) == -F(L): the first false-position point is the root
                (f"dyadic{n}-widen", w_F, w_R, s + 3.0, s + 2.5)]  # both ends above the root
    w_F, w_R = dyadic_pair(64, 0.0)
    out += [("dyadic64-zero", w_F, w_R, 0.0, 0.0),  # F(0) == 0 at both ends: the loop ends without an evaluation
            ("dyadic64-wide", w_F, w_R, 2.0, -1.0)]
    out += [("inf-both", np.full(5, np.inf), np.full(4097, np.inf), 1.0, -1.0)]  # F is NaN everywhere
    return out


def rootfind_configs():
    """(method, iterated, maximum_iterations, want_moments): the full product at 0 / 1 / 3 iterations; at 500 every method
    iterated, and false position not iterated (501 evaluations without a convergence test) once"""
    out = [(m, it, mx, wm) for m in range(3) for it in (1, 0) for mx in (0, 1, 3) for wm in (0, 1)]
    out += [(m, 1, 500, wm) for m in range(3) for wm in (0, 1)]
    out += [(0, 0, 500, 1)]
    return out


def make_states(problems, config, starts=(0.0, 1.0, -0.3)):
    """a ``BarState * P`` array: problem p with its bracket, start starts[p % 3], and the configuration"""
    from pymbar_amd import _lib

    method, iterated, maxit, want = config
    st = (_lib.BarState * len(problems))()
    for p, (_, _, _, U, L) in enumerate(problems):
        s = st[p]
        s.method, s.iterated, s.maximum_iterations, s.want_moments = method, iterated, maxit, want
        s.relative_tolerance = 1e-12
        s.DeltaF, s.UpperB, s.LowerB = starts[p % len(starts)], float(U), float(L)
    return st


def copy_states(st):
    out = type(st)()
    for p in range(len(st)):
        out[p] = type(st[p]).from_buffer_copy(st[p])
    return out


def drive_lockstep(zero, states, limit=6000):
    """Runs every state to its end through mbar_bar_step_host, all problems in lockstep: per pass one ``zero(DeltaF[P])`` call
    ([P][5]) per request slot.  Returns (passes, [problem went through the widening phase])."""
    P = len(states)
    for s in states:
        s.phase, s.status, s.moments_pending = 0, orc.RUNNING, 0
        orc.step_host(s, None)
    widened = [False] * P
    passes = 0
    while any(s.status == orc.RUNNING for s in states):
        assert passes < limit, "the host-driven root find did not end"
        F = np.zeros((P, 2))
        for r in range(2):
            need = [p for p in range(P) if states[p].status == orc.RUNNING and states[p].nreq > r]
            if need:
                d = np.zeros(P)
                d[need] = [states[p].req[r] for p in need]
                F[need, r] = np.asarray(zero(d))[need, 0]
        for p in range(P):
            if states[p].status == orc.RUNNING:
                orc.step_host(states[p], F[p])
                widened[p] = widened[p] or states[p].phase == 2
        passes += 1
    return passes, widened


def bits(v):
    return struct.pack("<d", float(v))


def same_bits(a, b):
    return bits(a) == bits(b) or (a != a and b != b)


def state_mismatches(dev, host):
    """the fields of STATE_FIELDS in which two final states differ (NaN equals NaN)"""
    return [f for f in STATE_FIELDS if not same_bits(getattr(dev, f), getattr(host, f))]


def exits_of(s, widened):
    """the named exits a final state stands for"""
    out = {("RUNNING", "DONE", "NAN_BRACKET", "BOUNDS", "NOT_CONVERGED")[s.status]}
    if s.method == 0 and s.status in (1, 4) and s.UpperB == 0.0 and s.LowerB == 0.0 and s.nzero == 2:
        out.add("no-evaluation")
    elif s.method == 0 and s.status in (1, 4) and s.FNew == 0.0 and s.relative_change == 1e-15:
        out.add("FNew==0")
    if widened:
        out.add("widened")
    return out


EXITS = ("DONE", "NOT_CONVERGED", "BOUNDS", "NAN_BRACKET", "FNew==0", "no-evaluation", "widened")
