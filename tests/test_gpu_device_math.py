"""The device exp / log of the evaluation sweeps and the resident probability matrix P, looked at ELEMENT BY ELEMENT on the
device, through the C ABI only.  Needs an MI355X (``-m gpu``).  The CPU side of the same functions is tests/test_device_math_tables.py.

Probe matrices
--------------
The only elementwise window on the fast exp / log of an evaluation sweep is logden (one value per sample).  Every column n of a
probe matrix is one controlled experiment: row kmax(n) holds c_n, row kprobe(n) holds c_n + d_n (d_n >= 0), every other row lies
1e6 kT above (its term is exactly 0 on the device and in long double) or holds +inf (second variant: the clamped code paths).
N_k = 1 for every state, so a_k = f_k + ln 1 = f_k exactly (no host logarithm in the budget).  kmax and kprobe rotate over all
rows as n advances: every 16-row block, every lane of a DPP row, every register slot carries the maximum and the probe somewhere,
and a reduction that drops one shows up as a wrong logden, not as a drift.  At f = 0 the device's scaled argument of the probe row is
t = fma(-v, LOG2E_S, RN(c LOG2E_S)) (v the probe row's entry), and (c_n, v_n) is searched with the CPU model
(tests/device_math_model.py) such that t lands EXACTLY on: every table index (t = -j), every rounding tie (t = -j - 1/2) and its two
fp64 neighbours -- which holds the wrap j = 2047 -> 0 between t = -1/2 and its neighbour below --, fractions just below 1 (the
exp2s_neg form), both subnormal boundaries 2^-1022 and 2^-1074, the clamp -1100 S and arguments far beyond it, and the arguments at
which the result flips with the last bit of a linear or quadratic polynomial coefficient (COEFFICIENT_PROBES of the model module).
c_n = 0 reaches three quarters of these arguments (RN(-d LOG2E_S) moves by up to 1.44 ulp per step of d); the rest take c_n = -2^k,
which makes the probe's entry smaller and its steps finer (_cv_for_argument).  For log_pos, (c_n, v_n) is searched such that the
device sum s = RN(e_max + e_probe) is the FIRST and the LAST fp64 mantissa of each of the 128 buckets (_cv_for_sum).  s >= 1 always in an
evaluation sweep on u (the largest term is 1), so other exponents of s come from columns where r rows tie at the maximum (s = r + e,
r up to 16); s < 1 occurs only in the sweeps on P (fmax(sv, 1e-300)), which have no elementwise output and are NOT covered here (the
model's log_pos is checked there on the CPU).  The same probes are run again with c_n of order one, +-1e4 and mixed signs, and with
f != 0.  The coverage is asserted exactly -- every target, no share (test_probe_plan_reaches_every_target).

Bit identity
------------
On a column with at most two nonzero terms nothing on the way to logden depends on the order of a sum or on a hardware estimate:
a - u, the maximum, m LOG2E_S, fma, the table exponential, ONE addition, log_pos, the closing fma.  The model restates that chain
instruction by instruction, and the test asserts logden(device) == logden(model) bit for bit on every such column, in every
layout.  A wrong table entry, coefficient digit, tie, wrap, bucket or dropped lane changes bits; the model reads its constants from
the source tree, and tests/test_device_math_tables.py pins those and the model to long double.  The same holds for P of the two
build sweeps (k_build_gram, k_build_sweep) up to the reciprocal: the model's recip_fast starts from RN(1/s) instead of the
hardware estimate, and two Newton steps end at the same bits unless 1/s lies within ~2^-104 of a rounding boundary.  One probe
column does sit there -- s = 1 - 2^-53 (largest term 1 - 2^-53 at an anchor f0 != 0, probe term subnormal), 1/s = 1 + 2^-53 + 2^-106,
where the device returns 1 and the model 1 + 2^-52 -- so wherever the model's result changes with a seed one fp64 step off
(model.recip_candidates), the device must return ONE of the listed candidates; everywhere else the one value.  No share is tolerated.

Bounds against long double: derived, not fitted.  u = 2^-53.
--------------------------------------------------------
rho_L = |LOG2E_S ln2 / S - 1| / u and rho_c = |LN2_OVER_S S / ln2 - 1| / u are the relative errors of the two rounded constants (both <= 1).
Write x_k = a_k - u_kn (exact value), m = max_k x_k, d_k = m - x_k, p_k the exact probability of row k in its column.
E_exp = 3.1 and the log_pos bound E_log(s) are the claims asserted on the CPU (test_device_math_tables.py).

logden, form fma(m2, LN2_OVER_S, log_pos(s)) (wave-tile kernels, one-read kernels):
  x_k carries u |x_k| (the subtraction); t_k = fma(x_k, LOG2E_S, -m2) carries rho_L u |x_k| (the constant) and u d_k (its rounding);
  the rounding of m2 = RN(m LOG2E_S) is common to shift and sum and cancels; e_k carries E_exp u; the sum R u for R additions;
  log_pos E_log(s) u; m2 LN2_OVER_S carries rho_c u |m|; the closing fma half an ulp of the result.  With |x_k| <= |m| + d_k:
    |err| <= u [ B |m| + A ],   B = 1 + rho_L + rho_c  (<= 3),
    A = E_exp + R + E_log(s) + (2 + rho_L) sum_k p_k d_k + ulp(logden) / (2 u).
logden, form m + log_pos(s) (few-state kernel): the shift is m itself while the sum is relative to m2 ln2 / S, off by (1 + rho_L) u |m|:
    B = 2 + 2 rho_L  (<= 4), the same A.
Layout-agnostic kernels (library exp / log; the control): B = 2, E_exp = 2 (1 ulp), E_log = 2 + ulp(log s)/u, R doubled (online rescaling).
The assertion uses 2 x (B |m| + A): the margin the issue prescribes.

P_kn, relative error, theta_k = the error of row k's exponent, in u (errors common to a column cancel in e_k / s):
  k_build_gram  x = fma(u, -LOG2E_S, RN(a LOG2E_S)), w = RN(m - x), e = exp2s_neg(w):  theta_k = |a_k| + (1 + rho_L) |x_k| + d_k + E_exp
  k_build_sweep x = RN(a - u), t = fma(x, LOG2E_S, -m2), e = exp2s(t):                  theta_k = (1 + rho_L) |x_k| + d_k + E_exp
    both: P = RN(e RN(1/s)):  rel err <= u [ theta_k + sum_j p_j theta_j + R + 2 ]  =  u [ C + D-terms ],  C = E_exp + R + 2 + (...)
  k_gram_quad   t = fma(u, -LOG2E_S, RN(RN(a LOG2E_S) - RN(logden LOG2E_S))), P = exp2s(t), no normalisation:
                theta_k = |a_k| + |logden_n| + |a_k - logden_n| + (1 + rho_L) |ln P| + E_exp + (error of the device logden_n, above)
  k_make_p      P = exp(RN(RN(a - u) - logden)) (library exp, 1 ulp = 2 u):  theta_k = |x_k| + |ln P| + 2 + (error of logden_n)
The growth with the distance |d| below the column maximum (and with |a|, |logden|) comes from forming the scaled argument with a
rounded LOG2E_S and rounded differences; it is a property of the design, written down here, not a defect.  Assertion: 2 x the bound.

Below the normal range (exact P < 2^-1022): the two build sweeps do NOT flush -- v_ldexp_f64 rounds once into the subnormal
range and the product with 1/s rounds once more -- so the value is within the relative bound plus ONE subnormal ulp (and bit-equal
to the model on probe columns); k_gram_quad and k_make_p flush every entry below 2^-1022 to exactly 0.  Either way the mass of a
column lost stays below K 2^-1022, far below the 1e-199 the header of mbar_k_pmode.hip promises.

Measured maxima per layout: profiles/device_math_accuracy.txt."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from pymbar_amd import testsystems as ts  # noqa: E402
from tests import device_math_model as M  # noqa: E402

LD = M.LD
U = LD(2.0) ** -53
C = M.constants()
S = C.S
RHO_L = float(abs(LD(C.LOG2E_S) * M.LN2_LD / S - 1) / U)
RHO_C = float(abs(LD(C.LN2_OVER_S) * S / M.LN2_LD - 1) / U)
BIG = 1.0e6      # kT above the column's offset: its term is exactly zero everywhere
MARGIN = 2.0
LMAX = 17        # live rows of a column: up to 16 tied at the maximum + the probe


@pytest.fixture(scope="module")
def DM():
    from pymbar_amd.device import DeviceMatrix

    return DeviceMatrix


# ---------------------------------------------------------------------------------------------------------------------
# the probe plan
# ---------------------------------------------------------------------------------------------------------------------
def _steps(x0, k):
    """x0 moved by -k .. k fp64 steps: shape (len(x0), 2k + 1)."""
    out = np.empty((x0.size, 2 * k + 1))
    out[:, k] = x0
    lo = hi = x0
    for i in range(1, k + 1):
        lo = np.nextafter(lo, -np.inf)
        hi = np.nextafter(hi, np.inf)
        out[:, k - i], out[:, k + i] = lo, hi
    return out


def two_row_arguments(c, v):
    """The device's scaled arguments (probe row, maximum row) of a column at a = 0 whose maximum row holds c and whose probe row
    holds v >= c:  m = -c, m2 = RN(m LOG2E_S), t = fma(x, LOG2E_S, -m2)."""
    m2 = (-c) * C.LOG2E_S
    return M.fma(-v, C.LOG2E_S, -m2), M.fma(-c, C.LOG2E_S, -m2)


def _cv_for_argument(target):
    """(c, v) with the probe's scaled argument == target exactly (target <= 0).  At c = 0 the argument is RN(-v LOG2E_S), which moves
    by up to 1.44 ulp per step of v, so about a quarter of all doubles are not reached; with the maximum row at c = -2^k (2^k <= d <
    2^(k+1): c LOG2E_S is exact, the maximum's own term stays exactly 1) the probe's entry v = c + d is smaller than d, its steps are
    at most 0.72 ulp of the argument, and every double is reached."""
    target = np.asarray(target, np.float64)
    n = target.size
    c_out, v_out, hit = np.zeros(n), np.zeros(n), np.zeros(n, bool)
    d0 = -target / C.LOG2E_S
    k = np.floor(np.log2(np.maximum(d0, 2.0 ** -1000)))
    for mode in range(3):
        todo = ~hit
        if not todo.any():
            break
        c = np.where(d0 > 0, np.zeros(n) if mode == 0 else -np.exp2(k - (mode - 1)), 0.0)[todo]
        cand = _steps((c * C.LOG2E_S - target[todo]) / C.LOG2E_S, 16)
        tp, _ = two_row_arguments(np.broadcast_to(c[:, None], cand.shape), cand)
        ok = (tp == target[todo][:, None]) & (cand >= c[:, None])
        h = ok.any(axis=1)
        idx = np.nonzero(todo)[0][h]
        c_out[idx], v_out[idx], hit[idx] = c[h], cand[np.arange(cand.shape[0]), np.argmax(ok, axis=1)][h], True
    return c_out, v_out, hit


def _cv_for_sum(target):
    """(c, v) with the device sum RN(e_max + e_probe) == target exactly (1 <= target < 2), searched with the model.  e moves by ~0.4
    of its grid per ulp of the argument and its own rounding can skip a value; offsets c = -(1 + i 2^-20) give other arguments AND a
    maximum term of 1 - 2^-53 (c LOG2E_S is not exact there: the maximum's argument is the residual of that product), which reaches
    the targets that c = 0 misses."""
    target = np.asarray(target, np.float64)
    n = target.size
    c_out, v_out, hit = np.zeros(n), np.zeros(n), np.zeros(n, bool)
    with np.errstate(divide="ignore"):
        d0 = np.where(target > 1.0, -np.log(np.maximum(target - 1.0, 1e-300)), 60.0)
    for c in [0.0] + [-(1.0 + i * 2.0 ** -20) for i in range(1, 64)]:
        todo = ~hit
        if not todo.any():
            break
        cand = _steps(c + d0[todo], 60)
        tp, tm = two_row_arguments(np.full_like(cand, c), cand)
        ok = ((M.exp2s(tm, True, C) + M.exp2s(tp, True, C)) == target[todo][:, None]) & (cand > c)
        h = ok.any(axis=1)
        idx = np.nonzero(todo)[0][h]
        c_out[idx], v_out[idx], hit[idx] = c, cand[np.arange(cand.shape[0]), np.argmax(ok, axis=1)][h], True
    return c_out, v_out, hit


_PLAN = None


def probe_plan():
    """The probe columns, independent of K: c (entry of the maximum row), v (entry of the probe row), d = v - c, ties (rows at the
    maximum), kind (0 index / tie / boundary probes, 1 log-bucket probes, 2 tied-maximum columns)."""
    global _PLAN
    if _PLAN is not None:
        return _PLAN
    j = np.arange(S, dtype=np.float64)
    targets = [-j, -(j + 0.5), np.nextafter(-(j + 0.5), 0.0), np.nextafter(-(j + 0.5), -np.inf)]
    jj = np.arange(0.0, 96.0)
    targets.append(-np.nextafter(jj + 1.0, 0.0))                                     # fract just below 1 (exp2s_neg), rint a hair off an integer
    for b in (1022.0, 1023.0, 1074.0, 1075.0):                                       # results on both sides of 2^-1022 and 2^-1074
        targets.append(-(S * b + np.arange(-3.0, 3.5, 0.5)))
    targets.append(np.array([C.EXP2_CLAMP, C.EXP2_CLAMP + 0.5, C.EXP2_CLAMP + 1.0, C.EXP2_CLAMP - 1.0, C.EXP2_CLAMP - 4096.0]))
    targets = np.concatenate(targets)
    c_arg, v_arg, hit_arg = _cv_for_argument(targets)
    far = np.array([800.0, 1000.0, 2.0e4, 7.5e5])                                    # beyond the clamp; -2.2e9 saturates the int32 conversion
    far = np.concatenate([far, M.coefficient_probe_d()])                              # results that flip with the last bit of a coefficient
    bj = np.arange(128)
    s_first = 1.0 + bj / 128.0
    s_last = np.nextafter(1.0 + (bj + 1.0) / 128.0, 0.0)
    c_sum, v_sum, hit_sum = _cv_for_sum(np.concatenate([s_first, s_last]))
    r_tied = np.array([2, 3, 4, 5, 7, 8, 9, 12, 15, 16] * 4)
    d_tied = np.repeat([0.0, 0.3, 2.0, 40.0], 10)
    c = np.concatenate([c_arg, np.zeros(far.size), c_sum, np.zeros(d_tied.size)])
    v = np.concatenate([v_arg, far, v_sum, d_tied])
    kind = np.concatenate([np.zeros(c_arg.size + far.size, int), np.ones(c_sum.size, int), np.full(d_tied.size, 2)])
    ties = np.concatenate([np.ones(c.size - d_tied.size, int), r_tied])
    _PLAN = dict(c=c, v=v, d=v - c, kind=kind, ties=ties, targets=targets, hit_arg=hit_arg, hit_sum=hit_sum,
                 s_targets=np.concatenate([s_first, s_last]))
    return _PLAN


OFFSETS = (0.0, 1.25, -3.75, 1.0e4, -1.0e4, 123.456, -0.001)


def probe_matrix(K, rows=None, posinf=False, offsets=OFFSETS, pad_to=64, extra_columns=None, plan=None):
    """u_kn (K x N) of the plan for the usable rows ``rows`` (default: all): the full plan with its own (c_n, v_n), then every 5th probe
    again at each of the other offsets (maximum row c, probe row RN(c + d_n)); N = 64 m - 5 (not a multiple of 16; the row pitch a multiple of 64, which the few-state kernel needs).
    Returns (u, live) with live[n] = the rows of column n that hold c_n (ties first) and the probe row last, -1 padded."""
    plan = plan or probe_plan()
    rows = np.arange(K) if rows is None else np.asarray(rows)
    R = rows.size
    assert offsets[0] == 0.0
    cols_v, cols_t, cols_c = [plan["v"]], [plan["ties"]], [plan["c"]]
    for i, c in enumerate(offsets[1:]):
        sel = np.arange(i, plan["d"].size, 5)
        cols_v.append(c + plan["d"][sel])
        cols_t.append(plan["ties"][sel])
        cols_c.append(np.full(sel.size, c))
    d, t, c = np.concatenate(cols_v), np.concatenate(cols_t), np.concatenate(cols_c)  # (d: the probe row's entry from here on)
    t = np.minimum(t, max(R - 1, 1))
    n_probe = d.size
    n_extra = 0 if extra_columns is None else extra_columns.shape[1]
    N = ((n_probe + n_extra + 5 + pad_to - 1) // pad_to) * pad_to - 5
    fill = N - n_probe - n_extra
    d = np.concatenate([d, np.linspace(0.01, 30.0, fill)])                       # (filler columns: c = 0)
    t = np.concatenate([t, np.ones(fill, int)])
    c = np.concatenate([c, np.zeros(fill)])
    n = np.arange(d.size)
    u = np.full((K, N), np.inf if posinf else BIG)
    if not posinf:
        u[:, : d.size] += c[None, :]
    live = np.full((d.size, LMAX), -1)
    kmax = n % R
    if R > 1:
        off = 1 + (n // R) % (R - 1)
        kprobe = (kmax + off) % R                         # every ordered pair of rows comes up as n advances
        for i in range(LMAX - 1):                         # rows tied at the maximum: kmax and the rows after it, skipping the probe row
            use = i < t
            if not use.any():
                break
            r = (kmax + i + (i >= off)) % R
            live[use, i] = rows[r[use]]
            u[rows[r[use]], n[use]] = c[use]
        live[:, LMAX - 1] = rows[kprobe]
        u[rows[kprobe], n] = d
    else:
        live[:, 0] = rows[0]
        u[rows[0], n] = c
    if n_extra:
        u[:, d.size:] = extra_columns
    return u, live, n_probe


def gather(a_k, u, live):
    """(x, mask): x[i, n] = a_k[live[n, i]] - u[live[n, i], n] in long double (exact for these magnitudes), -inf where padded."""
    n = np.arange(live.shape[0])
    x = np.full((LMAX, live.shape[0]), -np.inf, dtype=LD)
    xd = np.full((LMAX, live.shape[0]), -np.inf)
    for i in range(LMAX):
        ok = live[:, i] >= 0
        if ok.any():
            x[i, ok] = np.asarray(a_k, LD)[live[ok, i]] - u[live[ok, i], n[ok]].astype(LD)
            xd[i, ok] = np.asarray(a_k)[live[ok, i]] - u[live[ok, i], n[ok]]
    return x, xd


def reference_columns(x):
    """Long double: m, d_k, p_k, logden of the gathered columns."""
    m = np.max(x, axis=0)
    with np.errstate(invalid="ignore"):
        dk = np.where(np.isneginf(x), LD(0), m[None, :] - x)
        e = np.where(np.isneginf(x), LD(0), np.exp(-dk))
    s = e.sum(axis=0)
    return dict(m=m, d=dk, p=e / s, s=s, logden=m + np.log(s), nnz=(e > 0).sum(axis=0))


def logden_bound_u(ref, form):
    """The bound of the module docstring, in u, per column (without the margin)."""
    s64 = ref["s"].astype(np.float64)
    pd = (ref["p"] * ref["d"]).sum(axis=0).astype(np.float64)
    am = np.abs(ref["m"]).astype(np.float64)
    half_ulp = (M.ulp_of(ref["logden"]) / (2 * U)).astype(np.float64)
    R = np.maximum(ref["nnz"] - 1, 0)
    if form == "generic":
        e_log = 2.0 + (M.ulp_of(np.maximum(np.log(ref["s"]), LD(2.0) ** -60)) / U).astype(np.float64)
        return 2.0 * am + 2.0 + 2 * R + 2 + e_log + 3 * pd + half_ulp
    B = (1 + RHO_L + RHO_C) if form == "fma" else (2 + 2 * RHO_L)
    return B * am + M.E_EXP_CLAIM + R + M.log_bound_u(s64, np.log(ref["s"])) + (2 + RHO_L) * pd + half_ulp


def model_logden(a_k, xd, form, clamp):
    """The device chain on the gathered rows (fp64 x = a - u as the device forms it); valid bit for bit where nnz <= 2."""
    m = np.max(xd, axis=0)
    m2 = m * C.LOG2E_S
    with np.errstate(invalid="ignore"):
        t = M.fma(np.where(np.isneginf(xd), 0.0, xd), C.LOG2E_S, np.broadcast_to(-m2, xd.shape))
    t = np.where(np.isneginf(xd), -np.inf, t)
    e, parts = M.exp2s(np.where(np.isneginf(t), C.EXP2_CLAMP, t), clamp, C, parts=True)
    e = np.where(np.isneginf(t), 0.0, e)
    s = e.sum(axis=0)
    lg, lparts = M.log_pos(s, C, parts=True)
    out = M.fma(m2, C.LN2_OVER_S, lg) if form == "fma" else m + lg
    return out, e, s, parts, lparts


def test_probe_plan_reaches_every_target():
    """CPU-side part (no launch): EVERY planned probe hits its target exactly, by the model -- all 2048 table indices, all 2048 ties
    t = -(j + 1/2) (to even from both sides) and both fp64 neighbours of each, the wrap, both subnormal boundaries, the clamp; all 128
    log buckets at their first and at their last mantissa.  No share: one missed target fails."""
    plan = probe_plan()
    assert plan["hit_arg"].all(), plan["targets"][~plan["hit_arg"]][:10]
    assert plan["hit_sum"].all(), plan["s_targets"][~plan["hit_sum"]][:10]
    k0 = plan["kind"] == 0
    t, tmax = two_row_arguments(plan["c"][k0], plan["v"][k0])
    assert np.array_equal(t[:plan["targets"].size], plan["targets"]) and np.all(tmax == 0)
    e, p = M.exp2s(t, True, C, parts=True)
    assert set(p["j"].tolist()) == set(range(S))
    tie = slice(S, 2 * S)                                     # t = -(j + 1/2), j = 0 .. 2047: to even, z = -1/2 for even j, +1/2 for odd j
    jt = np.arange(S)
    assert np.array_equal(p["z"][tie], np.where(jt % 2 == 0, -0.5, 0.5))
    assert np.array_equal(p["si"][tie], -np.where(jt % 2 == 0, jt, jt + 1))
    assert np.all(np.abs(p["z"][2 * S:4 * S]) < 0.5) and np.array_equal(p["si"][2 * S:3 * S], -jt) and np.array_equal(p["si"][3 * S:4 * S], -(jt + 1))
    wrap = (p["q"] == -1) & (p["j"] == S - 1)
    assert wrap.any() and np.any((p["q"] == 0) & (p["j"] == 0) & (p["z"] == -0.5))          # t = -1/2 and its neighbour below
    assert np.any(e == 2.0 ** -1022) and np.any((e < 2.0 ** -1022) & (e > 0)) and np.any(e == 2.0 ** -1074)
    assert np.any((e == 0) & (t > C.EXP2_CLAMP)) and np.any(t == C.EXP2_CLAMP) and np.any(t < C.EXP2_CLAMP)
    # the build sweep's form on the columns at c = 0: w = RN(v LOG2E_S)
    c0 = plan["c"][k0] == 0
    en, pn = M.exp2s_neg(plan["v"][k0][c0] * C.LOG2E_S, False, C, parts=True)
    assert set(pn["j"].tolist()) == set(range(S)) and np.sum(pn["z"] > 1 - 2.0 ** -40) >= 64  # (fractions an ulp of w below 1)
    assert np.any(pn["si"] == -(1 << 31))                                                     # int32 saturation (d = 7.5e5)
    k1 = plan["kind"] == 1
    tp, tm = two_row_arguments(plan["c"][k1], plan["v"][k1])
    s = M.exp2s(tm, True, C) + M.exp2s(tp, True, C)
    _, lp = M.log_pos(s, C, parts=True)
    assert np.array_equal(s, plan["s_targets"])
    assert np.array_equal(lp["j"][:128], np.arange(128)) and np.array_equal(lp["j"][128:], np.arange(128))
    assert s[0] == 1.0 and s[-1] == np.nextafter(2.0, 0.0)


# ---------------------------------------------------------------------------------------------------------------------
# logden through every evaluation layout
# ---------------------------------------------------------------------------------------------------------------------
LAYOUTS = (
    # (id, K, options, form): the K sets of tests/test_gpu_parity.py, every one
    [(f"few-state K={K} small_k_kernel=1", K, {"small_k_kernel": 1}, "plain") for K in (2, 3, 5, 16, 17, 32)]
    + [(f"wave-tile K={K} small_k_kernel=0", K, {"small_k_kernel": 0}, "fma") for K in (2, 5, 17, 32)]
    + [(f"wave-tile K={K}", K, {}, "fma") for K in (33, 40, 64, 100, 112, 128)]
    + [(f"wide panels K={K} wide_k_kernel={w}", K, {"wide_k_kernel": w}, "fma") for K in (96, 100, 112, 128, 192, 256) for w in (1, 0)]
    + [(f"paneled K={K}", K, {}, "fma") for K in (129, 160, 192, 200, 256)]
    + [(f"one-read K={K}", K, {}, "fma") for K in (257, 300, 321, 512, 513, 600, 700, 768, 769, 1000, 1024)]
    + [(f"layout-agnostic K={K} force_generic={g}", K, {"force_generic": g}, "generic") for K, g in ((40, 1), (128, 1), (300, 1), (1025, 0), (1100, 1))]
)


def check_logden(got, a_k, u, live, form, clamp, tag, n_probe):
    x, xd = gather(a_k, u, live)
    ref = reference_columns(x)
    err = (np.abs(got.astype(LD) - ref["logden"]) / U).astype(np.float64)
    bound = logden_bound_u(ref, form)
    ratio = err / bound
    worst = int(np.argmax(ratio))
    small = np.abs(ref["m"]) <= 4
    line = (f"{tag}: worst |logden - long double| = {err[small].max():.2f} u where |m| <= 4, {err.max():.0f} u overall; "
            f"worst error / derived bound = {ratio[worst]:.3f} (column {worst}, |m| = {float(abs(ref['m'][worst])):.4g})")
    if form != "generic":
        model, e, s, parts, lparts = model_logden(a_k, xd, form, clamp)
        two = ref["nnz"] <= 2
        # (a subnormal second term does not count as nonzero in long double's sum of 1 + e, and not on the device either)
        same = model == got
        line += f"; bit-identical to the model on {int(np.sum(same & two))} of {int(np.sum(two))} columns with <= 2 terms"
        print(line)
        bad = np.nonzero(two & ~same)[0]
        assert bad.size == 0, (tag, bad[:8], got[bad[:8]], model[bad[:8]])
    else:
        print(line)
    assert np.all(err <= MARGIN * bound), (tag, worst, err[worst], bound[worst])


@pytest.mark.parametrize("tag,K,options,form", LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_logden_probes_in_every_evaluation_layout(DM, tag, K, options, form):
    """logden of the probe columns: bit-identical to the model where the column has at most two terms, within 2 x the derived bound of
    long double everywhere; finite matrix (the sweeps run without the exponential's clamp) and a matrix with +inf (with it);
    f = 0 (exact targeting) and, on the finite matrix, f != 0."""
    rng = np.random.default_rng(K)
    f1 = np.round(rng.uniform(-3.0, 3.0, K), 3)
    for posinf in (False, True):
        u, live, n_probe = probe_matrix(K, posinf=posinf)
        with DM.from_host(u) as dm:
            for k, v in options.items():
                dm.set_option(k, v)
            dm.set_Nk(np.ones(K))
            for f in ((np.zeros(K),) if posinf else (np.zeros(K), f1)):
                got = dm.logden(f)
                assert got.shape == (u.shape[1],)
                check_logden(got, f, u, live, form, True, f"{tag} {'+inf' if posinf else 'finite'} f{'=0' if not f.any() else '!=0'}", n_probe)


@pytest.mark.parametrize("K,options", [(5, {}), (32, {"small_k_kernel": 0}), (64, {}), (128, {}), (192, {"wide_k_kernel": 1}), (192, {"wide_k_kernel": 0}),
                                       (300, {}), (700, {}), (40, {"force_generic": 1})])
def test_two_candidates_in_one_sweep(DM, K, options):
    """Second candidate of a two-candidate sweep: e' = e c_k with c_k = exp(a'_k - a_k) from the host, no second exponential
    (lse_math2).  Checked through sumlogden on a 59-column probe matrix (few terms in the sum), c_k up to e^+-30.
    Budget per column: the single-candidate bound + 2 u (c_k: library exp, 1 ulp) + 1 u (the product) + u |a' - a| (its argument)
    + the same for the row of the maximum, which is the FIRST candidate's; the sum over columns adds half an ulp of the running sum per
    addition (59 + 10 additions)."""
    plan = probe_plan()
    sel = np.linspace(0, plan["d"].size - 1, 54).astype(int)
    rng = np.random.default_rng(100 + K)
    f = np.round(rng.uniform(-1.0, 1.0, K), 3)
    f2 = f + np.round(rng.uniform(-30.0, 30.0, K), 2)
    u, live, n_probe = probe_matrix(K, offsets=(0.0,), plan={k: plan[k][sel] for k in ("c", "v", "d", "ties")})
    form = "generic" if options.get("force_generic") else "fma"
    with DM.from_host(u) as dm:
        for k, v in options.items():
            dm.set_option(k, v)
        dm.set_Nk(np.ones(K))
        psum, sld, _ = dm.eval(np.stack([f, f2]))
    for i, fv in enumerate((f, f2)):
        x, _ = gather(fv, u, live)
        ref = reference_columns(x)
        want = ref["logden"].sum()
        extra = 0.0 if i == 0 else 2 * (3.0 + float(np.max(np.abs(f2 - f))))
        col = logden_bound_u(ref, form) + extra
        acc = (u.shape[1] + 10) * float(M.ulp_of(np.abs(ref["logden"]).sum()) / (2 * U))
        err = float(abs(LD(sld[i]) - want) / U)
        print(f"two candidates K={K} {options}: candidate {i}: |sumlogden - long double| = {err:.1f} u, bound {float(col.sum()) + acc:.1f} u")
        assert err <= MARGIN * (float(col.sum()) + acc)


# ---------------------------------------------------------------------------------------------------------------------
# the resident probability matrix
# ---------------------------------------------------------------------------------------------------------------------
def p_problem(K, unsampled, posinf_entries=False, seed=0):
    """Probe columns (offsets of order one only) + harmonic columns; N_k = 1 on the sampled states (a0 = f0 exactly), 0 on `unsampled`.
    f0 = 0 keeps the probes' scaled arguments exactly on their targets (a0 = 0 on every sampled state).  With N_k = 1 and thousands of
    columns this is no consistent MBAR problem (sum N_k != N: its equations have no solution), which does not matter for P -- it is
    built at the start point before the first iteration -- but a full Newton step from there can leave the 250 kT window of the
    anchor, and the loop would then hand back and re-anchor: the ONE iteration allowed takes a damped step (gamma = 1e-3)."""
    rows = np.array([k for k in range(K) if k not in unsampled])
    O_k = np.linspace(0.0, 3.0, K)
    K_k = np.linspace(1.0, 2.5, K)
    nh = np.full(K, 40)
    _, uh, _, _ = ts.harmonic_u_kn(O_k, K_k, nh, seed=seed + K)
    if posinf_entries:
        uh = uh.copy()
        rng = np.random.default_rng(seed)
        for _ in range(200):
            uh[rng.integers(0, K), rng.integers(0, uh.shape[1])] = np.inf
        for k in range(K):                                    # (a sampled state keeps finite energies on some column)
            uh[k, k] = 0.5
    # (offsets of order one only: the probes that the plan puts at c = -2^k, up to -512, run at c = 0 here, an ulp off their exact
    # argument.  k_gram_quad and k_make_p do not normalise, so the sum of one of their columns is off by ~1.4 u per kT of |logden_n|
    # -- the |logden_n| terms of their bound; measured at |logden| = 512, f0 != 0: 355 ulp -- and "within K ulps" holds for |logden| << K.)
    plan = probe_plan()
    far = np.abs(plan["c"]) > 4
    plan = dict(c=np.where(far, 0.0, plan["c"]), v=np.where(far, plan["d"], plan["v"]), d=plan["d"], ties=plan["ties"])
    u, live, n_probe = probe_matrix(K, rows=rows, offsets=(0.0, 1.25, -3.75), extra_columns=uh, plan=plan)
    N_k = np.ones(K)
    N_k[list(unsampled)] = 0
    f0 = np.zeros(K)
    return u, live, n_probe, N_k, f0, rows


def p_reference(u, N_k, f0):
    """Long double P = exp(a0 - u - logden(a0)) of the whole matrix, with what the bounds need."""
    a = np.where(N_k > 0, f0, -np.inf).astype(LD)
    with np.errstate(invalid="ignore"):
        x = a[:, None] - u.astype(LD)
    x = np.where(np.isnan(x), -np.inf, x)
    m = np.max(x, axis=0)
    d = np.where(np.isneginf(x), LD(0), m[None, :] - x)
    e = np.where(np.isneginf(x), LD(0), np.exp(-d))
    s = e.sum(axis=0)
    return dict(a=a, x=x, m=m, d=d, p=e / s, s=s, logden=m + np.log(s), nnz=(e > 0).sum(axis=0))


def p_bound_u(ref, builder, K):
    """Relative bound of every entry (u), from the module docstring; R: additions on a term's way through the sum (tree over the
    register blocks + 4 DPP steps + the cross-wave sum), at most nnz - 1."""
    ax = np.where(np.isneginf(ref["x"]), LD(0), np.abs(ref["x"])).astype(np.float64)
    d = ref["d"].astype(np.float64)
    p = ref["p"].astype(np.float64)
    aa = np.where(np.isneginf(ref["a"]), 0.0, np.abs(ref["a"]).astype(np.float64))[:, None]
    R = np.minimum(np.maximum(ref["nnz"] - 1, 0), 12).astype(np.float64)[None, :]
    if builder in ("k_build_gram", "k_build_sweep"):
        theta = (aa if builder == "k_build_gram" else 0.0) + (1 + RHO_L) * ax + d + M.E_EXP_CLAIM
        return theta + (p * theta).sum(axis=0)[None, :] + R + 2
    red = dict(m=ref["m"], d=ref["d"], p=ref["p"], s=ref["s"], logden=ref["logden"], nnz=np.minimum(ref["nnz"], 13))
    ld_err = logden_bound_u(red, "fma")[None, :]
    ld = np.abs(ref["logden"]).astype(np.float64)[None, :]
    with np.errstate(divide="ignore"):
        lnp = np.where(p > 0, np.abs(np.log(np.maximum(ref["p"], LD(10.0) ** -4000))).astype(np.float64), 0.0)
    if builder == "k_gram_quad":
        return aa + ld + np.abs(np.where(np.isneginf(ref["a"]), LD(0), ref["a"]).astype(np.float64)[:, None] - ref["logden"].astype(np.float64)[None, :]) \
            + (1 + RHO_L) * lnp + M.E_EXP_CLAIM + ld_err
    return ax + lnp + 2 + ld_err  # k_make_p


def model_p(u, live, f0, builder):
    """P of the probe columns' live rows by the model of the two build sweeps (bit for bit where the column has <= 2 terms)."""
    n = np.arange(live.shape[0])
    ul = np.full((LMAX, live.shape[0]), np.inf)
    al = np.zeros((LMAX, live.shape[0]))
    for i in range(LMAX):
        ok = live[:, i] >= 0
        ul[i, ok] = u[live[ok, i], n[ok]]
        al[i, ok] = f0[live[ok, i]]
    pad = np.isinf(ul)
    if builder == "k_build_gram":
        x = M.fma(np.where(pad, 0.0, ul), -C.LOG2E_S, al * C.LOG2E_S)
        x = np.where(pad, -np.inf, x)
        m = np.max(x, axis=0)
        w = np.where(pad, 2.0e9, m[None, :] - np.where(pad, 0.0, x))
        e = M.exp2s_neg(w, True, C)
    else:
        x = np.where(pad, -np.inf, al - np.where(pad, 0.0, ul))
        m = np.max(x, axis=0)
        m2 = m * C.LOG2E_S
        t = M.fma(np.where(pad, 0.0, x), C.LOG2E_S, np.broadcast_to(-m2, x.shape))
        e = M.exp2s(np.where(pad, C.EXP2_CLAMP, t), True, C)
    e = np.where(pad, 0.0, e)
    return e, e.sum(axis=0)


P_BUILDERS = [
    # (builder, K, options, weighted): which kernel writes P (mbar_loop_device.cpp)
    ("k_build_gram", 48, {}, False), ("k_build_gram", 128, {}, False), ("k_build_gram", 48, {}, True),
    ("k_build_sweep", 48, {"fused": 0}, False), ("k_build_sweep", 128, {"fused": 0}, False), ("k_build_sweep", 48, {"fused": 0}, True),
    ("k_gram_quad", 160, {}, False), ("k_gram_quad", 256, {}, False),
    ("k_make_p", 160, {}, True), ("k_make_p", 256, {}, True),
]


def build_and_download(DM, u, N_k, f0, options, weights):
    with DM.from_host(u) as dm:
        for k, v in options.items():
            dm.set_option(k, v)
        dm.set_Nk(N_k)
        dm.set_sample_weights(weights)
        _, res = dm.solve_adaptive(f0, min_sc_iter=0, maxiter=1, gamma=1e-3, check_convergence=False)
        assert res["builds"] == 1 and res["warm_starts"] == 0, res
        dm.set_option("debug_download_p", 1)
        try:
            P = dm.to_host()
        finally:
            dm.set_option("debug_download_p", 0)
        np.testing.assert_array_equal(dm.to_host(), u)
    return P


def check_p(P, u, live, n_probe, N_k, f0, builder, K, tag):
    ref = p_reference(u, N_k, f0)
    want = ref["p"]
    assert P.shape == u.shape and np.all(np.isfinite(P)) and np.all(P >= 0)
    assert np.all(P[N_k == 0] == 0.0), "rows of unsampled states must be exactly zero"
    bound = p_bound_u(ref, builder, K)
    tiny = LD(2.0) ** -1022
    eps = MARGIN * bound * float(U) + 2.0 ** -40
    hi = want >= tiny * (1 + eps)          # at or above the normal range, clear of the boundary: the relative bound
    lo = want < tiny * (1 - eps)           # below it: the subnormal rule of the builder (between the two: either)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(hi, np.abs(P.astype(LD) / np.where(hi, want, LD(1)) - 1) / U, LD(0)).astype(np.float64)
    ratio = rel / bound
    k, n = np.unravel_index(np.argmax(ratio), ratio.shape)
    line = f"{tag}: worst relative error {rel.max():.2f} u; worst error / derived bound {ratio[k, n]:.3f} (row {k}, column {n}, d = {float(ref['d'][k, n]):.4g})"
    print(line)
    assert ratio[k, n] <= MARGIN, (tag, k, n, rel[k, n], bound[k, n])
    sub_ulp = LD(2.0) ** -1074
    if builder in ("k_build_gram", "k_build_sweep"):
        # not flushed: ldexp rounds once into the subnormal range, the product with 1/s once more (half a subnormal ulp each)
        err_sub = (np.abs(P.astype(LD) - want) / sub_ulp).astype(np.float64)
        rel_share = (want[lo] * (MARGIN * bound[lo].astype(LD) * U) / sub_ulp).astype(np.float64)
        assert np.all(err_sub[lo] <= 1.0 + rel_share), tag
        kept = int(np.sum((P > 0) & (P < 2.0 ** -1022)))
        assert kept > 0
        line = f"  {kept} subnormal entries kept, worst {np.max(err_sub[lo] - rel_share):.2f} subnormal ulp beyond the relative share"
    else:
        # flushed: exactly zero below the normal range, and nothing subnormal anywhere
        assert np.all(P[lo] == 0.0), tag
        assert not np.any((P > 0) & (P < 2.0 ** -1022)), tag
        line = f"  {int(np.sum(lo & (want > 0)))} entries below 2^-1022 flushed to 0"
    lost = np.where(P == 0, want, LD(0)).sum(axis=0)
    assert float(lost.max()) < 1e-199
    colsum = P.astype(LD).sum(axis=0)
    cs_err = float(np.max(np.abs(colsum - 1)) / (2 * U))
    line += f"; column sums within {cs_err:.2f} ulp of 1"
    assert cs_err <= K
    if builder in ("k_build_gram", "k_build_sweep"):
        me, ms = model_p(u[:, :live.shape[0]], live, f0, builder)
        # the reciprocal: from the correctly rounded seed, and where 1/s sits next to a rounding boundary (recip_candidates differ: the
        # result then depends on the hardware estimate) either neighbour's outcome -- an explicit list of values, not a share
        r0, r_up, r_dn = M.recip_candidates(ms)
        seed_dep = (r0 != r_up) | (r0 != r_dn)
        two = reference_columns(gather(f0, u[:, :live.shape[0]], live)[0])["nnz"] <= 2
        n_idx = np.arange(live.shape[0])
        total = mism = other = 0
        where = []
        for i in (0, LMAX - 1):
            ok = two & (live[:, i] >= 0)
            got = P[live[ok, i], n_idx[ok]]
            total += int(ok.sum())
            bad = got != (me[i] * r0)[ok]
            alt = seed_dep[ok] & ((got == (me[i] * r_up)[ok]) | (got == (me[i] * r_dn)[ok]))
            other += int(np.sum(bad & alt))
            bad &= ~alt
            mism += int(bad.sum())
            where += [(int(live[n, i]), int(n), float(P[live[n, i], n]).hex(), float(me[i, n] * r0[n]).hex(), float(u[live[n, 0], n]), float(u[live[n, LMAX - 1], n]))
                      for n in n_idx[ok][bad][:4]]
        line += f"; {int(np.sum(seed_dep & two))} columns with a seed-dependent reciprocal, {other} entries on the other candidate"
        line += f"; bit-identical to the model on {total - mism} of {total} entries of columns with <= 2 terms"
        print(line)
        assert mism == 0, (tag, where)  # (row, column, device, model, entry of the maximum row, entry of the probe row)
    else:
        print(line)
    return ref, bound


@pytest.mark.parametrize("builder,K,options,weighted", P_BUILDERS, ids=[f"{b}-K{k}-{'weighted' if w else 'plain'}-{'-'.join(f'{a}{v}' for a, v in o.items())}" for b, k, o, w in P_BUILDERS])
def test_resident_probability_matrix_elementwise(DM, builder, K, options, weighted):
    """P of ONE build (builds == 1), downloaded through debug_download_p, against long double entry by entry.
    k_build_gram: K <= 128, fused loop (default); GENERAL = false on the plain first solve, true with sample weights or +inf entries.
    k_build_sweep: K <= 128, option fused = 0.   k_gram_quad (STOREP): 129 .. 256 states, fused, unweighted.
    k_make_p (launch_make_p): 129 .. 256 states with sample weights.  (Above 256 states the host-driven loop builds its P with the same
    kernel, but that matrix is not the device-resident loop's -- it is never marked valid for a warm start -- and the download hook
    refuses it; the kernel is the one checked here.)
    With sample weights P itself is unweighted (the multiplicity rides on the operand only).
    Limitation: WHICH kernel and template branch wrote P follows from mbar_loop_device.cpp and is not observable through the C ABI (the
    result record counts builds, not kernels); GENERAL = false / true of k_build_gram give the same bits on these matrices, so a
    plain solve that went through GENERAL = true would pass here."""
    unsampled = (5, K - 2)
    for posinf in (False, True):
        u, live, n_probe, N_k, f0, rows = p_problem(K, unsampled, posinf_entries=posinf)
        weights = None
        if weighted:
            weights = np.random.default_rng(K).integers(0, 4, u.shape[1]).astype(np.float64)
            weights[:8] = 1.0
        # anchor a0 = 0 (exact targeting), and on the finite matrix once more at an anchor of order one: the |a_k| terms of the bounds,
        # RN(a LOG2E_S) of k_build_gram, RN(aL - logden L) of k_gram_quad, RN(a - u) of the other two, each row with its OWN a_k
        f1 = np.where(N_k > 0, np.round(np.random.default_rng(7 * K).uniform(-1.5, 1.5, K), 3), 0.0)
        for fa in ((f0,) if posinf else (f0, f1)):
            P = build_and_download(DM, u, N_k, fa, options, weights)
            check_p(P, u, live, n_probe, N_k, fa, builder, K,
                    f"{builder} K={K} {options} {'weighted' if weighted else 'plain'}{' +inf' if posinf else ''} f0{'=0' if not fa.any() else '!=0'}")


@pytest.mark.parametrize("K,variants", [
    (48, [("k_build_gram", {}, False), ("k_build_sweep", {"fused": 0}, False), ("k_build_gram", {}, True)]),
    (160, [("k_gram_quad", {}, False), ("k_make_p", {}, True)]),
])
def test_p_builders_agree_on_the_same_matrix_and_anchor(DM, K, variants):
    """The builders that serve one range of state counts (<= 128: k_build_gram, k_build_sweep; 129 .. 256: k_gram_quad, k_make_p), on the
    same matrix and anchor: entries at or above 2^-1022 agree within the SUM of their bounds (x the margin)."""
    u, live, n_probe, N_k, f0, rows = p_problem(K, (5, K - 2))
    out = []
    for builder, options, weighted in variants:
        weights = np.random.default_rng(K).integers(0, 4, u.shape[1]).astype(np.float64) if weighted else None
        out.append((builder, build_and_download(DM, u, N_k, f0, options, weights)))
    ref = p_reference(u, N_k, f0)
    safe = ref["p"] >= LD(2.0) ** -1021
    for i in range(len(out)):
        for j in range(i + 1, len(out)):
            bsum = p_bound_u(ref, out[i][0], K) + p_bound_u(ref, out[j][0], K)
            with np.errstate(divide="ignore", invalid="ignore"):
                rel = np.where(safe, np.abs(out[i][1] / np.where(safe, out[j][1], 1.0) - 1) / float(U), 0.0)
            print(f"K={K}: {out[i][0]} vs {out[j][0]}: worst disagreement {rel.max():.2f} u, worst / summed bound {np.max(rel / bsum):.3f}")
            assert np.all(rel <= MARGIN * bsum)


@pytest.mark.parametrize("builder,weighted", [("k_gram_quad", False), ("k_make_p", True)])
def test_normal_entries_just_above_the_flush_threshold_are_kept(DM, builder, weighted):
    """The case that exposed it: k_gram_quad and k_make_p flushed "below 2.3e-308", which also zeroed the NORMAL entries in
    [2^-1022, 2.3e-308) -- relative error 1 where the bound is ~1e3 x 2^-53.  The threshold is the smallest normal number: every
    entry whose exact value lies in that sliver (clear of 2^-1022 by the bound) comes back nonzero and within the bound."""
    K = 160
    u, live, n_probe, N_k, f0, rows = p_problem(K, (5, K - 2))
    weights = np.random.default_rng(K).integers(0, 4, u.shape[1]).astype(np.float64) if weighted else None
    P = build_and_download(DM, u, N_k, f0, {}, weights)
    ref = p_reference(u, N_k, f0)
    bound = p_bound_u(ref, builder, K)
    tiny = LD(2.0) ** -1022
    sliver = (ref["p"] >= tiny * (1 + MARGIN * bound * float(U) + 2.0 ** -40)) & (ref["p"] < LD(2.3e-308))
    assert sliver.sum() >= 4, "the probes at t = -1022 S + 0.5 ... 3 must land in the sliver"
    assert np.all(P[sliver] >= 2.0 ** -1022)
    rel = (np.abs(P[sliver].astype(LD) / ref["p"][sliver] - 1) / U).astype(np.float64)
    print(f"{builder}: {int(sliver.sum())} entries in [2^-1022, 2.3e-308), worst relative error {rel.max():.1f} u (bound {bound[sliver].max():.0f} u)")
    assert np.all(rel <= MARGIN * bound[sliver])
