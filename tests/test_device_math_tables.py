"""The constants and the arithmetic of the hand-made device exp / log / reciprocal (pymbar_amd/csrc/mbar_device.h), checked on
the CPU against ``np.longdouble`` (64-bit mantissa): the tables entry by entry, the polynomials on dense grids, and the
step-by-step model of tests/device_math_model.py on grids that aim at every table index, the rounding ties, the table wrap, both
subnormal boundaries, the clamp and the int32 saturation.  No GPU is needed: the model reads the very files the compiler reads.

Units.  u = 2^-53 (half an fp64 ulp of a number in [1, 2)).  Relative errors are |got / want - 1| / u, absolute ones |got - want| / u.
Long-double slop: expl / logl / exp2l of glibc are good to 1 ulp of long double = 2^-63 relative = 2^-10 u; every bound below
carries SLOP = 2^-9 u (the reference's own error, twice over).

Claims asserted here (mbar_device.h states them next to the code):
  EXP2_POLY   relative error <= 9e-18 on z in [-1/2, 1/2]                     (exp2_table.inc: 8.57e-18)
  EXP2N_POLY  relative error <= 8.8e-18 on z in [0, 1]
  log1p       degree-6 Taylor polynomial, absolute error <= 2e-18 on |r| <= 2^-8
  exp2s_*     relative error <= E_EXP_CLAIM = 3.1 u for normal results: 1 u table entry (half an ulp of T in [1, 2)) + 1 u last
              fma of the polynomial (p in [1 - 2e-4, 1 + 2e-4]) + 1 u product T p + 0.1 u polynomial and inner roundings; ldexp is exact
              there.  Subnormal results: half a subnormal ulp more (ldexp rounds once, to nearest-even).
  log_pos     absolute error <= (1.6 + |e| / 2) u + 1 ulp(log s), s = 2^e m:  1 u from r = fma(m, 1/c_j, -1) (the
              rounded 1/c_j), 1/2 u from the rounded log c_j, |e| / 2 u from the rounded LN2, half an ulp of the result each from
              fma(e, LN2, log c_j) and from the closing fma.  NOT the flat "~2e-16" the header used to state: for s >= 4 the
              half ulps of the result dominate (log 1000 = 6.9 carries 8 u per ulp)."""
import numpy as np

from tests import device_math_model as M

LD = M.LD
U = LD(2.0) ** -53
SLOP = 2.0 ** -9  # in u
E_EXP_CLAIM = M.E_EXP_CLAIM
log_bound_u = M.log_bound_u
C = M.constants()
S = C.S


def rel_u(got, want):
    return np.abs(np.asarray(got, LD) / np.asarray(want, LD) - 1) / U


# ---------------------------------------------------------------------------------------------------------------------
# the model's own arithmetic
# ---------------------------------------------------------------------------------------------------------------------
def test_long_double_and_parser():
    assert np.finfo(LD).nmant == 63
    assert (C.EXP2_BITS, C.EXP2_DEG, S) == (11, 3, 2048)
    assert C.EXP2_TABLE.shape == (2048,) and C.LOG_TABLE.shape == (256,) and C.EXP2N_POLY.shape == (4,)
    assert C.EXP2_CLAMP == -1100.0 * 2048
    # LOG2E, LN2 are the correctly rounded constants
    assert abs(LD(C.LOG2E) - 1 / M.LN2_LD) <= LD(2.0) ** -53 * (1 + 2.0 ** -9)
    assert abs(LD(C.LN2) - M.LN2_LD) <= LD(2.0) ** -54 * (1 + 2.0 ** -9)


def test_model_fma_is_exact():
    rng = np.random.default_rng(11)
    n = 4000
    a = rng.standard_normal(n) * 2.0 ** rng.integers(-40, 40, n)
    b = rng.standard_normal(n) * 2.0 ** rng.integers(-40, 40, n)
    c = rng.standard_normal(n) * 2.0 ** rng.integers(-40, 40, n)
    c[:1500] = -(a * b)[:1500] * (1 + rng.integers(-3, 4, 1500) * 2.0 ** -52)     # cancellation: the low product bits decide
    a[1500:1700] = 1 + 2.0 ** -30                                                    # a b = half an ulp of c, +- a hair: ties
    b[1500:1700] = 2.0 ** -53 * (1 + 2.0 ** -30 * rng.integers(-1, 2, 200))
    c[1500:1700] = 1.0 + rng.integers(0, 4, 200) * 2.0 ** -52
    a[1700:1720], b[1700:1720] = 1e300, rng.standard_normal(20) * 2954.0            # the huge sentinels of the sweeps
    a[1720:1740], c[1720:1740] = 0.0, rng.standard_normal(20)
    a[1740:1760], b[1740:1760], c[1740:1760] = 2.0 ** -600, 2.0 ** -450 * rng.standard_normal(20), 2.0 ** -1060  # subnormal results
    got = M.fma(a, b, c)
    want = np.array([M.fma_fraction(x, y, z) for x, y, z in zip(a, b, c)])
    assert np.array_equal(got, want)
    assert np.array_equal(np.signbit(got), np.signbit(want))
    assert not np.array_equal(got[:1700], (a * b + c)[:1700])  # (the cases do tell an fma from multiply-add)


def test_model_ldexp_rounds_once_into_the_subnormal_range():
    rng = np.random.default_rng(12)
    x = 1.0 + rng.random(3000)
    x[:8] = [1.0, 1.5, 1.25, 1.75, 1.0 + 2.0 ** -52, 2.0 - 2.0 ** -52, 1.5 + 2.0 ** -52, 1.5 - 2.0 ** -52]
    q = rng.integers(-1080, -1015, x.size)
    q[:8] = -1075  # ties of the smallest subnormal and its neighbours
    got = M.ldexp(x, q)
    want = np.array([M.ldexp_fraction(v, k) for v, k in zip(x, q)])
    assert np.array_equal(got, want)
    assert got[0] == 0.0 and got[1] == 2.0 ** -1074 and got[4] == 2.0 ** -1074  # tie to even, above the tie
    assert M.ldexp(np.array([1.3]), np.array([-(1 << 20)]))[0] == 0.0 and np.isinf(M.ldexp(np.array([1.3]), np.array([1 << 20]))[0])


# ---------------------------------------------------------------------------------------------------------------------
# tables
# ---------------------------------------------------------------------------------------------------------------------
def test_exp_table_is_correctly_rounded():
    j = np.arange(S)
    want = np.exp2(j.astype(LD) / LD(S))
    err = np.abs(M.err_ulps(C.EXP2_TABLE, want))
    worst = int(np.argmax(err))
    print(f"EXP2_TABLE: worst |T[j] - 2^(j/S)| = {float(err[worst]):.4f} ulp at j = {worst}")
    assert C.EXP2_TABLE[0] == 1.0
    assert np.all(err <= 0.5 + SLOP / 2), (worst, float(err[worst]))  # (SLOP is in u = half ulps)
    assert np.all(np.diff(C.EXP2_TABLE) > 0) and C.EXP2_TABLE[-1] < 2.0


def test_log_table_pairs_and_buckets():
    j = np.arange(128)
    c = (1.0 + (j + 0.5) / 128.0) / 2.0                    # exact in fp64
    rc, lc = C.LOG_TABLE[0::2], C.LOG_TABLE[1::2]
    e_rc = np.abs(M.err_ulps(rc, 1 / c.astype(LD)))
    e_lc = np.abs(M.err_ulps(lc, np.log(c.astype(LD))))
    print(f"LOG_TABLE: worst 1/c_j {float(e_rc.max()):.4f} ulp, worst log c_j {float(e_lc.max()):.4f} ulp")
    assert np.all(e_rc <= 0.5 + SLOP / 2), int(np.argmax(e_rc))
    assert np.all(e_lc <= 0.5 + SLOP / 2), int(np.argmax(e_lc))
    first = (128.0 + j) / 256.0
    last = np.nextafter((129.0 + j) / 256.0, 0.0)
    for m in (first, last):
        assert np.array_equal(M.log_bucket(m), j)
        assert np.all(np.abs(m.astype(LD) / c.astype(LD) - 1) <= LD(2.0) ** -8)
    # the same through frexp at other exponents
    for e in (-1021, -40, -1, 0, 1, 2, 7, 1023):
        for m in (first, last):
            _, parts = M.log_pos(np.ldexp(m, e), C, parts=True)
            assert np.array_equal(parts["j"], j) and np.all(parts["e"] == e) and np.array_equal(parts["m"], m)


# ---------------------------------------------------------------------------------------------------------------------
# polynomials
# ---------------------------------------------------------------------------------------------------------------------
def _horner_ld(coef, z):
    p = np.zeros_like(z)
    for v in coef[::-1]:
        p = p * z + LD(v)
    return p


def poly_errors():
    z = np.linspace(LD(-0.5), LD(0.5), 400001, dtype=LD)
    e_p = float(np.max(np.abs(_horner_ld(C.EXP2_POLY, z) / np.exp2(z / S) - 1)))
    z = np.linspace(LD(0), LD(1), 400001, dtype=LD)
    e_n = float(np.max(np.abs(_horner_ld(C.EXP2N_POLY, z) / np.exp2(-z / S) - 1)))
    r = np.linspace(-LD(2.0) ** -8, LD(2.0) ** -8, 400001, dtype=LD)
    e_l = float(np.max(np.abs(_horner_ld(C.LOG1P, r) * r - np.log1p(r))))
    return e_p, e_n, e_l


def test_polynomials_within_their_stated_errors():
    e_p, e_n, e_l = poly_errors()
    print(f"EXP2_POLY rel err {e_p:.3e} (claim 9e-18); EXP2N_POLY rel err {e_n:.3e} (claim 8.8e-18); "
          f"log1p degree 6 abs err {e_l:.3e} (claim 2e-18)")
    assert C.EXP2_POLY[0] == 1.0 and C.EXP2N_POLY[0] == 1.0
    assert e_p <= 9e-18
    assert e_n <= 8.8e-18
    assert e_l <= 2e-18


# ---------------------------------------------------------------------------------------------------------------------
# model against long double on the edge grids
# ---------------------------------------------------------------------------------------------------------------------
def _neighbours(x):
    x = np.asarray(x, np.float64)
    return np.concatenate([x, np.nextafter(x, -np.inf), np.nextafter(x, np.inf)])


def exp_grid():
    """Arguments ts (units of 1/S) of 2^(ts/S): every table index at several exponents, every tie z = +-1/2 with its fp64
    neighbours (that includes the wrap j = 2047 -> 0), both subnormal boundaries, the clamp, zero."""
    j = np.arange(S, dtype=np.float64)
    parts = [j + S * q for q in (0, 1, -1, -7, -300, -1021, -1022, -1023, -1050, -1073, -1074, -1075)]
    parts += [_neighbours(j + 0.5 + S * q) for q in (0, -1, -2, -1022, -1023)]
    parts += [j + S * q + z for q in (0, -3) for z in (-0.4999, -0.25, 0.25, 0.4999)]
    for b in (-1022, -1074, -1075, -1076):
        parts.append(_neighbours(S * float(b) + np.arange(-3.0, 3.5, 0.5)))
    parts.append(_neighbours(np.array([0.0, C.EXP2_CLAMP, C.EXP2_CLAMP + 0.5, C.EXP2_CLAMP - 0.5, S * 1023.0, S * 1023.0 + 2047.49])))
    rng = np.random.default_rng(5)
    parts.append(rng.uniform(-1080.0 * S, 3.0 * S, 60000))
    return np.concatenate(parts)


def exp_errors(fn, ts, sign):
    """Worst relative error (u) over normal results, worst error in subnormal ulps beyond the relative share below 2^-1022."""
    got, parts = fn(ts, parts=True)
    want = M.ld_exp2s(sign * ts, C)
    normal = want >= LD(2.0) ** -1022
    finite = want < LD(2.0) ** 1024
    nrm = normal & finite
    e_rel = rel_u(got[nrm], want[nrm])
    sub = ~normal
    e_sub = np.abs(M.err_ulps(got[sub], want[sub])) if sub.any() else np.zeros(1)
    rel_share = want[sub] * (E_EXP_CLAIM * U) / LD(2.0) ** -1074 if sub.any() else np.zeros(1)
    return e_rel, e_sub, rel_share, parts, got, want


def test_exp2s_model_against_long_double():
    ts = exp_grid()
    worst = {}
    for name, clamp in (("exp2s_batch<CLAMP=true> / exp2s_fast / exp2s_batch2", True), ("exp2s_batch<CLAMP=false>", False)):
        e_rel, e_sub, share, parts, got, want = exp_errors(lambda t, parts: M.exp2s(t, clamp, C, parts), ts, 1.0)
        assert set(parts["j"].tolist()) == set(range(S))
        assert np.any(np.abs(parts["z"]) == 0.5)
        worst[name] = float(e_rel.max())
        print(f"E_exp  {name}: worst relative error {float(e_rel.max()):.3f} u = {float(e_rel.max()) / 2:.3f} ulp; "
              f"subnormal results: worst {float(e_sub.max()):.3f} subnormal ulp")
        assert e_rel.max() <= E_EXP_CLAIM + SLOP
        assert np.all(e_sub <= 0.5 + share + SLOP)
    # ties round to even: z = +1/2 below an even integer, -1/2 above it; the wrap takes q along
    r, p = M.exp2s(np.array([2047.5, 2048.5, -0.5, -1.5, 0.5, 1.5]), True, C, True)
    assert p["j"].tolist() == [0, 0, 0, 2046, 0, 2] and p["q"].tolist() == [1, 1, 0, -1, 0, 0]
    assert p["z"].tolist() == [-0.5, 0.5, -0.5, 0.5, 0.5, -0.5]
    # argument 0, the clamp (and everything below it, -inf and NaN included), int32 saturation without the clamp, overflow
    assert M.exp2s(np.array([0.0]))[0] == 1.0
    low = np.array([C.EXP2_CLAMP, C.EXP2_CLAMP - 1.0, -1e7, -3e9, -1e300, -np.inf, np.nan])
    assert np.all(M.exp2s(low, True) == 0.0)
    r, p = M.exp2s(np.array([-2147483648.0, -2147483649.0, -3e9, -1e15, -1e300, -1.7e308]), False, C, True)
    assert np.all(r == 0.0) and np.all(p["si"] == -(1 << 31)) and np.all(p["q"] == -(1 << 20)) and np.all(p["j"] == 0)
    assert np.isinf(M.exp2s(np.array([1024.0 * S]))[0]) and np.isfinite(M.exp2s(np.array([1024.0 * S - 1]))[0])
    # both sides of 2^-1022 and 2^-1074 exactly
    r = M.exp2s(np.array([-1022.0 * S, -1023.0 * S, -1074.0 * S, -1075.0 * S, -1075.0 * S + 1, -1076.0 * S]))
    assert r.tolist() == [2.0 ** -1022, 2.0 ** -1023, 2.0 ** -1074, 0.0, 2.0 ** -1074, 0.0]


def expn_grid():
    j = np.arange(S, dtype=np.float64)
    parts = [j + S * q for q in (0, 1, 6, 300, 1021, 1022, 1023, 1050, 1073, 1074, 1075)]
    parts += [np.nextafter(j + 1.0 + S * q, 0.0) for q in (0, 2, 1022)]              # z = the largest fraction below 1
    parts += [j + S * q + z for q in (0, 3) for z in (2.0 ** -30, 0.25, 0.5, 0.75, 0.9999)]
    for b in (1022, 1074, 1075, 1076):
        parts.append(_neighbours(S * float(b) + np.arange(-3.0, 3.5, 0.5)))
    parts.append(np.array([0.0, 2.0 ** -1074, 2.0 ** -60, np.nextafter(1.0, 0.0), 1.0, np.nextafter(2048.0, 0.0), 2048.0]))
    rng = np.random.default_rng(6)
    parts.append(rng.uniform(0.0, 1080.0 * S, 60000))
    return np.concatenate(parts)


def test_exp2s_neg_model_against_long_double():
    w = expn_grid()
    for name, clamp in (("exp2s_neg_batch<CLAMP=false>", False), ("exp2s_neg_batch<CLAMP=true>", True)):
        e_rel, e_sub, share, parts, got, want = exp_errors(lambda t, parts: M.exp2s_neg(t, clamp, C, parts), w, -1.0)
        assert set(parts["j"].tolist()) == set(range(S))
        assert parts["z"].max() == np.nextafter(1.0, 0.0) and parts["z"].min() == 0.0
        print(f"E_expn {name}: worst relative error {float(e_rel.max()):.3f} u = {float(e_rel.max()) / 2:.3f} ulp; "
              f"subnormal results: worst {float(e_sub.max()):.3f} subnormal ulp")
        assert e_rel.max() <= E_EXP_CLAIM + SLOP
        assert np.all(e_sub <= 0.5 + share + SLOP)
    # the negated truncating conversion: n = -trunc(w); n >> 11 floors, (n << 3) & mask wraps 0 -> 2047
    r, p = M.exp2s_neg(np.array([0.0, 0.75, 1.0, 1.5, 2047.0, 2048.0, 2049.0]), False, C, True)
    assert p["si"].tolist() == [0, 0, -1, -1, -2047, -2048, -2049]
    assert p["j"].tolist() == [0, 0, 2047, 2047, 1, 0, 2047] and p["q"].tolist() == [0, 0, -1, -1, -1, -1, -2]
    assert r[0] == 1.0 and r[5] == 0.5
    # int32 saturation for huge finite arguments (no clamp), +inf with the clamp
    r, p = M.exp2s_neg(np.array([2147483648.0, 3e9, 1e15, 2.0 ** 52, 1e300, 1.7e308]), False, C, True)
    assert np.all(r == 0.0) and np.all(p["si"] == -(1 << 31)) and np.all(p["z"] == 0.0)
    assert np.all(M.exp2s_neg(np.array([np.inf, 1e300, 2.0e9, 2.5e6]), True) == 0.0)
    r = M.exp2s_neg(np.array([1022.0 * S, 1023.0 * S, 1074.0 * S, 1075.0 * S, 1075.0 * S - 1, 1076.0 * S]))
    assert r.tolist() == [2.0 ** -1022, 2.0 ** -1023, 2.0 ** -1074, 0.0, 2.0 ** -1074, 0.0]


def log_grid():
    j = np.arange(128)
    first = (128.0 + j) / 256.0
    last = np.nextafter((129.0 + j) / 256.0, 0.0)
    mid = (128.5 + j) / 256.0
    parts = []
    for e in (-1021, -996, -300, -8, -2, -1, 0, 1, 2, 3, 4, 7, 10, 11, 64, 300, 1024):
        parts += [np.ldexp(first, e), np.ldexp(last, e), np.ldexp(mid, e)]
    one = np.array([1.0])
    for k in range(1, 40):
        parts += [1.0 + 2.0 ** -k * one, 1.0 - 2.0 ** -k * one]
    parts.append(np.array([1.0, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0), 1e-300, 1e300, 2.0 ** -1022, np.finfo(np.float64).max]))
    rng = np.random.default_rng(7)
    parts += [np.exp(rng.uniform(-20.0, 20.0, 40000)), 1.0 + rng.uniform(-2.0 ** -7, 2.0 ** -7, 20000), 1.0 + rng.random(20000),
              np.arange(1.0, 1100.0)]
    return np.concatenate(parts)


def test_log_pos_model_against_long_double():
    s = log_grid()
    got, parts = M.log_pos(s, C, parts=True)
    want = np.log(s.astype(LD))
    err = (np.abs(got.astype(LD) - want) / U).astype(np.float64)
    assert set(parts["j"].tolist()) == set(range(128))
    assert np.all(np.abs(parts["r"]) <= 2.0 ** -8)
    in12 = (s >= 1.0) & (s < 2.0)
    print(f"E_log  log_pos: worst absolute error {err[in12].max():.3f} u for s in [1, 2); {err[(s >= 0.5) & (s < 1)].max():.3f} u for s in [1/2, 1); "
          f"{err[(s >= 2) & (s <= 1100)].max():.3f} u for s in [2, 1100]; worst error / bound over the grid {np.max(err / log_bound_u(s, want)):.3f}")
    assert np.all(err <= log_bound_u(s, want) + SLOP)
    # (log_pos(1) is NOT exactly 0: 1 = 2^1 x 1/2 goes through bucket 0, and ln2 + log c_0 + log1p(r) leaves 0.39 u)
    assert abs(M.log_pos(np.array([1.0]))[0]) <= 2.0 ** -53
    # without the contraction of the closing multiply-add the same bound holds (the device code may be built either way)
    got2 = M.log_pos(s, C, contract=False)
    assert np.all(np.abs(got2.astype(LD) - want) / U <= log_bound_u(s, want) + 0.5 * (M.ulp_of(want) / U) + SLOP)


def test_recip_fast_model_is_the_correctly_rounded_reciprocal():
    rng = np.random.default_rng(8)
    s = np.concatenate([1.0 + rng.random(50000), np.exp(rng.uniform(0, 7, 20000)), np.arange(1.0, 1030.0), [2.0 ** -300, 1e300]])
    r = M.recip_fast(s)
    err = np.abs(M.err_ulps(r, 1 / s.astype(LD)))
    print(f"recip_fast (model, seed = RN(1/s)): worst error {float(err.max()):.4f} ulp")
    assert np.all(err <= 0.5 + SLOP)
    # a poor seed (2^-20 relative, far worse than the hardware estimate) ends at the same bits: after the first step the error is
    # 2^-40, the second returns RN((1/s)(1 - 2^-80)), which differs from RN(1/s) only where 1/s lies within 2^-80 of a rounding
    # boundary -- 2^-27 of all arguments, none among these 71 000.  Counted, not tolerated by a share.
    r2 = (1.0 / s) * (1 + 2.0 ** -20)
    for _ in range(2):
        r2 = M.fma(M.fma(-s, r2, 1.0), r2, r2)
    assert int(np.sum(r2 != r)) == 0


# ---------------------------------------------------------------------------------------------------------------------
# the polynomial coefficients, bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def _generator_line(script, *args):
    import os
    import subprocess
    import sys

    out = subprocess.run([sys.executable, os.path.join(M.ROOT, "tools", script), *args], check=True, capture_output=True, text=True).stdout
    line = [ln for ln in out.splitlines() if "_POLY[" in ln][0]
    return np.array([float.fromhex(t) if "0x" in t else float(t) for t in line[line.index("{") + 1:line.index("}")].split(",")])


def test_generators_reproduce_the_committed_polynomials():
    """tools/gen_exp2n_poly.py writes EXP2N_POLY of mbar_device.h, tools/gen_exp2_table.py EXP2_POLY of exp2_table.inc: every bit.
    (A changed last hex digit of a cubic coefficient moves the result by 2^-77 relative -- far below the error checks above.)"""
    assert np.array_equal(_generator_line("gen_exp2n_poly.py"), C.EXP2N_POLY)
    assert np.array_equal(_generator_line("gen_exp2_table.py", "--check"), C.EXP2_POLY)


def test_coefficient_probes_see_the_last_bit():
    import copy

    for (which, idx), hexes in M.COEFFICIENT_PROBES.items():
        d = np.array([float.fromhex(h) for h in hexes])
        w = d * C.LOG2E_S
        fn = (lambda cc: M.exp2s_neg(w, False, cc)) if which == "EXP2N_POLY" else (lambda cc: M.exp2s(-w, True, cc))
        base = fn(C)
        cp = copy.copy(C)                                    # the coefficient one ulp up (the direction the probes were searched in)
        arr = getattr(C, which).copy()
        arr[idx] = np.nextafter(arr[idx], np.inf)
        setattr(cp, which, arr)
        e1 = fn(cp)
        assert (e1 != base).all(), (which, idx)
        # what the device shows of it: P = e / (1 + e) of the build sweeps, logden = log(1 + e) of the evaluation sweeps
        p0, p1 = base * M.recip_fast(1.0 + base), e1 * M.recip_fast(1.0 + e1)
        assert (p0 != p1).any(), (which, idx)
        if which == "EXP2_POLY":
            assert (M.log_pos(1.0 + base) != M.log_pos(1.0 + e1)).any(), (which, idx)
