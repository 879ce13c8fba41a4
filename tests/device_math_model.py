"""The hand-made device exp / log / reciprocal of pymbar_amd/csrc/mbar_device.h restated in numpy, one statement per
device instruction and in the same order, so that half-ulp effects of the device functions can be resolved on the CPU.

* The constants are PARSED from the files the compiler reads (exp2_table.inc, log_table.inc, mbar_device.h): the model
  holds no copy of them, and a hand edit of a table shows up in the model as it does on the device.  The one exception are the six
  Taylor coefficients of log1p, which log_pos writes as literals inside its fma chain (1, -1/2, 1/3, -1/4, 1/5, -1/6): the model
  restates them (Constants.LOG1P).
* ``fma`` is exact (one rounding).  ``math.fma`` is used where the interpreter has it; otherwise the product is split
  error-free (Veltkamp / Dekker) and the three-term sum is rounded once with the round-to-odd scheme of Boldo and
  Melquiond ("Emulation of a FMA and correctly rounded sums", IEEE TC 2008); arguments outside the range where the split is
  safe go through ``fractions.Fraction``.  ``a * b + c`` is never used as a stand-in.
* ``ldexp`` rounds to nearest-even into the subnormal range in one step, as v_ldexp_f64 does.
* The high-precision reference everywhere is ``np.longdouble`` with a 64-bit mantissa (x86-64); the import fails loudly
  on a platform without it.

What the model does NOT reproduce bit for bit is the hardware reciprocal estimate (v_rcp_f64) under ``recip_fast``: the
model starts the two Newton steps from the correctly rounded 1/s.  After two steps the result no longer depends on the
seed except within ~2^-100 of a rounding boundary (see recip_fast below)."""
import math
import os
import re
from fractions import Fraction

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 2e-19, "np.longdouble has no 64-bit mantissa here: the reference would be fp64 against fp64"

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pymbar_amd", "csrc")

_HEX = r"[-+]?0x[0-9a-fA-F]+(?:\.[0-9a-fA-F]*)?p[-+]?\d+"
_NUM = r"(?:" + _HEX + r"|[-+]?\d+(?:\.\d*)?(?:[eE][-+]?\d+)?)"


def _num(tok):
    tok = tok.strip()
    return float.fromhex(tok) if "0x" in tok.lower() else float(tok)


def _read(name, csrc):
    with open(os.path.join(csrc, name)) as fh:
        return fh.read()


def _array(text, name, n=None):
    m = re.search(r"\b" + name + r"\[(\d+)\]\s*=\s*\{(.*?)\}\s*;", text, re.S)
    if not m:
        raise ValueError(f"{name}[] not found")
    vals = [_num(t) for t in re.findall(_NUM, m.group(2))]
    if len(vals) != int(m.group(1)) or (n is not None and len(vals) != n):
        raise ValueError(f"{name}: {len(vals)} literals for [{m.group(1)}]")
    return np.array(vals, dtype=np.float64)


def _scalar(text, name):
    m = re.search(r"\b" + name + r"\s*=\s*(" + _NUM + r")", text)
    if not m:
        raise ValueError(f"{name} not found")
    return _num(m.group(1))


class Constants:
    """Every constant of the device exp / log, read from ``csrc`` (default: this tree's pymbar_amd/csrc)."""

    def __init__(self, csrc=CSRC):
        et, lt, dh = _read("exp2_table.inc", csrc), _read("log_table.inc", csrc), _read("mbar_device.h", csrc)
        self.EXP2_BITS = int(_scalar(et, "EXP2_BITS"))
        self.EXP2_DEG = int(_scalar(et, "EXP2_DEG"))
        self.S = 1 << self.EXP2_BITS
        self.EXP2_POLY = _array(et, "EXP2_POLY", self.EXP2_DEG + 1)
        self.EXP2_TABLE = _array(et, "EXP2_TABLE", self.S)
        self.LOG_TABLE = _array(lt, "LOG_TABLE", 256)
        self.EXP2N_POLY = _array(dh, "EXP2N_POLY", 4)
        self.LOG2E = _scalar(dh, "LOG2E")
        self.LN2 = _scalar(dh, "LN2")
        m = re.search(r"EXP2_CLAMP\s*=\s*(" + _NUM + r")\s*\*\s*EXP2_S", dh)
        if not m:
            raise ValueError("EXP2_CLAMP = <number> * EXP2_S not found")
        self.EXP2_CLAMP = _num(m.group(1)) * self.S          # (exact: a power of two times a small integer)
        self.LOG2E_S = self.S * self.LOG2E                    # constexpr double products by 2^11: exact
        self.LN2_OVER_S = self.LN2 / self.S
        # the Taylor coefficients of log1p as log_pos writes them (fp64 literals / constant-folded quotients)
        self.LOG1P = np.array([1.0, -0.5, 1.0 / 3.0, -0.25, 0.2, -1.0 / 6.0])


_default = None


def constants():
    global _default
    if _default is None:
        _default = Constants()
    return _default


# ---------------------------------------------------------------------------------------------------------------------
# exact fused multiply-add
# ---------------------------------------------------------------------------------------------------------------------
HAVE_MATH_FMA = hasattr(math, "fma")


def fma_fraction(a, b, c):
    """Scalar reference: the exact a b + c rounded once (float(Fraction) rounds to nearest-even)."""
    a, b, c = float(a), float(b), float(c)
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    v = Fraction(a) * Fraction(b) + Fraction(c)
    if v == 0:  # sign of an exact zero: as IEEE (x + y with both zero keeps a common sign, else +0 in round-to-nearest)
        p = a * b
        return p + c if (p == 0 and c == 0) else 0.0
    try:
        return float(v)
    except OverflowError:
        return math.copysign(math.inf, v)


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _split(a):
    t = 134217729.0 * a  # 2^27 + 1
    hi = t - (t - a)
    return hi, a - hi


def _two_prod(a, b):
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _round_to_odd_sum(a, b):
    """a + b rounded to odd: the exact sum if representable, else the neighbour whose last mantissa bit is 1."""
    s, e = _two_sum(a, b)
    bits = np.ascontiguousarray(s).view(np.int64)
    fix = (e != 0) & ((bits & 1) == 0)
    # the other neighbour lies on the side of the error term: one step away from zero when e has the sign of s, else towards it
    # (sign-magnitude bits: +1 on the integer view grows the magnitude for either sign)
    step = np.where((e > 0) == (s > 0), 1, -1)
    return (bits + np.where(fix, step, 0)).view(np.float64)


def fma(a, b, c):
    """Elementwise fp64 fma(a, b, c) with ONE rounding (arrays broadcast)."""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    shape = a.shape
    a, b, c = a.ravel().copy(), b.ravel().copy(), c.ravel().copy()
    out = np.empty_like(a)
    if HAVE_MATH_FMA:
        out[:] = [math.fma(x, y, z) for x, y, z in zip(a.tolist(), b.tolist(), c.tolist())]
        return out.reshape(shape)
    with np.errstate(all="ignore"):
        aa, ab, ac = np.abs(a), np.abs(b), np.abs(c)
        p_abs = aa * ab
        # range in which Veltkamp's split neither overflows nor loses low bits to underflow, and the sums stay normal
        lo, hi = 2.0 ** -400, 2.0 ** 400
        safe = (((aa > lo) & (aa < hi)) | (aa == 0)) & (((ab > lo) & (ab < hi)) | (ab == 0)) & (((ac > 2.0 ** -800) & (ac < 2.0 ** 800)) | (ac == 0))
        safe &= (p_abs == 0) | (p_abs > 2.0 ** -800)
        zero_p = (a == 0) | (b == 0)
        ph, pl = _two_prod(a, b)
        th, tl = _two_sum(c, ph)
        v = _round_to_odd_sum(tl, pl)
        z = th + v
        # exact-zero results keep IEEE's sign rules through the plain expression
        z = np.where(zero_p, a * b + c, z)
        # the final sum must not be subnormal for the double rounding argument (2 extra bits) to hold
        safe &= (np.abs(z) > 2.0 ** -900) | (z == 0)
        safe &= ~((z == 0) & ~zero_p & ((th != 0) | (v != 0)))
    out[safe] = z[safe]
    for i in np.nonzero(~safe)[0]:
        out[i] = fma_fraction(a[i], b[i], c[i])
    return out.reshape(shape)


def ldexp(x, q):
    """x 2^q rounded once to nearest-even, gradual underflow included (v_ldexp_f64; q as wide as int32)."""
    x = np.asarray(x, np.float64)
    q = np.clip(np.asarray(q, np.int64), -5000, 5000).astype(np.int32)  # (beyond +-2200 every finite x is 0 or inf already)
    with np.errstate(all="ignore"):
        return np.ldexp(x, q)


def ldexp_fraction(x, q):
    """Scalar reference of ldexp: exact product rounded once."""
    if x == 0 or not math.isfinite(x):
        return x
    v = Fraction(x) * (Fraction(2) ** int(q))
    try:
        r = float(v)
    except OverflowError:
        return math.copysign(math.inf, x)
    return math.copysign(r, x)


def cvt_i32(x):
    """v_cvt_i32_f64: truncation towards zero, saturating (NaN gives 0)."""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        t = np.where(np.isnan(x), 0.0, np.clip(np.trunc(x), -2147483648.0, 2147483647.0))
    return t.astype(np.int64)


def fract(x):
    """v_fract_f64: x - floor(x), never 1 (clamped to the largest double below 1)."""
    x = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        return np.minimum(x - np.floor(x), np.nextafter(1.0, 0.0))


def table_index(si, C=None):
    """exp2_table_at: the byte offset (si << 3) & (bytes - 8), as an entry index."""
    C = C or constants()
    return (((np.asarray(si, np.int64) << 3) & (C.S * 8 - 8)) >> 3).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------
# the device functions
# ---------------------------------------------------------------------------------------------------------------------
def exp2_poly(z, C=None):
    C = C or constants()
    p = np.full(np.shape(z), C.EXP2_POLY[C.EXP2_DEG])
    for k in range(C.EXP2_DEG - 1, -1, -1):
        p = fma(p, z, C.EXP2_POLY[k])
    return p


def exp2s(ts, clamp=True, C=None, parts=False):
    """exp2s_fast / exp2s_batch<N, CLAMP> / exp2s_batch2: 2^(ts / S)."""
    C = C or constants()
    ts = np.asarray(ts, np.float64)
    t = np.fmax(ts, C.EXP2_CLAMP) if clamp else ts        # v_max_f64 (a NaN argument gives the clamp)
    s = np.rint(t)                                        # v_rndne_f64
    with np.errstate(invalid="ignore"):
        z = t - s                                         # exact
    si = cvt_i32(s)                                       # v_cvt_i32_f64 (saturates)
    q = si >> C.EXP2_BITS                                 # v_ashrrev_i32
    j = table_index(si, C)                                # v_lshlrev_b32 + v_and_b32 + ds_read_b64
    T = C.EXP2_TABLE[j]
    p = exp2_poly(z, C)                                   # three v_fma_f64
    r = ldexp(T * p, q)                                   # v_mul_f64, v_ldexp_f64
    return (r, dict(z=z, si=si, q=q, j=j)) if parts else r


def exp2s_neg(w, clamp=False, C=None, parts=False):
    """exp2s_neg_batch<N, CLAMP> / exp2s_neg_batch2: 2^(-w / S) for w >= 0."""
    C = C or constants()
    w = np.asarray(w, np.float64)
    t = np.fmin(w, 2.0e9) if clamp else w                 # v_min_f64 (CLAMP only)
    ni = cvt_i32(-t)                                      # v_cvt_i32_f64 with a negated source
    z = fract(t)                                          # v_fract_f64
    q = ni >> C.EXP2_BITS
    j = table_index(ni, C)
    T = C.EXP2_TABLE[j]
    p = np.full(w.shape, C.EXP2N_POLY[3])
    p = fma(p, z, C.EXP2N_POLY[2])
    p = fma(p, z, C.EXP2N_POLY[1])
    p = fma(p, z, C.EXP2N_POLY[0])
    r = ldexp(T * p, q)
    return (r, dict(z=z, si=ni, q=q, j=j)) if parts else r


def log_bucket(m):
    """The pair index log_pos reads for a mantissa m in [1/2, 1): (hi >> 9) & 0x7f0 is its byte offset."""
    hi = (np.asarray(m, np.float64).view(np.int64) >> 32).astype(np.int64)
    return ((hi >> 9) & 0x7F0) >> 4


def log_pos(s, C=None, parts=False, contract=True):
    """log_pos: log s for positive finite s.  ``contract``: the closing ``fma(ed, LN2, tc.y) + q * r`` as ONE fma, which is what
    hipcc's default -ffp-contract=fast makes of it (False: separate multiply and add)."""
    C = C or constants()
    s = np.asarray(s, np.float64)
    m, e = np.frexp(s)                                    # v_frexp_mant_f64, v_frexp_exp_i32_f64
    ed = e.astype(np.float64)                             # v_cvt_f64_i32
    j = log_bucket(m)
    rc, lc = C.LOG_TABLE[2 * j], C.LOG_TABLE[2 * j + 1]   # ds_read_b128
    r = fma(m, rc, -1.0)
    L = C.LOG1P
    q = np.full(s.shape, L[5])
    for k in (4, 3, 2, 1, 0):
        q = fma(q, r, L[k])
    base = fma(ed, C.LN2, lc)
    out = fma(q, r, base) if contract else base + q * r
    return (out, dict(m=m, e=e, j=j, r=r)) if parts else out


def recip_fast(s, seed_steps=0):
    """recip_fast: two Newton steps.  The model starts from the correctly rounded 1/s in place of v_rcp_f64's estimate.  With
    e = 1 - s r the second step returns RN(r (1 + e)) = RN((1/s)(1 - e^2)), |e| <= 2^-52 after the first step from either seed:
    the two agree unless 1/s lies within ~2^-104 relative of a rounding boundary.  That does happen: s = 1 - 2^-53 (a column whose
    largest term is 1 - 2^-53 and whose other terms vanish) has 1/s = 1 + 2^-53 + 2^-106, a hair above a tie; from r = 1 + 2^-52
    the steps stay there, from r = 1 they stay at 1 (RN(1 + 2^-53) ties to even).  ``seed_steps`` = +-1 starts the LAST step one
    fp64 step above / below RN(1/s): recip_candidates() lists what a seed-dependent argument can return."""
    s = np.asarray(s, np.float64)
    with np.errstate(divide="ignore"):
        r = 1.0 / s
    if seed_steps:
        r = np.nextafter(r, np.inf if seed_steps > 0 else -np.inf)
        return fma(fma(-s, r, 1.0), r, r)
    for _ in range(2):
        r = fma(fma(-s, r, 1.0), r, r)
    return r


def recip_candidates(s):
    """(r, r_up, r_down): recip_fast from the correctly rounded seed, and its last step taken from one fp64 step above / below
    RN(1/s) -- where the first step of a hardware seed can land.  Equal except next to a rounding boundary of 1/s."""
    return recip_fast(s), recip_fast(s, 1), recip_fast(s, -1)


# ---------------------------------------------------------------------------------------------------------------------
# long-double references and error measures
# ---------------------------------------------------------------------------------------------------------------------
LN2_LD = np.log(LD(2))


def ld_exp2s(ts, C=None):
    """2^(ts / S) in long double (ts an fp64 array: ts / S is exact in long double)."""
    C = C or constants()
    return np.exp2(np.asarray(ts, LD) / LD(C.S))


def ulp_of(x):
    """The fp64 ulp at |x| (x a long-double or fp64 array of normal magnitude); the subnormal spacing below 2^-1022."""
    x = np.abs(np.asarray(x, LD))
    _, e = np.frexp(np.maximum(x, LD(2.0) ** -1022))
    return np.ldexp(LD(1), np.maximum(e - 53, -1074))


def err_ulps(got, want):
    """(got - want) in fp64 ulps of ``want``."""
    return (np.asarray(got, LD) - np.asarray(want, LD)) / ulp_of(want)


# ---------------------------------------------------------------------------------------------------------------------
# the accuracy claims that mbar_device.h states, shared by the CPU and the GPU test module (u = 2^-53)
# ---------------------------------------------------------------------------------------------------------------------
U_LD = LD(2.0) ** -53
E_EXP_CLAIM = 3.1                                # exp2s_* / exp2s_neg_*: relative error of a normal result, in u
E_LOG_A, E_LOG_E, E_LOG_ULP = 1.6, 0.5, 1.0      # log_pos: absolute error (E_LOG_A + E_LOG_E |e|) u + E_LOG_ULP ulp(log s), s = 2^e m


def log_bound_u(s, want):
    """The log_pos claim above, in u, for arguments s with long-double logarithms ``want``."""
    _, e = np.frexp(np.asarray(s, np.float64))
    return E_LOG_A + E_LOG_E * np.abs(e) + E_LOG_ULP * (ulp_of(np.maximum(np.abs(want), LD(2.0) ** -60)) / U_LD).astype(np.float64)


# Arguments d (kT below a column's maximum, at offset 0 and f = 0) at which the RESULT of the device exponential changes when the
# named coefficient moves by one ulp -- found by search with the model (2^-10 of all arguments for the linear coefficient, 2^-22 z^2 for
# the quadratic one; the cubic one's last bit is worth 2^-90 and no fp64 result shows it: the generator test above pins it).  The GPU
# module runs them as probe columns, so that the bits the device returns there depend on the last bit of these coefficients.
COEFFICIENT_PROBES = {
    ("EXP2N_POLY", 1): ["0x1.a0dc30cf6e073p-13", "0x1.fb805dfd2ae1cp-13", "0x1.b220a78f2d8f6p-13", "0x1.d9f318cd73a0bp-13",
                        "0x1.4cb53decfaf5cp-12", "0x1.d42b339f9517fp-13"],
    ("EXP2N_POLY", 2): ["0x1.bd8547a039db6p-13", "0x1.140407ea25808p-12", "0x1.096b91ddfcb5dp-12", "0x1.2c266216d8c4ap-12"],
    ("EXP2_POLY", 1): ["0x1.6fbee8d3ef63dp-14", "0x1.46669874b08ddp-13", "0x1.5e506ce0e8904p-13", "0x1.2bc9c298eccf6p-13",
                       "0x1.5c5d73478ee61p-13", "0x1.030387b4c6fb4p-13"],
    ("EXP2_POLY", 2): ["0x1.2a51b84f90600p-13", "0x1.d59f213b8e41dp-14", "0x1.51692f487785cp-14", "0x1.44438797457e0p-13"],
}


def coefficient_probe_d():
    return np.array([float.fromhex(h) for hs in COEFFICIENT_PROBES.values() for h in hs])
