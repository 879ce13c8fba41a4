"""Constants of the build sweep's exponential (exp2s_neg_batch, mbar_device.h): the degree-3 near-minimax polynomial
(Chebyshev interpolant, 80-bit long double, rounded to fp64) of 2**(-z/S) on z in [0, 1], S = 2**BITS, monomial coefficients
in z with the constant term forced to 1 (exact at z = 0).  The same construction as tools/gen_exp2_table.py uses for
2**(z/S) on [-1/2, 1/2], on the other interval.  Prints the C initialiser of EXP2N_POLY, its maximal relative error (exact
arithmetic, rounded coefficients) and -- with --compare -- the error of the coefficients committed in mbar_device.h.
Run: python tools/gen_exp2n_poly.py [BITS] [--compare]"""
import os
import re
import sys

import numpy as np

args = [a for a in sys.argv[1:] if not a.startswith("--")]
BITS = int(args[0]) if args else 11
DEG = 3
S = 1 << BITS
LD = np.longdouble
n = DEG + 1
pi = LD("3.14159265358979323846264338327950288")
j = np.arange(n, dtype=LD)
nodes = np.cos((j + LD(0.5)) * pi / n)      # Chebyshev nodes y on [-1, 1];  z = (y + 1) / 2 on [0, 1]
f = np.exp2(-((nodes + 1) / 2) / LD(S))
c = np.array([(LD(2) / n) * np.sum(f * np.cos(k * (j + LD(0.5)) * pi / n)) for k in range(n)], dtype=LD)
c[0] /= 2
T = [np.zeros(n, dtype=LD) for _ in range(n)]
T[0][0] = 1
T[1][1] = 1
for k in range(1, n - 1):
    T[k + 1][1:] = 2 * T[k][:-1]
    T[k + 1] -= T[k - 1]
mono_y = sum(c[k] * T[k] for k in range(n))
# y = 2 z - 1: expand sum_k a_k (2 z - 1)^k into powers of z
mono_z = np.zeros(n, dtype=LD)
for k in range(n):
    term = np.zeros(n, dtype=LD)
    term[0] = 1
    for _ in range(k):
        nxt = np.zeros(n, dtype=LD)
        nxt[1:] += 2 * term[:-1]
        nxt -= term
        term = nxt
    mono_z += mono_y[k] * term
coef = np.array([float(v) for v in mono_z])
coef[0] = 1.0


def max_rel_err(cf):
    z = np.linspace(LD(0), LD(1), 400001, dtype=LD)
    p = np.zeros_like(z)
    for v in cf[::-1]:
        p = p * z + LD(v)
    return float(np.max(np.abs(p / np.exp2(-z / S) - 1)))


def c_literal(v):
    return ("-" if v < 0 else "") + float(abs(v)).hex()


print("constexpr double EXP2N_POLY[%d] = {%s};" % (n, ", ".join("1.0" if v == 1.0 else c_literal(v) for v in coef)))
print("max relative error of the rounded polynomial on [0, 1]: %.3e" % max_rel_err(coef))
if "--compare" in sys.argv:
    hdr = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "pymbar_amd", "csrc", "mbar_device.h")
    with open(hdr) as fh:
        m = re.search(r"EXP2N_POLY\[4\]\s*=\s*\{(.*?)\}", fh.read(), re.S)
    have = np.array([float.fromhex(t) if "0x" in t else float(t) for t in (s.strip() for s in m.group(1).split(","))])
    print("committed:  {%s}" % ", ".join(c_literal(v) for v in have))
    print("max relative error of the committed coefficients:      %.3e" % max_rel_err(have))
