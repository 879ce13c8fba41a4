"""Exact numpy oracle of the weighted kernel-density sum (test infrastructure for tests/test_kde_host.py and tests/test_gpu_kde.py):

    L[m, c] = log sum_n V[n, c] k_h(|q_m - x_n|) - log sum_n V[n, c] + log-normaliser(kernel, d, h)

evaluated over every pair in float64, in log space.  The normalisers are computed here on their own (closed forms for the two
kernels with unbounded support, Gauss-Legendre quadrature of the radial profile for the compact ones), not taken from the
library.  :class:`OracleKDE` has the interface of ``pymbar_amd.kde.DeviceKDE`` and stands in for it in CPU tests."""
import math

import numpy as np

KERNELS = ("gaussian", "tophat", "epanechnikov", "exponential", "linear", "cosine")


def _unit_ball_log_volume(d):
    return 0.5 * d * math.log(math.pi) - math.lgamma(0.5 * d + 1.0)


def _profile(kernel, r):
    """k(r) on the unit scale for r in [0, 1) (compact kernels)."""
    if kernel == "tophat":
        return np.ones_like(r)
    if kernel == "epanechnikov":
        return 1.0 - r * r
    if kernel == "linear":
        return 1.0 - r
    return np.cos(0.5 * np.pi * r)


def log_normaliser(kernel, d, h):
    if kernel == "gaussian":
        return -0.5 * d * math.log(2.0 * math.pi) - d * math.log(h)
    if kernel == "exponential":  # integral of exp(-r) over R^d = S_(d-1) Gamma(d)
        return -(math.log(d) + _unit_ball_log_volume(d) + math.lgamma(d)) - d * math.log(h)
    t, wq = np.polynomial.legendre.leggauss(64)
    r = 0.5 * (t + 1.0)
    radial = 0.5 * float(np.sum(wq * r ** (d - 1) * _profile(kernel, r)))
    return -(math.log(d) + _unit_ball_log_volume(d) + math.log(radial)) - d * math.log(h)


def log_kernel(kernel, X, Q, h):
    """(M, N) log k_h(|q_m - x_n|) without the normaliser; sklearn's formulas and support test dist < h."""
    r2 = np.zeros((Q.shape[0], X.shape[0]))
    for j in range(X.shape[1]):
        dx = Q[:, None, j] - X[None, :, j]
        r2 = r2 + dx * dx
    if kernel == "gaussian":
        return -0.5 * r2 / (h * h)
    dist = np.sqrt(r2)
    if kernel == "exponential":
        return -dist / h
    inside = dist < h
    with np.errstate(divide="ignore", invalid="ignore"):
        if kernel == "tophat":
            k = np.ones_like(dist)
        elif kernel == "epanechnikov":
            k = 1.0 - (dist * dist) / (h * h)
        elif kernel == "linear":
            k = 1.0 - dist / h
        else:
            k = np.cos(0.5 * np.pi * dist / h)
        return np.where(inside & (k > 0), np.log(np.where(inside, k, 1.0)), -np.inf)


def log_density(X, V, Q, kernel, h, block=None):
    """(M, C) exact log densities.  A column of zero total weight gives NaN."""
    X = np.asarray(X, dtype=np.float64)
    Q = np.asarray(Q, dtype=np.float64)
    V = np.asarray(V, dtype=np.float64)
    if V.ndim == 1:
        V = V[:, None]
    N, C = V.shape
    M = Q.shape[0]
    if block is None:  # (about 2^23 pairs per block: bounded temporaries)
        block = max(256, (1 << 23) // max(1, M))
    mrun = np.full(M, -np.inf)
    srun = np.zeros((M, C))
    any_w = V.max(axis=1) > 0
    for b0 in range(0, N, block):
        lk = log_kernel(kernel, X[b0:b0 + block], Q, h)
        lk_w = np.where(any_w[None, b0:b0 + block], lk, -np.inf)
        mb = lk_w.max(axis=1)
        with np.errstate(invalid="ignore"):
            E = np.where(np.isfinite(mb)[:, None], np.exp(lk - np.where(np.isfinite(mb), mb, 0.0)[:, None]), 0.0)
        sb = E @ V[b0:b0 + block]
        mnew = np.maximum(mrun, mb)
        safe = np.where(np.isfinite(mnew), mnew, 0.0)
        with np.errstate(invalid="ignore"):
            fa = np.where(np.isfinite(mrun), np.exp(mrun - safe), 0.0)
            fb = np.where(np.isfinite(mb), np.exp(mb - safe), 0.0)
        srun = srun * fa[:, None] + sb * fb[:, None]
        mrun = mnew
    W = V.sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        L = mrun[:, None] + np.log(srun) - np.log(W)[None, :] + log_normaliser(kernel, X.shape[1], h)
    L[:, W == 0] = np.nan
    # pairs whose terms all underflowed against the shared per-query maximum: their own maximum over the weighted samples
    redo = np.argwhere((srun < 1e-250) & (W > 0)[None, :] & (np.isfinite(mrun)[:, None] | (kernel in ("gaussian", "exponential"))))
    for m, c in redo:
        w = V[:, c]
        pos = w > 0
        t = log_kernel(kernel, X[pos], Q[m:m + 1], h)[0] + np.log(w[pos])
        tm = t.max()
        L[m, c] = (tm + np.log(np.sum(np.exp(t - tm))) if np.isfinite(tm) else -np.inf) - np.log(W[c]) + \
            log_normaliser(kernel, X.shape[1], h)
    return L


# ---- the same sum in long double --------------------------------------------------------------------------------------------
LD = np.longdouble
LD_PI = 4 * np.arctan(LD(1))


def _ld_log_unit_ball_volume(d):
    """log(pi^(d/2) / Gamma(d/2 + 1)) with Gamma(d/2 + 1) as a finite product (d <= 8 here, any d works)."""
    g = LD(1) if d % 2 == 0 else np.sqrt(LD_PI)
    a = LD(d) / 2
    while a > 0:
        g = g * a
        a = a - 1
    return LD(d) / 2 * np.log(LD_PI) - np.log(g)


def log_normaliser_ld(kernel, d, h):
    """:func:`log_normaliser` in long double, from the closed forms of the radial integrals int_0^1 r^(d-1) k(r) dr (the float64
    one integrates by quadrature: tests/test_kde_host.py holds the two against each other)."""
    h = LD(h)
    dlogh = d * np.log(h)
    if kernel == "gaussian":
        return -LD(d) / 2 * np.log(2 * LD_PI) - dlogh
    logS = np.log(LD(d)) + _ld_log_unit_ball_volume(d)  # surface of the unit sphere
    if kernel == "exponential":
        fact = LD(1)
        for i in range(2, d):
            fact = fact * i
        return -(logS + np.log(fact)) - dlogh
    if kernel == "tophat":
        radial = LD(1) / d
    elif kernel == "epanechnikov":
        radial = LD(1) / d - LD(1) / (d + 2)
    elif kernel == "linear":
        radial = LD(1) / d - LD(1) / (d + 1)
    else:  # I_n = int r^n cos(pi r / 2), J_n = int r^n sin(pi r / 2): I_n = 2/pi - (2n/pi) J_(n-1), J_n = (2n/pi) I_(n-1)
        I = J = 2 / LD_PI
        for n in range(1, d):
            I, J = 2 / LD_PI - (2 * n / LD_PI) * J, (2 * n / LD_PI) * I
        radial = I
    return -(logS + np.log(radial)) - dlogh


def log_kernel_ld(kernel, X, Q, h):
    """(M, N) log k_h in long double.  gaussian / exponential: from the float64 coordinates, every step in long double.  Compact
    kernels: the library specifies the support test in float64 -- ``r2 = r2 + dx*dx`` in coordinate order without fma, the float64
    square root, ``dist < h`` -- and sklearn's formulas are functions of that float64 ``dist``; both are reproduced here, and the
    kernel value of a pair inside the support is evaluated on that ``dist`` in long double."""
    X = np.asarray(X, dtype=np.float64)
    Q = np.asarray(Q, dtype=np.float64)
    hl = LD(h)
    if kernel in ("gaussian", "exponential"):
        r2 = np.zeros((Q.shape[0], X.shape[0]), dtype=LD)
        for j in range(X.shape[1]):
            dx = Q[:, None, j].astype(LD) - X[None, :, j].astype(LD)
            r2 = r2 + dx * dx
        return -r2 / (2 * hl * hl) if kernel == "gaussian" else -np.sqrt(r2) / hl
    r2 = np.zeros((Q.shape[0], X.shape[0]))
    with np.errstate(over="ignore"):
        for j in range(X.shape[1]):
            dx = Q[:, None, j] - X[None, :, j]
            r2 = r2 + dx * dx
        dist = np.sqrt(r2)
    inside = dist < float(h)
    u = np.where(inside, dist, 0.0).astype(LD) / hl
    if kernel == "tophat":
        k = np.ones_like(u)
    elif kernel == "epanechnikov":
        k = 1 - u * u
    elif kernel == "linear":
        k = 1 - u
    else:
        k = np.cos(LD_PI / 2 * u)
    with np.errstate(divide="ignore"):
        return np.where(inside & (k > 0), np.log(np.where(k > 0, k, LD(1))), -LD(np.inf))


def log_density_ld(X, V, Q, kernel, h):
    """``(L, cond)``: the (M, C) log densities of :func:`log_density` with every step in long double (per pair log k, per (query,
    column) the maximum over the samples of positive weight and the log-sum-exp, the column totals, the normaliser), rounded to
    float64 at the end -- a value below the float64 range becomes -inf; a column of zero total weight gives NaN.  ``cond[m, c]``
    is the number of samples of positive weight with a positive kernel value, the terms an entry is made of."""
    X = np.asarray(X, dtype=np.float64)
    Q = np.asarray(Q, dtype=np.float64)
    V = np.asarray(V, dtype=np.float64)
    if V.ndim == 1:
        V = V[:, None]
    M, C = Q.shape[0], V.shape[1]
    lk = log_kernel_ld(kernel, X, Q, h)
    lognorm = log_normaliser_ld(kernel, X.shape[1], h)
    L = np.full((M, C), np.nan, dtype=LD)
    cond = np.zeros((M, C), dtype=np.int64)
    for c in range(C):
        pos = V[:, c] > 0
        if not pos.any():
            continue
        t = lk[:, pos] + np.log(V[pos, c].astype(LD))[None, :]
        tm = t.max(axis=1)
        fin = np.isfinite(tm)
        cond[:, c] = np.sum(np.isfinite(t), axis=1)
        s = np.sum(np.exp(t[fin] - tm[fin, None]), axis=1)
        Lc = np.full(M, -LD(np.inf))
        Lc[fin] = tm[fin] + np.log(s)
        L[:, c] = Lc - np.log(np.sum(V[pos, c].astype(LD))) + lognorm
    with np.errstate(over="ignore"):
        return L.astype(np.float64), cond


def chunk_ranges(N, max_chunks, tile=64):
    """The sample ranges [n0, n1) of the chunks of an evaluation under the handle option ``"max_chunks"`` >= 1 (the host's cut:
    whole tiles of 64 samples, ceil(tiles / chunks) tiles per chunk; the padding of the last tile repeats the last sample)."""
    ntiles = (N + tile - 1) // tile
    want = max(1, min(max_chunks, ntiles))
    per = (ntiles + want - 1) // want * tile
    return [(n0, min(n0 + per, N)) for n0 in range(0, ntiles * tile, per)]


class OracleKDE:
    """Stand-in for ``pymbar_amd.kde.DeviceKDE`` on the CPU."""

    def __init__(self, X, kernel, bandwidth, device=None):
        self.X = np.array(X, dtype=np.float64)
        self.n_samples, self.dim = self.X.shape
        self.kernel, self.h = kernel, float(bandwidth)
        self.V = np.ones((self.n_samples, 1))
        self.n_columns = 1
        self.calls = 0

    def set_weights(self, V):
        V = np.asarray(V, dtype=np.float64)
        self.V = np.array(V[:, None] if V.ndim == 1 else V)
        self.n_columns = self.V.shape[1]

    def log_density(self, Q):
        self.calls += 1
        return log_density(self.X, self.V, np.asarray(Q, dtype=np.float64), self.kernel, self.h)

    def close(self):
        pass
