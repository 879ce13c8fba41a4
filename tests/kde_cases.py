"""Case builders of the kernel-density instantiation tests, shared by tests/test_kde_host.py (which checks on the CPU that every
case suits the oracles) and tests/test_gpu_kde.py (which runs them on the device).  All shapes are small: the matrix cases have
N = 3 * 64 + 5 samples (a ragged last tile, padding samples) and M = 256 + 3 queries (two query blocks, the second ragged).

``k_kde<KER, D, CB>`` has 72 bodies.  The dimension picks D: d = 1, 2, 3 -> D = d for gaussian / exponential, every other d and
every compact kernel -> the generic body (D = 0).  The column count picks CB, the smallest of 1, 4, 8, 16, 24, 32 that holds it:
C = 1 -> 1, 3 -> 4, 7 -> 8, 13 -> 16, 19 -> 24, 27 -> 32 (padding columns live in all but the first)."""
import functools

import numpy as np

from tests import kde_oracle

KERNELS = kde_oracle.KERNELS
UNBOUNDED = ("gaussian", "exponential")
COMPACT = ("tophat", "epanechnikov", "linear", "cosine")
N_MATRIX, M_MATRIX = 3 * 64 + 5, 256 + 3
C_TO_CB = {1: 1, 3: 4, 7: 8, 13: 16, 19: 24, 27: 32}
D_UNBOUNDED, D_COMPACT = (1, 2, 3, 4, 8), (1, 4, 8)
# bandwidths that leave a compact kernel some samples inside its support in every dimension (standard normal samples)
H_OF_D = {1: 0.35, 2: 0.5, 3: 0.7, 4: 1.0, 8: 2.5}


def matrix_cases():
    """(kernel, d, C) of all 72 bodies."""
    out = []
    for kernel in KERNELS:
        for d in (D_UNBOUNDED if kernel in UNBOUNDED else D_COMPACT):
            out += [(kernel, d, C) for C in C_TO_CB]
    return out


@functools.lru_cache(maxsize=None)
def matrix_case(kernel, d, C):
    """X, V, Q, h: about 20 % zero-weight rows, a zero-weight column when C >= 3, half of the queries among the samples, and the
    last two queries 40 h and 300 h outside the data."""
    rng = np.random.RandomState(10007 * KERNELS.index(kernel) + 101 * d + C)
    h = H_OF_D[d]
    N, M = N_MATRIX, M_MATRIX
    X = rng.normal(size=(N, d))
    V = rng.uniform(0.0, 2.0, size=(N, C)) * (rng.uniform(size=(N, 1)) > 0.2)
    if C >= 3:
        V[:, 1] = 0.0
    V[0] = rng.uniform(0.5, 1.0, size=C) * ((np.arange(C) != 1) | (C < 3))
    Q = rng.normal(scale=1.3, size=(M, d))
    near = rng.randint(0, N, size=M // 2)
    Q[: M // 2] = X[near] + 0.3 * h / np.sqrt(d) * rng.normal(size=(M // 2, d))
    Q[-1] = X.max(axis=0) + 40 * h
    Q[-2] = X.min(axis=0) - 300 * h
    for a in (X, V, Q):
        a.setflags(write=False)
    return X, V, Q, h


@functools.lru_cache(maxsize=None)
def matrix_oracle(kernel, d, C):
    """(L, cond) of :func:`kde_oracle.log_density_ld` for a matrix case: computed once, shared, read-only."""
    X, V, Q, h = matrix_case(kernel, d, C)
    L, cond = kde_oracle.log_density_ld(X, V, Q, kernel, h)
    L.setflags(write=False)
    return L, cond


def scaled_error(got, want):
    """max |got - want| / max(1, |want|) over the finite entries of ``want`` (0 if there is none)."""
    fin = np.isfinite(want)
    if not fin.any():
        return 0.0
    return float(np.max(np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin]))))


# ---- k_kde_exact: pairs the combine kernel flags -------------------------------------------------------------------------------
EXACT_DIMS = (1, 3, 8)
TINY = 1e-290  # (below the flag threshold 2^-900 = 1.2e-271, above the subnormals after a kernel value >= 1e-15)


def exact_case(kernel, d):
    """Two clusters A (at the origin) and B (50 h away, 1000 h for the exponential kernel: the other cluster's terms lie more
    than 900 doublings below the near one's), queries near A, near B and near neither.  Columns: 0 all samples; 1 only
    A; 2 only B; 3 A with weight 1e-290 and B with weight 1 (next to a weight-1 sample the column scale stays 1, so the sum of a
    query near A is positive and below 2^-900).  Near A, column 2 has only zero-weight samples inside a compact support, and the
    queries near neither cluster have no sample inside at all."""
    rng = np.random.RandomState(77 + d + 10 * KERNELS.index(kernel))
    h = H_OF_D[d]
    off = (1000.0 if kernel == "exponential" else 50.0) * h / np.sqrt(d)
    A = 0.5 * rng.normal(size=(100, d))
    B = 0.5 * rng.normal(size=(100, d)) + off
    X = np.vstack([A, B])
    V = np.ones((200, 4))
    V[100:, 1] = 0.0
    V[:100, 2] = 0.0
    V[:100, 3] = TINY
    qa = A[:10] + 0.2 * h / np.sqrt(d) * rng.normal(size=(10, d))
    qb = B[:10] + 0.2 * h / np.sqrt(d) * rng.normal(size=(10, d))
    qn = np.full((2, d), -off) + rng.normal(size=(2, d))
    return X, V, np.vstack([qa, qb, qn]), h


# ---- k_kde_combine: chunks far apart in their shifts --------------------------------------------------------------------------
def combine_case(kernel, order):
    """3 x 64 samples in d = 1 evaluated with max_chunks = 3, one tile per chunk, queries around the origin.  The tiles sit at
    distances whose largest terms lie about 0 (near), 600 (mid) and 1500 (far) doublings below one; ``order`` lists which of them
    chunk 0, 1, 2 hold."""
    rng = np.random.RandomState(5 + len(order[0]))
    h = 1.0
    if kernel == "gaussian":  # log2 k = -r^2 log2(e) / 2
        dist = {"near": 0.0, "mid": np.sqrt(2 * 600 / np.log2(np.e)), "far": np.sqrt(2 * 1500 / np.log2(np.e))}
    else:  # log2 k = -r log2(e)
        dist = {"near": 0.0, "mid": 600 / np.log2(np.e), "far": 1500 / np.log2(np.e)}
    X = np.concatenate([dist[name] + rng.uniform(0.5, 1.5, size=64) for name in order])[:, None]
    V = rng.uniform(0.5, 1.5, size=(192, 3))
    V[::5, 2] = 0.0
    Q = rng.uniform(-0.2, 0.2, size=(70, 1))
    return X, V, Q, h


def chunk_maxima_doublings(X, Q, kernel, h, max_chunks):
    """(M, chunks) the largest log2 k of each query over each chunk's samples (the chunk's shift, up to the deferred 256)."""
    lk = kde_oracle.log_kernel_ld(kernel, X, Q, h) / np.log(kde_oracle.LD(2))
    return np.stack([lk[:, a:b].max(axis=1) for a, b in kde_oracle.chunk_ranges(len(X), max_chunks)], axis=1).astype(np.float64)


# ---- the support boundary in d >= 2 ---------------------------------------------------------------------------------------------
def boundary_cases():
    """name -> (X, Q, h): one sample at the origin, and queries at the vectors v with |v| == h exactly in float64 arithmetic
    ((3, 4), (1, 2, 2), (2, 3, 6), eight +-1), at v with one coordinate moved one ulp and 2^-48 in or out, each for the bandwidths h, the
    next float64 above (the sample sits one ulp inside) and the next below."""
    out = {}
    geo = {"3-4-5": ([3.0, 4.0], 5.0), "1-2-2-3": ([1.0, 2.0, 2.0], 3.0), "2-3-6-7": ([2.0, 3.0, 6.0], 7.0),
           "ones8": ([1.0, -1.0, 1.0, 1.0, -1.0, -1.0, 1.0, -1.0], float(np.sqrt(np.float64(8.0))))}
    for name, (v, h0) in geo.items():
        v = np.array(v)
        rows = [v, -v]
        for j in (0, len(v) - 1):
            for toward in (0.0, np.inf):  # (one ulp of a coordinate rounds back to dist == h; 2^-48 of it does not)
                w = v.copy()
                w[j] = np.nextafter(v[j], np.sign(v[j]) * toward)
                rows.append(w)
                w = v.copy()
                w[j] = v[j] * (1.0 + (2.0 ** -48 if toward else -2.0 ** -48))
                rows.append(w)
        rows.append(0.5 * v)
        Q = np.array(rows)
        X = np.zeros((1, len(v)))
        for tag, h in (("h", h0), ("h_up", np.nextafter(h0, np.inf)), ("h_down", np.nextafter(h0, 0.0))):
            out[f"{name}/{tag}"] = (X, Q, float(h))
    return out


# ---- distances beyond the float64 range of r coef -----------------------------------------------------------------------------
def overflow_cases():
    """name -> (kernel, X, V, Q, h, far): 130 samples around the origin, 64 near queries and the far queries (rows ``far`` of Q)
    for which r^2, or r times the exponent's coefficient, overflows.  The log density there is finite in long double; rounded to
    float64 it is -inf or, for the exponential kernel, a finite number of the order of -r / h."""
    out = {}
    for name, kernel, d, h, fq in (("gaussian-d1", "gaussian", 1, 0.35, [[1e160], [-1e160], [3e153]]),
                                   ("gaussian-d3", "gaussian", 3, 0.7, [[1e160, 0.0, 0.0], [1e155, -1e155, 1e155]]),
                                   ("exponential-d1", "exponential", 1, 0.01, [[1e306], [-1e306]]),
                                   ("exponential-d2", "exponential", 2, 0.5, [[1e160, 1e160], [0.0, -1e200]])):
        rng = np.random.RandomState(len(name))
        X = rng.normal(size=(130, d))
        V = rng.uniform(0.5, 1.5, size=(130, 3))
        V[::4, 1] = 0.0
        near = rng.normal(size=(64, d))
        Q = np.vstack([near[:40], np.array(fq), near[40:]])  # (the far queries share a wave with near ones)
        out[name] = (kernel, X, V, Q, h, np.arange(40, 40 + len(fq)))
    return out
