"""Long-double oracle of the weighted B-spline moments (test infrastructure for tests/test_spline_fes_host.py and
tests/test_gpu_spline_fes.py):

    M[g, c, i] = sum over the samples n of group g of V[n, c] B_{i,k,t}(x_n)

with scipy's interval rule (find_interval, extrapolate=True) and the Cox-de Boor recursion, both evaluated here on their own in
np.longdouble, and the sums accumulated in np.longdouble.  :func:`abs_moments` gives sum |V B| for the error bound.
:class:`OracleBSplineMoments` has the interface of ``pymbar_amd.bspline.DeviceBSplineMoments`` and stands in for it in CPU
tests."""
import numpy as np

LD = np.longdouble


def intervals(t, k, x):
    """scipy's find_interval: the largest l in [k, n - 1] with t[l] <= x (k when x lies below t[k + 1])."""
    t = np.asarray(t, dtype=np.float64)
    n = len(t) - k - 1
    ub = np.searchsorted(t, np.asarray(x, dtype=np.float64), side="right")
    return np.clip(ub - 1, k, n - 1)


def basis_values(t, k, x, dtype=LD):
    """(N, k + 1) values of B_{l-k .. l} at x (long double) and the intervals l.  ``dtype=np.float64``: the same recursion, every
    operation rounded to float64 and none fused -- the operation order of scipy's own evaluation."""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    l = intervals(t, k, x)
    tl = np.asarray(t, dtype=dtype)
    xl = x.astype(dtype)
    h = np.zeros((len(x), k + 1), dtype=dtype)
    h[:, 0] = 1
    for j in range(1, k + 1):
        hh = h[:, :j].copy()
        h[:, 0] = 0
        for m in range(1, j + 1):
            xb = tl[l + m]
            xa = tl[l + m - j]
            same = xb == xa
            d = np.where(same, dtype(1), xb - xa)
            w = np.where(same, dtype(0), hh[:, m - 1] / d)
            h[:, m - 1] += w * (xb - xl)
            h[:, m] = w * (xl - xa)
    return h, l


def _accumulate(x, V, t, k, groups, G, absolute):
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    V = np.asarray(V, dtype=np.float64)
    if V.ndim == 1:
        V = V[:, None]
    nbasis = len(t) - k - 1
    g = np.zeros(len(x), dtype=np.int64) if groups is None else np.asarray(groups, dtype=np.int64).reshape(-1)
    out = np.zeros((G, V.shape[1], nbasis), dtype=LD)
    h, l = basis_values(t, k, x)
    Vl = V.astype(LD)
    if absolute:
        h, Vl = np.abs(h), np.abs(Vl)
    for j in range(k + 1):
        col = l - k + j
        for c in range(V.shape[1]):
            np.add.at(out[:, c, :], (g, col), h[:, j] * Vl[:, c])
    return out


def moments(x, V, t, k, groups=None, G=1):
    """(G, C, nbasis) moments in long double."""
    return _accumulate(x, V, t, k, groups, G, False)


def abs_moments(x, V, t, k, groups=None, G=1):
    """(G, C, nbasis) sums of |V B| (the scale of the error bound)."""
    return _accumulate(x, V, t, k, groups, G, True)


class OracleBSplineMoments:
    """Stand-in for ``pymbar_amd.bspline.DeviceBSplineMoments`` on the CPU."""

    def __init__(self, x, groups=None, n_groups=None, device=None):
        from pymbar_amd.utils import DataError

        self.x = np.array(np.asarray(x, dtype=np.float64).reshape(-1))
        if not np.all(np.isfinite(self.x)):
            raise DataError("sample coordinates must be finite")
        self.n_samples = len(self.x)
        self.groups = None
        self.n_groups = 1
        self.V = np.ones((self.n_samples, 1))
        self.n_columns = 1
        self.calls = 0
        if groups is not None:
            self.set_groups(groups, n_groups)

    def set_groups(self, groups, n_groups=None):
        self.groups = np.asarray(groups, dtype=np.int64).reshape(-1)
        self.n_groups = int(self.groups.max()) + 1 if n_groups is None else int(n_groups)

    def set_weights(self, V):
        from pymbar_amd.utils import DataError

        V = np.asarray(V, dtype=np.float64)
        if not np.all(np.isfinite(V)):
            raise DataError("weights must be finite")
        self.V = np.array(V[:, None] if V.ndim == 1 else V)
        self.n_columns = self.V.shape[1]

    def moments(self, t, k):
        from pymbar_amd.bspline import check_spline_shape

        t, k, _ = check_spline_shape(t, k)
        self.calls += 1
        return moments(self.x, self.V, t, k, self.groups, self.n_groups).astype(np.float64)

    def kernel_ms(self):
        return 0.0

    def close(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# ---- the cases of the instantiation tests of k_bspline<K, CB> (tests/test_gpu_spline_fes.py) ------------------------------------
# k_bspline<K, CB> has 8 x 6 bodies: K = 0 .. 7 is the degree, CB the smallest of 1, 2, 4, 8, 16, 32 that holds the C columns.
C_TO_CB = {1: 1, 2: 2, 3: 4, 7: 8, 13: 16, 29: 32}
SLAB_ENTRIES = 768  # (cell, column) entries of one output tile: tile_cells = 768 / CB


def knots(k, nbasis, lo=-1.0, hi=1.0, rng=None):
    inner = np.linspace(lo, hi, nbasis - k + 1)
    if rng is not None:  # non-uniform, with a repeated interior knot
        inner = np.sort(np.r_[lo, hi, rng.uniform(lo, hi, nbasis - k - 1)])
        if len(inner) > 4:
            inner[2] = inner[3]
    return np.r_[[lo] * k, inner, [hi] * k]


def tile_seams(k, nbasis, G, C):
    """The flattened cells g nbasis + i at which an output tile starts (all but the first)."""
    tile = SLAB_ENTRIES // C_TO_CB[C]
    return list(range(tile, G * nbasis, tile))


def cell_keys(x, groups, t, k):
    """The first flattened cell g nbasis + l - k of every sample (its k + 1 entries follow it in row g)."""
    return np.asarray(groups, dtype=np.int64) * (len(t) - k - 1) + intervals(t, k, x) - k


def matrix_case(k, C, N=700):
    """x, V, t, groups, G for one body: about 2.5 output tiles (G nbasis = 2.5 x 768 / CB cells), non-uniform knots with a repeated
    interior knot, x at every knot, at xrange[1], outside the range, and -- for k >= 1 -- on both sides of and across every tile
    seam that lies inside a row.  N = 700 is one sample chunk: three batches for wave 0 and a ragged last batch."""
    rng = np.random.default_rng(1000 * k + C)
    nbasis = 11 + k
    tile = SLAB_ENTRIES // C_TO_CB[C]
    G = -(-5 * tile // (2 * nbasis))
    t = knots(k, nbasis, rng=rng)
    xs, gs = [], []
    for f0 in tile_seams(k, nbasis, G, C):
        g, i = divmod(f0, nbasis)
        # intervals l whose entries l - k .. l end left of the seam, straddle it, start at it
        for l in [i - 1] + list(range(i, i + k)) + [i + k]:
            if k <= l <= nbasis - 1 and t[l] < t[l + 1]:
                xs.append(0.5 * (t[l] + t[l + 1]))
                gs.append(g)
    fixed = np.r_[xs, t, 1.0]
    x = np.r_[fixed, rng.uniform(-1.4, 1.4, N - len(fixed))]
    groups = np.r_[gs, rng.integers(0, G, N - len(gs))].astype(np.int64)
    perm = rng.permutation(N)
    return x[perm], rng.normal(size=(N, C))[perm], t, groups[perm], G


def scipy_case(k, N=300):
    """x, t for the comparison with scipy's design matrix bit for bit: non-uniform knots with a repeated interior knot, x at the
    knots, inside and outside the range; one sample per group (G = N)."""
    rng = np.random.default_rng(50 + k)
    t = knots(k, 11 + k, -1.0, 2.0, rng=rng)
    x = np.r_[t, 2.0, -1.0, rng.uniform(-1.5, 2.5, N - len(t) - 2)]
    return x, t


# ---- the cases of tests/golden/fes_spline.npz (tests/golden/make_golden_fes_spline.py) ------------------------------------------
def fkbias_list(centers, Ku):
    return [lambda x, c=c: (Ku / 2.0) * (x - c) ** 2 for c in centers]


def gaussian_prior(sigma):
    """log p(c) = -sum_i (c_{i+1} - c_i)^2 / (2 sigma^2) and its first two derivatives with respect to c[1:]."""
    a = 1.0 / (2.0 * sigma ** 2)

    def logprior(c):
        return -a * np.sum(np.diff(c) ** 2)

    def dlogprior(c):
        d = np.diff(c)
        g = np.zeros(len(c))
        g[:-1] += d
        g[1:] -= d
        return (2.0 * a * g)[1:]

    def ddlogprior(c):
        n = len(c)
        h = np.zeros([n, n])
        np.fill_diagonal(h, -2.0)
        np.fill_diagonal(h[1:], 1.0)
        np.fill_diagonal(h[:, 1:], 1.0)
        h[0, 0] = h[n - 1, n - 1] = -1.0
        return (2.0 * a * h)[1:, 1:]

    return logprior, dlogprior, ddlogprior


def spline_cases(g):
    """name -> spline_parameters of every fitted case of the fixture (fresh dicts)."""
    xrange = [float(v) for v in g["xrange"]]
    centers = g["bias_centers"]
    fk = fkbias_list(centers, float(g["Ku"]))
    bc = g["bin_centers"]

    def params(weights, nspline, kdegree, algo, init, opts, **extra):
        p = dict(spline_weights=weights, nspline=nspline, kdegree=kdegree, xrange=list(xrange), optimization_algorithm=algo,
                 spline_initialize=init, optimize_options=dict(opts), fkbias=fk, objective="ml", map_data=None)
        p.update(extra)
        return p

    lp, dlp, ddlp = gaussian_prior(float(g["sigma"]))
    return {
        "a": params("unbiasedstate", 4, 3, "Newton-CG", "explicit", {"disp": False, "tol": 1e-6}, xinit=bc,
                    yinit=0.5 * float(g["K0"]) * bc ** 2),
        "b": params("biasedstates", 10, 3, "BFGS", "zeros", {"disp": False, "gtol": 1e-6}),
        "c": params("simplesum", 10, 3, "L-BFGS-B", "bias_free_energies", {"disp": False, "gtol": 1e-8, "ftol": 1e-14},
                    bias_centers=centers),
        "c2": params("biasedstates", 3, 2, "Newton-CG", "bias_free_energies", {"disp": False, "tol": 1e-8}, bias_centers=centers),
        "c3": params("unbiasedstate", 6, 3, "CG", "bias_free_energies", {"disp": False, "gtol": 1e-6}),
        "c4": params("unbiasedstate", 6, 3, "TNC", "zeros", {"disp": False, "tol": 1e-10}),
        "c5": params("unbiasedstate", 6, 3, "SLSQP", "zeros", {"disp": False, "ftol": 1e-12}),
        "d": params("unbiasedstate", 8, 3, "Newton-CG", "zeros", {"disp": False, "tol": 1e-8}, objective="map",
                    map_data=dict(logprior=lp, dlogprior=dlp, ddlogprior=ddlp)),
    }
