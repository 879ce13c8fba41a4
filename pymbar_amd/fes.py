"""Histogram free energy surfaces on the MI355X path: the weight extraction of ``pymbar.FES``.

The reference's ``FES`` pulls two things out of its ``MBAR`` object (pymbar/fes.py:403-416, 1383-1406):

* the unnormalised log weights of the samples in the target potential ``u_n``,
  ``log_w_n = mbar._computeUnnormalizedLogWeights(u_n)`` (:410), from which the bin free energies are
  ``f_i = -logsumexp(log_w_n[samples of bin i])`` (:585);
* for analytical uncertainties, an ``N x (K + nbins)`` weight matrix -- ``exp(Log_W_nk)`` plus one column per populated
  bin, ``W[n, K+i] = exp(log_w_n + f_i)`` on the bin's samples and 0 elsewhere (:1388-1402) -- handed to
  ``_computeAsymptoticCovarianceMatrix`` (:1406).

Here neither matrix exists on the host.  A bin is an *unsampled state* of an augmented reduced-potential matrix whose
row is ``u_n`` on the bin's own samples and ``+inf`` (weight zero) everywhere else; the rows are built on the device from
one vector and one label array (``mbar_ctx_fill_masked_rows``), the bin free energies are the all-state log-space
reduction the solver already has (``mbar_lognum``: ``f_i = -log sum_{n in bin i} exp(-u_n - logden_n)``), and the
covariance input ``W^T W`` of the augmented weights is one MFMA Gram sweep (``mbar_gram_w``).

The histogram estimator's weight extraction is mirrored here (binning conventions, reference points and the uncertainty
formula of ``FES._get_fes_histogram``).  :class:`FES` puts it behind the reference's class interface together with kernel-density
surfaces, whose sums run in ``pymbar_amd.kde`` (its own device path, not the K x N matrix), and spline surfaces with the
reference's Monte Carlo sampler of the spline coefficients, whose sums over the samples are B-spline moments computed once per
fit in ``pymbar_amd.bspline``.

Above ``K + nbins = 256`` rows, and for every bootstrap replicate, a bin is not a row but a LABEL of the samples of the mbar's
own resident matrix (:func:`histogram_fes_labels`): the bin free energies are a segmented log-sum-exp over N numbers
(``mbar_bin_lognum``), and the covariance of the bins follows from the resident ``K x K`` Gram matrix, a ``K x nbins`` cross block
and the diagonal of the bin block (``mbar_bin_gram_w``) through a ``K x K`` eigenproblem -- no second matrix, no ``Theta`` of
order ``K + nbins``.  A bootstrap replicate is one re-solve on the resident matrix with draw counts as sample multiplicities plus
one pass over N numbers.
"""
import logging

import numpy as np

from .utils import ConvergenceError, DataError, ParameterError, bordered_theta_factors

logger = logging.getLogger(__name__)


def unnormalized_log_weights(mbar, u_n):
    """``log_w_n`` of pymbar/fes.py:410 (``-u_n - logden_n``, one device sweep)."""
    return mbar._computeUnnormalizedLogWeights(np.asarray(u_n, dtype=np.float64))


def label_samples(x_n, bin_edges):
    """Bin labels the way pymbar/fes.py:519-563 assigns them on a regular grid: ``sample_label[n]`` numbers the POPULATED
    bins in order of first appearance (the reference's ``bin_order``).  Like the reference, the two overflow regions are
    bins of their own when populated: samples left of the first edge (grid index -1 in some dimension; the reference
    labels them -1 and still gives that label a free energy and a covariance column, fes.py:537-547) and samples right
    of the last edge (``np.digitize`` index ``len(edges) - 1``).  Returns ``(sample_label, grid_of_label)`` with
    ``grid_of_label[i]`` the tuple of per-dimension grid indices of label ``i`` (``None`` for the left-overflow bin)."""
    x_n = np.asarray(x_n, dtype=np.float64)
    if x_n.ndim == 1:
        x_n = x_n[:, None]
    if np.ndim(bin_edges[0]) == 0:
        bin_edges = [bin_edges]
    dims = len(bin_edges)
    if x_n.shape[1] != dims:
        raise DataError("x_n and bin_edges have inconsistent dimension")
    N = len(x_n)
    if N == 0:
        return np.zeros(0, dtype=np.int64), []
    bin_n = [np.digitize(x_n[:, d], bin_edges[d]) - 1 for d in range(dims)]  # each in -1 .. len(edges) - 1
    sizes = tuple(len(bin_edges[d]) + 1 for d in range(dims))
    # one integer per grid cell (0 = "off the grid to the left in some dimension": all such samples share the reference's
    # label -1), then the populated cells numbered in order of first appearance -- without a Python loop over the samples
    left = np.zeros(N, dtype=bool)
    for b in bin_n:
        left |= b < 0
    P = float(np.prod(sizes, dtype=np.float64)) + 1.0
    if P >= 2.0 ** 62:
        # more cells than an int64 can number (many dimensions): sort the samples' index TUPLES instead of flat cell numbers
        stacked = np.stack([np.where(left, -1, b) for b in bin_n], axis=1)  # (all left-overflow samples share one tuple)
        tuples, first, inv = np.unique(stacked, axis=0, return_index=True, return_inverse=True)
        by_first = np.argsort(first, kind="stable")
        rank = np.empty(len(tuples), dtype=np.int64)
        rank[by_first] = np.arange(len(tuples))
        sample_label = rank[np.asarray(inv).reshape(-1)]
        grid = [None if t[0] < 0 else tuple(int(v) for v in t) for t in tuples[by_first]]
        return sample_label, grid
    flat = np.ravel_multi_index(tuple(b + 1 for b in bin_n), sizes) + 1
    flat[left] = 0
    P = int(P)
    if P <= 50_000_000 and P <= 8 * N + 1024:
        # a grid no larger than a few cells per sample: tabulate it (two int64 tables over the grid, no sort)
        first = np.full(P, N, dtype=np.int64)
        first[flat[::-1]] = np.arange(N - 1, -1, -1)  # (duplicates: the last write wins, so the smallest n is kept)
        cells = np.nonzero(first < N)[0]
        cells = cells[np.argsort(first[cells], kind="stable")]
        rank = np.zeros(P, dtype=np.int64)
        rank[cells] = np.arange(len(cells))
        sample_label = rank[flat]
    else:  # a fine grid and few samples (or a huge grid): sort the samples' cells instead of tabulating the grid
        cells, first, inv = np.unique(flat, return_index=True, return_inverse=True)
        by_first = np.argsort(first, kind="stable")
        rank = np.empty(len(cells), dtype=np.int64)
        rank[by_first] = np.arange(len(cells))
        sample_label = rank[inv]
        cells = cells[by_first]
    grid = [None if c == 0 else tuple(int(v) - 1 for v in np.unravel_index(int(c) - 1, sizes)) for c in cells]
    return sample_label, grid


def histogram_fes(mbar, u_n, sample_label, reference="from-lowest", reference_label=None, uncertainty_method="analytical",
                  theta_method=None):
    """Free energies of the populated histogram bins and their uncertainties, relative to a reference bin.

    ``sample_label[n]`` in ``[0, nbins)`` is the bin of sample ``n`` (-1: not in any bin); every label below ``nbins =
    max + 1`` must occur.  ``reference``: "from-lowest" (the bin of lowest free energy) or "from-specified"
    (``reference_label``) -- pymbar/fes.py:1362-1376.  ``uncertainty_method``: "analytical" (fes.py:1381-1415) or None.

    Returns ``dict(f_i, df_i, f_raw, reference, Theta)``; ``f_raw`` are the bin free energies before the reference
    is subtracted (``histogram_data["f"]`` of the reference)."""
    from .expectations import _augmented_solve, _resident_plus_rows

    u_n = np.ascontiguousarray(u_n, dtype=np.float64)
    sample_label = np.asarray(sample_label, dtype=np.int64)
    K, N = mbar.K, mbar.N
    if u_n.shape != (N,) or sample_label.shape != (N,):
        raise ParameterError("u_n and sample_label must have one entry per sample")
    nbins = int(sample_label.max()) + 1 if N > 0 else 0
    if nbins < 1:
        raise DataError("no sample falls into any bin")
    counts = np.bincount(sample_label[sample_label >= 0], minlength=nbins)
    if np.any(counts == 0):
        raise DataError(f"WARNING: bin {int(np.where(counts == 0)[0][0])} has no samples -- all bins must have at least one sample.")
    if uncertainty_method not in (None, "analytical"):
        raise ParameterError(f"Uncertainty_method {uncertainty_method} is not a valid option")

    dm, N_aug = _resident_plus_rows(mbar, nbins, getattr(mbar, "_device", None))
    try:
        dm.fill_masked_rows(K, nbins, u_n, sample_label)  # one "state" per bin: u_n on its samples, +inf elsewhere
        dm.set_Nk(N_aug)
        f_full, _ = _augmented_solve(dm, K, nbins, mbar.f_k)
        f_raw = f_full[K:].copy()  # = -logsumexp(log_w_n[bin])   (fes.py:585)
        j = _reference_bin(f_raw, reference, reference_label)
        out = dict(f_i=f_raw - f_raw[j], f_raw=f_raw, reference=j)
        if uncertainty_method == "analytical":
            G, wsum = dm.gram_w(f_full)
            Theta = mbar._theta_from_gram(G, N_aug.astype(np.int64), theta_method, wsum=wsum, dm=dm, f_full=f_full)
            d = np.diag(Theta)[K:]
            var = d + d[j] - 2.0 * Theta[K:, K + j]
            out["df_i"] = np.sqrt(np.maximum(var, 0.0))
            out["Theta"] = Theta
    finally:
        dm.close()
    return out


ROW_PATH_MAX_ROWS = 256  # K + nbins up to which FES builds one matrix row per bin (the matrix-core Gram panels end at 256 rows)


def _draw_bootstrap_indices(N_k, idx):
    """One bootstrap replicate's indices into ``idx``, from the global NumPy stream exactly as the reference draws them
    (pymbar/fes.py:395-405): per state the resampled indices, then the one int32 the per-state ``MBAR`` construction that is
    skipped here would draw for its seed (mbar.py:273-274)."""
    index = 0
    for k in range(len(N_k)):
        idx[index:index + N_k[k]] = index + np.random.randint(0, N_k[k], size=N_k[k])
        index += N_k[k]
        np.random.randint(np.iinfo(np.int32).max)
    return idx


# (shared with the scans over a linear family, pymbar_amd/scan.py: the same border, dense instead of diagonal)
_bordered_theta_factors = bordered_theta_factors


def _check_labels(mbar, u_n, sample_label):
    u_n = np.ascontiguousarray(u_n, dtype=np.float64)
    sample_label = np.asarray(sample_label, dtype=np.int64)
    N = mbar.N
    if u_n.shape != (N,) or sample_label.shape != (N,):
        raise ParameterError("u_n and sample_label must have one entry per sample")
    nbins = int(sample_label.max()) + 1 if N > 0 else 0
    if nbins < 1:
        raise DataError("no sample falls into any bin")
    if int(sample_label.min()) < -1:
        raise ParameterError("sample_label must lie in [-1, nbins)")
    return u_n, sample_label, nbins


def _binned_matrix(mbar, what):
    """The mbar's resident matrix, if its handle has the binned passes (``set_bins`` / ``bin_lognum`` / ``bin_gram_w``: the
    single-rank :class:`pymbar_amd.device.DeviceMatrix`); any other handle cannot label its samples."""
    dm = mbar._dm
    if getattr(dm, "nranks", 1) != 1 or not all(hasattr(dm, name) for name in ("set_bins", "bin_lognum", "bin_gram_w")):
        raise ParameterError(f"{what} need the binned passes of a single-rank device matrix and are {_NOT_HERE} for this handle")
    return dm


def _reference_bin(f_raw, reference, reference_label):
    nbins = len(f_raw)
    if reference == "from-lowest":
        return int(np.argmin(f_raw))
    if reference == "from-specified":
        if reference_label is None or not (0 <= int(reference_label) < nbins):
            raise ParameterError("Specified reference point for FES not given")
        return int(reference_label)
    raise ParameterError(f"reference point method {reference} is not supported for histogram surfaces here")


def histogram_fes_labels(mbar, u_n, sample_label, reference="from-lowest", reference_label=None, uncertainty_method="analytical",
                         theta_method=None, return_theta=False):
    """:func:`histogram_fes` with the bins as LABELS of the samples of ``mbar``'s own resident matrix: the same arguments, checks
    and result keys (``f_i, df_i, f_raw, reference``), no second device matrix and no ``Theta`` of order ``K + nbins``.

    The bin free energies are ``-mbar_bin_lognum``; the analytical uncertainties come from the resident ``W^T W``, the ``K x
    nbins`` cross block and the diagonal of the bin block (``mbar_bin_gram_w``) through :func:`_bordered_theta_factors`, and
    ``df_i^2 = Theta_ii + Theta_jj - 2 Theta_ij`` needs column ``j`` only.  ``theta_method``: None / "svd-ew" (the bordered
    form), "approximate" (``diag(d)``, the bin block of ``W^T W`` itself); "svd" is not offered on this path.
    ``return_theta=True`` adds ``Theta_bins`` (``nbins x nbins``) to the result."""
    from .utils import check_w_sums

    u_n, sample_label, nbins = _check_labels(mbar, u_n, sample_label)
    if uncertainty_method not in (None, "analytical"):
        raise ParameterError(f"Uncertainty_method {uncertainty_method} is not a valid option")
    if theta_method == "bootstrap":
        theta_method = None
    if theta_method == "svd":
        raise ParameterError("theta_method 'svd' needs the weight matrix itself and is not offered on the label path")
    if theta_method not in (None, "svd-ew", "approximate"):
        raise ParameterError(f"Method {theta_method} unrecognized.")
    dm = _binned_matrix(mbar, "histogram surfaces by bin label")
    dm.set_Nk(mbar.N_k)
    dm.set_bins(nbins, sample_label, u_n)
    try:
        f_raw = -dm.bin_lognum(mbar.f_k)  # = -logsumexp(log_w_n[bin])   (fes.py:585)
        if not np.all(np.isfinite(f_raw)):  # (a bin without samples has lognum = -inf: looked for only then)
            counts = np.bincount(sample_label[sample_label >= 0], minlength=nbins)
            if np.any(counts == 0):
                raise DataError(f"WARNING: bin {int(np.where(counts == 0)[0][0])} has no samples -- all bins must have at least one sample.")
        j = _reference_bin(f_raw, reference, reference_label)
        out = dict(f_i=f_raw - f_raw[j], f_raw=f_raw, reference=j)
        if uncertainty_method == "analytical":
            approximate = theta_method == "approximate"
            C, d, wsum = dm.bin_gram_w(mbar.f_k, f_raw, cross=not approximate)
            check_w_sums(wsum, 0.0)
            if approximate:
                var = d + d[j]
                var[j] = 0.0
                Y = g = None
            else:
                G, ws = mbar._gram_w()
                check_w_sums(ws, 0.0)
                Y, g = _bordered_theta_factors(G, C, mbar.N_k)
                col = Y.T @ (g * Y[:, j])  # column j of Y^T diag(g) Y
                border = np.einsum("ki,k,ki->i", Y, g, Y)
                diag_theta = d + border
                col[j] += d[j]
                var = diag_theta + diag_theta[j] - 2.0 * col
            out["df_i"] = np.sqrt(np.maximum(var, 0.0))
            if return_theta:
                out["Theta_bins"] = np.diag(d) if approximate else np.diag(d) + Y.T @ (g[:, None] * Y)
    finally:
        dm.set_bins(0)
    return out


_NOT_HERE = "not supported on this backend"
SPLINE_WEIGHTS = ("unbiasedstate", "biasedstates", "simplesum")
SPLINE_SCIPY_METHODS = ("Newton-CG", "CG", "BFGS", "L-BFGS-B", "TNC", "SLSQP")
_SPLINE_REQUIRED = ("spline_weights", "nspline", "kdegree", "xrange", "optimization_algorithm", "spline_initialize")
CUSTOM_NR_MAXITER = 500  # Newton steps of optimization_algorithm="Custom-NR" before ConvergenceError


class FES:
    """``pymbar.FES`` on the MI355X path (pymbar/fes.py:74-1609): the MBAR solve on the device, histogram surfaces through
    :func:`label_samples` / :func:`histogram_fes`, kernel-density surfaces through :class:`pymbar_amd.kde.KernelDensity`.

    Supported: ``fes_type="histogram"`` (``get_fes`` from-lowest / from-specified, uncertainties None, "analytical" or
    "bootstrap"; one matrix row per bin up to ``K + nbins = 256``, bins as labels of the resident samples above that and for every
    bootstrap replicate: :func:`histogram_fes_labels`),
    ``fes_type="kde"`` (from-lowest / from-specified / from-normalization, uncertainties None or "bootstrap") and
    ``fes_type="spline"`` (from-lowest / from-specified, uncertainties None or "bootstrap", information criteria, and the Monte
    Carlo sampler of the coefficients: ``sample_parameter_distribution``, ``get_confidence_intervals``, ``get_mc_data``).
    The histogram from-normalization / all-differences modes raise ``ParameterError``, as they do in the reference.  The deliberate
    differences from the reference are listed in INTEGRATION.md ("FES")."""

    _w_kn = None  # exp(mbar.Log_W_nk), built on first access and dropped by every new surface

    def __init__(self, u_kn, N_k, verbose=False, mbar_options=None, timings=True, **kwargs):
        from .mbar import MBAR
        from .utils import kln_to_kn

        for key, val in kwargs.items():
            logger.warning(f"Warning: parameter {key}={val} is unrecognized and unused.")
        self.N_k = np.array(N_k, dtype=np.int64)
        if np.ndim(u_kn) == 3:
            u_kn = kln_to_kn(u_kn, N_k=self.N_k)
        self.u_kn = np.array(u_kn, dtype=np.float64)
        K, N = self.u_kn.shape
        if np.sum(self.N_k) != N:
            raise ParameterError(
                "The sum of all N_k must equal the total number of samples (length of second dimension of u_kn.")
        self.K, self.N = K, N
        self.verbose = verbose
        self.timings = bool(timings)
        if mbar_options is None:
            self.mbar = MBAR(self.u_kn, self.N_k)
        else:  # the reference's defaults for the options it does not find (fes.py:160-200)
            opts = dict(mbar_options)
            for o in ("maximum_iterations", "relative_tolerance", "verbose", "initial_f_k", "solver_protocol", "initialize",
                      "x_kindices"):
                opts.setdefault(o, None)
            if opts["maximum_iterations"] is None:
                opts["maximum_iterations"] = 10000
            if opts["relative_tolerance"] is None:
                opts["relative_tolerance"] = 1.0e-7
            if opts["initialize"] is None:
                opts["initialize"] = "zeros"
            self.mbar = MBAR(self.u_kn, self.N_k, maximum_iterations=opts["maximum_iterations"],
                             relative_tolerance=opts["relative_tolerance"], verbose=bool(opts["verbose"]),
                             initial_f_k=opts["initial_f_k"], solver_protocol=opts["solver_protocol"],
                             initialize=opts["initialize"], x_kindices=opts["x_kindices"])
        self.fes_type = None
        self.kde = None
        self.kdes = None
        self.histogram_data = None
        self.histogram_datas = None
        self.n_bootstraps = 0
        self.bootstrap_weights = None
        self.spline_parameters = None
        self.spline_data = None
        self.fes_function = None
        self.fes_functions = None
        self.mc_data = None
        if self.verbose:
            logger.info("FES initialized")

    # ---- generate ---------------------------------------------------------------------------------------------------------
    def generate_fes(self, u_n, x_n, fes_type="histogram", histogram_parameters=None, kde_parameters=None,
                     spline_parameters=None, n_bootstraps=0, seed=-1):
        """Build the surface (pymbar/fes.py:221-438).  histogram: replicate b re-solves MBAR on the resident matrix with its draw
        counts as sample multiplicities and takes the bin free energies in one pass over N numbers (``_histogram_replicates``).
        kde: the replicates of ``n_bootstraps > 0`` draw from the global NumPy
        stream exactly as the reference does and become weight columns over the ORIGINAL positions (see ``_generate_kde``)."""
        from timeit import default_timer as timer

        from .utils import kn_to_n

        result_vals = dict()
        self.fes_type = fes_type
        if np.ndim(u_n) == 2:
            u_n = kn_to_n(u_n, N_k=self.N_k)
        self.u_n = np.asarray(u_n, dtype=np.float64)
        if seed >= 0:
            np.random.seed(seed)
        if not np.issubdtype(type(n_bootstraps), np.integer) or n_bootstraps == 1:
            raise ValueError(f"n_bootstraps must be an integer of 0 or >=2, it was set to {n_bootstraps}")
        self.n_bootstraps = n_bootstraps
        start = timer()
        x_n = np.asarray(x_n, dtype=np.float64)
        if x_n.ndim == 1:
            x_n = x_n.reshape(-1, 1)
        if fes_type == "histogram":
            self._generate_histogram(x_n, histogram_parameters, n_bootstraps)
        elif fes_type == "kde":
            self._generate_kde(x_n, kde_parameters, n_bootstraps)
        elif fes_type == "spline":
            self._generate_spline(x_n, spline_parameters, n_bootstraps)
        else:
            raise ParameterError(f"fes_type {fes_type} is not defined!")
        if self.timings:
            result_vals["timing"] = timer() - start
        return result_vals

    def _normalized_weights(self):
        log_w_n = self.mbar._computeUnnormalizedLogWeights(self.u_n)  # (fes.py:403-410)
        w_n = np.exp(log_w_n - np.max(log_w_n))
        return w_n / np.sum(w_n)

    def _generate_kde(self, x_n, kde_parameters, n_bootstraps):
        from .kde import SKLEARN_PARAMS, KernelDensity

        kde_parameters = {} if kde_parameters is None else kde_parameters
        for k in kde_parameters:
            if k not in SKLEARN_PARAMS:
                raise ParameterError(f"Warning: {k} is not a parameter in KernelDensity")
        kde = KernelDensity()
        kde.set_params(**{k: v for k, v in kde_parameters.items()})
        self.kde_parameters = kde_parameters
        if len(x_n) != self.N:
            raise DataError("x_n must have one row per sample")
        self.w_n = self._normalized_weights()
        self._w_kn = None
        kde.fit(x_n, sample_weight=self.w_n)
        self.kde = kde
        self._kde_dim = x_n.shape[1]
        # Replicate b of the reference (fes.py:385-400, 696) refits on x_n[bootstrap_indices] with the b = 0 weights self.w_n:
        # a KDE over the original positions with weights v_b[n] = sum of w_n[j] over the draws j with bootstrap_indices[j] = n.
        # Its per-replicate MBAR solves (fes.py:403, one per state) change nothing a KDE surface reads and are skipped; the draws
        # are the reference's, from the global stream, state by state, in the same order, and each skipped MBAR construction
        # still takes the one number it draws for its own seed (mbar.py:273-274).
        N_k = self.mbar.N_k
        cols = np.empty((self.N, n_bootstraps + 1), dtype=np.float64)
        cols[:, 0] = self.w_n
        idx = np.arange(0, self.N)
        for b in range(1, n_bootstraps + 1):
            _draw_bootstrap_indices(N_k, idx)
            cols[:, b] = np.bincount(idx, weights=self.w_n, minlength=self.N)
        self.bootstrap_weights = cols
        self.kdes = None  # (the replicates are the columns 1..B of bootstrap_weights, evaluated in one device pass)

    @property
    def w_kn(self):
        """``exp(mbar.Log_W_nk)`` (fes.py:413): built on first access only."""
        if self._w_kn is None:
            self._w_kn = np.exp(self.mbar.Log_W_nk)
        return self._w_kn

    def _histogram_rows(self, nbins):
        """Whether the surface builds one matrix row per bin (:func:`histogram_fes`) or labels the samples."""
        return self.K + nbins <= ROW_PATH_MAX_ROWS

    def _histogram_replicates(self, labels, nbins, n_bootstraps):
        """The bootstrap replicates of a histogram surface (pymbar/fes.py:388-424): the draws of the reference from the global
        stream, MBAR re-solved from ``mbar.f_k`` with the draw counts as sample multiplicities on the resident matrix (the
        reference's MBAR on the resampled matrix), and the bin free energies of the resampled data -- ``-mbar_bin_lognum`` with the
        same multiplicities -- in the b = 0 bin order.  A bin that drew no sample has ``f = +inf`` in that replicate.  No N-vector
        returns to the host per replicate."""
        from .mbar_solvers import solve_mbar_for_all_states

        mbar, N = self.mbar, self.N
        N_k = mbar.N_k
        dm = _binned_matrix(mbar, "histogram surfaces with n_bootstraps > 0")
        self.histogram_datas = []
        self._hist_f_boots = []
        idx = np.arange(0, N)
        dm.set_Nk(N_k)
        dm.set_bins(nbins, labels, self.u_n)
        try:
            for _ in range(n_bootstraps):
                _draw_bootstrap_indices(N_k, idx)
                counts = np.bincount(idx, minlength=N).astype(np.float64)
                dm.set_sample_weights(counts)
                f_b = solve_mbar_for_all_states(dm, N_k, mbar.f_k, mbar.states_with_samples, None)
                self.histogram_datas.append(dict(f=-dm.bin_lognum(f_b)))
                self._hist_f_boots.append(f_b)
        finally:
            dm.set_sample_weights(None)
            dm.set_Nk(N_k)
            dm.set_bins(0)

    def _generate_histogram(self, x_n, histogram_parameters, n_bootstraps=0):
        if histogram_parameters is None or "bin_edges" not in histogram_parameters:
            raise ParameterError("histogram_parameters['bin_edges'] cannot be undefined with fes_type = histogram")
        bins = histogram_parameters["bin_edges"]
        if np.ndim(bins[0]) == 0:
            bins = [bins]
        bins = [np.asarray(b, dtype=np.float64) for b in bins]
        self.histogram_parameters = dict(histogram_parameters, bin_edges=bins)
        if x_n.shape != (self.N, len(bins)):
            raise DataError("x_n and bin_edges have inconsistent dimension")
        if n_bootstraps > 0:
            _binned_matrix(self.mbar, "histogram surfaces with n_bootstraps > 0")
        self.w_n = self._normalized_weights()
        self._w_kn = None
        labels, grid = label_samples(x_n, bins)
        surface = histogram_fes if self._histogram_rows(len(grid)) else histogram_fes_labels
        raw = surface(self.mbar, self.u_n, labels, uncertainty_method=None)
        # bins are numbered in order of first appearance like the reference's bin_order (fes.py:552-560); grid_of_label[i] is
        # the tuple of grid indices of bin i (None: the bin of the samples left of the grid)
        self.histogram_data = dict(bins=bins, dims=len(bins), f=raw["f_raw"], sample_label=labels, grid_of_label=grid,
                                   label_of_grid={g: i for i, g in enumerate(grid) if g is not None})
        self.histogram_datas = None
        if n_bootstraps > 0:
            self._histogram_replicates(labels, len(grid), n_bootstraps)

    # ---- evaluate ---------------------------------------------------------------------------------------------------------
    def get_fes(self, x, reference_point="from-lowest", fes_reference=None, uncertainty_method=None):
        """Free energies (and uncertainties) at the points x (pymbar/fes.py:1167-1231)."""
        x = np.array(x, dtype=np.float64)
        if x.ndim <= 1:
            x = x.reshape(-1, 1)
        if self.fes_type == "histogram":
            return self._get_fes_histogram(x, reference_point, fes_reference, uncertainty_method)
        if self.fes_type == "kde":
            return self._get_fes_kde(x, reference_point, fes_reference, uncertainty_method)
        if self.fes_type == "spline":
            return self._get_fes_spline(x, reference_point, fes_reference, uncertainty_method)
        raise ParameterError(f"fes_type {self.fes_type} is not supported")

    def _get_fes_kde(self, x, reference_point, fes_reference, uncertainty_method):
        if x.shape[1] != self._kde_dim:
            raise DataError("query coordinates have inconsistent dimension with the data the FES is fit to.")
        if reference_point not in ("from-lowest", "from-specified", "from-normalization"):
            raise ParameterError(f"reference point choice {reference_point} for kde is unavailable")
        if uncertainty_method not in (None, "bootstrap"):
            raise ParameterError(f"Uncertainty method {uncertainty_method} for kde is not implemented")
        if uncertainty_method == "bootstrap" and self.n_bootstraps == 0:
            raise ParameterError("Cannot calculate bootstrap error of bootstrap KDE's not determined")
        M = len(x)
        q = x
        if reference_point == "from-specified":
            ref = np.array(fes_reference, dtype=np.float64).reshape(1, -1)
            if ref.shape[1] != self._kde_dim:
                raise DataError("fes_reference has inconsistent dimension with the data the FES is fit to.")
            q = np.vstack([x, ref])
        if uncertainty_method == "bootstrap":
            L = self.kde.score_samples_columns(q, self.bootstrap_weights)  # all replicates in one pass
        else:
            L = self.kde.score_samples(q)[:, None]
        f_all = -L[:, 0]
        f_i = f_all[:M]
        fmin = 0.0
        if reference_point == "from-lowest":
            fmin = np.min(f_i)
        elif reference_point == "from-specified":
            fmin = f_all[M]
        f_i = f_i - fmin
        df_i = None
        if uncertainty_method == "bootstrap":
            df_i = np.std(-L[:M, 1:] - fmin, axis=1)  # (from-normalization: no shift, the spread is the same)
        return {"f_i": f_i, "df_i": df_i}

    def _get_fes_histogram(self, x, reference_point, fes_reference, uncertainty_method):
        hd = self.histogram_data
        bins, dims = hd["bins"], hd["dims"]
        if x.shape[1] != dims:
            raise DataError("query coordinates have inconsistent dimension with the data the FES is fit to.")
        if uncertainty_method not in (None, "analytical", "bootstrap"):
            raise ParameterError(f"Uncertainty_method {uncertainty_method} is not a valid option")
        if uncertainty_method == "bootstrap" and not self.histogram_datas:
            raise ParameterError(f"bootstrap uncertainties of a histogram surface generated without replicates (n_bootstraps = 0) are {_NOT_HERE}")
        if reference_point in ("from-normalization", "all-differences"):  # (the reference raises for both too, fes.py:1369-1448)
            raise ParameterError(f"reference point {reference_point!r} for histogram surfaces is {_NOT_HERE}")
        ref_label = None
        if reference_point == "from-specified":
            if fes_reference is None:
                raise ParameterError("Specified reference point for FES not given")
            ref = np.atleast_1d(np.asarray(fes_reference, dtype=np.float64))
            g = tuple(int(np.digitize(ref[d], bins[d]) - 1) for d in range(dims))
            if any(gd < 0 or gd >= len(bins[d]) - 1 for d, gd in enumerate(g)) or g not in hd["label_of_grid"]:
                raise ParameterError(f"Specified reference point {ref} is not in a populated bin of the FES region")
            ref_label = hd["label_of_grid"][g]
        elif reference_point != "from-lowest":
            raise ParameterError(f"reference point {reference_point!r} is not a valid option")
        if uncertainty_method == "bootstrap":
            # pymbar/fes.py:1417-1422: the spread over the replicates of f^b_i - f^b_j, j from the b = 0 surface.  A replicate in
            # which bin i or the reference bin drew no sample (f = +inf) is left out of bin i's spread; fewer than two usable
            # replicates: NaN.  (The reference cannot broadcast such a replicate into its table and raises.)
            f_raw = hd["f"]
            j = _reference_bin(f_raw, reference_point, ref_label)
            fall = np.stack([h["f"] - h["f"][j] if np.isfinite(h["f"][j]) else np.full(len(f_raw), np.nan)
                             for h in self.histogram_datas], axis=1)
            fall[~np.isfinite(fall)] = np.nan
            usable = np.sum(~np.isnan(fall), axis=1)
            df = np.full(len(f_raw), np.nan)
            ok = usable >= 2
            if np.any(ok):
                df[ok] = np.nanstd(fall[ok], axis=1)
            res = dict(f_i=f_raw - f_raw[j], df_i=df)
        else:
            surface = histogram_fes if self._histogram_rows(len(hd["f"])) else histogram_fes_labels
            res = surface(self.mbar, self.u_n, hd["sample_label"], reference=reference_point, reference_label=ref_label,
                          uncertainty_method=uncertainty_method)
        # each query point to its bin (fes.py:1419-1440): NaN outside the grid and in bins without samples
        loc = np.stack([np.digitize(x[:, d], bins[d]) - 1 for d in range(dims)], axis=1)
        f_x = np.full(len(x), np.nan)
        df_x = np.full(len(x), np.nan)
        for i, l in enumerate(loc):
            if np.any(l < 0) or any(l[d] >= len(bins[d]) - 1 for d in range(dims)):
                continue
            j = hd["label_of_grid"].get(tuple(int(v) for v in l))
            if j is None:
                continue
            f_x[i] = res["f_i"][j]
            if uncertainty_method is not None:
                df_x[i] = res["df_i"][j]
        out = {"f_i": f_x}
        if uncertainty_method is not None:
            out["df_i"] = df_x
        return out

    # ---- spline surfaces (pymbar/fes.py:701-1166, 1611-2477) --------------------------------------------------------------
    def _setup_spline(self, spline_parameters):
        """Check and complete the parameters (the reference's ``_setup_fes_spline``) on a copy of the caller's dict."""
        sp = {} if spline_parameters is None else dict(spline_parameters)
        for key in _SPLINE_REQUIRED:
            if key not in sp:
                raise ParameterError(f"spline_parameters without '{key}' are {_NOT_HERE}")
        if sp["spline_weights"] not in SPLINE_WEIGHTS:
            raise ParameterError(f"spline_weights {sp['spline_weights']!r} is not one of {SPLINE_WEIGHTS}")
        if sp["spline_weights"] != "unbiasedstate" and "fkbias" not in sp:
            raise ParameterError(f"spline_parameters without 'fkbias' are {_NOT_HERE} for spline_weights {sp['spline_weights']!r}")
        sp.setdefault("objective", "ml")
        if sp["objective"] not in ("ml", "map"):
            raise ParameterError(f"objective may only be 'ml' or 'map': you have selected {sp['objective']}")
        if sp["objective"] == "ml":
            if sp.get("map_data") is not None:
                raise ParameterError("if 'objective' is 'ml' then 'map_data' structure containing priors should not be included")
            sp["map_data"] = dict(logprior=None, dlogprior=None, ddlogprior=None)
        else:
            if "map_data" not in sp:
                raise ParameterError("if 'objective' is 'map' you must include 'map_data' structure")
            if sp["map_data"] is None:
                raise ParameterError("MAP data must be defined if objective is MAP")
            for key, what in (("logprior", "log prior"), ("dlogprior", "d(log prior)"), ("ddlogprior", "d^2(log prior)")):
                if sp["map_data"].get(key) is None:
                    raise ParameterError(f"{what} must be included if objective is MAP")
        algorithm = sp["optimization_algorithm"]
        if algorithm != "Custom-NR":
            if algorithm not in SPLINE_SCIPY_METHODS:
                raise ParameterError(f"Optimization method {algorithm} is not supported")
            opts = dict(sp.get("optimize_options", {"disp": True, "ftol": 1e-7, "xtol": 1e-7}))
            sp["scipy_tol"] = opts.pop("tol", None)  # (scipy takes tol as an argument, not an option)
        else:
            opts = dict(sp.get("optimize_options", {}))
            if "gtol" not in opts:
                opts.setdefault("tol", 1e-7)
        sp["optimize_options"] = opts
        t = np.zeros(int(sp["nspline"]) + int(sp["kdegree"]) + 1)
        from .bspline import check_spline_shape

        check_spline_shape(t, int(sp["kdegree"]))
        self.spline_parameters = sp

    def _initial_spline_points(self):
        """``(xinit, yinit)`` of the three initialisations (the reference's ``_get_initial_spline_points``)."""
        from scipy.interpolate import make_lsq_spline

        sp = self.spline_parameters
        nspline, kdegree, xrange = int(sp["nspline"]), int(sp["kdegree"]), sp["xrange"]
        init = sp["spline_initialize"]
        if init == "bias_free_energies":
            f_k = self.mbar.f_k
            if "bias_centers" not in sp:  # equally spaced centres assumed
                return np.linspace(xrange[0], xrange[1], self.mbar.K + 1)[1:-1], f_k
            centers = np.asarray(sp["bias_centers"])
            order = np.argsort(centers)
            K = self.mbar.K
            if K >= 2 * nspline:
                return centers[order], f_k[order]
            # fewer states than twice the spline points: a coarser least-squares spline through the centres, sampled densely
            nfit = int(np.round(K / 2))
            tfit = self._knots(nfit, kdegree, xrange)
            coarse = make_lsq_spline(centers[order], f_k[order], tfit, k=kdegree)
            xinit = np.linspace(xrange[0], xrange[1], num=2 * nspline)
            return xinit, coarse(xinit)
        if init == "explicit":
            for key in ("xinit", "yinit"):
                if key not in sp:
                    raise ParameterError(f"spline_initialize set as explicit, but no {key} array specified")
            return np.asarray(sp["xinit"]), np.asarray(sp["yinit"])
        if init == "zeros":
            xinit = np.linspace(xrange[0], xrange[1], nspline + kdegree)
            return xinit, np.zeros(len(xinit))
        raise ParameterError(f"Initialization type {init} not recognized")

    @staticmethod
    def _knots(nspline, kdegree, xrange):
        """``nspline + kdegree + 1`` knots: kdegree + 1 at each end of xrange, equally spaced in between."""
        t = np.zeros(nspline + kdegree + 1)
        t[0:kdegree] = xrange[0]
        t[kdegree:nspline + 1] = np.linspace(xrange[0], xrange[1], num=nspline + 1 - kdegree, endpoint=True)
        t[nspline + 1:nspline + kdegree + 1] = xrange[1]
        return t

    def _initial_spline(self, xinit, yinit):
        """The starting spline, the basis elements and their integration ranges (the reference's ``_get_initial_spline``)."""
        from scipy.interpolate import BSpline, make_lsq_spline

        sp = self.spline_parameters
        nspline, kdegree = int(sp["nspline"]), int(sp["kdegree"])
        t = self._knots(nspline, kdegree, sp["xrange"])
        order = np.argsort(xinit)
        b = make_lsq_spline(xinit[order], yinit[order], t, k=kdegree)
        b.c = b.c - b.c[0]  # the surface is defined up to a constant: the first coefficient is held at zero
        basis = [BSpline(b.t, np.eye(nspline)[i], b.k) for i in range(nspline)]
        lo, hi = t[:nspline], t[kdegree + 1:kdegree + 1 + nspline]  # support of basis element i
        xrangei = np.stack([lo, hi], axis=1)
        xrangeij = np.stack([np.maximum(lo[:, None], lo[None, :]), np.minimum(hi[:, None], hi[None, :])], axis=2)
        return dict(initial_coefficients=b.c[1:], bspline_derivatives=basis, bspline=b, xrangei=xrangei, xrangeij=xrangeij)

    def _spline_columns(self, n_bootstraps):
        """Weight columns of the moments: b = 0 and one per bootstrap replicate, drawn from the global stream as the reference
        draws them (per state the resampled indices, then the one number each skipped per-state MBAR construction draws for its
        seed).  unbiasedstate: the replicate's normalised weights over the ORIGINAL positions -- draw counts times the weights
        of MBAR re-solved with the counts as sample multiplicities (the reference's MBAR on the resampled matrix, fes.py:382-395);
        biasedstates / simplesum: the draw counts (a column of ones for b = 0)."""
        from .mbar_solvers import solve_mbar_for_all_states

        mbar, N = self.mbar, self.N
        unbiased = self.spline_parameters["spline_weights"] == "unbiasedstate"
        cols = np.empty((N, n_bootstraps + 1), dtype=np.float64)
        cols[:, 0] = self.w_n if unbiased else 1.0
        self._spline_f_boots = []
        idx = np.arange(0, N)
        N_k = mbar.N_k
        for b in range(1, n_bootstraps + 1):
            _draw_bootstrap_indices(N_k, idx)
            counts = np.bincount(idx, minlength=N).astype(np.float64)
            if not unbiased:
                cols[:, b] = counts
                continue
            dm = mbar._dm
            dm.set_sample_weights(counts)
            try:
                f_b = solve_mbar_for_all_states(dm, N_k, mbar.f_k, mbar.states_with_samples, None)
            finally:
                dm.set_sample_weights(None)
            dm.set_Nk(N_k)
            log_w = -(self.u_n + dm.logden(f_b))
            drawn = counts > 0
            w = np.zeros(N)
            w[drawn] = counts[drawn] * np.exp(log_w[drawn] - np.max(log_w[drawn]))
            cols[:, b] = w / np.sum(w)
            self._spline_f_boots.append(f_b)
        return cols

    def _generate_spline(self, x_n, spline_parameters, n_bootstraps):
        from scipy.optimize import minimize

        from .bspline import DeviceBSplineMoments

        self._setup_spline(spline_parameters)
        sp = self.spline_parameters
        if x_n.shape != (self.N, 1):
            raise DataError("spline surfaces need one 1-D coordinate per sample (x_n of shape (N,) or (N, 1))")
        self.fes_function = None
        self.fes_functions = [] if n_bootstraps > 0 else None
        self.mc_data = None
        self._spline_cache = {}
        self.w_n = self._normalized_weights()
        self._w_kn = None
        self.spline_data = self._initial_spline(*self._initial_spline_points())
        cols = self._spline_columns(n_bootstraps)
        biased = sp["spline_weights"] != "unbiasedstate"
        K = self.mbar.K
        groups = np.asarray(self.mbar.x_kindices) if biased else None
        self._n_kind = np.bincount(np.asarray(self.mbar.x_kindices), minlength=K)
        with DeviceBSplineMoments(x_n[:, 0], groups=groups, n_groups=K if biased else None) as dev:
            dev.set_weights(cols)
            self._spline_M = dev.moments(self.spline_data["bspline"].t, int(sp["kdegree"]))  # (G, 1 + B, nspline)
        func, grad, hess = self._bspline_calculate_f, self._bspline_calculate_g, self._bspline_calculate_h
        for b in range(n_bootstraps + 1):
            x0 = (self.spline_data["initial_coefficients"] if b == 0 else self.spline_data["first_coefficients"]).copy()
            if sp["optimization_algorithm"] == "Custom-NR":
                xi = self._custom_newton_raphson(x0, b)
            else:
                res = minimize(func, x0, args=(b,), method=sp["optimization_algorithm"], jac=grad,
                               hess=hess if sp["optimization_algorithm"] == "Newton-CG" else None, tol=sp["scipy_tol"],
                               options=sp["optimize_options"])
                xi = res["x"]
            spline = self._val_to_spline(xi)
            if b == 0:
                self.spline_data["first_coefficients"] = xi
                mll = func(xi, 0)
                npar = len(xi)
                self.spline_data["aic"] = float(2 * npar + 2 * mll)
                self.spline_data["bic"] = float(2 * np.log(self.N) * npar + 2 * mll)
                self.fes_function = spline
            else:
                self.fes_functions.append(spline)

    def _custom_newton_raphson(self, xi, b):
        """optimization_algorithm="Custom-NR": Newton steps ``dx = lstsq(H, g)``; a step that raises the objective by more than
        10 % (or makes it infinite) is shortened to 0.9 of itself, up to 5 times (infinite: until finite); stop when the
        gradient norm is at most gtol (or tol)."""
        opts = self.spline_parameters["optimize_options"]
        tol = opts["gtol"] if "gtol" in opts else opts["tol"]
        func, grad, hess = self._bspline_calculate_f, self._bspline_calculate_g, self._bspline_calculate_h
        f = func(xi, b)
        for _ in range(CUSTOM_NR_MAXITER):
            g = grad(xi, b)
            gnorm = float(np.sqrt(np.dot(g, g)))
            if opts.get("disp"):
                logger.info(f"f = {f:.10f}. gradient norm = {gnorm:.10f}")
            if gnorm <= tol:
                return xi
            dx = np.linalg.lstsq(hess(xi, b), g, rcond=None)[0]
            xold, fold = xi, f
            xi = xold - dx
            f = func(xi, b)
            count = 0
            while (f >= fold * 1.1 and count < 5) or (not np.isfinite(f) and count < 200):
                dx = 0.9 * dx
                xi = xold - dx
                f = func(xi, b)
                count += 1
        raise ConvergenceError(f"Custom-NR did not reach gradient norm {tol} in {CUSTOM_NR_MAXITER} steps")

    def _val_to_spline(self, xi):
        """The BSpline with coefficients (c_0, xi) on the fitted knots (c_0 = 0)."""
        from scipy.interpolate import BSpline

        template = self.spline_data["bspline"]
        c = np.zeros(len(xi) + 1)
        c[0] = template.c[0]
        c[1:] = xi
        return BSpline(template.t, c, template.k)

    def _spline_scaling(self):
        K = self.mbar.K
        if self.spline_parameters["spline_weights"] == "simplesum":
            return (self.N / K) * np.ones(K)
        return self.mbar.N_k

    def _spline_integrals(self, xi, need_pE):
        """The reference's quadratures at xi, cached per xi (so that the Hessian needs no preceding gradient call):
        pF (unbiasedstate: the partition function of the surface; biased: one per state with its bias) and, with need_pE,
        the normalised Boltzmann averages of the basis elements 1 .. nspline-1 (pE, or gkquad[i, k] per state)."""
        from scipy.integrate import quad

        key = np.asarray(xi, dtype=np.float64).tobytes()
        ent = self._spline_cache.get(key)
        if ent is None:
            if len(self._spline_cache) > 8:
                self._spline_cache.clear()
            ent = self._spline_cache[key] = {}
        if "pF" in ent and (not need_pE or "pE" in ent):
            return ent
        sp = self.spline_parameters
        bloc = self._val_to_spline(xi)
        xr = sp["xrange"]
        basis = self.spline_data["bspline_derivatives"]
        xrangei = self.spline_data["xrangei"]
        nspline = int(sp["nspline"])
        if sp["spline_weights"] == "unbiasedstate":
            def boltz(x):
                return np.exp(-bloc(x))

            if "pF" not in ent:
                ent["pF"] = quad(boltz, xr[0], xr[1])[0]
            if need_pE:
                pE = np.zeros(nspline - 1)
                for i in range(nspline - 1):
                    pE[i] = quad(lambda x, i=i: basis[i + 1](x) * boltz(x), xrangei[i + 1, 0], xrangei[i + 1, 1])[0]
                    pE[i] /= ent["pF"]
                ent["pE"] = pE
        else:
            fkbias = sp["fkbias"]
            K = self.mbar.K

            def boltz(x, k):
                return np.exp(-bloc(x) - fkbias[k](x))

            if "pF" not in ent:
                ent["pF"] = np.array([quad(boltz, xr[0], xr[1], args=(k,))[0] for k in range(K)])
            if need_pE:
                gk = np.zeros([nspline - 1, K])
                for k in range(K):
                    for i in range(nspline - 1):
                        pE = quad(lambda x, k, i=i: basis[i + 1](x) * boltz(x, k), xrangei[i + 1, 0], xrangei[i + 1, 1],
                                  args=(k,))[0]
                        gk[i, k] = pE / ent["pF"][k]
                ent["pE"] = gk
        ent["bloc"] = bloc
        return ent

    def _spline_data_dot(self, c, b):
        """The data term sum over the samples of (weight) x s(x_n) for coefficients c, from the moments of column b."""
        M = self._spline_M
        w = self.spline_parameters["spline_weights"]
        if w == "unbiasedstate":
            return self.N * float(np.dot(c, M[0, b]))
        f = 0.0
        for k in range(self.mbar.K):
            if w == "biasedstates":
                f += float(np.dot(c, M[k, b]))
            else:
                f += (self.N / self.mbar.K) * (float(np.dot(c, M[k, b])) / self._n_kind[k])
        return f

    def _bspline_calculate_f(self, xi, b=0):
        """Minus the log likelihood (ml) or posterior (map) of the surface with coefficients (0, xi), replicate b
        (pymbar/fes.py:2102-2183): the data term from the moments, the partition functions by the reference's quadrature."""
        ent = self._spline_integrals(xi, need_pE=False)
        f = self._spline_data_dot(ent["bloc"].c, b)
        if self.spline_parameters["spline_weights"] == "unbiasedstate":
            f += self.N * np.log(ent["pF"])
        else:
            f += float(np.dot(self._spline_scaling(), np.log(ent["pF"])))
        logprior = self.spline_parameters["map_data"]["logprior"]
        if logprior is not None:
            f -= logprior(np.concatenate([[0], xi], axis=None))
        return float(f)

    def _bspline_calculate_g(self, xi, b=0):
        """Gradient of :meth:`_bspline_calculate_f` with respect to xi (pymbar/fes.py:2185-2298)."""
        ent = self._spline_integrals(xi, need_pE=True)
        M = self._spline_M
        w = self.spline_parameters["spline_weights"]
        if w == "unbiasedstate":
            g = self.N * M[0, b, 1:]
            g = g - self.N * ent["pE"]
        else:
            if w == "biasedstates":
                g = np.sum(M[:, b, 1:], axis=0)
            else:
                g = np.zeros(M.shape[2] - 1)
                for k in range(self.mbar.K):
                    g += (self.N / self.mbar.K) * (M[k, b, 1:] / self._n_kind[k])
            g = g - np.dot(ent["pE"], self._spline_scaling())
        dlogprior = self.spline_parameters["map_data"]["dlogprior"]
        if dlogprior is not None:
            g = g - dlogprior(np.concatenate([[0], xi], axis=None))
        return g

    def _bspline_calculate_h(self, xi, b=0):
        """Hessian of :meth:`_bspline_calculate_f` (pymbar/fes.py:2300-2414); it has no data term.  Self-contained: the
        averages it needs come from the cache of xi or are computed here."""
        from scipy.integrate import quad

        ent = self._spline_integrals(xi, need_pE=True)
        sp = self.spline_parameters
        nspline, kdegree = int(sp["nspline"]), int(sp["kdegree"])
        basis = self.spline_data["bspline_derivatives"]
        xrangeij = self.spline_data["xrangeij"]
        bloc, pF, pE = ent["bloc"], ent["pF"], ent["pE"]
        N = self.N
        if sp["spline_weights"] == "unbiasedstate":
            h = -N * np.outer(pE, pE)
            for i in range(nspline - 1):
                for j in range(0, i + 1):
                    if abs(i - j) <= kdegree:
                        q = quad(lambda x: basis[i + 1](x) * basis[j + 1](x) * np.exp(-bloc(x)), xrangeij[i + 1, j + 1, 0],
                                 xrangeij[i + 1, j + 1, 1])[0]
                        h[i, j] += N * q / pF
        else:
            fkbias = sp["fkbias"]
            scaling = self._spline_scaling()
            K = self.mbar.K
            h = np.zeros([nspline - 1, nspline - 1])
            for k in range(K):
                h += -scaling[k] * np.outer(pE[:, k], pE[:, k])
            for i in range(nspline - 1):
                for j in range(0, i + 1):
                    if abs(i - j) <= kdegree:
                        for k in range(K):
                            q = scaling[k] * quad(lambda x, k: basis[i + 1](x) * basis[j + 1](x) * np.exp(-bloc(x) - fkbias[k](x)),
                                                  xrangeij[i + 1, j + 1, 0], xrangeij[i + 1, j + 1, 1], args=(k,))[0]
                            h[i, j] += q / pF[k]
        for i in range(nspline - 1):
            for j in range(i + 1, nspline - 1):
                h[i, j] = h[j, i]
        ddlogprior = sp["map_data"]["ddlogprior"]
        if ddlogprior is not None:
            h = h - ddlogprior(np.concatenate([[0], xi], axis=None))
        return h

    def get_information_criteria(self, type="akaike"):
        """The Akaike or Bayesian information criterion of the fitted spline (pymbar/fes.py:1125-1166)."""
        if self.fes_type != "spline":
            raise ParameterError(f"Information criteria currently only defined for spline approaches, you are currently using {type}")
        if type in ("akaike", "Akaike", "AIC", "aic"):
            return self.spline_data["aic"]
        if type in ("bayesian", "Bayesian", "BIC", "bic"):
            return self.spline_data["bic"]
        raise ParameterError(f"Information criteria of type '{type}' not defined")

    def _get_fes_spline(self, x, reference_point, fes_reference, uncertainty_method):
        if x.shape[1] != 1:
            raise DataError("splines FES only supported in 1D")
        x = x[:, 0]
        f_i = self.fes_function(x)
        if reference_point == "from-lowest":
            fmin = np.min(f_i)
        elif reference_point == "from-specified":
            if fes_reference is None:
                raise ParameterError("Specified reference point for FES not given")
            fmin = float(self.fes_function(np.asarray(fes_reference, dtype=np.float64).reshape(-1)[0]))
        else:
            raise ParameterError(f"reference point {reference_point} not implemented for spline fes")
        f_i = f_i - fmin
        if uncertainty_method is None:
            df_i = None
        elif uncertainty_method == "bootstrap":
            if self.fes_functions is None:
                raise ParameterError("Cannot calculate via uncertainties error if bootstrapping was not performed running get_fes")
            fall = np.stack([fb(x) - fmin for fb in self.fes_functions], axis=-1)
            df_i = np.std(fall, axis=-1)
        else:
            raise ParameterError(f"Uncertainty method {uncertainty_method} for spline is not implemented")
        return {"f_i": f_i, "df_i": df_i}

    # ---- Monte Carlo over the spline coefficients (pymbar/fes.py:1690-2100) ------------------------------------------------
    def sample_parameter_distribution(self, x_n, mc_parameters=None, decorrelate=True, verbose=True):
        """Metropolis sampling of the normalised spline coefficients under the posterior of the fitted weighting
        (pymbar/fes.py:1690-1833): the same proposals, the same draws from the global stream in the same order, the same
        quadrature normalisation.  The likelihood's sums over x_n are moments computed once per call; the surface of
        ``get_fes`` is left as fitted (the chain's current spline is ``mc_data["bspline"]``)."""
        from scipy.integrate import quad
        from scipy.interpolate import BSpline

        from . import timeseries
        from .bspline import DeviceBSplineMoments

        if self.fes_type != "spline":
            raise ParameterError("Sampling of posterior is only supported for spline type")
        if self.spline_parameters is None:
            raise ParameterError("Must specify spline_parameters to sample the distributions")
        if self.fes_function is None:
            raise ParameterError("Need to generate an initial splined FES using generate_fes before performing MCMC sampling")
        sp = self.spline_parameters
        weights, xr = sp["spline_weights"], sp["xrange"]
        x_n = np.asarray(x_n, dtype=np.float64)
        if x_n.reshape(-1).shape != (self.N,):
            raise DataError("x_n must hold one 1-D coordinate per sample")
        mc = {} if mc_parameters is None else dict(mc_parameters)
        if mc_parameters is None:
            logger.info("Using default MC parameters")
        mc.setdefault("niterations", 5000)
        mc.setdefault("fraction_change", 0.01)
        mc.setdefault("sample_every", 50)
        mc.setdefault("print_every", 1000)
        mc.setdefault("logprior", lambda x: 0)
        niterations, sample_every = int(mc["niterations"]), int(mc["sample_every"])
        print_every, logprior = int(mc["print_every"]), mc["logprior"]

        base = self.fes_function
        t, kdeg = base.t, base.k
        norm = quad(lambda x: np.exp(-base(x)), xr[0], xr[1])[0]
        c = base.c + np.log(norm)
        self.mc_data = dict(original_spline=BSpline(t, c.copy(), kdeg), naccept=0)

        # the likelihood: the sums over x_n are c . moments (+ the bias sums of the biased weightings, fixed per call)
        K, N = self.mbar.K, self.N
        xk = np.asarray(self.mbar.x_kindices)
        if weights == "unbiasedstate":
            with DeviceBSplineMoments(x_n.reshape(-1)) as dev:
                dev.set_weights(self.w_n)
                m = dev.moments(t, kdeg)[0, 0]
        else:
            with DeviceBSplineMoments(x_n.reshape(-1), groups=xk, n_groups=K) as dev:
                Mk = dev.moments(t, kdeg)[:, 0]
            bias_sum = np.array([float(np.sum(sp["fkbias"][k](x_n[xk == k]))) for k in range(K)])
            n_k = np.bincount(xk, minlength=K)

        def loglikelihood(cc):
            spline = BSpline(t, cc, kdeg)
            if weights == "unbiasedstate":
                return N * float(np.dot(cc, m))
            ll = 0.0
            for k in range(K):
                lnZ = np.log(quad(lambda x, k: np.exp(-(spline(x) + sp["fkbias"][k](x))), xr[0], xr[1], args=(k,))[0])
                if weights == "simplesum":
                    ll += (N / K) * ((float(np.dot(cc, Mk[k])) + bias_sum[k]) / n_k[k])
                    ll += (N / K) * lnZ
                else:
                    ll += float(np.dot(cc, Mk[k])) + bias_sum[k]
                    ll += self.N_k[k] * lnZ
            return ll

        crange = np.max(c) - np.min(c)
        dc = mc["fraction_change"] * crange
        nsamples = (niterations + sample_every - 1) // sample_every
        csamples = np.zeros([len(c), nsamples])
        logposteriors = np.zeros(nsamples)
        current = loglikelihood(c) - logprior(c)
        for n in range(niterations):
            rchange = dc * np.random.normal()
            ci = np.random.randint(len(c))
            cnew = c.copy()
            cnew[ci] += rchange
            trial = BSpline(t, cnew, kdeg)
            cnew = cnew + np.log(quad(lambda x: np.exp(-trial(x)), xr[0], xr[1])[0])
            proposed = loglikelihood(cnew) - logprior(cnew)
            d = proposed - current
            if d <= 0 or np.random.random() < np.exp(-d):
                c, current = cnew, proposed
                self.mc_data["naccept"] += 1
            if n % sample_every == 0:
                csamples[:, n // sample_every] = c
                logposteriors[n // sample_every] = current
            if n % print_every == 0 and verbose:
                logger.info(f"MC Step {n} of {niterations}: log posterior {current}, coefficients {c}")
        if verbose:
            logger.info("Done MC sampling")
        t_mc, g_mc, g_c = 0, None, None
        if decorrelate:
            t_mc, g_mc, _ = timeseries.detect_equilibration(logposteriors)
            logger.info(f"First equilibration sample is {t_mc} of {len(logposteriors)}")
            equil = logposteriors[t_mc:]
            g_mc = timeseries.statistical_inefficiency(equil)
            if verbose:
                logger.info(f"Statistical inefficiency of log posterior is {g_mc:.3g}")
            g_c = np.array([timeseries.statistical_inefficiency(csamples[i, t_mc:]) for i in range(len(c))])
            if verbose:
                logger.info(f"Time series for spline parameters are : {g_c}")
            indices = timeseries.subsample_correlated_data(equil, g=g_mc)
            logposteriors = equil[indices]
            csamples = csamples[:, t_mc:][:, indices]
            if verbose:
                logger.info(f"samples after decorrelation : {csamples.shape[1]}")
        self.mc_data.update(bspline=BSpline(t, c, kdeg), samples=csamples, logposteriors=logposteriors, mc_parameters=mc,
                            acceptance_ratio=self.mc_data["naccept"] / niterations, nequil=t_mc, g_logposterior=g_mc,
                            g_parameters=g_c, g=g_mc)
        if verbose:
            logger.info(f"Acceptance rate : {self.mc_data['acceptance_ratio']:5.3f}")

    def get_confidence_intervals(self, xplot, plow, phigh, reference="zero"):
        """Percentiles of the sampled surfaces at xplot (pymbar/fes.py:1835-1902)."""
        from scipy.interpolate import BSpline

        if self.mc_data is None:
            raise DataError("No MC sampling has been done, cannot construct confidence intervals")
        xplot = np.asarray(xplot, dtype=np.float64)
        base = self.mc_data["original_spline"]
        csamples = self.mc_data["samples"]
        yvals = base(xplot)
        samplevals = np.stack([BSpline(base.t, csamples[:, n], base.k)(xplot) for n in range(csamples.shape[1])], axis=-1)
        if reference == "zero":
            ref = np.min(yvals)
        elif reference is None:
            ref = 0
        else:
            raise ParameterError(f"{reference} is not a valid value for 'reference'")
        return dict(plow=np.percentile(samplevals, plow, axis=-1) - ref, phigh=np.percentile(samplevals, phigh, axis=-1) - ref,
                    median=np.percentile(samplevals, 50, axis=-1) - ref, values=yvals - ref)

    def get_mc_data(self):
        """The Monte Carlo results of :meth:`sample_parameter_distribution` (pymbar/fes.py:1904-1929)."""
        if self.mc_data is None:
            raise DataError("No MC sampling has been done, cannot construct confidence intervals")
        return self.mc_data

    # ---- accessors --------------------------------------------------------------------------------------------------------
    def get_mbar(self):
        if self.mbar is not None:
            return self.mbar
        raise DataError("MBAR in the FES object is not initialized, cannot return it.")

    def get_kde(self):
        if self.fes_type == "kde":
            if self.kde is not None:
                return self.kde
            raise ParameterError("Can't return the KernelDensity object because kde not yet defined")
        raise ParameterError("Can't return the KernelDensity object because fes_type != kde")
