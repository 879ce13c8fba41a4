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
surfaces, whose sums run in ``pymbar_amd.kde`` (its own device path, not the K x N matrix); spline surfaces and the Monte Carlo
sampler of the reference are not provided.
"""
import logging

import numpy as np

from .utils import DataError, ParameterError

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
    from .device import DeviceMatrix
    from .expectations import _augmented_solve

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

    dm = DeviceMatrix.empty(K + nbins, N, device=getattr(mbar, "_device", None))
    try:
        dm.copy_rows_from(mbar._dm, 0, 0, K)
        dm.fill_masked_rows(K, nbins, u_n, sample_label)  # one "state" per bin: u_n on its samples, +inf elsewhere
        N_aug = np.zeros(K + nbins, dtype=np.float64)
        N_aug[:K] = mbar.N_k
        dm.set_Nk(N_aug)
        f_full, _ = _augmented_solve(dm, K, nbins, mbar.f_k)
        f_raw = f_full[K:].copy()  # = -logsumexp(log_w_n[bin])   (fes.py:585)
        if reference == "from-lowest":
            j = int(np.argmin(f_raw))
        elif reference == "from-specified":
            if reference_label is None or not (0 <= int(reference_label) < nbins):
                raise ParameterError("Specified reference point for FES not given")
            j = int(reference_label)
        else:
            raise ParameterError(f"reference point method {reference} is not supported for histogram surfaces here")
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


_NOT_HERE = "not supported on this backend"


class FES:
    """``pymbar.FES`` on the MI355X path (pymbar/fes.py:74-1609): the MBAR solve on the device, histogram surfaces through
    :func:`label_samples` / :func:`histogram_fes`, kernel-density surfaces through :class:`pymbar_amd.kde.KernelDensity`.

    Supported: ``fes_type="histogram"`` (``get_fes`` from-lowest / from-specified, uncertainties None or "analytical") and
    ``fes_type="kde"`` (from-lowest / from-specified / from-normalization, uncertainties None or "bootstrap").  Spline surfaces,
    histogram bootstraps and the histogram from-normalization / all-differences modes raise ``ParameterError``.  The deliberate
    differences from the reference are listed in INTEGRATION.md ("FES")."""

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
        if self.verbose:
            logger.info("FES initialized")

    # ---- generate ---------------------------------------------------------------------------------------------------------
    def generate_fes(self, u_n, x_n, fes_type="histogram", histogram_parameters=None, kde_parameters=None,
                     spline_parameters=None, n_bootstraps=0, seed=-1):
        """Build the surface (pymbar/fes.py:221-438).  kde: the replicates of ``n_bootstraps > 0`` draw from the global NumPy
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
            if n_bootstraps > 0:
                raise ParameterError(f"histogram surfaces with n_bootstraps > 0 are {_NOT_HERE}")
            self._generate_histogram(x_n, histogram_parameters)
        elif fes_type == "kde":
            self._generate_kde(x_n, kde_parameters, n_bootstraps)
        elif fes_type == "spline":
            raise ParameterError(f"fes_type 'spline' is {_NOT_HERE}")
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
            index = 0
            for k in range(self.mbar.K):
                idx[index:index + N_k[k]] = index + np.random.randint(0, N_k[k], size=N_k[k])
                index += N_k[k]
                np.random.randint(np.iinfo(np.int32).max)  # (the rseed draw of the skipped MBAR construction)
            cols[:, b] = np.bincount(idx, weights=self.w_n, minlength=self.N)
        self.bootstrap_weights = cols
        self.kdes = None  # (the replicates are the columns 1..B of bootstrap_weights, evaluated in one device pass)

    @property
    def w_kn(self):
        """``exp(mbar.Log_W_nk)`` (fes.py:413): built on first access only."""
        if getattr(self, "_w_kn", None) is None:
            self._w_kn = np.exp(self.mbar.Log_W_nk)
        return self._w_kn

    def _generate_histogram(self, x_n, histogram_parameters):
        if histogram_parameters is None or "bin_edges" not in histogram_parameters:
            raise ParameterError("histogram_parameters['bin_edges'] cannot be undefined with fes_type = histogram")
        bins = histogram_parameters["bin_edges"]
        if np.ndim(bins[0]) == 0:
            bins = [bins]
        bins = [np.asarray(b, dtype=np.float64) for b in bins]
        self.histogram_parameters = dict(histogram_parameters, bin_edges=bins)
        if x_n.shape != (self.N, len(bins)):
            raise DataError("x_n and bin_edges have inconsistent dimension")
        self.w_n = self._normalized_weights()
        self._w_kn = None
        labels, grid = label_samples(x_n, bins)
        raw = histogram_fes(self.mbar, self.u_n, labels, uncertainty_method=None)
        # bins are numbered in order of first appearance like the reference's bin_order (fes.py:552-560); grid_of_label[i] is
        # the tuple of grid indices of bin i (None: the bin of the samples left of the grid)
        self.histogram_data = dict(bins=bins, dims=len(bins), f=raw["f_raw"], sample_label=labels, grid_of_label=grid,
                                   label_of_grid={g: i for i, g in enumerate(grid) if g is not None})

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
        if uncertainty_method == "bootstrap":
            raise ParameterError(f"bootstrap uncertainties of histogram surfaces are {_NOT_HERE}")
        if uncertainty_method not in (None, "analytical"):
            raise ParameterError(f"Uncertainty_method {uncertainty_method} is not a valid option")
        if reference_point in ("from-normalization", "all-differences"):
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
        res = histogram_fes(self.mbar, self.u_n, hd["sample_label"], reference=reference_point, reference_label=ref_label,
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
