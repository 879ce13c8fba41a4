"""Golden fixture for kernel-density free energy surfaces, generated from the UNMODIFIED reference (fes_type="kde",
pymbar/fes.py:602-699, 1523-1609, on sklearn 0.24.2):

    PYTHONPATH=/root/reference /opt/conda/bin/python3.9 tests/golden/make_golden_fes_kde.py

(a) the 1-D umbrella system of fes_umbrella_1d.npz (its arrays are reused, not stored again), bandwidth 0.5 dx as in the
    reference's tests/test_fes.py:343-360, n_bootstraps = 10, seed 10: get_fes at the 15 bin centres and on a 200-point grid
    for the three reference points (bootstrap df_i for from-lowest / from-specified), and replicate 1's bootstrap indices.
(b) the reference's fes_2d system (tests/test_fes.py:190-300: 7 x 7 umbrellas x 300 samples, np.random.seed(4321) here),
    n_bootstraps = 4, seed 11, queries at bin_centers + delta: the reference's answers, each replicate's score_samples, and the
    exact log densities (scipy.special.logsumexp over every sample) of the same weights.
(c) sklearn's score_samples for all six kernels in 1-D on two small weighted sets (integer data with queries at exactly |r| = h,
    and real data), where the tree sum is exact.
Only data is stored; the samples of (b) are stored and its u_kn is rebuilt from them by the formula of the generator."""
import logging
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
logging.disable(logging.WARNING)
import pymbar  # noqa: E402
from pymbar import FES  # noqa: E402

assert os.path.realpath(pymbar.__file__).startswith("/root/reference"), pymbar.__file__
import sklearn  # noqa: E402
from scipy.special import logsumexp  # noqa: E402
from sklearn.neighbors import KernelDensity  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(pymbar.__file__), "tests"))
from test_fes import generate_fes_data  # noqa: E402

KERNELS = ["gaussian", "tophat", "epanechnikov", "exponential", "linear", "cosine"]


def replicate_indices(kde_b, x_n):
    """The bootstrap indices a replicate was fit on, recovered from the positions it holds (all samples are distinct)."""
    pos = {tuple(r): i for i, r in enumerate(x_n)}
    data = np.asarray(kde_b.tree_.data)
    return np.array([pos[tuple(r)] for r in data], dtype=np.int64)


def exact_log_density(x_n, w, q, h):
    d = x_n.shape[1]
    r2 = ((q[:, None, :] - x_n[None, :, :]) ** 2).sum(axis=2)
    return logsumexp(-0.5 * r2 / h ** 2, b=w[None, :], axis=1) - np.log(w.sum()) - 0.5 * d * np.log(2 * np.pi) - d * np.log(h)


def part_a(out):
    g = np.load(os.path.join(HERE, "fes_umbrella_1d.npz"))
    u_kn, N_k, u_n, x_n, edges = g["u_kn"], g["N_k"], g["u_n"], g["x_n"], g["bin_edges"]
    dx = edges[1] - edges[0]
    centers = 0.5 * (edges[1:] + edges[:-1])
    grid = np.linspace(edges[0] - 3 * dx, edges[-1] + 3 * dx, 200)
    fes = FES(u_kn, N_k)
    fes.generate_fes(u_n, x_n, fes_type="kde", kde_parameters={"bandwidth": 0.5 * dx}, n_bootstraps=10, seed=10)
    out["a_bandwidth"] = 0.5 * dx
    out["a_seed"] = np.int64(10)
    out["a_n_bootstraps"] = np.int64(10)
    out["a_w_n"] = fes.w_n
    out["a_idx1"] = replicate_indices(fes.kdes[0], x_n)
    out["a_centers"] = centers
    out["a_grid"] = grid
    for name, q in (("centers", centers), ("grid", grid)):
        lo = fes.get_fes(q, reference_point="from-lowest", uncertainty_method="bootstrap")
        sp = fes.get_fes(q, reference_point="from-specified", fes_reference=0.0, uncertainty_method="bootstrap")
        nz = fes.get_fes(q, reference_point="from-normalization", uncertainty_method=None)
        out[f"a_{name}_f_lowest"], out[f"a_{name}_df_lowest"] = lo["f_i"], lo["df_i"]
        out[f"a_{name}_f_specified"], out[f"a_{name}_df_specified"] = sp["f_i"], sp["df_i"]
        out[f"a_{name}_f_normalization"] = nz["f_i"]


def part_b(out):
    np.random.seed(4321)
    gridscale, nbinsperdim, K0, Ku, nsamples, delta = 0.2, 10, 20.0, 100, 300, 0.0001
    xrange = [[-3, 3], [-3, 3]]
    u_kn, u_n, x_n, _, _, _ = generate_fes_data(K0=K0, Ku=Ku, ndim=2, nsamples=nsamples, gridscale=gridscale, xrange=xrange)
    N_k = nsamples * np.ones(u_kn.shape[0], int)
    xmin, xmax = gridscale * (xrange[0][0] - 0.5), gridscale * (xrange[0][1] + 0.5)
    ymin, ymax = gridscale * (xrange[1][0] - 0.5), gridscale * (xrange[1][1] + 0.5)
    dx, dy = (xmax - xmin) / nbinsperdim, (ymax - ymin) / nbinsperdim
    centers = np.array([[xmin + dx * (i + 0.5), ymin + dy * (j + 0.5)] for i in range(nbinsperdim) for j in range(nbinsperdim)])
    q = centers + delta
    # the umbrella centres of the generator (its enumeration: dimension 0 fastest)
    nper = xrange[0][1] - xrange[0][0] + 1
    xu = np.array([[gridscale * ((i // 1) % nper + xrange[0][0]), gridscale * ((i // nper) % nper + xrange[1][0])]
                   for i in range(nper * nper)])
    rebuilt = np.array([u_n + 1.0 * (Ku / 2) * np.sum((x_n - xu[k]) ** 2, axis=1) for k in range(len(xu))])
    assert np.array_equal(rebuilt, u_kn)
    h = 0.5 * dx
    fes = FES(u_kn, N_k)
    fes.generate_fes(u_n, x_n, fes_type="kde", kde_parameters={"bandwidth": h}, n_bootstraps=4, seed=11)
    lo = fes.get_fes(q, reference_point="from-lowest", uncertainty_method="bootstrap")
    sp = fes.get_fes(q, reference_point="from-specified", fes_reference=[0, 0], uncertainty_method="bootstrap")
    nz = fes.get_fes(q, reference_point="from-normalization", uncertainty_method=None)
    qq = np.vstack([q, [[0.0, 0.0]]])
    ref_L = [fes.kde.score_samples(qq)]
    exact_L = [exact_log_density(x_n, fes.w_n, qq, h)]
    idx = []
    for kb in fes.kdes:
        i = replicate_indices(kb, x_n)
        idx.append(i)
        ref_L.append(kb.score_samples(qq))
        exact_L.append(exact_log_density(x_n, np.bincount(i, weights=fes.w_n, minlength=len(x_n)), qq, h))
    out.update(b_x_n=x_n, b_u_n=u_n, b_N_k=N_k, b_umbrella_centers=xu, b_K0=K0, b_Ku=float(Ku), b_beta=1.0, b_bandwidth=h,
               b_seed=np.int64(11), b_n_bootstraps=np.int64(4), b_queries=q, b_w_n=fes.w_n, b_f_k=fes.mbar.f_k,
               b_f_lowest=lo["f_i"], b_df_lowest=lo["df_i"], b_f_specified=sp["f_i"], b_df_specified=sp["df_i"],
               b_f_normalization=nz["f_i"], b_ref_L=np.array(ref_L).T, b_exact_L=np.array(exact_L).T,
               b_idx=np.array(idx, dtype=np.int32))


def part_c(out):
    rng = np.random.RandomState(5)
    xi = rng.randint(0, 20, size=40).astype(float)[:, None]
    wi = rng.uniform(0.1, 2.0, size=40)
    qi = np.arange(-4.0, 24.5, 0.5)[:, None]
    xr = rng.normal(0.0, 1.0, size=60)[:, None]
    wr = rng.uniform(0.05, 1.0, size=60)
    qr = np.linspace(-4.0, 4.0, 81)[:, None]
    out.update(c_kernels=np.array(KERNELS), c_int_x=xi, c_int_w=wi, c_int_q=qi, c_int_h=2.0, c_real_x=xr, c_real_w=wr, c_real_q=qr,
               c_real_h=0.7)
    for k in KERNELS:
        out[f"c_int_{k}"] = KernelDensity(kernel=k, bandwidth=2.0).fit(xi, sample_weight=wi).score_samples(qi)
        out[f"c_real_{k}"] = KernelDensity(kernel=k, bandwidth=0.7).fit(xr, sample_weight=wr).score_samples(qr)


def main():
    out = {}
    part_a(out)
    part_b(out)
    part_c(out)
    out["sklearn_version"] = np.array(sklearn.__version__)
    np.savez_compressed(os.path.join(HERE, "fes_kde.npz"), **out)
    print("b: exact vs reference, max |dL| =", np.nanmax(np.abs(out["b_exact_L"] - out["b_ref_L"])))


if __name__ == "__main__":
    main()
