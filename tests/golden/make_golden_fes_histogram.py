"""Golden fixture for histogram free energy surfaces with bootstrap uncertainties and on a 2-D grid of more than 200 bins,
generated from the UNMODIFIED reference (fes_type="histogram", pymbar/fes.py:388-424, 500-600, 1340-1480):

    PYTHONPATH=/root/reference /opt/conda/bin/python3.9 tests/golden/make_golden_fes_histogram.py

(a) the 1-D umbrella system of fes_umbrella_1d.npz (its arrays are reused, not stored again), n_bootstraps = 4, seed 10: each
    replicate's bootstrap indices (the global stream replayed: per state the indices, then the one int32 each per-state MBAR
    construction draws; asserted to reproduce the reference's own replicate surfaces), each replicate's h["f"], the same bin free
    energies from pymbar.MBAR(u_kn[:, idx], N_k, relative_tolerance=1e-12) ("tight"; the reference's replicates are solved to
    its default 1e-7), the measured max |loose - tight| as a_loose_gap, and get_fes at the centres of the populated grid bins,
    from-lowest and from-specified (0.0), with uncertainty_method="bootstrap".
(b) the reference's fes_2d system (tests/test_fes.py:190-300: 7 x 7 umbrellas x 300 samples, np.random.seed(4321): the samples
    of fes_kde.npz part (b), asserted equal and not stored again) on a 20 x 20 grid, so that K + nbins > 256: f, the sample
    labels, grid_of_label, and get_fes at the centres (+ delta) of the populated grid bins (for any other the reference raises
    KeyError), from-lowest and from-specified ([0, 0]), with uncertainty_method="analytical".
Only data is stored."""
import logging
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
logging.disable(logging.WARNING)
import pymbar  # noqa: E402
from pymbar import FES  # noqa: E402

assert os.path.realpath(pymbar.__file__).startswith("/root/reference"), pymbar.__file__
from scipy.special import logsumexp  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(pymbar.__file__), "tests"))
from test_fes import generate_fes_data  # noqa: E402


def bin_free_energies(mbar, u_n, labels, nbins):
    log_w = mbar._computeUnnormalizedLogWeights(u_n)
    return np.array([-logsumexp(log_w[labels == i]) for i in range(nbins)])


def part_a(out):
    g = np.load(os.path.join(HERE, "fes_umbrella_1d.npz"))
    u_kn, N_k, u_n, x_n, edges, labels = g["u_kn"], g["N_k"], g["u_n"], g["x_n"], g["bin_edges"], g["sample_label"]
    K, N, nbins = len(N_k), int(N_k.sum()), int(labels.max()) + 1
    B, seed = 4, 10
    fes = FES(u_kn, N_k)
    fes.generate_fes(u_n, x_n, fes_type="histogram", histogram_parameters={"bin_edges": edges}, n_bootstraps=B, seed=seed)
    assert np.allclose(fes.histogram_data["f"], g["f_raw"], rtol=0, atol=1e-12)
    ref_f = np.array([h["f"] for h in fes.histogram_datas])
    assert ref_f.shape == (B, nbins)  # (every replicate populates every bin)
    # the replicates' indices: the stream of generate_fes replayed
    np.random.seed(seed)
    idx_all = []
    idx = np.arange(N)
    for _ in range(B):
        index = 0
        for k in range(K):
            idx[index:index + N_k[k]] = index + np.random.randint(0, N_k[k], size=N_k[k])
            index += N_k[k]
            np.random.randint(np.iinfo(np.int32).max)
        idx_all.append(idx.copy())
    loose_f, tight_f, tight_fk = [], [], []
    for b in range(B):
        i = idx_all[b]
        loose = pymbar.MBAR(u_kn[:, i], N_k, initial_f_k=fes.mbar.f_k)
        loose_f.append(bin_free_energies(loose, u_n[i], labels[i], nbins))
        tight = pymbar.MBAR(u_kn[:, i], N_k, relative_tolerance=1e-12)
        tight_f.append(bin_free_energies(tight, u_n[i], labels[i], nbins))
        tight_fk.append(tight.f_k)
    replay = float(np.max(np.abs(np.array(loose_f) - ref_f)))
    assert replay < 1e-12, replay  # the replayed indices ARE the reference's
    centers = 0.5 * (edges[1:] + edges[:-1])
    grid = g["grid_of_label"]
    q = centers[grid[(grid >= 0) & (grid < len(centers))]]
    lo = fes.get_fes(q, reference_point="from-lowest", uncertainty_method="bootstrap")
    sp = fes.get_fes(q, reference_point="from-specified", fes_reference=0.0, uncertainty_method="bootstrap")
    out.update(a_seed=np.int64(seed), a_n_bootstraps=np.int64(B), a_idx=np.array(idx_all, dtype=np.int32), a_ref_f=ref_f,
               a_tight_f=np.array(tight_f), a_tight_f_k=np.array(tight_fk),
               a_loose_gap=np.float64(np.max(np.abs(ref_f - np.array(tight_f)))), a_queries=q,
               a_f_lowest=lo["f_i"], a_df_lowest=lo["df_i"], a_f_specified=sp["f_i"], a_df_specified=sp["df_i"])
    print("a: replay vs reference", replay, " loose gap", out["a_loose_gap"])


def part_b(out):
    np.random.seed(4321)
    gridscale, nbinsperdim, K0, Ku, nsamples, delta = 0.2, 20, 20.0, 100, 300, 0.0001
    xrange = [[-3, 3], [-3, 3]]
    u_kn, u_n, x_n, _, _, _ = generate_fes_data(K0=K0, Ku=Ku, ndim=2, nsamples=nsamples, gridscale=gridscale, xrange=xrange)
    kde = np.load(os.path.join(HERE, "fes_kde.npz"))
    assert np.array_equal(kde["b_x_n"], x_n) and np.array_equal(kde["b_u_n"], u_n)  # (the same samples: not stored again)
    xu = kde["b_umbrella_centers"]
    rebuilt = np.array([u_n + 1.0 * (Ku / 2) * np.sum((x_n - xu[k]) ** 2, axis=1) for k in range(len(xu))])
    assert np.array_equal(rebuilt, u_kn)
    N_k = nsamples * np.ones(u_kn.shape[0], int)
    xmin, xmax = gridscale * (xrange[0][0] - 0.5), gridscale * (xrange[0][1] + 0.5)
    ymin, ymax = gridscale * (xrange[1][0] - 0.5), gridscale * (xrange[1][1] + 0.5)
    dx, dy = (xmax - xmin) / nbinsperdim, (ymax - ymin) / nbinsperdim
    edges = [np.linspace(xmin, xmax, nbinsperdim + 1), np.linspace(ymin, ymax, nbinsperdim + 1)]
    centers = np.array([[xmin + dx * (i + 0.5), ymin + dy * (j + 0.5)] for i in range(nbinsperdim) for j in range(nbinsperdim)])
    q = centers + delta
    fes = FES(u_kn, N_k)
    fes.generate_fes(u_n, x_n, fes_type="histogram", histogram_parameters={"bin_edges": edges})
    hd = fes.histogram_data
    order = hd["bin_order"]
    # (the reference sizes f by its distinct grid CELLS, but all cells left of the grid in some dimension share the label -1
    # and one free energy: the entries behind the distinct labels are never written)
    nbins = len(order)
    assert np.all(hd["f"][nbins:] == 0)
    assert u_kn.shape[0] + nbins > 256, nbins
    labels = np.array([order[v] for v in hd["sample_label"]], dtype=np.int16)  # bins numbered in order of first appearance
    grid_of_label = np.full((nbins, 2), -1, dtype=np.int16)
    for cell, v in hd["bin_label"].items():
        if v >= 0:
            grid_of_label[order[v]] = cell
    # (the reference raises KeyError for a query in a grid bin without samples: only the populated ones are asked for)
    cells = np.array([np.digitize(q[:, d], edges[d]) - 1 for d in range(2)]).T
    q = q[[tuple(c) in hd["bin_label"] for c in cells]]
    lo = fes.get_fes(q, reference_point="from-lowest", uncertainty_method="analytical")
    sp = fes.get_fes(q, reference_point="from-specified", fes_reference=[0, 0], uncertainty_method="analytical")
    out.update(b_grid=np.int64(nbinsperdim), b_edges_x=edges[0], b_edges_y=edges[1], b_Ku=float(Ku), b_N_k=N_k, b_f_k=fes.mbar.f_k,
               b_f=hd["f"][:nbins], b_sample_label=labels, b_grid_of_label=grid_of_label, b_queries=q, b_f_lowest=lo["f_i"],
               b_df_lowest=lo["df_i"], b_f_specified=sp["f_i"], b_df_specified=sp["df_i"])
    print("b: grid", nbinsperdim, "queries", len(q), "populated bins", nbins, "K + nbins", u_kn.shape[0] + nbins)


def main():
    out = {}
    part_a(out)
    part_b(out)
    np.savez_compressed(os.path.join(HERE, "fes_histogram.npz"), **out)


if __name__ == "__main__":
    main()
