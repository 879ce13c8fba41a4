"""Golden fixture for kernel-density surfaces along a scan (MBAR.compute_scan_kde), generated from the UNMODIFIED reference
(fes_type="kde", pymbar/fes.py:602-699, 1523-1609, on sklearn 0.24.2):

    PYTHONPATH=/root/reference /opt/conda/bin/python3.9 tests/golden/make_golden_scan_kde.py

(1) 1-D: config 1 (config1_ho_K5_N5000.npz; its u_kn is reused and asserted equal, x_n is regenerated from seed 0).  The family is
    L = 12 harmonic oscillators (O_l in 0.5 .. 3.5, K_l in 1, 2, 4) on a 4 x 3 grid inside the hull of the five sampled ones, in the basis {x^2, x} of
    pymbar_amd.testsystems.harmonic_scan_family; 40 queries from just below the lowest sample to just above the highest one,
    bandwidth 0.2.  For every member FES.generate_fes(u_n=u_l, x_n, fes_type="kde", kde_parameters={"bandwidth": h}) and get_fes at
    the three reference points (from-specified at x = 1.0), and the EXACT log density at the queries and at x = 1.0 from the
    reference's own weights w_n, by logsumexp over every sample: where the density of a member is negligible (f_i beyond ~30) the tree
    sum of sklearn 0.24.2 is inexact in 1-D too, and the tests hold the reference's f_i only where it agrees with its own exact sum.
(2) 2-D: the umbrella system of fes_kde.npz (b) (its samples, u_n and umbrella centres are reused, not stored again), linear over
    [u_n, x^2 + y^2, x, y] (pymbar_amd.testsystems.umbrella_2d_family).  Members: five temperatures beta' u_n and two of the sampled
    umbrellas.  For every member the reference's own weights w_n after generate_fes(u_n=u_l), and from them the EXACT log density at
    the fixture's queries and at (0, 0) by logsumexp over every sample, as make_golden_fes_kde.py: exact_log_density does (sklearn's
    tree sum is inexact in 2-D), next to what score_samples returns.
Only data is stored.  (This docstring is the fixture's description: like the other scan fixtures it has no entry in MANIFEST.json,
which stays as it is.)"""
import importlib.util
import logging
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
logging.disable(logging.WARNING)
import pymbar  # noqa: E402
from pymbar import FES  # noqa: E402

assert os.path.realpath(pymbar.__file__).startswith("/root/reference"), pymbar.__file__
import sklearn  # noqa: E402
from scipy.special import logsumexp  # noqa: E402

spec = importlib.util.spec_from_file_location("ts", os.path.join(ROOT, "pymbar_amd", "testsystems.py"))
ts = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ts)


def exact_log_density(x_n, w, q, h):
    d = x_n.shape[1]
    r2 = ((q[:, None, :] - x_n[None, :, :]) ** 2).sum(axis=2)
    return logsumexp(-0.5 * r2 / h ** 2, b=w[None, :], axis=1) - np.log(w.sum()) - 0.5 * d * np.log(2 * np.pi) - d * np.log(h)


def part_1(out):
    g = np.load(os.path.join(HERE, "config1_ho_K5_N5000.npz"))
    x_n, u_kn, N_k, _, O_k, K_k = ts.config1(seed=0)
    assert np.array_equal(u_kn, g["u_kn"]) and np.array_equal(N_k, g["N_k"])
    O = np.linspace(0.5, 3.5, 4)
    Kf = np.array([1.0, 2.0, 4.0])
    O_l, K_l = [a.ravel() for a in np.meshgrid(O, Kf, indexing="ij")]
    basis, coeff, offset = ts.harmonic_scan_family(x_n, O_l, K_l)
    u_ln = coeff @ basis + offset[:, None]
    h = 0.2
    q = np.linspace(x_n.min() - 0.5, x_n.max() + 0.5, 40)
    fes = FES(u_kn, N_k, mbar_options=dict(relative_tolerance=1e-12))
    f_low, f_spec, f_norm, exact = [], [], [], []
    qq = np.append(q, 1.0).reshape(-1, 1)
    for u_l in u_ln:
        fes.generate_fes(u_l, x_n.reshape(-1, 1), fes_type="kde", kde_parameters={"bandwidth": h})
        exact.append(exact_log_density(x_n.reshape(-1, 1), fes.w_n, qq, h))
        f_low.append(fes.get_fes(q.reshape(-1, 1), reference_point="from-lowest", uncertainty_method=None)["f_i"])
        f_spec.append(fes.get_fes(q.reshape(-1, 1), reference_point="from-specified", fes_reference=[1.0], uncertainty_method=None)["f_i"])
        f_norm.append(fes.get_fes(q.reshape(-1, 1), reference_point="from-normalization", uncertainty_method=None)["f_i"])
    out.update(a_f_k=fes.mbar.f_k, a_O_l=O_l, a_K_l=K_l, a_coeff=coeff, a_offset=offset, a_bandwidth=h, a_queries=q, a_fes_reference=1.0,
               a_f_lowest=np.array(f_low), a_f_specified=np.array(f_spec), a_f_normalization=np.array(f_norm), a_exact_L=np.array(exact))
    print("1-D: exact vs tree, max |dL| =", np.max(np.abs(out["a_exact_L"][:, :-1] + out["a_f_normalization"])))
    assert all(np.all(np.isfinite(out[k])) for k in ("a_f_lowest", "a_f_specified", "a_f_normalization"))


def part_2(out):
    g = np.load(os.path.join(HERE, "fes_kde.npz"))
    x_n, u_n, N_k, xu, Ku, h, q = g["b_x_n"], g["b_u_n"], g["b_N_k"], g["b_umbrella_centers"], float(g["b_Ku"]), float(g["b_bandwidth"]), g["b_queries"]
    basis, coeff_k, offset_k = ts.umbrella_2d_family(x_n, u_n, xu, Ku)
    u_kn = coeff_k @ basis + offset_k[:, None]
    assert np.allclose(u_kn, np.array([u_n + (Ku / 2) * np.sum((x_n - xu[k]) ** 2, axis=1) for k in range(len(xu))]), rtol=1e-12, atol=1e-10)
    betas = np.array([0.8, 0.9, 1.0, 1.1, 1.25])
    sampled = np.array([24, 10])
    coeff = np.vstack([np.stack([betas, 0 * betas, 0 * betas, 0 * betas], axis=1), coeff_k[sampled]])
    offset = np.concatenate([np.zeros(len(betas)), offset_k[sampled]])
    u_ln = coeff @ basis + offset[:, None]
    qq = np.vstack([q, [[0.0, 0.0]]])
    fes = FES(u_kn, N_k, mbar_options=dict(relative_tolerance=1e-12))
    exact, ref = [], []
    for u_l in u_ln:
        fes.generate_fes(u_l, x_n, fes_type="kde", kde_parameters={"bandwidth": h})
        exact.append(exact_log_density(x_n, fes.w_n, qq, h))
        ref.append(fes.kde.score_samples(qq))
    out.update(b_f_k=fes.mbar.f_k, b_coeff=coeff, b_offset=offset, b_betas=betas, b_sampled=sampled, b_exact_L=np.array(exact),
               b_ref_L=np.array(ref))
    print("2-D: exact vs tree, max |dL| =", np.max(np.abs(out["b_exact_L"] - out["b_ref_L"])))


def main():
    out = {}
    part_1(out)
    part_2(out)
    out["sklearn_version"] = np.array(sklearn.__version__)
    np.savez_compressed(os.path.join(HERE, "scan_kde_ho_K5.npz"), **out)


if __name__ == "__main__":
    main()
