"""Golden fixture for spline free energy surfaces, generated from the UNMODIFIED reference (fes_type="spline",
pymbar/fes.py:701-1166, 1611-2477, on scipy 1.7):

    PYTHONPATH=/root/reference /opt/conda/bin/python3.9 tests/golden/make_golden_fes_spline.py

The system is the 1-D umbrella system of fes_umbrella_1d.npz (its arrays are reused, not stored again); the bias centres and
Ku are stored so that the tests rebuild the same fkbias callables, fkbias[k](x) = (Ku / 2) (x - centre_k)^2.  Cases:
(a)  unbiasedstate / Newton-CG / explicit init (the reference's own test: nspline 4, xinit the bin centres, yinit K0 x^2 / 2);
(b)  biasedstates / BFGS / zeros;
(c)  simplesum / L-BFGS-B / bias_free_energies with bias_centers (K < 2 nspline: the coarse least-squares branch);
(c2) biasedstates / Newton-CG / bias_free_energies with bias_centers, K >= 2 nspline (the centres themselves);
(c3) unbiasedstate / CG / bias_free_energies without bias_centers;
(c4) unbiasedstate / TNC / zeros;  (c5) unbiasedstate / SLSQP / zeros;
(d)  unbiasedstate / Newton-CG / map with a Gaussian smoothness prior (sigma stored);
(e)  n_bootstraps = 2, seeded, for unbiasedstate (e_u) and biasedstates (e_b): the replicate surfaces, bootstrap df_i, and each
     unbiasedstate replicate's f_b re-solved to 1e-12 (the reference's FES solves them to its default 1e-7);
(f)  a seeded 300-step MC (sample_every 10, decorrelate) on the fits of (a) and (b): samples, log posteriors, acceptance
     ratio, nequil, g values and get_confidence_intervals(5, 95).
For each fit: fes_function.c, get_fes on a grid (from-lowest; (a) also from-specified), AIC and BIC -- taken before any MC,
which mutates the reference's fes_function in place."""
import logging
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
logging.disable(logging.WARNING)
import pymbar  # noqa: E402
from pymbar import FES  # noqa: E402

assert os.path.realpath(pymbar.__file__).startswith("/root/reference"), pymbar.__file__

K0, KU, SIGMA = 20.0, 100.0, 2.0


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


def main():
    u = np.load(os.path.join(HERE, "fes_umbrella_1d.npz"))
    u_kn, N_k, u_n, x_n, edges = u["u_kn"], u["N_k"], u["u_n"], u["x_n"], u["bin_edges"]
    centers_b = 0.2 * np.arange(-3, 4, dtype=float)  # (make_golden_fes.py)
    xrange = [float(edges[0]), float(edges[-1])]
    bin_centers = 0.5 * (edges[1:] + edges[:-1])
    grid = np.linspace(xrange[0] - 0.1, xrange[1] + 0.1, 101)
    fk = fkbias_list(centers_b, KU)
    out = dict(bias_centers=centers_b, Ku=np.float64(KU), K0=np.float64(K0), sigma=np.float64(SIGMA),
               xrange=np.array(xrange), grid=grid, bin_centers=bin_centers)

    def params(weights, nspline, kdegree, algo, init, opts, **extra):
        p = dict(spline_weights=weights, nspline=nspline, kdegree=kdegree, xrange=list(xrange), optimization_algorithm=algo,
                 spline_initialize=init, optimize_options=dict(opts), fkbias=fk, objective="ml", map_data=None)
        p.update(extra)
        return p

    lp, dlp, ddlp = gaussian_prior(SIGMA)
    # (the reference completes the caller's dict in place -- map_data among others -- so every fit gets a fresh one)
    cases = lambda: {
        "a": params("unbiasedstate", 4, 3, "Newton-CG", "explicit", {"disp": False, "tol": 1e-6}, xinit=bin_centers,
                    yinit=0.5 * K0 * bin_centers ** 2),
        "b": params("biasedstates", 10, 3, "BFGS", "zeros", {"disp": False, "gtol": 1e-6}),
        "c": params("simplesum", 10, 3, "L-BFGS-B", "bias_free_energies", {"disp": False, "gtol": 1e-8, "ftol": 1e-14},
                    bias_centers=centers_b),
        "c2": params("biasedstates", 3, 2, "Newton-CG", "bias_free_energies", {"disp": False, "tol": 1e-8},
                     bias_centers=centers_b),
        "c3": params("unbiasedstate", 6, 3, "CG", "bias_free_energies", {"disp": False, "gtol": 1e-6}),
        "c4": params("unbiasedstate", 6, 3, "TNC", "zeros", {"disp": False, "tol": 1e-10}),
        "c5": params("unbiasedstate", 6, 3, "SLSQP", "zeros", {"disp": False, "ftol": 1e-12}),
        "d": params("unbiasedstate", 8, 3, "Newton-CG", "zeros", {"disp": False, "tol": 1e-8}, objective="map",
                    map_data=dict(logprior=lp, dlogprior=dlp, ddlogprior=ddlp)),
    }
    out["case_names"] = np.array(sorted(cases()))
    feses = {}
    for name, p in cases().items():
        fes = FES(u_kn, N_k)
        fes.generate_fes(u_n, x_n, fes_type="spline", spline_parameters=p)
        out[f"{name}_c"] = np.array(fes.fes_function.c)
        out[f"{name}_t"] = np.array(fes.fes_function.t)
        out[f"{name}_f_grid"] = fes.get_fes(grid, reference_point="from-lowest")["f_i"]
        out[f"{name}_aic"] = np.float64(np.squeeze(fes.get_information_criteria("aic")))
        out[f"{name}_bic"] = np.float64(np.squeeze(fes.get_information_criteria("bic")))
        out[f"{name}_w_n"] = fes.w_n
        feses[name] = fes
        print(name, np.array(fes.fes_function.c), out[f"{name}_aic"])
    out["a_f_specified"] = feses["a"].get_fes(grid, reference_point="from-specified", fes_reference=0.0)["f_i"].reshape(-1)

    # (e) bootstraps
    for name, base in (("e_u", "a"), ("e_b", "b")):
        seed = 7 if name == "e_u" else 8
        fes = FES(u_kn, N_k)
        fes.generate_fes(u_n, x_n, fes_type="spline", spline_parameters=cases()[base], n_bootstraps=2, seed=seed)
        out[f"{name}_seed"] = np.int64(seed)
        out[f"{name}_c"] = np.array(fes.fes_function.c)
        out[f"{name}_c_boot"] = np.stack([np.array(f.c) for f in fes.fes_functions])
        r = fes.get_fes(grid, reference_point="from-lowest", uncertainty_method="bootstrap")
        out[f"{name}_f_grid"], out[f"{name}_df_grid"] = r["f_i"], r["df_i"]
        # the replicates' draws again, each MBAR re-solved to 1e-12
        np.random.seed(seed)
        N = len(u_n)
        idx = np.arange(N)
        f_boots, idxs = [], []
        for b in range(2):
            off = 0
            for k in range(len(N_k)):
                idx[off:off + N_k[k]] = off + np.random.randint(0, N_k[k], size=N_k[k])
                off += N_k[k]
                np.random.randint(np.iinfo(np.int32).max)
            idxs.append(idx.copy())
        for ib in idxs:
            f_boots.append(pymbar.MBAR(u_kn[:, ib], N_k, initial_f_k=fes.mbar.f_k, relative_tolerance=1e-12).f_k)
        out[f"{name}_f_boots"] = np.array(f_boots)
        out[f"{name}_idx"] = np.array(idxs)

    # (f) MC on the fits of (a) and (b)
    for name, base in (("f_u", "a"), ("f_b", "b")):
        fes = feses[base]
        seed = 11 if name == "f_u" else 12
        out[f"{name}_c_start"] = np.array(fes.fes_function.c)
        np.random.seed(seed)
        mc_parameters = dict(niterations=300, fraction_change=0.02, sample_every=10, print_every=1000)
        fes.sample_parameter_distribution(x_n, mc_parameters=mc_parameters, decorrelate=True, verbose=False)
        mc = fes.get_mc_data()
        out[f"{name}_seed"] = np.int64(seed)
        out[f"{name}_samples"] = np.array(mc["samples"])
        out[f"{name}_logposteriors"] = np.array(mc["logposteriors"], dtype=np.float64).reshape(-1)
        out[f"{name}_acceptance"] = np.float64(mc["acceptance_ratio"])
        out[f"{name}_nequil"] = np.int64(mc["nequil"])
        out[f"{name}_g_logposterior"] = np.float64(mc["g_logposterior"])
        out[f"{name}_g_parameters"] = np.array(mc["g_parameters"])
        out[f"{name}_g"] = np.float64(mc["g"])
        ci = fes.get_confidence_intervals(grid, 5, 95)
        for key in ("plow", "phigh", "median", "values"):
            out[f"{name}_ci_{key}"] = np.array(ci[key])
        print(name, mc["acceptance_ratio"], mc["nequil"], np.shape(mc["samples"]))
    np.savez_compressed(os.path.join(HERE, "fes_spline.npz"), **out)


if __name__ == "__main__":
    main()
