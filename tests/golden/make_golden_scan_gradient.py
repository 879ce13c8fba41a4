"""Golden fixture for the derivatives of f and of the averages along a scan (MBAR.compute_scan_gradient), generated from the
UNMODIFIED reference (compute_expectations with u_kn=u_ln, pymbar/mbar.py):

    PYTHONPATH=<reference checkout>:tests/refshim python tests/golden/make_golden_scan_gradient.py

The reference has no derivative of its own; what it has are the raw moments the identities are made of,

    df/dp = <du/dp>,   d2f/dp dp' = <d2u/dp dp'> - Cov(du/dp, du/dp'),   d<A>/dp = -Cov(A, du/dp)

and the test forms the expected derivatives from them.  Two entries.

Config 1 (config1_ho_K5_N5000.npz; its u_kn is reused and asserted equal, x_n is regenerated from seed 0) with the 40 members of
scan_thermo_ho_K5.npz (O_l, K_l; the family {x^2, x} of pymbar_amd.testsystems.harmonic_scan_family): mu of
compute_expectations(A_n, u_kn=u_ln) for A = x^2 and x (mu_phi, 2 x L), their three products x^4, x^3, x^2 (mu_phiphi, in the order
(0, 0), (0, 1), (1, 1)), two observables A_q = cos x and x^2 sin x (mu_A, 2 x L) and their products with both features (mu_Aphi, 2 x
2 x L).

The seam (keys seam_*): the system of periodic_umbrella_K6.npz and its 40 unsampled restraint centres across the +-180 degree seam.
dl[l, n] = wrap(chi_n - chi0_l) is formed here in numpy per member; with state_dependent=True: mu of E, dl and dl^2 (seam_mu, 3 x L) and
of all their pairwise products (seam_mu2, 3 x 3 x L, symmetric).  Only data is stored."""
import importlib.util
import logging
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
logging.disable(logging.WARNING)
import pymbar  # noqa: E402

assert not os.path.realpath(pymbar.__file__).startswith(ROOT), pymbar.__file__  # (the reference, not this package)

spec = importlib.util.spec_from_file_location("ts", os.path.join(ROOT, "pymbar_amd", "testsystems.py"))
ts = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ts)


def observables(x_n):
    return np.stack([np.cos(x_n), x_n * x_n * np.sin(x_n)])


def mu_of(mbar, A_n, u_ln):
    return mbar.compute_expectations(np.array(A_n), u_kn=u_ln.copy(), compute_uncertainty=False)["mu"]


def mu_sd(mbar, A_ln, u_ln):
    return mbar.compute_expectations(np.array(A_ln), u_kn=u_ln.copy(), state_dependent=True, compute_uncertainty=False)["mu"]


def restrained(E, dl, beta, spring):
    return beta[:, None] * (E[None, :] + 0.5 * spring[:, None] * dl * dl)


def wrap(d, P=360.0):
    return d - P * np.rint(d / P)


def seam():
    g = np.load(os.path.join(HERE, "periodic_umbrella_K6.npz"))
    basis, _, _, _, _, _, N_k = ts.periodic_umbrella_family(K=6, n_per_state=300, seed=0)
    E, chi = basis
    assert np.array_equal(chi, g["chi_n"]) and np.array_equal(E, g["E_n"]) and np.array_equal(N_k, g["N_k"])
    u_kn = restrained(E, wrap(chi[None, :] - g["chi0_k"][:, None]), g["beta_k"], g["spring_k"])
    mbar = pymbar.MBAR(u_kn, N_k, relative_tolerance=1e-12)
    assert np.allclose(mbar.f_k, g["f_k"], rtol=0, atol=1e-10)
    chi0_l = g["chi0_l"]
    L = len(chi0_l)
    dl = wrap(chi[None, :] - chi0_l[:, None])
    u_ln = restrained(E, dl, np.ones(L), np.full(L, g["spring_k"][0]))
    phi = [np.repeat(E[None, :], L, axis=0), dl, dl * dl]
    mu = np.stack([mu_sd(mbar, p, u_ln) for p in phi])
    mu2 = np.empty((3, 3, L))
    for i in range(3):
        for j in range(i, 3):
            mu2[i, j] = mu2[j, i] = mu_sd(mbar, phi[i] * phi[j], u_ln)
    return dict(seam_mu=mu, seam_mu2=mu2, seam_f_k=mbar.f_k)


def main():
    g = np.load(os.path.join(HERE, "config1_ho_K5_N5000.npz"))
    t = np.load(os.path.join(HERE, "scan_thermo_ho_K5.npz"))
    x_n, u_kn, N_k, _, _, _ = ts.config1(seed=0)
    assert np.array_equal(u_kn, g["u_kn"]) and np.array_equal(N_k, g["N_k"])
    mbar = pymbar.MBAR(u_kn, N_k, relative_tolerance=1e-12)
    basis, coeff, offset = ts.harmonic_scan_family(x_n, t["O_l"], t["K_l"])
    assert np.array_equal(coeff, t["coeff"]) and np.array_equal(offset, t["offset"])
    u_ln = coeff @ basis + offset[:, None]
    phi = [basis[0], basis[1]]
    A = observables(x_n)
    out = dict(O_l=t["O_l"], K_l=t["K_l"], coeff=coeff, offset=offset, f_k=mbar.f_k)
    out["mu_phi"] = np.stack([mu_of(mbar, p, u_ln) for p in phi])
    out["mu_phiphi"] = np.stack([mu_of(mbar, phi[i] * phi[j], u_ln) for i, j in ((0, 0), (0, 1), (1, 1))])
    out["mu_A"] = np.stack([mu_of(mbar, a, u_ln) for a in A])
    out["mu_Aphi"] = np.stack([np.stack([mu_of(mbar, a * p, u_ln) for p in phi]) for a in A])
    out.update(seam())
    assert all(np.all(np.isfinite(v)) for v in out.values())
    np.savez_compressed(os.path.join(HERE, "scan_gradient_ho_K5.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
