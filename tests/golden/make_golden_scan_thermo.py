"""Golden fixture for entropy, enthalpy and heat capacity along a scan (MBAR.compute_scan_entropy_and_enthalpy), generated from the
UNMODIFIED reference (compute_entropy_and_enthalpy, pymbar/mbar.py:1524-1690; compute_expectations with state_dependent=True;
compute_multiple_expectations with compute_covariance=True):

    PYTHONPATH=<reference checkout> python3.9 tests/golden/make_golden_scan_thermo.py

The system is config 1 (config1_ho_K5_N5000.npz; its u_kn is reused and asserted equal, x_n is regenerated from seed 0).  The
family is L = 40 harmonic oscillators (O_l, K_l) on a 5 x 8 grid inside the hull of the five sampled ones, in the basis {x^2, x}
of pymbar_amd.testsystems.harmonic_scan_family, narrowed towards the hull's centre (the loop of make_golden_scan.py) until row 0
of every uncertainty of the reference is finite and below 1.  Stored: O_l, K_l, coeff, offset, row 0 of every array of
compute_entropy_and_enthalpy(u_kn=u_ln), mu of compute_expectations(u_ln**2, u_kn=u_ln, state_dependent=True), and for the 8
members PICK of compute_multiple_expectations([u_l, u_l^2], u_l, compute_covariance=True, return_theta=True) its mu, its 2 x 2
"covariances" (pick_cov: the reference returns the block of the log numerators there, mbar.py:1430) and the covariance of the two
averages themselves from its Theta, numerators minus denominator as the reference forms its own sigma (pick_cov_obs, mbar.py:1420).

A second entry (keys seam_*) is the system of periodic_umbrella_K6.npz (make_golden_periodic_umbrella.py: K = 6 umbrellas on a
torsion, 300 samples each, the dense matrices built with the reference example's distance on the circle) with that fixture's 40
unsampled restraint centres from 120 to 240 degrees, a sweep across the +-180 seam: row 0 of every array of
compute_entropy_and_enthalpy(u_kn=u_ln) and mu of u_ln and of u_ln^2 (state_dependent=True).  Only data is stored."""
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

PICK = np.array([0, 3, 9, 14, 20, 27, 33, 39])
NAMES = ("Delta_f", "dDelta_f", "Delta_u", "dDelta_u", "Delta_s", "dDelta_s")


def family(x_n, O_k, K_k, shrink):
    """5 x 8 members: O on a grid around the centre of [O_min, O_max], K geometric around the centre of [K_min, K_max]"""
    o_mid, o_half = 0.5 * (O_k.min() + O_k.max()), 0.5 * (O_k.max() - O_k.min()) * shrink
    lk_mid, lk_half = 0.5 * (np.log(K_k.min()) + np.log(K_k.max())), 0.5 * (np.log(K_k.max()) - np.log(K_k.min())) * shrink
    O = np.linspace(o_mid - o_half, o_mid + o_half, 5)
    Kf = np.exp(np.linspace(lk_mid - lk_half, lk_mid + lk_half, 8))
    O_l, K_l = [a.ravel() for a in np.meshgrid(O, Kf, indexing="ij")]
    return (O_l, K_l) + ts.harmonic_scan_family(x_n, O_l, K_l)


def restrained(E, chi, beta, spring, chi0):
    """u[l, n] = beta_l [E_n + spring_l / 2 d^2], d the distance on the circle of 360 degrees (make_golden_periodic_umbrella.py)"""
    d = np.abs(chi[None, :] - chi0[:, None])
    d = np.where(d > 180.0, 360.0 - d, d)
    return beta[:, None] * (E[None, :] + 0.5 * spring[:, None] * d * d)


def seam():
    g = np.load(os.path.join(HERE, "periodic_umbrella_K6.npz"))
    basis, coeff, center, harmonic, period, offset, N_k = ts.periodic_umbrella_family(K=6, n_per_state=300, seed=0)
    E, chi = basis
    assert np.array_equal(chi, g["chi_n"]) and np.array_equal(E, g["E_n"]) and np.array_equal(N_k, g["N_k"])
    u_kn = restrained(E, chi, g["beta_k"], g["spring_k"], g["chi0_k"])
    mbar = pymbar.MBAR(u_kn, N_k, relative_tolerance=1e-12)
    assert np.allclose(mbar.f_k, g["f_k"], rtol=0, atol=1e-10)
    chi0_l = g["chi0_l"]
    L = len(chi0_l)
    image = np.where(chi0_l > 180.0, chi0_l - 360.0, chi0_l)
    u_ln = restrained(E, chi, np.ones(L), np.full(L, g["spring_k"][0]), image)
    ee = mbar.compute_entropy_and_enthalpy(u_kn=u_ln.copy())
    out = {"seam_" + name: ee[name][0] for name in NAMES}
    out["seam_mu_u"] = mbar.compute_expectations(u_ln.copy(), u_kn=u_ln.copy(), state_dependent=True)["mu"]
    out["seam_mu_u2"] = mbar.compute_expectations((u_ln ** 2).copy(), u_kn=u_ln.copy(), state_dependent=True)["mu"]
    print("seam: max uncertainty in row 0", max(out["seam_" + n].max() for n in NAMES if n.startswith("d")))
    return out


def main():
    g = np.load(os.path.join(HERE, "config1_ho_K5_N5000.npz"))
    x_n, u_kn, N_k, _, O_k, K_k = ts.config1(seed=0)
    assert np.array_equal(u_kn, g["u_kn"]) and np.array_equal(N_k, g["N_k"])
    mbar = pymbar.MBAR(u_kn, N_k, relative_tolerance=1e-12)
    shrink = 1.0
    while True:
        O_l, K_l, basis, coeff, offset = family(x_n, O_k, K_k, shrink)
        u_ln = coeff @ basis + offset[:, None]
        ee = mbar.compute_entropy_and_enthalpy(u_kn=u_ln.copy())
        d = np.stack([ee[name][0] for name in NAMES if name.startswith("d")])
        if np.all(np.isfinite(d)) and np.all(d < 1.0):
            break
        shrink *= 0.9
        assert shrink > 0.05
    print("shrink", shrink, "max uncertainty in row 0", d.max(), "L", len(O_l))
    out = dict(shrink=np.float64(shrink), f_k=mbar.f_k, O_l=O_l, K_l=K_l, coeff=coeff, offset=offset, pick=PICK)
    for name in NAMES:
        out[name] = ee[name][0]
    out["mu_u2"] = mbar.compute_expectations((u_ln ** 2).copy(), u_kn=u_ln.copy(), state_dependent=True)["mu"]
    mu, cov, cov_obs = [], [], []
    for l in PICK:
        r = mbar.compute_multiple_expectations(np.stack([u_ln[l], u_ln[l] ** 2]), u_ln[l].copy(), compute_covariance=True,
                                               return_theta=True)
        mu.append(r["mu"])
        cov.append(r["covariances"])
        T = r["Theta"]  # (scaled by the observables: rows 0, 1 the numerators, rows 2, 3 the denominator)
        cov_obs.append(T[0:2, 0:2] + T[2:4, 2:4] - T[0:2, 2:4] - T[2:4, 0:2])
    out["pick_mu"], out["pick_cov"], out["pick_cov_obs"] = np.array(mu), np.array(cov), np.array(cov_obs)
    out.update(seam())
    assert all(np.all(np.isfinite(v)) for v in out.values())
    np.savez_compressed(os.path.join(HERE, "scan_thermo_ho_K5.npz"), **out)


if __name__ == "__main__":
    main()
