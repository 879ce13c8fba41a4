"""Golden fixture for reweighting scans over a linear family of unsampled states (MBAR.compute_scan), generated from the
UNMODIFIED reference (compute_perturbed_free_energies, pymbar/mbar.py:1442-1521; compute_expectations with u_kn, :1124-1312):

    PYTHONPATH=/root/reference /opt/conda/bin/python3.9 tests/golden/make_golden_scan.py

The system is config 1 (config1_ho_K5_N5000.npz; its u_kn is reused and asserted equal, x_n is regenerated from seed 0).  The
family is L = 300 harmonic oscillators (O_l, K_l) on a 15 x 20 grid inside the hull of the five sampled ones, in the basis
{x^2, x} of pymbar_amd.testsystems.harmonic_scan_family.  The grid is narrowed towards the hull's centre until every
dDelta_f[0, l] of the reference is finite and below 1.  Stored: O_l, K_l, coeff, offset, Delta_f[0, :] and dDelta_f[0, :] of
compute_perturbed_free_energies, mu and sigma of x and x^2 from compute_expectations(..., u_kn=u_ln).  Only data is stored."""
import importlib.util
import logging
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
logging.disable(logging.WARNING)
import pymbar  # noqa: E402

assert os.path.realpath(pymbar.__file__).startswith("/root/reference"), pymbar.__file__

spec = importlib.util.spec_from_file_location("ts", os.path.join(ROOT, "pymbar_amd", "testsystems.py"))
ts = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ts)


def family(x_n, O_k, K_k, shrink):
    """15 x 20 members: O on a grid around the centre of [O_min, O_max], K geometric around the centre of [K_min, K_max]"""
    o_mid, o_half = 0.5 * (O_k.min() + O_k.max()), 0.5 * (O_k.max() - O_k.min()) * shrink
    lk_mid, lk_half = 0.5 * (np.log(K_k.min()) + np.log(K_k.max())), 0.5 * (np.log(K_k.max()) - np.log(K_k.min())) * shrink
    O = np.linspace(o_mid - o_half, o_mid + o_half, 15)
    Kf = np.exp(np.linspace(lk_mid - lk_half, lk_mid + lk_half, 20))
    O_l, K_l = [a.ravel() for a in np.meshgrid(O, Kf, indexing="ij")]
    return (O_l, K_l) + ts.harmonic_scan_family(x_n, O_l, K_l)


def main():
    g = np.load(os.path.join(HERE, "config1_ho_K5_N5000.npz"))
    x_n, u_kn, N_k, _, O_k, K_k = ts.config1(seed=0)
    assert np.array_equal(u_kn, g["u_kn"]) and np.array_equal(N_k, g["N_k"])
    mbar = pymbar.MBAR(u_kn, N_k, relative_tolerance=1e-12)
    shrink = 1.0
    while True:
        O_l, K_l, basis, coeff, offset = family(x_n, O_k, K_k, shrink)
        u_ln = coeff @ basis + offset[:, None]
        assert np.allclose(u_ln, 0.5 * K_l[:, None] * (x_n[None, :] - O_l[:, None]) ** 2, rtol=1e-12, atol=1e-12)
        pert = mbar.compute_perturbed_free_energies(u_ln)
        d = pert["dDelta_f"][0]
        if np.all(np.isfinite(d)) and np.all(d < 1.0):
            break
        shrink *= 0.9
        assert shrink > 0.05
    print("shrink", shrink, "max dDelta_f[0]", d.max(), "L", len(O_l))
    out = dict(shrink=np.float64(shrink), f_k=mbar.f_k, O_l=O_l, K_l=K_l, coeff=coeff, offset=offset, Delta_f=pert["Delta_f"][0],
               dDelta_f=d)
    for name, A in (("x", x_n), ("x2", x_n * x_n)):
        r = mbar.compute_expectations(A.copy(), u_kn=u_ln, state_dependent=False)
        out["mu_" + name], out["sigma_" + name] = r["mu"], r["sigma"]
    np.savez_compressed(os.path.join(HERE, "scan_ho_K5_L300.npz"), **out)


if __name__ == "__main__":
    main()
