"""Golden fixture for the differences between any two members of a scan (MBAR.compute_scan_pairs), generated from the UNMODIFIED
reference (compute_perturbed_free_energies, pymbar/mbar.py:1442-1521; compute_expectations with u_kn and output="differences",
:1124-1312):

    PYTHONPATH=/root/reference /opt/conda/bin/python3.9 tests/golden/make_golden_scan_pairs.py

The system is config 1 (config1_ho_K5_N5000.npz; its u_kn is reused and asserted equal, x_n is regenerated from seed 0).  The
members are the 43 members np.arange(0, 300, 7) of the family of scan_ho_K5_L300.npz (make_golden_scan.py), in the basis {x^2, x}
of pymbar_amd.testsystems.harmonic_scan_family.  Stored: members, the full 43 x 43 Delta_f and dDelta_f of
compute_perturbed_free_energies(u_ln), and the full mu and sigma of compute_expectations(A, u_kn=u_ln, state_dependent=False,
output="differences") for A = x and x^2.  Every off-diagonal entry of the uncertainties is asserted finite and positive before
anything is stored.  Only data is stored.  (This docstring is the fixture's description: like scan_ho_K5_L300.npz it has no entry in
MANIFEST.json, which stays as it is.)"""
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

NAME = "scan_pairs_ho_K5.npz"


def main():
    g = np.load(os.path.join(HERE, "config1_ho_K5_N5000.npz"))
    scan = np.load(os.path.join(HERE, "scan_ho_K5_L300.npz"))
    x_n, u_kn, N_k, _, _, _ = ts.config1(seed=0)
    assert np.array_equal(u_kn, g["u_kn"]) and np.array_equal(N_k, g["N_k"])
    members = np.arange(0, 300, 7)
    basis, coeff, offset = ts.harmonic_scan_family(x_n, scan["O_l"][members], scan["K_l"][members])
    assert np.array_equal(coeff, scan["coeff"][members]) and np.array_equal(offset, scan["offset"][members])
    u_ln = coeff @ basis + offset[:, None]
    mbar = pymbar.MBAR(u_kn, N_k, relative_tolerance=1e-12)
    pert = mbar.compute_perturbed_free_energies(u_ln)
    out = dict(members=members, f_k=mbar.f_k, Delta_f=np.asarray(pert["Delta_f"]), dDelta_f=np.asarray(pert["dDelta_f"]))
    for name, A in (("x", x_n), ("x2", x_n * x_n)):
        r = mbar.compute_expectations(A.copy(), u_kn=u_ln, state_dependent=False, output="differences")
        out["mu_" + name], out["sigma_" + name] = np.asarray(r["mu"]), np.asarray(r["sigma"])
    L = len(members)
    off = ~np.eye(L, dtype=bool)
    for key, v in out.items():
        if v.ndim == 2:
            assert v.shape == (L, L), key
            assert np.all(np.isfinite(v)), key
    for key in ("dDelta_f", "sigma_x", "sigma_x2"):
        assert np.all(out[key][off] > 0.0), key
        print(key, "smallest off-diagonal", out[key][off].min(), "largest", out[key][off].max())
    np.savez_compressed(os.path.join(HERE, NAME), **out)


if __name__ == "__main__":
    main()
