"""Golden fixture for families with harmonic terms on a periodic coordinate (MBAR.from_family, compute_scan and compute_scan_fes
with periodic members), generated from the UNMODIFIED reference (pymbar.MBAR, pymbar.FES), by the recipe of the other
make_golden_*.py scripts: the reference checkout on PYTHONPATH, the interpreter that has its dependencies,

    PYTHONPATH=<reference checkout> python3.9 tests/golden/make_golden_periodic_umbrella.py

The system is umbrella sampling of a torsion on a cosine potential (pymbar_amd.testsystems.periodic_umbrella_family, seed 0): K = 6
umbrellas, 300 samples each.  The dense matrices are built here in numpy the way the reference's umbrella-sampling example treats
its torsion -- the distance to the centre is |chi - chi0|, and 360 minus that where it exceeds 180 -- not through this package's
family code.  Stored: the samples and the parameters; f_k, Delta_f and dDelta_f of the six umbrellas; the perturbed free energies
(row 0 of Delta_f / dDelta_f of compute_perturbed_free_energies) of 40 unsampled restraint centres that cross the +-180 seam
(120 .. 240 degrees); and the 30-bin histogram surface (get_fes at the bin centres, "from-lowest", analytical) of the unbiased
potential and of three of those centres.  Only data is stored."""
import importlib.util
import logging
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
logging.disable(logging.WARNING)
try:
    import numexpr  # noqa: F401
except ImportError:
    # An interpreter without numexpr: the reference imports it for two elementwise expressions of its logsumexp ("exp(a - a_max)",
    # "b * exp(a - a_max)").  They are evaluated by numpy instead, on the caller's variables as numexpr does; the reference's own
    # files stay as they are.  The stored numbers then differ from a run with numexpr by rounding at most (1e-15 relative, seven
    # orders below what the tests hold them to).
    import sys
    import types

    def _evaluate(expression):
        frame = sys._getframe(1)
        names = dict(frame.f_globals)
        names.update(frame.f_locals)
        return eval(expression, {"__builtins__": {}}, dict(names, exp=np.exp))

    sys.modules["numexpr"] = types.SimpleNamespace(evaluate=_evaluate)
import pymbar  # noqa: E402
from pymbar import FES  # noqa: E402

assert not os.path.realpath(pymbar.__file__).startswith(ROOT), pymbar.__file__  # (the reference, not this package)

spec = importlib.util.spec_from_file_location("ts", os.path.join(ROOT, "pymbar_amd", "testsystems.py"))
ts = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ts)

K, N_PER, L, NBINS = 6, 300, 40, 30
SURFACE_MEMBERS = (3, 20, 36)  # the centres whose surfaces are stored, next to the unbiased potential's


def restrained(E, chi, beta, spring, chi0):
    """u[l, n] = beta_l [E_n + spring_l / 2 d^2], d the distance on the circle of 360 degrees"""
    d = np.abs(chi[None, :] - chi0[:, None])
    d = np.where(d > 180.0, 360.0 - d, d)
    return beta[:, None] * (E[None, :] + 0.5 * spring[:, None] * d * d)


def main():
    basis, coeff, center, harmonic, period, offset, N_k = ts.periodic_umbrella_family(K=K, n_per_state=N_PER, seed=0)
    E, chi = basis
    beta_k, spring_k, chi0_k = coeff[:, 0], 2.0 * coeff[:, 1] / coeff[:, 0], center[:, 1]
    u_kn = restrained(E, chi, beta_k, spring_k, chi0_k)
    mbar = pymbar.MBAR(u_kn, N_k, relative_tolerance=1e-12)
    fed = mbar.compute_free_energy_differences()
    # the unsampled centres: the spring of the umbrellas, centres from 120 to 240 degrees (those above 180 lie outside the period:
    # the distance on the circle is taken to their image)
    chi0_l = np.linspace(120.0, 240.0, L)
    image = np.where(chi0_l > 180.0, chi0_l - 360.0, chi0_l)
    u_ln = restrained(E, chi, np.ones(L), np.full(L, spring_k[0]), image)
    pert = mbar.compute_perturbed_free_energies(u_ln)
    edges = np.linspace(-180.0, 180.0, NBINS + 1)
    edges[0], edges[-1] = -180.0 - 1e-9, 180.0 + 1e-9
    centers = 0.5 * (edges[1:] + edges[:-1])
    assert np.all(np.bincount(np.digitize(chi, edges) - 1, minlength=NBINS) > 0)  # every bin is populated
    fes = FES(u_kn, N_k, mbar_options=dict(relative_tolerance=1e-12))
    rows = dict(fes_f_raw=[], fes_f_i=[], fes_df_i=[])
    for u_n in [E] + [u_ln[l] for l in SURFACE_MEMBERS]:
        fes.generate_fes(u_n.copy(), chi.copy(), fes_type="histogram", histogram_parameters={"bin_edges": edges})
        hd = fes.histogram_data
        rows["fes_f_raw"].append([hd["f"][hd["bin_order"][hd["bin_label"][(i,)]]] for i in range(NBINS)])
        lo = fes.get_fes(centers, reference_point="from-lowest", uncertainty_method="analytical")
        rows["fes_f_i"].append(lo["f_i"])
        rows["fes_df_i"].append(lo["df_i"])
    rows = {k: np.array(v, dtype=np.float64) for k, v in rows.items()}
    assert all(np.all(np.isfinite(v)) for v in rows.values())
    np.savez_compressed(os.path.join(HERE, "periodic_umbrella_K6.npz"), chi_n=chi, E_n=E, N_k=N_k, beta_k=beta_k, spring_k=spring_k,
                        chi0_k=chi0_k, f_k=mbar.f_k, Delta_f=fed["Delta_f"], dDelta_f=fed["dDelta_f"], chi0_l=chi0_l,
                        pert_Delta_f=pert["Delta_f"][0], pert_dDelta_f=pert["dDelta_f"][0], bin_edges=edges,
                        surface_members=np.array(SURFACE_MEMBERS), **rows)


if __name__ == "__main__":
    main()
