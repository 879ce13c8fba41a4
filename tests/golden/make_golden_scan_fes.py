"""Golden fixture for histogram free energy surfaces along a scan (MBAR.compute_scan_fes), generated from the UNMODIFIED
reference (FES.generate_fes / get_fes with fes_type="histogram", pymbar/fes.py:500-600, 1340-1480), by the recipe of the other
make_golden_*.py scripts: the reference checkout on PYTHONPATH, the interpreter that has its dependencies,

    PYTHONPATH=<reference checkout> python3.9 tests/golden/make_golden_scan_fes.py

The system is config 1 (config1_ho_K5_N5000.npz; its u_kn is reused and asserted equal, x_n is regenerated from seed 0).  The
family is a sweep of a restraint centre: L = 8 harmonic restraints of one spring constant whose centres O_l cross the hull of the
five sampled oscillators, in the basis {x^2, x} of pymbar_amd.testsystems.harmonic_scan_family.  The histogram has 20 equal bins
over the data range (the outer edges a hair outside it, so that no sample is an overflow).  The sweep is narrowed towards the
hull's centre until every df_i of the reference is finite.  Stored per member, in grid order: f_i and df_i from get_fes at the
bin centres, "from-lowest" and "from-specified" (the bin of x_ref), uncertainty_method="analytical"; and the bin free energies
histogram_data["f"] in grid order.  Only data is stored."""
import importlib.util
import logging
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
logging.disable(logging.WARNING)
import pymbar  # noqa: E402
from pymbar import FES  # noqa: E402

assert not os.path.realpath(pymbar.__file__).startswith(ROOT), pymbar.__file__  # (the reference, not this package)

spec = importlib.util.spec_from_file_location("ts", os.path.join(ROOT, "pymbar_amd", "testsystems.py"))
ts = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ts)

L, NBINS, SPRING = 8, 20, 2.0


def main():
    g = np.load(os.path.join(HERE, "config1_ho_K5_N5000.npz"))
    x_n, u_kn, N_k, _, O_k, K_k = ts.config1(seed=0)
    assert np.array_equal(u_kn, g["u_kn"]) and np.array_equal(N_k, g["N_k"])
    span = x_n.max() - x_n.min()
    edges = np.linspace(x_n.min() - 1e-9 * span, x_n.max() + 1e-9 * span, NBINS + 1)
    centers = 0.5 * (edges[1:] + edges[:-1])
    assert np.all(np.bincount(np.digitize(x_n, edges) - 1, minlength=NBINS) > 0)  # every bin is populated
    x_ref = float(centers[NBINS // 2])
    fes = FES(u_kn, N_k, mbar_options=dict(relative_tolerance=1e-12))
    o_mid, o_half = 0.5 * (O_k.min() + O_k.max()), 0.5 * (O_k.max() - O_k.min())
    shrink = 1.0
    while True:
        O_l, K_l = np.linspace(o_mid - shrink * o_half, o_mid + shrink * o_half, L), np.full(L, SPRING)
        basis, coeff, offset = ts.harmonic_scan_family(x_n, O_l, K_l)
        u_ln = coeff @ basis + offset[:, None]
        assert np.allclose(u_ln, 0.5 * K_l[:, None] * (x_n[None, :] - O_l[:, None]) ** 2, rtol=1e-12, atol=1e-12)
        rows = dict(f_raw=[], f_lowest=[], df_lowest=[], f_specified=[], df_specified=[])
        for l in range(L):
            fes.generate_fes(u_ln[l].copy(), x_n.copy(), fes_type="histogram", histogram_parameters={"bin_edges": edges})
            hd = fes.histogram_data
            rows["f_raw"].append([hd["f"][hd["bin_order"][hd["bin_label"][(i,)]]] for i in range(NBINS)])
            lo = fes.get_fes(centers, reference_point="from-lowest", uncertainty_method="analytical")
            sp = fes.get_fes(centers, reference_point="from-specified", fes_reference=x_ref, uncertainty_method="analytical")
            rows["f_lowest"].append(lo["f_i"])
            rows["df_lowest"].append(lo["df_i"])
            rows["f_specified"].append(sp["f_i"])
            rows["df_specified"].append(sp["df_i"])
        rows = {k: np.array(v, dtype=np.float64) for k, v in rows.items()}
        if all(np.all(np.isfinite(v)) for v in rows.values()):
            break
        shrink *= 0.9
        assert shrink > 0.05
    print("shrink", shrink, "max df_i", rows["df_lowest"].max(), rows["df_specified"].max())
    np.savez_compressed(os.path.join(HERE, "scan_fes_ho_K5.npz"), shrink=np.float64(shrink), f_k=fes.mbar.f_k, O_l=O_l, K_l=K_l,
                        coeff=coeff, offset=offset, bin_edges=edges, x_ref=np.float64(x_ref), **rows)


if __name__ == "__main__":
    main()
