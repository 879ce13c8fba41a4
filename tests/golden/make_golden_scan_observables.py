"""Golden fixture for many observables along a scan (MBAR.compute_scan_expectations), generated from the UNMODIFIED reference
(compute_expectations with u_kn and uncertainty_method="approximate", pymbar/mbar.py:1124-1312, the Kong estimate at :1811):

    PYTHONPATH=/root/reference /opt/conda/bin/python3.9 tests/golden/make_golden_scan_observables.py

The system is config 1 (config1_ho_K5_N5000.npz; its u_kn is reused and asserted equal, x_n is regenerated from seed 0).  The
family is L = 24 harmonic oscillators (O_l, K_l) on a 4 x 6 grid in the interior of the hull of the five sampled ones, in the basis
{x^2, x} of pymbar_amd.testsystems.harmonic_scan_family.  The observables are x, x^2, cos x, sin 3x, |x|, tanh x and 1000 + x (an
indicator is left out: the reference's shift makes it log 0 and returns NaN).  Stored: O_l, K_l, coeff, offset, f_k and, per
observable and member, mu and the approximate sigma of compute_expectations(A, u_kn=u_ln, state_dependent=False).  Only data is
stored."""
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

NAMES = ("x", "x2", "cos_x", "sin_3x", "abs_x", "tanh_x", "1000_plus_x")


def observables(x_n):
    return np.stack([x_n, x_n * x_n, np.cos(x_n), np.sin(3.0 * x_n), np.abs(x_n), np.tanh(x_n), 1000.0 + x_n])


def family(x_n, O_k, K_k):
    """4 x 6 members strictly inside the hull: O on a grid over the middle 60 % of [O_min, O_max], K geometric over the middle 60 %
    of [log K_min, log K_max]"""
    o_mid, o_half = 0.5 * (O_k.min() + O_k.max()), 0.3 * (O_k.max() - O_k.min())
    lk_mid, lk_half = 0.5 * (np.log(K_k.min()) + np.log(K_k.max())), 0.3 * (np.log(K_k.max()) - np.log(K_k.min()))
    O = np.linspace(o_mid - o_half, o_mid + o_half, 4)
    Kf = np.exp(np.linspace(lk_mid - lk_half, lk_mid + lk_half, 6))
    O_l, K_l = [a.ravel() for a in np.meshgrid(O, Kf, indexing="ij")]
    return (O_l, K_l) + ts.harmonic_scan_family(x_n, O_l, K_l)


def main():
    g = np.load(os.path.join(HERE, "config1_ho_K5_N5000.npz"))
    x_n, u_kn, N_k, _, O_k, K_k = ts.config1(seed=0)
    assert np.array_equal(u_kn, g["u_kn"]) and np.array_equal(N_k, g["N_k"])
    mbar = pymbar.MBAR(u_kn, N_k, relative_tolerance=1e-12)
    O_l, K_l, basis, coeff, offset = family(x_n, O_k, K_k)
    u_ln = coeff @ basis + offset[:, None]
    assert np.allclose(u_ln, 0.5 * K_l[:, None] * (x_n[None, :] - O_l[:, None]) ** 2, rtol=1e-12, atol=1e-12)
    A_qn = observables(x_n)
    mu, sigma = np.zeros((len(A_qn), len(O_l))), np.zeros((len(A_qn), len(O_l)))
    for q, A in enumerate(A_qn):
        r = mbar.compute_expectations(A.copy(), u_kn=u_ln, state_dependent=False, uncertainty_method="approximate")
        mu[q], sigma[q] = r["mu"], r["sigma"]
    assert np.all(np.isfinite(mu)) and np.all(np.isfinite(sigma)) and np.all(sigma > 0.0)
    # the effective sample number of every member, from the reference's own weights
    logw = -u_ln - np.log(np.sum(N_k[:, None] * np.exp(mbar.f_k[:, None] - u_kn), axis=0))[None, :]
    w = np.exp(logw - logw.max(axis=1, keepdims=True))
    w /= w.sum(axis=1, keepdims=True)
    n_eff = 1.0 / np.sum(w * w, axis=1)
    print("L", len(O_l), "Q", len(A_qn), "min n_eff", n_eff.min(), "max sigma", sigma.max())
    np.savez_compressed(os.path.join(HERE, "scan_observables_ho_K5.npz"), names=np.array(NAMES), f_k=mbar.f_k, O_l=O_l, K_l=K_l, coeff=coeff,
                        offset=offset, mu=mu, sigma=sigma)


if __name__ == "__main__":
    main()
