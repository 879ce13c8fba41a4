"""Derivatives of f and of the averages along a scan (``MBAR.compute_scan_gradient``) on one MI355X, all in ONE process: kernel ms
of the moments pass (``mbar_scan_moments``, about the feature means) from the library's event timers, the wall time of the method
(both passes and the chain rule), and next to them the only exact route there was before: ``compute_scan(compute_uncertainty=False)``
called again and again with the features, their products (and the products with the observables) as STORED observables, three per
call -- which a family with harmonic terms does not have at all, because its features differ from member to member (it is left with
dense rows, ``8 L N`` bytes, and ``state_dependent=True``).

The system is the harmonic ladder of tools/bench_histogram.py (K = 128 states generated and solved in HBM); the members are
oscillators with centres across the ladder.  Cases: linear B = 2 with Q = 0 and Q = 2, linear B = 8, harmonic (B, H) = (8, 4).

    python tools/bench_scan_gradient.py [--reps 3] [--N 4000000] [--L 128,1024] [--out profiles/scan_gradient_bench.txt]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_histogram import resident_mbar, timed  # noqa: E402
from bench_scan import kernel_ms  # noqa: E402
from pymbar_amd import testsystems as ts  # noqa: E402
from pymbar_amd.scan import _shifted  # noqa: E402

EXTRA = (np.cos, np.sin, np.tanh, lambda x: np.cos(2.0 * x), lambda x: np.sin(2.0 * x), lambda x: 1.0 / (1.0 + x * x))


def family(x, O_k, L, B, H):
    """L oscillators across the ladder.  Linear: {x^2, x} and, for B = 8, six bounded features with small coefficients.  Harmonic (8, 4):
    the oscillator as ONE harmonic term on x about its centre, three more harmonic terms on bounded coordinates (two of them periodic)
    and four linear ones, all with small coefficients."""
    rng = np.random.default_rng(L + B)
    O_l = np.linspace(O_k[0], O_k[-1], L)
    K_l = np.full(L, 1.0 / (1.5 * (O_k[1] - O_k[0])) ** 2)
    if H == 0:
        basis, coeff, offset = ts.harmonic_scan_family(x, O_l, K_l)
        if B > 2:
            basis = np.vstack([basis] + [fn(x)[None, :] for fn in EXTRA[:B - 2]])
            coeff = np.hstack([coeff, rng.normal(0.0, 0.05, (L, B - 2))])
        return dict(basis_bn=basis, coeff_lb=coeff, offset_l=offset)
    hcoord = [x, 3.0 * np.sin(x), 2.0 * np.cos(x), 0.5 * x]
    period = [0.0, 0.0, 1.5, 1.0]
    basis = np.stack(hcoord[:H] + [fn(x) for fn in EXTRA[:B - H]])
    harmonic = np.arange(B) < H
    coeff = np.hstack([0.5 * K_l[:, None], rng.uniform(0.01, 0.05, (L, H - 1)), rng.normal(0.0, 0.05, (L, B - H))])
    center = np.hstack([O_l[:, None], rng.uniform(-1.0, 1.0, (L, H - 1)), np.zeros((L, B - H))])
    return dict(basis_bn=basis, coeff_lb=coeff, offset_l=np.zeros(L), center_lb=center, harmonic_b=harmonic,
                period_b=np.array(period[:H] + [0.0] * (B - H)))


def bench_case(m, x, O_k, L, B, H, Q, reps):
    dm = m._dm
    fam = family(x, O_k, L, B, H)
    A = np.stack([np.cos(x), x * x * np.sin(x)])[:Q] if Q else None
    out = dict(K=m.K, N=m.N, L=L, B=B, H=H, Q=Q, F=B + H)
    kinds = {k: fam[k] for k in ("harmonic_b", "period_b") if k in fam}
    cen = {k: fam[k] for k in ("center_lb",) if k in fam}
    t_qn = None if A is None else _shifted(A)[0]
    dm.set_option("timing", 1)
    dm.set_scan(fam["basis_bn"], t_qn, **kinds)
    centre = dm.scan_moments(m.f_k, fam["coeff_lb"], fam["offset_l"], None, **cen)[2].copy()
    out["moments_pass_kernel_ms"] = kernel_ms(dm, lambda: dm.scan_moments(m.f_k, fam["coeff_lb"], fam["offset_l"], centre, **cen), reps)
    out["plain_pass_a_kernel_ms"] = kernel_ms(dm, lambda: dm.scan_lognum(m.f_k, fam["coeff_lb"], fam["offset_l"], **cen), reps)
    dm.set_option("timing", 0)
    dm.set_scan(None)
    out["method_wall_ms"] = timed(lambda: m.compute_scan_gradient(A_qn=A, **fam), reps)
    res = m.compute_scan_gradient(A_qn=A, **fam)
    if H == 0:
        # the route of the parent commit: the features, their products and the products with the observables as stored observables
        basis = fam["basis_bn"]
        stored = [basis[i] for i in range(B)] + [basis[i] * basis[j] for i in range(B) for j in range(i, B)]
        if Q:
            stored += list(A) + [a * basis[i] for a in A for i in range(B)]
        groups = [np.stack(stored[i:i + 3]) for i in range(0, len(stored), 3)]
        out["stored_route_observables"], out["stored_route_calls"] = len(stored), len(groups)

        def route():
            return [m.compute_scan(fam["basis_bn"], fam["coeff_lb"], fam["offset_l"], g, compute_uncertainty=False)["mu"] for g in groups]

        out["stored_route_wall_ms"] = timed(route, max(1, reps - 1))
        mu = np.vstack(route())  # (n_stored, L)
        cov = mu[B] - mu[0] * mu[0]  # Var(phi_0) by the raw-moment route
        out["max_rel_var_phi0_difference"] = float(np.max(np.abs(res["feature_cov"][:, 0, 0] / cov - 1.0)))
        out["max_abs_grad_f_difference"] = float(np.max(np.abs(res["grad_f"] - mu[:B].T)))
    else:
        out["stored_route"] = "none: the features wrap(x - c_l) differ from member to member; the parent commit is left with dense rows"
        out["dense_rows_bytes"] = int(8 * L * m.N)
    for key in list(out):
        if key.endswith("_ms"):
            out[key + "_median"] = float(np.median(out[key]))
    if H == 0:
        out["stored_route_over_method"] = out["stored_route_wall_ms_median"] / out["method_wall_ms_median"]
    out["moments_over_plain_pass_a"] = out["moments_pass_kernel_ms_median"] / out["plain_pass_a_kernel_ms_median"]
    out["finite"] = bool(all(np.all(np.isfinite(res[k])) for k in ("f", "grad_f", "hess_f")))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--N", type=int, default=4000000)
    ap.add_argument("--L", default="128,1024")
    ap.add_argument("--K", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_gradient_bench.txt"))
    a = ap.parse_args()
    m, x, O_k = resident_mbar(a.K, a.N)
    m.u_kn, m.n_bootstraps = None, 0
    lines = []
    for L in [int(v) for v in a.L.split(",")]:
        for B, H, Q in ((2, 0, 0), (2, 0, 2), (8, 0, 0), (8, 4, 0)):
            r = bench_case(m, x, O_k, L, B, H, Q, a.reps)
            lines.append(json.dumps(r))
            print(lines[-1], file=sys.stderr, flush=True)
            with open(a.out, "w") as fh:  # (kept up to date case by case)
                fh.write("\n".join(lines) + "\n")
    m._dm.close()
    print(json.dumps(dict(bench="scan_gradient", cases=len(lines), out=a.out)))


if __name__ == "__main__":
    main()
