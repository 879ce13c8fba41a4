"""SURVEY.md 8(b) / INTEGRATION.md section 2, tested at the boundary itself: the reference's own, UNCHANGED ``pymbar.MBAR``
reaches its solver module through ``solve_mbar_for_all_states`` and ``mbar_log_W_nk`` only, and everything else it reports
(free energy differences with every uncertainty method, expectations, perturbed free energies, overlap, bootstraps) is computed
from what those return.  tests/golden/make_golden_boundary.py recorded every such call the unchanged class makes for the
default and "robust" protocols and four bootstrap replicates on three matrices, together with the reference's answers; here
each call is replayed, in order and with the same array objects, on ``pymbar_amd.mbar_solvers`` (CPU stand-in device) and must
reproduce the reference to 1e-12 (1e-10 for the solves of the bootstrapping object): the free energies against the
reference's stored answers, every log-weight matrix in full against the reference's one-line formula, which the fixture pins
to the reference's own values at sample indices.  tests/refshim/boundary_check.py runs
the class itself against a reference tree."""
import hashlib
import json

import numpy as np
from scipy.special import logsumexp

from pymbar_amd import testsystems as ts

# the inputs of tests/golden/make_golden_boundary.py, regenerated from their seeds (the fixture holds their SHA-256)
CASES = {
    "config1": lambda: ts.config1(seed=0)[1],
    "unsampled": lambda: ts.harmonic_u_kn([0, 1, 2, 3], [1, 2, 4, 8], [800, 0, 700, 800], seed=3)[1],
    "ladder_K12": lambda: ts.harmonic_u_kn(np.linspace(0, 3, 12), np.linspace(1, 3, 12), [400] * 12, seed=5)[1],
}


def _deviation(a, b):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    assert a.shape == b.shape, (a.shape, b.shape)
    return float(np.max(np.abs(a - b))) / max(1.0, float(np.max(np.abs(a)))) if a.size else 0.0


def test_unchanged_reference_MBAR_on_the_drop_in_solver_module(golden, monkeypatch):
    import pymbar_amd.device
    import pymbar_amd.mbar_solvers as amd_solvers
    from tests.cpu_standin import OracleMatrix

    uploads = []

    class Counting(OracleMatrix):
        @classmethod
        def from_host(cls, u_kn, device=None, columns=None):
            uploads.append(np.shape(u_kn))
            return super().from_host(u_kn, device=device, columns=columns)

    monkeypatch.setattr(pymbar_amd.device, "DeviceMatrix", Counting)
    g = golden("boundary_calls.npz")
    calls = json.loads(str(g["calls"]))
    inputs = {}
    for case, digest in json.loads(str(g["cases"])).items():
        inputs[case] = np.ascontiguousarray(CASES[case]())
        assert hashlib.sha256(inputs[case].tobytes()).hexdigest() == digest["sha256"], case
    matrices = {}  # the recorded array objects of the class, rebuilt once each: a call hands over the object the class did
    worst = {}
    uploads_by_phase = {}
    for i, c in enumerate(calls):
        case, j = c["case"], c["matrix"]
        if j not in matrices:
            gathered = inputs[case][:, g[f"columns{c['columns']}"].astype(np.intp)]
            matrices[j] = np.ascontiguousarray(gathered) if c["c_contiguous"] else np.asfortranarray(gathered)
        u_kn, N_k, f_k = matrices[j], g[f"{case}/N_k"], g[f"c{i}/f_k"]
        phase = f"{case}/{c['phase']}"
        if phase not in uploads_by_phase:
            uploads_by_phase[phase] = 0
            if c["phase"].startswith("construct/"):
                amd_solvers.drop_resident_cache()  # (a new object of the class: nothing of the previous one is resident)
        n0 = len(uploads)
        if c["fn"] == "solve_mbar_for_all_states":
            protocol = tuple(c["solver_protocol"])
            out = amd_solvers.solve_mbar_for_all_states(u_kn, N_k, f_k.copy(), g[f"c{i}/states_with_samples"], protocol)
            name, want = f"{phase}/f_k", g[f"c{i}/f_out"]
            tol = 1e-10 if c["phase"] == "construct/bootstrap" else 1e-12
        else:
            out = amd_solvers.mbar_log_W_nk(u_kn, N_k, f_k.copy())
            # the reference's answer is this one line (pymbar/mbar_solvers.py:447-448); the fixture pins it to the reference's
            # own log denominators at 64 sample indices
            log_den = logsumexp(f_k - u_kn.T, b=N_k, axis=1)
            sample = g[f"c{i}/sample_n"].astype(np.intp)
            assert _deviation(g[f"c{i}/log_denominator_sample"], log_den[sample]) <= 1e-14, (i, "restated log denominator")
            want = f_k - u_kn.T - log_den[:, np.newaxis]
            name, tol = f"{phase}/Log_W_nk", 1e-12
            assert np.shape(out) == (u_kn.shape[1], u_kn.shape[0])
        dev = _deviation(want, out)
        worst[name] = max(worst.get(name, 0.0), dev)
        assert dev <= tol, (i, name, dev, tol)
        uploads_by_phase[phase] += len(uploads) - n0
    assert len(calls) >= 40 and max(worst.values()) < 1e-9, worst
    # the drop-in keeps the matrix resident between the unchanged MBAR's calls into the solver module: one upload per object
    # (+ one per bootstrap replicate, each a freshly gathered matrix)
    for case in ("config1", "unsampled", "ladder_K12"):
        for proto in ("default", "robust"):
            assert uploads_by_phase[f"{case}/construct/{proto}"] == 1, uploads_by_phase
        assert uploads_by_phase[f"{case}/construct/bootstrap"] == 1 + 4, uploads_by_phase
