"""Every call the UNMODIFIED reference ``pymbar.MBAR`` makes into its solver module, recorded as a fixture.

    PYTHONPATH=<reference tree> /opt/conda/bin/python3.9 tests/golden/make_golden_boundary.py

The unchanged class reaches ``pymbar.mbar_solvers`` through two functions only (pymbar/mbar.py:413, 437 and 910
``solve_mbar_for_all_states``; :455 and 910 ``mbar_log_W_nk``); everything else it reports is computed from what those
return.  This script drives the class through the workload of tests/refshim/boundary_check.py -- three matrices, the default
and "robust" protocols, every uncertainty method, expectations, perturbed free energies, overlap, four bootstrap replicates
and bootstrapped expectations -- with the module behind ``pymbar.mbar.mbar_solvers`` wrapped so that each call is recorded:
its arguments (each matrix the class hands over as a column gather of the case's input, stored once per array object, so that a
replay can hand over the same object wherever the class did) and what the reference returned.
tests/test_reference_boundary.py replays the calls on ``pymbar_amd.mbar_solvers``.

``boundary_calls.npz`` (inputs regenerated from their seeds, as here; ``cases`` holds the SHA-256 of each matrix):
``cases`` and ``calls`` are JSON -- one entry per call, in order, naming its matrix j, that matrix's memory layout and its
column set; ``columns<s>`` (uint16) is column set s (array object j of the class = ``u_kn[:, columns<s>]`` of its case); per
call ``c<i>/f_k`` (the f_k handed in), ``c<i>/states_with_samples`` (solve calls) and the reference's answer: ``c<i>/f_out``
for a solve; for a log-weight call, whose answer is ``f_k - u_kn.T - log_denominator_n[:, None]`` with ``log_denominator_n =
logsumexp(f_k - u_kn.T, b=N_k, axis=1)`` (pymbar/mbar_solvers.py:447-448, checked here bit for bit), the reference's
``log_denominator_n`` at 64 seeded sample indices ``c<i>/sample_n`` -- enough to pin a restatement of that one line to the
reference, which is what the test compares the drop-in's whole N x K matrix against.
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

import pymbar  # noqa: E402  (the reference, from PYTHONPATH)
import pymbar.mbar  # noqa: E402

from pymbar_amd import testsystems as ts  # noqa: E402

ref_solvers = pymbar.mbar.mbar_solvers
assert os.path.realpath(ref_solvers.__file__).startswith(os.path.dirname(os.path.realpath(pymbar.__file__)))

CASES = {
    "config1": ts.config1(seed=0)[1:3],
    "unsampled": ts.harmonic_u_kn([0, 1, 2, 3], [1, 2, 4, 8], [800, 0, 700, 800], seed=3)[1:3],
    "ladder_K12": ts.harmonic_u_kn(np.linspace(0, 3, 12), np.linspace(1, 3, 12), [400] * 12, seed=5)[1:3],
}


def _plain(v):
    if isinstance(v, dict):
        return {k: _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    if isinstance(v, np.generic):
        return v.item()
    return v


class Recorder:
    """Stands in for the reference's solver module inside ``pymbar.mbar``: forwards everything, records the two calls."""

    def __init__(self):
        self.calls, self.arrays = [], {}
        self.case = self.phase = None
        self.col_of = None
        self.matrices = []  # every array object handed over, kept alive so that id() stays unique
        self.column_sets = {}  # bytes of a column set -> its index
        self.matrix_columns = []  # matrix j -> its column set

    def set_case(self, name):
        self.case = name
        base = CASES[name][0]
        self.col_of = {base[:, n].tobytes(): n for n in range(base.shape[1])}
        assert len(self.col_of) == base.shape[1]

    def _matrix(self, u_kn):
        for j, m in enumerate(self.matrices):
            if m is u_kn:
                return j
        assert u_kn.shape == CASES[self.case][0].shape
        cols = np.array([self.col_of[u_kn[:, n].tobytes()] for n in range(u_kn.shape[1])], dtype=np.uint16)
        assert u_kn.shape[1] <= np.iinfo(np.uint16).max + 1
        key = (self.case, cols.tobytes())
        if key not in self.column_sets:
            self.column_sets[key] = len(self.column_sets)
            self.arrays[f"columns{self.column_sets[key]}"] = cols
        self.matrix_columns.append(self.column_sets[key])
        self.matrices.append(u_kn)
        return len(self.matrices) - 1

    def _record(self, fn, u_kn, N_k, f_k, extra):
        i = len(self.calls)
        j = self._matrix(u_kn)
        assert np.array_equal(np.asarray(N_k, dtype=float), CASES[self.case][1].astype(float))
        self.arrays[f"c{i}/f_k"] = np.array(f_k, dtype=np.float64)
        entry = dict(fn=fn, case=self.case, phase=self.phase, matrix=j, columns=self.matrix_columns[j],
                     c_contiguous=bool(u_kn.flags.c_contiguous), **extra)
        self.calls.append(entry)
        return i

    def solve_mbar_for_all_states(self, u_kn, N_k, f_k, states_with_samples, solver_protocol):
        i = self._record("solve_mbar_for_all_states", u_kn, N_k, f_k, dict(solver_protocol=_plain(solver_protocol)))
        self.arrays[f"c{i}/states_with_samples"] = np.array(states_with_samples)
        out = ref_solvers.solve_mbar_for_all_states(u_kn, N_k, f_k, states_with_samples, solver_protocol)
        self.arrays[f"c{i}/f_out"] = np.array(out, dtype=np.float64)
        return out

    def mbar_log_W_nk(self, u_kn, N_k, f_k):
        i = self._record("mbar_log_W_nk", u_kn, N_k, f_k, {})
        out = ref_solvers.mbar_log_W_nk(u_kn, N_k, f_k)
        log_den = ref_solvers.logsumexp(f_k - u_kn.T, b=N_k, axis=1)
        assert np.array_equal(f_k - u_kn.T - log_den[:, np.newaxis], out)  # the matrix follows from the stored vector exactly
        sample = np.sort(np.random.default_rng(i).choice(len(log_den), size=min(64, len(log_den)), replace=False))
        self.arrays[f"c{i}/sample_n"] = sample.astype(np.uint16)
        self.arrays[f"c{i}/log_denominator_sample"] = np.array(log_den[sample], dtype=np.float64)
        return out

    def __getattr__(self, name):
        return getattr(ref_solvers, name)


rec = Recorder()
pymbar.mbar.mbar_solvers = rec
arrays = rec.arrays
for cname, (u_kn, N_k) in CASES.items():
    arrays[f"{cname}/N_k"] = N_k
    rec.set_case(cname)
    K, N = u_kn.shape
    A_n = np.random.default_rng(1).normal(size=N) ** 2 + 0.5
    for proto in (None, "robust"):
        rec.phase = f"construct/{proto or 'default'}"
        m = pymbar.MBAR(u_kn, N_k, solver_protocol=proto)
        rec.phase = f"consume/{proto or 'default'}"
        for method in (None, "svd", "approximate"):
            m.compute_free_energy_differences(uncertainty_method=method)
        m.compute_expectations(A_n)
        m.compute_perturbed_free_energies(u_kn[:2] * 1.1)
        m.compute_overlap()
    rec.phase = "construct/bootstrap"
    m = pymbar.MBAR(u_kn, N_k, n_bootstraps=4, rseed=11)
    rec.phase = "consume/bootstrap"
    m.compute_free_energy_differences(uncertainty_method="bootstrap")
    m.compute_expectations(A_n, uncertainty_method="bootstrap")
pymbar.mbar.mbar_solvers = ref_solvers

arrays["calls"] = np.array(json.dumps(rec.calls))
arrays["cases"] = np.array(json.dumps({c: {"sha256": hashlib.sha256(np.ascontiguousarray(u).tobytes()).hexdigest()}
                                       for c, (u, _) in CASES.items()}))
np.savez_compressed(os.path.join(HERE, "boundary_calls.npz"), **arrays)
for c in rec.calls:
    print(c["case"], c["phase"], c["fn"], "matrix", c["matrix"])
print(len(rec.calls), "calls;", os.path.getsize(os.path.join(HERE, "boundary_calls.npz")), "bytes")
