"""CPU stand-in of the linear-family builders of ``pymbar_amd.device.DeviceMatrix`` -- TEST INFRASTRUCTURE ONLY.

``u_model`` is the exact statement of ``k_fill_linear_rows``: the fma chain of the scan passes -- from the offset, ``b`` ascending,
one fma per term -- evaluated with the exact vectorised ``fma`` of ``tests/device_math_model.py``.  ``LinearOracleMatrix`` gives the
oracle handle of ``tests/cpu_standin.py`` ``from_linear`` / ``fill_linear_rows`` through it.  Nothing under ``pymbar_amd/`` imports this.
"""
import numpy as np

from tests.cpu_standin import OracleMatrix
from tests.device_math_model import fma


def u_model(basis_bn, coeff_kb, offset_k=None):
    """``u[k, n] = fma(coeff[k, B-1], basis[B-1, n], ... fma(coeff[k, 0], basis[0, n], offset[k]))``, (K, N) float64."""
    basis_bn = np.asarray(basis_bn, dtype=np.float64)
    coeff_kb = np.asarray(coeff_kb, dtype=np.float64)
    K, B = coeff_kb.shape
    offset_k = np.zeros(K) if offset_k is None else np.asarray(offset_k, dtype=np.float64)
    u = np.repeat(offset_k[:, None], basis_bn.shape[1], axis=1)
    for b in range(B):
        u = fma(coeff_kb[:, b:b + 1], basis_bn[b][None, :], u)
    return np.ascontiguousarray(u)


class LinearOracleMatrix(OracleMatrix):
    created = 0  # handles made since a test last reset it ("before any device matrix is created")

    def __init__(self, u_shard, allreduce=None):
        type(self).created += 1
        super().__init__(u_shard, allreduce=allreduce)

    @classmethod
    def from_linear(cls, basis_bn, coeff_kb, offset_k=None, device=None, columns=None, validate=True):
        u = u_model(basis_bn, coeff_kb, offset_k)
        if columns is not None:
            u = u[:, columns[0]:columns[1]]
        return cls(np.array(u))

    def fill_linear_rows(self, row0, basis_bn, coeff_rb, offset_r=None, col0=0, validate=True):
        rows = u_model(basis_bn, coeff_rb, offset_r)[:, col0:col0 + self.N_local]
        self.u[row0:row0 + rows.shape[0]] = rows
