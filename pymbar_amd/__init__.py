"""pymbar_amd -- the MBAR solver hot path of choderalab/pymbar on AMD MI355X (gfx950).

``pymbar_amd.mbar_solvers`` exports the names of ``pymbar.mbar_solvers``; ``pymbar_amd.MBAR`` mirrors
the solver-facing part of ``pymbar.MBAR``.  All K x N sweeps run in ``csrc/libmbar_hip.so``
(hand-written HIP, C ABI in ``include/mbar_hip.h``), reached through ctypes.  Importing the package
does not load the library or touch a GPU; the first computation does, and fails loudly if it cannot.
"""
from . import mbar_solvers, other_estimators, testsystems, utils
from ._lib import BackendUnavailable, MbarHipError, trim_device_cache
from .batch import MBARBatch, mbar_batch
from .fes import FES
from .mbar import MBAR
from .other_estimators import bar, bar_batch, bar_overlap, bar_zero, exp, exp_gauss
from .utils import ParameterError

__all__ = ["MBAR", "FES", "mbar_solvers", "other_estimators", "testsystems", "utils", "ParameterError", "BackendUnavailable",
           "MbarHipError", "trim_device_cache", "mbar_batch", "MBARBatch", "bar", "bar_batch", "bar_overlap", "bar_zero", "exp",
           "exp_gauss"]
__version__ = "0.1.0"
