"""Error tables of the kernel-density bodies (profiles/kde_instantiation_matrix.txt): for every case of the instantiation matrix of
tests/kde_cases.py, the scaled error max |L - L_ld| / max(1, |L_ld|) against the long-double oracle of (a) the float64 numpy oracle
(CPU, the baseline) and (b) the device at max_chunks = 1 and 2.  tests/test_gpu_kde.py takes its bound from the last table.

    python tools/kde_instantiation_matrix.py > profiles/kde_instantiation_matrix.txt
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pymbar_amd.kde import DeviceKDE  # noqa: E402
from tests import kde_cases, kde_oracle  # noqa: E402


def main():
    print("scaled error max |L - L_ld| / max(1, |L_ld|) over the finite entries; N = 197, M = 259 (tests/kde_cases.py: matrix_case)")
    print(f"{'kernel':13s} {'d':>2s} {'D':>2s} {'C':>3s} {'CB':>3s} {'float64 oracle':>15s} {'device chunks=1':>16s} {'device chunks=2':>16s}")
    worst = {}
    for kernel, d, C in kde_cases.matrix_cases():
        X, V, Q, h = kde_cases.matrix_case(kernel, d, C)
        L, _ = kde_cases.matrix_oracle(kernel, d, C)
        base = kde_cases.scaled_error(kde_oracle.log_density(X, V, Q, kernel, h), L)
        dev = []
        with DeviceKDE(X, kernel, h) as dk:
            dk.set_weights(V)
            for mc in (1, 2):
                dk.set_option("max_chunks", mc)
                dev.append(kde_cases.scaled_error(dk.log_density(Q), L))
        D = d if (kernel in kde_cases.UNBOUNDED and d <= 3) else 0
        print(f"{kernel:13s} {d:2d} {D:2d} {C:3d} {kde_cases.C_TO_CB[C]:3d} {base:15.3e} {dev[0]:16.3e} {dev[1]:16.3e}")
        w = worst.setdefault(kernel, [0.0, 0.0])
        w[0], w[1] = max(w[0], base), max(w[1], *dev)
    print()
    print(f"{'kernel':13s} {'float64 oracle max':>19s} {'device max':>12s}")
    for kernel, (b, v) in worst.items():
        print(f"{kernel:13s} {b:19.3e} {v:12.3e}")


if __name__ == "__main__":
    main()
