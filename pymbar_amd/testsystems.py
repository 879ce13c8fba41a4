"""Seeded synthetic inputs for the MBAR solver path (numpy only; no GPU needed).

These are the input generators of SURVEY.md section 8(d).  The harmonic and exponential ladders
draw their samples exactly the way the reference test systems do -- legacy
``np.random.seed(seed)`` followed by one ``normal``/``exponential`` draw per state, in state
order (pymbar/testsystems/harmonic_oscillators.py:154-188,
pymbar/testsystems/exponential_distributions.py) -- so a given ``seed`` yields bit-identical
``u_kn`` here and in the reference (checked in tests/golden/make_golden.py).

Analytical answers (harmonic_oscillators.py:92-96): ``f_k = -1/2 ln(2 pi / (beta K_k))``.
"""
import numpy as np

__all__ = [
    "harmonic_u_kn",
    "harmonic_free_energies",
    "harmonic_scan_family",
    "harmonic_linear_family",
    "exponential_u_kn",
    "exponential_free_energies",
    "config1",
    "config2",
    "config3_params",
    "config5",
    "ladder_params",
    "correlated_timeseries_example",
]


def harmonic_u_kn(O_k, K_k, N_k, seed=None, beta=1.0):
    """Sample ``N_k[k]`` points from each 1-D harmonic state and evaluate every state on them.

    Returns ``(x_n, u_kn, N_k, s_n)`` with ``u_kn[l, n] = beta/2 * K_l * (x_n - O_l)**2``.
    """
    O_k = np.asarray(O_k, dtype=np.float64)
    K_k = np.asarray(K_k, dtype=np.float64)
    N_k = np.array(N_k, dtype=int)
    if not (len(O_k) == len(K_k) == len(N_k)):
        raise ValueError("O_k, K_k and N_k must have one entry per state")
    np.random.seed(seed)
    n_tot = int(N_k.sum())
    x_n = np.empty(n_tot, dtype=np.float64)
    s_n = np.empty(n_tot, dtype=int)
    start = 0
    for k, n in enumerate(N_k):
        sigma = (beta * K_k[k]) ** -0.5
        x_n[start : start + n] = np.random.normal(loc=O_k[k], scale=sigma, size=n)
        s_n[start : start + n] = k
        start += n
    u_kn = np.empty((len(O_k), n_tot), dtype=np.float64)
    for l in range(len(O_k)):
        u_kn[l] = beta * 0.5 * K_k[l] * (x_n - O_k[l]) ** 2.0
    return x_n, u_kn, N_k, s_n


def harmonic_free_energies(K_k, beta=1.0, subtract_component=0):
    fe = -0.5 * np.log(2 * np.pi / (beta * np.asarray(K_k, dtype=np.float64)))
    if subtract_component is not None:
        fe = fe - fe[subtract_component]
    return fe


def harmonic_scan_family(x_n, O_l, K_l, beta=1.0):
    """The harmonic oscillators ``(O_l, K_l)`` as a linear family over the samples ``x_n`` for ``MBAR.compute_scan``:
    ``(basis_bn, coeff_lb, offset_l)`` with basis ``{x^2, x}``, so that ``coeff_lb @ basis_bn + offset_l[:, None]`` is
    ``u_ln[l, n] = beta/2 * K_l * (x_n - O_l)**2``."""
    x_n = np.asarray(x_n, dtype=np.float64)
    O_l = np.atleast_1d(np.asarray(O_l, dtype=np.float64))
    K_l = np.atleast_1d(np.asarray(K_l, dtype=np.float64))
    if O_l.shape != K_l.shape or O_l.ndim != 1:
        raise ValueError("O_l and K_l must have one entry per member")
    basis_bn = np.stack([x_n * x_n, x_n])
    coeff_lb = np.stack([0.5 * beta * K_l, -beta * K_l * O_l], axis=1)
    offset_l = 0.5 * beta * K_l * O_l * O_l
    return basis_bn, coeff_lb, offset_l


def harmonic_linear_family(O_k, K_k, N_k, seed=None, beta=1.0):
    """The harmonic-oscillator system of :func:`harmonic_u_kn` (same draws for the same ``seed``) as a linear family for
    ``MBAR.from_linear``, without the dense matrix: ``(basis_bn, coeff_kb, offset_k)`` with the basis ``[x^2, x]`` (``x_n`` is
    ``basis_bn[1]``), since ``u_k = beta (K_k / 2 x^2 - K_k O_k x + K_k O_k^2 / 2)``."""
    O_k = np.asarray(O_k, dtype=np.float64)
    K_k = np.asarray(K_k, dtype=np.float64)
    N_k = np.array(N_k, dtype=int)
    if not (len(O_k) == len(K_k) == len(N_k)):
        raise ValueError("O_k, K_k and N_k must have one entry per state")
    np.random.seed(seed)
    x_n = np.empty(int(N_k.sum()), dtype=np.float64)
    start = 0
    for k, n in enumerate(N_k):
        x_n[start : start + n] = np.random.normal(loc=O_k[k], scale=(beta * K_k[k]) ** -0.5, size=n)
        start += n
    return harmonic_scan_family(x_n, O_k, K_k, beta=beta)


def exponential_u_kn(rates, N_k, seed=None, beta=1.0):
    """Exponential-distribution ladder: ``u_kn[l, n] = beta * rate_l * x_n``."""
    rates = np.asarray(rates, dtype=np.float64)
    N_k = np.array(N_k, dtype=int)
    np.random.seed(seed)
    n_tot = int(N_k.sum())
    x_n = np.empty(n_tot, dtype=np.float64)
    s_n = np.empty(n_tot, dtype=int)
    start = 0
    for k, n in enumerate(N_k):
        x_n[start : start + n] = np.random.exponential(scale=rates[k] ** -1.0, size=n)
        s_n[start : start + n] = k
        start += n
    u_kn = np.empty((len(rates), n_tot), dtype=np.float64)
    for l in range(len(rates)):
        u_kn[l] = beta * rates[l] * x_n
    return x_n, u_kn, N_k, s_n


def exponential_free_energies(rates, beta=1.0, subtract_component=0):
    fe = np.log(beta * np.asarray(rates, dtype=np.float64))
    if subtract_component is not None:
        fe = fe - fe[subtract_component]
    return fe


def ladder_params(K):
    """Generator G of SURVEY.md 8(d): ``O_k = linspace(0, 4, K)``, ``K_k = linspace(1, 3, K)``."""
    return np.linspace(0.0, 4.0, K), np.linspace(1.0, 3.0, K)


def config1(seed=0):
    """BASELINE.json config 1: HarmonicOscillatorsTestCase defaults, K=5, N=5000."""
    O_k = (0, 1, 2, 3, 4)
    K_k = (1, 2, 4, 8, 16)
    return harmonic_u_kn(O_k, K_k, [1000] * 5, seed=seed) + (np.array(O_k, float), np.array(K_k, float))


def config2(seed=0, K=32, N=1_000_000):
    """BASELINE.json config 2: synthetic Gaussian ladder K=32, N=1e6 (equal N_k)."""
    O_k, K_k = ladder_params(K)
    return harmonic_u_kn(O_k, K_k, [N // K] * K, seed=seed) + (O_k, K_k)


def config3_params(K=128, N=10_000_000):
    """BASELINE.json config 3/4 parameters (the matrix itself is generated on the device)."""
    O_k, K_k = ladder_params(K)
    N_k = np.full(K, N // K, dtype=np.int64)
    return O_k, K_k, N_k


def config5(seed=0, K=40, n_per_state=2500, unsampled=(7, 23)):
    """BASELINE.json config 5: an alchemical-shaped ladder (K=40, N ~ 1e5) with force constants
    spaced geometrically 1 -> 16, small offsets, and two states carrying no samples."""
    K_k = np.geomspace(1.0, 16.0, K)
    O_k = np.linspace(0.0, 1.5, K)
    N_k = np.full(K, n_per_state, dtype=int)
    for k in unsampled:
        N_k[k] = 0
    return harmonic_u_kn(O_k, K_k, N_k, seed=seed) + (O_k, K_k)


def correlated_timeseries_example(N=10000, tau=5.0, seed=None):
    """A Gaussian AR(1) series of length N with correlation time tau (Janke, Eq. 41), as float32.

    Bit-identical to ``pymbar.testsystems.correlated_timeseries_example`` for the same seed: ``N`` standard normal draws from
    ``np.random.RandomState(seed)``, then ``A_0 = e_0`` and ``A_n = rho A_(n-1) + sigma e_n`` evaluated in fp64 and stored as float32
    after every step, with ``rho = exp(-1 / tau)`` and ``sigma = sqrt(1 - rho^2)``."""
    e = np.random.RandomState(seed).randn(N)
    rho = float(np.exp(-1.0 / tau))
    sigma = float(np.sqrt(1.0 - rho * rho))
    out = np.zeros([N], np.float32)
    if N == 0:
        return out
    prev = float(np.float32(e[0]))
    out[0] = prev
    for n in range(1, N):
        prev = float(np.float32(rho * prev + sigma * float(e[n])))
        out[n] = prev
    return out


def gaussian_work_example(N_F=200, N_R=200, mu_F=2.0, DeltaF=None, sigma_F=1.0, seed=None):
    """Forward and reverse Gaussian work samples related by the Crooks fluctuation theorem, as [w_F, w_R].

    Bit-identical to ``pymbar.testsystems.gaussian_work_example`` for the same arguments: exactly one of ``mu_F`` and ``DeltaF``
    is given and fixes the other through DeltaF = mu_F - sigma_F^2 / 2 (Zwanzig); the reverse distribution has mean
    -mu_F + sigma_F^2 and width sigma_F exp(mu_F - sigma_F^2 / 2 - DeltaF); ``N_F`` then ``N_R`` standard normal draws from
    ``np.random.RandomState(seed)`` are scaled and shifted (w = z sigma + mu)."""
    if (mu_F is not None) and (DeltaF is not None):
        raise ValueError("mu_F and DeltaF are not independent, and cannot both be specified; one must be set to None.")
    if (mu_F is None) and (DeltaF is None):
        raise ValueError("Either mu_F or DeltaF must be specified.")
    if mu_F is None:
        mu_F = DeltaF + sigma_F**2 / 2.0
    if DeltaF is None:
        DeltaF = mu_F - sigma_F**2 / 2.0
    rng = np.random.RandomState(seed)
    mu_R = -mu_F + sigma_F**2
    sigma_R = sigma_F * np.exp(mu_F - sigma_F**2 / 2.0 - DeltaF)
    w_F = rng.randn(N_F) * sigma_F + mu_F
    w_R = rng.randn(N_R) * sigma_R + mu_R
    return [w_F, w_R]
