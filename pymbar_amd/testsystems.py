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


def temperature_ladder_family(E_n, beta_l):
    """The potential energies ``E_n`` reweighted to the inverse temperatures ``beta_l`` as a linear family for ``MBAR.compute_scan`` and
    ``MBAR.compute_scan_entropy_and_enthalpy``: ``(basis_bn, coeff_lb, offset_l)`` with the one basis vector ``E_n`` and ``coeff =
    beta_l``, so that ``u_ln[l, n] = beta_l E_n``.  On such a ladder ``var_u`` of the latter method is ``C_v / k_B``."""
    E_n = np.asarray(E_n, dtype=np.float64)
    beta_l = np.atleast_1d(np.asarray(beta_l, dtype=np.float64))
    if E_n.ndim != 1 or beta_l.ndim != 1:
        raise ValueError("E_n must have one entry per sample and beta_l one per member")
    return E_n[None, :].copy(), beta_l[:, None].copy(), np.zeros(len(beta_l))


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


def family_u_kn(basis_bn, coeff_kb, offset_k=None, center_kb=None, harmonic_b=None, period_b=None):
    """The dense ``(K, N)`` matrix of a family with harmonic terms (``MBAR.from_family``) in plain numpy: ``u[k, n] = offset_k[k] +
    sum_b term_b``, a linear term ``coeff_kb[k, b] basis_bn[b, n]``, a harmonic one ``coeff_kb[k, b] w(basis_bn[b, n] - center_kb[k,
    b])^2`` with the minimum image ``w(d) = d - P rint(d / P)`` for ``P = period_b[b] > 0`` and ``w(d) = d`` for 0.  The statement of
    the family, not the device's rounding: the kernels evaluate one fixed chain of fused operations."""
    basis_bn = np.asarray(basis_bn, dtype=np.float64)
    coeff_kb = np.asarray(coeff_kb, dtype=np.float64)
    K, B = coeff_kb.shape
    u = np.zeros((K, basis_bn.shape[1])) + (0.0 if offset_k is None else np.asarray(offset_k, dtype=np.float64)[:, None])
    harmonic_b = np.zeros(B, dtype=bool) if harmonic_b is None else np.asarray(harmonic_b, dtype=bool)
    period_b = np.zeros(B) if period_b is None else np.asarray(period_b, dtype=np.float64)
    for b in range(B):
        if harmonic_b[b]:
            d = basis_bn[b][None, :] - np.asarray(center_kb, dtype=np.float64)[:, b:b + 1]
            if period_b[b] > 0:
                d = d - period_b[b] * np.rint(d / period_b[b])
            u += coeff_kb[:, b:b + 1] * d * d
        else:
            u += coeff_kb[:, b:b + 1] * basis_bn[b][None, :]
    return u


def periodic_umbrella_family(K=6, n_per_state=300, kappa=0.002, barrier=1.5, beta_k=None, seed=0):
    """Umbrella sampling of a torsion ``chi`` (degrees, period 360) on the cosine potential ``E(chi) = barrier (1 + cos(3 chi))``:
    ``K`` umbrellas ``u_k = beta_k [E + kappa / 2 wrap(chi - chi0_k)^2]`` with centres spread evenly over ``[-180, 180)``,
    ``n_per_state`` samples each, drawn from the exact density of their umbrella by inversion on a grid of 0.01 degrees.  Returns
    ``(basis_bn, coeff_kb, center_kb, harmonic_b, period_b, offset_k, N_k)`` as ``MBAR.from_family`` takes them: the basis is ``[E_n,
    chi_n]``, the first term linear (``beta_k``), the second harmonic with period 360 (``beta_k kappa / 2`` around ``chi0_k``).
    The umbrellas next to +-180 hold samples on both sides of the seam."""
    rng = np.random.default_rng(seed)
    chi0_k = -180.0 + 360.0 * (np.arange(K) + 0.5) / K
    beta_k = np.ones(K) if beta_k is None else np.asarray(beta_k, dtype=np.float64)
    energy = lambda chi: barrier * (1.0 + np.cos(np.deg2rad(3.0 * chi)))
    edges = np.linspace(-180.0, 180.0, 36001)
    mid = 0.5 * (edges[1:] + edges[:-1])
    chi_n = np.empty(K * n_per_state)
    for k in range(K):
        d = mid - chi0_k[k]
        d -= 360.0 * np.rint(d / 360.0)
        cdf = np.cumsum(np.exp(-beta_k[k] * (energy(mid) + 0.5 * kappa * d * d)))
        cell = np.searchsorted(cdf, rng.random(n_per_state) * cdf[-1])
        chi_n[k * n_per_state:(k + 1) * n_per_state] = edges[cell] + rng.random(n_per_state) * (edges[1] - edges[0])
    basis_bn = np.stack([energy(chi_n), chi_n])
    coeff_kb = np.stack([beta_k, 0.5 * beta_k * kappa], axis=1)
    center_kb = np.stack([np.zeros(K), chi0_k], axis=1)
    return (basis_bn, coeff_kb, center_kb, np.array([False, True]), np.array([0.0, 360.0]), np.zeros(K),
            np.full(K, n_per_state, dtype=np.int64))


def umbrella_2d_family(x_n, u_n, centers, Ku, beta=1.0):
    """A 2-D umbrella system as a LINEAR family over the basis ``[u_n, x^2 + y^2, x, y]``: state ``k`` is ``beta [u_n + Ku / 2 |x_n -
    centers[k]|^2]``, the system of the reference's ``fes_2d`` test (fixture (b) of tests/golden/fes_kde.npz).  ``x_n`` is ``(N, 2)``,
    ``u_n`` the unbiased reduced potential, ``centers`` ``(K, 2)``.  Returns ``(basis_bn, coeff_kb, offset_k)`` as ``MBAR.from_linear``
    and the scan methods take them; a temperature member ``beta' u_n`` of a scan is the row ``[beta', 0, 0, 0]``."""
    x_n = np.asarray(x_n, dtype=np.float64)
    centers = np.atleast_2d(np.asarray(centers, dtype=np.float64))
    if x_n.ndim != 2 or x_n.shape[1] != 2 or centers.shape[1] != 2:
        raise ValueError("x_n must be (N, 2) and centers (K, 2)")
    K = len(centers)
    basis_bn = np.stack([np.asarray(u_n, dtype=np.float64), x_n[:, 0] ** 2 + x_n[:, 1] ** 2, x_n[:, 0], x_n[:, 1]])
    coeff_kb = np.empty((K, 4))
    coeff_kb[:, 0] = beta
    coeff_kb[:, 1] = 0.5 * beta * Ku
    coeff_kb[:, 2] = -beta * Ku * centers[:, 0]
    coeff_kb[:, 3] = -beta * Ku * centers[:, 1]
    offset_k = 0.5 * beta * Ku * np.sum(centers * centers, axis=1)
    return basis_bn, coeff_kb, offset_k


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
