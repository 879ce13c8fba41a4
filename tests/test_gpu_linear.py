"""The linear policy of ``k_fill_rows`` (mbar_k_family.hip) / ``mbar_ctx_fill_linear_rows`` / ``MBAR.from_linear`` on an MI355X.

The exact statement of the kernel is ``u_model`` (tests/family_standin.py): the scan passes' fma chain -- from the offset, ``b``
ascending, one fma per term -- evaluated with the exact ``fma`` of tests/device_math_model.py.  "Same bits" is ``np.array_equal``.
The class tests compare with ``MBAR(u_model, N_k)`` on the same device: the same resident matrix, so the same bits in everything
computed from it."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import pymbar_amd  # noqa: E402
from pymbar_amd import _lib, testsystems  # noqa: E402
from pymbar_amd.device import DeviceMatrix, LoopbackGroup  # noqa: E402
from pymbar_amd.distributed import shard_bounds  # noqa: E402
from pymbar_amd.utils import DataError, ParameterError  # noqa: E402
from tests.conftest import load_golden  # noqa: E402
from tests.family_standin import u_model  # noqa: E402
from tests.test_gpu_loopback import run_ranks  # noqa: E402

# The geometry of k_fill_rows (mbar_scan.h): a lane owns 2 adjacent columns, 256 lanes per workgroup, at most 2048
# workgroups along the columns (the pairs go round them), 128 rows per row group (grid.y), the row loop unrolled by 4.  One pass of
# the largest grid covers 2048 * 256 * 2 = 1048576 columns; N2 is one more than twice that: a full pass, a full second pass and
# the odd last column.
FILL_THREADS, FILL_MAX_BLOCKS, FILL_ROWS = 256, 2048, 128
N2 = 2 * (FILL_MAX_BLOCKS * FILL_THREADS * 2) + 1

SHAPES = [
    (1, 1, 1),        # no whole pair at all: only the odd-column path
    (2, 3, 2),        # one pair + the odd column
    (5, 255, 3),      # odd N, last pair tile of the only workgroup not full
    (5, 256, 8),      # even N, B = 8
    (5, 257, 8),      # one column past a multiple of 16 (the row pitch grows by a tile)
    (33, 1000, 4),    # two workgroups along the columns (500 pairs), rows = 8 x 4 + 1
    (128, 513, 2),    # exactly one full row group; 256 pairs = one full workgroup, + the odd column
    (129, 511, 8),    # row group seam: a second group of one row; 255 pairs
    (131, 64, 3),     # second row group of 3 rows: the remainder of the row loop's unroll by 4
    (300, 77, 5),     # three row groups, the last of 44 rows; K > 256
    (2, 1026, 1),     # 513 pairs: a third workgroup with one pair
    (2, N2, 1),       # the grid-stride loop: full pass, second full pass, tail
]


def family(K, N, B, seed=None, offset=True):
    rng = np.random.default_rng(1000 * K + 10 * B + (N % 997) if seed is None else seed)
    basis = rng.normal(size=(B, N)) * rng.uniform(1.0, 10.0, size=(B, 1))
    coeff = rng.normal(size=(K, B)) * rng.uniform(1.0, 10.0, size=(K, 1))
    off = rng.normal(size=K) * 5.0 if offset else None
    return basis, coeff, off


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "K%d-N%d-B%d" % s)
def test_fill_has_the_models_bits(shape):
    K, N, B = shape
    basis, coeff, off = family(K, N, B)
    with DeviceMatrix.from_linear(basis, coeff, off) as dm:
        assert dm.shape == (K, N)
        got = dm.to_host()
    want = u_model(basis, coeff, off)
    assert np.array_equal(got, want), f"{int(np.sum(got != want))} of {got.size} entries differ"


def test_offset_none_is_zeros():
    basis, coeff, _ = family(5, 257, 3)
    with DeviceMatrix.from_linear(basis, coeff, None) as a, DeviceMatrix.from_linear(basis, coeff, np.zeros(5)) as b:
        ua, ub = a.to_host(), b.to_host()
    assert np.array_equal(ua, ub) and np.array_equal(ua, u_model(basis, coeff, None))


@pytest.mark.parametrize("row0,nrows", [(0, 1), (3, 2), (6, 1), (1, 5)])
def test_partial_fill_leaves_the_other_rows_alone(row0, nrows):
    K, N = 7, 301
    R = np.random.default_rng(5).normal(size=(K, N))
    basis, coeff, off = family(nrows, N, 3, seed=row0 + 11)
    with DeviceMatrix.from_host(R) as dm:
        v0 = dm._version
        dm.fill_linear_rows(row0, basis, coeff, off)
        assert dm._version > v0
        got = dm.to_host()
    want = R.copy()
    want[row0:row0 + nrows] = u_model(basis, coeff, off)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("shape", [(5, 257, 8), (128, 513, 2)], ids=lambda s: "K%d-N%d-B%d" % s)
def test_padding_is_untouched(shape):
    """The sweeps read whole tiles: with anything but zeros behind column N (or in the rows behind K) they would not return the
    bits they return on an uploaded copy of the same matrix."""
    K, N, B = shape
    basis, coeff, off = family(K, N, B)
    rng = np.random.default_rng(3)
    N_k = np.full(K, N // K)
    N_k[: N - N_k.sum()] += 1
    f = rng.normal(size=K)
    out = []
    for make in (lambda: DeviceMatrix.from_linear(basis, coeff, off), lambda: DeviceMatrix.from_host(u_model(basis, coeff, off))):
        with make() as dm:
            dm.set_Nk(N_k)
            out.append((dm.eval(f, gram=True), dm.lognum(f), dm.gram_w(f)))
    (ea, la, ga), (eb, lb, gb) = out
    for a, b in zip(ea + (la,) + ga, eb + (lb,) + gb):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("n0,n1", [(0, 129), (129, 301), (7, 8)])
def test_column_shards(n0, n1):
    basis, coeff, off = family(6, 301, 4)
    with DeviceMatrix.from_linear(basis, coeff, off, columns=(n0, n1)) as dm:
        assert dm.shape == (6, n1 - n0)
        got = dm.to_host()
    assert np.array_equal(got, u_model(basis, coeff, off)[:, n0:n1])


def test_errors_leave_the_context_usable():
    K, N = 4, 37
    basis, coeff, off = family(K, N, 2)
    dp = C.POINTER(C.c_double)
    with DeviceMatrix.empty(K, N) as dm:
        with pytest.raises(ValueError):
            dm.fill_linear_rows(0, basis[:0], coeff[:, :0])                                        # B = 0
        with pytest.raises(ValueError):
            dm.fill_linear_rows(0, np.tile(basis[:1], (9, 1)), np.tile(coeff[:, :1], (1, 9)))      # B = 9
        with pytest.raises(ValueError):
            dm.fill_linear_rows(0, basis[:, :N - 1], coeff, off)                                   # the basis does not cover the shard
        with pytest.raises(DataError):
            dm.fill_linear_rows(0, basis, np.where(coeff == coeff[1, 1], np.nan, coeff), off)
        with pytest.raises(_lib.MbarHipError):
            dm.fill_linear_rows(2, basis, coeff[:3], off[:3])                                      # rows [2, 5) of 4
        # the library's own checks, behind the Python ones
        big = np.ascontiguousarray(np.tile(basis[:1], (9, 1)))
        cf9 = np.ascontiguousarray(np.tile(coeff[:, :1], (1, 9)))
        args = lambda B, ld, col0, b=big, c=cf9: (dm._ctx, 0, K, B, b.ctypes.data_as(dp), ld, col0, c.ctypes.data_as(dp), None)  # noqa: E731
        for bad in (args(0, N, 0), args(9, N, 0), args(2, N - 1, 0), args(2, N, 1), args(2, N, -1)):
            assert dm._lib.mbar_ctx_fill_linear_rows(*bad) == -1
        assert dm._lib.mbar_ctx_fill_linear_rows(dm._ctx, 0, K, 2, None, N, 0, cf9.ctypes.data_as(dp), None) == -1
        assert dm._lib.mbar_ctx_fill_linear_rows(dm._ctx, 0, K, 2, big.ctypes.data_as(dp), N, 0, None, None) == -1
        assert dm._lib.mbar_ctx_fill_linear_rows(dm._ctx, K, 0, 2, big.ctypes.data_as(dp), N, 0, cf9.ctypes.data_as(dp), None) == 0  # nrows = 0
        assert np.array_equal(dm.to_host(), np.zeros((K, N)))
        dm.fill_linear_rows(0, basis, coeff, off)
        assert np.array_equal(dm.to_host(), u_model(basis, coeff, off))


def test_extension_contexts_are_refused():
    basis, coeff, off = family(120, 64, 2)
    dp = C.POINTER(C.c_double)
    with DeviceMatrix.from_linear(basis, coeff, off) as dm:
        ext = dm.extend(16)
        assert ext is not None
        try:
            rc = ext._lib.mbar_ctx_fill_linear_rows(ext._ctx, 0, 16, 2, basis.ctypes.data_as(dp), 64, 0, coeff.ctypes.data_as(dp), None)
            assert rc not in (0, -1) and "extension" in _lib.last_error(ext._ctx)
        finally:
            ext.close()
        assert np.array_equal(dm.to_host(), u_model(basis, coeff, off))


# ---- the class, end to end ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def config1():
    x_n, u_kn, N_k, _, O_k, K_k = testsystems.config1(seed=0)
    basis, coeff, offset = testsystems.harmonic_linear_family(O_k, K_k, N_k, seed=0)
    return dict(x_n=x_n, N_k=N_k, basis=basis, coeff=coeff, offset=offset, u_model=u_model(basis, coeff, offset), O_k=O_k, K_k=K_k)


def both(c, **kw):
    return (pymbar_amd.MBAR.from_linear(c["basis"], c["coeff"], c["N_k"], offset_k=c["offset"], **kw),
            pymbar_amd.MBAR(c["u_model"], c["N_k"], **kw))


def assert_same_dict(a, b):
    assert set(a) == set(b)
    for key in a:
        assert np.array_equal(a[key], b[key], equal_nan=True), key


@pytest.mark.parametrize("protocol", [None, "robust"])
def test_class_matches_the_dense_constructor(config1, protocol):
    m, d = both(config1, solver_protocol=protocol)
    try:
        assert np.array_equal(m.f_k, d.f_k)
        np.testing.assert_allclose(m.f_k, load_golden("config1_ho_K5_N5000.npz")["f_k"], rtol=0, atol=1e-10)
        assert_same_dict(m.compute_free_energy_differences(), d.compute_free_energy_differences())
        assert m._u_kn is None  # nothing so far read the host matrix
        u_ln = config1["u_model"][:3] * 1.1 + 0.3
        assert_same_dict(m.compute_perturbed_free_energies(u_ln), d.compute_perturbed_free_energies(u_ln))
        assert_same_dict(m.compute_expectations(config1["x_n"]), d.compute_expectations(config1["x_n"]))
        assert np.array_equal(m.u_kn, config1["u_model"]) and m.u_kn is m.u_kn
        assert m.upload_stats["upload_s"] > 0 and set(m.upload_stats) == {"upload_s", "upload_GBps"}
    finally:
        m.close()
        d.close()


@pytest.mark.parametrize("bootstrap_rng", ["reference", "device"])
def test_bootstraps_match_the_dense_constructor(config1, bootstrap_rng):
    m, d = both(config1, n_bootstraps=3, rseed=7, bootstrap_rng=bootstrap_rng)
    try:
        assert m.bootstrap_rng_used == d.bootstrap_rng_used == bootstrap_rng
        assert np.array_equal(m.f_k, d.f_k) and np.array_equal(m.f_k_boots, d.f_k_boots)
        assert np.array_equal(m.bootstrap_rints, d.bootstrap_rints)
        assert_same_dict(m.compute_free_energy_differences(uncertainty_method="bootstrap"),
                         d.compute_free_energy_differences(uncertainty_method="bootstrap"))
    finally:
        m.close()
        d.close()


def test_scan_defaults_to_the_constructors_basis(config1):
    c = config1
    m = pymbar_amd.MBAR.from_linear(c["basis"], c["coeff"], c["N_k"], offset_k=c["offset"], relative_tolerance=1e-12)
    try:
        O_l, K_l = np.linspace(0.0, 4.0, 9), np.linspace(1.0, 16.0, 9)
        _, coeff_l, offset_l = testsystems.harmonic_scan_family(c["x_n"], O_l, K_l)
        A = np.stack([c["x_n"], c["x_n"] ** 2])
        assert_same_dict(m.compute_scan(None, coeff_l, offset_l, A_qn=A), m.compute_scan(m.basis_bn, coeff_l, offset_l, A_qn=A))
        assert_same_dict(m.compute_scan(coeff_lb=coeff_l, offset_l=offset_l), m.compute_scan(c["basis"], coeff_l, offset_l))
        label = np.clip(np.floor(c["x_n"] + 1.0), 0, 5).astype(np.int32)
        assert_same_dict(m.compute_scan_fes(None, coeff_l, offset_l, sample_label=label),
                         m.compute_scan_fes(m.basis_bn, coeff_l, offset_l, sample_label=label))
        # a member with a sampled state's coefficients IS that state (its u has the state's bits): its f is the state's f_k
        own = m.compute_scan(coeff_lb=c["coeff"], offset_l=c["offset"], compute_uncertainty=False)
        print("max |f_scan - f_k| =", np.max(np.abs(own["f"] - m.f_k)))
        np.testing.assert_allclose(own["f"], m.f_k, rtol=0, atol=2e-11)
        assert m._u_kn is None
    finally:
        m.close()
    d = pymbar_amd.MBAR(c["u_model"], c["N_k"])
    try:
        with pytest.raises(ParameterError, match="from_linear"):
            d.compute_scan(None, c["coeff"], c["offset"])
    finally:
        d.close()


def test_more_than_128_states():
    K, per = 129, 4
    O_k, K_k = testsystems.ladder_params(K)
    N_k = np.full(K, per)
    basis, coeff, offset = testsystems.harmonic_linear_family(O_k, K_k, N_k, seed=1)
    assert basis.shape == (2, 516)
    m = pymbar_amd.MBAR.from_linear(basis, coeff, N_k, offset_k=offset)
    d = pymbar_amd.MBAR(u_model(basis, coeff, offset), N_k)
    try:
        assert np.all(np.isfinite(m.f_k)) and np.array_equal(m.f_k, d.f_k)
        assert_same_dict(m.compute_free_energy_differences(), d.compute_free_energy_differences())
        with pytest.raises(ParameterError, match="128"):
            m.compute_scan(coeff_lb=coeff[:3], offset_l=offset[:3])
    finally:
        m.close()
        d.close()


def test_two_logical_ranks(config1):
    """Each rank builds its column shard from the whole basis and its shard origin: the adaptive solve across the two is the solve
    across two ranks that uploaded the same shards."""
    c, K, N = config1, 5, 5000

    def solve(make):
        with LoopbackGroup(2) as grp:
            def worker(r):
                with make(shard_bounds(N, r, 2)) as dm:
                    dm.set_loopback(grp, r)
                    dm.set_Nk(c["N_k"])
                    f, res = dm.solve_adaptive(np.zeros(K), tol=1e-12, maxiter=200, history_rows=200)
                    dm.comm_destroy()
                    return f, res["iterations"], res["history"]

            return run_ranks(2, worker)

    lin = solve(lambda cols: DeviceMatrix.from_linear(c["basis"], c["coeff"], c["offset"], columns=cols))
    up = solve(lambda cols: DeviceMatrix.from_host(c["u_model"], columns=cols))
    for (fa, ia, ha), (fb, ib, hb) in zip(lin, up):
        assert np.array_equal(fa, fb) and ia == ib and np.array_equal(ha, hb)
    assert np.array_equal(lin[0][0], lin[1][0])
