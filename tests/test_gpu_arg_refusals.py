"""Every array a Python face hands to the library is length-checked first (``pymbar_amd._lib.f64`` / ``labels_i32``): an array one
entry too short or too long is refused in Python -- no library call is made with it -- and the object that refused it then answers
the correct call with the bits a fresh object gives.  The state of a ``DeviceMatrix`` that used to appear with the first ``set_*``
call is there from the constructor on.

The shapes are the smallest there are (3 states, 5 samples, 2 bins, 1 basis vector, 2 members; a batch of two problems of 2 states
and 4 samples): what is under test is the argument handling, not a kernel."""
import contextlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from pymbar_amd import _lib, batch  # noqa: E402
from pymbar_amd.device import DeviceMatrix  # noqa: E402
from pymbar_amd.utils import ParameterError  # noqa: E402

K, N, NBINS, B, L = 3, 5, 2, 1, 2
RNG = np.random.default_rng(20240607)
U = RNG.normal(size=(K, N))
N_K = np.array([2.0, 2.0, 1.0])
F = np.array([0.0, 0.3, -0.2])
LABEL = np.array([0, 1, -1, 1, 0])
V_N = RNG.normal(size=N)
BASIS = RNG.normal(size=(B, N))
T_QN = RNG.normal(size=(1, N))
COEFF = np.array([[0.5], [1.5]])
OFFSET = np.array([0.1, -0.1])
F_SCAN = np.array([0.2, 0.4])
CUM = np.array([0, 2, 4, 5])
ORDER = np.array([3, 0, 4, 1, 2])
KE = 126  # appended rows of the extended matrix: 129 rows in all, the fewest the library sweeps as one panel
ROWS_E = RNG.normal(size=(KE, N))
F_E = np.concatenate([F, RNG.normal(size=KE)])


class _NoCalls:
    def __getattr__(self, name):
        def call(*args):
            raise AssertionError(f"{name} was called with an argument that should have been refused")

        return call


@contextlib.contextmanager
def refused(*objs, error=ValueError):
    """The block raises ``error`` without a call into the library through one of ``objs``."""
    libs = [obj._lib for obj in objs]
    for obj in objs:
        obj._lib = _NoCalls()
    try:
        with pytest.raises(error):
            yield
    finally:
        for obj, lib in zip(objs, libs):
            obj._lib = lib


def wrong(a, axes=(0,)):
    """``a`` one entry too short and one too long along each of ``axes``."""
    a = np.asarray(a)
    for ax in axes:
        yield np.delete(a, -1, axis=ax)
        yield np.concatenate([a, np.take(a, [-1], axis=ax)], axis=ax)


def flat(x):
    if x is None:
        return []
    if isinstance(x, (tuple, list)):
        return [a for y in x for a in flat(y)]
    return [np.asarray(x)]


def assert_same(got, want, what):
    got, want = flat(got), flat(want)
    assert len(got) == len(want) and len(got) > 0, what
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and np.array_equal(a, b, equal_nan=True), f"{what}: output {i} differs from a fresh object's"


def matrix():
    """A resident matrix with everything set that the calls below read."""
    dm = DeviceMatrix.from_host(U)
    dm.set_Nk(N_K)
    dm.set_bins(NBINS, LABEL, V_N)
    dm.set_scan(BASIS)  # (no observables: the binned passes take none)
    dm.set_scan_bins(NBINS, LABEL)
    return dm


def _offset_eval(dm, f):
    dm.set_objective_offset(f)
    return dm.eval(F, use_offset=True)


# ---- DeviceMatrix: the free energies ------------------------------------------------------------------------------------------
F_CALLS = {
    "lognum": lambda dm, f: dm.lognum(f),
    "logden": lambda dm, f: dm.logden(f),
    "logw_kn": lambda dm, f: dm.logw_kn(f),
    "w_kn": lambda dm, f: dm.w_kn(f),
    "gram_w": lambda dm, f: dm.gram_w(f),
    "lognum_cached": lambda dm, f: dm.lognum_cached(f),
    "gram_w_cached": lambda dm, f: dm.gram_w_cached(f),
    "set_objective_offset": _offset_eval,
    "solve_adaptive": lambda dm, f: dm.solve_adaptive(f, tol=1e-10, maxiter=100)[0],
    "solve_sci": lambda dm, f: dm.solve_sci(f, tol=1e-10, maxiter=100)[0],
    "eval": lambda dm, f: dm.eval(f, gram=True),
    "bin_lognum": lambda dm, f: dm.bin_lognum(f),
    "bin_gram_w": lambda dm, f: dm.bin_gram_w(f, np.zeros(NBINS)),
    "scan_lognum": lambda dm, f: dm.scan_lognum(f, COEFF, OFFSET),
    "scan_gram_w": lambda dm, f: dm.scan_gram_w(f, COEFF, OFFSET, F_SCAN),
    "scan_energy_lognum": lambda dm, f: dm.scan_energy_lognum(f, COEFF, OFFSET),
    "scan_energy_gram_w": lambda dm, f: dm.scan_energy_gram_w(f, COEFF, OFFSET, F_SCAN),
    "scan_bin_lognum": lambda dm, f: dm.scan_bin_lognum(f, COEFF, OFFSET),
    "scan_bin_gram_w": lambda dm, f: dm.scan_bin_gram_w(f, COEFF, OFFSET, np.zeros((L, NBINS))),
}


@pytest.mark.parametrize("name", list(F_CALLS))
def test_matrix_refuses_f_of_the_wrong_length(name):
    call = F_CALLS[name]
    with matrix() as dm, matrix() as fresh:
        for bad in list(wrong(F)) + ([] if name == "eval" else [F[None, :]]):  # (a (1, K) array is eval's alone)
            with refused(dm):
                call(dm, bad)
        assert_same(call(dm, F), call(fresh, F), name)


# ---- DeviceMatrix: every other array --------------------------------------------------------------------------------------------
def _then(read):
    """A setter's effect, read back: ``call(dm, **arrays)`` followed by ``read(dm)``."""
    return lambda call: (lambda dm, **kw: (call(dm, **kw), read(dm))[1])


_lognum = _then(lambda dm: dm.lognum(F))
_rows = _then(lambda dm: dm.to_host())

# name: (call, the correct arrays, the axes along which each is wrong)
ARRAY_CALLS = {
    "set_Nk": (_lognum(lambda dm, N_k: dm.set_Nk(N_k)), dict(N_k=[1.0, 2.0, 2.0]), dict(N_k=(0,))),
    "set_sample_weights": (_lognum(lambda dm, c_n: dm.set_sample_weights(c_n)), dict(c_n=[1.0, 0.0, 2.0, 1.0, 1.0]), dict(c_n=(0,))),
    "draw_bootstrap_weights": (_lognum(lambda dm, order: dm.draw_bootstrap_weights(7, 1, CUM, order)), dict(order=ORDER),
                               dict(order=(0,))),
    "row_sub": (_rows(lambda dm, v_n: dm.row_sub(1, v_n)), dict(v_n=V_N), dict(v_n=(0,))),
    "rows_sub": (_rows(lambda dm, v_n: dm.rows_sub(1, 0, 1, v_n)), dict(v_n=V_N), dict(v_n=(0,))),
    "vec_logshift": (lambda dm, A_n: (dm.vec_logshift(A_n), dm.to_host()), dict(A_n=V_N), dict(A_n=(0,))),
    "upload_rows": (_rows(lambda dm, rows: dm.upload_rows(1, rows)), dict(rows=U[:2] + 1.0), dict(rows=(1,))),
    "fill_masked_rows": (_rows(lambda dm, v_n, label_n: dm.fill_masked_rows(1, 2, v_n, label_n)), dict(v_n=V_N, label_n=LABEL),
                         dict(v_n=(0,), label_n=(0,))),
    "fill_linear_rows": (_rows(lambda dm, coeff_rb, offset_r: dm.fill_linear_rows(1, BASIS, coeff_rb, offset_r)),
                         dict(coeff_rb=COEFF, offset_r=OFFSET), dict(coeff_rb=(1,), offset_r=(0,))),
    "set_bins": (_then(lambda dm: dm.bin_lognum(F))(lambda dm, label_n, v_n: dm.set_bins(NBINS, label_n, v_n)),
                 dict(label_n=LABEL[::-1], v_n=V_N + 1.0), dict(label_n=(0,), v_n=(0,))),
    "bin_gram_w": (lambda dm, f_bins: dm.bin_gram_w(F, f_bins), dict(f_bins=[0.1, 0.2]), dict(f_bins=(0,))),
    "set_scan": (_then(lambda dm: dm.scan_lognum(F, COEFF, OFFSET))(lambda dm, basis_bn, t_qn: dm.set_scan(basis_bn, t_qn)),
                 dict(basis_bn=BASIS + 1.0, t_qn=T_QN), dict(basis_bn=(1,), t_qn=(1,))),
    "scan_lognum": (lambda dm, coeff_lb, offset_l: dm.scan_lognum(F, coeff_lb, offset_l), dict(coeff_lb=COEFF, offset_l=OFFSET),
                    dict(coeff_lb=(1,), offset_l=(0,))),
    "scan_gram_w": (lambda dm, offset_l, f_scan: dm.scan_gram_w(F, COEFF, offset_l, f_scan), dict(offset_l=OFFSET, f_scan=F_SCAN),
                    dict(offset_l=(0,), f_scan=(0,))),
    "scan_energy_lognum": (lambda dm, center_u: dm.scan_energy_lognum(F, COEFF, OFFSET, center_u), dict(center_u=[0.5, -0.5]),
                           dict(center_u=(0,))),
    "set_scan_bins": (_then(lambda dm: dm.scan_bin_lognum(F, COEFF, OFFSET))(lambda dm, label_n: dm.set_scan_bins(NBINS, label_n)),
                      dict(label_n=LABEL[::-1]), dict(label_n=(0,))),
    "scan_bin_gram_w": (lambda dm, f_bins: dm.scan_bin_gram_w(F, COEFF, OFFSET, f_bins), dict(f_bins=np.full((L, NBINS), 0.1)),
                        dict(f_bins=(0, 1))),
}


@pytest.mark.parametrize("name", list(ARRAY_CALLS))
def test_matrix_refuses_an_array_of_the_wrong_length(name):
    call, good, axes = ARRAY_CALLS[name]
    with matrix() as dm, matrix() as fresh:
        for arg, ax in axes.items():
            for bad in wrong(good[arg], ax):
                with refused(dm):
                    call(dm, **dict(good, **{arg: bad}))
        assert_same(call(dm, **good), call(fresh, **good), name)


def test_labels_that_would_wrap_are_refused():
    with matrix() as dm, matrix() as fresh:
        for setter in (lambda m, lab: m.set_bins(NBINS, lab, V_N), lambda m, lab: m.set_scan_bins(NBINS, lab)):
            with refused(dm):
                setter(dm, np.array([0, 1, 2 ** 32 + 1, 1, 0]))
        # int32 labels are refused by the library, which keeps its bins: the matrix keeps the count that sizes its outputs
        with pytest.raises(ValueError, match=r"\[-1, nbins\)"):
            dm.set_scan_bins(NBINS, np.array([0, 1, NBINS, 1, 0], dtype=np.int32))
        assert_same((dm.bin_lognum(F), dm.scan_bin_lognum(F, COEFF, OFFSET)), (fresh.bin_lognum(F), fresh.scan_bin_lognum(F, COEFF, OFFSET)),
                    "bins")


# ---- ExtendedMatrix -------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def extended():
    with matrix() as base:
        ext = base.extend(KE)
        assert ext is not None
        with ext:
            ext.upload_rows(K, ROWS_E)
            yield ext


@pytest.mark.parametrize("name", ["lognum", "gram_w"])
def test_extended_matrix_refuses_f_of_the_wrong_length(name):
    with extended() as ext, extended() as fresh:
        for bad in list(wrong(F_E)) + [F]:  # (F: the resident states' alone)
            with refused(ext, ext.base):
                getattr(ext, name)(bad)
        assert_same(getattr(ext, name)(F_E), getattr(fresh, name)(F_E), name)


def test_extended_matrix_refuses_rows_of_the_wrong_length():
    with extended() as ext, extended() as fresh:
        for bad in wrong(ROWS_E[:2], (1,)):
            with refused(ext):
                ext.upload_rows(K, bad)
        for bad in wrong(V_N):
            with refused(ext):
                ext.rows_sub(K, 0, 2, bad)
        assert_same(ext.lognum(F_E), fresh.lognum(F_E), "lognum")


# ---- state that used to appear with the first set_* call ------------------------------------------------------------------------
def test_fresh_matrix_has_no_bins_and_no_basis():
    with DeviceMatrix.from_host(U) as dm:
        dm.set_Nk(N_K)
        with pytest.raises(_lib.MbarHipError, match="no bins on this context"):
            dm.bin_lognum(F)
        with pytest.raises(_lib.MbarHipError, match="no bins on this context"):
            dm.bin_gram_w(F, np.zeros(0))
        with pytest.raises(ValueError, match=r"no basis on this matrix \(set_scan first\)"):
            dm.scan_lognum(F, COEFF)
        with pytest.raises(ValueError, match=r"no basis on this matrix \(set_scan first\)"):
            dm.scan_bin_lognum(F, COEFF)


def test_releases_succeed_on_a_fresh_matrix():
    with DeviceMatrix.from_host(U) as dm, DeviceMatrix.from_host(U) as fresh:
        dm.set_bins(0)
        dm.set_scan(None)
        dm.set_scan_bins(0)
        for m in (dm, fresh):
            m.set_Nk(N_K)
        assert_same(dm.lognum(F), fresh.lognum(F), "lognum")
        dm.set_scan(BASIS)  # (and the matrix takes a basis afterwards)
        assert dm.scan_lognum(F, COEFF)[0].shape == (L,)


@pytest.mark.parametrize("order", [None, ORDER], ids=["default-layout", "order"])
def test_bootstrap_weights_do_not_depend_on_the_layout_key(order):
    def weights_seen(dm):
        return dm.lognum(F)

    with DeviceMatrix.from_host(U) as a, DeviceMatrix.from_host(U) as b:
        for m in (a, b):
            m.set_Nk(N_K)
        a.draw_bootstrap_weights(11, 1, CUM, order)  # no key: the arrays travel with the draw
        no_key = weights_seen(a)
        key = object()
        b.draw_bootstrap_weights(11, 1, CUM, order, layout_key=key)  # a new key: uploaded, then drawn
        new_key = weights_seen(b)
        b.set_sample_weights(None)
        unit = weights_seen(b)
        b.draw_bootstrap_weights(11, 1, None, None, layout_key=key)  # the key again: no array is read
        same_key = weights_seen(b)
        a.draw_bootstrap_weights(11, 1, CUM, order, layout_key=key)  # a key after no key, on the other matrix
        after = weights_seen(a)
    assert np.array_equal(no_key, new_key) and np.array_equal(no_key, same_key) and np.array_equal(no_key, after)
    assert not np.array_equal(no_key, unit)  # (the draw is not the unit weights: the comparison sees the weights)


# ---- DeviceBatch ----------------------------------------------------------------------------------------------------------------
BK, BN = 2, 4
BLOCKS = [np.ascontiguousarray(RNG.normal(size=(BK, BN))) for _ in range(2)]
BNKS = [np.array([2, 2]), np.array([3, 1])]
BF = np.zeros((2, batch.MAX_K))
BF[:, 1] = [0.2, -0.1]
EXT = [RNG.normal(size=(1, BN)), RNG.normal(size=(2, BN))]


def batch_states(idx):
    """States that are done at once (no iteration allowed): the passes below find every entry's state on the device."""
    st = (_lib.BatchState * len(idx))()
    sv = batch._states_view(st)
    sv["tol"], sv["gamma"], sv["maxiter"], sv["min_sc_iter"] = 1e-10, 1.0, 0, 0
    for i, p in enumerate(idx):
        sv["K"][i] = BK
        sv["Nk"][i, :BK] = BNKS[p]
        sv["f"][i, :BK] = BF[p, :BK]
    return st


@contextlib.contextmanager
def device_batch():
    with batch.DeviceBatch(BLOCKS) as h:
        h.solve(batch_states([0, 1]))
        h.set_replicas(np.array([0, 1, 1]), BNKS)
        h.replicas_draw(0, np.array([5, 6, 6], dtype=np.uint64), np.array([0, 0, 1]))
        h.replicas_solve(batch_states([0, 1, 1]))
        h.set_ext(EXT)
        yield h


SF = BF[[0, 1, 1]]
ON2, ON3 = np.ones(2, dtype=bool), np.ones(3, dtype=bool)
BATCH_CALLS = {
    "gram_w": (lambda h, F, mask: h.gram_w(F, mask), dict(F=BF, mask=ON2), dict(F=(0, 1), mask=(0,))),
    "replicas_gram_w": (lambda h, F, mask: h.replicas_gram_w(F, mask), dict(F=SF, mask=ON3), dict(F=(0, 1), mask=(0,))),
    "ext_lognum": (lambda h, F, mask: h.ext_lognum(F, mask), dict(F=BF, mask=ON2), dict(F=(0, 1), mask=(0,))),
    "ext_gram": (lambda h, F, f_ext, mask: h.ext_gram(F, f_ext, mask), dict(F=BF, f_ext=np.array([0.1, 0.2, 0.3]), mask=ON2),
                 dict(F=(0, 1), f_ext=(0,), mask=(0,))),
    "replica_set_weights": (lambda h, c_n: (h.replica_set_weights(1, c_n), h.replicas_gram_w(SF, ON3))[1],
                            dict(c_n=[1.0, 0.0, 2.0, 1.0]), dict(c_n=(0,))),
    "replicas_draw": (lambda h, seeds, replicates: (h.replicas_draw(1, seeds, replicates), h.replicas_gram_w(SF, ON3))[1],
                      dict(seeds=np.array([9, 8], dtype=np.uint64), replicates=np.array([2, 3])), dict(seeds=(0,), replicates=(0,))),
    "set_ext": (lambda h, r0, r1: (h.set_ext([r0, r1]), h.ext_lognum(BF, ON2))[1], dict(r0=EXT[0] + 1.0, r1=EXT[1]),
                dict(r0=(1,), r1=(1,))),
    "set_replicas": (lambda h, n0, n1: (h.set_replicas(np.array([0, 1]), [n0, n1]), h.replicas_draw(0, [3, 4], [0, 0]),
                                        h.replicas_solve(batch_states([0, 1])), h.replicas_gram_w(BF, ON2))[3],
                     dict(n0=BNKS[0], n1=BNKS[1]), dict(n0=(0,), n1=(0,))),
}


@pytest.mark.parametrize("name", list(BATCH_CALLS))
def test_batch_refuses_an_array_of_the_wrong_length(name):
    call, good, axes = BATCH_CALLS[name]
    with device_batch() as h, device_batch() as fresh:
        for arg, ax in axes.items():
            for bad in wrong(good[arg], ax):
                with refused(h):
                    call(h, **dict(good, **{arg: bad}))
        assert_same(call(h, **good), call(fresh, **good), name)


def test_batch_refuses_states_of_the_wrong_number():
    with device_batch() as h, device_batch() as fresh:
        for n, solve in ((1, h.solve), (3, h.solve), (2, h.replicas_solve), (4, h.replicas_solve)):
            with refused(h):
                solve(batch_states([0] * n))
        assert_same(h.gram_w(BF, ON2), fresh.gram_w(BF, ON2), "gram_w")


def test_batch_argument_errors_of_the_library_are_parameter_errors():
    with device_batch() as h:
        with pytest.raises(ParameterError, match="finite and >= 0"):
            h.replica_set_weights(0, np.full(BN, -1.0))


# ---- DeviceKDE, DeviceACF, DeviceBAR, DeviceBSplineMoments --------------------------------------------------------------------
def test_kde_refuses_arrays_of_the_wrong_length():
    from pymbar_amd.kde import DeviceKDE

    X, Q, V = RNG.normal(size=(5, 2)), RNG.normal(size=(3, 2)), np.abs(RNG.normal(size=(5, 2))) + 0.1

    def answer(dk):
        dk.set_weights(V)
        return dk.log_density(Q)

    with DeviceKDE(X, "gaussian", 0.7) as dk, DeviceKDE(X, "gaussian", 0.7) as fresh:
        for bad in list(wrong(V, (0,))) + list(wrong(V[:, 0], (0,))):
            with refused(dk):
                dk.set_weights(bad)
        for bad in list(wrong(Q, (1,))) + [Q[:, 0]]:
            with refused(dk):
                dk.log_density(bad)
        assert_same(answer(dk), answer(fresh), "log_density")
    with pytest.raises(ValueError):
        DeviceKDE(X[:, 0], "gaussian", 0.7)


def test_acf_refuses_a_second_series_of_another_length():
    from pymbar_amd.timeseries import DeviceACF

    a, b = RNG.normal(size=6), RNG.normal(size=6)
    for bad in wrong(b):
        with pytest.raises(ValueError, match="b must have shape"):
            DeviceACF(a, bad)
    with pytest.raises(ValueError, match="a must have shape"):
        DeviceACF(a.reshape(2, 3))
    with DeviceACF(a, b) as dev, DeviceACF(a, b) as fresh:
        assert_same(dev.lag_sums([0, 1], [0, 2]), fresh.lag_sums([0, 1], [0, 2]), "lag_sums")


def test_bar_refuses_free_energies_of_the_wrong_length():
    from pymbar_amd.other_estimators import DeviceBAR

    wF = [RNG.normal(size=4) for _ in range(3)]
    wR = [RNG.normal(size=3) for _ in range(3)]
    d = np.array([0.1, -0.2, 0.3])
    with DeviceBAR(wF, wR) as h, DeviceBAR(wF, wR) as fresh:
        for bad in list(wrong(d)) + [d[:1], d[None, :]]:  # (one value for all problems is a scalar, not a vector of one)
            with refused(h):
                h.zero(bad)
        assert_same(h.zero(d), fresh.zero(d), "zero")
        assert_same(h.zero(0.25), fresh.zero(np.full(3, 0.25)), "zero of a scalar")


def test_bspline_refuses_arrays_of_the_wrong_length():
    from pymbar_amd.bspline import DeviceBSplineMoments

    x = RNG.uniform(0.0, 1.0, size=5)
    g = np.array([0, 1, 1, 0, 1])
    V = RNG.normal(size=(5, 2))
    t = np.array([0.0, 0.0, 0.5, 1.0, 1.0])

    def answer(dev):
        dev.set_groups(g)
        dev.set_weights(V)
        return dev.moments(t, 1)

    with DeviceBSplineMoments(x) as dev, DeviceBSplineMoments(x) as fresh:
        for bad in wrong(g):
            with refused(dev, error=ParameterError):
                dev.set_groups(bad)
        for bad in list(wrong(V, (0,))) + list(wrong(V[:, 0], (0,))):
            with refused(dev, error=ParameterError):
                dev.set_weights(bad)
        assert_same(answer(dev), answer(fresh), "moments")
