"""The row and vector kernels of ``mbar_k_rows.hip`` on an MI355X, called directly through ``DeviceMatrix`` / ``ExtendedMatrix``.

Every operation that is one IEEE subtraction or a copy must return numpy's bits.  The shifts of the log-space operations are
``m - |4 eps m|`` of the row minimum ``m``, again to the bit.  The logged values lie within 2 ulp of ``np.log(x - shift)``: one
ulp for the device ``log`` (documented at 1 ulp) and one for the host's; where the kernel subtracts the logarithm from a state row,
the row must be ``state - L`` for an ``L`` within those 2 ulp.

The shapes enter every branch of the launch arithmetic: a single sample, one sample short of and past a workgroup of 256, two
workgroups of 2048 (the log-shift kernels give a workgroup 2048 samples), and ``256 * 2048 + 3`` samples, at which a grid capped
at 2048 workgroups goes round a second time and the row-minimum pass (256 workgroups of 2048) strides; 1025 rows make the row
loop (``gridDim.y`` capped at 1024) take a second trip.

``row_sub`` alone has a grid capped at 4096 workgroups of 256: it gets ``4096 * 256 + 3`` samples as well.

Rows outside an operation are read back and compared.  The padding columns behind N are not copied by ``to_host``; they show in
the sweeps, which read whole tiles: after every operation ``eval`` with the Gram matrix, ``lognum`` and ``gram_w`` must return
the bits they return on a fresh upload of the same N columns, whose padding is zero."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from pymbar_amd import _lib  # noqa: E402
from pymbar_amd.device import DeviceMatrix  # noqa: E402

EPS4 = 8.881784197001252e-16
N_BIG = 256 * 2048 + 3
# (N, rows of the operation): the big N with one row (a matrix of 3 rows, 12 MB); 1025 rows at a small N
SHAPES = [(1, 1), (1, 3), (255, 3), (257, 1), (257, 3), (2049, 3), (N_BIG, 1), (257, 1025)]
IDS = ["N%d-R%d" % s for s in SHAPES]


def same_bits(a, b):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64) == np.ascontiguousarray(b, dtype=np.float64).view(np.int64)


def assert_bits(got, want, what):
    ok = same_bits(got, want)
    assert ok.all(), f"{what}: {np.count_nonzero(~ok)} entries differ, first at {np.argwhere(~ok)[0]}"


def rows_of(K, N, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(K, N)) * rng.uniform(0.5, 20.0, size=(K, 1))


def shift_of(m):
    return m - np.abs(EPS4 * m)


def log_distance(got, arg, state=None):
    """Smallest k with got == state - (np.log(arg) moved by k ulp) per entry (99: none up to 2)."""
    with np.errstate(all="ignore"):
        L = np.log(arg)
        up = dn = L
        cands = [(0, L)]
        for k in (1, 2):
            up, dn = np.nextafter(up, np.inf), np.nextafter(dn, -np.inf)
            cands += [(k, up), (k, dn)]
        best = np.full(L.shape, 99)
        for k, c in reversed(cands):
            best = np.where(same_bits(c if state is None else state - c, got), k, best)
    return best


def observable_rows(R, N, seed):
    """Raw observable rows: row 0 has a negative minimum, row 1 (if any) the minimum 0, the others positive minima."""
    rng = np.random.default_rng(seed)
    A = rng.uniform(0.5, 50.0, size=(R, N)) * rng.uniform(0.1, 1e3, size=(R, 1))
    A[0] -= 1.25 * A[0].max() if N > 1 else 2.0 * A[0, 0]
    if R > 1:
        A[1] -= A[1].min()
        assert A[1].min() == 0.0
    assert A[0].min() < 0.0
    return A


def sweeps(dm, f):
    """Everything the whole-tile sweeps return at f, as a list of arrays."""
    return list(dm.eval(f, gram=True)) + [dm.lognum(f)] + list(dm.gram_w(f))


def counts(K, N):
    N_k = np.full(K, N // K)
    N_k[:N - N_k.sum()] += 1
    return N_k


def assert_zero_padding(dm, N_k, f, what):
    """The sweeps of dm return the bits of a fresh upload of its N columns."""
    with DeviceMatrix.from_host(dm.to_host()) as fresh:
        fresh.set_Nk(N_k)
        for i, (a, b) in enumerate(zip(sweeps(dm, f), sweeps(fresh, f))):
            assert_bits(a, b, f"sweep output {i} after {what}")


@pytest.mark.parametrize("N", [1, 255, 257, 2049])
def test_columns_behind_N_are_untouched(N):
    """Seven rows (a pitch of whole 64-sample tiles: 64, 256, 320 and 2112 columns for these N), every operation in turn."""
    K, R = 7, 3
    u, v = rows_of(K, N, 21), rows_of(1, N, 22)[0]
    label = np.random.default_rng(23).integers(-1, R, size=N).astype(np.int32)
    N_k, f = counts(K, N), np.linspace(0.0, 1.0, K)
    with DeviceMatrix.from_host(u) as dm:
        dm.set_Nk(N_k)
        for what, op in (("row_sub", lambda: dm.row_sub(6, v)),
                         ("rows_sub", lambda: dm.rows_sub(R, 0, R, v)),
                         ("rows_sub in place", lambda: dm.rows_sub(0, 0, R)),
                         ("rows_rsub", lambda: dm.rows_rsub(R, 0, R)),
                         ("rows_logshift", lambda: dm.rows_logshift(0, R)),  # (negative minima: every logarithm is finite)
                         ("vec_logshift + row_sub", lambda: (dm.vec_logshift(v), dm.row_sub(6, None))),
                         ("fill_masked_rows", lambda: dm.fill_masked_rows(R, 2, v, label))):
            op()
            assert np.isfinite(dm.to_host()).all() or what == "fill_masked_rows"
            assert_zero_padding(dm, N_k, f, what)


@pytest.mark.parametrize("N", [1, 255, 257, 2049])
def test_columns_behind_N_are_untouched_by_rows_obs_from_base(N):
    """The pair (6 resident rows, 113 appended ones) after the operation against a fresh pair that was given the final rows."""
    Kb, Ke, R = 6, 113, 3
    u, rows = rows_of(Kb, N, 24), rows_of(Ke, N, 25)
    N_k = np.concatenate([counts(Kb, N), np.zeros(Ke)])
    f = np.linspace(0.0, 1.0, Kb + Ke)

    def pair_sweeps(ext_rows, op):
        with DeviceMatrix.from_host(u) as base:
            base.set_Nk(N_k[:Kb])
            e = base.extend(Ke)
            assert e is not None
            with e, DeviceMatrix.empty(Ke, N) as out:
                e.upload_rows(Kb, ext_rows)
                op(e)
                out.copy_rows_from(e, 0, 0, Ke)  # (rows of the extension's own context)
                return out.to_host(), [e.lognum(f)] + list(e.gram_w(f))

    final, got = pair_sweeps(rows, lambda e: e.rows_obs_from_base(Kb, 0, R, R))
    assert np.isfinite(final).all() and not same_bits(final[:R], rows[:R]).all()
    _, want = pair_sweeps(final, lambda e: None)
    for i, (a, b) in enumerate(zip(got, want)):
        assert_bits(a, b, f"sweep output {i}")


# (row_sub has a grid of its own, capped at 4096 workgroups: the last N makes it go round a second time)
@pytest.mark.parametrize("N", [s[0] for s in SHAPES if s[1] == 1 or s[0] == 255] + [2049, 4096 * 256 + 3])
def test_row_sub(N):
    u, v = rows_of(3, N, 1), rows_of(1, N, 2)[0]
    with DeviceMatrix.from_host(u) as dm:
        dm.row_sub(1, v)
        want = u.copy()
        want[1] = u[1] - v
        assert_bits(dm.to_host(), want, "row_sub")
        dm.row_sub(2, None)  # the vector staged before
        want[2] = u[2] - v
        assert_bits(dm.to_host(), want, "row_sub again")


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_rows_sub(shape):
    N, R = shape
    u, v = rows_of(2 * R + 1, N, 3), rows_of(1, N, 4)[0]
    with DeviceMatrix.from_host(u) as dm:
        dm.rows_sub(R, 0, R, v)  # from another row block
        want = u.copy()
        want[R:2 * R] = u[:R] - v
        assert_bits(dm.to_host(), want, "rows_sub from another block")
        dm.rows_sub(0, 0, R)     # in place, the vector staged before
        want[:R] = u[:R] - v
        assert_bits(dm.to_host(), want, "rows_sub in place")


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_rows_rsub(shape):
    N, R = shape
    u = rows_of(2 * R + 1, N, 5)
    with DeviceMatrix.from_host(u) as dm:
        dm.rows_rsub(R, 0, R)
        want = u.copy()
        want[R:2 * R] = u[:R] - u[R:2 * R]
        assert_bits(dm.to_host(), want, "rows_rsub")


@pytest.mark.parametrize("shape", [(1, 3), (255, 3), (257, 3), (2049, 3), (N_BIG, 2)], ids=lambda s: "N%d-R%d" % s)
def test_fill_masked_rows(shape):
    N, R = shape
    u, v = rows_of(R + 1, N, 6), rows_of(1, N, 7)[0]
    label = np.random.default_rng(8).integers(-1, R + 2, size=N).astype(np.int32)  # -1, the rows, and two labels of no row
    label[0] = -1 if N > 1 else 0
    label[-1] = R + 1 if N > 1 else 0
    with DeviceMatrix.from_host(u) as dm:
        dm.fill_masked_rows(0, R, v, label)
        want = u.copy()
        for i in range(R):
            want[i] = np.where(label == i, v, np.inf)
        assert_bits(dm.to_host(), want, "fill_masked_rows")


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_rows_logshift(shape):
    N, R = shape
    A = observable_rows(R, N, 9)
    u = np.vstack([A, rows_of(1, N, 10)])
    with DeviceMatrix.from_host(u) as dm:
        shift = dm.rows_logshift(0, R)
        got = dm.to_host()
    want_shift = shift_of(A.min(axis=1))
    assert_bits(shift, want_shift, "shift")
    assert_bits(got[R], u[R], "the row behind the operation")
    d = log_distance(got[:R], A - want_shift[:, None])
    print(f"rows_logshift N={N} R={R}: largest distance to np.log {d.max()} ulp")
    assert d.max() <= 2


@pytest.mark.parametrize("N", [1, 255, 257, 2049, N_BIG])
def test_vec_logshift(N):
    A = observable_rows(1, N, 11)[0]  # a negative minimum (the next test has the minimum 0)
    u = rows_of(3, N, 12)
    with DeviceMatrix.from_host(u) as dm:
        shift = dm.vec_logshift(A)
        dm.row_sub(1, None)  # the staged log(A - shift) shows in the row it is subtracted from
        got = dm.to_host()
    want_shift = shift_of(A.min())
    assert_bits(shift, want_shift, "shift")
    assert_bits(got[[0, 2]], u[[0, 2]], "the rows outside the operation")
    d = log_distance(got[1], A - want_shift, state=u[1])
    print(f"vec_logshift N={N}: largest distance to np.log {d.max()} ulp")
    assert d.max() <= 2


def test_vec_logshift_of_a_zero_minimum():
    N = 2049
    A = observable_rows(2, N, 13)[1]
    u = rows_of(2, N, 14)
    with DeviceMatrix.from_host(u) as dm:
        shift = dm.vec_logshift(A)
        dm.row_sub(0, None)
        got = dm.to_host()
    assert shift == 0.0 and not np.signbit(shift)
    assert_bits(got[1], u[1], "the row outside the operation")
    d = log_distance(got[0], A, state=u[0])
    assert np.isposinf(got[0][A == 0.0]).all()  # u - log 0
    assert d.max() <= 2


@pytest.mark.parametrize("N", [1, 255, 257, 2049, N_BIG])
def test_rows_obs_from_base(N):
    """Three appended rows = state rows - log(observable rows - shift).  An extension exists only for 129 .. 256 padded rows in
    total (``mbar_ctx_create_ext``), so 113 rows are appended to 3 or 6 resident ones.  At the largest N that is an allocation of
    177 row pitches (0.74 GB) beyond the 3 resident rows' 12 MB; of it the operation and the test touch four rows (17 MB): the
    three written ones and a sentinel, copied to a small matrix to be read back.  Creating the extension zeroes its 63 padding rows."""
    R = 3
    Kb = R if N == N_BIG else 2 * R
    A = observable_rows(R, N, 15)
    state = rows_of(R, N, 16)
    u = A + 0.0 if Kb == R else np.vstack([state, A])  # at the largest N the observable rows are their own state rows
    if Kb == R:
        state = A
    sentinel = rows_of(1, N, 17)
    want_shift = shift_of(A.min(axis=1))
    with DeviceMatrix.from_host(u) as base:
        e = base.extend(113)
        assert e is not None
        with e, DeviceMatrix.empty(R + 1, N) as out:
            e.upload_rows(Kb + R, sentinel)
            for call in ("finds the minima", "is handed the minima"):
                shift = e.rows_obs_from_base(Kb, 0, Kb - R, R)
                out.copy_rows_from(e, 0, 0, R + 1)  # (rows of the extension's own context)
                got = out.to_host()
                assert_bits(shift, want_shift, f"shift, the call that {call}")
                assert_bits(got[R], sentinel[0], "the row behind the operation")
                d = log_distance(got[:R], A - want_shift[:, None], state=state)
                print(f"rows_obs_from_base N={N}, the call that {call}: largest distance to np.log {d.max()} ulp")
                assert d.max() <= 2
        assert_bits(base.to_host(), u, "the resident rows")


def test_weights_from_vec():
    """The weights (A - shift)^p formed on the device act like the same weights installed from the host.  exp and log are within
    an ulp or two on either side and |p log(A - shift)| < 8 here, so the weights agree to ~1e-15 relative and the logarithm of a
    sum of them to ~1e-15 absolute: 1e-13 is that with a margin of two decades."""
    K, N, p = 5, 2049, 2.0
    rng = np.random.default_rng(18)
    u = rows_of(K, N, 19) * 0.1
    A = rng.uniform(1.0, 3.0, size=N)
    N_k = np.array([500, 400, 449, 300, 400])
    f = np.linspace(0.0, 1.0, K)
    with DeviceMatrix.from_host(u) as dm:
        dm.set_Nk(N_k)
        shift = dm.vec_logshift(A)
        dm.weights_from_vec(p)
        got = dm.lognum(f)
        dm.set_sample_weights((A - shift) ** p)
        want = dm.lognum(f)
        dm.set_sample_weights(None)
        plain = dm.lognum(f)
    np.testing.assert_allclose(got, want, rtol=0.0, atol=1e-13)
    assert np.abs(got - plain).min() > 0.1  # the weights were in the sum


def test_weights_from_vec_overflow_is_an_error():
    A = np.array([1.0, 2.0, 1e100, 3.0])
    with DeviceMatrix.from_host(rows_of(2, 4, 20)) as dm:
        dm.vec_logshift(A)
        with pytest.raises(_lib.MbarHipError, match=r"\(A - shift\)\^power is not finite for some sample"):
            dm.weights_from_vec(4.0)
