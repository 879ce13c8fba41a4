"""The argument layer of ``pymbar_amd._lib`` (``f64``, ``labels_i32``, ``check``): what an array must look like before a Python
face hands it to the library.  Pure numpy and ctypes: the library is not loaded."""
import numpy as np
import pytest

from pymbar_amd import _lib
from pymbar_amd.utils import ParameterError


# ---- f64 ------------------------------------------------------------------------------------------------------------------------
def test_f64_passes_a_conforming_array_through():
    a = np.arange(6.0).reshape(2, 3)
    assert _lib.f64(a, (2, 3), "a") is a
    assert _lib.f64(a, (None, 3), "a") is a
    assert _lib.f64(a[1], (3,), "a") is not None and np.shares_memory(_lib.f64(a[1], (3,), "a"), a)  # (a contiguous run: no copy)


def test_f64_converts_a_list():
    out = _lib.f64([[1, 2], [3, 4]], (2, 2), "a")
    assert out.dtype == np.float64 and out.flags.c_contiguous
    np.testing.assert_array_equal(out, [[1.0, 2.0], [3.0, 4.0]])


@pytest.mark.parametrize("make", [lambda a: np.asfortranarray(a), lambda a: np.repeat(a, 2, axis=1)[:, ::2], lambda a: a.T.copy().T],
                         ids=["fortran", "strided", "transposed"])
def test_f64_makes_contiguous(make):
    a = np.arange(12.0).reshape(3, 4)
    b = make(a)
    assert not b.flags.c_contiguous
    out = _lib.f64(b, (3, 4), "a")
    assert out.flags.c_contiguous and out.dtype == np.float64
    np.testing.assert_array_equal(out, a)


def test_f64_converts_float32_and_integers():
    a = np.array([1.5, 2.5, -3.0], dtype=np.float32)
    out = _lib.f64(a, (3,), "a")
    assert out.dtype == np.float64
    np.testing.assert_array_equal(out, [1.5, 2.5, -3.0])
    assert _lib.f64(np.arange(3), (3,), "a").dtype == np.float64


@pytest.mark.parametrize("a, shape", [
    (np.zeros((2, 3)), (6,)),          # wrong rank
    (np.zeros(6), (2, 3)),
    (np.zeros((1, 3)), (3,)),          # (a row is not a vector)
    (np.zeros(3), (4,)),               # wrong extent: short
    (np.zeros(5), (4,)),               # long
    (np.zeros((2, 3)), (2, 4)),
    (np.zeros((2, 3)), (None, 4)),     # the wildcard frees one extent only
    (np.zeros((2, 3, 1)), (None, 3)),
    (np.float64(1.0), ()),             # (numpy makes a scalar a vector of one)
])
def test_f64_refuses_a_wrong_shape(a, shape):
    with pytest.raises(ValueError, match="a must have shape"):
        _lib.f64(a, shape, "a")


def test_f64_message_names_the_shape():
    with pytest.raises(ValueError, match=r"^f must have shape \(3,\)$"):
        _lib.f64(np.zeros(2), (3,), "f")
    with pytest.raises(ValueError, match=r"^rows must have shape \(\*, 5\)$"):
        _lib.f64(np.zeros((2, 4)), (None, 5), "rows")


def test_f64_wildcard():
    for n in (0, 1, 7):
        assert _lib.f64(np.zeros((n, 3)), (None, 3), "a").shape == (n, 3)
    assert _lib.f64(np.zeros((2, 5)), (None, None), "a").shape == (2, 5)


def test_f64_none_only_where_optional():
    assert _lib.f64(None, (3,), "a", optional=True) is None
    with pytest.raises(ValueError, match="a is required"):
        _lib.f64(None, (3,), "a")
    with pytest.raises(ValueError, match="a is required"):
        _lib.f64(None, (1,), "a")  # (not the vector [nan] that numpy makes of None)
    with pytest.raises(ValueError):
        _lib.f64(np.zeros(2), (3,), "a", optional=True)  # (optional is about None alone)


def test_f64_error_type():
    with pytest.raises(ParameterError, match="a must have shape"):
        _lib.f64(np.zeros(2), (3,), "a", error=ParameterError)
    with pytest.raises(ParameterError, match="a is required"):
        _lib.f64(None, (3,), "a", error=ParameterError)


# ---- labels_i32 -----------------------------------------------------------------------------------------------------------------
def test_labels_int64_in_range_narrow():
    lab = np.array([-1, 0, 3, 2, -1], dtype=np.int64)
    out = _lib.labels_i32(lab, 4, 5, "label_n")
    assert out.dtype == np.int32 and out.flags.c_contiguous
    np.testing.assert_array_equal(out, lab)
    np.testing.assert_array_equal(_lib.labels_i32([0, 1, 1], 2, 3, "label_n"), [0, 1, 1])


@pytest.mark.parametrize("bad", [2 ** 32 + 1, -2, 4, -2 ** 32], ids=["wraps-to-1", "below", "nbins", "wraps-to-0"])
def test_labels_out_of_range_are_refused_before_the_cast(bad):
    lab = np.array([0, bad, 1], dtype=np.int64)
    assert bad in (-2, 4) or 0 <= int(lab.astype(np.int32)[1]) < 4  # (the narrowing cast alone would let it through)
    with pytest.raises(ValueError, match=r"labels must lie in \[-1, nbins\)"):
        _lib.labels_i32(lab, 4, 3, "label_n")


def test_labels_int32_pass_through():
    lab = np.array([0, -1, 1], dtype=np.int32)
    assert _lib.labels_i32(lab, 2, 3, "label_n") is lab
    strided = np.array([0, 9, 1, 9, -1, 9], dtype=np.int32)[::2]
    out = _lib.labels_i32(strided, 2, 3, "label_n")
    assert out.flags.c_contiguous
    np.testing.assert_array_equal(out, [0, 1, -1])


@pytest.mark.parametrize("lab", [np.zeros(2, np.int32), np.zeros(4, np.int32), np.zeros((3, 1), np.int64), np.zeros(4, np.int64)])
def test_labels_wrong_length(lab):
    with pytest.raises(ValueError, match=r"label_n must have shape \(3,\)"):
        _lib.labels_i32(lab, 2, 3, "label_n")


# ---- check ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def stub_last_error(monkeypatch):
    seen = []

    def last_error(ctx=None):
        seen.append(ctx)
        return "the stub's message"

    monkeypatch.setattr(_lib, "last_error", last_error)
    monkeypatch.setattr(_lib, "load_library", lambda: pytest.fail("check() must not load the library here"))
    return seen


def test_check_ok(stub_last_error):
    assert _lib.MBAR_OK == 0 and _lib.MBAR_ERR_ARG == -1
    _lib.check(_lib.MBAR_OK)
    _lib.check(_lib.MBAR_OK, arg_error=ValueError)
    assert stub_last_error == []


@pytest.mark.parametrize("arg_error", [ValueError, ParameterError])
def test_check_arg_error(stub_last_error, arg_error):
    ctx = object()
    with pytest.raises(arg_error, match="^the stub's message$"):
        _lib.check(_lib.MBAR_ERR_ARG, ctx, arg_error=arg_error)
    assert stub_last_error == [ctx]  # (the message is the context's own)


def test_check_arg_error_unnamed(stub_last_error):
    with pytest.raises(_lib.MbarHipError, match="libmbar_hip error -1: the stub's message") as exc:
        _lib.check(_lib.MBAR_ERR_ARG)
    assert exc.value.code == _lib.MBAR_ERR_ARG


@pytest.mark.parametrize("code", [-2, -3, -4, 1, 7])
@pytest.mark.parametrize("arg_error", [None, ValueError])
def test_check_other_codes(stub_last_error, code, arg_error):
    with pytest.raises(_lib.MbarHipError, match="the stub's message") as exc:
        _lib.check(code, arg_error=arg_error)
    assert exc.value.code == code


def test_pointer_types():
    import ctypes as C

    a = np.arange(3, dtype=np.int32)
    assert _lib.ptr(a, _lib._i32p)[2] == 2 and isinstance(_lib.ptr(a, _lib._i32p), C.POINTER(C.c_int32))
    b = np.array([2 ** 63 + 5], dtype=np.uint64)
    assert _lib.ptr(b, _lib._u64p)[0] == 2 ** 63 + 5
    assert _lib.ptr(None, _lib._i32p) is None
