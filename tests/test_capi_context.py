"""The context behind the C ABI (pymbar_amd/csrc/mbar_ctx.h; mbar_capi.cpp the context and its buffers, mbar_eval.cpp the sweeps,
mbar_rows.cpp the writers of the matrix, mbar_ext.cpp the extension's entry points): what every writer of the resident matrix must
leave behind, buffers that grow while captured graphs hold their addresses, and the first call of a fresh context, which sizes the
buffers of all its launches before the first one.  Everything is compared bit for bit (``array_equal``, NaN equal to NaN) with
fresh contexts that saw only the final state.  Needs a real MI355X: run with ``-m gpu``."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from pymbar_amd.device import DeviceMatrix, _dptr  # noqa: E402
from tests.test_gpu_parity import random_problem  # noqa: E402


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def assert_same(got, want, tag):
    assert got.keys() == want.keys()
    for key in want:
        assert same(got[key], want[key]), f"{tag}: {key} differs"


def solve_outputs(f, res, prefix):
    out = {prefix + "f": f}
    for key, v in res.items():
        if key != "wall_ms" and v is not None:
            out[prefix + key] = v
    return out


def has_solve_sums(dm):
    return dm._lib.mbar_ctx_last_solve_psum(dm._ctx, _dptr(np.empty(dm.K))) == 0


def download(ctx_owner, K, N):
    out = np.empty((K, N))
    ctx_owner._check(ctx_owner._lib.mbar_ctx_download_u(ctx_owner._ctx, _dptr(out), N))
    return out


# ---- 1. every writer invalidates what depends on the matrix ----------------------------------------------------------

def evaluations(dm, f, prefix=""):
    """mbar_logden first: when slot 0 still counts as holding the log-denominators of this very f, it is served from there."""
    out = {prefix + "logden": dm.logden(f)}
    psum, sld, gram = dm.eval(f, gram=True)
    out.update({prefix + "psum": psum, prefix + "sumlogden": sld, prefix + "gram": gram})
    return out


def plain_outputs(dm, f):
    """A solve (it leaves its sums and, where the loop keeps one, the resident probability matrix), then the evaluations: the last
    thing the context did is mbar_logden at f, so the poison flags are set and slot 0 holds the log-denominators of f."""
    out = solve_outputs(*dm.solve_adaptive(np.zeros(dm.K), tol=1e-10, maxiter=200, min_sc_iter=0), prefix="solve ")
    out.update(evaluations(dm, f))
    return out


def after_a_write(dm, f):
    """What a context is asked after its matrix changed.  The evaluations come first, before any solve (a solve forgets slot 0
    and scans the matrix by itself): they alone show a writer that left the poison flags and slot 0 as they were."""
    out = evaluations(dm, f, prefix="first ")
    out.update(plain_outputs(dm, f))
    return out


def _upload_u(dm, u, rng):
    u2 = np.ascontiguousarray(u + rng.uniform(0.0, 1.0, size=u.shape))
    dm._check(dm._lib.mbar_ctx_upload_u(dm._ctx, _dptr(u2), u.shape[1], 0, u.shape[1], 0))


def _copy_rows(dm, u, rng):
    with DeviceMatrix.from_host(u[::-1] * 1.25) as other:
        dm.copy_rows_from(other, dst_row0=1, src_row0=2, nrows=2)


def _fill_masked_rows(dm, u, rng):
    # rows 3, 4 = v on the samples labelled 0, 1 and +inf (weight zero) elsewhere
    dm.fill_masked_rows(3, 2, rng.uniform(0.0, 2.0, size=u.shape[1]), rng.integers(0, 2, size=u.shape[1]))


def _generate_harmonic(dm, u, rng):
    N_k = np.full(dm.K, u.shape[1] // dm.K, dtype=np.int64)
    dm._check(dm._lib.mbar_ctx_generate_harmonic(dm._ctx, C.c_uint64(7), _dptr(np.linspace(0.0, 2.0, dm.K)), _dptr(np.linspace(1.0, 2.0, dm.K)),
                                                 N_k.ctypes.data_as(C.POINTER(C.c_int64)), 0))


def _nan_vector(N):
    v = np.linspace(-1.0, 1.0, N)
    v[17] = np.nan
    return v


def _with(rows, r, n, value):
    rows = rows.copy()
    rows[r, n] = value
    return rows


# the matrix the context starts with, where it is not the problem's own
PLAIN_STARTS = {"upload_rows_from_nan": lambda u: _with(u, 1, 40, np.nan)}
PLAIN_WRITERS = {
    # the two changes that flip the poison flag: every output NaN afterwards, resp. finite again
    "rows_sub_to_nan": lambda dm, u, rng: dm.rows_sub(3, 0, 2, _nan_vector(u.shape[1])),
    "upload_rows_from_nan": lambda dm, u, rng: dm.upload_rows(1, u[1:3]),
    "upload_u": _upload_u,
    "upload_rows": lambda dm, u, rng: dm.upload_rows(1, u[1:3] + 0.5),
    "copy_rows": _copy_rows,
    "row_sub": lambda dm, u, rng: dm.row_sub(2, rng.uniform(-1.0, 1.0, size=u.shape[1])),
    "rows_sub": lambda dm, u, rng: dm.rows_sub(3, 0, 2, rng.uniform(-1.0, 1.0, size=u.shape[1])),
    "rows_rsub": lambda dm, u, rng: dm.rows_rsub(3, 0, 2),
    "rows_logshift": lambda dm, u, rng: dm.rows_logshift(4, 1),
    "fill_masked_rows": _fill_masked_rows,
    "generate_harmonic": _generate_harmonic,
}


@pytest.mark.parametrize("writer", sorted(PLAIN_WRITERS))
def test_every_writer_of_the_matrix_invalidates_what_depends_on_it(writer):
    """K = 5, N = 300 (one padded block, fast path), one rank.  A context that has solved and evaluated at f is changed through one
    writer of the C ABI and evaluated again at the same f, first of all, then solved and evaluated once more: log-denominators,
    sums, Gram matrix and the new solve are those of a fresh context given the final matrix directly, and the sums of the solve
    before the change are withdrawn.  Two of the changes are what makes the matrix unusable (a NaN), resp. usable again."""
    K, N = 5, 300
    u, N_k, f = random_problem(K, N, seed=31)
    rng = np.random.default_rng(5)
    start = PLAIN_STARTS.get(writer, lambda u: u)(u)
    with DeviceMatrix.from_host(start) as dm:
        dm.set_Nk(N_k)
        before = plain_outputs(dm, f)
        assert bool(np.isnan(before["logden"]).all()) == bool(np.isnan(start).any())
        if np.isfinite(start).all():
            assert has_solve_sums(dm)
        PLAIN_WRITERS[writer](dm, u, rng)
        assert not has_solve_sums(dm), "the sums of the last solve outlived a change of the matrix"
        got = after_a_write(dm, f)
        final = dm.to_host()
        assert not same(final, start)
    with DeviceMatrix.from_host(final) as fresh:
        fresh.set_Nk(N_k)
        want = after_a_write(fresh, f)
    assert_same(got, want, writer)
    assert not same(got["first logden"], before["logden"])
    assert bool(np.isnan(got["first logden"]).all()) == bool(np.isnan(final).any())


def ext_outputs(e, base, f_base, f_ext):
    """mbar_lognum_ext and mbar_gram_w_ext, the latter with the base's own W^T W (thin rectangle: only the new entries are swept
    for) and without it (the joint panel)."""
    lib, Kt = e._lib, e.K
    out = {"lognum": np.empty(Kt - e.Kb)}
    e._check(lib.mbar_lognum_ext(e._ctx, base._ctx, _dptr(f_base), _dptr(out["lognum"])))
    gram_base = np.ascontiguousarray(base.gram_w(f_base)[0])
    for tag, gb in (("thin", _dptr(gram_base)), ("joint", None)):
        G, ws = np.empty((Kt, Kt)), np.empty(Kt)
        e._check(lib.mbar_gram_w_ext(e._ctx, base._ctx, _dptr(f_base), _dptr(f_ext), gb, _dptr(G), _dptr(ws)))
        out[tag + " gram"], out[tag + " wsum"] = G, ws
    return out


# per writer: (rows the extension starts with, the write), first a change that keeps everything finite, then one that flips the
# poison flag of the extension (the only thing an extension's sweeps take from its own invalidation)
EXT_WRITERS = {
    "rows_sub_from": [
        (lambda rows: rows, lambda e, K, N: e.rows_sub(K + 1, 3, 2, np.linspace(-1.0, 1.0, N))),            # finite -> finite (source: the base)
        (lambda rows: rows, lambda e, K, N: e.rows_sub(K + 3, K, 2, _nan_vector(N))),                        # finite -> NaN (source: its own rows)
    ],
    "rows_rsub_from": [
        (lambda rows: rows, lambda e, K, N: e.rows_rsub(K + 2, 7, 3)),                                       # finite -> finite
        (lambda rows: _with(rows, 4, 11, np.inf), lambda e, K, N: e.rows_rsub(K + 4, 9, 1)),                 # +inf (legal) -> -inf (poison)
    ],
    "rows_obs_from": [
        (lambda rows: rows, lambda e, K, N: e.rows_obs_from_base(K, 2, 5, 3)),                               # finite -> finite
        (lambda rows: _with(rows, 1, 40, np.nan), lambda e, K, N: e.rows_obs_from_base(K + 1, 6, 8, 1)),     # NaN -> finite
    ],
}


@pytest.mark.parametrize("writer", sorted(EXT_WRITERS))
def test_every_writer_of_an_extension_invalidates_what_depends_on_it(writer):
    """The three writers that exist on extensions only (source rows in the base or in the extension itself): a base of K = 120
    states (padded to 128) with 5 appended rows, N = 300.  Normalisers and W^T W of the pair after the write are those of a fresh
    pair that was given the final rows directly -- also when the write is what makes the extension's rows unusable, or usable again."""
    K, R, N = 120, 5, 300
    u, N_k, f = random_problem(K, N, seed=77)
    rng = np.random.default_rng(9)
    rows0 = u[rng.integers(0, K, size=R)] * 1.1 + rng.uniform(-0.5, 0.5, size=(R, 1))
    f_ext = np.linspace(-0.5, 0.5, R)

    def pair(rows):
        base = DeviceMatrix.from_host(u)
        base.set_Nk(N_k)
        e = base.extend(R)
        assert e is not None
        e.upload_rows(K, rows)
        return base, e

    for start, write in EXT_WRITERS[writer]:
        base, e = pair(start(rows0))
        try:
            before = ext_outputs(e, base, f, f_ext)
            write(e, K, N)
            final = download(e, R, N)
            got = ext_outputs(e, base, f, f_ext)
        finally:
            e.close()
            base.close()
        base, e = pair(final)
        try:
            want = ext_outputs(e, base, f, f_ext)
        finally:
            e.close()
            base.close()
        assert_same(got, want, writer)
        assert not same(got["lognum"], before["lognum"])
        poisoned = bool(np.isnan(final).any() or np.isneginf(final).any())
        assert bool(np.isnan(got["lognum"]).all()) == poisoned


# ---- 2. buffers that grow under captured graphs -----------------------------------------------------------------------

def _steps(K):
    f = np.linspace(0.0, 1.5, K)
    f2 = f + 0.05 * np.cos(np.arange(K))
    f2[0] = 0.0
    sci = lambda dm: solve_outputs(*dm.solve_sci(np.zeros(K), maxiter=48, check_convergence=False), prefix="")  # noqa: E731
    return [
        ("solve_sci (captures its batch)", sci),
        ("eval with the Gram matrix (red grows)", lambda dm: dict(zip(("psum", "sumlogden", "gram"), dm.eval(f, gram=True)))),
        ("lognum", lambda dm: {"lognum": dm.lognum(f)}),
        ("logw", lambda dm: {"logw": dm.logw_kn(f)}),
        ("solve_adaptive (captures its batch; ad, P, part_g)",
         lambda dm: solve_outputs(*dm.solve_adaptive(np.zeros(K), tol=1e-12, min_sc_iter=0, history_rows=50), prefix="")),
        ("eval with two candidates", lambda dm: dict(zip(("psum", "sumlogden"), dm.eval(np.stack([f, f2]))[:2]))),
        ("solve_sci again", sci),
    ]


@pytest.mark.parametrize("weighted", [False, True])
def test_buffers_that_grow_under_captured_graphs(weighted):
    """K = 40, N = 2001, all on ONE context: a self-consistent solve captures its batch; then an evaluation with the Gram matrix
    (the reduced outputs outgrow what the graph was captured with), normalisers, log W, an adaptive solve (its own graph and
    buffers), an evaluation of two candidates, and the first solve again.  Every output equals that of the same call on a fresh
    context."""
    K, N = 40, 2001
    u, N_k, _ = random_problem(K, N, seed=K + N)
    c_n = None
    if weighted:  # draw counts of one bootstrap replicate (they sum to N_k within each state's block)
        rng, c_n, first = np.random.default_rng(K), np.zeros(N), 0
        for n_k in N_k:
            if n_k > 0:
                c_n[first:first + n_k] = np.bincount(rng.integers(0, n_k, size=n_k), minlength=n_k)
            first += n_k

    def context():
        dm = DeviceMatrix.from_host(u)
        dm.set_Nk(N_k)
        dm.set_sample_weights(c_n)
        return dm

    steps = _steps(K)
    with context() as dm:
        got = [step(dm) for _, step in steps]
    assert same(got[0]["f"], got[-1]["f"])
    for (tag, step), g in zip(steps, got):
        with context() as fresh:
            assert_same(g, step(fresh), tag)


# ---- 3. the first call of a fresh context -----------------------------------------------------------------------------

def _counts(N, seed):
    """small integer multiplicities, some of them zero"""
    return np.random.default_rng(seed).integers(0, 4, size=N).astype(np.float64)


# (K, N, gram_quad or None: the default): few states (the evaluation sweep's records are the small ones, the Gram panel's the large
# ones), one full 128-state panel, 129 .. 256 states as ONE panel and as 128-state panels with their rectangles, and 257 .. 1024
# states (the split evaluation sweep, then a plan of three diagonal panels and four rectangles of unequal record sizes)
FIRST_CALLS = [(16, 4000, None), (128, 3000, None), (200, 3000, 1), (200, 3000, 0), (300, 2000, None)]


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("K,N,quad", FIRST_CALLS)
def test_first_evaluation_with_gram_of_a_fresh_context(K, N, quad, weighted):
    """An evaluation with the Gram matrix as the FIRST call of a context sizes the per-wave records and the reduction scratch for
    the evaluation sweep and for every launch of the Gram plan before anything is queued.  Its outputs are those of the same call
    repeated on that context (nothing grows any more), and those of a context whose buffers mbar_gram_w grew first."""
    u, N_k, f = random_problem(K, N, seed=K + N)
    c_n = _counts(N, K) if weighted else None

    def context():
        dm = DeviceMatrix.from_host(u)
        dm.set_Nk(N_k)
        dm.set_sample_weights(c_n)
        if quad is not None:
            dm.set_option("gram_quad", quad)
        return dm

    names = ("psum", "sumlogden", "gram")
    with context() as dm:
        first = dict(zip(names, dm.eval(f, gram=True)))
        again = dict(zip(names, dm.eval(f, gram=True)))
    with context() as grown:
        grown.gram_w(f)
        after = dict(zip(names, grown.eval(f, gram=True)))
    assert np.isfinite(first["gram"]).all() and first["gram"].shape == (K, K)
    assert_same(again, first, "the same call again")
    assert_same(after, first, "after mbar_gram_w grew the buffers")


def test_first_thin_gram_of_a_fresh_extension():
    """A base of K = 120 states (padded to 128), N = 3000, with 5 appended rows: W^T W of the pair from the base's kept W^T W -- the
    144-row rectangle, then the 16 x 16 block of the appended rows, whose launch geometry and record size differ -- as the first
    call of the extension and once more: the two launches' buffers are sized together, and both calls return the same bits."""
    K, R, N = 120, 5, 3000
    u, N_k, f = random_problem(K, N, seed=K + N)
    rng = np.random.default_rng(R)
    rows = u[rng.integers(0, K, size=R)] * 1.1 + rng.uniform(-0.5, 0.5, size=(R, 1))
    f_all = np.concatenate([f, np.linspace(-0.5, 0.5, R)])
    with DeviceMatrix.from_host(u) as base:
        base.set_Nk(N_k)
        e = base.extend(R)
        assert e is not None
        try:
            e.upload_rows(K, rows)
            first = dict(zip(("gram", "wsum"), e.gram_w(f_all)))
            again = dict(zip(("gram", "wsum"), e.gram_w(f_all)))
        finally:
            e.close()
    assert np.isfinite(first["gram"]).all() and first["gram"].shape == (K + R, K + R)
    assert_same(again, first, "the same call again")


# ---- 4. the self-consistent iteration on the evaluation sweeps that are not the fast one ----------------------------------------

@pytest.mark.parametrize("K,N,force_generic", [(300, 2000, 0), (40, 2001, 1)])
def test_solve_sci_iterates_on_the_device_copy_of_aden(K, N, force_generic):
    """More than 256 states (the split sweep) and force_generic = 1 (the layout-agnostic kernels): mbar_solve_sci drives run_lse
    itself, and between two sweeps only the update kernel writes the next a_k = f_k + ln N_k, on the device.  The context has
    evaluated at ANOTHER f before, so the host staging holds that call's a_k: a sweep that took its a_k from anywhere but the
    device vector would stall there.  The solve converges, and what it returns is a fixed point of the oracle's self-consistent
    update: with the relative stop test at tol = 1e-9 and |f| < 10 the last step was below 1e-8, rounding of the sums over 2000
    samples is orders below that, so 1e-7 bounds the residual."""
    from oracle import mbar_oracle as oracle

    u, N_k, f_other = random_problem(K, N, seed=K + N)
    with DeviceMatrix.from_host(u) as dm:
        dm.set_Nk(N_k)
        dm.set_option("force_generic", force_generic)
        dm.eval(f_other + 1.0)
        f, res = dm.solve_sci(np.zeros(K), tol=1e-9, maxiter=20000)
    assert res["success"] and res["iterations"] > 2
    sampled = N_k > 0
    assert np.abs(f[sampled]).max() < 10.0
    step = oracle.self_consistent_update(u, N_k.astype(np.float64), f)
    assert np.abs((step - step[0])[sampled] - (f - f[0])[sampled]).max() < 1e-7
