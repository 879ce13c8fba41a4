"""The primitives every estimate of the expectation family is built from, on the MI355X, against the long-double stand-in of
tests/expect_standin.py: ``mbar_lognum`` (k_lognum, k_lognum_merge, the multiplicity fold k_shift_logden, the merge across ranks),
``mbar_logw`` / ``mbar_w`` (k_logw, the row-block staging of logw_impl), ``mbar_gram_w`` (run_gram over every gram_plan: k_gram
diagonal panels clamped and unclamped, k_gram_quad trimmed and untrimmed, the 64 x 128 rectangles in both orientations, unpack_gram,
gram_operand_sums) and the extension forms ``mbar_lognum_ext`` / ``mbar_gram_w_ext`` (thin rectangle, joint 192- / 256-row panel of
k_gram_quad_split at every seam position).  The case tables, their data forms (plain, inf, weighted) and the path each id names are
those of the stand-in module; tests/test_expect_standin_host.py holds the conditions on the inputs and the path assertions.

The tile loops of the Gram sweeps run more than one trip only when a wave sees more than one tile: option ``grid_blocks`` = 1 forces
one workgroup (tests/test_gpu_fused_tile_loop.py has the N-to-tiles table), on an extension through ``mbar_ctx_set_option`` of its
own context.

Tolerances, from the project and not from the code under test:
  log W      bitwise equal to ``(f[:, None] - u) - logden_dev[None, :]`` in numpy float64: the kernel forms exactly these two
             subtractions in this order; ``-inf`` where the expression gives it; no NaN
  W          against the long-double exp of the device's own log W: |W - ref| <= 4 u |ref| (u = 2^-53; the 2 u that
             profiles/device_math_accuracy.txt section 3 charges the library exp, with that file's margin of 2), within 2 subnormal
             ulps below 2^-1022, exact 0 where log W is -inf
  lognum     rtol 1e-12, atol 1e-12 max(1, max_n |logden_n|) (tests/test_expectations.py; the scale term is the (A + B |m|) u growth
             of the log-denominator's error); -inf where the stand-in says so.  The device's logden is held to the same.
  W^T W      rtol 1e-10, atol 0 (tests/test_gpu_scan_pairs.py); exact 0 where the reference is exactly 0
  wsum       rtol 1e-10
Every case prints its worst errors (``-s``); profiles/expectation_primitives_matrix.txt is written from that output."""
import contextlib
import functools
import time

import numpy as np
import pytest

from pymbar_amd.device import DeviceMatrix, LoopbackGroup, _dptr
from tests import expect_standin as es
from tests.test_gpu_loopback import run_ranks

pytestmark = pytest.mark.gpu

U = 2.0**-53
TINY = np.finfo(np.float64).tiny
SUB_ULP = 2.0**-1074
R = es.R


@contextlib.contextmanager
def device_matrix(case, opts=None, grid=0):
    """The case's matrix with its N_k, multiplicities and options; grid_blocks goes back to 0 whatever happens"""
    with DeviceMatrix.from_host(case["u"]) as dm:
        dm.set_Nk(case["N_k"])
        if case["c"] is not None:
            dm.set_sample_weights(case["c"])
        for key, value in (opts or {}).items():
            dm.set_option(key, value)
        try:
            dm.set_option("grid_blocks", grid)
            yield dm
        finally:
            dm.set_option("grid_blocks", 0)


def worst_rel(got, want):
    """max |got - want| / |want| over the entries the reference has; where it is exactly 0 the device must be too"""
    want = np.asarray(want, dtype=R)
    zero = want.astype(np.float64) == 0.0
    assert np.all(got[zero] == 0.0), "an entry whose reference is exactly 0 is %g" % np.max(np.abs(got[zero]))
    assert np.all(np.isfinite(got))
    if zero.all():
        return 0.0
    return float(np.max(np.abs(got.astype(R)[~zero] - want[~zero]) / np.abs(want[~zero])))


def check_log_sums(got, want, scale, what):
    """lognum (or logden) against the stand-in: -inf where it says so; returns the worst |error| over its bound"""
    want = np.asarray(want, dtype=R)
    dead = np.isneginf(want.astype(np.float64))
    assert np.array_equal(np.isneginf(got), dead), (what, got, want)
    assert np.all(np.isfinite(got[~dead])), what
    if dead.all():
        return 0.0
    err = np.abs(got.astype(R)[~dead] - want[~dead])
    bound = 1e-12 * np.abs(want[~dead]) + 1e-12 * max(1.0, scale)
    worst = float(np.max(err / bound))
    print("   %s: worst |error| %.3e, %.3g of its bound (scale %.3g)" % (what, float(np.max(err)), worst, scale))
    assert worst <= 1.0, (what, float(np.max(err)))
    return worst


def check_lognum(dm, case, lognum_dev, ld=None, rows=None):
    """The device's logden and lognum (of the matrix, or of appended ``rows``) against the stand-in"""
    ld = es.logden(case["u"], case["N_k"], case["f"]) if ld is None else ld
    scale = float(np.max(np.abs(ld)))
    check_log_sums(dm.logden(case["f"]), ld, scale, "logden")
    want = es.lognum(case["u"] if rows is None else rows, None, None, case["c"], ld=ld)
    check_log_sums(lognum_dev, want, scale, "lognum")


def check_gram(got, want, zero_rows, what):
    """``(W^T W, wsum)`` of one call against the stand-in's: symmetric to the bit, exact zeros, rtol 1e-10"""
    (G, ws), (Gw, wsw) = got, want
    assert G.tobytes() == np.ascontiguousarray(G.T).tobytes(), what + ": W^T W is not its transpose"
    for k in zero_rows:
        assert np.all(G[k] == 0.0) and np.all(G[:, k] == 0.0) and ws[k] == 0.0, (what, k)
    eG, ew = worst_rel(G, Gw), worst_rel(ws, wsw)
    print("   %s: worst rel error W^T W %.3e, wsum %.3e" % (what, eG, ew))
    assert eG <= 1e-10 and ew <= 1e-10, (what, eG, ew)


# ---- A: lognum ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", es.lognum_seam_cases() + es.LOGNUM_CHUNK_CASES, ids=es.lognum_case_id)
def test_lognum_against_standin(spec):
    K, N, form = spec[:3]
    case = es.build(K, N, form)
    t0 = time.perf_counter()
    with device_matrix(case) as dm:
        got = dm.lognum(case["f"])
        again = dm.lognum(case["f"])
        ms = 1e3 * (time.perf_counter() - t0)
        print("\n[A] %s plan (tiles, per chunk, chunks, first/last trips) %s  %.1f ms" % (es.lognum_case_id(spec), es.lognum_plan(K, N), ms))
        assert got.tobytes() == again.tobytes()
        check_lognum(dm, case, got)
    if K > 256:
        es.build.cache_clear()


def test_lognum_multi_rank_merge():
    """Three logical ranks on unequal column shards: a state that is +inf on a whole shard (local maximum -inf: its record must
    drop out, not poison the sum) and one whose shard maxima lie 800 apart (that shard's rescale exp(hm - gm) is 0)"""
    m = es.MERGE_CASE
    case = es.build_merge_case()
    u, N_k, f = case["u"], case["N_k"], case["f"]
    with LoopbackGroup(len(m["shards"])) as grp:
        def worker(r):
            with DeviceMatrix.from_host(u, columns=m["shards"][r]) as dm:
                dm.set_loopback(grp, r)
                dm.set_Nk(N_k)
                out = dm.lognum(f), dm.logden(f)
                dm.comm_destroy()
                return out

        ranks = run_ranks(len(m["shards"]), worker, timeout=60.0)
    for ln, _ in ranks[1:]:
        assert ln.tobytes() == ranks[0][0].tobytes()  # every rank: identical bits
    ld = es.logden(u, N_k, f)
    scale = float(np.max(np.abs(ld)))
    print("\n[A] multi-rank merge K9-N1000 shards 300/423/277")
    check_log_sums(np.concatenate([r[1] for r in ranks]), ld, scale, "logden")
    check_log_sums(ranks[0][0], es.lognum(u, N_k, f, ld=ld), scale, "lognum")
    with DeviceMatrix.from_host(u) as one:
        one.set_Nk(N_k)
        check_log_sums(one.lognum(f), es.lognum(u, N_k, f, ld=ld), scale, "lognum, one rank")


def test_lognum_extreme_column_offsets():
    case = es.build_offset_case()
    with device_matrix(case) as dm:
        print("\n[A] extreme offsets K8-N257 (0, +-1e4 per column)")
        check_lognum(dm, case, dm.lognum(case["f"]))


# ---- B: log W and W -------------------------------------------------------------------------------------------------------------------
def logw_bits(case, ld_dev):
    with np.errstate(invalid="ignore"):
        return (case["f"][:, None] - case["u"]) - ld_dev[None, :]


def check_w(W, lw, what):
    """The device's W against the long-double exp of its own log W, every entry (in column blocks)"""
    assert np.all(W[np.isneginf(lw)] == 0.0) and np.all(W >= 0.0) and np.all(np.isfinite(W))
    worst_n = worst_s = 0.0
    for sl in es._col_blocks(*W.shape):
        ref = np.exp(lw[:, sl].astype(R))
        err = np.abs(W[:, sl].astype(R) - ref)
        normal = ref.astype(np.float64) >= TINY
        if normal.any():
            worst_n = max(worst_n, float(np.max(err[normal] / ref[normal])) / U)
        if (~normal).any():
            worst_s = max(worst_s, float(np.max(err[~normal])) / SUB_ULP)
    print("   %s: worst error of W %.3f u relative (normal), %.3f subnormal ulps below 2^-1022" % (what, worst_n, worst_s))
    assert worst_n <= 4.0 and worst_s <= 2.0, (what, worst_n, worst_s)


@pytest.mark.parametrize("K,N", es.logw_cases(), ids=lambda v: str(v))
def test_logw_and_w_elementwise(K, N):
    plain_bits = None
    for form in es.forms_for(K, es.FORMS):
        case = es.build(K, N, form)
        with device_matrix(case) as dm:
            t0 = time.perf_counter()
            ld_dev, lw, W = dm.logden(case["f"]), dm.logw_kn(case["f"]), dm.w_kn(case["f"])
            ms = 1e3 * (time.perf_counter() - t0)
        print("\n[B] K%d-N%d-%s plan (pitch, rows per block, blocks, trips) %s  %.1f ms" % (K, N, form, es.logw_plan(K, N), ms))
        assert not np.any(np.isnan(lw)) and not np.any(np.isnan(ld_dev))
        assert lw.tobytes() == logw_bits(case, ld_dev).tobytes(), "log W is not (f - u) - logden to the bit"
        assert np.array_equal(np.isneginf(lw), case["u"] == np.inf)
        check_w(W, lw, form)
        if form == "plain":
            plain_bits = lw.tobytes(), W.tobytes()
        if form == "weighted":  # the multiplicities must not change log W
            assert (lw.tobytes(), W.tobytes()) == plain_bits


def test_logw_grid_stride_second_trip():
    K, N = es.LOGW_STRIDE_CASE
    case = es.build(K, N, "plain")
    with device_matrix(case) as dm:
        t0 = time.perf_counter()
        ld_dev, lw, W = dm.logden(case["f"]), dm.logw_kn(case["f"]), dm.w_kn(case["f"])
        ms = 1e3 * (time.perf_counter() - t0)
    print("\n[B] K%d-N%d-plain plan %s  %.1f ms" % (K, N, es.logw_plan(K, N), ms))
    assert lw.tobytes() == logw_bits(case, ld_dev).tobytes()
    check_w(W, lw, "all %d entries" % W.size)
    es.build.cache_clear()


def test_logw_c_abi_with_a_wider_output_pitch():
    K, N, extra = es.LOGW_LD_CASE
    case = es.build(K, N, "inf")
    sentinel = -12345.678
    with device_matrix(case) as dm:
        f = np.ascontiguousarray(case["f"])
        want_lw, want_w = dm.logw_kn(f), dm.w_kn(f)
        for entry, want in ((dm._lib.mbar_logw, want_lw), (dm._lib.mbar_w, want_w)):
            out = np.full((K, N + extra), sentinel)
            dm._check(entry(dm._ctx, _dptr(f), _dptr(out), N + extra))
            assert np.all(out[:, N:] == sentinel), "columns behind N were written"
            assert np.ascontiguousarray(out[:, :N]).tobytes() == want.tobytes()
    print("\n[B] K%d-N%d-inf ld_out = N + %d: the %d columns behind N untouched, the rest the bits of ld_out = N" % (K, N, extra, extra))


def test_w_underflows_gradually():
    case = es.build_underflow_case()
    with device_matrix(case) as dm:
        ld_dev, lw, W = dm.logden(case["f"]), dm.logw_kn(case["f"]), dm.w_kn(case["f"])
    assert lw.tobytes() == logw_bits(case, ld_dev).tobytes()
    n = len(es.UNDERFLOW_TARGETS)
    np.testing.assert_allclose(lw[2, :n], es.UNDERFLOW_TARGETS, rtol=0, atol=1e-9)
    sub = (W[2] > 0) & (W[2] < TINY)
    print("\n[B] underflow K3-N64: %d subnormal, %d zero, %d normal below 1e-300" % (sub.sum(), np.sum(W[2] == 0), np.sum((W[2] >= TINY) & (W[2] < 1e-300))))
    assert sub.sum() >= 4 and np.sum(W[2, :n] == 0.0) >= 4 and np.sum((W[2] >= TINY) & (W[2] < 1e-300)) >= 4
    check_w(W, lw, "underflow")


def test_logw_second_staging_block():
    """K = 5, N = 2^23 + 1: three rows fit the 256 MiB staging buffer, rows 3 and 4 go through its second block.  Bitwise in float64."""
    K, N = es.LOGW_STAGE_CASE
    assert es.logw_plan(K, N)[1:3] == (3, 2)
    case = es.build(K, N, "plain")
    with device_matrix(case) as dm:
        ld_dev = dm.logden(case["f"])
        t0 = time.perf_counter()
        lw = dm.logw_kn(case["f"])
        ms = 1e3 * (time.perf_counter() - t0)
    print("\n[B] K%d-N%d-plain plan %s  logw_kn %.1f ms" % (K, N, es.logw_plan(K, N), ms))
    for k in range(K):
        assert lw[k].tobytes() == ((case["f"][k] - case["u"][k]) - ld_dev).tobytes(), k
    es.build.cache_clear()


# ---- C: gram_w ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def gram_reference(K, N, form):
    case = es.build(K, N, form)
    G, ws = es.gram_w(case["u"], case["N_k"], case["f"], case["c"])
    return case, (G, ws)


def run_gram_case(tag, K, N, opts, form, grid):
    case, want = gram_reference(K, N, form)
    with device_matrix(case, opts, grid) as dm:
        t0 = time.perf_counter()
        G, ws = dm.gram_w(case["f"])
        ms = 1e3 * (time.perf_counter() - t0)
        G2, ws2 = dm.gram_w(case["f"])
    print("\n[C] %s  %.1f ms" % (tag, ms))
    assert G.tobytes() == G2.tobytes() and ws.tobytes() == ws2.tobytes(), "two identical calls differ"
    check_gram((G, ws), want, [] if form != "inf" else [case["allinf"]], "gram_w")


@pytest.mark.parametrize("spec", es.gram_plan_cases(), ids=es.gram_plan_id)
def test_gram_w_plans(spec):
    K, opts, path, form = spec
    run_gram_case(es.gram_plan_id(spec) + " default grid: at most one tile per stream", K, es.GRAM_PLAN_N, opts, form, 0)


@pytest.mark.parametrize("K,state,path", es.GRAM_ZERO_ROW_CASES)
def test_gram_w_is_exactly_zero_along_an_all_inf_row(K, state, path):
    """The all-+inf row inside a chosen block of a one-read panel, default grid and one workgroup: exact zeros along it, same bits
    from call to call (an accumulator that starts from what the previous launch left in its register fails both)"""
    case = es.build_zero_row_case(K, state)
    want = es.gram_w(case["u"], case["N_k"], case["f"])
    for grid in (0, 1):
        with device_matrix(case, grid=grid) as dm:
            runs = [dm.gram_w(case["f"]) for _ in range(3)]
        print("\n[C] zero row K%d state %d %s grid_blocks %d" % (K, state, path, grid))
        for G, ws in runs[1:]:
            assert G.tobytes() == runs[0][0].tobytes() and ws.tobytes() == runs[0][1].tobytes()
        check_gram(runs[0], want, [state], "gram_w")


@pytest.mark.parametrize("spec", es.gram_tile_cases(), ids=es.gram_tile_id)
def test_gram_w_tile_counts(spec):
    K, N, opts, path, tiles, form = spec
    run_gram_case(es.gram_tile_id(spec) + " one workgroup", K, N, opts, form, 1)


# ---- D: extensions ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spec", es.ext_cases(), ids=es.ext_case_id)
def test_extension_lognum_and_gram(spec):
    Kb, R_, N, grid, paths, form = spec
    case = es.build_ext(Kb, R_, N, form)
    fb, fe = np.ascontiguousarray(case["f"]), np.ascontiguousarray(case["f_ext"])
    Kt = Kb + R_
    with device_matrix(case) as base:
        e = base.extend(R_)
        assert e is not None, "the library refused an extension the table holds"
        with e:
            e.upload_rows(Kb, case["rows"])
            lib = e._lib
            try:
                e._check(lib.mbar_ctx_set_option(e._ctx, b"grid_blocks", grid))
                ln = np.empty(R_)
                e._check(lib.mbar_lognum_ext(e._ctx, base._ctx, _dptr(fb), _dptr(ln)))
                assert e.lognum(np.concatenate([fb, fe]))[Kb:].tobytes() == ln.tobytes()
                got = {}
                for kind in sorted(paths):
                    gb = np.ascontiguousarray(base.gram_w(fb)[0]) if kind == "thin" else None
                    runs = []
                    for _ in range(2):
                        G, ws = np.empty((Kt, Kt)), np.empty(Kt)
                        t0 = time.perf_counter()
                        e._check(lib.mbar_gram_w_ext(e._ctx, base._ctx, _dptr(fb), _dptr(fe), _dptr(gb), _dptr(G), _dptr(ws)))
                        runs.append((G, ws, 1e3 * (time.perf_counter() - t0)))
                    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes(), kind
                    got[kind] = runs[0]
                print("\n[D] %s  %s" % (es.ext_case_id(spec), "  ".join("%s %.1f ms" % (k, v[2]) for k, v in got.items())))
                check_lognum(base, case, ln, rows=case["rows"])
            finally:
                e._check(lib.mbar_ctx_set_option(e._ctx, b"grid_blocks", 0))
    want = es.gram_w_ext(case["u"], case["rows"], case["N_k"], case["f"], case["f_ext"], case["c"])
    zero = [] if form != "inf" else [case["allinf"], Kb + case["ext_allinf"]]
    for kind, (G, ws, _) in got.items():
        check_gram((G, ws), want, zero, kind + " " + paths[kind])


def test_extension_refusals_follow_the_host_arithmetic():
    for Kb, R_ in es.EXT_REFUSALS:
        assert es.ext_plan(Kb, R_) is None
        with DeviceMatrix.empty(Kb, 64) as base:
            e = base.extend(R_)
            try:
                assert e is None, (Kb, R_)
            finally:
                if e is not None:
                    e.close()
    for Kb, R_ in [(5, 113), (100, 17), (128, 1), (128, 128), (17, 224)]:  # the edges on the accepting side
        assert es.ext_plan(Kb, R_) is not None
        with DeviceMatrix.empty(Kb, 64) as base:
            e = base.extend(R_)
            assert e is not None, (Kb, R_)
            e.close()
