"""The stand-in of the expectation family's primitives (tests/expect_standin.py) and its case tables, on the CPU: the stand-in against
``oracle.mbar_oracle`` and ``tests.cpu_standin.OracleMatrix`` on small problems; every case of the tables built and run through the
stand-in alone (the staging case of log W, 4.2e7 entries, reduced to its arithmetic), with the conditions the device test relies on; and
every case against the path its id names, re-derived from the shape the way the library's host code chooses it (padded_K, gram_plan,
lognum_tiles_per_chunk / lognum_chunks, live_blocks and the trim rule, need / Kp_ext / split_rows of an extension, rows_per of
logw_impl) -- a table entry that no longer lands where its id says fails here."""
import numpy as np
import pytest

from oracle import mbar_oracle as oracle
from tests import expect_standin as es
from tests.cpu_standin import OracleMatrix

TINY = np.finfo(np.float64).tiny


def as64(x):
    return np.asarray(x, dtype=np.float64)


# ---- the stand-in against the project's float64 oracles -----------------------------------------------------------------------------
@pytest.mark.parametrize("K,N,form", [(5, 300, "plain"), (9, 211, "inf"), (17, 400, "weighted"), (40, 333, "plain")])
def test_standin_matches_the_float64_oracles(K, N, form):
    case = es.build(K, N, form)
    u, N_k, f, c = case["u"], case["N_k"], case["f"], case["c"]
    ld = es.logden(u, N_k, f)
    np.testing.assert_allclose(as64(ld), oracle.log_denominator(u, N_k.astype(float), f), rtol=1e-13, atol=1e-13)
    lw = as64(es.logw(u, N_k, f))
    with np.errstate(invalid="ignore"):
        np.testing.assert_allclose(lw, oracle.mbar_log_W_nk(u, N_k.astype(float), f).T, rtol=1e-13, atol=1e-12)
        np.testing.assert_allclose(as64(es.w(u, N_k, f)), oracle.mbar_W_nk(u, N_k.astype(float), f).T, rtol=1e-11, atol=0)
    om = OracleMatrix(u)
    om.set_Nk(N_k)
    if c is not None:
        om.set_sample_weights(c)  # (the gathered replicate)
    G, ws = es.gram_w(u, N_k, f, c)
    ln = as64(es.lognum(u, N_k, f, c))
    with np.errstate(divide="ignore", invalid="ignore"):
        Go, wso = om.gram_w(f)
        lno = om.lognum(f)
    np.testing.assert_allclose(as64(G), Go, rtol=1e-11, atol=0)
    np.testing.assert_allclose(as64(ws), wso, rtol=1e-12, atol=0)
    finite = np.isfinite(ln)
    np.testing.assert_allclose(ln[finite], lno[finite], rtol=1e-12, atol=1e-12)
    if form == "inf":
        k = case["allinf"]
        assert ln[k] == -np.inf and finite.sum() == K - 1
        assert np.all(as64(G)[k] == 0.0) and np.all(as64(G)[:, k] == 0.0) and ws[k] == 0.0
    # sum_k N_k W_nk = 1: the identity mbar_gram_w takes wsum from
    np.testing.assert_allclose(as64(N_k.astype(es.R) @ G), as64(ws), rtol=1e-15)


def test_shards_and_extension_forms():
    case = es.build_ext(17, 20, 300, "inf")
    u, N_k, f, rows, f_ext = case["u"], case["N_k"], case["f"], case["rows"], case["f_ext"]
    ld = es.logden(u, N_k, f)
    whole = es.lognum(u, N_k, f)
    parts = [es.lognum_parts(u[:, a:b], ld[a:b]) for a, b in ((0, 1), (1, 130), (130, 300))]
    got = es.combine_parts(parts)
    fin = np.isfinite(whole)
    assert np.array_equal(fin, np.isfinite(got)) and np.all(np.abs(got[fin] - whole[fin]) < 1e-17)
    uu, NN, ff = es.stacked(u, rows, N_k, f, f_ext)
    le = es.lognum_ext(u, rows, N_k, f)
    both = es.lognum(uu, NN, ff)
    assert le[case["ext_allinf"]] == -np.inf and np.isfinite(np.delete(le, case["ext_allinf"])).all()
    np.testing.assert_array_equal(as64(le), as64(both[17:]))
    G, ws = es.gram_w_ext(u, rows, N_k, f, f_ext)
    Gb, wb = es.gram_w(u, N_k, f)
    assert np.array_equal(G[:17, :17], Gb) and np.array_equal(ws[:17], wb) and np.array_equal(G, G.T)
    assert np.all(G[17 + case["ext_allinf"]] == 0)


# ---- the conditions on the inputs ---------------------------------------------------------------------------------------------------
def check_forms(case):
    u, N_k, c = case["u"], case["N_k"], case["c"]
    K, N = u.shape
    assert N_k.sum() == N and N_k[0] > 0 and np.all(np.abs(case["f"]) <= 3.0) and case["f"][0] == 0.0
    if K >= 4:
        assert np.sum(N_k == 0) >= 2
    assert np.all(np.isfinite(u[case["s_n"], np.arange(N)]))  # a finite sampled entry in every column
    assert not np.any(np.isnan(u)) and not np.any(u == -np.inf)
    if case["form"] == "inf":
        k = case["allinf"]
        assert N_k[k] == 0 and np.all(u[k] == np.inf) and np.isinf(u).sum() >= N
    else:
        assert np.all(np.isfinite(u))
    if case["form"] == "weighted":
        assert np.all(c == np.round(c)) and es.weights_ok(c)
        start = 0
        for n_k in N_k:  # draws WITHIN each state
            assert c[start:start + n_k].sum() == n_k
            start += n_k
        if N >= 16:
            assert np.mean(c == 0) >= 0.2 and c.max() >= 3
        elif N >= 3:
            assert np.any(c == 0) and c.max() >= 2
    else:
        assert c is None


def check_lognum(ln, allinf_rows):
    ln = as64(ln)
    for k in range(len(ln)):
        assert (ln[k] == -np.inf) if k in allinf_rows else np.isfinite(ln[k]), (k, ln[k])


def check_gram(G, ws, zero_rows):
    G, ws = as64(G), as64(ws)
    assert np.array_equal(G, G.T)
    nz = G != 0.0
    assert np.all(G[nz] > 1e-280) and np.all(G[nz] >= TINY)
    rows_zero = np.where(~nz.any(axis=1))[0]
    assert sorted(rows_zero) == sorted(zero_rows)  # exact zeros: the all-+inf rows and nothing else
    assert np.all(np.isfinite(ws)) and np.all(np.delete(ws, list(zero_rows)) > 0)


@pytest.mark.parametrize("spec", es.lognum_seam_cases(), ids=es.lognum_case_id)
def test_lognum_seam_case(spec):
    K, N, form = spec
    case = es.build(K, N, form)
    check_forms(case)
    check_lognum(es.lognum(case["u"], case["N_k"], case["f"], case["c"]), [] if form != "inf" else [case["allinf"]])
    ntiles, tpc, chunks, _ = es.lognum_plan(K, N)
    assert tpc == 1 and chunks == ntiles == (N + 63) // 64 <= 256


@pytest.mark.parametrize("spec", es.LOGNUM_CHUNK_CASES, ids=es.lognum_case_id)
def test_lognum_chunk_case_reaches_its_loop(spec):
    K, N, form, tiles, tpc, chunks, last = spec
    got = es.lognum_plan(K, N)
    assert got[:3] == (tiles, tpc, chunks) and got[3][1] == last
    if tpc == 1:
        assert chunks > 256  # k_lognum_merge walks its strided loop a second time (256 threads)
    if tpc == 2:
        assert got[3][0] == (1, 0, 0) and last == (0, 1, 1)  # one pair trip; a full tile plus the ragged one
    if tpc == 3:
        assert got[3][0] == (1, 1, 0) and last == (0, 0, 1)  # pair plus single; the ragged tile alone
    assert N % 64 != 0
    case = es.build(K, N, form)
    check_forms(case)
    check_lognum(es.lognum(case["u"], case["N_k"], case["f"], case["c"]), [])
    if K > 256:
        es.build.cache_clear()


def test_lognum_merge_and_offset_cases():
    m = es.MERGE_CASE
    case = es.build_merge_case()
    u, N_k, f = case["u"], case["N_k"], case["f"]
    assert [b - a for a, b in m["shards"]] == [300, 423, 277] and m["shards"][-1][1] == m["N"]
    ld = es.logden(u, N_k, f)
    parts = [es.lognum_parts(u[:, a:b], ld[a:b]) for a, b in m["shards"]]
    assert parts[m["inf_shard"]][0][m["inf_state"]] == -np.inf
    assert sum(np.isfinite(p[0][m["inf_state"]]) for p in parts) == 2
    far = [float(p[0][m["far_state"]]) for p in parts]
    assert max(far) - far[m["far_shard"]] > 600 and np.exp(far[m["far_shard"]] - max(far)) == 0.0
    check_lognum(es.combine_parts(parts), [])
    np.testing.assert_allclose(as64(es.combine_parts(parts)), as64(es.lognum(u, N_k, f)), rtol=1e-17)
    case = es.build_offset_case()
    off = case["offsets"]
    assert set(off) == {0.0, 1e4, -1e4} and np.array_equal(case["u"] - off[None, :] + off[None, :], case["u"])
    ld = es.logden(case["u"], case["N_k"], case["f"])
    assert 9e3 < np.max(np.abs(as64(ld))) < 1.1e4
    check_lognum(es.lognum(case["u"], case["N_k"], case["f"]), [])


@pytest.mark.parametrize("K,N", es.logw_cases())
def test_logw_case(K, N):
    for form in es.forms_for(K, es.FORMS):
        case = es.build(K, N, form)
        check_forms(case)
        lw = as64(es.logw(case["u"], case["N_k"], case["f"]))
        assert not np.any(np.isnan(lw)) and not np.any(lw == np.inf)
        assert np.array_equal(lw == -np.inf, case["u"] == np.inf)
    plain, weighted = es.build(K, N, "plain"), es.build(K, N, "weighted")
    assert np.array_equal(plain["u"], weighted["u"]) and np.array_equal(plain["f"], weighted["f"])  # same matrix, so the same log W
    ld, rows_per, blocks, trips = es.logw_plan(K, N)
    assert blocks == 1 and trips == 1 and ld >= N


def test_logw_special_cases_reach_their_paths():
    assert es.logw_plan(*es.LOGW_STRIDE_CASE)[2:] == (1, 2)
    assert es.logw_plan(es.LOGW_STRIDE_CASE[0], 524288)[3] == 1
    case = es.build(*es.LOGW_STRIDE_CASE, "plain")
    check_forms(case)
    lw = as64(es.logw(case["u"], case["N_k"], case["f"]))
    wt = as64(es.w(case["u"], case["N_k"], case["f"]))
    assert np.all(np.isfinite(lw)) and np.all(wt > 0.0) and np.all(wt < 1.0)
    es.build.cache_clear()
    # (the one case reduced to its arithmetic: 4.2e7 entries; the device test compares it bitwise in float64)
    K, N = es.LOGW_STAGE_CASE
    ld, rows_per, blocks, _ = es.logw_plan(K, N)
    assert (ld, rows_per, blocks) == (2**23 + 64, 3, 2)
    assert es.logw_plan(K, 6710800)[1:3] == (5, 1)  # (a second block takes more than 256 MiB of log W: K ld > 2^25)
    K, N, extra = es.LOGW_LD_CASE
    assert extra == 3 and es.logw_plan(K, N)[2:] == (1, 1)
    case = es.build_underflow_case()
    wt = as64(es.w(case["u"], case["N_k"], case["f"]))[2]
    assert np.sum((wt > 0) & (wt < TINY)) >= 4 and np.sum(wt == 0.0) >= 4 and np.sum((wt >= TINY) & (wt < 1e-300)) >= 4
    lw = as64(es.logw(case["u"], case["N_k"], case["f"]))[2, :len(es.UNDERFLOW_TARGETS)]
    np.testing.assert_allclose(lw, es.UNDERFLOW_TARGETS, rtol=0, atol=1e-9)


def gram_reference_conditions(case):
    G, ws = es.gram_w(case["u"], case["N_k"], case["f"], case["c"])
    check_gram(G, ws, [] if case["form"] != "inf" else [case["allinf"]])


@pytest.mark.parametrize("spec", es.gram_plan_cases(), ids=es.gram_plan_id)
def test_gram_plan_case(spec):
    K, opts, path, form = spec
    assert es.gram_path(K, form, **opts) == path
    assert max(es.stream_tiles(es.GRAM_PLAN_N, "workgroup" if path.startswith("quad") else "wave")) == 1
    case = es.build(K, es.GRAM_PLAN_N, form)
    check_forms(case)
    for border in (128, 256):
        if K > border:  # a state on either side of every panel border is unsampled
            assert case["N_k"][border - 1] == 0 and case["N_k"][border] == 0
    gram_reference_conditions(case)


@pytest.mark.parametrize("K,state,path", es.GRAM_ZERO_ROW_CASES)
def test_gram_zero_row_case(K, state, path):
    assert es.gram_path(K, "inf") == path
    case = es.build_zero_row_case(K, state)
    check_forms(case)
    assert case["allinf"] == state
    gram_reference_conditions(case)


def test_gram_plan_table_covers_the_plans():
    paths = {p for _, _, p, _ in es.gram_plan_cases()}
    for nb in (1, 2, 3, 4, 5, 6, 8):
        assert any(p.startswith("diag%dx1-" % nb) for p in paths)
    assert {"diag8x1-2buf-clamped", "diag8x1-2buf-unclamped", "diag5x1-1buf", "diag6x1-2buf"} <= paths
    assert {"quad12-live9-trim", "quad12-live10-trim", "quad12-live0-full", "quad12-live11-full", "quad12-live12-full",
            "quad16-live13-trim", "quad16-live14-trim", "quad16-live15-full", "quad16-live16-full"} <= paths
    # the transposed rectangle is add_rect(p, b.r0, a.r0, 4, 8): I below J
    assert (False, 128, 0, 4, 8) in es.gram_plan(192, False) and (False, 256, 128, 4, 8) in es.gram_plan(320, False)
    assert [it for it in es.gram_plan(256, False) if not it[0]] == [(False, 0, 128, 4, 8), (False, 64, 128, 4, 8)]
    assert len(es.gram_plan(384, False)) == 9 and [es.padded_K(k) for k in (1, 16, 17, 128, 129, 192, 193, 257, 384)] == [16, 16, 32, 128, 192, 192, 256, 320, 384]


@pytest.mark.parametrize("spec", es.gram_tile_cases(), ids=es.gram_tile_id)
def test_gram_tile_case(spec):
    K, N, opts, path, tiles, form = spec
    assert es.gram_path(K, form, **opts) == path
    if tiles.startswith("waves"):
        assert "".join(str(t) for t in es.stream_tiles(N, "wave", grid_blocks=1)) == tiles[5:]
    else:
        assert es.stream_tiles(N, "workgroup", grid_blocks=1) == [int(tiles[6:])]
    case = es.build(K, N, form)
    check_forms(case)
    gram_reference_conditions(case)


def test_gram_tile_table_covers_the_loop_states():
    waves = {t for *_, t, _ in es.gram_tile_cases() if t.startswith("waves")}
    assert {"waves1000", "waves1100", "waves1111", "waves2111", "waves2222", "waves3222", "waves4333", "waves5555", "waves6555"} == waves
    assert sorted({int(t[6:]) for *_, t, _ in es.gram_tile_cases() if t.startswith("stream")}) == [1, 2, 3, 4, 5, 7, 8]
    ragged = {N % 16 != 0 for N in es.QUAD_TILES}
    parity = {(es.QUAD_TILES[N] % 2, N % 16 != 0) for N in es.QUAD_TILES}
    assert ragged == {True, False} and {(0, True), (1, True)} <= parity  # a ragged last tile on either buffer


@pytest.mark.parametrize("spec", es.ext_cases(), ids=es.ext_case_id)
def test_extension_case(spec):
    Kb, R, N, grid, paths, form = spec
    plan = es.ext_plan(Kb, R)
    assert plan is not None and plan["split_rows"] == es.padded_K(Kb) and plan["rows"] == plan["split_rows"] + plan["Kp_ext"]
    assert 128 < plan["need"] <= plan["rows"] and plan["Kp_ext"] >= R
    assert es.ext_path(Kb, R, gram_base=False) == paths["joint"]
    if "thin" in paths:
        assert es.ext_path(Kb, R, gram_base=True) == paths["thin"]
    else:
        assert es.ext_path(Kb, R, gram_base=True) == paths["joint"]  # (a base's W^T W would not change the path)
    case = es.build_ext(Kb, R, N, form)
    check_forms(case)
    rows = case["rows"]
    assert rows.shape == (R, N) and not np.any(np.isnan(rows)) and not np.any(rows == -np.inf)
    zero = [] if form != "inf" else [case["allinf"], Kb + case["ext_allinf"]]
    le = es.lognum_ext(case["u"], rows, case["N_k"], case["f"], case["c"])
    check_lognum(le, [] if form != "inf" else [case["ext_allinf"]])
    G, ws = es.gram_w_ext(case["u"], rows, case["N_k"], case["f"], case["f_ext"], case["c"])
    check_gram(G, ws, zero)


def test_extension_table_and_refusals():
    for Kb, R, rows, split, live, trimmed in es.JOINT_CASES:
        p = es.ext_plan(Kb, R)
        assert (p["rows"], p["split_rows"], p["live"], p["trimmed"], p["thin"]) == (rows, split, live, trimmed, False), (Kb, R, p)
    assert {p["split_rows"] for p in (es.ext_plan(Kb, R) for Kb, R, *_ in es.JOINT_CASES)} == {16, 32, 48, 64, 112, 128}
    for Kb, R in es.THIN_CASES:
        assert es.ext_plan(Kb, R, gram_base=True)["thin"] and not es.ext_plan(Kb, R)["thin"]
    assert not es.ext_plan(128, 17, gram_base=True)["thin"] and es.ext_plan(112, 16, gram_base=True) is None
    for Kb, R in es.EXT_REFUSALS:
        assert es.ext_plan(Kb, R) is None, (Kb, R)
    tiles = [es.stream_tiles(N, "workgroup", grid_blocks=1)[0] for N in es.EXT_TILE_NS]
    assert tiles == [1, 1, 2, 3, 5, 7]
    assert ["".join(map(str, es.stream_tiles(N, "wave", grid_blocks=1))) for N in es.EXT_TILE_NS] == ["1000", "1000", "1100", "1110", "2111", "2221"]
