"""CPU stand-in for the primitives of the expectation family -- TEST INFRASTRUCTURE ONLY: ``mbar_lognum``, ``mbar_logw`` / ``mbar_w``,
``mbar_gram_w`` and their extension forms ``mbar_lognum_ext`` / ``mbar_gram_w_ext`` in plain numpy long double, in column blocks of
at most ~2e6 matrix entries.  A ``+inf`` entry is weight zero; a state whose row is all ``+inf`` has ``lognum = -inf`` and exact zeros
in ``W^T W``.  Shards are combined in long double (``combine_parts``).

Also: what the library's host code will choose for a shape, re-derived in Python (``padded_K``, ``gram_plan``, ``gram_path``,
``stream_tiles``, ``lognum_plan``, ``ext_plan``, ``logw_plan``), the builder of the harmonic-ladder inputs in their three data forms
(plain, inf, weighted) and the case tables of tests/test_gpu_expect_primitives.py.  tests/test_expect_standin_host.py checks on the
CPU that every table entry suits the stand-in and reaches the path its id names.

K = 1 has no inf form: the one state drew every sample, so by the form's own definition (``+inf`` only where a state did not draw the
sample, the all-``+inf`` row on an unsampled state) there is nothing to set; the tables hold K = 1 as plain (and weighted) only."""
import functools

import numpy as np

from pymbar_amd import testsystems as ts

R = np.longdouble
BLOCK_ENTRIES = 2_000_000
FORMS = ("plain", "inf", "weighted")


def _col_blocks(K, N):
    step = max(1, BLOCK_ENTRIES // max(int(K), 1))
    for n0 in range(0, N, step):
        yield slice(n0, min(N, n0 + step))


# ---- the stand-in ---------------------------------------------------------------------------------------------------------------------
def logden(u, N_k, f):
    """``log sum_k N_k exp(f_k - u_kn)`` per sample, long double (N,)"""
    u = np.asarray(u)
    N_k = np.asarray(N_k, dtype=np.float64)
    sampled = N_k > 0
    a = (np.asarray(f, dtype=R)[sampled] + np.log(N_k[sampled].astype(R)))[:, None]
    us = u[sampled]
    out = np.empty(u.shape[1], dtype=R)
    with np.errstate(invalid="ignore", divide="ignore"):
        for sl in _col_blocks(len(a), u.shape[1]):
            x = a - us[:, sl].astype(R)
            m = x.max(axis=0)
            ms = np.where(np.isfinite(m), m, R(0))
            out[sl] = np.where(np.isfinite(m), ms + np.log(np.exp(x - ms).sum(axis=0)), m)
    return out


def _log_c(c_n, N):
    if c_n is None:
        return None
    with np.errstate(divide="ignore"):
        return np.log(np.asarray(c_n, dtype=R).reshape(N))


def lognum_parts(u, ld, c_n=None):
    """``(m_k, s_k)`` with ``sum_n c_n exp(-u_kn - ld_n) = s_k exp(m_k)`` for the columns given, long double"""
    u = np.asarray(u)
    K, N = u.shape
    lc = _log_c(c_n, N)
    parts = []
    with np.errstate(invalid="ignore"):
        for sl in _col_blocks(K, N):
            x = -u[:, sl].astype(R) - ld[sl][None, :]
            if lc is not None:
                x = x + lc[sl][None, :]
            m = x.max(axis=1) if x.shape[1] else np.full(K, -np.inf, dtype=R)
            ms = np.where(np.isfinite(m), m, R(0))
            parts.append((m, np.exp(x - ms[:, None]).sum(axis=1)))
    return combine_parts(parts, log=False) if parts else (np.full(K, -np.inf, dtype=R), np.zeros(K, dtype=R))


def combine_parts(parts, log=True):
    """The (max, sum) records of blocks or shards folded in long double; ``log``: the log of the total, ``-inf`` where nothing is left"""
    ms = np.stack([p[0] for p in parts])
    ss = np.stack([p[1] for p in parts])
    m = ms.max(axis=0)
    msafe = np.where(np.isfinite(m), m, R(0))
    with np.errstate(invalid="ignore", divide="ignore"):
        s = np.where(np.isfinite(ms), ss * np.exp(ms - msafe[None, :]), R(0)).sum(axis=0)
        if not log:
            return m, s
        return np.where(s > 0, msafe + np.log(s), -np.inf).astype(R)


def lognum(u, N_k, f, c_n=None, ld=None):
    """``log sum_n c_n exp(-u_kn - logden_n)`` for every row, long double (K,)"""
    ld = logden(u, N_k, f) if ld is None else ld
    return combine_parts([lognum_parts(u, ld, c_n)])


def logw(u, N_k, f, ld=None):
    """``f_k - u_kn - logden_n``, long double (K, N)"""
    u = np.asarray(u)
    ld = logden(u, N_k, f) if ld is None else ld
    out = np.empty(u.shape, dtype=R)
    fk = np.asarray(f, dtype=R)[:, None]
    for sl in _col_blocks(*u.shape):
        out[:, sl] = fk - u[:, sl].astype(R) - ld[sl][None, :]
    return out


def w(u, N_k, f, ld=None):
    return np.exp(logw(u, N_k, f, ld))


def gram_w(u, N_k, f, c_n=None):
    """``(sum_n c_n W_ni W_nj, sum_n c_n W_nj)``, long double"""
    u = np.asarray(u)
    K, N = u.shape
    ld = logden(u, N_k, f)
    fk = np.asarray(f, dtype=R)[:, None]
    c = None if c_n is None else np.asarray(c_n, dtype=R)
    G, ws = np.zeros((K, K), dtype=R), np.zeros(K, dtype=R)
    for sl in _col_blocks(K, N):
        W = np.exp(fk - u[:, sl].astype(R) - ld[sl][None, :])
        Wc = W if c is None else W * c[sl][None, :]
        G += Wc @ W.T
        ws += Wc.sum(axis=1)
    return (G + G.T) / 2, ws  # (c W_i W_j and c W_j W_i round apart in the last long-double bit)


def stacked(u, rows, N_k, f, f_ext):
    """``[resident rows | appended rows]`` as one problem: N_k = 0 on the appended rows"""
    rows = np.atleast_2d(rows)
    return np.vstack([u, rows]), np.concatenate([np.asarray(N_k, dtype=np.float64), np.zeros(len(rows))]), np.concatenate([f, f_ext])


def lognum_ext(u, rows, N_k, f, c_n=None):
    """lognum of the appended rows with the base's log-denominators"""
    return lognum(np.atleast_2d(rows), None, None, c_n, ld=logden(u, N_k, f))


def gram_w_ext(u, rows, N_k, f, f_ext, c_n=None):
    return gram_w(*stacked(u, rows, N_k, f, f_ext), c_n=c_n)


# ---- what the library's host code chooses -------------------------------------------------------------------------------------------
TS, LN_TILE, LN_ROWS = 16, 64, 8


def padded_K(K):
    return (K + 15) // 16 * 16 if K <= 128 else (K + 63) // 64 * 64


def row_pitch(K, N):
    """mbar_ctx_create: whole 16-sample tiles, whole 64-sample tiles up to 32 padded states"""
    unit = 64 if padded_K(K) <= 32 else TS
    return max(unit, (N + unit - 1) // unit * unit)


def gram_plan(Kp, quad):
    """The items of gram_plan (mbar_eval.cpp): ``(diag, ri, rj, nbi, nbj)`` in launch order"""
    width = Kp if (Kp <= 128 or quad) else 128
    panels, r = [], 0
    while r < Kp:
        nb = width // 16 if Kp - r >= width else (Kp - r) // 16
        panels.append((r, nb))
        r += 16 * nb
    items = [(True, r0, r0, nb, nb) for r0, nb in panels]
    for ia, (ra, _) in enumerate(panels):
        for rb, nbb in panels[ia + 1:]:
            if nbb == 8:
                items += [(False, ra + 64 * h, rb, 4, 8) for h in range(2)]
            else:
                assert nbb == 4
                items.append((False, rb, ra, 4, 8))
    return items


def gram_path(K, form="plain", gram_quad=1, quad_trim=1):
    """Name of the launches mbar_gram_w makes for K states, e.g. ``diag8x1-2buf-unclamped``, ``quad12-live9-trim``,
    ``diag8x1+diag4x1+rectT4x8x1`` (rectT: the I panel lies below the J panel, the transposed rectangle)"""
    Kp = padded_K(K)
    quad = bool(gram_quad) and 128 < Kp <= 256
    items = gram_plan(Kp, quad)
    if quad:
        assert len(items) == 1
        nbt = items[0][3]
        live = (K + 15) // 16 if quad_trim else 0
        return "quad%d-live%d-%s" % (nbt, live, "trim" if 0 < live <= nbt - 2 else "full")
    if len(items) == 1:
        nb = items[0][3]
        name = "diag%dx1-%dbuf" % (nb, 1 if nb * 16 <= 80 else 2)
        return name + (("-clamped" if form == "inf" else "-unclamped") if nb == 8 else "")
    count = {}
    for diag, ri, rj, nbi, nbj in items:
        key = "diag%d" % nbi if diag else ("rectT" if ri > rj else "rect") + "%dx%d" % (nbi, nbj)
        count[key] = count.get(key, 0) + 1
    return "+".join("%sx%d" % kv for kv in count.items())


def stream_tiles(N, kind, grid_blocks=0, num_cu=256):
    """Tiles of 16 samples per tile stream.  ``wave``: k_gram (diagonal panels up to 128 rows, rectangles), one stream per wave, four
    waves per workgroup, a workgroup for every four tiles; ``workgroup``: the one-read kernels, four waves on one shared stream, a
    workgroup per tile.  Both up to ``grid_blocks`` workgroups (0: one per CU; narrow diagonal panels may get more, which for the
    table's N changes nothing: a workgroup for every four tiles is fewer)."""
    ntiles = (N + TS - 1) // TS
    cap = grid_blocks if grid_blocks > 0 else num_cu
    if kind == "wave":
        streams = 4 * min(max(1, (ntiles + 3) // 4), cap)
    else:
        streams = min(max(1, ntiles), cap)
    return [len(range(s, ntiles, streams)) for s in range(streams)]


def lognum_plan(K, N):
    """``(tiles of 64 samples, tiles per chunk, chunks, [(pair trips, single full tiles, ragged tiles)] of the first and last chunk)``"""
    ntiles = (N + LN_TILE - 1) // LN_TILE
    nsb = (K + LN_ROWS - 1) // LN_ROWS
    tpc = max(1, (ntiles + max(1, 16384 // nsb) - 1) // max(1, 16384 // nsb))
    chunks = max(1, (ntiles + tpc - 1) // tpc)

    def trips(c):
        t0, t1 = c * tpc, min(ntiles, (c + 1) * tpc)
        tfull = t1 if t1 * LN_TILE <= N else t1 - 1
        full = max(0, tfull - t0)
        return (full // 2, full % 2, t1 - max(tfull, t0))

    return ntiles, tpc, chunks, [trips(0), trips(chunks - 1)]


def ext_plan(Kb, R, gram_base=False, quad_trim=1):
    """mbar_ctx_create_ext and mbar_gram_w_ext: ``None`` where the library refuses, else a dict (need, Kp_ext, rows, split_rows, live,
    trimmed, thin)"""
    Kpb = padded_K(Kb)
    need = Kpb + (R + 15) // 16 * 16
    if R < 1 or Kpb > 128 or need <= 128 or need > 256:
        return None
    rows = 192 if need <= 192 else 256
    live = (Kpb + R + 15) // 16 if quad_trim else 0
    thin = bool(gram_base) and R <= 16 and Kpb == 128
    return dict(need=need, Kp_ext=rows - Kpb, rows=rows, split_rows=Kpb, live=live, trimmed=0 < live <= rows // 16 - 2, thin=thin)


def ext_path(Kb, R, gram_base=False, quad_trim=1):
    p = ext_plan(Kb, R, gram_base, quad_trim)
    if p is None:
        return "refused"
    if p["thin"]:
        return "thin1x8+diag1"
    return "split%d-at%d-live%d-%s" % (p["rows"] // 16, p["split_rows"], p["live"], "trim" if p["trimmed"] else "full")


def logw_plan(K, N):
    """logw_impl and launch_logw: ``(row pitch, rows per staging block, staging blocks, grid-stride trips of a row)``"""
    ld = row_pitch(K, N)
    rows_per = max(1, min(K, (256 << 20) // (ld * 8)))
    threads = 256 * min(2048, max(1, (N + 255) // 256))
    return ld, rows_per, (K + rows_per - 1) // rows_per, (N + threads - 1) // threads


# ---- the inputs ---------------------------------------------------------------------------------------------------------------------
def unsampled_states(K, form):
    """States without samples: two from K = 4 on (one from K = 2 in the inf form, for its all-+inf row), plus the two states on
    either side of every 128-state panel border.  Never state 0 (the gauge).  The first one carries the all-+inf row."""
    if K >= 4:
        out = [K // 3, 2 * K // 3]
    elif K >= 2 and form == "inf":
        out = [K - 1]
    else:
        out = []
    for border in (128, 256):
        if K > border:
            out += [k for k in (border - 1, border) if k not in out]
    return out


def _draw_counts(N_k, rng):
    c = np.zeros(int(N_k.sum()))
    start = 0
    for n_k in N_k:
        if n_k > 0:
            c[start:start + n_k] = np.bincount(rng.randint(0, n_k, size=n_k), minlength=n_k)
        start += n_k
    return c


def weights_ok(c):
    """The conditions on a weighted form (module docstring of the device test)"""
    N = len(c)
    if N >= 16:
        return np.mean(c == 0) >= 0.2 and c.max() >= 3
    if N >= 3:
        return np.any(c == 0) and c.max() >= 2
    return True  # (N = 1: the one sample is drawn once; N = 2 does not occur)


@functools.lru_cache(maxsize=8)
def build(K, N, form, unsampled=None):
    """A harmonic ladder of K states and N samples in one of the three data forms: ``dict(u, N_k, f, c, s_n, allinf)``; arrays read-only.
    The sampled states are at most N // 8 (so a state's bootstrap draw counts hold zeros) spread evenly over the ladder."""
    assert form in FORMS and not (K == 1 and form == "inf")
    seed = 100003 * K + N
    rng = np.random.RandomState(seed % (2**31))
    un = unsampled_states(K, form) if unsampled is None else list(unsampled)
    cand = [k for k in range(K) if k not in un]
    n_samp = min(len(cand), max(1, N // 8))
    sampled = [cand[i] for i in sorted(set(np.linspace(0, len(cand) - 1, n_samp).round().astype(int)))]
    N_k = np.zeros(K, dtype=np.int64)
    N_k[sampled] = 1 + rng.multinomial(N - len(sampled), np.ones(len(sampled)) / len(sampled))
    O_k, K_k = ts.ladder_params(K) if K > 1 else (np.zeros(1), np.ones(1))
    _, u, N_k, s_n = ts.harmonic_u_kn(O_k, K_k, N_k, seed=seed % (2**31))
    f = ts.harmonic_free_energies(K_k) + rng.uniform(-1.0, 1.0, size=K)
    f[0] = 0.0
    c, allinf = None, None
    if form == "inf":
        mask = rng.random_sample(u.shape) < 0.05
        mask[s_n, np.arange(N)] = False
        mask[mask.all(axis=1)] = False  # (few samples: no row but the one below is all +inf)
        u[mask] = np.inf
        allinf = un[0]
        u[allinf] = np.inf
    elif form == "weighted":
        for _ in range(400):
            c = _draw_counts(N_k, rng)
            if weights_ok(c):
                break
        else:
            raise AssertionError("no bootstrap replicate with the zeros and repeats asked for: K=%d N=%d" % (K, N))
    for a in (u, N_k, f, s_n) + (() if c is None else (c,)):
        a.setflags(write=False)
    return dict(u=u, N_k=N_k, f=f, c=c, s_n=s_n, allinf=allinf, K=K, N=N, form=form)


@functools.lru_cache(maxsize=8)
def build_ext(Kb, R, N, form):
    """``build(Kb, N, form)`` plus R appended rows -- rescaled and shifted copies of resident rows plus noise -- and their f; in the
    inf form appended row R // 2 is all +inf"""
    case = dict(build(Kb, N, form))
    rng = np.random.RandomState(7919 * Kb + 31 * R + N)
    pick = rng.choice([k for k in range(Kb) if k != case["allinf"]], size=R)
    rows = case["u"][pick] * rng.uniform(0.8, 1.3, size=(R, 1)) + rng.uniform(-0.5, 0.5, size=(R, 1)) + 0.05 * rng.standard_normal((R, N))
    if form == "inf":
        rows[R // 2] = np.inf
    f_ext = rng.uniform(-1.0, 1.0, size=R)
    rows.setflags(write=False)
    f_ext.setflags(write=False)
    case.update(rows=rows, f_ext=f_ext, R=R, ext_allinf=R // 2 if form == "inf" else None)
    return case


def forms_for(K, forms):
    return [fm for fm in forms if not (K == 1 and fm == "inf")]


# ---- table A: lognum ------------------------------------------------------------------------------------------------------------------
def lognum_seam_cases():
    """Row-group seams (8 rows per wave) x tile seams (64 samples per tile): ``(K, N, form)``"""
    return [(K, N, fm) for K in (1, 7, 8, 9, 17) for N in (1, 63, 64, 65, 129) for fm in forms_for(K, ("plain", "inf"))]


# (K, N, form, tiles, tiles per chunk, chunks, trips of the last chunk (pairs, single full tiles, ragged tiles))
LOGNUM_CHUNK_CASES = [
    (5, 16449, "plain", 258, 1, 258, (0, 0, 1)),
    (5, 16449, "weighted", 258, 1, 258, (0, 0, 1)),
    (1024, 12353, "plain", 194, 2, 97, (0, 1, 1)),
    (1024, 20001, "weighted", 313, 3, 105, (0, 0, 1)),
]


def lognum_case_id(spec):
    if len(spec) == 3:
        return "K%d-N%d-%s" % spec
    K, N, fm, tiles, tpc, chunks, last = spec
    return "K%d-N%d-%s-%dtiles-%dperchunk-%dchunks-last%d.%d.%d" % ((K, N, fm, tiles, tpc, chunks) + last)


MERGE_CASE = dict(K=9, N=1000, shards=((0, 300), (300, 723), (723, 1000)), inf_state=3, inf_shard=1, far_state=6, far_shard=2, far_by=800.0)


def build_merge_case():
    """Table A's multi-rank case: state ``inf_state`` is +inf on the whole of shard ``inf_shard`` (local maximum -inf); state
    ``far_state`` lies ``far_by`` higher on shard ``far_shard``, so that shard's sum is rescaled by exp(-far_by) = 0.  Both are
    unsampled states: the log-denominators do not move."""
    m = MERGE_CASE
    case = dict(build(m["K"], m["N"], "plain"))
    u = case["u"].copy()
    assert case["N_k"][m["inf_state"]] == 0 and case["N_k"][m["far_state"]] == 0
    n0, n1 = m["shards"][m["inf_shard"]]
    u[m["inf_state"], n0:n1] = np.inf
    n0, n1 = m["shards"][m["far_shard"]]
    u[m["far_state"], n0:n1] += m["far_by"]
    case["u"] = u
    return case


OFFSET_CASE = (8, 257)


def build_offset_case():
    """Table A's extreme offsets: 0, +1e4 or -1e4 added to all rows of a column"""
    case = dict(build(OFFSET_CASE[0], OFFSET_CASE[1], "plain"))
    off = np.random.RandomState(5).choice([0.0, 1.0e4, -1.0e4], size=case["N"])
    case["u"] = case["u"] + off[None, :]
    case["offsets"] = off
    return case


# ---- table B: log W and W -------------------------------------------------------------------------------------------------------------
def logw_cases():
    return [(K, N) for K in (1, 5, 130) for N in (1, 255, 257, 2049)]


LOGW_STRIDE_CASE = (2, 524288 + 257)   # two grid-stride trips
LOGW_LD_CASE = (5, 257, 3)             # ld_out = N + 3
LOGW_STAGE_CASE = (5, 2**23 + 1)       # rows_per = 3: two staging blocks
UNDERFLOW_CASE = (3, 64)
UNDERFLOW_TARGETS = (-692.0, -696.0, -700.0, -706.0, -710.0, -720.0, -730.0, -740.0, -746.0, -750.0, -800.0, -1000.0)


def build_underflow_case():
    """K = 3, N = 64: the unsampled state 2 is given log W = UNDERFLOW_TARGETS on its first samples -- four normal weights below
    1e-300, four subnormal ones and four that are exactly 0"""
    K, N = UNDERFLOW_CASE
    case = dict(build(K, N, "plain", unsampled=(2,)))
    assert case["N_k"][2] == 0
    u = case["u"].copy()
    ld = logden(u, case["N_k"], case["f"]).astype(np.float64)
    t = np.asarray(UNDERFLOW_TARGETS)
    u[2, :len(t)] = case["f"][2] - ld[:len(t)] - t
    case["u"] = u
    return case


# ---- table C: gram_w ------------------------------------------------------------------------------------------------------------------
# (K, options, the path of the plain form, forms)
GRAM_PLAN_CASES = (
    [(K, {}, p, FORMS) for K, p in ((1, "diag1x1-1buf"), (15, "diag1x1-1buf"), (16, "diag1x1-1buf"), (17, "diag2x1-1buf"), (33, "diag3x1-1buf"),
                                    (64, "diag4x1-1buf"), (65, "diag5x1-1buf"), (80, "diag5x1-1buf"), (81, "diag6x1-2buf"),
                                    (113, "diag8x1-2buf-unclamped"), (128, "diag8x1-2buf-unclamped"))]
    + [(129, {}, "quad12-live9-trim", FORMS), (160, {}, "quad12-live10-trim", FORMS), (160, {"quad_trim": 0}, "quad12-live0-full", FORMS),
       (161, {}, "quad12-live11-full", FORMS), (192, {}, "quad12-live12-full", FORMS), (193, {}, "quad16-live13-trim", FORMS),
       (224, {}, "quad16-live14-trim", FORMS), (225, {}, "quad16-live15-full", FORMS), (256, {}, "quad16-live16-full", FORMS),
       (129, {"gram_quad": 0}, "diag8x1+diag4x1+rectT4x8x1", FORMS), (256, {"gram_quad": 0}, "diag8x2+rect4x8x2", FORMS),
       (257, {}, "diag8x2+diag4x1+rect4x8x2+rectT4x8x2", ("plain", "weighted")), (384, {}, "diag8x3+rect4x8x6", ("plain", "weighted"))])
GRAM_PLAN_N = 1000


def gram_plan_cases():
    return [(K, opts, path.replace("unclamped", "clamped") if fm == "inf" else path, fm)
            for K, opts, path, forms in GRAM_PLAN_CASES for fm in forms_for(K, forms)]


def gram_plan_id(spec):
    K, opts, path, fm = spec
    return "K%d-%s%s-%s" % (K, "".join("%s%d-" % kv for kv in opts.items()), path, fm)


# tiles per wave of one workgroup (tests/test_gpu_fused_tile_loop.py has the table) and tiles on the shared stream of a one-read panel
WAVE_TILES = {1: "1000", 15: "1000", 16: "1000", 17: "1100", 63: "1111", 64: "1111", 65: "2111", 128: "2222", 129: "3222", 200: "4333",
              319: "5555", 321: "6555"}
QUAD_TILES = {1: 1, 16: 1, 17: 2, 33: 3, 49: 4, 65: 5, 97: 7, 113: 8}
RECT_NS = (17, 65, 129)


def gram_tile_cases():
    """``(K, N, options, path, tiles, form)`` with grid_blocks = 1"""
    out = []
    for fm in ("plain", "weighted"):
        for K, path in ((16, "diag1x1-1buf"), (80, "diag5x1-1buf"), (96, "diag6x1-2buf"), (128, "diag8x1-2buf-unclamped")):
            out += [(K, N, {}, path, "waves" + t, fm) for N, t in WAVE_TILES.items()]
        for K, path in ((160, "quad12-live10-trim"), (256, "quad16-live16-full")):
            out += [(K, N, {}, path, "stream%d" % t, fm) for N, t in QUAD_TILES.items()]
        out += [(129, N, {"gram_quad": 0}, "diag8x1+diag4x1+rectT4x8x1", "waves" + WAVE_TILES[N], fm) for N in RECT_NS]
    return out


def gram_tile_id(spec):
    K, N, opts, path, tiles, fm = spec
    return "K%d-N%d-%s%s-%s-%s" % (K, N, "".join("%s%d-" % kv for kv in opts.items()), path, tiles, fm)


# The all-+inf row placed inside a chosen block of 16 states of a one-read panel: (K, state, path).  W^T W must be EXACTLY 0 along
# it, which shows an accumulator that did not start from zero (block (2, 6) of the trimmed 192-row panel once did not)
GRAM_ZERO_ROW_CASES = [(150, 33, "quad12-live10-trim"), (150, 97, "quad12-live10-trim"), (180, 33, "quad12-live12-full"),
                       (180, 50, "quad12-live12-full"), (240, 33, "quad16-live15-full"), (200, 97, "quad16-live13-trim")]


def build_zero_row_case(K, state):
    return build(K, GRAM_PLAN_N, "inf", unsampled=(state,) + tuple(k for k in unsampled_states(K, "inf") if k != state))


# ---- table D: extensions -------------------------------------------------------------------------------------------------------------
THIN_CASES = [(113, 1), (128, 15), (128, 16)]
# (Kb, R, panel rows, split_rows, live blocks, trimmed)
JOINT_CASES = [(5, 130, 192, 16, 10, True), (5, 150, 192, 16, 11, False), (64, 65, 192, 64, 9, True), (100, 17, 192, 112, 9, True),
               (128, 17, 192, 128, 10, True), (128, 64, 192, 128, 12, False),
               (17, 200, 256, 32, 15, False), (40, 150, 256, 48, 13, True), (128, 65, 256, 128, 13, True), (128, 97, 256, 128, 15, False),
               (128, 128, 256, 128, 16, False)]
EXT_N = 1000
EXT_TILE_SHAPES = [(5, 130), (128, 17), (40, 150), (128, 128), (128, 15)]
EXT_TILE_NS = (1, 16, 17, 33, 65, 97)


def _joint_path(rows, split, live, trimmed):
    return "split%d-at%d-live%d-%s" % (rows // 16, split, live, "trim" if trimmed else "full")


def ext_cases():
    """``(Kb, R, N, grid_blocks, {"thin": path} | {"joint": path}, form)``: a thin case runs with and without gram_base"""
    joint = {(Kb, R): _joint_path(*rest) for Kb, R, *rest in JOINT_CASES}
    thin_joint = {(113, 1): "split12-at128-live9-trim", (128, 15): "split12-at128-live9-trim", (128, 16): "split12-at128-live9-trim"}
    out = []
    for fm in FORMS:
        out += [(Kb, R, EXT_N, 0, dict(thin="thin1x8+diag1", joint=thin_joint[(Kb, R)]), fm) for Kb, R in THIN_CASES]
        out += [(Kb, R, EXT_N, 0, dict(joint=joint[(Kb, R)]), fm) for Kb, R, *_ in JOINT_CASES]
        for Kb, R in EXT_TILE_SHAPES:
            paths = dict(thin="thin1x8+diag1", joint=thin_joint[(Kb, R)]) if (Kb, R) in THIN_CASES else dict(joint=joint[(Kb, R)])
            out += [(Kb, R, N, 1, paths, fm) for N in EXT_TILE_NS]
    return out


def ext_case_id(spec):
    Kb, R, N, grid, paths, fm = spec
    return "Kb%d-R%d-N%d-%s%s-%s" % (Kb, R, N, "grid1-" if grid else "", "+".join(paths[k] for k in sorted(paths, reverse=True)), fm)


# (Kb, R) the library must refuse: too few rows in all, too many, a base above 128 states
EXT_REFUSALS = [(5, 100), (5, 112), (100, 16), (128, 129), (17, 225), (129, 16), (200, 20)]
