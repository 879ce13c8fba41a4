"""Cases, oracle, bound and branch model of the binned passes by bin label (``mbar_ctx_set_bins`` / ``mbar_bin_lognum`` /
``mbar_bin_gram_w``; mbar_k_hist.hip, mbar_hist.cpp) -- TEST INFRASTRUCTURE ONLY, shared by tests/test_gpu_fes_histogram.py (device),
tests/test_fes_histogram_host.py (the model's own checks, on the CPU) and tools/hist_acf_branch_matrix.py.

Error bound of a binned sum (``bin_bound``).  Every term is positive, so a bin's sum of ``n_i`` terms carries at most
``(n_i - 1) u`` relative (``u = 2^-53``; each term passes through at most ``n_i - 1`` additions however the chunks group them; the
compensated merges add less) plus the largest relative error of a term.  A term is a product of ``E`` device exponentials (``E = 1``
for lognum and wsum, 2 for cross and diag); each carries the pinned ``3.1 u`` of ``exp2s_fast``
(tests/test_device_math_tables.py, profiles/device_math_accuracy.txt) plus ``2^-52 max|argument|`` for its rounded argument,
the products and the multiplicity add one ``u`` per multiplication (``E + 1`` of them at most).  ``lognum = max + log(sum)`` gets the
same figure as an absolute error.  The oracle works on the device's own downloaded ``u``, ``logden(f)`` and ``v``, so only the binned
passes are under test.  An exponential whose argument is ``-inf`` (``u`` or ``v`` = ``+inf``) is an exact zero: it carries no
error, and its argument does not enter the bound.

Branch model.  ``chunk_table`` restates the host's chunk table (chunks close at every multiple of 2048 samples and before a 65th
distinct bin of the sweep's tile; slots number a chunk's bins in order of first appearance), ``step_census`` the per-step loop of
``k_hist_vec`` / ``k_hist_cross``: a wave walks its chunk in steps of 64 samples from the chunk start; per step, over the samples
with ``c_n > 0``, up to ``HIST_ROUNDS`` butterflies take one distinct slot each (the lowest remaining lane's first) and what is
left is handed over sample by sample."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
E_EXP = 3.1  # (u) pinned relative error of the device exp

HIST_SLOTS, HIST_CHUNK_SAMPLES, HIST_ROUNDS, HIST_ROWS, NO_SLOT = 64, 2048, 8, 16, 255


def potentials(rng, K, N):
    """u, N_k, f, v as in ``awkward_case``: harmonic wells along a line plus noise, counts as even as N allows."""
    x = rng.normal(0.0, 1.0, N)
    centers = np.linspace(-2.0, 2.0, K)
    u = 0.5 * (x[None, :] - centers[:, None]) ** 2 * 4.0 + rng.normal(0.0, 0.05, (K, N))
    N_k = np.full(K, N // K)
    N_k[: N - N_k.sum()] += 1
    f = rng.normal(0.0, 0.5, K)
    v = rng.uniform(0.0, 5.0, N)
    return u, N_k, f, v


def multiplicities(rng, N):
    """0 .. 3 with 30 % zeros"""
    c = rng.integers(1, 4, N).astype(np.float64)
    c[rng.random(N) < 0.30] = 0.0
    return c


def awkward_case(seed=3):
    """K = 130 (two row blocks past 128, nine groups of 16 rows), N = 3001 (no multiple of 64), 300 bins with random labels so
    that chunks close on the 64-bin cap, 5 % of the labels -1, multiplicities 0 .. 3 with 30 % zeros, bin 298 with a single
    sample, bin 299 with three samples that all have multiplicity 0."""
    rng = np.random.default_rng(seed)
    K, N, nbins = 130, 3001, 300
    u, N_k, f, v = potentials(rng, K, N)
    labels = rng.integers(0, 298, N)
    labels[rng.random(N) < 0.05] = -1
    c = multiplicities(rng, N)
    labels[1234], c[1234] = 298, 2.0
    labels[[17, 1500, 2999]], c[[17, 1500, 2999]] = 299, 0.0
    return dict(K=K, N=N, nbins=nbins, u=u, N_k=N_k, f=f, v=v, labels=labels, c=c)


# ---- label patterns and the case set ---------------------------------------------------------------------------------------------
# (pattern, nbins); "sorted" has 128 bins so that a chunk of 2048 sorted samples stays below 64 of them
PATTERNS = (("sorted", 128), ("eight", 300), ("nine", 300), ("distinct", 300), ("distinct", 64), ("late65", 65), ("gaps", 300))
CHUNKS_AT_4500 = (3, 9, 11, 71, 3, 4)  # the first six patterns, single sweep
ALL_N = (1, 63, 64, 65, 2047, 2048, 2049, 4500)
ALL_K = (1, 15, 16, 17, 33)
WEIGHTINGS = ("none", "ones", "mult")


def pattern_labels(pattern, N, nbins, seed=0):
    n = np.arange(N)
    if pattern == "sorted":
        return n * nbins // N
    if pattern == "eight":
        return (n // 64 * 8 + n % 8) % nbins
    if pattern in ("nine", "gaps"):
        lab = (n // 64 * 9 + n % 9) % nbins
        if pattern == "gaps":
            rng = np.random.default_rng(100 + seed)
            lab[rng.random(N) < 0.05] = -1
            lab[2048:4096] = -1  # a chunk without bins
            lab[128:192] = -1  # one whole step inside a chunk
        return lab
    if pattern == "distinct":
        return n % nbins
    if pattern == "late65":
        lab = n % 64
        if N > 2047:
            lab[2047] = 64  # the 65th bin of [0, 2048) at its last sample: a one-sample chunk
        return lab
    if pattern == "random":
        rng = np.random.default_rng(100 + seed)
        lab = rng.integers(0, nbins, N)
        lab[rng.random(N) < 0.05] = -1
        return lab
    raise ValueError(pattern)


def make_case(pattern, nbins, N, K, seed=7):
    rng = np.random.default_rng([seed, N, K])
    u, N_k, f, v = potentials(rng, K, N)
    labels = pattern_labels(pattern, N, nbins, seed)
    c = multiplicities(rng, N)
    # one bin (the last one drawn) with only zero-multiplicity samples, where another bin is left
    drawn = np.unique(labels[labels >= 0])
    if drawn.size > 1:
        c[labels == drawn[-1]] = 0.0
    return dict(name=f"{pattern}{nbins}-N{N}-K{K}", K=K, N=N, nbins=nbins, u=u, N_k=N_k, f=f, v=v, labels=labels, c=c)


def case_keys():
    """(pattern, nbins, N, K): every pattern at N = 4500 with K = 17, every N with distinct (300 bins) and nine at K = 16,
    every K with nine at N = 2049."""
    keys = [(p, nb, 4500, 17) for p, nb in PATTERNS]
    keys += [(p, 300, N, 16) for p in ("distinct", "nine") for N in ALL_N]
    keys += [("nine", 300, 2049, K) for K in ALL_K if K != 16]
    return keys


def weights_of(case, weighting):
    """the multiplicities handed to ``set_sample_weights`` (None: the unweighted path) and their values"""
    if weighting == "none":
        return None, np.ones(case["N"])
    if weighting == "ones":
        return np.ones(case["N"]), np.ones(case["N"])
    return case["c"], case["c"]


# ---- the model of the chunk table and of the step loop ---------------------------------------------------------------------------
def tiles_of(nbins, sweeps):
    return [(t * nbins // sweeps, (t + 1) * nbins // sweeps) for t in range(sweeps)]


def chunk_table(labels, b0, b1):
    """([(n0, n1, nb), ...], slot[n]) of the bins [b0, b1)"""
    labels = np.asarray(labels)
    N = len(labels)
    slot = np.full(N, NO_SLOT, dtype=np.int64)
    chunks, seen, start, fence = [], {}, 0, HIST_CHUNK_SAMPLES
    inside = np.flatnonzero((labels >= b0) & (labels < b1))  # (the other samples open and close nothing)
    for n, b in zip(inside.tolist(), labels[inside].tolist()):
        while n >= fence:
            chunks.append((start, fence, len(seen)))
            seen, start, fence = {}, fence, fence + HIST_CHUNK_SAMPLES
        if b not in seen:
            if len(seen) == HIST_SLOTS:
                chunks.append((start, n, len(seen)))
                seen, start = {}, n
            seen[b] = len(seen)
        slot[n] = seen[b]
    while fence < N:
        chunks.append((start, fence, len(seen)))
        seen, start, fence = {}, fence, fence + HIST_CHUNK_SAMPLES
    if N > 0:
        chunks.append((start, N, len(seen)))
    return chunks, slot


def model_chunks(labels, nbins, sweeps):
    """what ``bins_info()["chunks"]`` reports: the chunks of every tile"""
    return sum(len(chunk_table(labels, b0, b1)[0]) for b0, b1 in tiles_of(nbins, sweeps))


def step_census(labels, c, nbins, sweeps=1):
    """Per step of every chunk with bins, of every tile: (distinct slots, samples handed over) over the samples with c_n > 0,
    plus the chunk lengths, the bins per chunk and the highest slot and lane a live sample uses."""
    out = dict(steps=[], chunk_len=[], chunk_nb=[], max_slot=-1, max_lane=-1)
    for b0, b1 in tiles_of(nbins, sweeps):
        chunks, slot = chunk_table(labels, b0, b1)
        for n0, n1, nb in chunks:
            out["chunk_len"].append(n1 - n0)
            out["chunk_nb"].append(nb)
            if nb == 0:
                continue  # (the wave returns)
            for base in range(n0, n1, 64):
                end = min(base + 64, n1)
                live = [(lane, int(slot[base + lane])) for lane in range(end - base)
                        if slot[base + lane] != NO_SLOT and c[base + lane] > 0]
                distinct = len({s for _, s in live})
                left = live
                for _ in range(HIST_ROUNDS):
                    if not left:
                        break
                    left = [(lane, s) for lane, s in left if s != left[0][1]]
                out["steps"].append((distinct, len(left)))
                if live:
                    out["max_slot"] = max(out["max_slot"], max(s for _, s in live))
                    out["max_lane"] = max(out["max_lane"], live[-1][0])
    return out


def census_line(cs):
    d = sorted({s[0] for s in cs["steps"]})
    h = sorted({s[1] for s in cs["steps"]})
    return (f"chunks {len(cs['chunk_len']):3d} (len {min(cs['chunk_len'])}..{max(cs['chunk_len'])}, empty {sum(nb == 0 for nb in cs['chunk_nb'])})"
            f" slots/step {d[0]}..{d[-1]} handed {h[0]}..{h[-1]} max slot {cs['max_slot']} lane {cs['max_lane']}")


# ---- oracle and bound --------------------------------------------------------------------------------------------------------------
def oracle(u, logden, v, f, labels, c, nbins, f_bins=None):
    """Long-double lognum, cross, diag, wsum with f_bins = -lognum (or the given one), their bounds, from the device's own u /
    logden.  A sample counts when c_n > 0 and v_n < +inf; one pass over the samples sorted by label."""
    K = u.shape[0]
    x = -(v.astype(LD) + logden.astype(LD))
    fl = f.astype(LD)
    absf = float(np.abs(f).max())
    lognum = np.full(nbins, -np.inf, dtype=LD)
    cross, diag, wsum = np.zeros((K, nbins), dtype=LD), np.zeros(nbins, dtype=LD), np.zeros(nbins, dtype=LD)
    n_i, arg = np.zeros(nbins), np.zeros(nbins)
    keep = np.flatnonzero((labels >= 0) & (c > 0) & (x > -np.inf))
    keep = keep[np.argsort(labels[keep], kind="stable")]
    edges = np.searchsorted(labels[keep], np.arange(nbins + 1))
    for i in range(nbins):
        m = keep[edges[i]:edges[i + 1]]
        n_i[i] = m.size
        if not m.size:
            continue
        xm, cm = x[m], c[m].astype(LD)
        mx = xm.max()
        lognum[i] = mx + np.log(np.sum(cm * np.exp(xm - mx)))
        b = xm - (lognum[i] if f_bins is None else -LD(f_bins[i]))  # log B_n at f_bins = -lognum
        B = np.exp(b)
        wsum[i], diag[i] = np.sum(cm * B), np.sum(cm * B * B)
        um = u[:, m]
        logW = fl[:, None] - um.astype(LD) - logden[m].astype(LD)[None, :]
        cross[:, i] = np.exp(logW) @ (cm * B)
        fin = np.isfinite(um)
        arg[i] = float(max(np.abs(xm).max(), np.abs(xm - mx).max(), np.abs(b).max(), np.abs(logW[fin]).max(initial=0.0),
                           absf + np.abs(um[fin]).max(initial=0.0)))
    return dict(lognum=lognum, cross=cross, diag=diag, wsum=wsum, n_i=n_i, arg=arg)


def bin_bound(o, n_exp):
    """Relative bound of a bin's sum whose terms hold n_exp exponentials (module docstring)."""
    return (np.maximum(o["n_i"] - 1, 0) + n_exp * (E_EXP + 2.0 * o["arg"]) + (n_exp + 1)) * U


def error_ratios(r, o):
    """worst error / bound of lognum, wsum, diag, cross over the bins with a drawn sample (the bound of ``bin_bound``, no factor)"""
    live = o["n_i"] > 0
    out = {}
    if not live.any():
        return dict(lognum=0.0, wsum=0.0, diag=0.0, cross=0.0)
    out["lognum"] = float(np.max(np.abs(r["lognum"][live].astype(LD) - o["lognum"][live]) / bin_bound(o, 1)[live]))
    for name, n_exp in (("wsum", 1), ("diag", 2)):
        out[name] = float(np.max(np.abs(r[name].astype(LD) - o[name])[live] / (bin_bound(o, n_exp) * np.abs(o[name]))[live]))
    err = np.abs(r["cross"].astype(LD) - o["cross"])[:, live]
    ref = (bin_bound(o, 2)[None, :] * np.abs(o["cross"]))[:, live]
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(err == 0, 0.0, err / ref)  # (a cross entry that is an exact zero: u = +inf on every sample of the bin)
    out["cross"] = float(np.max(q))
    return out


def assert_within(r, o, factor=1.0, label=""):
    """Every bin with a drawn sample within ``factor * bin_bound`` of the oracle; -inf and exact zeros for the others."""
    live = o["n_i"] > 0
    for name in ("lognum", "cross", "diag", "wsum"):
        assert not np.any(np.isnan(r[name])), (label, name)
    print(label, "worst error / bound:", {k: round(q, 4) for k, q in error_ratios(r, o).items()})
    err = np.abs(r["lognum"][live].astype(LD) - o["lognum"][live])
    assert np.all(err <= factor * bin_bound(o, 1)[live]), label
    assert np.all(np.isneginf(r["lognum"][~live])), label
    for name, n_exp in (("wsum", 1), ("diag", 2)):
        err = np.abs(r[name].astype(LD) - o[name])
        assert np.all(err <= factor * bin_bound(o, n_exp) * np.abs(o[name])), (label, name)
        assert np.all(r[name][~live] == 0), (label, name)
    err = np.abs(r["cross"].astype(LD) - o["cross"])
    assert np.all(err <= factor * bin_bound(o, 2)[None, :] * np.abs(o["cross"])), label
    assert np.all(r["cross"][:, ~live] == 0), label


# ---- running the passes ------------------------------------------------------------------------------------------------------------
def passes_on(dm, case, weights, f_bins=None):
    """set_sample_weights, set_bins, pass A, pass B (f_bins = -lognum unless given) on a device matrix or its CPU stand-in"""
    dm.set_sample_weights(weights)
    dm.set_bins(case["nbins"], case["labels"], case["v"])
    info = dm.bins_info()
    lognum = dm.bin_lognum(case["f"])
    fb = -lognum if f_bins is None else f_bins
    X, d, w = dm.bin_gram_w(case["f"], fb)
    return dict(lognum=lognum, cross=X, diag=d, wsum=w, info=info, f_bins=fb)


def run_weighting(dm, case, weighting):
    """One weighting of a case on an open device matrix, with the oracle on the device's own u and logden."""
    weights, c = weights_of(case, weighting)
    r = passes_on(dm, case, weights)
    _, r["diag_only"], r["wsum_only"] = dm.bin_gram_w(case["f"], r["f_bins"], cross=False)
    r["logden"] = dm.logden(case["f"])  # (under the same weights as the passes)
    r["oracle"] = oracle(dm.to_host(), r["logden"], case["v"], case["f"], case["labels"], c, case["nbins"])
    return r


def open_matrix(case, part_bytes=None):
    from pymbar_amd.device import DeviceMatrix

    dm = DeviceMatrix.from_host(case["u"])
    dm.set_Nk(case["N_k"])
    if part_bytes is not None:
        dm.set_option("hist_part_bytes", part_bytes)
    return dm


def part_bytes_for(case, sweeps):
    """a ``hist_part_bytes`` under which ``set_bins`` settles on ``sweeps`` sweeps (it doubles the tile count, capped at nbins,
    until the largest tile's records fit): the record bytes of the wanted tiling"""
    def worst(T):
        return max(sum(nb for _, _, nb in chunk_table(case["labels"], b0, b1)[0]) for b0, b1 in tiles_of(case["nbins"], T))

    if sweeps == case["nbins"]:
        return 1  # (no tiling fits: the doubling ends at one bin per sweep)
    T = 1
    while T < sweeps:
        assert worst(T) > worst(sweeps), "the wanted tiling needs no fewer record bytes than a coarser one"
        T *= 2
    assert T == sweeps, "set_bins reaches only powers of two and nbins"
    return worst(sweeps) * (case["K"] + 2) * 8


def run_passes(case, part_bytes=None, perm=None):
    from pymbar_amd.device import DeviceMatrix

    p = slice(None) if perm is None else perm
    with DeviceMatrix.from_host(case["u"][:, p]) as dm:
        dm.set_Nk(case["N_k"])
        if part_bytes is not None:
            dm.set_option("hist_part_bytes", part_bytes)
        labels, v, c = case["labels"][p], case["v"][p], case["c"][p]
        dm.set_sample_weights(c)
        dm.set_bins(case["nbins"], labels, v)
        info = dm.bins_info()
        lognum = dm.bin_lognum(case["f"])
        X, d, w = dm.bin_gram_w(case["f"], -lognum)
        again = (dm.bin_lognum(case["f"]), dm.bin_gram_w(case["f"], -lognum))
        dm.set_bins(case["nbins"], labels, v)
        third = (dm.bin_lognum(case["f"]), dm.bin_gram_w(case["f"], -lognum))
        dm.set_sample_weights(None)
        logden, u_dev = dm.logden(case["f"]), dm.to_host()
    return dict(lognum=lognum, cross=X, diag=d, wsum=w, info=info, again=again, third=third, logden=logden, u=u_dev, labels=labels, v=v, c=c)
