// Host side of the histogram surfaces by bin label (include/mbar_hip.h, "histogram bins by label"): the chunk table of a label
// array (built once per mbar_ctx_set_bins, O(N)), the tiling of the bins under the record budget, and the two binned passes over
// the context's resident matrix.  Kernels: mbar_k_hist.hip.
#include "mbar_ctx.h"
#include "mbar_hist.h"

using namespace mbar;
using namespace mbar::host;

namespace {

struct HostTile {
    int64_t b0 = 0, b1 = 0;
    std::vector<int64_t> chunk_n, chunk_rec, bin_ptr, bin_rec;
    std::vector<uint8_t> slot;
    int64_t nrec() const { return (int64_t)bin_rec.size(); }
};

// Chunks of the samples for the bins [b0, b1): contiguous, closed at every multiple of HIST_CHUNK_SAMPLES and before a 65th distinct
// bin; slot[n] numbers a chunk's bins in order of first appearance; the records of a bin are listed in chunk order.  Blocks of
// HIST_CHUNK_SAMPLES samples are independent, so up to 8 host threads build runs of blocks: the table does not depend on their number.
struct TilePiece {
    std::vector<int64_t> chunk_end;  // end of each chunk of the piece
    std::vector<int32_t> chunk_nb;   // its number of distinct bins
    std::vector<int32_t> rec_bin;    // the bins of its records, chunk by chunk
};

void build_piece(const int32_t* label, int64_t n0, int64_t n1, int64_t nbins, int64_t b0, int64_t b1, uint8_t* slot, TilePiece& out) {
    std::vector<int64_t> stamp((size_t)nbins, -1);
    std::vector<uint8_t> slot_of((size_t)nbins, 0);
    int64_t chunk = 0;
    int used = 0;
    auto close = [&](int64_t n) {
        out.chunk_end.push_back(n);
        out.chunk_nb.push_back(used);
        ++chunk;
        used = 0;
    };
    for (int64_t n = n0; n < n1; ++n) {
        if (n > n0 && n % HIST_CHUNK_SAMPLES == 0) close(n);
        const int64_t lab = label[n];
        if (lab < b0 || lab >= b1) {
            slot[n] = (uint8_t)HIST_NO_SLOT;
            continue;
        }
        if (stamp[(size_t)lab] != chunk) {
            if (used == HIST_SLOTS) close(n);
            stamp[(size_t)lab] = chunk;
            slot_of[(size_t)lab] = (uint8_t)used++;
            out.rec_bin.push_back((int32_t)lab);
        }
        slot[n] = slot_of[(size_t)lab];
    }
    if (n1 > n0) close(n1);
}

HostTile build_tile(const int32_t* label, int64_t N, int64_t nbins, int64_t b0, int64_t b1) {
    HostTile t;
    t.b0 = b0;
    t.b1 = b1;
    t.slot.resize((size_t)N);
    const int64_t blocks = (N + HIST_CHUNK_SAMPLES - 1) / HIST_CHUNK_SAMPLES;
    const int64_t hw = (int64_t)std::thread::hardware_concurrency();
    const int64_t nthr = std::max<int64_t>(1, std::min<int64_t>({(int64_t)8, hw > 0 ? hw : 1, blocks / 64}));
    std::vector<TilePiece> pieces((size_t)nthr);
    auto run = [&](int64_t p) {
        const int64_t n0 = std::min(N, (p * blocks / nthr) * HIST_CHUNK_SAMPLES), n1 = std::min(N, ((p + 1) * blocks / nthr) * HIST_CHUNK_SAMPLES);
        build_piece(label, n0, n1, nbins, b0, b1, t.slot.data(), pieces[(size_t)p]);
    };
    std::vector<std::thread> team;
    for (int64_t p = 1; p < nthr; ++p) team.emplace_back(run, p);
    run(0);
    for (std::thread& th : team) th.join();
    std::vector<int32_t> rec_bin;
    t.chunk_n.push_back(0);
    t.chunk_rec.push_back(0);
    for (const TilePiece& pc : pieces) {
        for (size_t c = 0; c < pc.chunk_end.size(); ++c) {
            t.chunk_n.push_back(pc.chunk_end[c]);
            t.chunk_rec.push_back(t.chunk_rec.back() + pc.chunk_nb[c]);
        }
        rec_bin.insert(rec_bin.end(), pc.rec_bin.begin(), pc.rec_bin.end());
    }
    t.bin_ptr.assign((size_t)nbins + 1, 0);
    for (int32_t b : rec_bin) ++t.bin_ptr[(size_t)b + 1];
    for (int64_t i = 0; i < nbins; ++i) t.bin_ptr[(size_t)i + 1] += t.bin_ptr[(size_t)i];
    t.bin_rec.resize(rec_bin.size());
    std::vector<int64_t> fill(t.bin_ptr.begin(), t.bin_ptr.end() - 1);
    for (size_t r = 0; r < rec_bin.size(); ++r) t.bin_rec[(size_t)fill[(size_t)rec_bin[r]]++] = (int64_t)r;
    return t;
}

// (the label path serves any number of states)
int hist_ready(mbar_ctx* c, const char* who) { return passes_ready(c, who, "the binned passes", 0); }

HistSweep sweep_of(const mbar_ctx* c, const HistTile& t) {
    HistSweep h;
    h.N = c->N;
    h.nbins = c->hist_nbins;
    h.b0 = t.b0;
    h.b1 = t.b1;
    h.nchunks = t.nchunks;
    h.nrec = t.nrec;
    h.chunk_n = t.chunk_n;
    h.chunk_rec = t.chunk_rec;
    h.slot = t.slot;
    h.bin_ptr = t.bin_ptr;
    h.bin_rec = t.bin_rec;
    h.label = c->hist_label;
    h.v = c->hist_v;
    h.logden = c->logden[0];
    h.cw = c->weighted ? c->cw.p : nullptr;
    return h;
}

}  // namespace

extern "C" {

int mbar_ctx_set_bins(mbar_ctx* c, int64_t nbins, const int32_t* label_host, const double* v_host) {
    int rc = hist_ready(c, "mbar_ctx_set_bins");
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (nbins == 0) {
        c->hist_nbins = 0;
        c->hist_tiles.clear();
        c->hist_label.reset();
        c->hist_v.reset();
        c->hist_rec.reset();
        c->hist_out.reset();
        return MBAR_OK;
    }
    if (nbins < 0 || nbins > 0x7fffffff || !label_host || !v_host) return fail(c, MBAR_ERR_ARG, "mbar_ctx_set_bins: bad argument");
    const int64_t N = c->N;
    bool bad_label = false, bad_v = false;
    for (int64_t n = 0; n < N; ++n) {
        bad_label |= (label_host[n] < -1) | (label_host[n] >= nbins);
        bad_v |= (v_host[n] != v_host[n]) | (v_host[n] == -std::numeric_limits<double>::infinity());
    }
    if (bad_label) return fail(c, MBAR_ERR_ARG, "mbar_ctx_set_bins: labels must lie in [-1, nbins)");
    if (bad_v) return fail(c, MBAR_ERR_ARG, "mbar_ctx_set_bins: the target potential must not hold NaN or -inf");
    // tiles of bins: as few as keep the records of one sweep ((K + 2) doubles per record) within the budget
    const int64_t per_rec = (c->K + 2) * (int64_t)sizeof(double);
    std::vector<HostTile> tiles;
    for (int64_t T = 1;; T = std::min(nbins, 2 * T)) {
        tiles.clear();
        int64_t worst = 0;
        for (int64_t t = 0; t < T; ++t) {
            tiles.push_back(build_tile(label_host, N, nbins, t * nbins / T, (t + 1) * nbins / T));
            worst = std::max(worst, tiles.back().nrec());
        }
        if (worst * per_rec <= c->opt_hist_part_bytes || T >= nbins) break;
    }
    c->hist_tiles.clear();
    int64_t worst = 0;
    for (const HostTile& t : tiles) {
        c->hist_tiles.emplace_back();
        HistTile& d = c->hist_tiles.back();
        d.b0 = t.b0;
        d.b1 = t.b1;
        d.nchunks = (int64_t)t.chunk_n.size() - 1;
        d.nrec = t.nrec();
        HIPCHK(c, put(d.chunk_n, t.chunk_n));
        HIPCHK(c, put(d.chunk_rec, t.chunk_rec));
        HIPCHK(c, put(d.bin_ptr, t.bin_ptr));
        HIPCHK(c, put(d.bin_rec, t.bin_rec));
        HIPCHK(c, put(d.slot, t.slot));
        worst = std::max(worst, d.nrec);
    }
    HIPCHK(c, c->hist_label.upload(label_host, (size_t)std::max<int64_t>(N, 1)));
    HIPCHK(c, c->hist_v.upload(v_host, (size_t)std::max<int64_t>(N, 1)));
    HIPCHK(c, c->hist_rec.grow((size_t)std::max<int64_t>(worst, 1) * (size_t)(c->K + 2)));
    HIPCHK(c, c->hist_out.grow((size_t)nbins * (size_t)(c->K + 4)));
    c->hist_nbins = nbins;
    return MBAR_OK;
}

int mbar_ctx_bins_info(mbar_ctx* c, int64_t* sweeps, int64_t* chunks, int64_t* record_bytes) {
    if (!c) return fail(c, MBAR_ERR_ARG, "NULL argument");
    if (c->hist_nbins < 1) return fail(c, MBAR_ERR_STATE, "mbar_ctx_bins_info: no bins on this context (mbar_ctx_set_bins first)");
    int64_t nch = 0, worst = 0;
    for (const HistTile& t : c->hist_tiles) {
        nch += t.nchunks;
        worst = std::max(worst, t.nrec);
    }
    if (sweeps) *sweeps = (int64_t)c->hist_tiles.size();
    if (chunks) *chunks = nch;
    if (record_bytes) *record_bytes = worst * (c->K + 2) * (int64_t)sizeof(double);
    return MBAR_OK;
}

int mbar_bin_lognum(mbar_ctx* c, const double* f, double* lognum_bins) {
    int rc = hist_ready(c, "mbar_bin_lognum");
    if (rc) return rc;
    if (!f || !lognum_bins) return fail(c, MBAR_ERR_ARG, "NULL argument");
    if (c->hist_nbins < 1) return fail(c, MBAR_ERR_STATE, "mbar_bin_lognum: no bins on this context (mbar_ctx_set_bins first)");
    HIPCHK(c, hipSetDevice(c->device));
    bool nan = false;
    rc = pass_logden(c, f, &nan);
    if (rc) return rc;
    const int64_t nbins = c->hist_nbins;
    if (nan) {
        std::fill(lognum_bins, lognum_bins + nbins, std::numeric_limits<double>::quiet_NaN());
        return MBAR_OK;
    }
    double* binmax = c->hist_out;
    double* out = binmax + nbins;
    double* rec = c->hist_rec;
    {
        ScopedTimer t(c, MBAR_TIMER_OTHER);
        for (const HistTile& tile : c->hist_tiles) {
            const HistSweep h = sweep_of(c, tile);
            HIPCHK(c, launch_hist_vec(c->stream, h, HIST_MAX, nullptr, rec, nullptr));
            HIPCHK(c, launch_hist_vec_combine(c->stream, h, HIST_MAX, rec, nullptr, nullptr, binmax, nullptr));
            HIPCHK(c, launch_hist_vec(c->stream, h, HIST_SUMEXP, binmax, rec, nullptr));
            HIPCHK(c, launch_hist_vec_combine(c->stream, h, HIST_SUMEXP, rec, nullptr, binmax, out, nullptr));
        }
    }
    HIPCHK(c, hipMemcpyAsync(lognum_bins, out, (size_t)nbins * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return sync_stream(c);
}

int mbar_bin_gram_w(mbar_ctx* c, const double* f, const double* f_bins, double* cross, double* diag, double* wsum_bins) {
    int rc = hist_ready(c, "mbar_bin_gram_w");
    if (rc) return rc;
    if (!f || !f_bins || !diag || !wsum_bins) return fail(c, MBAR_ERR_ARG, "NULL argument");
    if (c->hist_nbins < 1) return fail(c, MBAR_ERR_STATE, "mbar_bin_gram_w: no bins on this context (mbar_ctx_set_bins first)");
    HIPCHK(c, hipSetDevice(c->device));
    bool nan = false;
    rc = pass_logden(c, f, &nan);
    if (rc) return rc;
    const int64_t nbins = c->hist_nbins, K = c->K;
    for (int64_t i = 0; i < nbins; ++i) nan = nan || std::isnan(f_bins[i]);
    if (nan) {
        const double q = std::numeric_limits<double>::quiet_NaN();
        if (cross) std::fill(cross, cross + (size_t)K * nbins, q);
        std::fill(diag, diag + nbins, q);
        std::fill(wsum_bins, wsum_bins + nbins, q);
        return MBAR_OK;
    }
    double* d_w = c->hist_out + nbins;
    double* d_diag = d_w + nbins;
    double* d_cross = d_diag + nbins;
    double* d_fbin = d_cross + (size_t)K * nbins;
    double* rec_a = c->hist_rec;
    HIPCHK(c, hipMemcpyAsync(d_f(c), f, (size_t)K * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_fbin, f_bins, (size_t)nbins * sizeof(double), hipMemcpyHostToDevice, c->stream));
    {
        ScopedTimer t(c, MBAR_TIMER_OTHER);
        for (const HistTile& tile : c->hist_tiles) {
            const HistSweep h = sweep_of(c, tile);
            double* rec_b = rec_a + tile.nrec;
            HIPCHK(c, launch_hist_vec(c->stream, h, HIST_NORM, d_fbin, rec_a, rec_b));
            HIPCHK(c, launch_hist_vec_combine(c->stream, h, HIST_NORM, rec_a, rec_b, nullptr, d_w, d_diag));
            if (cross) {
                HIPCHK(c, launch_hist_cross(c->stream, h, c->u, c->ld, K, d_f(c), d_fbin, rec_a));
                HIPCHK(c, launch_hist_cross_combine(c->stream, h, K, rec_a, d_cross));
            }
        }
    }
    HIPCHK(c, hipMemcpyAsync(wsum_bins, d_w, (size_t)nbins * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(diag, d_diag, (size_t)nbins * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (cross) HIPCHK(c, hipMemcpyAsync(cross, d_cross, (size_t)K * nbins * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return sync_stream(c);
}

}  // extern "C"
