// Host side of the histogram free energy surfaces along a scan (include/mbar_hip.h, "histogram surfaces along a scan"): the
// stable counting sort of the samples by bin, the chunk tables of the two passes, the member panels of pass A and the bin groups
// of pass B under the record budget, and the C ABI.  Kernels: mbar_k_scanbin.hip.
#include "mbar_ctx.h"

using namespace mbar;
using namespace mbar::host;

namespace {

// perm (sorted position -> sample, ascending n inside a bin, label -1 dropped) and bin_start[nbins + 1]; false: a label outside
// [-1, nbins)
bool bins_table(int64_t N, int64_t nbins, const int32_t* label, int32_t* perm, int64_t* bin_start) {
    std::fill(bin_start, bin_start + nbins + 1, (int64_t)0);
    for (int64_t n = 0; n < N; ++n) {
        const int64_t lab = label[n];
        if (lab < -1 || lab >= nbins) return false;
        if (lab >= 0) ++bin_start[lab + 1];
    }
    for (int64_t i = 0; i < nbins; ++i) bin_start[i + 1] += bin_start[i];
    std::vector<int64_t> fill(bin_start, bin_start + nbins);
    for (int64_t n = 0; n < N; ++n)
        if (label[n] >= 0) perm[fill[(size_t)label[n]]++] = (int32_t)n;
    return true;
}

// chunks of at most `len` sorted positions, cut from the start of every bin: the bin of each chunk and the first chunk of each bin
void chunk_table(const std::vector<int64_t>& bin_start, int64_t len, std::vector<int32_t>& chunk_bin, std::vector<int64_t>& bin_chunk0) {
    const int64_t nbins = (int64_t)bin_start.size() - 1;
    bin_chunk0.assign((size_t)nbins + 1, 0);
    chunk_bin.clear();
    for (int64_t i = 0; i < nbins; ++i) {
        const int64_t nch = (bin_start[(size_t)i + 1] - bin_start[(size_t)i] + len - 1) / len;
        bin_chunk0[(size_t)i + 1] = bin_chunk0[(size_t)i] + nch;
        chunk_bin.insert(chunk_bin.end(), (size_t)nch, (int32_t)i);
    }
}

template <class T>
hipError_t put(DevBuf<T>& d, const std::vector<T>& h) {
    return h.empty() ? d.grow(1) : d.upload(h.data(), h.size());
}

void release(mbar_ctx* c) {
    c->scanbin_nbins = c->scanbin_chunks_a = c->scanbin_chunks_b = 0;
    c->scanbin_perm.reset();
    c->scanbin_start.reset();
    c->scanbin_cbin_a.reset();
    c->scanbin_cbin_b.reset();
    c->scanbin_c0_a.reset();
    c->scanbin_c0_b.reset();
    c->scanbin_fbins.reset();
    c->scanbin_c0_b_host.clear();
}

ScanBins bins_of(const mbar_ctx* c) {
    ScanBins sb;
    sb.nbins = c->scanbin_nbins;
    sb.perm = c->scanbin_perm;
    sb.bin_start = c->scanbin_start;
    return sb;
}

// the checks both passes share, after scan_ready
int pass_ready(mbar_ctx* c, const std::string& who) {
    if (c->scan_B < 1) return fail(c, MBAR_ERR_STATE, who + ": no basis on this context (mbar_ctx_set_scan first)");
    if (c->scan_Q != 0) return fail(c, MBAR_ERR_STATE, who + ": the binned scan passes take a family without observables (Q = 0)");
    if (c->scanbin_nbins < 1) return fail(c, MBAR_ERR_STATE, who + ": no bins on this context (mbar_ctx_set_scan_bins first)");
    return MBAR_OK;
}

}  // namespace

extern "C" {

int mbar_scan_bins_table(int64_t N, int64_t nbins, const int32_t* label, int32_t* perm_out, int64_t* bin_start_out) {
    if (N < 0 || nbins < 1 || nbins > 0x7fffffff || (N > 0 && (!label || !perm_out)) || !bin_start_out)
        return fail(nullptr, MBAR_ERR_ARG, "mbar_scan_bins_table: bad argument");
    if (N >= ((int64_t)1 << 31)) return fail(nullptr, MBAR_ERR_STATE, "mbar_scan_bins_table: the sorted positions are 32-bit, N must stay below 2^31");
    if (!bins_table(N, nbins, label, perm_out, bin_start_out)) return fail(nullptr, MBAR_ERR_ARG, "mbar_scan_bins_table: labels must lie in [-1, nbins)");
    return MBAR_OK;
}

int mbar_ctx_set_scan_bins(mbar_ctx* c, int64_t nbins, const int32_t* label_host) {
    int rc = scan_ready(c, "mbar_ctx_set_scan_bins");
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (nbins == 0) {
        release(c);
        return MBAR_OK;
    }
    if (nbins < 0 || nbins > 0x7fffffff || !label_host) return fail(c, MBAR_ERR_ARG, "mbar_ctx_set_scan_bins: bad argument");
    const int64_t N = c->N;
    if (N >= ((int64_t)1 << 31)) return fail(c, MBAR_ERR_STATE, "mbar_ctx_set_scan_bins: the sorted positions are 32-bit, N must stay below 2^31");
    std::vector<int32_t> perm((size_t)std::max<int64_t>(N, 1));
    std::vector<int64_t> bin_start((size_t)nbins + 1);
    if (!bins_table(N, nbins, label_host, perm.data(), bin_start.data()))
        return fail(c, MBAR_ERR_ARG, "mbar_ctx_set_scan_bins: labels must lie in [-1, nbins)");
    std::vector<int32_t> cbin_a, cbin_b;
    std::vector<int64_t> c0_a, c0_b;
    chunk_table(bin_start, SCAN_VCHUNK, cbin_a, c0_a);
    chunk_table(bin_start, SCAN_CHUNK, cbin_b, c0_b);
    release(c);
    HIPCHK(c, c->scanbin_perm.upload(perm.data(), perm.size()));
    HIPCHK(c, put(c->scanbin_start, bin_start));
    HIPCHK(c, put(c->scanbin_cbin_a, cbin_a));
    HIPCHK(c, put(c->scanbin_cbin_b, cbin_b));
    HIPCHK(c, put(c->scanbin_c0_a, c0_a));
    HIPCHK(c, put(c->scanbin_c0_b, c0_b));
    c->scanbin_chunks_a = (int64_t)cbin_a.size();
    c->scanbin_chunks_b = (int64_t)cbin_b.size();
    c->scanbin_c0_b_host = std::move(c0_b);
    c->scanbin_nbins = nbins;
    return MBAR_OK;
}

int mbar_scan_bin_lognum(mbar_ctx* c, const double* f, int64_t L, const double* coeff, const double* offset, double* lognum) {
    int rc = scan_ready(c, "mbar_scan_bin_lognum");
    if (rc) return rc;
    if (!f || !coeff || !lognum || L < 1) return fail(c, MBAR_ERR_ARG, "mbar_scan_bin_lognum: bad argument");
    rc = pass_ready(c, "mbar_scan_bin_lognum");
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    bool nan = false;
    rc = scan_logden(c, f, &nan);
    if (rc) return rc;
    const int64_t B = c->scan_B, nbins = c->scanbin_nbins;
    if (nan) {
        std::fill(lognum, lognum + (size_t)L * nbins, std::numeric_limits<double>::quiet_NaN());
        return MBAR_OK;
    }
    rc = scan_upload_members(c, L, coeff, offset, nullptr);
    if (rc) return rc;
    const ScanData d = scan_data_of(c);
    const ScanBins sb = bins_of(c);
    ScanBinTable t;
    t.nchunks = c->scanbin_chunks_a;
    t.chunk_bin = c->scanbin_cbin_a;
    t.bin_chunk0 = c->scanbin_c0_a;
    // members in panels of a multiple of 64 whose records ([chunk][member]) fit the budget ("scan_part_bytes"): a (member, bin)'s
    // sums do not depend on the cut
    const int64_t nch = std::max<int64_t>(t.nchunks, 1);
    int64_t pw = c->opt_scan_part_bytes / (nch * (int64_t)sizeof(double)) / 64 * 64;
    pw = std::min<int64_t>(std::max<int64_t>(pw, 64), (L + 63) / 64 * 64);
    HIPCHK(c, c->scan_part.grow((size_t)nch * (size_t)pw));
    HIPCHK(c, c->scan_out.grow((size_t)L * (size_t)nbins + (size_t)nbins * (size_t)pw));
    double* d_lognum = c->scan_out;
    double* d_M = d_lognum + L * nbins;  // [bin][member of the panel]
    const double* d_coeff = c->scan_in;
    const double* d_off = d_coeff + L * B;
    {
        ScopedTimer timer(c, MBAR_TIMER_OTHER);
        for (int64_t p0 = 0; p0 < L; p0 += pw) {
            const int64_t pl = std::min(pw, L - p0);
            HIPCHK(c, launch_scanbin_vec(c->stream, d, sb, t, false, pl, d_coeff + p0 * B, d_off + p0, nullptr, c->scan_part));
            HIPCHK(c, launch_scanbin_vec_merge(c->stream, sb, t, false, pl, c->scan_part, d_M, nullptr));
            HIPCHK(c, launch_scanbin_vec(c->stream, d, sb, t, true, pl, d_coeff + p0 * B, d_off + p0, d_M, c->scan_part));
            HIPCHK(c, launch_scanbin_vec_merge(c->stream, sb, t, true, pl, c->scan_part, d_M, d_lognum + p0 * nbins));
        }
    }
    HIPCHK(c, hipMemcpyAsync(lognum, d_lognum, (size_t)L * nbins * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return sync_stream(c);
}

int mbar_scan_bin_gram_w(mbar_ctx* c, const double* f, int64_t L, const double* coeff, const double* offset, const double* f_bins,
                         double* cross, double* diag, double* wsum) {
    int rc = scan_ready(c, "mbar_scan_bin_gram_w");
    if (rc) return rc;
    if (!f || !coeff || !f_bins || !diag || !wsum || L < 1) return fail(c, MBAR_ERR_ARG, "mbar_scan_bin_gram_w: bad argument");
    rc = pass_ready(c, "mbar_scan_bin_gram_w");
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    bool nan = false;
    rc = scan_logden(c, f, &nan);
    if (rc) return rc;
    const int64_t B = c->scan_B, K = c->K, nbins = c->scanbin_nbins;
    const size_t LB = (size_t)L * (size_t)nbins;
    for (size_t x = 0; x < LB; ++x) nan = nan || std::isnan(f_bins[x]);
    if (nan) {
        const double q = std::numeric_limits<double>::quiet_NaN();
        if (cross) std::fill(cross, cross + (size_t)K * LB, q);
        std::fill(diag, diag + LB, q);
        std::fill(wsum, wsum + LB, q);
        return MBAR_OK;
    }
    rc = scan_upload_members(c, L, coeff, offset, nullptr);
    if (rc) return rc;
    HIPCHK(c, c->scanbin_fbins.grow(LB));
    HIPCHK(c, hipMemcpyAsync(c->scanbin_fbins, f_bins, LB * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const ScanData d = scan_data_of(c);
    const ScanBins sb = bins_of(c);
    ScanBinTable t;
    t.nchunks = c->scanbin_chunks_b;
    t.chunk_bin = c->scanbin_cbin_b;
    t.bin_chunk0 = c->scanbin_c0_b;
    const int nb = cross ? scan_nb_for(K) : 0;
    // groups of whole bins whose records fit the budget ("scan_part_bytes"; a single bin is never split): one sweep per group, and
    // a (member, bin)'s sums do not depend on the cut
    const int64_t rec = scanbin_record_doubles(nb);
    const int64_t max_chunks = std::max<int64_t>(c->opt_scan_part_bytes / (rec * (int64_t)sizeof(double)), 1);
    const std::vector<int64_t>& c0 = c->scanbin_c0_b_host;
    std::vector<int64_t> group{0};  // first bin of every group, then nbins
    for (int64_t i = 1; i < nbins; ++i)
        if (c0[(size_t)i + 1] - c0[(size_t)group.back()] > max_chunks) group.push_back(i);
    group.push_back(nbins);
    int64_t worst = 1;
    for (size_t g = 0; g + 1 < group.size(); ++g) worst = std::max(worst, c0[(size_t)group[g + 1]] - c0[(size_t)group[g]]);
    HIPCHK(c, c->scan_part.grow((size_t)worst * (size_t)rec));
    HIPCHK(c, c->scan_out.grow(LB * SCANBIN_NV + (cross ? (size_t)K * LB : 0)));
    double* d_vec = c->scan_out;
    double* d_cross = d_vec + LB * SCANBIN_NV;
    const double* d_coeff = c->scan_in;
    const double* d_off = d_coeff + L * B;
    HIPCHK(c, hipMemcpyAsync(d_f(c), f, (size_t)K * sizeof(double), hipMemcpyHostToDevice, c->stream));
    {
        ScopedTimer timer(c, MBAR_TIMER_OTHER);
        for (size_t g = 0; g + 1 < group.size(); ++g) {
            const int64_t b0 = group[g], b1 = group[g + 1], g0 = c0[(size_t)b0], g1 = c0[(size_t)b1];
            for (int64_t p0 = 0; p0 < L; p0 += 256) {  // the group's samples of the resident matrix are read once per panel
                HIPCHK(c, launch_scanbin_cross(c->stream, d, sb, t, g0, g1, nb, c->u, c->ld, K, d_f(c), L, p0, d_coeff, d_off, c->scanbin_fbins,
                                               c->scan_part));
                HIPCHK(c, launch_scanbin_cross_merge(c->stream, sb, t, g0, b0, b1, nb, K, L, p0, c->scan_part, d_cross, d_vec));
            }
        }
    }
    std::vector<double> vec(LB * SCANBIN_NV);
    HIPCHK(c, hipMemcpyAsync(vec.data(), d_vec, vec.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (cross) HIPCHK(c, hipMemcpyAsync(cross, d_cross, (size_t)K * LB * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    rc = sync_stream(c);
    if (rc) return rc;
    for (size_t x = 0; x < LB; ++x) {
        wsum[x] = vec[x * SCANBIN_NV];
        diag[x] = vec[x * SCANBIN_NV + 1];
    }
    return MBAR_OK;
}

}  // extern "C"
