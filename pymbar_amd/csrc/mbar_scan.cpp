// Host side of the reweighting scans over a linear family of unsampled states (include/mbar_hip.h, "reweighting scans") and of the
// histogram free energy surfaces along such a scan ("histogram surfaces along a scan"): the upload of the basis and observable
// vectors, the stable counting sort of the samples by bin and the chunk tables of the two passes, the member panels and the bin
// groups under the record budget, and the C ABI.  Kernels: mbar_k_scan.hip, one source for both cuts of the samples.
#include "mbar_ctx.h"
#include "mbar_scan_moments.h"

#include <initializer_list>

using namespace mbar;
using namespace mbar::host;

namespace {

constexpr int64_t SCAN_MAX_K = 128;  // one W tile of the cross kernel

int scan_ready(mbar_ctx* c, const char* who) { return passes_ready(c, who, "the scan passes", SCAN_MAX_K); }

ScanData scan_data_of(const mbar_ctx* c) {
    ScanData d;
    d.N = c->N;
    d.ldv = c->ld;
    d.B = (int)c->scan_B;
    d.Q = (int)c->scan_Q;
    d.basis = c->scan_vec;
    d.t = c->scan_vec.p + c->scan_B * c->ld;
    d.logden = c->logden[0];
    d.cw = c->weighted ? c->cw.p : nullptr;
    return d;
}

// The two sweeps on the context's family: the linear instantiations unless a harmonic term is set (mbar_ctx_set_scan_terms); l0:
// the member the coeff / offset pointers of a pass-A panel start at (pass B takes the whole arrays and its own p0).  obs: where the
// observables come from, the stored ones of the context (ScanStored) or the members' own reduced potential (ScanEnergy, whole cut).
ScanHarmonic harmonic_of(const mbar_ctx* c) { return ScanHarmonic{c->scan_terms, c->scan_center.p}; }
template <class Cut, class Obs>
hipError_t sweep_vec(mbar_ctx* c, const ScanData& d, const Cut& cut, const Obs& obs, bool sum, int64_t l0, int64_t L, const double* coeff,
                     const double* offset, const double* M, double* rec) {
    if (c->scan_terms.mask) return launch_scan_vec(c->stream, d, cut, harmonic_of(c).from(l0), obs.from(l0), sum, L, coeff, offset, M, rec);
    return launch_scan_vec(c->stream, d, cut, ScanLinear{}, obs.from(l0), sum, L, coeff, offset, M, rec);
}
template <class Cut, class Obs>
hipError_t sweep_cross(mbar_ctx* c, const ScanData& d, const Cut& cut, const Obs& obs, int nb, int64_t L, int64_t p0, const double* coeff,
                       const double* offset, const double* fnorm) {
    if (c->scan_terms.mask)
        return launch_scan_cross(c->stream, d, cut, harmonic_of(c), obs, nb, c->u, c->ld, c->K, d_f(c), L, p0, coeff, offset, fnorm, c->scan_part);
    return launch_scan_cross(c->stream, d, cut, ScanLinear{}, obs, nb, c->u, c->ld, c->K, d_f(c), L, p0, coeff, offset, fnorm, c->scan_part);
}

// blocks of 16 members per wave of pass B on the context's family
template <class Obs>
int scan_mb_of(const mbar_ctx* c, int J) { return c->scan_terms.mask ? Obs::template mb<ScanHarmonic>(J) : Obs::template mb<ScanLinear>(J); }

void release_terms(mbar_ctx* c) {
    c->scan_terms = FamilyTerms{};
    c->scan_center_L = 0;
    c->scan_center.reset();
}

// How the four passes open.  scan_open: the limits of the context, the caller's own argument check (args_ok), what the family
// needs on the context, the device.
int scan_open(mbar_ctx* c, const std::string& who, bool args_ok, bool binned, int64_t L) {
    int rc = scan_ready(c, who.c_str());
    if (rc) return rc;
    if (!args_ok) return fail(c, MBAR_ERR_ARG, who + ": bad argument");
    if (c->scan_B < 1) return fail(c, MBAR_ERR_STATE, who + ": no basis on this context (mbar_ctx_set_scan first)");
    if (binned && c->scan_Q != 0) return fail(c, MBAR_ERR_STATE, who + ": the binned scan passes take a family without observables (Q = 0)");
    if (binned && c->scanbin_nbins < 1) return fail(c, MBAR_ERR_STATE, who + ": no bins on this context (mbar_ctx_set_scan_bins first)");
    if (c->scan_terms.mask && c->scan_center_L != L)
        return fail(c, MBAR_ERR_STATE, who + ": the family has harmonic terms and " +
                                           (c->scan_center_L ? "the centres on this context are those of " + std::to_string(c->scan_center_L) +
                                                                   " members, not of " + std::to_string(L)
                                                             : std::string("no centres are set")) +
                                           " (mbar_ctx_set_scan_centers first)");
    HIPCHK(c, hipSetDevice(c->device));
    return MBAR_OK;
}

// scan_begin, once the sizes are known: the log-denominators of f; with an unusable matrix or f, or a NaN among the members'
// normalisers fnorm[nnorm] (NULL: none), or with *done set by the caller (a NaN among what only it takes), every output is filled with NaN and *done is set (the call returns MBAR_OK); otherwise
// scan_part / scan_out are sized for the call's partial records and merged outputs (part_doubles, out_doubles: before anything of
// the call is queued), coeff | offset (NULL: zeros) | room for L normalisers go to the device and *d is the family as the kernels
// see it.
struct ScanOut {
    double* p;  // (NULL: not asked for)
    size_t n;
};
int scan_begin(mbar_ctx* c, const double* f, int64_t L, const double* coeff, const double* offset, const double* fnorm, size_t nnorm,
               std::initializer_list<ScanOut> outs, size_t part_doubles, size_t out_doubles, bool* done, ScanData* d, size_t in_extra = 0) {
    bool nan = false;
    if (c->scan_terms.mask)  // (the linear family keeps what it always did with such a member)
        for (int64_t x = 0; x < L * c->scan_B; ++x)
            if (!std::isfinite(coeff[x])) return fail(c, MBAR_ERR_ARG, "the coefficients of a family with harmonic terms must be finite");
    int rc = pass_logden(c, f, &nan);
    if (rc) return rc;
    nan = nan || *done;
    for (size_t x = 0; x < nnorm; ++x) nan = nan || std::isnan(fnorm[x]);
    *done = nan;
    if (nan) {
        for (const ScanOut& o : outs)
            if (o.p) std::fill(o.p, o.p + o.n, std::numeric_limits<double>::quiet_NaN());
        return MBAR_OK;
    }
    const int64_t B = c->scan_B;
    // coeff | offset | normalisers | centres of the energy observable | in_extra: the centres of the features (mbar_scan_moments)
    HIPCHK(c, c->scan_in.grow((size_t)L * (size_t)(B + 3) + in_extra));
    HIPCHK(c, c->scan_part.grow(part_doubles));
    HIPCHK(c, c->scan_out.grow(out_doubles));
    double* d_coeff = c->scan_in;
    double* d_off = d_coeff + L * B;
    HIPCHK(c, hipMemcpyAsync(d_coeff, coeff, (size_t)L * B * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (offset) HIPCHK(c, hipMemcpyAsync(d_off, offset, (size_t)L * sizeof(double), hipMemcpyHostToDevice, c->stream));
    else HIPCHK(c, hipMemsetAsync(d_off, 0, (size_t)L * sizeof(double), c->stream));
    *d = scan_data_of(c);
    return MBAR_OK;
}

// member panels of pass A: a multiple of 64 members whose records ([chunk][member][J]) fit the budget ("scan_part_bytes"); a
// member's sums, and a (member, bin)'s, do not depend on the cut
int64_t vec_panel(const mbar_ctx* c, int64_t nchunks, int64_t J, int64_t L) {
    const int64_t pw = c->opt_scan_part_bytes / (nchunks * J * (int64_t)sizeof(double)) / 64 * 64;
    return std::min<int64_t>(std::max<int64_t>(pw, 64), (L + 63) / 64 * 64);
}

// ---- the binned cut: the samples sorted by bin, and the chunk tables ----
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

// every bin of the context and every chunk of pass A's table (pass_b = false) or of pass B's
ScanBinned binned_of(const mbar_ctx* c, bool pass_b) {
    ScanBinned s;
    s.sb.nbins = c->scanbin_nbins;
    s.sb.perm = c->scanbin_perm;
    s.sb.bin_start = c->scanbin_start;
    s.t.nchunks = pass_b ? c->scanbin_chunks_b : c->scanbin_chunks_a;
    s.t.chunk_bin = pass_b ? c->scanbin_cbin_b : c->scanbin_cbin_a;
    s.t.bin_chunk0 = pass_b ? c->scanbin_c0_b : c->scanbin_c0_a;
    s.b0_ = s.c0_ = 0;
    s.b1_ = s.sb.nbins;
    s.c1_ = s.t.nchunks;
    return s;
}

// ---- the two passes of the whole cut, written once for either kind of observable ----
// The observables of a whole-cut call: the context's stored ones (J = 1 + Q), or the members' own reduced potential about
// center_u[L] (NULL: zeros) with J = 2 or 3 (the context's Q is ignored).
struct WholeObs {
    bool energy = false;
    const double* center_u = nullptr;
    int64_t J = 0;
};
bool obs_ok(const WholeObs& o) { return !o.energy || o.J == 2 || o.J == 3; }
bool obs_nan(const WholeObs& o, int64_t L) {
    bool nan = false;
    if (o.energy && o.center_u)
        for (int64_t l = 0; l < L; ++l) nan = nan || std::isnan(o.center_u[l]);
    return nan;
}
// the family as the kernels of the call see it, and the centres of the energy observable behind the normalisers in scan_in
int obs_begin(mbar_ctx* c, const WholeObs& o, int64_t L, ScanData* d, ScanEnergy* e) {
    if (!o.energy) return MBAR_OK;
    for (int64_t l = 0; o.center_u && l < L; ++l)
        if (std::isinf(o.center_u[l])) return fail(c, MBAR_ERR_ARG, "the centres of the energy observable must be finite");
    d->Q = (int)o.J - 1;
    double* d_cu = c->scan_in.p + L * (c->scan_B + 2);
    if (o.center_u) HIPCHK(c, hipMemcpyAsync(d_cu, o.center_u, (size_t)L * sizeof(double), hipMemcpyHostToDevice, c->stream));
    else HIPCHK(c, hipMemsetAsync(d_cu, 0, (size_t)L * sizeof(double), c->stream));
    e->center_u = d_cu;
    return MBAR_OK;
}

int whole_lognum(mbar_ctx* c, const char* who, const WholeObs& o, const double* f, int64_t L, const double* coeff, const double* offset,
                 double* lognum, double* mean) {
    int rc = scan_open(c, who, f && coeff && lognum && L >= 1 && obs_ok(o), false, L);
    if (rc) return rc;
    const int64_t B = c->scan_B, J = o.energy ? o.J : 1 + c->scan_Q;
    bool done = obs_nan(o, L);
    ScanData d;
    ScanEnergy energy{nullptr};
    const int64_t nchunks = std::max<int64_t>((c->N + SCAN_VCHUNK - 1) / SCAN_VCHUNK, 1);
    const int64_t pw = vec_panel(c, nchunks, J, L);
    rc = scan_begin(c, f, L, coeff, offset, nullptr, 0, {{lognum, (size_t)L}, {mean, (size_t)(L * J)}},
                    (size_t)nchunks * (size_t)pw * (size_t)J, (size_t)L * (size_t)(2 + J), &done, &d);
    if (rc || done) return rc;
    rc = obs_begin(c, o, L, &d, &energy);
    if (rc) return rc;
    double* d_M = c->scan_out;
    double* d_lognum = d_M + L;
    double* d_mean = d_lognum + L;
    const double* d_coeff = c->scan_in;
    const double* d_off = d_coeff + L * B;
    const ScanWhole cut{};
    auto sweep = [&](bool sum, int64_t p0, int64_t pl, const double* M) {
        if (o.energy) return sweep_vec(c, d, cut, energy, sum, p0, pl, d_coeff + p0 * B, d_off + p0, M, c->scan_part);
        return sweep_vec(c, d, cut, ScanStored{}, sum, p0, pl, d_coeff + p0 * B, d_off + p0, M, c->scan_part);
    };
    {
        ScopedTimer timer(c, MBAR_TIMER_OTHER);
        for (int64_t p0 = 0; p0 < L; p0 += pw) {
            const int64_t pl = std::min(pw, L - p0);
            HIPCHK(c, sweep(false, p0, pl, nullptr));
            HIPCHK(c, launch_scan_vec_merge(c->stream, d, cut, false, pl, c->scan_part, d_M + p0, nullptr, nullptr));
            HIPCHK(c, sweep(true, p0, pl, d_M + p0));
            HIPCHK(c, launch_scan_vec_merge(c->stream, d, cut, true, pl, c->scan_part, d_M + p0, d_lognum + p0, d_mean + p0 * J));
        }
    }
    HIPCHK(c, hipMemcpyAsync(lognum, d_lognum, (size_t)L * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (mean) HIPCHK(c, hipMemcpyAsync(mean, d_mean, (size_t)L * J * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return sync_stream(c);
}

// refrows: refcol[L][J] of the stored observables, refblock[L][2][J] of the energy observable
int whole_gram_w(mbar_ctx* c, const char* who, const WholeObs& o, const double* f, int64_t L, const double* coeff, const double* offset,
                 const double* f_scan, int64_t r, double* cross, double* within, double* refrows, double* wsum) {
    int rc = scan_open(c, who, f && coeff && f_scan && within && refrows && wsum && L >= 1 && r >= 0 && r < L && obs_ok(o), false, L);
    if (rc) return rc;
    const int64_t B = c->scan_B, K = c->K;
    const int J = o.energy ? (int)o.J : 1 + (int)c->scan_Q, NW = J * (J + 1) / 2;
    const int NR = (o.energy ? ScanEnergy::ref_rows : ScanStored::ref_rows) * J, NV = o.energy ? ScanEnergy::nv(J) : ScanStored::nv(J);
    bool done = obs_nan(o, L);
    ScanData d;
    ScanEnergy energy{nullptr};
    const int nb = cross ? scan_nb_for(K) : 0;
    const int64_t nchunks = (c->N + SCAN_CHUNK - 1) / SCAN_CHUNK;
    const int mb = o.energy ? scan_mb_of<ScanEnergy>(c, J) : scan_mb_of<ScanStored>(c, J);
    const int64_t pw = 64 * mb;
    rc = scan_begin(c, f, L, coeff, offset, f_scan, (size_t)L,
                    {{cross, (size_t)K * L * J}, {within, (size_t)(L * NW)}, {refrows, (size_t)(L * NR)}, {wsum, (size_t)L}},
                    (size_t)std::max<int64_t>(nchunks, 1) * (size_t)scan_record_doubles(nb, J, NV, mb),
                    (size_t)L * (size_t)NV + (cross ? (size_t)K * L * J : 0), &done, &d);
    if (rc || done) return rc;
    rc = obs_begin(c, o, L, &d, &energy);
    if (rc) return rc;
    double* d_vec = c->scan_out;
    double* d_cross = d_vec + L * NV;
    const double* d_coeff = c->scan_in;
    const double* d_off = d_coeff + L * B;
    double* d_fscan = c->scan_in.p + L * (B + 1);
    HIPCHK(c, hipMemcpyAsync(d_fscan, f_scan, (size_t)L * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_f(c), f, (size_t)K * sizeof(double), hipMemcpyHostToDevice, c->stream));
    ScanWhole cut;
    cut.ref = r;
    {
        ScopedTimer timer(c, MBAR_TIMER_OTHER);
        for (int64_t p0 = 0; p0 < L; p0 += pw) {  // the resident matrix is read once per panel
            if (o.energy) {
                HIPCHK(c, sweep_cross(c, d, cut, energy, nb, L, p0, d_coeff, d_off, d_fscan));
                HIPCHK(c, (launch_scan_cross_merge<ScanWhole, ScanEnergy>(c->stream, d, cut, nb, mb, K, L, p0, c->scan_part, d_cross, d_vec)));
            } else {
                HIPCHK(c, sweep_cross(c, d, cut, ScanStored{}, nb, L, p0, d_coeff, d_off, d_fscan));
                HIPCHK(c, (launch_scan_cross_merge<ScanWhole, ScanStored>(c->stream, d, cut, nb, mb, K, L, p0, c->scan_part, d_cross, d_vec)));
            }
        }
    }
    std::vector<double> vec((size_t)L * NV);
    HIPCHK(c, hipMemcpyAsync(vec.data(), d_vec, vec.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (cross) HIPCHK(c, hipMemcpyAsync(cross, d_cross, (size_t)K * L * J * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    rc = sync_stream(c);
    if (rc) return rc;
    for (int64_t l = 0; l < L; ++l) {
        const double* v = vec.data() + l * NV;
        wsum[l] = v[0];
        std::copy(v + 1, v + 1 + NR, refrows + l * NR);
        std::copy(v + 1 + NR, v + NV, within + l * NW);
    }
    return MBAR_OK;
}

}  // namespace

extern "C" {

int mbar_ctx_set_scan(mbar_ctx* c, int64_t B, const double* basis, int64_t Q, const double* t) {
    int rc = scan_ready(c, "mbar_ctx_set_scan");
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    release_terms(c);  // (a new basis, or none: all-linear again)
    if (B == 0) {
        c->scan_B = c->scan_Q = 0;
        c->scan_vec.reset();
        c->scan_in.reset();
        c->scan_part.reset();
        c->scan_out.reset();
        return MBAR_OK;
    }
    if (B < 1 || B > SCAN_MAX_B || Q < 0 || Q > SCAN_MAX_Q || !basis || (Q > 0 && !t))
        return fail(c, MBAR_ERR_ARG, "mbar_ctx_set_scan: 1 <= B <= 8 basis vectors and 0 <= Q <= 3 observables");
    const int64_t N = c->N, ld = c->ld;
    HIPCHK(c, c->scan_vec.grow((size_t)(B + Q) * (size_t)ld));
    HIPCHK(c, hipMemset(c->scan_vec, 0, (size_t)(B + Q) * (size_t)ld * sizeof(double)));
    HIPCHK(c, hipMemcpy2D(c->scan_vec, (size_t)ld * sizeof(double), basis, (size_t)N * sizeof(double), (size_t)N * sizeof(double), (size_t)B,
                          hipMemcpyHostToDevice));
    if (Q > 0)
        HIPCHK(c, hipMemcpy2D(c->scan_vec.p + B * ld, (size_t)ld * sizeof(double), t, (size_t)N * sizeof(double), (size_t)N * sizeof(double),
                              (size_t)Q, hipMemcpyHostToDevice));
    c->scan_B = B;
    c->scan_Q = Q;
    return MBAR_OK;
}

int mbar_ctx_set_scan_terms(mbar_ctx* c, const int32_t* kind, const double* period) {
    int rc = scan_ready(c, "mbar_ctx_set_scan_terms");
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!kind) {
        release_terms(c);
        return MBAR_OK;
    }
    if (c->scan_B < 1) return fail(c, MBAR_ERR_STATE, "mbar_ctx_set_scan_terms: no basis on this context (mbar_ctx_set_scan first)");
    FamilyTerms terms;
    rc = family_terms(c, "mbar_ctx_set_scan_terms", c->scan_B, kind, period, &terms);
    if (rc) return rc;
    release_terms(c);  // (centres of another family's slots mean nothing)
    c->scan_terms = terms;
    return MBAR_OK;
}

int mbar_ctx_set_scan_centers(mbar_ctx* c, int64_t L, const double* center) {
    int rc = scan_ready(c, "mbar_ctx_set_scan_centers");
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (L == 0 || !center) {
        if (L != 0) return fail(c, MBAR_ERR_ARG, "mbar_ctx_set_scan_centers: NULL centres for L != 0 members");
        c->scan_center_L = 0;
        return MBAR_OK;
    }
    if (L < 0) return fail(c, MBAR_ERR_ARG, "mbar_ctx_set_scan_centers: L must not be negative");
    if (c->scan_B < 1) return fail(c, MBAR_ERR_STATE, "mbar_ctx_set_scan_centers: no basis on this context (mbar_ctx_set_scan first)");
    const int64_t B = c->scan_B;
    for (int64_t x = 0; x < L * B; ++x)
        if (!std::isfinite(center[x])) return fail(c, MBAR_ERR_ARG, "mbar_ctx_set_scan_centers: the centres must be finite");
    // the centres of the harmonic terms, in ascending b, as the kernels keep them: [L][SCAN_MAX_H]
    std::vector<double> packed((size_t)L * SCAN_MAX_H, 0.0);
    for (int64_t l = 0; l < L; ++l) {
        int h = 0;
        for (int64_t b = 0; b < B; ++b)
            if ((c->scan_terms.mask >> b) & 1u) packed[(size_t)l * SCAN_MAX_H + h++] = center[l * B + b];
    }
    c->scan_center_L = 0;
    HIPCHK(c, c->scan_center.upload(packed.data(), packed.size()));
    c->scan_center_L = L;
    return MBAR_OK;
}

int mbar_scan_lognum(mbar_ctx* c, const double* f, int64_t L, const double* coeff, const double* offset, double* lognum, double* mean) {
    return whole_lognum(c, "mbar_scan_lognum", WholeObs{}, f, L, coeff, offset, lognum, mean);
}

int mbar_scan_gram_w(mbar_ctx* c, const double* f, int64_t L, const double* coeff, const double* offset, const double* f_scan, int64_t r,
                     double* cross, double* within, double* refcol, double* wsum) {
    return whole_gram_w(c, "mbar_scan_gram_w", WholeObs{}, f, L, coeff, offset, f_scan, r, cross, within, refcol, wsum);
}

// The members' own Gram block for the reference members rows[R]: one launch and one merge per (row panel, member panel), the row
// panels cut as scan_pair_nb_for says (a function of the reference members left and J alone), the member panels those of pass B.
int mbar_scan_pair_gram(mbar_ctx* c, const double* f, int64_t L, const double* coeff, const double* offset, const double* f_scan, int64_t R,
                        const int64_t* rows, double* pair) {
    bool ok = f && coeff && f_scan && rows && pair && L >= 1 && R >= 1;
    for (int64_t r = 0; ok && r < R; ++r) ok = rows[r] >= 0 && rows[r] < L;
    for (int64_t l = 0; ok && l < L; ++l) ok = std::isfinite(f_scan[l]);
    int rc = scan_open(c, "mbar_scan_pair_gram", ok, false, L);
    if (rc) return rc;
    const int64_t B = c->scan_B;
    const int J = 1 + (int)c->scan_Q;
    const int mb = scan_mb_of<ScanStored>(c, J);
    const int64_t pw = 64 * mb, nchunks = std::max<int64_t>((c->N + SCAN_CHUNK - 1) / SCAN_CHUNK, 1);
    const size_t out_doubles = (size_t)R * (size_t)L * (size_t)(J * J);
    bool done = false;
    ScanData d;
    // (the record of the widest row panel the call can meet; the reference members ride behind the other inputs in scan_in)
    rc = scan_begin(c, f, L, coeff, offset, nullptr, 0, {{pair, out_doubles}},
                    (size_t)nchunks * (size_t)scan_pair_record_doubles(scan_pair_nb_for(R, J), J, mb), out_doubles, &done, &d, (size_t)R);
    if (rc || done) return rc;
    const double* d_coeff = c->scan_in;
    const double* d_off = d_coeff + L * B;
    double* d_fscan = c->scan_in.p + L * (B + 1);
    static_assert(sizeof(int64_t) == sizeof(double), "the reference members ride in scan_in");
    int64_t* d_rows = reinterpret_cast<int64_t*>(c->scan_in.p + L * (B + 3));
    double* d_pair = c->scan_out;
    HIPCHK(c, hipMemcpyAsync(d_fscan, f_scan, (size_t)L * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_rows, rows, (size_t)R * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    {
        ScopedTimer timer(c, MBAR_TIMER_OTHER);
        for (int64_t r0 = 0; r0 < R;) {  // row panels: the widest while more than a narrow one's reference members are left
            const int nb = scan_pair_nb_for(R - r0, J);
            const int rm = (int)std::min<int64_t>(R - r0, scan_pair_rows(nb, J));
            for (int64_t p0 = 0; p0 < L; p0 += pw) {
                if (c->scan_terms.mask)
                    HIPCHK(c, launch_scan_pair(c->stream, d, harmonic_of(c), nb, L, p0, d_rows + r0, rm, d_coeff, d_off, d_fscan, c->scan_part));
                else
                    HIPCHK(c, launch_scan_pair(c->stream, d, ScanLinear{}, nb, L, p0, d_rows + r0, rm, d_coeff, d_off, d_fscan, c->scan_part));
                HIPCHK(c, launch_scan_pair_merge(c->stream, d, nb, mb, L, p0, rm, c->scan_part, d_pair + r0 * L * J * J));
            }
            r0 += rm;
        }
    }
    HIPCHK(c, hipMemcpyAsync(pair, d_pair, out_doubles * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return sync_stream(c);
}

int mbar_scan_energy_lognum(mbar_ctx* c, const double* f, int64_t L, const double* coeff, const double* offset, const double* center_u,
                            int64_t J, double* lognum, double* mean) {
    return whole_lognum(c, "mbar_scan_energy_lognum", WholeObs{true, center_u, J}, f, L, coeff, offset, lognum, mean);
}

int mbar_scan_energy_gram_w(mbar_ctx* c, const double* f, int64_t L, const double* coeff, const double* offset, const double* center_u,
                            int64_t J, const double* f_scan, int64_t r, double* cross, double* within, double* refblock, double* wsum) {
    return whole_gram_w(c, "mbar_scan_energy_gram_w", WholeObs{true, center_u, J}, f, L, coeff, offset, f_scan, r, cross, within, refblock, wsum);
}

int mbar_scan_moments(mbar_ctx* c, const double* f, int64_t L, const double* coeff, const double* offset, const double* center_phi,
                      double* lognum, double* mean, double* m1, double* m2, double* ma) {
    const char* who = "mbar_scan_moments";
    int rc = scan_open(c, who, f && coeff && lognum && mean && m1 && m2 && (ma || (c && c->scan_Q == 0)) && L >= 1, false, L);
    if (rc) return rc;
    const int B = (int)c->scan_B, Q = (int)c->scan_Q, J = 1 + Q;
    const int H = __builtin_popcount(c->scan_terms.mask), F = B + H, NT = F * (F + 1) / 2;
    if (center_phi)
        for (int64_t x = 0; x < L * F; ++x)
            if (!std::isfinite(center_phi[x])) return fail(c, MBAR_ERR_ARG, std::string(who) + ": the centres of the features must be finite");
    ScanMoments mom = scan_moments_bucket(B, H);
    const std::vector<int> slot = moment_slots(c->scan_terms, B, mom);
    const int FB = mom.slots(), R = mom.record(Q);
    const int64_t nchunks = std::max<int64_t>((c->N + SCAN_VCHUNK - 1) / SCAN_VCHUNK, 1);
    const MomentSizes z = moment_sizes(c->opt_scan_part_bytes, nchunks, R, L);
    bool done = false;
    ScanData d;
    rc = scan_begin(c, f, L, coeff, offset, nullptr, 0,
                    {{lognum, (size_t)L}, {mean, (size_t)(L * J)}, {m1, (size_t)(L * F)}, {m2, (size_t)(L * NT)}, {ma, (size_t)(L * Q * F)}},
                    std::max(z.part, (size_t)nchunks * (size_t)z.panel), z.out, &done, &d, (size_t)L * (size_t)FB);
    if (rc || done) return rc;
    double* d_M = c->scan_out;
    double* d_lognum = d_M + L;
    double* d_out = d_lognum + L;
    const double* d_coeff = c->scan_in;
    const double* d_off = d_coeff + L * B;
    double* d_cphi = c->scan_in.p + L * (B + 3);
    std::vector<double> packed((size_t)L * (size_t)FB, 0.0);
    if (center_phi)
        for (int64_t l = 0; l < L; ++l)
            for (int i = 0; i < F; ++i) packed[(size_t)(l * FB + slot[(size_t)i])] = center_phi[l * F + i];
    HIPCHK(c, hipMemcpyAsync(d_cphi, packed.data(), packed.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    mom.center_phi = d_cphi;
    const ScanWhole cut{};
    {
        ScopedTimer timer(c, MBAR_TIMER_OTHER);
        for (int64_t p0 = 0; p0 < L; p0 += z.panel) {
            const int64_t pl = std::min(z.panel, L - p0);
            HIPCHK(c, sweep_vec(c, d, cut, ScanStored{}, false, p0, pl, d_coeff + p0 * B, d_off + p0, nullptr, c->scan_part));
            HIPCHK(c, launch_scan_vec_merge(c->stream, d, cut, false, pl, c->scan_part, d_M + p0, nullptr, nullptr));
            if (c->scan_terms.mask)
                HIPCHK(c, launch_scan_moments(c->stream, d, harmonic_of(c).from(p0), mom.from(p0), pl, d_coeff + p0 * B, d_off + p0, d_M + p0, c->scan_part));
            else
                HIPCHK(c, launch_scan_moments(c->stream, d, ScanLinear{}, mom.from(p0), pl, d_coeff + p0 * B, d_off + p0, d_M + p0, c->scan_part));
            HIPCHK(c, launch_scan_moments_merge(c->stream, d, mom, pl, c->scan_part, d_M + p0, d_lognum + p0, d_out + p0 * R));
        }
    }
    std::vector<double> out((size_t)L * (size_t)R);
    HIPCHK(c, hipMemcpyAsync(lognum, d_lognum, (size_t)L * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(out.data(), d_out, out.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    rc = sync_stream(c);
    if (rc) return rc;
    for (int64_t l = 0; l < L; ++l)
        moment_outputs(out.data() + l * R, Q, mom, slot, mean + l * J, m1 + l * F, m2 + l * NT, ma ? ma + l * Q * F : nullptr);
    return MBAR_OK;
}

// ---- many observables along a scan ----

int mbar_ctx_set_scan_obs(mbar_ctx* c, int64_t Q, const double* a_host, int64_t ld_host) {
    const char* who = "mbar_ctx_set_scan_obs";
    int rc = scan_ready(c, who);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (Q == 0) {
        c->scan_obs_Q = 0;
        c->scan_obs.reset();
        return MBAR_OK;
    }
    const int64_t N = c->N, ld = c->ld;
    if (Q < 0 || !a_host || ld_host < N) return fail(c, MBAR_ERR_ARG, std::string(who) + ": Q >= 0 rows of N doubles at a pitch of at least N");
    for (int64_t q = 0; q < Q; ++q)
        for (int64_t n = 0; n < N; ++n)
            if (!std::isfinite(a_host[q * ld_host + n])) return fail(c, MBAR_ERR_ARG, std::string(who) + ": the observables must be finite");
    c->scan_obs_Q = 0;
    HIPCHK(c, c->scan_obs.grow((size_t)Q * (size_t)ld));
    HIPCHK(c, hipMemset(c->scan_obs, 0, (size_t)Q * (size_t)ld * sizeof(double)));
    HIPCHK(c, hipMemcpy2D(c->scan_obs, (size_t)ld * sizeof(double), a_host, (size_t)ld_host * sizeof(double), (size_t)N * sizeof(double), (size_t)Q,
                          hipMemcpyHostToDevice));
    c->scan_obs_Q = Q;
    return MBAR_OK;
}

// One launch and one merge per (mode, member panel, observable panel): the member panels are those of pass B at the mode's operand
// columns, the observable panels 128 rows (the last one the narrowest instantiation that holds it).
int mbar_scan_obs_sums(mbar_ctx* c, const double* f, int64_t L, const double* coeff, const double* offset, const double* f_scan, double* s1,
                       double* t1, double* t2, double* wsum, double* w2sum) {
    const char* who = "mbar_scan_obs_sums";
    const bool second = t1 || t2 || w2sum;
    int rc = scan_open(c, who, f && coeff && f_scan && s1 && wsum && L >= 1 && (!second || (t1 && t2 && w2sum)), false, L);
    if (rc) return rc;
    if (c->scan_obs_Q < 1) return fail(c, MBAR_ERR_STATE, std::string(who) + ": no observables on this context (mbar_ctx_set_scan_obs first)");
    const int64_t B = c->scan_B, Q = c->scan_obs_Q, ld = c->ld;
    const size_t LQ = (size_t)L * (size_t)Q;
    constexpr int64_t QP = 128;  // observables of a panel: one tile of the widest instantiation
    const int64_t nchunks = std::max<int64_t>((c->N + SCAN_CHUNK - 1) / SCAN_CHUNK, 1);
    const int nb_max = scan_nb_for(std::min(Q, QP));
    int64_t record = 0;
    for (int mode = second ? 1 : 0; mode <= (second ? 2 : 0); ++mode) {
        const int J = scan_obs_columns(mode);
        record = std::max(record, scan_obs_record_doubles(nb_max, J, scan_mb_of<ScanStored>(c, J)));
    }
    bool done = false;
    ScanData d;
    rc = scan_begin(c, f, L, coeff, offset, f_scan, (size_t)L, {{s1, LQ}, {t1, LQ}, {t2, LQ}, {wsum, (size_t)L}, {w2sum, (size_t)L}},
                    (size_t)nchunks * (size_t)record, 3 * LQ + 2 * (size_t)L, &done, &d);
    if (rc || done) return rc;
    double* d_s1 = c->scan_out;
    double* d_t1 = d_s1 + LQ;
    double* d_t2 = d_t1 + LQ;
    double* d_wsum = d_t2 + LQ;
    double* d_w2sum = d_wsum + L;
    const double* d_coeff = c->scan_in;
    const double* d_off = d_coeff + L * B;
    double* d_fscan = c->scan_in.p + L * (B + 1);
    HIPCHK(c, hipMemcpyAsync(d_fscan, f_scan, (size_t)L * sizeof(double), hipMemcpyHostToDevice, c->stream));
    {
        ScopedTimer timer(c, MBAR_TIMER_OTHER);
        for (int mode = second ? 1 : 0; mode <= (second ? 2 : 0); ++mode) {
            const int mb = scan_mb_of<ScanStored>(c, scan_obs_columns(mode));
            double* out0 = mode == 2 ? d_t2 : d_s1;
            double* out1 = mode == 1 ? d_t1 : nullptr;
            for (int64_t p0 = 0; p0 < L; p0 += 64 * mb)
                for (int64_t qb = 0; qb < Q; qb += QP) {
                    const int64_t nq = std::min(QP, Q - qb);
                    const int nb = scan_nb_for(nq);
                    const double* a = c->scan_obs.p + qb * ld;
                    if (c->scan_terms.mask)
                        HIPCHK(c, launch_scan_obs(c->stream, d, harmonic_of(c), nb, mode, a, nq, L, p0, d_coeff, d_off, d_fscan, c->scan_part));
                    else
                        HIPCHK(c, launch_scan_obs(c->stream, d, ScanLinear{}, nb, mode, a, nq, L, p0, d_coeff, d_off, d_fscan, c->scan_part));
                    const bool vec = qb == 0 && mode != 2;  // wsum and w2sum: the first observable panel's
                    HIPCHK(c, launch_scan_obs_merge(c->stream, d, nb, mode, mb, L, Q, p0, qb, nq, c->scan_part, out0, out1, vec ? d_wsum : nullptr,
                                                    vec && second ? d_w2sum : nullptr));
                }
        }
    }
    HIPCHK(c, hipMemcpyAsync(s1, d_s1, LQ * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(wsum, d_wsum, (size_t)L * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (second) {
        HIPCHK(c, hipMemcpyAsync(t1, d_t1, LQ * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(t2, d_t2, LQ * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(w2sum, d_w2sum, (size_t)L * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    return sync_stream(c);
}

// ---- kernel-density surfaces along a scan ----

int mbar_ctx_set_scan_points(mbar_ctx* c, int64_t d, const double* x_host, int64_t ld_host) {
    const char* who = "mbar_ctx_set_scan_points";
    int rc = scan_ready(c, who);
    if (rc) return rc;
    const int64_t N = c->N, ld = c->ld;
    // (refused before the block is touched)
    if (d < 0 || d > SCANKDE_MAX_D || (d > 0 && (!x_host || ld_host < N)))
        return fail(c, MBAR_ERR_ARG, std::string(who) + ": d = 0, 1 or 2 rows of N doubles at a pitch of at least N");
    for (int64_t k = 0; k < d; ++k)
        for (int64_t n = 0; n < N; ++n)
            if (!std::isfinite(x_host[k * ld_host + n])) return fail(c, MBAR_ERR_ARG, std::string(who) + ": the points must be finite");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->scan_pts_d = 0;
    if (d == 0) {
        c->scan_pts.reset();
        return MBAR_OK;
    }
    HIPCHK(c, c->scan_pts.grow((size_t)d * (size_t)ld));
    HIPCHK(c, hipMemset(c->scan_pts, 0, (size_t)d * (size_t)ld * sizeof(double)));
    HIPCHK(c, hipMemcpy2D(c->scan_pts, (size_t)ld * sizeof(double), x_host, (size_t)ld_host * sizeof(double), (size_t)N * sizeof(double), (size_t)d,
                          hipMemcpyHostToDevice));
    c->scan_pts_d = d;
    return MBAR_OK;
}

// One launch and one merge per (member panel, query panel): the member panels are those of mbar_scan_obs_sums' first moments, the
// query panels 128 queries (the last one the narrowest instantiation that holds it).  Then the pairs the merge left as NaN, of
// members with weight, in batches of KDE_EXACT_BATCH through the exact kernel.
int mbar_scan_kde_sums(mbar_ctx* c, const double* f, int64_t L, const double* coeff, const double* offset, const double* f_scan, int64_t M,
                       const double* q, double bandwidth, const double* period, double* logsum, double* wsum, int64_t* n_exact) {
    const char* who = "mbar_scan_kde_sums";
    int rc = scan_open(c, who, f && coeff && f_scan && q && logsum && wsum && n_exact && L >= 1 && M >= 1, false, L);
    if (rc) return rc;
    if (c->scan_pts_d < 1) return fail(c, MBAR_ERR_STATE, std::string(who) + ": no points on this context (mbar_ctx_set_scan_points first)");
    const int dim = (int)c->scan_pts_d;
    const double inv2h2 = 0.5 / (bandwidth * bandwidth);
    if (!(bandwidth > 0.0) || !std::isfinite(bandwidth) || !std::isfinite(inv2h2) || !(inv2h2 > 0.0))
        return fail(c, MBAR_ERR_ARG, std::string(who) + ": the bandwidth must be positive and finite, and so must 1 / 2h^2");
    for (int64_t x = 0; x < (int64_t)dim * M; ++x)
        if (!std::isfinite(q[x])) return fail(c, MBAR_ERR_ARG, std::string(who) + ": the queries must be finite");
    for (int k = 0; period && k < dim; ++k)
        if (!(period[k] >= 0.0) || !std::isfinite(period[k])) return fail(c, MBAR_ERR_ARG, std::string(who) + ": a period is 0 (none) or positive and finite");
    *n_exact = 0;
    const int64_t B = c->scan_B;
    const size_t LM = (size_t)L * (size_t)M;
    constexpr int64_t QP = 128;                  // queries of a panel: one tile of the widest instantiation
    constexpr int64_t KDE_EXACT_BATCH = 1 << 16;  // pairs of one launch of the exact kernel
    const int64_t nchunks = std::max<int64_t>((c->N + SCAN_CHUNK - 1) / SCAN_CHUNK, 1);
    const int mb = scan_mb_of<ScanStored>(c, 1);
    const int64_t record = scan_kde_record_doubles(scan_nb_for(std::min(M, QP)), mb);
    const size_t batch = (size_t)std::min<int64_t>(KDE_EXACT_BATCH, (int64_t)LM);
    bool done = false;
    ScanData d;
    // out: logsum | wsum | the exact kernel's results | its pairs (two int64 each); in, behind the members': the queries
    rc = scan_begin(c, f, L, coeff, offset, f_scan, (size_t)L, {{logsum, LM}, {wsum, (size_t)L}}, (size_t)nchunks * (size_t)record,
                    LM + (size_t)L + 3 * batch, &done, &d, (size_t)dim * (size_t)M);
    if (rc || done) return rc;
    double* d_logsum = c->scan_out;
    double* d_wsum = d_logsum + LM;
    double* d_exact = d_wsum + L;
    int64_t* d_pairs = reinterpret_cast<int64_t*>(d_exact + batch);
    const double* d_coeff = c->scan_in;
    const double* d_off = d_coeff + L * B;
    double* d_fscan = c->scan_in.p + L * (B + 1);
    double* d_q = c->scan_in.p + L * (B + 3);
    HIPCHK(c, hipMemcpyAsync(d_fscan, f_scan, (size_t)L * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(d_q, q, (size_t)dim * (size_t)M * sizeof(double), hipMemcpyHostToDevice, c->stream));
    const ScanKde kd = scan_kde_make(dim, c->scan_pts, d_q, M, M, bandwidth, period);
    {
        ScopedTimer timer(c, MBAR_TIMER_OTHER);
        for (int64_t p0 = 0; p0 < L; p0 += 64 * mb)
            for (int64_t qb = 0; qb < M; qb += QP) {
                const int64_t nq = std::min(QP, M - qb);
                const int nb = scan_nb_for(nq);
                if (c->scan_terms.mask)
                    HIPCHK(c, launch_scan_kde(c->stream, d, harmonic_of(c), kd, nb, qb, nq, L, p0, d_coeff, d_off, d_fscan, c->scan_part));
                else
                    HIPCHK(c, launch_scan_kde(c->stream, d, ScanLinear{}, kd, nb, qb, nq, L, p0, d_coeff, d_off, d_fscan, c->scan_part));
                HIPCHK(c, launch_scan_kde_merge(c->stream, d, kd, nb, mb, L, p0, qb, nq, c->scan_part, d_logsum, qb == 0 ? d_wsum : nullptr));
            }
    }
    HIPCHK(c, hipMemcpyAsync(logsum, d_logsum, LM * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(wsum, d_wsum, (size_t)L * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    rc = sync_stream(c);
    if (rc) return rc;
    // ---- the exact path: a NaN of a member with weight
    std::vector<int64_t> pairs;
    for (int64_t l = 0; l < L; ++l) {
        if (!(wsum[l] > 0.0)) continue;
        for (int64_t m = 0; m < M; ++m)
            if (std::isnan(logsum[l * M + m])) {
                pairs.push_back(l);
                pairs.push_back(m);
            }
    }
    const int64_t npairs = (int64_t)pairs.size() / 2;
    std::vector<double> exact(npairs > 0 ? batch : 0);
    for (int64_t i0 = 0; i0 < npairs; i0 += (int64_t)batch) {
        const int64_t nb = std::min<int64_t>((int64_t)batch, npairs - i0);
        HIPCHK(c, hipMemcpyAsync(d_pairs, pairs.data() + 2 * i0, (size_t)nb * 2 * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
        {
            ScopedTimer timer(c, MBAR_TIMER_OTHER);
            if (c->scan_terms.mask)
                HIPCHK(c, launch_scan_kde_exact(c->stream, d, harmonic_of(c), kd, nb, d_pairs, d_coeff, d_off, d_fscan, d_exact));
            else
                HIPCHK(c, launch_scan_kde_exact(c->stream, d, ScanLinear{}, kd, nb, d_pairs, d_coeff, d_off, d_fscan, d_exact));
        }
        HIPCHK(c, hipMemcpyAsync(exact.data(), d_exact, (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        rc = sync_stream(c);
        if (rc) return rc;
        for (int64_t i = 0; i < nb; ++i) logsum[pairs[2 * (i0 + i)] * M + pairs[2 * (i0 + i) + 1]] = exact[i];
    }
    *n_exact = npairs;
    return MBAR_OK;
}

// ---- histogram surfaces along a scan ----

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
    int rc = scan_open(c, "mbar_scan_bin_lognum", f && coeff && lognum && L >= 1, true, L);
    if (rc) return rc;
    const int64_t B = c->scan_B, nbins = c->scanbin_nbins;
    bool done = false;
    ScanData d;
    const ScanBinned cut = binned_of(c, false);
    const int64_t nch = std::max<int64_t>(cut.t.nchunks, 1);
    const int64_t pw = vec_panel(c, nch, 1, L);
    rc = scan_begin(c, f, L, coeff, offset, nullptr, 0, {{lognum, (size_t)L * nbins}}, (size_t)nch * (size_t)pw,
                    (size_t)L * (size_t)nbins + (size_t)nbins * (size_t)pw, &done, &d);
    if (rc || done) return rc;
    double* d_lognum = c->scan_out;
    double* d_M = d_lognum + L * nbins;  // [bin][member of the panel]
    const double* d_coeff = c->scan_in;
    const double* d_off = d_coeff + L * B;
    {
        ScopedTimer timer(c, MBAR_TIMER_OTHER);
        for (int64_t p0 = 0; p0 < L; p0 += pw) {
            const int64_t pl = std::min(pw, L - p0);
            HIPCHK(c, sweep_vec(c, d, cut, ScanStored{}, false, p0, pl, d_coeff + p0 * B, d_off + p0, nullptr, c->scan_part));
            HIPCHK(c, launch_scan_vec_merge(c->stream, d, cut, false, pl, c->scan_part, d_M, nullptr, nullptr));
            HIPCHK(c, sweep_vec(c, d, cut, ScanStored{}, true, p0, pl, d_coeff + p0 * B, d_off + p0, d_M, c->scan_part));
            HIPCHK(c, launch_scan_vec_merge(c->stream, d, cut, true, pl, c->scan_part, d_M, d_lognum + p0 * nbins, nullptr));
        }
    }
    HIPCHK(c, hipMemcpyAsync(lognum, d_lognum, (size_t)L * nbins * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return sync_stream(c);
}

int mbar_scan_bin_gram_w(mbar_ctx* c, const double* f, int64_t L, const double* coeff, const double* offset, const double* f_bins,
                         double* cross, double* diag, double* wsum) {
    int rc = scan_open(c, "mbar_scan_bin_gram_w", f && coeff && f_bins && diag && wsum && L >= 1, true, L);
    if (rc) return rc;
    const int64_t B = c->scan_B, K = c->K, nbins = c->scanbin_nbins;
    const size_t LB = (size_t)L * (size_t)nbins;
    bool done = false;
    ScanData d;
    ScanBinned cut = binned_of(c, true);
    const int nb = cross ? scan_nb_for(K) : 0;
    // groups of whole bins whose records fit the budget ("scan_part_bytes"; a single bin is never split): one sweep per group, and
    // a (member, bin)'s sums do not depend on the cut
    const int mb = scan_mb_of<ScanStored>(c, 1);
    const int64_t rec = scan_record_doubles(nb, 1, SCANBIN_NV, mb);
    const int64_t max_chunks = std::max<int64_t>(c->opt_scan_part_bytes / (rec * (int64_t)sizeof(double)), 1);
    const std::vector<int64_t>& c0 = c->scanbin_c0_b_host;
    std::vector<int64_t> group{0};  // first bin of every group, then nbins
    for (int64_t i = 1; i < nbins; ++i)
        if (c0[(size_t)i + 1] - c0[(size_t)group.back()] > max_chunks) group.push_back(i);
    group.push_back(nbins);
    int64_t worst = 1;
    for (size_t g = 0; g + 1 < group.size(); ++g) worst = std::max(worst, c0[(size_t)group[g + 1]] - c0[(size_t)group[g]]);
    HIPCHK(c, c->scanbin_fbins.grow(LB));  // (the stream is idle here)
    rc = scan_begin(c, f, L, coeff, offset, f_bins, LB, {{cross, (size_t)K * LB}, {diag, LB}, {wsum, LB}}, (size_t)worst * (size_t)rec,
                    LB * SCANBIN_NV + (cross ? (size_t)K * LB : 0), &done, &d);
    if (rc || done) return rc;
    HIPCHK(c, hipMemcpyAsync(c->scanbin_fbins, f_bins, LB * sizeof(double), hipMemcpyHostToDevice, c->stream));
    double* d_vec = c->scan_out;
    double* d_cross = d_vec + LB * SCANBIN_NV;
    const double* d_coeff = c->scan_in;
    const double* d_off = d_coeff + L * B;
    const int64_t pw = 64 * mb;
    HIPCHK(c, hipMemcpyAsync(d_f(c), f, (size_t)K * sizeof(double), hipMemcpyHostToDevice, c->stream));
    {
        ScopedTimer timer(c, MBAR_TIMER_OTHER);
        for (size_t g = 0; g + 1 < group.size(); ++g) {
            cut.b0_ = group[g], cut.b1_ = group[g + 1];
            cut.c0_ = c0[(size_t)cut.b0_], cut.c1_ = c0[(size_t)cut.b1_];
            for (int64_t p0 = 0; p0 < L; p0 += pw) {  // the group's samples of the resident matrix are read once per panel
                HIPCHK(c, sweep_cross(c, d, cut, ScanStored{}, nb, L, p0, d_coeff, d_off, c->scanbin_fbins.p));
                HIPCHK(c, (launch_scan_cross_merge<ScanBinned, ScanStored>(c->stream, d, cut, nb, mb, K, L, p0, c->scan_part, d_cross, d_vec)));
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
