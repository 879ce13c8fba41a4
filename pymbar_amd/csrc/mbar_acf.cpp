// Host side of the lagged fluctuation sums (include/mbar_hip.h, "timeseries"): the mbar_acf handle (on the handle layer of
// mbar_handle.h), which keeps one series (or the concatenation of K segments) resident on a device with its suffix sums, the lag
// schedule of the reference's stopping rule and the raw lag sums.  Kernels: mbar_k_acf.hip.
#include <cmath>

#include "mbar_handle.h"
#include "mbar_acf.h"

using namespace mbar;
using namespace mbar::host;

struct mbar_acf : Handle {
    int kind = ACF_AUTO, nacc = 1;
    int64_t T = 0, ldx = 0, ntiles = 0, K = 1;
    int64_t last_change = -1;           // last n with A_n != A_n+1 (or B_n != B_n+1): suffixes from s > last_change are constant
    std::vector<int64_t> seg;           // segment lengths
    DevBuf<double2> A;                  // [ldx] A - shift_a as hi + lo (exact)
    DevBuf<double2> b_own;              // [ldx] B - shift_b (cross-correlation only)
    DevBuf<int> rem;                    // [ldx]
    DevBuf<double2> SA;                 // [ldx] suffix sums of A'
    DevBuf<double2> sb_own;             // [ldx] suffix sums of B' (cross-correlation only)
    DevBuf<double2> tot, off;           // [ACF_MAX_LAGS][nacc][ntiles]
    DevBuf<int> active;                 // [ntiles]
    DevBuf<int> oid;                    // [ldx]
    // rule state, one entry per origin (grown on demand)
    DevBuf<double> g, sig2;
    DevBuf<double2> dA, dB;
    DevBuf<int> status;
    DevBuf<int64_t> stop;
    DevBuf<double> ct;
    DevBuf<double2> q;
    DevBuf<int64_t> orig;
    DevBuf<double> xab, xba;
    // B and its suffix sums: A's for the autocorrelation
    double2* B() const { return b_own ? b_own : A; }
    double2* SB() const { return sb_own ? sb_own : SA; }
};

namespace {

AcfLaunch base_launch(const mbar_acf* h) {
    AcfLaunch a{};
    a.kind = h->kind;
    a.nacc = h->nacc;
    a.A = h->A;
    a.B = h->B();
    a.rem = h->rem;
    a.T = h->T;
    a.ldx = h->ldx;
    a.ntiles = h->ntiles;
    a.tot = h->tot;
    a.off = h->off;
    return a;
}

// tiles that hold a product of lags >= tmin: positions n < T - tmin
int64_t last_product_tile(const mbar_acf* h, int64_t tmin) {
    if (tmin > h->T - 1) return -1;
    return (h->T - 1 - tmin) / ACF_TILE;
}

// the number of (n, n + t) pairs inside one segment
double valid_pairs(const mbar_acf* h, int64_t t) {
    double d = 0.0;
    for (int64_t n : h->seg)
        if (t < n) d += (double)(n - t);
    return d;
}

// The reference's lag schedule.  Entry 0 is lag 0 (the variance step of the rule), then t = 1, 2, 3, ... or (fast) 1, 2, 4, 7, 11, ...;
// inc is the increment the rule weights entry k with and adds to t.
struct Schedule {
    bool fast;
    int64_t k = 0, t = 0, inc = 0;
    void next() {
        if (k == 0) {
            t = 1;
            inc = 1;
        } else {
            t += inc;
            if (fast) ++inc;
        }
        ++k;
    }
};

// entries of the schedule with a lag below tmax (lag 0 included)
int64_t schedule_entries(bool fast, int64_t tmax) {
    Schedule sch{fast};
    int64_t n = 0;
    while (sch.k == 0 || sch.t < tmax) {
        ++n;
        sch.next();
    }
    return n;
}

// Runs the stopping rule: origins o * nskip (o < norig) of one series, or the single origin of the K-segment form.  The host only
// reads the running origins per tile between lag blocks (8, 16, 32, then 64 lags).
int run_rule(mbar_acf* h, int mode, int64_t nskip, int64_t norig, int fast, int64_t mintime, int fft, bool record_ct) {
    HIPCHK(nullptr, hipSetDevice(h->device));
    const size_t n = (size_t)norig;
    HIPCHK(nullptr, h->g.grow(n));
    HIPCHK(nullptr, h->sig2.grow(n));
    HIPCHK(nullptr, h->dA.grow(n));
    HIPCHK(nullptr, h->dB.grow(n));
    HIPCHK(nullptr, h->status.grow(n));
    HIPCHK(nullptr, h->stop.grow(n));
    int64_t maxN = 0;
    for (int64_t L : h->seg) maxN = std::max(maxN, L);
    // every origin's lags stay below its end: T - s for the suffix form (fft: <= T - s - 1), max N_k - 1 for the segments
    const int64_t tmax = mode == ACF_RULE_SUFFIX ? h->T : maxN;
    if (record_ct) HIPCHK(nullptr, h->ct.grow((size_t)schedule_entries(fast != 0, tmax)));
    AcfRule ru{};
    ru.mode = mode;
    ru.fft = fft;
    ru.nskip = nskip;
    ru.norig = norig;
    ru.mintime = mintime;
    ru.navg = (double)h->T / (double)h->seg.size();
    ru.tend = maxN - 1;
    ru.SA = h->SA;
    ru.SB = h->SB();
    ru.g = h->g;
    ru.sig2 = h->sig2;
    ru.dA = h->dA;
    ru.dB = h->dB;
    ru.status = h->status;
    ru.stop = h->stop;
    ru.ct = record_ct ? h->ct : nullptr;
    ru.active = h->active;
    HIPCHK(nullptr, launch_acf_rule_init(h->stream, ru, h->T, mode == ACF_RULE_SUFFIX ? h->last_change : h->T));
    int64_t c_lo = 0, c_hi = ((norig - 1) * nskip) / ACF_TILE;
    Schedule sch{fast != 0};
    int width = 8;
    std::vector<int> act;
    while (true) {
        AcfLaunch a = base_launch(h);
        a.kbase = sch.k;
        a.nl = 0;
        while (a.nl < width && (sch.k == 0 || sch.t < tmax)) {
            a.lag[a.nl] = sch.t;
            a.inc[a.nl] = sch.inc;
            a.den[a.nl] = sch.k == 0 ? (double)h->T : valid_pairs(h, sch.t);
            ++a.nl;
            sch.next();
        }
        if (a.nl == 0) return fail(nullptr, MBAR_ERR_NUMERIC, "the lag schedule ended with running origins");
        a.tile_lo = c_lo;
        a.atile_hi = std::min(h->ntiles - 1, last_product_tile(h, a.lag[0]));
        HIPCHK(nullptr, launch_acf_tiles(h->stream, a));
        HIPCHK(nullptr, launch_acf_scan(h->stream, a));
        HIPCHK(nullptr, launch_acf_rule(h->stream, a, ru, c_lo, c_hi));
        act.resize((size_t)(c_hi - c_lo + 1));
        HIPCHK(nullptr, hipMemcpyAsync(act.data(), h->active + c_lo, act.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(nullptr, hipStreamSynchronize(h->stream));
        int64_t lo = -1, hi = -1;
        for (size_t i = 0; i < act.size(); ++i)
            if (act[i] > 0) {
                if (lo < 0) lo = c_lo + (int64_t)i;
                hi = c_lo + (int64_t)i;
            }
        if (lo < 0) break;
        c_lo = lo;
        c_hi = hi;
        width = std::min(ACF_MAX_LAGS, width * 2);
    }
    return MBAR_OK;
}

int copy_rule(mbar_acf* h, int64_t norig, double* g, int64_t* stop, int32_t* status) {
    HIPCHK(nullptr, hipMemcpyAsync(g, h->g, norig * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (stop) HIPCHK(nullptr, hipMemcpyAsync(stop, h->stop, norig * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    if (status) HIPCHK(nullptr, hipMemcpyAsync(status, h->status, norig * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(nullptr, hipStreamSynchronize(h->stream));
    return MBAR_OK;
}

}  // namespace

extern "C" {

int mbar_acf_create(mbar_acf** out, int device, int64_t T, const double* a, const double* b, int64_t K, const int64_t* seg,
                    double shift_a, double shift_b) {
    if (!out) return bad_arg("out is NULL");
    *out = nullptr;
    if (T < 1 || !a) return bad_arg("need at least one value");
    if (T >= ((int64_t)1 << 31) - ACF_TILE) return bad_arg("series longer than 2^31 - 2^12 values");
    if (K < 1 || !seg) return bad_arg("need at least one segment");
    int64_t sum = 0;
    for (int64_t k = 0; k < K; ++k) {
        if (seg[k] < 1) return bad_arg("segment lengths must be positive");
        sum += seg[k];
    }
    if (sum != T) return bad_arg("segment lengths must add up to T");
    if (!std::isfinite(shift_a) || !std::isfinite(shift_b)) return bad_arg("shifts must be finite");
    for (int64_t i = 0; i < T; ++i)
        if (!std::isfinite(a[i]) || (b && !std::isfinite(b[i]))) return bad_arg("the series must be finite");
    return create_handle(out, device, [&](mbar_acf* h, const DevInfo&) {
        h->kind = b ? ACF_CROSS : ACF_AUTO;
        h->nacc = b ? 2 : 1;
        h->T = T;
        h->K = K;
        h->seg.assign(seg, seg + K);
        h->ldx = (T / ACF_TILE + 1) * ACF_TILE;  // (> T: position T exists and holds zeros)
        h->ntiles = h->ldx / ACF_TILE;
        for (int64_t i = 0; i + 1 < T; ++i)
            if (a[i] != a[i + 1] || (b && b[i] != b[i + 1])) h->last_change = i;
        const size_t ldx = (size_t)h->ldx;
        HIPCHK(nullptr, h->SA.grow(ldx));
        HIPCHK(nullptr, h->tot.grow((size_t)ACF_MAX_LAGS * 2 * h->ntiles));
        HIPCHK(nullptr, h->off.grow((size_t)ACF_MAX_LAGS * 2 * h->ntiles));
        HIPCHK(nullptr, h->active.grow((size_t)h->ntiles));
        HIPCHK(nullptr, h->oid.grow(ldx));
        if (b) HIPCHK(nullptr, h->sb_own.grow(ldx));
        // x - shift exactly, as the rounded difference and its error (TwoSum)
        std::vector<double2> stage(ldx, double2{0.0, 0.0});
        auto shifted = [&](const double* x, double m) {
            for (int64_t i = 0; i < T; ++i) {
                const double s = x[i] - m, bb = s - x[i];
                stage[i] = double2{s, (x[i] - (s - bb)) + (-m - bb)};
            }
        };
        shifted(a, shift_a);
        HIPCHK(nullptr, h->A.upload(stage.data(), ldx));
        if (b) {
            shifted(b, shift_b);
            HIPCHK(nullptr, h->b_own.upload(stage.data(), ldx));
        }
        std::vector<int> rem(ldx, 0);
        int64_t pos = 0;
        for (int64_t k = 0; k < K; ++k)
            for (int64_t i = 0; i < seg[k]; ++i, ++pos) rem[pos] = (int)(seg[k] - i);
        HIPCHK(nullptr, h->rem.upload(rem.data(), ldx));
        HIPCHK(nullptr, hipMemset(h->active, 0, (size_t)h->ntiles * sizeof(int)));
        // suffix sums of A' (and B'): the plain term at lag 0 over every tile, stored at every position
        for (int which = 0; which < (b ? 2 : 1); ++which) {
            AcfLaunch l = base_launch(h);
            l.kind = ACF_PLAIN;
            l.nacc = 1;
            l.A = which ? h->B() : h->A;
            l.nl = 1;
            l.lag[0] = 0;
            l.tile_lo = 0;
            l.atile_hi = h->ntiles - 1;
            HIPCHK(nullptr, launch_acf_tiles(h->stream, l));
            HIPCHK(nullptr, launch_acf_scan(h->stream, l));
            HIPCHK(nullptr, launch_acf_store(h->stream, l, 0, h->ntiles - 1, nullptr, which ? h->SB() : h->SA, h->ldx));
        }
        HIPCHK(nullptr, hipStreamSynchronize(h->stream));
        return MBAR_OK;
    });
}

void mbar_acf_destroy(mbar_acf* h) { destroy_handle(h); }

int mbar_acf_suffix_g(mbar_acf* h, int64_t nskip, int fast, int64_t mintime, int fft, double* g, int64_t* stop, int32_t* status) {
    if (!h) return bad_arg("acf is NULL");
    if (h->K != 1) return bad_arg("suffix origins need one segment");
    if (nskip < 1) return bad_arg("nskip must be >= 1");
    if (h->T < 2) return bad_arg("need at least two values");
    if (!g) return bad_arg("g is NULL");
    const int64_t norig = (h->T - 2) / nskip + 1;  // origins 0, nskip, ... < T - 1
    int rc = run_rule(h, ACF_RULE_SUFFIX, nskip, norig, fft ? 0 : fast, mintime, fft, false);
    if (rc) return rc;
    return copy_rule(h, norig, g, stop, status);
}

int mbar_acf_multiple_g(mbar_acf* h, int fast, int64_t mintime, double* g, int64_t* stop, int32_t* status, int64_t ct_cap,
                        double* ct) {
    if (!h) return bad_arg("acf is NULL");
    if (h->kind != ACF_AUTO) return bad_arg("the multiple form is an autocorrelation");
    if (!g) return bad_arg("g is NULL");
    int64_t maxN = 0;
    for (int64_t L : h->seg) maxN = std::max(maxN, L);
    const int64_t entries = schedule_entries(fast != 0, maxN);
    if (ct && ct_cap < entries) return bad_arg("ct_cap is below mbar_acf_schedule_length");
    int rc = run_rule(h, ACF_RULE_MULTIPLE, h->T, 1, fast, mintime, 0, ct != nullptr);
    if (rc) return rc;
    rc = copy_rule(h, 1, g, stop, status);
    if (rc) return rc;
    if (ct) HIPCHK(nullptr, hipMemcpy(ct, h->ct, entries * sizeof(double), hipMemcpyDeviceToHost));
    return MBAR_OK;
}

int mbar_acf_schedule_length(int fast, int64_t tmax, int64_t* out) {
    if (!out) return bad_arg("out is NULL");
    *out = schedule_entries(fast != 0, tmax);
    return MBAR_OK;
}

int mbar_acf_lag_sums(mbar_acf* h, int64_t nlags, const int64_t* lags, int64_t norig, const int64_t* origins, int segments,
                      double* xab, double* xba) {
    if (!h) return bad_arg("acf is NULL");
    if (nlags < 0 || norig < 1 || !origins || (nlags > 0 && (!lags || !xab))) return bad_arg("bad arguments");
    if (!segments && h->K != 1) return bad_arg("suffix sums need one segment");
    for (int64_t i = 0; i < nlags; ++i)
        if (lags[i] < 0) return bad_arg("lags must be >= 0");
    for (int64_t i = 0; i < norig; ++i)
        if (origins[i] < 0 || origins[i] >= h->T || (i > 0 && origins[i] <= origins[i - 1]))
            return bad_arg("origins must be increasing positions of the series");
    if (nlags == 0) return MBAR_OK;
    HIPCHK(nullptr, hipSetDevice(h->device));
    // positions whose suffix sums are stored: the origins and T (segment mode: the end of the last range)
    std::vector<int64_t> pos(origins, origins + norig);
    pos.push_back(h->T);
    HIPCHK(nullptr, h->orig.upload(pos.data(), pos.size()));
    HIPCHK(nullptr, launch_acf_fill_int(h->stream, h->oid, h->ldx, -1));
    HIPCHK(nullptr, launch_acf_scatter_oid(h->stream, h->oid, h->orig, (int64_t)pos.size()));
    const int64_t ldo = norig + 1;
    HIPCHK(nullptr, h->q.grow((size_t)ACF_MAX_LAGS * h->nacc * ldo));
    HIPCHK(nullptr, h->xab.grow((size_t)nlags * norig));
    HIPCHK(nullptr, h->xba.grow((size_t)nlags * norig));
    const int64_t c_lo = origins[0] / ACF_TILE, c_hi = h->T / ACF_TILE;
    for (int64_t j0 = 0; j0 < nlags; j0 += ACF_MAX_LAGS) {
        AcfLaunch a = base_launch(h);
        a.nl = (int)std::min<int64_t>(ACF_MAX_LAGS, nlags - j0);
        int64_t tmin = lags[j0];
        for (int j = 0; j < a.nl; ++j) {
            a.lag[j] = lags[j0 + j];
            tmin = std::min(tmin, a.lag[j]);
        }
        a.tile_lo = c_lo;
        a.atile_hi = std::min(h->ntiles - 1, last_product_tile(h, tmin));
        HIPCHK(nullptr, launch_acf_tiles(h->stream, a));
        HIPCHK(nullptr, launch_acf_scan(h->stream, a));
        HIPCHK(nullptr, launch_acf_store(h->stream, a, c_lo, c_hi, h->oid, h->q, ldo));
        HIPCHK(nullptr, launch_acf_finish(h->stream, a, h->q, norig, h->orig, segments, h->SA, h->SB(), h->xab, h->xba, j0));
    }
    HIPCHK(nullptr, hipMemcpyAsync(xab, h->xab, (size_t)nlags * norig * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (xba) HIPCHK(nullptr, hipMemcpyAsync(xba, h->xba, (size_t)nlags * norig * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(nullptr, hipStreamSynchronize(h->stream));
    return MBAR_OK;
}

}  // extern "C"
