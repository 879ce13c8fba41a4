// Host side of the lagged fluctuation sums (include/mbar_hip.h, "timeseries"): the mbar_acf handle, which keeps one series (or
// the concatenation of K segments) resident on a device with its suffix sums, the lag schedule of the reference's stopping rule
// and the raw lag sums.  Kernels: mbar_k_acf.hip.
#include <cmath>

#include "mbar_ctx.h"

using namespace mbar;
using namespace mbar::host;

struct mbar_acf {
    int device = 0, kind = ACF_AUTO, nacc = 1;
    int64_t T = 0, ldx = 0, ntiles = 0, K = 1;
    int64_t last_change = -1;           // last n with A_n != A_n+1 (or B_n != B_n+1): suffixes from s > last_change are constant
    std::vector<int64_t> seg;           // segment lengths
    hipStream_t stream = nullptr;
    double2* A = nullptr;               // [ldx] A - shift_a as hi + lo (exact)
    double2* B = nullptr;               // [ldx] (== A for the autocorrelation)
    int* rem = nullptr;                 // [ldx]
    double2* SA = nullptr;              // [ldx] suffix sums of A'
    double2* SB = nullptr;              // [ldx] (== SA for the autocorrelation)
    double2* tot = nullptr;             // [ACF_MAX_LAGS][nacc][ntiles]
    double2* off = nullptr;
    int* active = nullptr;              // [ntiles]
    int* oid = nullptr;                 // [ldx]
    // rule state, one entry per origin (grown on demand)
    double *g = nullptr, *sig2 = nullptr;
    double2 *dA = nullptr, *dB = nullptr;
    int* status = nullptr;
    int64_t* stop = nullptr;
    size_t state_n = 0;
    double* ct = nullptr;
    size_t ct_n = 0;
    double2* q = nullptr;
    size_t q_n = 0;
    int64_t* orig = nullptr;
    size_t orig_n = 0;
    double *xab = nullptr, *xba = nullptr;
    size_t xab_n = 0, xba_n = 0;
};

namespace {

int afail(const std::string& msg, int code = MBAR_ERR_ARG) { return fail(nullptr, code, msg); }

#define AHIP(expr)                                                                                        \
    do {                                                                                                  \
        hipError_t _e = (expr);                                                                           \
        if (_e != hipSuccess) return afail(std::string(#expr) + ": " + hipGetErrorString(_e), MBAR_ERR_HIP); \
    } while (0)

template <typename T>
hipError_t grow(T** p, size_t* have, size_t want) {
    if (*have >= want) return hipSuccess;
    if (*p) {
        hipError_t e = cache_free(*p);
        if (e != hipSuccess) return e;
    }
    *p = nullptr;
    *have = 0;
    hipError_t e = cache_malloc((void**)p, want * sizeof(T));
    if (e == hipSuccess) *have = want;
    return e;
}

AcfLaunch base_launch(const mbar_acf* h) {
    AcfLaunch a{};
    a.kind = h->kind;
    a.nacc = h->nacc;
    a.A = h->A;
    a.B = h->B;
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

int grow_state(mbar_acf* h, size_t n) {
    if (h->state_n >= n) return MBAR_OK;
    for (void** p : {(void**)&h->g, (void**)&h->sig2, (void**)&h->dA, (void**)&h->dB, (void**)&h->status, (void**)&h->stop}) {
        if (*p) AHIP(cache_free(*p));
        *p = nullptr;
    }
    h->state_n = 0;
    for (void** p : {(void**)&h->g, (void**)&h->sig2, (void**)&h->stop}) AHIP(cache_malloc(p, n * sizeof(double)));
    for (void** p : {(void**)&h->dA, (void**)&h->dB}) AHIP(cache_malloc(p, n * sizeof(double2)));
    AHIP(cache_malloc((void**)&h->status, n * sizeof(int)));
    h->state_n = n;
    return MBAR_OK;
}

// Runs the stopping rule: origins o * nskip (o < norig) of one series, or the single origin of the K-segment form.  The host only
// reads the running origins per tile between lag blocks (8, 16, 32, then 64 lags).
int run_rule(mbar_acf* h, int mode, int64_t nskip, int64_t norig, int fast, int64_t mintime, int fft, bool record_ct) {
    AHIP(hipSetDevice(h->device));
    int rc = grow_state(h, (size_t)norig);
    if (rc) return rc;
    int64_t maxN = 0;
    for (int64_t L : h->seg) maxN = std::max(maxN, L);
    // every origin's lags stay below its end: T - s for the suffix form (fft: <= T - s - 1), max N_k - 1 for the segments
    const int64_t tmax = mode == ACF_RULE_SUFFIX ? h->T : maxN;
    if (record_ct) AHIP(grow(&h->ct, &h->ct_n, (size_t)schedule_entries(fast != 0, tmax)));
    AcfRule ru{};
    ru.mode = mode;
    ru.fft = fft;
    ru.nskip = nskip;
    ru.norig = norig;
    ru.mintime = mintime;
    ru.navg = (double)h->T / (double)h->seg.size();
    ru.tend = maxN - 1;
    ru.SA = h->SA;
    ru.SB = h->SB;
    ru.g = h->g;
    ru.sig2 = h->sig2;
    ru.dA = h->dA;
    ru.dB = h->dB;
    ru.status = h->status;
    ru.stop = h->stop;
    ru.ct = record_ct ? h->ct : nullptr;
    ru.active = h->active;
    AHIP(launch_acf_rule_init(h->stream, ru, h->T, mode == ACF_RULE_SUFFIX ? h->last_change : h->T));
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
        if (a.nl == 0) return afail("the lag schedule ended with running origins", MBAR_ERR_NUMERIC);
        a.tile_lo = c_lo;
        a.atile_hi = std::min(h->ntiles - 1, last_product_tile(h, a.lag[0]));
        AHIP(launch_acf_tiles(h->stream, a));
        AHIP(launch_acf_scan(h->stream, a));
        AHIP(launch_acf_rule(h->stream, a, ru, c_lo, c_hi));
        act.resize((size_t)(c_hi - c_lo + 1));
        AHIP(hipMemcpyAsync(act.data(), h->active + c_lo, act.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        AHIP(hipStreamSynchronize(h->stream));
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
    AHIP(hipMemcpyAsync(g, h->g, norig * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (stop) AHIP(hipMemcpyAsync(stop, h->stop, norig * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    if (status) AHIP(hipMemcpyAsync(status, h->status, norig * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    AHIP(hipStreamSynchronize(h->stream));
    return MBAR_OK;
}

}  // namespace

extern "C" {

int mbar_acf_create(mbar_acf** out, int device, int64_t T, const double* a, const double* b, int64_t K, const int64_t* seg,
                    double shift_a, double shift_b) {
    if (!out) return afail("out is NULL");
    *out = nullptr;
    if (T < 1 || !a) return afail("need at least one value");
    if (T >= ((int64_t)1 << 31) - ACF_TILE) return afail("series longer than 2^31 - 2^12 values");
    if (K < 1 || !seg) return afail("need at least one segment");
    int64_t sum = 0;
    for (int64_t k = 0; k < K; ++k) {
        if (seg[k] < 1) return afail("segment lengths must be positive");
        sum += seg[k];
    }
    if (sum != T) return afail("segment lengths must add up to T");
    if (!std::isfinite(shift_a) || !std::isfinite(shift_b)) return afail("shifts must be finite");
    for (int64_t i = 0; i < T; ++i)
        if (!std::isfinite(a[i]) || (b && !std::isfinite(b[i]))) return afail("the series must be finite");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1)
        return afail("no HIP device visible (libmbar_hip needs an MI355X / gfx950 GPU)", MBAR_ERR_NODEVICE);
    if (device < 0 || device >= n) return afail("device index out of range");
    AHIP(hipSetDevice(device));
    hipDeviceProp_t p;
    AHIP(hipGetDeviceProperties(&p, device));
    if (std::strncmp(p.gcnArchName, "gfx950", 6) != 0)
        return afail(std::string("device is ") + p.gcnArchName + ", this library is built for gfx950 only", MBAR_ERR_NODEVICE);
    mbar_acf* h = new mbar_acf();
    g_live_contexts.fetch_add(1);
    h->device = device;
    h->kind = b ? ACF_CROSS : ACF_AUTO;
    h->nacc = b ? 2 : 1;
    h->T = T;
    h->K = K;
    h->seg.assign(seg, seg + K);
    h->ldx = (T / ACF_TILE + 1) * ACF_TILE;  // (> T: position T exists and holds zeros)
    h->ntiles = h->ldx / ACF_TILE;
    for (int64_t i = 0; i + 1 < T; ++i)
        if (a[i] != a[i + 1] || (b && b[i] != b[i + 1])) h->last_change = i;
    int rc = MBAR_OK;
    auto hip = [&](hipError_t e, const char* what) {
        if (e != hipSuccess && rc == MBAR_OK) rc = afail(std::string(what) + ": " + hipGetErrorString(e), MBAR_ERR_HIP);
        return rc == MBAR_OK;
    };
    const size_t ldx = (size_t)h->ldx;
    if (hip(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking), "hipStreamCreateWithFlags") &&
        hip(cache_malloc((void**)&h->A, ldx * sizeof(double2)), "cache_malloc") &&
        hip(cache_malloc((void**)&h->rem, ldx * sizeof(int)), "cache_malloc") &&
        hip(cache_malloc((void**)&h->SA, ldx * sizeof(double2)), "cache_malloc") &&
        hip(cache_malloc((void**)&h->tot, (size_t)ACF_MAX_LAGS * 2 * h->ntiles * sizeof(double2)), "cache_malloc") &&
        hip(cache_malloc((void**)&h->off, (size_t)ACF_MAX_LAGS * 2 * h->ntiles * sizeof(double2)), "cache_malloc") &&
        hip(cache_malloc((void**)&h->active, (size_t)h->ntiles * sizeof(int)), "cache_malloc") &&
        hip(cache_malloc((void**)&h->oid, ldx * sizeof(int)), "cache_malloc") &&
        (!b || (hip(cache_malloc((void**)&h->B, ldx * sizeof(double2)), "cache_malloc") &&
                hip(cache_malloc((void**)&h->SB, ldx * sizeof(double2)), "cache_malloc")))) {
        if (!b) {
            h->B = h->A;
            h->SB = h->SA;
        }
        // x - shift exactly, as the rounded difference and its error (TwoSum)
        std::vector<double2> stage(ldx, double2{0.0, 0.0});
        auto shifted = [&](const double* x, double m) {
            for (int64_t i = 0; i < T; ++i) {
                const double s = x[i] - m, bb = s - x[i];
                stage[i] = double2{s, (x[i] - (s - bb)) + (-m - bb)};
            }
        };
        shifted(a, shift_a);
        hip(hipMemcpy(h->A, stage.data(), ldx * sizeof(double2), hipMemcpyHostToDevice), "hipMemcpy");
        if (b) {
            shifted(b, shift_b);
            hip(hipMemcpy(h->B, stage.data(), ldx * sizeof(double2), hipMemcpyHostToDevice), "hipMemcpy");
        }
        std::vector<int> rem(ldx, 0);
        int64_t pos = 0;
        for (int64_t k = 0; k < K; ++k)
            for (int64_t i = 0; i < seg[k]; ++i, ++pos) rem[pos] = (int)(seg[k] - i);
        hip(hipMemcpy(h->rem, rem.data(), ldx * sizeof(int), hipMemcpyHostToDevice), "hipMemcpy");
        hip(hipMemset(h->active, 0, (size_t)h->ntiles * sizeof(int)), "hipMemset");
        // suffix sums of A' (and B'): the plain term at lag 0 over every tile, stored at every position
        for (int which = 0; which < (b ? 2 : 1) && rc == MBAR_OK; ++which) {
            AcfLaunch l = base_launch(h);
            l.kind = ACF_PLAIN;
            l.nacc = 1;
            l.A = which ? h->B : h->A;
            l.nl = 1;
            l.lag[0] = 0;
            l.tile_lo = 0;
            l.atile_hi = h->ntiles - 1;
            hip(launch_acf_tiles(h->stream, l), "launch_acf_tiles") && hip(launch_acf_scan(h->stream, l), "launch_acf_scan") &&
                hip(launch_acf_store(h->stream, l, 0, h->ntiles - 1, nullptr, which ? h->SB : h->SA, h->ldx), "launch_acf_store");
        }
        if (rc == MBAR_OK) hip(hipStreamSynchronize(h->stream), "hipStreamSynchronize");
    }
    if (rc != MBAR_OK) {
        const std::string msg = mbar_last_error(nullptr);
        mbar_acf_destroy(h);
        return afail(msg, rc);
    }
    *out = h;
    return MBAR_OK;
}

void mbar_acf_destroy(mbar_acf* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->B == h->A) h->B = nullptr;
    if (h->SB == h->SA) h->SB = nullptr;
    for (void* p : {(void*)h->A, (void*)h->B, (void*)h->rem, (void*)h->SA, (void*)h->SB, (void*)h->tot, (void*)h->off, (void*)h->active,
                    (void*)h->oid, (void*)h->g, (void*)h->sig2, (void*)h->dA, (void*)h->dB, (void*)h->status, (void*)h->stop, (void*)h->ct,
                    (void*)h->q, (void*)h->orig, (void*)h->xab, (void*)h->xba})
        if (p) (void)cache_free(p);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    if (g_live_contexts.fetch_sub(1) == 1) g_mem.trim_to(g_mem.idle_limit());
}

int mbar_acf_suffix_g(mbar_acf* h, int64_t nskip, int fast, int64_t mintime, int fft, double* g, int64_t* stop, int32_t* status) {
    if (!h) return afail("acf is NULL");
    if (h->K != 1) return afail("suffix origins need one segment");
    if (nskip < 1) return afail("nskip must be >= 1");
    if (h->T < 2) return afail("need at least two values");
    if (!g) return afail("g is NULL");
    const int64_t norig = (h->T - 2) / nskip + 1;  // origins 0, nskip, ... < T - 1
    int rc = run_rule(h, ACF_RULE_SUFFIX, nskip, norig, fft ? 0 : fast, mintime, fft, false);
    if (rc) return rc;
    return copy_rule(h, norig, g, stop, status);
}

int mbar_acf_multiple_g(mbar_acf* h, int fast, int64_t mintime, double* g, int64_t* stop, int32_t* status, int64_t ct_cap,
                        double* ct) {
    if (!h) return afail("acf is NULL");
    if (h->kind != ACF_AUTO) return afail("the multiple form is an autocorrelation");
    if (!g) return afail("g is NULL");
    int64_t maxN = 0;
    for (int64_t L : h->seg) maxN = std::max(maxN, L);
    const int64_t entries = schedule_entries(fast != 0, maxN);
    if (ct && ct_cap < entries) return afail("ct_cap is below mbar_acf_schedule_length");
    int rc = run_rule(h, ACF_RULE_MULTIPLE, h->T, 1, fast, mintime, 0, ct != nullptr);
    if (rc) return rc;
    rc = copy_rule(h, 1, g, stop, status);
    if (rc) return rc;
    if (ct) AHIP(hipMemcpy(ct, h->ct, entries * sizeof(double), hipMemcpyDeviceToHost));
    return MBAR_OK;
}

int mbar_acf_schedule_length(int fast, int64_t tmax, int64_t* out) {
    if (!out) return afail("out is NULL");
    *out = schedule_entries(fast != 0, tmax);
    return MBAR_OK;
}

int mbar_acf_lag_sums(mbar_acf* h, int64_t nlags, const int64_t* lags, int64_t norig, const int64_t* origins, int segments,
                      double* xab, double* xba) {
    if (!h) return afail("acf is NULL");
    if (nlags < 0 || norig < 1 || !origins || (nlags > 0 && (!lags || !xab))) return afail("bad arguments");
    if (!segments && h->K != 1) return afail("suffix sums need one segment");
    for (int64_t i = 0; i < nlags; ++i)
        if (lags[i] < 0) return afail("lags must be >= 0");
    for (int64_t i = 0; i < norig; ++i)
        if (origins[i] < 0 || origins[i] >= h->T || (i > 0 && origins[i] <= origins[i - 1]))
            return afail("origins must be increasing positions of the series");
    if (nlags == 0) return MBAR_OK;
    AHIP(hipSetDevice(h->device));
    // positions whose suffix sums are stored: the origins and T (segment mode: the end of the last range)
    std::vector<int64_t> pos(origins, origins + norig);
    pos.push_back(h->T);
    AHIP(grow(&h->orig, &h->orig_n, pos.size()));
    AHIP(hipMemcpy(h->orig, pos.data(), pos.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    AHIP(launch_acf_fill_int(h->stream, h->oid, h->ldx, -1));
    AHIP(launch_acf_scatter_oid(h->stream, h->oid, h->orig, (int64_t)pos.size()));
    const int64_t ldo = norig + 1;
    AHIP(grow(&h->q, &h->q_n, (size_t)ACF_MAX_LAGS * h->nacc * ldo));
    AHIP(grow(&h->xab, &h->xab_n, (size_t)nlags * norig));
    AHIP(grow(&h->xba, &h->xba_n, (size_t)nlags * norig));
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
        AHIP(launch_acf_tiles(h->stream, a));
        AHIP(launch_acf_scan(h->stream, a));
        AHIP(launch_acf_store(h->stream, a, c_lo, c_hi, h->oid, h->q, ldo));
        AHIP(launch_acf_finish(h->stream, a, h->q, norig, h->orig, segments, h->SA, h->SB, h->xab, h->xba, j0));
    }
    AHIP(hipMemcpyAsync(xab, h->xab, (size_t)nlags * norig * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (xba) AHIP(hipMemcpyAsync(xba, h->xba, (size_t)nlags * norig * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    AHIP(hipStreamSynchronize(h->stream));
    return MBAR_OK;
}

}  // extern "C"
