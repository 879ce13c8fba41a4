// Host side of the weighted kernel-density sums (include/mbar_hip.h, "weighted kernel-density sums"): the mbar_kde handle (on the
// handle layer of mbar_handle.h), the per-column scaling of the weights and their passes, and the exact recomputation of the rare
// (query, column) pairs the combine kernel flags.  Kernels: mbar_k_kde.hip.
#include <cmath>
#include <string>

#include "mbar_handle.h"
#include "mbar_kde.h"

using namespace mbar;
using namespace mbar::host;

struct mbar_kde : Handle {
    int kernel = 0, d = 1, num_cu = 256;
    int64_t N = 0, ldx = 0;
    int64_t max_chunks = 0;          // option "max_chunks": cap of the sample chunks of an evaluation (0: none)
    double h = 1.0, lognorm = 0.0;
    DevBuf<double> X;                // [d][ldx]
    // weights: every column scaled by a power of two, so that its largest entry lies in [1, 2), and the log of the column totals
    ColumnPasses V{{1, 4, 8, 16, 24, 32}};
    std::vector<double> logW;        // [C]
    DevBuf<double> logW_d;           // [KDE_MAX_CB] of the pass on the device
    DevBuf<double> part, Q;
    DevBuf<double> out;              // [M][cb] log densities of a pass, then the recomputed pairs
    DevBuf<int> flag;
    DevBuf<int64_t> pq;
};

namespace {

// log of the normaliser 1 / integral over R^d of k(|x| / h), k the kernel on the unit scale.  With V_d = pi^(d/2) / Gamma(d/2 + 1)
// the volume of the unit d-ball and S_(d-1) = d V_d its surface, the integral is S_(d-1) int_0^1 r^(d-1) k(r) dr h^d:
//   gaussian      (2 pi)^(d/2)          exp(-r^2 / 2) over all r
//   tophat        V_d
//   epanechnikov  S_(d-1) (1/d - 1/(d+2))  = 2 V_d / (d + 2)
//   exponential   S_(d-1) Gamma(d)          = V_d d!
//   linear        S_(d-1) (1/d - 1/(d+1))  = V_d / (d + 1)
//   cosine        S_(d-1) I_(d-1),  I_n = int_0^1 r^n cos(pi r / 2) dr by parts: I_n = 2/pi - (2n/pi) J_(n-1), J_n = (2n/pi) I_(n-1),
//                 J_n = int_0^1 r^n sin(pi r / 2) dr, I_0 = J_0 = 2/pi
double log_norm(int kernel, int d, double h) {
    const double pi = 3.14159265358979323846;
    const double logVd = 0.5 * d * std::log(pi) - std::lgamma(0.5 * d + 1.0);
    const double dlogh = d * std::log(h);
    switch (kernel) {
        case KDE_GAUSSIAN: return -0.5 * d * std::log(2.0 * pi) - dlogh;
        case KDE_TOPHAT: return -logVd - dlogh;
        case KDE_EPANECHNIKOV: return std::log(0.5 * (d + 2)) - logVd - dlogh;
        case KDE_EXPONENTIAL: return -logVd - std::lgamma(d + 1.0) - dlogh;
        case KDE_LINEAR: return std::log((double)(d + 1)) - logVd - dlogh;
        default: {
            // (the recursion cancels: I_7 = 0.087 from terms of order one after seven steps that each amplify the error by
            // 2n / pi.  In fp64 it left 2.3e-13 in the d = 8 normaliser; in long double it is exact to fp64.)
            const long double pil = 3.14159265358979323846264338327950288L;
            long double I = 2.0L / pil, J = 2.0L / pil;
            for (int n = 1; n < d; ++n) {
                const long double In = 2.0L / pil - (2.0L * n / pil) * J;
                J = (2.0L * n / pil) * I;
                I = In;
            }
            return -std::log(d * std::exp(logVd) * (double)I) - dlogh;
        }
    }
}

// Neumaier-compensated sum (the column totals: N up to 1e9 positive terms)
double csum(const double* v, int64_t n, int64_t stride) {
    double s = 0.0, comp = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        const double x = v[i * stride];
        const double t = s + x;
        comp += std::fabs(s) >= std::fabs(x) ? (s - t) + x : (x - t) + s;
        s = t;
    }
    return s + comp;
}

// the weights and log column totals of columns [c0, c0 + cv) as a pass of width cb
int upload_pass(mbar_kde* k, int64_t c0, int cv, int cb) {
    if (k->V.holds(c0, cb)) return MBAR_OK;
    std::vector<double> lw(KDE_MAX_CB, 0.0);
    for (int c = 0; c < cv; ++c) lw[c] = k->logW[c0 + c];
    HIPCHK(nullptr, hipMemcpy(k->logW_d, lw.data(), lw.size() * sizeof(double), hipMemcpyHostToDevice));
    return k->V.upload(c0, cv, cb, k->ldx);
}

}  // namespace

extern "C" {

int mbar_kde_log_norm(int kernel, int d, double bandwidth, double* out) {
    if (!out) return bad_arg("out is NULL");
    if (kernel < 0 || kernel > KDE_COSINE) return bad_arg("unknown kernel");
    if (d < 1 || d > KDE_MAX_D) return bad_arg("d must be 1 .. 8");
    if (!(bandwidth > 0.0) || !std::isfinite(bandwidth)) return bad_arg("bandwidth must be positive and finite");
    *out = log_norm(kernel, d, bandwidth);
    return MBAR_OK;
}

int mbar_kde_create(mbar_kde** out, int device, int kernel, int d, int64_t N, const double* x, double bandwidth) {
    if (!out) return bad_arg("out is NULL");
    *out = nullptr;
    if (kernel < 0 || kernel > KDE_COSINE) return bad_arg("unknown kernel");
    if (d < 1 || d > KDE_MAX_D) return bad_arg("d must be 1 .. 8");
    if (N < 1 || !x) return bad_arg("need at least one sample");
    if (!(bandwidth > 0.0) || !std::isfinite(bandwidth)) return bad_arg("bandwidth must be positive and finite");
    for (int64_t i = 0; i < N * d; ++i)
        if (!std::isfinite(x[i])) return bad_arg("sample coordinates must be finite");
    return create_handle(out, device, [&](mbar_kde* k, const DevInfo& di) {
        k->kernel = kernel;
        k->d = d;
        k->N = N;
        k->h = bandwidth;
        k->lognorm = log_norm(kernel, d, bandwidth);
        k->num_cu = di.num_cu;
        k->ldx = (N + KDE_TILE - 1) / KDE_TILE * KDE_TILE;
        HIPCHK(nullptr, k->logW_d.grow(KDE_MAX_CB));
        // coordinate-major, padded with copies of the last sample (weight zero: they add nothing, and they never hold a
        // query's running shift above what a real sample gives)
        std::vector<double> stage((size_t)d * k->ldx);
        for (int j = 0; j < d; ++j)
            for (int64_t i = 0; i < k->ldx; ++i) stage[(size_t)j * k->ldx + i] = x[(i < N ? i : N - 1) * d + j];
        HIPCHK(nullptr, k->X.upload(stage.data(), stage.size()));
        std::vector<double> ones((size_t)N, 1.0);
        return mbar_kde_set_weights(k, 1, ones.data());
    });
}

void mbar_kde_destroy(mbar_kde* k) { destroy_handle(k); }

int mbar_kde_set_weights(mbar_kde* k, int64_t C, const double* v) {
    if (!k) return bad_arg("kde is NULL");
    if (C < 1 || !v) return bad_arg("need at least one weight column");
    const int64_t N = k->N;
    std::vector<double> colmax((size_t)C, 0.0);
    for (int64_t n = 0; n < N; ++n)
        for (int64_t c = 0; c < C; ++c) {
            const double w = v[n * C + c];
            if (!std::isfinite(w) || w < 0.0) return bad_arg("weights must be finite and non-negative");
            if (w > colmax[c]) colmax[c] = w;
        }
    // a power-of-two scale per column (exact): the largest weight lies in [1, 2), so that N 2^257 bounds every device sum
    std::vector<double> scale((size_t)C, 1.0);
    for (int64_t c = 0; c < C; ++c)
        if (colmax[c] > 0.0) scale[c] = std::ldexp(1.0, -std::ilogb(colmax[c]));
    double* Vh = k->V.reset(N, C);
    for (int64_t n = 0; n < N; ++n)
        for (int64_t c = 0; c < C; ++c) Vh[(size_t)n * C + c] = v[n * C + c] * scale[c];
    k->logW.assign((size_t)C, 0.0);
    for (int64_t c = 0; c < C; ++c) k->logW[c] = std::log(csum(Vh + c, N, C));  // (log 0 = -inf: a column without weight)
    HIPCHK(nullptr, hipSetDevice(k->device));
    if (C <= KDE_MAX_CB) return upload_pass(k, 0, (int)C, k->V.width(C));  // (one pass: stays resident between calls)
    return MBAR_OK;
}

int mbar_kde_set_option(mbar_kde* k, const char* key, int64_t value) {
    if (!key || std::string(key) != "max_chunks") return bad_arg("unknown kde option (known: \"max_chunks\")");
    if (value < 0) return bad_arg("max_chunks must be >= 0 (0: the default cut)");
    if (!k) return bad_arg("kde is NULL");
    k->max_chunks = value;  // (read by the next mbar_kde_eval)
    return MBAR_OK;
}

int mbar_kde_eval(mbar_kde* k, int64_t M, const double* q, double* out) {
    if (!k) return bad_arg("kde is NULL");
    if (M < 0 || (M > 0 && (!q || !out))) return bad_arg("bad query arguments");
    if (M == 0) return MBAR_OK;
    const int d = k->d;
    for (int64_t i = 0; i < M * d; ++i)
        if (!std::isfinite(q[i])) return bad_arg("query coordinates must be finite");
    HIPCHK(nullptr, hipSetDevice(k->device));
    const int64_t qblocks = (M + 255) / 256, ldq = qblocks * 256;
    {
        std::vector<double> stage((size_t)d * ldq);
        for (int j = 0; j < d; ++j)
            for (int64_t i = 0; i < ldq; ++i) stage[(size_t)j * ldq + i] = q[(i < M ? i : M - 1) * d + j];
        HIPCHK(nullptr, k->Q.upload(stage.data(), stage.size()));
    }
    // grid: 256 queries x one chunk of whole tiles per workgroup, about four workgroups per CU (their LDS allows four)
    const int64_t ntiles = k->ldx / KDE_TILE;
    int64_t want = (4 * (int64_t)k->num_cu + qblocks - 1) / qblocks;
    if (k->max_chunks >= 1 && want > k->max_chunks) want = k->max_chunks;  // (option "max_chunks"; 0: the rule above alone)
    if (want < 1) want = 1;
    if (want > ntiles) want = ntiles;
    if (want > 65535) want = 65535;
    const int64_t chunk = (ntiles + want - 1) / want * KDE_TILE;
    const int64_t nchunks = (k->ldx + chunk - 1) / chunk;
    const double LOG2E_ = 1.4426950408889634074;
    const double S = (double)(1 << 11);  // 2^EXP2_BITS of mbar_device.h
    KdeLaunch a;
    a.kernel = k->kernel;
    a.d = d;
    a.X = k->X;
    a.ldx = k->ldx;
    a.Q = k->Q;
    a.ldq = ldq;
    a.M = M;
    a.h = k->h;
    a.inv_h = 1.0 / k->h;
    a.inv_h2 = 1.0 / (k->h * k->h);
    a.coef = k->kernel == KDE_GAUSSIAN ? -S * LOG2E_ * 0.5 * a.inv_h2 : -S * LOG2E_ * a.inv_h;
    a.qblocks = qblocks;
    a.nchunks = nchunks;
    a.chunk = chunk;
    std::vector<double> hout;
    std::vector<int> hflag;
    const int64_t C = k->V.C;
    for (int64_t c0 = 0; c0 < C; c0 += KDE_MAX_CB) {
        const int cv = (int)std::min<int64_t>(KDE_MAX_CB, C - c0);
        const int cb = k->V.width(cv);
        int rc = upload_pass(k, c0, cv, cb);
        if (rc) return rc;
        a.cb = cb;
        a.V = k->V.dev;
        HIPCHK(nullptr, k->part.grow((size_t)nchunks * (cb + 1) * ldq));
        HIPCHK(nullptr, k->out.grow((size_t)M * cv));
        HIPCHK(nullptr, k->flag.grow((size_t)M * cv));
        a.part = k->part;
        HIPCHK(nullptr, launch_kde(k->stream, a));
        HIPCHK(nullptr, launch_kde_combine(k->stream, a, cv, k->logW_d, k->lognorm, k->out, k->flag));
        hout.resize((size_t)M * cv);
        hflag.resize((size_t)M * cv);
        HIPCHK(nullptr, hipMemcpyAsync(hout.data(), k->out, hout.size() * sizeof(double), hipMemcpyDeviceToHost, k->stream));
        HIPCHK(nullptr, hipMemcpyAsync(hflag.data(), k->flag, hflag.size() * sizeof(int), hipMemcpyDeviceToHost, k->stream));
        HIPCHK(nullptr, hipStreamSynchronize(k->stream));
        std::vector<int64_t> pairs;
        for (int64_t i = 0; i < M; ++i)
            for (int c = 0; c < cv; ++c)
                if (hflag[(size_t)i * cv + c]) {
                    pairs.push_back(i);
                    pairs.push_back(c);
                }
        const int64_t np = (int64_t)pairs.size() / 2;
        if (np > 0) {  // every term of these pairs underflowed against the shared shift: their own maximum, in log space
            HIPCHK(nullptr, k->pq.upload(pairs.data(), pairs.size()));
            HIPCHK(nullptr, launch_kde_exact(k->stream, a, k->N, np, k->pq, k->logW_d, k->lognorm, k->out));
            std::vector<double> redo((size_t)np);
            HIPCHK(nullptr, hipMemcpyAsync(redo.data(), k->out, redo.size() * sizeof(double), hipMemcpyDeviceToHost, k->stream));
            HIPCHK(nullptr, hipStreamSynchronize(k->stream));
            for (int64_t p = 0; p < np; ++p) hout[(size_t)pairs[2 * p] * cv + pairs[2 * p + 1]] = redo[p];
        }
        for (int64_t i = 0; i < M; ++i)
            for (int c = 0; c < cv; ++c) out[i * C + c0 + c] = hout[(size_t)i * cv + c];
    }
    return MBAR_OK;
}

}  // extern "C"
