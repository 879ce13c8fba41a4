// Host side of the reweighting scans over a linear family of unsampled states (include/mbar_hip.h, "reweighting scans"): the
// upload of the basis and observable vectors, the member panels of the two passes under the record budget, and the C ABI.
// Kernels: mbar_k_scan.hip.
#include "mbar_ctx.h"

using namespace mbar;
using namespace mbar::host;

namespace {
constexpr int64_t SCAN_MAX_K = 128;  // one W tile of the cross kernel
}  // namespace

namespace mbar {
namespace host {

int scan_ready(mbar_ctx* c, const char* who) {
    if (!c) return fail(c, MBAR_ERR_ARG, "NULL argument");
    if (c->ext_base) return fail(c, MBAR_ERR_STATE, std::string(who) + ": an extension context holds rows only");
    if (c->nranks > 1 || stream_transport(c) || c->host_reduce)
        return fail(c, MBAR_ERR_STATE, std::string(who) + ": the scan passes serve single-rank contexts only (a transport is attached)");
    if (wide_pitch(c)) return fail(c, MBAR_ERR_STATE, std::string(who) + ": the scan passes do not serve wide-pitch matrices (row pitch x 56 bytes >= 4 GiB)");
    if (c->K > SCAN_MAX_K) return fail(c, MBAR_ERR_STATE, std::string(who) + ": the scan passes serve at most 128 states");
    return MBAR_OK;
}

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

// the log-denominators of f into slot 0; *nan_out: the matrix or f is unusable and every output is NaN
int scan_logden(mbar_ctx* c, const double* f, bool* nan_out) {
    int rc = eval_core(c, f, 1, 0, c->logden[0], nullptr, nullptr, nullptr, nullptr);
    if (rc) return rc;
    *nan_out = c->u_poison || !f_is_finite(c, f, 1);
    return MBAR_OK;
}

// coeff | offset | f_scan of the call's members on the device (offset NULL: zeros; f_scan NULL: not uploaded)
int scan_upload_members(mbar_ctx* c, int64_t L, const double* coeff, const double* offset, const double* f_scan) {
    const int64_t B = c->scan_B;
    HIPCHK(c, c->scan_in.grow((size_t)L * (size_t)(B + 2)));
    double* d_coeff = c->scan_in;
    double* d_off = d_coeff + L * B;
    HIPCHK(c, hipMemcpyAsync(d_coeff, coeff, (size_t)L * B * sizeof(double), hipMemcpyHostToDevice, c->stream));
    if (offset) HIPCHK(c, hipMemcpyAsync(d_off, offset, (size_t)L * sizeof(double), hipMemcpyHostToDevice, c->stream));
    else HIPCHK(c, hipMemsetAsync(d_off, 0, (size_t)L * sizeof(double), c->stream));
    if (f_scan) HIPCHK(c, hipMemcpyAsync(d_off + L, f_scan, (size_t)L * sizeof(double), hipMemcpyHostToDevice, c->stream));
    return MBAR_OK;
}

}  // namespace host
}  // namespace mbar

extern "C" {

int mbar_ctx_set_scan(mbar_ctx* c, int64_t B, const double* basis, int64_t Q, const double* t) {
    int rc = scan_ready(c, "mbar_ctx_set_scan");
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
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

int mbar_scan_lognum(mbar_ctx* c, const double* f, int64_t L, const double* coeff, const double* offset, double* lognum, double* mean) {
    int rc = scan_ready(c, "mbar_scan_lognum");
    if (rc) return rc;
    if (!f || !coeff || !lognum || L < 1) return fail(c, MBAR_ERR_ARG, "mbar_scan_lognum: bad argument");
    if (c->scan_B < 1) return fail(c, MBAR_ERR_STATE, "mbar_scan_lognum: no basis on this context (mbar_ctx_set_scan first)");
    HIPCHK(c, hipSetDevice(c->device));
    bool nan = false;
    rc = scan_logden(c, f, &nan);
    if (rc) return rc;
    const int64_t B = c->scan_B, J = 1 + c->scan_Q;
    if (nan) {
        const double q = std::numeric_limits<double>::quiet_NaN();
        std::fill(lognum, lognum + L, q);
        if (mean) std::fill(mean, mean + L * J, q);
        return MBAR_OK;
    }
    rc = scan_upload_members(c, L, coeff, offset, nullptr);
    if (rc) return rc;
    const ScanData d = scan_data_of(c);
    // members in panels of a multiple of 64 whose records ([chunk][member][J]) fit the budget ("scan_part_bytes"): a member's sums
    // do not depend on the cut
    const int64_t nchunks = (c->N + SCAN_VCHUNK - 1) / SCAN_VCHUNK;
    int64_t pw = c->opt_scan_part_bytes / (std::max<int64_t>(nchunks, 1) * J * (int64_t)sizeof(double)) / 64 * 64;
    pw = std::min<int64_t>(std::max<int64_t>(pw, 64), (L + 63) / 64 * 64);
    HIPCHK(c, c->scan_part.grow((size_t)std::max<int64_t>(nchunks, 1) * (size_t)pw * (size_t)J));
    HIPCHK(c, c->scan_out.grow((size_t)L * (size_t)(2 + J)));
    double* d_M = c->scan_out;
    double* d_lognum = d_M + L;
    double* d_mean = d_lognum + L;
    const double* d_coeff = c->scan_in;
    const double* d_off = d_coeff + L * B;
    {
        ScopedTimer timer(c, MBAR_TIMER_OTHER);
        for (int64_t p0 = 0; p0 < L; p0 += pw) {
            const int64_t pl = std::min(pw, L - p0);
            HIPCHK(c, launch_scan_vec(c->stream, d, false, pl, d_coeff + p0 * B, d_off + p0, nullptr, c->scan_part));
            HIPCHK(c, launch_scan_vec_merge(c->stream, d, false, pl, c->scan_part, d_M + p0, nullptr, nullptr));
            HIPCHK(c, launch_scan_vec(c->stream, d, true, pl, d_coeff + p0 * B, d_off + p0, d_M + p0, c->scan_part));
            HIPCHK(c, launch_scan_vec_merge(c->stream, d, true, pl, c->scan_part, d_M + p0, d_lognum + p0, d_mean + p0 * J));
        }
    }
    HIPCHK(c, hipMemcpyAsync(lognum, d_lognum, (size_t)L * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (mean) HIPCHK(c, hipMemcpyAsync(mean, d_mean, (size_t)L * J * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return sync_stream(c);
}

int mbar_scan_gram_w(mbar_ctx* c, const double* f, int64_t L, const double* coeff, const double* offset, const double* f_scan, int64_t r,
                     double* cross, double* within, double* refcol, double* wsum) {
    int rc = scan_ready(c, "mbar_scan_gram_w");
    if (rc) return rc;
    if (!f || !coeff || !f_scan || !within || !refcol || !wsum || L < 1 || r < 0 || r >= L)
        return fail(c, MBAR_ERR_ARG, "mbar_scan_gram_w: bad argument");
    if (c->scan_B < 1) return fail(c, MBAR_ERR_STATE, "mbar_scan_gram_w: no basis on this context (mbar_ctx_set_scan first)");
    HIPCHK(c, hipSetDevice(c->device));
    bool nan = false;
    rc = scan_logden(c, f, &nan);
    if (rc) return rc;
    const int64_t B = c->scan_B, K = c->K;
    const int J = 1 + (int)c->scan_Q, NW = J * (J + 1) / 2, NV = scan_nv(J);
    for (int64_t l = 0; l < L; ++l) nan = nan || std::isnan(f_scan[l]);
    if (nan) {
        const double q = std::numeric_limits<double>::quiet_NaN();
        if (cross) std::fill(cross, cross + (size_t)K * L * J, q);
        std::fill(within, within + L * NW, q);
        std::fill(refcol, refcol + L * J, q);
        std::fill(wsum, wsum + L, q);
        return MBAR_OK;
    }
    rc = scan_upload_members(c, L, coeff, offset, f_scan);
    if (rc) return rc;
    const ScanData d = scan_data_of(c);
    const int nb = cross ? scan_nb_for(K) : 0;
    const int64_t nchunks = (c->N + SCAN_CHUNK - 1) / SCAN_CHUNK;
    const int64_t pw = 64 * scan_mb(J);
    HIPCHK(c, c->scan_part.grow((size_t)std::max<int64_t>(nchunks, 1) * (size_t)scan_record_doubles(nb, J)));
    HIPCHK(c, c->scan_out.grow((size_t)L * (size_t)NV + (cross ? (size_t)K * L * J : 0)));
    double* d_vec = c->scan_out;
    double* d_cross = d_vec + L * NV;
    const double* d_coeff = c->scan_in;
    const double* d_off = d_coeff + L * B;
    const double* d_fscan = d_off + L;
    HIPCHK(c, hipMemcpyAsync(d_f(c), f, (size_t)K * sizeof(double), hipMemcpyHostToDevice, c->stream));
    {
        ScopedTimer timer(c, MBAR_TIMER_OTHER);
        for (int64_t p0 = 0; p0 < L; p0 += pw) {  // the resident matrix is read once per panel
            HIPCHK(c, launch_scan_cross(c->stream, d, nb, c->u, c->ld, K, d_f(c), L, p0, d_coeff, d_off, d_fscan, r, c->scan_part));
            HIPCHK(c, launch_scan_cross_merge(c->stream, d, nb, K, L, p0, c->scan_part, d_cross, d_vec));
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
        std::copy(v + 1, v + 1 + J, refcol + l * J);
        std::copy(v + 1 + J, v + NV, within + l * NW);
    }
    return MBAR_OK;
}

}  // extern "C"
