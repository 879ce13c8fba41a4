// Host side of libmbar_hip.so, the writers of the resident matrix (mbar_ctx.h lists the files of the context layer): uploads, row
// arithmetic, log shifts, masked, linear and family fills, the harmonic generator -- each ends in matrix_touched -- and the
// download.  The rows an extension context takes from its base are written in mbar_ext.cpp.
#include "mbar_ctx.h"

using namespace mbar;
using namespace mbar::host;

namespace mbar {
namespace host {

int family_terms(mbar_ctx* c, const char* who, int64_t B, const int32_t* kind, const double* period, FamilyTerms* out) {
    FamilyTerms t{};
    int H = 0;
    for (int64_t b = 0; b < B; ++b) {
        if (!kind[b]) continue;
        const double P = period ? period[b] : 0.0;
        if (!std::isfinite(P) || P < 0.0 || (P > 0.0 && !std::isfinite(1.0 / P)))
            return fail(c, MBAR_ERR_ARG, std::string(who) + ": the period of a harmonic term must be finite and not negative (0: not periodic)");
        if (++H > MBAR_SCAN_MAX_H)
            return fail(c, MBAR_ERR_ARG, std::string(who) + ": at most " + std::to_string(MBAR_SCAN_MAX_H) + " terms of a family may be harmonic");
        t.mask |= 1u << b;
        t.period[b] = P;
        t.rperiod[b] = P > 0.0 ? 1.0 / P : 0.0;
    }
    *out = t;
    return MBAR_OK;
}

}  // namespace host
}  // namespace mbar

extern "C" {

int mbar_ctx_upload_u(mbar_ctx* c, const double* u_host, int64_t ld_host, int64_t col0_host, int64_t ncols,
                      int64_t col0_dev) {
    if (!c || !u_host) return fail(c, MBAR_ERR_ARG, "NULL argument");
    if (ncols < 0 || col0_dev < 0 || col0_dev + ncols > c->N || col0_host < 0 || col0_host + ncols > ld_host)
        return fail(c, MBAR_ERR_ARG, "column range out of bounds");
    if (ncols == 0) return MBAR_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy2DAsync(c->u + col0_dev, (size_t)c->ld * sizeof(double), u_host + col0_host,
                               (size_t)ld_host * sizeof(double), (size_t)ncols * sizeof(double), (size_t)c->K,
                               hipMemcpyHostToDevice, c->stream));
    matrix_touched(c);
    return sync_stream(c);
}

int mbar_ctx_upload_rows(mbar_ctx* c, int64_t row0, int64_t nrows, const double* rows_host, int64_t ld_host) {
    if (!c || !rows_host) return fail(c, MBAR_ERR_ARG, "NULL argument");
    if (!rows_in_range(c, row0, nrows) || ld_host < c->N) return fail(c, MBAR_ERR_ARG, "row range out of bounds");
    if (nrows == 0) return MBAR_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpy2DAsync(c->u + row0 * c->ld, (size_t)c->ld * sizeof(double), rows_host,
                               (size_t)ld_host * sizeof(double), (size_t)c->N * sizeof(double), (size_t)nrows,
                               hipMemcpyHostToDevice, c->stream));
    matrix_touched(c);
    return sync_stream(c);
}

int mbar_ctx_copy_rows(mbar_ctx* dst, int64_t dst_row0, mbar_ctx* src, int64_t src_row0, int64_t nrows) {
    if (!dst || !src) return fail(dst, MBAR_ERR_ARG, "NULL argument");
    if (dst->device != src->device || dst->N != src->N) return fail(dst, MBAR_ERR_ARG, "contexts must share device and N_local");
    if (!rows_in_range(dst, dst_row0, nrows) || !rows_in_range(src, src_row0, nrows)) return fail(dst, MBAR_ERR_ARG, "row range out of bounds");
    if (nrows == 0) return MBAR_OK;
    HIPCHK(dst, hipSetDevice(dst->device));
    HIPCHK(dst, hipStreamSynchronize(src->stream));  // whatever produced the source rows has finished
    if (dst->ld == src->ld)  // same pitch (same N_local): the rows are one contiguous block, padding included (it is zero in both)
        HIPCHK(dst, hipMemcpyAsync(dst->u + dst_row0 * dst->ld, src->u + src_row0 * src->ld, (size_t)nrows * dst->ld * sizeof(double),
                                   hipMemcpyDeviceToDevice, dst->stream));
    else
        HIPCHK(dst, hipMemcpy2DAsync(dst->u + dst_row0 * dst->ld, (size_t)dst->ld * sizeof(double), src->u + src_row0 * src->ld,
                                     (size_t)src->ld * sizeof(double), (size_t)dst->N * sizeof(double), (size_t)nrows,
                                     hipMemcpyDeviceToDevice, dst->stream));
    matrix_touched(dst);
    return sync_stream(dst);
}

// The staging vector of the row operations (one N_local-vector, allocated at its first use) ...
static hipError_t need_vec_tmp(mbar_ctx* c) { return c->vec_tmp.grow((size_t)c->ld); }
// ... holding v_host, or (NULL) still what the previous call put there: one observable at many states
static int stage_vec(mbar_ctx* c, const double* v_host) {
    HIPCHK(c, need_vec_tmp(c));
    if (v_host) {
        c->vec_holds_logshift = false;
        HIPCHK(c, hipMemcpyAsync(c->vec_tmp, v_host, (size_t)c->N * sizeof(double), hipMemcpyHostToDevice, c->stream));
    }
    return MBAR_OK;
}

int mbar_ctx_row_sub(mbar_ctx* c, int64_t row, const double* v_host) {
    if (!c) return fail(c, MBAR_ERR_ARG, "NULL argument");
    if (row < 0 || row >= c->K) return fail(c, MBAR_ERR_ARG, "row out of range");
    if (!v_host && !c->vec_tmp) return fail(c, MBAR_ERR_STATE, "mbar_ctx_row_sub: no vector has been uploaded yet");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = stage_vec(c, v_host);
    if (rc) return rc;
    HIPCHK(c, launch_row_sub(c->stream, c->u + row * c->ld, c->vec_tmp, c->N));
    matrix_touched(c);
    return sync_stream(c);
}

// dst rows = src rows - v (v_host, or NULL: the vector staged in dst by the previous call / mbar_ctx_vec_logshift); src is dst or its
// base.  `who`: the entry point, for the error strings.
static int rows_sub_from(const char* who, mbar_ctx* dst, int64_t dst_row0, mbar_ctx* src, int64_t src_row0, int64_t nrows,
                         const double* v_host) {
    if (!dst || !src) return fail(dst, MBAR_ERR_ARG, "NULL argument");
    if (src != dst && dst->ext_base != src) return fail(dst, MBAR_ERR_ARG, std::string(who) + ": src must be dst or its base");
    if (!rows_in_range(dst, dst_row0, nrows) || !rows_in_range(src, src_row0, nrows)) return fail(dst, MBAR_ERR_ARG, "row range out of bounds");
    if (src == dst && dst_row0 != src_row0 && dst_row0 < src_row0 + nrows && src_row0 < dst_row0 + nrows)
        return fail(dst, MBAR_ERR_ARG, std::string(who) + ": the row ranges overlap");
    if (!v_host && !dst->vec_tmp) return fail(dst, MBAR_ERR_STATE, std::string(who) + ": no vector has been uploaded yet");
    if (nrows == 0) return MBAR_OK;
    HIPCHK(dst, hipSetDevice(dst->device));
    if (src != dst) HIPCHK(dst, hipStreamSynchronize(src->stream));
    int rc = stage_vec(dst, v_host);
    if (rc) return rc;
    HIPCHK(dst, launch_rows_sub(dst->stream, dst->u + dst_row0 * dst->ld, src->u + src_row0 * src->ld, dst->ld, nrows, dst->vec_tmp, dst->N));
    matrix_touched(dst);
    return sync_stream(dst);
}
int mbar_ctx_rows_sub(mbar_ctx* c, int64_t dst_row0, int64_t src_row0, int64_t nrows, const double* v_host) {
    return rows_sub_from("mbar_ctx_rows_sub", c, dst_row0, c, src_row0, nrows, v_host);
}
int mbar_ctx_rows_sub_from(mbar_ctx* dst, int64_t dst_row0, mbar_ctx* src, int64_t src_row0, int64_t nrows, const double* v_host) {
    return rows_sub_from("mbar_ctx_rows_sub_from", dst, dst_row0, src, src_row0, nrows, v_host);
}

// dst rows = src rows - dst rows; src is dst or its base
static int rows_rsub_from(const char* who, mbar_ctx* dst, int64_t dst_row0, mbar_ctx* src, int64_t src_row0, int64_t nrows) {
    if (!dst || !src) return fail(dst, MBAR_ERR_ARG, "NULL argument");
    if (src != dst && dst->ext_base != src) return fail(dst, MBAR_ERR_ARG, std::string(who) + ": src must be dst or its base");
    if (!rows_in_range(dst, dst_row0, nrows) || !rows_in_range(src, src_row0, nrows)) return fail(dst, MBAR_ERR_ARG, "row range out of bounds");
    if (src == dst && dst_row0 < src_row0 + nrows && src_row0 < dst_row0 + nrows)
        return fail(dst, MBAR_ERR_ARG, std::string(who) + ": the row ranges overlap");
    if (nrows == 0) return MBAR_OK;
    HIPCHK(dst, hipSetDevice(dst->device));
    if (src != dst) HIPCHK(dst, hipStreamSynchronize(src->stream));
    HIPCHK(dst, launch_rows_rsub(dst->stream, dst->u + dst_row0 * dst->ld, src->u + src_row0 * src->ld, dst->ld, nrows, dst->N));
    matrix_touched(dst);
    return sync_stream(dst);
}
int mbar_ctx_rows_rsub(mbar_ctx* c, int64_t dst_row0, int64_t src_row0, int64_t nrows) {
    return rows_rsub_from("mbar_ctx_rows_rsub", c, dst_row0, c, src_row0, nrows);
}
int mbar_ctx_rows_rsub_from(mbar_ctx* dst, int64_t dst_row0, mbar_ctx* src, int64_t src_row0, int64_t nrows) {
    return rows_rsub_from("mbar_ctx_rows_rsub_from", dst, dst_row0, src, src_row0, nrows);
}

// shared tail of the two log-shift entry points: `base` holds nrows rows of raw observable values, scratch nrows * 257 doubles
static int logshift_rows(mbar_ctx* c, double* base, int64_t nrows, double* shift_host) {
    double* shift_dev = c->scratch + (size_t)nrows * 256;
    HIPCHK(c, launch_rows_logshift(c->stream, base, c->ld, nrows, c->N, c->scratch, shift_dev));
    HIPCHK(c, hipMemcpyAsync(shift_host, shift_dev, (size_t)nrows * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    return sync_stream(c);
}

int mbar_ctx_rows_logshift(mbar_ctx* c, int64_t row0, int64_t nrows, double* shift_out) {
    if (!c || !shift_out) return fail(c, MBAR_ERR_ARG, "NULL argument");
    if (!rows_in_range(c, row0, nrows)) return fail(c, MBAR_ERR_ARG, "row range out of bounds");
    if (nrows == 0) return MBAR_OK;
    if (c->nranks > 1) return fail(c, MBAR_ERR_STATE, "mbar_ctx_rows_logshift: the minimum is taken over this context's samples only");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = ensure(c, c->scratch, (size_t)nrows * 257);
    if (rc) return rc;
    matrix_touched(c);
    return logshift_rows(c, c->u + row0 * c->ld, nrows, shift_out);
}

int mbar_ctx_vec_logshift(mbar_ctx* c, const double* A_host, double* shift_out) {
    if (!c || !A_host || !shift_out) return fail(c, MBAR_ERR_ARG, "NULL argument");
    if (c->nranks > 1) return fail(c, MBAR_ERR_STATE, "mbar_ctx_vec_logshift: the minimum is taken over this context's samples only");
    HIPCHK(c, hipSetDevice(c->device));
    int lrc = ensure(c, c->scratch, 257);  // (before the vector's copy is queued)
    if (!lrc) lrc = stage_vec(c, A_host);
    if (lrc) return lrc;
    lrc = logshift_rows(c, c->vec_tmp, 1, shift_out);
    c->vec_holds_logshift = lrc == MBAR_OK;
    return lrc;
}

int mbar_ctx_fill_masked_rows(mbar_ctx* c, int64_t row0, int64_t nrows, const double* v_host, const int32_t* label_host) {
    if (!c || !v_host || !label_host) return fail(c, MBAR_ERR_ARG, "NULL argument");
    if (!rows_in_range(c, row0, nrows)) return fail(c, MBAR_ERR_ARG, "row range out of bounds");
    if (nrows == 0) return MBAR_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, need_vec_tmp(c));
    DevBuf<int> dlabel;
    HIPCHK(c, dlabel.grow((size_t)c->N));
    c->vec_holds_logshift = false;
    hipError_t e = hipMemcpyAsync(c->vec_tmp, v_host, (size_t)c->N * sizeof(double), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dlabel, label_host, (size_t)c->N * sizeof(int), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = launch_fill_masked_rows(c->stream, c->u + row0 * c->ld, c->ld, c->N, nrows, c->vec_tmp, dlabel);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(c, MBAR_ERR_HIP, std::string("mbar_ctx_fill_masked_rows: ") + hipGetErrorString(e));
    matrix_touched(c);
    flush_timers(c);
    return MBAR_OK;
}

// mbar_ctx_fill_family_rows and mbar_ctx_fill_linear_rows (who) are one call.  What both refuse first, in this order:
static int fill_rows_refused(mbar_ctx* c, const char* who, int64_t row0, int64_t nrows, int64_t B, const double* basis_host, int64_t ld_host,
                             int64_t col0_host, const double* coeff) {
    if (!c || !basis_host || !coeff) return fail(c, MBAR_ERR_ARG, "NULL argument");
    if (c->ext_base) return fail(c, MBAR_ERR_STATE, std::string(who) + ": not offered on an extension context");
    if (B < 1 || B > SCAN_MAX_B) return fail(c, MBAR_ERR_ARG, std::string(who) + ": 1 <= B <= 8 basis vectors");
    if (!rows_in_range(c, row0, nrows)) return fail(c, MBAR_ERR_ARG, "row range out of bounds");
    if (col0_host < 0 || ld_host < 0 || col0_host > ld_host || c->N > ld_host - col0_host)
        return fail(c, MBAR_ERR_ARG, "column range out of bounds");
    return MBAR_OK;
}

// and the fill itself, of arguments that passed fill_rows_refused; center is read when terms.mask names a harmonic term
static int fill_rows(mbar_ctx* c, const char* who, int64_t row0, int64_t nrows, int64_t B, const double* basis_host, int64_t ld_host,
                     int64_t col0_host, const double* coeff, const double* center, const double* offset, const FamilyTerms& terms) {
    if (nrows == 0) return MBAR_OK;
    if (c->N == 0) {  // (a shard without columns: nothing to write)
        matrix_touched(c);
        return MBAR_OK;
    }
    HIPCHK(c, hipSetDevice(c->device));
    // the basis shard in a block of the cache, at the matrix's own pitch (whole 16-sample tiles: every column pair is aligned; what
    // lies behind column N_local of the block is never read), and coeff[nrows][B] | offset[nrows] | center[nrows][B] (with a
    // harmonic term only: the kernel of a family without one does not read them); both blocks go back to the cache on return,
    // after the stream has been drained
    DevBuf<double> dbasis, dmembers;
    HIPCHK(c, dbasis.grow((size_t)B * (size_t)c->ld));
    HIPCHK(c, dmembers.grow((size_t)nrows * (size_t)((terms.mask ? 2 : 1) * B + 1)));
    double* d_coeff = dmembers;
    double* d_off = d_coeff + nrows * B;
    double* d_center = terms.mask ? d_off + nrows : nullptr;
    const size_t members = (size_t)nrows * B * sizeof(double);
    hipError_t e = hipMemcpy2DAsync(dbasis, (size_t)c->ld * sizeof(double), basis_host + col0_host, (size_t)ld_host * sizeof(double),
                                    (size_t)c->N * sizeof(double), (size_t)B, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_coeff, coeff, members, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess)
        e = offset ? hipMemcpyAsync(d_off, offset, (size_t)nrows * sizeof(double), hipMemcpyHostToDevice, c->stream)
                   : hipMemsetAsync(d_off, 0, (size_t)nrows * sizeof(double), c->stream);
    if (e == hipSuccess && d_center) e = hipMemcpyAsync(d_center, center, members, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        ScopedTimer t(c, MBAR_TIMER_OTHER);
        e = launch_fill_rows(c->stream, c->u + row0 * c->ld, c->ld, c->N, nrows, (int)B, dbasis, c->ld, d_coeff, d_center, d_off, terms);
    }
    matrix_touched(c);
    // (drained on the error path too: the two blocks must not return to the cache with a copy into them in flight)
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail(c, MBAR_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
    flush_timers(c);
    return MBAR_OK;
}

int mbar_ctx_fill_linear_rows(mbar_ctx* c, int64_t row0, int64_t nrows, int64_t B, const double* basis_host, int64_t ld_host,
                              int64_t col0_host, const double* coeff, const double* offset) {
    const char* who = "mbar_ctx_fill_linear_rows";
    int rc = fill_rows_refused(c, who, row0, nrows, B, basis_host, ld_host, col0_host, coeff);
    if (rc) return rc;
    return fill_rows(c, who, row0, nrows, B, basis_host, ld_host, col0_host, coeff, nullptr, offset, FamilyTerms{});
}

int mbar_ctx_fill_family_rows(mbar_ctx* c, int64_t row0, int64_t nrows, int64_t B, const double* basis_host, int64_t ld_host,
                              int64_t col0_host, const double* coeff, const double* center, const double* offset, const int32_t* kind,
                              const double* period) {
    const char* who = "mbar_ctx_fill_family_rows";
    int rc = fill_rows_refused(c, who, row0, nrows, B, basis_host, ld_host, col0_host, coeff);
    if (rc) return rc;
    FamilyTerms terms{};
    if (kind) {
        rc = family_terms(c, who, B, kind, period, &terms);
        if (rc) return rc;
    }
    if (terms.mask && !center) return fail(c, MBAR_ERR_ARG, "mbar_ctx_fill_family_rows: a family with harmonic terms needs its centres");
    for (int64_t x = 0; x < nrows * B; ++x)
        if (!std::isfinite(coeff[x]) || (terms.mask && !std::isfinite(center[x])))
            return fail(c, MBAR_ERR_ARG, "mbar_ctx_fill_family_rows: the coefficients and the centres must be finite");
    return fill_rows(c, who, row0, nrows, B, basis_host, ld_host, col0_host, coeff, center, offset, terms);
}

int mbar_ctx_download_u(mbar_ctx* c, double* out, int64_t ld_out) {
    if (!c || !out || ld_out < c->N) return fail(c, MBAR_ERR_ARG, "bad argument");
    HIPCHK(c, hipSetDevice(c->device));
    const double* src = c->u;
    if (c->opt_debug_download_p) {  // (tests: the resident probability matrix of the last adaptive solve instead of u)
        if (!c->P || !c->P_valid) return fail(c, MBAR_ERR_STATE, "no resident probability matrix on this context");
        src = c->P;
    }
    HIPCHK(c, hipMemcpy2DAsync(out, (size_t)ld_out * sizeof(double), src, (size_t)c->ld * sizeof(double),
                               (size_t)c->N * sizeof(double), (size_t)c->K, hipMemcpyDeviceToHost, c->stream));
    return sync_stream(c);
}

int mbar_ctx_generate_harmonic(mbar_ctx* c, uint64_t seed, const double* O_k, const double* K_k,
                               const int64_t* N_k_global, int64_t n_global0) {
    if (!c || !O_k || !K_k || !N_k_global) return fail(c, MBAR_ERR_ARG, "NULL argument");
    HIPCHK(c, hipSetDevice(c->device));
    std::vector<int64_t> cum((size_t)c->K + 1, 0);
    for (int64_t k = 0; k < c->K; ++k) cum[k + 1] = cum[k] + N_k_global[k];
    if (n_global0 < 0 || n_global0 + c->N > cum[c->K]) return fail(c, MBAR_ERR_ARG, "shard exceeds sum(N_k)");
    double* dO = d_misc(c);
    double* dK = d_misc(c) + c->Kp;
    int64_t* dC = reinterpret_cast<int64_t*>(d_misc(c) + 2 * c->Kp);
    HIPCHK(c, hipMemcpyAsync(dO, O_k, c->K * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dK, K_k, c->K * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(dC, cum.data(), (c->K + 1) * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    {
        ScopedTimer t(c, MBAR_TIMER_OTHER);
        HIPCHK(c, launch_generate_harmonic(c->stream, c->u, c->ld, c->N, c->K, seed, dO, dK, dC, n_global0));
    }
    matrix_touched(c);
    return sync_stream(c);
}

}  // extern "C"
