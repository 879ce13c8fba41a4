// Host side of libmbar_hip.so, the entry points that take an extension context and its base (mbar_ctx.h lists the files of the
// context layer; mbar_ctx_create_ext is with the other constructor in mbar_capi.cpp): the rows of an extension are appended to a
// resident matrix without a copy of it, and swept together with it.
#include "mbar_ctx.h"

using namespace mbar;
using namespace mbar::host;

extern "C" {

static int ext_pair_ok(mbar_ctx* ext, mbar_ctx* base, const char* who) {
    if (!ext || !base) return fail(ext, MBAR_ERR_ARG, std::string(who) + ": NULL context");
    if (ext->ext_base != base) return fail(ext, MBAR_ERR_ARG, std::string(who) + ": the first context is not an extension of the second");
    return MBAR_OK;
}
// What the two sweeps over an extension begin with: the base's log-denominators at f_base in its slot 0 (its error is the call's,
// with `who` in front), the extension's rows checked; *nan_out: base, f_base or the extension's rows make every output NaN
static int ext_logden(mbar_ctx* ext, mbar_ctx* base, const char* who, const double* f_base, bool* nan_out) {
    HIPCHK(ext, hipSetDevice(ext->device));
    int rc = pass_logden(base, f_base, nan_out);
    if (rc) return fail(ext, rc, std::string(who) + ": " + mbar_last_error(base));
    rc = refresh_poison(ext);
    *nan_out = *nan_out || ext->u_poison;
    return rc;
}

// dst rows = base rows [state_row0 ..) - log(base rows [obs_row0 ..) - shift_r), shift_r = min_r - |4 eps min_r| (mbar.py:827-832)
// handed back: observables that ARE rows of the resident matrix (entropy / enthalpy: the reduced potentials), each at its own
// state, in one read of the rows concerned -- no copy of them, no pass in place
// min_in (or NULL): the minima of the observable rows, as min_out of an earlier call on the same resident rows handed them back --
// the pass that finds them is skipped then; min_out (or NULL) receives them.
int mbar_ctx_rows_obs_from(mbar_ctx* dst, int64_t dst_row0, mbar_ctx* base, int64_t state_row0, int64_t obs_row0, int64_t nrows,
                           double* shift_out, const double* min_in, double* min_out) {
    int rc = ext_pair_ok(dst, base, "mbar_ctx_rows_obs_from");
    if (rc) return rc;
    if (!shift_out) return fail(dst, MBAR_ERR_ARG, "NULL argument");
    if (!rows_in_range(dst, dst_row0, nrows) || !rows_in_range(base, state_row0, nrows) || !rows_in_range(base, obs_row0, nrows))
        return fail(dst, MBAR_ERR_ARG, "row range out of bounds");
    if (nrows == 0) return MBAR_OK;
    HIPCHK(dst, hipSetDevice(dst->device));
    HIPCHK(dst, hipStreamSynchronize(base->stream));
    rc = ensure(dst, dst->scratch, (size_t)nrows * 257);
    if (rc) return rc;
    double* shift_dev = dst->scratch + (size_t)nrows * 256;
    if (min_in) HIPCHK(dst, hipMemcpyAsync(dst->scratch, min_in, (size_t)nrows * sizeof(double), hipMemcpyHostToDevice, dst->stream));
    HIPCHK(dst, launch_rows_obs(dst->stream, dst->u + dst_row0 * dst->ld, base->u + obs_row0 * base->ld, base->u + state_row0 * base->ld,
                                dst->ld, nrows, dst->N, dst->scratch, shift_dev, min_in != nullptr));
    HIPCHK(dst, hipMemcpyAsync(shift_out, shift_dev, (size_t)nrows * sizeof(double), hipMemcpyDeviceToHost, dst->stream));
    matrix_touched(dst);
    rc = sync_stream(dst);
    if (rc) return rc;
    if (min_out) {  // shift = m - |4 eps m|  <=>  m = shift / (1 -+ 4 eps): the minimum itself is what the kernel reduces, so hand back ITS bits
        if (min_in) {
            std::copy(min_in, min_in + nrows, min_out);
        } else {
            // (the partial minima are still in the scratch rows: reduce them on the host, the same fmin)
            const int64_t want = (dst->N + 2047) / 2048;
            const int64_t gx = want < 256 ? (want < 1 ? 1 : want) : 256;
            std::vector<double> part((size_t)nrows * gx);
            HIPCHK(dst, hipMemcpy(part.data(), dst->scratch, part.size() * sizeof(double), hipMemcpyDeviceToHost));
            for (int64_t r = 0; r < nrows; ++r) {
                double m = std::numeric_limits<double>::infinity();
                for (int64_t i = 0; i < gx; ++i) m = std::fmin(m, part[(size_t)r * gx + i]);
                min_out[r] = m;
            }
        }
    }
    return MBAR_OK;
}

// Log normalisers of the extension's rows as unsampled states of the base's mixture at f_base (K_base entries):
// lognum_ext[r] = log sum_n c_n exp(-row_rn - logden_n(f_base)) with the base's log-denominators and sample multiplicities.
int mbar_lognum_ext(mbar_ctx* ext, mbar_ctx* base, const double* f_base, double* lognum_ext) {
    int rc = ext_pair_ok(ext, base, "mbar_lognum_ext");
    if (rc) return rc;
    if (!f_base || !lognum_ext) return fail(ext, MBAR_ERR_ARG, "NULL argument");
    bool nan = false;
    rc = ext_logden(ext, base, "mbar_lognum_ext", f_base, &nan);
    if (rc) return rc;
    if (nan) {
        fill_nan(lognum_ext, ext->K);
        return MBAR_OK;
    }
    std::vector<double> hm, hs;
    rc = lognum_sweep(ext, base, hm, hs);
    if (rc) return rc;
    for (int64_t k = 0; k < ext->K; ++k) lognum_ext[k] = hm[k] + std::log(hs[k]);
    return MBAR_OK;
}

// W^T W of the weight columns of [base rows | extension rows] at (f_base, f_ext): ONE one-read sweep over the two matrices
// (gramW: (K_base + K_ext)^2 row-major; wsum as in mbar_gram_w, with N_k = 0 for the extension's rows).
// gram_base (or NULL): W^T W of the base's own states at f_base (mbar_gram_w of the base: the caller keeps it across calls).  With
// it, and at most 16 appended rows on a base of 128 padded states, only the new entries are computed: a 16 x 128 rectangle between
// the appended block row and the resident panel + the 16 x 16 block of the appended rows (a fifth of the joint sweep's matrix
// instructions; the sweep is then bound by HBM and the operands' exponentials).
int mbar_gram_w_ext(mbar_ctx* ext, mbar_ctx* base, const double* f_base, const double* f_ext, const double* gram_base, double* gramW,
                    double* wsum) {
    int rc = ext_pair_ok(ext, base, "mbar_gram_w_ext");
    if (rc) return rc;
    if (!f_base || !f_ext || !gramW) return fail(ext, MBAR_ERR_ARG, "NULL argument");
    bool nan = false;
    rc = ext_logden(ext, base, "mbar_gram_w_ext", f_base, &nan);
    if (rc) return rc;
    const int64_t Kb = base->K, Ke = ext->K, Kt = Kb + Ke, rows = base->Kp + ext->Kp;
    bool finite = true;
    for (int64_t k = 0; k < Ke; ++k) finite = finite && std::isfinite(f_ext[k]);
    if (nan || !finite) {
        fill_nan(gramW, (size_t)Kt * Kt);
        fill_nan(wsum, Kt);
        return MBAR_OK;
    }
    const int64_t ntiles = (ext->N + TS - 1) / TS;
    // first row of the extension, counted in row pitches from the base's matrix
    const int64_t row_e = (reinterpret_cast<intptr_t>(ext->u) - reinterpret_cast<intptr_t>(base->u)) / (intptr_t)((size_t)base->ld * sizeof(double));
    double* an_dev = ext->small;  // (small_doubles(256) of them)
    const double* logden = base->logden[0];
    // operand constants of the joint panel: f_base, padding, f_ext, padding (-inf: a zero operand); `rows_j`: the panel's rows
    auto operands = [&](int64_t rows_j) {
        std::vector<double> an = padded_operand(f_base, Kb, rows_j);
        std::copy(f_ext, f_ext + Ke, an.begin() + base->Kp);
        return an;
    };
    if (gram_base && Ke <= 16 && base->Kp == 128) {
        // rectangle: I = the appended block row, J = the resident panel; then the appended rows among themselves.  Both launches'
        // records are sized before the first one is queued
        const LaunchGeom g = gram_geometry(144, false, ext->num_cu, ntiles, ext->opt_grid);
        const LaunchGeom gd = gram_geometry(16, true, ext->num_cu, ntiles, ext->opt_grid);
        RecordNeed need;
        need.add(g.nwaves, (size_t)8 * 256);
        need.add(gd.nwaves, 256);
        rc = reserve(ext, need);
        if (!rc) rc = ensure_red(ext, (size_t)9 * 256);
        if (rc) return rc;
        HIPCHK(ext, fold_weights(base, ext->stream, 0.5, logden));  // sum_n c_n p p^T: each operand carries sqrt(c_n), folded into the exponent
        const std::vector<double> an = operands(128 + 16);  // [f_base padded to 128 | f_ext padded to 16]
        HIPCHK(ext, hipMemcpyAsync(an_dev, an.data(), an.size() * sizeof(double), hipMemcpyHostToDevice, ext->stream));
        rc = launch_and_reduce(ext, g.nwaves, (size_t)8 * 256, ext->red, [&]() -> int {
            HIPCHK(ext, launch_gram_thin(ext->stream, g, base->u, base->ld, base->N, an_dev + 128, an_dev, logden, row_e, 0, ext->part));
            return MBAR_OK;
        });
        if (rc) return rc;
        rc = launch_and_reduce(ext, gd.nwaves, 256, ext->red + 8 * 256, [&]() -> int {
            LoopCtl lo;
            HIPCHK(ext, launch_gram_diag(ext->stream, 1, gd, ext->u, ext->ld, ext->N, an_dev + 128, logden, 0, ext->part, nullptr, lo));
            return MBAR_OK;
        });
        if (rc) return rc;
        rc = fetch_red(ext, (size_t)9 * 256);
        if (rc) return rc;
        for (int64_t i = 0; i < Kb; ++i)
            for (int64_t j = 0; j < Kb; ++j) gramW[(size_t)i * Kt + j] = gram_base[(size_t)i * Kb + j];
        for (int64_t r = 0; r < Ke; ++r) {
            for (int64_t j = 0; j < Kb; ++j) {
                const double v = ext->hred[(size_t)(j / 16) * 256 + r * 16 + (j % 16)];  // block (0, J): element (r, q)
                gramW[(size_t)(Kb + r) * Kt + j] = v;
                gramW[(size_t)j * Kt + Kb + r] = v;
            }
            for (int64_t q = 0; q < Ke; ++q) gramW[(size_t)(Kb + r) * Kt + Kb + q] = ext->hred[(size_t)8 * 256 + r * 16 + q];
        }
    } else {
        const int nbt = (int)(rows / 16);
        GramPlan plan = gram_plan(rows, true);
        const size_t total = plan.total_blocks * 256;
        LaunchGeom g = gram_quad_geometry(nbt, ext->num_cu, ntiles, ext->opt_grid);
        // (padding blocks at the END of the joint panel are left out of the sweep like quad_trim does for one matrix)
        g.live_blocks = ext->opt_quad_trim ? (int)((base->Kp + Ke + 15) / 16) : 0;
        RecordNeed need;
        need.add(g.nwaves, total);
        rc = reserve(ext, need);
        if (!rc) rc = ensure_red(ext, total);
        if (rc) return rc;
        const std::vector<double> an = operands(rows);
        HIPCHK(ext, hipMemcpyAsync(an_dev, an.data(), an.size() * sizeof(double), hipMemcpyHostToDevice, ext->stream));
        HIPCHK(ext, fold_weights(base, ext->stream, 0.5, logden));
        rc = launch_and_reduce(ext, g.nwaves, total, ext->red, [&]() -> int {
            HIPCHK(ext, launch_gram_quad_split(ext->stream, nbt, g, base->u, base->ld, base->N, an_dev, logden, ext->part, base->Kp, row_e));
            return MBAR_OK;
        });
        if (rc) return rc;
        rc = fetch_red(ext, total);
        if (rc) return rc;
        std::vector<double> Gp((size_t)rows * rows, 0.0);
        unpack_gram(plan, ext->hred, rows, Gp.data());
        auto src = [&](int64_t k) { return k < Kb ? k : base->Kp + (k - Kb); };
        for (int64_t i = 0; i < Kt; ++i)
            for (int64_t j = 0; j < Kt; ++j) gramW[(size_t)i * Kt + j] = Gp[(size_t)src(i) * rows + src(j)];
    }
    if (wsum) {  // sum_n W_nj with N_k = 0 for the appended rows
        std::vector<double> Nk((size_t)Kt, 0.0);
        for (int64_t k = 0; k < Kb; ++k) Nk[k] = base->Nk[k];
        gram_operand_sums(gramW, Kt, Nk.data(), wsum);
    }
    return MBAR_OK;
}

}  // extern "C"
