// ---- many small MBAR problems (mbar_k_batch.hip; C ABI in mbar_batch.cpp) ----------------------------------------------------
#pragma once
#include "mbar_common.h"

namespace mbar {

// The adaptive loop of mbar_solvers.py:575-640 for one problem as a resumable state machine over mbar_batch_state.  A pass
// evaluates, at each of the nreq requested f vectors, lognum_k = log sum_n exp(-logden_n - u_kn) for every state and, at
// req[gram_req], the Gram matrix sum_n p_ni p_nj (p_nk = N_k W_nk).  batch_advance consumes one pass; when it leaves the state in
// BATCH_PH_NEWTON the caller factors H = diag(psum) - Gram of the live states (batch_newton_* below, or the workgroup-parallel
// version of the step kernel), stores the direction in x and calls it again, which forms the next two candidates.  The same
// function runs in k_batch_step and in mbar_batch_step_host.  The unknowns are the sampled states but the first (the gauge
// state s0 of the reduced problem of mbar_solvers.py:1002-1006); unsampled states keep their f and carry no weight.
enum : int64_t { BATCH_RUNNING = 0, BATCH_DONE = 1, BATCH_FALLBACK = 2 };
enum : int64_t { BATCH_PH_INIT = 0, BATCH_PH_GRAM = 1, BATCH_PH_NEWTON = 2, BATCH_PH_CAND = 3, BATCH_PH_LAST = 4, BATCH_PH_FINAL = 5,
                 BATCH_PH_IDLE = 6 };

MBAR_HD inline int batch_first_sampled(const mbar_batch_state& s) {
    for (int k = 0; k < (int)s.K; ++k)
        if (s.Nk[k] > 0) return k;
    return -1;
}
MBAR_HD inline int batch_sampled_count(const mbar_batch_state& s) {
    int m = 0;
    for (int k = 0; k < (int)s.K; ++k) m += s.Nk[k] > 0;
    return m;
}
// psum of the sampled states from lognum at f
MBAR_HD inline void batch_set_point(mbar_batch_state& s, const double* f, const double* lognum) {
#pragma clang fp contract(off)
    for (int k = 0; k < (int)s.K; ++k) {
        s.f[k] = f[k];
        s.lognum[k] = lognum[k];
        s.psum[k] = s.Nk[k] > 0 ? s.Nk[k] * exp(f[k] + lognum[k]) : 0.0;
    }
}
MBAR_HD inline void batch_end(mbar_batch_state& s, int64_t status, int64_t success) {
    s.status = status;
    s.success = success;
    s.nreq = 0;
    s.gram_req = -1;
    s.phase = BATCH_PH_IDLE;
}
// the pass that evaluates f alone (with its Gram matrix when `gram`)
MBAR_HD inline void batch_request_point(mbar_batch_state& s, bool gram, int64_t phase) {
    for (int k = 0; k < (int)s.K; ++k) s.req[0][k] = s.f[k];
    s.nreq = 1;
    s.gram_req = gram ? 0 : -1;
    s.gram_w = 0;
    s.phase = phase;
}

// lognum: [nreq][K] at the requests of the last pass (unused in BATCH_PH_INIT and BATCH_PH_NEWTON)
MBAR_HD inline int64_t batch_advance(mbar_batch_state& s, const double* lognum) {
#pragma clang fp contract(off)
    if (s.status != BATCH_RUNNING) return s.status;
    const int K = (int)s.K;
    const int s0 = batch_first_sampled(s);
    switch (s.phase) {
    case BATCH_PH_INIT: {
        // gauge of mbar_solvers.py:1003-1006 on the sampled states; one sampled state: no solve, f_s0 = 0
        s.iterations = s.nr_iter = s.sci_iter = s.choices = 0;
        s.success = 0;
        s.newton_bad = 0;
        if (s0 < 0) {
            batch_end(s, BATCH_FALLBACK, 0);
            return s.status;
        }
        const double f0 = s.f[s0];
        for (int k = 0; k < K; ++k)
            if (s.Nk[k] > 0) s.f[k] = s.f[k] - f0;
        if (batch_sampled_count(s) == 1 || s.maxiter <= 0) {
            batch_request_point(s, false, BATCH_PH_LAST);
            return s.status;
        }
        batch_request_point(s, true, BATCH_PH_GRAM);
        return s.status;
    }
    case BATCH_PH_LAST: {
        double f[MBAR_BATCH_MAX_K];
        for (int k = 0; k < K; ++k) f[k] = s.f[k];
        batch_set_point(s, f, lognum);
        batch_end(s, BATCH_DONE, batch_sampled_count(s) == 1 ? 1 : 0);
        return s.status;
    }
    case BATCH_PH_GRAM: {
        double f[MBAR_BATCH_MAX_K];
        for (int k = 0; k < K; ++k) f[k] = s.f[k];
        batch_set_point(s, f, lognum);
        s.phase = BATCH_PH_NEWTON;  // the caller factors H at f with the Gram matrix of this pass
        return s.status;
    }
    case BATCH_PH_NEWTON: {
        if (s.newton_bad) {
            batch_end(s, BATCH_FALLBACK, 0);
            return s.status;
        }
        // f_sci = -lognum, re-zeroed on s0 (mbar_solvers.py:587-588); f_nr = f - gamma (H^+ g - (H^+ g)_s0) (:582-584)
        const double z = -s.lognum[s0];
        for (int k = 0; k < K; ++k) {
            const bool live = s.Nk[k] > 0;
            s.req[0][k] = live ? -s.lognum[k] - z : s.f[k];
            s.req[1][k] = (live && k != s0) ? s.f[k] - s.gamma * s.x[k] : s.f[k];
        }
        s.nreq = 2;
        s.gram_w = 0;
        // the Gram matrix of the candidate that will most likely be accepted: Newton-Raphson, unless self-consistent steps are forced
        s.gram_req = s.sci_iter < s.min_sc_iter ? 0 : 1;
        s.phase = BATCH_PH_CAND;
        return s.status;
    }
    case BATCH_PH_CAND: {
        double gn[2] = {0.0, 0.0};
        for (int r = 0; r < 2; ++r)
            for (int k = 0; k < K; ++k)
                if (s.Nk[k] > 0) {
                    const double g = s.Nk[k] * exp(s.req[r][k] + lognum[r * K + k]) - s.Nk[k];
                    gn[r] = gn[r] + g * g;
                }
        s.gnorm_sci = sqrt(gn[0]);
        s.gnorm_nr = sqrt(gn[1]);
        // mbar_solvers.py:607; a NaN Newton-Raphson candidate loses to a finite self-consistent one
        const bool nan_nr = gn[1] != gn[1] && gn[0] == gn[0];
        const int c = (gn[0] < gn[1] || s.sci_iter < s.min_sc_iter || nan_nr) ? 0 : 1;
        // relative change of :627-633 over the sampled states but s0
        double max_delta = -INFINITY, max_diff = -INFINITY;
        bool nan_seen = false;
        const double zcut = 1e-8 < s.tol ? 1e-8 : s.tol;
        for (int k = 0; k < K; ++k) {
            if (!(s.Nk[k] > 0) || k == s0) continue;
            const double fn = s.req[c][k];
            double div = fabs(fn);
            if (div < zcut) div = 1.0;
            const double d = fabs(fn - s.f[k]) / div;
            const double e = fabs(s.req[0][k] - s.req[1][k]) / div;
            if (d != d) nan_seen = true;
            max_delta = d > max_delta ? d : max_delta;
            max_diff = e > max_diff ? e : max_diff;
        }
        if (nan_seen) max_delta = NAN;  // (np.max propagates NaN)
        s.max_delta = max_delta;
        s.max_diff = max_diff;
        if (c == 0) s.sci_iter += 1;
        else {
            s.nr_iter += 1;
            if (s.iterations < 63) s.choices |= (int64_t)1 << s.iterations;
        }
        s.iterations += 1;
        batch_set_point(s, s.req[c], lognum + c * K);
        if (max_delta != max_delta || (max_delta < s.tol && max_diff < sqrt(s.tol))) {
            batch_end(s, BATCH_DONE, 1);
            return s.status;
        }
        if (s.iterations >= s.maxiter) {
            batch_end(s, BATCH_DONE, 0);
            return s.status;
        }
        // the Gram matrix of this pass is the accepted point's, or close enough to it
        if (c == s.gram_req || max_diff <= 1e-10) {
            s.phase = BATCH_PH_NEWTON;
            return s.status;
        }
        batch_request_point(s, true, BATCH_PH_GRAM);
        return s.status;
    }
    default:
        batch_end(s, BATCH_FALLBACK, 0);
        return s.status;
    }
}

// Mean gradient over the sampled states.  numpy.linalg.lstsq(H, g) (mbar_solvers.py:582) answers for the part of g orthogonal to
// H's null vector 1 only; sum_k g_k is zero up to round-off, and that round-off, solved for in the gauge-fixed system, would move
// the Newton step by (round-off) / (smallest eigenvalue of H).  The right-hand side is therefore g - mean(g) on the sampled states.
MBAR_HD inline double batch_gradient_mean(const mbar_batch_state& s) {
#pragma clang fp contract(off)
    double sum = 0.0;
    int m = 0;
    for (int k = 0; k < (int)s.K; ++k)
        if (s.Nk[k] > 0) {
            sum = sum + (s.psum[k] - s.Nk[k]);
            m += 1;
        }
    return m > 0 ? sum / m : 0.0;
}
// Newton system of the live states (sampled, not s0) in ascending order: A[i * lda + j] = H_ij, b_i = g_i.  H = diag(psum) - G.
// Pivots at or below eps * m * max psum, or not finite, count as zero (the threshold of k_newton).
MBAR_HD inline double batch_pivot_threshold(const mbar_batch_state& s, int m) {
    double pmax = 0.0;
    for (int k = 0; k < (int)s.K; ++k)
        if (s.Nk[k] > 0 && s.psum[k] > pmax) pmax = s.psum[k];
    return pmax * 2.220446049250313e-16 * (double)(m > 0 ? m : 1);
}
// Serial LDL^T in place (lower triangle; A[j][j] <- d_j, A[i][j] <- l_ij) and solve; returns false on a pivot that counts as zero
MBAR_HD inline bool batch_ldlt_solve(double* A, int lda, double* b, int m, double thr) {
#pragma clang fp contract(off)
    for (int j = 0; j < m; ++j) {
        const double d = A[j * lda + j];
        if (!(d > thr) || !(d - d == 0.0)) return false;  // (d - d == 0: finite)
        for (int i = j + 1; i < m; ++i) {
            const double a = A[i * lda + j];
            const double l = a / d;
            for (int k = j + 1; k <= i; ++k) A[i * lda + k] = A[i * lda + k] - l * A[k * lda + j];
        }
        // (the column is scaled after the update: the update above read its unscaled entries)
        for (int i = j + 1; i < m; ++i) A[i * lda + j] = A[i * lda + j] / d;
    }
    for (int j = 0; j < m; ++j)
        for (int i = j + 1; i < m; ++i) b[i] = b[i] - A[i * lda + j] * b[j];
    for (int j = 0; j < m; ++j) b[j] = b[j] / A[j * lda + j];
    for (int j = m - 1; j >= 0; --j)
        for (int i = 0; i < j; ++i) b[i] = b[i] - A[j * lda + i] * b[j];
    return true;
}

// Device side.  Problem p: rows of K[p] states, N[p] samples at u + uoff[p] (row-major, ld N[p]); its chunks cbeg[p] ..
// cbeg[p + 1] of MBAR_BATCH_CHUNK columns each (the last one shorter), chunk c's partial record at part + coff[c]:
// [2][K] maxima, [2][K] scaled sums, [K][K] Gram.  Chunks are launched in four width classes (8, 16, 32, 64 states).
// The same struct describes a set of replica slots (bootstrap replicates): "problem" s is then a slot, uoff[s] and N[s] are those
// of its base problem (the block is shared, nothing is copied), its chunks, partial records and state are its own, and sample n
// counts cw[cwoff[s] + n] times (the weighted instantiation of the evaluation kernel; cw is NULL for the problems themselves).
constexpr int BATCH_WG = 256;
struct BatchData {
    const double* u;
    const int64_t* uoff;     // [P]
    const int64_t* N;        // [P]
    const int64_t* cbeg;     // [P + 1]
    const int* cprob;        // [nchunks]
    const int64_t* cn0;      // [nchunks] first column of the chunk in its problem
    const int64_t* coff;     // [nchunks] offset of the chunk's partial record
    double* part;
    int64_t P, nchunks;
    const double* cw;        // per-sample multiplicities of replica slots, or NULL
    const int64_t* cwoff;    // [P] offset of slot s's multiplicities in cw
};
// evaluation pass over the chunks list[0 .. n) of one width class kb; with d.cw (and d.cwoff) the weighted form: every sum over
// samples becomes sum_n c_n (...)
hipError_t launch_batch_eval(hipStream_t st, int kb, const BatchData& d, const int* list, int64_t n, const mbar_batch_state* states);
// Draw counts of the slots first .. first + count of the replica set d into d.cw (zeroed by the caller): position j of slot s
// draws bootstrap_draw(seed[s], replicate[s], j, n_k) within the run of its state, cum[base[s]][0 .. K] being the runs' bounds
// (rows of MBAR_BATCH_MAX_K + 1).  One workgroup per chunk; chunk0 / nchunk: the chunks of those slots.
hipError_t launch_batch_draw(hipStream_t st, const BatchData& d, int64_t chunk0, int64_t nchunk, const int64_t* base,
                             const int64_t* Kp, const int64_t* cum, const uint64_t* seed, const int64_t* replicate, double* cw);
// merge + one step of every running problem; FINAL problems: out_gram / out_wsum at their packed offsets goff / woff
hipError_t launch_batch_step(hipStream_t st, const BatchData& d, mbar_batch_state* states, int* active, double* out_gram,
                             double* out_wsum, const int64_t* goff, const int64_t* woff);

// Extension rows of the problems (mbar_batch_set_ext): problem p has R[p] rows of N[p] reduced potentials at e + eoff[p] (row-major,
// ld N[p]); its per-row values (f_ext, lognum_ext) are packed at roff[p].  Chunk c's record of the rows' sums is at lpart + lcoff[c]:
// [R] maxima, [R] scaled sums.  f and Nk: rows of MBAR_BATCH_MAX_K per problem; problems with mask[p] == 0 are skipped.
struct BatchExt {
    const double* e;
    const int64_t* eoff;     // [P]
    const int64_t* K;        // [P]
    const int64_t* R;        // [P]
    const int64_t* roff;     // [P]
    const int64_t* lcoff;    // [nchunks]
    double* lpart;
    const double* f;         // [P][MBAR_BATCH_MAX_K]
    const double* Nk;        // [P][MBAR_BATCH_MAX_K]
    const double* fext;      // packed like lognum_ext (the Gram pass only)
    const int32_t* mask;     // [P]
};
// The rows' sums: one workgroup per chunk of d, then one per problem that merges the chunk records in chunk order into
// lognum_ext (device, packed)
hipError_t launch_batch_ext_lognum(hipStream_t st, const BatchData& d, const BatchExt& x, double* lognum_ext);
// The augmented Gram pass over n work items of the width class ab (16, 32, 64, 128 >= K + R): item w is run wrun[w] of problem
// wprob[w] -- the chunks wrun[w] * MBAR_BATCH_EXT_RUN .. of that problem -- and writes the record ((K + R)^2 Gram, K + R column
// sums) at gpart + wgoff[w]
hipError_t launch_batch_ext_gram(hipStream_t st, int ab, const BatchData& d, const BatchExt& x, int64_t n, const int* wprob,
                                 const int* wrun, const int64_t* wgoff, double* gpart);
// Merge of the records of the n problems gprob[0 .. n): problem gprob[q]'s nrun[q] records start at gpart + gbase[q]; the sums, in
// run order, go to ogram + ogoff[p] and owsum + owoff[p]
hipError_t launch_batch_ext_gram_merge(hipStream_t st, const BatchExt& x, int64_t n, const int* gprob, const int64_t* gbase,
                                       const int* nrun, const double* gpart, double* ogram, double* owsum, const int64_t* ogoff,
                                       const int64_t* owoff);

}  // namespace mbar
