// Host side of mbar_batch (include/mbar_hip.h, "many small MBAR problems in one call"): the handle (on the handle layer of
// mbar_ctx.h), which keeps P problems' reduced potentials resident on a device, cut into chunks, and drives their adaptive loops.
// Kernels: mbar_k_batch.hip; the loop's state machine: batch_advance in mbar_internal.h.
#include <cmath>

#include "mbar_ctx.h"

using namespace mbar;
using namespace mbar::host;

namespace {

constexpr int NCLASS = 4;
constexpr int CLASS_K[NCLASS] = {8, 16, 32, 64};

int class_of(int64_t K) {
    for (int i = 0; i < NCLASS; ++i)
        if (K <= CLASS_K[i]) return i;
    return NCLASS - 1;
}

}  // namespace

struct mbar_batch : Handle {
    int64_t P = 0, nchunks = 0;
    std::vector<int64_t> K, N;
    int64_t ngram = 0, nwsum = 0;              // packed sizes of the covariance outputs
    int64_t nclass[NCLASS] = {0, 0, 0, 0};     // chunks per width class
    DevBuf<double> u;                          // the problems' blocks, concatenated
    DevBuf<int64_t> uoff, dN, cbeg, cn0, coff, goff, woff;
    DevBuf<int> cprob;
    DevBuf<int> lists[NCLASS];                 // chunk indices of each width class
    DevBuf<double> part;                       // chunk partial records
    DevBuf<mbar_batch_state> states;           // [P]
    DevBuf<int> active;                        // [P]
    DevBuf<double> ogram, owsum;
};

namespace {

BatchData data_of(const mbar_batch* h) {
    BatchData d{};
    d.u = h->u;
    d.uoff = h->uoff;
    d.N = h->dN;
    d.cbeg = h->cbeg;
    d.cprob = h->cprob;
    d.cn0 = h->cn0;
    d.coff = h->coff;
    d.part = h->part;
    d.P = h->P;
    d.nchunks = h->nchunks;
    return d;
}

int run_pass(mbar_batch* h, const BatchData& d) {
    for (int i = 0; i < NCLASS; ++i) HIPCHK(nullptr, launch_batch_eval(h->stream, CLASS_K[i], d, h->lists[i], h->nclass[i], h->states));
    HIPCHK(nullptr, launch_batch_step(h->stream, d, h->states, h->active, h->ogram, h->owsum, h->goff, h->woff));
    return MBAR_OK;
}

}  // namespace

extern "C" {

int mbar_batch_create(mbar_batch** out, int device, int64_t P, const int64_t* K, const int64_t* N, const double* const* u) {
    if (!out) return bad_arg("out is NULL");
    *out = nullptr;
    if (P < 1 || !K || !N || !u) return bad_arg("need at least one problem");
    if (P > (int64_t)1 << 30) return bad_arg("too many problems");
    std::vector<int64_t> uoff(P), cbeg(P + 1, 0), cn0, coff, goff(P), woff(P);
    std::vector<int> cprob;
    std::vector<int> lists[NCLASS];
    int64_t total = 0, rec = 0, ng = 0, nw = 0;
    for (int64_t p = 0; p < P; ++p) {
        if (K[p] < 1 || K[p] > MBAR_BATCH_MAX_K)
            return bad_arg("problem " + std::to_string(p) + ": K = " + std::to_string(K[p]) + " is outside 1 .. " +
                           std::to_string(MBAR_BATCH_MAX_K));
        if (N[p] < 1) return bad_arg("problem " + std::to_string(p) + ": no samples");
        if (!u[p]) return bad_arg("problem " + std::to_string(p) + ": u is NULL");
        const double* x = u[p];
        for (int64_t i = 0; i < K[p] * N[p]; ++i)
            if (std::isnan(x[i]) || x[i] == -INFINITY) return bad_arg("problem " + std::to_string(p) + ": u_kn holds NaN or -inf");
        uoff[p] = total;
        total += K[p] * N[p];
        goff[p] = ng;
        ng += K[p] * K[p];
        woff[p] = nw;
        nw += K[p];
        const int cls = class_of(K[p]);
        for (int64_t n0 = 0; n0 < N[p]; n0 += MBAR_BATCH_CHUNK) {
            lists[cls].push_back((int)cn0.size());
            cprob.push_back((int)p);
            cn0.push_back(n0);
            coff.push_back(rec);
            rec += 4 * K[p] + K[p] * K[p];
        }
        cbeg[p + 1] = (int64_t)cn0.size();
    }
    if ((int64_t)cn0.size() > ((int64_t)1 << 31) - 1) return bad_arg("too many chunks");
    return create_handle(out, device, [&](mbar_batch* h, const DevInfo&) {
        h->P = P;
        h->nchunks = (int64_t)cn0.size();
        h->K.assign(K, K + P);
        h->N.assign(N, N + P);
        h->ngram = ng;
        h->nwsum = nw;
        size_t free_b = 0, total_b = 0;
        const size_t need = ((size_t)total + (size_t)rec + (size_t)(ng + nw)) * sizeof(double) +
                            (size_t)P * (sizeof(mbar_batch_state) + 64) + (size_t)h->nchunks * 32;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && need > total_b)
            return fail(nullptr, MBAR_ERR_ARG, "the batch needs " + std::to_string(need >> 20) + " MB of device memory; the device has " +
                                                   std::to_string(total_b >> 20) + " MB");
        (void)hipGetLastError();
        HIPCHK(nullptr, h->u.grow((size_t)total));
        HIPCHK(nullptr, h->uoff.grow((size_t)P));
        HIPCHK(nullptr, h->dN.grow((size_t)P));
        HIPCHK(nullptr, h->cbeg.grow((size_t)(P + 1)));
        HIPCHK(nullptr, h->cn0.grow((size_t)h->nchunks));
        HIPCHK(nullptr, h->coff.grow((size_t)h->nchunks));
        HIPCHK(nullptr, h->cprob.grow((size_t)h->nchunks));
        HIPCHK(nullptr, h->goff.grow((size_t)P));
        HIPCHK(nullptr, h->woff.grow((size_t)P));
        HIPCHK(nullptr, h->part.grow((size_t)rec));
        HIPCHK(nullptr, h->states.grow((size_t)P));
        HIPCHK(nullptr, h->active.grow((size_t)P));
        HIPCHK(nullptr, h->ogram.grow((size_t)ng));
        HIPCHK(nullptr, h->owsum.grow((size_t)nw));
        for (int64_t p = 0; p < P; ++p)
            HIPCHK(nullptr, hipMemcpy(h->u + uoff[p], u[p], (size_t)(K[p] * N[p]) * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(nullptr, hipMemcpy(h->uoff, uoff.data(), (size_t)P * sizeof(int64_t), hipMemcpyHostToDevice));
        HIPCHK(nullptr, hipMemcpy(h->dN, N, (size_t)P * sizeof(int64_t), hipMemcpyHostToDevice));
        HIPCHK(nullptr, hipMemcpy(h->cbeg, cbeg.data(), (size_t)(P + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
        HIPCHK(nullptr, hipMemcpy(h->cn0, cn0.data(), cn0.size() * sizeof(int64_t), hipMemcpyHostToDevice));
        HIPCHK(nullptr, hipMemcpy(h->coff, coff.data(), coff.size() * sizeof(int64_t), hipMemcpyHostToDevice));
        HIPCHK(nullptr, hipMemcpy(h->cprob, cprob.data(), cprob.size() * sizeof(int), hipMemcpyHostToDevice));
        HIPCHK(nullptr, hipMemcpy(h->goff, goff.data(), (size_t)P * sizeof(int64_t), hipMemcpyHostToDevice));
        HIPCHK(nullptr, hipMemcpy(h->woff, woff.data(), (size_t)P * sizeof(int64_t), hipMemcpyHostToDevice));
        for (int i = 0; i < NCLASS; ++i) {
            h->nclass[i] = (int64_t)lists[i].size();
            if (lists[i].empty()) continue;
            HIPCHK(nullptr, h->lists[i].grow(lists[i].size()));
            HIPCHK(nullptr, hipMemcpy(h->lists[i], lists[i].data(), lists[i].size() * sizeof(int), hipMemcpyHostToDevice));
        }
        return MBAR_OK;
    });
}

void mbar_batch_destroy(mbar_batch* h) { destroy_handle(h); }

int mbar_batch_solve(mbar_batch* h, mbar_batch_state* states, int64_t* passes) {
    if (!h) return bad_arg("batch is NULL");
    if (!states) return bad_arg("states is NULL");
    int64_t maxit = 0;
    for (int64_t p = 0; p < h->P; ++p) {
        mbar_batch_state& s = states[p];
        if (s.K != h->K[p]) return bad_arg("problem " + std::to_string(p) + ": K of the state differs from the handle's");
        double n = 0.0;
        for (int k = 0; k < (int)s.K; ++k) {
            if (!(s.Nk[k] >= 0) || !std::isfinite(s.f[k])) return bad_arg("problem " + std::to_string(p) + ": bad N_k or f_k");
            n += s.Nk[k];
        }
        if (n != (double)h->N[p]) return bad_arg("problem " + std::to_string(p) + ": N_k does not sum to the number of samples");
        if (!(s.tol > 0) || !std::isfinite(s.gamma)) return bad_arg("problem " + std::to_string(p) + ": bad tol or gamma");
        maxit = std::max(maxit, s.maxiter);
        s.phase = BATCH_PH_INIT;
        s.status = BATCH_RUNNING;
        batch_advance(s, nullptr);  // the first request
    }
    HIPCHK(nullptr, hipSetDevice(h->device));
    const BatchData d = data_of(h);
    HIPCHK(nullptr, hipMemcpyAsync(h->states, states, (size_t)h->P * sizeof(mbar_batch_state), hipMemcpyHostToDevice, h->stream));
    // Passes in groups of 4, 8, 16, 16, ...: between groups the host reads one int per problem.  A finished problem costs one
    // early-exiting workgroup per chunk.  An iteration takes one pass, or two when the speculated Gram matrix was the wrong one.
    const int64_t limit = 2 * maxit + 64;
    std::vector<int> act((size_t)h->P);
    int64_t done = 0;
    int group = 4;
    for (;;) {
        for (int k = 0; k < group; ++k) {
            int rc = run_pass(h, d);
            if (rc) return rc;
        }
        done += group;
        HIPCHK(nullptr, hipMemcpyAsync(act.data(), h->active, act.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(nullptr, hipStreamSynchronize(h->stream));
        bool any = false;
        for (int a : act) any = any || a != 0;
        if (!any) break;
        if (done > limit) return fail(nullptr, MBAR_ERR_NUMERIC, "the adaptive loops did not end within the pass limit");
        group = std::min(16, group * 2);
    }
    HIPCHK(nullptr, hipMemcpyAsync(states, h->states, (size_t)h->P * sizeof(mbar_batch_state), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(nullptr, hipStreamSynchronize(h->stream));
    if (passes) *passes = done;
    return MBAR_OK;
}

int mbar_batch_gram_w(mbar_batch* h, const double* f, const int32_t* mask, double* gram, double* wsum) {
    if (!h) return bad_arg("batch is NULL");
    if (!f || !mask || !gram || !wsum) return bad_arg("f / mask / gram / wsum is NULL");
    std::vector<mbar_batch_state> st((size_t)h->P);
    HIPCHK(nullptr, hipSetDevice(h->device));
    HIPCHK(nullptr, hipMemcpyAsync(st.data(), h->states, st.size() * sizeof(mbar_batch_state), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(nullptr, hipStreamSynchronize(h->stream));
    for (int64_t p = 0; p < h->P; ++p) {
        mbar_batch_state& s = st[p];
        s.nreq = 0;
        s.phase = BATCH_PH_IDLE;
        if (!mask[p]) continue;
        s.K = h->K[p];
        for (int k = 0; k < (int)s.K; ++k) {
            if (!std::isfinite(f[p * MBAR_BATCH_MAX_K + k])) return bad_arg("problem " + std::to_string(p) + ": f is not finite");
            s.req[0][k] = f[p * MBAR_BATCH_MAX_K + k];
        }
        s.phase = BATCH_PH_FINAL;
        s.nreq = 1;
        s.gram_req = 0;
        s.gram_w = 1;
    }
    const BatchData d = data_of(h);
    HIPCHK(nullptr, hipMemcpyAsync(h->states, st.data(), st.size() * sizeof(mbar_batch_state), hipMemcpyHostToDevice, h->stream));
    int rc = run_pass(h, d);
    if (rc) return rc;
    if (h->ngram > 0) HIPCHK(nullptr, hipMemcpyAsync(gram, h->ogram, (size_t)h->ngram * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (h->nwsum > 0) HIPCHK(nullptr, hipMemcpyAsync(wsum, h->owsum, (size_t)h->nwsum * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(nullptr, hipStreamSynchronize(h->stream));
    return MBAR_OK;
}

int mbar_batch_step_host(mbar_batch_state* state, const double* lognum, const double* gram) {
    if (!state) return bad_arg("state is NULL");
    mbar_batch_state& s = *state;
    if (s.K < 1 || s.K > MBAR_BATCH_MAX_K) return bad_arg("K is outside 1 .. 64");
    if (s.phase != BATCH_PH_INIT && s.status == BATCH_RUNNING && s.nreq > 0 && !lognum) return bad_arg("lognum is NULL");
    if (s.status == BATCH_RUNNING && s.phase != BATCH_PH_INIT && s.gram_req >= 0 && !gram) return bad_arg("gram is NULL");
    batch_advance(s, lognum);
    if (s.status == BATCH_RUNNING && s.phase == BATCH_PH_NEWTON) {
        const int K = (int)s.K, s0 = batch_first_sampled(s);
        std::vector<int> idx;
        for (int k = 0; k < K; ++k)
            if (s.Nk[k] > 0 && k != s0) idx.push_back(k);
        const int m = (int)idx.size();
        std::vector<double> A((size_t)m * m), b((size_t)m);
        const double gbar = batch_gradient_mean(s);
        for (int i = 0; i < m; ++i) {
            for (int j = 0; j < m; ++j) A[(size_t)i * m + j] = (i == j ? s.psum[idx[i]] : 0.0) - gram[idx[i] * K + idx[j]];
            b[i] = (s.psum[idx[i]] - s.Nk[idx[i]]) - gbar;
        }
        const bool ok = batch_ldlt_solve(A.data(), m, b.data(), m, batch_pivot_threshold(s, m));
        s.newton_bad = ok ? 0 : 1;
        for (int k = 0; k < K; ++k) s.x[k] = 0.0;
        if (ok)
            for (int i = 0; i < m; ++i) s.x[idx[i]] = b[i];
        batch_advance(s, nullptr);
    }
    return (int)s.status;
}

}  // extern "C"
