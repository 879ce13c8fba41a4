// Host side of mbar_batch (include/mbar_hip.h, "many small MBAR problems in one call"): the handle (on the handle layer of
// mbar_ctx.h), which keeps P problems' reduced potentials resident on a device, cut into chunks, and drives their adaptive loops.
// Replica slots (bootstrap replicates: solves that share a problem's block and weigh its samples by draw counts) are a second
// set of chunks, records and states over the same blocks.  Kernels: mbar_k_batch.hip; the loop's state machine: batch_advance in
// mbar_internal.h.
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

// R replica slots of a batch: what mbar_batch holds per problem, per slot, plus the multiplicities
struct BatchReplicas {
    int64_t R = 0, nchunks = 0, ngram = 0, nwsum = 0, ncw = 0;
    std::vector<int64_t> base, K, N, cwoff_h, cbeg_h;
    int64_t nclass[NCLASS] = {0, 0, 0, 0};
    DevBuf<int64_t> uoff, dN, cbeg, cn0, coff, goff, woff, cwoff, dbase, replicate;
    DevBuf<uint64_t> seed;
    DevBuf<int> cprob;
    DevBuf<int> lists[NCLASS];
    DevBuf<double> part, cw;
    DevBuf<mbar_batch_state> states;
    DevBuf<int> active;
    DevBuf<double> ogram, owsum;               // (made by the first mbar_batch_replicas_gram_w)
    DevBuf<int64_t> cum, dK;                   // per problem: the bounds of the states' runs (MBAR_BATCH_MAX_K + 1 each) and K
};

struct mbar_batch : Handle {
    int64_t P = 0, nchunks = 0;
    std::vector<int64_t> K, N, uoff_h;
    size_t need = 0;                           // device bytes of the problems themselves
    std::unique_ptr<BatchReplicas> rep;
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

// One set of solves over the resident blocks: the problems themselves, or the replica slots
struct BatchView {
    BatchData d;
    const DevBuf<int>* lists;
    const int64_t* nclass;
    mbar_batch_state* states;
    int* active;
    double *ogram, *owsum;
    const int64_t *goff, *woff;
    const std::vector<int64_t>*K, *N;
    int64_t ngram, nwsum;
    const char* what;
};

BatchView view_of(mbar_batch* h) {
    return BatchView{data_of(h), h->lists, h->nclass, h->states, h->active, h->ogram, h->owsum, h->goff, h->woff, &h->K, &h->N,
                     h->ngram, h->nwsum, "problem"};
}

BatchView replica_view_of(mbar_batch* h) {
    BatchReplicas* r = h->rep.get();
    BatchData d{};
    d.u = h->u;
    d.uoff = r->uoff;
    d.N = r->dN;
    d.cbeg = r->cbeg;
    d.cprob = r->cprob;
    d.cn0 = r->cn0;
    d.coff = r->coff;
    d.part = r->part;
    d.P = r->R;
    d.nchunks = r->nchunks;
    d.cw = r->cw;
    d.cwoff = r->cwoff;
    return BatchView{d, r->lists, r->nclass, r->states, r->active, r->ogram, r->owsum, r->goff, r->woff, &r->K, &r->N,
                     r->ngram, r->nwsum, "slot"};
}

int run_pass(mbar_batch* h, const BatchView& v) {
    for (int i = 0; i < NCLASS; ++i) {
        if (v.d.cw) HIPCHK(nullptr, launch_batch_eval_weighted(h->stream, CLASS_K[i], v.d, v.lists[i], v.nclass[i], v.states));
        else HIPCHK(nullptr, launch_batch_eval(h->stream, CLASS_K[i], v.d, v.lists[i], v.nclass[i], v.states));
    }
    HIPCHK(nullptr, launch_batch_step(h->stream, v.d, v.states, v.active, v.ogram, v.owsum, v.goff, v.woff));
    return MBAR_OK;
}

int solve_view(mbar_batch* h, const BatchView& v, mbar_batch_state* states, int64_t* passes) {
    const int64_t P = v.d.P;
    const std::string what = v.what;
    int64_t maxit = 0;
    for (int64_t p = 0; p < P; ++p) {
        mbar_batch_state& s = states[p];
        if (s.K != (*v.K)[p]) return bad_arg(what + " " + std::to_string(p) + ": K of the state differs from the handle's");
        double n = 0.0;
        for (int k = 0; k < (int)s.K; ++k) {
            if (!(s.Nk[k] >= 0) || !std::isfinite(s.f[k])) return bad_arg(what + " " + std::to_string(p) + ": bad N_k or f_k");
            n += s.Nk[k];
        }
        if (n != (double)(*v.N)[p]) return bad_arg(what + " " + std::to_string(p) + ": N_k does not sum to the number of samples");
        if (!(s.tol > 0) || !std::isfinite(s.gamma)) return bad_arg(what + " " + std::to_string(p) + ": bad tol or gamma");
        maxit = std::max(maxit, s.maxiter);
        s.phase = BATCH_PH_INIT;
        s.status = BATCH_RUNNING;
        batch_advance(s, nullptr);  // the first request
    }
    HIPCHK(nullptr, hipSetDevice(h->device));
    HIPCHK(nullptr, hipMemcpyAsync(v.states, states, (size_t)P * sizeof(mbar_batch_state), hipMemcpyHostToDevice, h->stream));
    // Passes in groups of 4, 8, 16, 16, ...: between groups the host reads one int per problem.  A finished problem costs one
    // early-exiting workgroup per chunk.  An iteration takes one pass, or two when the speculated Gram matrix was the wrong one.
    const int64_t limit = 2 * maxit + 64;
    std::vector<int> act((size_t)P);
    int64_t done = 0;
    int group = 4;
    for (;;) {
        for (int k = 0; k < group; ++k) {
            int rc = run_pass(h, v);
            if (rc) return rc;
        }
        done += group;
        HIPCHK(nullptr, hipMemcpyAsync(act.data(), v.active, act.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(nullptr, hipStreamSynchronize(h->stream));
        bool any = false;
        for (int a : act) any = any || a != 0;
        if (!any) break;
        if (done > limit) return fail(nullptr, MBAR_ERR_NUMERIC, "the adaptive loops did not end within the pass limit");
        group = std::min(16, group * 2);
    }
    HIPCHK(nullptr, hipMemcpyAsync(states, v.states, (size_t)P * sizeof(mbar_batch_state), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(nullptr, hipStreamSynchronize(h->stream));
    if (passes) *passes = done;
    return MBAR_OK;
}

int gram_w_view(mbar_batch* h, const BatchView& v, const double* f, const int32_t* mask, double* gram, double* wsum) {
    const int64_t P = v.d.P;
    const std::string what = v.what;
    std::vector<mbar_batch_state> st((size_t)P);
    HIPCHK(nullptr, hipSetDevice(h->device));
    HIPCHK(nullptr, hipMemcpyAsync(st.data(), v.states, st.size() * sizeof(mbar_batch_state), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(nullptr, hipStreamSynchronize(h->stream));
    for (int64_t p = 0; p < P; ++p) {
        mbar_batch_state& s = st[p];
        s.nreq = 0;
        s.phase = BATCH_PH_IDLE;
        if (!mask[p]) continue;
        s.K = (*v.K)[p];
        for (int k = 0; k < (int)s.K; ++k) {
            if (!std::isfinite(f[p * MBAR_BATCH_MAX_K + k])) return bad_arg(what + " " + std::to_string(p) + ": f is not finite");
            s.req[0][k] = f[p * MBAR_BATCH_MAX_K + k];
        }
        s.phase = BATCH_PH_FINAL;
        s.nreq = 1;
        s.gram_req = 0;
        s.gram_w = 1;
    }
    HIPCHK(nullptr, hipMemcpyAsync(v.states, st.data(), st.size() * sizeof(mbar_batch_state), hipMemcpyHostToDevice, h->stream));
    int rc = run_pass(h, v);
    if (rc) return rc;
    if (v.ngram > 0) HIPCHK(nullptr, hipMemcpyAsync(gram, v.ogram, (size_t)v.ngram * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    if (v.nwsum > 0) HIPCHK(nullptr, hipMemcpyAsync(wsum, v.owsum, (size_t)v.nwsum * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(nullptr, hipStreamSynchronize(h->stream));
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
        h->uoff_h = uoff;
        size_t free_b = 0, total_b = 0;
        const size_t need = ((size_t)total + (size_t)rec + (size_t)(ng + nw)) * sizeof(double) +
                            (size_t)P * (sizeof(mbar_batch_state) + 64) + (size_t)h->nchunks * 32;
        h->need = need;
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
    return solve_view(h, view_of(h), states, passes);
}

int mbar_batch_gram_w(mbar_batch* h, const double* f, const int32_t* mask, double* gram, double* wsum) {
    if (!h) return bad_arg("batch is NULL");
    if (!f || !mask || !gram || !wsum) return bad_arg("f / mask / gram / wsum is NULL");
    return gram_w_view(h, view_of(h), f, mask, gram, wsum);
}

int mbar_batch_set_replicas(mbar_batch* h, int64_t R, const int64_t* base, const int64_t* Nk) {
    if (!h) return bad_arg("batch is NULL");
    HIPCHK(nullptr, hipSetDevice(h->device));
    HIPCHK(nullptr, hipStreamSynchronize(h->stream));
    h->rep.reset();
    if (R == 0) return MBAR_OK;
    if (R < 0 || !base || !Nk) return bad_arg("replica slots: need base problems and their N_k");
    if (R > (int64_t)1 << 30) return bad_arg("too many replica slots");
    auto r = std::make_unique<BatchReplicas>();
    r->R = R;
    r->base.assign(base, base + R);
    r->K.resize((size_t)R);
    r->N.resize((size_t)R);
    r->cwoff_h.resize((size_t)R);
    r->cbeg_h.assign((size_t)R + 1, 0);
    std::vector<int64_t> uoff((size_t)R), cn0, coff, goff((size_t)R), woff((size_t)R);
    std::vector<int64_t> cum((size_t)h->P * (MBAR_BATCH_MAX_K + 1), 0);
    std::vector<char> seen((size_t)h->P, 0);
    std::vector<int> cprob;
    std::vector<int> lists[NCLASS];
    int64_t rec = 0, ng = 0, nw = 0, ncw = 0;
    for (int64_t s = 0; s < R; ++s) {
        const int64_t p = base[s];
        if (p < 0 || p >= h->P) return bad_arg("slot " + std::to_string(s) + ": base problem " + std::to_string(p) + " is not in the batch");
        const int64_t K = h->K[p], N = h->N[p];
        if (!seen[p]) {
            int64_t* cm = cum.data() + p * (MBAR_BATCH_MAX_K + 1);
            for (int64_t k = 0; k < K; ++k) {
                if (Nk[p * MBAR_BATCH_MAX_K + k] < 0) return bad_arg("problem " + std::to_string(p) + ": N_k has a negative entry");
                cm[k + 1] = cm[k] + Nk[p * MBAR_BATCH_MAX_K + k];
            }
            if (cm[K] != N) return bad_arg("problem " + std::to_string(p) + ": N_k does not sum to the number of samples");
            seen[p] = 1;
        }
        r->K[s] = K;
        r->N[s] = N;
        uoff[s] = h->uoff_h[p];
        r->cwoff_h[s] = ncw;
        ncw += N;
        goff[s] = ng;
        ng += K * K;
        woff[s] = nw;
        nw += K;
        const int cls = class_of(K);
        for (int64_t n0 = 0; n0 < N; n0 += MBAR_BATCH_CHUNK) {
            lists[cls].push_back((int)cn0.size());
            cprob.push_back((int)s);
            cn0.push_back(n0);
            coff.push_back(rec);
            rec += 4 * K + K * K;
        }
        r->cbeg_h[s + 1] = (int64_t)cn0.size();
        if ((int64_t)cn0.size() > ((int64_t)1 << 31) - 1) return bad_arg("too many replica chunks");
    }
    r->nchunks = (int64_t)cn0.size();
    r->ngram = ng;
    r->nwsum = nw;
    r->ncw = ncw;
    size_t free_b = 0, total_b = 0;
    const size_t need = ((size_t)ncw + (size_t)rec) * sizeof(double) + (size_t)R * (sizeof(mbar_batch_state) + 96) +
                        (size_t)r->nchunks * 32 + cum.size() * sizeof(int64_t);
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && need + h->need > total_b)
        return fail(nullptr, MBAR_ERR_ARG, "the replica slots need " + std::to_string(need >> 20) + " MB of device memory for their "
                    "multiplicities, records and states on top of the batch's " + std::to_string(h->need >> 20) +
                    " MB; the device has " + std::to_string(total_b >> 20) + " MB");
    (void)hipGetLastError();
    HIPCHK(nullptr, r->uoff.grow((size_t)R));
    HIPCHK(nullptr, r->dN.grow((size_t)R));
    HIPCHK(nullptr, r->cbeg.grow((size_t)R + 1));
    HIPCHK(nullptr, r->cn0.grow(cn0.size()));
    HIPCHK(nullptr, r->coff.grow(coff.size()));
    HIPCHK(nullptr, r->cprob.grow(cprob.size()));
    HIPCHK(nullptr, r->goff.grow((size_t)R));
    HIPCHK(nullptr, r->woff.grow((size_t)R));
    HIPCHK(nullptr, r->cwoff.grow((size_t)R));
    HIPCHK(nullptr, r->dbase.grow((size_t)R));
    HIPCHK(nullptr, r->replicate.grow((size_t)R));
    HIPCHK(nullptr, r->seed.grow((size_t)R));
    HIPCHK(nullptr, r->part.grow((size_t)rec));
    HIPCHK(nullptr, r->cw.grow((size_t)ncw));
    HIPCHK(nullptr, r->states.grow((size_t)R));
    HIPCHK(nullptr, r->active.grow((size_t)R));
    HIPCHK(nullptr, r->cum.grow(cum.size()));
    HIPCHK(nullptr, r->dK.grow((size_t)h->P));
    const size_t w = sizeof(int64_t);
    HIPCHK(nullptr, hipMemcpy(r->uoff, uoff.data(), (size_t)R * w, hipMemcpyHostToDevice));
    HIPCHK(nullptr, hipMemcpy(r->dN, r->N.data(), (size_t)R * w, hipMemcpyHostToDevice));
    HIPCHK(nullptr, hipMemcpy(r->cbeg, r->cbeg_h.data(), ((size_t)R + 1) * w, hipMemcpyHostToDevice));
    HIPCHK(nullptr, hipMemcpy(r->cn0, cn0.data(), cn0.size() * w, hipMemcpyHostToDevice));
    HIPCHK(nullptr, hipMemcpy(r->coff, coff.data(), coff.size() * w, hipMemcpyHostToDevice));
    HIPCHK(nullptr, hipMemcpy(r->cprob, cprob.data(), cprob.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPCHK(nullptr, hipMemcpy(r->goff, goff.data(), (size_t)R * w, hipMemcpyHostToDevice));
    HIPCHK(nullptr, hipMemcpy(r->woff, woff.data(), (size_t)R * w, hipMemcpyHostToDevice));
    HIPCHK(nullptr, hipMemcpy(r->cwoff, r->cwoff_h.data(), (size_t)R * w, hipMemcpyHostToDevice));
    HIPCHK(nullptr, hipMemcpy(r->dbase, base, (size_t)R * w, hipMemcpyHostToDevice));
    HIPCHK(nullptr, hipMemcpy(r->cum, cum.data(), cum.size() * w, hipMemcpyHostToDevice));
    HIPCHK(nullptr, hipMemcpy(r->dK, h->K.data(), (size_t)h->P * w, hipMemcpyHostToDevice));
    for (int i = 0; i < NCLASS; ++i) {
        r->nclass[i] = (int64_t)lists[i].size();
        if (lists[i].empty()) continue;
        HIPCHK(nullptr, r->lists[i].grow(lists[i].size()));
        HIPCHK(nullptr, hipMemcpy(r->lists[i], lists[i].data(), lists[i].size() * sizeof(int), hipMemcpyHostToDevice));
    }
    // every slot starts as the plain data: c_n = 1
    HIPCHK(nullptr, launch_fill(h->stream, r->cw, 1.0, ncw));
    HIPCHK(nullptr, hipStreamSynchronize(h->stream));
    h->rep = std::move(r);
    return MBAR_OK;
}

int mbar_batch_replica_set_weights(mbar_batch* h, int64_t slot, const double* c_n) {
    if (!h) return bad_arg("batch is NULL");
    if (!h->rep) return bad_arg("mbar_batch_replica_set_weights: no replica slots (mbar_batch_set_replicas first)");
    BatchReplicas* r = h->rep.get();
    if (slot < 0 || slot >= r->R) return bad_arg("mbar_batch_replica_set_weights: slot " + std::to_string(slot) + " of " + std::to_string(r->R));
    if (!c_n) return bad_arg("mbar_batch_replica_set_weights: c_n is NULL");
    const int64_t N = r->N[slot];
    for (int64_t i = 0; i < N; ++i)
        if (!(c_n[i] >= 0.0) || !std::isfinite(c_n[i]))
            return bad_arg("mbar_batch_replica_set_weights: sample weights must be finite and >= 0");
    HIPCHK(nullptr, hipSetDevice(h->device));
    HIPCHK(nullptr, hipMemcpyAsync(r->cw + r->cwoff_h[slot], c_n, (size_t)N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(nullptr, hipStreamSynchronize(h->stream));
    return MBAR_OK;
}

int mbar_batch_replicas_draw(mbar_batch* h, int64_t first, int64_t count, const uint64_t* seed, const int64_t* replicate) {
    if (!h) return bad_arg("batch is NULL");
    if (!h->rep) return bad_arg("mbar_batch_replicas_draw: no replica slots (mbar_batch_set_replicas first)");
    BatchReplicas* r = h->rep.get();
    if (first < 0 || count < 0 || first + count > r->R) return bad_arg("mbar_batch_replicas_draw: slots outside 0 .. " + std::to_string(r->R));
    if (count == 0) return MBAR_OK;
    if (!seed || !replicate) return bad_arg("mbar_batch_replicas_draw: seed / replicate is NULL");
    for (int64_t i = 0; i < count; ++i)
        if (replicate[i] < 0) return bad_arg("mbar_batch_replicas_draw: negative replicate");
    HIPCHK(nullptr, hipSetDevice(h->device));
    HIPCHK(nullptr, hipMemcpyAsync(r->seed + first, seed, (size_t)count * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(nullptr, hipMemcpyAsync(r->replicate + first, replicate, (size_t)count * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    const int64_t w0 = r->cwoff_h[first], w1 = first + count < r->R ? r->cwoff_h[first + count] : r->ncw;
    HIPCHK(nullptr, hipMemsetAsync(r->cw + w0, 0, (size_t)(w1 - w0) * sizeof(double), h->stream));
    const BatchView v = replica_view_of(h);
    HIPCHK(nullptr, launch_batch_draw(h->stream, v.d, r->cbeg_h[first], r->cbeg_h[first + count] - r->cbeg_h[first], r->dbase, r->dK,
                                      r->cum, r->seed, r->replicate, r->cw));
    HIPCHK(nullptr, hipStreamSynchronize(h->stream));  // (seed / replicate are the caller's again)
    return MBAR_OK;
}

int mbar_batch_replicas_solve(mbar_batch* h, mbar_batch_state* states, int64_t* passes) {
    if (!h) return bad_arg("batch is NULL");
    if (!h->rep) return bad_arg("mbar_batch_replicas_solve: no replica slots (mbar_batch_set_replicas first)");
    if (!states) return bad_arg("states is NULL");
    return solve_view(h, replica_view_of(h), states, passes);
}

int mbar_batch_replicas_gram_w(mbar_batch* h, const double* f, const int32_t* mask, double* gram, double* wsum) {
    if (!h) return bad_arg("batch is NULL");
    if (!h->rep) return bad_arg("mbar_batch_replicas_gram_w: no replica slots (mbar_batch_set_replicas first)");
    if (!f || !mask || !gram || !wsum) return bad_arg("f / mask / gram / wsum is NULL");
    BatchReplicas* r = h->rep.get();
    HIPCHK(nullptr, hipSetDevice(h->device));
    HIPCHK(nullptr, r->ogram.grow((size_t)r->ngram));
    HIPCHK(nullptr, r->owsum.grow((size_t)r->nwsum));
    return gram_w_view(h, replica_view_of(h), f, mask, gram, wsum);
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
