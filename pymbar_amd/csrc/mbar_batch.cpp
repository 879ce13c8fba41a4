// Host side of mbar_batch (include/mbar_hip.h, "many small MBAR problems in one call"): the handle (on the handle layer of
// mbar_handle.h), which keeps P problems' reduced potentials resident on a device, cut into chunks, and drives their adaptive loops.
// Replica slots (bootstrap replicates: solves that share a problem's block and weigh its samples by draw counts) are a second
// set of chunks, records and states over the same blocks.  Extension rows (the expectation family: new states and observables as
// states with no samples) lie next to the blocks, with the two passes over them.  Kernels: mbar_k_batch.hip; the loop's state
// machine: batch_advance in mbar_batch.h.
#include <cmath>
#include <memory>

#include "mbar_handle.h"
#include "mbar_batch.h"

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

// One set of solves over the resident blocks: the problems themselves, or the replica slots.  Entry e has K[e] states and N[e]
// samples, the chunks cbeg_h[e] .. cbeg_h[e + 1], its own partial records and state, and its packed covariance outputs.
struct BatchSet {
    int64_t count = 0, nchunks = 0;
    int64_t ngram = 0, nwsum = 0;              // packed sizes of the covariance outputs
    std::vector<int64_t> K, N, cbeg_h, cwoff_h;
    int64_t nclass[NCLASS] = {0, 0, 0, 0};     // chunks per width class
    DevBuf<int64_t> uoff, dN, cbeg, cn0, coff, goff, woff;
    DevBuf<int> cprob;
    DevBuf<int> lists[NCLASS];                 // chunk indices of each width class
    DevBuf<double> part;                       // chunk partial records
    DevBuf<mbar_batch_state> states;           // [count]
    DevBuf<int> active;                        // [count]
    DevBuf<double> ogram, owsum;
    DevBuf<double> cw;                         // per-sample multiplicities, entry e's at cwoff_h[e] (slots only: empty for the
    DevBuf<int64_t> cwoff;                     // problems, whose samples count once)
};

// R replica slots of a batch: a set, plus what only slots have -- their base problems and the draws of their multiplicities
struct BatchReplicas : BatchSet {
    int64_t ncw = 0;
    std::vector<int64_t> base;
    DevBuf<int64_t> dbase, replicate;
    DevBuf<uint64_t> seed;
    DevBuf<int64_t> cum, dK;                   // per problem: the bounds of the states' runs (MBAR_BATCH_MAX_K + 1 each) and K
};

// Extension rows of the problems (the expectation family): the rows, the chunk records of their sums, the arguments of a pass and
// the packed outputs of the augmented Gram pass
struct BatchExtRows {
    int64_t nrows = 0, ngram = 0, nwsum = 0;   // sum of R, of (K + R)^2, of K + R
    std::vector<int64_t> R, roff_h, ogoff_h, owoff_h;
    DevBuf<double> e, lpart, f, Nk, fext, olognum, gpart, ogram, owsum;
    DevBuf<int64_t> eoff, dK, dR, roff, lcoff, ogoff, owoff, wgoff, gbase;
    DevBuf<int32_t> mask;
    DevBuf<int> wprob, wrun, gprob, nrun;
};

struct mbar_batch : Handle {
    std::vector<int64_t> uoff_h;
    size_t need = 0;                           // device bytes of the problems themselves
    DevBuf<double> u;                          // the problems' blocks, concatenated
    BatchSet prob;
    std::unique_ptr<BatchReplicas> rep;
    std::unique_ptr<BatchExtRows> ext;
};

namespace {

// The tables of a set's layout that only the device reads, between build_layout and upload_layout
struct SetTables {
    std::vector<int64_t> uoff, cn0, coff, goff, woff;
    std::vector<int> cprob;
    std::vector<int> lists[NCLASS];
    int64_t rec = 0;                           // doubles of the partial records
};

// The layout of a set of K.size() entries, entry e with K[e] states and N[e] samples at the block offset uoff[e]: its chunks
// of MBAR_BATCH_CHUNK columns, each in the list of its width class and with a partial record, and the packed output offsets.
// false: more chunks than an int indexes.
bool build_layout(BatchSet& s, SetTables& t, std::vector<int64_t> K, std::vector<int64_t> N, std::vector<int64_t> uoff) {
    s.count = (int64_t)K.size();
    s.cbeg_h.assign(K.size() + 1, 0);
    t.goff.resize(K.size());
    t.woff.resize(K.size());
    for (int64_t e = 0; e < s.count; ++e) {
        t.goff[e] = s.ngram;
        s.ngram += K[e] * K[e];
        t.woff[e] = s.nwsum;
        s.nwsum += K[e];
        const int cls = class_of(K[e]);
        for (int64_t n0 = 0; n0 < N[e]; n0 += MBAR_BATCH_CHUNK) {
            t.lists[cls].push_back((int)t.cn0.size());
            t.cprob.push_back((int)e);
            t.cn0.push_back(n0);
            t.coff.push_back(t.rec);
            t.rec += 4 * K[e] + K[e] * K[e];
        }
        s.cbeg_h[e + 1] = (int64_t)t.cn0.size();
        if ((int64_t)t.cn0.size() > ((int64_t)1 << 31) - 1) return false;
    }
    s.nchunks = (int64_t)t.cn0.size();
    for (int i = 0; i < NCLASS; ++i) s.nclass[i] = (int64_t)t.lists[i].size();
    s.K = std::move(K);
    s.N = std::move(N);
    t.uoff = std::move(uoff);
    return true;
}

int upload_layout(BatchSet& s, const SetTables& t) {
    const size_t n = (size_t)s.count;
    HIPCHK(nullptr, s.uoff.upload(t.uoff.data(), n));
    HIPCHK(nullptr, s.dN.upload(s.N.data(), n));
    HIPCHK(nullptr, s.cbeg.upload(s.cbeg_h.data(), n + 1));
    HIPCHK(nullptr, s.cn0.upload(t.cn0.data(), t.cn0.size()));
    HIPCHK(nullptr, s.coff.upload(t.coff.data(), t.coff.size()));
    HIPCHK(nullptr, s.cprob.upload(t.cprob.data(), t.cprob.size()));
    HIPCHK(nullptr, s.goff.upload(t.goff.data(), n));
    HIPCHK(nullptr, s.woff.upload(t.woff.data(), n));
    HIPCHK(nullptr, s.part.grow((size_t)t.rec));
    HIPCHK(nullptr, s.states.grow(n));
    HIPCHK(nullptr, s.active.grow(n));
    for (int i = 0; i < NCLASS; ++i)
        if (!t.lists[i].empty()) HIPCHK(nullptr, s.lists[i].upload(t.lists[i].data(), t.lists[i].size()));
    return MBAR_OK;
}

BatchData data(const BatchSet& s, const double* u) {
    BatchData d{};
    d.u = u;
    d.uoff = s.uoff;
    d.N = s.dN;
    d.cbeg = s.cbeg;
    d.cprob = s.cprob;
    d.cn0 = s.cn0;
    d.coff = s.coff;
    d.part = s.part;
    d.P = s.count;
    d.nchunks = s.nchunks;
    d.cw = s.cw;
    d.cwoff = s.cwoff;
    return d;
}

int run_pass(mbar_batch* h, BatchSet& s) {
    const BatchData d = data(s, h->u);
    for (int i = 0; i < NCLASS; ++i) HIPCHK(nullptr, launch_batch_eval(h->stream, CLASS_K[i], d, s.lists[i], s.nclass[i], s.states));
    HIPCHK(nullptr, launch_batch_step(h->stream, d, s.states, s.active, s.ogram, s.owsum, s.goff, s.woff));
    return MBAR_OK;
}

// `what`: the noun of an entry in the messages ("problem" / "slot")
int solve_set(mbar_batch* h, BatchSet& v, const std::string& what, mbar_batch_state* states, int64_t* passes) {
    int64_t maxit = 0;
    for (int64_t p = 0; p < v.count; ++p) {
        mbar_batch_state& s = states[p];
        if (s.K != v.K[p]) return bad_arg(what + " " + std::to_string(p) + ": K of the state differs from the handle's");
        double n = 0.0;
        for (int k = 0; k < (int)s.K; ++k) {
            if (!(s.Nk[k] >= 0) || !std::isfinite(s.f[k])) return bad_arg(what + " " + std::to_string(p) + ": bad N_k or f_k");
            n += s.Nk[k];
        }
        if (n != (double)v.N[p]) return bad_arg(what + " " + std::to_string(p) + ": N_k does not sum to the number of samples");
        if (!(s.tol > 0) || !std::isfinite(s.gamma)) return bad_arg(what + " " + std::to_string(p) + ": bad tol or gamma");
        maxit = std::max(maxit, s.maxiter);
        s.phase = BATCH_PH_INIT;
        s.status = BATCH_RUNNING;
        batch_advance(s, nullptr);  // the first request
    }
    HIPCHK(nullptr, hipSetDevice(h->device));
    // An iteration takes one pass, or two when the speculated Gram matrix was the wrong one.
    const int64_t limit = 2 * maxit + 64;
    return run_passes(h->stream, states, v.states.p, v.active.p, v.count, limit, "the adaptive loops did not end within the pass limit",
                      passes, [&] { return run_pass(h, v); });
}

int gram_w_set(mbar_batch* h, BatchSet& v, const std::string& what, const double* f, const int32_t* mask, double* gram,
               double* wsum) {
    std::vector<mbar_batch_state> st((size_t)v.count);
    HIPCHK(nullptr, hipSetDevice(h->device));
    HIPCHK(nullptr, v.ogram.grow((size_t)v.ngram));  // (the problems' are made by mbar_batch_create, the slots' here)
    HIPCHK(nullptr, v.owsum.grow((size_t)v.nwsum));
    HIPCHK(nullptr, hipMemcpyAsync(st.data(), v.states, st.size() * sizeof(mbar_batch_state), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(nullptr, hipStreamSynchronize(h->stream));
    for (int64_t p = 0; p < v.count; ++p) {
        mbar_batch_state& s = st[p];
        s.nreq = 0;
        s.phase = BATCH_PH_IDLE;
        if (!mask[p]) continue;
        s.K = v.K[p];
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
    std::vector<int64_t> uoff(P);
    int64_t total = 0;
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
    }
    BatchSet set;
    SetTables t;
    if (!build_layout(set, t, std::vector<int64_t>(K, K + P), std::vector<int64_t>(N, N + P), std::move(uoff)))
        return bad_arg("too many chunks");
    return create_handle(out, device, [&](mbar_batch* h, const DevInfo&) {
        h->prob = std::move(set);
        BatchSet& s = h->prob;
        h->uoff_h = t.uoff;
        size_t free_b = 0, total_b = 0;
        const size_t need = ((size_t)total + (size_t)t.rec + (size_t)(s.ngram + s.nwsum)) * sizeof(double) +
                            (size_t)P * (sizeof(mbar_batch_state) + 64) + (size_t)s.nchunks * 32;
        h->need = need;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && need > total_b)
            return fail(nullptr, MBAR_ERR_ARG, "the batch needs " + std::to_string(need >> 20) + " MB of device memory; the device has " +
                                                   std::to_string(total_b >> 20) + " MB");
        (void)hipGetLastError();
        HIPCHK(nullptr, h->u.grow((size_t)total));
        int rc = upload_layout(s, t);
        if (rc) return rc;
        HIPCHK(nullptr, s.ogram.grow((size_t)s.ngram));
        HIPCHK(nullptr, s.owsum.grow((size_t)s.nwsum));
        for (int64_t p = 0; p < P; ++p)
            HIPCHK(nullptr, hipMemcpy(h->u + t.uoff[p], u[p], (size_t)(K[p] * N[p]) * sizeof(double), hipMemcpyHostToDevice));
        return MBAR_OK;
    });
}

void mbar_batch_destroy(mbar_batch* h) { destroy_handle(h); }

int mbar_batch_solve(mbar_batch* h, mbar_batch_state* states, int64_t* passes) {
    if (!h) return bad_arg("batch is NULL");
    if (!states) return bad_arg("states is NULL");
    return solve_set(h, h->prob, "problem", states, passes);
}

int mbar_batch_gram_w(mbar_batch* h, const double* f, const int32_t* mask, double* gram, double* wsum) {
    if (!h) return bad_arg("batch is NULL");
    if (!f || !mask || !gram || !wsum) return bad_arg("f / mask / gram / wsum is NULL");
    return gram_w_set(h, h->prob, "problem", f, mask, gram, wsum);
}

int mbar_batch_set_replicas(mbar_batch* h, int64_t R, const int64_t* base, const int64_t* Nk) {
    if (!h) return bad_arg("batch is NULL");
    HIPCHK(nullptr, hipSetDevice(h->device));
    HIPCHK(nullptr, hipStreamSynchronize(h->stream));
    h->rep.reset();
    if (R == 0) return MBAR_OK;
    if (R < 0 || !base || !Nk) return bad_arg("replica slots: need base problems and their N_k");
    if (R > (int64_t)1 << 30) return bad_arg("too many replica slots");
    const int64_t P = h->prob.count;
    auto r = std::make_unique<BatchReplicas>();
    r->base.assign(base, base + R);
    r->cwoff_h.resize((size_t)R);
    std::vector<int64_t> K((size_t)R), N((size_t)R), uoff((size_t)R);
    std::vector<int64_t> cum((size_t)P * (MBAR_BATCH_MAX_K + 1), 0);
    std::vector<char> seen((size_t)P, 0);
    for (int64_t s = 0; s < R; ++s) {
        const int64_t p = base[s];
        if (p < 0 || p >= P) return bad_arg("slot " + std::to_string(s) + ": base problem " + std::to_string(p) + " is not in the batch");
        K[s] = h->prob.K[p];
        N[s] = h->prob.N[p];
        if (!seen[p]) {
            int64_t* cm = cum.data() + p * (MBAR_BATCH_MAX_K + 1);
            for (int64_t k = 0; k < K[s]; ++k) {
                if (Nk[p * MBAR_BATCH_MAX_K + k] < 0) return bad_arg("problem " + std::to_string(p) + ": N_k has a negative entry");
                cm[k + 1] = cm[k] + Nk[p * MBAR_BATCH_MAX_K + k];
            }
            if (cm[K[s]] != N[s]) return bad_arg("problem " + std::to_string(p) + ": N_k does not sum to the number of samples");
            seen[p] = 1;
        }
        uoff[s] = h->uoff_h[p];
        r->cwoff_h[s] = r->ncw;
        r->ncw += N[s];
    }
    SetTables t;
    if (!build_layout(*r, t, std::move(K), std::move(N), std::move(uoff))) return bad_arg("too many replica chunks");
    size_t free_b = 0, total_b = 0;
    const size_t need = ((size_t)r->ncw + (size_t)t.rec) * sizeof(double) + (size_t)R * (sizeof(mbar_batch_state) + 96) +
                        (size_t)r->nchunks * 32 + cum.size() * sizeof(int64_t);
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && need + h->need > total_b)
        return fail(nullptr, MBAR_ERR_ARG, "the replica slots need " + std::to_string(need >> 20) + " MB of device memory for their "
                    "multiplicities, records and states on top of the batch's " + std::to_string(h->need >> 20) +
                    " MB; the device has " + std::to_string(total_b >> 20) + " MB");
    (void)hipGetLastError();
    int rc = upload_layout(*r, t);
    if (rc) return rc;
    HIPCHK(nullptr, r->cwoff.upload(r->cwoff_h.data(), (size_t)R));
    HIPCHK(nullptr, r->dbase.upload(base, (size_t)R));
    HIPCHK(nullptr, r->cum.upload(cum.data(), cum.size()));
    HIPCHK(nullptr, r->dK.upload(h->prob.K.data(), (size_t)P));
    HIPCHK(nullptr, r->replicate.grow((size_t)R));
    HIPCHK(nullptr, r->seed.grow((size_t)R));
    HIPCHK(nullptr, r->cw.grow((size_t)r->ncw));
    // every slot starts as the plain data: c_n = 1
    HIPCHK(nullptr, launch_fill(h->stream, r->cw, 1.0, r->ncw));
    HIPCHK(nullptr, hipStreamSynchronize(h->stream));
    h->rep = std::move(r);
    return MBAR_OK;
}

int mbar_batch_replica_set_weights(mbar_batch* h, int64_t slot, const double* c_n) {
    if (!h) return bad_arg("batch is NULL");
    if (!h->rep) return bad_arg("mbar_batch_replica_set_weights: no replica slots (mbar_batch_set_replicas first)");
    BatchReplicas* r = h->rep.get();
    if (slot < 0 || slot >= r->count)
        return bad_arg("mbar_batch_replica_set_weights: slot " + std::to_string(slot) + " of " + std::to_string(r->count));
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
    if (first < 0 || count < 0 || first + count > r->count)
        return bad_arg("mbar_batch_replicas_draw: slots outside 0 .. " + std::to_string(r->count));
    if (count == 0) return MBAR_OK;
    if (!seed || !replicate) return bad_arg("mbar_batch_replicas_draw: seed / replicate is NULL");
    for (int64_t i = 0; i < count; ++i)
        if (replicate[i] < 0) return bad_arg("mbar_batch_replicas_draw: negative replicate");
    HIPCHK(nullptr, hipSetDevice(h->device));
    HIPCHK(nullptr, hipMemcpyAsync(r->seed + first, seed, (size_t)count * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(nullptr, hipMemcpyAsync(r->replicate + first, replicate, (size_t)count * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    const int64_t w0 = r->cwoff_h[first], w1 = first + count < r->count ? r->cwoff_h[first + count] : r->ncw;
    HIPCHK(nullptr, hipMemsetAsync(r->cw + w0, 0, (size_t)(w1 - w0) * sizeof(double), h->stream));
    HIPCHK(nullptr, launch_batch_draw(h->stream, data(*r, h->u), r->cbeg_h[first], r->cbeg_h[first + count] - r->cbeg_h[first],
                                      r->dbase, r->dK, r->cum, r->seed, r->replicate, r->cw));
    HIPCHK(nullptr, hipStreamSynchronize(h->stream));  // (seed / replicate are the caller's again)
    return MBAR_OK;
}

int mbar_batch_replicas_solve(mbar_batch* h, mbar_batch_state* states, int64_t* passes) {
    if (!h) return bad_arg("batch is NULL");
    if (!h->rep) return bad_arg("mbar_batch_replicas_solve: no replica slots (mbar_batch_set_replicas first)");
    if (!states) return bad_arg("states is NULL");
    return solve_set(h, *h->rep, "slot", states, passes);
}

int mbar_batch_replicas_gram_w(mbar_batch* h, const double* f, const int32_t* mask, double* gram, double* wsum) {
    if (!h) return bad_arg("batch is NULL");
    if (!h->rep) return bad_arg("mbar_batch_replicas_gram_w: no replica slots (mbar_batch_set_replicas first)");
    if (!f || !mask || !gram || !wsum) return bad_arg("f / mask / gram / wsum is NULL");
    return gram_w_set(h, *h->rep, "slot", f, mask, gram, wsum);
}

int mbar_batch_set_ext(mbar_batch* h, const int64_t* R, const double* const* e) {
    if (!h) return bad_arg("batch is NULL");
    HIPCHK(nullptr, hipSetDevice(h->device));
    HIPCHK(nullptr, hipStreamSynchronize(h->stream));
    if (!R) {
        h->ext.reset();
        return MBAR_OK;
    }
    const BatchSet& s = h->prob;
    const int64_t P = s.count;
    auto x = std::make_unique<BatchExtRows>();
    x->R.assign((size_t)P, 0);
    x->roff_h.resize((size_t)P);
    x->ogoff_h.resize((size_t)P);
    x->owoff_h.resize((size_t)P);
    std::vector<int64_t> eoff((size_t)P), lcoff((size_t)s.nchunks);
    int64_t total = 0, lrec = 0;
    for (int64_t p = 0; p < P; ++p) {
        const int64_t r = R[p];
        if (r < 0 || s.K[p] + r > MBAR_BATCH_MAX_AUG)
            return bad_arg("problem " + std::to_string(p) + ": K + extension rows = " + std::to_string(s.K[p] + r) + " is outside " +
                           std::to_string(s.K[p]) + " .. " + std::to_string(MBAR_BATCH_MAX_AUG));
        if (r > 0) {
            if (!e || !e[p]) return bad_arg("problem " + std::to_string(p) + ": extension rows are NULL");
            const double* v = e[p];
            for (int64_t i = 0; i < r * s.N[p]; ++i)
                if (std::isnan(v[i]) || v[i] == -INFINITY)
                    return bad_arg("problem " + std::to_string(p) + ": extension rows hold NaN or -inf");
        }
        x->R[p] = r;
        x->roff_h[p] = x->nrows;
        x->nrows += r;
        x->ogoff_h[p] = x->ngram;
        x->ngram += (s.K[p] + r) * (s.K[p] + r);
        x->owoff_h[p] = x->nwsum;
        x->nwsum += s.K[p] + r;
        eoff[p] = total;
        total += r * s.N[p];
        for (int64_t c = s.cbeg_h[p]; c < s.cbeg_h[p + 1]; ++c) {
            lcoff[c] = lrec;
            lrec += 2 * r;
        }
    }
    size_t free_b = 0, total_b = 0;
    const size_t need = ((size_t)total + (size_t)lrec + 2 * (size_t)x->nrows + (size_t)(x->ngram + x->nwsum) +
                         2 * (size_t)P * MBAR_BATCH_MAX_K) * sizeof(double) + (size_t)P * 64 + (size_t)s.nchunks * 8;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && need + h->need > total_b)
        return fail(nullptr, MBAR_ERR_ARG, "the extension rows need " + std::to_string(need >> 20) + " MB of device memory for " +
                    std::to_string(x->nrows) + " rows, their chunk records and outputs on top of the batch's " +
                    std::to_string(h->need >> 20) + " MB; the device has " + std::to_string(total_b >> 20) + " MB");
    (void)hipGetLastError();
    h->ext.reset();  // (the new rows passed every check: only now do the earlier ones go)
    HIPCHK(nullptr, x->e.grow((size_t)std::max<int64_t>(total, 1)));  // (a batch may have no rows at all: the passes still run)
    for (int64_t p = 0; p < P; ++p)
        if (x->R[p] > 0)
            HIPCHK(nullptr, hipMemcpy(x->e + eoff[p], e[p], (size_t)(x->R[p] * s.N[p]) * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(nullptr, x->eoff.upload(eoff.data(), (size_t)P));
    HIPCHK(nullptr, x->dK.upload(s.K.data(), (size_t)P));
    HIPCHK(nullptr, x->dR.upload(x->R.data(), (size_t)P));
    HIPCHK(nullptr, x->roff.upload(x->roff_h.data(), (size_t)P));
    HIPCHK(nullptr, x->lcoff.upload(lcoff.data(), lcoff.size()));
    HIPCHK(nullptr, x->ogoff.upload(x->ogoff_h.data(), (size_t)P));
    HIPCHK(nullptr, x->owoff.upload(x->owoff_h.data(), (size_t)P));
    HIPCHK(nullptr, x->lpart.grow((size_t)std::max<int64_t>(lrec, 1)));
    HIPCHK(nullptr, x->f.grow((size_t)P * MBAR_BATCH_MAX_K));
    HIPCHK(nullptr, x->Nk.grow((size_t)P * MBAR_BATCH_MAX_K));
    HIPCHK(nullptr, x->fext.grow((size_t)std::max<int64_t>(x->nrows, 1)));
    HIPCHK(nullptr, x->olognum.grow((size_t)std::max<int64_t>(x->nrows, 1)));
    HIPCHK(nullptr, x->mask.grow((size_t)P));
    h->ext = std::move(x);
    return MBAR_OK;
}

namespace {

// The arguments of a pass over the extension rows on the device: f, the problems' N_k as the last solve left them in their
// states, and the mask
int ext_arguments(mbar_batch* h, const double* f, const int32_t* mask, BatchExt* out) {
    BatchSet& s = h->prob;
    BatchExtRows& x = *h->ext;
    const int64_t P = s.count;
    std::vector<mbar_batch_state> st((size_t)P);
    HIPCHK(nullptr, hipSetDevice(h->device));
    HIPCHK(nullptr, hipMemcpyAsync(st.data(), s.states, st.size() * sizeof(mbar_batch_state), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(nullptr, hipStreamSynchronize(h->stream));
    std::vector<double> fv((size_t)P * MBAR_BATCH_MAX_K, 0.0), nk((size_t)P * MBAR_BATCH_MAX_K, 0.0);
    for (int64_t p = 0; p < P; ++p) {
        if (!mask[p]) continue;
        double n = 0.0;
        for (int64_t k = 0; k < s.K[p]; ++k) {
            const double v = f[p * MBAR_BATCH_MAX_K + k];
            if (!std::isfinite(v)) return bad_arg("problem " + std::to_string(p) + ": f is not finite");
            fv[(size_t)(p * MBAR_BATCH_MAX_K + k)] = v;
            nk[(size_t)(p * MBAR_BATCH_MAX_K + k)] = st[(size_t)p].Nk[k];
            n += st[(size_t)p].Nk[k];
        }
        if (st[(size_t)p].K != s.K[p] || n != (double)s.N[p])
            return bad_arg("problem " + std::to_string(p) + ": its state holds no N_k (mbar_batch_solve first)");
    }
    HIPCHK(nullptr, hipMemcpyAsync(x.f, fv.data(), fv.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(nullptr, hipMemcpyAsync(x.Nk, nk.data(), nk.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(nullptr, hipMemcpyAsync(x.mask, mask, (size_t)P * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(nullptr, hipStreamSynchronize(h->stream));  // (the host vectors go)
    BatchExt d{};
    d.e = x.e;
    d.eoff = x.eoff;
    d.K = x.dK;
    d.R = x.dR;
    d.roff = x.roff;
    d.lcoff = x.lcoff;
    d.lpart = x.lpart;
    d.f = x.f;
    d.Nk = x.Nk;
    d.fext = x.fext;
    d.mask = x.mask;
    *out = d;
    return MBAR_OK;
}

constexpr int NEXT = 4;
constexpr int EXT_AB[NEXT] = {16, 32, 64, 128};

}  // namespace

int mbar_batch_ext_lognum(mbar_batch* h, const double* f, const int32_t* mask, double* lognum_ext) {
    if (!h) return bad_arg("batch is NULL");
    if (!f || !mask || !lognum_ext) return bad_arg("f / mask / lognum_ext is NULL");
    if (!h->ext) return bad_arg("mbar_batch_ext_lognum: no extension rows (mbar_batch_set_ext first)");
    BatchExtRows& x = *h->ext;
    if (x.nrows == 0) return MBAR_OK;
    BatchExt d;
    int rc = ext_arguments(h, f, mask, &d);
    if (rc) return rc;
    HIPCHK(nullptr, launch_batch_ext_lognum(h->stream, data(h->prob, h->u), d, x.olognum));
    std::vector<double> out((size_t)x.nrows);
    HIPCHK(nullptr, hipMemcpyAsync(out.data(), x.olognum, out.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(nullptr, hipStreamSynchronize(h->stream));
    for (int64_t p = 0; p < h->prob.count; ++p)
        if (mask[p]) std::copy(out.begin() + x.roff_h[p], out.begin() + x.roff_h[p] + x.R[p], lognum_ext + x.roff_h[p]);
    return MBAR_OK;
}

int mbar_batch_ext_gram(mbar_batch* h, const double* f, const double* f_ext, const int32_t* mask, int64_t group_bytes, double* gram,
                        double* wsum) {
    if (!h) return bad_arg("batch is NULL");
    if (!f || !mask || !gram || !wsum) return bad_arg("f / mask / gram / wsum is NULL");
    if (!h->ext) return bad_arg("mbar_batch_ext_gram: no extension rows (mbar_batch_set_ext first)");
    BatchSet& s = h->prob;
    BatchExtRows& x = *h->ext;
    if (!f_ext && x.nrows > 0) return bad_arg("f_ext is NULL");
    const int64_t P = s.count;
    // work items: run after run of every masked-in problem, in groups of problems whose records take at most group_bytes
    struct Group {
        size_t w0[NEXT + 1];  // its items of each width class in the class's list
        size_t q0, q1;        // its problems in gprob
    };
    std::vector<int> wprob[NEXT], wrun[NEXT], gprob, nrun;
    std::vector<int64_t> wgoff[NEXT], gbase;
    std::vector<Group> groups;
    int64_t used = 0, most = 0;
    for (int64_t p = 0; p < P; ++p) {
        if (!mask[p]) continue;
        for (int64_t r = 0; r < x.R[p]; ++r)
            if (!std::isfinite(f_ext[x.roff_h[p] + r]))
                return bad_arg("problem " + std::to_string(p) + ": f_ext of row " + std::to_string(r) + " is not finite");
        const int64_t A = s.K[p] + x.R[p], sz = A * A + A;
        const int64_t chunks = s.cbeg_h[p + 1] - s.cbeg_h[p];
        const int64_t runs = (chunks + MBAR_BATCH_EXT_RUN - 1) / MBAR_BATCH_EXT_RUN;
        if (groups.empty() || (group_bytes > 0 && used > 0 && (used + runs * sz) * (int64_t)sizeof(double) > group_bytes)) {
            Group g{};
            for (int i = 0; i < NEXT; ++i) g.w0[i] = wprob[i].size();
            g.q0 = g.q1 = gprob.size();
            groups.push_back(g);
            used = 0;
        }
        int cls = 0;
        while (EXT_AB[cls] < A) ++cls;
        gprob.push_back((int)p);
        gbase.push_back(used);
        nrun.push_back((int)runs);
        for (int64_t r = 0; r < runs; ++r) {
            wprob[cls].push_back((int)p);
            wrun[cls].push_back((int)r);
            wgoff[cls].push_back(used + r * sz);
        }
        used += runs * sz;
        most = std::max(most, used);
        groups.back().q1 = gprob.size();
    }
    if (groups.empty()) return MBAR_OK;
    BatchExt d;
    int rc = ext_arguments(h, f, mask, &d);
    if (rc) return rc;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && (size_t)most * sizeof(double) > total_b)
        return fail(nullptr, MBAR_ERR_ARG, "the Gram records of one group need " + std::to_string(((size_t)most * sizeof(double)) >> 20) +
                    " MB of device memory; the device has " + std::to_string(total_b >> 20) + " MB");
    (void)hipGetLastError();
    if (x.nrows > 0)
        HIPCHK(nullptr, hipMemcpyAsync(x.fext, f_ext, (size_t)x.nrows * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(nullptr, hipStreamSynchronize(h->stream));
    // one list per table, the classes one after the other
    std::vector<int> wp, wr;
    std::vector<int64_t> wg;
    size_t cbase[NEXT];
    for (int i = 0; i < NEXT; ++i) {
        cbase[i] = wp.size();
        wp.insert(wp.end(), wprob[i].begin(), wprob[i].end());
        wr.insert(wr.end(), wrun[i].begin(), wrun[i].end());
        wg.insert(wg.end(), wgoff[i].begin(), wgoff[i].end());
    }
    HIPCHK(nullptr, x.wprob.upload(wp.data(), wp.size()));
    HIPCHK(nullptr, x.wrun.upload(wr.data(), wr.size()));
    HIPCHK(nullptr, x.wgoff.upload(wg.data(), wg.size()));
    HIPCHK(nullptr, x.gprob.upload(gprob.data(), gprob.size()));
    HIPCHK(nullptr, x.gbase.upload(gbase.data(), gbase.size()));
    HIPCHK(nullptr, x.nrun.upload(nrun.data(), nrun.size()));
    HIPCHK(nullptr, x.gpart.grow((size_t)most));
    HIPCHK(nullptr, x.ogram.grow((size_t)x.ngram));
    HIPCHK(nullptr, x.owsum.grow((size_t)x.nwsum));
    const BatchData bd = data(s, h->u);
    for (size_t g = 0; g < groups.size(); ++g) {
        const Group& gr = groups[g];
        for (int i = 0; i < NEXT; ++i) {
            const size_t w1 = g + 1 < groups.size() ? groups[g + 1].w0[i] : wprob[i].size();
            const size_t o = cbase[i] + gr.w0[i];
            HIPCHK(nullptr, launch_batch_ext_gram(h->stream, EXT_AB[i], bd, d, (int64_t)(w1 - gr.w0[i]), x.wprob + o, x.wrun + o,
                                                  x.wgoff + o, x.gpart));
        }
        HIPCHK(nullptr, launch_batch_ext_gram_merge(h->stream, d, (int64_t)(gr.q1 - gr.q0), x.gprob + gr.q0, x.gbase + gr.q0,
                                                    x.nrun + gr.q0, x.gpart, x.ogram, x.owsum, x.ogoff, x.owoff));
    }
    std::vector<double> og((size_t)x.ngram), ow((size_t)x.nwsum);
    HIPCHK(nullptr, hipMemcpyAsync(og.data(), x.ogram, og.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(nullptr, hipMemcpyAsync(ow.data(), x.owsum, ow.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(nullptr, hipStreamSynchronize(h->stream));
    for (int64_t p = 0; p < P; ++p) {
        if (!mask[p]) continue;
        const int64_t A = s.K[p] + x.R[p];
        std::copy(og.begin() + x.ogoff_h[p], og.begin() + x.ogoff_h[p] + A * A, gram + x.ogoff_h[p]);
        std::copy(ow.begin() + x.owoff_h[p], ow.begin() + x.owoff_h[p] + A, wsum + x.owoff_h[p]);
    }
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
