// Host side of the BAR and EXP estimators (include/mbar_hip.h, "BAR and EXP estimators"): the mbar_bar handle (on the handle
// layer of mbar_handle.h), which keeps P problems' forward and reverse work values resident on a device, cut into chunks with their
// minima, and drives the root find.
// Kernels: mbar_k_bar.hip; the root find's state machine: bar_advance in mbar_bar.h.
#include <cmath>

#include "mbar_handle.h"
#include "mbar_bar.h"

using namespace mbar;
using namespace mbar::host;

struct mbar_bar : Handle {
    int64_t P = 0, nchunks = 0, nvalues = 0;
    std::vector<int64_t> nside;               // [2 P] values per side
    std::vector<double> M;                    // [P]
    DevBuf<double> w;                         // [nvalues]: every forward value, then every reverse value
    DevBuf<int64_t> start;                    // [nchunks]
    DevBuf<int> len, seg;
    DevBuf<double> wmin;
    DevBuf<int64_t> cbeg;                     // [2 P + 1]
    DevBuf<double> dM;                        // [P]
    DevBuf<int64_t> dnside;                   // [2 P]
    DevBuf<BarPartial> part;                  // [2][nchunks]
    DevBuf<mbar_bar_state> states;            // [P]
    DevBuf<int> active;                       // [P]
    DevBuf<double> out;                       // [P][5] (moments: [2 P][5])
    DevBuf<double> scratch;                   // [2 nchunks + 6 P]
};

namespace {

BarData data_of(const mbar_bar* h) {
    BarData d{};
    d.w = h->w;
    d.start = h->start;
    d.len = h->len;
    d.seg = h->seg;
    d.wmin = h->wmin;
    d.cbeg = h->cbeg;
    d.M = h->dM;
    d.P = h->P;
    d.nchunks = h->nchunks;
    return d;
}

int need_both_sides(const mbar_bar* h) {
    for (int64_t s = 0; s < 2 * h->P; ++s)
        if (h->nside[s] == 0) return bad_arg("problem " + std::to_string(s / 2) + " has an empty side");
    return MBAR_OK;
}

}  // namespace

extern "C" {

int mbar_bar_create(mbar_bar** out, int device, int64_t P, const int64_t* n_f, const double* w_f, const int64_t* n_r,
                    const double* w_r) {
    if (!out) return bad_arg("out is NULL");
    *out = nullptr;
    if (P < 1 || !n_f || !n_r) return bad_arg("need at least one problem");
    int64_t tf = 0, tr = 0;
    for (int64_t p = 0; p < P; ++p) {
        if (n_f[p] < 0 || n_r[p] < 0) return bad_arg("problem " + std::to_string(p) + ": negative length");
        tf += n_f[p];
        tr += n_r[p];
    }
    if ((tf > 0 && !w_f) || (tr > 0 && !w_r)) return bad_arg("work values are NULL");
    // chunk table: sides in the order 2 p + (0 forward, 1 reverse), each cut into chunks of MBAR_BAR_CHUNK; minima on the way
    std::vector<int64_t> start, cbeg(1, 0), nside(2 * P);
    std::vector<int> len, seg;
    std::vector<double> wmin;
    int64_t off_f = 0, off_r = tf;
    for (int64_t p = 0; p < P; ++p)
        for (int side = 0; side < 2; ++side) {
            const int64_t n = side ? n_r[p] : n_f[p];
            const int64_t base = side ? off_r : off_f;
            const double* x = (side ? w_r + (off_r - tf) : w_f + off_f);
            nside[2 * p + side] = n;
            for (int64_t i0 = 0; i0 < n; i0 += MBAR_BAR_CHUNK) {
                const int l = (int)std::min<int64_t>(MBAR_BAR_CHUNK, n - i0);
                double m = INFINITY;
                for (int i = 0; i < l; ++i) {
                    const double v = x[i0 + i];
                    if (std::isnan(v) || v == -INFINITY)
                        return bad_arg("problem " + std::to_string(p) + ": " + (side ? "w_R" : "w_F") + " holds NaN or -inf");
                    m = std::min(m, v);
                }
                start.push_back(base + i0);
                len.push_back(l);
                seg.push_back((int)(2 * p + side));
                wmin.push_back(m);
            }
            cbeg.push_back((int64_t)start.size());
            if (side) off_r += n;
            else off_f += n;
        }
    return create_handle(out, device, [&](mbar_bar* h, const DevInfo&) {
        h->P = P;
        h->nchunks = (int64_t)start.size();
        h->nvalues = tf + tr;
        h->nside = nside;
        h->M.resize(P);
        for (int64_t p = 0; p < P; ++p) h->M[p] = std::log((double)n_f[p] / (double)n_r[p]);
        const size_t nc = (size_t)std::max<int64_t>(1, h->nchunks);
        HIPCHK(nullptr, h->w.grow((size_t)std::max<int64_t>(1, h->nvalues)));
        HIPCHK(nullptr, h->start.grow(nc));
        HIPCHK(nullptr, h->len.grow(nc));
        HIPCHK(nullptr, h->seg.grow(nc));
        HIPCHK(nullptr, h->wmin.grow(nc));
        HIPCHK(nullptr, h->part.grow(2 * nc));
        HIPCHK(nullptr, h->states.grow((size_t)P));
        HIPCHK(nullptr, h->active.grow((size_t)P));
        HIPCHK(nullptr, h->out.grow((size_t)(10 * P)));
        HIPCHK(nullptr, h->scratch.grow(2 * nc + (size_t)(6 * P)));
        if (tf > 0) HIPCHK(nullptr, hipMemcpy(h->w, w_f, (size_t)tf * sizeof(double), hipMemcpyHostToDevice));
        if (tr > 0) HIPCHK(nullptr, hipMemcpy(h->w + tf, w_r, (size_t)tr * sizeof(double), hipMemcpyHostToDevice));
        if (h->nchunks > 0) {
            HIPCHK(nullptr, hipMemcpy(h->start, start.data(), start.size() * sizeof(int64_t), hipMemcpyHostToDevice));
            HIPCHK(nullptr, hipMemcpy(h->len, len.data(), len.size() * sizeof(int), hipMemcpyHostToDevice));
            HIPCHK(nullptr, hipMemcpy(h->seg, seg.data(), seg.size() * sizeof(int), hipMemcpyHostToDevice));
            HIPCHK(nullptr, hipMemcpy(h->wmin, wmin.data(), wmin.size() * sizeof(double), hipMemcpyHostToDevice));
        }
        HIPCHK(nullptr, h->cbeg.upload(cbeg.data(), cbeg.size()));
        HIPCHK(nullptr, h->dM.upload(h->M.data(), (size_t)P));
        HIPCHK(nullptr, h->dnside.upload(nside.data(), (size_t)(2 * P)));
        HIPCHK(nullptr, hipMemset(h->scratch, 0, (2 * nc + (size_t)(6 * P)) * sizeof(double)));
        return MBAR_OK;
    });
}

void mbar_bar_destroy(mbar_bar* h) { destroy_handle(h); }

int mbar_bar_zero(mbar_bar* h, const double* deltaf, double* out) {
    if (!h) return bad_arg("bar is NULL");
    if (!deltaf || !out) return bad_arg("deltaf / out is NULL");
    int rc = need_both_sides(h);
    if (rc) return rc;
    HIPCHK(nullptr, hipSetDevice(h->device));
    std::vector<mbar_bar_state> st((size_t)h->P);
    for (int64_t p = 0; p < h->P; ++p) {
        st[p] = mbar_bar_state{};
        st[p].status = BAR_RUNNING;
        st[p].nreq = 1;
        st[p].req[0] = deltaf[p];
    }
    const BarData d = data_of(h);
    HIPCHK(nullptr, hipMemcpyAsync(h->states, st.data(), st.size() * sizeof(mbar_bar_state), hipMemcpyHostToDevice, h->stream));
    HIPCHK(nullptr, launch_bar_eval(h->stream, d, h->states, h->part));
    HIPCHK(nullptr, launch_bar_step(h->stream, d, h->states, h->part, 0, h->out, h->active));
    HIPCHK(nullptr, hipMemcpyAsync(out, h->out, (size_t)(5 * h->P) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(nullptr, hipStreamSynchronize(h->stream));
    return MBAR_OK;
}

int mbar_bar_solve(mbar_bar* h, mbar_bar_state* states, int64_t* passes) {
    if (!h) return bad_arg("bar is NULL");
    if (!states) return bad_arg("states is NULL");
    int rc = need_both_sides(h);
    if (rc) return rc;
    int64_t maxit = 0;
    for (int64_t p = 0; p < h->P; ++p) {
        mbar_bar_state& s = states[p];
        if (s.method < BAR_FALSE_POSITION || s.method > BAR_SELF_CONSISTENT)
            return bad_arg("problem " + std::to_string(p) + ": unknown method");
        if (s.maximum_iterations < 0) return bad_arg("problem " + std::to_string(p) + ": maximum_iterations < 0");
        maxit = std::max(maxit, s.maximum_iterations);
        s.phase = BAR_PH_INIT;
        s.status = BAR_RUNNING;
        s.moments_pending = 0;
        bar_advance(s, nullptr);  // the first requests
    }
    HIPCHK(nullptr, hipSetDevice(h->device));
    const BarData d = data_of(h);
    // The reference's loops all end (the widening overflows to NaN after ~1100 steps); the limit below only guards the host
    // against a state machine that would not.
    const int64_t limit = maxit + 1 + 4096;
    return run_passes(h->stream, states, h->states.p, h->active.p, h->P, limit, "the root find did not end within the pass limit",
                      passes, [&]() -> int {
                          HIPCHK(nullptr, launch_bar_eval(h->stream, d, h->states, h->part));
                          HIPCHK(nullptr, launch_bar_step(h->stream, d, h->states, h->part, 1, h->out, h->active));
                          return MBAR_OK;
                      });
}

int mbar_bar_moments(mbar_bar* h, double* out) {
    if (!h) return bad_arg("bar is NULL");
    if (!out) return bad_arg("out is NULL");
    HIPCHK(nullptr, hipSetDevice(h->device));
    const BarData d = data_of(h);
    HIPCHK(nullptr, launch_bar_moments(h->stream, d, h->dnside, h->scratch, h->out));
    HIPCHK(nullptr, hipMemcpyAsync(out, h->out, (size_t)(10 * h->P) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(nullptr, hipStreamSynchronize(h->stream));
    return MBAR_OK;
}

int mbar_bar_step_host(mbar_bar_state* state, const double* F) {
    if (!state) return bad_arg("state is NULL");
    if (state->phase != BAR_PH_INIT && state->status == BAR_RUNNING && !F) return bad_arg("F is NULL");
    return (int)bar_advance(*state, F);
}

}  // extern "C"
