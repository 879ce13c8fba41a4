// Host side of the BAR and EXP estimators (include/mbar_hip.h, "BAR and EXP estimators"): the mbar_bar handle, which keeps P
// problems' forward and reverse work values resident on a device, cut into chunks with their minima, and drives the root find.
// Kernels: mbar_k_bar.hip; the root find's state machine: bar_advance in mbar_internal.h.
#include <cmath>

#include "mbar_ctx.h"

using namespace mbar;
using namespace mbar::host;

struct mbar_bar {
    int device = 0;
    int64_t P = 0, nchunks = 0, nvalues = 0;
    hipStream_t stream = nullptr;
    std::vector<int64_t> nside;        // [2 P] values per side
    std::vector<double> M;             // [P]
    double* w = nullptr;               // [nvalues]: every forward value, then every reverse value
    int64_t* start = nullptr;          // [nchunks]
    int* len = nullptr;
    int* seg = nullptr;
    double* wmin = nullptr;
    int64_t* cbeg = nullptr;           // [2 P + 1]
    double* dM = nullptr;              // [P]
    int64_t* dnside = nullptr;         // [2 P]
    BarPartial* part = nullptr;        // [2][nchunks]
    mbar_bar_state* states = nullptr;  // [P]
    int* active = nullptr;             // [P]
    double* out = nullptr;             // [P][5] (moments: [2 P][5])
    double* scratch = nullptr;         // [2 nchunks + 6 P]
};

namespace {

int bfail(const std::string& msg, int code = MBAR_ERR_ARG) { return fail(nullptr, code, msg); }

#define BHIP(expr)                                                                                        \
    do {                                                                                                  \
        hipError_t _e = (expr);                                                                           \
        if (_e != hipSuccess) return bfail(std::string(#expr) + ": " + hipGetErrorString(_e), MBAR_ERR_HIP); \
    } while (0)

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
        if (h->nside[s] == 0) return bfail("problem " + std::to_string(s / 2) + " has an empty side");
    return MBAR_OK;
}

}  // namespace

extern "C" {

int mbar_bar_create(mbar_bar** out, int device, int64_t P, const int64_t* n_f, const double* w_f, const int64_t* n_r,
                    const double* w_r) {
    if (!out) return bfail("out is NULL");
    *out = nullptr;
    if (P < 1 || !n_f || !n_r) return bfail("need at least one problem");
    int64_t tf = 0, tr = 0;
    for (int64_t p = 0; p < P; ++p) {
        if (n_f[p] < 0 || n_r[p] < 0) return bfail("problem " + std::to_string(p) + ": negative length");
        tf += n_f[p];
        tr += n_r[p];
    }
    if ((tf > 0 && !w_f) || (tr > 0 && !w_r)) return bfail("work values are NULL");
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
                        return bfail("problem " + std::to_string(p) + ": " + (side ? "w_R" : "w_F") + " holds NaN or -inf");
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
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1)
        return bfail("no HIP device visible (libmbar_hip needs an MI355X / gfx950 GPU)", MBAR_ERR_NODEVICE);
    if (device < 0 || device >= n) return bfail("device index out of range");
    BHIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    BHIP(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return bfail(std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only", MBAR_ERR_NODEVICE);
    mbar_bar* h = new mbar_bar();
    g_live_contexts.fetch_add(1);
    h->device = device;
    h->P = P;
    h->nchunks = (int64_t)start.size();
    h->nvalues = tf + tr;
    h->nside = nside;
    h->M.resize(P);
    for (int64_t p = 0; p < P; ++p) h->M[p] = std::log((double)n_f[p] / (double)n_r[p]);
    int rc = MBAR_OK;
    auto hip = [&](hipError_t e, const char* what) {
        if (e != hipSuccess && rc == MBAR_OK) rc = bfail(std::string(what) + ": " + hipGetErrorString(e), MBAR_ERR_HIP);
        return rc == MBAR_OK;
    };
    const size_t nc = (size_t)std::max<int64_t>(1, h->nchunks);
    auto alloc = [&](void** p, size_t bytes) { return hip(cache_malloc(p, std::max<size_t>(bytes, 8)), "cache_malloc"); };
    if (hip(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking), "hipStreamCreateWithFlags") &&
        alloc((void**)&h->w, (size_t)h->nvalues * sizeof(double)) && alloc((void**)&h->start, nc * sizeof(int64_t)) &&
        alloc((void**)&h->len, nc * sizeof(int)) && alloc((void**)&h->seg, nc * sizeof(int)) &&
        alloc((void**)&h->wmin, nc * sizeof(double)) && alloc((void**)&h->cbeg, (size_t)(2 * P + 1) * sizeof(int64_t)) &&
        alloc((void**)&h->dM, (size_t)P * sizeof(double)) && alloc((void**)&h->dnside, (size_t)(2 * P) * sizeof(int64_t)) &&
        alloc((void**)&h->part, 2 * nc * sizeof(BarPartial)) && alloc((void**)&h->states, (size_t)P * sizeof(mbar_bar_state)) &&
        alloc((void**)&h->active, (size_t)P * sizeof(int)) && alloc((void**)&h->out, (size_t)(10 * P) * sizeof(double)) &&
        alloc((void**)&h->scratch, (2 * nc + (size_t)(6 * P)) * sizeof(double))) {
        if (tf > 0) hip(hipMemcpy(h->w, w_f, (size_t)tf * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy");
        if (tr > 0) hip(hipMemcpy(h->w + tf, w_r, (size_t)tr * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy");
        if (h->nchunks > 0) {
            hip(hipMemcpy(h->start, start.data(), start.size() * sizeof(int64_t), hipMemcpyHostToDevice), "hipMemcpy");
            hip(hipMemcpy(h->len, len.data(), len.size() * sizeof(int), hipMemcpyHostToDevice), "hipMemcpy");
            hip(hipMemcpy(h->seg, seg.data(), seg.size() * sizeof(int), hipMemcpyHostToDevice), "hipMemcpy");
            hip(hipMemcpy(h->wmin, wmin.data(), wmin.size() * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy");
        }
        hip(hipMemcpy(h->cbeg, cbeg.data(), cbeg.size() * sizeof(int64_t), hipMemcpyHostToDevice), "hipMemcpy");
        hip(hipMemcpy(h->dM, h->M.data(), (size_t)P * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy");
        hip(hipMemcpy(h->dnside, nside.data(), (size_t)(2 * P) * sizeof(int64_t), hipMemcpyHostToDevice), "hipMemcpy");
        hip(hipMemset(h->scratch, 0, (2 * nc + (size_t)(6 * P)) * sizeof(double)), "hipMemset");
    }
    if (rc != MBAR_OK) {
        const std::string msg = mbar_last_error(nullptr);
        mbar_bar_destroy(h);
        return bfail(msg, rc);
    }
    *out = h;
    return MBAR_OK;
}

void mbar_bar_destroy(mbar_bar* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    for (void* p : {(void*)h->w, (void*)h->start, (void*)h->len, (void*)h->seg, (void*)h->wmin, (void*)h->cbeg, (void*)h->dM,
                    (void*)h->dnside, (void*)h->part, (void*)h->states, (void*)h->active, (void*)h->out, (void*)h->scratch})
        if (p) (void)cache_free(p);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
    if (g_live_contexts.fetch_sub(1) == 1) g_mem.trim_to(g_mem.idle_limit());
}

int mbar_bar_zero(mbar_bar* h, const double* deltaf, double* out) {
    if (!h) return bfail("bar is NULL");
    if (!deltaf || !out) return bfail("deltaf / out is NULL");
    int rc = need_both_sides(h);
    if (rc) return rc;
    BHIP(hipSetDevice(h->device));
    std::vector<mbar_bar_state> st((size_t)h->P);
    for (int64_t p = 0; p < h->P; ++p) {
        st[p] = mbar_bar_state{};
        st[p].status = BAR_RUNNING;
        st[p].nreq = 1;
        st[p].req[0] = deltaf[p];
    }
    const BarData d = data_of(h);
    BHIP(hipMemcpyAsync(h->states, st.data(), st.size() * sizeof(mbar_bar_state), hipMemcpyHostToDevice, h->stream));
    BHIP(launch_bar_eval(h->stream, d, h->states, h->part));
    BHIP(launch_bar_step(h->stream, d, h->states, h->part, 0, h->out, h->active));
    BHIP(hipMemcpyAsync(out, h->out, (size_t)(5 * h->P) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    BHIP(hipStreamSynchronize(h->stream));
    return MBAR_OK;
}

int mbar_bar_solve(mbar_bar* h, mbar_bar_state* states, int64_t* passes) {
    if (!h) return bfail("bar is NULL");
    if (!states) return bfail("states is NULL");
    int rc = need_both_sides(h);
    if (rc) return rc;
    int64_t maxit = 0;
    for (int64_t p = 0; p < h->P; ++p) {
        mbar_bar_state& s = states[p];
        if (s.method < BAR_FALSE_POSITION || s.method > BAR_SELF_CONSISTENT)
            return bfail("problem " + std::to_string(p) + ": unknown method");
        if (s.maximum_iterations < 0) return bfail("problem " + std::to_string(p) + ": maximum_iterations < 0");
        maxit = std::max(maxit, s.maximum_iterations);
        s.phase = BAR_PH_INIT;
        s.status = BAR_RUNNING;
        s.moments_pending = 0;
        bar_advance(s, nullptr);  // the first requests
    }
    BHIP(hipSetDevice(h->device));
    const BarData d = data_of(h);
    BHIP(hipMemcpyAsync(h->states, states, (size_t)h->P * sizeof(mbar_bar_state), hipMemcpyHostToDevice, h->stream));
    // Passes in groups of 4, 8, 16, 16, ...: between groups the host reads one int per problem.  A finished problem costs one
    // early-exiting workgroup per chunk.  The reference's loops all end (the widening overflows to NaN after ~1100 steps); the
    // limit below only guards the host against a state machine that would not.
    const int64_t limit = maxit + 1 + 4096;
    std::vector<int> act((size_t)h->P);
    int64_t done = 0;
    int group = 4;
    for (;;) {
        for (int k = 0; k < group; ++k) {
            BHIP(launch_bar_eval(h->stream, d, h->states, h->part));
            BHIP(launch_bar_step(h->stream, d, h->states, h->part, 1, h->out, h->active));
        }
        done += group;
        BHIP(hipMemcpyAsync(act.data(), h->active, act.size() * sizeof(int), hipMemcpyDeviceToHost, h->stream));
        BHIP(hipStreamSynchronize(h->stream));
        bool any = false;
        for (int a : act) any = any || a != 0;
        if (!any) break;
        if (done > limit) return bfail("the root find did not end within the pass limit", MBAR_ERR_NUMERIC);
        group = std::min(16, group * 2);
    }
    BHIP(hipMemcpyAsync(states, h->states, (size_t)h->P * sizeof(mbar_bar_state), hipMemcpyDeviceToHost, h->stream));
    BHIP(hipStreamSynchronize(h->stream));
    if (passes) *passes = done;
    return MBAR_OK;
}

int mbar_bar_moments(mbar_bar* h, double* out) {
    if (!h) return bfail("bar is NULL");
    if (!out) return bfail("out is NULL");
    BHIP(hipSetDevice(h->device));
    const BarData d = data_of(h);
    BHIP(launch_bar_moments(h->stream, d, h->dnside, h->scratch, h->out));
    BHIP(hipMemcpyAsync(out, h->out, (size_t)(10 * h->P) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    BHIP(hipStreamSynchronize(h->stream));
    return MBAR_OK;
}

int mbar_bar_step_host(mbar_bar_state* state, const double* F) {
    if (!state) return bfail("state is NULL");
    if (state->phase != BAR_PH_INIT && state->status == BAR_RUNNING && !F) return bfail("F is NULL");
    return (int)bar_advance(*state, F);
}

}  // extern "C"
