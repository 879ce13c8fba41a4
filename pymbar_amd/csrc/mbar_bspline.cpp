// Host side of the weighted B-spline moments (include/mbar_hip.h, "weighted B-spline moments"): the mbar_bspline handle, its
// device buffers (taken from the block cache of mbar_ctx.h), the column passes, the grid (sample chunks x output tiles) and the
// transpose of the combined sums into G x C x nbasis.  Kernels: mbar_k_bspline.hip.
#include <cmath>

#include "mbar_ctx.h"

using namespace mbar;
using namespace mbar::host;

struct mbar_bspline {
    int device = 0, G = 1;
    int64_t N = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double last_ms = 0.0;
    double* X = nullptr;             // [N]
    int* g = nullptr;                // [N] (NULL: one group)
    // weights: host copy of every column and the device buffer of one pass
    int64_t C = 0;
    std::vector<double> Vh;          // [N][C]
    double* V = nullptr;
    size_t v_doubles = 0;
    int64_t v_pass = -1;             // first column of the pass the device buffer holds (-1: none)
    int v_cb = 0;
    double* t = nullptr;             // [BSP_MAX_BASIS + BSP_MAX_K + 1]
    double* part = nullptr;
    size_t part_doubles = 0;
    double* out = nullptr;
    size_t out_doubles = 0;
};

namespace {

int bfail(const std::string& msg, int code = MBAR_ERR_ARG) { return fail(nullptr, code, msg); }

#define BHIP(expr)                                                                                        \
    do {                                                                                                  \
        hipError_t _e = (expr);                                                                           \
        if (_e != hipSuccess) return bfail(std::string(#expr) + ": " + hipGetErrorString(_e), MBAR_ERR_HIP); \
    } while (0)

template <typename T>
hipError_t grow(T** p, size_t* have, size_t want) {
    if (*have >= want) return hipSuccess;
    if (*p) {
        hipError_t e = cache_free(*p);
        if (e != hipSuccess) return e;
    }
    *p = nullptr;
    *have = 0;
    hipError_t e = cache_malloc((void**)p, want * sizeof(T));
    if (e == hipSuccess) *have = want;
    return e;
}

int pass_width(int64_t cols) {
    static const int cbs[] = {1, 2, 4, 8, 16, 32};
    for (int cb : cbs)
        if (cb >= cols) return cb;
    return BSP_MAX_CB;
}

int upload_pass(mbar_bspline* b, int64_t c0, int cv, int cb) {
    if (b->v_pass == c0 && b->v_cb == cb) return MBAR_OK;
    BHIP(grow(&b->V, &b->v_doubles, (size_t)b->N * cb));
    std::vector<double> stage((size_t)b->N * cb, 0.0);
    for (int64_t n = 0; n < b->N; ++n)
        for (int c = 0; c < cv; ++c) stage[(size_t)n * cb + c] = b->Vh[(size_t)n * b->C + c0 + c];
    BHIP(hipMemcpy(b->V, stage.data(), stage.size() * sizeof(double), hipMemcpyHostToDevice));
    b->v_pass = c0;
    b->v_cb = cb;
    return MBAR_OK;
}

}  // namespace

extern "C" {

int mbar_bspline_create(mbar_bspline** out, int device, int64_t N, const double* x) {
    if (!out) return bfail("out is NULL");
    *out = nullptr;
    if (N < 1 || !x) return bfail("need at least one sample");
    for (int64_t i = 0; i < N; ++i)
        if (!std::isfinite(x[i])) return bfail("sample coordinates must be finite");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n < 1)
        return bfail("no HIP device visible (libmbar_hip needs an MI355X / gfx950 GPU)", MBAR_ERR_NODEVICE);
    if (device < 0 || device >= n) return bfail("device index out of range");
    BHIP(hipSetDevice(device));
    hipDeviceProp_t p;
    BHIP(hipGetDeviceProperties(&p, device));
    if (std::strncmp(p.gcnArchName, "gfx950", 6) != 0)
        return bfail(std::string("device is ") + p.gcnArchName + ", this library is built for gfx950 only", MBAR_ERR_NODEVICE);
    mbar_bspline* b = new mbar_bspline();
    g_live_contexts.fetch_add(1);
    b->device = device;
    b->N = N;
    int rc = MBAR_OK;
    auto hip = [&](hipError_t e, const char* what) {
        if (e != hipSuccess && rc == MBAR_OK) rc = bfail(std::string(what) + ": " + hipGetErrorString(e), MBAR_ERR_HIP);
        return rc == MBAR_OK;
    };
    if (hip(hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking), "hipStreamCreateWithFlags") &&
        hip(hipEventCreate(&b->ev0), "hipEventCreate") && hip(hipEventCreate(&b->ev1), "hipEventCreate") &&
        hip(cache_malloc((void**)&b->X, (size_t)N * sizeof(double)), "cache_malloc") &&
        hip(cache_malloc((void**)&b->t, (size_t)(BSP_MAX_BASIS + BSP_MAX_K + 1) * sizeof(double)), "cache_malloc"))
        hip(hipMemcpy(b->X, x, (size_t)N * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy");
    if (rc == MBAR_OK) {
        std::vector<double> ones((size_t)N, 1.0);
        rc = mbar_bspline_set_weights(b, 1, ones.data());
    }
    if (rc != MBAR_OK) {
        const std::string msg = mbar_last_error(nullptr);
        mbar_bspline_destroy(b);
        return bfail(msg, rc);
    }
    *out = b;
    return MBAR_OK;
}

void mbar_bspline_destroy(mbar_bspline* b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    for (void* p : {(void*)b->X, (void*)b->g, (void*)b->V, (void*)b->t, (void*)b->part, (void*)b->out})
        if (p) (void)cache_free(p);
    if (b->ev0) (void)hipEventDestroy(b->ev0);
    if (b->ev1) (void)hipEventDestroy(b->ev1);
    if (b->stream) (void)hipStreamDestroy(b->stream);
    delete b;
    if (g_live_contexts.fetch_sub(1) == 1) g_mem.trim_to(g_mem.idle_limit());
}

int mbar_bspline_set_groups(mbar_bspline* b, int G, const int* g) {
    if (!b) return bfail("bspline is NULL");
    if (G < 1 || G > BSP_MAX_GROUPS) return bfail("G must be 1 .. 1024");
    BHIP(hipSetDevice(b->device));
    if (!g) {
        if (G != 1) return bfail("labels are needed for more than one group");
        if (b->g) BHIP(cache_free(b->g));
        b->g = nullptr;
        b->G = 1;
        return MBAR_OK;
    }
    for (int64_t n = 0; n < b->N; ++n)
        if (g[n] < 0 || g[n] >= G) return bfail("group labels must lie in [0, G)");
    if (!b->g) BHIP(cache_malloc((void**)&b->g, (size_t)b->N * sizeof(int)));
    BHIP(hipMemcpy(b->g, g, (size_t)b->N * sizeof(int), hipMemcpyHostToDevice));
    b->G = G;
    return MBAR_OK;
}

int mbar_bspline_set_weights(mbar_bspline* b, int64_t C, const double* v) {
    if (!b) return bfail("bspline is NULL");
    if (C < 1 || !v) return bfail("need at least one weight column");
    const size_t len = (size_t)b->N * C;
    for (size_t i = 0; i < len; ++i)
        if (!std::isfinite(v[i])) return bfail("weights must be finite");
    b->Vh.assign(v, v + len);
    b->C = C;
    b->v_pass = -1;
    BHIP(hipSetDevice(b->device));
    if (C <= BSP_MAX_CB) return upload_pass(b, 0, (int)C, pass_width(C));  // (one pass: stays resident between calls)
    return MBAR_OK;
}

int mbar_bspline_moments(mbar_bspline* b, int k, int nbasis, const double* t, double* out) {
    if (!b) return bfail("bspline is NULL");
    if (!t || !out) return bfail("t and out must not be NULL");
    if (k < 0 || k > BSP_MAX_K) return bfail("k must be 0 .. 7");
    if (nbasis < k + 1 || nbasis > BSP_MAX_BASIS) return bfail("nbasis must be k + 1 .. 1024");
    const int nt = nbasis + k + 1;
    for (int i = 0; i < nt; ++i) {
        if (!std::isfinite(t[i])) return bfail("knots must be finite");
        if (i > 0 && t[i] < t[i - 1]) return bfail("knots must be non-decreasing");
    }
    BHIP(hipSetDevice(b->device));
    BHIP(hipMemcpy(b->t, t, (size_t)nt * sizeof(double), hipMemcpyHostToDevice));
    const int G = b->G;
    const int cells = G * nbasis;
    // samples: chunks of a multiple of 256 (about 16 batches per wave), fewer when the chunk partials would exceed 2^25 doubles
    const int64_t N = b->N;
    int64_t chunk = 4096;
    const int64_t budget = (int64_t)1 << 25;
    while ((N + chunk - 1) / chunk * (int64_t)cells * BSP_MAX_CB > budget && chunk < N) chunk *= 2;
    const int64_t nchunks = (N + chunk - 1) / chunk;
    BsplineLaunch a;
    a.k = k;
    a.nbasis = nbasis;
    a.X = b->X;
    a.G = b->g;
    a.N = N;
    a.t = b->t;
    a.nchunks = nchunks;
    a.chunk = chunk;
    a.cells = cells;
    std::vector<double> hout;
    double total_ms = 0.0;
    for (int64_t c0 = 0; c0 < b->C; c0 += BSP_MAX_CB) {
        const int cv = (int)std::min<int64_t>(BSP_MAX_CB, b->C - c0);
        const int cb = pass_width(cv);
        int rc = upload_pass(b, c0, cv, cb);
        if (rc) return rc;
        a.cb = cb;
        a.V = b->V;
        a.tile_cells = std::min(cells, BSP_SLAB_ENTRIES / cb);
        a.ntiles = (cells + a.tile_cells - 1) / a.tile_cells;
        const size_t len = (size_t)cells * cb;
        BHIP(grow(&b->part, &b->part_doubles, (size_t)nchunks * len));
        BHIP(grow(&b->out, &b->out_doubles, len));
        a.part = b->part;
        BHIP(hipEventRecord(b->ev0, b->stream));
        BHIP(launch_bspline(b->stream, a));
        BHIP(launch_bspline_combine(b->stream, a, b->out));
        BHIP(hipEventRecord(b->ev1, b->stream));
        hout.resize(len);
        BHIP(hipMemcpyAsync(hout.data(), b->out, len * sizeof(double), hipMemcpyDeviceToHost, b->stream));
        BHIP(hipStreamSynchronize(b->stream));
        float ms = 0.0f;
        BHIP(hipEventElapsedTime(&ms, b->ev0, b->ev1));
        total_ms += ms;
        // [cell = g nbasis + i][cb] -> out[g][C][nbasis]
        for (int g = 0; g < G; ++g)
            for (int c = 0; c < cv; ++c)
                for (int i = 0; i < nbasis; ++i)
                    out[((size_t)g * b->C + c0 + c) * nbasis + i] = hout[((size_t)g * nbasis + i) * cb + c];
    }
    b->last_ms = total_ms;
    return MBAR_OK;
}

int mbar_bspline_kernel_ms(mbar_bspline* b, double* ms) {
    if (!b || !ms) return bfail("bspline and ms must not be NULL");
    *ms = b->last_ms;
    return MBAR_OK;
}

}  // extern "C"
