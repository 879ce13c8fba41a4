// Host side of the weighted B-spline moments (include/mbar_hip.h, "weighted B-spline moments"): the mbar_bspline handle (on the
// handle layer of mbar_handle.h, which also holds its weight columns), the grid (sample chunks x output tiles) and the
// transpose of the combined sums into G x C x nbasis.  Kernels: mbar_k_bspline.hip.
#include <cmath>

#include "mbar_handle.h"
#include "mbar_bspline.h"

using namespace mbar;
using namespace mbar::host;

struct mbar_bspline : Handle {
    int G = 1;
    int64_t N = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    double last_ms = 0.0;
    DevBuf<double> X;                // [N]
    DevBuf<int> g;                   // [N] (empty: one group)
    ColumnPasses V{{1, 2, 4, 8, 16, 32}};
    DevBuf<double> t;                // [BSP_MAX_BASIS + BSP_MAX_K + 1]
    DevBuf<double> part, out;
    ~mbar_bspline() {
        if (ev0) (void)hipEventDestroy(ev0);
        if (ev1) (void)hipEventDestroy(ev1);
    }
};

extern "C" {

int mbar_bspline_create(mbar_bspline** out, int device, int64_t N, const double* x) {
    if (!out) return bad_arg("out is NULL");
    *out = nullptr;
    if (N < 1 || !x) return bad_arg("need at least one sample");
    for (int64_t i = 0; i < N; ++i)
        if (!std::isfinite(x[i])) return bad_arg("sample coordinates must be finite");
    return create_handle(out, device, [&](mbar_bspline* b, const DevInfo&) {
        b->N = N;
        HIPCHK(nullptr, hipEventCreate(&b->ev0));
        HIPCHK(nullptr, hipEventCreate(&b->ev1));
        HIPCHK(nullptr, b->X.upload(x, (size_t)N));
        HIPCHK(nullptr, b->t.grow((size_t)(BSP_MAX_BASIS + BSP_MAX_K + 1)));
        std::vector<double> ones((size_t)N, 1.0);
        return mbar_bspline_set_weights(b, 1, ones.data());
    });
}

void mbar_bspline_destroy(mbar_bspline* b) { destroy_handle(b); }

int mbar_bspline_set_groups(mbar_bspline* b, int G, const int* g) {
    if (!b) return bad_arg("bspline is NULL");
    if (G < 1 || G > BSP_MAX_GROUPS) return bad_arg("G must be 1 .. 1024");
    HIPCHK(nullptr, hipSetDevice(b->device));
    if (!g) {
        if (G != 1) return bad_arg("labels are needed for more than one group");
        b->g.reset();
        b->G = 1;
        return MBAR_OK;
    }
    for (int64_t n = 0; n < b->N; ++n)
        if (g[n] < 0 || g[n] >= G) return bad_arg("group labels must lie in [0, G)");
    HIPCHK(nullptr, b->g.upload(g, (size_t)b->N));
    b->G = G;
    return MBAR_OK;
}

int mbar_bspline_set_weights(mbar_bspline* b, int64_t C, const double* v) {
    if (!b) return bad_arg("bspline is NULL");
    if (C < 1 || !v) return bad_arg("need at least one weight column");
    const size_t len = (size_t)b->N * C;
    for (size_t i = 0; i < len; ++i)
        if (!std::isfinite(v[i])) return bad_arg("weights must be finite");
    b->V.reset(b->N, C, v);
    HIPCHK(nullptr, hipSetDevice(b->device));
    if (C <= BSP_MAX_CB) return b->V.upload(0, (int)C, b->V.width(C), b->N);  // (one pass: stays resident between calls)
    return MBAR_OK;
}

int mbar_bspline_moments(mbar_bspline* b, int k, int nbasis, const double* t, double* out) {
    if (!b) return bad_arg("bspline is NULL");
    if (!t || !out) return bad_arg("t and out must not be NULL");
    if (k < 0 || k > BSP_MAX_K) return bad_arg("k must be 0 .. 7");
    if (nbasis < k + 1 || nbasis > BSP_MAX_BASIS) return bad_arg("nbasis must be k + 1 .. 1024");
    const int nt = nbasis + k + 1;
    for (int i = 0; i < nt; ++i) {
        if (!std::isfinite(t[i])) return bad_arg("knots must be finite");
        if (i > 0 && t[i] < t[i - 1]) return bad_arg("knots must be non-decreasing");
    }
    HIPCHK(nullptr, hipSetDevice(b->device));
    HIPCHK(nullptr, hipMemcpy(b->t, t, (size_t)nt * sizeof(double), hipMemcpyHostToDevice));
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
    const int64_t C = b->V.C;
    for (int64_t c0 = 0; c0 < C; c0 += BSP_MAX_CB) {
        const int cv = (int)std::min<int64_t>(BSP_MAX_CB, C - c0);
        const int cb = b->V.width(cv);
        int rc = b->V.upload(c0, cv, cb, N);
        if (rc) return rc;
        a.cb = cb;
        a.V = b->V.dev;
        a.tile_cells = std::min(cells, BSP_SLAB_ENTRIES / cb);
        a.ntiles = (cells + a.tile_cells - 1) / a.tile_cells;
        const size_t len = (size_t)cells * cb;
        HIPCHK(nullptr, b->part.grow((size_t)nchunks * len));
        HIPCHK(nullptr, b->out.grow(len));
        a.part = b->part;
        HIPCHK(nullptr, hipEventRecord(b->ev0, b->stream));
        HIPCHK(nullptr, launch_bspline(b->stream, a));
        HIPCHK(nullptr, launch_bspline_combine(b->stream, a, b->out));
        HIPCHK(nullptr, hipEventRecord(b->ev1, b->stream));
        hout.resize(len);
        HIPCHK(nullptr, hipMemcpyAsync(hout.data(), b->out, len * sizeof(double), hipMemcpyDeviceToHost, b->stream));
        HIPCHK(nullptr, hipStreamSynchronize(b->stream));
        float ms = 0.0f;
        HIPCHK(nullptr, hipEventElapsedTime(&ms, b->ev0, b->ev1));
        total_ms += ms;
        // [cell = g nbasis + i][cb] -> out[g][C][nbasis]
        for (int g = 0; g < G; ++g)
            for (int c = 0; c < cv; ++c)
                for (int i = 0; i < nbasis; ++i)
                    out[((size_t)g * C + c0 + c) * nbasis + i] = hout[((size_t)g * nbasis + i) * cb + c];
    }
    b->last_ms = total_ms;
    return MBAR_OK;
}

int mbar_bspline_kernel_ms(mbar_bspline* b, double* ms) {
    if (!b || !ms) return bad_arg("bspline and ms must not be NULL");
    *ms = b->last_ms;
    return MBAR_OK;
}

}  // extern "C"
