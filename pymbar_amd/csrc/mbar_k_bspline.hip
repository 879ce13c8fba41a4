// gfx950 (CDNA4 / MI355X) kernels of the weighted B-spline moments behind the spline surfaces of pymbar_amd.FES:
//   M[g, c, i] = sum over the samples n of group g of V[n, c] B_{i,k,t}(x_n),   i = 0 .. nbasis - 1
// with B_{i,k,t} what scipy.interpolate.BSpline(t, e_i, k) returns with extrapolate=True.  One of the translation units of
// libmbar_hip.so; the host side is mbar_bspline.cpp, the launcher declarations are in mbar_bspline.h.  DESIGN.md ("Spline
// surfaces") has the numbers.
//
// Layout.  Samples x: [N], group labels g: [N] int32 (NULL: one group), weights of one column batch V: [N][CB].  The knots sit in
// LDS.  A sample's interval l is scipy's find_interval: the largest l in [k, nbasis - 1] with t[l] <= x (k below t[k+1]), found by
// binary search over the knots; its k + 1 non-zero bases B_{l-k .. l} come from the Cox-de Boor recursion in scipy's own
// operation order (no contraction), so they are bit-identical to scipy's design matrix.
//
// Cells.  A sample's contributions go to the k + 1 consecutive entries of row g that start at its cell key = g nbasis + l - k.
// The output is tiled over the flattened (g, i) entries (blockIdx.y; one tile unless G nbasis CB exceeds a wave slab), the
// samples over contiguous chunks (blockIdx.x).  Every wave of a workgroup walks its own batches of 64 samples of the chunk and
// merges them deterministically: while lanes are left, the lowest remaining lane's cell is the round's cell, the lanes with that
// cell reduce their (k + 1) CB products in a fixed butterfly, and lane 0 adds the results into the wave's own LDS slab with a
// compensated (Neumaier) sum.  At the end the four slabs are merged in wave order and written to the chunk's slot of `part`;
// k_bspline_combine adds the chunk slots in chunk order (compensated).  No floating-point atomics: two identical calls return
// identical bits.  A wave costs one round per distinct cell among its 64 samples: umbrella data (ordered by state, a few
// intervals per state) needs one or two, random x over many groups and intervals up to 64.
#include "mbar_device.h"
#include "mbar_bspline.h"

namespace mbar {

namespace {
constexpr int BSP_THREADS = 256;
constexpr int BSP_WAVES = BSP_THREADS / 64;

// Neumaier step: (s, e) += v
__device__ __forceinline__ void bsp_neumaier(double& s, double& e, double v) {
    const double t = s + v;
    e += fabs(s) >= fabs(v) ? (s - t) + v : (v - t) + s;
    s = t;
}

// the k + 1 non-zero bases at x on interval l (scipy's _deBoor_D with m = 0, same operation order)
template <int K>
__device__ __forceinline__ void deboor(const double* __restrict__ t, double x, int l, double (&h)[K + 1]) {
#pragma clang fp contract(off)
    h[0] = 1.0;
#pragma unroll
    for (int j = 1; j <= K; ++j) {
        double hh[K + 1];
#pragma unroll
        for (int n = 0; n < j; ++n) hh[n] = h[n];
        h[0] = 0.0;
#pragma unroll
        for (int n = 1; n <= j; ++n) {
            const double xb = t[l + n];
            const double xa = t[l + n - j];
            if (xb == xa) {
                h[n] = 0.0;
                continue;
            }
            const double w = hh[n - 1] / (xb - xa);
            h[n - 1] += w * (xb - x);
            h[n] = w * (x - xa);
        }
    }
}

__device__ __forceinline__ double bsp_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
}  // namespace

template <int K, int CB>
__global__ void __launch_bounds__(BSP_THREADS)
k_bspline(const double* __restrict__ X, const int* __restrict__ Gl, const double* __restrict__ V, int64_t N,
          const double* __restrict__ t, int nbasis, int64_t chunk, int cells, int tile_cells, double* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) double bsp_smem[];
    const int nt = nbasis + K + 1;
    const int ntpad = (nt + 1) & ~1;
    double* ts = bsp_smem;
    const int f0 = (int)blockIdx.y * tile_cells;
    const int tc = min(tile_cells, cells - f0);
    const int slab = tile_cells * CB * 2;  // (sum, compensation) per entry
    double* slabs = bsp_smem + ntpad;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < nt; i += BSP_THREADS) ts[i] = t[i];
    for (int i = tid; i < BSP_WAVES * slab; i += BSP_THREADS) slabs[i] = 0.0;
    __syncthreads();
    double* my = slabs + wave * slab;
    const int64_t n0 = (int64_t)blockIdx.x * chunk;
    const int64_t n1 = n0 + chunk < N ? n0 + chunk : N;
    for (int64_t base = n0 + wave * 64; base < n1; base += BSP_THREADS) {
        const int64_t n = base + lane;
        const bool active = n < n1;
        const double x = active ? X[n] : ts[K];
        const int g = (active && Gl) ? Gl[n] : 0;
        // find_interval: first j in [K + 1, nbasis) with t[j] > x, minus one
        int lo = K + 1, hi = nbasis;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (ts[mid] <= x) lo = mid + 1;
            else hi = mid;
        }
        const int l = lo - 1;
        double b[K + 1];
        deboor<K>(ts, x, l, b);
        double v[CB];
#pragma unroll
        for (int c = 0; c < CB; ++c) v[c] = active ? V[n * CB + c] : 0.0;
        const int key = g * nbasis + (l - K);
        const bool live = active && key + K >= f0 && key < f0 + tc;
        uint64_t left = __ballot(live);
        while (left) {
            const int leader = __ffsll((unsigned long long)left) - 1;
            const int kl = __shfl(key, leader, 64);
            const bool mine = live && key == kl;
#pragma unroll
            for (int j = 0; j <= K; ++j) {
                const int f = kl + j - f0;
#pragma unroll
                for (int c = 0; c < CB; ++c) {
                    const double s = bsp_wave_sum(mine ? b[j] * v[c] : 0.0);
                    if (lane == 0 && f >= 0 && f < tc) {
                        double* e = my + (f * CB + c) * 2;
                        double s0 = e[0], c0 = e[1];
                        bsp_neumaier(s0, c0, s);
                        e[0] = s0;
                        e[1] = c0;
                    }
                }
            }
            left &= ~__ballot(mine);
        }
    }
    __syncthreads();
    double* out = part + (int64_t)blockIdx.x * ((int64_t)cells * CB) + (int64_t)f0 * CB;
    for (int e = tid; e < tc * CB; e += BSP_THREADS) {
        double s = 0.0, c = 0.0;
#pragma unroll
        for (int w = 0; w < BSP_WAVES; ++w) {
            bsp_neumaier(s, c, slabs[w * slab + 2 * e]);
            c += slabs[w * slab + 2 * e + 1];
        }
        out[e] = s + c;
    }
}

// out[x] = sum over the chunks, in chunk order (compensated), of part[chunk][x]
__global__ void __launch_bounds__(256)
k_bspline_combine(const double* __restrict__ part, int64_t nchunks, int64_t len, double* __restrict__ out) {
    const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (x >= len) return;
    double s = 0.0, c = 0.0;
    for (int64_t b = 0; b < nchunks; ++b) bsp_neumaier(s, c, part[b * len + x]);
    out[x] = s + c;
}

// ---- launchers -------------------------------------------------------------------------------------------------------------
size_t bspline_lds_bytes(int k, int nbasis, int tile_cells, int cb) {
    const int nt = nbasis + k + 1;
    return (size_t)((nt + 1) & ~1) * 8 + (size_t)BSP_WAVES * tile_cells * cb * 16;
}

namespace {
template <int K, int CB>
hipError_t launch_bspline_t(hipStream_t s, const BsplineLaunch& a) {
    const size_t lds = bspline_lds_bytes(K, a.nbasis, a.tile_cells, CB);
    hipLaunchKernelGGL((k_bspline<K, CB>), dim3((unsigned)a.nchunks, (unsigned)a.ntiles), dim3(BSP_THREADS), lds, s, a.X, a.G, a.V, a.N,
                       a.t, a.nbasis, a.chunk, a.cells, a.tile_cells, a.part);
    return hipGetLastError();
}
template <int K>
hipError_t launch_bspline_cb(hipStream_t s, const BsplineLaunch& a) {
    switch (a.cb) {
        case 1: return launch_bspline_t<K, 1>(s, a);
        case 2: return launch_bspline_t<K, 2>(s, a);
        case 4: return launch_bspline_t<K, 4>(s, a);
        case 8: return launch_bspline_t<K, 8>(s, a);
        case 16: return launch_bspline_t<K, 16>(s, a);
        case 32: return launch_bspline_t<K, 32>(s, a);
        default: return hipErrorInvalidValue;
    }
}
}  // namespace

hipError_t launch_bspline(hipStream_t s, const BsplineLaunch& a) {
    if (a.nbasis < a.k + 1 || a.nbasis > BSP_MAX_BASIS || a.tile_cells < 1 || a.tile_cells * a.cb > BSP_SLAB_ENTRIES) return hipErrorInvalidValue;
    switch (a.k) {
        case 0: return launch_bspline_cb<0>(s, a);
        case 1: return launch_bspline_cb<1>(s, a);
        case 2: return launch_bspline_cb<2>(s, a);
        case 3: return launch_bspline_cb<3>(s, a);
        case 4: return launch_bspline_cb<4>(s, a);
        case 5: return launch_bspline_cb<5>(s, a);
        case 6: return launch_bspline_cb<6>(s, a);
        case 7: return launch_bspline_cb<7>(s, a);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_bspline_combine(hipStream_t s, const BsplineLaunch& a, double* out) {
    const int64_t len = (int64_t)a.cells * a.cb;
    hipLaunchKernelGGL(k_bspline_combine, dim3((unsigned)((len + 255) / 256)), dim3(256), 0, s, a.part, a.nchunks, len, out);
    return hipGetLastError();
}

}  // namespace mbar
