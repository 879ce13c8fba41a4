// gfx950 (CDNA4 / MI355X) kernels of the MBAR solver hot path -- the passes over N-vectors, matrix rows and partial records:
// record reductions, log-space per-state sums, log W, the boundary check, vector fills, generators, and the row operations of
// the expectation family.
// One of the translation units of libmbar_hip.so (compiled in parallel by pymbar_amd/_build.py): the shared device helpers and
// the data-layout notes are in mbar_sweep_device.h, the host-side interface of the launchers in mbar_internal.h.  The K x K work of
// the solver loops is in mbar_k_loop.hip.
#include "mbar_device.h"
#include "mbar_internal.h"

namespace mbar {

// ---------------------------------------------------------------------------------------------
// Sums of partial records
// ---------------------------------------------------------------------------------------------
// Element i of the records [blockIdx.y * chunk, ... + chunk) of `part`, added in ascending order
__device__ __forceinline__ double chunk_sum(const double* __restrict__ part, int64_t nparts, int64_t count, int64_t chunk, int64_t i) {
    const int64_t p0 = (int64_t)blockIdx.y * chunk;
    const int64_t p1 = p0 + chunk < nparts ? p0 + chunk : nparts;
    double s = 0.0;
#pragma unroll 8  // (same summation order; eight loads in flight)
    for (int64_t p = p0; p < p1; ++p) s += part[p * count + i];
    return s;
}
__global__ void __launch_bounds__(256)
k_reduce(const double* __restrict__ part, int64_t nparts, int64_t count, int64_t chunk,
         double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    out[(int64_t)blockIdx.y * count + i] = chunk_sum(part, nparts, count, chunk, i);
}
// Same reduction as k_reduce for TWO partial-record arrays with the same number of records in one launch
// (blocks [0, gxA) work on A, the rest on B; identical summation order).
__global__ void __launch_bounds__(256)
k_reduce2(const double* __restrict__ partA, int64_t countA, const double* __restrict__ partB, int64_t countB,
          int64_t nparts, int64_t chunk, double* __restrict__ outA, double* __restrict__ outB) {
    const int64_t gxA = (countA + 255) / 256;
    const bool isB = (int64_t)blockIdx.x >= gxA;
    const double* part = isB ? partB : partA;
    const int64_t count = isB ? countB : countA;
    double* out = isB ? outB : outA;
    const int64_t i = ((int64_t)blockIdx.x - (isB ? gxA : 0)) * blockDim.x + threadIdx.x;
    if (i >= count) return;
    out[(int64_t)blockIdx.y * count + i] = chunk_sum(part, nparts, count, chunk, i);
}

// ---------------------------------------------------------------------------------------------
// Log-space per-state sums and log W
// ---------------------------------------------------------------------------------------------
// Robust per-state log-sum-exp over samples (log space, like the reference's second logsumexp, mbar_solvers.py:240-241):
//   lognum_k = log sum_n exp(anum_k - u_kn - logden_n)   for ALL states (unsampled ones have no usable shift a priori).
// One wave owns LN_ROWS state rows x a contiguous range of samples, ONE SAMPLE PER LANE per 64-sample tile, and keeps a
// running (max, scaled sum) per state in registers:  d = x - m;  e = exp(-|d|);  s = d > 0 ? s e + 1 : s + e;  m = max(m, x)
// -- one table exponential per matrix element, no cross-lane traffic inside the loop (the previous version reduced
// across the wave twice per state per 512 samples and called the library exp: VALU-bound at 3.8 TB/s).  The LN_ROWS
// row loads of a tile are independent 512-byte requests; two tiles are in flight per wave.  Each wave emits one
// (max, sum) record per state; k_lognum_merge combines them.
constexpr int LN_ROWS = 8;
constexpr int LN_TILE = 64;
template <bool MASKED>
__device__ __forceinline__ void lognum_tile(const double* __restrict__ u, int64_t ld, int64_t N, int64_t K, int64_t k0,
                                            int64_t n, const double* __restrict__ logden, const double (&a)[LN_ROWS],
                                            double (&m)[LN_ROWS], double (&s)[LN_ROWS]) {
    const bool ok = !MASKED || n < N;
    const int64_t nn = ok ? n : 0;
    double v[LN_ROWS];
#pragma unroll
    for (int i = 0; i < LN_ROWS; ++i) v[i] = (k0 + i < K) ? u[(k0 + i) * ld + nn] : 0.0;
    const double nl = -logden[nn];
#pragma unroll
    for (int i = 0; i < LN_ROWS; ++i) {
        double x = (a[i] + nl) - v[i];
        if (MASKED && !ok) x = -INFINITY;
        const double d = x - m[i];  // NaN only for -inf - -inf: laundered to e = 0 by the clamp, and "d > 0" is false
        const double e = exp2s_fast(-fabs(d) * LOG2E_S);
        s[i] = d > 0.0 ? fma(s[i], e, 1.0) : s[i] + e;
        m[i] = fmax(m[i], x);
    }
}
__global__ void __launch_bounds__(256)
k_lognum(const double* __restrict__ u, int64_t ld, int64_t N, int64_t K,
         const double* __restrict__ anum, const double* __restrict__ logden,
         double* __restrict__ pmax, double* __restrict__ psum, int64_t nchunks, int64_t tiles_per_chunk) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    exp_table_init(smem);
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t nsb = (K + LN_ROWS - 1) / LN_ROWS;
    const int64_t w = (int64_t)blockIdx.x * 4 + wave;  // neighbouring waves: same sample range, different state rows
    const int64_t c = w / nsb, k0 = (w % nsb) * LN_ROWS;
    if (c >= nchunks) return;
    double a[LN_ROWS], m[LN_ROWS], s[LN_ROWS];
#pragma unroll
    for (int i = 0; i < LN_ROWS; ++i) {
        a[i] = (k0 + i < K) ? anum[k0 + i] : 0.0;
        m[i] = -INFINITY;
        s[i] = 0.0;
    }
    const int64_t ntiles = (N + LN_TILE - 1) / LN_TILE;
    const int64_t t0 = c * tiles_per_chunk;
    int64_t t1 = t0 + tiles_per_chunk;
    if (t1 > ntiles) t1 = ntiles;
    const int64_t tfull = (t1 * LN_TILE <= N) ? t1 : t1 - 1;  // only the very last tile of the matrix can be ragged
    int64_t t = t0;
    for (; t + 1 < tfull; t += 2) {
        lognum_tile<false>(u, ld, N, K, k0, t * LN_TILE + lane, logden, a, m, s);
        lognum_tile<false>(u, ld, N, K, k0, (t + 1) * LN_TILE + lane, logden, a, m, s);
    }
    for (; t < tfull; ++t) lognum_tile<false>(u, ld, N, K, k0, t * LN_TILE + lane, logden, a, m, s);
    for (; t < t1; ++t) lognum_tile<true>(u, ld, N, K, k0, t * LN_TILE + lane, logden, a, m, s);
#pragma unroll
    for (int i = 0; i < LN_ROWS; ++i) {
        const double mw = wave_max(m[i]);
        const double sc = (m[i] > -INFINITY) ? s[i] * exp(m[i] - mw) : 0.0;  // (mw = -inf only if every lane's m is)
        const double sw = wave_sum(sc);
        if (lane == 0 && k0 + i < K) {
            pmax[(k0 + i) * nchunks + c] = mw;
            psum[(k0 + i) * nchunks + c] = sw;
        }
    }
}

__global__ void __launch_bounds__(256)
k_lognum_merge(const double* __restrict__ pmax, const double* __restrict__ psum, int64_t nchunks,
               double* __restrict__ out_max, double* __restrict__ out_sum) {
    __shared__ double red[8];
    const int64_t k = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double m = -INFINITY;
    for (int64_t c = threadIdx.x; c < nchunks; c += blockDim.x) m = fmax(m, pmax[k * nchunks + c]);
    m = wave_max(m);
    if (lane == 0) red[wave] = m;
    __syncthreads();
    m = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    double s = 0.0;
    if (m > -INFINITY)
        for (int64_t c = threadIdx.x; c < nchunks; c += blockDim.x) {
            const double pm = pmax[k * nchunks + c];
            if (pm > -INFINITY) s += psum[k * nchunks + c] * exp(pm - m);
        }
    s = wave_sum(s);
    if (lane == 0) red[4 + wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        out_max[k] = m;
        out_sum[k] = red[4] + red[5] + red[6] + red[7];
    }
}

template <bool EXP>  // EXP: the weights themselves (mbar_solvers.py:476-486 takes exp of the log weights on the host)
__global__ void __launch_bounds__(256)
k_logw(const double* __restrict__ u, int64_t ld, int64_t N, const double* __restrict__ f,
       const double* __restrict__ logden, double* __restrict__ out, int64_t ld_out) {
    const int64_t k = blockIdx.y;
    const double fk = f[k];
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < N; n += (int64_t)gridDim.x * blockDim.x) {
        const double lw = fk - u[k * ld + n] - logden[n];
        out[k * ld_out + n] = EXP ? exp(lw) : lw;
    }
}

// ---------------------------------------------------------------------------------------------
// The matrix at the boundary, and N-vectors
// ---------------------------------------------------------------------------------------------
// Boundary check of the matrix: bit 0 = some entry is NaN, bit 1 = some entry is -inf, bit 2 = some entry is +inf (legal:
// such a sample simply has zero weight in that state).  The fast exp of the sweeps launders NaN, so a poisoned matrix
// is flagged here once and every reduced output is then reported as NaN, like the reference would compute.
__global__ void __launch_bounds__(256)
k_check_u(const double* __restrict__ u, int64_t ld, int64_t N, int* __restrict__ flags) {
    const int64_t k = blockIdx.y;
    int f = 0;
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < N; n += (int64_t)gridDim.x * blockDim.x) {
        const double v = u[k * ld + n];
        if (v != v) f |= 1;
        if (v == -INFINITY) f |= 2;
        if (v == INFINITY) f |= 4;  // legal (weight zero), but the unclamped Gram sweep must not see it
    }
    if (f) atomicOr(flags, f);
}

// out[n] = logden[n] - alpha * ln(cw[n]): folds per-sample multiplicities into the exponent of the kernels that take
// logden as an input (alpha = 1/2: each MFMA operand of the Gram sweep carries sqrt(c_n); alpha = 1: the log-space
// per-state reduction).  c_n = 0 gives +inf, i.e. weight zero.
__global__ void __launch_bounds__(256)
k_shift_logden(const double* __restrict__ logden, const double* __restrict__ cw, double alpha, int64_t N,
               double* __restrict__ out, const int* __restrict__ ctl, int64_t slot_stride) {
    if (ctl) {
        if (ctl[CTL_DONE] != 0) return;
        logden += (int64_t)ctl[CTL_SLOT] * slot_stride;
    }
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < N; n += (int64_t)gridDim.x * blockDim.x) {
        const double c = cw[n];
        out[n] = c > 0.0 ? logden[n] - alpha * log(c) : INFINITY;
    }
}

__global__ void __launch_bounds__(256) k_fill(double* __restrict__ v, double value, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) v[i] = value;
}
// zero fill at HBM write speed (16 bytes per lane and store; hipMemsetAsync's fill kernel runs at ~1 TB/s: 20 ms for the 20 GB of an
// augmented matrix of the expectation family, 10 ms for config 3's matrix in front of its upload)
__global__ void __launch_bounds__(256) k_zero16(uint4* __restrict__ p, size_t n16) {
    const uint4 z = make_uint4(0u, 0u, 0u, 0u);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x) p[i] = z;
}
// dst = sqrt(src): the roots of the sample multiplicities for the matrix-core operands of the weighted sweeps
__global__ void __launch_bounds__(256) k_sqrt_vec(double* __restrict__ dst, const double* __restrict__ src, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) dst[i] = sqrt(src[i]);
}
// cw[n] = exp(p v[n]), cwsq[n] = exp(p v[n] / 2) for n < N: per-sample weights A'^p from the staging vector log A' of an observable
// (mbar_ctx_weights_from_vec; the padding behind N keeps its zeros)
__global__ void __launch_bounds__(256)
k_weights_from_log(const double* __restrict__ v, double p, int64_t n, double* __restrict__ cw, double* __restrict__ cwsq,
                   int* __restrict__ overflow) {
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const double x = p * v[i];
        const double e = exp(x);
        cw[i] = e;
        cwsq[i] = exp(0.5 * x);
        bad |= !(e <= 1.79e308);  // inf (the observable spans more than 1e308^(1/p)) or NaN
    }
    if (bad) atomicOr(overflow, 1);
}

// ---------------------------------------------------------------------------------------------
// Generators: the harmonic-oscillator test matrix and the bootstrap draw
// ---------------------------------------------------------------------------------------------
// The state s whose run of positions holds j: cum[s] <= j < cum[s + 1] (empty states have empty runs)
__device__ __forceinline__ int64_t run_of(const int64_t* __restrict__ cum, int64_t K, int64_t j) {
    int64_t lo = 0, hi = K;
    while (hi - lo > 1) {
        const int64_t mid = (lo + hi) >> 1;
        if (cum[mid] <= j) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ void __launch_bounds__(256)
k_generate_harmonic(double* __restrict__ u, int64_t ld, int64_t N, int64_t K, uint64_t seed,
                    const double* __restrict__ O_k, const double* __restrict__ K_k,
                    const int64_t* __restrict__ cumN, int64_t n_global0) {
    for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < N; n += (int64_t)gridDim.x * blockDim.x) {
        const int64_t ng = n_global0 + n;
        const int64_t lo = run_of(cumN, K, ng);
        const uint64_t key = seed * 0xD1342543DE82EF95ull + 2ull * (uint64_t)ng;
        const uint64_t r1 = splitmix64(key), r2 = splitmix64(key + 1ull);
        const double u1 = ((double)(r1 >> 11) + 0.5) * (1.0 / 9007199254740992.0);
        const double u2 = ((double)(r2 >> 11) + 0.5) * (1.0 / 9007199254740992.0);
        const double z = sqrt(-2.0 * log(u1)) * cos(6.283185307179586476925286766559 * u2);
        const double x = O_k[lo] + z / sqrt(K_k[lo]);
        for (int64_t l = 0; l < K; ++l) {
            const double d = x - O_k[l];
            u[l * ld + n] = 0.5 * K_k[l] * d * d;
        }
    }
}
// One bootstrap replicate as draw counts (mbar.py:417-449: every state redraws its N_k samples from its own samples): slot j of the
// state whose run of positions contains j draws one of that run's positions; the sample there gets one more count.
__global__ void __launch_bounds__(256)
k_bootstrap_counts(uint64_t seed, int64_t replicate, const int64_t* __restrict__ cum, int64_t K, int64_t total,
                   const int64_t* __restrict__ order, int64_t n0, int64_t N, double* __restrict__ cw) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < total; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t lo = run_of(cum, K, j);
        const int64_t start = cum[lo], nk = cum[lo + 1] - start;
        const int64_t pos = start + bootstrap_draw(seed, (uint64_t)replicate, (uint64_t)j, (uint64_t)nk);
        const int64_t sample = (order ? order[pos] : pos) - n0;
        if (sample >= 0 && sample < N) atomicAdd(cw + sample, 1.0);
    }
}

// ---------------------------------------------------------------------------------------------
// The matrix-core probe and the resident probability matrix of 129 .. 256 states
// ---------------------------------------------------------------------------------------------
// fp64 MFMA peak probe: 4 independent accumulators per wave, nothing else in the loop
// (same kernel as tools/mfma_peak.hip; 64 cycles per instruction per SIMD on gfx950).
__global__ void k_mfma_peak(int iters, double* sink) {
    v4d c[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) c[i] = v4d{0.0, 0.0, 0.0, 0.0};
    const double a = 1.0 + threadIdx.x * 1e-9, b = 1.0 - threadIdx.x * 1e-9;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 4; ++i) c[i] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c[i], 0, 0, 0);
    }
    double v = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) v += c[i][0] + c[i][3];
    if (v == 12345.678) sink[threadIdx.x] = v;  // never true: keeps the loop alive
}

// P = exp(aden_k - u_kn - logden_n) for the rows / samples of a shard (padding: 0; entries below the normal range are flushed to
// zero): the resident probability matrix of 129 .. 256 states, built from the log-denominators an evaluation sweep left behind.
__global__ void __launch_bounds__(256)
k_make_p(const double* __restrict__ u, int64_t ld, int64_t N, int64_t rows, const double* __restrict__ aden,
         const double* __restrict__ logden, double* __restrict__ P) {
    const int64_t per_row = ld / 2;  // two samples per thread
    const int64_t total = rows * per_row;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = e / per_row, n = (e - k * per_row) * 2;
        const double a = aden[k];
        const double2 uv = *reinterpret_cast<const double2*>(u + k * ld + n);
        double2 pv;
        pv.x = (n < N) ? exp(a - uv.x - logden[n]) : 0.0;
        pv.y = (n + 1 < N) ? exp(a - uv.y - logden[n + 1]) : 0.0;
        // (flush below the normal range -- the bound is 2^-1022 itself: 2.3e-308 used to zero the normal entries in [2^-1022, 2.3e-308)
        // as well; also a = -inf: unsampled / padded state)
        if (!(pv.x >= 0x1p-1022)) pv.x = 0.0;
        if (!(pv.y >= 0x1p-1022)) pv.y = 0.0;
        *reinterpret_cast<double2*>(P + k * ld + n) = pv;
    }
}

// ---------------------------------------------------------------------------------------------
// Row operations of the expectation family and the histogram (rows `ld` apart; grid.y walks the rows)
// ---------------------------------------------------------------------------------------------
// rows[i][n] = (label[n] == i) ? v[n] : +inf  for i < nrows: one "state" per histogram bin whose only samples are the
// bin's own (a +inf reduced potential is weight zero).  grid.y = row.
__global__ void __launch_bounds__(256)
k_fill_masked_rows(double* __restrict__ rows, int64_t ld, int64_t n, const double* __restrict__ v,
                   const int* __restrict__ label) {
    const int i = blockIdx.y;
    double* row = rows + (int64_t)i * ld;
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x)
        row[k] = label[k] == i ? v[k] : INFINITY;
}
// dst[r][i] = src[r][i] - v[i] for r < nrows (dst == src: in place)
__global__ void __launch_bounds__(256) k_rows_sub(double* __restrict__ dst, const double* __restrict__ src, int64_t ld, int64_t nrows,
                                                  const double* __restrict__ v, int64_t n) {
    for (int64_t r = blockIdx.y; r < nrows; r += gridDim.y)
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
            dst[r * ld + i] = src[r * ld + i] - v[i];
}
// dst[r][i] = src[r][i] - dst[r][i]  (the observable rows arrive as log A and leave as u - log A)
__global__ void __launch_bounds__(256) k_rows_rsub(double* __restrict__ dst, const double* __restrict__ src, int64_t ld, int64_t nrows,
                                                   int64_t n) {
    for (int64_t r = blockIdx.y; r < nrows; r += gridDim.y)
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
            dst[r * ld + i] = src[r * ld + i] - dst[r * ld + i];
}
// Observables into log space on the device (mbar.py:858-867 shifts every observable to be positive, :886-903 takes its log):
//   level 1: part[r][blockIdx.x] = min over a slice of row r;
//   level 2: shift_r = min_r - |4 eps min_r| (so that the smallest shifted value is a positive number of relative size 4 eps, or
//            zero when the minimum is zero -- the reference's choice), row r <- log(row r - shift_r) in place, shift_r handed back.
__global__ void __launch_bounds__(256) k_rows_min_partial(const double* __restrict__ base, int64_t ld, int64_t nrows, int64_t n,
                                                          double* __restrict__ part) {
    __shared__ double red[4];
    for (int64_t r = blockIdx.y; r < nrows; r += gridDim.y) {
        double m = INFINITY;
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
            m = fmin(m, base[r * ld + i]);
        m = -block256_max(-m, red);
        if (threadIdx.x == 0) part[r * gridDim.x + blockIdx.x] = m;
        __syncthreads();
    }
}
// The shift of observable row r from its `nparts` partial minima, for every thread of the workgroup; block x = 0 hands it back.
__device__ __forceinline__ double row_shift(const double* __restrict__ part, int nparts, int64_t r, double* red /*[4]*/,
                                            double* __restrict__ shift_out) {
    double m = INFINITY;
    for (int i = threadIdx.x; i < nparts; i += blockDim.x) m = fmin(m, part[r * nparts + i]);
    m = -block256_max(-m, red);
    const double shift = m - fabs(8.881784197001252e-16 * m);  // 4 eps (mbar.py:827-832)
    if (blockIdx.x == 0 && threadIdx.x == 0) shift_out[r] = shift;
    return shift;
}
__global__ void __launch_bounds__(256) k_rows_logshift(double* __restrict__ base, int64_t ld, int64_t nrows, int64_t n,
                                                       const double* __restrict__ part, int nparts, double* __restrict__ shift_out) {
    __shared__ double red[4];
    for (int64_t r = blockIdx.y; r < nrows; r += gridDim.y) {
        const double shift = row_shift(part, nparts, r, red, shift_out);
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
            base[r * ld + i] = log(base[r * ld + i] - shift);
        __syncthreads();
    }
}
// dst_r = state_r - log(obs_r - shift_r) with shift_r as in k_rows_logshift, from the same partial minima: observables that are rows of
// a resident matrix, each at its own state, written straight into the rows of an extension context (mbar_ctx_rows_obs_from)
__global__ void __launch_bounds__(256) k_rows_obs(double* __restrict__ dst, const double* __restrict__ obs, const double* __restrict__ state,
                                                  int64_t ld, int64_t nrows, int64_t n, const double* __restrict__ part, int nparts,
                                                  double* __restrict__ shift_out) {
    __shared__ double red[4];
    for (int64_t r = blockIdx.y; r < nrows; r += gridDim.y) {
        const double shift = row_shift(part, nparts, r, red, shift_out);
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
            dst[r * ld + i] = state[r * ld + i] - log(obs[r * ld + i] - shift);
        __syncthreads();
    }
}


// ---------------------------------------------------------------------------------------------
// host-side launchers
// ---------------------------------------------------------------------------------------------

// Workgroups of a grid-stride pass over n items, per_block to a workgroup: at least one, at most cap
static unsigned blocks_for(int64_t n, int64_t per_block, int64_t cap) {
    const int64_t want = (n + per_block - 1) / per_block;
    return (unsigned)(want < 1 ? 1 : want > cap ? cap : want);
}

// Levels of a record sum.  Up to 32 records are added by one launch; more go in chunks of 32 into n1 chunk sums (grid.y = n1),
// which a second launch adds up.  first_only: the caller adds the chunk sums itself, whatever their number.
struct ReduceLevels {
    int64_t chunk;  // records per workgroup of the first launch
    int64_t n1;     // sums it leaves per element (1: they are the result)
};
static ReduceLevels reduce_levels(int64_t nparts, bool first_only = false) {
    if (nparts <= 32 && !first_only) return {nparts, 1};
    return {32, (nparts + 31) / 32};
}

hipError_t launch_reduce(hipStream_t s, const double* part, int64_t nparts, int64_t count, double* scratch,
                         double* out) {
    const unsigned gx = (unsigned)((count + 255) / 256);
    const ReduceLevels lv = reduce_levels(nparts);
    hipLaunchKernelGGL(k_reduce, dim3(gx, (unsigned)lv.n1), dim3(256), 0, s, part, nparts, count, lv.chunk, lv.n1 > 1 ? scratch : out);
    if (lv.n1 > 1) hipLaunchKernelGGL(k_reduce, dim3(gx, 1), dim3(256), 0, s, (const double*)scratch, lv.n1, count, lv.n1, out);
    return hipGetLastError();
}

// first level only of the two-level reduction: out[c][i] = sum over the c-th chunk of 32 records; returns #chunks
hipError_t launch_reduce_level1(hipStream_t s, const double* part, int64_t nparts, int64_t count, double* out,
                                int64_t* nchunks) {
    const ReduceLevels lv = reduce_levels(nparts, true);
    const unsigned gx = (unsigned)((count + 255) / 256);
    hipLaunchKernelGGL(k_reduce, dim3(gx, (unsigned)lv.n1), dim3(256), 0, s, part, nparts, count, lv.chunk, out);
    *nchunks = lv.n1;
    return hipGetLastError();
}

hipError_t launch_reduce2(hipStream_t s, const double* partA, int64_t countA, const double* partB, int64_t countB,
                          int64_t nparts, double* scratch, double* outA, double* outB) {
    const unsigned gx = (unsigned)((countA + 255) / 256 + (countB + 255) / 256);
    const ReduceLevels lv = reduce_levels(nparts);
    double* midA = lv.n1 > 1 ? scratch : outA;
    double* midB = lv.n1 > 1 ? scratch + lv.n1 * countA : outB;
    hipLaunchKernelGGL(k_reduce2, dim3(gx, (unsigned)lv.n1), dim3(256), 0, s, partA, countA, partB, countB, nparts, lv.chunk, midA, midB);
    if (lv.n1 > 1)
        hipLaunchKernelGGL(k_reduce2, dim3(gx, 1), dim3(256), 0, s, (const double*)midA, countA, (const double*)midB, countB, lv.n1,
                           lv.n1, outA, outB);
    return hipGetLastError();
}

// Sample ranges of the per-state log-space reduction: enough waves (state-row groups x ranges) to fill the chip a few
// times over, each with a long run of tiles.
static int64_t lognum_tiles_per_chunk(int64_t N, int64_t K) {
    const int64_t ntiles = (N + LN_TILE - 1) / LN_TILE;
    const int64_t nsb = (K + LN_ROWS - 1) / LN_ROWS;
    int64_t target = 16384 / nsb;
    if (target < 1) target = 1;
    int64_t tpc = (ntiles + target - 1) / target;
    return tpc < 1 ? 1 : tpc;
}
int64_t lognum_chunks(int64_t N, int64_t K) {
    const int64_t ntiles = (N + LN_TILE - 1) / LN_TILE;
    const int64_t tpc = lognum_tiles_per_chunk(N, K);
    const int64_t n = (ntiles + tpc - 1) / tpc;
    return n < 1 ? 1 : n;  // (an empty shard still launches: its record is (max = -inf, sum = 0))
}

hipError_t launch_lognum(hipStream_t s, const double* u, int64_t ld, int64_t N, int64_t K, const double* anum,
                         const double* logden, double* pmax, double* psum, int64_t nchunks) {
    const int64_t nsb = (K + LN_ROWS - 1) / LN_ROWS;
    const int64_t waves = nsb * nchunks;
    hipLaunchKernelGGL(k_lognum, dim3((unsigned)((waves + 3) / 4)), dim3(256), EXP_TABLE_BYTES, s, u, ld, N, K, anum, logden, pmax,
                       psum, nchunks, lognum_tiles_per_chunk(N, K));
    return hipGetLastError();
}

hipError_t launch_lognum_merge(hipStream_t s, const double* pmax, const double* psum, int64_t K, int64_t nchunks,
                               double* out_max, double* out_sum) {
    hipLaunchKernelGGL(k_lognum_merge, dim3((unsigned)K), dim3(256), 0, s, pmax, psum, nchunks, out_max, out_sum);
    return hipGetLastError();
}

hipError_t launch_logw(hipStream_t s, const double* u, int64_t ld, int64_t N, int64_t K, const double* f,
                       const double* logden, double* out, int64_t ld_out, bool exponentiate) {
    const dim3 grid(blocks_for(N, 256, 2048), (unsigned)K);
    if (exponentiate)
        hipLaunchKernelGGL(k_logw<true>, grid, dim3(256), 0, s, u, ld, N, f, logden, out, ld_out);
    else
        hipLaunchKernelGGL(k_logw<false>, grid, dim3(256), 0, s, u, ld, N, f, logden, out, ld_out);
    return hipGetLastError();
}

hipError_t launch_check_u(hipStream_t s, const double* u, int64_t ld, int64_t N, int64_t K, int* flags) {
    hipLaunchKernelGGL(k_check_u, dim3(blocks_for(N, 256, 1024), (unsigned)K), dim3(256), 0, s, u, ld, N, flags);
    return hipGetLastError();
}

hipError_t launch_shift_logden(hipStream_t s, const double* logden, const double* cw, double alpha, int64_t N,
                               double* out, const LoopCtl& lc) {
    hipLaunchKernelGGL(k_shift_logden, dim3(blocks_for(N, 256, 2048)), dim3(256), 0, s, logden, cw, alpha, N, out, lc.ctl,
                       lc.slot_stride);
    return hipGetLastError();
}

hipError_t launch_fill(hipStream_t s, double* v, double value, int64_t n) {
    hipLaunchKernelGGL(k_fill, dim3(blocks_for(n, 256, 2048)), dim3(256), 0, s, v, value, n);
    return hipGetLastError();
}
hipError_t launch_zero(hipStream_t s, void* p, size_t bytes) {
    if (bytes == 0) return hipSuccess;
    if ((bytes & 15) != 0 || ((uintptr_t)p & 15) != 0 || bytes < (size_t)1 << 16) return hipMemsetAsync(p, 0, bytes, s);
    const size_t n16 = bytes / 16;
    hipLaunchKernelGGL(k_zero16, dim3(blocks_for((int64_t)n16, 256, 8192)), dim3(256), 0, s, (uint4*)p, n16);
    return hipGetLastError();
}
hipError_t launch_sqrt_vec(hipStream_t s, double* dst, const double* src, int64_t n) {
    hipLaunchKernelGGL(k_sqrt_vec, dim3(blocks_for(n, 256, 2048)), dim3(256), 0, s, dst, src, n);
    return hipGetLastError();
}
hipError_t launch_weights_from_log(hipStream_t s, const double* v, double p, int64_t n, double* cw, double* cwsq, int* overflow) {
    hipLaunchKernelGGL(k_weights_from_log, dim3(blocks_for(n, 256, 2048)), dim3(256), 0, s, v, p, n, cw, cwsq, overflow);
    return hipGetLastError();
}

hipError_t launch_generate_harmonic(hipStream_t s, double* u, int64_t ld, int64_t N, int64_t K, uint64_t seed,
                                    const double* O_k, const double* K_k, const int64_t* cumN,
                                    int64_t n_global0) {
    hipLaunchKernelGGL(k_generate_harmonic, dim3(blocks_for(N, 256, 4096)), dim3(256), 0, s, u, ld, N, K, seed, O_k, K_k, cumN,
                       n_global0);
    return hipGetLastError();
}
hipError_t launch_bootstrap_counts(hipStream_t s, uint64_t seed, int64_t replicate, const int64_t* cum, int64_t K, int64_t total,
                                   const int64_t* order, int64_t n0, int64_t N, double* cw) {
    hipLaunchKernelGGL(k_bootstrap_counts, dim3(blocks_for(total, 256, 4096)), dim3(256), 0, s, seed, replicate, cum, K, total, order, n0,
                       N, cw);
    return hipGetLastError();
}

hipError_t launch_mfma_peak(hipStream_t s, int blocks, int iters, double* sink) {
    hipLaunchKernelGGL(k_mfma_peak, dim3(blocks), dim3(256), 0, s, iters, sink);
    return hipGetLastError();
}
hipError_t launch_make_p(hipStream_t s, int num_cu, const double* u, int64_t ld, int64_t N, int64_t rows, const double* aden,
                         const double* logden, double* P) {
    hipLaunchKernelGGL(k_make_p, dim3((unsigned)(num_cu * 8)), dim3(256), 0, s, u, ld, N, rows, aden, logden, P);
    return hipGetLastError();
}

hipError_t launch_fill_masked_rows(hipStream_t s, double* rows, int64_t ld, int64_t n, int64_t nrows, const double* v,
                                   const int* label) {
    hipLaunchKernelGGL(k_fill_masked_rows, dim3(blocks_for(n, 256, 2048), (unsigned)nrows), dim3(256), 0, s, rows, ld, n, v, label);
    return hipGetLastError();
}
hipError_t launch_rows_sub(hipStream_t s, double* dst, const double* src, int64_t ld, int64_t nrows, const double* v, int64_t n) {
    hipLaunchKernelGGL(k_rows_sub, dim3(blocks_for(n, 256, 2048), blocks_for(nrows, 1, 1024)), dim3(256), 0, s, dst, src, ld, nrows, v, n);
    return hipGetLastError();
}
// row[i] -= v[i]: one row in place, with a grid of its own (up to 4096 workgroups)
hipError_t launch_row_sub(hipStream_t s, double* row, const double* v, int64_t n) {
    hipLaunchKernelGGL(k_rows_sub, dim3(blocks_for(n, 256, 4096), 1), dim3(256), 0, s, row, (const double*)row, (int64_t)0, (int64_t)1, v, n);
    return hipGetLastError();
}
hipError_t launch_rows_rsub(hipStream_t s, double* dst, const double* src, int64_t ld, int64_t nrows, int64_t n) {
    hipLaunchKernelGGL(k_rows_rsub, dim3(blocks_for(n, 256, 2048), blocks_for(nrows, 1, 1024)), dim3(256), 0, s, dst, src, ld, nrows, n);
    return hipGetLastError();
}
hipError_t launch_rows_logshift(hipStream_t s, double* base, int64_t ld, int64_t nrows, int64_t n, double* part, double* shift_out) {
    const dim3 grid(blocks_for(n, 2048, 256), blocks_for(nrows, 1, 1024));
    hipLaunchKernelGGL(k_rows_min_partial, grid, dim3(256), 0, s, base, ld, nrows, n, part);
    hipLaunchKernelGGL(k_rows_logshift, grid, dim3(256), 0, s, base, ld, nrows, n, part, (int)grid.x, shift_out);
    return hipGetLastError();
}
// have_min: part[r] already holds the minimum of observable row r (one entry per row: the caller kept it from an earlier call on
// the same resident rows) -- the pass over the rows that finds it is skipped
hipError_t launch_rows_obs(hipStream_t s, double* dst, const double* obs, const double* state, int64_t ld, int64_t nrows, int64_t n,
                           double* part, double* shift_out, bool have_min) {
    const dim3 grid(blocks_for(n, 2048, 256), blocks_for(nrows, 1, 1024));
    if (!have_min) hipLaunchKernelGGL(k_rows_min_partial, grid, dim3(256), 0, s, obs, ld, nrows, n, part);
    hipLaunchKernelGGL(k_rows_obs, grid, dim3(256), 0, s, dst, obs, state, ld, nrows, n, (const double*)part, have_min ? 1 : (int)grid.x,
                       shift_out);
    return hipGetLastError();
}

}  // namespace mbar
