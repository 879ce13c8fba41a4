// gfx950 (CDNA4 / MI355X) kernels of the histogram surfaces by bin LABEL (pymbar_amd.fes.histogram_fes_labels): a bin is a label
// of the samples, not a row of a second matrix.  One of the translation units of libmbar_hip.so; the host side (chunk table,
// C ABI) is mbar_hist.cpp, the launcher declarations are in mbar_hist.h.  DESIGN.md section 16 has the derivation.
//
//   pass A   lognum_bin[i] = log sum_{n in bin i} c_n exp(-v_n - logden_n)            (three N-vectors, no matrix)
//   pass B   cross[k][i]   = sum_{n in bin i} c_n W_nk B_n,   W_nk = exp(f_k - u_kn - logden_n),  B_n = exp(f_bin[label_n] - v_n - logden_n)
//            wsum_bin[i]   = sum_{n in bin i} c_n B_n,        diag[i] = sum_{n in bin i} c_n B_n^2
//
// Chunk table (host, O(N), once per label array).  The samples are cut into contiguous chunks of at most HIST_CHUNK_SAMPLES
// samples that touch at most HIST_SLOTS = 64 distinct bins; slot[n] numbers the bins of a chunk in order of first appearance
// (HIST_NO_SLOT: the sample is in no bin of this sweep).  Chunk c owns the records chunk_rec[c] .. chunk_rec[c + 1], one per slot.
//
// Sums.  ONE wave owns a chunk (pass B: a chunk and HIST_ROWS rows of the matrix) and lane s owns the accumulators of slot s, in
// registers: no LDS accumulators, no atomics.  The wave walks the chunk in steps of 64 samples with lanes along n (coalesced, the
// matrix in its natural order).  Per step, the lowest remaining lane's slot is reduced over its lanes by the fixed xor butterfly
// and added by the owning lane, up to HIST_ROUNDS times (data ordered by state: one or a few slots per step); samples still left
// after that are handed to their owning lanes one at a time, in ascending n (v_readlane of a wave-uniform index).  The combine
// kernels merge a bin's records in chunk order through the host-built bin -> record list (compensated sums; maxima for the first
// half of pass A).  Every order is a function of the labels, N, K and the record budget only: two identical calls return
// identical bits.
//
// Pass A takes the maximum per BIN first (records of maxima, merged), then sums exp(x - max_bin): every term costs one
// exponential whose argument is <= 0, and a bin whose terms all underflow against the global maximum keeps its finite value.
#include "mbar_device.h"
#include "mbar_hist.h"

namespace mbar {

namespace {
constexpr int HV_THREADS = 256;
constexpr int HIST_ROUNDS = 8;  // butterflies per step before the per-sample hand-over (a butterfly costs about eight hand-overs)

__device__ __forceinline__ double hist_exp(double x) { return exp2s_fast(x * LOG2E_S); }

// value of lane j (wave-uniform j)
__device__ __forceinline__ double hist_readlane(double x, int j) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), j);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), j);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ void hist_neumaier(double& s, double& e, double v) {
    const double t = s + v;
    e += fabs(s) >= fabs(v) ? (s - t) + v : (v - t) + s;
    s = t;
}
}  // namespace

// One wave per chunk.  MODE HIST_MAX: rec_a = max of x_n = -v_n - logden_n over the slot's samples with c_n > 0;
// HIST_SUMEXP: rec_a = sum c_n exp(x_n - bin_in[label_n]);  HIST_NORM: rec_a = sum c_n B_n, rec_b = sum c_n B_n^2 with
// B_n = exp(bin_in[label_n] + x_n).
template <int MODE>
__global__ void __launch_bounds__(HV_THREADS)
k_hist_vec(HistSweep h, const double* __restrict__ bin_in, double* __restrict__ rec_a, double* __restrict__ rec_b) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    exp_table_init(smem);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t c = (int64_t)blockIdx.x * (HV_THREADS / 64) + wave;
    if (c >= h.nchunks) return;
    const int64_t n0 = h.chunk_n[c], n1 = h.chunk_n[c + 1];
    const int64_t r0 = h.chunk_rec[c];
    const int nb = (int)(h.chunk_rec[c + 1] - r0);
    if (nb <= 0) return;
    double a = MODE == HIST_MAX ? -INFINITY : 0.0, b = 0.0;
    for (int64_t base = n0; base < n1; base += 64) {
        const int64_t n = base + lane;
        int sl = n < n1 ? (int)h.slot[n] : HIST_NO_SLOT;
        double cn = 0.0;
        if (sl != HIST_NO_SLOT) cn = h.cw ? h.cw[n] : 1.0;
        if (!(cn > 0.0)) sl = HIST_NO_SLOT;
        double x = MODE == HIST_MAX ? -INFINITY : 0.0, y = 0.0;
        if (sl != HIST_NO_SLOT) {
            const double arg = -h.v[n] - h.logden[n];
            if (MODE == HIST_MAX) {
                x = arg;
            } else if (MODE == HIST_SUMEXP) {
                x = cn * hist_exp(arg - bin_in[h.label[n]]);
            } else {
                const double B = hist_exp(bin_in[h.label[n]] + arg);
                x = cn * B;
                y = x * B;
            }
        }
        // up to HIST_ROUNDS distinct slots: one butterfly each (the lowest remaining lane's slot first) ...
        uint64_t left = __ballot(sl != HIST_NO_SLOT);
        for (int round = 0; left && round < HIST_ROUNDS; ++round) {
            const int sj = __builtin_amdgcn_readlane(sl, __ffsll((unsigned long long)left) - 1);
            const bool mine = sl == sj;
            if (MODE == HIST_MAX) {
                const double t = wave_max(mine ? x : -INFINITY);
                if (lane == sj) a = fmax(a, t);
            } else {
                const double t = wave_sum(mine ? x : 0.0);
                if (lane == sj) a += t;
                if (MODE == HIST_NORM) {
                    const double t2 = wave_sum(mine ? y : 0.0);
                    if (lane == sj) b += t2;
                }
            }
            left &= ~__ballot(mine);
        }
        // ... the samples left after that go to their owning lanes one at a time, in ascending n
        while (left) {
            const int j = __ffsll((unsigned long long)left) - 1;
            left &= left - 1;
            const int sj = __builtin_amdgcn_readlane(sl, j);
            const double xj = hist_readlane(x, j);
            if (MODE == HIST_MAX) {
                if (lane == sj) a = fmax(a, xj);
            } else {
                if (lane == sj) a += xj;
                if (MODE == HIST_NORM) {
                    const double yj = hist_readlane(y, j);
                    if (lane == sj) b += yj;
                }
            }
        }
    }
    if (lane < nb) {
        rec_a[r0 + lane] = a;
        if (MODE == HIST_NORM) rec_b[r0 + lane] = b;
    }
}

// One thread per bin of the sweep's tile [b0, b1): its records merged in chunk order.  HIST_MAX: out_a = the maximum (-inf: no
// record); HIST_SUMEXP: out_a = binmax + log(sum) (-inf when the sum is 0); HIST_NORM: out_a, out_b = the two sums.
template <int MODE>
__global__ void __launch_bounds__(HV_THREADS)
k_hist_vec_combine(HistSweep h, const double* __restrict__ rec_a, const double* __restrict__ rec_b, const double* __restrict__ binmax,
                   double* __restrict__ out_a, double* __restrict__ out_b) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    exp_table_init(smem);
    __syncthreads();
    const int64_t i = h.b0 + (int64_t)blockIdx.x * HV_THREADS + threadIdx.x;
    if (i >= h.b1) return;
    const int64_t p0 = h.bin_ptr[i], p1 = h.bin_ptr[i + 1];
    if (MODE == HIST_MAX) {
        double m = -INFINITY;
        for (int64_t p = p0; p < p1; ++p) m = fmax(m, rec_a[h.bin_rec[p]]);
        out_a[i] = m;
        return;
    }
    double s = 0.0, e = 0.0, s2 = 0.0, e2 = 0.0;
    for (int64_t p = p0; p < p1; ++p) {
        const int64_t r = h.bin_rec[p];
        hist_neumaier(s, e, rec_a[r]);
        if (MODE == HIST_NORM) hist_neumaier(s2, e2, rec_b[r]);
    }
    s += e;
    if (MODE == HIST_SUMEXP) {
        out_a[i] = s > 0.0 ? binmax[i] + log_pos(s) : -INFINITY;
    } else {
        out_a[i] = s;
        out_b[i] = s2 + e2;
    }
}

// One wave per (chunk, HIST_ROWS rows): part[(chunk_rec[c] + s) * K + k] = sum over the chunk's samples of slot s of c_n W_nk B_n
__global__ void __launch_bounds__(64)
k_hist_cross(HistSweep h, const double* __restrict__ u, int64_t ld, int64_t K, const double* __restrict__ f,
             const double* __restrict__ f_bins, double* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    exp_table_init(smem);
    __syncthreads();
    const int lane = threadIdx.x;
    const int64_t c = blockIdx.x;
    const int64_t k0 = (int64_t)blockIdx.y * HIST_ROWS;
    const int64_t n0 = h.chunk_n[c], n1 = h.chunk_n[c + 1];
    const int64_t r0 = h.chunk_rec[c];
    const int nb = (int)(h.chunk_rec[c + 1] - r0);
    if (nb <= 0) return;
    double fk[HIST_ROWS], acc[HIST_ROWS];
#pragma unroll
    for (int r = 0; r < HIST_ROWS; ++r) {
        fk[r] = k0 + r < K ? f[k0 + r] : 0.0;
        acc[r] = 0.0;
    }
    for (int64_t base = n0; base < n1; base += 64) {
        const int64_t n = base + lane;
        int sl = n < n1 ? (int)h.slot[n] : HIST_NO_SLOT;
        double cn = 0.0;
        if (sl != HIST_NO_SLOT) cn = h.cw ? h.cw[n] : 1.0;
        if (!(cn > 0.0)) sl = HIST_NO_SLOT;
        const bool live = sl != HIST_NO_SLOT;
        double val[HIST_ROWS];
        double lden = 0.0, cb = 0.0;
        if (live) {
            lden = h.logden[n];
            cb = cn * hist_exp(f_bins[h.label[n]] - h.v[n] - lden);
        }
#pragma unroll
        for (int r = 0; r < HIST_ROWS; ++r) {
            double w = 0.0;
            if (live && k0 + r < K) w = hist_exp(fk[r] - u[(k0 + r) * ld + n] - lden) * cb;
            val[r] = w;
        }
        uint64_t left = __ballot(live);
        for (int round = 0; left && round < HIST_ROUNDS; ++round) {  // one butterfly per distinct slot, lowest remaining lane first
            const int sj = __builtin_amdgcn_readlane(sl, __ffsll((unsigned long long)left) - 1);
            const bool mine = sl == sj;
#pragma unroll
            for (int r = 0; r < HIST_ROWS; ++r) {
                const double t = wave_sum(mine ? val[r] : 0.0);
                if (lane == sj) acc[r] += t;
            }
            left &= ~__ballot(mine);
        }
        while (left) {  // more distinct slots than that: the remaining samples one at a time, in ascending n
            const int j = __ffsll((unsigned long long)left) - 1;
            left &= left - 1;
            const int sj = __builtin_amdgcn_readlane(sl, j);
#pragma unroll
            for (int r = 0; r < HIST_ROWS; ++r) {
                const double t = hist_readlane(val[r], j);
                if (lane == sj) acc[r] += t;
            }
        }
    }
    if (lane < nb) {
        double* out = part + (r0 + lane) * K + k0;
#pragma unroll
        for (int r = 0; r < HIST_ROWS; ++r)
            if (k0 + r < K) out[r] = acc[r];
    }
}

// cross[k][i] for the bins i of the tile: the records of bin i merged in chunk order (compensated)
__global__ void __launch_bounds__(HV_THREADS)
k_hist_cross_combine(HistSweep h, int64_t K, const double* __restrict__ part, double* __restrict__ cross) {
    const int64_t x = (int64_t)blockIdx.x * HV_THREADS + threadIdx.x;
    if (x >= (h.b1 - h.b0) * K) return;
    const int64_t i = h.b0 + x / K, k = x % K;
    double s = 0.0, e = 0.0;
    for (int64_t p = h.bin_ptr[i]; p < h.bin_ptr[i + 1]; ++p) hist_neumaier(s, e, part[h.bin_rec[p] * K + k]);
    cross[k * h.nbins + i] = s + e;
}

// ---- launchers -------------------------------------------------------------------------------------------------------------
hipError_t launch_hist_vec(hipStream_t s, const HistSweep& h, int mode, const double* bin_in, double* rec_a, double* rec_b) {
    if (h.nchunks < 1) return hipSuccess;
    const dim3 grid((unsigned)((h.nchunks + HV_THREADS / 64 - 1) / (HV_THREADS / 64)));
    if (mode == HIST_MAX) hipLaunchKernelGGL(k_hist_vec<HIST_MAX>, grid, dim3(HV_THREADS), EXP_TABLE_BYTES, s, h, bin_in, rec_a, rec_b);
    else if (mode == HIST_SUMEXP) hipLaunchKernelGGL(k_hist_vec<HIST_SUMEXP>, grid, dim3(HV_THREADS), EXP_TABLE_BYTES, s, h, bin_in, rec_a, rec_b);
    else if (mode == HIST_NORM) hipLaunchKernelGGL(k_hist_vec<HIST_NORM>, grid, dim3(HV_THREADS), EXP_TABLE_BYTES, s, h, bin_in, rec_a, rec_b);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_hist_vec_combine(hipStream_t s, const HistSweep& h, int mode, const double* rec_a, const double* rec_b,
                                   const double* binmax, double* out_a, double* out_b) {
    if (h.b1 <= h.b0) return hipSuccess;
    const dim3 grid((unsigned)((h.b1 - h.b0 + HV_THREADS - 1) / HV_THREADS));
    if (mode == HIST_MAX) hipLaunchKernelGGL(k_hist_vec_combine<HIST_MAX>, grid, dim3(HV_THREADS), EXP_TABLE_BYTES, s, h, rec_a, rec_b, binmax, out_a, out_b);
    else if (mode == HIST_SUMEXP) hipLaunchKernelGGL(k_hist_vec_combine<HIST_SUMEXP>, grid, dim3(HV_THREADS), EXP_TABLE_BYTES, s, h, rec_a, rec_b, binmax, out_a, out_b);
    else if (mode == HIST_NORM) hipLaunchKernelGGL(k_hist_vec_combine<HIST_NORM>, grid, dim3(HV_THREADS), EXP_TABLE_BYTES, s, h, rec_a, rec_b, binmax, out_a, out_b);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_hist_cross(hipStream_t s, const HistSweep& h, const double* u, int64_t ld, int64_t K, const double* f,
                             const double* f_bins, double* part) {
    if (h.nchunks < 1 || K < 1) return hipSuccess;
    if (h.nchunks > 0x7fffffff) return hipErrorInvalidValue;
    const dim3 grid((unsigned)h.nchunks, (unsigned)((K + HIST_ROWS - 1) / HIST_ROWS));
    if (grid.y > 65535u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_hist_cross, grid, dim3(64), EXP_TABLE_BYTES, s, h, u, ld, K, f, f_bins, part);
    return hipGetLastError();
}

hipError_t launch_hist_cross_combine(hipStream_t s, const HistSweep& h, int64_t K, const double* part, double* cross) {
    const int64_t len = (h.b1 - h.b0) * K;
    if (len < 1) return hipSuccess;
    hipLaunchKernelGGL(k_hist_cross_combine, dim3((unsigned)((len + HV_THREADS - 1) / HV_THREADS)), dim3(HV_THREADS), 0, s, h, K, part, cross);
    return hipGetLastError();
}

}  // namespace mbar
