// gfx950 (CDNA4 / MI355X) kernels of the histogram free energy surfaces along a scan (MBAR.compute_scan_fes): the scan passes of
// mbar_k_scan.hip with the samples sorted by histogram bin, so that every (member, bin) pair gets the sums a member gets there.
// One of the translation units of libmbar_hip.so; the host side (sort, chunk tables, bin groups, C ABI) is mbar_scanbin.cpp, the
// launcher declarations are in mbar_internal.h.  DESIGN.md section 18 has the layout and the cost model.
//
//   x_ln = -u_l(n) - logden_n,  u_l(n) = fma(coeff[l][B-1], basis[B-1][n], ... fma(coeff[l][0], basis[0][n], offset[l]))   (Q = 0)
//
//   pass A   M_li = max_{n in i: c_n > 0} x_ln,  lognum[l][i] = M_li + log sum_{n in i} c_n exp(x_ln - M_li)      (no matrix)
//   pass B   Bv = exp(f_bins[l][i] + x_ln) for n in i,  W_nk = exp(f_k - u_kn - logden_n)
//            cross[k][l][i] = sum_{n in i} c_n W_nk Bv        fp64 matrix cores: A operand = W tile, B operand = c Bv, from registers
//            diag[l][i] = sum c_n Bv^2,  wsum[l][i] = sum c_n Bv
//
// Layout.  perm lists the samples bin by bin, ascending n inside a bin (a stable counting sort on the host; label -1 dropped).  A
// chunk is a run of sorted positions of ONE bin, cut from the start of the bin: at most SCAN_VCHUNK positions in pass A, SCAN_CHUNK
// in pass B.  Pass A is k_scan_vec with n = perm[p] (still wave-uniform loads); pass B is k_scan_cross at J = 1 whose tile is 16
// consecutive sorted positions: the W tile and the basis values are gathered through perm, positions past the bin's end carry
// c = 0, and the reference column is gone.
//
// Order.  A (member, bin) output is the same sequence of operations on the bin's own samples in ascending n whatever the other
// members, the other bins, the bin's number, the panel or the bin group are; the merge kernels add a (member, bin)'s chunk records
// in chunk order (compensated).  With one bin that holds every sample the chunks are the chunks of mbar_k_scan.hip and the
// operations are its operations: the outputs are the bits of mbar_scan_lognum / mbar_scan_gram_w.  No atomics.  Every fused
// multiply-add is written as one and nothing else is contracted, for the reason given in mbar_k_scan.hip.
#include "mbar_device.h"

#pragma clang fp contract(off)

namespace mbar {

namespace {
// sorted positions [p0, p1) of chunk c of a table whose chunks hold at most `len` positions, and its bin
__device__ __forceinline__ void chunk_range(const ScanBins& sb, const ScanBinTable& t, int64_t c, int64_t len, int64_t& bin, int64_t& p0,
                                            int64_t& p1) {
    bin = t.chunk_bin[c];
    const int64_t end = sb.bin_start[bin + 1];
    p0 = sb.bin_start[bin] + (c - t.bin_chunk0[bin]) * len;
    p1 = p0 + len < end ? p0 + len : end;
}
}  // namespace

// One wave per (chunk, 64 members).  SUM = false: rec[chunk][l] = max of x_ln over the chunk's samples with c_n > 0; SUM = true:
// rec[chunk][l] = sum c_n exp(x_ln - M[bin][l]).
template <bool SUM>
__global__ void __launch_bounds__(SV_THREADS)
k_scanbin_vec(ScanData d, ScanBins sb, ScanBinTable t, int64_t L, const double* __restrict__ coeff, const double* __restrict__ offset,
              const double* __restrict__ M, double* __restrict__ rec) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (SUM) {
        exp_table_init(smem);
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t c = (int64_t)blockIdx.x * (SV_THREADS / 64) + wave;
    if (c >= t.nchunks) return;
    int64_t bin, p0, p1;
    chunk_range(sb, t, c, SCAN_VCHUNK, bin, p0, p1);
    const int64_t l = (int64_t)blockIdx.y * 64 + lane;
    const bool live = l < L;
    double cf[SCAN_MAX_B];
#pragma unroll
    for (int b = 0; b < SCAN_MAX_B; ++b) cf[b] = (live && b < d.B) ? coeff[l * d.B + b] : 0.0;
    const double off = live ? offset[l] : 0.0;
    const double Ml = (SUM && live) ? M[bin * L + l] : 0.0;
    double acc = SUM ? 0.0 : -INFINITY;
    for (int64_t p = p0; p < p1; ++p) {  // (p is wave-uniform: perm and the per-sample values are scalar loads)
        const int64_t n = sb.perm[p];
        const double cn = d.cw ? d.cw[n] : 1.0;
        if (!(cn > 0.0)) continue;
        const double x = scan_x(d, cf, off, n);
        if (!SUM) {
            acc = fmax(acc, x);
        } else {
            const double e = cn * scan_exp(x - Ml);
            acc += e;
        }
    }
    if (live) rec[c * L + l] = acc;
}

// One thread per (bin, member): its chunk records merged in chunk order.  SUM = false: M[bin][l] = the maximum; SUM = true:
// lognum[l][bin] = M + log S (-inf when no sample of the bin has c_n > 0).
template <bool SUM>
__global__ void __launch_bounds__(SV_THREADS)
k_scanbin_vec_merge(ScanBins sb, ScanBinTable t, int64_t L, const double* __restrict__ rec, double* __restrict__ M,
                    double* __restrict__ lognum) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (SUM) {
        exp_table_init(smem);
        __syncthreads();
    }
    const int64_t x = (int64_t)blockIdx.x * SV_THREADS + threadIdx.x;
    if (x >= sb.nbins * L) return;
    const int64_t l = x % L, bin = x / L;
    const int64_t c0 = t.bin_chunk0[bin], c1 = t.bin_chunk0[bin + 1];
    if (!SUM) {
        double m = -INFINITY;
        for (int64_t c = c0; c < c1; ++c) m = fmax(m, rec[c * L + l]);
        M[bin * L + l] = m;
        return;
    }
    double s = 0.0, e = 0.0;
    for (int64_t c = c0; c < c1; ++c) scan_neumaier(s, e, rec[c * L + l]);
    s += e;
    lognum[l * sb.nbins + bin] = s > 0.0 ? M[bin * L + l] + log_pos(s) : -INFINITY;
}

// ---- pass B --------------------------------------------------------------------------------------------------------------------
// Record of one workgroup (one chunk of SCAN_CHUNK sorted positions of a bin, panel of 256 members), NCB = 4 column blocks per wave:
//   cross part  [wave][I < NB][mb < 4][r < 4][lane]   the MFMA accumulators as they are: element (state 16 I + (lane >> 4) + 4 r,
//                                                     member block mb, column lane & 15)
//   vec part    [pm < 256][SCANBIN_NV]                wsum | diag
// Member pm of the panel sits in block pm / 16 = mb * 4 + wave, as in k_scan_cross.
template <int NB>
__global__ void __launch_bounds__(256)
k_scanbin_cross(ScanData d, ScanBins sb, ScanBinTable t, int64_t c0, const double* __restrict__ u, int64_t ld, int64_t K,
                const double* __restrict__ f, int64_t L, int64_t p0, const double* __restrict__ coeff, const double* __restrict__ offset,
                const double* __restrict__ f_bins, double* __restrict__ part) {
    constexpr int MB = 4, NV = SCANBIN_NV;
    constexpr int W_DOUBLES = NB * 16 * SCAN_PITCH;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    exp_table_init(smem);
    double* Wt = reinterpret_cast<double*>(smem + EXP_TABLE_BYTES);  // [16 NB][SCAN_PITCH]
    double* sv = Wt + W_DOUBLES;                                     // cn[16] | lden[16] | basis[B][16]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 15, q4 = lane >> 4;
    int64_t bin, q0c, q1c;
    chunk_range(sb, t, c0 + blockIdx.x, SCAN_CHUNK, bin, q0c, q1c);
    // blocks of 16 members this wave owns, and how many of them hold a member at all
    const int64_t pl = L - p0 < 64 * MB ? L - p0 : 64 * MB;  // members of the panel
    const int nblk = (int)((pl + 15) / 16);
    int mine = 0;
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) mine += (mb * 4 + wave) < nblk;
    mine = __builtin_amdgcn_readfirstlane(mine);

    double cf[MB][SCAN_MAX_B], off[MB], fs[MB];
    bool mlive[MB];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
        const int64_t pm = (int64_t)(mb * 4 + wave) * 16 + col;
        mlive[mb] = pm < pl;
        const int64_t l = p0 + pm;
#pragma unroll
        for (int b = 0; b < SCAN_MAX_B; ++b) cf[mb][b] = (mlive[mb] && b < d.B) ? coeff[l * d.B + b] : 0.0;
        off[mb] = mlive[mb] ? offset[l] : 0.0;
        fs[mb] = mlive[mb] ? f_bins[l * sb.nbins + bin] : 0.0;
        if (fs[mb] == INFINITY) {  // an empty bin of this member: exact zeros
            mlive[mb] = false;
            fs[mb] = 0.0;
        }
    }
    // fill roles: thread tid forms W of state 16 I + (tid >> 4) at tile position tid & 15; threads 0 .. 15 also the sample's scalars
    const int fs_s = tid & 15, fs_r = tid >> 4;
    double fk[NB > 0 ? NB : 1];
#pragma unroll
    for (int I = 0; I < NB; ++I) fk[I] = 16 * I + fs_r < K ? f[16 * I + fs_r] : 0.0;

    v4d acc[NB > 0 ? NB * MB : 1];
#pragma unroll
    for (int i = 0; i < (NB > 0 ? NB * MB : 1); ++i) acc[i] = v4d{0.0, 0.0, 0.0, 0.0};
    double vs[MB][NV];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int v = 0; v < NV; ++v) vs[mb][v] = 0.0;

    __syncthreads();  // the exp table
    for (int64_t q0 = q0c; q0 < q1c; q0 += 16) {
        // ---- fill: the gathered W tile and the per-sample values of the tile
        {
            const int64_t q = q0 + fs_s;
            int64_t n = 0;
            double cn = 0.0, lden = 0.0;
            if (q < q1c) {
                n = sb.perm[q];
                cn = d.cw ? d.cw[n] : 1.0;
                if (cn > 0.0) lden = d.logden[n];
                else cn = 0.0;
            }
            const bool slive = cn > 0.0;
#pragma unroll
            for (int I = 0; I < NB; ++I) {
                const int64_t k = 16 * I + fs_r;
                double w = 0.0;
                if (slive && k < K) w = scan_exp(fk[I] - u[k * ld + n] - lden);
                Wt[(16 * I + fs_r) * SCAN_PITCH + fs_s] = w;
            }
            if (tid < 16) {
                sv[fs_s] = cn;
                sv[16 + fs_s] = lden;
            }
            if (fs_r < d.B) sv[32 + fs_r * 16 + fs_s] = slive ? d.basis[(int64_t)fs_r * d.ldv + n] : 0.0;
        }
        __syncthreads();
        // ---- products: four groups of four positions
        if (mine > 0) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int s = 4 * g + q4;
                double a[NB > 0 ? NB : 1];
#pragma unroll
                for (int I = 0; I < NB; ++I) a[I] = Wt[(16 * I + col) * SCAN_PITCH + s];
                const double cn = sv[s], lden = sv[16 + s];
                double bas[SCAN_MAX_B];
#pragma unroll
                for (int b = 0; b < SCAN_MAX_B; ++b) bas[b] = b < d.B ? sv[32 + b * 16 + s] : 0.0;
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) {
                    if (mb < mine) {  // (wave-uniform)
                        double uu = off[mb];
#pragma unroll
                        for (int b = 0; b < SCAN_MAX_B; ++b)
                            if (b < d.B) uu = fma(cf[mb][b], bas[b], uu);
                        double bv = scan_exp(fs[mb] + (-uu - lden));
                        if (!(cn > 0.0) || !mlive[mb]) bv = 0.0;
                        const double cb = cn * bv;
                        vs[mb][0] += cb;
                        vs[mb][1] = fma(bv, cb, vs[mb][1]);
#pragma unroll
                        for (int I = 0; I < NB; ++I)
                            acc[I * MB + mb] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[I], cb, acc[I * MB + mb], 0, 0, 0);
                    }
                }
            }
        }
        __syncthreads();
    }
    // ---- the record
    constexpr int64_t CROSS_DOUBLES = (int64_t)4 * NB * MB * 256;
    double* rec = part + (int64_t)blockIdx.x * (CROSS_DOUBLES + (int64_t)64 * MB * NV);
#pragma unroll
    for (int i = 0; i < NB * MB; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) rec[(((int64_t)wave * NB * MB + i) * 4 + r) * 64 + lane] = acc[i][r];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            double x = vs[mb][v];
            x += __shfl_xor(x, 16);
            x += __shfl_xor(x, 32);
            if (lane < 16) rec[CROSS_DOUBLES + ((int64_t)(mb * 4 + wave) * 16 + lane) * NV + v] = x;
        }
}

// The records of the panel and of the bins [b0, b1) merged per bin in chunk order (c0: the first chunk of bin b0, record 0).
// Threads [0, nb pl K): cross[k][p0 + pm][bin]; threads behind them, [0, nb pl NV): vec[p0 + pm][bin][v].
__global__ void __launch_bounds__(SV_THREADS)
k_scanbin_cross_merge(ScanBins sb, ScanBinTable t, int64_t c0, int64_t b0, int64_t b1, int NB, int64_t K, int64_t L, int64_t p0, int64_t pl,
                      const double* __restrict__ part, double* __restrict__ cross, double* __restrict__ vec) {
    constexpr int MB = 4, NV = SCANBIN_NV;
    const int64_t cross_doubles = (int64_t)4 * NB * MB * 256, stride = cross_doubles + (int64_t)64 * MB * NV;
    const int64_t nbg = b1 - b0, ncross = NB > 0 ? nbg * pl * K : 0;
    int64_t x = (int64_t)blockIdx.x * SV_THREADS + threadIdx.x;
    int64_t at, bin;
    double* out;
    if (x < ncross) {
        const int64_t pm = x % pl, k = (x / pl) % K;
        bin = b0 + x / (pl * K);
        const int64_t blk = pm / 16, colm = pm % 16, wave = blk % 4, mb = blk / 4;
        const int64_t I = k / 16, row = k % 16, r = row >> 2, lane = (row & 3) * 16 + colm;
        at = (((wave * NB + I) * MB + mb) * 4 + r) * 64 + lane;
        out = cross + (k * L + p0 + pm) * sb.nbins + bin;
    } else {
        x -= ncross;
        if (x >= nbg * pl * NV) return;
        const int64_t pm = x % pl, v = (x / pl) % NV;
        bin = b0 + x / (pl * NV);
        at = cross_doubles + pm * NV + v;
        out = vec + ((p0 + pm) * sb.nbins + bin) * NV + v;
    }
    double s = 0.0, e = 0.0;
    for (int64_t c = t.bin_chunk0[bin]; c < t.bin_chunk0[bin + 1]; ++c) scan_neumaier(s, e, part[(c - c0) * stride + at]);
    *out = s + e;
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------
hipError_t launch_scanbin_vec(hipStream_t s, const ScanData& d, const ScanBins& sb, const ScanBinTable& t, bool sum, int64_t L,
                              const double* coeff, const double* offset, const double* M, double* rec) {
    if (L < 1 || t.nchunks < 1) return hipSuccess;
    const int64_t gx = (t.nchunks + SV_THREADS / 64 - 1) / (SV_THREADS / 64);
    const dim3 grid((unsigned)gx, (unsigned)((L + 63) / 64));
    if (gx > 0x7fffffff || grid.y > 65535u) return hipErrorInvalidValue;
    if (sum) hipLaunchKernelGGL(k_scanbin_vec<true>, grid, dim3(SV_THREADS), EXP_TABLE_BYTES, s, d, sb, t, L, coeff, offset, M, rec);
    else hipLaunchKernelGGL(k_scanbin_vec<false>, grid, dim3(SV_THREADS), EXP_TABLE_BYTES, s, d, sb, t, L, coeff, offset, M, rec);
    return hipGetLastError();
}

hipError_t launch_scanbin_vec_merge(hipStream_t s, const ScanBins& sb, const ScanBinTable& t, bool sum, int64_t L, const double* rec,
                                    double* M, double* lognum) {
    if (L < 1 || sb.nbins < 1) return hipSuccess;
    const int64_t blocks = (sb.nbins * L + SV_THREADS - 1) / SV_THREADS;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks);
    if (sum) hipLaunchKernelGGL(k_scanbin_vec_merge<true>, grid, dim3(SV_THREADS), EXP_TABLE_BYTES, s, sb, t, L, rec, M, lognum);
    else hipLaunchKernelGGL(k_scanbin_vec_merge<false>, grid, dim3(SV_THREADS), EXP_TABLE_BYTES, s, sb, t, L, rec, M, lognum);
    return hipGetLastError();
}

int64_t scanbin_record_doubles(int nb) { return (int64_t)4 * nb * 4 * 256 + (int64_t)64 * 4 * SCANBIN_NV; }

// nb: scan_nb_for(K), or 0 (no cross block: the per-(member, bin) sums only)
hipError_t launch_scanbin_cross(hipStream_t s, const ScanData& d, const ScanBins& sb, const ScanBinTable& t, int64_t c0, int64_t c1, int nb,
                                const double* u, int64_t ld, int64_t K, const double* f, int64_t L, int64_t p0, const double* coeff,
                                const double* offset, const double* f_bins, double* part) {
    if (c1 <= c0 || p0 >= L) return hipSuccess;
    if (K > 16 * (int64_t)nb && nb > 0) return hipErrorInvalidValue;
    if (c1 - c0 > 0x7fffffff || c1 > t.nchunks) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(c1 - c0));
    const size_t lds = EXP_TABLE_BYTES + ((size_t)nb * 16 * SCAN_PITCH + 32 + (size_t)SCAN_MAX_B * 16) * sizeof(double);
    switch (nb) {
#define MBAR_CASE(NB_)                                                                                                               \
    case NB_:                                                                                                                        \
        hipLaunchKernelGGL((k_scanbin_cross<NB_>), grid, dim3(256), lds, s, d, sb, t, c0, u, ld, K, f, L, p0, coeff, offset, f_bins, part); \
        break;
        MBAR_CASE(0) MBAR_CASE(1) MBAR_CASE(2) MBAR_CASE(4) MBAR_CASE(8)
#undef MBAR_CASE
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_scanbin_cross_merge(hipStream_t s, const ScanBins& sb, const ScanBinTable& t, int64_t c0, int64_t b0, int64_t b1, int nb,
                                      int64_t K, int64_t L, int64_t p0, const double* part, double* cross, double* vec) {
    if (b1 <= b0 || p0 >= L) return hipSuccess;
    const int64_t pl = L - p0 < 256 ? L - p0 : 256;
    const int64_t threads = (b1 - b0) * ((nb > 0 ? pl * K : 0) + pl * SCANBIN_NV);
    const int64_t blocks = (threads + SV_THREADS - 1) / SV_THREADS;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_scanbin_cross_merge, dim3((unsigned)blocks), dim3(SV_THREADS), 0, s, sb, t, c0, b0, b1, nb, K, L, p0, pl, part, cross,
                       vec);
    return hipGetLastError();
}

}  // namespace mbar
