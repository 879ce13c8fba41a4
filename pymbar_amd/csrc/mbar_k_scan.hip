// gfx950 (CDNA4 / MI355X) kernels of the reweighting scans over a linear family of unsampled states (MBAR.compute_scan):
// member l is the state u_l(n) = sum_b coeff[l][b] basis[b][n] + offset[l], B coefficients instead of a row of N doubles.  One of the
// translation units of libmbar_hip.so; the host side (panels, C ABI) is mbar_scan.cpp, the launcher declarations are in
// mbar_internal.h.  DESIGN.md section 17 has the derivation.
//
//   x_ln = -u_l(n) - logden_n,  u_l(n) = fma(coeff[l][B-1], basis[B-1][n], ... fma(coeff[l][0], basis[0][n], offset[l]))
//   t_0n = 1, t_jn = A_jn - s_j (j = 1 .. Q),  J = 1 + Q
//
//   pass A   M_l = max_{n: c_n > 0} x_ln,  S_lj = sum_n c_n exp(x_ln - M_l) t_jn      (B + Q + 2 N-vectors twice, no matrix)
//   pass B   b_ln = exp(f_scan_l + x_ln),  W_nk = exp(f_k - u_kn - logden_n)
//            cross[k][l][j]  = sum_n c_n W_nk b_ln t_jn         fp64 matrix cores: A operand = W tile, B operand = c b t, from registers
//            within[l][i][j] = sum_n c_n b_ln^2 t_in t_jn,  refcol[l][j] = sum_n c_n b_rn b_ln t_jn,  wsum[l] = sum_n c_n b_ln
//
// Pass A: one wave per (SCAN_VCHUNK samples, 64 members), lane = member, the samples walked in ascending n (the per-sample values
// are wave-uniform loads).  Pass B: one workgroup of four waves per (SCAN_CHUNK samples, panel of 64 MB members).  Per tile of 16
// samples the workgroup forms the W tile of all K <= 128 states once, in LDS, in the natural order of the matrix (coalesced); every
// wave then reads it in the MFMA A layout (lane l: state 16 I + (l & 15), sample 4 g + (l >> 4)) against its own MB blocks of 16
// members: lane l generates b of member (l & 15) at sample 4 g + (l >> 4) -- one table exponential -- and J multiplies give the J
// B operands.  The per-member sums are lane-local and folded over the four sample groups at the end, in a fixed order.
//
// Order.  The cut of N into chunks depends on N alone; a member's sums are the same sequence of operations wherever it sits in
// the call (which wave, which block, which lane column); the merge kernels add a member's chunk records in chunk order
// (compensated).  No atomics: two identical calls return identical bits, and member l's outputs do not depend on the others.
// Every fused multiply-add below is written as one (fma, MFMA) and nothing else is contracted: left to the compiler, "wsum += c_n
// b_ln" became one fma at every unrolled site of k_scan_cross<0, J> but only at some of the sites of <NB > 0, J> (a rounded product
// and an addition at the others), so that cross = NULL changed wsum by an ulp wherever a multiplicity c_n makes c_n b_ln inexact.
#include "mbar_device.h"

#pragma clang fp contract(off)

namespace mbar {

// (SV_THREADS, SCAN_PITCH, scan_exp, scan_neumaier and scan_x are in mbar_device.h: the binned scan kernels share them)

// One wave per (chunk of SCAN_VCHUNK samples, 64 members).  SUM = false: rec[chunk][l] = max of x_ln over the chunk's samples with
// c_n > 0; SUM = true: rec[(chunk L + l) J + j] = sum c_n exp(x_ln - M_l) t_jn.
template <bool SUM>
__global__ void __launch_bounds__(SV_THREADS)
k_scan_vec(ScanData d, int64_t L, const double* __restrict__ coeff, const double* __restrict__ offset, const double* __restrict__ M,
           double* __restrict__ rec) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (SUM) {
        exp_table_init(smem);
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t c = (int64_t)blockIdx.x * (SV_THREADS / 64) + wave;
    const int64_t nchunks = (d.N + SCAN_VCHUNK - 1) / SCAN_VCHUNK;
    if (c >= nchunks) return;
    const int64_t l = (int64_t)blockIdx.y * 64 + lane;
    const bool live = l < L;
    const int J = 1 + d.Q;
    double cf[SCAN_MAX_B];
#pragma unroll
    for (int b = 0; b < SCAN_MAX_B; ++b) cf[b] = (live && b < d.B) ? coeff[l * d.B + b] : 0.0;
    const double off = live ? offset[l] : 0.0;
    const double Ml = (SUM && live) ? M[l] : 0.0;
    double acc[1 + SCAN_MAX_Q];
    acc[0] = SUM ? 0.0 : -INFINITY;
#pragma unroll
    for (int j = 1; j <= SCAN_MAX_Q; ++j) acc[j] = 0.0;
    const int64_t n0 = c * SCAN_VCHUNK, n1 = n0 + SCAN_VCHUNK < d.N ? n0 + SCAN_VCHUNK : d.N;
    for (int64_t n = n0; n < n1; ++n) {  // (n is wave-uniform: the per-sample values are scalar loads)
        const double cn = d.cw ? d.cw[n] : 1.0;
        if (!(cn > 0.0)) continue;
        const double x = scan_x(d, cf, off, n);
        if (!SUM) {
            acc[0] = fmax(acc[0], x);
        } else {
            const double e = cn * scan_exp(x - Ml);
            acc[0] += e;
#pragma unroll
            for (int j = 1; j <= SCAN_MAX_Q; ++j)
                if (j < J) acc[j] = fma(e, d.t[(int64_t)(j - 1) * d.ldv + n], acc[j]);
        }
    }
    if (!live) return;
    if (!SUM) {
        rec[c * L + l] = acc[0];
    } else {
#pragma unroll
        for (int j = 0; j <= SCAN_MAX_Q; ++j)
            if (j < J) rec[(c * L + l) * J + j] = acc[j];
    }
}

// One thread per member: its chunk records merged in chunk order.  SUM = false: M[l] = the maximum; SUM = true: lognum[l] = M_l +
// log S_l0 (-inf when no sample has c_n > 0), mean[l][j] = S_lj / S_l0.
template <bool SUM>
__global__ void __launch_bounds__(SV_THREADS)
k_scan_vec_merge(int64_t nchunks, int64_t L, int J, const double* __restrict__ rec, double* __restrict__ M, double* __restrict__ lognum,
                 double* __restrict__ mean) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (SUM) {
        exp_table_init(smem);
        __syncthreads();
    }
    const int64_t l = (int64_t)blockIdx.x * SV_THREADS + threadIdx.x;
    if (l >= L) return;
    if (!SUM) {
        double m = -INFINITY;
        for (int64_t c = 0; c < nchunks; ++c) m = fmax(m, rec[c * L + l]);
        M[l] = m;
        return;
    }
    double s0 = 0.0;
    for (int j = 0; j < J; ++j) {
        double s = 0.0, e = 0.0;
        for (int64_t c = 0; c < nchunks; ++c) scan_neumaier(s, e, rec[(c * L + l) * J + j]);
        s += e;
        if (j == 0) {
            s0 = s;
            lognum[l] = s > 0.0 ? M[l] + log_pos(s) : -INFINITY;
            mean[l * J] = 1.0;
        } else {
            mean[l * J + j] = s / s0;
        }
    }
}

// ---- pass B --------------------------------------------------------------------------------------------------------------------
// Record of one workgroup (chunk c of SCAN_CHUNK samples, panel of 64 MB members), MB = scan_mb(J), NCB = MB J column blocks per wave:
//   cross part  [wave][I < NB][cb < NCB][r < 4][lane]   the MFMA accumulators as they are: element (state 16 I + (lane >> 4) + 4 r,
//                                                       member block mb = cb / J, column lane & 15, observable j = cb % J)
//   vec part    [pm < 64 MB][NV]                        wsum | refcol[J] | within[i <= j], NV = 1 + J + J (J + 1) / 2
// Member pm of the panel sits in block pm / 16 = mb * 4 + wave (the blocks go round the waves, so a short panel keeps all four busy).
template <int NB, int J>
__global__ void __launch_bounds__(256)
k_scan_cross(ScanData d, const double* __restrict__ u, int64_t ld, int64_t K, const double* __restrict__ f, int64_t L, int64_t p0,
             const double* __restrict__ coeff, const double* __restrict__ offset, const double* __restrict__ f_scan, int64_t ref,
             double* __restrict__ part) {
    constexpr int MB = scan_mb(J), NCB = MB * J, NV = scan_nv(J), Q = J - 1;
    constexpr int W_DOUBLES = NB * 16 * SCAN_PITCH;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    exp_table_init(smem);
    double* Wt = reinterpret_cast<double*>(smem + EXP_TABLE_BYTES);  // [16 NB][SCAN_PITCH]
    double* sv = Wt + W_DOUBLES;                                     // cn[16] | lden[16] | br[16] | basis[B][16] | t[Q][16]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 15, q4 = lane >> 4;
    const int64_t c = blockIdx.x;
    const int64_t n0c = c * SCAN_CHUNK, n1c = n0c + SCAN_CHUNK < d.N ? n0c + SCAN_CHUNK : d.N;
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
        fs[mb] = mlive[mb] ? f_scan[l] : 0.0;
    }
    // fill roles: thread tid forms W of state 16 I + (tid >> 4) at sample tid & 15; threads 0 .. 15 also the sample's scalars
    const int fs_s = tid & 15, fs_r = tid >> 4;
    double fk[NB > 0 ? NB : 1];
#pragma unroll
    for (int I = 0; I < NB; ++I) fk[I] = 16 * I + fs_r < K ? f[16 * I + fs_r] : 0.0;
    double cr[SCAN_MAX_B], offr = 0.0, fsr = 0.0;  // the reference member: b_rn is formed exactly as that member's own b
#pragma unroll
    for (int b = 0; b < SCAN_MAX_B; ++b) cr[b] = 0.0;
    if (tid < 16) {
#pragma unroll
        for (int b = 0; b < SCAN_MAX_B; ++b)
            if (b < d.B) cr[b] = coeff[ref * d.B + b];
        offr = offset[ref];
        fsr = f_scan[ref];
    }

    v4d acc[NB > 0 ? NB * NCB : 1];
#pragma unroll
    for (int i = 0; i < (NB > 0 ? NB * NCB : 1); ++i) acc[i] = v4d{0.0, 0.0, 0.0, 0.0};
    double vs[MB][NV];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int v = 0; v < NV; ++v) vs[mb][v] = 0.0;

    __syncthreads();  // the exp table
    for (int64_t n0 = n0c; n0 < n1c; n0 += 16) {
        // ---- fill: W tile and the per-sample values of the tile
        {
            const int64_t n = n0 + fs_s;
            double cn = 0.0, lden = 0.0;
            if (n < n1c) {
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
                double br = 0.0;
                if (slive) {
                    double ur = offr;
#pragma unroll
                    for (int b = 0; b < SCAN_MAX_B; ++b)
                        if (b < d.B) ur = fma(cr[b], d.basis[(int64_t)b * d.ldv + n], ur);
                    br = scan_exp(fsr + (-ur - lden));
                }
                sv[fs_s] = cn;
                sv[16 + fs_s] = lden;
                sv[32 + fs_s] = br;
            }
            if (fs_r < d.B + Q) {
                double v = 0.0;
                if (slive) v = fs_r < d.B ? d.basis[(int64_t)fs_r * d.ldv + n] : d.t[(int64_t)(fs_r - d.B) * d.ldv + n];
                sv[48 + fs_r * 16 + fs_s] = v;
            }
        }
        __syncthreads();
        // ---- products: four groups of four samples
        if (mine > 0) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int s = 4 * g + q4;
                double a[NB > 0 ? NB : 1];
#pragma unroll
                for (int I = 0; I < NB; ++I) a[I] = Wt[(16 * I + col) * SCAN_PITCH + s];
                const double cn = sv[s], lden = sv[16 + s], br = sv[32 + s];
                double bas[SCAN_MAX_B], tj[J];
#pragma unroll
                for (int b = 0; b < SCAN_MAX_B; ++b) bas[b] = b < d.B ? sv[48 + b * 16 + s] : 0.0;
                tj[0] = 1.0;
#pragma unroll
                for (int j = 1; j < J; ++j) tj[j] = sv[48 + (d.B + j - 1) * 16 + s];
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
                        double z[J];
#pragma unroll
                        for (int j = 0; j < J; ++j) z[j] = cb * tj[j];
                        vs[mb][0] += cb;
#pragma unroll
                        for (int j = 0; j < J; ++j) vs[mb][1 + j] = fma(z[j], br, vs[mb][1 + j]);
                        int v = 1 + J;
#pragma unroll
                        for (int i = 0; i < J; ++i) {
                            const double bi = bv * tj[i];
#pragma unroll
                            for (int j = i; j < J; ++j) {
                                vs[mb][v] = fma(bi, z[j], vs[mb][v]);
                                ++v;
                            }
                        }
#pragma unroll
                        for (int I = 0; I < NB; ++I)
#pragma unroll
                            for (int j = 0; j < J; ++j)
                                acc[I * NCB + mb * J + j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[I], z[j], acc[I * NCB + mb * J + j], 0, 0, 0);
                    }
                }
            }
        }
        __syncthreads();
    }
    // ---- the record
    constexpr int64_t CROSS_DOUBLES = (int64_t)4 * NB * NCB * 256;
    double* rec = part + c * (CROSS_DOUBLES + (int64_t)64 * MB * NV);
#pragma unroll
    for (int i = 0; i < NB * NCB; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) rec[(((int64_t)wave * NB * NCB + i) * 4 + r) * 64 + lane] = acc[i][r];
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

// The records of the panel merged in chunk order.  Threads [0, pl J K): cross[k][p0 + pm][j]; threads behind them, [0, pl NV):
// vec[p0 + pm][v].
__global__ void __launch_bounds__(SV_THREADS)
k_scan_cross_merge(int64_t nchunks, int NB, int J, int64_t K, int64_t L, int64_t p0, int64_t pl, const double* __restrict__ part,
                   double* __restrict__ cross, double* __restrict__ vec) {
    const int MB = scan_mb(J), NCB = MB * J, NV = scan_nv(J);
    const int64_t cross_doubles = (int64_t)4 * NB * NCB * 256, stride = cross_doubles + (int64_t)64 * MB * NV;
    const int64_t ncross = NB > 0 ? pl * J * K : 0;
    int64_t x = (int64_t)blockIdx.x * SV_THREADS + threadIdx.x;
    int64_t at;
    double* out;
    if (x < ncross) {
        const int64_t pm = x % pl, j = (x / pl) % J, k = x / (pl * J);
        const int64_t blk = pm / 16, colm = pm % 16, wave = blk % 4, mb = blk / 4;
        const int64_t I = k / 16, row = k % 16, r = row >> 2, lane = (row & 3) * 16 + colm;
        at = (((wave * NB + I) * NCB + mb * J + j) * 4 + r) * 64 + lane;
        out = cross + (k * L + p0 + pm) * J + j;
    } else {
        x -= ncross;
        if (x >= pl * NV) return;
        const int64_t pm = x / NV, v = x % NV;
        at = cross_doubles + pm * NV + v;
        out = vec + (p0 + pm) * NV + v;
    }
    double s = 0.0, e = 0.0;
    for (int64_t c = 0; c < nchunks; ++c) scan_neumaier(s, e, part[c * stride + at]);
    *out = s + e;
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------
hipError_t launch_scan_vec(hipStream_t s, const ScanData& d, bool sum, int64_t L, const double* coeff, const double* offset,
                           const double* M, double* rec) {
    if (L < 1 || d.N < 1) return hipSuccess;
    const int64_t nchunks = (d.N + SCAN_VCHUNK - 1) / SCAN_VCHUNK;
    const dim3 grid((unsigned)((nchunks + SV_THREADS / 64 - 1) / (SV_THREADS / 64)), (unsigned)((L + 63) / 64));
    if (grid.y > 65535u) return hipErrorInvalidValue;
    if (sum) hipLaunchKernelGGL(k_scan_vec<true>, grid, dim3(SV_THREADS), EXP_TABLE_BYTES, s, d, L, coeff, offset, M, rec);
    else hipLaunchKernelGGL(k_scan_vec<false>, grid, dim3(SV_THREADS), EXP_TABLE_BYTES, s, d, L, coeff, offset, M, rec);
    return hipGetLastError();
}

hipError_t launch_scan_vec_merge(hipStream_t s, const ScanData& d, bool sum, int64_t L, const double* rec, double* M, double* lognum,
                                 double* mean) {
    if (L < 1) return hipSuccess;
    const int64_t nchunks = (d.N + SCAN_VCHUNK - 1) / SCAN_VCHUNK;
    const dim3 grid((unsigned)((L + SV_THREADS - 1) / SV_THREADS));
    if (sum) hipLaunchKernelGGL(k_scan_vec_merge<true>, grid, dim3(SV_THREADS), EXP_TABLE_BYTES, s, nchunks, L, 1 + d.Q, rec, M, lognum, mean);
    else hipLaunchKernelGGL(k_scan_vec_merge<false>, grid, dim3(SV_THREADS), EXP_TABLE_BYTES, s, nchunks, L, 1 + d.Q, rec, M, lognum, mean);
    return hipGetLastError();
}

int scan_nb_for(int64_t K) {  // blocks of 16 states the cross kernel is instantiated for
    const int need = (int)((K + 15) / 16);
    return need <= 1 ? 1 : need <= 2 ? 2 : need <= 4 ? 4 : 8;
}

int64_t scan_record_doubles(int nb, int J) {
    const int MB = scan_mb(J);
    return (int64_t)4 * nb * MB * J * 256 + (int64_t)64 * MB * scan_nv(J);
}

template <int NB>
static hipError_t launch_scan_cross_nb(hipStream_t s, const ScanData& d, dim3 grid, size_t lds, const double* u, int64_t ld, int64_t K,
                                       const double* f, int64_t L, int64_t p0, const double* coeff, const double* offset,
                                       const double* f_scan, int64_t ref, double* part) {
    switch (1 + d.Q) {
#define MBAR_CASE(J_)                                                                                                            \
    case J_:                                                                                                                     \
        hipLaunchKernelGGL((k_scan_cross<NB, J_>), grid, dim3(256), lds, s, d, u, ld, K, f, L, p0, coeff, offset, f_scan, ref, part); \
        break;
        MBAR_CASE(1) MBAR_CASE(2) MBAR_CASE(3) MBAR_CASE(4)
#undef MBAR_CASE
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// nb: scan_nb_for(K), or 0 (no cross block: the per-member sums only)
hipError_t launch_scan_cross(hipStream_t s, const ScanData& d, int nb, const double* u, int64_t ld, int64_t K, const double* f, int64_t L,
                             int64_t p0, const double* coeff, const double* offset, const double* f_scan, int64_t ref, double* part) {
    if (d.N < 1 || p0 >= L) return hipSuccess;
    if (K > 16 * (int64_t)nb && nb > 0) return hipErrorInvalidValue;
    const int64_t nchunks = (d.N + SCAN_CHUNK - 1) / SCAN_CHUNK;
    if (nchunks > 0x7fffffff) return hipErrorInvalidValue;
    const dim3 grid((unsigned)nchunks);
    const size_t lds = EXP_TABLE_BYTES + ((size_t)nb * 16 * SCAN_PITCH + 48 + (size_t)(SCAN_MAX_B + SCAN_MAX_Q) * 16) * sizeof(double);
    switch (nb) {
        case 0: return launch_scan_cross_nb<0>(s, d, grid, lds, u, ld, K, f, L, p0, coeff, offset, f_scan, ref, part);
        case 1: return launch_scan_cross_nb<1>(s, d, grid, lds, u, ld, K, f, L, p0, coeff, offset, f_scan, ref, part);
        case 2: return launch_scan_cross_nb<2>(s, d, grid, lds, u, ld, K, f, L, p0, coeff, offset, f_scan, ref, part);
        case 4: return launch_scan_cross_nb<4>(s, d, grid, lds, u, ld, K, f, L, p0, coeff, offset, f_scan, ref, part);
        case 8: return launch_scan_cross_nb<8>(s, d, grid, lds, u, ld, K, f, L, p0, coeff, offset, f_scan, ref, part);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_scan_cross_merge(hipStream_t s, const ScanData& d, int nb, int64_t K, int64_t L, int64_t p0, const double* part,
                                   double* cross, double* vec) {
    if (d.N < 1 || p0 >= L) return hipSuccess;
    const int J = 1 + d.Q;
    const int64_t nchunks = (d.N + SCAN_CHUNK - 1) / SCAN_CHUNK;
    const int64_t pl = L - p0 < 64 * scan_mb(J) ? L - p0 : 64 * scan_mb(J);
    const int64_t threads = (nb > 0 ? pl * J * K : 0) + pl * scan_nv(J);
    hipLaunchKernelGGL(k_scan_cross_merge, dim3((unsigned)((threads + SV_THREADS - 1) / SV_THREADS)), dim3(SV_THREADS), 0, s, nchunks, nb, J,
                       K, L, p0, pl, part, cross, vec);
    return hipGetLastError();
}

}  // namespace mbar
