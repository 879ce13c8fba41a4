// gfx950 (CDNA4 / MI355X) kernels of the reweighting scans over a linear family of unsampled states (MBAR.compute_scan) and of the
// histogram free energy surfaces along such a scan (MBAR.compute_scan_fes): member l is the state u_l(n) = sum_b coeff[l][b]
// basis[b][n] + offset[l], B coefficients instead of a row of N doubles.  One of the translation units of libmbar_hip.so; the host
// side (panels, sort, chunk tables, bin groups, C ABI) is mbar_scan.cpp, the cuts and the launcher declarations are in
// mbar_scan.h.  DESIGN.md sections 17 and 18 have the derivation, the layout and the cost model.
//
//   x_ln = -u_l(n) - logden_n,  u_l(n) = fma(coeff[l][B-1], basis[B-1][n], ... fma(coeff[l][0], basis[0][n], offset[l]))
//   t_0n = 1, t_jn = A_jn - s_j (j = 1 .. Q),  J = 1 + Q
//
//   pass A   M_l = max_{n: c_n > 0} x_ln,  S_lj = sum_n c_n exp(x_ln - M_l) t_jn      (B + Q + 2 N-vectors twice, no matrix)
//   pass B   b_ln = exp(f_scan_l + x_ln),  W_nk = exp(f_k - u_kn - logden_n)
//            cross[k][l][j]  = sum_n c_n W_nk b_ln t_jn         fp64 matrix cores: A operand = W tile, B operand = c b t, from registers
//            within[l][i][j] = sum_n c_n b_ln^2 t_in t_jn,  refcol[l][j] = sum_n c_n b_rn b_ln t_jn,  wsum[l] = sum_n c_n b_ln
//
// Every kernel is written once, for a cut of the samples given as a template argument (ScanWhole, ScanBinned: mbar_scan.h).  The
// whole cut sums over every sample in its own order, in chunks of SCAN_VCHUNK / SCAN_CHUNK samples.  The binned cut gives every
// (member, bin) pair the sums a member gets there, over the bin's samples alone: perm lists the samples bin by bin, ascending n
// inside a bin (a stable counting sort on the host; label -1 dropped), a chunk is a run of sorted positions of ONE bin, cut from
// the start of the bin, and sample n = perm[p] (still wave-uniform loads in pass A; a gather of the W tile and the basis values in
// pass B, where positions past the bin's end carry c = 0).  Its normaliser is f_bins[l][bin] (+inf: an empty bin of that member,
// exact zeros), it takes Q = 0 (J = 1), and it has no reference member: refcol, the b_rn row and its LDS are compiled out, the vec
// record is wsum | diag (diag = within at J = 1).
//
// Pass A: one wave per (chunk, 64 members), lane = member, the positions walked in ascending order (the per-sample values are
// wave-uniform loads).  Pass B: one workgroup of four waves per (chunk, panel of 64 MB members).  Per tile of 16 positions the
// workgroup forms the W tile of all K <= 128 states once, in LDS, in the natural order of the matrix (coalesced on the whole cut);
// every wave then reads it in the MFMA A layout (lane l: state 16 I + (l & 15), position 4 g + (l >> 4)) against its own MB blocks
// of 16 members: lane l generates b of member (l & 15) at position 4 g + (l >> 4) -- one table exponential -- and J multiplies give
// the J B operands.  The per-member sums are lane-local and folded over the four position groups at the end, in a fixed order.
//
// Order.  The cut into chunks depends on N alone, or on the labels alone; a member's sums are the same sequence of operations
// wherever it sits in the call (which wave, which block, which lane column), and a (member, bin)'s whatever the other bins, the
// bin's number or the bin group are; the merge kernels add the chunk records in chunk order (compensated).  No atomics: two
// identical calls return identical bits, and member l's outputs do not depend on the others.  With one bin that holds every sample
// the binned chunks are the whole cut's chunks and the operations are the same code: the outputs are the bits of mbar_scan_lognum
// / mbar_scan_gram_w.  Every fused multiply-add below is written as one (fma, MFMA) and nothing else is contracted: left to the
// compiler, "wsum += c_n b_ln" became one fma at every unrolled site of k_scan_cross<0, J> but only at some of the sites of
// <NB > 0, J> (a rounded product and an addition at the others), so that cross = NULL changed wsum by an ulp wherever a
// multiplicity c_n makes c_n b_ln inexact.
//
// The family.  The two sweeps are also written once for the kind of the members' terms, a second policy next to the cut (Fam =
// ScanLinear, ScanHarmonic: mbar_scan.h): u_l is the chain of family_term (mbar_scan_device.h) -- the function the fill kernels write
// the resident rows with -- and a harmonic term fma(coeff, w(basis - center)^2, u) with its minimum image w replaces the linear fma
// where the wave-uniform mask says so (mbar_ctx_set_scan_terms).  The harmonic policy keeps the centres of
// its at most SCAN_MAX_H harmonic terms per member in registers next to the coefficients, and therefore narrower panels of pass B
// (ScanHarmonic::mb: at the linear family's widths the instantiations of 8 blocks of states spilled); under ScanLinear every trace
// of them is compiled out, the kernels take no family argument, and the sweeps are the operations, in the order, this file had
// before the policy existed.  The merges know neither kind (the cross merge is told the panel width).
//
// The observables.  A third policy says where t_j comes from (Obs = ScanStored, ScanEnergy: mbar_scan.h).  ScanStored reads d.t, the
// same for every member: every instantiation this file had, with the argument blocks and instruction streams it had.  ScanEnergy is
// the member's own reduced potential (MBAR.compute_scan_entropy_and_enthalpy): t_1 = u_l(n) - center_u[l] from
// the u the chain produced for x_ln, t_2 = t_1 t_1, J = 2 or 3, whole cut only; pass B then keeps refblock[i < 2][J] where the
// stored kind keeps refcol[J], because the reference member's t_1 is its own.
// ScanMoments (mbar_scan.h) adds to the stored observables the features the chain itself is made of and accumulates their first and
// second moments (mbar_scan_moments): pass A on the whole cut, in a sweep and a merge of its own below
// (k_scan_moments, k_scan_moments_merge), between the maxima launch and the outputs of the ScanStored pass A, whose bits it keeps.
//
// The members' own Gram block (MBAR.compute_scan_pairs, mbar_scan_pair_gram): pass B once more with the rows
// of the LDS tile being (reference member, i) instead of sampled states, pair[r][l][i][j] = sum_n c_n (b_rn t_in)(b_ln t_jn), in a
// sweep and a merge of its own (k_scan_pair, k_scan_pair_merge) behind the merge of pass B; whole cut, stored observables.
//
// Many observables (MBAR.compute_scan_expectations, mbar_scan_obs_sums): pass B a third time, the rows of the LDS
// tile being observables the context keeps resident (any number of them, in panels of 128), s1[l][q] = sum_n c_n b_ln a_qn and its
// two second-moment companions, in a sweep and a merge of its own (k_scan_obs, k_scan_obs_merge); whole cut.
//
// Kernel-density surfaces (MBAR.compute_scan_kde, mbar_scan_kde_sums): k_scan_obs's first moments with the tile
// COMPUTED, the gaussian kernel values of up to 128 queries against the 16 positions (k_scan_kde, k_scan_kde_merge), and the pairs
// whose terms all underflow once more in log space (k_scan_kde_exact); whole cut.  At the end of the file.
#include "mbar_device.h"
#include "mbar_scan_device.h"

#pragma clang fp contract(off)

namespace mbar {

constexpr int SV_THREADS = 256;
constexpr int SCAN_PITCH = 17;  // doubles per state row of the W tile in LDS (16 samples + 1: the column read spreads over the banks)

__device__ __forceinline__ double scan_exp(double x) { return exp2s_fast(x * LOG2E_S); }

__device__ __forceinline__ void scan_neumaier(double& s, double& e, double v) {
    const double t = s + v;
    e += fabs(s) >= fabs(v) ? (s - t) + v : (v - t) + s;
    s = t;
}

// One wave per (chunk, 64 members).  SUM = false: rec[chunk][l] = max of x_ln over the chunk's samples with c_n > 0; SUM = true:
// rec[(chunk L + l) J + j] = sum c_n exp(x_ln - M[bin][l]) t_jn.
// (Arg: nothing under ScanLinear and ScanStored, whose kernels keep the argument block -- and with it the instruction stream -- they
// had before the family and observable policies existed; the ScanHarmonic and / or the ScanEnergy themselves otherwise.  Under
// ScanEnergy t_1 = u_l(n) - center_u[l] from the u the chain produced for x, t_2 = t_1 t_1; acc[0] is the chain it always was.)
template <bool SUM, class Cut, class Fam, class Obs, class... Arg>
__global__ void __launch_bounds__(SV_THREADS)
k_scan_vec(ScanData d, Cut cut, int64_t L, const double* __restrict__ coeff, const double* __restrict__ offset,
           const double* __restrict__ M, double* __restrict__ rec, Arg... arg) {
    const Fam fam = scan_arg<Fam>(arg...);
    const Obs obs = scan_arg<Obs>(arg...);
    static_assert(!Obs::energy || (SUM && !Cut::binned), "the energy observable: the sums of the whole cut");
    constexpr int MAX_Q = Cut::binned ? 0 : Obs::energy ? 2 : SCAN_MAX_Q;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (SUM) {
        exp_table_init(smem);
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t c = (int64_t)blockIdx.x * (SV_THREADS / 64) + wave;  // the record; the chunk is c0() + c
    if (cut.c0() + c >= cut.c1(d.N, SCAN_VCHUNK)) return;
    int64_t bin, p0, p1;
    cut.range(cut.c0() + c, d.N, SCAN_VCHUNK, bin, p0, p1);
    const int64_t l = (int64_t)blockIdx.y * 64 + lane;
    const bool live = l < L;
    const int J = Cut::binned ? 1 : 1 + d.Q;
    double cf[SCAN_MAX_B];
#pragma unroll
    for (int b = 0; b < SCAN_MAX_B; ++b) cf[b] = (live && b < d.B) ? coeff[l * d.B + b] : 0.0;
    const double off = live ? offset[l] : 0.0;
    double cen[SCAN_MAX_H];
    family_load_centers(fam, live, l, cen);
    const double Ml = (SUM && live) ? M[bin * L + l] : 0.0;
    double cu = 0.0;  // (ScanEnergy: the member's centre)
    if constexpr (Obs::energy) cu = live ? obs.center_u[l] : 0.0;
    double acc[1 + MAX_Q];
    acc[0] = SUM ? 0.0 : -INFINITY;
#pragma unroll
    for (int j = 1; j <= MAX_Q; ++j) acc[j] = 0.0;
    for (int64_t p = p0; p < p1; ++p) {  // (p is wave-uniform: perm and the per-sample values are scalar loads)
        const int64_t n = cut.sample(p);
        const double cn = d.cw ? d.cw[n] : 1.0;
        if (!(cn > 0.0)) continue;
        const double ul = scan_u(d, fam, cf, cen, off, n);
        const double x = scan_x_of(d, ul, n);
        if (!SUM) {
            acc[0] = fmax(acc[0], x);
        } else {
            const double e = cn * scan_exp(x - Ml);
            acc[0] += e;
            if constexpr (Obs::energy) {
                const double t1 = ul - cu;
                acc[1] = fma(e, t1, acc[1]);
                if (J > 2) acc[2] = fma(e, t1 * t1, acc[2]);
            } else {
#pragma unroll
                for (int j = 1; j <= MAX_Q; ++j)
                    if (j < J) acc[j] = fma(e, d.t[(int64_t)(j - 1) * d.ldv + n], acc[j]);
            }
        }
    }
    if (!live) return;
    if (!SUM) {
        rec[c * L + l] = acc[0];
    } else {
#pragma unroll
        for (int j = 0; j <= MAX_Q; ++j)
            if (j < J) rec[(c * L + l) * J + j] = acc[j];
    }
}

// One thread per (bin, member): its chunk records merged in chunk order.  SUM = false: M[bin][l] = the maximum; SUM = true:
// lognum[l][bin] = M + log S_0 (-inf when no sample of the bin has c_n > 0) and, on the whole cut, mean[l][j] = S_j / S_0.
template <bool SUM, class Cut>
__global__ void __launch_bounds__(SV_THREADS)
k_scan_vec_merge(ScanData d, Cut cut, int64_t L, const double* __restrict__ rec, double* __restrict__ M, double* __restrict__ lognum,
                 double* __restrict__ mean) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    if (SUM) {
        exp_table_init(smem);
        __syncthreads();
    }
    const int64_t x = (int64_t)blockIdx.x * SV_THREADS + threadIdx.x;
    if (x >= (cut.b1() - cut.b0()) * L) return;
    const int64_t xb = Cut::binned ? x / L : 0;  // (the whole cut is one bin: no division)
    const int64_t l = x - xb * L, bin = cut.b0() + xb;
    const int J = Cut::binned ? 1 : 1 + d.Q;
    int64_t c0, c1;
    cut.bin_chunks(bin, d.N, SCAN_VCHUNK, c0, c1);
    // (the records are walked by a pointer: with the index written out, the compiler multiplied it out again at every chunk)
    if (!SUM) {
        double m = -INFINITY;
        const double* r = rec + (c0 - cut.c0()) * L + l;
        for (int64_t c = c0; c < c1; ++c, r += L) m = fmax(m, *r);
        M[bin * L + l] = m;
        return;
    }
    double s0 = 0.0;
    for (int j = 0; j < J; ++j) {
        double s = 0.0, e = 0.0;
        const double* r = rec + ((c0 - cut.c0()) * L + l) * J + j;
        for (int64_t c = c0; c < c1; ++c, r += L * J) scan_neumaier(s, e, *r);
        s += e;
        if (j == 0) {
            s0 = s;
            lognum[l * cut.nbins() + bin] = s > 0.0 ? M[bin * L + l] + log_pos(s) : -INFINITY;
            if constexpr (!Cut::binned) mean[l * J] = 1.0;
        } else {
            mean[l * J + j] = s / s0;
        }
    }
}

// ---- the moments of the features (mbar_scan_moments) -------------------------------------------------------
// One wave per (chunk, 64 members), lane = member, as k_scan_vec<true>; e, x_ln and u_l come from the one evaluation of the chain,
// which also hands out what every term was made of.  HB, BB: the bucket of ScanMoments (mbar_scan.h), FB = HB + BB slots, B <= BB terms
// of which at most HB are harmonic.  S0 and S_q are the operations of k_scan_vec<true, ScanWhole, Fam, ScanStored>.  The record is
// rec[chunk][r][L]: lane-contiguous stores.
template <int HB, int BB, class Fam, class... Arg>
__global__ void __launch_bounds__(SV_THREADS)
k_scan_moments(ScanData d, int64_t L, const double* __restrict__ coeff, const double* __restrict__ offset, const double* __restrict__ M,
               const double* __restrict__ cphi, double* __restrict__ rec, Arg... arg) {
    static_assert(Fam::harmonic == (HB > 0) && HB <= SCAN_MAX_H && BB <= SCAN_MAX_B, "the bucket and the family");
    constexpr int FB = HB + BB, NT = FB * (FB + 1) / 2;
    const Fam fam = scan_arg<Fam>(arg...);
    const ScanWhole cut{};
    extern __shared__ __attribute__((aligned(16))) char smem[];
    exp_table_init(smem);
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t c = (int64_t)blockIdx.x * (SV_THREADS / 64) + wave;
    if (c >= cut.c1(d.N, SCAN_VCHUNK)) return;
    int64_t bin, p0, p1;
    cut.range(c, d.N, SCAN_VCHUNK, bin, p0, p1);
    const int64_t l = (int64_t)blockIdx.y * 64 + lane;
    const bool live = l < L;
    const int Q = d.Q;
    double cf[BB];
#pragma unroll
    for (int b = 0; b < BB; ++b) cf[b] = (live && b < d.B) ? coeff[l * d.B + b] : 0.0;
    const double off = live ? offset[l] : 0.0;
    double cen[SCAN_MAX_H];
    family_load_centers(fam, live, l, cen);
    const double Ml = live ? M[l] : 0.0;
    double cp[FB];
#pragma unroll
    for (int i = 0; i < FB; ++i) cp[i] = live ? cphi[l * FB + i] : 0.0;
    double s0 = 0.0, sq[SCAN_MAX_Q], sa[FB], sb[NT], sc[SCAN_MAX_Q][FB];
#pragma unroll
    for (int q = 0; q < SCAN_MAX_Q; ++q) {
        sq[q] = 0.0;
#pragma unroll
        for (int i = 0; i < FB; ++i) sc[q][i] = 0.0;
    }
#pragma unroll
    for (int i = 0; i < FB; ++i) sa[i] = 0.0;
#pragma unroll
    for (int k = 0; k < NT; ++k) sb[k] = 0.0;
    for (int64_t n = p0; n < p1; ++n) {  // (n is wave-uniform: the per-sample values are scalar loads)
        const double cn = d.cw ? d.cw[n] : 1.0;
        if (!(cn > 0.0)) continue;
        double dl[BB];
        const double ul = scan_u(d, fam, cf, cen, off, n, dl);
        const double x = scan_x_of(d, ul, n);
        const double e = cn * scan_exp(x - Ml);
        s0 += e;
        // the features by slot, about the member's centres
        double dv[FB];
        if constexpr (HB > 0) {
            double sqr[HB];
#pragma unroll
            for (int h = 0; h < HB; ++h) sqr[h] = 0.0;
#pragma unroll
            for (int b = 0; b < BB; ++b)
                if ((fam.terms.mask >> b) & 1u) {  // (wave-uniform, and so is the slot)
                    const int slot = __popc(fam.terms.mask & ((1u << b) - 1u));
                    const double q2 = dl[b] * dl[b];
#pragma unroll
                    for (int h = 0; h < HB; ++h) sqr[h] = slot == h ? q2 : sqr[h];
                }
#pragma unroll
            for (int h = 0; h < HB; ++h) dv[h] = sqr[h] - cp[h];
        }
#pragma unroll
        for (int b = 0; b < BB; ++b) dv[HB + b] = dl[b] - cp[HB + b];
#pragma unroll
        for (int q = 0; q < SCAN_MAX_Q; ++q)
            if (q < Q) {
                const double t = d.t[(int64_t)q * d.ldv + n];
                sq[q] = fma(e, t, sq[q]);
                const double et = e * t;
#pragma unroll
                for (int i = 0; i < FB; ++i) sc[q][i] = fma(et, dv[i], sc[q][i]);
            }
        int k = 0;
#pragma unroll
        for (int i = 0; i < FB; ++i) {
            sa[i] = fma(e, dv[i], sa[i]);
            const double w = e * dv[i];
#pragma unroll
            for (int j = i; j < FB; ++j) {
                sb[k] = fma(w, dv[j], sb[k]);
                ++k;
            }
        }
    }
    if (!live) return;
    const int R = 1 + Q + FB + NT + Q * FB;
    double* r = rec + (c * R) * L + l;
    *r = s0;
    r += L;
#pragma unroll
    for (int q = 0; q < SCAN_MAX_Q; ++q)
        if (q < Q) {
            *r = sq[q];
            r += L;
        }
#pragma unroll
    for (int i = 0; i < FB; ++i, r += L) *r = sa[i];
#pragma unroll
    for (int k = 0; k < NT; ++k, r += L) *r = sb[k];
#pragma unroll
    for (int q = 0; q < SCAN_MAX_Q; ++q)
        if (q < Q) {
#pragma unroll
            for (int i = 0; i < FB; ++i, r += L) *r = sc[q][i];
        }
}

// One thread per (sum r, member l): its chunk records merged in chunk order, then divided by the member's S0 (every thread merges
// that too).  lognum and out[l][0 .. Q] are the operations of k_scan_vec_merge<true, ScanWhole>.
__global__ void __launch_bounds__(SV_THREADS)
k_scan_moments_merge(ScanData d, int64_t L, int R, const double* __restrict__ rec, const double* __restrict__ M, double* __restrict__ lognum,
                     double* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    exp_table_init(smem);
    __syncthreads();
    const int64_t x = (int64_t)blockIdx.x * SV_THREADS + threadIdx.x;
    if (x >= L * R) return;
    const int64_t r = x / L, l = x - r * L;
    const int64_t nchunks = (d.N + SCAN_VCHUNK - 1) / SCAN_VCHUNK, stride = (int64_t)R * L;
    double s0 = 0.0, e0 = 0.0;
    const double* p = rec + l;
    for (int64_t c = 0; c < nchunks; ++c, p += stride) scan_neumaier(s0, e0, *p);
    s0 += e0;
    if (r == 0) {
        lognum[l] = s0 > 0.0 ? M[l] + log_pos(s0) : -INFINITY;
        out[l * R] = 1.0;
        return;
    }
    double s = 0.0, e = 0.0;
    p = rec + r * L + l;
    for (int64_t c = 0; c < nchunks; ++c, p += stride) scan_neumaier(s, e, *p);
    s += e;
    out[l * R + r] = s / s0;
}

// ---- pass B --------------------------------------------------------------------------------------------------------------------
// Record of one workgroup (one chunk of SCAN_CHUNK positions, panel of 64 MB members), MB = Fam::mb(J), NCB = MB J column blocks
// per wave:
//   cross part  [wave][I < NB][cb < NCB][r < 4][lane]   the MFMA accumulators as they are: element (state 16 I + (lane >> 4) + 4 r,
//                                                       member block mb = cb / J, column lane & 15, observable j = cb % J)
//   vec part    [pm < 64 MB][NV]                        whole cut: wsum | refcol[J] | within[i <= j], NV = scan_nv(J)
//                                                       binned cut: wsum | diag, NV = SCANBIN_NV
// Member pm of the panel sits in block pm / 16 = mb * 4 + wave (the blocks go round the waves, so a short panel keeps all four busy).
// Obs = ScanEnergy: t_j is the member's own (t_1 = u_l(n) - center_u[l] from the chain's u, t_2 = t_1 t_1: per member block where the
// stored kind has it per sample), no t rows in sv, and the fill stage stores t_r1 of the reference member next to b_rn, for the second
// row of refblock (MB = Obs::mb<Fam>(J), NV = Obs::nv(J)).
template <int NB, int J, class Cut, class Fam, class Obs, class... Arg>
__global__ void __launch_bounds__(256)
k_scan_cross(ScanData d, Cut cut, const double* __restrict__ u, int64_t ld, int64_t K, const double* __restrict__ f, int64_t L, int64_t p0,
             const double* __restrict__ coeff, const double* __restrict__ offset, const double* __restrict__ fnorm,
             double* __restrict__ part, Arg... arg) {
    const Fam fam = scan_arg<Fam>(arg...);
    const Obs obs = scan_arg<Obs>(arg...);
    constexpr bool REF = !Cut::binned;  // the reference member
    constexpr bool ENERGY = Obs::energy;
    static_assert(REF || J == 1, "the binned cut takes no observables");
    static_assert(!ENERGY || (REF && (J == 2 || J == 3)), "the energy observable: the whole cut, J = 2 or 3");
    constexpr int MB = Obs::template mb<Fam>(J), NCB = MB * J, NV = REF ? Obs::nv(J) : SCANBIN_NV;
    constexpr int Q = ENERGY ? 0 : J - 1;               // t rows in sv
    constexpr int VW = REF ? 1 + Obs::ref_rows * J : 1;  // where within starts in the vec record
    constexpr int SVB = REF ? (ENERGY ? 64 : 48) : 32;   // where the basis rows start in sv
    constexpr int W_DOUBLES = NB * 16 * SCAN_PITCH;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    exp_table_init(smem);
    double* Wt = reinterpret_cast<double*>(smem + EXP_TABLE_BYTES);  // [16 NB][SCAN_PITCH]
    double* sv = Wt + W_DOUBLES;  // cn[16] | lden[16] | (REF: br[16]) | (ENERGY: tr1[16]) | basis[B][16] | t[Q][16]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 15, q4 = lane >> 4;
    int64_t bin, q0c, q1c;
    cut.range(cut.c0() + blockIdx.x, d.N, SCAN_CHUNK, bin, q0c, q1c);
    // blocks of 16 members this wave owns, and how many of them hold a member at all
    const int64_t pl = L - p0 < 64 * MB ? L - p0 : 64 * MB;  // members of the panel
    const int nblk = (int)((pl + 15) / 16);
    int mine = 0;
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) mine += (mb * 4 + wave) < nblk;
    mine = __builtin_amdgcn_readfirstlane(mine);

    double cf[MB][SCAN_MAX_B], off[MB], fs[MB];
    double cen[Fam::harmonic ? MB : 1][SCAN_MAX_H];  // (the harmonic family alone keeps its members' centres)
    double cu[ENERGY ? MB : 1];  // (the energy observable alone keeps its members' centres)
    bool mlive[MB];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
        const int64_t pm = (int64_t)(mb * 4 + wave) * 16 + col;
        mlive[mb] = pm < pl;
        const int64_t l = p0 + pm;
        if constexpr (ENERGY) cu[mb] = mlive[mb] ? obs.center_u[l] : 0.0;
#pragma unroll
        for (int b = 0; b < SCAN_MAX_B; ++b) cf[mb][b] = (mlive[mb] && b < d.B) ? coeff[l * d.B + b] : 0.0;
        off[mb] = mlive[mb] ? offset[l] : 0.0;
        if constexpr (Fam::harmonic) family_load_centers(fam, mlive[mb], l, cen[mb]);
        fs[mb] = mlive[mb] ? fnorm[l * cut.nbins() + bin] : 0.0;
        if constexpr (Cut::binned) {
            if (fs[mb] == INFINITY) {  // an empty bin of this member: exact zeros
                mlive[mb] = false;
                fs[mb] = 0.0;
            }
        }
    }
    // fill roles: thread tid forms W of state 16 I + (tid >> 4) at tile position tid & 15; threads 0 .. 15 also the sample's scalars
    const int fs_s = tid & 15, fs_r = tid >> 4;
    double fk[NB > 0 ? NB : 1];
#pragma unroll
    for (int I = 0; I < NB; ++I) fk[I] = 16 * I + fs_r < K ? f[16 * I + fs_r] : 0.0;
    double cr[REF ? SCAN_MAX_B : 1], offr = 0.0, fsr = 0.0;  // the reference member: b_rn is formed exactly as that member's own b
    if constexpr (REF) {
#pragma unroll
        for (int b = 0; b < SCAN_MAX_B; ++b) cr[b] = 0.0;
        if (tid < 16) {
#pragma unroll
            for (int b = 0; b < SCAN_MAX_B; ++b)
                if (b < d.B) cr[b] = coeff[cut.ref * d.B + b];
            offr = offset[cut.ref];
            fsr = fnorm[cut.ref];
        }
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
    for (int64_t q0 = q0c; q0 < q1c; q0 += 16) {
        // ---- fill: W tile and the per-sample values of the tile
        {
            const int64_t q = q0 + fs_s;
            int64_t n = 0;
            double cn = 0.0, lden = 0.0;
            if (q < q1c) {
                n = cut.sample(q);
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
                if constexpr (REF) {
                    double br = 0.0;
                    if (slive) {
                        double ur = offr, cenr[SCAN_MAX_H];  // (its centres are read per tile: sixteen lanes, no registers held)
                        family_load_centers(fam, true, cut.ref, cenr);
#pragma unroll
                        for (int b = 0; b < SCAN_MAX_B; ++b)
                            if (b < d.B) ur = family_term(fam, b, ur, cr[b], d.basis[(int64_t)b * d.ldv + n], family_center(fam, b, cenr));
                        br = scan_exp(fsr + (-ur - lden));
                        // (ScanEnergy: t_r1 as that member's own t_1; its centre is read per tile like the family's)
                        if constexpr (ENERGY) sv[48 + fs_s] = ur - obs.center_u[cut.ref];
                    }
                    sv[32 + fs_s] = br;
                    if constexpr (ENERGY)
                        if (!slive) sv[48 + fs_s] = 0.0;
                }
            }
            if (fs_r < d.B + Q) {
                double v = 0.0;
                if (slive) v = (Q == 0 || fs_r < d.B) ? d.basis[(int64_t)fs_r * d.ldv + n] : d.t[(int64_t)(fs_r - d.B) * d.ldv + n];
                sv[SVB + fs_r * 16 + fs_s] = v;
            }
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
                double br = 0.0;
                if constexpr (REF) br = sv[32 + s];
                double bas[SCAN_MAX_B], tj[J];
#pragma unroll
                for (int b = 0; b < SCAN_MAX_B; ++b) bas[b] = b < d.B ? sv[SVB + b * 16 + s] : 0.0;
                tj[0] = 1.0;
#pragma unroll
                for (int j = 1; j < J; ++j) tj[j] = ENERGY ? 0.0 : sv[SVB + (d.B + j - 1) * 16 + s];
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) {
                    if (mb < mine) {  // (wave-uniform)
                        double uu = off[mb];
#pragma unroll
                        for (int b = 0; b < SCAN_MAX_B; ++b)
                            if (b < d.B) uu = family_term(fam, b, uu, cf[mb][b], bas[b], family_center(fam, b, cen[Fam::harmonic ? mb : 0]));
                        double bv = scan_exp(fs[mb] + (-uu - lden));
                        if (!(cn > 0.0) || !mlive[mb]) bv = 0.0;
                        const double cb = cn * bv;
                        if constexpr (ENERGY) {  // (tj is this member block's own from here on)
                            tj[1] = uu - cu[mb];
                            if constexpr (J > 2) tj[2] = tj[1] * tj[1];
                        }
                        double z[J];
#pragma unroll
                        for (int j = 0; j < J; ++j) z[j] = cb * tj[j];
                        vs[mb][0] += cb;
                        if constexpr (REF) {
#pragma unroll
                            for (int j = 0; j < J; ++j) vs[mb][1 + j] = fma(z[j], br, vs[mb][1 + j]);
                        }
                        if constexpr (ENERGY) {
                            const double brt = br * sv[48 + s];  // (b_rn t_r1: the same product in every member block)
#pragma unroll
                            for (int j = 0; j < J; ++j) vs[mb][1 + J + j] = fma(z[j], brt, vs[mb][1 + J + j]);
                        }
                        int v = VW;
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
    double* rec = part + (int64_t)blockIdx.x * (CROSS_DOUBLES + (int64_t)64 * MB * NV);
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

// The records of the panel and of the launch's bins merged per bin in chunk order.  Threads [0, nbg pl J K):
// cross[k][p0 + pm][bin][j]; threads behind them, [0, nbg pl NV): vec[p0 + pm][bin][v].
template <class Cut, class Obs>
__global__ void __launch_bounds__(SV_THREADS)
k_scan_cross_merge(ScanData d, Cut cut, int NB, int64_t K, int64_t L, int64_t p0, int64_t pl, const double* __restrict__ part,
                   double* __restrict__ cross, double* __restrict__ vec, int MB) {
    const int J = Cut::binned ? 1 : 1 + d.Q;
    const int NCB = MB * J, NV = Cut::binned ? SCANBIN_NV : Obs::nv(J);
    const int64_t cross_doubles = (int64_t)4 * NB * NCB * 256, stride = cross_doubles + (int64_t)64 * MB * NV;
    const int64_t nbg = cut.b1() - cut.b0(), ncross = NB > 0 ? nbg * pl * J * K : 0;
    int64_t x = (int64_t)blockIdx.x * SV_THREADS + threadIdx.x;
    int64_t at, bin;
    double* out;
    if (x < ncross) {
        const int64_t pm = x % pl, j = (x / pl) % J, k = (x / (pl * J)) % K;
        bin = cut.b0() + x / (pl * J * K);
        const int64_t blk = pm / 16, colm = pm % 16, wave = blk % 4, mb = blk / 4;
        const int64_t I = k / 16, row = k % 16, r = row >> 2, lane = (row & 3) * 16 + colm;
        at = (((wave * NB + I) * NCB + mb * J + j) * 4 + r) * 64 + lane;
        out = cross + ((k * L + p0 + pm) * cut.nbins() + bin) * J + j;
    } else {
        x -= ncross;
        if (x >= nbg * pl * NV) return;
        const int64_t pm = x % pl, v = (x / pl) % NV;
        bin = cut.b0() + x / (pl * NV);
        at = cross_doubles + pm * NV + v;
        out = vec + ((p0 + pm) * cut.nbins() + bin) * NV + v;
    }
    int64_t c0, c1;
    cut.bin_chunks(bin, d.N, SCAN_CHUNK, c0, c1);
    double s = 0.0, e = 0.0;
    const double* r = part + (c0 - cut.c0()) * stride + at;
    for (int64_t c = c0; c < c1; ++c, r += stride) scan_neumaier(s, e, *r);
    *out = s + e;
}

// ---- the member-member Gram block (mbar_scan_pair_gram) -----------------------------------------------------
//   pair[r][l][i][j] = sum_n c_n (b_{rows[r]} n t_in)(b_ln t_jn)
// k_scan_cross with the rows of the LDS tile being (reference member, i) instead of sampled states: row m J + i of the tile is b t_i
// of the panel's m-th reference member, RMAX = 16 NB / J of them (at J = 3 the last 16 NB - 3 RMAX rows stay zero).  The parameters
// of the panel's reference members (coeff | offset | f_scan | centres, PAIR_RP doubles each) are staged in LDS once; in the fill
// stage thread tid forms b of the members (tid >> 4) + 16 mm at tile position tid & 15 by exactly the operations of the product
// stage -- the chain of family_term over the same basis values, then scan_exp(fs + (-u - lden)) -- so that, without sample weights,
// element (r, l, i, j) and element (l, r, j, i) are the same products in the other order of their factors, accumulated over the
// same positions in the same order: the same bits.  An element's operations do not depend on the row it has in the tile, on NB or
// on its column.  The record is the cross part of k_scan_cross's: [wave][I < NB][cb < NCB][r < 4][lane].
constexpr int PAIR_RP = SCAN_MAX_B + 2 + SCAN_MAX_H;

template <int NB, int J, class Fam, class... Arg>
__global__ void __launch_bounds__(256)
k_scan_pair(ScanData d, int64_t L, int64_t p0, const int64_t* __restrict__ rows, int rm, const double* __restrict__ coeff,
            const double* __restrict__ offset, const double* __restrict__ fnorm, double* __restrict__ part, Arg... arg) {
    const Fam fam = scan_arg<Fam>(arg...);
    const ScanWhole cut{};
    constexpr int MB = Fam::mb(J), NCB = MB * J, Q = J - 1;
    constexpr int RMAX = scan_pair_rows(NB, J), RPT = (RMAX + 15) / 16;  // reference members of a panel, and of one fill thread
    constexpr int SVB = 32;                                              // where the basis rows start in sv
    constexpr int W_DOUBLES = NB * 16 * SCAN_PITCH;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    exp_table_init(smem);
    double* Wt = reinterpret_cast<double*>(smem + EXP_TABLE_BYTES);  // [16 NB][SCAN_PITCH]
    double* sv = Wt + W_DOUBLES;                                     // cn[16] | lden[16] | basis[B][16] | t[Q][16]
    double* rp = sv + SVB + (SCAN_MAX_B + SCAN_MAX_Q) * 16;          // [RMAX][PAIR_RP]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 15, q4 = lane >> 4;
    int64_t bin, q0c, q1c;
    cut.range(blockIdx.x, d.N, SCAN_CHUNK, bin, q0c, q1c);
    const int64_t pl = L - p0 < 64 * MB ? L - p0 : 64 * MB;  // members of the panel
    const int nblk = (int)((pl + 15) / 16);
    int mine = 0;
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) mine += (mb * 4 + wave) < nblk;
    mine = __builtin_amdgcn_readfirstlane(mine);

    double cf[MB][SCAN_MAX_B], off[MB], fs[MB];
    double cen[Fam::harmonic ? MB : 1][SCAN_MAX_H];
    bool mlive[MB];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
        const int64_t pm = (int64_t)(mb * 4 + wave) * 16 + col;
        mlive[mb] = pm < pl;
        const int64_t l = p0 + pm;
#pragma unroll
        for (int b = 0; b < SCAN_MAX_B; ++b) cf[mb][b] = (mlive[mb] && b < d.B) ? coeff[l * d.B + b] : 0.0;
        off[mb] = mlive[mb] ? offset[l] : 0.0;
        if constexpr (Fam::harmonic) family_load_centers(fam, mlive[mb], l, cen[mb]);
        fs[mb] = mlive[mb] ? fnorm[l] : 0.0;
    }
    // the parameters of the panel's reference members, and a tile of zeros (rows nobody owns stay zero)
    for (int x = tid; x < RMAX * PAIR_RP; x += 256) {
        const int m = x / PAIR_RP, k = x - m * PAIR_RP;
        double v = 0.0;
        if (m < rm) {
            const int64_t l = rows[m];
            if (k < SCAN_MAX_B) v = k < d.B ? coeff[l * d.B + k] : 0.0;
            else if (k == SCAN_MAX_B) v = offset[l];
            else if (k == SCAN_MAX_B + 1) v = fnorm[l];
            else if constexpr (Fam::harmonic) v = fam.center[l * SCAN_MAX_H + (k - SCAN_MAX_B - 2)];
        }
        rp[x] = v;
    }
    for (int x = tid; x < W_DOUBLES; x += 256) Wt[x] = 0.0;
    const int fs_s = tid & 15, fs_r = tid >> 4;

    v4d acc[NB * NCB];
#pragma unroll
    for (int i = 0; i < NB * NCB; ++i) acc[i] = v4d{0.0, 0.0, 0.0, 0.0};

    __syncthreads();  // the exp table, the parameters
    for (int64_t q0 = q0c; q0 < q1c; q0 += 16) {
        // ---- fill: the row tile and the per-sample values of the tile
        {
            const int64_t q = q0 + fs_s;
            int64_t n = 0;
            double cn = 0.0, lden = 0.0;
            if (q < q1c) {
                n = q;
                cn = d.cw ? d.cw[n] : 1.0;
                if (cn > 0.0) lden = d.logden[n];
                else cn = 0.0;
            }
            const bool slive = cn > 0.0;
            double bas[SCAN_MAX_B], tq[J];
#pragma unroll
            for (int b = 0; b < SCAN_MAX_B; ++b) bas[b] = (slive && b < d.B) ? d.basis[(int64_t)b * d.ldv + n] : 0.0;
            tq[0] = 1.0;
#pragma unroll
            for (int j = 1; j < J; ++j) tq[j] = slive ? d.t[(int64_t)(j - 1) * d.ldv + n] : 0.0;
#pragma unroll
            for (int mm = 0; mm < RPT; ++mm) {
                const int m = fs_r + 16 * mm;
                if (m < RMAX) {
                    double br = 0.0;
                    if (slive && m < rm) {
                        const double* pr = rp + m * PAIR_RP;
                        double ur = pr[SCAN_MAX_B], cenr[SCAN_MAX_H];
#pragma unroll
                        for (int h = 0; h < SCAN_MAX_H; ++h) cenr[h] = Fam::harmonic ? pr[SCAN_MAX_B + 2 + h] : 0.0;
#pragma unroll
                        for (int b = 0; b < SCAN_MAX_B; ++b)
                            if (b < d.B) ur = family_term(fam, b, ur, pr[b], bas[b], family_center(fam, b, cenr));
                        br = scan_exp(pr[SCAN_MAX_B + 1] + (-ur - lden));
                    }
#pragma unroll
                    for (int i = 0; i < J; ++i) Wt[(m * J + i) * SCAN_PITCH + fs_s] = br * tq[i];
                }
            }
            if (tid < 16) {
                sv[fs_s] = cn;
                sv[16 + fs_s] = lden;
            }
            if (fs_r < d.B + Q) {
                double v = 0.0;
                if (slive) v = (Q == 0 || fs_r < d.B) ? d.basis[(int64_t)fs_r * d.ldv + n] : d.t[(int64_t)(fs_r - d.B) * d.ldv + n];
                sv[SVB + fs_r * 16 + fs_s] = v;
            }
        }
        __syncthreads();
        // ---- products: four groups of four positions
        if (mine > 0) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int s = 4 * g + q4;
                double a[NB];
#pragma unroll
                for (int I = 0; I < NB; ++I) a[I] = Wt[(16 * I + col) * SCAN_PITCH + s];
                const double cn = sv[s], lden = sv[16 + s];
                double bas[SCAN_MAX_B], tj[J];
#pragma unroll
                for (int b = 0; b < SCAN_MAX_B; ++b) bas[b] = b < d.B ? sv[SVB + b * 16 + s] : 0.0;
                tj[0] = 1.0;
#pragma unroll
                for (int j = 1; j < J; ++j) tj[j] = sv[SVB + (d.B + j - 1) * 16 + s];
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) {
                    if (mb < mine) {  // (wave-uniform)
                        double uu = off[mb];
#pragma unroll
                        for (int b = 0; b < SCAN_MAX_B; ++b)
                            if (b < d.B) uu = family_term(fam, b, uu, cf[mb][b], bas[b], family_center(fam, b, cen[Fam::harmonic ? mb : 0]));
                        double bv = scan_exp(fs[mb] + (-uu - lden));
                        if (!(cn > 0.0) || !mlive[mb]) bv = 0.0;
                        const double cb = cn * bv;
                        double z[J];
#pragma unroll
                        for (int j = 0; j < J; ++j) z[j] = cb * tj[j];
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
    double* rec = part + (int64_t)blockIdx.x * ((int64_t)4 * NB * NCB * 256);
#pragma unroll
    for (int i = 0; i < NB * NCB; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) rec[(((int64_t)wave * NB * NCB + i) * 4 + r) * 64 + lane] = acc[i][r];
}

// One thread per (row rho = m J + i of the row panel, member pm of the member panel, j): its chunk records added in chunk order,
// compensated, into pair[m][p0 + pm][i][j] (pair: at the row panel's first reference member, rows of L J J doubles).
__global__ void __launch_bounds__(SV_THREADS)
k_scan_pair_merge(int64_t nchunks, int NB, int J, int MB, int rm, int64_t L, int64_t p0, int64_t pl, const double* __restrict__ part,
                  double* __restrict__ pair) {
    const int NCB = MB * J;
    const int64_t stride = (int64_t)4 * NB * NCB * 256;
    const int64_t x = (int64_t)blockIdx.x * SV_THREADS + threadIdx.x;
    if (x >= (int64_t)rm * J * pl * J) return;
    const int64_t pm = x % pl, j = (x / pl) % J, rho = x / (pl * J);
    const int64_t m = rho / J, i = rho - m * J;
    const int64_t blk = pm / 16, colm = pm % 16, wave = blk % 4, mb = blk / 4;
    const int64_t I = rho / 16, row = rho % 16, r = row >> 2, lane = (row & 3) * 16 + colm;
    const int64_t at = (((wave * NB + I) * NCB + mb * J + j) * 4 + r) * 64 + lane;
    double s = 0.0, e = 0.0;
    const double* p = part + at;
    for (int64_t c = 0; c < nchunks; ++c, p += stride) scan_neumaier(s, e, *p);
    pair[((m * L + p0 + pm) * J + i) * J + j] = s + e;
}

// ---- many observables along a scan (mbar_scan_obs_sums) ------------------------------------------------------
//   MODE 0   s1[l][q] = sum_n c_n b_ln a_qn                                              tile a,   z = (c b)
//   MODE 1   s1 and t1[l][q] = sum_n c_n b_ln^2 a_qn                                     tile a,   z = (c b, c b b)
//   MODE 2   t2[l][q] = sum_n c_n b_ln^2 a_qn^2                                          tile a a, z = (c b b)
// k_scan_cross with the rows of the LDS tile being stored observables instead of sampled states: one workgroup owns one chunk, one
// panel of 64 MB members (MB = Fam::mb(J), J = 2 in mode 1 and 1 otherwise) and one panel of nq <= 16 NB observables, the rows of a
// (pitch d.ldv).  The fill stage loads the tile as it lies in memory (thread tid: row 16 I + (tid >> 4), position tid & 15) with exact
// zeros where c_n <= 0, past nq and past the chunk; the product stage is k_scan_cross's, b formed by the same operations.  wsum =
// sum c b and w2sum = sum c b b are lane-local as there (one addition, one fma per position) and written by every workgroup; the host
// merges those of the first observable panel.  An element's operations depend neither on the row it has in the tile nor on NB, the
// member's column or MB; s1 is the same instruction sequence in modes 0 and 1.  The record is the cross part of k_scan_cross's,
// [wave][I < NB][cb < NCB][r < 4][lane], then [pm < 64 MB][wsum | w2sum].
constexpr int SCANOBS_NV = 2;

template <int NB, int MODE, class Fam, class... Arg>
__global__ void __launch_bounds__(256)
k_scan_obs(ScanData d, const double* __restrict__ a, int nq, int64_t L, int64_t p0, const double* __restrict__ coeff,
           const double* __restrict__ offset, const double* __restrict__ fnorm, double* __restrict__ part, Arg... arg) {
    const Fam fam = scan_arg<Fam>(arg...);
    const ScanWhole cut{};
    constexpr int J = MODE == 1 ? 2 : 1, MB = Fam::mb(J), NCB = MB * J, NV = SCANOBS_NV;
    static_assert(NB * NCB <= 32, "at most 32 accumulator blocks per wave");
    constexpr int SVB = 32;  // where the basis rows start in sv
    constexpr int W_DOUBLES = NB * 16 * SCAN_PITCH;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    exp_table_init(smem);
    double* Wt = reinterpret_cast<double*>(smem + EXP_TABLE_BYTES);  // [16 NB][SCAN_PITCH]
    double* sv = Wt + W_DOUBLES;                                     // cn[16] | lden[16] | basis[B][16]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 15, q4 = lane >> 4;
    int64_t bin, q0c, q1c;
    cut.range(blockIdx.x, d.N, SCAN_CHUNK, bin, q0c, q1c);
    const int64_t pl = L - p0 < 64 * MB ? L - p0 : 64 * MB;  // members of the panel
    const int nblk = (int)((pl + 15) / 16);
    int mine = 0;
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) mine += (mb * 4 + wave) < nblk;
    mine = __builtin_amdgcn_readfirstlane(mine);

    double cf[MB][SCAN_MAX_B], off[MB], fs[MB];
    double cen[Fam::harmonic ? MB : 1][SCAN_MAX_H];
    bool mlive[MB];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
        const int64_t pm = (int64_t)(mb * 4 + wave) * 16 + col;
        mlive[mb] = pm < pl;
        const int64_t l = p0 + pm;
#pragma unroll
        for (int b = 0; b < SCAN_MAX_B; ++b) cf[mb][b] = (mlive[mb] && b < d.B) ? coeff[l * d.B + b] : 0.0;
        off[mb] = mlive[mb] ? offset[l] : 0.0;
        if constexpr (Fam::harmonic) family_load_centers(fam, mlive[mb], l, cen[mb]);
        fs[mb] = mlive[mb] ? fnorm[l] : 0.0;
    }
    const int fs_s = tid & 15, fs_r = tid >> 4;

    v4d acc[NB * NCB];
#pragma unroll
    for (int i = 0; i < NB * NCB; ++i) acc[i] = v4d{0.0, 0.0, 0.0, 0.0};
    double vs[MB][NV];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int v = 0; v < NV; ++v) vs[mb][v] = 0.0;

    __syncthreads();  // the exp table
    for (int64_t q0 = q0c; q0 < q1c; q0 += 16) {
        // ---- fill: the observable tile and the per-sample values of the tile
        {
            const int64_t q = q0 + fs_s;
            int64_t n = 0;
            double cn = 0.0, lden = 0.0;
            if (q < q1c) {
                n = q;
                cn = d.cw ? d.cw[n] : 1.0;
                if (cn > 0.0) lden = d.logden[n];
                else cn = 0.0;
            }
            const bool slive = cn > 0.0;
#pragma unroll
            for (int I = 0; I < NB; ++I) {
                const int row = 16 * I + fs_r;
                double v = 0.0;
                if (slive && row < nq) {
                    v = a[(int64_t)row * d.ldv + n];
                    if constexpr (MODE == 2) v = v * v;
                }
                Wt[row * SCAN_PITCH + fs_s] = v;
            }
            if (tid < 16) {
                sv[fs_s] = cn;
                sv[16 + fs_s] = lden;
            }
            if (fs_r < d.B) sv[SVB + fs_r * 16 + fs_s] = slive ? d.basis[(int64_t)fs_r * d.ldv + n] : 0.0;
        }
        __syncthreads();
        // ---- products: four groups of four positions
        if (mine > 0) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int s = 4 * g + q4;
                double at[NB];
#pragma unroll
                for (int I = 0; I < NB; ++I) at[I] = Wt[(16 * I + col) * SCAN_PITCH + s];
                const double cn = sv[s], lden = sv[16 + s];
                double bas[SCAN_MAX_B];
#pragma unroll
                for (int b = 0; b < SCAN_MAX_B; ++b) bas[b] = b < d.B ? sv[SVB + b * 16 + s] : 0.0;
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) {
                    if (mb < mine) {  // (wave-uniform)
                        double uu = off[mb];
#pragma unroll
                        for (int b = 0; b < SCAN_MAX_B; ++b)
                            if (b < d.B) uu = family_term(fam, b, uu, cf[mb][b], bas[b], family_center(fam, b, cen[Fam::harmonic ? mb : 0]));
                        double bv = scan_exp(fs[mb] + (-uu - lden));
                        if (!(cn > 0.0) || !mlive[mb]) bv = 0.0;
                        const double cb = cn * bv;
                        double z[J];
                        z[0] = MODE == 2 ? cb * bv : cb;
                        if constexpr (MODE == 1) z[1] = cb * bv;
                        vs[mb][0] += cb;
                        vs[mb][1] = fma(bv, cb, vs[mb][1]);
#pragma unroll
                        for (int I = 0; I < NB; ++I)
#pragma unroll
                            for (int j = 0; j < J; ++j)
                                acc[I * NCB + mb * J + j] = __builtin_amdgcn_mfma_f64_16x16x4f64(at[I], z[j], acc[I * NCB + mb * J + j], 0, 0, 0);
                    }
                }
            }
        }
        __syncthreads();
    }
    // ---- the record
    constexpr int64_t CROSS_DOUBLES = (int64_t)4 * NB * NCB * 256;
    double* rec = part + (int64_t)blockIdx.x * (CROSS_DOUBLES + (int64_t)64 * MB * NV);
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

// The chunk records of one (member panel, observable panel) added in chunk order, compensated.  Threads [0, pl J nq): column j of
// member p0 + pm and observable qb + qi into out0 (j = 0) or out1 (j = 1), L x Q row-major; threads behind them, [0, pl NV): wsum
// into vec0[p0 + pm], w2sum into vec1 (a NULL destination: nobody wants it).
__global__ void __launch_bounds__(SV_THREADS)
k_scan_obs_merge(int64_t nchunks, int NB, int J, int MB, int64_t Q, int64_t p0, int64_t pl, int64_t qb, int64_t nq,
                 const double* __restrict__ part, double* __restrict__ out0, double* __restrict__ out1, double* __restrict__ vec0,
                 double* __restrict__ vec1) {
    const int NCB = MB * J;
    const int64_t cross_doubles = (int64_t)4 * NB * NCB * 256, stride = cross_doubles + (int64_t)64 * MB * SCANOBS_NV;
    int64_t x = (int64_t)blockIdx.x * SV_THREADS + threadIdx.x;
    int64_t at;
    double* out;
    if (x < pl * J * nq) {
        const int64_t pm = x % pl, j = (x / pl) % J, qi = x / (pl * J);
        const int64_t blk = pm / 16, colm = pm % 16, wave = blk % 4, mb = blk / 4;
        const int64_t I = qi / 16, row = qi % 16, r = row >> 2, lane = (row & 3) * 16 + colm;
        at = (((wave * NB + I) * NCB + mb * J + j) * 4 + r) * 64 + lane;
        out = (j == 0 ? out0 : out1) + (p0 + pm) * Q + qb + qi;
    } else {
        x -= pl * J * nq;
        if (x >= pl * SCANOBS_NV) return;
        const int64_t pm = x % pl, v = x / pl;
        double* dst = v == 0 ? vec0 : vec1;
        if (!dst) return;
        at = cross_doubles + pm * SCANOBS_NV + v;
        out = dst + p0 + pm;
    }
    double s = 0.0, e = 0.0;
    const double* r = part + at;
    for (int64_t c = 0; c < nchunks; ++c, r += stride) scan_neumaier(s, e, *r);
    *out = s + e;
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------
// launch(the policies that travel as kernel arguments...): the family if it is harmonic, then the observable if it is the energy
template <class Fam, class Obs, class F>
static void with_policy_args(const Fam& fam, const Obs& obs, F&& launch) {
    if constexpr (Fam::harmonic && Obs::energy) launch(fam, obs);
    else if constexpr (Fam::harmonic) launch(fam);
    else if constexpr (Obs::energy) launch(obs);
    else launch();
}

template <class Cut, class Fam, class Obs>
hipError_t launch_scan_vec(hipStream_t s, const ScanData& d, const Cut& cut, const Fam& fam, const Obs& obs, bool sum, int64_t L,
                           const double* coeff, const double* offset, const double* M, double* rec) {
    if constexpr (Obs::energy) {
        if (!sum) return launch_scan_vec(s, d, cut, fam, ScanStored{}, false, L, coeff, offset, M, rec);
        if (d.Q < 1 || d.Q > 2) return hipErrorInvalidValue;
    }
    const int64_t nchunks = cut.c1(d.N, SCAN_VCHUNK) - cut.c0();
    if (L < 1 || nchunks < 1) return hipSuccess;
    const int64_t gx = (nchunks + SV_THREADS / 64 - 1) / (SV_THREADS / 64);
    const dim3 grid((unsigned)gx, (unsigned)((L + 63) / 64));
    if (gx > 0x7fffffff || grid.y > 65535u) return hipErrorInvalidValue;
    with_policy_args(fam, obs, [&](auto... a) {
        if (sum) hipLaunchKernelGGL((k_scan_vec<true, Cut, Fam, Obs, decltype(a)...>), grid, dim3(SV_THREADS), EXP_TABLE_BYTES, s, d, cut, L, coeff, offset, M, rec, a...);
        else if constexpr (!Obs::energy)
            hipLaunchKernelGGL((k_scan_vec<false, Cut, Fam, Obs, decltype(a)...>), grid, dim3(SV_THREADS), EXP_TABLE_BYTES, s, d, cut, L, coeff, offset, M, rec, a...);
    });
    return hipGetLastError();
}

template <class Cut>
hipError_t launch_scan_vec_merge(hipStream_t s, const ScanData& d, const Cut& cut, bool sum, int64_t L, const double* rec, double* M,
                                 double* lognum, double* mean) {
    const int64_t nbg = cut.b1() - cut.b0();
    if (L < 1 || nbg < 1) return hipSuccess;
    const int64_t blocks = (nbg * L + SV_THREADS - 1) / SV_THREADS;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks);
    if (sum) hipLaunchKernelGGL((k_scan_vec_merge<true, Cut>), grid, dim3(SV_THREADS), EXP_TABLE_BYTES, s, d, cut, L, rec, M, lognum, mean);
    else hipLaunchKernelGGL((k_scan_vec_merge<false, Cut>), grid, dim3(SV_THREADS), EXP_TABLE_BYTES, s, d, cut, L, rec, M, lognum, mean);
    return hipGetLastError();
}

template <class Fam>
hipError_t launch_scan_moments(hipStream_t s, const ScanData& d, const Fam& fam, const ScanMoments& mom, int64_t L, const double* coeff,
                               const double* offset, const double* M, double* rec) {
    const int64_t nchunks = (d.N + SCAN_VCHUNK - 1) / SCAN_VCHUNK;
    if (L < 1 || nchunks < 1) return hipSuccess;
    if (d.B < 1 || d.B > mom.bb || d.Q < 0 || d.Q > SCAN_MAX_Q) return hipErrorInvalidValue;
    const int64_t gx = (nchunks + SV_THREADS / 64 - 1) / (SV_THREADS / 64);
    const dim3 grid((unsigned)gx, (unsigned)((L + 63) / 64));
    if (gx > 0x7fffffff || grid.y > 65535u) return hipErrorInvalidValue;
#define MBAR_CASE(HB_, BB_)                                                                                                              \
    if (mom.hb == HB_ && mom.bb == BB_) {                                                                                                \
        if constexpr (Fam::harmonic) {                                                                                                   \
            if (__builtin_popcount(fam.terms.mask) > HB_ || (fam.terms.mask >> BB_) != 0) return hipErrorInvalidValue;                   \
            hipLaunchKernelGGL((k_scan_moments<HB_, BB_, Fam, Fam>), grid, dim3(SV_THREADS), EXP_TABLE_BYTES, s, d, L, coeff, offset, M, \
                               mom.center_phi, rec, fam);                                                                                \
        } else {                                                                                                                         \
            hipLaunchKernelGGL((k_scan_moments<HB_, BB_, Fam>), grid, dim3(SV_THREADS), EXP_TABLE_BYTES, s, d, L, coeff, offset, M,      \
                               mom.center_phi, rec);                                                                                     \
        }                                                                                                                                \
        return hipGetLastError();                                                                                                        \
    }
    if constexpr (Fam::harmonic) {
        MBAR_CASE(1, 3) MBAR_CASE(4, 8)
    } else {
        MBAR_CASE(0, 2) MBAR_CASE(0, 8)
    }
#undef MBAR_CASE
    return hipErrorInvalidValue;
}
template hipError_t launch_scan_moments<ScanLinear>(hipStream_t, const ScanData&, const ScanLinear&, const ScanMoments&, int64_t, const double*,
                                                    const double*, const double*, double*);
template hipError_t launch_scan_moments<ScanHarmonic>(hipStream_t, const ScanData&, const ScanHarmonic&, const ScanMoments&, int64_t,
                                                      const double*, const double*, const double*, double*);

hipError_t launch_scan_moments_merge(hipStream_t s, const ScanData& d, const ScanMoments& mom, int64_t L, const double* rec, const double* M,
                                     double* lognum, double* out) {
    if (L < 1 || d.N < 1) return hipSuccess;
    const int R = mom.record(d.Q);
    const int64_t blocks = (L * R + SV_THREADS - 1) / SV_THREADS;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_scan_moments_merge, dim3((unsigned)blocks), dim3(SV_THREADS), EXP_TABLE_BYTES, s, d, L, R, rec, M, lognum, out);
    return hipGetLastError();
}

int scan_nb_for(int64_t K) {  // blocks of 16 states the cross kernel is instantiated for
    const int need = (int)((K + 15) / 16);
    return need <= 1 ? 1 : need <= 2 ? 2 : need <= 4 ? 4 : 8;
}

int64_t scan_record_doubles(int nb, int J, int nv, int MB) {
    return (int64_t)4 * nb * MB * J * 256 + (int64_t)64 * MB * nv;
}

// the ladder over J: the whole cut is instantiated for J = 1 .. 4 (the energy observable: J = 2, 3), the binned cut for J = 1
template <int NB, class Cut, class Fam, class Obs>
static hipError_t launch_scan_cross_nb(hipStream_t s, const ScanData& d, const Cut& cut, const Fam& fam, const Obs& obs, dim3 grid, size_t lds,
                                       const double* u, int64_t ld, int64_t K, const double* f, int64_t L, int64_t p0, const double* coeff,
                                       const double* offset, const double* fnorm, double* part) {
    switch (Cut::binned ? 1 : 1 + d.Q) {
#define MBAR_CASE(J_)                                                                                                                    \
    case J_:                                                                                                                             \
        if constexpr ((J_ == 1 || !Cut::binned) && (!Obs::energy || J_ == 2 || J_ == 3))                                                 \
            with_policy_args(fam, obs, [&](auto... a) {                                                                                  \
                hipLaunchKernelGGL((k_scan_cross<NB, J_, Cut, Fam, Obs, decltype(a)...>), grid, dim3(256), lds, s, d, cut, u, ld, K, f,  \
                                   L, p0, coeff, offset, fnorm, part, a...);                                                             \
            });                                                                                                                          \
        else                                                                                                                             \
            return hipErrorInvalidValue;                                                                                                 \
        break;
        MBAR_CASE(1) MBAR_CASE(2) MBAR_CASE(3) MBAR_CASE(4)
#undef MBAR_CASE
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// nb: scan_nb_for(K), or 0 (no cross block: the per-member sums only)
template <class Cut, class Fam, class Obs>
hipError_t launch_scan_cross(hipStream_t s, const ScanData& d, const Cut& cut, const Fam& fam, const Obs& obs, int nb, const double* u,
                             int64_t ld, int64_t K, const double* f, int64_t L, int64_t p0, const double* coeff, const double* offset,
                             const double* fnorm, double* part) {
    const int64_t c0 = cut.c0(), c1 = cut.c1(d.N, SCAN_CHUNK);
    if (c1 <= c0 || p0 >= L) return hipSuccess;
    if (K > 16 * (int64_t)nb && nb > 0) return hipErrorInvalidValue;
    if (c1 - c0 > 0x7fffffff) return hipErrorInvalidValue;
    if constexpr (Cut::binned)
        if (c1 > cut.t.nchunks) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(c1 - c0));
    // sv: cn | lden | (the whole cut: br) | basis rows | (the whole cut: t rows; the energy observable has tr1 and no t rows)
    const size_t sv = Cut::binned ? 32 + (size_t)SCAN_MAX_B * 16 : 48 + (size_t)(SCAN_MAX_B + SCAN_MAX_Q) * 16;
    const size_t lds = EXP_TABLE_BYTES + ((size_t)nb * 16 * SCAN_PITCH + sv) * sizeof(double);
    switch (nb) {
#define MBAR_CASE(NB_) \
    case NB_: return launch_scan_cross_nb<NB_>(s, d, cut, fam, obs, grid, lds, u, ld, K, f, L, p0, coeff, offset, fnorm, part);
        MBAR_CASE(0) MBAR_CASE(1) MBAR_CASE(2) MBAR_CASE(4) MBAR_CASE(8)
#undef MBAR_CASE
        default: return hipErrorInvalidValue;
    }
}

template <class Cut, class Obs>
hipError_t launch_scan_cross_merge(hipStream_t s, const ScanData& d, const Cut& cut, int nb, int mb, int64_t K, int64_t L, int64_t p0,
                                   const double* part, double* cross, double* vec) {
    const int64_t nbg = cut.b1() - cut.b0();
    if (nbg < 1 || p0 >= L || (!Cut::binned && d.N < 1)) return hipSuccess;  // (a bin without a chunk still gets its zeros)
    const int J = Cut::binned ? 1 : 1 + d.Q;
    const int64_t pl = L - p0 < 64 * mb ? L - p0 : 64 * mb;
    const int64_t threads = nbg * ((nb > 0 ? pl * J * K : 0) + pl * (Cut::binned ? SCANBIN_NV : Obs::nv(J)));
    const int64_t blocks = (threads + SV_THREADS - 1) / SV_THREADS;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL((k_scan_cross_merge<Cut, Obs>), dim3((unsigned)blocks), dim3(SV_THREADS), 0, s, d, cut, nb, K, L, p0, pl, part, cross, vec, mb);
    return hipGetLastError();
}

// ---- the member-member Gram block: nb = scan_pair_nb_for(rows left, J), rm <= scan_pair_rows(nb, J) reference members rows[0 .. rm)
int scan_pair_nb_for(int64_t R, int J) { return R <= scan_pair_rows(2, J) ? 2 : 8; }

int64_t scan_pair_record_doubles(int nb, int J, int MB) { return (int64_t)4 * nb * MB * J * 256; }

template <class Fam>
hipError_t launch_scan_pair(hipStream_t s, const ScanData& d, const Fam& fam, int nb, int64_t L, int64_t p0, const int64_t* rows, int rm,
                            const double* coeff, const double* offset, const double* fnorm, double* part) {
    const int64_t nchunks = (d.N + SCAN_CHUNK - 1) / SCAN_CHUNK;
    const int J = 1 + d.Q;
    if (nchunks < 1 || p0 >= L) return hipSuccess;
    if (nchunks > 0x7fffffff || J < 1 || J > 1 + SCAN_MAX_Q || (nb != 2 && nb != 8) || rm < 1 || rm > scan_pair_rows(nb, J))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)nchunks);
    const size_t lds = EXP_TABLE_BYTES + ((size_t)nb * 16 * SCAN_PITCH + 32 + (size_t)(SCAN_MAX_B + SCAN_MAX_Q) * 16 +
                                          (size_t)scan_pair_rows(nb, J) * PAIR_RP) * sizeof(double);
#define MBAR_CASE(NB_, J_)                                                                                                                   \
    if (nb == NB_ && J == J_) {                                                                                                              \
        if constexpr (Fam::harmonic)                                                                                                         \
            hipLaunchKernelGGL((k_scan_pair<NB_, J_, Fam, Fam>), grid, dim3(256), lds, s, d, L, p0, rows, rm, coeff, offset, fnorm, part, fam); \
        else                                                                                                                                 \
            hipLaunchKernelGGL((k_scan_pair<NB_, J_, Fam>), grid, dim3(256), lds, s, d, L, p0, rows, rm, coeff, offset, fnorm, part);        \
        return hipGetLastError();                                                                                                            \
    }
    MBAR_CASE(2, 1) MBAR_CASE(2, 2) MBAR_CASE(2, 3) MBAR_CASE(2, 4) MBAR_CASE(8, 1) MBAR_CASE(8, 2) MBAR_CASE(8, 3) MBAR_CASE(8, 4)
#undef MBAR_CASE
    return hipErrorInvalidValue;
}
template hipError_t launch_scan_pair<ScanLinear>(hipStream_t, const ScanData&, const ScanLinear&, int, int64_t, int64_t, const int64_t*, int,
                                                 const double*, const double*, const double*, double*);
template hipError_t launch_scan_pair<ScanHarmonic>(hipStream_t, const ScanData&, const ScanHarmonic&, int, int64_t, int64_t, const int64_t*, int,
                                                   const double*, const double*, const double*, double*);

hipError_t launch_scan_pair_merge(hipStream_t s, const ScanData& d, int nb, int mb, int64_t L, int64_t p0, int rm, const double* part,
                                  double* pair) {
    if (p0 >= L || d.N < 1) return hipSuccess;
    const int J = 1 + d.Q;
    const int64_t pl = L - p0 < 64 * mb ? L - p0 : 64 * mb;
    const int64_t blocks = ((int64_t)rm * J * pl * J + SV_THREADS - 1) / SV_THREADS;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_scan_pair_merge, dim3((unsigned)blocks), dim3(SV_THREADS), 0, s, (d.N + SCAN_CHUNK - 1) / SCAN_CHUNK, nb, J, mb, rm, L, p0, pl,
                       part, pair);
    return hipGetLastError();
}

// ---- many observables along a scan: nb = scan_nb_for(nq) blocks of 16 observables, mode 0, 1 or 2 (k_scan_obs)
int scan_obs_columns(int mode) { return mode == 1 ? 2 : 1; }

int64_t scan_obs_record_doubles(int nb, int J, int MB) { return (int64_t)4 * nb * MB * J * 256 + (int64_t)64 * MB * SCANOBS_NV; }

template <class Fam>
hipError_t launch_scan_obs(hipStream_t s, const ScanData& d, const Fam& fam, int nb, int mode, const double* a, int64_t nq, int64_t L,
                           int64_t p0, const double* coeff, const double* offset, const double* fnorm, double* part) {
    const int64_t nchunks = (d.N + SCAN_CHUNK - 1) / SCAN_CHUNK;
    if (nchunks < 1 || p0 >= L) return hipSuccess;
    if (nchunks > 0x7fffffff || nq < 1 || nq > 16 * (int64_t)nb || d.B < 1 || d.B > SCAN_MAX_B) return hipErrorInvalidValue;
    const dim3 grid((unsigned)nchunks);
    const size_t lds = EXP_TABLE_BYTES + ((size_t)nb * 16 * SCAN_PITCH + 32 + (size_t)SCAN_MAX_B * 16) * sizeof(double);
#define MBAR_CASE(NB_, MODE_)                                                                                                              \
    if (nb == NB_ && mode == MODE_) {                                                                                                      \
        if constexpr (Fam::harmonic)                                                                                                       \
            hipLaunchKernelGGL((k_scan_obs<NB_, MODE_, Fam, Fam>), grid, dim3(256), lds, s, d, a, (int)nq, L, p0, coeff, offset, fnorm, part, fam); \
        else                                                                                                                               \
            hipLaunchKernelGGL((k_scan_obs<NB_, MODE_, Fam>), grid, dim3(256), lds, s, d, a, (int)nq, L, p0, coeff, offset, fnorm, part);  \
        return hipGetLastError();                                                                                                          \
    }
#define MBAR_MODES(NB_) MBAR_CASE(NB_, 0) MBAR_CASE(NB_, 1) MBAR_CASE(NB_, 2)
    MBAR_MODES(1) MBAR_MODES(2) MBAR_MODES(4) MBAR_MODES(8)
#undef MBAR_MODES
#undef MBAR_CASE
    return hipErrorInvalidValue;
}
template hipError_t launch_scan_obs<ScanLinear>(hipStream_t, const ScanData&, const ScanLinear&, int, int, const double*, int64_t, int64_t,
                                                int64_t, const double*, const double*, const double*, double*);
template hipError_t launch_scan_obs<ScanHarmonic>(hipStream_t, const ScanData&, const ScanHarmonic&, int, int, const double*, int64_t, int64_t,
                                                  int64_t, const double*, const double*, const double*, double*);

hipError_t launch_scan_obs_merge(hipStream_t s, const ScanData& d, int nb, int mode, int mb, int64_t L, int64_t Q, int64_t p0, int64_t qb,
                                 int64_t nq, const double* part, double* out0, double* out1, double* vec0, double* vec1) {
    if (p0 >= L || d.N < 1) return hipSuccess;
    const int J = scan_obs_columns(mode);
    const int64_t pl = L - p0 < 64 * mb ? L - p0 : 64 * mb;
    const int64_t blocks = (pl * J * nq + pl * SCANOBS_NV + SV_THREADS - 1) / SV_THREADS;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_scan_obs_merge, dim3((unsigned)blocks), dim3(SV_THREADS), 0, s, (d.N + SCAN_CHUNK - 1) / SCAN_CHUNK, nb, J, mb, Q, p0, pl,
                       qb, nq, part, out0, out1, vec0, vec1);
    return hipGetLastError();
}

#define MBAR_SWEEPS(Cut, Fam, Obs)                                                                                                      \
    template hipError_t launch_scan_vec<Cut, Fam, Obs>(hipStream_t, const ScanData&, const Cut&, const Fam&, const Obs&, bool, int64_t,          \
                                                       const double*, const double*, const double*, double*);                                    \
    template hipError_t launch_scan_cross<Cut, Fam, Obs>(hipStream_t, const ScanData&, const Cut&, const Fam&, const Obs&, int, const double*,   \
                                                         int64_t, int64_t, const double*, int64_t, int64_t, const double*, const double*,        \
                                                         const double*, double*);
#define MBAR_MERGES(Cut, Obs)                                                                                                                    \
    template hipError_t launch_scan_cross_merge<Cut, Obs>(hipStream_t, const ScanData&, const Cut&, int, int, int64_t, int64_t, int64_t,         \
                                                          const double*, double*, double*);
#define MBAR_CUT(Cut)                                                                                                                            \
    MBAR_SWEEPS(Cut, ScanLinear, ScanStored)                                                                                                     \
    MBAR_SWEEPS(Cut, ScanHarmonic, ScanStored)                                                                                                   \
    MBAR_MERGES(Cut, ScanStored)                                                                                                                 \
    template hipError_t launch_scan_vec_merge<Cut>(hipStream_t, const ScanData&, const Cut&, bool, int64_t, const double*, double*, double*,     \
                                                   double*);
MBAR_CUT(ScanWhole)
MBAR_CUT(ScanBinned)
MBAR_SWEEPS(ScanWhole, ScanLinear, ScanEnergy)
MBAR_SWEEPS(ScanWhole, ScanHarmonic, ScanEnergy)
MBAR_MERGES(ScanWhole, ScanEnergy)
#undef MBAR_CUT
#undef MBAR_MERGES
#undef MBAR_SWEEPS

// ---- kernel-density surfaces along a scan (mbar_scan_kde_sums) -----------------------------------------------
// The gaussian density of EVERY member of the family at M query points,
//   S[l][m] = sum_n c_n b_ln k(q_m, x_n),   b_ln = exp(f_scan[l] - u_l(n) - logden_n),   k = exp(-r^2 / 2h^2),
// an (M x N)(N x L) product with BOTH operands generated on the device: the member weight from the B numbers per sample as in pass B,
// the kernel value from the d coordinates per sample the context keeps (mbar_ctx_set_scan_points).  k_scan_kde is k_scan_obs (mode 0)
// with another fill stage: where that one loads a tile of stored observables, this one computes the tile k(q_i, x_n) of 16 NB queries x
// 16 positions, NB exponentials per thread.  Everything behind the fill -- the product stage, the record, the chunks cut by N alone,
// the member panels -- is that kernel's, so one member exponential serves up to 128 queries and one kernel exponential every member of
// the panel.  k <= 1 and c_n b_ln <= 1 for a normalised member: the sums cannot overflow and carry no running shift.
// k_scan_kde_merge adds the chunk records in chunk order, compensated, and writes log S; a pair whose sum is not >= 2^-900 (underflow,
// or a NaN) gets a NaN there, and the host hands the pairs of members with wsum > 0 among them to k_scan_kde_exact, which works in
// plain log space with the pair's own maximum.  The displacement of a coordinate with period P > 0 is the minimum image, formed by
// the operations of the harmonic chain (family_term): dl = q - x; dl = fma(-P, rint(dl rP), dl).
namespace {
constexpr double SCANKDE_FLAG_BELOW = 0x1p-900;  // merged sums not at or above this are recomputed by k_scan_kde_exact

// the displacement of coordinate k from a sample to a query
__device__ __forceinline__ double scan_kde_dl(const ScanKde& kd, int k, double q, double x) {
    double dl = q - x;
    const double P = kd.period[k];
    if (P > 0.0) {
        const double m = rint(dl * kd.rperiod[k]);
        dl = fma(-P, m, dl);
    }
    return dl;
}
}  // namespace

// One workgroup owns one chunk, one panel of 64 MB members (MB = Fam::mb(1)) and one panel of nq <= 16 NB queries, those from qb on.
// Fill: thread tid computes the NB values of rows 16 I + (tid >> 4) at position tid & 15 -- D subtractions, the wrap where a period is
// set, r^2 by fma in coordinate order, exp2s_fast(r^2 coef) -- with exact zeros where c_n <= 0, past nq and past the chunk.  The
// queries of the panel wait in LDS ([D][16 NB]).  The record is k_scan_obs's with one per-member sum: [wave][I < NB][mb < MB][r < 4]
// [lane], then [pm < 64 MB] wsum.  An element's operations depend neither on the row it has in the tile nor on NB, the member's
// column or MB.
template <int NB, int D, class Fam, class... Arg>
__global__ void __launch_bounds__(256)
k_scan_kde(ScanData d, ScanKde kd, int64_t qb, int nq, int64_t L, int64_t p0, const double* __restrict__ coeff,
           const double* __restrict__ offset, const double* __restrict__ fnorm, double* __restrict__ part, Arg... arg) {
    const Fam fam = scan_arg<Fam>(arg...);
    const ScanWhole cut{};
    constexpr int MB = Fam::mb(1);
    static_assert(NB * MB <= 32, "at most 32 accumulator blocks per wave");
    constexpr int SVB = 32;  // where the basis rows start in sv
    constexpr int W_DOUBLES = NB * 16 * SCAN_PITCH;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    exp_table_init(smem);
    double* Wt = reinterpret_cast<double*>(smem + EXP_TABLE_BYTES);  // [16 NB][SCAN_PITCH]
    double* sv = Wt + W_DOUBLES;                                     // cn[16] | lden[16] | basis[SCAN_MAX_B][16]
    double* qs = sv + SVB + SCAN_MAX_B * 16;                         // [D][16 NB]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int col = lane & 15, q4 = lane >> 4;
    int64_t bin, q0c, q1c;
    cut.range(blockIdx.x, d.N, SCAN_CHUNK, bin, q0c, q1c);
    const int64_t pl = L - p0 < 64 * MB ? L - p0 : 64 * MB;  // members of the panel
    const int nblk = (int)((pl + 15) / 16);
    int mine = 0;
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) mine += (mb * 4 + wave) < nblk;
    mine = __builtin_amdgcn_readfirstlane(mine);

    double cf[MB][SCAN_MAX_B], off[MB], fs[MB];
    double cen[Fam::harmonic ? MB : 1][SCAN_MAX_H];
    bool mlive[MB];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
        const int64_t pm = (int64_t)(mb * 4 + wave) * 16 + col;
        mlive[mb] = pm < pl;
        const int64_t l = p0 + pm;
#pragma unroll
        for (int b = 0; b < SCAN_MAX_B; ++b) cf[mb][b] = (mlive[mb] && b < d.B) ? coeff[l * d.B + b] : 0.0;
        off[mb] = mlive[mb] ? offset[l] : 0.0;
        if constexpr (Fam::harmonic) family_load_centers(fam, mlive[mb], l, cen[mb]);
        fs[mb] = mlive[mb] ? fnorm[l] : 0.0;
    }
    const int fs_s = tid & 15, fs_r = tid >> 4;
    for (int i = tid; i < D * 16 * NB; i += 256) {
        const int k = i / (16 * NB), row = i % (16 * NB);
        qs[i] = row < nq ? kd.q[(int64_t)k * kd.ldq + qb + row] : 0.0;
    }

    v4d acc[NB * MB];
#pragma unroll
    for (int i = 0; i < NB * MB; ++i) acc[i] = v4d{0.0, 0.0, 0.0, 0.0};
    double vs[MB];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) vs[mb] = 0.0;

    __syncthreads();  // the exp table, the queries
    for (int64_t q0 = q0c; q0 < q1c; q0 += 16) {
        // ---- fill: the kernel tile and the per-sample values of the tile
        {
            const int64_t q = q0 + fs_s;
            int64_t n = 0;
            double cn = 0.0, lden = 0.0;
            if (q < q1c) {
                n = q;
                cn = d.cw ? d.cw[n] : 1.0;
                if (cn > 0.0) lden = d.logden[n];
                else cn = 0.0;
            }
            const bool slive = cn > 0.0;
            double xc[D];
#pragma unroll
            for (int k = 0; k < D; ++k) xc[k] = slive ? kd.x[(int64_t)k * d.ldv + n] : 0.0;
#pragma unroll
            for (int I = 0; I < NB; ++I) {
                const int row = 16 * I + fs_r;
                double v = 0.0;
                if (slive && row < nq) {
                    double r2 = 0.0;
#pragma unroll
                    for (int k = 0; k < D; ++k) {
                        const double dl = scan_kde_dl(kd, k, qs[k * 16 * NB + row], xc[k]);
                        r2 = fma(dl, dl, r2);
                    }
                    v = exp2s_fast(r2 * kd.coef);
                }
                Wt[row * SCAN_PITCH + fs_s] = v;
            }
            if (tid < 16) {
                sv[fs_s] = cn;
                sv[16 + fs_s] = lden;
            }
            if (fs_r < d.B) sv[SVB + fs_r * 16 + fs_s] = slive ? d.basis[(int64_t)fs_r * d.ldv + n] : 0.0;
        }
        __syncthreads();
        // ---- products: four groups of four positions (k_scan_obs's, one operand column per member)
        if (mine > 0) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int s = 4 * g + q4;
                double at[NB];
#pragma unroll
                for (int I = 0; I < NB; ++I) at[I] = Wt[(16 * I + col) * SCAN_PITCH + s];
                const double cn = sv[s], lden = sv[16 + s];
                double bas[SCAN_MAX_B];
#pragma unroll
                for (int b = 0; b < SCAN_MAX_B; ++b) bas[b] = b < d.B ? sv[SVB + b * 16 + s] : 0.0;
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) {
                    if (mb < mine) {  // (wave-uniform)
                        double uu = off[mb];
#pragma unroll
                        for (int b = 0; b < SCAN_MAX_B; ++b)
                            if (b < d.B) uu = family_term(fam, b, uu, cf[mb][b], bas[b], family_center(fam, b, cen[Fam::harmonic ? mb : 0]));
                        double bv = scan_exp(fs[mb] + (-uu - lden));
                        if (!(cn > 0.0) || !mlive[mb]) bv = 0.0;
                        const double cb = cn * bv;
                        vs[mb] += cb;
#pragma unroll
                        for (int I = 0; I < NB; ++I) acc[I * MB + mb] = __builtin_amdgcn_mfma_f64_16x16x4f64(at[I], cb, acc[I * MB + mb], 0, 0, 0);
                    }
                }
            }
        }
        __syncthreads();
    }
    // ---- the record
    constexpr int64_t CROSS_DOUBLES = (int64_t)4 * NB * MB * 256;
    double* rec = part + (int64_t)blockIdx.x * (CROSS_DOUBLES + (int64_t)64 * MB);
#pragma unroll
    for (int i = 0; i < NB * MB; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) rec[(((int64_t)wave * NB * MB + i) * 4 + r) * 64 + lane] = acc[i][r];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
        double x = vs[mb];
        x += __shfl_xor(x, 16);
        x += __shfl_xor(x, 32);
        if (lane < 16) rec[CROSS_DOUBLES + (int64_t)(mb * 4 + wave) * 16 + lane] = x;
    }
}

// The chunk records of one (member panel, query panel) added in chunk order, compensated.  Threads [0, pl nq): member p0 + pm and
// query qb + qi, logsum[(p0 + pm) M + qb + qi] = log S, or NaN where !(S >= 2^-900): the exact kernel's, if the member has weight.
// Threads behind them, [0, pl): wsum[p0 + pm] (a NULL destination: another query panel wrote it).
__global__ void __launch_bounds__(SV_THREADS)
k_scan_kde_merge(int64_t nchunks, int NB, int MB, int64_t M, int64_t p0, int64_t pl, int64_t qb, int64_t nq, const double* __restrict__ part,
                 double* __restrict__ logsum, double* __restrict__ wsum) {
    const int64_t cross_doubles = (int64_t)4 * NB * MB * 256, stride = cross_doubles + (int64_t)64 * MB;
    int64_t x = (int64_t)blockIdx.x * SV_THREADS + threadIdx.x;
    int64_t at;
    double* out;
    const bool cross = x < pl * nq;
    if (cross) {
        const int64_t pm = x % pl, qi = x / pl;
        const int64_t blk = pm / 16, colm = pm % 16, wave = blk % 4, mb = blk / 4;
        const int64_t I = qi / 16, row = qi % 16, r = row >> 2, lane = (row & 3) * 16 + colm;
        at = (((wave * NB + I) * MB + mb) * 4 + r) * 64 + lane;
        out = logsum + (p0 + pm) * M + qb + qi;
    } else {
        x -= pl * nq;
        if (x >= pl || !wsum) return;
        at = cross_doubles + x;
        out = wsum + p0 + x;
    }
    double s = 0.0, e = 0.0;
    const double* r = part + at;
    for (int64_t c = 0; c < nchunks; ++c, r += stride) scan_neumaier(s, e, *r);
    s += e;
    if (cross) s = s >= SCANKDE_FLAG_BELOW ? log(s) : NAN;
    *out = s;
}

// One workgroup per pair (member pairs[2 i], query pairs[2 i + 1]): two passes over the samples in plain log space -- the maximum
// over the samples with c_n > 0 of (f_scan[l] - u_l(n) - logden_n) - r^2 / 2h^2, then the sum of c_n exp(. - max) -- with fixed-order
// tree reductions; out[i] = max + log(sum), -inf when no sample has c_n > 0 or every term is below the fp64 range.  A displacement
// whose square overflows is measured in units of its largest coordinate as k_kde_exact does: never NaN for finite input.
template <class Fam, class... Arg>
__global__ void __launch_bounds__(256)
k_scan_kde_exact(ScanData d, ScanKde kd, const int64_t* __restrict__ pairs, const double* __restrict__ coeff,
                 const double* __restrict__ offset, const double* __restrict__ fnorm, double* __restrict__ out, Arg... arg) {
    const Fam fam = scan_arg<Fam>(arg...);
    __shared__ double red[256];
    const int64_t l = pairs[2 * blockIdx.x], m = pairs[2 * blockIdx.x + 1];
    const int tid = threadIdx.x;
    double cf[SCAN_MAX_B], cen[SCAN_MAX_H];
#pragma unroll
    for (int b = 0; b < SCAN_MAX_B; ++b) cf[b] = b < d.B ? coeff[l * d.B + b] : 0.0;
    family_load_centers(fam, true, l, cen);
    const double off = offset[l], fs = fnorm[l];
    double qc[SCANKDE_MAX_D];
#pragma unroll
    for (int k = 0; k < SCANKDE_MAX_D; ++k) qc[k] = k < kd.d ? kd.q[(int64_t)k * kd.ldq + m] : 0.0;
    const double inv_h2 = kd.inv_h * kd.inv_h;
    auto logterm = [&](int64_t n) -> double {
        const double cn = d.cw ? d.cw[n] : 1.0;
        if (!(cn > 0.0)) return -INFINITY;
        const double uu = scan_u(d, fam, cf, cen, off, n);
        const double x = fs + (-uu - d.logden[n]);
        double r2 = 0.0;
#pragma unroll
        for (int k = 0; k < SCANKDE_MAX_D; ++k)
            if (k < kd.d) {
                const double dl = scan_kde_dl(kd, k, qc[k], kd.x[(int64_t)k * d.ldv + n]);
                r2 = fma(dl, dl, r2);
            }
        double lk;
        if (r2 < INFINITY) {
            lk = -0.5 * r2 * inv_h2;
        } else {
            // r^2 is beyond the fp64 range, r / h need not be: halved displacements (q - x itself may overflow where no period
            // folds it) in units of the largest one
            double hd[SCANKDE_MAX_D], amax = 0.0;
#pragma unroll
            for (int k = 0; k < SCANKDE_MAX_D; ++k) {
                hd[k] = 0.0;
                if (k < kd.d) {
                    const double xk = kd.x[(int64_t)k * d.ldv + n];
                    hd[k] = kd.period[k] > 0.0 ? 0.5 * scan_kde_dl(kd, k, qc[k], xk) : 0.5 * qc[k] - 0.5 * xk;
                }
                amax = fmax(amax, fabs(hd[k]));
            }
            double u2 = 0.0;
#pragma unroll
            for (int k = 0; k < SCANKDE_MAX_D; ++k) {
                const double u = hd[k] / amax;
                u2 = fma(u, u, u2);
            }
            const double rh = 2.0 * (amax * kd.inv_h * sqrt(u2));  // r / h (inf when that is out of range too)
            lk = -0.5 * rh * rh;
        }
        return x + lk;
    };
    double mx = -INFINITY;
    for (int64_t n = tid; n < d.N; n += 256) mx = fmax(mx, logterm(n));
    red[tid] = mx;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) red[tid] = fmax(red[tid], red[tid + w]);
        __syncthreads();
    }
    mx = red[0];
    __syncthreads();
    double s = 0.0;
    if (mx > -INFINITY)
        for (int64_t n = tid; n < d.N; n += 256) {
            const double t = logterm(n);
            if (t > -INFINITY) s = fma(d.cw ? d.cw[n] : 1.0, exp(t - mx), s);
        }
    red[tid] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) out[blockIdx.x] = mx > -INFINITY ? mx + log(red[0]) : -INFINITY;
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------
ScanKde scan_kde_make(int d, const double* x, const double* q, int64_t ldq, int64_t M, double h, const double* period) {
    ScanKde kd{};
    kd.d = d;
    kd.x = x;
    kd.q = q;
    kd.ldq = ldq;
    kd.M = M;
    kd.inv_h = 1.0 / h;
    kd.coef = -(LOG2E_S * (0.5 / (h * h)));
    for (int k = 0; k < SCANKDE_MAX_D; ++k) {
        const double P = (period && k < d) ? period[k] : 0.0;
        kd.period[k] = P;
        kd.rperiod[k] = P > 0.0 ? 1.0 / P : 0.0;
    }
    return kd;
}

int64_t scan_kde_record_doubles(int nb, int mb) { return (int64_t)4 * nb * mb * 256 + (int64_t)64 * mb; }

template <class Fam>
hipError_t launch_scan_kde(hipStream_t s, const ScanData& d, const Fam& fam, const ScanKde& kd, int nb, int64_t qb, int64_t nq, int64_t L,
                           int64_t p0, const double* coeff, const double* offset, const double* fnorm, double* part) {
    const int64_t nchunks = (d.N + SCAN_CHUNK - 1) / SCAN_CHUNK;
    if (nchunks < 1 || p0 >= L) return hipSuccess;
    if (nchunks > 0x7fffffff || nq < 1 || nq > 16 * (int64_t)nb || qb < 0 || qb + nq > kd.M || d.B < 1 || d.B > SCAN_MAX_B)
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)nchunks);
    const size_t lds = EXP_TABLE_BYTES + ((size_t)nb * 16 * SCAN_PITCH + 32 + (size_t)SCAN_MAX_B * 16 + (size_t)SCANKDE_MAX_D * 16 * nb) * sizeof(double);
#define MBAR_CASE(NB_, D_)                                                                                                                  \
    if (nb == NB_ && kd.d == D_) {                                                                                                          \
        if constexpr (Fam::harmonic)                                                                                                        \
            hipLaunchKernelGGL((k_scan_kde<NB_, D_, Fam, Fam>), grid, dim3(256), lds, s, d, kd, qb, (int)nq, L, p0, coeff, offset, fnorm, part, fam); \
        else                                                                                                                                \
            hipLaunchKernelGGL((k_scan_kde<NB_, D_, Fam>), grid, dim3(256), lds, s, d, kd, qb, (int)nq, L, p0, coeff, offset, fnorm, part);  \
        return hipGetLastError();                                                                                                           \
    }
#define MBAR_DIMS(NB_) MBAR_CASE(NB_, 1) MBAR_CASE(NB_, 2)
    MBAR_DIMS(1) MBAR_DIMS(2) MBAR_DIMS(4) MBAR_DIMS(8)
#undef MBAR_DIMS
#undef MBAR_CASE
    return hipErrorInvalidValue;
}
template hipError_t launch_scan_kde<ScanLinear>(hipStream_t, const ScanData&, const ScanLinear&, const ScanKde&, int, int64_t, int64_t, int64_t,
                                                int64_t, const double*, const double*, const double*, double*);
template hipError_t launch_scan_kde<ScanHarmonic>(hipStream_t, const ScanData&, const ScanHarmonic&, const ScanKde&, int, int64_t, int64_t,
                                                  int64_t, int64_t, const double*, const double*, const double*, double*);

hipError_t launch_scan_kde_merge(hipStream_t s, const ScanData& d, const ScanKde& kd, int nb, int mb, int64_t L, int64_t p0, int64_t qb,
                                 int64_t nq, const double* part, double* logsum, double* wsum) {
    if (p0 >= L || d.N < 1) return hipSuccess;
    const int64_t pl = L - p0 < 64 * mb ? L - p0 : 64 * mb;
    const int64_t blocks = (pl * nq + pl + SV_THREADS - 1) / SV_THREADS;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_scan_kde_merge, dim3((unsigned)blocks), dim3(SV_THREADS), 0, s, (d.N + SCAN_CHUNK - 1) / SCAN_CHUNK, nb, mb, kd.M, p0, pl,
                       qb, nq, part, logsum, wsum);
    return hipGetLastError();
}

template <class Fam>
hipError_t launch_scan_kde_exact(hipStream_t s, const ScanData& d, const Fam& fam, const ScanKde& kd, int64_t npairs, const int64_t* pairs,
                                 const double* coeff, const double* offset, const double* fnorm, double* out) {
    if (npairs <= 0) return hipSuccess;
    if (npairs > 0x7fffffff || d.N < 1 || kd.d < 1 || kd.d > SCANKDE_MAX_D) return hipErrorInvalidValue;
    if constexpr (Fam::harmonic)
        hipLaunchKernelGGL((k_scan_kde_exact<Fam, Fam>), dim3((unsigned)npairs), dim3(256), 0, s, d, kd, pairs, coeff, offset, fnorm, out, fam);
    else
        hipLaunchKernelGGL((k_scan_kde_exact<Fam>), dim3((unsigned)npairs), dim3(256), 0, s, d, kd, pairs, coeff, offset, fnorm, out);
    return hipGetLastError();
}
template hipError_t launch_scan_kde_exact<ScanLinear>(hipStream_t, const ScanData&, const ScanLinear&, const ScanKde&, int64_t, const int64_t*,
                                                      const double*, const double*, const double*, double*);
template hipError_t launch_scan_kde_exact<ScanHarmonic>(hipStream_t, const ScanData&, const ScanHarmonic&, const ScanKde&, int64_t,
                                                        const int64_t*, const double*, const double*, const double*, double*);

}  // namespace mbar
