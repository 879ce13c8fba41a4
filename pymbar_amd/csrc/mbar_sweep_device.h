// Device-side helpers of the solver's sweep kernels (mbar_k_eval.hip, mbar_k_gram.hip, mbar_k_quad.hip, mbar_k_pmode.hip,
// mbar_k_fused.hip; mbar_k_loop.hip reads one of the constants): tile staging, the log-sum-exp groups, the constants they share.
//
// Data layout.  u is the (Kp x ld) row-major fp64 matrix of reduced potentials u[k][n] of this
// rank's column shard (Kp = padded state count, ld = N rounded up to 16; padding is zero-filled and
// masked).  The fast kernels process "wave tiles" of 16 consecutive samples x all states: one
// 128-byte line per state row, staged into a wave-private LDS buffer by LDS-DMA
// (global_load_lds_dwordx4, 8 rows per instruction).  Inside LDS, row k is stored rotated by
// (k & 14) doubles so that the MFMA-operand read -- lane l holds state 16*I + (l & 15) of sample
// 4*g + (l >> 4), the A/B layout of v_mfma_f64_16x16x4_f64 -- is a conflict-free ds_read_b64.
// In that layout
//   * the per-sample reduction over states (log-sum-exp denominator, mbar_solvers.py:238) is an
//     in-register reduction over the block index I plus a 16-lane DPP butterfly,
//   * the per-state reduction over samples (numerator sums, mbar_solvers.py:240-241) is a plain
//     per-lane accumulation, and
//   * the K x K contraction W^T W of the Hessian (mbar_solvers.py:407) is
//     acc[I][J] += mfma_f64_16x16x4(p[I], p[J]) with no data movement at all.
// Waves never synchronise with each other; every wave streams its own tiles (tile index strided by
// the number of waves in the grid) with a one-tile DMA prefetch.
#ifndef MBAR_SWEEP_DEVICE_H
#define MBAR_SWEEP_DEVICE_H
#include "mbar_device.h"
#include "mbar_internal.h"

#include <hip/hip_ext.h>
#include <type_traits>

namespace mbar {

// Log-sum-exp step for TWO 4-sample groups of a tile at once (independent chains interleaved):
//   x = a - u;  m2 = 32 log2(e) max_k x;  e = 2^((32 log2(e) x - m2)/32);  s = sum_k e;  acc[0] += e / s
// A second candidate f' costs no second exp: exp(a'_k - u_kn - m) = e_kn * c_k with the per-state constant
// c_k = exp(a'_k - a_k), so  e' = e c,  s' = sum_k e',  acc[1] += e' / s'  (3 fp64 ops per element instead of ~20).
// logden_f = m2 ln2/32 + log s_f for both candidates (same shift m2).
// logden_n = shift + log(sum) for every candidate with ONE log per tile: all 16 lanes of a DPP row hold the sums of
// all candidates of their sample, so lanes ks in [4f, 4f+4) evaluate candidate f ((ks & 3) = the group whose
// sample this lane kept).  objl accumulates this lane's objective terms; its candidate is (ks >> 2).
template <int NF>
__device__ __forceinline__ void logden_out(double mm, const double (&ss)[NF], int ks, bool sample_ok, int64_t n,
                                           double wn, double* __restrict__ logden0, double* __restrict__ logden1,
                                           const double* __restrict__ dn, double& objl) {
    const bool second = NF == 2 && (ks & 4);
    const double s_first = ss[0], s_second = ss[NF - 1];  // (scalars: a select on ss[] itself becomes a scratch array)
    const double ldv = fma(mm, LN2_OVER_S, log_pos(second ? s_second : s_first));
    if (sample_ok && ks < 4 * NF) {
        double* out = second ? logden1 : logden0;
        if (out) out[n] = ldv;
        objl = fma(wn, dn ? (ldv - dn[n]) : ldv, objl);
    }
}
template <int NF>
__device__ __forceinline__ void objective_out(double objl, int ks, int lane, double* __restrict__ obj_part, int64_t rec) {
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        const double o = wave_sum((ks >> 2) == f ? objl : 0.0);
        if (lane == 0) obj_part[rec * NF + f] = o;
    }
}
template <int NB>
__device__ __forceinline__ void lse_load2(const char* cbuf, int rd0, int rd1, const double (&a)[NB],
                                          double (&x0)[NB], double (&x1)[NB]) {
    // all 2 NB reads are issued before the first use: left to itself hipcc interleaves the subtractions with the reads in
    // three batches, and every batch ends in an s_waitcnt that exposes a full LDS round trip to the lone wave
#pragma unroll
    for (int I = 0; I < NB; ++I) {
        x0[I] = *reinterpret_cast<const double*>(cbuf + I * (16 * TS * 8) + rd0);
        x1[I] = *reinterpret_cast<const double*>(cbuf + I * (16 * TS * 8) + rd1);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int I = 0; I < NB; ++I) {
        x0[I] = a[I] - x0[I];
        x1[I] = a[I] - x1[I];
    }
}
template <int NB, int NF, bool SPLIT = false>
__device__ __forceinline__ void lse_math2(double (&x0)[NB], double (&x1)[NB], const double (&c)[NB],
                                          double (&acc)[NF][NB], double w0, double w1, double& m2_0, double& m2_1,
                                          double (&s0)[NF], double (&s1)[NF]) {
    double m0 = tree_max<NB>(x0), m1 = tree_max<NB>(x1);
    row16_max2(m0, m1);
    m2_0 = m0 * LOG2E_S;
    m2_1 = m1 * LOG2E_S;
#pragma unroll
    for (int I = 0; I < NB; ++I) {
        x0[I] = fma(x0[I], LOG2E_S, -m2_0);
        x1[I] = fma(x1[I], LOG2E_S, -m2_1);
    }
    if constexpr (SPLIT) {  // (register budget of two waves per SIMD: half the look-ups in flight at a time)
        exp2s_batch<NB>(x0);
        exp2s_batch<NB>(x1);
    } else {
        exp2s_batch2<NB>(x0, x1);
    }
    // Second candidate: e'_k = e_k c_k.  Only its sum needs the products (an FMA dot instead of NB multiplies + a
    // tree of adds); the per-state accumulator takes the UNSCALED e_k r' and the constant c_k is applied once to
    // the reduced sums on the host (mbar_eval.cpp: eval_core).
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        s0[f] = f == 0 ? tree_sum<NB>(x0) : dot_sum<NB>(x0, c);
        s1[f] = f == 0 ? tree_sum<NB>(x1) : dot_sum<NB>(x1, c);
        row16_sum2(s0[f], s1[f]);
        const double r0 = w0 * recip_fast(s0[f]), r1 = w1 * recip_fast(s1[f]);  // w: sample multiplicity (0 on padding)
#pragma unroll
        for (int I = 0; I < NB; ++I) acc[f][I] = fma(x1[I], r1, fma(x0[I], r0, acc[f][I]));
    }
}
template <int NB, int NF>
__device__ __forceinline__ void lse_two_groups(const char* cbuf, int rd0, int rd1,
                                               const double (&a)[NB], const double (&c)[NB], double (&acc)[NF][NB],
                                               double w0, double w1, double& m2_0, double& m2_1,
                                               double (&s0)[NF], double (&s1)[NF]) {
    double x0[NB], x1[NB];
    lse_load2<NB>(cbuf, rd0, rd1, a, x0, x1);
    lse_math2<NB, NF>(x0, x1, c, acc, w0, w1, m2_0, m2_1, s0, s1);
}

// Single-group versions for wide panels (NB > 8), where two groups in the exp pipeline at once would spill registers.
template <int NB>
__device__ __forceinline__ void lse_load1(const char* cbuf, int rd0, const double (&a)[NB], double (&x0)[NB]) {
#pragma unroll
    for (int I = 0; I < NB; ++I) x0[I] = *reinterpret_cast<const double*>(cbuf + I * (16 * TS * 8) + rd0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int I = 0; I < NB; ++I) x0[I] = a[I] - x0[I];
}
template <int NB, int NF>
__device__ __forceinline__ void lse_math1(double (&x0)[NB], const double (&c)[NB], double (&acc)[NF][NB], double w0,
                                          double& m2_0, double (&s0)[NF]) {
    m2_0 = row16_max(tree_max<NB>(x0)) * LOG2E_S;
#pragma unroll
    for (int I = 0; I < NB; ++I) x0[I] = fma(x0[I], LOG2E_S, -m2_0);
    exp2s_batch<NB>(x0);
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        s0[f] = row16_sum(f == 0 ? tree_sum<NB>(x0) : dot_sum<NB>(x0, c));
        const double r0 = w0 * recip_fast(s0[f]);
#pragma unroll
        for (int I = 0; I < NB; ++I) acc[f][I] = fma(x0[I], r0, acc[f][I]);
    }
}
template <int NB, int NF>
__device__ __forceinline__ void lse_one_group(const char* cbuf, int rd0, const double (&a)[NB],
                                              const double (&c)[NB], double (&acc)[NF][NB], double w0, double& m2_0,
                                              double (&s0)[NF]) {
    double x0[NB];
    lse_load1<NB>(cbuf, rd0, a, x0);
    lse_math1<NB, NF>(x0, c, acc, w0, m2_0, s0);
}
// Two consecutive groups g, g+1 of a tile; (mm, ss[]) capture the (shift, sums) of the sample this lane will write.
template <int NB, int NF>
__device__ __forceinline__ void lse_group_pair(const char* cbuf, const char* wslot, int rd_base,
                                               const int (&pos)[GROUPS], int g, const double (&a)[NB],
                                               const double (&c)[NB], double (&acc)[NF][NB], int ks, int ns,
                                               double& mm, double (&ss)[NF]) {
    double m2a, m2b, sa[NF], sb[NF];
    // per-sample multiplicities (1 for plain data, bootstrap counts otherwise, 0 on the padding) from the tile's slot
    const double va = *reinterpret_cast<const double*>(wslot + (4 * g + ns) * 8);
    const double vb = *reinterpret_cast<const double*>(wslot + (4 * (g + 1) + ns) * 8);
    if constexpr (NB <= 8) {
        lse_two_groups<NB, NF>(cbuf, rd_base + pos[g], rd_base + pos[g + 1], a, c, acc, va, vb, m2a, m2b, sa, sb);
    } else {
        lse_one_group<NB, NF>(cbuf, rd_base + pos[g], a, c, acc, va, m2a, sa);
        lse_one_group<NB, NF>(cbuf, rd_base + pos[g + 1], a, c, acc, vb, m2b, sb);
    }
    if ((ks & 3) == g) {
        mm = m2a;
#pragma unroll
        for (int f = 0; f < NF; ++f) ss[f] = sa[f];
    }
    if ((ks & 3) == g + 1) {
        mm = m2b;
#pragma unroll
        for (int f = 0; f < NF; ++f) ss[f] = sb[f];
    }
}

// Stage one wave tile (ROWS state rows x 16 samples starting at column n0) into `dst`.
// DMA instruction j fills LDS bytes [1024 j, 1024 j + 1024): lane l -> row 8j + (l >> 3),
// positions 2(l & 7), 2(l & 7)+1 of that row, which hold samples (pos - (row & 14)) & 15.
// The per-lane part of the source address depends on j only through its parity (row & 14 = ((l >> 3) & 6) |
// 8 (j & 1)), so it is two loop-invariant 32-bit byte offsets (StageOffsets) added to a wave-uniform base:
// the DMA is issued as `global_load_lds_dwordx4 voff, s[base]` with no per-instruction VALU address math.
// rowmap(tile_row) gives the global row (8-row groups never straddle a panel).
// WIDE: the row pitch is so large (N_local >= 7.6e7) that 7 ld 8 + 120 does not fit 32 bits; the lane offsets are then
// 64-bit and every DMA pays one 64-bit VALU add (own kernel instantiations, selected by the launchers).
template <bool WIDE>
struct StageOffsetsT {
    typedef typename std::conditional<WIDE, uint64_t, uint32_t>::type off_t;
    off_t off[2];
};
typedef StageOffsetsT<false> StageOffsets;
template <bool WIDE = false>
__device__ __forceinline__ StageOffsetsT<WIDE> make_stage_offsets(int64_t ld, int lane) {
    StageOffsetsT<WIDE> so;
    const int r = lane >> 3, pos = 2 * (lane & 7);
#pragma unroll
    for (int par = 0; par < 2; ++par) {
        const int smp = (pos - ((r & 6) | (par << 3))) & 15;
        so.off[par] = (typename StageOffsetsT<WIDE>::off_t)(((int64_t)r * ld + smp) * 8);
    }
    return so;
}
// cache-policy bits of the tile loads (aux operand of global_load_lds: 1 = sc0, 2 = nt, 16 = sc1): the default policy measured
// best (profiles/r3_ab_streaming_hints.txt)
#ifndef MBAR_DMA_AUX
#define MBAR_DMA_AUX 0
#endif
template <bool DMA>
__device__ __forceinline__ void stage_piece(const double* __restrict__ ubase /*wave-uniform*/, uint64_t voff,
                                            char* dst /*wave-uniform*/, int lane) {
    const char* src = reinterpret_cast<const char*>(ubase) + voff;
    if constexpr (DMA) {
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)dst, 16, 0, MBAR_DMA_AUX);
    } else {
        *reinterpret_cast<double2*>(dst + lane * 16) = *reinterpret_cast<const double2*>(src);
    }
}
template <bool DMA>
__device__ __forceinline__ void stage_piece(const double* __restrict__ ubase /*wave-uniform*/, uint32_t voff,
                                            char* dst /*wave-uniform*/, int lane) {
    // Launder the base through an SGPR constraint: loop strength reduction otherwise turns every DMA address of
    // the tile loop into its own 64-bit per-lane induction variable (2 VGPRs + a 64-bit VALU add per instruction
    // per tile) and the instruction loses its scalar-base form.
    // The 32-bit lane offset is laundered too, so that its zero-extension stays in the block of the DMA (instruction
    // selection is per basic block and only matches base + zext(offset) when it sees both).
    uint64_t ub = reinterpret_cast<uint64_t>(ubase);
    asm("" : "+s"(ub));
    asm("" : "+v"(voff));
    const char* src = reinterpret_cast<const char*>(ub) + voff;
    if constexpr (DMA) {
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                         (__attribute__((address_space(3))) void*)dst, 16, 0, MBAR_DMA_AUX);
    } else {
        *reinterpret_cast<double2*>(dst + lane * 16) = *reinterpret_cast<const double2*>(src);
    }
}
template <int ROWS, bool DMA, int J0, int JSTEP, typename RowMap, typename SO>
__device__ __forceinline__ void stage_tile(const double* __restrict__ u, int64_t ld, int64_t n0, char* dst, int lane,
                                           const SO& so, RowMap rowmap) {
    constexpr int NDMA = ROWS / 8;
#pragma unroll
    for (int j = J0; j < NDMA; j += JSTEP)
        stage_piece<DMA>(u + rowmap(8 * j) * ld + rowmap.cols(j, n0), so.off[j & 1], dst + j * 1024, lane);
}

// Stage the 16 per-sample values v[n0 .. n0+16) (128 bytes) behind a tile: lanes 0..7 move 16 bytes each.
// Going through LDS-DMA (instead of an ordinary VGPR load) keeps hipcc from draining the whole DMA
// prefetch with an s_waitcnt vmcnt(0) at the first use of the loaded register.
template <bool DMA>
__device__ __forceinline__ void stage_vec16(const double* __restrict__ v, int64_t n0, char* dst, int lane) {
    if (lane < 8) stage_piece<DMA>(v + n0, (uint32_t)(lane * 16), dst, lane);
}

// Pin a loaded value into its register *now*: the compiler must place the s_waitcnt for the load here
// (before any DMA is in flight) instead of a conservative vmcnt(0) at the first use inside the loop.
__device__ __forceinline__ void settle(double& x) { asm volatile("" : "+v"(x)); }

// A global load the compiler does not know to be one: issued AHEAD of LDS-DMA requests whose number depends on control flow,
// its result would otherwise be waited for with a conservative s_waitcnt vmcnt(0) -- i.e. for the tile behind it as well.  The
// caller waits by hand (wait_vm_for: vmcnt(N) with N <= the requests issued after these loads) before the first use.  Only
// safe for loads issued before every compiler-tracked memory operation of the kernel (the counter retires in order).
__device__ __forceinline__ double load_untracked(const double* p) {
    double v;
    asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(v) : "v"(p) : "memory");
    return v;
}
template <int N>
__device__ __forceinline__ void wait_vm_for(double& a, double& b, double& c, double& d, double& e, double (&r)[16]) {
    asm volatile("s_waitcnt vmcnt(%21)"
                 : "+v"(a), "+v"(b), "+v"(c), "+v"(d), "+v"(e), "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]),
                   "+v"(r[6]), "+v"(r[7]), "+v"(r[8]), "+v"(r[9]), "+v"(r[10]), "+v"(r[11]), "+v"(r[12]), "+v"(r[13]), "+v"(r[14]), "+v"(r[15])
                 : "n"(N)
                 : "memory");
}
// Workgroup barrier for LDS traffic only: __syncthreads() carries a release fence that also waits for every outstanding global
// request (vmcnt(0)) -- i.e. for LDS-DMA tiles in flight that the code between two such barriers has no business waiting for.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
template <int N>
__device__ __forceinline__ void wait_vm() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// `live`: bit j set = the 8 rows of DMA piece j matter.  A piece whose rows all carry a per-state constant that makes their
// terms exactly zero (exp(-inf - u): padding rows of the device matrix, states without samples) is requested from the FIRST tile's
// columns instead of the current tile's: the same 1 KB every time (an L2 hit instead of HBM traffic), the same instruction
// stream, the same LDS layout, and whatever lands there is multiplied by zero like the real rows would have been.
struct RowIdentity {
    int64_t row0;
    uint32_t live = 0xffffffffu;
    __device__ __forceinline__ int64_t operator()(int tr) const { return row0 + tr; }
    __device__ __forceinline__ int64_t cols(int j, int64_t n0) const { return ((live >> j) & 1u) ? n0 : 0; }
};
struct RowTwoPanels {
    int64_t row_i0, row_j0;
    int split;
    uint32_t live = 0xffffffffu;
    __device__ __forceinline__ int64_t operator()(int tr) const {
        return tr < split ? row_i0 + tr : row_j0 + (tr - split);
    }
    __device__ __forceinline__ int64_t cols(int j, int64_t n0) const { return ((live >> j) & 1u) ? n0 : 0; }
};
// Live mask of a panel's DMA pieces from the per-state constants of its rows in the Gram / evaluation layout (lane & 15 = state
// within block I): piece 2 I + h is dead when its 8 constants all equal `dead` (-inf exponent constants, zero multipliers).
template <int NB>
__device__ __forceinline__ uint32_t live_piece_mask(const double (&a)[NB], double dead) {
    uint32_t m = 0;
#pragma unroll
    for (int I = 0; I < NB; ++I) {
        const unsigned long long b = __ballot(a[I] != dead);
        m |= ((b & 0xffull) ? 1u : 0u) << (2 * I);
        m |= ((b & 0xff00ull) ? 1u : 0u) << (2 * I + 1);
    }
    return m;
}

// ---- constants shared by several kernel families --------------------------------------------------------------------
constexpr int lse_waves(int nb) { return nb <= 2 ? 16 : (nb <= 4 ? 8 : (nb <= 8 ? 4 : 2)); }
constexpr int TSS = 64;  // samples per tile of the small-K kernel
constexpr int GRAM_AGPR_BLOCKS = 31;
// Finite stand-ins for the infinities of the operand exponent when the sweep runs without the exponential's clamp
constexpr double GRAM_NEG_HUGE = -2.9e303, LOGDEN_HUGE = 1e300;
constexpr int FUSED_PSUM1_FROM_GRAM_NB = 8;

static inline int blocks_per_cu_for(size_t lds_bytes) {
    int b = (int)((160 * 1024) / lds_bytes);
    if (b < 1) b = 1;
    if (b > 4) b = 4;
    return b;
}

static inline bool stage_offsets_wide(int64_t ld) { return (uint64_t)ld * 56u + 128u >= (1ull << 32); }

// (defined in mbar_k_quad.hip; launch_fused in mbar_k_fused.hip hands 129 .. 256 states to it)
hipError_t launch_fused_quad(hipStream_t s, int nbt, const LaunchGeom& g, const double* P, int64_t ld, int64_t N, const double* cmul,
                             const double* cw, const double* wsq, double* rinv0, double* gp, double* pp, const LoopCtl& lc);

}  // namespace mbar
#endif  // MBAR_SWEEP_DEVICE_H
