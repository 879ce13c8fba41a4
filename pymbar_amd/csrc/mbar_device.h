// gfx950 (CDNA4 / MI355X) kernels of libmbar_hip.so: the device-side helpers every kernel translation unit (mbar_k_*.hip) shares --
// wave and DPP primitives, the table-driven exp / log and the fast reciprocal, in-lane trees.  What only the solver's sweep kernels
// use (tile staging, the log-sum-exp groups, their constants) is in mbar_sweep_device.h, the chain of the scan and family-fill
// kernels in mbar_scan_device.h.
#ifndef MBAR_DEVICE_H
#define MBAR_DEVICE_H
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace mbar {

typedef double v4d __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------
// small device helpers
// ---------------------------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ double dpp_move(double x) {
    int lo = __double2loint(x), hi = __double2hiint(x);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xF, 0xF, true);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xF, 0xF, true);
    return __hiloint2double(hi, lo);
}
// All-reduce over the 16 lanes of a DPP row (= the 16 states a sample has in one register):
// quad_perm xor 1, quad_perm xor 2, row_half_mirror, row_mirror.
__device__ __forceinline__ double row16_max(double x) {
    x = fmax(x, dpp_move<0xB1>(x));
    x = fmax(x, dpp_move<0x4E>(x));
    x = fmax(x, dpp_move<0x141>(x));
    x = fmax(x, dpp_move<0x140>(x));
    return x;
}
// Lane N of every 16-lane row to all lanes of that row (gfx90a+: the one DPP control 64-bit moves accept).
template <int N>
__device__ __forceinline__ double row16_bcast(double x) {
    double r;
    asm("v_mov_b64_dpp %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "=v"(r) : "v"(x), "n"(N));
    return r;
}
// acc += x * (lane N of r's 16-lane row): the broadcast rides in the fused multiply-add's own DPP operand -- the same operation, and
// the same bits, as fma(x, row16_bcast<N>(r), acc) without the move.  (As with every DPP read the compiler cannot see: r must have
// been written at least two wait states earlier.)
template <int N>
__device__ __forceinline__ void fmac_row16_bcast(double& acc, double r, double x) {
    asm("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(r), "v"(x), "n"(N));
}
__device__ __forceinline__ double row16_sum(double x) {
    x += dpp_move<0xB1>(x);
    x += dpp_move<0x4E>(x);
    x += dpp_move<0x141>(x);
    x += dpp_move<0x140>(x);
    return x;
}
// The value of lane (l ^ M): across the 16-lane rows through the LDS crossbar (ds_bpermute), inside a row by DPP -- row_ror:8,
// two bank-masked row shifts by 4, the quad permutes -- whose latency is an instruction's, not a round trip's.  A butterfly
// built from it adds the same pairs in the same order as one built from __shfl_xor.
template <int M>
__device__ __forceinline__ double lane_xor(double x) {
    if constexpr (M >= 16) {
        return __shfl_xor(x, M);
    } else if constexpr (M == 8) {
        return dpp_move<0x128>(x);
    } else if constexpr (M == 4) {
        int lo = __double2loint(x), hi = __double2hiint(x);
        int tl = __builtin_amdgcn_update_dpp(lo, lo, 0x104, 0xF, 0x5, false);  // quads 0, 2: lane l + 4 (row_shl:4)
        tl = __builtin_amdgcn_update_dpp(tl, lo, 0x114, 0xF, 0xA, false);      // quads 1, 3: lane l - 4 (row_shr:4)
        int th = __builtin_amdgcn_update_dpp(hi, hi, 0x104, 0xF, 0x5, false);
        th = __builtin_amdgcn_update_dpp(th, hi, 0x114, 0xF, 0xA, false);
        return __hiloint2double(th, tl);
    } else if constexpr (M == 2) {
        return dpp_move<0x4E>(x);
    } else {
        return dpp_move<0xB1>(x);
    }
}
__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m);
    return x;
}
__device__ __forceinline__ double wave_max(double x) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) x = fmax(x, __shfl_xor(x, m));
    return x;
}
// fixed-order sums / maxima over a workgroup of 256 threads
__device__ __forceinline__ double block256_sum(double v, double* red /*[4]*/) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
__device__ __forceinline__ double block256_max(double v, double* red /*[4]*/) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

// exp built for instruction count (gfx950 issues one fp64 VALU op per ~5.6 cycles per SIMD and fp64 MFMA does
// not overlap with VALU -- profiles/r1_*microbench.txt -- so every fp64 instruction here is kernel time).
// 2^(t/S) for t = S x log2(e), S = 2^EXP2_BITS = 2048:   s = rint(max(t, EXP2_CLAMP));  z = t - s in [-1/2, 1/2];
//   j = s & (S-1), q = s >> EXP2_BITS;   result = ldexp(T[j] * P(z), q),  T[j] = 2^(j/S) from a 16 KB LDS table at
//   LDS offset 0, P = degree-3 polynomial of 2^(z/S) (error 9e-18; tools/gen_exp2_table.py).  Nine fp64 + three
//   integer instructions (the library exp needs ~25).  Relative error of the whole function <= 3.1 x 2^-53 (1.55 ulp: half an ulp
//   each from the table entry, the last fma of the polynomial and the product; measured 2.82 x 2^-53); results below 2^-1022 are NOT
//   flushed: v_ldexp_f64 rounds them once, to nearest-even, into the subnormal range.  The table entries (correctly rounded), the
//   polynomial's 9e-18 and the 3.1 x 2^-53 are asserted by tests/test_device_math_tables.py against a step-by-step model of this
//   function; tests/test_gpu_device_math.py asserts that the device returns the model's bits.
//   exp(-inf) = 0 through the clamp, overflow gives inf through
//   ldexp; NaN arguments are laundered to 0 by the clamp, which is why NaN / -inf entries of u_kn and non-finite f_k
//   are detected at the boundary instead (mbar_eval.cpp).
#include "exp2_table.inc"
#include "log_table.inc"
constexpr double LOG2E = 0x1.71547652b82fep+0, LN2 = 0x1.62e42fefa39efp-1;
constexpr double EXP2_S = (double)(1 << EXP2_BITS);
constexpr double LOG2E_S = EXP2_S * LOG2E, LN2_OVER_S = LN2 / EXP2_S;
constexpr double EXP2_CLAMP = -1100.0 * EXP2_S;
constexpr int EXP2_TABLE_BYTES = (1 << EXP2_BITS) * 8;
constexpr int LOG_TABLE_BYTES = 256 * 8;
constexpr int EXP_TABLE_BYTES = EXP2_TABLE_BYTES + LOG_TABLE_BYTES;  // LDS reserved for both look-up tables
constexpr int EXP_TABLE_DMA_PER_WAVE = (EXP_TABLE_BYTES / 1024 + 7) / 8;  // requests per wave of exp_table_init_dma in an 8-wave workgroup
typedef __attribute__((address_space(3))) const double lds_cdouble;
// Every thread block copies the table to LDS offset 0 (its dynamic LDS starts there: the kernels have no static
// __shared__), so a look-up address is just the masked integer -- no base add.  Callers barrier afterwards.
__device__ __forceinline__ void exp_table_init(char* smem) {
    if ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem != 0u) __builtin_trap();
    for (int i = threadIdx.x; i < (1 << EXP2_BITS); i += blockDim.x) reinterpret_cast<double*>(smem)[i] = EXP2_TABLE[i];
    for (int i = threadIdx.x; i < 256; i += blockDim.x)
        reinterpret_cast<double*>(smem + EXP2_TABLE_BYTES)[i] = LOG_TABLE[i];
}
// The same copy as LDS-DMA requests (1 KB per instruction, 18 in all, shared out over the waves): asynchronous, nothing passes
// through registers, and -- issued BEFORE a kernel's first tile request -- it does not queue behind it.  The caller waits for
// its own requests (s_waitcnt vmcnt(0)) and passes a workgroup barrier before the first look-up.
__device__ __forceinline__ void exp_table_init_dma(char* smem) {
    if ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) char*)smem != 0u) __builtin_trap();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), nwv = blockDim.x >> 6;
    constexpr int NCH = EXP_TABLE_BYTES / 1024, NCH_EXP = EXP2_TABLE_BYTES / 1024;
    // (every wave issues the same number of requests, EXP_TABLE_DMA_PER_WAVE for eight waves -- a chunk requested twice lands
    // twice with the same bytes -- so that a caller can count them in an s_waitcnt)
    const int per_wave = (NCH + nwv - 1) / nwv;
    for (int i = 0; i < per_wave; ++i) {
        const int c = (wave + i * nwv) % NCH;
        const char* src = c < NCH_EXP ? reinterpret_cast<const char*>(EXP2_TABLE) + c * 1024
                                      : reinterpret_cast<const char*>(LOG_TABLE) + (c - NCH_EXP) * 1024;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + lane * 16),
                                         (__attribute__((address_space(3))) void*)(smem + c * 1024), 16, 0, 0);
    }
}
__device__ __forceinline__ double exp2_table_at(int si) {
    return *(lds_cdouble*)(uintptr_t)(uint32_t)((si << 3) & (EXP2_TABLE_BYTES - 8));
}
__device__ __forceinline__ double exp2_poly(double z) {
    double p = EXP2_POLY[EXP2_DEG];
#pragma unroll
    for (int k = EXP2_DEG - 1; k >= 0; --k) p = fma(p, z, EXP2_POLY[k]);
    return p;
}
__device__ __forceinline__ double exp2s_fast(double ts) {  // 2^(ts / S)
    const double t = fmax(ts, EXP2_CLAMP);
    const double s = __builtin_rint(t);
    const double z = t - s;
    const int si = (int)s;
    const double T = exp2_table_at(si);
    return ldexp(T * exp2_poly(z), si >> EXP2_BITS);
}
// log s for positive finite s (the per-sample sums of the evaluation sweep), 12 fp64 + 2 integer instructions
// (the library log is ~50 and keeps a dozen constants in registers):  s = 2^e m, m in [1/2, 1); the top 7 mantissa
// bits pick c_j with |m / c_j - 1| <= 2^-8 from the 2 KB LDS table behind the exp table (tools/gen_log_table.py);
// log s = e ln2 + log c_j + log1p(r), r = m / c_j - 1, log1p by its degree-6 Taylor polynomial (absolute error 2e-18).
// Absolute error <= (1.6 + |e| / 2) x 2^-53 + one ulp of the result: ~2e-16 (measured 1.8 x 2^-53) for s in [1, 2), but the two half
// ulps of the result -- fma(e, LN2, log c_j) and the closing fma, which hipcc contracts from "+ q * r" -- dominate from s = 4 on
// (1.1e-15 = 10 x 2^-53 at s = 1000).  log_pos(1) is 4.3e-17, not 0 (1 = 2^1 x 1/2 goes through bucket 0).  The table pairs, the
// 2e-18 and the bound are asserted by tests/test_device_math_tables.py; the device's bits by tests/test_gpu_device_math.py.
// s = 0 / negative are not supported.
typedef double v2d __attribute__((ext_vector_type(2)));
__device__ __forceinline__ double log_pos(double s) {
    const double m = __builtin_amdgcn_frexp_mant(s);
    const double ed = (double)__builtin_amdgcn_frexp_exp(s);
    const uint32_t off = (uint32_t)(__double2hiint(m) >> 9) & 0x7f0u;
    const v2d tc = *(__attribute__((address_space(3))) const v2d*)(uintptr_t)(uint32_t)(EXP2_TABLE_BYTES + off);
    const double r = fma(m, tc.x, -1.0);
    double q = -1.0 / 6.0;
    q = fma(q, r, 0.2);
    q = fma(q, r, -0.25);
    q = fma(q, r, 1.0 / 3.0);
    q = fma(q, r, -0.5);
    q = fma(q, r, 1.0);
    return fma(ed, LN2, tc.y) + q * r;
}
// The same exp for N independent arguments, written as three stages separated by scheduling barriers: with one
// or two waves per SIMD nothing else hides the LDS latency of the table look-up, and hipcc's own schedule leaves
// only a handful of instructions between each ds_read and its use.  Stage 1 issues all N table reads, stage 2 (the
// polynomials) runs while they are in flight, stage 3 combines.  x[] in: ts, out: 2^(ts/S).
// CLAMP = false: the arguments are known to be finite (callers substitute finite sentinels for their -inf cases and the
// matrix holds no +inf): one v_max_f64 per element less.  Finite arguments of any size are safe without the clamp --
// v_cvt_i32_f64 saturates, so a hugely negative argument ends in ldexp(..., -2^20) = 0.
template <int N, bool CLAMP = true>
__device__ __forceinline__ void exp2s_batch(double (&x)[N]) {
    double T[N];
    int q[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const double t = CLAMP ? fmax(x[i], EXP2_CLAMP) : x[i];
        const double s = __builtin_rint(t);
        x[i] = t - s;
        const int si = (int)s;
        q[i] = si >> EXP2_BITS;
        T[i] = exp2_table_at(si);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < N; ++i) x[i] = exp2_poly(x[i]);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < N; ++i) x[i] = ldexp(T[i] * x[i], q[i]);
}
template <int N>
__device__ __forceinline__ void exp2s_batch2(double (&x0)[N], double (&x1)[N]) {  // two argument sets, one pipeline
    double T0[N], T1[N];
    int q0[N], q1[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const double t0 = fmax(x0[i], EXP2_CLAMP), t1 = fmax(x1[i], EXP2_CLAMP);
        const double s0 = __builtin_rint(t0), s1 = __builtin_rint(t1);
        x0[i] = t0 - s0;
        x1[i] = t1 - s1;
        const int i0 = (int)s0, i1 = (int)s1;
        q0[i] = i0 >> EXP2_BITS;
        q1[i] = i1 >> EXP2_BITS;
        T0[i] = exp2_table_at(i0);
        T1[i] = exp2_table_at(i1);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        x0[i] = exp2_poly(x0[i]);
        x1[i] = exp2_poly(x1[i]);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        x0[i] = ldexp(T0[i] * x0[i], q0[i]);
        x1[i] = ldexp(T1[i] * x1[i], q1[i]);
    }
}
// 2^(-w/S) for w >= 0 (round 6; the build sweep's exponential, where the argument is "column maximum minus entry" and can
// be formed non-negative EXACTLY): floor and fraction come straight from the argument -- n = -trunc(w) (one conversion with a
// negated source), z = fract(w) in [0, 1) (one instruction) -- instead of rint / subtract / convert, and no clamp is needed below:
//   2^(-w/S) = 2^(n/S) 2^(-z/S) = ldexp(T[n & (S-1)] * Q(z), n >> EXP2_BITS),  Q = degree-3 polynomial of 2^(-z/S) on [0, 1]
// (error 8.8e-18; generated by tools/gen_exp2n_poly.py, which reproduces the four coefficients below bit for bit; the 8.8e-18 and
// the function's relative error <= 3.1 x 2^-53, measured 2.49 x 2^-53, are asserted by tests/test_device_math_tables.py).
// Eight fp64 + three integer instructions (exp2s_batch: nine + three, + the clamp).  Huge
// finite w is safe (v_cvt_i32_f64 saturates, ldexp(.., -2^20) = 0); CLAMP = true also takes w = +inf (matrices with +inf entries).
constexpr double EXP2N_POLY[4] = {1.0, -0x1.62e42fefa3028p-12, 0x1.ebfbdf9648000p-25, -0x1.c69cea0000000p-38};
template <int N, bool CLAMP>
__device__ __forceinline__ void exp2s_neg_batch(double (&w)[N]) {
    double T[N];
    int q[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const double t = CLAMP ? fmin(w[i], 2.0e9) : w[i];
        const int ni = (int)(-t);
        w[i] = __builtin_amdgcn_fract(t);
        q[i] = ni >> EXP2_BITS;
        T[i] = exp2_table_at(ni);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double p = EXP2N_POLY[3];
        p = fma(p, w[i], EXP2N_POLY[2]);
        p = fma(p, w[i], EXP2N_POLY[1]);
        w[i] = fma(p, w[i], EXP2N_POLY[0]);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < N; ++i) w[i] = ldexp(T[i] * w[i], q[i]);
}
template <int N, bool CLAMP>
__device__ __forceinline__ void exp2s_neg_batch2(double (&w0)[N], double (&w1)[N]) {  // two argument sets, one pipeline
    double T0[N], T1[N];
    int q0[N], q1[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const double t0 = CLAMP ? fmin(w0[i], 2.0e9) : w0[i], t1 = CLAMP ? fmin(w1[i], 2.0e9) : w1[i];
        const int n0 = (int)(-t0), n1 = (int)(-t1);
        w0[i] = __builtin_amdgcn_fract(t0);
        w1[i] = __builtin_amdgcn_fract(t1);
        q0[i] = n0 >> EXP2_BITS;
        q1[i] = n1 >> EXP2_BITS;
        T0[i] = exp2_table_at(n0);
        T1[i] = exp2_table_at(n1);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        double p0 = EXP2N_POLY[3], p1 = EXP2N_POLY[3];
        p0 = fma(p0, w0[i], EXP2N_POLY[2]);
        p1 = fma(p1, w1[i], EXP2N_POLY[2]);
        p0 = fma(p0, w0[i], EXP2N_POLY[1]);
        p1 = fma(p1, w1[i], EXP2N_POLY[1]);
        w0[i] = fma(p0, w0[i], EXP2N_POLY[0]);
        w1[i] = fma(p1, w1[i], EXP2N_POLY[0]);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        w0[i] = ldexp(T0[i] * w0[i], q0[i]);
        w1[i] = ldexp(T1[i] * w1[i], q1[i]);
    }
}
// 1 / s for s > 0: hardware estimate + two Newton steps (the divide expansion costs twice as many instructions).  Measured, not
// proved: from the correctly rounded seed and from a seed 2^-20 off the model ends within 0.5000 ulp and at the same bits on 71 000
// arguments (tests/test_device_math_tables.py); the device's P equals the model's bits on every probe entry (tests/test_gpu_device_math.py)
__device__ __forceinline__ double recip_fast(double s) {
    double r = __builtin_amdgcn_rcp(s);
    r = fma(fma(-s, r, 1.0), r, r);
    r = fma(fma(-s, r, 1.0), r, r);
    return r;
}

// In-lane reductions over the NB registers of a sample as a pairwise tree (dependent depth log2 NB instead of NB:
// with one or two waves per SIMD the chain latency of fp64 ops is exposed).
template <int NB>
__device__ __forceinline__ double tree_max(const double (&x)[NB]) {
    double t[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) t[i] = x[i];
#pragma unroll
    for (int n = NB; n > 1; n -= n / 2) {
#pragma unroll
        for (int i = 0; i < n / 2; ++i) t[i] = fmax(t[i], t[n - 1 - i]);
    }
    return t[0];
}
template <int NB>
__device__ __forceinline__ double tree_sum(const double (&x)[NB]) {
    double t[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) t[i] = x[i];
#pragma unroll
    for (int n = NB; n > 1; n -= n / 2) {
#pragma unroll
        for (int i = 0; i < n / 2; ++i) t[i] += t[n - 1 - i];
    }
    return t[0];
}
// sum_i x_i c_i as two interleaved FMA chains (NB + 1 instructions; a product array + tree_sum takes 2 NB - 1)
template <int NB>
__device__ __forceinline__ double dot_sum(const double (&x)[NB], const double (&c)[NB]) {
    if constexpr (NB == 1) {
        return x[0] * c[0];
    } else {
        double e = x[0] * c[0], o = x[1] * c[1];
#pragma unroll
        for (int i = 2; i + 1 < NB; i += 2) {
            e = fma(x[i], c[i], e);
            o = fma(x[i + 1], c[i + 1], o);
        }
        if constexpr (NB & 1) e = fma(x[NB - 1], c[NB - 1], e);
        return e + o;
    }
}
// 16-lane all-reduce of two independent values at once (the two dependency chains interleave)
__device__ __forceinline__ void row16_max2(double& a, double& b) {
    a = fmax(a, dpp_move<0xB1>(a));   b = fmax(b, dpp_move<0xB1>(b));
    a = fmax(a, dpp_move<0x4E>(a));   b = fmax(b, dpp_move<0x4E>(b));
    a = fmax(a, dpp_move<0x141>(a));  b = fmax(b, dpp_move<0x141>(b));
    a = fmax(a, dpp_move<0x140>(a));  b = fmax(b, dpp_move<0x140>(b));
}
__device__ __forceinline__ void row16_sum2(double& a, double& b) {
    a += dpp_move<0xB1>(a);   b += dpp_move<0xB1>(b);
    a += dpp_move<0x4E>(a);   b += dpp_move<0x4E>(b);
    a += dpp_move<0x141>(a);  b += dpp_move<0x141>(b);
    a += dpp_move<0x140>(a);  b += dpp_move<0x140>(b);
}

}  // namespace mbar
#endif  // MBAR_DEVICE_H
