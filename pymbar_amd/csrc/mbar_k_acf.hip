// gfx950 (CDNA4 / MI355X) kernels of the lagged fluctuation sums behind pymbar_amd.timeseries (statistical inefficiency,
// equilibration detection, correlation functions).  One of the translation units of libmbar_hip.so: launchers declared in
// mbar_acf.h, C ABI in mbar_acf.cpp, design and numbers in DESIGN.md ("Timeseries").
//
// The series is held shifted by one constant per series (A' = A - m_A, B' = B - m_B), padded with zeros to the pitch ldx (a
// multiple of ACF_TILE, > T), with rem[n] = the positions left in n's segment (the partner n + t is valid iff t < rem[n]).  For a
// block of lags, lag-major:
//   k_acf_tiles   one wave per tile of ACF_TILE positions: the sum of the tile's products A'_n B'_n+t for every lag
//   k_acf_scan    one workgroup per lag: off[tile] = sum over the later tiles, in a fixed order
//   k_acf_rule    the tiles that hold running origins: an in-tile suffix scan gives Q_t(s) = sum_{n >= s} A'_n B'_n+t at every
//                 position, the suffix means enter through the suffix sums SA / SB of A' / B',
//                     X_s(t) = Q_t(s) - d_B sum_{[s, T-t)} A' - d_A sum_{[s+t, T)} B' + (N - t) d_A d_B,
//                 and one thread per origin runs the reference's stopping rule over the block's lags in order
//   k_acf_store   the same suffix sums, stored at requested positions (raw lag sums, and SA / SB themselves)
// Every sum is double-double: TwoProduct (fma) and TwoSum inside a thread, full double-double additions across threads and
// tiles, so that the expansion of X stays exact where an origin's mean lies many sigma from the shift.  No atomics; every
// reduction has a fixed order, so two identical calls return identical bits.
#include "mbar_device.h"
#include "mbar_acf.h"

#pragma clang fp contract(off)

namespace mbar {

namespace {
constexpr int ACF_WAVES = ACF_WG / 64;

struct dd {
    double hi, lo;
};

__device__ __forceinline__ dd two_sum(double a, double b) {
    const double s = a + b;
    const double bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}
__device__ __forceinline__ dd fast_two_sum(double a, double b) {
    const double s = a + b;
    return {s, b - (s - a)};
}
__device__ __forceinline__ dd two_prod(double a, double b) {
    const double p = a * b;
    return {p, __fma_rn(a, b, -p)};
}
__device__ __forceinline__ dd dd_add(dd a, dd b) {
    dd s = two_sum(a.hi, b.hi);
    const dd t = two_sum(a.lo, b.lo);
    s.lo += t.hi;
    s = fast_two_sum(s.hi, s.lo);
    s.lo += t.lo;
    return fast_two_sum(s.hi, s.lo);
}
__device__ __forceinline__ dd dd_neg(dd a) { return {-a.hi, -a.lo}; }
__device__ __forceinline__ dd dd_sub(dd a, dd b) { return dd_add(a, dd_neg(b)); }
// product of two double-doubles (the lo x lo term is below the result's last bit)
__device__ __forceinline__ dd dd_mul(dd a, dd b) {
    const dd p = two_prod(a.hi, b.hi);
    return fast_two_sum(p.hi, __fma_rn(a.hi, b.lo, __fma_rn(a.lo, b.hi, p.lo)));
}
__device__ __forceinline__ dd dd_mul_d(dd a, double b) {
    const dd p = two_prod(a.hi, b);
    return fast_two_sum(p.hi, __fma_rn(a.lo, b, p.lo));
}
__device__ __forceinline__ dd ld2(const double2* p, int64_t i) {
    const double2 v = p[i];
    return {v.x, v.y};
}
// quotient of a double-double by a double, as a double-double
__device__ __forceinline__ dd dd_div_d(dd a, double b) {
    const double q = a.hi / b;
    const dd qb = two_prod(q, b);
    const double r = ((a.hi - qb.hi) - qb.lo) + a.lo;
    return fast_two_sum(q, r / b);
}
// product of two values held as hi + lo, unnormalised: TwoProduct of the high parts, the cross terms folded into the error
__device__ __forceinline__ dd dd_prod(dd x, dd y) {
    const dd p = two_prod(x.hi, y.hi);
    return {p.hi, __fma_rn(x.hi, y.lo, __fma_rn(x.lo, y.hi, p.lo))};
}
// compensated accumulation inside a thread (TwoSum on the high parts, plain sum of the errors)
__device__ __forceinline__ void acc_add(dd& acc, dd p) {
    const dd q = two_sum(acc.hi, p.hi);
    acc.hi = q.hi;
    acc.lo += q.lo + p.lo;
}
__device__ __forceinline__ dd shfl_down_dd(dd v, int off) { return {__shfl_down(v.hi, off), __shfl_down(v.lo, off)}; }

// Sum of the values of the threads with a higher index (exclusive suffix) and the workgroup total, in a fixed order.
__device__ dd block_excl_suffix(dd v, dd* lds, dd& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    dd inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const dd o = shfl_down_dd(inc, off);
        if (lane + off < 64) inc = dd_add(inc, o);
    }
    dd ex = shfl_down_dd(inc, 1);
    if (lane == 63) ex = dd{0.0, 0.0};
    if (lane == 0) lds[w] = inc;
    __syncthreads();
    dd later{0.0, 0.0};
    for (int k = ACF_WAVES - 1; k > w; --k) later = dd_add(lds[k], later);
    dd all{0.0, 0.0};
    for (int k = ACF_WAVES - 1; k >= 0; --k) all = dd_add(lds[k], all);
    total = all;
    __syncthreads();
    return dd_add(ex, later);
}

__device__ __forceinline__ int block_sum_int(int v, int* lds) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    int s = 0;
    for (int k = 0; k < ACF_WAVES; ++k) s += lds[k];
    return s;
}

// The R positions of a thread: its A' values (and B' for the cross form) and segment remainders.
template <int KIND>
struct Positions {
    dd x[ACF_R], y[ACF_R];
    int rem[ACF_R];
    __device__ void load(const AcfLaunch& a, int64_t n0) {
#pragma unroll
        for (int r = 0; r < ACF_R; ++r) {
            x[r] = ld2(a.A, n0 + r);
            y[r] = KIND == ACF_CROSS ? ld2(a.B, n0 + r) : dd{0.0, 0.0};
            rem[r] = a.rem[n0 + r];
        }
    }
    // products of lag t: p0 = A'_n B'_n+t (A'_n A'_n+t, A'_n), p1 = B'_n A'_n+t (cross only); zero for invalid pairs
    __device__ void products(const AcfLaunch& a, int64_t n0, int64_t t, dd* p0, dd* p1) const {
#pragma unroll
        for (int r = 0; r < ACF_R; ++r) {
            p0[r] = dd{0.0, 0.0};
            p1[r] = dd{0.0, 0.0};
            if (t < (int64_t)rem[r]) {
                if (KIND == ACF_PLAIN) {
                    p0[r] = x[r];
                } else if (KIND == ACF_AUTO) {
                    p0[r] = dd_prod(x[r], ld2(a.A, n0 + r + t));
                } else {
                    p0[r] = dd_prod(x[r], ld2(a.B, n0 + r + t));
                    p1[r] = dd_prod(y[r], ld2(a.A, n0 + r + t));
                }
            }
        }
    }
};

__device__ __forceinline__ dd thread_total(const dd* p) {
    dd acc{0.0, 0.0};
#pragma unroll
    for (int r = ACF_R - 1; r >= 0; --r) acc_add(acc, p[r]);
    return two_sum(acc.hi, acc.lo);
}

// Tile totals: one wave per tile, lane l taking the positions l, l + 64, l + 128, ... of the tile (every load coalesced), so that
// the cross-lane reduction of a lag is paid once per ACF_TILE / 64 products and needs no barrier.
__device__ __forceinline__ dd wave_total(dd v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = dd_add(v, shfl_down_dd(v, off));
    return v;  // (lane 0)
}

template <int KIND>
__global__ void __launch_bounds__(ACF_WG) k_acf_tiles(AcfLaunch a) {
    const int lane = threadIdx.x & 63;
    const int64_t tile = a.tile_lo + (int64_t)blockIdx.x * ACF_WAVES + (threadIdx.x >> 6);
    if (tile > a.atile_hi) return;  // (wave-uniform)
    const int64_t base = tile * ACF_TILE + lane;
    for (int j = 0; j < a.nl; ++j) {
        const int64_t t = a.lag[j];
        dd acc0{0.0, 0.0}, acc1{0.0, 0.0};
#pragma unroll 8
        for (int c = 0; c < ACF_TILE / 64; ++c) {
            const int64_t n = base + (int64_t)c * 64;
            if (t < (int64_t)a.rem[n]) {
                const dd x = ld2(a.A, n);
                if (KIND == ACF_PLAIN) {
                    acc_add(acc0, x);
                } else if (KIND == ACF_AUTO) {
                    acc_add(acc0, dd_prod(x, ld2(a.A, n + t)));
                } else {
                    acc_add(acc0, dd_prod(x, ld2(a.B, n + t)));
                    acc_add(acc1, dd_prod(ld2(a.B, n), ld2(a.A, n + t)));
                }
            }
        }
        const dd t0 = wave_total(two_sum(acc0.hi, acc0.lo));
        if (lane == 0) a.tot[(int64_t)(j * a.nacc) * a.ntiles + tile] = double2{t0.hi, t0.lo};
        if (KIND == ACF_CROSS) {
            const dd t1 = wave_total(two_sum(acc1.hi, acc1.lo));
            if (lane == 0) a.tot[(int64_t)(j * a.nacc + 1) * a.ntiles + tile] = double2{t1.hi, t1.lo};
        }
    }
}

// one workgroup per (lag, accumulator): off[i] = sum of tot over tiles (i, atile_hi], chunked per thread, fixed order
__global__ void __launch_bounds__(ACF_WG) k_acf_scan(AcfLaunch a) {
    __shared__ dd lds[ACF_WAVES];
    const int64_t series = blockIdx.x;
    const double2* tot = a.tot + series * a.ntiles;
    double2* off = a.off + series * a.ntiles;
    const int64_t lo = a.tile_lo, cnt = a.atile_hi - a.tile_lo + 1;
    const int64_t chunk = (cnt + ACF_WG - 1) / ACF_WG;
    const int64_t b = lo + (int64_t)threadIdx.x * chunk;
    const int64_t e = min(b + chunk, lo + cnt);
    dd s{0.0, 0.0};
    for (int64_t i = e - 1; i >= b; --i) s = dd_add(ld2(tot, i), s);
    dd total;
    dd run = block_excl_suffix(s, lds, total);
    for (int64_t i = e - 1; i >= b; --i) {
        off[i] = double2{run.hi, run.lo};
        run = dd_add(ld2(tot, i), run);
    }
}

// Walks one lag of a thread's positions from the last to the first and calls at(r, q0, q1) with q0 / q1 = Q_t(n0 + r), the suffix
// sums of the two accumulators (q1: cross form only).
template <int KIND, typename F>
__device__ __forceinline__ void suffix_walk(const AcfLaunch& a, int64_t tile, int j, const dd* p0, const dd* p1, dd* lds, F at) {
    dd tot;
    const bool has_off = tile <= a.atile_hi;
    const dd ex0 = block_excl_suffix(thread_total(p0), lds, tot);
    dd run0 = has_off ? dd_add(ld2(a.off, (int64_t)(j * a.nacc) * a.ntiles + tile), ex0) : ex0;
    dd run1{0.0, 0.0};
    if (KIND == ACF_CROSS) {
        const dd ex1 = block_excl_suffix(thread_total(p1), lds, tot);
        run1 = has_off ? dd_add(ld2(a.off, (int64_t)(j * a.nacc + 1) * a.ntiles + tile), ex1) : ex1;
    }
#pragma unroll
    for (int r = ACF_R - 1; r >= 0; --r) {
        run0 = dd_add(run0, p0[r]);
        if (KIND == ACF_CROSS) run1 = dd_add(run1, p1[r]);
        at(r, run0, run1);
    }
}

template <int KIND>
__global__ void __launch_bounds__(ACF_WG) k_acf_store(AcfLaunch a, int64_t c_lo, const int* oid, double2* out, int64_t ldo) {
    __shared__ dd lds[ACF_WAVES];
    const int64_t tile = c_lo + blockIdx.x;
    const int64_t n0 = tile * ACF_TILE + (int64_t)threadIdx.x * ACF_R;
    Positions<KIND> P;
    P.load(a, n0);
    for (int j = 0; j < a.nl; ++j) {
        dd p0[ACF_R], p1[ACF_R];
        P.products(a, n0, a.lag[j], p0, p1);
        suffix_walk<KIND>(a, tile, j, p0, p1, lds, [&](int r, dd q0, dd q1) {
            const int64_t idx = oid ? (int64_t)oid[n0 + r] : n0 + r;
            if (idx < 0) return;
            out[(int64_t)(j * a.nacc) * ldo + idx] = double2{q0.hi, q0.lo};
            if (KIND == ACF_CROSS) out[(int64_t)(j * a.nacc + 1) * ldo + idx] = double2{q1.hi, q1.lo};
        });
    }
}

// X_AB(s, t) about the suffix means (dA, dB) of origin s of a series of length T:
//   Q_AB - dB (SA[s] - SA[T-t]) - dA SB[s+t] + (N - t) dA dB
__device__ __forceinline__ dd x_about_means(dd q, const double2* SA, const double2* SB, int64_t s, int64_t t, int64_t T, dd dA, dd dB) {
    const dd sa = dd_sub(ld2(SA, s), ld2(SA, T - t));
    const dd sb = ld2(SB, s + t);
    dd x = dd_sub(q, dd_mul(sa, dB));
    x = dd_sub(x, dd_mul(sb, dA));
    return dd_add(x, dd_mul_d(dd_mul(dA, dB), (double)(T - s - t)));
}

template <int KIND>
__global__ void __launch_bounds__(ACF_WG) k_acf_rule(AcfLaunch a, AcfRule ru, int64_t c_lo) {
    __shared__ dd lds[ACF_WAVES];
    __shared__ int ilds[ACF_WAVES];
    const int64_t tile = c_lo + blockIdx.x;
    const int64_t n0 = tile * ACF_TILE + (int64_t)threadIdx.x * ACF_R;
    Positions<KIND> P;
    P.load(a, n0);
    int64_t oi[ACF_R];
    double g[ACF_R];
    int st[ACF_R];
#pragma unroll
    for (int r = 0; r < ACF_R; ++r) {
        const int64_t n = n0 + r;
        oi[r] = (n % ru.nskip == 0 && n / ru.nskip < ru.norig) ? n / ru.nskip : -1;
        st[r] = oi[r] >= 0 ? ru.status[oi[r]] : -1;
        g[r] = oi[r] >= 0 ? ru.g[oi[r]] : 0.0;
    }
    for (int j = 0; j < a.nl; ++j) {
        const int64_t t = a.lag[j];
        dd p0[ACF_R], p1[ACF_R];
        P.products(a, n0, t, p0, p1);
        suffix_walk<KIND>(a, tile, j, p0, p1, lds, [&](int r, dd q0, dd q1) {
            if (st[r] != ACF_RUNNING) return;
            const int64_t o = oi[r], s = n0 + r;
            double X, N, Nw;
            int64_t tend;
            if (ru.mode == ACF_RULE_SUFFIX) {
                const dd dA = ld2(ru.dA, o), dB = ld2(ru.dB, o);
                const dd xab = x_about_means(q0, ru.SA, ru.SB, s, t, a.T, dA, dB);
                if (t == 0) {
                    X = xab.hi;
                } else if (KIND == ACF_CROSS) {
                    X = dd_add(xab, x_about_means(q1, ru.SB, ru.SA, s, t, a.T, dB, dA)).hi;
                } else {
                    X = 2.0 * xab.hi;
                }
                N = (double)(a.T - s);
                Nw = N;
                tend = a.T - s - (ru.fft ? 0 : 1);
            } else {
                X = q0.hi;  // (the shift is the mean: no deviation terms)
                N = (double)a.T;
                Nw = ru.navg;
                tend = ru.tend;
            }
            if (t == 0) {
                const double sig2 = X / N;
                ru.sig2[o] = sig2;
                if (sig2 == 0.0) {
                    st[r] = ACF_ZERO_VARIANCE;
                } else if (1 >= tend) {
                    st[r] = ACF_END;
                    ru.stop[o] = 1;
                }
                return;
            }
            const double sig2 = ru.sig2[o];
            double C;
            if (ru.mode == ACF_RULE_SUFFIX) {
                C = X / (2.0 * (double)(a.T - s - t) * sig2);
            } else {
                C = X / a.den[j];
                C = C / sig2;
            }
            if (o == 0 && ru.ct) ru.ct[a.kbase + j] = C;
            if (C <= 0.0 && t > ru.mintime) {
                st[r] = ACF_STOPPED;
                ru.stop[o] = t;
                return;
            }
            g[r] += 2.0 * C * (1.0 - (double)t / Nw) * (double)a.inc[j];
            if (t + a.inc[j] >= tend) {
                st[r] = ACF_END;
                ru.stop[o] = t + a.inc[j];
            }
        });
    }
    int running = 0;
#pragma unroll
    for (int r = 0; r < ACF_R; ++r) {
        if (oi[r] < 0) continue;
        ru.status[oi[r]] = st[r];
        ru.g[oi[r]] = (st[r] != ACF_RUNNING && g[r] < 1.0) ? 1.0 : g[r];
        running += st[r] == ACF_RUNNING;
    }
    running = block_sum_int(running, ilds);
    if (threadIdx.x == 0) ru.active[tile] = running;
}

__global__ void k_acf_rule_init(AcfRule ru, int64_t T, int64_t last_change) {
    const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= ru.norig) return;
    const int64_t s = o * ru.nskip;
    dd dA{0.0, 0.0}, dB{0.0, 0.0};
    if (ru.mode == ACF_RULE_SUFFIX) {
        dA = dd_div_d(ld2(ru.SA, s), (double)(T - s));
        dB = dd_div_d(ld2(ru.SB, s), (double)(T - s));
    }
    ru.dA[o] = double2{dA.hi, dA.lo};
    ru.dB[o] = double2{dB.hi, dB.lo};
    ru.g[o] = 1.0;
    ru.sig2[o] = 0.0;
    ru.stop[o] = 0;
    ru.status[o] = s > last_change ? ACF_ZERO_VARIANCE : ACF_RUNNING;
}

// one thread per (lag j, origin o) of the block
__global__ void k_acf_finish(AcfLaunch a, const double2* q, int64_t norig, const int64_t* orig, int segments, const double2* SA,
                             const double2* SB, double* xab, double* xba, int64_t j0) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)a.nl * norig) return;
    const int nacc = a.nacc;
    const int64_t T = a.T;
    const int j = (int)(i / norig);
    const int64_t o = i - (int64_t)j * norig, t = a.lag[j];
    const int64_t ldo = norig + 1;
    const int64_t out = (j0 + j) * norig + o;
    if (segments) {
        xab[out] = dd_sub(ld2(q, (int64_t)(j * nacc) * ldo + o), ld2(q, (int64_t)(j * nacc) * ldo + o + 1)).hi;
        if (nacc == 2) xba[out] = dd_sub(ld2(q, (int64_t)(j * nacc + 1) * ldo + o), ld2(q, (int64_t)(j * nacc + 1) * ldo + o + 1)).hi;
        else xba[out] = xab[out];
        return;
    }
    const int64_t s = orig[o], N = T - s;
    if (t >= N) {
        xab[out] = 0.0;
        xba[out] = 0.0;
        return;
    }
    const dd dA = dd_div_d(ld2(SA, s), (double)N), dB = dd_div_d(ld2(SB, s), (double)N);
    xab[out] = x_about_means(ld2(q, (int64_t)(j * nacc) * ldo + o), SA, SB, s, t, T, dA, dB).hi;
    xba[out] = nacc == 2 ? x_about_means(ld2(q, (int64_t)(j * nacc + 1) * ldo + o), SB, SA, s, t, T, dB, dA).hi : xab[out];
}

__global__ void k_acf_fill_int(int* p, int64_t n, int v) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

__global__ void k_acf_scatter_oid(int* oid, const int64_t* orig, int64_t norig) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < norig) oid[orig[i]] = (int)i;
}

unsigned blocks_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }
}  // namespace

#define ACF_DISPATCH(KERNEL, GRID, ...)                                                                  \
    switch (a.kind) {                                                                                     \
        case ACF_AUTO: hipLaunchKernelGGL(KERNEL<ACF_AUTO>, GRID, dim3(ACF_WG), 0, s, __VA_ARGS__); break;   \
        case ACF_CROSS: hipLaunchKernelGGL(KERNEL<ACF_CROSS>, GRID, dim3(ACF_WG), 0, s, __VA_ARGS__); break; \
        case ACF_PLAIN: hipLaunchKernelGGL(KERNEL<ACF_PLAIN>, GRID, dim3(ACF_WG), 0, s, __VA_ARGS__); break; \
        default: return hipErrorInvalidValue;                                                             \
    }

hipError_t launch_acf_tiles(hipStream_t s, const AcfLaunch& a) {
    if (a.atile_hi < a.tile_lo || a.nl < 1) return hipSuccess;
    ACF_DISPATCH(k_acf_tiles, dim3(blocks_of(a.atile_hi - a.tile_lo + 1, ACF_WAVES)), a);
    return hipGetLastError();
}

hipError_t launch_acf_scan(hipStream_t s, const AcfLaunch& a) {
    if (a.atile_hi < a.tile_lo || a.nl < 1) return hipSuccess;
    hipLaunchKernelGGL(k_acf_scan, dim3((unsigned)(a.nl * a.nacc)), dim3(ACF_WG), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_acf_store(hipStream_t s, const AcfLaunch& a, int64_t c_lo, int64_t c_hi, const int* oid, double2* out, int64_t ldo) {
    if (c_hi < c_lo || a.nl < 1) return hipSuccess;
    ACF_DISPATCH(k_acf_store, dim3((unsigned)(c_hi - c_lo + 1)), a, c_lo, oid, out, ldo);
    return hipGetLastError();
}

hipError_t launch_acf_rule(hipStream_t s, const AcfLaunch& a, const AcfRule& r, int64_t c_lo, int64_t c_hi) {
    if (c_hi < c_lo || a.nl < 1) return hipSuccess;
    if (a.kind == ACF_AUTO)
        hipLaunchKernelGGL(k_acf_rule<ACF_AUTO>, dim3((unsigned)(c_hi - c_lo + 1)), dim3(ACF_WG), 0, s, a, r, c_lo);
    else if (a.kind == ACF_CROSS)
        hipLaunchKernelGGL(k_acf_rule<ACF_CROSS>, dim3((unsigned)(c_hi - c_lo + 1)), dim3(ACF_WG), 0, s, a, r, c_lo);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}
#undef ACF_DISPATCH

hipError_t launch_acf_rule_init(hipStream_t s, const AcfRule& r, int64_t T, int64_t last_change) {
    if (r.norig < 1) return hipSuccess;
    hipLaunchKernelGGL(k_acf_rule_init, dim3(blocks_of(r.norig, 256)), dim3(256), 0, s, r, T, last_change);
    return hipGetLastError();
}

hipError_t launch_acf_finish(hipStream_t s, const AcfLaunch& a, const double2* q, int64_t norig, const int64_t* orig, int segments,
                             const double2* SA, const double2* SB, double* xab, double* xba, int64_t j0) {
    if (a.nl < 1 || norig < 1) return hipSuccess;
    hipLaunchKernelGGL(k_acf_finish, dim3(blocks_of((int64_t)a.nl * norig, 256)), dim3(256), 0, s, a, q, norig, orig, segments, SA, SB,
                       xab, xba, j0);
    return hipGetLastError();
}

hipError_t launch_acf_fill_int(hipStream_t s, int* p, int64_t n, int v) {
    if (n < 1) return hipSuccess;
    hipLaunchKernelGGL(k_acf_fill_int, dim3(blocks_of(n, 256)), dim3(256), 0, s, p, n, v);
    return hipGetLastError();
}

hipError_t launch_acf_scatter_oid(hipStream_t s, int* oid, const int64_t* orig, int64_t norig) {
    if (norig < 1) return hipSuccess;
    hipLaunchKernelGGL(k_acf_scatter_oid, dim3(blocks_of(norig, 256)), dim3(256), 0, s, oid, orig, norig);
    return hipGetLastError();
}

}  // namespace mbar
