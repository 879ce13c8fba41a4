// gfx950 (CDNA4 / MI355X) kernels of the weighted kernel-density sum behind pymbar_amd.kde / pymbar_amd.FES:
//   L[m, c] = log sum_n V[n, c] k_h(|q_m - x_n|) - log sum_n V[n, c] + log-normaliser
// One of the translation units of libmbar_hip.so: the shared device helpers (exp2 table, exp2s) are in mbar_device.h, the host
// side of the launchers in mbar_kde.h, the C ABI in mbar_kde.cpp.  DESIGN.md ("Kernel-density surfaces") has the numbers.
//
// Layout.  Samples X: [d][ldx] (coordinate-major, ldx = N rounded up to KDE_TILE, padding = copies of the last sample with weight
// zero), weights of one column batch V: [ldx][CB] (the CB weights of a sample are contiguous), queries Q: [d][ldq].  For the two
// kernels with unbounded support (gaussian, exponential) the exp2s argument (units of 1/S doublings, mbar_device.h) of a pair
// is t = coef r^2 (coef = -S log2(e) / 2h^2) or t = coef r (coef = -S log2(e) / h), folded with the shift into one FMA; the
// compact kernels evaluate sklearn's own formulas on dist = sqrt(r^2), so that the support test `dist < h` decides r == h the
// same way.
//
// k_kde: one query per lane (256 per workgroup), one contiguous chunk of samples per workgroup (blockIdx.y), staged through LDS
// in tiles of KDE_TILE samples that every lane reads as a broadcast.  The kernel is evaluated ONCE per pair and accumulated
// into all CB columns with one fp64 FMA each.  Unbounded kernels accumulate V exp2s(t - m) against a per-query running shift m
// (online log-sum-exp with a deferred maximum, cdna_hip_programming.md T13): m only moves when a term would exceed 2^256, and
// then every column sum is multiplied by 2^((m_old - m_new)/S) before the new term is added -- the term that moves m is
// exponentiated after the decision, so nothing at the old scale survives unscaled.  fp64 holds N 2^257 for any N, and the
// rescale is a rare, data-dependent branch (tests/test_gpu_kde.py forces it).  Each workgroup writes (m, sums) of its chunk to
// a fixed slot; k_kde_combine merges the chunks in chunk order (bit-identical results from call to call).
//
// The shift is shared by the columns and includes zero-weight samples, so a column whose own nearest weighted sample is more
// than ~900 doublings below the shift would lose its terms to underflow.  k_kde_combine flags such (query, column) pairs
// (sum < 2^-900 with a positive column total) and k_kde_exact recomputes them with their own maximum over the samples of
// positive weight, in plain log space: the result is the exact, finite log density wherever one exists.
//
// A pair so far apart that r^2, or r coef, overflows (|q - x| beyond ~1e154 for the gaussian kernel) makes the exp2s argument
// -inf, and exp2s(-inf) is inf - inf = NaN in every column sum of that query (and of no other: a query is a lane).  The common
// path does not test for it: k_kde_combine flags a NaN sum like a small one, and k_kde_exact -- which measures an overflowing
// distance in units of its largest coordinate difference -- returns the value the exact log density rounds to: finite where
// -r / h or -r^2 / 2h^2 is inside the fp64 range, -inf below it, never NaN.
#include "mbar_device.h"
#include "mbar_kde.h"

namespace mbar {

namespace {
constexpr int KDE_THREADS = 256;
constexpr double KDE_THR = 256.0 * EXP2_S;   // deferred-max threshold (exp2s units): terms stay below 2^256
constexpr double KDE_M0 = -1.0e300;          // initial shift: the first term always moves it (finite: no inf - inf)
constexpr double KDE_FLAG_BELOW = 0x1p-900;  // combined sums below this (positive total weight) are recomputed by k_kde_exact
constexpr double HALF_PI = 1.57079632679489661923;

template <int KER>
constexpr bool kde_unbounded() { return KER == KDE_GAUSSIAN || KER == KDE_EXPONENTIAL; }

// 2^(z/S) for finite z <= KDE_THR (no clamp: v_cvt_i32_f64 saturates, so a hugely negative z gives ldexp(., -2^20) = 0)
__device__ __forceinline__ double kde_exp2s(double z) {
    const double s = __builtin_rint(z);
    const int si = (int)s;
    return ldexp(exp2_table_at(si) * exp2_poly(z - s), si >> EXP2_BITS);
}

// compact kernels: sklearn's formulas on dist = sqrt(sum dx^2) (uncontracted, in coordinate order, correctly rounded sqrt)
template <int KER>
__device__ __forceinline__ double kde_compact(double dist, double h, double inv_h, double inv_h2) {
    if (!(dist < h)) return 0.0;
    if constexpr (KER == KDE_TOPHAT) return 1.0;
    else if constexpr (KER == KDE_EPANECHNIKOV) return 1.0 - __dmul_rn(dist, dist) * inv_h2;
    else if constexpr (KER == KDE_LINEAR) return 1.0 - dist * inv_h;
    else return cos(HALF_PI * dist * inv_h);
}
}  // namespace

// D = 1, 2, 3: compile-time dimension; D = 0: generic, dg <= KDE_MAX_D at run time.
template <int KER, int D, int CB>
__global__ void __launch_bounds__(KDE_THREADS)
k_kde(const double* __restrict__ X, int64_t ldx, int dg, const double* __restrict__ V, const double* __restrict__ Q, int64_t ldq,
      int64_t M, double coef, double h, double inv_h, double inv_h2, int64_t chunk, double* __restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr bool UNB = kde_unbounded<KER>();
    constexpr int DD = D > 0 ? D : KDE_MAX_D;
    const int nd = D > 0 ? D : dg;
    if constexpr (UNB) exp_table_init(smem);
    double* xs = reinterpret_cast<double*>(smem + (UNB ? EXP_TABLE_BYTES : 0));  // [DD][KDE_TILE]
    double* vs = xs + DD * KDE_TILE;                                               // [KDE_TILE][CB]
    const int tid = threadIdx.x;
    const int64_t q = (int64_t)blockIdx.x * KDE_THREADS + tid;
    const int64_t qq = q < M ? q : M - 1;
    double qc[DD];
#pragma unroll
    for (int k = 0; k < DD; ++k) qc[k] = (D > 0 || k < nd) ? Q[k * ldq + qq] : 0.0;
    double acc[CB];
#pragma unroll
    for (int c = 0; c < CB; ++c) acc[c] = 0.0;
    double m = UNB ? KDE_M0 : 0.0;
    const int64_t n0 = (int64_t)blockIdx.y * chunk;
    const int64_t n1 = n0 + chunk < ldx ? n0 + chunk : ldx;
    for (int64_t t0 = n0; t0 < n1; t0 += KDE_TILE) {
        __syncthreads();  // (the previous tile is consumed; the first pass also orders the table copy)
        for (int i = tid; i < nd * KDE_TILE; i += KDE_THREADS) xs[i] = X[(int64_t)(i / KDE_TILE) * ldx + t0 + (i % KDE_TILE)];
        for (int i = tid; i < KDE_TILE * CB; i += KDE_THREADS) vs[i] = V[t0 * CB + i];
        __syncthreads();
#pragma unroll 2
        for (int j = 0; j < KDE_TILE; ++j) {
            double e;
            if constexpr (UNB) {
                double r2 = 0.0;
#pragma unroll
                for (int k = 0; k < DD; ++k) {
                    if (D > 0 || k < nd) {
                        const double dx = qc[k] - xs[k * KDE_TILE + j];
                        r2 = fma(dx, dx, r2);
                    }
                }
                const double r = KER == KDE_GAUSSIAN ? r2 : (D == 1 ? fabs(qc[0] - xs[j]) : sqrt(r2));
                double z = fma(r, coef, -m);
                // (a wave-uniform test: the common path has no divergent branch around the exponential)
                if (__builtin_expect(__any(z > KDE_THR), 0)) {
                    if (z > KDE_THR) {
                        // the shift moves to this term: every column sum still at the old shift is rescaled once, and
                        // this term (exponentiated below, after the decision) enters at the new one
                        const double tt = r * coef;
                        const double f = exp2s_fast(m - tt);
#pragma unroll
                        for (int c = 0; c < CB; ++c) acc[c] *= f;
                        m = tt;
                        z = fma(r, coef, -m);
                    }
                }
                e = kde_exp2s(z);
            } else {
                double r2 = 0.0;
#pragma unroll
                for (int k = 0; k < DD; ++k) {
                    if (D > 0 || k < nd) {
                        const double dx = qc[k] - xs[k * KDE_TILE + j];
                        r2 = __dadd_rn(r2, __dmul_rn(dx, dx));
                    }
                }
                e = kde_compact<KER>(sqrt(r2), h, inv_h, inv_h2);
            }
            const double* vj = vs + j * CB;
#pragma unroll
            for (int c = 0; c < CB; ++c) acc[c] = fma(vj[c], e, acc[c]);
        }
    }
    if (q < M) {
        double* rec = part + (int64_t)blockIdx.y * (CB + 1) * ldq + q;
        rec[0] = m;
#pragma unroll
        for (int c = 0; c < CB; ++c) rec[(int64_t)(c + 1) * ldq] = acc[c];
    }
}

// out[q * ldo + c] for c < cv: chunks merged in chunk order; flag[q * cv + c] = 1 where k_kde_exact must recompute
__global__ void __launch_bounds__(256)
k_kde_combine(const double* __restrict__ part, int64_t nchunks, int CB, int64_t ldq, int64_t M, int cv, const double* __restrict__ logW,
              double lognorm, int unbounded, double* __restrict__ out, int* __restrict__ flag) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int c = blockIdx.y;
    if (q >= M || c >= cv) return;
    const int64_t stride = (int64_t)(CB + 1) * ldq;
    double mx = -INFINITY;
    for (int64_t b = 0; b < nchunks; ++b) mx = fmax(mx, part[b * stride + q]);
    double s = 0.0;
    for (int64_t b = 0; b < nchunks; ++b) {
        const double v = part[b * stride + (int64_t)(c + 1) * ldq + q];
        if (!unbounded) {
            s += v;
        } else {
            // (a chunk far below the largest shift: scale in log space, so that a large sum is not flushed with its factor)
            const double dm = (part[b * stride + q] - mx) / EXP2_S;
            s += dm > -960.0 ? v * exp2(dm) : (v > 0.0 ? exp2(dm + log2(v)) : 0.0);
        }
    }
    const double lw = logW[c];
    double L;
    int fl = 0;
    if (!(lw > -INFINITY)) {
        L = NAN;  // a column of zero total weight has no density
    } else {
        L = (unbounded ? mx * LN2_OVER_S : 0.0) + log(s) - lw + lognorm;
        // (unbounded kernels: also a NaN sum -- a pair whose r coef overflowed to -inf put inf - inf into every column of its
        // query; k_kde_exact works in log space and gives such a query its finite value, or -inf below the fp64 range)
        fl = unbounded ? !(s >= KDE_FLAG_BELOW) : (s < KDE_FLAG_BELOW && s > 0.0);
    }
    out[q * cv + c] = L;
    flag[q * cv + c] = fl;
}

// One workgroup per flagged pair (query pq[2i], column pq[2i+1] of the batch): two passes over the N real samples in plain log
// space -- the maximum of log V + log k over the samples of positive weight, then the sum of exp(. - max) -- with fixed-order
// tree reductions.  out[i] = the log density (-inf if no weighted sample has a positive kernel value).
template <int KER>
__global__ void __launch_bounds__(256)
k_kde_exact(const double* __restrict__ X, int64_t ldx, int dg, int64_t N, const double* __restrict__ V, int CB,
            const double* __restrict__ Q, int64_t ldq, const int64_t* __restrict__ pq, double h, double inv_h, double inv_h2,
            const double* __restrict__ logW, double lognorm, double* __restrict__ out) {
    __shared__ double red[256];
    const int64_t q = pq[2 * blockIdx.x];
    const int c = (int)pq[2 * blockIdx.x + 1];
    const int tid = threadIdx.x;
    double qc[KDE_MAX_D];
#pragma unroll
    for (int k = 0; k < KDE_MAX_D; ++k) qc[k] = k < dg ? Q[k * ldq + q] : 0.0;
    auto logterm = [&](int64_t n) -> double {
        const double v = V[n * CB + c];
        if (!(v > 0.0)) return -INFINITY;
        double r2 = 0.0;
#pragma unroll
        for (int k = 0; k < KDE_MAX_D; ++k) {
            if (k < dg) {
                const double dx = qc[k] - X[k * ldx + n];
                r2 = kde_unbounded<KER>() ? fma(dx, dx, r2) : __dadd_rn(r2, __dmul_rn(dx, dx));
            }
        }
        double lk;
        if constexpr (kde_unbounded<KER>()) {
            if (r2 < INFINITY) {
                lk = KER == KDE_GAUSSIAN ? -0.5 * r2 * inv_h2 : -sqrt(r2) * inv_h;
            } else {
                // r^2 is beyond the fp64 range, r / h need not be: the distance in units of the largest |dx| (halved
                // coordinates, exact at this size: q - x itself may overflow).  Rolled loops on the coordinates in memory:
                // this path is rare and must not cost the common one registers.
                double amax = 0.0;
#pragma unroll 1
                for (int k = 0; k < dg; ++k) amax = fmax(amax, fabs(0.5 * Q[k * ldq + q] - 0.5 * X[k * ldx + n]));
                double u2 = 0.0;
#pragma unroll 1
                for (int k = 0; k < dg; ++k) {
                    const double u = (0.5 * Q[k * ldq + q] - 0.5 * X[k * ldx + n]) / amax;
                    u2 = fma(u, u, u2);
                }
                const double rh = 2.0 * (amax * inv_h * sqrt(u2));  // r / h (inf when that is out of range too)
                lk = KER == KDE_GAUSSIAN ? -0.5 * rh * rh : -rh;
            }
        } else {
            const double kv = kde_compact<KER>(sqrt(r2), h, inv_h, inv_h2);
            if (!(kv > 0.0)) return -INFINITY;
            lk = log(kv);
        }
        return lk + log(v);
    };
    double mx = -INFINITY;
    for (int64_t n = tid; n < N; n += 256) mx = fmax(mx, logterm(n));
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
        for (int64_t n = tid; n < N; n += 256) s += exp(logterm(n) - mx);
    red[tid] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
    if (tid == 0) out[blockIdx.x] = mx > -INFINITY ? mx + log(red[0]) - logW[c] + lognorm : -INFINITY;
}

// ---- launchers -------------------------------------------------------------------------------------------------------------
size_t kde_lds_bytes(int kernel, int d, int cb) {
    const int dd = d <= 3 ? d : KDE_MAX_D;
    const bool unb = kernel == KDE_GAUSSIAN || kernel == KDE_EXPONENTIAL;
    return (unb ? (size_t)EXP_TABLE_BYTES : 0) + (size_t)dd * KDE_TILE * 8 + (size_t)KDE_TILE * cb * 8;
}

namespace {
template <int KER, int D, int CB>
hipError_t launch_kde_t(hipStream_t s, const KdeLaunch& a) {
    const size_t lds = kde_lds_bytes(KER, D > 0 ? D : KDE_MAX_D, CB);
    hipLaunchKernelGGL((k_kde<KER, D, CB>), dim3((unsigned)a.qblocks, (unsigned)a.nchunks), dim3(KDE_THREADS), lds, s, a.X, a.ldx, a.d,
                       a.V, a.Q, a.ldq, a.M, a.coef, a.h, a.inv_h, a.inv_h2, a.chunk, a.part);
    return hipGetLastError();
}
template <int KER, int D>
hipError_t launch_kde_cb(hipStream_t s, const KdeLaunch& a) {
    switch (a.cb) {
        case 1: return launch_kde_t<KER, D, 1>(s, a);
        case 4: return launch_kde_t<KER, D, 4>(s, a);
        case 8: return launch_kde_t<KER, D, 8>(s, a);
        case 16: return launch_kde_t<KER, D, 16>(s, a);
        case 24: return launch_kde_t<KER, D, 24>(s, a);
        case 32: return launch_kde_t<KER, D, 32>(s, a);
        default: return hipErrorInvalidValue;
    }
}
template <int KER>
hipError_t launch_kde_unb(hipStream_t s, const KdeLaunch& a) {
    switch (a.d) {
        case 1: return launch_kde_cb<KER, 1>(s, a);
        case 2: return launch_kde_cb<KER, 2>(s, a);
        case 3: return launch_kde_cb<KER, 3>(s, a);
        default: return launch_kde_cb<KER, 0>(s, a);
    }
}
}  // namespace

hipError_t launch_kde(hipStream_t s, const KdeLaunch& a) {
    if (a.d < 1 || a.d > KDE_MAX_D) return hipErrorInvalidValue;
    // (compact kernels: the generic-dimension body only -- the unbounded two are the ones a surface is usually built with)
    switch (a.kernel) {
        case KDE_GAUSSIAN: return launch_kde_unb<KDE_GAUSSIAN>(s, a);
        case KDE_EXPONENTIAL: return launch_kde_unb<KDE_EXPONENTIAL>(s, a);
        case KDE_TOPHAT: return launch_kde_cb<KDE_TOPHAT, 0>(s, a);
        case KDE_EPANECHNIKOV: return launch_kde_cb<KDE_EPANECHNIKOV, 0>(s, a);
        case KDE_LINEAR: return launch_kde_cb<KDE_LINEAR, 0>(s, a);
        case KDE_COSINE: return launch_kde_cb<KDE_COSINE, 0>(s, a);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_kde_combine(hipStream_t s, const KdeLaunch& a, int cv, const double* logW, double lognorm, double* out, int* flag) {
    const bool unb = a.kernel == KDE_GAUSSIAN || a.kernel == KDE_EXPONENTIAL;
    hipLaunchKernelGGL(k_kde_combine, dim3((unsigned)((a.M + 255) / 256), (unsigned)cv), dim3(256), 0, s, a.part, a.nchunks, a.cb, a.ldq,
                       a.M, cv, logW, lognorm, unb ? 1 : 0, out, flag);
    return hipGetLastError();
}

hipError_t launch_kde_exact(hipStream_t s, const KdeLaunch& a, int64_t N, int64_t npairs, const int64_t* pq, const double* logW,
                            double lognorm, double* out) {
    if (npairs <= 0) return hipSuccess;
#define KDE_EXACT(K)                                                                                                           \
    hipLaunchKernelGGL(k_kde_exact<K>, dim3((unsigned)npairs), dim3(256), 0, s, a.X, a.ldx, a.d, N, a.V, a.cb, a.Q, a.ldq, pq, a.h, \
                       a.inv_h, a.inv_h2, logW, lognorm, out)
    switch (a.kernel) {
        case KDE_GAUSSIAN: KDE_EXACT(KDE_GAUSSIAN); break;
        case KDE_EXPONENTIAL: KDE_EXACT(KDE_EXPONENTIAL); break;
        case KDE_TOPHAT: KDE_EXACT(KDE_TOPHAT); break;
        case KDE_EPANECHNIKOV: KDE_EXACT(KDE_EPANECHNIKOV); break;
        case KDE_LINEAR: KDE_EXACT(KDE_LINEAR); break;
        case KDE_COSINE: KDE_EXACT(KDE_COSINE); break;
        default: return hipErrorInvalidValue;
    }
#undef KDE_EXACT
    return hipGetLastError();
}

}  // namespace mbar
