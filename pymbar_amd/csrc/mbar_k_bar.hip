// gfx950 (CDNA4 / MI355X) kernels of the BAR and EXP estimators behind pymbar_amd.other_estimators.  One of the translation units
// of libmbar_hip.so: launchers declared in mbar_bar.h, C ABI in mbar_bar.cpp, design and numbers in DESIGN.md ("BAR and EXP").
//
// Every side (forward or reverse work values of one problem) is cut into chunks of MBAR_BAR_CHUNK values; one workgroup handles
// one chunk.  The Fermi factor's log, log f(x) = -softplus(x), is decreasing in w on both sides (x_F = M + w - DeltaF,
// x_R = w + DeltaF - M), so the chunk's largest term is the one at its minimum w, known since the upload.  Each chunk sums
// exp(log f_i - log f_max) in [1, MBAR_BAR_CHUNK] (and the squares) with its shift -softplus(x_min) held as hi + lo: no term can
// overflow, and none is lost to underflow that is not below 2^-1074 of the chunk's largest.
//   k_bar_eval     every chunk of every running problem at its one or two requested DeltaF values, one load of w for both
//   k_bar_step     one workgroup per problem: merges the partials of each side in a fixed order and advances the problem's root
//                  find (bar_advance, mbar_bar.h) -- or stores the sums for mbar_bar_zero
//   k_bar_mom*     the one-sided moments of EXP: logsumexp(-w), sum x and sum (x - mean)^2 of x = exp(-w - max(-w)), sum w and
//                  sum (w - mean)^2, each a fixed-order two-level reduction
// No atomics: every reduction has a fixed order that depends on the side's length alone, so two identical calls return identical
// bits and a problem's answer does not depend on the other problems of the batch.
#include "mbar_device.h"
#include "mbar_bar.h"

namespace mbar {

namespace {

struct dd2 {
    double hi, lo;
};
__device__ __forceinline__ dd2 two_sum(double a, double b) {
    const double s = a + b;
    const double bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}

// log(1 + exp(-|x|)), the part of softplus(x) = max(x, 0) + log(1 + exp(-|x|)) in (0, log 2]
__device__ __forceinline__ double softplus_tail(double x) { return log1p(exp(-fabs(x))); }

// fixed-order sum over the workgroup: a butterfly inside each wave, then the waves in order (result valid in thread 0)
template <int N>
__device__ __forceinline__ void block_sum(double (&v)[N], double (*lds)[BAR_WG / 64]) {
#pragma unroll
    for (int k = 0; k < N; ++k)
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_xor(v[k], o, 64);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < N; ++k) lds[k][wv] = v[k];
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < N; ++k) {
            double s = lds[k][0];
            for (int j = 1; j < BAR_WG / 64; ++j) s += lds[k][j];
            v[k] = s;
        }
}

__device__ __forceinline__ double block_max(double v, double* lds) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __syncthreads();
    if (lane == 0) lds[wv] = v;
    __syncthreads();
    double m = lds[0];
    for (int j = 1; j < BAR_WG / 64; ++j) m = fmax(m, lds[j]);
    return m;
}

// the DeltaF values a problem needs this pass (0: nothing)
__device__ __forceinline__ int requests(const mbar_bar_state& st, double* x) {
    if (st.status == BAR_RUNNING) {
        x[0] = st.req[0];
        x[1] = st.req[1];
        return st.nreq < 0 ? 0 : (st.nreq > 2 ? 2 : (int)st.nreq);
    }
    if (st.moments_pending) {
        x[0] = st.iterated ? st.DeltaF : st.DeltaF_initial;
        return 1;
    }
    return 0;
}

__global__ void __launch_bounds__(BAR_WG) k_bar_eval(BarData d, const mbar_bar_state* __restrict__ states, BarPartial* __restrict__ part) {
    __shared__ double lds[2][BAR_WG / 64];
    const int64_t c = blockIdx.x;
    const int sg = d.seg[c];
    const int64_t p = sg >> 1;
    const int side = sg & 1;
    double req[2];
    const int nreq = requests(states[p], req);
    if (nreq == 0) return;
    const double wmin = d.wmin[c];
    if (wmin == INFINITY) {  // every value is +inf: every factor is 0
        if (threadIdx.x == 0)
            for (int r = 0; r < nreq; ++r) part[r * d.nchunks + c] = BarPartial{-INFINITY, 0.0, 0.0, 0.0};
        return;
    }
    const int len = d.len[c];
    const double* __restrict__ w = d.w + d.start[c];
    double v[BAR_PER_THREAD];
#pragma unroll
    for (int j = 0; j < BAR_PER_THREAD; ++j) {
        const int i = threadIdx.x + j * BAR_WG;
        v[j] = i < len ? w[i] : INFINITY;  // +inf: a factor of exactly 0
    }
    const double M = d.M[p];
    for (int r = 0; r < nreq; ++r) {
        // x = (w + c1) + c2: forward (w - DeltaF) + M, reverse (w + DeltaF) - M
        const double c1 = side ? req[r] : -req[r];
        const double c2 = side ? -M : M;
        const dd2 a = two_sum(wmin, c1);
        const dd2 b = two_sum(a.hi, c2);
        const double xmin = b.hi;
        const double lmin = softplus_tail(xmin);
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int j = 0; j < BAR_PER_THREAD; ++j) {
            const double x = (v[j] + c1) + c2;
            // log f_i - log f_max = softplus(x_min) - softplus(x_i); for x_min, x_i > 0 the linear parts differ by w_min - w_i
            const double lin = x > 0.0 ? (xmin > 0.0 ? wmin - v[j] : -x) : 0.0;
            const double t = exp(lin + (lmin - softplus_tail(x)));
            s1 += t;
            s2 += t * t;
        }
        double s[2] = {s1, s2};
        block_sum<2>(s, lds);
        if (threadIdx.x == 0) {
            // shift = -softplus(x_min) as hi + lo
            double hi, lo;
            if (xmin > 0.0) {
                const dd2 h = two_sum(xmin, lmin);
                hi = h.hi;
                lo = h.lo + (a.lo + b.lo);
            } else {
                hi = lmin;
                lo = 0.0;
            }
            part[r * d.nchunks + c] = BarPartial{-hi, -lo, s[0], s[1]};
        }
    }
}

// log sum and log sum of squares of one side from its chunk partials, in a fixed order (valid in thread 0)
__device__ void merge_side(const BarPartial* __restrict__ part, int64_t beg, int64_t end, double* lds, double (*lds2)[BAR_WG / 64],
                           double& l1, double& l2) {
    double m = -INFINITY;
    for (int64_t c = beg + threadIdx.x; c < end; c += BAR_WG) m = fmax(m, part[c].hi);
    const double L = block_max(m, lds);
    double s[2] = {0.0, 0.0};
    if (L != -INFINITY)
        for (int64_t c = beg + threadIdx.x; c < end; c += BAR_WG) {
            const BarPartial q = part[c];
            if (q.s1 == 0.0) continue;
            const double e = (q.hi - L) + q.lo;
            s[0] += q.s1 * exp(e);
            s[1] += q.s2 * exp(2.0 * e);
        }
    block_sum<2>(s, lds2);
    if (L == -INFINITY) {
        l1 = l2 = -INFINITY;
    } else {
        l1 = L + log(s[0]);
        l2 = 2.0 * L + log(s[1]);
    }
}

__global__ void __launch_bounds__(BAR_WG) k_bar_step(BarData d, mbar_bar_state* __restrict__ states, const BarPartial* __restrict__ part,
                                                     int advance, double* __restrict__ out, int* __restrict__ active) {
    __shared__ double lds[BAR_WG / 64];
    __shared__ double lds2[2][BAR_WG / 64];
    const int64_t p = blockIdx.x;
    double req[2];
    const int nreq = requests(states[p], req);
    if (nreq == 0) {
        if (threadIdx.x == 0 && advance) active[p] = 0;
        return;
    }
    double F[2], l[4] = {0.0, 0.0, 0.0, 0.0};
    for (int r = 0; r < nreq; ++r) {
        const BarPartial* pr = part + r * d.nchunks;
        double lF1, lF2, lR1, lR2;
        merge_side(pr, d.cbeg[2 * p], d.cbeg[2 * p + 1], lds, lds2, lF1, lF2);
        merge_side(pr, d.cbeg[2 * p + 1], d.cbeg[2 * p + 2], lds, lds2, lR1, lR2);
        F[r] = lF1 - lR1;
        if (r == 0) {
            l[0] = lF1;
            l[1] = lR1;
            l[2] = lF2;
            l[3] = lR2;
        }
    }
    if (threadIdx.x != 0) return;
    if (!advance) {
        out[5 * p] = F[0];
        for (int k = 0; k < 4; ++k) out[5 * p + 1 + k] = l[k];
        return;
    }
    mbar_bar_state st = states[p];
    if (st.status == BAR_RUNNING) {
        bar_advance(st, F);
        if (st.status == BAR_DONE && st.want_moments) st.moments_pending = 1;
    } else {
        for (int k = 0; k < 4; ++k) st.moments[k] = l[k];
        st.moments_pending = 0;
    }
    states[p] = st;
    active[p] = (st.status == BAR_RUNNING || st.moments_pending) ? 1 : 0;
}

// ---- one-sided moments ------------------------------------------------------------------------------------------------------------
// aux[s][3] = (min w of the side, mean w, mean x); scratch part[2][nchunks]
__global__ void __launch_bounds__(BAR_WG) k_bar_mom_chunk(BarData d, int stage, const double* __restrict__ aux, double* __restrict__ part) {
    __shared__ double lds[2][BAR_WG / 64];
    const int64_t c = blockIdx.x;
    const int sg = d.seg[c];
    const int len = d.len[c];
    const double* __restrict__ w = d.w + d.start[c];
    const double wmin_c = d.wmin[c];
    const double wmin_s = aux[3 * sg], mw = aux[3 * sg + 1], mx = aux[3 * sg + 2];
    double s[2] = {0.0, 0.0};
#pragma unroll 4
    for (int j = 0; j < BAR_PER_THREAD; ++j) {
        const int i = threadIdx.x + j * BAR_WG;
        if (i >= len) break;
        const double v = w[i];
        if (stage == 0) {
            // exp(-w) shifted by the chunk's largest, and w itself
            s[0] += wmin_c == INFINITY ? 0.0 : exp(wmin_c - v);
            s[1] += v;
        } else if (stage == 1) {
            // x = exp(-w - max(-w)) as the reference forms it, and the centred square of w
            s[0] += exp(-v - (-wmin_s));
            const double dw = v - mw;
            s[1] += dw * dw;
        } else {
            const double dx = exp(-v - (-wmin_s)) - mx;
            s[0] += dx * dx;
        }
    }
    block_sum<2>(s, lds);
    if (threadIdx.x == 0) {
        part[c] = s[0];
        part[d.nchunks + c] = s[1];
    }
}

// one workgroup per side: the side's chunks in a fixed order
__global__ void __launch_bounds__(BAR_WG) k_bar_mom_merge(BarData d, int stage, const int64_t* __restrict__ nside, const double* __restrict__ part,
                                                          double* __restrict__ aux, double* __restrict__ out) {
    __shared__ double lds[BAR_WG / 64];
    __shared__ double lds2[2][BAR_WG / 64];
    const int64_t sg = blockIdx.x;
    const int64_t beg = d.cbeg[sg], end = d.cbeg[sg + 1];
    const double n = (double)nside[sg];
    double* o = out + 5 * sg;
    double* a = aux + 3 * sg;
    if (stage == 0) {
        double m = INFINITY;
        for (int64_t c = beg + threadIdx.x; c < end; c += BAR_WG) m = fmin(m, d.wmin[c]);
        const double wmin = -block_max(-m, lds);
        double s[2] = {0.0, 0.0};
        for (int64_t c = beg + threadIdx.x; c < end; c += BAR_WG) {
            if (d.wmin[c] != INFINITY) s[0] += part[c] * exp(wmin - d.wmin[c]);
            s[1] += part[d.nchunks + c];  // (a side of +inf values: sum w = +inf, as the reference's)
        }
        block_sum<2>(s, lds2);
        if (threadIdx.x == 0) {
            o[0] = wmin == INFINITY ? -INFINITY : -wmin + log(s[0]);
            o[3] = s[1];
            a[0] = wmin;
            a[1] = end > beg ? s[1] / n : 0.0;
        }
    } else {
        double s[2] = {0.0, 0.0};
        for (int64_t c = beg + threadIdx.x; c < end; c += BAR_WG) {
            s[0] += part[c];
            s[1] += part[d.nchunks + c];
        }
        block_sum<2>(s, lds2);
        if (threadIdx.x == 0) {
            if (stage == 1) {
                o[1] = s[0];
                o[4] = s[1];
                a[2] = end > beg ? s[0] / n : 0.0;
            } else {
                o[2] = s[0];
            }
        }
    }
}

}  // namespace

hipError_t launch_bar_eval(hipStream_t st, const BarData& d, const mbar_bar_state* states, BarPartial* part) {
    if (d.nchunks == 0) return hipSuccess;
    hipLaunchKernelGGL(k_bar_eval, dim3((unsigned)d.nchunks), dim3(BAR_WG), 0, st, d, states, part);
    return hipGetLastError();
}

hipError_t launch_bar_step(hipStream_t st, const BarData& d, mbar_bar_state* states, const BarPartial* part, int advance, double* out,
                           int* active) {
    hipLaunchKernelGGL(k_bar_step, dim3((unsigned)d.P), dim3(BAR_WG), 0, st, d, states, part, advance, out, active);
    return hipGetLastError();
}

hipError_t launch_bar_moments(hipStream_t st, const BarData& d, const int64_t* nside, double* scratch, double* out) {
    double* part = scratch;
    double* aux = scratch + 2 * d.nchunks;
    for (int stage = 0; stage < 3; ++stage) {
        if (d.nchunks > 0) hipLaunchKernelGGL(k_bar_mom_chunk, dim3((unsigned)d.nchunks), dim3(BAR_WG), 0, st, d, stage, aux, part);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_bar_mom_merge, dim3((unsigned)(2 * d.P)), dim3(BAR_WG), 0, st, d, stage, nside, part, aux, out);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace mbar
