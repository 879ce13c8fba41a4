// ---- weighted kernel-density sum (mbar_k_kde.hip; C ABI in mbar_kde.cpp) ---------------------------------------------------
#pragma once
#include "mbar_common.h"

namespace mbar {

enum : int { KDE_GAUSSIAN = 0, KDE_TOPHAT = 1, KDE_EPANECHNIKOV = 2, KDE_EXPONENTIAL = 3, KDE_LINEAR = 4, KDE_COSINE = 5 };
constexpr int KDE_MAX_D = 8;    // dimensions of the generic body (1, 2, 3 have bodies of their own)
constexpr int KDE_TILE = 64;    // samples per LDS tile: the sample pitch ldx is a multiple of it
constexpr int KDE_MAX_CB = 32;  // weight columns per pass; a pass runs with the smallest of {1, 4, 8, 16, 24, 32} that holds its columns
struct KdeLaunch {
    int kernel, d, cb;
    const double* X;   // [d][ldx] samples
    int64_t ldx;
    const double* V;   // [ldx][cb] weights of the pass
    const double* Q;   // [d][ldq] queries
    int64_t ldq, M;
    double coef;       // gaussian: -S log2(e) / 2h^2 (times r^2), exponential: -S log2(e) / h (times r); S = 2^EXP2_BITS
    double h, inv_h, inv_h2;
    int64_t qblocks, nchunks, chunk;  // grid: 256 queries x `chunk` samples per workgroup
    double* part;      // [nchunks][cb + 1][ldq]
};
size_t kde_lds_bytes(int kernel, int d, int cb);
hipError_t launch_kde(hipStream_t s, const KdeLaunch& a);
// out[q * cv + c] = log density of query q, column c < cv; flag[q * cv + c] = 1: recompute with launch_kde_exact
hipError_t launch_kde_combine(hipStream_t s, const KdeLaunch& a, int cv, const double* logW, double lognorm, double* out, int* flag);
// pq: [npairs][2] (query, column of the pass); out[i]: the log density of pair i
hipError_t launch_kde_exact(hipStream_t s, const KdeLaunch& a, int64_t N, int64_t npairs, const int64_t* pq, const double* logW,
                            double lognorm, double* out);

}  // namespace mbar
