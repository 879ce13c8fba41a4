// ---- lagged fluctuation sums of a timeseries (mbar_k_acf.hip; C ABI in mbar_acf.cpp) ----------------------------------------
#pragma once
#include "mbar_common.h"

namespace mbar {

constexpr int ACF_WG = 256;                 // threads per workgroup
constexpr int ACF_R = 8;                     // consecutive positions per thread
constexpr int ACF_TILE = ACF_WG * ACF_R;     // positions per tile (one workgroup); the pitch ldx is a multiple, > T
constexpr int ACF_MAX_LAGS = 64;             // lags per launch (one lag block)
enum : int { ACF_AUTO = 0, ACF_CROSS = 1, ACF_PLAIN = 2 };   // term of a position: A'_n A'_n+t / both A'_n B'_n+t and B'_n A'_n+t / A'_n
enum : int { ACF_RULE_SUFFIX = 0, ACF_RULE_MULTIPLE = 1 };   // stopping rule of every suffix origin / of the one origin of K segments
enum : int { ACF_RUNNING = 0, ACF_STOPPED = 1, ACF_ZERO_VARIANCE = 2, ACF_END = 3 };
struct AcfLaunch {
    int kind, nacc;                 // nacc: accumulators per lag (2 for ACF_CROSS, else 1)
    const double2* A;               // [ldx] A - shift_a as an unevaluated sum hi + lo (exact), zero past T
    const double2* B;               // [ldx] B - shift_b (== A for ACF_AUTO)
    const int* rem;                 // [ldx] positions left in the segment of n (n + t is a valid partner iff t < rem[n]); 0 past T
    int64_t T, ldx, ntiles;
    int nl;                         // lags in this block
    int64_t lag[ACF_MAX_LAGS];      // the block's lags (lag 0: the variance step of the rule)
    int64_t inc[ACF_MAX_LAGS];      // the rule's increment at that lag
    double den[ACF_MAX_LAGS];       // ACF_RULE_MULTIPLE: the number of valid pairs at that lag
    int64_t kbase;                  // schedule index of lag[0] (where the rule records C of origin 0)
    int64_t tile_lo, atile_hi;      // tiles [tile_lo, atile_hi] hold every product of the block
    double2* tot;                   // [nl][nacc][ntiles] tile totals
    double2* off;                   // [nl][nacc][ntiles] sums over the later tiles
};
struct AcfRule {
    int mode, fft;
    int64_t nskip, norig;           // origins o * nskip, o < norig
    int64_t mintime;
    double navg;                    // ACF_RULE_MULTIPLE: weight normaliser; loop while t < tend
    int64_t tend;                   // ACF_RULE_MULTIPLE: max segment length - 1
    const double2* SA;              // [ldx] suffix sums of A' (ACF_RULE_SUFFIX)
    const double2* SB;
    double* g;                      // [norig] running g, then the result
    double* sig2;                   // [norig]
    double2* dA;                    // [norig] suffix mean of A', double-double (zero: ACF_RULE_MULTIPLE)
    double2* dB;
    int* status;                    // [norig] ACF_RUNNING / ACF_STOPPED / ACF_ZERO_VARIANCE / ACF_END
    int64_t* stop;                  // [norig] lag of the stop (ACF_STOPPED: last evaluated; ACF_END: first not evaluated)
    double* ct;                     // C of origin 0 by schedule index (or null)
    int* active;                    // [ntiles] running origins per tile after the block
};
// tile totals of every lag of the block over tiles [tile_lo, atile_hi]
hipError_t launch_acf_tiles(hipStream_t s, const AcfLaunch& a);
// off = sums over the later tiles, in a fixed order
hipError_t launch_acf_scan(hipStream_t s, const AcfLaunch& a);
// the suffix sums Q_t(n) of the tiles [c_lo, c_hi]; written (dd) to out[(j nacc + acc) ldo + idx] for idx = oid[n] >= 0 (all n
// when oid is null)
hipError_t launch_acf_store(hipStream_t s, const AcfLaunch& a, int64_t c_lo, int64_t c_hi, const int* oid, double2* out, int64_t ldo);
// the stopping rule at every running origin of the tiles [c_lo, c_hi], one lag of the block after the other
hipError_t launch_acf_rule(hipStream_t s, const AcfLaunch& a, const AcfRule& r, int64_t c_lo, int64_t c_hi);
// rule state of every origin: the suffix means from SA / SB, g = 1, constant suffixes (s > last_change) zero-variance
hipError_t launch_acf_rule_init(hipStream_t s, const AcfRule& r, int64_t T, int64_t last_change);
// X of the raw sums from the stored Q: suffix mode (the suffix means of origin o), or segment mode (Q(o_i) - Q(o_i+1))
hipError_t launch_acf_finish(hipStream_t s, const AcfLaunch& a, const double2* q, int64_t norig, const int64_t* orig, int segments,
                             const double2* SA, const double2* SB, double* xab, double* xba, int64_t j0);
hipError_t launch_acf_fill_int(hipStream_t s, int* p, int64_t n, int v);
hipError_t launch_acf_scatter_oid(hipStream_t s, int* oid, const int64_t* orig, int64_t norig);

}  // namespace mbar
