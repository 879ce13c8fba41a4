// ---- the scan kernels (mbar_k_scan.hip); the fill kernel of mbar_k_family.hip follows the same chain --------------------------
#ifndef MBAR_SCAN_DEVICE_H
#define MBAR_SCAN_DEVICE_H
#include "mbar_scan.h"

#include <type_traits>

namespace mbar {

// One term of a member's chain, THE statement of it on the device: the fill kernels and both scan passes come through here, so a
// scan member with a sampled state's parameters has that state's row to the bit.  u: the chain so far, v = basis[b][n], c: the
// member's centre of term b (read at a harmonic term only).  The kind of term b is wave-uniform (terms.mask); the linear family
// is the one fma it always was.  Every operation is rounded once: rint is v_rndne_f64 (ties to even), a tie dl = +-P / 2 gives the
// same dl dl either way.
// (the forms with a last argument also hand out what the term was made of, for the moments of mbar_scan_moments: v itself at a
// linear term, the wrapped displacement dl at a harmonic one; the forms without it are the same operations)
__device__ __forceinline__ double family_term(const ScanLinear&, int, double u, double cf, double v, double, double& dl) {
    dl = v;
    return fma(cf, v, u);
}
__device__ __forceinline__ double family_term(const FamilyTerms& terms, int b, double u, double cf, double v, double c, double& dl) {
#pragma clang fp contract(off)
    dl = v;
    if (!((terms.mask >> b) & 1u)) return fma(cf, v, u);
    dl = v - c;
    const double P = terms.period[b];
    if (P > 0.0) {
        const double m = rint(dl * terms.rperiod[b]);
        dl = fma(-P, m, dl);
    }
    const double q = dl * dl;
    return fma(cf, q, u);
}
__device__ __forceinline__ double family_term(const ScanHarmonic& fam, int b, double u, double cf, double v, double c, double& dl) {
    return family_term(fam.terms, b, u, cf, v, c, dl);
}
template <class Terms>
__device__ __forceinline__ double family_term(const Terms& terms, int b, double u, double cf, double v, double c) {
    double dl;
    return family_term(terms, b, u, cf, v, c, dl);
}
// the centre of term b among a member's centres in registers (cen: the harmonic terms' in ascending b); the slot is wave-uniform
__device__ __forceinline__ double family_center(const ScanLinear&, int, const double (&)[SCAN_MAX_H]) { return 0.0; }
__device__ __forceinline__ double family_center(const ScanHarmonic& fam, int b, const double (&cen)[SCAN_MAX_H]) {
    const int s = __popc(fam.terms.mask & ((1u << b) - 1u));
    // (the four values are read BEFORE the choice: a choice among the loads themselves is folded into one load at a computed
    // index, and the array then lives in scratch)
    const double c0 = cen[0], c1 = cen[1], c2 = cen[2], c3 = cen[3];
    double c = c3;
    c = s == 2 ? c2 : c;
    c = s == 1 ? c1 : c;
    c = s == 0 ? c0 : c;
    return c;
}
// a member's centres from center[l][SCAN_MAX_H] (zeros for a member that is not live, and in the linear family)
__device__ __forceinline__ void family_load_centers(const ScanLinear&, bool, int64_t, double (&cen)[SCAN_MAX_H]) {
#pragma unroll
    for (int h = 0; h < SCAN_MAX_H; ++h) cen[h] = 0.0;
}
__device__ __forceinline__ void family_load_centers(const ScanHarmonic& fam, bool live, int64_t l, double (&cen)[SCAN_MAX_H]) {
#pragma unroll
    for (int h = 0; h < SCAN_MAX_H; ++h) cen[h] = live ? fam.center[l * SCAN_MAX_H + h] : 0.0;
}

// u_l(n) with the fixed chain over ascending b, and x_ln = -u_l(n) - logden_n from it
// (dl[b]: basis[b][n] of a linear term, the wrapped displacement of a harmonic one, 0 for b >= B; NB: the terms the caller's
// instantiation serves, B <= NB)
template <int NB, class Fam>
__device__ __forceinline__ double scan_u(const ScanData& d, const Fam& fam, const double (&cf)[NB], const double (&cen)[SCAN_MAX_H],
                                         double off, int64_t n, double (&dl)[NB]) {
    double u = off;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        dl[b] = 0.0;
        if (b < d.B) u = family_term(fam, b, u, cf[b], d.basis[(int64_t)b * d.ldv + n], family_center(fam, b, cen), dl[b]);
    }
    return u;
}
template <class Fam>
__device__ __forceinline__ double scan_u(const ScanData& d, const Fam& fam, const double (&cf)[SCAN_MAX_B], const double (&cen)[SCAN_MAX_H],
                                         double off, int64_t n) {
    double dl[SCAN_MAX_B];
    return scan_u(d, fam, cf, cen, off, n, dl);
}
__device__ __forceinline__ double scan_x_of(const ScanData& d, double u, int64_t n) { return -u - d.logden[n]; }

// The trailing arguments of a sweep kernel: a policy that carries data (ScanHarmonic, ScanEnergy) travels as one, an empty one
// (ScanLinear, ScanStored) as none, so that its kernels keep the argument block they had before the other kind existed.  The T
// among them, or T{}.
template <class T>
__device__ __forceinline__ T scan_arg() { return T{}; }
template <class T, class A0, class... A>
__device__ __forceinline__ T scan_arg(const A0& a0, const A&... a) {
    if constexpr (std::is_same<T, A0>::value) return a0;
    else return scan_arg<T>(a...);
}

}  // namespace mbar
#endif  // MBAR_SCAN_DEVICE_H
