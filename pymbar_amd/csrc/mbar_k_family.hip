// gfx950 (CDNA4 / MI355X) kernel that writes rows of the resident matrix from a family with HARMONIC terms
// (mbar_ctx_fill_family_rows, MBAR.from_family): umbrella sampling on a periodic coordinate, u_r(n) = beta_r [E_n + kappa_r / 2
// wrap(chi_n - chi0_r)^2].  Row r of the call is
//
//   u_r(n) = offset[r] + sum_b term_b(r, n),  b ascending            linear term    fma(coeff[r][b], basis[b][n], u)
//                                                                     harmonic term  dl = basis[b][n] - center[r][b]
//                                                                                    P_b > 0: dl = fma(-P_b, rint(dl rP_b), dl)
//                                                                                    fma(coeff[r][b], dl dl, u)
//
// the chain of family_term (mbar_device.h), which the scan passes of mbar_k_scan.hip evaluate too: a scan member with a sampled
// state's parameters has that state's u to the bit.  One of the translation units of libmbar_hip.so; the host side is
// mbar_capi.cpp, the launcher declaration is in mbar_internal.h.  DESIGN.md section 20 has the chain and its cost.
//
// The geometry is that of k_fill_linear_rows (mbar_k_linear.hip), store-bound: a lane owns the two adjacent columns 2 p, 2 p + 1 (one
// aligned 16-byte store), reads its 2 B basis values once and keeps them while it walks the FILL_ROWS rows of the group
// (blockIdx.y); coeff, center and offset of a row are wave-uniform (scalar loads), and so is the kind of a term (terms.mask, a
// kernel argument: a scalar branch per term, no divergence).  A harmonic term costs six fp64 operations per element instead of one
// against the 8 bytes stored.  An odd N leaves one column behind the whole pairs: the first workgroup of every row group writes it,
// one thread per row.  Nothing is written at or behind column N (the padding up to the pitch stays zero) or outside the nrows rows.
#include "mbar_device.h"

#pragma clang fp contract(off)

namespace mbar {

template <int B>
__global__ void __launch_bounds__(FILL_THREADS)
k_fill_family_rows(double* __restrict__ rows, int64_t ld, int64_t N, int64_t nrows, const double* __restrict__ basis, int64_t ldb,
                   const double* __restrict__ coeff, const double* __restrict__ center, const double* __restrict__ offset,
                   FamilyTerms terms) {
    const int64_t r0 = (int64_t)blockIdx.y * FILL_ROWS;
    const int64_t r1 = r0 + FILL_ROWS < nrows ? r0 + FILL_ROWS : nrows;
    const int64_t npairs = N >> 1;  // whole pairs; the last column of an odd N follows the loop
    for (int64_t p = (int64_t)blockIdx.x * FILL_THREADS + threadIdx.x; p < npairs; p += (int64_t)gridDim.x * FILL_THREADS) {
        double2 bv[B];
#pragma unroll
        for (int b = 0; b < B; ++b) bv[b] = *reinterpret_cast<const double2*>(basis + (int64_t)b * ldb + 2 * p);
        double* dst = rows + r0 * ld + 2 * p;
#pragma unroll 2
        for (int64_t r = r0; r < r1; ++r, dst += ld) {  // (r is wave-uniform: coeff, center and offset come through scalar loads)
            double x0 = offset[r], x1 = x0;
#pragma unroll
            for (int b = 0; b < B; ++b) {
                const double cf = coeff[r * B + b], c = center[r * B + b];
                x0 = family_term(terms, b, x0, cf, bv[b].x, c);
                x1 = family_term(terms, b, x1, cf, bv[b].y, c);
            }
            *reinterpret_cast<double2*>(dst) = make_double2(x0, x1);
        }
    }
    if ((N & 1) && blockIdx.x == 0) {  // column N - 1 of an odd N: one 8-byte store per row, thread = row of the group
        const int64_t n = N - 1, r = r0 + threadIdx.x;
        if (r < r1) {
            double x = offset[r];
#pragma unroll
            for (int b = 0; b < B; ++b) x = family_term(terms, b, x, coeff[r * B + b], basis[(int64_t)b * ldb + n], center[r * B + b]);
            rows[r * ld + n] = x;
        }
    }
}

template <int B>
static void fill_family_launch(hipStream_t s, dim3 grid, double* rows, int64_t ld, int64_t N, int64_t nrows, const double* basis,
                               int64_t ldb, const double* coeff, const double* center, const double* offset, const FamilyTerms& terms) {
    hipLaunchKernelGGL(k_fill_family_rows<B>, grid, dim3(FILL_THREADS), 0, s, rows, ld, N, nrows, basis, ldb, coeff, center, offset, terms);
}

// rows, basis: 16-byte aligned, ld and ldb even (the pair loads and stores); 1 <= B <= SCAN_MAX_B, N >= 1, nrows >= 1
hipError_t launch_fill_family_rows(hipStream_t s, double* rows, int64_t ld, int64_t N, int64_t nrows, int B, const double* basis,
                                   int64_t ldb, const double* coeff, const double* center, const double* offset, const FamilyTerms& terms) {
    if (B < 1 || B > SCAN_MAX_B || N < 1 || nrows < 1 || (ld & 1) || (ldb & 1) || ld < N || ldb < N) return hipErrorInvalidValue;
    if (terms.mask >> B) return hipErrorInvalidValue;
    static_assert(FILL_ROWS <= FILL_THREADS, "the odd column is written by one thread per row of the group");
    const int64_t want = (N / 2 + FILL_THREADS - 1) / FILL_THREADS;
    const dim3 grid((unsigned)(want < 1 ? 1 : want < FILL_MAX_BLOCKS ? want : FILL_MAX_BLOCKS), (unsigned)((nrows + FILL_ROWS - 1) / FILL_ROWS));
    switch (B) {
#define MBAR_CASE(B_) \
    case B_: fill_family_launch<B_>(s, grid, rows, ld, N, nrows, basis, ldb, coeff, center, offset, terms); break;
        MBAR_CASE(1) MBAR_CASE(2) MBAR_CASE(3) MBAR_CASE(4) MBAR_CASE(5) MBAR_CASE(6) MBAR_CASE(7)
        default: fill_family_launch<8>(s, grid, rows, ld, N, nrows, basis, ldb, coeff, center, offset, terms); break;
#undef MBAR_CASE
    }
    return hipGetLastError();
}

}  // namespace mbar
