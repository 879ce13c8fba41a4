// gfx950 (CDNA4 / MI355X) kernel that writes rows of the resident matrix from a family of states (mbar_ctx_fill_family_rows and
// mbar_ctx_fill_linear_rows, MBAR.from_family and MBAR.from_linear): B <= 8 parameters per row and B shared N-vectors instead of a
// row of N doubles over the bus.  Row r of the call is
//
//   u_r(n) = offset[r] + sum_b term_b(r, n),  b ascending            linear term    fma(coeff[r][b], basis[b][n], u)
//                                                                     harmonic term  dl = basis[b][n] - center[r][b]
//                                                                                    P_b > 0: dl = fma(-P_b, rint(dl rP_b), dl)
//                                                                                    fma(coeff[r][b], dl dl, u)
//
// the chain of family_term (mbar_scan_device.h), which the scan passes of mbar_k_scan.hip evaluate too: a scan member with a sampled
// state's parameters has that state's u to the bit.  A harmonic term is umbrella sampling on a periodic coordinate, u_r(n) = beta_r
// [E_n + kappa_r / 2 wrap(chi_n - chi0_r)^2].  One of the translation units of libmbar_hip.so; the host side is mbar_rows.cpp, the
// launcher declaration is in mbar_scan.h.  DESIGN.md section 19 has the geometry and the byte counts, section 20 the chain and its cost.
//
// Store-bound: 8 nrows N bytes out, 8 B N in per row group.  A lane owns the two adjacent columns 2 p, 2 p + 1 (the row pitch is a
// multiple of 16 doubles and the matrix starts on an allocation, so the pair is one aligned 16-byte store), reads its 2 B basis
// values once and keeps them in registers while it walks the FILL_ROWS rows of the group (blockIdx.y); the parameters of a row are
// wave-uniform (scalar loads).  The pairs go round a grid of at most FILL_MAX_BLOCKS workgroups.  An odd N leaves one column
// behind the whole pairs: the first workgroup of every row group writes it, one thread per row (FILL_ROWS <= FILL_THREADS).
// Nothing is written at or behind column N (the padding up to the pitch stays zero) or outside the nrows rows.
//
// Two policies, chosen by the launcher on terms.mask as the scan passes choose theirs.  ScanLinear, a family without a harmonic
// term: one fma per term, and no trace of the other kind -- center is never read (it may be NULL), there is no mask test, the row
// loop is unrolled by 4.  FamilyTerms: the kind of a term is wave-uniform too (terms.mask, a kernel argument: a scalar branch per
// term, no divergence), a harmonic term costs six fp64 operations per element instead of one against the 8 bytes stored, and the
// row loop is unrolled by 2.
#include "mbar_device.h"
#include "mbar_scan_device.h"

#pragma clang fp contract(off)

namespace mbar {

// what the two policies do not share: the rows of one trip of the row loop, and whether a row has centres at all
template <class Terms> struct FillPolicy;
template <> struct FillPolicy<ScanLinear> {
    static constexpr int unroll = 4;
    static __device__ __forceinline__ double center(const double*, int64_t) { return 0.0; }
};
template <> struct FillPolicy<FamilyTerms> {
    static constexpr int unroll = 2;
    static __device__ __forceinline__ double center(const double* center, int64_t i) { return center[i]; }
};

template <int B, class Terms>
__global__ void __launch_bounds__(FILL_THREADS)
k_fill_rows(double* __restrict__ rows, int64_t ld, int64_t N, int64_t nrows, const double* __restrict__ basis, int64_t ldb,
            const double* __restrict__ coeff, const double* __restrict__ center, const double* __restrict__ offset, Terms terms) {
    using Policy = FillPolicy<Terms>;
    const int64_t r0 = (int64_t)blockIdx.y * FILL_ROWS;
    const int64_t r1 = r0 + FILL_ROWS < nrows ? r0 + FILL_ROWS : nrows;
    const int64_t npairs = N >> 1;  // whole pairs; the last column of an odd N follows the loop
    for (int64_t p = (int64_t)blockIdx.x * FILL_THREADS + threadIdx.x; p < npairs; p += (int64_t)gridDim.x * FILL_THREADS) {
        const int64_t n = 2 * p;  // the lane's pair of columns
        double2 bv[B];
#pragma unroll
        for (int b = 0; b < B; ++b) bv[b] = *reinterpret_cast<const double2*>(basis + (int64_t)b * ldb + n);
        double* dst = rows + r0 * ld + n;
#pragma unroll Policy::unroll
        for (int64_t r = r0; r < r1; ++r, dst += ld) {  // (r is wave-uniform: coeff, center and offset come through scalar loads)
            double x0 = offset[r], x1 = x0;
#pragma unroll
            for (int b = 0; b < B; ++b) {
                const double cf = coeff[r * B + b], c = Policy::center(center, r * B + b);
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
            for (int b = 0; b < B; ++b)
                x = family_term(terms, b, x, coeff[r * B + b], basis[(int64_t)b * ldb + n], Policy::center(center, r * B + b));
            rows[r * ld + n] = x;
        }
    }
}

template <class Terms>
static void fill_launch(hipStream_t s, dim3 grid, double* rows, int64_t ld, int64_t N, int64_t nrows, int B, const double* basis,
                        int64_t ldb, const double* coeff, const double* center, const double* offset, const Terms& terms) {
    switch (B) {
#define MBAR_CASE(B_)                                                                                                             \
    case B_:                                                                                                                      \
        hipLaunchKernelGGL((k_fill_rows<B_, Terms>), grid, dim3(FILL_THREADS), 0, s, rows, ld, N, nrows, basis, ldb, coeff, center, \
                           offset, terms);                                                                                        \
        break;
        MBAR_CASE(1) MBAR_CASE(2) MBAR_CASE(3) MBAR_CASE(4) MBAR_CASE(5) MBAR_CASE(6) MBAR_CASE(7) MBAR_CASE(8)
#undef MBAR_CASE
    }
}

// rows, basis: 16-byte aligned, ld and ldb even (the pair loads and stores); 1 <= B <= SCAN_MAX_B, N >= 1, nrows >= 1
hipError_t launch_fill_rows(hipStream_t s, double* rows, int64_t ld, int64_t N, int64_t nrows, int B, const double* basis, int64_t ldb,
                            const double* coeff, const double* center, const double* offset, const FamilyTerms& terms) {
    if (B < 1 || B > SCAN_MAX_B || N < 1 || nrows < 1 || (ld & 1) || (ldb & 1) || ld < N || ldb < N) return hipErrorInvalidValue;
    if (terms.mask >> B || (terms.mask && !center)) return hipErrorInvalidValue;
    static_assert(FILL_ROWS <= FILL_THREADS, "the odd column is written by one thread per row of the group");
    const int64_t want = (N / 2 + FILL_THREADS - 1) / FILL_THREADS;
    const dim3 grid((unsigned)(want < 1 ? 1 : want < FILL_MAX_BLOCKS ? want : FILL_MAX_BLOCKS), (unsigned)((nrows + FILL_ROWS - 1) / FILL_ROWS));
    if (terms.mask)
        fill_launch(s, grid, rows, ld, N, nrows, B, basis, ldb, coeff, center, offset, terms);
    else
        fill_launch(s, grid, rows, ld, N, nrows, B, basis, ldb, coeff, center, offset, ScanLinear{});
    return hipGetLastError();
}

}  // namespace mbar
