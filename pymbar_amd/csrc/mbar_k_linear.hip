// gfx950 (CDNA4 / MI355X) kernel that writes rows of the resident matrix from a linear family (mbar_ctx_fill_linear_rows,
// MBAR.from_linear): row r of the call is the state u_r(n) = sum_b coeff[r][b] basis[b][n] + offset[r], B <= 8 coefficients and
// B shared N-vectors instead of a row of N doubles over the bus.  One of the translation units of libmbar_hip.so; the host side is
// mbar_capi.cpp, the launcher declaration is in mbar_internal.h.  DESIGN.md section 19 has the byte counts.
//
//   rows[r][n] = fma(coeff[r][B-1], basis[B-1][n], ... fma(coeff[r][0], basis[0][n], offset[r]))        0 <= n < N, 0 <= r < nrows
//
// the chain of scan_x (mbar_device.h): from the offset, b ascending, one fma per term, nothing else contracted -- a scan member with
// a sampled state's coefficients has that state's u to the bit.
//
// Store-bound: 8 nrows N bytes out, 8 B N in per row group.  A lane owns the two adjacent columns 2 p, 2 p + 1 (the row pitch is a
// multiple of 16 doubles and the matrix starts on an allocation, so the pair is one aligned 16-byte store), reads its 2 B basis
// values once and keeps them in registers while it walks the FILL_ROWS rows of the group (blockIdx.y); coeff and offset of a row
// are wave-uniform (scalar loads).  The pairs go round a grid of at most FILL_MAX_BLOCKS workgroups.  An odd N leaves one column
// behind the whole pairs: the first workgroup of every row group writes it, one thread per row (FILL_ROWS <= FILL_THREADS).
// Nothing is written at or behind column N (the padding up to the pitch stays zero) or outside the nrows rows.
#include "mbar_device.h"

#pragma clang fp contract(off)

namespace mbar {

template <int B>
__global__ void __launch_bounds__(FILL_THREADS)
k_fill_linear_rows(double* __restrict__ rows, int64_t ld, int64_t N, int64_t nrows, const double* __restrict__ basis, int64_t ldb,
                   const double* __restrict__ coeff, const double* __restrict__ offset) {
    const int64_t r0 = (int64_t)blockIdx.y * FILL_ROWS;
    const int64_t r1 = r0 + FILL_ROWS < nrows ? r0 + FILL_ROWS : nrows;
    const int64_t npairs = N >> 1;  // whole pairs; the last column of an odd N follows the loop
    for (int64_t p = (int64_t)blockIdx.x * FILL_THREADS + threadIdx.x; p < npairs; p += (int64_t)gridDim.x * FILL_THREADS) {
        double2 bv[B];
#pragma unroll
        for (int b = 0; b < B; ++b) bv[b] = *reinterpret_cast<const double2*>(basis + (int64_t)b * ldb + 2 * p);
        double* dst = rows + r0 * ld + 2 * p;
#pragma unroll 4
        for (int64_t r = r0; r < r1; ++r, dst += ld) {  // (r is wave-uniform: coeff and offset come through scalar loads)
            double x0 = offset[r], x1 = x0;
#pragma unroll
            for (int b = 0; b < B; ++b) {
                const double cf = coeff[r * B + b];
                x0 = fma(cf, bv[b].x, x0);
                x1 = fma(cf, bv[b].y, x1);
            }
            *reinterpret_cast<double2*>(dst) = make_double2(x0, x1);
        }
    }
    if ((N & 1) && blockIdx.x == 0) {  // column N - 1 of an odd N: one 8-byte store per row, thread = row of the group
        const int64_t n = N - 1, r = r0 + threadIdx.x;
        if (r < r1) {
            double x = offset[r];
#pragma unroll
            for (int b = 0; b < B; ++b) x = fma(coeff[r * B + b], basis[(int64_t)b * ldb + n], x);
            rows[r * ld + n] = x;
        }
    }
}

template <int B>
static void fill_linear_launch(hipStream_t s, dim3 grid, double* rows, int64_t ld, int64_t N, int64_t nrows, const double* basis,
                               int64_t ldb, const double* coeff, const double* offset) {
    hipLaunchKernelGGL(k_fill_linear_rows<B>, grid, dim3(FILL_THREADS), 0, s, rows, ld, N, nrows, basis, ldb, coeff, offset);
}

// rows, basis: 16-byte aligned, ld and ldb even (the pair loads and stores); 1 <= B <= SCAN_MAX_B, N >= 1, nrows >= 1
hipError_t launch_fill_linear_rows(hipStream_t s, double* rows, int64_t ld, int64_t N, int64_t nrows, int B, const double* basis,
                                   int64_t ldb, const double* coeff, const double* offset) {
    if (B < 1 || B > SCAN_MAX_B || N < 1 || nrows < 1 || (ld & 1) || (ldb & 1) || ld < N || ldb < N) return hipErrorInvalidValue;
    static_assert(FILL_ROWS <= FILL_THREADS, "the odd column is written by one thread per row of the group");
    const int64_t want = (N / 2 + FILL_THREADS - 1) / FILL_THREADS;
    const dim3 grid((unsigned)(want < 1 ? 1 : want < FILL_MAX_BLOCKS ? want : FILL_MAX_BLOCKS), (unsigned)((nrows + FILL_ROWS - 1) / FILL_ROWS));
    switch (B) {
        case 1: fill_linear_launch<1>(s, grid, rows, ld, N, nrows, basis, ldb, coeff, offset); break;
        case 2: fill_linear_launch<2>(s, grid, rows, ld, N, nrows, basis, ldb, coeff, offset); break;
        case 3: fill_linear_launch<3>(s, grid, rows, ld, N, nrows, basis, ldb, coeff, offset); break;
        case 4: fill_linear_launch<4>(s, grid, rows, ld, N, nrows, basis, ldb, coeff, offset); break;
        case 5: fill_linear_launch<5>(s, grid, rows, ld, N, nrows, basis, ldb, coeff, offset); break;
        case 6: fill_linear_launch<6>(s, grid, rows, ld, N, nrows, basis, ldb, coeff, offset); break;
        case 7: fill_linear_launch<7>(s, grid, rows, ld, N, nrows, basis, ldb, coeff, offset); break;
        default: fill_linear_launch<8>(s, grid, rows, ld, N, nrows, basis, ldb, coeff, offset); break;
    }
    return hipGetLastError();
}

}  // namespace mbar
