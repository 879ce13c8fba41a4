// ---- weighted B-spline moments (mbar_k_bspline.hip; C ABI in mbar_bspline.cpp) ---------------------------------------------
#pragma once
#include "mbar_common.h"

namespace mbar {

constexpr int BSP_MAX_K = 7;             // spline degree
constexpr int BSP_MAX_BASIS = 1024;      // basis functions
constexpr int BSP_MAX_GROUPS = 1024;     // sample groups
constexpr int BSP_MAX_CB = 32;           // weight columns per pass; a pass runs with the smallest of {1, 2, 4, 8, 16, 32} that holds them
constexpr int BSP_SLAB_ENTRIES = 768;    // (cell, column) entries of one wave's LDS slab: 4 slabs + knots stay below 64 KB
struct BsplineLaunch {
    int k, nbasis, cb;
    const double* X;   // [N] samples
    const int* G;      // [N] group labels (NULL: one group)
    const double* V;   // [N][cb] weights of the pass
    int64_t N;
    const double* t;   // [nbasis + k + 1] knots
    int64_t nchunks, chunk;  // grid x: `chunk` samples (a multiple of 256) per workgroup
    int cells, tile_cells, ntiles;  // grid y: tiles of `tile_cells` of the cells = G nbasis output rows
    double* part;      // [nchunks][cells][cb]
};
size_t bspline_lds_bytes(int k, int nbasis, int tile_cells, int cb);
hipError_t launch_bspline(hipStream_t s, const BsplineLaunch& a);
// out[cell * cb + c] = the chunk partials summed in chunk order
hipError_t launch_bspline_combine(hipStream_t s, const BsplineLaunch& a, double* out);

}  // namespace mbar
