// ---- histogram bins by label (mbar_k_hist.hip; chunk table and C ABI in mbar_hist.cpp) -------------------------------------
#pragma once
#include "mbar_common.h"

namespace mbar {

constexpr int HIST_SLOTS = 64;            // distinct bins of one chunk: lane s of the chunk's wave owns slot s
constexpr int HIST_NO_SLOT = 255;         // slot of a sample that is in no bin of the sweep
constexpr int HIST_CHUNK_SAMPLES = 2048;  // longest chunk
constexpr int HIST_ROWS = 16;             // matrix rows of one wave of pass B
enum { HIST_MAX = 0, HIST_SUMEXP = 1, HIST_NORM = 2 };
// One sweep over the bins [b0, b1) (labels outside it count as -1): the chunk table of that tile and the per-sample vectors
struct HistSweep {
    int64_t N, nbins, b0, b1, nchunks, nrec;
    const int64_t* chunk_n;    // [nchunks + 1] sample range of chunk c
    const int64_t* chunk_rec;  // [nchunks + 1] record range of chunk c: one record per slot
    const uint8_t* slot;       // [N] chunk-local slot (HIST_NO_SLOT: none)
    const int64_t* bin_ptr;    // [nbins + 1] range in bin_rec of bin i
    const int64_t* bin_rec;    // [nrec] the records of a bin, in chunk order
    const int32_t* label;      // [N]
    const double* v;           // [N] target potential
    const double* logden;      // [N]
    const double* cw;          // [N] multiplicities (NULL: 1)
};
// per-slot records of a per-sample quantity (HIST_MAX / HIST_SUMEXP / HIST_NORM, see k_hist_vec) and their merge per bin
hipError_t launch_hist_vec(hipStream_t s, const HistSweep& h, int mode, const double* bin_in, double* rec_a, double* rec_b);
hipError_t launch_hist_vec_combine(hipStream_t s, const HistSweep& h, int mode, const double* rec_a, const double* rec_b,
                                   const double* binmax, double* out_a, double* out_b);
// part[rec][K] = the chunk's sums of c_n W_nk B_n per slot; cross[k][nbins] = the records of a bin merged in chunk order
hipError_t launch_hist_cross(hipStream_t s, const HistSweep& h, const double* u, int64_t ld, int64_t K, const double* f,
                             const double* f_bins, double* part);
hipError_t launch_hist_cross_combine(hipStream_t s, const HistSweep& h, int64_t K, const double* part, double* cross);

}  // namespace mbar
