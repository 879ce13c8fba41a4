// Internal interface between the host side (the mbar_*.cpp files; mbar_ctx.h, their shared header, lists them by role) and the
// gfx950 kernels (mbar_k_*.hip).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mbar_hip.h"

namespace mbar {

constexpr int TS = 16;       // samples per wave tile (one 128-byte line per state row)
constexpr int GROUPS = 4;    // 4-sample MFMA groups per tile
constexpr int MAX_FAST_K = 256;   // fast (LDS-staged, MFMA-layout) kernels handle K <= 256
constexpr int PANEL = 64;    // Gram panel width (states) when K > 128

// Rounded-up state count of the device matrix.
inline int64_t padded_K(int64_t K) {
    if (K <= 128) return (K + 15) / 16 * 16;
    return (K + PANEL - 1) / PANEL * PANEL;
}
// Supported block counts (16 states each) of the fused evaluation kernel.
inline int lse_nb_for(int64_t Kp) {
    static const int nbs[] = {1, 2, 3, 4, 5, 6, 7, 8, 12, 16};
    int need = (int)(Kp / 16);
    for (int nb : nbs) if (nb >= need) return nb;
    return 0;
}

// Bootstrap draws as a counter-based stream (mbar_ctx_draw_bootstrap_weights on the device, mbar_bootstrap_draws on the host: the
// same function of (seed, replicate, slot)): slot j of a state with n samples draws position bootstrap_draw(...) in [0, n).
// Two rounds of the splitmix64 finaliser over key and counter; the range reduction is a 64 x 64 -> high-64 multiply (bias <= n / 2^64).
#if defined(__HIPCC__)
#define MBAR_HD __host__ __device__
#else
#define MBAR_HD
#endif
MBAR_HD inline uint64_t bootstrap_mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
MBAR_HD inline int64_t bootstrap_draw(uint64_t seed, uint64_t replicate, uint64_t slot, uint64_t n) {
    const uint64_t key = bootstrap_mix64(seed + 0x9E3779B97F4A7C15ull * (replicate + 1));
    const uint64_t z = bootstrap_mix64(bootstrap_mix64(key ^ (slot * 0xD1342543DE82EF95ull)) + slot);
    return (int64_t)(((unsigned __int128)z * (unsigned __int128)n) >> 64);
}

// Control words of the device-resident solver loop (ints in device memory).  Kernels that are handed a pointer to them
// exit at once when CTL_DONE is set (iterations enqueued past convergence are no-ops) and pick the logden vector of the
// current f from three rotating slots (base + slot * slot_stride), so that a whole iteration can be enqueued -- or
// replayed from a hipGraph -- without the host knowing which candidate the previous one accepted.
enum : int {
    CTL_SLOT = 0,    // logden slot of the current f
    CTL_DONE = 1,    // 0 = running, 1 = converged, 2 = handed back to the host (CTL_REASON says why), 3 = fused loop paused:
                     // the accepted candidate is not the one whose Gram matrix the sweep speculated on, the host enqueues
                     // the separate Gram sweep and resumes
    CTL_ITER = 2,    // iterations executed
    CTL_SCI = 3,     // ... of which self-consistent steps were accepted
    CTL_NR = 4,      // ... of which Newton-Raphson steps were accepted
    CTL_REASON = 5,  // 1 = Newton system not positive definite, 2 = candidates too far apart for the fused sweep,
                     // 3 = non-finite candidate
    CTL_NEEDGRAM = 6,  // fused sweep: 1 = the accepted candidate's Gram matrix is NOT the speculated one: run the Gram sweep
    CTL_GRAMSWEEPS = 7,  // separate Gram sweeps requested so far
    CTL_SPEC = 8,    // fused sweep: candidate whose Gram matrix the sweep accumulates (always the SECOND multiplier row it is
                     // handed): 1 = Newton-Raphson (default), 0 = self-consistent (while self-consistent steps are forced,
                     // mbar_solvers.py:607 `sci_iter < min_sc_iter`: k_newton then hands the two rows over in swapped order)
    CTL_LIGHT = 9,   // fused loop: 1 = BOTH candidates of the coming sweep already satisfy the stop test (mbar_solvers.py:636) against
                     // the current f, so this iteration is the last whichever of them wins and nobody will need the Gram
                     // matrix the fused sweep would accumulate: the fused sweep returns at once and the plain two-candidate
                     // sweep on P (k_psweep, launched right behind it and idle otherwise) evaluates the candidates instead; the
                     // one-read fused sweep of 129 .. 256 states switches to an evaluation-only body of its own
    CTL_LIGHTS = 10,  // iterations evaluated that way
    CTL_WORDS = 12
};
struct LoopCtl {
    const int* ctl = nullptr;
    int64_t slot_stride = 0;
    // optional: events bound to the kernel dispatch itself (hipExtLaunchKernelGGL): start / stop time stamps of the
    // kernel with no marker packets in the stream (an event record between two kernels costs ~6 us of idle queue)
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
    // the matrix holds no +inf entry: the full 128-state Gram panel may run its exponentials without the clamp
    bool unclamped = false;
    // the matrix handed to the Gram launcher is the resident probability matrix (P mode)
    bool pmode = false;
    // the Gram launch is conditional: the kernel exits at once unless CTL_NEEDGRAM is set (fused-sweep loop)
    bool cond_needgram = false;
    // the evaluation sweep on P is conditional: it exits at once unless CTL_LIGHT is set (last iteration of the fused loop)
    bool light_only = false;
};

struct LaunchGeom {
    int blocks;        // grid size
    int waves;         // waves per block
    int nwaves;        // number of partial records of the main output (per wave, or per tile stream)
    int psum_records;  // number of partial records of the per-state sums (Gram kernels)
    int variant;       // kernel variant chosen (see lse_geometry / gram_geometry)
    size_t lds_bytes;
    int live_blocks = 0;  // k_gram_quad / k_fused_quad: blocks of 16 states that hold real states (0: all of the panel's)
    int balanced = 0;     // few-state kernels: the waves' tile streams start workgroup-major (see lse_small_first_tile)
};

// ---- evaluation pass -------------------------------------------------------------------------
// psum_part: [nwaves][nf][16*nb], obj_part: [nwaves][nf]; logden0/1 may be null (not stored).
// cw: per-sample multiplicities (ld doubles: 1 for plain data, bootstrap counts otherwise, 0 on the padding).
// variant: flags of the specialised kernels the context qualifies for (0x10: few-state kernel, one sample per lane, K <= 32,
// one candidate; 0x20: single-buffer kernel for 129..256 states); the geometry records its choice in LaunchGeom::variant
// (1 = k_lse, one tile stream per wave; 4 = k_lse_small; 5 = k_lse_wide)
LaunchGeom lse_geometry(int nb, int nf, int num_cu, int64_t ntiles, int64_t grid_override, int variant);
hipError_t launch_lse(hipStream_t s, int nb, int nf, const LaunchGeom& g,
                      const double* u, int64_t ld, int64_t N, const double* aden /*[nf][16nb]*/,
                      const double* cw, double* logden0, double* logden1, const double* dn,
                      double* psum_part, double* obj_part, const LoopCtl& lc = LoopCtl());

// ---- Gram pass (known logden) ------------------------------------------------------------------
// Diagonal panel: states [row0, row0+16nb) against themselves, nblk = nb(nb+1)/2 blocks, block b
// enumerates (I,J) with I<=J in row-major order.  Off-diagonal panel pair: nbi x nbj blocks.
// gram_part: [nwaves][nblk][256], psum_part: [nwaves][16*nb] (diag only; may be null for off-diag).
LaunchGeom gram_geometry(int tile_rows, bool diag, int num_cu, int64_t ntiles, int64_t grid_override);
hipError_t launch_gram_diag(hipStream_t s, int nb, const LaunchGeom& g, const double* u,
                            int64_t ld, int64_t N, const double* anum /*indexed from row0*/,
                            const double* logden, int64_t row0, double* gram_part, double* psum_part,
                            const LoopCtl& lc = LoopCtl());
// (pmode: `u` is the resident probability matrix, `logden` the reciprocals 1 / s_n, the anum vectors are not read)
hipError_t launch_gram_thin(hipStream_t s, const LaunchGeom& g, const double* u, int64_t ld, int64_t N, const double* ai,
                            const double* aj, const double* logden, int64_t ri, int64_t rj, double* gp);
hipError_t launch_gram_off(hipStream_t s, int nbj /*4 or 8*/, const LaunchGeom& g, const double* u, int64_t ld,
                           int64_t N, const double* anum_i, const double* anum_j, const double* logden,
                           int64_t row_i0, int64_t row_j0, double* gram_part, bool pmode = false);

// 129 .. 256 states (nbt = 12 or 16 blocks of 16) in ONE read: the four waves of a workgroup share a tile stream and split
// the nbt (nbt + 1) / 2 upper-triangular blocks; gram_part: [blocks][nblk][256], block b = (I, J), I <= J, row-major.
// LDS-DMA staging only.  lc.pmode: `u` is the resident probability matrix, `logden` the reciprocals 1 / s_n.
LaunchGeom gram_quad_geometry(int nbt, int num_cu, int64_t ntiles, int64_t grid_override);
// Pout (classic operands only): the operand tiles exp(anum - u - logden) are also written out there (the probability matrix)
// P mode only: nbi (4 / 8) x 16 blocks between the panels at rows ri and rj of the resident probability matrix, see k_gram_rect
hipError_t launch_gram_rect(hipStream_t s, int nbi, const LaunchGeom& g, const double* P, int64_t ld, int64_t N, int64_t ri, int64_t rj,
                            const double* rinv, double* gram_part);
hipError_t launch_gram_quad(hipStream_t s, int nbt, const LaunchGeom& g, const double* u, int64_t ld, int64_t N,
                            const double* anum, const double* logden, double* gram_part, const LoopCtl& lc = LoopCtl(),
                            double* Pout = nullptr);
hipError_t launch_gram_quad_split(hipStream_t s, int nbt, const LaunchGeom& g, const double* u, int64_t ld, int64_t N, const double* anum,
                                  const double* logden, double* gram_part, int64_t split_rows, int64_t row_j0);

// ---- layout-agnostic fallbacks (any K) ---------------------------------------------------------
// 257 .. 512 states in one read: nf = 2 evaluates a second candidate through the ratio row aden[rows + k] = exp(a'_k - a_k)
// (per-state sums without that factor); psum_part [blocks][nf][rows], obj_part [blocks][nf]
hipError_t launch_lse_split(hipStream_t s, int num_cu, int nf, const double* u, int64_t ld, int64_t N, int64_t rows, const double* aden,
                            const double* cw, double* logden, double* logden1, const double* dn, double* psum_part, double* obj_part,
                            int* blocks_out, const double* ld_anchor = nullptr /* P mode: u = P, aden = multipliers, see k_lse_split */);
hipError_t launch_lse_generic(hipStream_t s, int num_cu, const double* u, int64_t ld, int64_t N, int64_t K,
                              const double* aden, const double* cw, double* logden, const double* dn,
                              double* obj_part /*[blocks]*/, int* blocks_out);
hipError_t launch_colsum_generic(hipStream_t s, int num_cu, const double* u, int64_t ld, int64_t N, int64_t K,
                                 const double* anum, const double* cw, const double* logden,
                                 double* psum_part /*[blocks_x][K]*/, int* blocks_out);

// ---- few states: a whole self-consistent iteration in one launch (mbar_k_eval.hip) ------------------------------------------
// Few states (K <= 32, single rank): update + sweep of ONE self-consistent iteration in one launch (k_sci_small).  Double
// buffers by parity p of the iteration: the launch reads rec[p ^ 1] (nrec records of 16 nb doubles: the per-state sums of the
// previous sweep, one per workgroup of the SAME geometry) and state[p ^ 1] (the previous f), writes rec[p], state[p], the
// history row and the relative change.
struct SciLoopArgs {
    const double* Nk;
    const double* lnNk;
    int K;
    int first;        // gauge state
    double tol;
    double* state;    // [2][16 nb]
    double* rec;      // [2][nrec][16 nb]
    int64_t nrec;
    double* f_hist;   // [16 nb] row of the batch history this iteration fills
    double* delta_out;
    int parity;
    uint32_t live;    // bit j: rows 2j, 2j+1 hold a state with samples (the others are not streamed from HBM)
    int balanced;     // tile streams start workgroup-major (LaunchGeom::balanced; the previous sweep's records do not care)
    int pingpong;     // odd iterations sweep the tiles in descending order (cache re-use between consecutive sweeps)
    long long* stamps;  // MBAR_DEBUG_STAMPS: [2][8] phase stamps (100 MHz) of thread 0 of workgroups 0 and gridDim.x / 2, or nullptr
};
hipError_t launch_sci_small(hipStream_t s, int nb, const LaunchGeom& g, const double* u, int64_t ld, int64_t N, const double* cw,
                            const SciLoopArgs& q);

// ---- mbar_k_rows.hip: passes over N-vectors, matrix rows and partial records -------------------------------------------------
// out[i] = sum_p part[p*count + i]; scratch must hold ceil(nparts/32)*count doubles.
hipError_t launch_reduce(hipStream_t s, const double* part, int64_t nparts, int64_t count,
                         double* scratch, double* out);
hipError_t launch_reduce_level1(hipStream_t s, const double* part, int64_t nparts, int64_t count, double* out,
                                int64_t* nchunks);
// Two partial-record arrays with the same number of records reduced by one pair of launches (same summation order as
// launch_reduce on each): outA[i] = sum_p partA[p*countA + i], outB likewise.  scratch: ceil(nparts/32)*(countA+countB).
hipError_t launch_reduce2(hipStream_t s, const double* partA, int64_t countA, const double* partB, int64_t countB,
                          int64_t nparts, double* scratch, double* outA, double* outB);
// robust per-state log-sum-exp over n of (anum_k - u_kn - logden_n): partial (max,sum) per chunk
hipError_t launch_lognum(hipStream_t s, const double* u, int64_t ld, int64_t N, int64_t K,
                         const double* anum, const double* logden,
                         double* pmax /*[K][nchunks]*/, double* psum /*[K][nchunks]*/, int64_t nchunks);
int64_t lognum_chunks(int64_t N, int64_t K);
hipError_t launch_lognum_merge(hipStream_t s, const double* pmax, const double* psum, int64_t K,
                               int64_t nchunks, double* out_max /*[K]*/, double* out_sum /*[K]*/);
hipError_t launch_logw(hipStream_t s, const double* u, int64_t ld, int64_t N, int64_t K,
                       const double* f, const double* logden, double* out, int64_t ld_out, bool exponentiate = false);
// flags |= 1 if any u[k][n] is NaN, |= 2 if any is -inf (k < K, n < N)
hipError_t launch_check_u(hipStream_t s, const double* u, int64_t ld, int64_t N, int64_t K, int* flags);
// out[n] = logden[n] - alpha ln cw[n] (+inf where cw = 0)
hipError_t launch_shift_logden(hipStream_t s, const double* logden, const double* cw, double alpha, int64_t N,
                               double* out, const LoopCtl& lc = LoopCtl());
hipError_t launch_fill(hipStream_t s, double* v, double value, int64_t n);
// zero fill at HBM write speed (hipMemsetAsync below 64 KB or for unaligned ranges)
hipError_t launch_zero(hipStream_t s, void* p, size_t bytes);
hipError_t launch_sqrt_vec(hipStream_t s, double* dst, const double* src, int64_t n);  // dst[i] = sqrt(src[i])
// (*overflow, zeroed by the caller, is set when a weight is not finite)
hipError_t launch_weights_from_log(hipStream_t s, const double* v, double p, int64_t n, double* cw, double* cwsq, int* overflow);
hipError_t launch_generate_harmonic(hipStream_t s, double* u, int64_t ld, int64_t N, int64_t K,
                                    uint64_t seed, const double* O_k, const double* K_k,
                                    const int64_t* cumN /*[K+1]*/, int64_t n_global0);
// cw[sample] += 1 for every draw of the replicate whose sample lies in this shard [n0, n0 + N) (cw zeroed by the caller; the adds are
// of exact small integers: order-independent).  cum: [K + 1] positions of the states' runs; order: sample index of a position, or NULL
hipError_t launch_bootstrap_counts(hipStream_t s, uint64_t seed, int64_t replicate, const int64_t* cum, int64_t K, int64_t total,
                                   const int64_t* order, int64_t n0, int64_t N, double* cw);
hipError_t launch_mfma_peak(hipStream_t s, int blocks, int iters, double* sink);
// 129 .. 256 states: P = exp(aden_k - u_kn - logden_n) (rows = padded state count; padding and sub-normal entries: 0)
hipError_t launch_make_p(hipStream_t s, int num_cu, const double* u, int64_t ld, int64_t N, int64_t rows, const double* aden,
                         const double* logden, double* P);
// rows[i][k] = label[k] == i ? v[k] : +inf,  i < nrows (row pitch ld)
hipError_t launch_fill_masked_rows(hipStream_t s, double* rows, int64_t ld, int64_t n, int64_t nrows, const double* v,
                                   const int* label);
hipError_t launch_row_sub(hipStream_t s, double* row, const double* v, int64_t n);  // row[i] -= v[i]
hipError_t launch_rows_sub(hipStream_t s, double* dst, const double* src, int64_t ld, int64_t nrows, const double* v, int64_t n);
hipError_t launch_rows_rsub(hipStream_t s, double* dst, const double* src, int64_t ld, int64_t nrows, int64_t n);
// rows r < nrows of base (pitch ld, n valid entries): row <- log(row - shift_r), shift_r = min_r - |4 eps min_r| -> shift_out[r]
// (device); part: scratch of 256 * nrows doubles
hipError_t launch_rows_logshift(hipStream_t s, double* base, int64_t ld, int64_t nrows, int64_t n, double* part, double* shift_out);
hipError_t launch_rows_obs(hipStream_t s, double* dst, const double* obs, const double* state, int64_t ld, int64_t nrows, int64_t n,
                           double* part, double* shift_out, bool have_min = false);

// ---- mbar_k_loop.hip: the K x K work of the solver loops --------------------------------------------------------------------
// device-resident SCI step: sums `nparts` partial psum records (row pitch `rows`), then
// f' = f - log(psum/N_k) on sampled states, gauge, aden' = f' + ln N_k; f' also goes to f_hist
hipError_t launch_sci_update(hipStream_t s, const double* part, int64_t nparts, int64_t rows, const double* Nk,
                             const double* lnNk, int64_t K, int64_t Kp, int first_state, double tol, double* f,
                             double* aden, double* f_hist, double* delta_out);
// In-process all-reduce (several contexts of one process on one device): out[i] = op over the ranks' buffers, in rank order
struct LoopSrc {
    const double* p[8];
    int n;
};
hipError_t launch_loop_reduce(hipStream_t s, const LoopSrc& src, int64_t count, int op /*0 sum, 1 max*/, double* out);

// Device-resident adaptive iteration (mbar_solvers.py:575-640 without the host in the loop).
// State of one solve, all in device memory.  Up to 128 padded states (one diagonal Gram panel).
struct AdaptArgs {
    const double* gram_red;  // reduced Gram blocks of the panel, block b = (I, J), I <= J, row-major 16 x 16 each
    const double* lse_red;   // reduced outputs of the two-candidate sweep: psum[2][Kp], then 2 objective sums
    double* f;               // [Kp] current free energies
    double* psum;            // [Kp] sum_n p_nk at f
    double* cand;            // [2][Kp] f_sci, f_nr
    double* ratio;           // [Kp] exp(aden_nr - aden_sci): the fused sweep returns the second candidate's sums unscaled
    double* aden;            // [2][Kp] input of the sweep: aden of f_sci, then ratio
    double* anum;            // [Kp] f + ln N_k (-inf for unsampled / padded states): operand constant of the Gram pass
    const double* Nk;        // [Kp]
    const double* lnNk;      // [Kp]
    const int* sampled;      // [m] states with N_k > 0, ascending
    int m, K, Kp;
    int* ctl;                // CTL_WORDS ints
    const double* prm;       // gamma, tol, min_sc_iter, check_convergence
    double* state;           // [0] max_delta of the last iteration
    double* hist;            // rows of 4 doubles {choice, |g_sci|, |g_nr|, max_delta}
    int64_t hist_cap;
    // P mode: the sweeps work on P = exp(a0 - u - logden(a0)); aden then holds the multipliers exp(a - a0) of BOTH
    // candidates, ccur those of the current f (the Gram kernel returns G with both factors still to be applied)
    int pmode;
    const double* a0;        // [Kp] aden at the build point (-inf for unsampled / padded states)
    double* ccur;            // [Kp]
    // fused sweep: the Gram matrix in gram_red was accumulated with the multipliers cgram (the speculated Newton-Raphson
    // candidate's, or the current f's after a separate Gram sweep)
    int fused;
    double* cgram;           // [Kp]
    // fused loop: the last iteration may run without its Gram matrix (CTL_LIGHT); 0 = never (small problems: an idle launch
    // per iteration would cost more than the one lighter sweep saves)
    int light_ok;
    // MBAR_DEBUG_STAMPS=1: shader-clock stamps of the phases of k_select_newton (thread 0; [16] per launch slot, 64 slots)
    long long* stamps;
    // K x K Newton solve up to 128 states: 1 = blocked LDL^T on the matrix cores (newton_body_ldlt), 0 = register Gauss-Jordan
    int newton_ldlt;
};
// K x K Newton system (gauge-fixed, Gauss-Jordan in registers, one workgroup) + both candidates + sweep inputs
hipError_t launch_newton(hipStream_t s, const AdaptArgs& a);
// ... for 128 .. 255 unknowns: blocked Cholesky in device memory (a pair of small kernels per block column of 32);
// work: NEWTON_CHOL_WORK doubles
constexpr size_t NEWTON_CHOL_WORK = (size_t)256 * 256 + 8;
hipError_t launch_newton_chol(hipStream_t s, const AdaptArgs& a, double* work);
// gradient norms of both candidates, choice (mbar_solvers.py:607), convergence test (:627-640), next Gram operand
hipError_t launch_select(hipStream_t s, const AdaptArgs& a);
// selection of one iteration + Newton solve of the next in one launch (fused loop, up to 127 unknowns)
hipError_t launch_select_newton(hipStream_t s, const AdaptArgs& a);
// fused loop paused by k_select (CTL_DONE = 3): clear the pause and the Gram request (in front of the Gram sweep)
hipError_t launch_ctl_resume(hipStream_t s, int* ctl);

// ---- P mode: resident probability matrix P = exp(a0 - u - logden(a0)) (see k_psweep) ----------------------------------
LaunchGeom psweep_geometry(int nb, int num_cu, int64_t ntiles, int64_t grid_override);
// cmul: [nf][16 nb] multipliers exp(a - a0); rinv0 = base of the three slot vectors when lc.ctl is set
hipError_t launch_psweep(hipStream_t s, int nb, int nf, const LaunchGeom& g, const double* P, int64_t ld, int64_t N,
                         const double* cmul, const double* cw, double* rinv0, double* rinv1, double* psum_part,
                         const LoopCtl& lc = LoopCtl());
// fused sweep: both candidates' normalisers / per-state sums + the Gram matrix of the second (Newton-Raphson) candidate
// unit: cw is all ones (a context without sample weights) -- up to 128 states the kernel specialised for it runs (same grid, same
// sums to the bit); the geometry and the launch must be given the same value
LaunchGeom fused_geometry(int nb, int num_cu, int64_t ntiles, int64_t grid_override, bool unit = false);
hipError_t launch_fused(hipStream_t s, int nb, const LaunchGeom& g, const double* P, int64_t ld, int64_t N, const double* cmul,
                        const double* cw, const double* wsq, bool unit, double* rinv_base, double* gram_part, double* psum_part,
                        const LoopCtl& lc);
// fused build: the single-candidate sweep at the anchor point (psum partial records [nwaves][16 nb]) that also writes P and
// fills the reciprocal slot with ones
LaunchGeom build_sweep_geometry(int nb, int num_cu, int64_t ntiles, int64_t grid_override);
hipError_t launch_build_sweep(hipStream_t s, int nb, const LaunchGeom& g, const double* u, int64_t ld, int64_t N,
                              const double* aden, const double* cw, double* P, double* rinv_slot, double* psum_part);
// ... and the Gram matrix at the anchor point as well (gram partial records in the fused sweep's per-wave layout and count).  It
// leaves NO per-state sums: they are the row sums of that Gram matrix (host::gram_row_sums on the reduced blocks).  general: the samples
// carry multiplicities (wsq = their square roots; otherwise any vector of ld doubles) or the matrix holds +inf entries.
LaunchGeom build_gram_geometry(int nb, int num_cu, int64_t ntiles, int64_t grid_override);
hipError_t launch_build_gram(hipStream_t s, int nb, const LaunchGeom& g, const double* u, int64_t ld, int64_t N,
                             const double* aden, const double* wsq, bool general, double* P, double* rinv_slot, double* gram_part);
hipError_t launch_rinv_from_logden(hipStream_t s, const double* ld0, const double* ldv, const double* cw, bool weighted, int64_t N,
                                   double* out);
hipError_t launch_rinv_weighted(hipStream_t s, const double* rinv, const double* cw, int64_t N, double* out,
                                const LoopCtl& lc = LoopCtl());


// ---- weighted kernel-density sum (mbar_k_kde.hip; C ABI in mbar_kde.cpp) ---------------------------------------------------
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

// ---- weighted B-spline moments (mbar_k_bspline.hip; C ABI in mbar_bspline.cpp) ---------------------------------------------
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

// ---- histogram bins by label (mbar_k_hist.hip; chunk table and C ABI in mbar_hist.cpp) -------------------------------------
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

// ---- reweighting scans over a linear family of unsampled states, and the histogram surfaces along a scan (mbar_k_scan.hip;
// panels, tables, bin groups and C ABI in mbar_scan.cpp) ------------------------------------------------------------------------
constexpr int SCAN_MAX_B = MBAR_SCAN_MAX_B;  // basis vectors
constexpr int SCAN_MAX_Q = MBAR_SCAN_MAX_Q;  // observables
constexpr int SCAN_VCHUNK = 2048;            // samples of one wave of pass A
constexpr int SCAN_CHUNK = 8192;             // samples of one workgroup of pass B: the cut of N depends on N alone
// blocks of 16 members per wave of pass B for J = 1 + Q operand columns per member, and per-member sums of its vec record
constexpr int scan_mb(int J) { return J == 1 ? 4 : J == 2 ? 2 : 1; }
constexpr int scan_nv(int J) { return 1 + J + J * (J + 1) / 2; }
constexpr int SCANBIN_NV = 2;  // per (member, bin) sums of a binned pass-B record: wsum | diag
struct ScanData {
    int64_t N, ldv;
    int B, Q;
    const double* basis;   // [B][ldv]
    const double* t;       // [Q][ldv] shifted observables (> 0)
    const double* logden;  // [N]
    const double* cw;      // [N] multiplicities (NULL: 1)
};
// The samples sorted by bin (perm: sorted position -> sample, ascending n inside a bin) and cut into chunks that never straddle a
// bin: chunk c of a table belongs to bin chunk_bin[c] and is that bin's chunk number c - bin_chunk0[bin], positions bin_start[bin]
// + chunk number x chunk length onward.  With one bin holding every sample the cut is the cut of the scan passes.
struct ScanBinTable {
    int64_t nchunks = 0;
    const int32_t* chunk_bin = nullptr;   // [nchunks]
    const int64_t* bin_chunk0 = nullptr;  // [nbins + 1]
};
struct ScanBins {
    int64_t nbins;
    const int32_t* perm;       // [bin_start[nbins]]
    const int64_t* bin_start;  // [nbins + 1]
};
// The cut of the samples a launch sums over, the compile-time policy of the kernels: the bins [b0(), b1()) and their chunks
// [c0(), c1()) of at most len positions (chunk c0() writes record 0), the positions [p0, p1) of chunk c and its bin, the sample at
// position p.  The whole cut also carries what only it has, the reference member of pass B.
struct ScanWhole {  // every sample in its own order, as one bin: chunk c is [c len, min(N, (c + 1) len))
    static constexpr bool binned = false;
    int64_t ref = 0;
    MBAR_HD int64_t nbins() const { return 1; }
    MBAR_HD int64_t b0() const { return 0; }
    MBAR_HD int64_t b1() const { return 1; }
    MBAR_HD int64_t c0() const { return 0; }
    MBAR_HD int64_t c1(int64_t N, int64_t len) const { return (N + len - 1) / len; }
    MBAR_HD void bin_chunks(int64_t, int64_t N, int64_t len, int64_t& ca, int64_t& cb) const { ca = 0, cb = c1(N, len); }
    MBAR_HD void range(int64_t c, int64_t N, int64_t len, int64_t& bin, int64_t& p0, int64_t& p1) const {
        bin = 0;
        p0 = c * len;
        p1 = p0 + len < N ? p0 + len : N;
    }
    MBAR_HD int64_t sample(int64_t p) const { return p; }
};
struct ScanBinned {  // the sorted positions of the bins [b0_, b1_), whose chunks in table t are [c0_, c1_)
    static constexpr bool binned = true;
    ScanBins sb;
    ScanBinTable t;
    int64_t b0_, b1_, c0_, c1_;
    MBAR_HD int64_t nbins() const { return sb.nbins; }
    MBAR_HD int64_t b0() const { return b0_; }
    MBAR_HD int64_t b1() const { return b1_; }
    MBAR_HD int64_t c0() const { return c0_; }
    MBAR_HD int64_t c1(int64_t, int64_t) const { return c1_; }
    MBAR_HD void bin_chunks(int64_t bin, int64_t, int64_t, int64_t& ca, int64_t& cb) const { ca = t.bin_chunk0[bin], cb = t.bin_chunk0[bin + 1]; }
    MBAR_HD void range(int64_t c, int64_t, int64_t len, int64_t& bin, int64_t& p0, int64_t& p1) const {
        bin = t.chunk_bin[c];
        const int64_t end = sb.bin_start[bin + 1];
        p0 = sb.bin_start[bin] + (c - t.bin_chunk0[bin]) * len;
        p1 = p0 + len < end ? p0 + len : end;
    }
    MBAR_HD int64_t sample(int64_t p) const { return sb.perm[p]; }
};
// The kind of the terms of a member, the second compile-time policy of the scan kernels (and, as FamilyTerms, the wave-uniform
// argument of the family fill): u_l(n) = offset[l] + sum_b term_b, b ascending, a linear term fma(coeff, basis, u), a harmonic one
//   dl = basis - center;  P > 0: m = rint(dl rP), dl = fma(-P, m, dl);  u = fma(coeff, dl dl, u)
// (family_term in mbar_device.h: every operation rounded once).  ScanLinear is the family of mbar_ctx_set_scan alone: its
// instantiations carry no trace of the other kind.
constexpr int SCAN_MAX_H = MBAR_SCAN_MAX_H;  // harmonic terms
struct FamilyTerms {
    uint32_t mask = 0;           // bit b: term b is harmonic
    double period[SCAN_MAX_B];   // P_b of a harmonic term (0: not periodic)
    double rperiod[SCAN_MAX_B];  // 1.0 / P_b, rounded once on the host (0 where P_b = 0)
};
struct ScanLinear {
    static constexpr bool harmonic = false;
    static constexpr int mb(int J) { return scan_mb(J); }
    MBAR_HD ScanLinear from(int64_t) const { return *this; }
};
struct ScanHarmonic {
    static constexpr bool harmonic = true;
    // narrower panels of pass B than the linear family's: with its members' centres next to the coefficients the widest
    // instantiations (8 blocks of states) would not fit the register file at 4 (J = 1) or 2 (J = 2) blocks of members per wave
    static constexpr int mb(int J) { return J == 1 ? 2 : 1; }
    FamilyTerms terms;
    const double* center;  // [L][SCAN_MAX_H] on the device: the centres of the harmonic terms in ascending b, zeros behind them
    MBAR_HD ScanHarmonic from(int64_t l0) const {  // the family as the members [l0, L) see it
        ScanHarmonic h = *this;
        h.center += l0 * SCAN_MAX_H;
        return h;
    }
};
// Cut = ScanWhole or ScanBinned (Q = 0), Fam = ScanLinear or ScanHarmonic in the two sweeps; the merges know neither kind.
// pass A over the members [0, L) of coeff / offset: per-chunk records of the maxima (sum = false: rec[chunk][L]) or of the J scaled
// sums (rec[chunk][L][J]), and their merge in chunk order into M[bin][L] (bin-major, of this member panel), or into
// lognum[l][bin] (row pitch nbins) and, on the whole cut, mean[L][J]
template <class Cut, class Fam>
hipError_t launch_scan_vec(hipStream_t s, const ScanData& d, const Cut& cut, const Fam& fam, bool sum, int64_t L, const double* coeff,
                           const double* offset, const double* M, double* rec);
template <class Cut>
hipError_t launch_scan_vec_merge(hipStream_t s, const ScanData& d, const Cut& cut, bool sum, int64_t L, const double* rec, double* M,
                                 double* lognum, double* mean);
// pass B for the panel of members [p0, p0 + 64 mb) of L, mb = Fam::mb(J): part[chunk - c0][scan_record_doubles(nb, J, nv, mb)], then
// cross[k][l][bin][j] (K x L x nbins x J) and vec[l][bin][nv].  Whole cut: nv = scan_nv(J), vec = wsum | refcol[J] | within[i <= j],
// fnorm = f_scan[L]; binned cut: J = 1, nv = SCANBIN_NV, vec = wsum | diag, fnorm = f_bins[L][nbins] (+inf: an empty bin of that
// member, exact zeros).  nb = scan_nb_for(K) blocks of 16 states, or 0: no cross block.
int scan_nb_for(int64_t K);
int64_t scan_record_doubles(int nb, int J, int nv, int mb);
template <class Cut, class Fam>
hipError_t launch_scan_cross(hipStream_t s, const ScanData& d, const Cut& cut, const Fam& fam, int nb, const double* u, int64_t ld, int64_t K,
                             const double* f, int64_t L, int64_t p0, const double* coeff, const double* offset, const double* fnorm,
                             double* part);
template <class Cut>
hipError_t launch_scan_cross_merge(hipStream_t s, const ScanData& d, const Cut& cut, int nb, int mb, int64_t K, int64_t L, int64_t p0,
                                   const double* part, double* cross, double* vec);

// ---- rows of the resident matrix from a family of states (mbar_k_family.hip; C ABI: mbar_ctx_fill_family_rows and ----------
// ---- mbar_ctx_fill_linear_rows in mbar_rows.cpp) -----------------------------------------------------------------------------
constexpr int FILL_THREADS = 256;      // a lane owns two adjacent columns: 512 columns per workgroup and pass
constexpr int FILL_ROWS = 128;         // rows a lane writes from one read of its basis values (grid.y = row groups)
constexpr int FILL_MAX_BLOCKS = 2048;  // grid.x; the column pairs go round it
// rows[r][n] = offset[r] + sum_b term_b for r < nrows, n < N: the chain of family_term and scan_x, b ascending.  rows (pitch ld) and
// basis (pitch ldb) 16-byte aligned with even pitches; coeff[nrows][B], center[nrows][B], offset[nrows] on the device.
// terms.mask == 0, every term linear, rows[r][n] = fma(coeff[r][B-1], basis[B-1][n], ... fma(coeff[r][0], basis[0][n], offset[r])):
// the ScanLinear instantiation, which never reads center (NULL will do); otherwise the FamilyTerms one
hipError_t launch_fill_rows(hipStream_t s, double* rows, int64_t ld, int64_t N, int64_t nrows, int B, const double* basis, int64_t ldb,
                            const double* coeff, const double* center, const double* offset, const FamilyTerms& terms);

// ---- lagged fluctuation sums of a timeseries (mbar_k_acf.hip; C ABI in mbar_acf.cpp) ----------------------------------------
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


// ---- BAR root find (mbar_k_bar.hip; C ABI in mbar_bar.cpp) ---------------------------------------------------------------------
// The reference's bracket / false-position / bisection / self-consistent loop (pymbar other_estimators.bar) as a resumable state
// machine: each call consumes F at the previous requests and either issues the next requests (nreq = 1 or 2) or ends (status != 0).
// The same function runs in the step kernel and in mbar_bar_step_host.  Contraction is off so that every operation is the one
// IEEE operation of the reference's Python floats (no fma), in the reference's order.
enum : int64_t { BAR_RUNNING = 0, BAR_DONE = 1, BAR_NAN_BRACKET = 2, BAR_BOUNDS = 3, BAR_NOT_CONVERGED = 4 };
enum : int64_t { BAR_FALSE_POSITION = 0, BAR_BISECTION = 1, BAR_SELF_CONSISTENT = 2 };
enum : int64_t { BAR_PH_INIT = 0, BAR_PH_BRACKET0 = 1, BAR_PH_WIDEN = 2, BAR_PH_LOOP = 3 };

MBAR_HD inline void bar_finish_loop(mbar_bar_state& s, bool broke) {
    // after `for iteration in range(maximum_iterations + 1)`: iteration holds the last value whether the loop broke or not
    if (!broke) s.iteration = s.maximum_iterations;
    s.nreq = 0;
    s.status = (s.iterated && !(s.iteration < s.maximum_iterations)) ? BAR_NOT_CONVERGED : BAR_DONE;
}

MBAR_HD inline int64_t bar_advance(mbar_bar_state& s, const double* F) {
#pragma clang fp contract(off)
    if (s.status != BAR_RUNNING) return s.status;
    const bool bracketed = s.method != BAR_SELF_CONSISTENT;
    switch (s.phase) {
    case BAR_PH_INIT:
        s.DeltaF_initial = s.DeltaF;
        s.iteration = 0;
        s.nzero = 0;
        if (bracketed) {
            s.req[0] = s.UpperB;
            s.req[1] = s.LowerB;
            s.nreq = 2;
            s.phase = BAR_PH_BRACKET0;
            return s.status;
        }
        break;  // to the loop, iteration 0
    case BAR_PH_BRACKET0:
    case BAR_PH_WIDEN: {
        s.FUpperB = F[0];
        s.FLowerB = F[1];
        s.nzero += 2;
        if (s.phase == BAR_PH_BRACKET0 && (s.FUpperB != s.FUpperB || s.FLowerB != s.FLowerB)) {
            s.DeltaF = 0.0;
            s.nreq = 0;
            s.status = BAR_NAN_BRACKET;
            return s.status;
        }
        if (s.FUpperB * s.FLowerB > 0) {
            // widen: max(abs(.), 0.1) keeps its first argument unless 0.1 is larger (Python's max)
            const double FAve = (s.UpperB + s.LowerB) / 2;
            const double du = fabs(s.UpperB - FAve), dl = fabs(s.LowerB - FAve);
            s.UpperB = s.UpperB - (0.1 > du ? 0.1 : du);
            s.LowerB = s.LowerB + (0.1 > dl ? 0.1 : dl);
            s.req[0] = s.UpperB;
            s.req[1] = s.LowerB;
            s.nreq = 2;
            s.phase = BAR_PH_WIDEN;
            return s.status;
        }
        break;  // to the loop, iteration 0
    }
    case BAR_PH_LOOP: {
        // the body of one iteration after its evaluation
        s.nzero += 1;
        if (s.method == BAR_SELF_CONSISTENT) s.DeltaF = -F[0] + s.DeltaF;
        else s.FNew = F[0];
        if (s.method == BAR_FALSE_POSITION && s.FNew == 0) {
            s.relative_change = 1e-15;
            bar_finish_loop(s, true);
            return s.status;
        }
        goto check;
    }
    default:
        s.status = BAR_BOUNDS;
        return s.status;
    }
    // top of the loop at s.iteration
    for (;;) {
        s.DeltaF_old = s.DeltaF;
        if (s.method == BAR_FALSE_POSITION) {
            if (s.LowerB == 0.0 && s.UpperB == 0.0) {
                // no evaluation: FNew = 0 ends the loop
                s.DeltaF = 0.0;
                s.FNew = 0.0;
                s.relative_change = 1e-15;
                bar_finish_loop(s, true);
                return s.status;
            }
            s.DeltaF = s.UpperB - s.FUpperB * (s.UpperB - s.LowerB) / (s.FUpperB - s.FLowerB);
        } else if (s.method == BAR_BISECTION) {
            s.DeltaF = (s.UpperB + s.LowerB) / 2;
        }
        s.req[0] = s.DeltaF;
        s.nreq = 1;
        s.phase = BAR_PH_LOOP;
        return s.status;
    check:
        if (s.DeltaF == 0.0) {
            bar_finish_loop(s, true);
            return s.status;
        }
        if (s.iterated) {
            s.relative_change = fabs((s.DeltaF - s.DeltaF_old) / s.DeltaF);
            if (s.iteration > 0 && s.relative_change < s.relative_tolerance) {
                bar_finish_loop(s, true);
                return s.status;
            }
        }
        if (bracketed) {
            if (s.FUpperB * s.FNew < 0) {
                s.LowerB = s.DeltaF;
                s.FLowerB = s.FNew;
            } else if (s.FLowerB * s.FNew <= 0) {
                s.UpperB = s.DeltaF;
                s.FUpperB = s.FNew;
            } else {
                s.nreq = 0;
                s.status = BAR_BOUNDS;
                return s.status;
            }
        }
        if (s.iteration == s.maximum_iterations) {
            bar_finish_loop(s, false);
            return s.status;
        }
        s.iteration += 1;
    }
}

// Device side.  Values of every side are cut into chunks of MBAR_BAR_CHUNK (chunk c: side seg[c] = 2 p + (0 F, 1 R), values
// [start[c], start[c] + len[c]) of w, minimum wmin[c]); the chunks of one side are consecutive, cbeg[s] .. cbeg[s + 1].
constexpr int BAR_WG = 256;
constexpr int BAR_PER_THREAD = MBAR_BAR_CHUNK / BAR_WG;
struct BarData {
    const double* w;
    const int64_t* start;
    const int* len;
    const int* seg;
    const double* wmin;      // [nchunks] minimum of the chunk (+inf: every value is +inf)
    const int64_t* cbeg;     // [2 P + 1]
    const double* M;         // [P] log(n_F / n_R)
    int64_t P, nchunks;
};
// partial of a chunk at one DeltaF: the shift (hi + lo, -inf for a chunk of +inf values) and the sums of the shifted factors and
// of their squares
struct BarPartial {
    double hi, lo, s1, s2;
};
// evaluation pass: every chunk of every problem still running, at its requests; part[(r * nchunks) + c]
hipError_t launch_bar_eval(hipStream_t st, const BarData& d, const mbar_bar_state* states, BarPartial* part);
// merge of the partials and one step of every running state (advance != 0), or (advance == 0) out[p][5] of the first request
hipError_t launch_bar_step(hipStream_t st, const BarData& d, mbar_bar_state* states, const BarPartial* part, int advance,
                           double* out, int* status);
// one-sided moments of every side: out[s][5] (include/mbar_hip.h, mbar_bar_moments); scratch: [3][nchunks]
hipError_t launch_bar_moments(hipStream_t st, const BarData& d, const int64_t* nside, double* scratch, double* out);

// ---- many small MBAR problems (mbar_k_batch.hip; C ABI in mbar_batch.cpp) ----------------------------------------------------
// The adaptive loop of mbar_solvers.py:575-640 for one problem as a resumable state machine over mbar_batch_state.  A pass
// evaluates, at each of the nreq requested f vectors, lognum_k = log sum_n exp(-logden_n - u_kn) for every state and, at
// req[gram_req], the Gram matrix sum_n p_ni p_nj (p_nk = N_k W_nk).  batch_advance consumes one pass; when it leaves the state in
// BATCH_PH_NEWTON the caller factors H = diag(psum) - Gram of the live states (batch_newton_* below, or the workgroup-parallel
// version of the step kernel), stores the direction in x and calls it again, which forms the next two candidates.  The same
// function runs in k_batch_step and in mbar_batch_step_host.  The unknowns are the sampled states but the first (the gauge
// state s0 of the reduced problem of mbar_solvers.py:1002-1006); unsampled states keep their f and carry no weight.
enum : int64_t { BATCH_RUNNING = 0, BATCH_DONE = 1, BATCH_FALLBACK = 2 };
enum : int64_t { BATCH_PH_INIT = 0, BATCH_PH_GRAM = 1, BATCH_PH_NEWTON = 2, BATCH_PH_CAND = 3, BATCH_PH_LAST = 4, BATCH_PH_FINAL = 5,
                 BATCH_PH_IDLE = 6 };

MBAR_HD inline int batch_first_sampled(const mbar_batch_state& s) {
    for (int k = 0; k < (int)s.K; ++k)
        if (s.Nk[k] > 0) return k;
    return -1;
}
MBAR_HD inline int batch_sampled_count(const mbar_batch_state& s) {
    int m = 0;
    for (int k = 0; k < (int)s.K; ++k) m += s.Nk[k] > 0;
    return m;
}
// psum of the sampled states from lognum at f
MBAR_HD inline void batch_set_point(mbar_batch_state& s, const double* f, const double* lognum) {
#pragma clang fp contract(off)
    for (int k = 0; k < (int)s.K; ++k) {
        s.f[k] = f[k];
        s.lognum[k] = lognum[k];
        s.psum[k] = s.Nk[k] > 0 ? s.Nk[k] * exp(f[k] + lognum[k]) : 0.0;
    }
}
MBAR_HD inline void batch_end(mbar_batch_state& s, int64_t status, int64_t success) {
    s.status = status;
    s.success = success;
    s.nreq = 0;
    s.gram_req = -1;
    s.phase = BATCH_PH_IDLE;
}
// the pass that evaluates f alone (with its Gram matrix when `gram`)
MBAR_HD inline void batch_request_point(mbar_batch_state& s, bool gram, int64_t phase) {
    for (int k = 0; k < (int)s.K; ++k) s.req[0][k] = s.f[k];
    s.nreq = 1;
    s.gram_req = gram ? 0 : -1;
    s.gram_w = 0;
    s.phase = phase;
}

// lognum: [nreq][K] at the requests of the last pass (unused in BATCH_PH_INIT and BATCH_PH_NEWTON)
MBAR_HD inline int64_t batch_advance(mbar_batch_state& s, const double* lognum) {
#pragma clang fp contract(off)
    if (s.status != BATCH_RUNNING) return s.status;
    const int K = (int)s.K;
    const int s0 = batch_first_sampled(s);
    switch (s.phase) {
    case BATCH_PH_INIT: {
        // gauge of mbar_solvers.py:1003-1006 on the sampled states; one sampled state: no solve, f_s0 = 0
        s.iterations = s.nr_iter = s.sci_iter = s.choices = 0;
        s.success = 0;
        s.newton_bad = 0;
        if (s0 < 0) {
            batch_end(s, BATCH_FALLBACK, 0);
            return s.status;
        }
        const double f0 = s.f[s0];
        for (int k = 0; k < K; ++k)
            if (s.Nk[k] > 0) s.f[k] = s.f[k] - f0;
        if (batch_sampled_count(s) == 1 || s.maxiter <= 0) {
            batch_request_point(s, false, BATCH_PH_LAST);
            return s.status;
        }
        batch_request_point(s, true, BATCH_PH_GRAM);
        return s.status;
    }
    case BATCH_PH_LAST: {
        double f[MBAR_BATCH_MAX_K];
        for (int k = 0; k < K; ++k) f[k] = s.f[k];
        batch_set_point(s, f, lognum);
        batch_end(s, BATCH_DONE, batch_sampled_count(s) == 1 ? 1 : 0);
        return s.status;
    }
    case BATCH_PH_GRAM: {
        double f[MBAR_BATCH_MAX_K];
        for (int k = 0; k < K; ++k) f[k] = s.f[k];
        batch_set_point(s, f, lognum);
        s.phase = BATCH_PH_NEWTON;  // the caller factors H at f with the Gram matrix of this pass
        return s.status;
    }
    case BATCH_PH_NEWTON: {
        if (s.newton_bad) {
            batch_end(s, BATCH_FALLBACK, 0);
            return s.status;
        }
        // f_sci = -lognum, re-zeroed on s0 (mbar_solvers.py:587-588); f_nr = f - gamma (H^+ g - (H^+ g)_s0) (:582-584)
        const double z = -s.lognum[s0];
        for (int k = 0; k < K; ++k) {
            const bool live = s.Nk[k] > 0;
            s.req[0][k] = live ? -s.lognum[k] - z : s.f[k];
            s.req[1][k] = (live && k != s0) ? s.f[k] - s.gamma * s.x[k] : s.f[k];
        }
        s.nreq = 2;
        s.gram_w = 0;
        // the Gram matrix of the candidate that will most likely be accepted: Newton-Raphson, unless self-consistent steps are forced
        s.gram_req = s.sci_iter < s.min_sc_iter ? 0 : 1;
        s.phase = BATCH_PH_CAND;
        return s.status;
    }
    case BATCH_PH_CAND: {
        double gn[2] = {0.0, 0.0};
        for (int r = 0; r < 2; ++r)
            for (int k = 0; k < K; ++k)
                if (s.Nk[k] > 0) {
                    const double g = s.Nk[k] * exp(s.req[r][k] + lognum[r * K + k]) - s.Nk[k];
                    gn[r] = gn[r] + g * g;
                }
        s.gnorm_sci = sqrt(gn[0]);
        s.gnorm_nr = sqrt(gn[1]);
        // mbar_solvers.py:607; a NaN Newton-Raphson candidate loses to a finite self-consistent one
        const bool nan_nr = gn[1] != gn[1] && gn[0] == gn[0];
        const int c = (gn[0] < gn[1] || s.sci_iter < s.min_sc_iter || nan_nr) ? 0 : 1;
        // relative change of :627-633 over the sampled states but s0
        double max_delta = -INFINITY, max_diff = -INFINITY;
        bool nan_seen = false;
        const double zcut = 1e-8 < s.tol ? 1e-8 : s.tol;
        for (int k = 0; k < K; ++k) {
            if (!(s.Nk[k] > 0) || k == s0) continue;
            const double fn = s.req[c][k];
            double div = fabs(fn);
            if (div < zcut) div = 1.0;
            const double d = fabs(fn - s.f[k]) / div;
            const double e = fabs(s.req[0][k] - s.req[1][k]) / div;
            if (d != d) nan_seen = true;
            max_delta = d > max_delta ? d : max_delta;
            max_diff = e > max_diff ? e : max_diff;
        }
        if (nan_seen) max_delta = NAN;  // (np.max propagates NaN)
        s.max_delta = max_delta;
        s.max_diff = max_diff;
        if (c == 0) s.sci_iter += 1;
        else {
            s.nr_iter += 1;
            if (s.iterations < 63) s.choices |= (int64_t)1 << s.iterations;
        }
        s.iterations += 1;
        batch_set_point(s, s.req[c], lognum + c * K);
        if (max_delta != max_delta || (max_delta < s.tol && max_diff < sqrt(s.tol))) {
            batch_end(s, BATCH_DONE, 1);
            return s.status;
        }
        if (s.iterations >= s.maxiter) {
            batch_end(s, BATCH_DONE, 0);
            return s.status;
        }
        // the Gram matrix of this pass is the accepted point's, or close enough to it
        if (c == s.gram_req || max_diff <= 1e-10) {
            s.phase = BATCH_PH_NEWTON;
            return s.status;
        }
        batch_request_point(s, true, BATCH_PH_GRAM);
        return s.status;
    }
    default:
        batch_end(s, BATCH_FALLBACK, 0);
        return s.status;
    }
}

// Mean gradient over the sampled states.  numpy.linalg.lstsq(H, g) (mbar_solvers.py:582) answers for the part of g orthogonal to
// H's null vector 1 only; sum_k g_k is zero up to round-off, and that round-off, solved for in the gauge-fixed system, would move
// the Newton step by (round-off) / (smallest eigenvalue of H).  The right-hand side is therefore g - mean(g) on the sampled states.
MBAR_HD inline double batch_gradient_mean(const mbar_batch_state& s) {
#pragma clang fp contract(off)
    double sum = 0.0;
    int m = 0;
    for (int k = 0; k < (int)s.K; ++k)
        if (s.Nk[k] > 0) {
            sum = sum + (s.psum[k] - s.Nk[k]);
            m += 1;
        }
    return m > 0 ? sum / m : 0.0;
}
// Newton system of the live states (sampled, not s0) in ascending order: A[i * lda + j] = H_ij, b_i = g_i.  H = diag(psum) - G.
// Pivots at or below eps * m * max psum, or not finite, count as zero (the threshold of k_newton).
MBAR_HD inline double batch_pivot_threshold(const mbar_batch_state& s, int m) {
    double pmax = 0.0;
    for (int k = 0; k < (int)s.K; ++k)
        if (s.Nk[k] > 0 && s.psum[k] > pmax) pmax = s.psum[k];
    return pmax * 2.220446049250313e-16 * (double)(m > 0 ? m : 1);
}
// Serial LDL^T in place (lower triangle; A[j][j] <- d_j, A[i][j] <- l_ij) and solve; returns false on a pivot that counts as zero
MBAR_HD inline bool batch_ldlt_solve(double* A, int lda, double* b, int m, double thr) {
#pragma clang fp contract(off)
    for (int j = 0; j < m; ++j) {
        const double d = A[j * lda + j];
        if (!(d > thr) || !(d - d == 0.0)) return false;  // (d - d == 0: finite)
        for (int i = j + 1; i < m; ++i) {
            const double a = A[i * lda + j];
            const double l = a / d;
            for (int k = j + 1; k <= i; ++k) A[i * lda + k] = A[i * lda + k] - l * A[k * lda + j];
        }
        // (the column is scaled after the update: the update above read its unscaled entries)
        for (int i = j + 1; i < m; ++i) A[i * lda + j] = A[i * lda + j] / d;
    }
    for (int j = 0; j < m; ++j)
        for (int i = j + 1; i < m; ++i) b[i] = b[i] - A[i * lda + j] * b[j];
    for (int j = 0; j < m; ++j) b[j] = b[j] / A[j * lda + j];
    for (int j = m - 1; j >= 0; --j)
        for (int i = 0; i < j; ++i) b[i] = b[i] - A[j * lda + i] * b[j];
    return true;
}

// Device side.  Problem p: rows of K[p] states, N[p] samples at u + uoff[p] (row-major, ld N[p]); its chunks cbeg[p] ..
// cbeg[p + 1] of MBAR_BATCH_CHUNK columns each (the last one shorter), chunk c's partial record at part + coff[c]:
// [2][K] maxima, [2][K] scaled sums, [K][K] Gram.  Chunks are launched in four width classes (8, 16, 32, 64 states).
// The same struct describes a set of replica slots (bootstrap replicates): "problem" s is then a slot, uoff[s] and N[s] are those
// of its base problem (the block is shared, nothing is copied), its chunks, partial records and state are its own, and sample n
// counts cw[cwoff[s] + n] times (the weighted instantiation of the evaluation kernel; cw is NULL for the problems themselves).
constexpr int BATCH_WG = 256;
struct BatchData {
    const double* u;
    const int64_t* uoff;     // [P]
    const int64_t* N;        // [P]
    const int64_t* cbeg;     // [P + 1]
    const int* cprob;        // [nchunks]
    const int64_t* cn0;      // [nchunks] first column of the chunk in its problem
    const int64_t* coff;     // [nchunks] offset of the chunk's partial record
    double* part;
    int64_t P, nchunks;
    const double* cw;        // per-sample multiplicities of replica slots, or NULL
    const int64_t* cwoff;    // [P] offset of slot s's multiplicities in cw
};
// evaluation pass over the chunks list[0 .. n) of one width class kb; with d.cw (and d.cwoff) the weighted form: every sum over
// samples becomes sum_n c_n (...)
hipError_t launch_batch_eval(hipStream_t st, int kb, const BatchData& d, const int* list, int64_t n, const mbar_batch_state* states);
// Draw counts of the slots first .. first + count of the replica set d into d.cw (zeroed by the caller): position j of slot s
// draws bootstrap_draw(seed[s], replicate[s], j, n_k) within the run of its state, cum[base[s]][0 .. K] being the runs' bounds
// (rows of MBAR_BATCH_MAX_K + 1).  One workgroup per chunk; chunk0 / nchunk: the chunks of those slots.
hipError_t launch_batch_draw(hipStream_t st, const BatchData& d, int64_t chunk0, int64_t nchunk, const int64_t* base,
                             const int64_t* Kp, const int64_t* cum, const uint64_t* seed, const int64_t* replicate, double* cw);
// merge + one step of every running problem; FINAL problems: out_gram / out_wsum at their packed offsets goff / woff
hipError_t launch_batch_step(hipStream_t st, const BatchData& d, mbar_batch_state* states, int* active, double* out_gram,
                             double* out_wsum, const int64_t* goff, const int64_t* woff);

// Extension rows of the problems (mbar_batch_set_ext): problem p has R[p] rows of N[p] reduced potentials at e + eoff[p] (row-major,
// ld N[p]); its per-row values (f_ext, lognum_ext) are packed at roff[p].  Chunk c's record of the rows' sums is at lpart + lcoff[c]:
// [R] maxima, [R] scaled sums.  f and Nk: rows of MBAR_BATCH_MAX_K per problem; problems with mask[p] == 0 are skipped.
struct BatchExt {
    const double* e;
    const int64_t* eoff;     // [P]
    const int64_t* K;        // [P]
    const int64_t* R;        // [P]
    const int64_t* roff;     // [P]
    const int64_t* lcoff;    // [nchunks]
    double* lpart;
    const double* f;         // [P][MBAR_BATCH_MAX_K]
    const double* Nk;        // [P][MBAR_BATCH_MAX_K]
    const double* fext;      // packed like lognum_ext (the Gram pass only)
    const int32_t* mask;     // [P]
};
// The rows' sums: one workgroup per chunk of d, then one per problem that merges the chunk records in chunk order into
// lognum_ext (device, packed)
hipError_t launch_batch_ext_lognum(hipStream_t st, const BatchData& d, const BatchExt& x, double* lognum_ext);
// The augmented Gram pass over n work items of the width class ab (16, 32, 64, 128 >= K + R): item w is run wrun[w] of problem
// wprob[w] -- the chunks wrun[w] * MBAR_BATCH_EXT_RUN .. of that problem -- and writes the record ((K + R)^2 Gram, K + R column
// sums) at gpart + wgoff[w]
hipError_t launch_batch_ext_gram(hipStream_t st, int ab, const BatchData& d, const BatchExt& x, int64_t n, const int* wprob,
                                 const int* wrun, const int64_t* wgoff, double* gpart);
// Merge of the records of the n problems gprob[0 .. n): problem gprob[q]'s nrun[q] records start at gpart + gbase[q]; the sums, in
// run order, go to ogram + ogoff[p] and owsum + owoff[p]
hipError_t launch_batch_ext_gram_merge(hipStream_t st, const BatchExt& x, int64_t n, const int* gprob, const int64_t* gbase,
                                       const int* nrun, const double* gpart, double* ogram, double* owsum, const int64_t* ogoff,
                                       const int64_t* owoff);

}  // namespace mbar
