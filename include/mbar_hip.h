/*
 * mbar_hip.h -- C ABI of libmbar_hip.so: the MI355X (gfx950) MBAR solver hot path.
 *
 * This is the drop-in boundary for ONE path of choderalab/pymbar: the array math and solver
 * loops of pymbar/mbar_solvers.py (reference paths below are relative to the pymbar source
 * tree).  The reference is pure Python with no FFI; the binding a pymbar maintainer would add is
 * a ctypes module exporting the same names as pymbar.mbar_solvers (see INTEGRATION.md and
 * pymbar_amd/mbar_solvers.py, which is that module).
 *
 * Conventions
 *   - plain C, no torch / no C++ types; every pointer is a host pointer to caller-owned memory
 *     unless stated otherwise; all floating point is IEEE fp64; sizes are int64_t.
 *   - return value 0 = MBAR_OK, negative = error; mbar_last_error() gives the message.
 *   - a context owns the device-resident (K x N_local) reduced-potential matrix of ONE rank and
 *     is not thread-safe (one context per caller thread).  One process drives one GPU.
 *   - "p_nk" below is N_k * W_nk = N_k exp(f_k - u_kn) / sum_j N_j exp(f_j - u_jn): the
 *     probability that sample n was drawn from state k (rows sum to 1; 0 for unsampled states).
 *     With s_k = sum_n W_nk:  gradient g_k = N_k (s_k - 1) = psum_k - N_k   (mbar_solvers.py:284-292)
 *                             SCI      f'_k = f_k - log s_k                   (mbar_solvers.py:231-242)
 *                             Hessian  H = diag(psum) - gram                  (mbar_solvers.py:395-411)
 *   - when a communicator is attached (mbar_ctx_comm_init / mbar_ctx_set_host_allreduce) every
 *     reduced output (psum, sumlogden, gram, lognum) is the sum over all ranks' column shards.
 */
#ifndef MBAR_HIP_H
#define MBAR_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mbar_ctx mbar_ctx;

#define MBAR_OK 0
#define MBAR_ERR_ARG (-1)      /* bad argument                                   */
#define MBAR_ERR_HIP (-2)      /* a HIP runtime call failed                      */
#define MBAR_ERR_NODEVICE (-3) /* no usable gfx950 device                        */
#define MBAR_ERR_STATE (-4)    /* call sequence error (e.g. N_k not set)         */
#define MBAR_ERR_COMM (-5)     /* RCCL / host all-reduce failure                 */
#define MBAR_ERR_NUMERIC (-6)  /* non-finite intermediate where one is not legal */

/* mbar_eval flags */
#define MBAR_EVAL_GRAM 1u        /* also accumulate gram_ij = sum_n p_ni p_nj at f[0]          */
#define MBAR_EVAL_USE_OFFSET 2u  /* sumlogden = sum_n (logden_n - d_n), d_n from mbar_ctx_set_objective_offset */

/* kernel classes for mbar_ctx_timing */
#define MBAR_TIMER_LSE 0    /* per-sample log-sum-exp + per-state sums (evaluation pass)   */
#define MBAR_TIMER_GRAM 1   /* fp64 MFMA Gram / Hessian pass                              */
#define MBAR_TIMER_REDUCE 2 /* partial-sum reductions                                      */
#define MBAR_TIMER_OTHER 3  /* logW writer, robust per-state LSE, generator, P-mode build  */
#define MBAR_TIMER_FUSED 4  /* fused sweep of the adaptive loop (candidates + MFMA Gram)   */
#define MBAR_TIMER_NEWTON 5 /* K x K Newton solve + candidate selection (timing level 3 only)   */
#define MBAR_TIMER_COMM 6   /* the per-iteration all-reduce on the stream (timing level 3 only) */
#define MBAR_TIMER_COUNT 7

/* ---- library / device -------------------------------------------------------------------- */
int mbar_version(void);
/* Message of the last error on this context (ctx may be NULL: last error of a failed create). */
const char* mbar_last_error(const mbar_ctx* ctx);
int mbar_device_count(int* count);
int mbar_device_info(int device, char* name, int name_len, int* compute_units, int64_t* total_mem_bytes);

/* ---- context ------------------------------------------------------------------------------- */
/* Allocate a context on `device` for K states and N_local samples (this rank's column shard).
 * Replaces the implicit "arrays live in host RAM" of the reference (mbar.py:243). */
int mbar_ctx_create(mbar_ctx** out, int device, int64_t K, int64_t N_local);
void mbar_ctx_destroy(mbar_ctx* ctx);
int mbar_ctx_synchronize(mbar_ctx* ctx);
/* Device and pinned-host blocks freed by contexts are kept for re-use (hipMalloc / hipFree cost more than a sweep at the
 * sizes pymbar is typically run at, and 0.3-0.7 s for the 6-8 GB augmented matrix of an expectation call at K=128, N=4e6);
 * bounded by MBAR_CACHE_MB (environment; default an eighth of the device's memory; 0 = off) WHILE the process has a context,
 * and cut back to MBAR_CACHE_IDLE_MB (default 1024) when its last context is destroyed; an allocation that fails empties
 * the cache and is tried again.  This returns every parked block to the driver. */
int mbar_cache_trim(void);
/* Environment variables read by the library (diagnostics; none changes a result):
 *   MBAR_CACHE_MB        bound of the block cache above (MBAR_CACHE_IDLE_MB: what it keeps once no context is left)
 *   MBAR_HOST_THREADS    team size of the host-side K x K factorisation (default: one thread per 96 unknowns, at most 16 and at
 *                        most the cores that share the L3 cache with the caller's core; the team's worker threads are created on
 *                        first use, parked between calls and kept on those cores -- the caller's own thread is never touched)
 *   MBAR_HOST_TEAM_AFFINITY  0 = leave the placement of the team's workers to the scheduler
 *   MBAR_DEBUG_TIMING    per-iteration wall-clock split of the host-driven loops and of the host factorisation on stderr
 *   MBAR_DEBUG_STAMPS    in-kernel time stamps on stderr: the phases of k_select_newton (selection / set-up / elimination /
 *                        candidates, shader clocks) and of k_sci_small (tables, update, first tile, sweep per wave, fold) */
/* 128-bit content digest of a HOST buffer, computed at memory speed on `threads` host threads (0 = all cores).  The reference's
 * module-level functions are pure functions of the u_kn they are handed (mbar_solvers.py:260-292: every call reads the current
 * array); the Python binding keeps device copies of recently seen host matrices and re-uses one only when the digest of the
 * bytes now behind the address equals the digest of what it uploaded.  A change of ONE element always changes the digest. */
int mbar_host_digest(const void* data, int64_t nbytes, int threads, uint64_t* out2);
/* The K x K step of the adaptive iteration as the HOST-driven loop runs it (more than 256 states, host transport):
 * x = H^+ g - (H^+ g)[0] (mbar_solvers.py:582-583: numpy.linalg.lstsq(H, g) then the gauge shift).  H (m x m, row-major) is the
 * Hessian on the states with samples, positive semi-definite with null vector 1: the gauge-fixed (m-1) x (m-1) block is solved by
 * Cholesky factorisation -- from 320 unknowns on in column blocks whose rows are shared out over a team of host threads, results
 * independent of the team size -- and only if that breaks down (disconnected states) by the minimum-norm pseudo-inverse.
 * threads = 0: what the solver loop does; threads > 0: the blocked factorisation with that team size (tests).  Host only. */
int mbar_host_newton_direction(const double* H, const double* g, int m, int threads, double* x);
/* hipDeviceSynchronize on `device` (every stream of every context): the bracket of a timed region. */
int mbar_device_synchronize(int device);
/* Tuning / test knobs.  Every key selects between code paths that are BOTH needed somewhere (a fallback when memory is short,
 * a transport that needs the host in the loop, a state count outside a kernel's range), so that tests and A/B measurements can
 * force the path a default configuration would not take; the defaults are the measured best.  (Rounds 1-3 carried further keys
 * for kernel variants that were measured never-best -- "staging", "lse_variant", "gram_variant", "persistent" -- removed in
 * round 4 with their kernels; profiles/README.md keeps the measurements.)
 *   "grid_blocks"    0 = auto
 *   "force_generic"  1 = layout-agnostic fallback kernels for any K (what K > 512 runs)
 *   "check_finite"   default 1: NaN / -inf scan of the matrix after every upload
 *   "small_k_kernel" 1 = one-sample-per-lane sweep for K <= 32, single candidate (default), 0 = the general sweep
 *   "wide_k_kernel"  1 = single-buffer sweep with four waves per CU for 129 <= K <= 256 (default), 0 = the general sweep
 *   "device_loop"    1 = adaptive iterations run device-resident where possible (default), 0 = host-driven loop (what the
 *                    host all-reduce transport and K > 256 run)
 *   "adapt_batch"    adaptive iterations enqueued between two looks at the control words (default 8)
 *   "hist_part_bytes" byte budget of the partial records of one sweep of the binned passes (default 256 MiB); read by
 *                    mbar_ctx_set_bins, which cuts the bins into tiles -- one sweep each -- until a sweep's records fit
 *   "scan_part_bytes" byte budget of the partial records of one launch of pass A of the scans (default 256 MiB); read by
 *                    mbar_scan_lognum, which cuts the members into panels of a multiple of 64 (at least 64) whose records fit
 *   "pmode"          1 = the device-resident loop keeps P = exp(a0 - u - logden(a0)) resident (one more K x N array, built
 *                    once per solve) and sweeps that: no exponentials in the loop (default); 0 = sweeps recompute them from u
 *                    (what runs when P does not fit on some rank)
 *   "fused"          1 = in P mode ONE sweep per iteration: the candidate sweep also accumulates the Gram matrix of the
 *                    candidate about to be accepted, a separate Gram sweep runs only when that speculation is rejected
 *                    (default); 0 = two sweeps per iteration on P (evaluation + Gram): the A/B of the fusion
 *   "gram_quad"      1 = 129 <= K <= 256: the Gram sweep reads the matrix ONCE, the four waves of a workgroup share the tile
 *                    stream and split the panel's 78 / 136 blocks (default); 0 = 128-state panels + 64 x 128 rectangles
 *                    (2.5 reads: what K > 256 runs)
 *   "device_loop_wide" 1 = the device-resident loop also serves 129 <= K <= 256 (Newton system by a blocked Cholesky
 *                    factorisation in device memory; default); 0 = host-driven loop there
 *   "wide_pmode"     1 = 129 <= K <= 256 also keep a resident probability matrix and run ONE fused sweep per iteration
 *                    (k_fused_quad; default); 0 = two sweeps on u there (what runs when P does not fit)
 *   "quad_trim"      1 = 129 .. 160 and 193 .. 224 states: the one-read Gram / fused sweeps skip the two padding blocks of the
 *                    192- / 256-row panel (default); 0 = the whole panel
 *   "host_pmode"     above 256 states the host-driven loop also builds a resident probability matrix once per solve and runs
 *                    BOTH of its sweeps on it (one multiplication per element instead of an exponential): 2 = Gram sweep in
 *                    256-state panels, one read each, + 128 x 256 rectangles (default); 1 = in the 128-state panels and 64 x 128
 *                    rectangles of the sweep on u; 0 = both sweeps on u (what runs when P does not fit)
 *   "rect_waves"     8 = the 128 x 256 rectangles of that Gram sweep run two waves per SIMD (default); 4 = one
 *   "newton_ldlt"    up to 128 states: 1 = the K x K Newton solve of the device-resident loop (mbar_solvers.py:581-583) is a blocked
 *                    LDL^T factorisation on the fp64 matrix cores, pivots from the last state upwards, two barriers per 16 pivots
 *                    (default; k_select_newton 66 -> 37 us at 127 unknowns); 0 = the register Gauss-Jordan solve of rounds 2-5
 *                    (also: environment variable MBAR_NEWTON_LDLT)
 *   "pcache"         1 = the resident probability matrix outlives the solve that built it: a later adaptive solve on the same
 *                    matrix whose start lies within 200 kT of its anchor (bootstrap replicates, protocol stages) starts with
 *                    one fused sweep instead of the build sweep (default); 0 = every solve builds (cold-solve timings)
 *   "debug_download_p" test-only hook: 1 = mbar_ctx_download_u hands back the resident probability matrix P of the last
 *                    device-resident adaptive solve (K <= 256) instead of u, and fails with MBAR_ERR_STATE when the context
 *                    holds none; 0 = u (default).  tests/test_gpu_device_math.py checks P entry by entry through it
 *   "merge_select"   1 = the selection of iteration i and the Newton solve of iteration i + 1 share a launch (default)
 *   "light_last"     fused loop: when BOTH candidates of the coming sweep already meet the stop test of
 *                    mbar_solvers.py:627-636 against the current f, the iteration is the last whichever of them wins and the Gram
 *                    matrix the fused sweep would accumulate is never used: the plain two-candidate sweep on P evaluates them
 *                    instead (k_psweep, launched behind the fused sweep every iteration and idle otherwise; at config 3 1.9 ms
 *                    in place of 3.1; 129 .. 256 states: an evaluation-only body of k_fused_quad, no extra launch).  1 = from 65
 *                    states and 5e7 matrix entries per rank on (default: elsewhere the
 *                    idle launch per iteration costs more than the lighter sweep saves -- with 64 states and fewer both sweeps
 *                    are HBM-bound), 2 = always, 0 = never
 *   "fused_general"  fused loop up to 128 states: 0 = a context without sample weights runs the fused sweep specialised for unit
 *                    multiplicities (no weights in the tile, no multiplications by one, the multipliers of the normalisers'
 *                    matrix steps in registers; default);
 *                    1 = it runs the general kernel, which a weighted context (bootstrap draw counts, observable weights)
 *                    always runs.  Same grid, same partial records, same order of every sum: the results are identical to the
 *                    bit (tests/test_gpu_fused_variants.py) -- the A/B arm of tools/ab_fused_general.py
 *   "direct_results" 1 = mbar_eval on one rank without the Gram matrix: the last reduction level writes the sums into pinned host
 *                    memory itself instead of a device buffer + a copy (default); 0 = always through the device buffer
 *   "sci_merged"     1 = pure self-consistent iteration, K <= 32, one rank: update + sweep of an iteration in ONE launch
 *                    (k_sci_small; default); 0 = sweep + single-workgroup update kernel (what several ranks and K > 32 run)
 *   "graph", "sci_batch"             hipGraph batching of the solver loops
 *   "timing"         HIP-event timers (mbar_ctx_timing): 0 = off (default: an event pair per sweep costs ~10 us, a fifth of an
 *                    iteration at the problem sizes pymbar is mostly used on), 1 = event records around a launch, 2 = events
 *                    bound to the kernel dispatch in the device-resident loop (no marker packets between kernels), 3 = level 1 plus
 *                    event pairs around the reduction, the all-reduce and the Newton / selection launches of every iteration of
 *                    the device-resident loop (the per-iteration split {sweep, reduce, all-reduce, Newton + selection} that
 *                    explains a multi-GPU run; ~6 more marker packets per iteration) */
int mbar_ctx_set_option(mbar_ctx* ctx, const char* key, int64_t value);

/* ---- data ---------------------------------------------------------------------------------- */
/* Copy columns [col0_host, col0_host+ncols) of a C-contiguous host matrix u_host[K][ld_host]
 * (the u_kn of mbar_solvers.py:174-203, row pitch ld_host) into device columns
 * [col0_dev, col0_dev+ncols) of this rank's shard. */
int mbar_ctx_upload_u(mbar_ctx* ctx, const double* u_host, int64_t ld_host, int64_t col0_host,
                      int64_t ncols, int64_t col0_dev);
int mbar_ctx_download_u(mbar_ctx* ctx, double* out, int64_t ld_out);
/* Row-level assembly of an AUGMENTED matrix on the device -- the expectation family (mbar.py:732-1001) appends one
 * row per new state (u_ln) and one per observable (u_ln - log A_n) to the resident u_kn; none of it needs the host
 * N x (K + NL + S) array the reference builds (mbar.py:886-903).
 *   upload_rows: whole rows [row0, row0 + nrows) from a C-contiguous host array rows_host[nrows][ld_host >= N_local];
 *   copy_rows:   device-to-device from another context on the same device with the same N_local;
 *   row_sub:     u[row][n] -= v_host[n]  (v = log A_n); v_host = NULL subtracts the vector of the previous call again;
 *   rows_sub:    u[dst_row0 + r][n] = u[src_row0 + r][n] - v_host[n] for r < nrows in ONE launch (one observable evaluated at
 *                a run of states: the state rows are copied and shifted in the same pass); dst_row0 == src_row0: in place,
 *                otherwise the ranges must not overlap; v_host = NULL as for row_sub;
 *   rows_rsub:   u[dst_row0 + r][n] = u[src_row0 + r][n] - u[dst_row0 + r][n]: many DIFFERENT observables -- their log A rows are
 *                uploaded in one upload_rows call and turned into observable rows in one launch (disjoint ranges). */
int mbar_ctx_upload_rows(mbar_ctx* ctx, int64_t row0, int64_t nrows, const double* rows_host, int64_t ld_host);
int mbar_ctx_copy_rows(mbar_ctx* dst, int64_t dst_row0, mbar_ctx* src, int64_t src_row0, int64_t nrows);
int mbar_ctx_row_sub(mbar_ctx* ctx, int64_t row, const double* v_host);
int mbar_ctx_rows_sub(mbar_ctx* ctx, int64_t dst_row0, int64_t src_row0, int64_t nrows, const double* v_host);
int mbar_ctx_rows_rsub(mbar_ctx* ctx, int64_t dst_row0, int64_t src_row0, int64_t nrows);
/* Observables into log space ON THE DEVICE (mbar.py:858-867: every observable is shifted to be positive; :886-903: its log
 * enters the augmented log-weight matrix): rows [row0, row0 + nrows) hold raw observable values A_i[n] (uploaded with
 * mbar_ctx_upload_rows, or copied from a resident matrix with mbar_ctx_copy_rows) and leave as log(A_i[n] - shift_i) with
 * shift_i = min_n A_i[n] - |4 eps min_n A_i[n]| (shift_out[i]; the reference's A_min - logfactor, which the host adds back to
 * the expectation) -- in place of three host passes over nrows x N doubles and nrows N libm logarithms.  mbar_ctx_rows_rsub then
 * turns them into observable rows u - log A.  Single-context matrices only (the minimum is not reduced across ranks). */
int mbar_ctx_rows_logshift(mbar_ctx* ctx, int64_t row0, int64_t nrows, double* shift_out);
/* The same for ONE observable evaluated at many states: A[N_local] (host) is uploaded into the context's staging vector and
 * becomes log(A - shift) there; mbar_ctx_rows_sub / mbar_ctx_row_sub with v = NULL then subtract it. */
int mbar_ctx_vec_logshift(mbar_ctx* ctx, const double* A, double* shift_out);
/* Free-energy-surface histograms (fes.py:1383-1402: one extra column of W per populated bin, W[n, K+i] = exp(log_w_n + f_i)
 * on the bin's samples and 0 elsewhere): rows [row0, row0 + nrows) of the augmented matrix become
 *   u[row0 + i][n] = label[n] == i ? v[n] : +inf      (v = the target potential u_n; label[n] = bin of sample n, -1 = none)
 * built on the device from ONE vector and ONE label array -- the N x (K + nbins) host matrix of the reference is never
 * formed.  A +inf entry is a sample of weight zero in that state. */
int mbar_ctx_fill_masked_rows(mbar_ctx* ctx, int64_t row0, int64_t nrows, const double* v_host, const int32_t* label_host);
/* Rows of the resident matrix from a FAMILY OF STATES instead of an upload: rows [row0, row0 + nrows) become
 *   u[row0 + r][n] = offset[r] + sum_{b < B} term_b(r, n), b ascending, from the offset:                    0 <= n < N_local
 *     kind[b] == 0   linear     u = fma(coeff[r][b], basis[b][n], u)
 *     kind[b] != 0   harmonic   d = basis[b][n] - center[r][b]
 *                               period[b] > 0:  m = rint(d * rP), d = fma(-period[b], m, d)      rP = 1.0 / period[b], rounded once
 *                               q = d * d;  u = fma(coeff[r][b], q, u)
 * every operation rounded once, nothing else contracted, rint to nearest even (a tie d = +-P / 2 gives the same q either way:
 * the value is continuous there).  Linear terms alone are a temperature ladder beta_k E, pressures beta (E + p_k V), harmonic
 * umbrellas (linear in E, x^2, x, 1), linear alchemical coupling; a harmonic term is umbrella sampling on a periodic coordinate,
 * u_k(n) = beta_k [E_n + kappa_k / 2 wrap(chi_n - chi0_k)^2], whose minimum image depends on sample AND state and is linear in no
 * basis.  Every sampled state of such a simulation is B <= MBAR_SCAN_MAX_B parameters over B shared per-sample vectors, and 8 B N
 * bytes cross the bus instead of 8 K N.  basis_host[B][ld_host] is C-contiguous and its columns [col0_host, col0_host + N_local)
 * are this context's samples (a rank passes the whole basis and its shard origin, as with mbar_ctx_upload_u; no communication);
 * coeff[nrows][B]; offset[nrows] or NULL (zeros).  At most MBAR_SCAN_MAX_H terms may be harmonic; period[b] = 0: a harmonic term
 * that is not periodic; center[nrows][B] and period[B] are read at the harmonic terms only (center NULL: allowed when no term is
 * harmonic; period NULL: no term is periodic); kind NULL: every term linear.  The chain is the one the scan passes evaluate
 * (mbar_scan_lognum, mbar_ctx_set_scan_terms): a scan member with a sampled state's coeff, center and offset has that state's row
 * to the bit.  The basis shard is staged in a temporary device block that is released before return; the call returns with the
 * stream idle.  Any K the context supports; nothing is written outside the row range or behind column N_local.  MBAR_ERR_ARG: NULL
 * basis_host / coeff, B outside [1, 8], a row range outside [0, K], a column range outside ld_host, more than MBAR_SCAN_MAX_H
 * harmonic terms, a negative or non-finite period, harmonic terms without center, a non-finite coefficient or centre;
 * MBAR_ERR_STATE: an extension context (mbar_ctx_create_ext).  nrows = 0: MBAR_OK. */
#define MBAR_SCAN_MAX_H 4
int mbar_ctx_fill_family_rows(mbar_ctx* ctx, int64_t row0, int64_t nrows, int64_t B, const double* basis_host, int64_t ld_host,
                              int64_t col0_host, const double* coeff, const double* center, const double* offset, const int32_t* kind,
                              const double* period);
/* mbar_ctx_fill_family_rows with center = kind = period = NULL, a LINEAR FAMILY: u[row0 + r][n] = fma(coeff[r][B-1], basis[B-1][n],
 * ... fma(coeff[r][0], basis[0][n], offset[r])), the same bits, and the coefficients are not looked at on the host. */
int mbar_ctx_fill_linear_rows(mbar_ctx* ctx, int64_t row0, int64_t nrows, int64_t B, const double* basis_host, int64_t ld_host,
                              int64_t col0_host, const double* coeff, const double* offset);
/* Fill the shard on the device with the synthetic harmonic ladder of SURVEY.md 8(d):
 * global sample n (n_global0 <= n < n_global0+N_local) belongs to the state given by the
 * cumulative N_k_global, x_n ~ Normal(O_s, K_s^-1/2) from a counter-based RNG keyed by
 * (seed, n), u[l][n] = K_l (x_n - O_l)^2 / 2.  Same data for any sharding of n. */
int mbar_ctx_generate_harmonic(mbar_ctx* ctx, uint64_t seed, const double* O_k, const double* K_k,
                               const int64_t* N_k_global, int64_t n_global0);
/* GLOBAL sample counts per state as doubles (the float cast of mbar_solvers.py:792); zeros allowed:
 * such states contribute nothing to denominators (mbar_solvers.py:238 with b=N_k). */
int mbar_ctx_set_Nk(mbar_ctx* ctx, const double* N_k);

/* Per-sample multiplicities c_n >= 0 for this rank's N_local samples (NULL restores c_n = 1).  Every sum over
 * samples becomes sum_n c_n (...): a bootstrap replicate (mbar.py:417-449, resampling the columns of u_kn within each
 * state) is the vector of draw counts, so replicates re-use the resident matrix instead of a gathered copy. */
int mbar_ctx_set_sample_weights(mbar_ctx* ctx, const double* c_n);

/* A bootstrap replicate DRAWN ON THE DEVICE (extension: the reference draws with numpy's generator on the host, one pass over
 * N integers + a bincount per replicate -- 33 ms of host work at N = 4e6 where the replicate's solve takes 5): the multiplicities
 * c_n of mbar_ctx_set_sample_weights become the draw counts of replicate `replicate` of the counter-based stream `seed` -- slot j
 * (position j in state order, 0 <= j < cumN[K_states]) of the state that owns positions cumN[k] .. cumN[k+1]-1 draws one of
 * those positions, a pure function of (seed, replicate, j); order[p] (or NULL: p itself) is the sample at position p, for
 * x_kindices other than the default; n_global0 = first global sample of this rank's shard.  mbar_bootstrap_draws returns the
 * SAME draws on the host as the reference's bootstrap_rints row (mbar.py:433: rints[sample of slot j] = sample drawn): host only,
 * no context.  Same-seed determinism (tests/test_mbar.py:533-545 of the reference) holds by construction. */
int mbar_ctx_draw_bootstrap_weights(mbar_ctx* ctx, uint64_t seed, int64_t replicate, const int64_t* cumN, int64_t K_states,
                                    const int64_t* order, int64_t n_global0);
/* The layout (cumN[K_states + 1], order[cumN[K_states]] or NULL) validated and uploaded ONCE; mbar_ctx_draw_bootstrap_weights with
 * cumN = NULL (K_states, order ignored / NULL) then draws on it -- no host pass over N integers per replicate (with arrays in the
 * call their content is digested on every call to see whether the device copy is still the right one). */
int mbar_ctx_set_bootstrap_layout(mbar_ctx* ctx, const int64_t* cumN, int64_t K_states, const int64_t* order);
int mbar_bootstrap_draws(uint64_t seed, int64_t replicate, const int64_t* cumN, int64_t K_states, const int64_t* order,
                         int64_t* rints_out);

/* Per-sample weights c_n = (A_n - shift)^power from the observable mbar_ctx_vec_logshift left in the staging vector (as
 * log(A_n - shift)), formed on the device: no upload, no host pass over N doubles.  What it is for: ONE observable evaluated at
 * the resident states (compute_expectations(A_n), mbar.py:1039-1312) needs no augmented matrix at all -- the weight column of
 * "A at state l" is A'_n W_nl up to a constant, so the observable rows' normalisers are mbar_lognum with weights A' and the
 * covariance input of mbar.py:886-903 is the three weighted Gram matrices sum_n A'^p W W^T, p = 0, 1, 2, of the RESIDENT matrix
 * (mbar_gram_w with these weights).  mbar_ctx_set_sample_weights(ctx, NULL) restores c_n = 1. */
int mbar_ctx_weights_from_vec(mbar_ctx* ctx, double power);

/* ---- multi-GPU (one process per GPU; N sharded; one small all-reduce per pass) ------------- */
int mbar_comm_unique_id(void* id128);                 /* rank 0: ncclGetUniqueId (128 bytes)     */
int mbar_ctx_comm_init(mbar_ctx* ctx, const void* id128, int rank, int nranks); /* RCCL over xGMI */
/* Fallback transport: fn(buf, count, op, user) must all-reduce `count` doubles in place
 * (op 0 = sum, 1 = max) across ranks on the host. */
typedef int (*mbar_allreduce_fn)(double* buf, int64_t count, int op, void* user);
/* Replaces an RCCL communicator if one is attached (the two transports never coexist on a context). */
int mbar_ctx_set_host_allreduce(mbar_ctx* ctx, mbar_allreduce_fn fn, void* user, int rank, int nranks);
/* Detach whatever transport is attached (RCCL communicator destroyed, in-process group left); the context is single-rank again.  When
 * RCCL cannot be initialised on EVERY rank, every rank must call this before falling back to the host transport. */
int mbar_ctx_comm_destroy(mbar_ctx* ctx);

/* In-process transport: several contexts of ONE process on ONE device (one caller thread each) all-reduce on their compute
 * streams -- events across the streams, a rendezvous of the caller threads per collective, no host-device synchronisation.
 * It drives the same code as an RCCL communicator (collectives on the stream: the device-resident solver loop runs across
 * the "ranks"), which RCCL itself cannot be made to do on a one-GPU box (it refuses two ranks on one device); results are
 * summed in rank order on every rank, hence bit-identical across ranks.  nranks <= 8; every rank must issue the same calls. */
typedef struct mbar_loopback mbar_loopback;
int mbar_loopback_create(mbar_loopback** out, int nranks);
void mbar_loopback_destroy(mbar_loopback* group);
int mbar_ctx_set_loopback(mbar_ctx* ctx, mbar_loopback* group, int rank);

/* ---- L1 evaluation (replaces mbar_solvers.py L1 functions) -------- */
/* One fused sweep of u_kn for nf (1 or 2) free-energy vectors f[nf][K]:
 *   psum[i][k]   = sum_n p_nk(f_i)              (K per f; 0 for states with N_k = 0)
 *   sumlogden[i] = sum_n logden_n(f_i)  [ - d_n with MBAR_EVAL_USE_OFFSET ]
 *   gram[K][K]   = sum_n p_ni p_nj at f_0       (only with MBAR_EVAL_GRAM; fp64 MFMA)
 * logden_n(f_i) stays on the device in slot i.  Any output pointer may be NULL. */
int mbar_eval(mbar_ctx* ctx, const double* f, int nf, unsigned flags, double* psum,
              double* sumlogden, double* gram);
/* d_n := logden_n(f0): the per-sample offset that replaces precondition_u_kn
 * (mbar_solvers.py:697-707) for the objective; f0 = NULL clears it. */
int mbar_ctx_set_objective_offset(mbar_ctx* ctx, const double* f0);
/* lognum_k = log sum_n exp(-logden_n(f) - u_kn) for ALL K states (unsampled ones included),
 * in log space like mbar_solvers.py:240-241; self_consistent_update = -lognum. */
int mbar_lognum(mbar_ctx* ctx, const double* f, double* lognum);
/* logden_n(f) for this rank's samples (mbar_solvers.py:238). */
int mbar_logden(mbar_ctx* ctx, const double* f, double* out_n);
/* log W_nk = f_k - u_kn - logden_n written as out[k][n] with row pitch ld_out (this rank's
 * shard).  Memory-identical to the reference's F-ordered (N, K) result (mbar_solvers.py:439-449). */
int mbar_logw(mbar_ctx* ctx, const double* f, double* out_kn, int64_t ld_out);
/* The weights themselves, W_kn = exp(log W_kn) (mbar_solvers.py:476-486 `mbar_W_nk`: exp of the log weights, taken on the host
 * there -- 1 s of single-threaded numpy for config 3's 1.28e9 entries), same layout as mbar_logw. */
int mbar_w(mbar_ctx* ctx, const double* f, double* out_kn, int64_t ld_out);
/* gramW[K][K] = sum_n W_ni W_nj and wsum[k] = sum_n W_nk for ALL states (W^T W of
 * mbar.py:1816,1849 and compute_overlap mbar.py:606); fp64 MFMA. */
int mbar_gram_w(mbar_ctx* ctx, const double* f, double* gramW, double* wsum);

/* ---- histogram bins by label ----------------------------------------------------------------
 * The bins of a histogram free energy surface as LABELS of the samples of the resident matrix (pymbar/fes.py:575-595,
 * 1383-1406) -- no row per bin, no second matrix.  Single-rank contexts with a normal row pitch only: a context with a
 * transport attached, an extension context or a wide-pitch matrix gets MBAR_ERR_STATE naming the limit.
 *   mbar_ctx_set_bins   label[n] in [-1, nbins) is the bin of sample n (-1: none), v[n] the target potential (finite or +inf);
 *                       both are uploaded once, the label range is validated, and the chunk table of the labels is built on the
 *                       host in O(N): contiguous chunks of at most 2048 samples touching at most 64 distinct bins.  The partial
 *                       records of one sweep ((K + 2) doubles per (chunk, bin of the chunk)) are bounded by the option
 *                       "hist_part_bytes" as it stands at this call: above it the bins are cut into tiles, one sweep per tile
 *                       (labels outside the tile count as -1).  nbins = 0 releases everything.
 *   mbar_ctx_bins_info  sweeps per pass, chunks in all, bytes of the largest sweep's partial records (any pointer may be NULL).
 *   mbar_bin_lognum     lognum_bins[i] = log sum_{n in bin i} c_n exp(-v_n - logden_n(f)), in log space against the bin's OWN
 *                       maximum; -inf for a bin none of whose samples has c_n > 0 (c_n: mbar_ctx_set_sample_weights /
 *                       mbar_ctx_draw_bootstrap_weights).  The bin free energy is -lognum_bins[i].
 *   mbar_bin_gram_w     with B_n = exp(f_bins[label_n] - v_n - logden_n(f)) and W_nk = exp(f_k - u_kn - logden_n(f)):
 *                       cross[k][i] = sum_{n in i} c_n W_nk B_n (K x nbins, row-major; NULL: not computed),
 *                       diag[i] = sum_{n in i} c_n B_n^2, wsum_bins[i] = sum_{n in i} c_n B_n (1 at f_bins = -lognum_bins):
 *                       the border of W^T W that the covariance of the bins needs next to mbar_gram_w of the resident states.
 *                       The matrix is read once, in its natural order.
 * No floating-point atomics: every sum's order is a function of (labels, N, K, nbins, "hist_part_bytes"), two identical calls
 * return identical bits.  Kernel time is booked under MBAR_TIMER_OTHER. */
int mbar_ctx_set_bins(mbar_ctx* ctx, int64_t nbins, const int32_t* label_host, const double* v_host);
int mbar_ctx_bins_info(mbar_ctx* ctx, int64_t* sweeps, int64_t* chunks, int64_t* record_bytes);
int mbar_bin_lognum(mbar_ctx* ctx, const double* f, double* lognum_bins);
int mbar_bin_gram_w(mbar_ctx* ctx, const double* f, const double* f_bins, double* cross, double* diag, double* wsum_bins);

/* ---- reweighting scans over a linear family of unsampled states ------------------------------
 * Solve once, then reweight to L states that were never sampled (a temperature, pressure or lambda grid, a sweep of a restraint
 * centre): member l is u_l(n) = sum_b coeff[l][b] basis[b][n] + offset[l], B <= MBAR_SCAN_MAX_B coefficients instead of a matrix
 * row of N doubles.  Nothing of size L x N is allocated.  Single-rank contexts with a normal row pitch and at most 128 states
 * only: any other context gets MBAR_ERR_STATE naming the limit.  With x_ln = -u_l(n) - logden_n(f) (u_l as one fma chain over
 * ascending b), t_0n = 1, t_jn = t[j - 1][n] (j = 1 .. Q: the observables, shifted positive by the caller), J = 1 + Q and c_n the
 * sample multiplicities:
 *   mbar_ctx_set_scan   uploads the B + Q N-vectors (row-major, B x N and Q x N) once; B = 0 releases them.
 *   mbar_scan_lognum    pass A.  M_l = max_{c_n > 0} x_ln, S_lj = sum_n c_n exp(x_ln - M_l) t_jn, lognum[l] = M_l + log S_l0
 *                       (f_l = -lognum[l]), mean[l][j] = S_lj / S_l0 (L x J; NULL: not returned).  Every member is referred to its
 *                       OWN maximum.  Reads B + Q + 2 N-vectors twice, never the matrix.  offset NULL: zeros.
 *   mbar_scan_gram_w    pass B.  b_ln = exp(f_scan[l] + x_ln), W_nk = exp(f_k - u_kn - logden_n), r the reference member:
 *                       cross[k][l][j] = sum_n c_n W_nk b_ln t_jn (K x L x J; NULL: not computed) on the fp64 matrix cores, the
 *                       b t operand generated in registers; within[l][i <= j] = sum_n c_n b_ln^2 t_in t_jn (L x J (J + 1) / 2,
 *                       row-major upper triangle), refcol[l][j] = sum_n c_n b_rn b_ln t_jn (L x J), wsum[l] = sum_n c_n b_ln (1 at
 *                       f_scan = -lognum).  The matrix is read once per panel of 64 .. 256 members.
 * No floating-point atomics; the samples are cut into chunks by N alone and merged in chunk order: two identical calls return
 * identical bits, and member l's outputs do not depend on the other members of the call, nor on where the member panels of
 * pass A are cut: they are the same bits for any value of "scan_part_bytes".  Kernel time: MBAR_TIMER_OTHER. */
#define MBAR_SCAN_MAX_B 8
#define MBAR_SCAN_MAX_Q 3
int mbar_ctx_set_scan(mbar_ctx* ctx, int64_t B, const double* basis, int64_t Q, const double* t);
int mbar_scan_lognum(mbar_ctx* ctx, const double* f, int64_t L, const double* coeff, const double* offset, double* lognum, double* mean);
int mbar_scan_gram_w(mbar_ctx* ctx, const double* f, int64_t L, const double* coeff, const double* offset, const double* f_scan,
                     int64_t r, double* cross, double* within, double* refcol, double* wsum);
/* Scans over a family with HARMONIC terms (a sweep of a restraint centre on a torsion): the chain of mbar_ctx_fill_family_rows.
 *   mbar_ctx_set_scan_terms     kind[B], period[B] of the basis uploaded by mbar_ctx_set_scan (call it after that one).  kind NULL,
 *                               or another mbar_ctx_set_scan, returns to the all-linear family.  Drops the centres.  MBAR_ERR_ARG:
 *                               more than MBAR_SCAN_MAX_H harmonic terms, a negative or non-finite period; MBAR_ERR_STATE: no basis.
 *   mbar_ctx_set_scan_centers   center[L][B] of the members the next scan calls take (read at the harmonic terms only), kept until
 *                               replaced; L = 0 drops them.  MBAR_ERR_ARG: a non-finite centre.
 * mbar_scan_lognum, mbar_scan_gram_w and the two binned passes below then run on the context's family: with a harmonic term set
 * and the centres missing or of another L they return MBAR_ERR_STATE with a message that names the call, a non-finite
 * coefficient is MBAR_ERR_ARG.  With every term linear they are the calls, and return the bits, they always were.  Everything
 * said above of order, determinism and independence of the members holds for either kind. */
int mbar_ctx_set_scan_terms(mbar_ctx* ctx, const int32_t* kind, const double* period);
int mbar_ctx_set_scan_centers(mbar_ctx* ctx, int64_t L, const double* center);
/* The member's OWN reduced potential as the observable (entropy, enthalpy and heat capacity along a scan): the two passes above with
 *   t_0 = 1,  t_1 = u_l(n) - center_u[l],  t_2 = t_1 t_1        J = 2 or 3 (anything else: MBAR_ERR_ARG)
 * where u_l(n) is the value the chain produced for x_ln (not a second evaluation) and every operation is rounded once.  The basis
 * is the one of mbar_ctx_set_scan with any Q -- its observables are ignored --, the family kinds those of mbar_ctx_set_scan_terms /
 * mbar_ctx_set_scan_centers; limits, panels, chunks, merges, determinism, independence of the members and the timer are those of
 * mbar_scan_lognum / mbar_scan_gram_w.  center_u[L]: a centre per member (finite; NULL: zeros).  With center_u = <u_l>, mean[l][1] is
 * ~ 0 and mean[l][2] - mean[l][1]^2 is the fluctuation of u_l without a cancellation of order <u>^2.
 *   mbar_scan_energy_lognum   pass A: lognum[l] has the bits mbar_scan_lognum returns for the same members (the max launch and the
 *                             chain of S_l0 are the same operations); mean[l][j] = S_lj / S_l0 with the member's own t_j (L x J).
 *   mbar_scan_energy_gram_w   pass B: cross, within and wsum as in mbar_scan_gram_w with the member's own t_j; the reference member's
 *                             observable is its own too, so refcol becomes refblock[l][i][j] = sum_n c_n (b_rn t_ri)(b_ln t_lj),
 *                             i = 0, 1, j < J (L x 2 x J). */
int mbar_scan_energy_lognum(mbar_ctx* ctx, const double* f, int64_t L, const double* coeff, const double* offset, const double* center_u,
                            int64_t J, double* lognum, double* mean);
int mbar_scan_energy_gram_w(mbar_ctx* ctx, const double* f, int64_t L, const double* coeff, const double* offset, const double* center_u,
                            int64_t J, const double* f_scan, int64_t r, double* cross, double* within, double* refblock, double* wsum);

/* The members' own Gram block, for differences between ANY two members of a scan (MBAR.compute_scan_pairs): on the family of
 * mbar_ctx_set_scan / mbar_ctx_set_scan_terms / mbar_ctx_set_scan_centers with its Q observables, for the R reference members
 * rows[R] (indices into the call's L members; they may repeat),
 *   pair[r][l][i][j] = sum_n c_n (b_{rows[r]} n t_in)(b_ln t_jn)        R x L x J x J, row-major
 * with b_ln = exp(f_scan[l] + x_ln) as in mbar_scan_gram_w: pair[r][l][0][j] is the refcol[l][j] that call returns for r = rows[r],
 * pair[r][rows[r]][i][j] the reference member's own within.  Both operands are generated on the device from the B numbers per
 * sample -- the (reference member, i) rows once per tile of 16 samples in LDS, the members' columns in registers -- and multiplied
 * on the fp64 matrix cores; nothing of size L x N is stored and the resident matrix is read only through logden_n(f).  The
 * reference members are taken in panels of 32 / J or 128 / J, the members in the panels of mbar_scan_gram_w; one launch per pair of
 * panels costs (reference members + members of the panels) x N exponentials and 2 x (rows of the panel) x (members) x J x N flop.
 * A member's b is formed by the same operations as a row and as a column.  No floating-point atomics; chunks of 8192 samples cut
 * by N alone and merged in chunk order: two identical calls return identical bits, element (r, l, i, j) does not depend on the
 * other members or reference members of the call nor on where they sit, and without sample weights pair[r][l][i][j] and the
 * pair[l'][r'][j][i] of the same two members are the same bits.  Limits and state errors are those of mbar_scan_gram_w;
 * MBAR_ERR_ARG: R < 1, a row outside [0, L), a NULL pointer, a non-finite f_scan.  A NaN in f fills pair with NaN (MBAR_OK).
 * Kernel time: MBAR_TIMER_OTHER. */
int mbar_scan_pair_gram(mbar_ctx* ctx, const double* f, int64_t L, const double* coeff, const double* offset, const double* f_scan,
                        int64_t R, const int64_t* rows, double* pair);

/* The FEATURES the chain is made of next to the stored observables (derivatives of f and of the averages along a scan): pass A once
 * more, on the family of mbar_ctx_set_scan / mbar_ctx_set_scan_terms / mbar_ctx_set_scan_centers with its Q observables.  Walking the
 * terms in ascending b, a linear term contributes the feature phi = basis[b][n], a harmonic one two, dl_b then dl_b^2 with dl_b the
 * wrapped displacement exactly as the chain forms it (dl = v - c; P > 0: dl = fma(-P, rint(dl rP), dl)): F = B + H <= 12 features.
 * With e = c_n exp(x_ln - M_l), d_i = phi_i - center_phi[l][i] and the sums S0 = sum e, S_q = sum e t_qn, A_i = sum e d_i,
 * B_ij = sum e d_i d_j, C_qi = sum e t_qn d_i (every difference and product rounded once, every accumulation one fma, chunks
 * merged in chunk order, compensated):
 *   lognum[l], mean[l][1 + Q]   the bits mbar_scan_lognum returns for the same call
 *   m1[l][i]  = A_i / S0        <phi_i - c_i>_l                                   (L x F)
 *   m2[l][ij] = B_ij / S0       <(phi_i - c_i)(phi_j - c_j)>_l, i <= j            (L x F (F + 1) / 2, row-major upper triangle)
 *   ma[l][q][i] = C_qi / S0     <t_q (phi_i - c_i)>_l                             (L x Q x F; may be NULL when Q = 0)
 * center_phi[L][F] (finite, else MBAR_ERR_ARG; NULL: zeros): with center_phi = <phi>_l of a first call the covariances m2 - m1 m1^T
 * and ma - mean m1 carry no cancellation of order <phi>^2.  e, x_ln, u_l and dl come from ONE evaluation of the chain: the pass
 * costs about L N exponentials plus F (F + 3) / 2 + Q (F + 1) fused multiply-adds per (member, sample) and reads the B + Q + 2
 * N-vectors twice, never the matrix.  Limits, determinism, independence of the members, the timer and "scan_part_bytes" (now
 * with the record of 1 + Q + F' + F' (F' + 1) / 2 + Q F' doubles per member and chunk, F' the feature slots of the kernel's
 * bucket) are those of mbar_scan_lognum. */
int mbar_scan_moments(mbar_ctx* ctx, const double* f, int64_t L, const double* coeff, const double* offset, const double* center_phi,
                      double* lognum, double* mean, double* m1, double* m2, double* ma);

/* MANY observables along a scan (MBAR.compute_scan_expectations): a fit against hundreds of experimental numbers, a distribution
 * function with one observable per bin.  The observables are kept on the context, apart from the Q <= MBAR_SCAN_MAX_Q ones of
 * mbar_ctx_set_scan, and the sums are an (L x N)(N x Q) product on the fp64 matrix cores: the member operand is generated in
 * registers as in mbar_scan_gram_w, against tiles of 16 samples x up to 128 observables in LDS, so one member exponential serves
 * up to 128 observables.
 *   mbar_ctx_set_scan_obs   uploads Q >= 1 rows of N doubles (host rows of pitch ld_host >= N) into a block the context owns, at the
 *                           device pitch of the basis; the limit on Q is memory.  Q = 0 releases the block.  The block does not
 *                           depend on mbar_ctx_set_scan: it survives a change of basis, term kinds, centres and sample weights, and
 *                           is dropped at destroy or when replaced.  MBAR_ERR_ARG: a NULL pointer with Q > 0, Q < 0, ld_host < N, a
 *                           non-finite entry (the block on the context is left as it was).
 *   mbar_scan_obs_sums      on the family currently set (mbar_ctx_set_scan / mbar_ctx_set_scan_terms / mbar_ctx_set_scan_centers), with
 *                           b_ln = exp(f_scan[l] + x_ln) formed by the operations mbar_scan_gram_w uses for a member column, c_n the
 *                           multiplicities and a_qn the stored rows:
 *                             s1[l][q] = sum_n c_n b_ln a_qn          t1[l][q] = sum_n c_n b_ln^2 a_qn       (L x Q, row-major)
 *                             t2[l][q] = sum_n c_n b_ln^2 a_qn^2      wsum[l] = sum_n c_n b_ln               w2sum[l] = sum_n c_n b_ln^2
 *                           t1, t2 and w2sum are all NULL (only the first-moment launches run) or all non-NULL (else MBAR_ERR_ARG).
 * The members are taken in the panels of mbar_scan_gram_w, the observables in panels of 128 (the last one of 16, 32, 64 or 128
 * rows); one launch per pair of panels costs (members of the panel) x N exponentials and 2 x members x observables x N flop per
 * sum.  The resident matrix is read only through logden_n(f), and nothing of size L x N exists.  No floating-point atomics; chunks
 * of 8192 samples cut by N alone and merged in chunk order, compensated: two identical calls return identical bits, and element
 * (l, q) does not depend on L, Q, the other members or observables, where member l sits in the call or where row q sits among the
 * stored rows; s1 and wsum are the same bits with and without the second moments.  A NaN in f or f_scan fills the outputs with
 * NaN (MBAR_OK).  Limits, state and argument errors are those of mbar_scan_gram_w; MBAR_ERR_STATE also when no observables are set.
 * Kernel time: MBAR_TIMER_OTHER. */
int mbar_ctx_set_scan_obs(mbar_ctx* ctx, int64_t Q, const double* a_host, int64_t ld_host);
int mbar_scan_obs_sums(mbar_ctx* ctx, const double* f, int64_t L, const double* coeff, const double* offset, const double* f_scan,
                       double* s1, double* t1, double* t2, double* wsum, double* w2sum);

/* KERNEL-DENSITY surfaces along a scan (MBAR.compute_scan_kde): the gaussian density of every member of the family at M query points,
 * F(x; T) on a ladder or F(phi, psi; restraint centre), without a dense u_l, an upload or a weight evaluation per member.  The sums
 * are an (M x N)(N x L) product on the fp64 matrix cores with BOTH operands generated on the device: the member weight from the B
 * numbers per sample as in mbar_scan_obs_sums, the kernel value from the d coordinates per sample kept here.
 *   mbar_ctx_set_scan_points  uploads the d = 1 or 2 coordinates of the N samples (host rows of pitch ld_host >= N, coordinate-major)
 *                             into a block the context owns, at the device pitch of the basis.  d = 0 releases the block.  Like the
 *                             block of mbar_ctx_set_scan_obs it does not depend on mbar_ctx_set_scan and survives the other scan
 *                             calls.  MBAR_ERR_ARG: d outside [0, 2], a NULL pointer with d > 0, ld_host < N, a non-finite entry --
 *                             refused before the block on the context is touched.
 *   mbar_scan_kde_sums        on the family currently set, with b_ln = exp(f_scan[l] + x_ln) formed by the operations
 *                             mbar_scan_gram_w uses for a member column, c_n the multiplicities, q the M queries (coordinate-major,
 *                             d rows of M doubles), h = bandwidth and r the distance from x_n to q_m:
 *                               logsum[l][m] = log sum_n c_n b_ln exp(-r^2 / 2h^2)     (L x M, row-major)      wsum[l] = sum_n c_n b_ln
 *                             period: NULL or d entries, 0 = not periodic; where P > 0 the displacement of that coordinate is the
 *                             minimum image dl = q - x; dl = fma(-P, rint(dl / P), dl), the operations of a periodic harmonic term
 *                             (1 / P rounded once).  NULL and zeros are the same call.  The log density of member l is logsum[l][m] -
 *                             log wsum[l] + mbar_kde_log_norm(gaussian, d, h): the normaliser is the unwrapped kernel's.
 * The members are taken in the panels of mbar_scan_obs_sums, the queries in panels of 128 (the last one of 16, 32, 64 or 128); one
 * launch per pair of panels costs (members of the panel) x N member exponentials, (queries of the panel) x N kernel exponentials and
 * 2 x members x queries x N flop.  k <= 1 and c_n b_ln <= 1 for a normalised member, so the sums carry no running shift; a pair whose
 * sum is not >= 2^-900 (every term underflowed, or a NaN) of a member with wsum > 0 is recomputed in plain log space with its own
 * maximum, one workgroup per pair, fixed-order tree reductions: finite wherever a term is inside the fp64 range, -inf below it, never
 * NaN for finite input (a distance whose square overflows is measured in units of its largest coordinate); *n_exact: how many pairs
 * took this path.  A member with wsum = 0 keeps NaN.  No floating-point atomics; chunks of 8192 samples cut by N alone and merged in
 * chunk order, compensated: two identical calls return identical bits, and element (l, m) does not depend on L, M, the other members
 * or queries, or where member l and query m sit in the call.  A NaN in f or f_scan fills the outputs with NaN (MBAR_OK, *n_exact = 0).
 * Limits, state and argument errors are those of mbar_scan_gram_w; MBAR_ERR_STATE also when no points are set; MBAR_ERR_ARG: M < 1, a
 * non-finite query, a bandwidth that is not positive and finite (or whose 1 / 2h^2 is not), a negative or non-finite period.
 * Kernel time: MBAR_TIMER_OTHER. */
int mbar_ctx_set_scan_points(mbar_ctx* ctx, int64_t d, const double* x_host, int64_t ld_host);
int mbar_scan_kde_sums(mbar_ctx* ctx, const double* f, int64_t L, const double* coeff, const double* offset, const double* f_scan, int64_t M,
                       const double* q, double bandwidth, const double* period, double* logsum, double* wsum, int64_t* n_exact);

/* ---- histogram surfaces along a scan ---------------------------------------------------------
 * The histogram free energy surface of EVERY member of a scan: the bins are labels of the resident samples as in "histogram bins
 * by label", the target states are the members of the family uploaded by mbar_ctx_set_scan (with Q = 0).  Nothing of size L x N is
 * built or uploaded.  Same limits as the scan passes (single rank, normal row pitch, at most 128 states; else MBAR_ERR_STATE naming
 * the limit), and N < 2^31.  With x_ln and c_n as above and label_n in [-1, nbins) (-1: in no bin):
 *   mbar_ctx_set_scan_bins  validates the labels and sorts the samples by bin on the host, O(N), stable: perm (sorted position ->
 *                           sample, ascending n inside a bin, label -1 dropped) and bin_start[nbins + 1], both uploaded.  A chunk
 *                           is a run of sorted positions of ONE bin, cut from the start of the bin: at most 2048 positions in
 *                           pass A, 8192 in pass B; the chunk tables are a function of (label, N) alone.  nbins = 0 releases.
 *   mbar_scan_bins_table    the same perm (N entries of room, bin_start[nbins] of them written) and bin_start on the host: host
 *                           only, no context.
 *   mbar_scan_bin_lognum    pass A.  lognum[l][i] = log sum_{n in i} c_n exp(x_ln) (L x nbins), every (member, bin) pair referred
 *                           to its OWN maximum; -inf where no sample of the bin has c_n > 0.  The bin free energy of member l is
 *                           -lognum[l][i].  Never reads the matrix.  offset NULL: zeros.
 *   mbar_scan_bin_gram_w    pass B.  Bv = exp(f_bins[l][i] + x_ln) for n in i, W_nk = exp(f_k - u_kn - logden_n):
 *                           cross[k][l][i] = sum_{n in i} c_n W_nk Bv (K x L x nbins; NULL: not computed) on the fp64 matrix cores,
 *                           the W tile gathered through perm and the Bv operand generated in registers; diag[l][i] = sum c_n Bv^2,
 *                           wsum[l][i] = sum c_n Bv (1 at f_bins = -lognum).  f_bins[l][i] = +inf (an empty bin) gives exact zeros.
 *                           The samples in bins are read once per panel of 256 members.  The partial records of one sweep are
 *                           bounded by "scan_part_bytes": above it the bins are processed in groups of whole bins, one sweep per
 *                           group (a single bin is never split).
 * No floating-point atomics.  A (member, bin) output depends on that member and on the bin's own samples in ascending n only: not
 * on the other members, the other bins, the bin's number, the panel cut or "scan_part_bytes".  With nbins = 1 and every label 0
 * pass A returns the bits of mbar_scan_lognum's lognum and pass B those of mbar_scan_gram_w's cross[:, :, 0], within[:, 0] and
 * wsum: the same chunk cut, the same operations.  Kernel time: MBAR_TIMER_OTHER. */
int mbar_ctx_set_scan_bins(mbar_ctx* ctx, int64_t nbins, const int32_t* label_host);
int mbar_scan_bins_table(int64_t N, int64_t nbins, const int32_t* label, int32_t* perm_out, int64_t* bin_start_out);
int mbar_scan_bin_lognum(mbar_ctx* ctx, const double* f, int64_t L, const double* coeff, const double* offset, double* lognum);
int mbar_scan_bin_gram_w(mbar_ctx* ctx, const double* f, int64_t L, const double* coeff, const double* offset, const double* f_bins,
                         double* cross, double* diag, double* wsum);

/* ---- extension contexts: rows appended to a resident matrix without a copy of it ------------
 * The general path of the expectation family (pymbar/mbar.py:886-903 builds an N x (K + NL + S) host array of log weights;
 * rounds 3-5 of this library copied the resident matrix device to device into a (K + NL + S)-row one per call).  An extension
 * context holds ONLY the new rows (new states, observables as unsampled states) -- same device, samples and row pitch as `base`,
 * its storage a whole number of row pitches away from base's -- and the sweeps below read [rows of base | rows of ext]:
 *   mbar_ctx_create_ext      base of at most 128 states on one rank, 129 .. 256 rows in total (else MBAR_ERR_ARG: the caller
 *                            falls back to an augmented copy); rows are written with mbar_ctx_upload_rows / mbar_ctx_copy_rows /
 *                            mbar_ctx_rows_logshift / mbar_ctx_vec_logshift on the extension and the three calls below;
 *   mbar_ctx_rows_sub_from   dst rows = src rows - v  (src = dst or its base; v as in mbar_ctx_rows_sub);
 *   mbar_ctx_rows_rsub_from  dst rows = src rows - dst rows;
 *   mbar_ctx_rows_obs_from   dst rows = base rows[state_row0 ..) - log(base rows[obs_row0 ..) - shift_r), shift_r as in
 *                            mbar_ctx_rows_logshift, handed back (observables that ARE resident rows: entropy / enthalpy); min_out /
 *                            min_in (or NULL): the rows' minima out of one call and into the next on the same resident rows, which
 *                            then skips the pass that finds them;
 *   mbar_lognum_ext          log normalisers of the extension's rows at f_base (the base's log-denominators / multiplicities);
 *   mbar_gram_w_ext          W^T W of [base | ext] at (f_base, f_ext), (K_base + K_ext)^2 row-major, ONE one-read sweep of both
 *                            matrices (k_gram_quad_split); wsum as in mbar_gram_w (N_k = 0 for the extension's rows).  gram_base
 *                            (or NULL) = mbar_gram_w of the base at f_base, kept by the caller: with it and at most 16 appended
 *                            rows only the new entries are computed (a 16 x 128 rectangle + a 16 x 16 block);
 * Evaluations and solves on an extension context fail with MBAR_ERR_STATE; destroy it before its base. */
int mbar_ctx_create_ext(mbar_ctx** out, mbar_ctx* base, int64_t K_rows);
int mbar_ctx_rows_sub_from(mbar_ctx* dst, int64_t dst_row0, mbar_ctx* src, int64_t src_row0, int64_t nrows, const double* v_host);
int mbar_ctx_rows_rsub_from(mbar_ctx* dst, int64_t dst_row0, mbar_ctx* src, int64_t src_row0, int64_t nrows);
int mbar_ctx_rows_obs_from(mbar_ctx* dst, int64_t dst_row0, mbar_ctx* base, int64_t state_row0, int64_t obs_row0, int64_t nrows,
                           double* shift_out, const double* min_in, double* min_out);
int mbar_lognum_ext(mbar_ctx* ext, mbar_ctx* base, const double* f_base, double* lognum_ext);
int mbar_gram_w_ext(mbar_ctx* ext, mbar_ctx* base, const double* f_base, const double* f_ext, const double* gram_base, double* gramW,
                    double* wsum);

/* ---- solver loops (replace adaptive(), mbar_solvers.py:510-667) ---------------------------- */
typedef struct mbar_solve_result {
    int64_t iterations; /* iterations executed                                   */
    int64_t nr_iter;    /* ... of which Newton-Raphson steps were accepted       */
    int64_t sci_iter;   /* ... of which self-consistent steps were accepted      */
    int32_t success;    /* convergence test of mbar_solvers.py:636 met           */
    int32_t gram_sweeps; /* separate Gram sweeps executed (fused loop: rejected speculations only)     */
    double max_delta;   /* last relative change                                  */
    double gnorm;       /* |g| at the returned f                                 */
    double wall_ms;     /* host wall time of the loop                            */
    int32_t warm_starts; /* device-resident loop entries that re-used the resident probability matrix of an earlier solve */
    int32_t builds;      /* ... that built it (build sweep)                       */
    int32_t light_sweeps; /* fused loop: iterations whose sweep ran WITHOUT the speculated Gram matrix because both candidates already
                           * met the stop test against the current f (the last iteration of a solve; option "light_last") */
    int32_t fused_unit;   /* device-resident loop entries whose fused sweep was the kernel specialised for unit sample multiplicities
                           * (a context without sample weights, up to 128 states, option "fused_general" = 0); 0: the general kernel */
} mbar_solve_result;

/* Adaptive NR/SCI on the states with N_k > 0 (others are left untouched).  f_inout[K].
 * history (may be NULL): rows of 4 doubles {choice(0 sci,1 nr), |g_sci|, |g_nr|, max_delta}.
 * check_convergence = 0 runs exactly maxiter iterations (benchmarking).
 * Up to 256 states the whole iteration is device-resident: K x K Newton solve (up to 128 states in one workgroup's
 * registers, 129 .. 256 by a blocked Cholesky factorisation in device memory), candidate construction, ONE fused sweep for
 * both candidates' gradients and the next Hessian's Gram matrix, choice and convergence test; the host reads a few control
 * words per batch of iterations (replayed from a hipGraph on a single rank), with ONE ncclAllReduce on the stream per
 * iteration across ranks; when the accepted candidate is not the one the sweep speculated on, the loop pauses and the host
 * enqueues that candidate's Gram sweep.  With the host all-reduce transport, above 256 states, or when the device hands a
 * solve back (Newton system not positive definite, candidates > 250 kT from the anchor of the sweeps, non-finite candidate)
 * the same iteration runs host-driven. */
int mbar_solve_adaptive(mbar_ctx* ctx, double* f_inout, double tol, int64_t maxiter,
                        int64_t min_sc_iter, double gamma, int check_convergence,
                        double* history, int64_t history_rows, mbar_solve_result* result);
/* psum[k] = sum_n p_nk at the f the last mbar_solve_adaptive on this context returned (its gradient is psum - N_k, the
 * all-state self-consistent update of sampled states f - log(psum / N_k)): what mbar_solvers.py:939 and :1012 recompute
 * with one more sweep each after a solve.  MBAR_ERR_STATE when there is none (no solve yet, or the matrix / N_k / the sample
 * weights changed since). */
int mbar_ctx_last_solve_psum(mbar_ctx* ctx, double* psum);
/* Pure self-consistent iteration, device-resident (f update and convergence measure on the
 * device).  K <= 32 on one rank: ONE launch per iteration (the update rides in the prologue of the sweep); odd iterations
 * sweep the tiles in descending order ("sci_pingpong": a sweep starts with what the previous one left in the caches).  The
 * host looks at the relative changes after the first batch ("sci_batch", 16) and then after as many iterations as their
 * geometric decay predicts are left (at most 256); without the convergence test it does not look until the end. */
int mbar_solve_sci(mbar_ctx* ctx, double* f_inout, double tol, int64_t maxiter, int check_convergence,
                   mbar_solve_result* result);

/* ---- measurement --------------------------------------------------------------------------- */
/* Accumulated HIP-event time and launch count of one kernel class since the last reset. */
int mbar_ctx_timing(mbar_ctx* ctx, int which, double* total_ms, int64_t* launches);
int mbar_ctx_timing_reset(mbar_ctx* ctx);
/* Peak-rate micro-benchmark of v_mfma_f64_16x16x4_f64 on this device (TFLOP/s). */
int mbar_mfma_f64_peak(mbar_ctx* ctx, double* tflops);

/* ---- weighted kernel-density sums (pymbar_amd.kde.KernelDensity, fes_type="kde" of pymbar_amd.FES) ----------------------
 * A handle holds N samples of dimension d (1 <= d <= 8) resident on one device, one kernel and one bandwidth h, and C columns
 * of non-negative sample weights V (N x C).  mbar_kde_eval returns for M query points
 *     L[m, c] = log sum_n V[n, c] k_h(|q_m - x_n|) - log sum_n V[n, c] + log-normaliser(kernel, d, h)
 * (euclidean distance), which is what sklearn.neighbors.KernelDensity(kernel, bandwidth=h).fit(X, sample_weight=V[:, c])
 * .score_samples(Q) computes -- exactly: the sum runs over every pair, in log space with a running per-query shift, so the log
 * density stays finite and exact where every term underflows (gaussian / exponential far from the data).  Compact kernels
 * give -inf where no sample of positive weight lies strictly inside the support (|q - x| < h, sklearn's convention), a column of
 * zero total weight gives NaN.  Two identical calls return identical bits (partial sums merged in a fixed order).  Columns are
 * processed in passes of up to 32: device memory is (d + min(C, 32)) N doubles plus O(M) per pass; with C <= 32 the weights stay
 * resident between calls.  Buffers come from the block cache of mbar_cache_trim.  Errors: mbar_last_error(NULL).
 * Not thread-safe (one handle per caller thread). */
typedef struct mbar_kde mbar_kde;
#define MBAR_KDE_GAUSSIAN 0
#define MBAR_KDE_TOPHAT 1
#define MBAR_KDE_EPANECHNIKOV 2
#define MBAR_KDE_EXPONENTIAL 3
#define MBAR_KDE_LINEAR 4
#define MBAR_KDE_COSINE 5
/* x: N x d row-major host array (finite), bandwidth > 0.  The weights start as one column of ones. */
int mbar_kde_create(mbar_kde** out, int device, int kernel, int d, int64_t N, const double* x, double bandwidth);
void mbar_kde_destroy(mbar_kde* kde);
/* v: N x C row-major host array, finite and >= 0 (zero weights are legal and contribute nothing). */
int mbar_kde_set_weights(mbar_kde* kde, int64_t C, const double* v);
/* q: M x d row-major host array (finite); out: M x C row-major host array of log densities. */
int mbar_kde_eval(mbar_kde* kde, int64_t M, const double* q, double* out);
/* Options of a handle.  "max_chunks": the largest number of sample chunks (workgroups along the samples) of the next
 * mbar_kde_eval calls; 0 (default): ceil(4 num_cu / query blocks), any value >= 1 caps that number (it stays at most the number
 * of 64-sample tiles).  Results for different cuts agree to rounding; for one cut they are the same bits from call to call.
 * An unknown key or a negative value is MBAR_ERR_ARG. */
int mbar_kde_set_option(mbar_kde* kde, const char* key, int64_t value);
/* The log-normaliser log(1 / integral of k_h over R^d) the library adds (host only; tests / documentation). */
int mbar_kde_log_norm(int kernel, int d, double bandwidth, double* out);

/* ---- lagged fluctuation sums of a timeseries (pymbar_amd.timeseries) ---------------------------------------------------------
 * A handle holds T values of a series A (and of B for a cross-correlation; NULL: the autocorrelation) resident on one device,
 * split into K segments of lengths seg[0..K) (sum T; K = 1 for one series).  The device holds A' = A - shift_a, B' = B - shift_b;
 * products A'_n B'_(n+t) never cross a segment boundary.  Every sum is double-double with a fixed reduction order: two identical
 * calls return identical bits.  Device memory: about 40 bytes per value, plus 48 bytes per origin of a rule.  Errors:
 * mbar_last_error(NULL).  Not thread-safe (one handle per caller thread).
 *
 * For an origin s of one series (N = T - s values, suffix means mu_A, mu_B of A[s:], B[s:]) and lag t < N:
 *     X_AB(s, t) = sum_{n = s}^{T-1-t} (A_n - mu_A)(B_(n+t) - mu_B),   X_BA likewise with A and B exchanged.
 * The stopping rule of pymbar.timeseries.statistical_inefficiency runs on the device, one thread per origin:
 *     sigma2 = X_AB(s, 0) / N;  then for t = 1, 2, 3, ... (fast: 1, 2, 4, 7, 11, ... with increment 1, 2, 3, ...) while t < N - 1
 *     (fft: t < N): C = (X_AB + X_BA) / (2 (N - t) sigma2); stop when C <= 0 and t > mintime; g += 2 C (1 - t / N) increment;
 *     finally g = max(g, 1).
 * status: 1 = stopped by the C test at lag stop[o] (the last lag evaluated), 3 = ran to the end (stop[o]: the first lag not
 * evaluated), 2 = zero variance (the suffix is constant, or sigma2 == 0): g = 1, the caller decides. */
typedef struct mbar_acf mbar_acf;
int mbar_acf_create(mbar_acf** out, int device, int64_t T, const double* a, const double* b, int64_t K, const int64_t* seg,
                    double shift_a, double shift_b);
void mbar_acf_destroy(mbar_acf* acf);
/* The rule at every origin s = o nskip < T - 1 (o < (T - 2) / nskip + 1; K must be 1); g, stop, status: one entry per origin
 * (stop, status may be NULL).  With fft the rule runs with fast off and through t = N - 1. */
int mbar_acf_suffix_g(mbar_acf* acf, int64_t nskip, int fast, int64_t mintime, int fft, double* g, int64_t* stop, int32_t* status);
/* The rule of statistical_inefficiency_multiple over the K segments (autocorrelation; shift_a must be the mean of all values):
 * sigma2 = sum A'^2 / T, C = (sum of the valid products / their count) / sigma2, loop while t < max N_k - 1, weight
 * (1 - t / (T / K)).  ct (or NULL): C by schedule entry (entry 0 is lag 0, not written), ct_cap >= mbar_acf_schedule_length(fast,
 * max N_k); entries up to the stop are written. */
int mbar_acf_multiple_g(mbar_acf* acf, int fast, int64_t mintime, double* g, int64_t* stop, int32_t* status, int64_t ct_cap,
                        double* ct);
/* Entries of the lag schedule with a lag below tmax, lag 0 included (host only). */
int mbar_acf_schedule_length(int fast, int64_t tmax, int64_t* out);
/* Raw lag sums for nlags lags and norig increasing origins; xab, xba: [nlags][norig] (xba may be NULL).  segments == 0 (K = 1):
 * X_AB(s, t), X_BA(s, t) about the suffix means, 0 for t >= N.  segments != 0: sum over n in [o_i, o_(i+1)) (o_norig = T) of
 * A'_n B'_(n+t) (B'_n A'_(n+t)) over the valid pairs, about the shifts. */
int mbar_acf_lag_sums(mbar_acf* acf, int64_t nlags, const int64_t* lags, int64_t norig, const int64_t* origins, int segments,
                      double* xab, double* xba);

/* ---- BAR and EXP estimators (pymbar_amd.other_estimators) -----------------------------------------------------------------
 * A handle holds P independent problems resident on one device: problem p has n_f[p] forward work values and n_r[p] reverse
 * ones (w_f, w_r: the problems' values concatenated in order).  Each side is cut into chunks of MBAR_BAR_CHUNK values, fixed
 * whatever P and the other problems are; chunk partials merge in a fixed order, so two identical calls return identical bits and
 * a problem's answer does not depend on the batch it is in.  Values may be +inf (a Fermi factor / exp(-w) of 0); NaN and -inf are
 * rejected.  A side may be empty only for the one-sided moments (mbar_bar_moments); the BAR calls need both sides.
 *
 * With M = log(n_f / n_r), x_F = M + w_F - DeltaF and x_R = w_R + DeltaF - M:
 *     log_numer = log sum_F 1 / (1 + exp(x_F)),   log_denom = log sum_R 1 / (1 + exp(x_R)),   F(DeltaF) = log_numer - log_denom,
 * each sum in log space with a per-chunk shift fixed by the chunk's minimum w (the largest term), so no term is lost to
 * overflow or underflow.  log_numer2 / log_denom2 are the same sums of the squared factors.  Errors: mbar_last_error(NULL). */
#define MBAR_BAR_CHUNK 4096
/* state of the reference's BAR root find for one problem (bar(), other_estimators.py), advanced by mbar_bar_step_host on the
 * host and by the same function on the device.  Callers fill method (0 false-position, 1 bisection, 2 self-consistent
 * iteration), iterated, maximum_iterations, relative_tolerance, DeltaF (the start) and, for methods 0 / 1, UpperB / LowerB (the
 * bracket: exp(w_F) and -exp(w_R)); everything else zero.  want_moments: after a normal end, one more pass stores
 * moments = (log_numer, log_denom, log_numer2, log_denom2) at DeltaF (iterated) or DeltaF_initial. */
typedef struct mbar_bar_state {
    double DeltaF, DeltaF_old, DeltaF_initial, UpperB, LowerB, FUpperB, FLowerB, FNew, relative_change, relative_tolerance;
    double req[2];          /* the DeltaF values the next pass evaluates (nreq of them) */
    double moments[4];
    int64_t method, iterated, maximum_iterations, iteration, phase, status, nreq, nzero, want_moments, moments_pending;
} mbar_bar_state;
/* status: 0 running, 1 ended normally, 2 NaN at a bracket end (Delta_f = 0), 3 no bound on the root (BoundsError),
 * 4 iteration limit (ConvergenceError).  nzero: evaluations of F so far. */
typedef struct mbar_bar mbar_bar;
int mbar_bar_create(mbar_bar** out, int device, int64_t P, const int64_t* n_f, const double* w_f, const int64_t* n_r,
                    const double* w_r);
void mbar_bar_destroy(mbar_bar* bar);
/* out[p][5] = (F, log_numer, log_denom, log_numer2, log_denom2) at DeltaF = deltaf[p], every problem in one pass. */
int mbar_bar_zero(mbar_bar* bar, const double* deltaf, double* out);
/* Runs the root find of every problem to its end on the device: states[P] in (initial), out (final); passes: evaluation passes
 * enqueued (or NULL).  The host reads only the status block between groups of passes. */
int mbar_bar_solve(mbar_bar* bar, mbar_bar_state* states, int64_t* passes);
/* One-sided moments of every side s = 2 p + (0 forward, 1 reverse), out[s][5]:
 *     (logsumexp(-w), sum x, sum (x - mean x)^2, sum w, sum (w - mean w)^2),  x = exp(-w - max(-w)), means over the side.
 * An empty side gives (-inf, 0, 0, 0, 0). */
int mbar_bar_moments(mbar_bar* bar, double* out);
/* Advances one state on the host with the same function the device runs: F[0..nreq) are F at req[0..nreq) (ignored in the
 * first call, which issues the first requests).  Returns the status.  Needs no GPU. */
int mbar_bar_step_host(mbar_bar_state* state, const double* F);

/* ---- weighted B-spline moments (fes_type="spline" of pymbar_amd.FES) ---------------------------------------------------------
 * A handle holds N samples x (finite) resident on one device, optional group labels g (N values in [0, G), G <= 1024; default
 * one group) and C columns of finite sample weights V (N x C).  mbar_bspline_moments returns, for a knot vector t of nbasis + k + 1
 * non-decreasing finite values (0 <= k <= 7, k + 1 <= nbasis <= 1024),
 *     M[g, c, i] = sum over the samples n with g_n = g of V[n, c] B_{i,k,t}(x_n),   i = 0 .. nbasis - 1,
 * with B_{i,k,t} the basis element scipy.interpolate.BSpline(t, e_i, k) evaluates with extrapolate=True: samples below t[k] use
 * the first polynomial piece, samples at or above t[nbasis] the last one.  The partial sums are merged in a fixed order without
 * floating-point atomics: two identical calls return identical bits.  Columns are processed in passes of up to 32; with C <= 32
 * the weights stay resident between calls.  Errors: mbar_last_error(NULL).  Not thread-safe (one handle per caller thread). */
typedef struct mbar_bspline mbar_bspline;
/* x: N host values (finite).  The handle starts with one group and one column of ones. */
int mbar_bspline_create(mbar_bspline** out, int device, int64_t N, const double* x);
void mbar_bspline_destroy(mbar_bspline* bs);
/* g: N host labels in [0, G) (NULL: every sample in group 0 and G = 1). */
int mbar_bspline_set_groups(mbar_bspline* bs, int G, const int* g);
/* v: N x C row-major host array of finite weights. */
int mbar_bspline_set_weights(mbar_bspline* bs, int64_t C, const double* v);
/* t: nbasis + k + 1 host knots; out: G x C x nbasis row-major host array. */
int mbar_bspline_moments(mbar_bspline* bs, int k, int nbasis, const double* t, double* out);
/* Device time of the last mbar_bspline_moments call's kernels (all passes, HIP events), in ms. */
int mbar_bspline_kernel_ms(mbar_bspline* bs, double* ms);

/* ---- many small MBAR problems in one call (pymbar_amd.mbar_batch) -----------------------------------------------------------
 * A handle holds P independent problems resident on one device: problem p is a K[p] x N[p] row-major block of reduced
 * potentials (1 <= K[p] <= MBAR_BATCH_MAX_K, N[p] >= 1; u: the blocks concatenated in order; +inf allowed, NaN and -inf
 * rejected).  Each problem's columns are cut into chunks of MBAR_BATCH_CHUNK, fixed whatever the other problems are; chunk
 * partials merge in a fixed order without atomics, so two identical calls return identical bits and a problem's answer does
 * not depend on the batch it is in.  The adaptive loop of mbar_solvers.py:575-640 runs per problem as a resumable state machine
 * (mbar_batch_step_host on the host, the same function on the device).  Bootstrap replicates of the problems are solved as
 * replica slots over the same resident blocks (below).  Errors: mbar_last_error(NULL).  Not thread-safe (one handle per caller
 * thread). */
#define MBAR_BATCH_MAX_K 64
#define MBAR_BATCH_CHUNK 256
/* One problem's solve.  Callers fill K, Nk (samples per state, zeros allowed, at least one > 0), f (the start), tol, gamma,
 * maxiter, min_sc_iter; everything else zero.  lognum[k] = log sum_n exp(-logden_n - u_kn) at f for every state k and
 * psum[k] = N_k exp(f_k + lognum_k) when the solve has ended.  status: 0 running, 1 ended (success: converged), 2 a Newton pivot
 * counted as zero or was not finite (the caller finishes the problem on the host). */
typedef struct mbar_batch_state {
    double f[MBAR_BATCH_MAX_K];
    double req[2][MBAR_BATCH_MAX_K];  /* the f vectors the next pass evaluates (nreq of them; [0] f_sci, [1] f_nr) */
    double lognum[MBAR_BATCH_MAX_K];
    double psum[MBAR_BATCH_MAX_K];
    double Nk[MBAR_BATCH_MAX_K];
    double x[MBAR_BATCH_MAX_K];       /* Newton direction of the live states (between the two halves of a step) */
    double tol, gamma, max_delta, max_diff, gnorm_sci, gnorm_nr;
    int64_t K, maxiter, min_sc_iter, iterations, nr_iter, sci_iter, choices; /* choices: bit i = 1 when iteration i took NR */
    int64_t phase, status, success, nreq, gram_req, gram_w, newton_bad;
} mbar_batch_state;
typedef struct mbar_batch mbar_batch;
/* u[p]: host pointer to problem p's K[p] x N[p] row-major block. */
int mbar_batch_create(mbar_batch** out, int device, int64_t P, const int64_t* K, const int64_t* N, const double* const* u);
void mbar_batch_destroy(mbar_batch* b);
/* Runs every problem's solve to its end: states[P] in (initial), out (final); passes: evaluation passes enqueued (or NULL).
 * The host reads one int per problem between groups of passes. */
int mbar_batch_solve(mbar_batch* b, mbar_batch_state* states, int64_t* passes);
/* For the problems with mask[p] != 0, at f[p][0 .. K[p]) (the final free energies, every state): gram = W^T W (K[p] x K[p]) and
 * wsum = sum_n W_nk, packed problem after problem (K[p]^2 resp. K[p] doubles each; entries of masked-out problems untouched). */
int mbar_batch_gram_w(mbar_batch* b, const double* f, const int32_t* mask, double* gram, double* wsum);
/* One step of a state on the host with the same state machine the device runs: lognum[r][K] = lognum at req[r] for the nreq
 * requests of the last pass (ignored in the first call, which issues the first requests), gram[K][K] = sum_n p_ni p_nj
 * (p_nk = N_k W_nk) at req[gram_req] (NULL when gram_req < 0).  Returns the status.  Needs no GPU. */
int mbar_batch_step_host(mbar_batch_state* state, const double* lognum, const double* gram);

/* ---- replica slots: bootstrap replicates solved next to the problems they resample ------------------------------------------
 * A slot is a solve that shares the resident block, K, N and chunking of a base problem and has its own chunk records, its own
 * mbar_batch_state and per-sample multiplicities c_n >= 0: every sum over samples becomes sum_n c_n (...), the log-denominator of
 * a sample is unchanged, and a chunk with no drawn sample contributes nothing.  A bootstrap replicate (mbar.py:417-449) is the
 * vector of draw counts: nothing is gathered, no block is copied.  The state machine is that of the problems (mbar_batch_step_host).
 * A slot's result depends on its problem, its multiplicities and its start alone; two identical calls return identical bits.
 *
 * mbar_batch_set_replicas declares R slots (replacing earlier ones; R = 0 releases them): base[s] is slot s's problem,
 * Nk[p][MBAR_BATCH_MAX_K] the samples per state of problem p (read for the problems that are some slot's base; they must sum
 * to N[p]), which fix the default layout of the draws -- the states' runs in order.  Multiplicities start as 1.  The device memory of
 * the multiplicities (N doubles per slot), records and states is checked up front (MBAR_ERR_ARG with the sizes in the message). */
int mbar_batch_set_replicas(mbar_batch* b, int64_t R, const int64_t* base, const int64_t* Nk);
/* Slot `slot`'s multiplicities from a host vector of N[base[slot]] doubles, finite and >= 0 (as mbar_ctx_set_sample_weights). */
int mbar_batch_replica_set_weights(mbar_batch* b, int64_t slot, const double* c_n);
/* The multiplicities of the slots first .. first + count drawn ON THE DEVICE in one launch: slot first + i gets the draw counts of
 * replicate replicate[i] of the counter-based stream seed[i] over the default layout -- the draws mbar_bootstrap_draws(seed[i],
 * replicate[i], cumN, K, NULL, .) returns on the host.  Counts are exact integers held as doubles (sums of 1.0). */
int mbar_batch_replicas_draw(mbar_batch* b, int64_t first, int64_t count, const uint64_t* seed, const int64_t* replicate);
/* mbar_batch_solve for the slots: states[R] in (initial), out (final). */
int mbar_batch_replicas_solve(mbar_batch* b, mbar_batch_state* states, int64_t* passes);
/* mbar_batch_gram_w for the slots: gram = sum_n c_n W_ni W_nj and wsum = sum_n c_n W_nk at f[s][0 .. K), packed slot after slot. */
int mbar_batch_replicas_gram_w(mbar_batch* b, const double* f, const int32_t* mask, double* gram, double* wsum);

/* ---- extension rows: the expectation family of a batch (pymbar_amd.MBARBatch) --------------------------------------------------
 * Problem p gets R[p] >= 0 extension rows, an R[p] x N[p] row-major block of reduced potentials e_rn resident next to its own
 * block: new states and observables written as states with no samples (expectations.py), which do not enter the log-denominator.
 * K[p] + R[p] <= MBAR_BATCH_MAX_AUG; +inf allowed, NaN and -inf rejected.  The two passes below read N_k from the problems' states
 * as mbar_batch_solve left them on the device (as mbar_batch_gram_w does) and take f[p][0 .. K[p]) in rows of MBAR_BATCH_MAX_K;
 * per-row values (lognum_ext, f_ext) are packed problem after problem, R[p] doubles each.  Same rules as the passes above: chunks
 * of MBAR_BATCH_CHUNK samples, no atomics, partials merged in chunk order, so two identical calls return identical bits and a
 * problem's bits depend neither on the batch it is in nor on the grouping of the Gram pass.
 *
 * mbar_batch_set_ext replaces any earlier rows (R = NULL releases them); e[p] may be NULL where R[p] = 0.  The
 * device memory of the rows and their chunk records is checked up front (MBAR_ERR_ARG with the sizes in the message); a call
 * that is rejected (MBAR_ERR_ARG) leaves the earlier rows in place. */
#define MBAR_BATCH_MAX_AUG 128
int mbar_batch_set_ext(mbar_batch* b, const int64_t* R, const double* const* e);
/* lognum_ext[p][r] = log sum_n exp(-logden_n(f) - e_rn) for the problems with mask[p] != 0 (log space, the chunk maximum as the
 * shift; a row whose terms are all zero gives -inf; entries of masked-out problems untouched). */
int mbar_batch_ext_lognum(mbar_batch* b, const double* f, const int32_t* mask, double* lognum_ext);
/* gram = Q^T Q ((K[p] + R[p])^2 doubles per problem, bit-symmetric) and wsum = the column sums of Q (K[p] + R[p] doubles), packed
 * problem after problem, for the problems with mask[p] != 0.  Q_nk = exp(f_k - u_kn - logden_n) for the K[p] states (W of
 * mbar_batch_gram_w), then exp(f_ext_r - e_rn - logden_n) for the rows (f_ext finite).  A workgroup owns MBAR_BATCH_EXT_RUN
 * consecutive chunks of a problem and writes one partial record for them; the problems are swept in groups whose records take at
 * most group_bytes of device memory (at least one problem per group; <= 0: no limit). */
#define MBAR_BATCH_EXT_RUN 4
int mbar_batch_ext_gram(mbar_batch* b, const double* f, const double* f_ext, const int32_t* mask, int64_t group_bytes, double* gram,
                        double* wsum);

#ifdef __cplusplus
}
#endif
#endif /* MBAR_HIP_H */
