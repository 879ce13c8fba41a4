// Internal header of the host side of libmbar_hip.so (not part of the public ABI): the context, its timers, and the
// helpers the translation units of the context layer share, one file per role:
//   mbar_capi.cpp   context lifecycle and buffers (constructors, destroy, ensure / reserve, options, N_k, sample weights,
//                   bootstrap draws, timing)
//   mbar_eval.cpp   the evaluation engine (run_lse, the Gram plans, run_gram, eval_core) and the evaluation entry points
//   mbar_rows.cpp   every writer of the resident matrix, and its download
//   mbar_ext.cpp    the entry points that take an extension context and its base
//   mbar_loops.cpp  the two solve entry points, the self-consistent loop, and what the solver loops share
//   mbar_loop_device.cpp, mbar_loop_host.cpp  the adaptive loop the reference writes in Python: device-resident, host-driven
//   mbar_scan.cpp, mbar_hist.cpp  the scan passes and the binned passes
//   mbar_comm.cpp   RCCL loader, in-process transport, all-reduce
//   mbar_host.cpp   allocator state and the handle layer's definitions, host-side K x K linear algebra, content digest
// The handles of the other backends (mbar_kde.cpp, mbar_acf.cpp, mbar_bar.cpp, mbar_bspline.cpp, mbar_batch.cpp) use the layer
// below the context alone, mbar_handle.h: Handle, DevBuf, create_handle / destroy_handle, ColumnPasses, run_passes.
#pragma once
#include "mbar_handle.h"
#include "mbar_internal.h"
#include "mbar_scan.h"  // (FamilyTerms, a member of the context)

#include <dlfcn.h>
#include <sched.h>
#include <unistd.h>
#include <rccl/rccl.h>

#include <chrono>
#include <condition_variable>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <limits>
#include <memory>
#include <thread>

namespace mbar {
namespace host {

struct RcclApi {
    void* handle = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    bool load(std::string& err) {
        if (handle) return true;
        const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        for (const char* n : names) {
            handle = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
            if (handle) break;
        }
        if (!handle) {
            err = std::string("dlopen(librccl) failed: ") + dlerror();
            return false;
        }
        GetUniqueId = (decltype(GetUniqueId))dlsym(handle, "ncclGetUniqueId");
        CommInitRank = (decltype(CommInitRank))dlsym(handle, "ncclCommInitRank");
        AllReduce = (decltype(AllReduce))dlsym(handle, "ncclAllReduce");
        CommDestroy = (decltype(CommDestroy))dlsym(handle, "ncclCommDestroy");
        GetErrorString = (decltype(GetErrorString))dlsym(handle, "ncclGetErrorString");
        if (!GetUniqueId || !CommInitRank || !AllReduce || !CommDestroy) {
            err = "librccl is missing a required symbol";
            return false;
        }
        return true;
    }
};
extern RcclApi g_rccl;

struct TimerPair {
    hipEvent_t a, b;
    int which;
};

}  // namespace host
}  // namespace mbar
using mbar::host::TimerPair;

// In-process transport: the contexts of several caller threads on ONE device meet in a stream-ordered all-reduce (events
// across their streams, a rendezvous of the host threads per collective, no host-device synchronisation).  It drives exactly
// the code a RCCL communicator drives -- the collective sits on the compute stream, so the device-resident loop runs across
// "ranks" -- and exists so that this code can be tested on a one-GPU box (RCCL refuses two ranks on one device).
struct mbar_loopback {
    int nranks = 0, device = -1;
    std::mutex mu;
    std::condition_variable cv;
    int arrived = 0;
    uint64_t gen = 0;
    bool broken = false;
    std::vector<const double*> src;
    std::vector<int64_t> cnt;
    std::vector<int> op;
    std::vector<hipEvent_t> ready, done;
    std::vector<double*> tmp;
    std::vector<size_t> tmp_doubles;
    std::vector<int> attached;
};

// Histogram bins by label (mbar_ctx_set_bins): the chunk table of one tile of bins on the device (mbar_hist.cpp)
struct HistTile {
    int64_t b0 = 0, b1 = 0, nchunks = 0, nrec = 0;
    DevBuf<int64_t> chunk_n, chunk_rec, bin_ptr, bin_rec;
    DevBuf<uint8_t> slot;
};

struct mbar_ctx {
    int device = 0;
    int num_cu = 256;
    hipStream_t stream = nullptr;
    int64_t K = 0, Kp = 0, N = 0, ld = 0;
    bool have_Nk = false;
    bool u_checked = false, u_poison = false;  // NaN / -inf entries found in the matrix
    // logden[0] holds the per-sample log-denominators of THIS f (for the current matrix and N_k): the class methods ask for the
    // log-space numerators, W^T W, log W ... at the same f_k one after the other, and each would otherwise begin with the same
    // evaluation sweep (config 3: 1.9 ms each, five of them in one compute_expectations call)
    std::vector<double> ld0_f;
    bool ld0_valid = false;
    bool u_posinf = true;                      // +inf entries (legal) may be present: keep the exponentials clamped
    std::vector<double> Nk, lnNk;   // K
    std::vector<int> sampled;       // indices with N_k > 0
    // device: every DevBuf member owns its block of the cache and gives it back when the context is deleted (mbar_ctx_destroy
    // drains the stream first); the raw pointers next to them are views into those blocks
    DevBuf<double> u_alloc;         // the matrix's allocation
    double* u = nullptr;            // ... and the matrix: the allocation's start, or (extension contexts) the first address in it
                                    // that lies a whole number of row pitches from the base's matrix
    mbar_ctx* ext_base = nullptr;   // extension contexts (mbar_ctx_create_ext): the context whose rows theirs are appended to
    DevBuf<double> logden_alloc;    // three logden vectors in ONE allocation ...
    double* logden[3] = {nullptr, nullptr, nullptr};  // ... and the three slots in it
    DevBuf<double> dn;              // objective offsets (or null)
    DevBuf<double> cw;              // per-sample multiplicities (ld doubles; 1 on data, 0 on padding by default)
    DevBuf<double> lden_eff;        // logden - alpha ln c for the kernels that consume logden (only when weighted)
    bool weighted = false;
    DevBuf<double> small;           // aden[2][Kp] | anum[Kp] | f[Kp] | Nk[Kp] | lnNk[Kp] | delta[...]
    DevBuf<double> part;            // per-wave partial records
    DevBuf<double> scratch;         // level-1 reduction scratch
    DevBuf<double> red;             // reduced outputs (contiguous: psum | obj | gram blocks)
    DevBuf<double, true> hred;      // pinned host mirror of red
    DevBuf<double, true> hstage;    // pinned staging for the small per-sweep uploads (2 Kp doubles), no sync needed
    DevBuf<double> lognum_part;
    DevBuf<double> f_hist;          // SCI f history [batch][Kp]
    DevBuf<double> vec_tmp;         // staging for one N_local-vector (mbar_ctx_row_sub)
    DevBuf<int64_t> boot_idx;       // bootstrap draws: cum[K + 1] | order[total] (mbar_ctx_draw_bootstrap_weights keeps the last layout)
    size_t boot_idx_words = 0;      // words of the layout it holds
    uint64_t boot_layout_digest[2] = {0, 0};
    int64_t boot_states = 0, boot_total = 0;  // the layout on the device: number of runs, positions in total
    bool boot_has_order = false;
    bool vec_holds_logshift = false;  // vec_tmp holds log(A - shift) of mbar_ctx_vec_logshift (and not some other call's vector)
    // captured SCI batch (launch-bound loop: 3 small kernels per iteration replayed from a hipGraph)
    hipGraphExec_t sci_graph = nullptr;
    int64_t sci_graph_batch = 0, sci_graph_sig = 0;
    double sci_graph_tol = 0.0;
    // device-resident adaptive loop: solver state (f, psum, candidates, ratio, parameters, history), control words and
    // the sampled-state list live on the device; a batch of whole iterations can be replayed from a hipGraph
    DevBuf<double> ad;
    int64_t ad_hist_cap = 0;
    DevBuf<int> ad_ints;            // ctl[CTL_WORDS] | sampled[Kp]
    DevBuf<int, true> h_ctl;        // pinned mirror of the control words
    hipGraphExec_t ad_graph = nullptr;
    int64_t ad_graph_batch = 0, ad_graph_sig = 0;
    // P mode of that loop: resident probability matrix exp(a0 - u - logden(a0)), Kp x ld doubles, built once per solve
    DevBuf<double> P;
    bool P_failed = false;          // the allocation did not fit: stay in the classic mode for the life of the context
    DevBuf<double> pm_vec;          // a0[Kp] | ccur[Kp] | cgram[Kp]
    DevBuf<double> pm_ld0;          // host-driven loop on P (257 .. 1024 states): log-denominators at the anchor, ld doubles
    DevBuf<double> part_g;          // Gram partial records of the fused-sweep loop (the psum records use `part`)
    DevBuf<double> cwsq;            // sqrt of the per-sample multiplicities (only when weighted; else cw itself serves)
    DevBuf<double> chol;            // workspace of the blocked Cholesky Newton solve (129 .. 256 states)
    // histogram bins by label: labels and target potential (N each), one chunk table per tile of bins, the partial records of one
    // sweep and the merged outputs (binmax | lognum or wsum | diag | cross[K][nbins] | f_bins)
    int64_t hist_nbins = 0;
    DevBuf<int32_t> hist_label;
    DevBuf<double> hist_v;
    std::vector<HistTile> hist_tiles;
    DevBuf<double> hist_rec, hist_out;
    // scans over a linear family (mbar_ctx_set_scan): basis[B][ld] | t[Q][ld], the members of one call (coeff | offset | f_scan),
    // the partial records of one panel and the merged outputs
    int64_t scan_B = 0, scan_Q = 0;
    DevBuf<double> scan_vec, scan_in, scan_part, scan_out;
    // the kind of the family's terms (mbar_ctx_set_scan_terms; mask 0: all linear) and, for a family with harmonic terms, the
    // centres of the next scan calls' members (mbar_ctx_set_scan_centers): [scan_center_L][SCAN_MAX_H], the harmonic terms' in
    // ascending b (scan_center_L = 0: none)
    mbar::FamilyTerms scan_terms{};
    int64_t scan_center_L = 0;
    DevBuf<double> scan_center;
    // many observables along a scan (mbar_ctx_set_scan_obs): a[scan_obs_Q][ld], a block of its own next to the family's
    int64_t scan_obs_Q = 0;
    DevBuf<double> scan_obs;
    // kernel-density surfaces along a scan (mbar_ctx_set_scan_points): x[scan_pts_d][ld], the coordinates of the samples
    int64_t scan_pts_d = 0;
    DevBuf<double> scan_pts;
    // histogram surfaces along a scan (mbar_ctx_set_scan_bins): the samples sorted by bin and the chunk tables of the two passes
    // (chunks of SCAN_VCHUNK / SCAN_CHUNK sorted positions, cut from the start of every bin); the host keeps pass B's chunk
    // offsets to group the bins under the record budget
    int64_t scanbin_nbins = 0, scanbin_chunks_a = 0, scanbin_chunks_b = 0;
    DevBuf<int32_t> scanbin_perm, scanbin_cbin_a, scanbin_cbin_b;
    DevBuf<int64_t> scanbin_start, scanbin_c0_a, scanbin_c0_b;
    std::vector<int64_t> scanbin_c0_b_host;
    DevBuf<double> scanbin_fbins;
    long long* stamps = nullptr;    // MBAR_DEBUG_STAMPS: phase stamps of k_select_newton (64 launches x 16); hipMalloc, debug only
    // P outlives the solve that built it: a later solve on the same matrix whose start lies within the window of the anchor
    // (bootstrap replicates, protocol stages, continuation) starts with ONE fused sweep instead of the build sweep
    std::vector<double> last_psum;  // per-state sums at the f the last adaptive solve returned (empty: none)
    bool P_valid = false;
    std::vector<double> P_a0;       // anchor of the resident probability matrix: aden at the build point (Kp entries)
    // options
    int64_t opt_grid = 0, opt_force_generic = 0, opt_check_finite = 1, opt_sci_batch = 16, opt_timing = 0, opt_graph = 1, opt_small = 1, opt_wide = 1;
    int64_t opt_device_loop = 1, opt_adapt_batch = 8, opt_pmode = 1, opt_fused = 1, opt_quad = 1, opt_device_loop_wide = 1, opt_pcache = 1, opt_merge_select = 1, opt_sci_merged = 1, opt_wide_pmode = 1, opt_quad_trim = 1, opt_light_last = 1, opt_direct_results = 1, opt_debug_download_p = 0, opt_fused_general = 0;
    int64_t opt_small_balanced = 1, opt_sci_pingpong = 1, opt_host_pmode = 2, opt_rect_waves = 8, opt_newton_ldlt = 1;
    int64_t opt_hist_part_bytes = (int64_t)1 << 28;  // byte budget of the partial records of one sweep of the binned passes
    int64_t opt_scan_part_bytes = (int64_t)1 << 28;  // byte budget of the partial records of one member panel of pass A of the scans, and of one sweep of the binned scan passes

    // comm
    ncclComm_t comm = nullptr;
    mbar_loopback* loop = nullptr;  // in-process transport (tests): like comm, a collective on the compute stream
    mbar_allreduce_fn host_reduce = nullptr;
    void* host_reduce_user = nullptr;
    int rank = 0, nranks = 1;
    // timing
    std::vector<TimerPair> pending;
    std::vector<hipEvent_t> pool;
    double t_ms[MBAR_TIMER_COUNT] = {0, 0, 0, 0, 0};
    int64_t t_n[MBAR_TIMER_COUNT] = {0, 0, 0, 0, 0};
    std::string error;
};


namespace mbar {
namespace host {

hipEvent_t get_event(mbar_ctx* c);
// Event pair around the work enqueued in its scope (when the "timing" option is set, or when `enable` says so)
struct ScopedTimer {
    mbar_ctx* c;
    TimerPair tp;
    bool on;
    ScopedTimer(mbar_ctx* c_, int which) : ScopedTimer(c_, which, c_->opt_timing != 0) {}
    ScopedTimer(mbar_ctx* c_, int which, bool enable) : c(c_), on(false) {
        tp.a = tp.b = nullptr;
        if (!enable) return;
        tp.a = get_event(c);
        tp.b = get_event(c);
        tp.which = which;
        if (tp.a && tp.b) {
            on = hipEventRecord(tp.a, c->stream) == hipSuccess;
        }
    }
    ~ScopedTimer() {
        if (on) {
            (void)hipEventRecord(tp.b, c->stream);
            c->pending.push_back(tp);
        }
    }
};
// Event pair for ONE sweep of the device-resident loop, made before its launch.  "timing" 2: the events ride on the kernel dispatch
// itself, bound to it through `lc` (the LoopCtl the launch is about to get); otherwise event records around the launch(es) in scope.
struct LaunchTimer {
    mbar_ctx* c;
    TimerPair tp;
    bool armed, ext;
    LaunchTimer(mbar_ctx* c_, int which, bool timed, LoopCtl& lc) : c(c_), tp{nullptr, nullptr, which} {
        if (timed) {
            tp.a = get_event(c);
            tp.b = get_event(c);
        }
        armed = tp.a && tp.b;
        ext = armed && c->opt_timing == 2;
        if (ext) {
            lc.ev_start = tp.a;
            lc.ev_stop = tp.b;
        } else if (armed) {
            (void)hipEventRecord(tp.a, c->stream);
        }
    }
    ~LaunchTimer() {
        if (armed && !ext) (void)hipEventRecord(tp.b, c->stream);
        if (armed) c->pending.push_back(tp);
    }
};

// layout of c->small (doubles)
inline double* d_aden(mbar_ctx* c) { return c->small; }                      // [2][Kp]
inline double* d_anum(mbar_ctx* c) { return c->small + 2 * c->Kp; }          // [Kp]
inline double* d_f(mbar_ctx* c) { return c->small + 3 * c->Kp; }             // [Kp]
inline double* d_Nk(mbar_ctx* c) { return c->small + 4 * c->Kp; }            // [Kp]
inline double* d_lnNk(mbar_ctx* c) { return c->small + 5 * c->Kp; }          // [Kp]
inline double* d_delta(mbar_ctx* c) { return c->small + 6 * c->Kp; }         // [256]
inline double* d_misc(mbar_ctx* c) { return c->small + 6 * c->Kp + 256; }    // [4*Kp]
inline size_t small_doubles(int64_t Kp) { return (size_t)(10 * Kp + 256); }


// a transport whose collective is enqueued on the compute stream (no host in the loop)
inline bool stream_transport(const mbar_ctx* c) { return c->comm != nullptr || c->loop != nullptr; }

struct GramPlan {
    struct Item { bool diag; int64_t ri, rj; int nbi, nbj; int nblk; size_t off; };
    std::vector<Item> items;
    size_t total_blocks = 0;
};

// ---- mbar_capi.cpp: context lifecycle and buffers ----
void flush_timers(mbar_ctx* c);
int sync_stream(mbar_ctx* c);
int drop_graphs(mbar_ctx* c);
// The sizing rule of the context's work buffers: an entry point sizes part, scratch, red / hred for everything it is about to
// enqueue BEFORE its first launch -- ensure / ensure_red / reserve are never reached with work of the same call in flight (a
// block they replace goes back to the shared pool at once).  Should a call get there all the same, they drain the stream first.
int ensure(mbar_ctx* c, DevBuf<double>& buf, size_t want);  // grow, after drop_graphs: captured graphs hold these pointers
int ensure_red(mbar_ctx* c, size_t want);                   // red and its pinned mirror grow together
// What the launches of one call need of part and of the level-1 reduction scratch: the largest of their per-wave record sets
struct RecordNeed {
    size_t part = 0, scratch = 0;
    void add(int nwaves, size_t rec) {  // one launch that leaves `nwaves` records of `rec` doubles
        part = std::max(part, (size_t)nwaves * rec);
        scratch = std::max(scratch, ((size_t)nwaves / 32 + 1) * rec);
    }
};
int reserve(mbar_ctx* c, const RecordNeed& need);
int need_zeroed_vec(mbar_ctx* c, DevBuf<double>& v);  // one ld-vector, allocated and zeroed at its first use
int refresh_poison(mbar_ctx* c);
// What the binned passes (mbar_hist.cpp) and the scan passes (mbar_scan.cpp) ask of a context before anything else.
// family: "the binned passes" / "the scan passes", as the messages word it; max_K: the most states the family serves, 0: no limit.
int passes_ready(mbar_ctx* c, const char* who, const char* family, int64_t max_K);
// the refusal of the entry points an extension context does not serve
inline int ext_holds_rows_only(mbar_ctx* c, const char* who) {
    return fail(c, MBAR_ERR_STATE, std::string(who) + ": an extension context holds rows only (mbar_lognum_ext / mbar_gram_w_ext sweep them)");
}

// ---- mbar_eval.cpp: the evaluation engine ----
bool f_is_finite(const mbar_ctx* c, const double* f, int nf);
bool wide_pitch(const mbar_ctx* c);
int lse_variant_for(const mbar_ctx* c);
bool use_fast(const mbar_ctx* c);
void build_aden(const mbar_ctx* c, const double* f, double* out, int64_t rows);
bool split_sweep_ok(const mbar_ctx* c, int64_t rows);
int run_lse(mbar_ctx* c, int nf, int64_t rows, double* ld0, double* ld1, bool use_offset);
GramPlan gram_plan(int64_t Kp, bool quad = false);
GramPlan gram_plan_pmode(int64_t Kp);
bool use_quad(const mbar_ctx* c);
GramPlan plan_for(const mbar_ctx* c);
int quad_live_blocks(const mbar_ctx* c);
// part and scratch for every launch of run_gram on this plan (pmode: on a resident probability matrix); geom (if any) receives the
// launch geometry of every item.  run_gram calls it itself; a caller that enqueues anything before run_gram calls it first.
int reserve_gram(mbar_ctx* c, const GramPlan& plan, bool pmode, std::vector<LaunchGeom>* geom = nullptr);
int run_gram(mbar_ctx* c, const double* anum_dev, const double* logden, size_t red_off, const GramPlan& plan, const double* pmat = nullptr);
// One Gram launch and the reduction of its per-wave records: `nwaves` records of `rec` doubles, which launch() (a callable that
// returns an MBAR code) leaves in c->part, summed into `dst`.  part and scratch hold them already (reserve).
template <class Launch>
int launch_and_reduce(mbar_ctx* c, int nwaves, size_t rec, double* dst, Launch&& launch) {
    {
        ScopedTimer t(c, MBAR_TIMER_GRAM);
        int rc = launch();
        if (rc) return rc;
    }
    ScopedTimer t(c, MBAR_TIMER_REDUCE);
    HIPCHK(c, launch_reduce(c->stream, c->part, nwaves, (int64_t)rec, c->scratch, dst));
    return MBAR_OK;
}
// logden with the multiplicities of `w` folded in, logden - alpha ln c_n, written to w->lden_eff on `stream` (unweighted: logden
// stays): alpha 1/2 where each of two operands carries sqrt(c_n) (Gram sweeps), 1 for sum_n c_n exp(...)
hipError_t fold_weights(mbar_ctx* w, hipStream_t stream, double alpha, const double*& logden);
// f[K] padded with -inf (an operand that is zero) to `rows` entries
std::vector<double> padded_operand(const double* f, int64_t K, int64_t rows);
// the first `total` doubles of red, all-reduced, in hred; the stream is idle afterwards
int fetch_red(mbar_ctx* c, size_t total);
void gram_operand_sums(const double* G, int64_t K, const double* w, double* out);
void unpack_gram(const GramPlan& plan, const double* blocks, int64_t K, double* G);
// psum[k] = sum_j G[k][j] from the reduced upper-triangular blocks of ONE diagonal panel of nb x 16 states (host copy; block (I, J >= I)
// at ((I nb - I (I - 1) / 2) + (J - I)) * 256, element (r, q) at r * 16 + q): with the rows of p summing to one that is sum_n c_n p_kn.
void gram_row_sums(const double* blocks, int nb, int64_t K, double* psum);
int64_t lse_rows(const mbar_ctx* c);
// A NaN or -inf entry of the matrix, or a non-finite f_k of a state with samples, makes every sum NaN (the reference's logsumexp
// over all samples propagates it into every f_k): no sweep runs, eval_core and the entry points built on it fill their outputs
// with NaN and return MBAR_OK
inline bool unusable(const mbar_ctx* c, const double* f, int nf = 1) { return c->u_poison || !f_is_finite(c, f, nf); }
inline void fill_nan(double* out, size_t n) {
    if (out) std::fill(out, out + n, std::numeric_limits<double>::quiet_NaN());
}
int eval_core(mbar_ctx* c, const double* f, int nf, unsigned flags, double* ld0, double* ld1, double* psum,
              double* sumlogden, double* gram);
// the log-denominators of f into slot 0; *nan_out: the matrix or f is unusable and every output is NaN
int pass_logden(mbar_ctx* c, const double* f, bool* nan_out);
// One log-normaliser sweep: log sum_n c_n exp(-row_kn - logden_n) of the K rows of `c` (a context, or an extension) against the
// log-denominators in slot 0 of `den` (c itself, or the extension's base) and den's multiplicities, as per-row maximum hm and
// sum hs of this rank: the normaliser is hm + log(hs)
int lognum_sweep(mbar_ctx* c, mbar_ctx* den, std::vector<double>& hm, std::vector<double>& hs);

// ---- mbar_rows.cpp: the writers of the matrix ----
// What every writer of the matrix leaves behind: the poison flags (and with them the log-denominators kept in slot 0, see
// refresh_poison), the resident probability matrix and the last solve's sums all describe the matrix as it was
inline void matrix_touched(mbar_ctx* c) {
    c->u_checked = false;
    c->P_valid = false;
    c->last_psum.clear();
}
// rows [row0, row0 + nrows) are rows of the context
inline bool rows_in_range(const mbar_ctx* c, int64_t row0, int64_t nrows) { return row0 >= 0 && nrows >= 0 && row0 + nrows <= c->K; }
// kind[B] (non-zero: harmonic) and period[B] (NULL: no term is periodic; read at the harmonic terms only) of a family as the
// kernels take them; MBAR_ERR_ARG naming `who` for more than MBAR_SCAN_MAX_H harmonic terms or a negative or non-finite period
int family_terms(mbar_ctx* c, const char* who, int64_t B, const int32_t* kind, const double* period, FamilyTerms* out);

// ---- mbar_comm.cpp: transports ----
bool loop_barrier(mbar_loopback* g);
void loop_break(mbar_loopback* g);
int allreduce_loop(mbar_ctx* c, double* dev, int64_t count, int op);
int allreduce_dev(mbar_ctx* c, double* dev, int64_t count, int op);
int allreduce_host(mbar_ctx* c, double* host, int64_t count, int op);
int agree_with_rank0(mbar_ctx* c, double* v, int64_t count);

// ---- mbar_host.cpp: host-side K x K algebra ----
double now_ms();
bool chol_solve(std::vector<double>& A, std::vector<double>& b, int m);
int host_team_size(int m);
bool chol_solve_blocked(const double* A, size_t lda, std::vector<double>& b, int m, int threads);
void host_team_run(int threads, const std::function<void(int)>& fn);  // fn(0) on the caller, fn(1 .. threads-1) on the parked team
void jacobi_eigh(std::vector<double> A, int m, std::vector<double>& w, std::vector<double>& V);
void newton_direction(const std::vector<double>& H, const std::vector<double>& g, int m, std::vector<double>& x);
// the host-driven loop's Newton matrix straight from the reduced Gram blocks, dealt over the host team
void unpack_gram_to_hessian(const GramPlan& plan, const double* blocks, int64_t K, const double* factor, const int* pos, int m, double* H,
                            int threads);

// ---- mbar_loops.cpp: what the solver loops share ----
// What both solve entry points do before their first real step: the refusals, the device made current, *t0 (now_ms()), slot 0's
// log-denominators declared stale -- `guard` repeats that on EVERY way out, error returns included: the loops use the slot vectors
// for their own purposes, and an evaluation inside them marks slot 0 valid again before the loop overwrites it -- and the poison
// flags brought up to date.  What a poisoned matrix or a non-finite start means is the caller's business.
struct Ld0Guard {
    mbar_ctx* c = nullptr;
    ~Ld0Guard() { if (c) c->ld0_valid = false; }
};
int enter_solve(mbar_ctx* c, const double* f_inout, const char* who, Ld0Guard& guard, double* t0);
// A decision that changes the SEQUENCE of collectives must be the same on every rank: `ok` is MIN-reduced over the ranks
int agree_all_ok(mbar_ctx* c, bool& ok);
// Captures `batch` calls of enqueue(b), b = 0 .. batch - 1, on the context's stream and instantiates them as *exec (which must be
// null).  Nothing may allocate inside enqueue; the eager warm-up that sets the kernel attributes stays with the caller.
int capture_batch(mbar_ctx* c, hipGraphExec_t* exec, int64_t batch, const std::function<int(int64_t)>& enqueue);
// MBAR_DEBUG_STAMPS: *out = the context's stamp buffer (STAMP_WORDS words: 64 launches x 16 and one spare row), allocated at its
// first use and zeroed on the stream -- all of it; nullptr when the variable is not set
constexpr size_t STAMP_WORDS = 65 * 16;
int debug_stamps(mbar_ctx* c, long long** out);

// ---- mbar_loop_host.cpp: the host-driven adaptive loop ----
int adaptive_host_loop(mbar_ctx* c, std::vector<double>& f, double tol, int64_t maxiter, int64_t min_sc_iter, double gamma,
                       int check_convergence, double* history, int64_t history_rows, mbar_solve_result& res,
                       std::vector<double>& psum, double& max_delta);

// ---- mbar_loop_device.cpp: the device-resident adaptive loop ----
bool device_loop_eligible(const mbar_ctx* c);
int adaptive_device_loop(mbar_ctx* c, std::vector<double>& f, double tol, int64_t maxiter, int64_t min_sc_iter, double gamma,
                         int check_convergence, double* history, int64_t history_rows, mbar_solve_result& res,
                         std::vector<double>& psum, double& max_delta, bool& handed_back);

}  // namespace host
}  // namespace mbar
