// Internal header of the host side of libmbar_hip.so (not part of the public ABI): the context, the caching allocator, and the
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
//   mbar_host.cpp   allocator state, host-side K x K linear algebra, content digest
// The handles of the other backends (mbar_kde.cpp, mbar_acf.cpp, mbar_bar.cpp, mbar_bspline.cpp, mbar_batch.cpp) share the layer
// below the context: Handle, DevBuf, create_handle / destroy_handle, ColumnPasses, run_passes.
#pragma once
#include "../../include/mbar_hip.h"
#include "mbar_internal.h"

#include <dlfcn.h>
#include <sched.h>
#include <unistd.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <atomic>
#include <thread>
#include <unordered_map>
#include <vector>


namespace mbar {
namespace host {

extern thread_local std::string g_last_error;

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

// ---- caching allocator ----------------------------------------------------------------------------------------------
// hipMalloc / hipFree / hipHostMalloc cost 0.1 - 1 ms each (hipFree also synchronises the device): a context makes ~15
// allocations, and pymbar's real workloads (K ~ 40, N ~ 1e5: sweeps of ~10 us) build and drop contexts all the time -- the
// MBAR object, one augmented matrix per expectation call, one temporary per module-level function call.  Freed blocks are
// therefore kept (per device, bounded: MBAR_CACHE_MB, default an eighth of the device's memory -- 36 GB of 288: room for config 3's
// matrix + probability matrix or one augmented expectation matrix, while other users of the GPU keep 7/8 -- and 64 MB of
// pinned host memory; blocks of more than half the bound go straight back to the driver) and handed out again to requests of
// about the same size.  (The bound used to be 2 GB: the augmented matrix of an expectation call at K=128, N=4e6 is 6-8 GB, and
// its hipMalloc / hipFree pair cost 0.3-0.7 s per call against 15-45 ms of work.)  An allocation that fails empties the cache
// and is tried again, and mbar_cache_trim() hands everything back.  Every API call of this library leaves its stream idle
// before it frees anything, so a cached block has no work in flight.
struct MemCache {
    struct Pool {
        std::multimap<size_t, void*> free_blocks;
        size_t cached = 0, limit = 0;
    };
    std::mutex mu;
    std::map<int, Pool> dev;                       // device ordinal -> pool
    Pool pinned;
    std::unordered_map<void*, std::pair<size_t, int>> live;  // every block handed out: size, device (-1 = pinned host)
    bool configured = false;
    void configure() {
        if (configured) return;
        configured = true;
        if (const char* e = std::getenv("MBAR_CACHE_MB")) {
            dev_limit = (size_t)std::strtoull(e, nullptr, 10) << 20;
            limit_from_env = true;
        }
        pinned.limit = limit_from_env ? std::min<size_t>(dev_limit, (size_t)64 << 20) : (size_t)64 << 20;
    }
    size_t dev_limit = (size_t)2048 << 20;
    bool limit_from_env = false;
    size_t device_limit() const {  // (called with the device current)
        if (limit_from_env) return dev_limit;
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
            (void)hipGetLastError();
            return dev_limit;
        }
        return std::max(dev_limit, total_b / 8);
    }
    static size_t round_up(size_t b) { return (b + 4095) / 4096 * 4096; }
    static void* take(Pool& p, size_t want) {
        auto it = p.free_blocks.lower_bound(want);
        if (it == p.free_blocks.end() || it->first > want + want / 4 + 65536) return nullptr;  // (no big block for a small request)
        void* q = it->second;
        p.cached -= it->first;
        p.free_blocks.erase(it);
        return q;
    }
    hipError_t alloc(void** out, size_t bytes, bool host) {
        std::lock_guard<std::mutex> lock(mu);
        configure();
        const size_t want = round_up(bytes ? bytes : 1);
        int d = -1;
        if (!host) {
            hipError_t e = hipGetDevice(&d);
            if (e != hipSuccess) return e;
        }
        Pool& p = host ? pinned : dev[d];
        if (!host && p.limit == 0) p.limit = device_limit();
        size_t got = want;
        void* q = take(p, want);
        if (q) {
            got = live[q].first;
        } else {
            hipError_t e = host ? hipHostMalloc(&q, want, hipHostMallocDefault) : hipMalloc(&q, want);
            if (e != hipSuccess && !p.free_blocks.empty()) {  // out of memory with blocks parked here: give them back, retry
                (void)hipGetLastError();
                for (auto& kv : p.free_blocks) {
                    live.erase(kv.second);
                    if (host) (void)hipHostFree(kv.second); else (void)hipFree(kv.second);
                }
                p.free_blocks.clear();
                p.cached = 0;
                e = host ? hipHostMalloc(&q, want, hipHostMallocDefault) : hipMalloc(&q, want);
            }
            if (e != hipSuccess) return e;
            live[q] = {want, d};
        }
        (void)got;
        *out = q;
        return hipSuccess;
    }
    hipError_t release(void* q) {
        if (!q) return hipSuccess;
        std::lock_guard<std::mutex> lock(mu);
        auto it = live.find(q);
        if (it == live.end()) return hipErrorInvalidValue;
        const size_t sz = it->second.first;
        const int d = it->second.second;
        Pool& p = d < 0 ? pinned : dev[d];
        if (p.cached + sz <= p.limit && sz <= p.limit / 2) {
            p.free_blocks.emplace(sz, q);
            p.cached += sz;
            return hipSuccess;
        }
        live.erase(it);
        return d < 0 ? hipHostFree(q) : hipFree(q);
    }
    // Parked device blocks beyond `keep_bytes` per device go back to the driver, largest first (called when the process's last
    // context is destroyed: a drop-in that is done with its matrices must not sit on an eighth of a shared GPU)
    void trim_to(size_t keep_bytes) {
        std::lock_guard<std::mutex> lock(mu);
        for (auto& dp : dev) {
            Pool& p = dp.second;
            while (p.cached > keep_bytes && !p.free_blocks.empty()) {
                auto it = std::prev(p.free_blocks.end());
                live.erase(it->second);
                (void)hipSetDevice(dp.first);
                (void)hipFree(it->second);
                p.cached -= it->first;
                p.free_blocks.erase(it);
            }
        }
    }
    size_t idle_limit() {
        if (const char* e = std::getenv("MBAR_CACHE_IDLE_MB")) return (size_t)std::strtoull(e, nullptr, 10) << 20;
        return (size_t)1024 << 20;
    }
    void trim() {
        std::lock_guard<std::mutex> lock(mu);
        for (auto& dp : dev) {
            for (auto& kv : dp.second.free_blocks) {
                live.erase(kv.second);
                (void)hipSetDevice(dp.first);
                (void)hipFree(kv.second);
            }
            dp.second.free_blocks.clear();
            dp.second.cached = 0;
        }
        for (auto& kv : pinned.free_blocks) {
            live.erase(kv.second);
            (void)hipHostFree(kv.second);
        }
        pinned.free_blocks.clear();
        pinned.cached = 0;
    }
};
extern MemCache g_mem;
extern std::atomic<int> g_live_contexts;
struct DevInfo {
    int num_cu = 256;
    std::string arch;
};
extern std::mutex g_dev_mu;
extern std::map<int, DevInfo> g_dev_info;
extern std::map<int, std::vector<hipStream_t>> g_stream_pool;
inline hipError_t cache_malloc(void** p, size_t bytes) { return g_mem.alloc(p, bytes, false); }
inline hipError_t cache_free(void* p) { return g_mem.release(p); }
inline hipError_t cache_host_malloc(void** p, size_t bytes) { return g_mem.alloc(p, bytes, true); }
inline hipError_t cache_host_free(void* p) { return g_mem.release(p); }

// One block of the cache, owned: freed when the owner goes
// (Pinned: page-locked host memory of the same cache, mapped into the device's address space)
template <typename T, bool Pinned = false>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;  // capacity in elements
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), n(o.n) {
        o.p = nullptr;
        o.n = 0;
    }
    DevBuf& operator=(DevBuf&& o) noexcept {
        std::swap(p, o.p);
        std::swap(n, o.n);
        return *this;
    }
    ~DevBuf() { reset(); }
    operator T*() const { return p; }
    void reset() {
        if (p) (void)cache_free(p);
        p = nullptr;
        n = 0;
    }
    // at least `want` elements (contents are not kept)
    auto grow(size_t want) -> hipError_t {
        if (n >= want) return hipSuccess;
        if (p) {
            hipError_t e = cache_free(p);
            if (e != hipSuccess) return e;
        }
        p = nullptr;
        n = 0;
        hipError_t e = g_mem.alloc((void**)&p, want * sizeof(T), Pinned);
        if (e == hipSuccess) n = want;
        return e;
    }
    // grow(count), then the synchronous copy of `count` elements from the host to the buffer's start
    auto upload(const T* src, size_t count) -> hipError_t {
        hipError_t e = grow(count);
        return e != hipSuccess ? e : hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice);
    }
};
// a host table on the device (an empty one still gets a block: the kernels are handed its pointer)
template <class T>
hipError_t put(DevBuf<T>& d, const std::vector<T>& h) {
    return h.empty() ? d.grow(1) : d.upload(h.data(), h.size());
}

struct TimerPair {
    hipEvent_t a, b;
    int which;
};


}  // namespace host
}  // namespace mbar
using mbar::host::TimerPair;
using mbar::host::DevBuf;

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

int fail(mbar_ctx* c, int code, const std::string& msg);
#define HIPCHK(ctx, expr)                                                                        \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess)                                                                    \
            return fail(ctx, MBAR_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));   \
    } while (0)
inline int bad_arg(const std::string& msg) { return fail(nullptr, MBAR_ERR_ARG, msg); }

// ---- the handles of the other backends (mbar_kde, mbar_acf, mbar_bar, mbar_bspline, mbar_batch) -----------------------------
// A handle derives from Handle, holds its device memory in DevBuf members, is made by create_handle and released by
// destroy_handle: no buffer list to keep in step with the struct.

// Makes `device` current after checking that it exists and is a gfx950; its properties are looked up once per process
int open_device(int device, DevInfo* out);

// Device and stream of a handle, and its place among the live contexts (the last one to go trims the cache)
struct Handle {
    int device = 0;
    hipStream_t stream = nullptr;
    Handle() { g_live_contexts.fetch_add(1); }
    Handle(const Handle&) = delete;
    Handle& operator=(const Handle&) = delete;
    ~Handle() {
        if (stream) (void)hipStreamDestroy(stream);
        if (g_live_contexts.fetch_sub(1) == 1) g_mem.trim_to(g_mem.idle_limit());
    }
};

// The stream is drained before the members give their blocks back: the pool is shared, and no block may return to it while a
// kernel still uses it
template <class H>
void destroy_handle(H* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    delete h;
}

// Opens the device, makes the handle with its own stream and runs init(h, device info); on a failure the handle is destroyed
// and the first error stays the last one
template <class H, class Init>
int create_handle(H** out, int device, Init&& init) {
    DevInfo di;
    int rc = open_device(device, &di);
    if (rc) return rc;
    H* h = new H();
    h->device = device;
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    rc = e == hipSuccess ? init(h, di)
                         : fail(nullptr, MBAR_ERR_HIP, std::string("hipStreamCreateWithFlags: ") + hipGetErrorString(e));
    if (rc != MBAR_OK) {
        const std::string msg = g_last_error;
        destroy_handle(h);
        return fail(nullptr, rc, msg);
    }
    *out = h;
    return MBAR_OK;
}

// The pass driver of the batched state machines (mbar_batch, mbar_bar), with the handle's device current: the P host states go
// to `dev`, then pass() runs in groups of 4, 8, 16, 16, ...: between groups the host reads one int per problem (`active`).  A
// finished problem costs one early-exiting workgroup per chunk.  More than `limit` passes with a problem still active:
// MBAR_ERR_NUMERIC with `over_limit`.  At the end the states come back and *passes (if any) is the number of passes.
template <class State, class Pass>
int run_passes(hipStream_t stream, State* host, State* dev, const int* active, int64_t P, int64_t limit, const char* over_limit,
               int64_t* passes, Pass&& pass) {
    HIPCHK(nullptr, hipMemcpyAsync(dev, host, (size_t)P * sizeof(State), hipMemcpyHostToDevice, stream));
    std::vector<int> act((size_t)P);
    int64_t done = 0;
    int group = 4;
    for (;;) {
        for (int k = 0; k < group; ++k) {
            int rc = pass();
            if (rc) return rc;
        }
        done += group;
        HIPCHK(nullptr, hipMemcpyAsync(act.data(), active, act.size() * sizeof(int), hipMemcpyDeviceToHost, stream));
        HIPCHK(nullptr, hipStreamSynchronize(stream));
        bool any = false;
        for (int a : act) any = any || a != 0;
        if (!any) break;
        if (done > limit) return fail(nullptr, MBAR_ERR_NUMERIC, over_limit);
        group = std::min(16, group * 2);
    }
    HIPCHK(nullptr, hipMemcpyAsync(host, dev, (size_t)P * sizeof(State), hipMemcpyDeviceToHost, stream));
    HIPCHK(nullptr, hipStreamSynchronize(stream));
    if (passes) *passes = done;
    return MBAR_OK;
}

// Weight columns: the host copy of every column and the device buffer of one pass of cb columns ([pitch][cb], zero on the
// padding columns and rows).  `widths` are the pass widths the kernels are instantiated for, ascending.
struct ColumnPasses {
    std::vector<int> widths;
    std::vector<double> host;  // [rows][C]
    int64_t rows = 0, C = 0;
    DevBuf<double> dev;
    int64_t pass = -1;  // first column of the pass the device buffer holds (-1: none)
    int cb = 0;
    explicit ColumnPasses(std::vector<int> w) : widths(std::move(w)) {}
    // the smallest width that holds `cols` columns
    int width(int64_t cols) const {
        for (int w : widths)
            if (w >= cols) return w;
        return widths.back();
    }
    // new columns ([rows][C]): a copy of v, or (v NULL) a host copy for the caller to fill; nothing is on the device
    double* reset(int64_t rows_, int64_t C_, const double* v = nullptr) {
        rows = rows_;
        C = C_;
        if (v) host.assign(v, v + rows * C);
        else host.resize((size_t)rows * C);
        pass = -1;
        return host.data();
    }
    bool holds(int64_t c0, int width_) const { return pass == c0 && cb == width_; }
    // columns [c0, c0 + cv) as a pass of width w, rows padded to `pitch` (no copy when the buffer holds them)
    int upload(int64_t c0, int cv, int w, int64_t pitch);
};


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
