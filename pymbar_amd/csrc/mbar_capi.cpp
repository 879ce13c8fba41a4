// Host side of libmbar_hip.so, the context itself (mbar_ctx.h lists the files of the context layer and what each holds): the two
// constructors and the destructor, the buffers a context grows (ensure, ensure_red, reserve), options, N_k, sample weights and
// bootstrap draws, timing.  The entry points are those of the C ABI declared in include/mbar_hip.h.  No PyTorch, no BLAS/LAPACK.
#include "mbar_ctx.h"

using namespace mbar;
using namespace mbar::host;

namespace mbar {
namespace host {

int fail(mbar_ctx* c, int code, const std::string& msg) {
    if (c) c->error = msg;
    g_last_error = msg;
    return code;
}
// ---- timing --------------------------------------------------------------------------------
hipEvent_t get_event(mbar_ctx* c) {
    if (!c->pool.empty()) {
        hipEvent_t e = c->pool.back();
        c->pool.pop_back();
        return e;
    }
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}
void flush_timers(mbar_ctx* c) {
    for (auto& tp : c->pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, tp.a, tp.b) == hipSuccess) {
            c->t_ms[tp.which] += ms;
            c->t_n[tp.which] += 1;
        }
        c->pool.push_back(tp.a);
        c->pool.push_back(tp.b);
    }
    c->pending.clear();
}
int sync_stream(mbar_ctx* c) {
    HIPCHK(c, hipStreamSynchronize(c->stream));
    flush_timers(c);
    return MBAR_OK;
}

// ---- device buffer helpers -------------------------------------------------------------------
int drop_graphs(mbar_ctx* c) {  // captured batches hold buffer pointers, sizes and the sampled-state set
    if (c->sci_graph || c->ad_graph) HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->sci_graph) {
        HIPCHK(c, hipGraphExecDestroy(c->sci_graph));
        c->sci_graph = nullptr;
    }
    if (c->ad_graph) {
        HIPCHK(c, hipGraphExecDestroy(c->ad_graph));
        c->ad_graph = nullptr;
    }
    return MBAR_OK;
}
// The rule of these three is stated at their declarations (mbar_ctx.h): sized before the first launch of a call.  The backstop of
// that rule: a block about to be replaced while the stream still has work is replaced after the work has finished (the query's
// "not ready" must not stay behind as the thread's last error: the launchers read that after a launch).  Never reached inside
// capture_batch -- the loops size everything before they capture -- where a query would invalidate the capture.
int ensure(mbar_ctx* c, DevBuf<double>& buf, size_t want) {
    if (buf.n >= want) return MBAR_OK;
    int rc = drop_graphs(c);
    if (rc) return rc;
    if (buf.p && hipStreamQuery(c->stream) == hipErrorNotReady) {
        (void)hipGetLastError();
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    HIPCHK(c, buf.grow(want));
    return MBAR_OK;
}
int ensure_red(mbar_ctx* c, size_t want) {  // red and its pinned mirror grow together
    int rc = ensure(c, c->red, want);
    if (!rc) HIPCHK(c, c->hred.grow(want));
    return rc;
}
int reserve(mbar_ctx* c, const RecordNeed& need) {
    int rc = ensure(c, c->part, need.part);
    return rc ? rc : ensure(c, c->scratch, need.scratch);
}
// One vector of ld doubles, allocated and zeroed at its first use (what is written later stops at N: the padding stays zero)
int need_zeroed_vec(mbar_ctx* c, DevBuf<double>& v) {
    if (v) return MBAR_OK;
    HIPCHK(c, v.grow((size_t)c->ld));
    HIPCHK(c, hipMemsetAsync(v, 0, (size_t)c->ld * sizeof(double), c->stream));
    return MBAR_OK;
}
// ... and the two that only a weighted context has: lden_eff, cwsq
static int need_weight_vecs(mbar_ctx* c) {
    int rc = need_zeroed_vec(c, c->lden_eff);
    return rc ? rc : need_zeroed_vec(c, c->cwsq);
}

// Scan the matrix once after it changed; a NaN or -inf entry poisons every reduced output (reference
// behaviour: logsumexp over all samples propagates it into every f_k).
int refresh_poison(mbar_ctx* c) {
    if (c->u_checked) return MBAR_OK;
    c->ld0_valid = false;  // (every change of the matrix or of the transport clears u_checked)
    int* dflags = reinterpret_cast<int*>(d_delta(c) + 255);
    HIPCHK(c, hipMemsetAsync(dflags, 0, sizeof(int), c->stream));
    HIPCHK(c, launch_check_u(c->stream, c->u, c->ld, c->N, c->K, dflags));
    int h = 0;
    HIPCHK(c, hipMemcpyAsync(&h, dflags, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->nranks > 1) {
        // a NaN in ONE shard poisons the sums of every rank: agree on the flag, so that all ranks take the same early
        // return (a clean rank would otherwise wait in the all-reduce of a sweep the poisoned rank never launches)
        double v[2] = {(h & 3) ? 1.0 : 0.0, (h & 4) ? 1.0 : 0.0};
        int rc = allreduce_host(c, v, 2, 1);
        if (rc) return rc;
        h = (v[0] > 0.0 ? 1 : 0) | (v[1] > 0.0 ? 4 : 0);
    }
    c->u_poison = (h & 3) != 0;
    c->u_posinf = (h & 4) != 0;
    c->u_checked = true;
    return MBAR_OK;
}

int passes_ready(mbar_ctx* c, const char* who, const char* family, int64_t max_K) {
    if (!c) return fail(c, MBAR_ERR_ARG, "NULL argument");
    const std::string head = std::string(who) + ": ", fam = family;
    if (c->ext_base) return fail(c, MBAR_ERR_STATE, head + "an extension context holds rows only");
    if (c->nranks > 1 || stream_transport(c) || c->host_reduce)
        return fail(c, MBAR_ERR_STATE, head + fam + " serve single-rank contexts only (a transport is attached)");
    if (wide_pitch(c)) return fail(c, MBAR_ERR_STATE, head + fam + " do not serve wide-pitch matrices (row pitch x 56 bytes >= 4 GiB)");
    if (max_K > 0 && c->K > max_K) return fail(c, MBAR_ERR_STATE, head + fam + " serve at most " + std::to_string(max_K) + " states");
    return MBAR_OK;
}

}  // namespace host
}  // namespace mbar

// The two context constructors: a HIP error destroys the half-made context `c` and is the call's error
#define CRT(expr)                                                                                   \
    do {                                                                                            \
        hipError_t _e = (expr);                                                                     \
        if (_e != hipSuccess) {                                                                     \
            int rc_ = fail(nullptr, MBAR_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
            mbar_ctx_destroy(c);                                                                    \
            return rc_;                                                                             \
        }                                                                                           \
    } while (0)
// (stream creation costs milliseconds: streams of destroyed contexts are kept for the next one on the device; null: none is kept)
static hipStream_t take_pooled_stream(int device) {
    std::lock_guard<std::mutex> lock(g_dev_mu);
    auto& pool = g_stream_pool[device];
    if (pool.empty()) return nullptr;
    hipStream_t s = pool.back();
    pool.pop_back();
    return s;
}

// What the two constructors share, around matrix(), which allocates and initialises the matrix and the vectors of its length: the
// context's place among the live ones, its stream, the small vectors (for Kp_small padded states) and the staging behind them
template <class Matrix>
static int construct(mbar_ctx** out, mbar_ctx* c, int64_t Kp_small, Matrix&& matrix) {
    g_live_contexts.fetch_add(1);
    CRT(hipSetDevice(c->device));
    c->stream = take_pooled_stream(c->device);
    if (!c->stream) CRT(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    int rc = matrix();
    if (rc) return rc;
    CRT(c->small.grow(small_doubles(Kp_small)));
    CRT(c->hstage.grow((size_t)4 * Kp_small));
    CRT(hipMemsetAsync(c->small, 0, small_doubles(Kp_small) * sizeof(double), c->stream));
    CRT(hipStreamSynchronize(c->stream));
    c->Nk.assign(c->K, 0.0);
    c->lnNk.assign(c->K, 0.0);
    *out = c;
    return MBAR_OK;
}

// =================================================================================================
// C ABI
// =================================================================================================
extern "C" {

int mbar_version(void) { return 101; }

const char* mbar_last_error(const mbar_ctx* ctx) { return ctx ? ctx->error.c_str() : g_last_error.c_str(); }

int mbar_device_count(int* count) {
    if (!count) return fail(nullptr, MBAR_ERR_ARG, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return fail(nullptr, MBAR_ERR_NODEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    }
    *count = n;
    return MBAR_OK;
}

int mbar_device_info(int device, char* name, int name_len, int* compute_units, int64_t* total_mem_bytes) {
    hipDeviceProp_t p;
    hipError_t e = hipGetDeviceProperties(&p, device);
    if (e != hipSuccess) return fail(nullptr, MBAR_ERR_NODEVICE, std::string("hipGetDeviceProperties: ") + hipGetErrorString(e));
    if (name && name_len > 0) {
        std::snprintf(name, (size_t)name_len, "%s (%s)", p.name[0] ? p.name : "AMD Instinct MI355X", p.gcnArchName);
    }
    if (compute_units) *compute_units = p.multiProcessorCount;
    if (total_mem_bytes) *total_mem_bytes = (int64_t)p.totalGlobalMem;
    return MBAR_OK;
}

int mbar_ctx_create(mbar_ctx** out, int device, int64_t K, int64_t N_local) {
    if (!out) return fail(nullptr, MBAR_ERR_ARG, "out is NULL");
    *out = nullptr;
    // (N_local = 0 is a legal shard: with more ranks than 16-sample tiles a rank owns no column, yet it must take part in every
    // collective of the loop; it keeps one all-padding tile so that every kernel has something to launch on)
    if (K < 1 || N_local < 0) return fail(nullptr, MBAR_ERR_ARG, "K must be >= 1 and N_local >= 0");
    DevInfo di;
    int rc = open_device(device, &di);
    if (rc) return rc;
    mbar_ctx* c = new mbar_ctx();
    c->device = device;
    c->num_cu = di.num_cu;
    c->K = K;
    c->Kp = padded_K(K);
    c->N = N_local;
    // row pitch: whole 16-sample tiles; whole 64-sample tiles where the few-state evaluation kernel may run (K <= 32)
    c->ld = c->Kp <= 32 ? (N_local + 63) / 64 * 64 : (N_local + TS - 1) / TS * TS;
    if (c->ld == 0) c->ld = c->Kp <= 32 ? 64 : TS;
    return construct(out, c, c->Kp, [c]() -> int {
        const size_t ubytes = (size_t)c->Kp * c->ld * sizeof(double);
        CRT(c->u_alloc.grow((size_t)c->Kp * c->ld));
        c->u = c->u_alloc;
        CRT(launch_zero(c->stream, c->u, ubytes));
        // three logden vectors in ONE allocation: the device-resident loop addresses them as base + slot * ld
        CRT(c->logden_alloc.grow((size_t)3 * c->ld));
        CRT(launch_zero(c->stream, c->logden_alloc, (size_t)3 * c->ld * sizeof(double)));
        for (int i = 0; i < 3; ++i) c->logden[i] = c->logden_alloc + i * c->ld;
        CRT(c->cw.grow((size_t)c->ld));
        CRT(launch_zero(c->stream, c->cw, (size_t)c->ld * sizeof(double)));
        if (c->N > 0) CRT(launch_fill(c->stream, c->cw, 1.0, c->N));  // (unit multiplicities, 0 on the padding: filled on the device)
        return MBAR_OK;
    });
}

// ---- extension contexts: rows appended to a resident matrix WITHOUT a copy of it (the general path of the expectation family,
// pymbar/mbar.py:886-903 builds an N x (K + NL + S) host array there) -------------------------------------------------------------
// The extension holds only the new rows -- same device, N_local and row pitch as `base` -- and its storage starts a whole number
// of row pitches away from base's, so that a one-read sweep addresses [rows of base | rows of ext] as ONE 192- / 256-row panel
// (k_gram_quad_split).  K_rows real rows; the allocated rows make 16 ceil(base K / 16) + rows = 192 or 256.
int mbar_ctx_create_ext(mbar_ctx** out, mbar_ctx* base, int64_t K_rows) {
    if (!out) return fail(nullptr, MBAR_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (!base || K_rows < 1) return fail(base, MBAR_ERR_ARG, "mbar_ctx_create_ext: base context and K_rows >= 1");
    if (base->ext_base) return fail(base, MBAR_ERR_ARG, "mbar_ctx_create_ext: the base is an extension itself");
    const int64_t need = base->Kp + (K_rows + 15) / 16 * 16;
    if (base->Kp > 128 || need <= 128 || need > 256 || base->nranks > 1 || wide_pitch(base) || !use_fast(base) || !base->opt_quad)
        return fail(base, MBAR_ERR_ARG, "mbar_ctx_create_ext: needs a base of at most 128 states on one rank and 129 .. 256 rows in total");
    const int64_t Kp_ext = (need <= 192 ? 192 : 256) - base->Kp;
    mbar_ctx* c = new mbar_ctx();
    c->device = base->device;
    c->K = K_rows;
    c->Kp = Kp_ext;
    c->N = base->N;
    c->ld = base->ld;
    c->num_cu = base->num_cu;
    c->ext_base = base;
    return construct(out, c, 256, [c, base]() -> int {
        const size_t pitch = (size_t)c->ld * sizeof(double);
        CRT(c->u_alloc.grow((size_t)(c->Kp + 1) * c->ld));
        {   // first address of the allocation that is congruent to base->u modulo the row pitch
            const uintptr_t a = reinterpret_cast<uintptr_t>(c->u_alloc.p), b = reinterpret_cast<uintptr_t>(base->u);
            const uintptr_t r = a >= b ? (a - b) % pitch : (pitch - (b - a) % pitch) % pitch;
            c->u = reinterpret_cast<double*>(a + (r == 0 ? 0 : pitch - r));
        }
        // (only what no row operation writes is zeroed -- the padding rows and the padding columns behind N_local: the K_rows real rows
        // are whole-row uploads, copies or kernel outputs of the caller before the first sweep; zeroing 128 rows x 4e6 samples was
        // 0.8 ms of a 20 ms call)
        if (c->Kp > c->K) CRT(launch_zero(c->stream, c->u + (size_t)c->K * c->ld, (size_t)(c->Kp - c->K) * pitch));
        if (c->ld > c->N)
            CRT(hipMemset2DAsync(c->u + c->N, pitch, 0, (size_t)(c->ld - c->N) * sizeof(double), (size_t)c->K, c->stream));
        CRT(c->logden_alloc.grow((size_t)3 * 16));  // (never swept on its own: the log-denominators are the base's)
        c->logden[0] = c->logden[1] = c->logden[2] = c->logden_alloc;
        return MBAR_OK;
    });
}
#undef CRT

// What is not memory goes here; the buffers go back to the cache with their owning members in `delete c` -- after the stream has
// been drained (the pool is shared: no block may return to it while a kernel still uses it) and before the cache is trimmed
void mbar_ctx_destroy(mbar_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    flush_timers(c);
    for (auto e : c->pool) (void)hipEventDestroy(e);
    if (c->comm && g_rccl.CommDestroy) g_rccl.CommDestroy(c->comm);
    if (c->ad_graph) (void)hipGraphExecDestroy(c->ad_graph);
    if (c->sci_graph) (void)hipGraphExecDestroy(c->sci_graph);
    if (c->stamps) (void)hipFree(c->stamps);
    if (c->stream) {  // (idle: synchronised above) kept for the next context on this device
        std::lock_guard<std::mutex> lock(g_dev_mu);
        auto& pool = g_stream_pool[c->device];
        if (pool.size() < 8)
            pool.push_back(c->stream);
        else
            (void)hipStreamDestroy(c->stream);
    }
    delete c;
    if (g_live_contexts.fetch_sub(1) == 1) g_mem.trim_to(g_mem.idle_limit());
}

int mbar_ctx_synchronize(mbar_ctx* c) {
    if (!c) return fail(nullptr, MBAR_ERR_ARG, "ctx is NULL");
    HIPCHK(c, hipSetDevice(c->device));
    return sync_stream(c);
}

int mbar_device_synchronize(int device) {
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return fail(nullptr, MBAR_ERR_HIP, std::string("hipDeviceSynchronize: ") + hipGetErrorString(e));
    return MBAR_OK;
}

int mbar_ctx_set_option(mbar_ctx* c, const char* key, int64_t value) {
    if (!c || !key) return fail(c, MBAR_ERR_ARG, "NULL argument");
    const std::string k(key);
    if (k == "grid_blocks") c->opt_grid = value;
    else if (k == "force_generic") c->opt_force_generic = value;
    else if (k == "small_k_kernel") c->opt_small = value;
    else if (k == "wide_k_kernel") c->opt_wide = value;
    else if (k == "check_finite") c->opt_check_finite = value;
    else if (k == "timing") c->opt_timing = value;
    else if (k == "graph") c->opt_graph = value;
    else if (k == "sci_batch") c->opt_sci_batch = value < 1 ? 1 : (value > 256 ? 256 : value);
    else if (k == "device_loop") c->opt_device_loop = value;
    else if (k == "pmode") c->opt_pmode = value;
    else if (k == "fused") c->opt_fused = value;
    else if (k == "gram_quad") c->opt_quad = value;
    else if (k == "device_loop_wide") c->opt_device_loop_wide = value;
    else if (k == "pcache") c->opt_pcache = value;
    else if (k == "merge_select") c->opt_merge_select = value;
    else if (k == "light_last") c->opt_light_last = value;
    else if (k == "fused_general") {
        c->opt_fused_general = value ? 1 : 0;
        (void)drop_graphs(c);  // (a captured batch holds the launches of the other kernel)
    }
    else if (k == "debug_download_p") c->opt_debug_download_p = value;
    else if (k == "direct_results") c->opt_direct_results = value;
    else if (k == "sci_merged") c->opt_sci_merged = value;
    else if (k == "host_pmode") c->opt_host_pmode = value;
    else if (k == "rect_waves") c->opt_rect_waves = value == 8 ? 8 : 4;
    else if (k == "newton_ldlt") {
        c->opt_newton_ldlt = value ? 1 : 0;
        (void)drop_graphs(c);
    }
    else if (k == "sci_pingpong") {
        c->opt_sci_pingpong = value;
        (void)drop_graphs(c);
    }
    else if (k == "small_balanced") {
        c->opt_small_balanced = value;
        (void)drop_graphs(c);
    }
    else if (k == "wide_pmode") c->opt_wide_pmode = value;
    else if (k == "quad_trim") {
        c->opt_quad_trim = value;
        c->P_valid = false;  // (the trimmed build never writes the padding rows of P, the untrimmed sweeps read them)
    }
    else if (k == "hist_part_bytes") c->opt_hist_part_bytes = value < 1 ? 1 : value;  // (read by the next mbar_ctx_set_bins)
    else if (k == "scan_part_bytes") c->opt_scan_part_bytes = value < 1 ? 1 : value;  // (read by the next mbar_scan_lognum / mbar_scan_bin_lognum / mbar_scan_bin_gram_w)
    else if (k == "adapt_batch") c->opt_adapt_batch = value < 1 ? 1 : (value > 64 ? 64 : value);
    else return fail(c, MBAR_ERR_ARG, "unknown option: " + k);
    return MBAR_OK;
}

int mbar_ctx_set_Nk(mbar_ctx* c, const double* N_k) {
    if (!c || !N_k) return fail(c, MBAR_ERR_ARG, "NULL argument");
    c->sampled.clear();
    for (int64_t k = 0; k < c->K; ++k) {
        if (!(N_k[k] >= 0.0) || !std::isfinite(N_k[k])) return fail(c, MBAR_ERR_ARG, "N_k must be finite and >= 0");
        c->Nk[k] = N_k[k];
        c->lnNk[k] = N_k[k] > 0.0 ? std::log(N_k[k]) : -std::numeric_limits<double>::infinity();
        if (N_k[k] > 0.0) c->sampled.push_back((int)k);
    }
    if (c->sampled.empty()) return fail(c, MBAR_ERR_ARG, "at least one state must have samples");
    HIPCHK(c, hipSetDevice(c->device));
    {
        int rc = drop_graphs(c);  // the captured adaptive batch bakes in the sampled-state count
        if (rc) return rc;
    }
    std::vector<double> h(2 * (size_t)c->Kp, 0.0);
    for (int64_t k = 0; k < c->Kp; ++k) {
        h[k] = k < c->K ? c->Nk[k] : 0.0;
        h[c->Kp + k] = k < c->K ? c->lnNk[k] : -std::numeric_limits<double>::infinity();
    }
    HIPCHK(c, hipMemcpyAsync(d_Nk(c), h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->P_valid = false;  // (the rows of P of states without samples are zero: the set may have changed)
    c->ld0_valid = false;
    c->last_psum.clear();
    c->have_Nk = true;
    return MBAR_OK;
}

int mbar_ctx_set_sample_weights(mbar_ctx* c, const double* c_n) {
    if (c && c->ext_base) return ext_holds_rows_only(c, "mbar_ctx_set_sample_weights");
    if (!c) return fail(c, MBAR_ERR_ARG, "NULL argument");
    HIPCHK(c, hipSetDevice(c->device));
    bool weighted = false;
    if (c_n) {  // (validated in place: no host copy of the vector; a draw-count vector of a 1e8-sample matrix is 0.8 GB)
        bool bad = false;
        for (int64_t n = 0; n < c->N; ++n) {
            bad |= !(c_n[n] >= 0.0) || !(c_n[n] <= 1.7976931348623157e308);
            weighted |= c_n[n] != 1.0;
        }
        if (bad) return fail(c, MBAR_ERR_ARG, "sample weights must be finite and >= 0");
    }
    if (weighted) {  // (an unweighted call allocates nothing)
        int rc = need_zeroed_vec(c, c->lden_eff);
        if (rc) return rc;
        HIPCHK(c, hipMemcpyAsync(c->cw, c_n, (size_t)c->N * sizeof(double), hipMemcpyHostToDevice, c->stream));
        rc = need_zeroed_vec(c, c->cwsq);
        if (rc) return rc;
        // sqrt(c_n) for the MFMA operands of the fused sweep (plain 0 / 1 weights are their own square roots)
        HIPCHK(c, launch_sqrt_vec(c->stream, c->cwsq, c->cw, c->N));
    } else {
        HIPCHK(c, launch_fill(c->stream, c->cw, 1.0, c->N));  // (the padding behind N stays 0)
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->weighted = weighted;
    c->last_psum.clear();
    return MBAR_OK;
}

// The layout of the bootstrap draws (runs of the states + optional position -> sample map) on the device: validated and uploaded
// ONCE per layout.  The per-replicate call then passes cumN = NULL and touches no host array of N integers.
static int upload_bootstrap_layout(mbar_ctx* c, const int64_t* cumN, int64_t K_states, const int64_t* order, const uint64_t dg[2]) {
    const int64_t total = cumN[K_states];
    const size_t words = (size_t)(K_states + 1) + (order ? (size_t)total : 0);
    if (order)
        for (int64_t p = 0; p < total; ++p)
            if (order[p] < 0 || order[p] >= total) return fail(c, MBAR_ERR_ARG, "bootstrap layout: order entry out of range");
    HIPCHK(c, c->boot_idx.grow(words));
    HIPCHK(c, hipMemcpyAsync(c->boot_idx, cumN, (size_t)(K_states + 1) * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    if (order)
        HIPCHK(c, hipMemcpyAsync(c->boot_idx + K_states + 1, order, (size_t)total * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (the host arrays may go away)
    c->boot_idx_words = words;
    c->boot_layout_digest[0] = dg[0];
    c->boot_layout_digest[1] = dg[1];
    c->boot_states = K_states;
    c->boot_total = total;
    c->boot_has_order = order != nullptr;
    return MBAR_OK;
}

static int check_bootstrap_layout(mbar_ctx* c, const int64_t* cumN, int64_t K_states) {
    if (K_states < 1) return fail(c, MBAR_ERR_ARG, "bootstrap layout: K_states must be >= 1");
    if (cumN[0] != 0) return fail(c, MBAR_ERR_ARG, "bootstrap layout: cumN[0] must be 0");
    for (int64_t k = 0; k < K_states; ++k)
        if (cumN[k + 1] < cumN[k]) return fail(c, MBAR_ERR_ARG, "bootstrap layout: cumN must not decrease");
    return MBAR_OK;
}

int mbar_ctx_set_bootstrap_layout(mbar_ctx* c, const int64_t* cumN, int64_t K_states, const int64_t* order) {
    if (!c || !cumN) return fail(c, MBAR_ERR_ARG, "NULL argument");
    int rc = check_bootstrap_layout(c, cumN, K_states);
    if (rc) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t none[2] = {0, 0};  // (no content digest: a later call that passes its arrays again uploads again)
    return upload_bootstrap_layout(c, cumN, K_states, order, none);
}

int mbar_ctx_draw_bootstrap_weights(mbar_ctx* c, uint64_t seed, int64_t replicate, const int64_t* cumN, int64_t K_states,
                                    const int64_t* order, int64_t n_global0) {
    if (c && c->ext_base) return ext_holds_rows_only(c, "mbar_ctx_draw_bootstrap_weights");
    if (!c) return fail(c, MBAR_ERR_ARG, "NULL argument");
    if (replicate < 0 || n_global0 < 0) return fail(c, MBAR_ERR_ARG, "mbar_ctx_draw_bootstrap_weights: bad argument");
    HIPCHK(c, hipSetDevice(c->device));
    if (!cumN) {  // the layout of mbar_ctx_set_bootstrap_layout (or of an earlier call with arrays)
        if (!c->boot_idx || c->boot_states < 1)
            return fail(c, MBAR_ERR_STATE, "mbar_ctx_draw_bootstrap_weights: no layout on this context (mbar_ctx_set_bootstrap_layout first)");
        if (order) return fail(c, MBAR_ERR_ARG, "mbar_ctx_draw_bootstrap_weights: order without cumN");
    } else {
        int rc = check_bootstrap_layout(c, cumN, K_states);
        if (rc) return rc;
        // arrays handed over with the call: uploaded only when their content differs from what is there (a digest of the order
        // array is a host pass over N integers -- callers with many replicates use mbar_ctx_set_bootstrap_layout + cumN = NULL)
        const int64_t total_in = cumN[K_states];
        const size_t words = (size_t)(K_states + 1) + (order ? (size_t)total_in : 0);
        uint64_t dg[2], a[2], b[2] = {0, 0};
        (void)mbar_host_digest(cumN, (int64_t)((K_states + 1) * sizeof(int64_t)), 1, a);
        if (order) (void)mbar_host_digest(order, (int64_t)((size_t)total_in * sizeof(int64_t)), 0, b);
        dg[0] = (a[0] ^ (b[0] * 0x9E3779B97F4A7C15ull) ^ (uint64_t)words) | 1u;  // (never the "no digest" value of set_bootstrap_layout)
        dg[1] = a[1] ^ (b[1] * 0xC2B2AE3D27D4EB4Full) ^ (order ? 1u : 0u);
        if (!c->boot_idx || c->boot_idx_words != words || c->boot_layout_digest[0] != dg[0] || c->boot_layout_digest[1] != dg[1]) {
            rc = upload_bootstrap_layout(c, cumN, K_states, order, dg);
            if (rc) return rc;
        }
    }
    K_states = c->boot_states;
    const int64_t total = c->boot_total;
    const bool has_order = c->boot_has_order;
    if (total < n_global0 + c->N) return fail(c, MBAR_ERR_ARG, "mbar_ctx_draw_bootstrap_weights: the runs do not cover this shard");
    {
        int rc = need_weight_vecs(c);
        if (rc) return rc;
    }
    HIPCHK(c, launch_fill(c->stream, c->cw, 0.0, c->N));
    HIPCHK(c, launch_bootstrap_counts(c->stream, seed, replicate, c->boot_idx, K_states, total, has_order ? c->boot_idx + K_states + 1 : nullptr,
                                      n_global0, c->N, c->cw));
    HIPCHK(c, launch_sqrt_vec(c->stream, c->cwsq, c->cw, c->N));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->weighted = true;
    c->last_psum.clear();
    return MBAR_OK;
}

int mbar_ctx_weights_from_vec(mbar_ctx* c, double power) {
    if (c && c->ext_base) return ext_holds_rows_only(c, "mbar_ctx_weights_from_vec");
    if (!c) return fail(c, MBAR_ERR_ARG, "NULL argument");
    if (!c->vec_tmp || !c->vec_holds_logshift)
        return fail(c, MBAR_ERR_STATE, "mbar_ctx_weights_from_vec: no observable in the staging vector (mbar_ctx_vec_logshift first; "
                                       "mbar_ctx_row_sub / rows_sub / fill_masked_rows re-use that vector)");
    if (!(std::fabs(power) <= 8.0)) return fail(c, MBAR_ERR_ARG, "mbar_ctx_weights_from_vec: |power| must be <= 8");
    HIPCHK(c, hipSetDevice(c->device));
    {
        int rc = need_weight_vecs(c);
        if (rc) return rc;
    }
    int* flag = reinterpret_cast<int*>(d_misc(c));
    int overflow = 0;
    HIPCHK(c, hipMemsetAsync(flag, 0, sizeof(int), c->stream));
    HIPCHK(c, launch_weights_from_log(c->stream, c->vec_tmp, power, c->N, c->cw, c->cwsq, flag));
    HIPCHK(c, hipMemcpyAsync(&overflow, flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->weighted = true;
    c->last_psum.clear();
    if (overflow)  // (the weights are formed in LINEAR space here: an observable spanning more than ~1e154 overflows its square)
        return fail(c, MBAR_ERR_NUMERIC, "mbar_ctx_weights_from_vec: (A - shift)^power is not finite for some sample; use the log-space path");
    return MBAR_OK;
}

int mbar_ctx_timing(mbar_ctx* c, int which, double* total_ms, int64_t* launches) {
    if (!c || which < 0 || which >= MBAR_TIMER_COUNT) return fail(c, MBAR_ERR_ARG, "bad argument");
    if (total_ms) *total_ms = c->t_ms[which];
    if (launches) *launches = c->t_n[which];
    return MBAR_OK;
}

int mbar_ctx_timing_reset(mbar_ctx* c) {
    if (!c) return fail(c, MBAR_ERR_ARG, "NULL argument");
    for (int i = 0; i < MBAR_TIMER_COUNT; ++i) {
        c->t_ms[i] = 0.0;
        c->t_n[i] = 0;
    }
    return MBAR_OK;
}

int mbar_mfma_f64_peak(mbar_ctx* c, double* tflops) {
    if (!c || !tflops) return fail(c, MBAR_ERR_ARG, "NULL argument");
    HIPCHK(c, hipSetDevice(c->device));
    const int blocks = c->num_cu * 2, iters = 20000;
    hipEvent_t a, b;
    HIPCHK(c, hipEventCreate(&a));
    HIPCHK(c, hipEventCreate(&b));
    HIPCHK(c, launch_mfma_peak(c->stream, blocks, 100, d_misc(c)));  // warm-up
    HIPCHK(c, hipEventRecord(a, c->stream));
    HIPCHK(c, launch_mfma_peak(c->stream, blocks, iters, d_misc(c)));
    HIPCHK(c, hipEventRecord(b, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float ms = 0.f;
    HIPCHK(c, hipEventElapsedTime(&ms, a, b));
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    const double flop = (double)blocks * 4 /*waves*/ * iters * 4 /*mfma*/ * 2048.0;
    *tflops = flop / (ms * 1e-3) * 1e-12;
    return MBAR_OK;
}

}  // extern "C"

