// The layer below the context that every host-side handle of libmbar_hip.so shares (not part of the public ABI): the last error,
// the caching allocator and DevBuf, fail / HIPCHK, and what makes a backend's handle -- Handle, create_handle / destroy_handle,
// run_passes, ColumnPasses.  The backends that are no context (mbar_kde.cpp, mbar_acf.cpp, mbar_bar.cpp, mbar_bspline.cpp,
// mbar_batch.cpp) include this header and their family's; the context (mbar_ctx.h) builds on it.  Defined in mbar_host.cpp
// (fail: mbar_capi.cpp).
#pragma once
#include "../../include/mbar_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <map>
#include <mutex>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

struct mbar_ctx;  // (mbar_ctx.h: fail records the message in the context it is given, if any)

namespace mbar {
namespace host {

extern thread_local std::string g_last_error;

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

}  // namespace host
}  // namespace mbar
using mbar::host::DevBuf;
